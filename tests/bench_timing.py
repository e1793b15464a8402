"""The timing the tests/bench_*.py scripts share: a batch of launches between two events, how many launches make a batch, the median and
spread over the rounds, and several codes measured in alternation."""
import torch


def batch_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def launches_for(fn, batch_seconds, cap):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t = batch_ms(fn, 2)
    return max(1, min(cap, int(batch_seconds * 1e3 / max(t, 1e-3)) + 1))


def stats(v):
    """(median, (max - min) / median)"""
    v = sorted(v)
    med = v[len(v) // 2]
    return med, (v[-1] - v[0]) / med


def measure(runs, rounds, batch_seconds):
    k = {c: launches_for(fn, batch_seconds, 20000) for c, fn in runs.items()}
    times = {c: [] for c in runs}
    for _ in range(rounds):                                           # alternate the codes inside every round
        for c, fn in runs.items():
            times[c].append(batch_ms(fn, k[c]))
    return {c: stats(v) + (k[c],) for c, v in times.items()}
