"""bench.py's host-side pieces that need no GPU: the command line and --dump-outputs' writer."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_command_line_has_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for opt in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert opt in r.stdout, opt


def _outputs():
    g = torch.Generator().manual_seed(5)
    return {"big": torch.randn(3, 1000, 700, generator=g), "small": torch.randn(4, 5, generator=g),
            "wide": torch.randn(6, generator=g, dtype=torch.float64), "flag": torch.tensor([True, False]),
            "total": torch.tensor(2.5), "note": "not an array"}


def _modules():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Conv1d(1, 4, 3), torch.nn.BatchNorm1d(4)), torch.nn.Linear(7, 2)


def test_dump_outputs_writes_every_array_and_a_fixed_sample(tmp_path):
    out, (G, D) = _outputs(), _modules()
    idx = bench.dump_outputs(out, (G, D), "train", str(tmp_path / "a"))
    names = {"big", "small", "wide", "flag", "total", "generator_state", "detector_state"}
    assert set(idx) == names and sorted(os.listdir(tmp_path / "a")) == sorted(f"{k}.npy" for k in names)
    a = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in names}
    assert a["wide"].dtype == np.float64 and all(a[k].dtype == np.float32 for k in names - {"wide"})
    np.testing.assert_array_equal(a["small"], out["small"].numpy().reshape(-1))
    np.testing.assert_array_equal(a["flag"], [1.0, 0.0])
    assert a["total"].tolist() == [2.5] and idx["total"] == [[], 1]
    # a larger output: DUMP_MAX_ELEMS of its elements, at sorted indices that depend on its size alone
    assert idx["big"] == [[3, 1000, 700], bench.DUMP_MAX_ELEMS] and a["big"].size == bench.DUMP_MAX_ELEMS
    g = torch.Generator().manual_seed(bench.DUMP_SAMPLE_SEED)
    pick = torch.randint(0, out["big"].numel(), (bench.DUMP_MAX_ELEMS,), generator=g).sort().values
    np.testing.assert_array_equal(a["big"], out["big"].reshape(-1)[pick].numpy())
    # module state after the step: every floating-point state_dict entry (parameters, BatchNorm running statistics) in order
    want = torch.cat([v.reshape(-1).float() for v in G.state_dict().values() if v.is_floating_point()])
    np.testing.assert_array_equal(a["generator_state"], want.numpy())
    assert a["detector_state"].size == 7 * 2 + 2
    # the same arguments give the same files
    bench.dump_outputs(_outputs(), _modules(), "train", str(tmp_path / "b"))
    for k in names:
        np.testing.assert_array_equal(np.load(tmp_path / "b" / f"{k}.npy"), a[k])


def test_dump_outputs_eval_mode_has_no_module_state(tmp_path):
    idx = bench.dump_outputs(_outputs(), _modules(), "fwd", str(tmp_path))
    assert "generator_state" not in idx and "detector_state" not in idx


def test_dump_outputs_refuses_more_than_64_mb(tmp_path):
    many = {f"x{i}": torch.zeros(bench.DUMP_MAX_ELEMS + 1) for i in range(17)}     # 17 x 4 MiB samples
    try:
        bench.dump_outputs(many, _modules(), "fwd", str(tmp_path))
    except AssertionError as e:
        assert "64 MB" in str(e)
    else:
        raise AssertionError("dump_outputs wrote more than 64 MB")
