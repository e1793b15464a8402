"""torch.autograd.Function wrappers over the C ABI (include/wm_hip.h).

PyTorch is used here for device memory, streams and the autograd tape only; every
arithmetic step of the hot path is a launch into libwm_hip.so.  Each Function mirrors one
block of the reference graph (py/main16.py:112-186, :53-81, :192-217).
"""
from __future__ import annotations

import contextlib
import os
from typing import NamedTuple, Optional

import torch

from ._host import _chk, _chk_int, _chk_positive, _f32, _p, _seed64, _stream
from ._lib import lib

NCU = 256            # workgroups the persistent kernels are sized for (MI355X CU count)
BN_EPS = 1e-5        # nn.BatchNorm1d defaults (py/main16.py:117,120)
BN_MOMENTUM = 0.1


def _frames(x: torch.Tensor, name: str, ch: int) -> torch.Tensor:
    x = _chk(x, name, 3)
    if x.shape[1] != ch:
        raise ValueError(f"{name}: expected {ch} channels, got shape {tuple(x.shape)}")
    if x.shape[2] % 4 != 0:
        raise ValueError(f"{name}: clip length must be a multiple of 4 samples, got {x.shape[2]}")
    return x


# ---------------------------------------------------------------------------------------------- grad mode
# Inside Function.forward autograd has already switched grad mode off, and ctx.needs_input_grad only mirrors the
# inputs' requires_grad flags -- under torch.no_grad() a module with trainable parameters still reports True there.
# The forward-only fast paths (two-launch inference ResBlock, LSTM without saved activations) must key on "will a
# backward ever run", i.e. on the grad mode of the CALLER: GradAwareFunction.apply records it before dispatch.
_GRAD = {"on": True}


class GradAwareFunction(torch.autograd.Function):
    @classmethod
    def apply(cls, *args, **kwargs):
        _GRAD["on"] = torch.is_grad_enabled()
        return super().apply(*args, **kwargs)


def wants_grad(ctx) -> bool:
    """True when the tape is recording AND some input asks for a gradient"""
    return _GRAD["on"] and any(ctx.needs_input_grad)


def _single_backward(ctx, what):
    """the recurrences overwrite their saved gate activations with da in place (no second 4-5 GB buffer at B=256):
    a second backward over a retained graph would read da as if it were activations -- refuse it loudly"""
    if getattr(ctx, "_wm_consumed", False):
        raise RuntimeError(f"{what}: backward was already run once on this graph; the saved gate activations were "
                           "overwritten in place (retain_graph=True / per-loss backward calls are not supported -- "
                           "sum the losses and call backward once, as py/main16.py:275-277 does)")
    ctx._wm_consumed = True


# ---------------------------------------------------------------------------------------------- side stream
# Weight-gradient GEMMs do not feed the data path of backward.  When the parameters carry a pre-allocated gradient
# destination (optim.FlatAdam sets p._wm_grad = view of the flat gradient bucket and enables this), they are
# launched on a second HIP stream and ACCUMULATE straight into that bucket (the Function then returns None for
# them), so they overlap with the latency-bound LSTM recurrence and the HBM-bound element-wise kernels of the main
# stream.  optim.FlatAdam.finish_backward() joins the streams before the all-reduce / update.
_ASYNC = {"on": False, "side": None, "deferred": []}


def set_async_wgrad(on: bool):
    _ASYNC["on"] = bool(on)


def side_stream():
    if _ASYNC["side"] is None:
        _ASYNC["side"] = torch.cuda.Stream()
    return _ASYNC["side"]


def release_deferred_wgrads():
    """Weight-gradient GEMMs queued so far start now, on the side stream, behind everything the current stream has been
    given up to this point.  Called right before the LSTM BPTT launch (the 8 ms during which the matrix cores are idle and
    each CU holds only one 152-register recurrence workgroup) and from join_side_stream()."""
    pend, _ASYNC["deferred"] = _ASYNC["deferred"], []
    if not pend:
        return
    main, side = torch.cuda.current_stream(), side_stream()
    ev = torch.cuda.Event()
    ev.record(main)
    with torch.cuda.stream(side):
        side.wait_event(ev)
        for inputs, fn in pend:
            for t in inputs:
                if t is not None:
                    t.record_stream(side)
            fn()


def join_side_stream():
    release_deferred_wgrads()
    if _ASYNC["side"] is not None:
        torch.cuda.current_stream().wait_stream(_ASYNC["side"])


def _gdst(*params):
    """gradient destinations registered on the parameters (None when the async path is off)"""
    return tuple(getattr(p, "_wm_grad", None) if _ASYNC["on"] else None for p in params)


def _on_side(inputs, fn, defer=True):
    """queue fn() (kernel launches) for the side stream.  defer=True: held back until release_deferred_wgrads() -- launched
    at once they would only take turns with the main stream's convolutions (both want whole CUs); released at the start of
    the LSTM BPTT they fill the CUs' idle matrix cores instead."""
    _ASYNC["deferred"].append((inputs, fn))
    if not defer:
        release_deferred_wgrads()


def _wgrad_dst(gdst, device, *shapes):
    """(tensors for the weight-gradient kernel, accumulate, launch): with destinations registered (gdst, views of the flat gradient bucket) the
    kernel ACCUMULATES into them, queued for the side stream by launch(inputs it reads, fn); else it fills fresh `shapes`, launched in line"""
    if all(g is not None for g in gdst):
        return gdst, True, _on_side
    return tuple(_f32(*shape, device=device) for shape in shapes), False, lambda inputs, fn: fn()


# ---------------------------------------------------------------------------------------------- path switches
# Every path switch, by the name switches() / set_switch() take: (store, key, environment variable, default, library entry point | None,
# what on | off selects).  store[key] holds the live value: plain dicts (_CONV, _LSTM, main14b_2's _GCONV and its module globals) read
# directly on the hot path and by bench.py.  The variable: "1" = on, else off (schedule: an integer).  A library entry point: the value
# also lives in libwm_hip.so and set_switch() calls it -- at import ONLY when the variable is present (importing needs no built library).
SWITCHES = {
    "bf16x6": ("conv", "bf16x6", "WM_CONV_BF16X6", True, None, "64->64 convolutions on the bf16x6 / f16 split builds | native fp32 MFMA"),
    "schedule": ("conv", "schedule", "WM_CONV_BF_SCHEDULE", 2, "wm_set_conv_bf_schedule", "an integer: 2 register-resident weights + interleaved split | 0 phase-serial"),
    "one_launch_eval": ("conv", "one_launch_eval", "WM_RESBLOCK_ONE_LAUNCH", True, None, "inference ResBlock as one launch | two"),
    "fused_bwd": ("conv", "fused_bwd", "WM_FUSED_BWD", True, None, "ResBlock backward: data + weight gradient of a convolution in one launch | two"),
    "mask_on_load": ("conv", "mask_on_load", "WM_MASK_ON_LOAD", True, None, "fused ResBlock backward masks g on load | writes the masked gradient first"),
    "pair_fold": ("conv", "pair_fold", "WM_PAIR_FOLD", True, None, "two ResBlocks in a row as one tape node | two nodes"),
    "bwd_f16x3": ("conv", "bwd_f16x3", "WM_BWD_F16X3", True, None, "fused ResBlock backward on the f16 two-piece split | bf16x6"),
    "fwd_f16x3": ("conv", "fwd_f16x3", "WM_FWD_F16X3", True, None, "ResBlock forward convolutions on the f16 two-piece split | bf16x6"),
    "conv7_f16x3": ("conv", "conv7_f16x3", "WM_CONV7_F16X3", True, None, "ConvTranspose1d(64,64,7) on the f16 two-piece split | bf16x6"),
    "eval_f16x3": ("conv", "eval_f16x3", "WM_EVAL_F16X3", True, None, "one-launch inference ResBlock on the f16 two-piece split | bf16x6"),
    "lstm_fused": ("lstm", "fused", "WM_LSTM_FUSED", True, None, "LSTM input projection inside the recurrence kernel | wm_lstm_xproj + wm_lstm_fwd"),
    "lstm_bwd_fused": ("lstm", "bwd_fused", "WM_LSTM_BWD_FUSED", False, None, "wm_lstm_bwd + wm_lstm_dx as one launch | two (the default)"),
    "lstm_bwd_ws": ("lstm", "bwd_ws", "WM_LSTM_BWD_WS", True, None, "LSTM weight gradients on helper waves beside the BPTT | wm_lstm_bwd + wm_lstm_wgrad"),
    "lstm_fwd_ws": ("lstm", "fwd_ws", "WM_LSTM_FWD_WS", True, "wm_set_lstm_fwd_wave_specialised", "LSTM forward input projection on helper waves | in the recurrence's own waves"),
    "gconv_f16x3": ("gconv", "f16x3", "WM_GCONV_F16X3", True, None, "main14b_2 generic convolutions on the f16 two-piece split | native fp32 MFMA"),
    "fused_strided_dgrad": ("main14b_2", "_FUSED_STRIDED_DGRAD", "WM_FUSED_STRIDED_DGRAD", True, None, "main14b_2 down-sampling block: both data gradients into x in one launch | two"),
}


def read_switches(environ) -> dict:
    """{"conv": {key: value}, "lstm": {...}, "gconv": {...}, "main14b_2": {...}, "library": [names]}: what every switch starts with under `environ` (pure: no
    store, no library call).  "library": the library-backed switches whose variable is present -- only those must reach libwm_hip.so"""
    out = {"conv": {}, "lstm": {}, "gconv": {}, "main14b_2": {}, "library": []}
    for name, (store, key, env, default, libfn, _) in SWITCHES.items():
        raw = environ.get(env)
        out[store][key] = default if raw is None else int(raw) if type(default) is int else raw == "1"
        if libfn and raw is not None:
            out["library"].append(name)
    return out


_LIVE = read_switches(os.environ)
_CONV, _LSTM, _GCONV = _LIVE["conv"], _LIVE["lstm"], _LIVE["gconv"]


def bind_store(store, namespace):
    """a module that keeps its switches as plain globals (main14b_2) hands over its namespace: seeded with the starting values, it IS the store"""
    namespace.update(_LIVE[store])
    _LIVE[store] = namespace


def set_switch(name, value):
    """the common setter: store[key] = value (and the library's copy, for a library-backed switch)"""
    store, key, _, default, libfn, _ = SWITCHES[name]
    value = type(default)(value)
    if libfn:
        getattr(lib, libfn)(int(value), None)
    _LIVE[store][key] = value


for _name in _LIVE["library"]:
    set_switch(_name, _LIVE[SWITCHES[_name][0]][SWITCHES[_name][1]])


@contextlib.contextmanager
def switches(**values):
    """run a block under other switch values (names: SWITCHES); the PREVIOUS values come back on exit, also when the block raises.
    An unknown name raises KeyError before anything changes.  For tests and diagnostics, not for the step path."""
    prev = {name: _LIVE[SWITCHES[name][0]][SWITCHES[name][1]] for name in values}
    try:
        for name, value in values.items():
            set_switch(name, value)
        yield
    finally:
        for name, value in prev.items():
            set_switch(name, value)


def set_conv_bf_schedule(schedule: int):
    """0: phase-serial kernel, 2: register-resident weights + interleaved split (csrc/conv64_fwd.hip)."""
    set_switch("schedule", schedule)


def set_conv_bf16x6(on: bool):
    set_switch("bf16x6", on)


def set_fused_backward(on: bool):
    """ResBlock backward: data gradient + weight gradient of each convolution in ONE launch (wm_dwgrad64_bf, default) or as two
    (wm_conv64_bf + wm_wgrad64_bf).  WM_FUSED_BWD=0/1 in the environment sets the default."""
    set_switch("fused_bwd", on)


def set_mask_on_load(on: bool):
    """fused ResBlock backward: 1 (default) the masked gradient dz2 = g * (out > 0) is never written -- the reduction pass forms
    only the BatchNorm sums and wm_dwgrad64_bf masks g on load; 0 it is materialised first.  WM_MASK_ON_LOAD=0/1 sets the default."""
    set_switch("mask_on_load", on)


def set_bwd_f16x3(on: bool):
    """fused ResBlock backward arithmetic: 1 (default) f16 two-piece split, three products per product on the f16 matrix cores
    (half the matrix work of bf16x6; power-of-two scales from max |w| and max |A| max |dz| keep the operands in the f16 range),
    0 bf16x6 as in the forward.  WM_BWD_F16X3=0/1 sets the default."""
    set_switch("bwd_f16x3", on)


def set_fwd_f16x3(on: bool):
    """ResBlock forward convolutions launched through wm_conv64_bf (schedule 2, T % 128 == 0): 1 (default) the f16 two-piece split
    (three products per product instead of six; weights scaled by a power of two from max |w|, activations unscaled), 0 bf16x6.
    WM_FWD_F16X3=0/1 sets the default.  The one-launch inference ResBlock has its own switch (set_eval_f16x3)."""
    set_switch("fwd_f16x3", on)


def set_eval_f16x3(on: bool):
    """one-launch inference ResBlock (wm_resblock_eval_bf): 1 (default) the f16 two-piece split, 0 bf16x6.  WM_EVAL_F16X3=0/1."""
    set_switch("eval_f16x3", on)


def pack_w64_h(w: torch.Tensor, mode: int) -> torch.Tensor:
    wph = torch.empty(2 * 3 * 4096 + 4, dtype=torch.int16, device=w.device)      # two f16 pieces + {ws, 1 / ws}
    lib.wm_pack_w64_h(_p(w), _p(wph), mode, _stream())
    return wph


def set_pair_fold(on: bool):
    """two ResBlocks in a row (encoder.1 -> encoder.2, model.1 -> model.2) as ONE tape node whose backward lets the second block's
    conv1 launch also do the first block's ReLU backward and BatchNorm sums (no reduction pass for the first block).
    WM_PAIR_FOLD=0/1 sets the default; off = two ResBlockFn nodes."""
    set_switch("pair_fold", on)


def set_resblock_one_launch(on: bool):
    """inference ResBlock: one launch (wm_resblock_eval_bf, default) or the two-launch form (conv1; conv2 with BN2 + add + ReLU
    in its epilogue).  WM_RESBLOCK_ONE_LAUNCH=0/1 in the environment sets the default."""
    set_switch("one_launch_eval", on)


def conv_bf16x6() -> bool:
    return _CONV["bf16x6"]


def pack_w64_bf(w: torch.Tensor, mode: int) -> torch.Tensor:
    wpb = torch.empty(3 * 3 * 4096, dtype=torch.int16, device=w.device)
    lib.wm_pack_w64_bf(_p(w), _p(wpb), mode, _stream())
    return wpb


def set_conv7_f16x3(on: bool):
    """ConvTranspose1d(64,64,7) forward / data gradient / weight gradient (T % 128 == 0): 1 (default) the f16 two-piece split (three
    products per product; weights scaled by a power of two from max |w|, the incoming gradient by one from max |g| -- one streaming
    pass over g, wm_gscale_absmax), 0 bf16x6.  WM_CONV7_F16X3=0/1 sets the default."""
    set_switch("conv7_f16x3", on)


def pack_w64_h7(w: torch.Tensor, mode: int) -> torch.Tensor:
    wph = torch.empty(2 * 7 * 4096 + 4, dtype=torch.int16, device=w.device)      # two f16 pieces + {ws, 1 / ws}
    lib.wm_pack_w64_h7(_p(w), _p(wph), mode, _stream())
    return wph


def set_lstm_fwd_wave_specialised(on: bool):
    """LSTM forward (wm_lstm_fwd_fused): 1 (default) the input projection of the next 32-step chunk runs on four helper waves beside the
    recurrence, 0 inside the recurrence's own waves.  Bit-identical results.  WM_LSTM_FWD_WS=0/1 sets the default."""
    set_switch("lstm_fwd_ws", on)


def set_lstm_bwd_wave_specialised(on: bool):
    """LSTM backward: 1 (default) wm_lstm_bwd_wgrad -- the weight gradients are formed by four helper waves beside the recurrence, from
    the chunk of da it has just finished (T % 32 == 0, T >= 64); 0 wm_lstm_bwd followed by wm_lstm_wgrad.  WM_LSTM_BWD_WS=0/1."""
    set_switch("lstm_bwd_ws", on)


# The ResBlock in front of a head (decoder.1 -> Conv1d(64,1,1), model.2 -> Conv1d(64,1+bits,1)) leaves its tail -- BN2 + residual add +
# ReLU -- to the head's forward kernel, and the Detector head also sums both BCE terms and forms their gradient on load in its
# backward (wm_head1_tail_fwd, wm_headN_tail_fwd, wm_headN_bwd_bce).  WM_TAIL_IN_HEAD=0/1 sets the default ("1" = on, else off).
# Measured at B = 256: -0.7 ms of 48.6 per step.
_HEADS = {"tail_in_head": os.environ.get("WM_TAIL_IN_HEAD", "1") == "1"}


def set_tail_in_head(on: bool):
    """1 (default): ResBlockHead1Fn / DetectorTailFn where they apply (training-mode blocks, no forward hooks, no side-stream weight
    gradients); 0: every ResBlock ends in wm_bn_add_relu(_mask) and the losses run wm_bce_fwd / wm_bce_bwd.  Same results bit for bit,
    except the two BCE sums (fp32 partial sums grouped differently)."""
    _HEADS["tail_in_head"] = bool(on)


# A ResBlock followed by another consumer of its output inside one tape node (encoder.1 -> encoder.2 -> LSTM, model.1 -> model.2)
# leaves its tail to that consumer's forward kernel, which forms relu(x + sc2 * y2 + sh2) while it stages its input and writes `out`
# and the sign bits as side products: the next block's conv1 (wm_conv64_bf_tail) and the LSTM's helper waves (wm_lstm_fwd_tail).
# WM_TAIL_IN_CONSUMER=0/1 sets the default ("1" = on, else off).  Kept outside SWITCHES like _HEADS.
def read_tail_in_consumer(environ) -> bool:
    """what the switch starts with under `environ` (pure, as read_switches)"""
    return environ.get("WM_TAIL_IN_CONSUMER", "1") == "1"


_TAILC = {"on": read_tail_in_consumer(os.environ)}


def set_tail_in_consumer(on: bool):
    """1 (default): the tails of encoder.1, encoder.2 and model.1 are formed by the kernel that reads them next, where
    tail_in_consumer_applies(); 0: each of them is a wm_bn_add_relu(_mask) launch.  Bit-identical either way: the same expression
    element by element, no sum is regrouped."""
    _TAILC["on"] = bool(on)


# The train step's EncoderLSTMFn forms the LSTM input gradient inside the wave-specialised BPTT launch (wm_lstm_bwd_wgrad_dx): da is
# neither written to memory nor read back by wm_lstm_dx.  WM_LSTM_DX_IN_BWD=0/1 sets the default ("1" = on, else off).  Kept outside
# SWITCHES like _TAILC; plain LSTMFn always runs wm_lstm_bwd_wgrad + wm_lstm_dx.
def read_lstm_dx_in_bwd(environ) -> bool:
    """what the switch starts with under `environ` (pure, as read_switches)"""
    return environ.get("WM_LSTM_DX_IN_BWD", "1") == "1"


_LSTM_DX = {"in_bwd": read_lstm_dx_in_bwd(os.environ)}


def set_lstm_dx_in_bwd(on: bool):
    """1 (default): EncoderLSTMFn's backward is one wm_lstm_bwd_wgrad_dx launch where _lstm_bwd's conditions hold (wave-specialised
    BPTT, T % 32 == 0, T >= 64, no side-stream weight gradients); 0: wm_lstm_bwd_wgrad + wm_lstm_dx.  Bit-identical either way."""
    _LSTM_DX["in_bwd"] = bool(on)


# decoder.1's backward never sees the gradient frame behind the Conv1d(64, 1, 1) head: dout[b,c,t] = hw[c] g[b,t] is formed on load by its
# three readers (wm_relu_bwd_reduce_mask_r1, wm_dwgrad64_bf_r1 twice) and wm_head1_bwd writes dw and db only.  WM_HEAD1_RANK1=0/1 sets
# the default ("1" = on, else off).  Kept outside SWITCHES like _TAILC.
def read_head1_rank1(environ) -> bool:
    """what the switch starts with under `environ` (pure, as read_switches)"""
    return environ.get("WM_HEAD1_RANK1", "1") == "1"


_HEAD1_R1 = {"on": read_head1_rank1(os.environ)}


def set_head1_rank1(on: bool):
    """1 (default): ResBlockHead1Fn's backward passes (g, hw) down instead of the frame where head1_rank1_applies(); 0: wm_head1_bwd
    writes the frame and the block's backward reads it.  Bit-identical either way: the same single multiply, no sum is regrouped."""
    _HEAD1_R1["on"] = bool(on)


def head1_rank1_applies(x) -> bool:
    """the switch and what the three rank-one launches need: the fused backward in its f16 build with the mask applied on load,
    T % 64 == 0, no side-stream weight gradients"""
    return bool(_HEAD1_R1["on"] and x.is_cuda and x.dim() == 3 and x.shape[-1] % 64 == 0 and _CONV["bf16x6"] and _CONV["fused_bwd"]
                and _CONV["bwd_f16x3"] and _CONV["mask_on_load"] and not _ASYNC["on"])


def _tail_in_consumer_launches(x, lstm: bool = False) -> bool:
    """the switch and what the two launches need: the f16 pipelined forward (the tail prologue exists in that build only, so
    T % 128 == 0); lstm=True adds the wave-specialised fused LSTM forward.  What a tape node asks inside its forward, where autograd
    has gradients switched off."""
    ok = (_TAILC["on"] and x.is_cuda and x.dim() == 3 and x.shape[-1] % 128 == 0 and _CONV["bf16x6"] and _CONV["fwd_f16x3"]
          and _CONV["schedule"] == 2)
    return bool(ok and (not lstm or (_LSTM["fused"] and _LSTM["fwd_ws"])))


def tail_in_consumer_applies(x, lstm: bool = False) -> bool:
    """_tail_in_consumer_launches and the pair node's own precondition (pair_node_applies).  The caller adds: training-mode blocks, no
    forward hooks."""
    return _tail_in_consumer_launches(x, lstm) and bool(pair_node_applies(x))


# The stem's output y0 = Conv1d(1, 64, 7, padding=3)(s) is formed by the first ResBlock's conv1 launch while it stages its input
# (wm_conv64_bf_stem, which also writes y0 for the second block's conv1) and by that block's conv1 pair in the backward
# (wm_dwgrad64_bf_stem): no wm_stem_fwd launch, two frame passes less per network.  WM_STEM_IN_CONV1=0/1 sets the default ("1" = on,
# else off).  Kept outside SWITCHES like _TAILC.
def read_stem_in_conv1(environ) -> bool:
    """what the switch starts with under `environ` (pure, as read_switches)"""
    return environ.get("WM_STEM_IN_CONV1", "1") == "1"


_STEMC = {"on": read_stem_in_conv1(os.environ)}


def set_stem_in_conv1(on: bool):
    """1 (default): the nodes behind a stem take the clips and the stem's parameters (StemEncoderLSTMFn, StemDetectorTailFn,
    StemResBlockPairFn) where stem_in_conv1_applies(); 0: StemFn in front of the nodes of today.  Bit-identical either way: the formed
    element is stem_fwd_kernel's own fmaf chain, no sum is regrouped."""
    _STEMC["on"] = bool(on)


def _stem_in_conv1_launches(s) -> bool:
    """the switch and what wm_conv64_bf_stem needs: the tail-in-consumer launches' conditions on a [B,1,T] fp32 clip batch.  What a
    tape node asks inside its forward, where autograd has gradients switched off."""
    return bool(_STEMC["on"] and s.dim() == 3 and s.shape[1] == 1 and s.dtype == torch.float32 and _tail_in_consumer_launches(s))


def stem_in_conv1_applies(s, lstm: bool = False) -> bool:
    """_stem_in_conv1_launches and the nodes' own precondition: tail_in_consumer_applies (so: gradients wanted, the fused backward, no
    side-stream weight gradients).  The caller adds: training-mode blocks, no forward hooks on the stem and the blocks."""
    return _stem_in_conv1_launches(s) and tail_in_consumer_applies(s, lstm)


def _stem_in_dwgrad_launches(x) -> bool:
    """what wm_dwgrad64_bf_stem needs beyond the switch: the fused backward in its f16 build (asked in a node's backward)"""
    return bool(_STEMC["on"] and _CONV["bwd_f16x3"] and x.shape[-1] % 64 == 0)


def set_gconv_f16x3(on: bool):
    """generic convolution family (wm_gconv: forward, transposed, data gradients) for layers with Cin % 16 == 0: 1 (default) the f16
    two-piece split on the f16 matrix cores (wm_gconv_h; weights scaled by 2^8, a gradient input from max |g|, an activation from max |x|
    per clip), 0 native fp32
    MFMA.  WM_GCONV_F16X3=0/1 sets the default."""
    set_switch("gconv_f16x3", on)


# max |g| per producer workgroup of gradient tensors whose producer formed it anyway, keyed by the tensor OBJECT (a weak reference
# guards against a recycled id) and its version counter: a hit saves the consumer's streaming pass over g, a miss is merely slower.
# The version matters: autograd sums the gradients of a tensor with several consumers IN PLACE into the first one that arrived, after
# its producer noted the maximum -- a bumped version means the noted maximum no longer describes the tensor.
_GMAX = {}


def _note_gmax(t: torch.Tensor, maxes: torch.Tensor, per_clip: bool = False):
    """maxes: max |t| of everything the producer stored, as one or more partial maxima (per_clip: one per clip, t.shape[0] of them)"""
    import weakref
    if len(_GMAX) > 256:
        _GMAX.clear()
    _GMAX[id(t)] = (weakref.ref(t), t._version, maxes, per_clip)


def _noted(t: torch.Tensor, pop: bool):
    e = _GMAX.pop(id(t), None) if pop else _GMAX.get(id(t))
    return e if e is not None and e[0]() is t and e[1] == t._version else None


def gscale_of(g: torch.Tensor, log2_target: float = 12.0) -> torch.Tensor:
    """{gs, 1 / gs} for gradient g: from its producer's maxima when it left them (no pass over g), else wm_gscale_absmax"""
    e = _noted(g, pop=True)
    if e is not None:
        gsc = _f32(2, device=g.device)
        lib.wm_gscale_from_max(_p(e[2]), e[2].numel(), float(log2_target), _p(gsc), _stream())
        return gsc
    return gscale_absmax(g, log2_target)


_ZPOOL = {"buf": None, "used": 0}


def zeroed_slots(n: int, device) -> torch.Tensor:
    """n zero floats for a launch's atomic-max output: slices of a pool zeroed once and never handed out twice (no fill launch per layer)"""
    p = _ZPOOL
    if p["buf"] is None or p["buf"].device != torch.device(device) or p["used"] + n > p["buf"].numel():
        p["buf"], p["used"] = torch.zeros(max(1 << 16, n), dtype=torch.float32, device=device), 0
    s = p["buf"][p["used"]:p["used"] + n]
    p["used"] += n
    return s


def amax_per_clip(x: torch.Tensor) -> torch.Tensor:
    """max |x| per clip of activation x [NB][...] -- the per-clip input scale of wm_gconv_h (per_clip = 1): the maxima its producer left
    (the producing wm_gconv_h's ymax), else one pass over x.  Per clip, so that a clip's result never depends on the rest of the batch."""
    e = _noted(x, pop=False)
    if e is not None and e[3]:
        return e[2]
    NB = x.shape[0]
    m = zeroed_slots(NB, x.device)
    lib.wm_absmax_rows(_p(x), NB, x.numel() // NB, _p(m), _stream())
    _note_gmax(x, m, per_clip=True)              # kept for the next consumer of the same x (a block's conv1 and skip conv)
    return m


def gscale_absmax(g: torch.Tensor, log2_target: float = 12.0) -> torch.Tensor:
    """{gs, 1 / gs}: the power of two that puts max |g| into (2^(L-1), 2^L] -- the input scale of the f16 two-piece split kernels"""
    gsc, scratch = _f32(2, device=g.device), _f32(1024, device=g.device)
    lib.wm_gscale_absmax(_p(g), g.numel(), _p(scratch), float(log2_target), _p(gsc), _stream())
    return gsc


def pack_w64_bf7(w: torch.Tensor, mode: int) -> torch.Tensor:
    wpb = torch.empty(3 * 7 * 4096, dtype=torch.int16, device=w.device)
    lib.wm_pack_w64_bf7(_p(w), _p(wpb), mode, _stream())
    return wpb


def _conv3(x, x2, w, mode, pa, pb, pc, bias, e1, ea, eb, y, stats, B, T, pro, epi):
    """one k3 64->64 convolution launch in the selected arithmetic mode (mode: 0 forward, 1 data gradient)"""
    if _CONV["bf16x6"]:
        h = (_CONV["fwd_f16x3"] and mode == 0 and (pro, epi) in ((0, 0), (1, 0), (1, 4)) and _CONV["schedule"] == 2 and T % 128 == 0)
        lib.wm_conv64_bf(_p(x), _p(x2), _p(pack_w64_h(w, 0) if h else pack_w64_bf(w, mode)), _p(pa), _p(pb), _p(pc), _p(bias), _p(e1),
                         _p(ea), _p(eb), _p(y), _p(stats), B, T, pro, epi, 1 if h else 0, _stream())
    else:
        lib.wm_conv64(_p(x), _p(x2), _p(pack_w64(w, 3, mode)), _p(pa), _p(pb), _p(pc), _p(bias), _p(e1), _p(ea), _p(eb), _p(y),
                      _p(stats), B, T, 3, pro, epi, _stream())


def pack_w64(w: torch.Tensor, kw: int, mode: int) -> torch.Tensor:
    wp = _f32(kw * 4096, device=w.device)
    lib.wm_pack_w64(_p(w), _p(wp), kw, mode, _stream())
    return wp


# ----------------- the tape's state, by name: tuples still (save_for_backward(*saved), len(), slicing, a caller's plain tuple work as before)
_T = Optional[torch.Tensor]
_bn_consts = torch.Tensor.unbind                # (cst) -> sc1, sh1, mean1, is1, sc2, sh2, mean2, is2: the rows of a block's [8,64] cst
# a ResBlock's parameters, then its BatchNorm buffers, in modules._rb_args order; its gradients come back in the same shape (_block_grads)
BlockParams = NamedTuple("BlockParams", [(n, _T) for n in "w1 b1 g1 be1 w2 b2 g2 be2 rm1 rv1 nbt1 rm2 rv2 nbt2".split()])
LstmSaved = NamedTuple("LstmSaved", [(n, _T) for n in "x h gates cst w_ih w_hh".split()])          # what _lstm_fwd keeps for _lstm_bwd


class BlockSaved(NamedTuple):
    """what _resblock_fwd keeps for a backward; mask = the sign bits of the output (None until a tail is formed), cst = _bn_consts"""
    x: _T; y1: _T; y2: _T; mask: _T; cst: _T; w1: _T; w2: _T; g1: _T; g2: _T
    sc2 = property(lambda self: self.cst[4])    # BN2's scale and shift: what a consumer needs to form the tail relu(x + y2 * sc2 + sh2)
    sh2 = property(lambda self: self.cst[5])


def _block_grads(grads):                        # (dw1, db1, dg1, dbe1, dw2, db2, dg2, dbe2) at their BlockParams positions, None for the buffers
    return BlockParams(*grads, None, None, None, None, None, None)


def _cut(seq, *types):
    """seq (a node's *args, its ctx.saved_tensors) by name: one tuple per type of `types`, in order, then the rest as a tuple"""
    ends = [sum(len(t._fields) for t in types[:i + 1]) for i in range(len(types))]
    return (*(t._make(seq[e - len(t._fields):e]) for t, e in zip(types, ends)), tuple(seq[ends[-1]:]))


# ------------------------------------------------------------------------------------------ ResBlock
def _resblock_fwd(x, params, training, want_grad, tail=True, pending=None, stem=None):
    """relu(x + BN2(conv2(relu(BN1(conv1(x)))))) for a BlockParams: (out, saved), a BlockSaved | None from the inference launches.  No ctx.
    tail=False (training mode only): stop in front of the tail -- (None, saved) with mask = None; the kernel that follows forms
    out = relu(x + y2 * saved.sc2 + saved.sh2) and the mask (ResBlockHead1Fn, DetectorTailFn, or the next block through `pending`).
    pending (training mode, tail_in_consumer_applies): the `saved` of the block in front, run with tail=False; x is ignored.  This
    block's conv1 launch (wm_conv64_bf_tail) forms that block's tail on load and writes it -- this block's x -- and its mask; the
    return value is then (out, saved, that mask).
    stem = (s, w, b) of the Conv1d(1, 64, 7) in front (x is ignored): this block's x is that stem's output, formed and written by the
    conv1 launch itself (wm_conv64_bf_stem) where _stem_in_conv1_launches(s) in training mode, else by wm_stem_fwd first."""
    w1, b1, g1, be1, w2, b2, g2, be2, rm1, rv1, nbt1, rm2, rv2, nbt2 = BlockParams._make(params)
    if pending is not None:
        pending = BlockSaved._make(pending)
        px, py2 = pending.x, pending.y2
        x, pmask = torch.empty_like(px), _tail_mask(px, want_grad)
    if stem is not None:
        ss, sw, sb = stem
        x = _f32(ss.shape[0], 64, ss.shape[2], device=ss.device)
        if not (training and _stem_in_conv1_launches(ss)):
            lib.wm_stem_fwd(_p(ss), _p(sw), _p(sb), _p(x), ss.shape[0], ss.shape[2], _stream())
            stem = None
    x = _frames(x, "ResBlock input", 64)
    B, _, T = x.shape
    dev, st = x.device, _stream()
    out = torch.empty_like(x) if tail else None
    cst = _f32(8, 64, device=dev)       # sc1 sh1 mean1 is1 sc2 sh2 mean2 is2
    sc1, sh1, mu1, is1, sc2, sh2, mu2, is2 = _bn_consts(cst)
    if training:
        y1, y2 = torch.empty_like(x), torch.empty_like(x)
        stats = _f32(NCU * 128, device=dev)
        if pending is not None:
            lib.wm_conv64_bf_tail(_p(px), _p(py2), _p(pack_w64_h(w1, 0)), _p(pending.sc2), _p(pending.sh2), _p(b1), _p(x), _p(pmask), _p(y1),
                                  _p(stats), B, T, st)
        elif stem is not None:
            lib.wm_conv64_bf_stem(_p(ss), _p(sw), _p(sb), _p(pack_w64_h(w1, 0)), _p(b1), _p(x), _p(y1), _p(stats), B, T, st)
        else:
            _conv3(x, None, w1, 0, None, None, None, b1, None, None, None, y1, stats, B, T, 0, 0)
        lib.wm_bn_finalize(_p(stats), NCU, float(B * T), _p(g1), _p(be1), _p(rm1), _p(rv1), _p(nbt1), BN_MOMENTUM, BN_EPS,
                           _p(sc1), _p(sh1), _p(mu1), _p(is1), st)
        _conv3(y1, None, w2, 0, sc1, sh1, None, b2, None, None, None, y2, stats, B, T, 1, 0)
        lib.wm_bn_finalize(_p(stats), NCU, float(B * T), _p(g2), _p(be2), _p(rm2), _p(rv2), _p(nbt2), BN_MOMENTUM, BN_EPS,
                           _p(sc2), _p(sh2), _p(mu2), _p(is2), st)
    else:
        lib.wm_bn_eval_scale_shift(_p(g1), _p(be1), _p(rm1), _p(rv1), BN_EPS, _p(sc1), _p(sh1), st)
        lib.wm_bn_eval_scale_shift(_p(g2), _p(be2), _p(rm2), _p(rv2), BN_EPS, _p(sc2), _p(sh2), st)
        if not want_grad and _CONV["bf16x6"] and _CONV["one_launch_eval"]:
            # inference: the whole block is ONE launch -- x in, out out, the intermediate activation stays in LDS
            h = _CONV["eval_f16x3"]                     # f16 two-piece split (three products per product) | bf16x6
            wp1 = torch.empty((2 * 3 * 4096 + 4) if h else 3 * 3 * 4096, dtype=torch.int16, device=dev)   # both images alive at the launch
            wp2 = torch.empty_like(wp1)
            pack = lib.wm_pack_w64_h_scaled if h else lib.wm_pack_w64_bf_scaled
            pack(_p(w1), _p(sc1), _p(wp1), st)
            pack(_p(w2), _p(sc2), _p(wp2), st)
            lib.wm_resblock_eval_bf(_p(x), _p(wp1), _p(wp2), _p(b1), _p(sc1), _p(sh1), _p(b2), _p(sc2), _p(sh2), _p(out), B, T,
                                    1 if h else 0, st)
            return out, None
        y1 = torch.empty_like(x)
        _conv3(x, None, w1, 0, None, None, None, b1, None, None, None, y1, None, B, T, 0, 0)
        if not want_grad and _CONV["bf16x6"] and _CONV["schedule"] == 2 and T % 128 == 0:
            # inference: BN2 + residual add + ReLU ride in conv2's epilogue -- the block is two launches
            _conv3(y1, None, w2, 0, sc1, sh1, None, b2, x, sc2, sh2, out, None, B, T, 1, 4)
            return out, None
        y2 = torch.empty_like(x)
        _conv3(y1, None, w2, 0, sc1, sh1, None, b2, None, None, None, y2, None, B, T, 1, 0)
        # saved (mean, invstd) for an eval-mode backward = running statistics
        mu1.copy_(rm1); is1.copy_(torch.rsqrt(rv1 + BN_EPS)); mu2.copy_(rm2); is2.copy_(torch.rsqrt(rv2 + BN_EPS))
    more = () if pending is None else (pmask,)
    if not tail:
        return (None, BlockSaved(x, y1, y2, None, cst, w1, w2, g1, g2)) + more
    if want_grad:
        # the backward needs only the SIGN of `out`: one bit per element, written beside it (a frame pass less in backward)
        mask = torch.empty(B * 64 * ((T + 31) // 32), dtype=torch.int32, device=dev)
        lib.wm_bn_add_relu_mask(_p(x), _p(y2), _p(sc2), _p(sh2), _p(out), _p(mask), B, T, st)
    else:
        mask = None
        lib.wm_bn_add_relu(_p(x), _p(y2), _p(sc2), _p(sh2), _p(out), B, T, st)
    return (out, BlockSaved(x, y1, y2, mask, cst, w1, w2, g1, g2)) + more


class ResBlockFn(GradAwareFunction):
    """relu(x + BN2(conv2(relu(BN1(conv1(x))))))  -- ResBlock.forward, py/main16.py:124-125."""

    @staticmethod
    def forward(ctx, x, *args):
        params, (training,) = _cut(args, BlockParams)
        out, saved = _resblock_fwd(x, params, training, wants_grad(ctx))
        if saved is not None:
            ctx.training = bool(training)
            ctx.gdst = _gdst(params.w1, params.b1, params.w2, params.b2)
            ctx.save_for_backward(*saved)
        return out

    @staticmethod
    def backward(ctx, g_out):
        dx, *grads = _resblock_bwd(ctx.saved_tensors, ctx.training, ctx.gdst, g_out)
        return (dx,) + _block_grads(grads) + (None,)                          # (training: none)


def _resblock_bwd(saved, training, gdst, g_out):
    """Backward of one ResBlock: (dx, dw1, db1, dg1, dbe1, dw2, db2, dg2, dbe2).  The fused path where it applies, else one launch per
    product; gdst = the four weight-gradient destinations of _gdst (all None: fresh tensors, launched in line)."""
    x, y1, y2, mask, cst, w1, w2, g1, g2 = saved = BlockSaved._make(saved)
    sc1, sh1, mu1, is1, sc2, sh2, mu2, is2 = _bn_consts(cst)
    g_out = g_out.contiguous()
    B, _, T = x.shape
    dev, st, ev, n = x.device, _stream(), 0 if training else 1, float(B * T)
    if _CONV["bf16x6"] and _CONV["fused_bwd"] and T % 64 == 0 and not all(g is not None for g in gdst):
        dx, grads, _ = _resblock_bwd_fused(saved, training, g_out)
        return (dx,) + grads
    (dw1, db1, dw2, db2), acc, launch = _wgrad_dst(gdst, dev, w1.shape, (64,), w2.shape, (64,))
    part = _f32(max(B, 1) * 128, device=dev)
    dz2 = torch.empty_like(x)
    lib.wm_relu_bwd_reduce_mask(_p(g_out), _p(mask), _p(y2), _p(dz2), _p(part), None, B, T, st)
    k2, dg2, dbe2 = _f32(4, 64, device=dev), _f32(64, device=dev), _f32(64, device=dev)     # k: A, B (hi), B (lo), C -- B as hi + lo words
    lib.wm_bn_bwd_finalize(_p(part), B, n, _p(g2), _p(mu2), _p(is2), _p(k2[0]), _p(k2[1]), _p(k2[3]), _p(dg2), _p(dbe2), 0, ev, None, 0, None, st)
    # conv2: data gradient (+ ReLU mask + BN1-backward reductions in the epilogue) and weight gradient
    dz1, stats = torch.empty_like(x), _f32(NCU * 128, device=dev)
    _conv3(dz2, y2, w2, 1, k2[0], k2[1], k2[3], None, y1, sc1, sh1, dz1, stats, B, T, 3, 1)

    def wgrad(dz, y, k, xin, sc, sh, xpro, dw, db):
        wpart = _f32(2 * NCU * (3 * 4096 + 64), device=dev)
        if _CONV["bf16x6"]:
            lib.wm_wgrad64_bf(_p(dz), _p(y), _p(k[0]), _p(k[1]), _p(k[3]), _p(xin), _p(sc), _p(sh), _p(wpart), _p(dw), _p(db),
                              B, T, 3, xpro, 3 if acc else 0, _stream())
        else:
            lib.wm_wgrad64(_p(dz), _p(y), _p(k[0]), _p(k[1]), _p(k[3]), _p(xin), _p(sc), _p(sh), _p(wpart), _p(dw), _p(db),
                           B, T, 3, 3, xpro, 0, 1 if acc else 0, _stream())
    launch((dz2, y2, k2, y1, cst), lambda: wgrad(dz2, y2, k2, y1, sc1, sh1, 1, dw2, db2))
    k1, dg1, dbe1 = _f32(4, 64, device=dev), _f32(64, device=dev), _f32(64, device=dev)
    lib.wm_bn_bwd_finalize(_p(stats), NCU, n, _p(g1), _p(mu1), _p(is1), _p(k1[0]), _p(k1[1]), _p(k1[3]), _p(dg1), _p(dbe1), 0, ev, None, 0, None, st)
    # conv1: data gradient + residual path, weight gradient
    dx = torch.empty_like(x)
    _conv3(dz1, y1, w1, 1, k1[0], k1[1], k1[3], None, dz2, None, None, dx, None, B, T, 3, 2)
    launch((dz1, y1, k1, x), lambda: wgrad(dz1, y1, k1, x, None, None, 0, dw1, db1))
    g1_, g2_ = ((None, None),) * 2 if acc else ((dw1, db1), (dw2, db2))     # (dw / db stay bound: the queued launches read them later)
    return (dx,) + g1_ + (dg1, dbe1) + g2_ + (dg2, dbe2)


def _resblock_bwd_fused(saved, training, g_out, pre=None, fold=None, rank1=None, stem=None):
    """Backward of one ResBlock on the fused path (data + weight gradient of each convolution in one launch, T % 64 == 0).
    g_out: gradient w.r.t. the block output.  `pre` = (stats partials [NCU,2,64], max |dz| per workgroup [NCU]) when g_out ALREADY is
    dz2 = g (out > 0) and its two BatchNorm sums exist (made by the next block's folded conv1 launch): no reduction pass, no mask.
    `fold` = (mask, y2) of the block BEFORE this one: the conv1 launch then writes that block's dz2 instead of the plain input
    gradient and returns (its BatchNorm-sum partials, its max |dz| per workgroup) as the third value.
    `rank1` = (g1 [B,1,T], hw [1,64,1]), g_out None, neither `pre` nor `fold` (head1_rank1_applies): dout = hw[c] g1[b,t] is formed on load.
    `stem` = (s, w, b) of the Conv1d(1, 64, 7) whose output is this block's x (with `pre`): where _stem_in_dwgrad_launches, the conv1
    pair forms its weight-gradient operand from them instead of reading x (wm_dwgrad64_bf_stem).
    Returns (dx, (dw1, db1, dg1, dbe1, dw2, db2, dg2, dbe2), fold outputs | None)."""
    if (rank1 is not None and (pre is not None or fold is not None)) or (stem is not None and pre is None):
        raise ValueError("_resblock_bwd_fused: rank1 goes with neither pre nor fold, and stem needs pre")
    x, y1, y2, mask, cst, w1, w2, g1, g2 = BlockSaved._make(saved)
    sc1, sh1, mu1, is1, sc2, sh2, mu2, is2 = _bn_consts(cst)
    B, _, T = x.shape
    dev, st, ev, n = x.device, _stream(), 0 if training else 1, float(B * T)
    h, pack = (1, pack_w64_h) if _CONV["bwd_f16x3"] else (0, pack_w64_bf)      # the launches' arithmetic; the f16 split needs max |dz|
    k2, dg2, dbe2 = _f32(4, 64, device=dev), _f32(64, device=dev), _f32(64, device=dev)     # k: A, B (hi), B (lo), C -- B as hi + lo words
    gs2 = _f32(2, device=dev) if h else None
    if rank1 is not None:
        part, dzm = _f32(max(B, 1) * 128, device=dev), _f32(B * 64, device=dev)
        lib.wm_relu_bwd_reduce_mask_r1(*map(_p, rank1), _p(mask), _p(y2), _p(part), _p(dzm), B, T, st)
        gsrc, gm, sums = None, mask, (_p(part), B, _p(dzm), B * 64)
    elif pre is not None:
        gsrc, gm, sums = g_out, None, (_p(pre[0]), NCU, _p(pre[1]) if h else None, NCU)
    else:
        # dz2 = g_out * (out > 0) is never written (default): the reduction pass only forms the two BatchNorm sums, and the two
        # convolution-backward launches mask g_out with the same bits while they load it (wm_dwgrad64_bf's gmask)
        part, dzm = _f32(max(B, 1) * 128, device=dev), (_f32(B * 64, device=dev) if h else None)
        dz2 = None if _CONV["mask_on_load"] else torch.empty_like(x)
        lib.wm_relu_bwd_reduce_mask(_p(g_out), _p(mask), _p(y2), _p(dz2), _p(part), _p(dzm), B, T, st)
        gsrc, gm, sums = *((g_out, mask) if dz2 is None else (dz2, None)), (_p(part), B, _p(dzm), B * 64)
    lib.wm_bn_bwd_finalize(sums[0], sums[1], n, _p(g2), _p(mu2), _p(is2), _p(k2[0]), _p(k2[1]), _p(k2[3]), _p(dg2), _p(dbe2), 0, ev,
                           sums[2], sums[3], _p(gs2), st)         # sums: partials, their count, max |dz2| per slot, the slots
    # conv2: data gradient (+ ReLU mask + BN1-backward reductions in the epilogue) and weight gradient
    dz1, stats = torch.empty_like(x), _f32(NCU * 128, device=dev)
    dzm1 = _f32(NCU, device=dev) if h else None          # max |dz1| per workgroup, written by the conv2-pair launch
    dw2, db2, dw1, db1 = torch.empty_like(w2), _f32(64, device=dev), torch.empty_like(w1), _f32(64, device=dev)
    wpart = _f32(NCU * (3 * 4096 + 64), device=dev)

    def pair(*, g, y, k, w, out, dw, db, gs, omax, xw=None, xa=None, xb=None, e1=None, ea=None, eb=None, stats=None, xpro=0, epi=2,
             stem=None):    # one pair launch, argument names as in wm_dwgrad64_bf's prototype; its _r1 twin under rank1, _stem with `stem`
        head = (_p(g), _p(y), _p(k[0]), _p(k[1]), _p(k[3]), _p(pack(w, 1)))
        if stem is not None:
            return lib.wm_dwgrad64_bf_stem(*head, _p(e1), _p(out), _p(wpart), _p(dw), _p(db), B, T, 0, _p(gs), _p(omax), *map(_p, stem), st)
        entry = lib.wm_dwgrad64_bf if rank1 is None else lib.wm_dwgrad64_bf_r1
        entry(*head, _p(xw), _p(xa), _p(xb), _p(e1), _p(ea), _p(eb), _p(out), _p(stats), _p(wpart), _p(dw), _p(db), B, T, xpro, epi, 0,
              _p(gm), h, _p(gs), _p(omax), *map(_p, rank1 or ()), st)
    pair(g=gsrc, y=y2, k=k2, w=w2, xw=y1, xa=sc1, xb=sh1, xpro=1, e1=y1, ea=sc1, eb=sh1, epi=1, out=dz1, stats=stats, omax=dzm1,
         dw=dw2, db=db2, gs=gs2)
    k1, dg1, dbe1 = _f32(4, 64, device=dev), _f32(64, device=dev), _f32(64, device=dev)
    gs1 = _f32(2, device=dev) if h else None
    lib.wm_bn_bwd_finalize(_p(stats), NCU, n, _p(g1), _p(mu1), _p(is1), _p(k1[0]), _p(k1[1]), _p(k1[3]), _p(dg1), _p(dbe1), 0, ev,
                           _p(dzm1), NCU, _p(gs1), st)
    dx, fout = torch.empty_like(x), None
    conv1 = dict(g=dz1, y=y1, k=k1, w=w1, out=dx, dw=dw1, db=db1, gs=gs1)
    if fold is not None and gm is not None:
        # conv1 pair that also does the PREVIOUS block's ReLU backward and BatchNorm sums (epi 8): dx leaves as that block's dz2
        pmask, py2 = fold
        fpart, fmax = _f32(NCU * 128, device=dev), (_f32(NCU, device=dev) if h else None)
        pair(xw=x, e1=gsrc, ea=py2, eb=pmask, epi=8, stats=fpart, omax=fmax, **conv1)
        fout = (fpart, fmax)
    else:
        xmax = _f32(NCU, device=dev) if h else None          # max |dx| per workgroup: a consumer that splits dx into f16 pieces
        if stem is not None and _stem_in_dwgrad_launches(x):
            pair(e1=gsrc, omax=xmax, stem=stem, **conv1)
        else:
            pair(xw=x, e1=gsrc, omax=xmax, **conv1)          # (rank1: gsrc is None, the addend is formed on load)
        if h:
            _note_gmax(dx, xmax)                             # (ConvT7Fn.backward) then needs no pass over it for its scale
    return dx, (dw1, db1, dg1, dbe1, dw2, db2, dg2, dbe2), fout


def pair_node_applies(x) -> bool:
    """ResBlockPairFn's precondition on input and switches (the caller adds: both blocks in training mode, no forward hooks)"""
    return (torch.is_grad_enabled() and x.is_cuda and x.dim() == 3 and x.shape[-1] % 64 == 0 and _CONV["bf16x6"]
            and _CONV["fused_bwd"] and _CONV["mask_on_load"] and _CONV["pair_fold"] and not _ASYNC["on"])


def _pair_fwd(x, p1, p2, training, want_grad, tail=True, stem=None):
    """Two ResBlocks in a row, the second up to `tail` (as _resblock_fwd's): (out | None, first, second), the two blocks' `saved`; stem
    as _resblock_fwd's.  Where the tail-in-consumer launches apply, the second block's conv1 launch forms the first block's tail."""
    if training and _tail_in_consumer_launches(x if stem is None else stem[0]):
        _, first = _resblock_fwd(x, p1, True, want_grad, tail=False, stem=stem)
        out, second, pmask = _resblock_fwd(None, p2, True, want_grad, tail=tail, pending=first)
        return out, first._replace(mask=pmask), second
    mid, first = _resblock_fwd(x, p1, training, want_grad, stem=stem)
    out, second = _resblock_fwd(mid, p2, training, want_grad, tail=tail)
    return out, first, second


def _pair_bwd(first, second, training, g_out, stem=None):
    """ResBlockPairFn's backward on _pair_fwd's two `saved`: (dx, both blocks' _block_grads in a row).  stem: unused if nothing was folded"""
    dmid, grads2, fout = _resblock_bwd_fused(second, training, g_out, fold=(first.mask, first.y2))
    dx, grads1, _ = _resblock_bwd_fused(first, training, dmid, pre=fout, stem=stem if stem and fout else None)
    return dx, _block_grads(grads1) + _block_grads(grads2)


class ResBlockPairFn(GradAwareFunction):
    """Two ResBlocks in a row (py/main16.py:135-136 encoder.1 -> encoder.2, :178-179 model.1 -> model.2) as one tape node.
    Forward = _resblock_fwd twice.  Backward: the second block's conv1 launch (data + weight gradient) applies the
    FIRST block's ReLU mask to the gradient it has just formed and accumulates that block's two BatchNorm sums in its epilogue
    (wm_dwgrad64_bf epi 8), so the first block needs no reduction pass and the gradient between the blocks is written once, masked.
    Used by modules.resblock_pair when the fused path applies (bf16x6, T % 64 == 0, mask-on-load, gradients wanted)."""

    @staticmethod
    def forward(ctx, x, *args):
        return _pair_node_fwd(ctx, x, args, None)

    @staticmethod
    def backward(ctx, g_out):
        return _behind_stem(ctx, *_pair_node_bwd(ctx, g_out))


def _pair_node_fwd(ctx, x, args, stem):
    p1, p2, (training,) = _cut(args, BlockParams, BlockParams)
    out, first, second = _pair_fwd(x, p1, p2, training, wants_grad(ctx), stem=stem)
    ctx.save_for_backward(*first, *second, *(stem or ()))
    ctx.training = bool(training)
    return out


def _pair_node_bwd(ctx, g_out):
    first, second, stem = _cut(ctx.saved_tensors, BlockSaved, BlockSaved)
    dx, grads = _pair_bwd(first, second, ctx.training, g_out.contiguous(), stem)
    return dx, grads + (None,), stem                                          # (training: none)


def _behind_stem(ctx, dx, rest, stem, between=()):
    """a node's return value: (dx,) -- behind a saved stem (ds, dw, db) from wm_stem_bwd on dx, exactly as StemFn.backward runs it --
    then `between` (the arguments in front of the blocks' that get no gradient), then rest (the gradients of `args`)"""
    if not stem:
        return (dx,) + between + rest
    s, w, _ = stem
    return _stem_bwd(s, w, dx, ctx.grad_rows, ctx.needs_input_grad[0]) + between + rest


class StemResBlockPairFn(GradAwareFunction):
    """model.0 -> model.1 -> model.2 (py/main16.py:177-179) as one tape node where stem_in_conv1_applies(s): ResBlockPairFn on the
    stem's output, which model.1's conv1 launch forms from the clips and writes (wm_conv64_bf_stem), and which model.1's conv1 pair in
    the backward forms again instead of reading it (wm_dwgrad64_bf_stem).  Inputs (s, stem w, stem b, grad_rows | None, ...
    ResBlockPairFn's); backward = ResBlockPairFn's, then StemFn's."""

    @staticmethod
    def forward(ctx, s, sw, sb, grad_rows, *args):
        s = _frames(s, "clip batch", 1)
        ctx.grad_rows = _stem_grad_rows(grad_rows, s.shape[0])
        return _pair_node_fwd(ctx, None, args, (s, sw, sb))

    @staticmethod
    def backward(ctx, g_out):
        return _behind_stem(ctx, *_pair_node_bwd(ctx, g_out), between=(None,))                  # (grad_rows: none)


# ------------------------------------------------------------------------------------------ stem / heads
class StemFn(torch.autograd.Function):
    """Conv1d(1, 64, 7, padding=3) -- py/main16.py:134 / :177."""

    @staticmethod
    def forward(ctx, s, w, b, grad_rows=None):
        s = _frames(s, "clip batch", 1)
        B, _, T = s.shape
        y = _f32(B, 64, T, device=s.device)
        lib.wm_stem_fwd(_p(s), _p(w), _p(b), _p(y), B, T, _stream())
        ctx.save_for_backward(s, w)
        ctx.grad_rows = _stem_grad_rows(grad_rows, B)
        return y

    @staticmethod
    def backward(ctx, g):
        s, w = ctx.saved_tensors
        return _stem_bwd(s, w, g, ctx.grad_rows, ctx.needs_input_grad[0]) + (None,)


def _stem_grad_rows(grad_rows, B):
    return B if grad_rows is None else max(0, min(int(grad_rows), B))


def _stem_bwd(s, w, g, grad_rows, need_ds):
    """StemFn's backward launch on the gradient g of the stem's output: (ds | None, dw, db)"""
    g = g.contiguous()
    B, _, T = s.shape
    ds = None
    if need_ds:                            # rows >= grad_rows are known not to need a gradient (the clean half): left zero
        ds = torch.empty_like(s) if grad_rows == B else torch.zeros_like(s)
    part = _f32(2 * NCU * 512, device=s.device)
    dw, db = torch.empty_like(w), _f32(64, device=s.device)
    lib.wm_stem_bwd(_p(g), _p(s), _p(w), _p(ds), _p(part), _p(dw), _p(db), B, T, grad_rows, 0, _stream())
    return ds, dw, db


class Head1Fn(torch.autograd.Function):
    """Conv1d(64, 1, 1) -- Generator.decoder[2], py/main16.py:146."""

    @staticmethod
    def forward(ctx, x, w, b):
        x = _frames(x, "head input", 64)
        B, _, T = x.shape
        y = _f32(B, 1, T, device=x.device)
        lib.wm_head1_fwd(_p(x), _p(w), _p(b), _p(y), B, T, _stream())
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = g.contiguous()
        B, _, T = x.shape
        dx = torch.empty_like(x)
        part = _f32(1024 * 65, device=x.device)
        dw, db = torch.empty_like(w), _f32(1, device=x.device)
        lib.wm_head1_bwd(_p(g), _p(x), _p(w), _p(dx), _p(part), _p(dw), _p(db), B, T, 0, _stream())
        return dx, dw, db


class HeadNFn(torch.autograd.Function):
    """Conv1d(64, 1+bits, 1) followed by permute(0,2,1) -- Detector, py/main16.py:180,186.
    Returns a contiguous (B, T, 1+bits) tensor (the reference returns a view of the same shape)."""

    @staticmethod
    def forward(ctx, x, w, b):
        x = _frames(x, "head input", 64)
        B, _, T = x.shape
        NO = w.shape[0]
        if not 1 <= NO <= 64:
            raise ValueError(f"Detector head: 1+message_bits must be in 1..64 (message ids are int64, so a message "
                             f"carries at most 63 bits), got {NO}")
        y = _f32(B, T, NO, device=x.device)
        lib.wm_headN_fwd(_p(x), _p(w), _p(b), _p(y), B, T, NO, _stream())
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = g.contiguous()
        B, _, T = x.shape
        NO = w.shape[0]
        dx = torch.empty_like(x)
        part = _f32(NCU * (NO * 64 + NO), device=x.device)
        dw, db = torch.empty_like(w), _f32(NO, device=x.device)
        lib.wm_headN_bwd(_p(g), _p(x), _p(w), _p(dx), _p(part), _p(dw), _p(db), B, T, NO, 0, _stream())
        return dx, dw, db


# ------------------------------------------------------------------------------------------ last ResBlock + head
def tail_in_head_applies(x) -> bool:
    """the switch and what both nodes below ask of their input (the caller adds: training-mode blocks, no forward hooks)"""
    return _HEADS["tail_in_head"] and x.is_cuda and x.dim() == 3 and not _ASYNC["on"]


def _tail_mask(x, want_grad):
    B, _, T = x.shape
    return torch.empty(B * 64 * ((T + 31) // 32), dtype=torch.int32, device=x.device) if want_grad else None


class ResBlockHead1Fn(GradAwareFunction):
    """decoder.1 -> decoder.2 (py/main16.py:145-146) in training mode as one tape node: the block's tail is formed inside the head's
    forward kernel (wm_head1_tail_fwd), so its output frame is written once and not read back.  Backward = Head1Fn's, then ResBlockFn's."""

    @staticmethod
    def forward(ctx, x, *args):
        params, (hw, hb) = _cut(args, BlockParams)
        want = wants_grad(ctx)
        _, saved = _resblock_fwd(x, params, True, want, tail=False)
        x = saved.x
        B, _, T = x.shape
        out, mask = torch.empty_like(x), _tail_mask(x, want)
        y = _f32(B, 1, T, device=x.device)
        lib.wm_head1_tail_fwd(_p(x), _p(saved.y2), _p(saved.sc2), _p(saved.sh2), _p(hw), _p(hb), _p(out), _p(mask), _p(y), B, T, _stream())
        if want:
            ctx.save_for_backward(*saved._replace(mask=mask), out, hw)
        return y

    @staticmethod
    def backward(ctx, g):
        saved, (out, hw) = _cut(ctx.saved_tensors, BlockSaved)
        B, _, T = out.shape
        g = g.contiguous()
        part = _f32(1024 * 65, device=out.device)
        dhw, dhb = torch.empty_like(hw), _f32(1, device=out.device)
        if head1_rank1_applies(out):
            # dout[b,c,t] = hw[c] g[b,t] stays out of memory: the block's three readers of it form it on load
            lib.wm_head1_bwd(_p(g), _p(out), _p(hw), None, _p(part), _p(dhw), _p(dhb), B, T, 0, _stream())
            dx, grads, _ = _resblock_bwd_fused(saved, True, None, rank1=(g, hw))
        else:
            dout = torch.empty_like(out)
            lib.wm_head1_bwd(_p(g), _p(out), _p(hw), _p(dout), _p(part), _p(dhw), _p(dhb), B, T, 0, _stream())
            dx, *grads = _resblock_bwd(saved, True, (None,) * 4, dout)
        return (dx,) + _block_grads(grads) + (dhw, dhb)


class DetectorTailFn(GradAwareFunction):
    """model.1 -> model.2 -> model.3 (py/main16.py:178-180) with both BCE terms (:252-264) as one tape node, for the train step on
    the fused path (pair_node_applies).  Forward: ResBlockPairFn's, except that model.2's tail, the head and the two loss sums are one
    launch (wm_headN_tail_fwd) -> (logits, loc, bce).  Backward: the head's backward forms the losses' gradient from the logits while
    it loads them (wm_headN_bwd_bce), then ResBlockPairFn's backward.  A gradient arriving on `logits` takes the unfused route:
    wm_bce_bwd's tensor plus that gradient through wm_headN_bwd."""

    @staticmethod
    def forward(ctx, x, message, *args):
        return _detector_tail_fwd(ctx, x, message, args, None)

    @staticmethod
    def backward(ctx, g_logits, g_loc, g_bce):
        return _behind_stem(ctx, *_detector_tail_bwd(ctx, g_logits, g_loc, g_bce), between=(None,))          # (message: none)


class StemDetectorTailFn(GradAwareFunction):
    """model.0 in front of DetectorTailFn as one tape node where stem_in_conv1_applies(s): as StemResBlockPairFn.  Inputs (s, stem w,
    stem b, grad_rows | None, message, ... DetectorTailFn's); backward = DetectorTailFn's, then StemFn's."""

    @staticmethod
    def forward(ctx, s, sw, sb, grad_rows, message, *args):
        s = _frames(s, "clip batch", 1)
        ctx.grad_rows = _stem_grad_rows(grad_rows, s.shape[0])
        return _detector_tail_fwd(ctx, None, message, args, (s, sw, sb))

    @staticmethod
    def backward(ctx, g_logits, g_loc, g_bce):
        return _behind_stem(ctx, *_detector_tail_bwd(ctx, g_logits, g_loc, g_bce), between=(None, None))     # (grad_rows, message: none)


def _detector_tail_fwd(ctx, x, message, args, stem):
    p1, p2, (hw, hb) = _cut(args, BlockParams, BlockParams)
    want = wants_grad(ctx)
    _, first, second = _pair_fwd(x, p1, p2, True, want, tail=False, stem=stem)
    mid = second.x
    R, _, T = mid.shape
    NO, B, dev = hw.shape[0], message.shape[0], mid.device
    out, mask = torch.empty_like(mid), _tail_mask(mid, want)
    logits = _f32(R, T, NO, device=dev)
    part = _f32(2 * R * ((T + 255) // 256), device=dev)
    losses = torch.zeros(2, dtype=torch.float32, device=dev)
    lib.wm_headN_tail_fwd(_p(mid), _p(second.y2), _p(second.sc2), _p(second.sh2), _p(hw), _p(hb), _p(message), B, _p(part),
                          _p(losses[0]), _p(losses[1]), _p(out), _p(mask), _p(logits), R, T, NO, _stream())
    ctx.set_materialize_grads(False)
    if want:
        ctx.save_for_backward(*first, *second._replace(mask=mask), out, hw, logits, message, *(stem or ()))
    return logits, losses[0], losses[1]


def _detector_tail_bwd(ctx, g_logits, g_loc, g_bce):
    first, second, (out, hw, logits, message, *stem) = _cut(ctx.saved_tensors, BlockSaved, BlockSaved)
    R, T, NO = logits.shape
    dev, st = logits.device, _stream()
    gl = g_loc.contiguous().float().reshape(1) if g_loc is not None else torch.zeros(1, device=dev)
    gb = g_bce.contiguous().float().reshape(1) if g_bce is not None else torch.zeros(1, device=dev)
    dout = torch.empty_like(out)
    part = _f32(NCU * (NO * 64 + NO), device=dev)
    dhw, dhb = torch.empty_like(hw), _f32(NO, device=dev)
    if g_logits is None:
        lib.wm_headN_bwd_bce(_p(logits), _p(message), _p(gl), _p(gb), _p(out), _p(hw), _p(dout), _p(part), _p(dhw), _p(dhb),
                             message.shape[0], R, T, NO, 0, st)
    else:
        d = torch.empty_like(logits)
        lib.wm_bce_bwd(_p(logits), _p(message), _p(gl), _p(gb), _p(d), message.shape[0], R, T, NO, st)
        d += g_logits
        lib.wm_headN_bwd(_p(d), _p(out), _p(hw), _p(dout), _p(part), _p(dhw), _p(dhb), R, T, NO, 0, st)
    dx, grads = _pair_bwd(first, second, True, dout, stem)
    return dx, grads + (dhw, dhb), stem


# ------------------------------------------------------------------------------------------ LSTM
class LSTMFn(GradAwareFunction):
    """nn.LSTM(64,64,batch_first=True) on channel-first frames: (B,64,T) -> (B,64,T); the two permutes of
    py/main16.py:152,154 are folded into the kernels' addressing."""

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh):
        need_grad = wants_grad(ctx)
        h, saved = _lstm_fwd(x, w_ih, w_hh, b_ih, b_hh, need_grad)
        if need_grad:
            ctx.gdst = _gdst(w_ih, w_hh, b_ih, b_hh)
            ctx.save_for_backward(*saved)
        return h

    @staticmethod
    def backward(ctx, dh):
        saved = ctx.saved_tensors
        _single_backward(ctx, "LSTMFn")
        return _lstm_bwd(saved, ctx.gdst, dh)


def _lstm_fwd(x, w_ih, w_hh, b_ih, b_hh, need_grad, tail=None):
    """LSTMFn's forward: (h, saved) with saved = an LstmSaved for _lstm_bwd, None unless need_grad.  No ctx.
    tail = (xres, y2, sc2, sh2, mask | None) of the ResBlock in front (tail_in_consumer_applies with lstm=True; x is ignored): the
    launch (wm_lstm_fwd_tail) forms that block's output on load and writes it -- the LSTM's x -- and the mask."""
    if tail is not None:
        xres, y2, sc2, sh2, mask = tail
        x = torch.empty_like(xres)
    x = _frames(x, "LSTM input", 64)
    B, _, T = x.shape
    dev, st = x.device, _stream()
    h = torch.empty_like(x)
    release_deferred_wgrads()                  # side stream: work queued for "beside the recurrence" starts now (eval_forward)
    cst = _f32(B, T, 64, device=dev) if need_grad else None
    if tail is not None:
        gates = _f32(B, T, 256, device=dev) if need_grad else None
        lib.wm_lstm_fwd_tail(_p(xres), _p(y2), _p(sc2), _p(sh2), _p(x), _p(mask), _p(w_ih), _p(b_ih), _p(b_hh), _p(w_hh), _p(h),
                             _p(gates), _p(cst), B, T, st)
    elif _LSTM["fused"] and T >= 8:             # input projection inside the recurrence kernel (no xp tensor)
        gates = _f32(B, T, 256, device=dev) if need_grad else None
        lib.wm_lstm_fwd_fused(_p(x), _p(w_ih), _p(b_ih), _p(b_hh), _p(w_hh), _p(h), _p(gates), _p(cst), B, T, st)
    else:
        xp = _f32(B, T, 256, device=dev)
        lib.wm_lstm_xproj(_p(x), _p(w_ih), _p(b_ih), _p(b_hh), _p(xp), B, T, st)
        gates = xp if need_grad else None       # activations overwrite the projections in place
        lib.wm_lstm_fwd(_p(xp), _p(w_hh), _p(h), _p(gates), _p(cst), B, T, st)
    return h, (LstmSaved(x, h, gates, cst, w_ih, w_hh) if need_grad else None)


def _lstm_bwd(saved, gdst, dh, dx_inside=False):
    """LSTMFn's backward on _lstm_fwd's saved tensors: (dx, dw_ih, dw_hh, db_ih, db_hh); gdst = the four destinations of _gdst.
    dx_inside (EncoderLSTMFn, set_lstm_dx_in_bwd): dx comes out of the wave-specialised BPTT launch itself, unless the side-stream
    option is on.  (The library's own fp32 choice, wm_set_lstm_dx_bf16x6(0), is not visible here: the entry point honours it.)"""
    x, h, gates, cst, w_ih, w_hh = LstmSaved._make(saved)
    dh = dh.contiguous()
    B, _, T = x.shape
    dev, st = x.device, _stream()
    dx = torch.empty_like(x)
    release_deferred_wgrads()                  # side stream: the queued weight-gradient GEMMs run beside the recurrence
    dst, acc, launch = _wgrad_dst(gdst, dev, w_ih.shape, w_hh.shape, (256,), (256,))     # dwi, dwh, dbi, dbh
    if _LSTM["bwd_ws"] and not _LSTM["bwd_fused"] and T % 32 == 0 and T >= 64:
        part = _f32(B * (256 * 128 + 256), device=dev)       # (this launch accumulates into the flat store from the main stream)
        if dx_inside and not _ASYNC["on"]:
            lib.wm_lstm_bwd_wgrad_dx(_p(gates), _p(cst), _p(dh), _p(w_hh), _p(w_ih), _p(x), _p(h), _p(part), *map(_p, dst), _p(dx),
                                     B, T, int(acc), st)
            return (dx,) + ((None,) * 4 if acc else dst)
        lib.wm_lstm_bwd_wgrad(_p(gates), _p(cst), _p(dh), _p(w_hh), _p(x), _p(h), _p(part), *map(_p, dst), B, T, int(acc), st)
        lib.wm_lstm_dx(_p(gates), _p(w_ih), _p(dx), B, T, st)
        return (dx,) + ((None,) * 4 if acc else dst)
    if _LSTM["bwd_fused"]:                    # measured: no faster than the two launches; off by default
        lib.wm_lstm_bwd_fused(_p(gates), _p(cst), _p(dh), _p(w_hh), _p(w_ih), _p(dx), B, T, st)   # gates now holds da
    else:
        lib.wm_lstm_bwd(_p(gates), _p(cst), _p(dh), _p(w_hh), B, T, st)      # gates now holds da
        lib.wm_lstm_dx(_p(gates), _p(w_ih), _p(dx), B, T, st)

    def wg():
        part = _f32(NCU * (256 * 128 + 256), device=dev)
        lib.wm_lstm_wgrad(_p(gates), _p(x), _p(h), _p(part), *map(_p, dst), B, T, int(acc), _stream())
    launch((gates, x, h), wg)
    return (dx,) + ((None,) * 4 if acc else dst)


class EncoderLSTMFn(GradAwareFunction):
    """encoder.1 -> encoder.2 -> lstm (py/main16.py:135-136, :152-154) as one tape node, for the train step where
    tail_in_consumer_applies(x, lstm=True): encoder.1's tail is formed by encoder.2's conv1 launch (wm_conv64_bf_tail) and encoder.2's
    by the LSTM forward's helper waves (wm_lstm_fwd_tail), so neither block has a tail launch of its own.  The saved tensors are
    ResBlockPairFn's eighteen and LSTMFn's six; backward = LSTMFn's, then ResBlockPairFn's."""

    @staticmethod
    def forward(ctx, x, *args):
        return _encoder_lstm_fwd(ctx, x, args, None)

    @staticmethod
    def backward(ctx, dh):
        return _behind_stem(ctx, *_encoder_lstm_bwd(ctx, dh))


class StemEncoderLSTMFn(GradAwareFunction):
    """encoder.0 in front of EncoderLSTMFn as one tape node where stem_in_conv1_applies(s, lstm=True): as StemResBlockPairFn.  Inputs
    (s, stem w, stem b, ... EncoderLSTMFn's); backward = EncoderLSTMFn's, then StemFn's."""

    @staticmethod
    def forward(ctx, s, sw, sb, *args):
        s = _frames(s, "clip batch", 1)
        ctx.grad_rows = s.shape[0]
        return _encoder_lstm_fwd(ctx, None, args, (s, sw, sb))

    @staticmethod
    def backward(ctx, dh):
        return _behind_stem(ctx, *_encoder_lstm_bwd(ctx, dh))


def _encoder_lstm_fwd(ctx, x, args, stem):
    p1, p2, (w_ih, w_hh, b_ih, b_hh) = _cut(args, BlockParams, BlockParams)
    want = wants_grad(ctx)
    _, first, second = _pair_fwd(x, p1, p2, True, want, tail=False, stem=stem)
    mask = _tail_mask(second.x, want)
    h, lsaved = _lstm_fwd(None, w_ih, w_hh, b_ih, b_hh, want, tail=(second.x, second.y2, second.sc2, second.sh2, mask))
    if want:
        ctx.gdst = _gdst(w_ih, w_hh, b_ih, b_hh)
        ctx.save_for_backward(*first, *second._replace(mask=mask), *lsaved, *(stem or ()))
    return h


def _encoder_lstm_bwd(ctx, dh):
    first, second, lsaved, stem = _cut(ctx.saved_tensors, BlockSaved, BlockSaved, LstmSaved)
    _single_backward(ctx, "EncoderLSTMFn")
    dmid, *lgrads = _lstm_bwd(lsaved, ctx.gdst, dh, dx_inside=_LSTM_DX["in_bwd"])
    dx, grads = _pair_bwd(first, second, True, dmid, stem)
    return dx, grads + tuple(lgrads), stem


# ------------------------------------------------------------------------------------------ embedding + convT
# The reference's nn.Embedding raises IndexError for an out-of-range message id (on its CUDA device: a device-side assert that
# surfaces at a later synchronisation).  Three modes (set_index_check / WM_CHECK_INDEX):
#   "sync"     (default) read the 4-byte error flag back at once and raise -- one device->host sync per Generator call;
#   "deferred" copy the flag to pinned memory asynchronously and raise at the NEXT lookup (or check_message_ids()): no
#              sync, the launch queue never drains -- what train_step uses (a mid-step sync costs the config-5 step 6 ms: its
#              LSTM chain is 200 short launches the host can only cover when it runs ahead);
#   "off"      no check (out-of-range ids read as a zero row).
_CHECK_INDEX = {"mode": {"1": "sync", "0": "off"}.get(os.environ.get("WM_CHECK_INDEX", "1"), os.environ.get("WM_CHECK_INDEX", "sync")),
                "pending": []}


def set_index_check(mode):
    """True / "sync" | "deferred" | False / "off" """
    _CHECK_INDEX["mode"] = {True: "sync", False: "off"}.get(mode, mode)
    if _CHECK_INDEX["mode"] not in ("sync", "deferred", "off"):
        raise ValueError("index check mode must be 'sync', 'deferred' or 'off'")


@contextlib.contextmanager
def index_check_mode(mode=None):
    """context manager: run a block under another index-check mode; None (a train step's forward): "sync" becomes "deferred", the others stay"""
    prev = _CHECK_INDEX["mode"]
    set_index_check(("deferred" if prev == "sync" else prev) if mode is None else mode)
    try:
        yield
    finally:
        _CHECK_INDEX["mode"] = prev


def index_check() -> str:                       # "sync" | "deferred" | "off"
    return _CHECK_INDEX["mode"]


def check_message_ids(wait=True, what="an earlier Generator call"):
    """raise IndexError if a deferred message-id check has failed (wait=False: only look at flags that have already landed)"""
    keep = []
    for ev, host, nrows in _CHECK_INDEX["pending"]:
        if not wait and not ev.query():
            keep.append((ev, host, nrows))
            continue
        ev.synchronize()
        if int(host[0]) != 0:
            _CHECK_INDEX["pending"] = []
            raise IndexError(f"message id out of range for an embedding table of {nrows} rows (deferred check of {what})")
    _CHECK_INDEX["pending"] = keep


def drop_pending_message_checks():
    """forget deferred checks that have not been read yet (their step was abandoned)"""
    _CHECK_INDEX["pending"] = []


def _note_index_error(err, nrows):
    """err: int32 device tensor (non-zero = some id was out of range), handled according to the current mode"""
    mode = _CHECK_INDEX["mode"]
    if mode == "off":
        return
    if mode == "sync":
        if int(err.item()) != 0:
            raise IndexError(f"message id out of range for an embedding table of {nrows} rows")
        return
    check_message_ids(wait=False)                    # flags of earlier calls that have landed by now
    host = torch.empty(1, dtype=torch.int32, pin_memory=True)
    host.copy_(err, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    _CHECK_INDEX["pending"].append((ev, host, nrows))


class EmbedFn(torch.autograd.Function):
    """nn.Embedding lookup, py/main16.py:158 (dense gradient like the reference's sparse=False table)."""

    @staticmethod
    def forward(ctx, table, message):
        table = _chk(table, "embedding.weight", 2)
        message = _chk(message, "message", 1, torch.int64)
        B = message.shape[0]
        vec = _f32(B, 64, device=table.device)
        err = torch.zeros(1, dtype=torch.int32, device=table.device)
        lib.wm_embed_gather(_p(table), _p(message), _p(vec), B, table.shape[0], _p(err), _stream())
        _note_index_error(err, table.shape[0])                 # nn.Embedding raises IndexError (py/main16.py:158)
        ctx.save_for_backward(message)
        ctx.nrows = table.shape[0]
        return vec

    @staticmethod
    def backward(ctx, dvec):
        (message,) = ctx.saved_tensors
        dtable = torch.zeros(ctx.nrows, 64, dtype=torch.float32, device=dvec.device)
        lib.wm_embed_scatter_add(_p(dtable), _p(message), _p(dvec.contiguous()), message.shape[0], ctx.nrows, _stream())
        return dtable, None


def _conv7_arith(T) -> str:
    """arithmetic of the 7-tap 64->64 convolution on clips of T samples (forward, data gradient and weight gradient alike)"""
    return "fp32" if not _CONV["bf16x6"] else "f16x3" if _CONV["conv7_f16x3"] and T % 128 == 0 else "bf16x6"


def _conv7(arith, x, w, wmode, vec, b, y, B, T, pro, epi, gsc, st):
    """one k7 64->64 convolution launch (wmode / epi 2 / 0: ConvTranspose1d forward, 3 / 3: its data gradient) in arithmetic `arith`"""
    if arith == "fp32":
        lib.wm_conv64(_p(x), None, _p(pack_w64(w, 7, wmode)), _p(vec), None, None, _p(b), None, None, None, _p(y), None, B, T, 7, pro, epi, st)
    else:
        h = arith == "f16x3"
        lib.wm_conv64_bf7(_p(x), _p((pack_w64_h7 if h else pack_w64_bf7)(w, wmode)), _p(vec), _p(b), _p(y), B, T, pro, epi, int(h), _p(gsc), st)


class ConvT7Fn(torch.autograd.Function):
    """ConvTranspose1d(64,64,7,padding=3) applied to x + emb[:, :, None]  (py/main16.py:144,156-161);
    `vec` (B,64) is the looked-up embedding row or None."""

    @staticmethod
    def forward(ctx, x, vec, w, b):
        x = _frames(x, "decoder input", 64)
        B, _, T = x.shape
        y = torch.empty_like(x)
        _conv7(_conv7_arith(T), x, w, 2, vec, b, y, B, T, 2 if vec is not None else 0, 0, None, _stream())
        ctx.has_vec = vec is not None
        ctx.gdst = _gdst(w, b)
        ctx.save_for_backward(x, w, vec if vec is not None else x.new_empty(0))
        return y

    @staticmethod
    def backward(ctx, g):
        x, w, vec = ctx.saved_tensors
        vec = vec if ctx.has_vec else None
        g = g.contiguous()
        B, _, T = x.shape
        dev, st = x.device, _stream()
        dx = torch.empty_like(x)
        arith = _conv7_arith(T)
        h = arith == "f16x3"
        gsc = gscale_of(g) if h else None               # the scale both f16-split launches apply to g (.contiguous() above returns g itself)
        _conv7(arith, g, w, 3, None, None, dx, B, T, 0, 3, gsc, st)
        (dw, db), acc, launch = _wgrad_dst(ctx.gdst, dev, w.shape, (64,))
        pro = 2 if vec is not None else 0

        def wg():
            part = _f32(2 * NCU * (7 * 4096 + 64), device=dev)
            if arith == "fp32":
                lib.wm_wgrad64(_p(g), None, None, None, None, _p(x), _p(vec), None, _p(part), _p(dw), _p(db), B, T, 7, 0, pro, 1, int(acc),
                               _stream())
            else:
                lib.wm_wgrad64_bf7(_p(g), _p(x), _p(vec), _p(part), _p(dw), _p(db), B, T, pro, int(acc), int(h), _p(gsc), _stream())
        launch((g, x, vec, gsc), wg)
        dvec = None
        if vec is not None and ctx.needs_input_grad[1]:
            dvec = _f32(B, 64, device=dev)
            lib.wm_rowsum(_p(dx), _p(dvec), B * 64, T, st)
        return (dx, dvec) + ((None, None) if acc else (dw, db))


# ------------------------------------------------------------------------------------------ delta post-processing
class PostprocFn(torch.autograd.Function):
    """stages bit0 fir_lowpass | bit1 clamp_peak | bit2 limit_rms, fused (py/main16.py:53-72, :245-247)."""

    @staticmethod
    def forward(ctx, delta, taps, thr, max_rms, eps, stages):
        delta = _frames(delta, "delta", 1)
        B, _, T = delta.shape
        dev = delta.device
        out = torch.empty_like(delta)
        need = ctx.needs_input_grad[0]
        f = torch.empty_like(delta) if need else None
        stats = _f32(B, 2, device=dev)
        lib.wm_postproc_fwd(_p(delta), _p(taps), taps.numel(), thr, max_rms, eps, stages, _p(f), _p(out), _p(stats), B, T, _stream())
        if need:
            ctx.save_for_backward(f, stats, taps)
        ctx.cfg = (thr, max_rms, stages)
        return out

    @staticmethod
    def backward(ctx, g):
        f, stats, taps = ctx.saved_tensors
        thr, max_rms, stages = ctx.cfg
        g = g.contiguous()
        B, _, T = f.shape
        d = torch.empty_like(f)
        lib.wm_postproc_bwd(_p(g), _p(f), _p(stats), _p(taps), taps.numel(), thr, max_rms, stages, _p(d), B, T, _stream())
        return d, None, None, None, None, None


# ------------------------------------------------------------------------------------------ losses
class _SpectralLossFn(torch.autograd.Function):
    """Shared shape of the three STFT losses: the kernel returns the loss AND d loss / d signal, the tape
    only scales the cached gradient by the incoming scalar."""

    @staticmethod
    def forward(ctx, kind, clean, sig, tables):
        sig2 = _chk(sig, "signal", 3)
        B, _, T = sig2.shape
        dev, st = sig2.device, _stream()
        need = ctx.needs_input_grad[2]
        n_fft, hop = {"mel": (1024, 256), "loud": (2048, 512), "hf": (512, 128)}[kind]
        F = 1 + T // hop
        loss = _f32(1, device=dev)
        part = _f32(B * F, device=dev)
        gfr = _f32(B * F * n_fft, device=dev) if need else None
        dsig = torch.empty_like(sig2) if need else None
        if kind == "mel":
            c2 = _chk(clean, "clean", 3)
            fb, klo, khi, mlo = tables
            lib.wm_mel_loss(_p(c2), _p(sig2), _p(fb), _p(klo), _p(khi), _p(mlo), _p(gfr), _p(part), _p(loss), _p(dsig), B, T, st)
        elif kind == "loud":
            c2 = _chk(clean, "clean", 3)
            lib.wm_loud_loss(_p(c2), _p(sig2), 0.01, _p(gfr), _p(part), _p(loss), _p(dsig), B, T, st)
        else:
            lib.wm_hf_penalty(_p(sig2), int(tables), _p(gfr), _p(part), _p(loss), _p(dsig), B, T, st)
        if need:
            ctx.save_for_backward(dsig)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dsig,) = ctx.saved_tensors
        return None, None, dsig * g, None


class BCEFn(torch.autograd.Function):
    """loc_loss and bce of py/main16.py:252-264 from one pass over the (2B,T,1+bits) logits."""

    @staticmethod
    def forward(ctx, logits, message):
        logits = _chk(logits, "logits", 3)
        message = _chk(message, "message", 1, torch.int64)
        R, T, NO = logits.shape
        B = message.shape[0]
        if R != 2 * B:
            raise ValueError(f"logits must hold [watermarked; clean] = 2*B clips, got {R} for B={B}")
        dev = logits.device
        part = _f32(2 * R * ((T * NO + 4095) // 4096), device=dev)
        out = torch.zeros(2, dtype=torch.float32, device=dev)
        lib.wm_bce_fwd(_p(logits), _p(message), _p(part), _p(out[0]), _p(out[1]), B, R, T, NO, _stream())
        ctx.save_for_backward(logits, message)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_loc, g_bce):
        logits, message = ctx.saved_tensors
        R, T, NO = logits.shape
        gl = g_loc.contiguous().float().reshape(1) if g_loc is not None else torch.zeros(1, device=logits.device)
        gb = g_bce.contiguous().float().reshape(1) if g_bce is not None else torch.zeros(1, device=logits.device)
        d = torch.empty_like(logits)
        lib.wm_bce_bwd(_p(logits), _p(message), _p(gl), _p(gb), _p(d), message.shape[0], R, T, NO, _stream())
        return d, None


class L1Fn(torch.autograd.Function):
    """F.l1_loss(delta, 0), py/main16.py:266."""

    @staticmethod
    def forward(ctx, x):
        x = _chk(x, "delta")
        out = _f32(1, device=x.device)
        part = _f32(256, device=x.device)
        lib.wm_l1_fwd(_p(x), _p(part), _p(out), x.numel(), _stream())
        ctx.save_for_backward(x)
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        dx = torch.empty_like(x)
        lib.wm_l1_bwd(_p(x), _p(g.contiguous().float().reshape(1)), _p(dx), x.numel(), _stream())
        return dx


from .dsp import (  # noqa: E402,F401  the waveform ops live in dsp.py; ops.<name> stays their public spelling
    RESAMPLE_LOWPASS_WIDTH, RESAMPLE_ROLLOFF, _RESAMPLE_HOST, _rate, resample_length, resample_table, resample_tile_periods,
    resample, resample_add, resample_adjoint_table, _resample_rows_launch, _rows_length, resample_rows, ResampleRowsFn,
    BIQUAD_MODES, BIQUAD_IDENTITY, _BIQUAD_COEFFS, _BIQUAD_PLAN, biquad_lowpass_coeffs, _biquad_coeffs, biquad_warm, biquad_plan, biquad,
    PcmCodecFn,
    DistortFn,
    MDCT_HOPS, MDCT_BANDS, MDCT_GRAD_MODES, mdct_default_floor_step, mdct_frames, mdct_plan, mdct_kcut, mdct_codec, MdctCodecFn,
    FIR_MAX_TAPS, _fir_taps, fir_rows, FirRowsFn, rir_synth,
    TIME_WARP_MAX_TABLE, _time_warp_dims, _TIME_WARP_HOST, time_warp_table, _time_warp_table_on, time_warp, TimeWarpFn,
    WSOLA_MAX_N, _wsola_dims, _WSOLA_HOST, wsola_window, _wsola_window_on, wsola_frames, wsola, WsolaFn,
    LPC_FRAMES, LPC_MAX_ORDER, LPC_GRAD_MODES, LPC_FLOOR_STEP, _LPC_HOST, _lpc_dims, lpc_tables, _lpc_tables_on, lpc_frames,
    lpc_codec, LpcCodecFn,
    stoi_plan, _stoi_rows, stoi,
    SPLICE_MAX_SPANS, SPLICE_MAX_N, label_words, _lab, SpliceFn, splice, MaskedBCEFn, loc_threshold_logit, loc_counts,
    CLIP_SCORES_MAX_T, ClipScores, clip_scores_plan, clip_scores, ClipFeaturesPlan, clip_features_plan, clip_features,
)
