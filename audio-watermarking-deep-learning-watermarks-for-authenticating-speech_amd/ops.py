"""torch.autograd.Function wrappers over the C ABI (include/wm_hip.h).

PyTorch is used here for device memory, streams and the autograd tape only; every
arithmetic step of the hot path is a launch into libwm_hip.so.  Each Function mirrors one
block of the reference graph (py/main16.py:112-186, :53-81, :192-217).
"""
from __future__ import annotations

import collections
import contextlib
import math
import os

import torch

from ._lib import lib

NCU = 256            # workgroups the persistent kernels are sized for (MI355X CU count)
BN_EPS = 1e-5        # nn.BatchNorm1d defaults (py/main16.py:117,120)
BN_MOMENTUM = 0.1


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _chk(t: torch.Tensor, name: str, ndim: int | None = None, dtype=torch.float32) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: the watermark hot path runs on the GPU only (got a {t.device} tensor); "
                           "there is no CPU fallback")
    if t.dtype != dtype:
        raise ValueError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"{name}: expected {ndim} dims, got shape {tuple(t.shape)}")
    return t.contiguous()


def _chk_int(v, name, lo=None, hi=None, what=None):
    """v where it is an int (bools refused), in [lo, hi] where a range is given; `what` replaces "an int in [lo, hi]" in the message"""
    if isinstance(v, bool) or not isinstance(v, int) or not (lo is None or lo <= v <= hi):
        raise ValueError(f"{name}: expected {what or f'an int in [{lo}, {hi}]'}, got {v!r}")
    return v


def _chk_positive(v, name):
    """v where it is a positive finite number (bools refused)"""
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v <= 0:
        raise ValueError(f"{name} must be a positive finite number, got {v!r}")
    return v


def _seed64(seed):
    """the seed's low 64 bits as the signed value the launchers take (they split it into the key's two halves)"""
    seed = int(seed) & (2 ** 64 - 1)
    return seed - 2 ** 64 if seed >= 2 ** 63 else seed


def _frames(x: torch.Tensor, name: str, ch: int) -> torch.Tensor:
    x = _chk(x, name, 3)
    if x.shape[1] != ch:
        raise ValueError(f"{name}: expected {ch} channels, got shape {tuple(x.shape)}")
    if x.shape[2] % 4 != 0:
        raise ValueError(f"{name}: clip length must be a multiple of 4 samples, got {x.shape[2]}")
    return x


def _f32(*shape, device):
    return torch.empty(shape, dtype=torch.float32, device=device)


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


# ------------------------------------------------------------------------------------------ ResBlock
def _resblock_fwd(x, params, training, want_grad, tail=True, pending=None):
    """relu(x + BN2(conv2(relu(BN1(conv1(x)))))) for params = (w1, b1, g1, be1, w2, b2, g2, be2, rm1, rv1, nbt1, rm2, rv2, nbt2).
    Returns (out, saved): saved = (x, y1, y2, mask, cst, w1, w2, g1, g2) for a backward, None from the inference launches.  No ctx.
    tail=False (training mode only): stop in front of the tail -- (None, saved) with mask = None; the kernel that follows forms
    out = relu(x + y2 * cst[4] + cst[5]) and the mask (ResBlockHead1Fn, DetectorTailFn, or the next block through `pending`).
    pending (training mode, tail_in_consumer_applies): the `saved` of the block in front, run with tail=False; x is ignored.  This
    block's conv1 launch (wm_conv64_bf_tail) forms that block's tail on load and writes it -- this block's x -- and its mask; the
    return value is then (out, saved, that mask)."""
    w1, b1, g1, be1, w2, b2, g2, be2, rm1, rv1, nbt1, rm2, rv2, nbt2 = params
    if pending is not None:
        px, py2, pcst = pending[0], pending[2], pending[4]
        x, pmask = torch.empty_like(px), _tail_mask(px, want_grad)
    x = _frames(x, "ResBlock input", 64)
    B, _, T = x.shape
    dev, st = x.device, _stream()
    out = torch.empty_like(x) if tail else None
    cst = _f32(8, 64, device=dev)       # sc1 sh1 mean1 is1 sc2 sh2 mean2 is2
    sc1, sh1, mu1, is1, sc2, sh2, mu2, is2 = cst.unbind(0)
    if training:
        y1, y2 = torch.empty_like(x), torch.empty_like(x)
        stats = _f32(NCU * 128, device=dev)
        if pending is not None:
            lib.wm_conv64_bf_tail(_p(px), _p(py2), _p(pack_w64_h(w1, 0)), _p(pcst[4]), _p(pcst[5]), _p(b1), _p(x), _p(pmask), _p(y1),
                                  _p(stats), B, T, st)
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
        return (None, (x, y1, y2, None, cst, w1, w2, g1, g2)) + more
    if want_grad:
        # the backward needs only the SIGN of `out`: one bit per element, written beside it (a frame pass less in backward)
        mask = torch.empty(B * 64 * ((T + 31) // 32), dtype=torch.int32, device=dev)
        lib.wm_bn_add_relu_mask(_p(x), _p(y2), _p(sc2), _p(sh2), _p(out), _p(mask), B, T, st)
    else:
        mask = None
        lib.wm_bn_add_relu(_p(x), _p(y2), _p(sc2), _p(sh2), _p(out), B, T, st)
    return (out, (x, y1, y2, mask, cst, w1, w2, g1, g2)) + more


class ResBlockFn(GradAwareFunction):
    """relu(x + BN2(conv2(relu(BN1(conv1(x))))))  -- ResBlock.forward, py/main16.py:124-125."""

    @staticmethod
    def forward(ctx, x, *args):
        params, training = args[:14], args[14]
        out, saved = _resblock_fwd(x, params, training, wants_grad(ctx))
        if saved is not None:
            ctx.training = bool(training)
            ctx.gdst = _gdst(params[0], params[1], params[4], params[5])      # w1, b1, w2, b2
            ctx.save_for_backward(*saved)
        return out

    @staticmethod
    def backward(ctx, g_out):
        return _resblock_bwd(ctx.saved_tensors, ctx.training, ctx.gdst, g_out) + (None,) * 7


def _resblock_bwd(saved, training, gdst, g_out):
    """Backward of one ResBlock: (dx, dw1, db1, dg1, dbe1, dw2, db2, dg2, dbe2).  The fused path where it applies, else one launch per
    product; gdst = the four weight-gradient destinations of _gdst (all None: fresh tensors, launched in line)."""
    x, y1, y2, mask, cst, w1, w2, g1, g2 = saved
    sc1, sh1, mu1, is1, sc2, sh2, mu2, is2 = cst.unbind(0)
    g_out = g_out.contiguous()
    B, _, T = x.shape
    dev, st = x.device, _stream()
    ev = 0 if training else 1
    n = float(B * T)
    if _CONV["bf16x6"] and _CONV["fused_bwd"] and T % 64 == 0 and not all(g is not None for g in gdst):
        dx, grads, _ = _resblock_bwd_fused(saved, training, g_out)
        return (dx,) + grads
    (dw1, db1, dw2, db2), acc, launch = _wgrad_dst(gdst, dev, w1.shape, (64,), w2.shape, (64,))
    part = _f32(max(B, 1) * 128, device=dev)
    dz2 = torch.empty_like(x)
    lib.wm_relu_bwd_reduce_mask(_p(g_out), _p(mask), _p(y2), _p(dz2), _p(part), None, B, T, st)
    k2 = _f32(4, 64, device=dev)          # A, B (hi), B (lo), C  -- B is handed over as hi + lo words
    dg2, dbe2 = _f32(64, device=dev), _f32(64, device=dev)
    lib.wm_bn_bwd_finalize(_p(part), B, n, _p(g2), _p(mu2), _p(is2), _p(k2[0]), _p(k2[1]), _p(k2[3]), _p(dg2), _p(dbe2), 0, ev, None, 0, None, st)
    # conv2: data gradient (+ ReLU mask + BN1-backward reductions in the epilogue) and weight gradient
    dz1 = torch.empty_like(x)
    stats = _f32(NCU * 128, device=dev)
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
    k1 = _f32(4, 64, device=dev)
    dg1, dbe1 = _f32(64, device=dev), _f32(64, device=dev)
    lib.wm_bn_bwd_finalize(_p(stats), NCU, n, _p(g1), _p(mu1), _p(is1), _p(k1[0]), _p(k1[1]), _p(k1[3]), _p(dg1), _p(dbe1), 0, ev, None, 0, None, st)
    # conv1: data gradient + residual path, weight gradient
    dx = torch.empty_like(x)
    _conv3(dz1, y1, w1, 1, k1[0], k1[1], k1[3], None, dz2, None, None, dx, None, B, T, 3, 2)
    launch((dz1, y1, k1, x), lambda: wgrad(dz1, y1, k1, x, None, None, 0, dw1, db1))
    g1_, g2_ = ((None, None),) * 2 if acc else ((dw1, db1), (dw2, db2))     # (dw / db stay bound: the queued launches read them later)
    return (dx,) + g1_ + (dg1, dbe1) + g2_ + (dg2, dbe2)


def _resblock_bwd_fused(saved, training, g_out, pre=None, fold=None):
    """Backward of one ResBlock on the fused path (data + weight gradient of each convolution in one launch, T % 64 == 0).
    g_out: gradient w.r.t. the block output.  `pre` = (stats partials [NCU,2,64], max |dz| per workgroup [NCU]) when g_out ALREADY is
    dz2 = g (out > 0) and its two BatchNorm sums exist (made by the next block's folded conv1 launch): no reduction pass, no mask.
    `fold` = (mask, y2) of the block BEFORE this one: the conv1 launch then writes that block's dz2 instead of the plain input
    gradient and returns (its BatchNorm-sum partials, its max |dz| per workgroup) as the third value.
    Returns (dx, (dw1, db1, dg1, dbe1, dw2, db2, dg2, dbe2), fold outputs | None)."""
    x, y1, y2, mask, cst, w1, w2, g1, g2 = saved
    sc1, sh1, mu1, is1, sc2, sh2, mu2, is2 = cst.unbind(0)
    B, _, T = x.shape
    dev, st = x.device, _stream()
    ev = 0 if training else 1
    n = float(B * T)
    h = 1 if _CONV["bwd_f16x3"] else 0        # arithmetic of the two launches; the f16 split needs the gradient's scale (max |dz|)
    pack = pack_w64_h if h else pack_w64_bf
    k2 = _f32(4, 64, device=dev)          # A, B (hi), B (lo), C  -- B is handed over as hi + lo words
    dg2, dbe2 = _f32(64, device=dev), _f32(64, device=dev)
    gs2 = _f32(2, device=dev) if h else None
    if pre is not None:
        ppart, pmax = pre
        gsrc, gm = g_out, None
        lib.wm_bn_bwd_finalize(_p(ppart), NCU, n, _p(g2), _p(mu2), _p(is2), _p(k2[0]), _p(k2[1]), _p(k2[3]), _p(dg2), _p(dbe2), 0, ev,
                               _p(pmax) if h else None, NCU, _p(gs2), st)
    else:
        # dz2 = g_out * (out > 0) is never written (default): the reduction pass only forms the two BatchNorm sums, and the two
        # convolution-backward launches mask g_out with the same bits while they load it (wm_dwgrad64_bf's gmask)
        part = _f32(max(B, 1) * 128, device=dev)
        dzm = _f32(B * 64, device=dev) if h else None
        dz2 = None if _CONV["mask_on_load"] else torch.empty_like(x)
        lib.wm_relu_bwd_reduce_mask(_p(g_out), _p(mask), _p(y2), _p(dz2), _p(part), _p(dzm), B, T, st)
        lib.wm_bn_bwd_finalize(_p(part), B, n, _p(g2), _p(mu2), _p(is2), _p(k2[0]), _p(k2[1]), _p(k2[3]), _p(dg2), _p(dbe2), 0, ev,
                               _p(dzm), B * 64, _p(gs2), st)
        gsrc, gm = (g_out, mask) if dz2 is None else (dz2, None)
    # conv2: data gradient (+ ReLU mask + BN1-backward reductions in the epilogue) and weight gradient
    dz1 = torch.empty_like(x)
    stats = _f32(NCU * 128, device=dev)
    dzm1 = _f32(NCU, device=dev) if h else None          # max |dz1| per workgroup, written by the conv2-pair launch
    dw2, db2, dw1, db1 = torch.empty_like(w2), _f32(64, device=dev), torch.empty_like(w1), _f32(64, device=dev)
    wpart = _f32(NCU * (3 * 4096 + 64), device=dev)
    lib.wm_dwgrad64_bf(_p(gsrc), _p(y2), _p(k2[0]), _p(k2[1]), _p(k2[3]), _p(pack(w2, 1)), _p(y1), _p(sc1), _p(sh1),
                       _p(y1), _p(sc1), _p(sh1), _p(dz1), _p(stats), _p(wpart), _p(dw2), _p(db2), B, T, 1, 1, 0, _p(gm), h, _p(gs2), _p(dzm1), st)
    k1 = _f32(4, 64, device=dev)
    dg1, dbe1 = _f32(64, device=dev), _f32(64, device=dev)
    gs1 = _f32(2, device=dev) if h else None
    lib.wm_bn_bwd_finalize(_p(stats), NCU, n, _p(g1), _p(mu1), _p(is1), _p(k1[0]), _p(k1[1]), _p(k1[3]), _p(dg1), _p(dbe1), 0, ev,
                           _p(dzm1), NCU, _p(gs1), st)
    dx = torch.empty_like(x)
    fout = None
    if fold is not None and gm is not None:
        # conv1 pair that also does the PREVIOUS block's ReLU backward and BatchNorm sums (epi 8): dx leaves as that block's dz2
        pmask, py2 = fold
        fpart = _f32(NCU * 128, device=dev)
        fmax = _f32(NCU, device=dev) if h else None
        lib.wm_dwgrad64_bf(_p(dz1), _p(y1), _p(k1[0]), _p(k1[1]), _p(k1[3]), _p(pack(w1, 1)), _p(x), None, None,
                           _p(gsrc), _p(py2), _p(pmask), _p(dx), _p(fpart), _p(wpart), _p(dw1), _p(db1), B, T, 0, 8, 0, _p(gm), h, _p(gs1), _p(fmax), st)
        fout = (fpart, fmax)
    else:
        xmax = _f32(NCU, device=dev) if h else None          # max |dx| per workgroup: a consumer that splits dx into f16 pieces
        lib.wm_dwgrad64_bf(_p(dz1), _p(y1), _p(k1[0]), _p(k1[1]), _p(k1[3]), _p(pack(w1, 1)), _p(x), None, None,
                           _p(gsrc), None, None, _p(dx), None, _p(wpart), _p(dw1), _p(db1), B, T, 0, 2, 0, _p(gm), h, _p(gs1), _p(xmax), st)
        if h:
            _note_gmax(dx, xmax)                             # (ConvT7Fn.backward) then needs no pass over it for its scale
    return dx, (dw1, db1, dg1, dbe1, dw2, db2, dg2, dbe2), fout


def pair_node_applies(x) -> bool:
    """ResBlockPairFn's precondition on input and switches (the caller adds: both blocks in training mode, no forward hooks)"""
    return (torch.is_grad_enabled() and x.is_cuda and x.dim() == 3 and x.shape[-1] % 64 == 0 and _CONV["bf16x6"]
            and _CONV["fused_bwd"] and _CONV["mask_on_load"] and _CONV["pair_fold"] and not _ASYNC["on"])


def _pair_fwd(x, p1, p2, training, want_grad, tail=True):
    """Two ResBlocks in a row, the second one up to `tail` (as _resblock_fwd's): (out | None, first, second), the two blocks' `saved`.
    Where the tail-in-consumer launches apply, the first block's tail is formed by the second block's conv1 launch; same tensors
    either way."""
    if training and _tail_in_consumer_launches(x):
        _, first = _resblock_fwd(x, p1, True, want_grad, tail=False)
        out, second, pmask = _resblock_fwd(None, p2, True, want_grad, tail=tail, pending=first)
        return out, first[:3] + (pmask,) + first[4:], second
    mid, first = _resblock_fwd(x, p1, training, want_grad)
    out, second = _resblock_fwd(mid, p2, training, want_grad, tail=tail)
    return out, first, second


class ResBlockPairFn(GradAwareFunction):
    """Two ResBlocks in a row (py/main16.py:135-136 encoder.1 -> encoder.2, :178-179 model.1 -> model.2) as one tape node.
    Forward = _resblock_fwd twice.  Backward: the second block's conv1 launch (data + weight gradient) applies the
    FIRST block's ReLU mask to the gradient it has just formed and accumulates that block's two BatchNorm sums in its epilogue
    (wm_dwgrad64_bf epi 8), so the first block needs no reduction pass and the gradient between the blocks is written once, masked.
    Used by modules.resblock_pair when the fused path applies (bf16x6, T % 64 == 0, mask-on-load, gradients wanted)."""

    @staticmethod
    def forward(ctx, x, *args):
        p1, p2, training = args[:14], args[14:28], args[28]
        out, first, second = _pair_fwd(x, p1, p2, training, wants_grad(ctx))
        ctx.save_for_backward(*(first + second))
        ctx.training = bool(training)
        return out

    @staticmethod
    def backward(ctx, g_out):
        sv = ctx.saved_tensors
        s1_, s2_ = sv[:9], sv[9:]
        g_out = g_out.contiguous()
        dmid, grads2, fout = _resblock_bwd_fused(s2_, ctx.training, g_out, fold=(s1_[3], s1_[2]))
        dx, grads1, _ = _resblock_bwd_fused(s1_, ctx.training, dmid, pre=fout)
        return (dx,) + grads1 + (None,) * 6 + grads2 + (None,) * 6 + (None,)


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
        ctx.grad_rows = B if grad_rows is None else max(0, min(int(grad_rows), B))
        return y

    @staticmethod
    def backward(ctx, g):
        s, w = ctx.saved_tensors
        g = g.contiguous()
        B, _, T = s.shape
        ds = None
        if ctx.needs_input_grad[0]:        # rows >= grad_rows are known not to need a gradient (the clean half): left zero
            ds = torch.empty_like(s) if ctx.grad_rows == B else torch.zeros_like(s)
        part = _f32(2 * NCU * 512, device=s.device)
        dw, db = torch.empty_like(w), _f32(64, device=s.device)
        lib.wm_stem_bwd(_p(g), _p(s), _p(w), _p(ds), _p(part), _p(dw), _p(db), B, T, ctx.grad_rows, 0, _stream())
        return ds, dw, db, None


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
        params, hw, hb = args[:14], args[14], args[15]
        want = wants_grad(ctx)
        _, saved = _resblock_fwd(x, params, True, want, tail=False)
        x, _, y2, _, cst = saved[:5]
        B, _, T = x.shape
        out, mask = torch.empty_like(x), _tail_mask(x, want)
        y = _f32(B, 1, T, device=x.device)
        lib.wm_head1_tail_fwd(_p(x), _p(y2), _p(cst[4]), _p(cst[5]), _p(hw), _p(hb), _p(out), _p(mask), _p(y), B, T, _stream())
        if want:
            ctx.save_for_backward(*(saved[:3] + (mask,) + saved[4:] + (out, hw)))
        return y

    @staticmethod
    def backward(ctx, g):
        sv = ctx.saved_tensors
        out, hw = sv[9], sv[10]
        B, _, T = out.shape
        dout = torch.empty_like(out)
        part = _f32(1024 * 65, device=out.device)
        dhw, dhb = torch.empty_like(hw), _f32(1, device=out.device)
        lib.wm_head1_bwd(_p(g.contiguous()), _p(out), _p(hw), _p(dout), _p(part), _p(dhw), _p(dhb), B, T, 0, _stream())
        return _resblock_bwd(sv[:9], True, (None,) * 4, dout) + (None,) * 6 + (dhw, dhb)


class DetectorTailFn(GradAwareFunction):
    """model.1 -> model.2 -> model.3 (py/main16.py:178-180) with both BCE terms (:252-264) as one tape node, for the train step on
    the fused path (pair_node_applies).  Forward: ResBlockPairFn's, except that model.2's tail, the head and the two loss sums are one
    launch (wm_headN_tail_fwd) -> (logits, loc, bce).  Backward: the head's backward forms the losses' gradient from the logits while
    it loads them (wm_headN_bwd_bce), then ResBlockPairFn's backward.  A gradient arriving on `logits` takes the unfused route:
    wm_bce_bwd's tensor plus that gradient through wm_headN_bwd."""

    @staticmethod
    def forward(ctx, x, message, *args):
        p1, p2, hw, hb = args[:14], args[14:28], args[28], args[29]
        want = wants_grad(ctx)
        _, first, second = _pair_fwd(x, p1, p2, True, want, tail=False)
        mid, y2, cst = second[0], second[2], second[4]
        R, _, T = mid.shape
        NO, B, dev = hw.shape[0], message.shape[0], mid.device
        out, mask = torch.empty_like(mid), _tail_mask(mid, want)
        logits = _f32(R, T, NO, device=dev)
        part = _f32(2 * R * ((T + 255) // 256), device=dev)
        losses = torch.zeros(2, dtype=torch.float32, device=dev)
        lib.wm_headN_tail_fwd(_p(mid), _p(y2), _p(cst[4]), _p(cst[5]), _p(hw), _p(hb), _p(message), B, _p(part), _p(losses[0]), _p(losses[1]),
                              _p(out), _p(mask), _p(logits), R, T, NO, _stream())
        ctx.set_materialize_grads(False)
        if want:
            ctx.save_for_backward(*(first + second[:3] + (mask,) + second[4:] + (out, hw, logits, message)))
        return logits, losses[0], losses[1]

    @staticmethod
    def backward(ctx, g_logits, g_loc, g_bce):
        sv = ctx.saved_tensors
        s1_, s2_, (out, hw, logits, message) = sv[:9], sv[9:18], sv[18:]
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
        dmid, grads2, fout = _resblock_bwd_fused(s2_, True, dout, fold=(s1_[3], s1_[2]))
        dx, grads1, _ = _resblock_bwd_fused(s1_, True, dmid, pre=fout)
        return (dx, None) + grads1 + (None,) * 6 + grads2 + (None,) * 6 + (dhw, dhb)


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
    """LSTMFn's forward: (h, saved) with saved = (x, h, gates, cst, w_ih, w_hh) for _lstm_bwd, None unless need_grad.  No ctx.
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
    return h, ((x, h, gates, cst, w_ih, w_hh) if need_grad else None)


def _lstm_bwd(saved, gdst, dh, dx_inside=False):
    """LSTMFn's backward on _lstm_fwd's saved tensors: (dx, dw_ih, dw_hh, db_ih, db_hh); gdst = the four destinations of _gdst.
    dx_inside (EncoderLSTMFn, set_lstm_dx_in_bwd): dx comes out of the wave-specialised BPTT launch itself, unless the side-stream
    option is on.  (The library's own fp32 choice, wm_set_lstm_dx_bf16x6(0), is not visible here: the entry point honours it.)"""
    x, h, gates, cst, w_ih, w_hh = saved
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
        p1, p2, (w_ih, w_hh, b_ih, b_hh) = args[:14], args[14:28], args[28:32]
        want = wants_grad(ctx)
        _, first, second = _pair_fwd(x, p1, p2, True, want, tail=False)
        mid, y2, cst = second[0], second[2], second[4]
        mask = _tail_mask(mid, want)
        h, lsaved = _lstm_fwd(None, w_ih, w_hh, b_ih, b_hh, want, tail=(mid, y2, cst[4], cst[5], mask))
        if want:
            ctx.gdst = _gdst(w_ih, w_hh, b_ih, b_hh)
            ctx.save_for_backward(*(first + second[:3] + (mask,) + second[4:] + lsaved))
        return h

    @staticmethod
    def backward(ctx, dh):
        sv = ctx.saved_tensors
        _single_backward(ctx, "EncoderLSTMFn")
        s1_, s2_ = sv[:9], sv[9:18]
        lgrads = _lstm_bwd(sv[18:], ctx.gdst, dh, dx_inside=_LSTM_DX["in_bwd"])
        dmid, grads2, fout = _resblock_bwd_fused(s2_, True, lgrads[0], fold=(s1_[3], s1_[2]))
        dx, grads1, _ = _resblock_bwd_fused(s1_, True, dmid, pre=fout)
        return (dx,) + grads1 + (None,) * 6 + grads2 + (None,) * 6 + lgrads[1:]


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


# ---------------------------------------------------------------------------------------------- sample-rate conversion
# torchaudio.functional.resample with its documented defaults (resampling_method="sinc_interp_hann", lowpass_filter_width=6,
# rolloff=0.99), restated from the published description.  The reference resamples every file that is not at 16 kHz before a
# model sees it (py/main16.py:717-720).  The table is formed in float64 and rounded once to float32; the clamp of the filter
# argument makes every tap beyond +-6 zero crossings exactly 0.0, so only each phase's run of non-zero taps goes to the device.
RESAMPLE_LOWPASS_WIDTH = 6
RESAMPLE_ROLLOFF = 0.99
_RESAMPLE_HOST = {}      # (orig, new) -> table dict (CPU tensors)
_RESAMPLE_DEV = {}       # (orig, new, device) -> (taps, first) on the device


def _rate(v, name):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or v != int(v) or int(v) <= 0:
        raise ValueError(f"{name} must be a positive integer number of Hz, got {v!r}")
    return int(v)


def resample_length(n, orig_freq, new_freq):
    """ceil(new * n / orig): the number of samples torchaudio keeps for an input of n"""
    g = math.gcd(int(orig_freq), int(new_freq))
    P, Q = int(orig_freq) // g, int(new_freq) // g
    return -((-Q * int(n)) // P)


def resample_table(orig_freq, new_freq):
    """Host tables of one rate pair (cached): P, Q, width, K = 2*width + P, the dense float32 table `dense` (Q, K), and the compact
    one the kernel reads: `taps` (Q, W) with `first` (Q,) int32 such that dense[i, first[i]:first[i]+W] == taps[i] and every other
    entry of dense is 0.0.  W is the longest run of non-zero taps over the phases, made odd where K allows (LDS banks)."""
    orig_freq, new_freq = _rate(orig_freq, "orig_freq"), _rate(new_freq, "new_freq")
    key = (orig_freq, new_freq)
    if key in _RESAMPLE_HOST:
        return _RESAMPLE_HOST[key]
    g = math.gcd(orig_freq, new_freq)
    P, Q = orig_freq // g, new_freq // g
    if P == Q:       # equal rates: the identity as a one-tap table (only the segment padding of the kernel is used)
        tab = {"P": 1, "Q": 1, "width": 0, "K": 1, "W": 1, "dense": torch.ones(1, 1), "taps": torch.ones(1, 1),
               "first": torch.zeros(1, dtype=torch.int32)}
        _RESAMPLE_HOST[key] = tab
        return tab
    lpw = RESAMPLE_LOWPASS_WIDTH
    base = min(P, Q) * RESAMPLE_ROLLOFF
    width = int(math.ceil(lpw * P / base))
    K = 2 * width + P
    j = torch.arange(-width, width + P, dtype=torch.float64)[None, :] / P
    i = torch.arange(0, -Q, -1, dtype=torch.float64)[:, None] / Q
    t = ((i + j) * base).clamp_(-lpw, lpw)
    window = torch.cos(t * math.pi / lpw / 2) ** 2
    t = t * math.pi
    sinc = torch.where(t == 0, torch.ones_like(t), torch.sin(t) / t)
    dense = (sinc * (window * (base / P))).to(torch.float32)                   # (Q, K), the one rounding
    nz = dense != 0
    assert bool(nz.any(dim=1).all())
    idx = torch.arange(K)
    lo = torch.where(nz, idx, K).min(dim=1).values
    hi = torch.where(nz, idx, -1).max(dim=1).values
    W = int((hi - lo + 1).max())
    if W % 2 == 0 and W < K:
        W += 1
    first = torch.minimum(lo, torch.tensor(K - W)).to(torch.int32)
    taps = torch.stack([dense[q, int(first[q]):int(first[q]) + W] for q in range(Q)]).contiguous()
    tab = {"P": P, "Q": Q, "width": width, "K": K, "W": W, "dense": dense, "taps": taps, "first": first}
    _RESAMPLE_HOST[key] = tab
    return tab


def resample_tile_periods(orig_freq, new_freq):
    """output periods (Q samples each) one workgroup of the LDS kernel handles at a time; 0: the table does not fit LDS and the
    one-thread-per-sample kernel runs"""
    import ctypes
    tab = resample_table(orig_freq, new_freq)
    out = (ctypes.c_longlong * 1)()
    lib.wm_resample_plan(tab["P"], tab["Q"], tab["width"], tab["W"], ctypes.addressof(out), None)
    return int(out[0])


def resample(x, orig_freq, new_freq, seg_len=0, out=None):
    """Channel mean + sinc resampling of a CUDA waveform (C, N) or (N,) in one launch.  seg_len = 0: (1, L) with
    L = ceil(new * N / orig).  seg_len > 0: (S, 1, seg_len), S = ceil(L / seg_len), the tail of the last segment zero -- the
    Generator / Detector batch of the recording.  Equal rates with seg_len = 0 return x unchanged.  `out` (optional): a
    contiguous fp32 CUDA buffer of exactly the result's size to write into."""
    tab = resample_table(orig_freq, new_freq)
    seg_len = int(seg_len)
    if seg_len < 0:
        raise ValueError(f"seg_len must be >= 0, got {seg_len}")
    if isinstance(x, torch.Tensor) and x.dim() == 1:
        x = x.unsqueeze(0)
    x = _chk(x, "waveform", 2)
    if tab["K"] == 1 and seg_len == 0 and out is None:
        return x
    C, N = x.shape
    if C < 1:
        raise ValueError("waveform: needs at least one channel")
    L = -((-tab["Q"] * N) // tab["P"])
    S = -(-L // seg_len) if seg_len else 1
    total = S * seg_len if seg_len else L
    dkey = (int(orig_freq), int(new_freq), x.device)
    if dkey not in _RESAMPLE_DEV:
        _RESAMPLE_DEV[dkey] = (tab["taps"].to(x.device), tab["first"].to(x.device))
    taps, first = _RESAMPLE_DEV[dkey]
    if out is None:
        out = _f32(total, device=x.device)
    else:
        if not out.is_contiguous() or _chk(out, "out").numel() != total or out.device != x.device:
            raise ValueError(f"out: expected {total} floats on {x.device}, got {out.numel()} on {out.device}")
    lib.wm_resample(_p(x), _p(taps), _p(first), _p(out), C, N, tab["P"], tab["Q"], tab["width"], tab["W"], L, total, _stream())
    return out.view(S, 1, seg_len) if seg_len else out.view(1, L)


def resample_add(x, delta, orig_freq, delta_freq=16000, out=None, want_up=True):
    """The way back of the embed path in one launch: `delta` (at delta_freq) resampled to the recording's rate `orig_freq` and added to
    every channel of the recording `x` ((C, N) or (N,), fp32, CUDA).  `delta`: any contiguous fp32 CUDA tensor, read flat; its first
    n_d = resample_length(N, orig_freq, delta_freq) samples count, the rest is never read.  Returns (out (C, N), up (1, N) or None):
    up is ops.resample(delta[:n_d], delta_freq, orig_freq)[:, :N] bit for bit, out[c] = x[c] + up[0].  `out` (optional): a contiguous
    (C, N) fp32 buffer to write into; it may be x itself.  want_up=False: up is neither formed in memory nor returned."""
    tab = resample_table(delta_freq, orig_freq)
    inplace = out is x
    if isinstance(x, torch.Tensor) and x.dim() == 1:
        x = x.unsqueeze(0)                      # a view: an in-place sum still lands in the caller's (N,) tensor
    if isinstance(x, torch.Tensor) and x.dim() != 2:
        raise ValueError(f"waveform: expected (channels, samples) or (samples,), got shape {tuple(x.shape)}")
    if inplace and not x.is_contiguous():
        raise ValueError("out: an in-place sum needs a contiguous waveform")
    x = _chk(x, "waveform", 2)
    delta = _chk(delta, "delta")
    C, N = x.shape
    if C < 1:
        raise ValueError("waveform: needs at least one channel")
    n_d = resample_length(N, orig_freq, delta_freq)
    if delta.numel() < n_d:
        raise ValueError(f"delta: {N} samples at {orig_freq} Hz need {n_d} at {delta_freq} Hz, got {delta.numel()}")
    if delta.device != x.device:
        raise ValueError(f"delta: on {delta.device}, the waveform is on {x.device}")
    if out is None:
        out = _f32(C, N, device=x.device)
    elif inplace:
        out = x                                 # the (C, N) view of the caller's tensor
    elif (not out.is_contiguous() or tuple(_chk(out, "out").shape) != (C, N) or out.device != x.device):
        raise ValueError(f"out: expected a contiguous ({C}, {N}) buffer on {x.device}, got {tuple(out.shape)} on {out.device}")
    up = _f32(1, N, device=x.device) if want_up else None
    dkey = (int(delta_freq), int(orig_freq), x.device)
    if dkey not in _RESAMPLE_DEV:
        _RESAMPLE_DEV[dkey] = (tab["taps"].to(x.device), tab["first"].to(x.device))
    taps, first = _RESAMPLE_DEV[dkey]
    lib.wm_resample_add(_p(delta), _p(taps), _p(first), _p(x), _p(out), _p(up), C, N, n_d, tab["P"], tab["Q"], tab["width"], tab["W"],
                        _stream())
    return out, up


def resample_adjoint_table(orig_freq, new_freq):
    """Host table (cached) with which wm_resample_rows is the ADJOINT of the orig -> new resampler.  Write A for the (L, N) matrix of one
    row, A[m*Q + i][m*P + j - width] = dense[i][j].  Shifting the input index by P shifts the output index by Q with the same coefficients,
    so dx[n] = sum_o A[o][n] * dy[o] is itself a polyphase filter: P phases (n = m*P + p), stride Q through dy,
        dx[m*P + p] = sum_s c[p][s] * dy[m*Q + s],   c[p][s] = dense[s mod Q][-(s div Q)*P + p + width]   (0 outside dense),
    the float32 values of `dense` rearranged, nothing rounded again.  Returned in resample_table's layout with P' = Q, Q' = P:
    taps' (P, W') and first' (P,) int32 with taps'[p][k] = c[p][first'[p] + k - width'], every c outside that run exactly 0.0.
    width' is the smallest that keeps every run inside the K' = 2*width' + P' taps of a phase, so the kernels' clamp of first' to
    [0, 2*width' + P' - W'] moves no phase (asserted); W' is made odd where K' allows, as resample_table does."""
    orig_freq, new_freq = _rate(orig_freq, "orig_freq"), _rate(new_freq, "new_freq")
    key = (orig_freq, new_freq, "adjoint")
    if key in _RESAMPLE_HOST:
        return _RESAMPLE_HOST[key]
    tab = resample_table(orig_freq, new_freq)
    if tab["K"] == 1:                # equal rates: the identity is its own adjoint
        _RESAMPLE_HOST[key] = tab
        return tab
    P, Q, width, K, dense = tab["P"], tab["Q"], tab["width"], tab["K"], tab["dense"]
    # column j of dense belongs to the adjoint phase p = (j - width) mod P at the period offset d = (j - width - p) / P; its row i is s = i - d*Q
    nz = dense != 0
    rows = torch.arange(Q)[:, None]
    j = torch.arange(K)
    p_of = (j - width) % P
    d_of = (j - width - p_of) // P
    far = 1 << 40                                                             # beyond every s: a column without a non-zero tap never wins
    col_lo = torch.where(nz, rows, far).min(dim=0).values - d_of * Q          # (K,): lowest / highest s with a non-zero tap, per column
    col_hi = torch.where(nz, rows, -far).max(dim=0).values - d_of * Q
    lo = torch.full((P,), far, dtype=torch.int64).scatter_reduce(0, p_of, col_lo, "amin")
    hi = torch.full((P,), -far, dtype=torch.int64).scatter_reduce(0, p_of, col_hi, "amax")
    assert bool((lo <= hi).all()), "an input phase no output reads"
    Pa, Qa = Q, P
    wa = max(int(-lo.min()), int(hi.max()) - Pa + 1, 0)
    Ka = 2 * wa + Pa
    W = int((hi - lo + 1).max())
    if W % 2 == 0 and W < Ka:
        W += 1
    first = torch.minimum(lo + wa, torch.tensor(Ka - W))
    assert W <= Ka and int(first.min()) >= 0 and int(first.max()) <= 2 * wa + Pa - W, "the kernel would clamp a phase of the adjoint table"
    s = first[:, None] + torch.arange(W)[None, :] - wa                        # (P, W)
    i = s % Q
    jj = -((s - i) // Q) * P + torch.arange(P)[:, None] + width
    inside = (jj >= 0) & (jj < K)
    taps = torch.where(inside, dense[i, jj.clamp(0, K - 1)], torch.zeros(())).contiguous()
    assert int((taps != 0).sum()) == int(nz.sum()), "the adjoint table lost a tap"
    out = {"P": Pa, "Q": Qa, "width": wa, "K": Ka, "W": W, "taps": taps, "first": first.to(torch.int32)}
    _RESAMPLE_HOST[key] = out
    return out


def _resample_rows_launch(x, tab, dkey, L):
    rows, N = x.shape
    if dkey not in _RESAMPLE_DEV:
        _RESAMPLE_DEV[dkey] = (tab["taps"].to(x.device), tab["first"].to(x.device))
    taps, first = _RESAMPLE_DEV[dkey]
    y = _f32(rows, L, device=x.device)
    lib.wm_resample_rows(_p(x), _p(taps), _p(first), _p(y), rows, N, L, tab["P"], tab["Q"], tab["width"], tab["W"], _stream())
    return y


def _rows_length(N, orig_freq, new_freq, length):
    full = resample_length(N, orig_freq, new_freq)
    if length is None:
        return full
    _chk_int(length, "length", 0, full, f"an int in [0, {full}] (what {N} samples give)")
    return length


def resample_rows(x, orig_freq, new_freq, length=None):
    """Sinc resampling of every row of a CUDA fp32 (rows, N) tensor by itself, one launch of wm_resample_rows: (rows, L) with
    L = resample_length(N, orig, new), or its first `length` samples.  No mixdown: row r is ops.resample(x[r:r+1], orig, new)[0] bit for
    bit.  Equal rates return x (x[:, :length] when cut)."""
    tab = resample_table(orig_freq, new_freq)
    x = _chk(x, "x", 2)
    L = _rows_length(x.shape[1], orig_freq, new_freq, length)
    if tab["K"] == 1:
        return x if L == x.shape[1] else x[:, :L]
    return _resample_rows_launch(x, tab, (int(orig_freq), int(new_freq), x.device), L)


class ResampleRowsFn(torch.autograd.Function):
    """y = A x per row (resample_rows); dx = A^T dy, the same launch with resample_adjoint_table on (dy, rows, L -> N).  Nothing is saved
    but the rates and the lengths."""

    @staticmethod
    def forward(ctx, x, orig_freq, new_freq, length=None):
        ctx.rates, ctx.n = (int(orig_freq), int(new_freq)), x.shape[1]
        return resample_rows(x, orig_freq, new_freq, length)

    @staticmethod
    def backward(ctx, dy):
        orig, new = ctx.rates
        dy = _chk(dy, "dy", 2)
        tab = resample_adjoint_table(orig, new)
        if tab["K"] == 1:
            dx = torch.nn.functional.pad(dy, (0, ctx.n - dy.shape[1]))
        else:
            dx = _resample_rows_launch(dy, tab, (orig, new, dy.device, "adjoint"), ctx.n)
        return dx, None, None, None


# ---------------------------------------------------------------------------------------------- biquad + 16-bit PCM codec
# The reference's 16-bit save path (py/main15.py:850-867: 7 kHz biquad low-pass -> clamp -> x32767 -> int16) and main15c's
# perceptual_postprocess (round(lowpass_biquad(x, 16000, 7000) * 32767) / 32767 on s_w inside the train / validation step) as one
# launch of wm_biquad.  The section is the RBJ cookbook low-pass torchaudio.functional.lowpass_biquad is published as.
BIQUAD_MODES = {"float": 0, "round": 1, "pcm16": 2}
BIQUAD_IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0)       # the quantiser alone
_BIQUAD_COEFFS = {}
_BIQUAD_PLAN = {}


def biquad_lowpass_coeffs(sample_rate, cutoff_freq, Q=0.707):
    """(b0, b1, b2, a1, a2) of the low-pass section exactly as inference.lowpass_biquad forms it: float64, divided by a0, each value
    rounded once to float32 (returned as Python floats that hold those float32 values).  Host-only, cached."""
    key = (sample_rate, cutoff_freq, Q)
    try:
        return _BIQUAD_COEFFS[key]
    except (KeyError, TypeError):
        pass
    for v, name in ((sample_rate, "sample_rate"), (cutoff_freq, "cutoff_freq"), (Q, "Q")):
        _chk_positive(v, name)
    if 2.0 * float(cutoff_freq) >= float(sample_rate):
        raise ValueError(f"cutoff_freq must lie below half the sample rate, got {cutoff_freq} Hz at {sample_rate} Hz")
    import numpy as np
    w0 = 2.0 * math.pi * float(cutoff_freq) / float(sample_rate)
    alpha = math.sin(w0) / (2.0 * float(Q))
    cw = math.cos(w0)
    b = np.array([(1.0 - cw) / 2.0, 1.0 - cw, (1.0 - cw) / 2.0], dtype=np.float64)
    a = np.array([1.0 + alpha, -2.0 * cw, 1.0 - alpha], dtype=np.float64)
    b32, a32 = (b / a[0]).astype(np.float32), (a / a[0]).astype(np.float32)
    out = (float(b32[0]), float(b32[1]), float(b32[2]), float(a32[1]), float(a32[2]))
    _BIQUAD_COEFFS[key] = out
    return out


def _biquad_coeffs(coeffs):
    import numpy as np
    try:
        c = tuple(float(v) for v in coeffs)
    except TypeError:
        raise ValueError(f"coeffs: expected (b0, b1, b2, a1, a2), got {coeffs!r}") from None
    if len(c) != 5 or not all(math.isfinite(v) and float(np.float32(v)) == v for v in c):
        raise ValueError(f"coeffs: expected five finite float32 values (b0, b1, b2, a1, a2), got {coeffs!r}")
    return c


def biquad_warm(coeffs):
    """the smallest W with r^W <= 2^-40, r the pole radius of 1 / (1 + a1 z^-1 + a2 z^-2): the warm-up after which a recursion started
    from a zero state has forgotten that (0 for a section without poles).  An unstable section (r >= 1) raises ValueError."""
    _, _, _, a1, a2 = _biquad_coeffs(coeffs)
    disc = a1 * a1 - 4.0 * a2
    r = math.sqrt(a2) if disc < 0 else (abs(a1) + math.sqrt(disc)) / 2.0
    if r >= 1.0:
        raise ValueError(f"coeffs: the section is not stable (pole radius {r})")
    if r == 0.0:
        return 0
    W = max(0, int(math.ceil(-40.0 * math.log(2.0) / math.log(r))) - 1)
    while r ** W > 2.0 ** -40:
        W += 1
    return W


def biquad_plan(coeffs):
    """(warm, chunk) wm_biquad runs this section with: the time-parallel kernel with chunks of `chunk` samples and biquad_warm(coeffs)
    samples of warm-up, or (-1, 0), one lane per row, where the library finds that warm-up too long.  A function of the coefficients alone."""
    import ctypes
    c = _biquad_coeffs(coeffs)
    if c not in _BIQUAD_PLAN:
        W = biquad_warm(c)
        out = (ctypes.c_int * 1)()
        lib.wm_biquad_plan(W, ctypes.addressof(out), None)
        _BIQUAD_PLAN[c] = (W, int(out[0])) if out[0] else (-1, 0)
    return _BIQUAD_PLAN[c]


def biquad(x, coeffs, *, clamp=True, mode="float", reverse=False, mask_out=False, mask_in=None, out=None):
    """Second-order section along the last axis of a contiguous fp32 CUDA tensor (all leading axes are rows, each from a zero state),
    one launch (wm_biquad).  mode "float": clamp(y, -1, 1) (clamp=False: y) | "round": round(clamp(y) * 32767) / 32767 | "pcm16": int16
    codes (clamp(y) * 32767).to(int16).  reverse: flip(filter(flip(x))), the adjoint.  mask_out: also returns the int32 bit mask of
    |y| <= 1 ((rows, ceil(n / 32)), bit t % 32 of word t / 32) as (out, mask).  mask_in: such a mask, applied to x on load.  `out`: a
    contiguous buffer of x's shape (int16 for "pcm16") that does not overlap x."""
    if mode not in BIQUAD_MODES:
        raise ValueError(f"mode must be one of {sorted(BIQUAD_MODES)}, got {mode!r}")
    if isinstance(x, torch.Tensor) and not x.is_cuda:
        raise ValueError(f"x: ops.biquad runs on the GPU only (got a {x.device} tensor); perceptual_postprocess / encode_pcm16 take CPU tensors")
    c = _biquad_coeffs(coeffs)
    x = _chk(x, "x")
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError(f"x: needs at least one row of at least one sample, got shape {tuple(x.shape)}")
    n = x.shape[-1]
    rows = x.numel() // n
    if mode == "pcm16" and not clamp:
        raise ValueError('mode "pcm16" needs clamp=True (the int16 cast is defined on [-1, 1] only)')
    if mask_out and reverse:
        raise ValueError("mask_out is not available with reverse=True")
    warm, _ = biquad_plan(c)
    odt = torch.int16 if mode == "pcm16" else torch.float32
    if out is None:
        out = torch.empty(x.shape, dtype=odt, device=x.device)
    else:
        if not isinstance(out, torch.Tensor) or not out.is_cuda or out.device != x.device or out.dtype != odt or \
                not out.is_contiguous() or out.shape != x.shape:
            raise ValueError(f"out: expected a contiguous {odt} buffer of shape {tuple(x.shape)} on {x.device}")
        xa, oa = x.data_ptr(), out.data_ptr()
        if xa < oa + out.numel() * out.element_size() and oa < xa + x.numel() * 4:
            raise ValueError("out: overlaps x (the filter reads x behind the samples it writes; in place is not supported)")
    nw = (n + 31) // 32
    if mask_in is not None:
        mask_in = _chk(mask_in, "mask_in", None, torch.int32)
        if mask_in.numel() != rows * nw or mask_in.device != x.device:
            raise ValueError(f"mask_in: expected {rows} x {nw} int32 words on {x.device}, got {mask_in.numel()} on {mask_in.device}")
    mask = torch.empty(rows, nw, dtype=torch.int32, device=x.device) if mask_out else None
    lib.wm_biquad(_p(x), _p(out), _p(mask), _p(mask_in), *c, rows, n, warm, BIQUAD_MODES[mode], int(bool(clamp)), int(bool(reverse)),
                  _stream())
    return (out, mask) if mask_out else out


class PcmCodecFn(torch.autograd.Function):
    """main15c's perceptual_postprocess, round(clamp(biquad(x)) * 32767) / 32767, on the tape.  grad "reference": the output is
    non-differentiable, as in torch (torch.round has a zero gradient, so nothing downstream of the codec reaches the Generator; marking
    it also spares the Detector an input gradient that would be multiplied by zero).  grad "straight_through" (no counterpart in the
    reference): the rounding passes the gradient unchanged, the clamp where its saved bit is set, the filter through its adjoint --
    one reverse launch with mask_in."""

    @staticmethod
    def forward(ctx, x, coeffs, grad):
        if grad not in ("reference", "straight_through"):
            raise ValueError(f'grad must be "reference" or "straight_through", got {grad!r}')
        ctx.coeffs = coeffs
        if grad == "reference" or not ctx.needs_input_grad[0]:
            out = biquad(x, coeffs, mode="round")
            ctx.mark_non_differentiable(out)
            ctx.st = False
            return out
        out, mask = biquad(x, coeffs, mode="round", mask_out=True)
        ctx.save_for_backward(mask)
        ctx.st = True
        return out

    @staticmethod
    def backward(ctx, g):
        if not ctx.st:
            return None, None, None
        (mask,) = ctx.saved_tensors
        return biquad(g.contiguous(), ctx.coeffs, clamp=False, reverse=True, mask_in=mask), None, None


# ---------------------------------------------------------------------------------------------- channel distortions
class DistortFn(torch.autograd.Function):
    """wm_distort on the tape: y = g_r x + s_r z per row of a contiguous fp32 CUDA tensor (all leading axes are rows), with the row's gain,
    SNR and noise coin drawn in the kernel from (seed, draw, row0 + r).  bounds = (gain_lo, gain_hi, snr_lo, snr_hi, p_noise).  Returns
    (y, stat), stat (rows, 4) = {g_r, s_r, ms_r, snr_db_r or inf}, not differentiable.  Saved for the backward: x and stat -- never the
    noise, which wm_distort_bwd regenerates from the same counters.  through: the noise level s_r takes part in the gradient."""

    @staticmethod
    def _scratch(rows, n, device):
        import ctypes
        need = ctypes.c_longlong(0)
        lib.wm_distort_plan(rows, n, ctypes.addressof(need), None)
        return _f32(need.value, device=device)

    @staticmethod
    def forward(ctx, x, bounds, seed, draw, row0, through):
        x = _chk(x, "x")
        if x.dim() < 1 or x.numel() == 0:
            raise ValueError(f"x: needs at least one row of at least one sample, got shape {tuple(x.shape)}")
        n = x.shape[-1]
        rows = x.numel() // n
        ctx.key = (rows, n, int(row0), _seed64(seed), int(draw))
        ctx.through = bool(through)
        y, stat = torch.empty_like(x), _f32(rows, 4, device=x.device)
        lib.wm_distort(_p(x), _p(y), _p(stat), _p(DistortFn._scratch(rows, n, x.device)), *ctx.key, *map(float, bounds), _stream())
        ctx.save_for_backward(x, stat)
        ctx.mark_non_differentiable(stat)
        return y, stat

    @staticmethod
    def backward(ctx, g, _gstat):
        x, stat = ctx.saved_tensors
        g = _chk(g, "grad")
        dx = torch.empty_like(x)
        lib.wm_distort_bwd(_p(g), _p(x), _p(stat), _p(dx), _p(DistortFn._scratch(*ctx.key[:2], x.device)), *ctx.key, int(ctx.through),
                           _stream())
        return dx, None, None, None, None, None


# ---------------------------------------------------------------------------------------------- transform-codec stand-in
# Lapped MDCT -> per-band quantiser -> bandwidth cut -> synthesis (wm_mdct_codec, csrc/mdct_codec.hip): the signal path lossy codecs share,
# as a step of the graph.  A stand-in for compression, not an MP3 / AAC encoder: parity with a real encoder is unmeasured.
MDCT_HOPS = (128, 256, 512)
MDCT_BANDS = (4, 8, 16, 32)
MDCT_GRAD_MODES = ("straight_through", "dead_zone")


def mdct_default_floor_step(hop):
    """2^-15 * sqrt(hop / 2): the coefficient step whose time-domain noise equals the 16-bit grid's (synthesis scales coefficient variance
    by 2 / hop)"""
    return 2.0 ** -15 * math.sqrt(hop / 2.0)


def mdct_frames(n, hop):
    """F = ceil(n / hop) + 1: the frames of a row of n samples"""
    return -(-int(n) // int(hop)) + 1


def mdct_plan(n, hop):
    """(frames a workgroup transforms, workgroups per row) wm_mdct_codec runs a row of n samples with: a function of (n, hop) alone"""
    import ctypes
    frames, wgs = ctypes.c_int(0), ctypes.c_longlong(0)
    lib.wm_mdct_codec_plan(int(n), int(hop), ctypes.addressof(frames), ctypes.addressof(wgs), None)
    return frames.value, wgs.value


def mdct_kcut(hop, band, bandwidth_hz=None, sample_rate=16000):
    """The first coefficient the bandwidth cut zeroes: floor(bandwidth_hz * 2 hop / sample_rate) rounded down to a multiple of `band`
    (coefficient k sits at (k + 1/2) sample_rate / (2 hop) Hz); None: hop, no cut.  A cut below one band, or above Nyquist, is refused."""
    if hop not in MDCT_HOPS:
        raise ValueError(f"hop must be one of {MDCT_HOPS}, got {hop!r}")
    if band not in MDCT_BANDS:
        raise ValueError(f"band must be one of {MDCT_BANDS}, got {band!r}")
    if bandwidth_hz is None:
        return hop
    for v, name in ((bandwidth_hz, "bandwidth_hz"), (sample_rate, "sample_rate")):
        _chk_positive(v, name)
    if 2.0 * bandwidth_hz > sample_rate:
        raise ValueError(f"bandwidth_hz must not lie above half the sample rate, got {bandwidth_hz} Hz at {sample_rate} Hz")
    kcut = int(math.floor(bandwidth_hz * 2 * hop / sample_rate)) // band * band
    if kcut < band:
        raise ValueError(f"bandwidth_hz {bandwidth_hz} Hz keeps less than one band of {band} coefficients at hop {hop}")
    return kcut


def mdct_codec(x, snr_db, *, hop=256, band=8, kcut=None, bandwidth_hz=None, sample_rate=16000, floor_step=None, quantise=True,
               codes_out=False, mask_in=None):
    """One launch of wm_mdct_codec along the last axis of a contiguous fp32 CUDA tensor (all leading axes are rows): MDCT analysis at hop
    `hop`, coefficients k >= kcut (given, or mdct_kcut(hop, band, bandwidth_hz, sample_rate); neither: hop, no cut) and those where mask_in
    holds 0 set to zero, the per-band quantiser at the per-row SNR snr_db
    (a (rows,) fp32 CUDA tensor, values in [0, 60]; ignored with quantise=False, where None is allowed) with floor_step (None:
    mdct_default_floor_step(hop)), synthesis with overlap-add.  codes_out: also returns the int16 codes, (rows, mdct_frames(n, hop), hop),
    as (y, codes).  mask_in: an int16 tensor of that shape.  A stand-in for lossy compression; parity with MP3 / AAC is unmeasured."""
    x = _chk(x, "x")
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError(f"x: needs at least one row of at least one sample, got shape {tuple(x.shape)}")
    if kcut is not None and bandwidth_hz is not None:
        raise ValueError("give kcut or bandwidth_hz, not both")
    derived = mdct_kcut(hop, band, bandwidth_hz, sample_rate)                    # hop and band from their sets
    if kcut is None:
        kcut = derived
    if isinstance(kcut, bool) or not isinstance(kcut, int) or kcut % band or not band <= kcut <= hop:
        raise ValueError(f"kcut: expected a multiple of band = {band} in [{band}, {hop}], got {kcut!r}")
    if floor_step is None:
        floor_step = mdct_default_floor_step(hop)
    _chk_positive(floor_step, "floor_step")
    if codes_out and not quantise:
        raise ValueError("codes_out needs quantise=True: the linear map has no codes")
    n = x.shape[-1]
    rows = x.numel() // n
    F = mdct_frames(n, hop)
    if snr_db is None and not quantise:
        snr_db = torch.zeros(rows, dtype=torch.float32, device=x.device)
    snr_db = _chk(snr_db, "snr_db", 1)
    if snr_db.shape[0] != rows or snr_db.device != x.device:
        raise ValueError(f"snr_db: expected {rows} values on {x.device}, got shape {tuple(snr_db.shape)} on {snr_db.device}")
    if mask_in is not None:
        mask_in = _chk(mask_in, "mask_in", None, torch.int16)
        if mask_in.numel() != rows * F * hop or mask_in.device != x.device:
            raise ValueError(f"mask_in: expected {rows} x {F} x {hop} int16 values on {x.device}, got shape {tuple(mask_in.shape)}")
    y = torch.empty_like(x)
    codes = torch.empty(rows, F, hop, dtype=torch.int16, device=x.device) if codes_out else None
    lib.wm_mdct_codec(_p(x), _p(y), _p(codes), _p(mask_in), _p(snr_db), rows, n, hop, band, kcut, float(floor_step), int(bool(quantise)),
                      _stream())
    return (y, codes) if codes_out else y


class MdctCodecFn(torch.autograd.Function):
    """y = synthesis(Q(cut(analysis(x)))) per row (mdct_codec) on the tape.  With the quantiser off the map A = synthesis . cut . analysis is
    symmetric, so the backward is the same launch with quantise=False on dy:
      grad "straight_through": dx = A dy -- the quantiser is taken for the identity, the bandwidth cut is kept, nothing is saved;
      grad "dead_zone":        dx = A_mask dy -- coefficients whose forward code was 0 pass no gradient; the forward's int16 codes are saved
                               and handed to the backward launch as mask_in.
    The step follows the band's own energy and so depends on x; that dependence is NOT differentiated (the step is a constant of the
    backward pass, as the rounding is)."""

    @staticmethod
    def forward(ctx, x, snr_db, hop, band, kcut, floor_step, grad):
        if grad not in MDCT_GRAD_MODES:
            raise ValueError(f"grad must be one of {MDCT_GRAD_MODES}, got {grad!r}")
        ctx.cfg = (hop, band, kcut, floor_step)
        ctx.dead = grad == "dead_zone" and ctx.needs_input_grad[0]
        if ctx.dead:
            y, codes = mdct_codec(x, snr_db, hop=hop, band=band, kcut=kcut, floor_step=floor_step, codes_out=True)
            ctx.save_for_backward(codes)
            return y
        return mdct_codec(x, snr_db, hop=hop, band=band, kcut=kcut, floor_step=floor_step)

    @staticmethod
    def backward(ctx, g):
        hop, band, kcut, floor_step = ctx.cfg
        mask = ctx.saved_tensors[0] if ctx.dead else None
        dx = mdct_codec(g.contiguous(), None, hop=hop, band=band, kcut=kcut, floor_step=floor_step, quantise=False, mask_in=mask)
        return dx, None, None, None, None, None, None


# ---------------------------------------------------------------------------------------------- reverb / echo
# Per-row causal FIR convolution (wm_fir_rows, csrc/fir_rows.hip) and synthetic room responses (wm_rir_synth, csrc/distort.hip): the long
# convolutive channel as a step of the graph.
FIR_MAX_TAPS = 16384


def _fir_taps(h, rows, device):
    h = _chk(h, "h")
    if h.dim() not in (1, 2) or h.shape[-1] < 1 or h.shape[-1] > FIR_MAX_TAPS:
        raise ValueError(f"h: expected (K,) or (rows, K) with 1 <= K <= {FIR_MAX_TAPS}, got shape {tuple(h.shape)}")
    if h.dim() == 2 and h.shape[0] != rows:
        raise ValueError(f"h: expected one response, or one per row ({rows}), got shape {tuple(h.shape)}")
    if h.device != device:
        raise ValueError(f"h: expected a tensor on {device}, got one on {h.device}")
    return h


def fir_rows(x, h, reverse=False):
    """One launch of wm_fir_rows along the last axis of a contiguous fp32 CUDA tensor (all leading axes are rows):
    y[r][t] = sum_k h_r[k] x[r][t - k], the first n samples of the full convolution, every row from silence; h is (K,), one response for
    all rows, or (rows, K), one per row.  reverse=True: y[r][t] = sum_k h_r[k] x[r][t + k], the transposed map (the backward pass)."""
    x = _chk(x, "x")
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError(f"x: needs at least one row of at least one sample, got shape {tuple(x.shape)}")
    n = x.shape[-1]
    rows = x.numel() // n
    h = _fir_taps(h, rows, x.device)
    K = h.shape[-1]
    y = torch.empty_like(x)
    lib.wm_fir_rows(_p(x), _p(h), _p(y), rows, n, K, K if h.dim() == 2 else 0, int(bool(reverse)), _stream())
    return y


class FirRowsFn(torch.autograd.Function):
    """y = H x per row (fir_rows) on the tape.  Saved for the backward: h alone; dx = H^T dy is the same launch with reverse=True.  h is a
    CONSTANT of the graph: no gradient flows to it (a response is measured or drawn, not trained)."""

    @staticmethod
    def forward(ctx, x, h):
        y = fir_rows(x, h)
        ctx.save_for_backward(h)
        return y

    @staticmethod
    def backward(ctx, g):
        return fir_rows(g.contiguous(), ctx.saved_tensors[0], reverse=True), None


def rir_synth(params, taps, sample_rate=16000, seed=0, draw=0, row0=0):
    """One launch of wm_rir_synth: (rows, taps) fp32 synthetic room responses from params, a (rows, 2) fp32 CUDA tensor of {rt60 in seconds,
    direct-to-reverberant ratio in dB} per row -- exponentially decaying Gaussian noise behind a direct tap, unit energy, NOT a room
    simulation.  Row r is a function of (seed, draw, row0 + r, params[r], taps, sample_rate) alone."""
    params = _chk(params, "params", 2)
    if params.shape[0] < 1 or params.shape[1] != 2:
        raise ValueError(f"params: expected (rows, 2) with at least one row, got shape {tuple(params.shape)}")
    _chk_int(taps, "taps", 1, FIR_MAX_TAPS)
    _chk_positive(sample_rate, "sample_rate")
    rows = params.shape[0]
    _chk_int(draw, "draw", 0, 2 ** 32 - 1)
    _chk_int(row0, "row0", 0, 2 ** 32 - rows)
    h = _f32(rows, taps, device=params.device)
    lib.wm_rir_synth(_p(params), _p(h), rows, taps, float(sample_rate), row0, _seed64(seed), draw, _stream())
    return h


# ---------------------------------------------------------------------------------------------- speed change / wow and flutter
# Time warp through a windowed-sinc interpolator (wm_time_warp, csrc/time_warp.hip): the output reads the input at a position that
# advances `speed` samples per sample, wobbles sinusoidally and starts a cut in.  The desynchronising channel as a step of the graph.
TIME_WARP_MAX_TABLE = 128 * 1024 // 4           # floats


def _time_warp_dims(zeros, res):
    _chk_int(zeros, "zeros", 4, 32)
    _chk_int(res, "res", 64, 1024)
    if res & (res - 1):
        raise ValueError(f"res: expected a power of two, got {res}")
    if zeros * res + 2 > TIME_WARP_MAX_TABLE:
        raise ValueError(f"zeros * res + 2 = {zeros * res + 2} floats is above the {TIME_WARP_MAX_TABLE} (128 KiB) a table may take")


_TIME_WARP_HOST = {}     # (zeros, res) -> the table (a CPU tensor)
_TIME_WARP_DEV = {}      # (zeros, res, device) -> the same on the device


def time_warp_table(zeros=16, res=512):
    """The interpolator's half response, a (zeros * res + 2,) fp32 CPU tensor (cached; do not write to it): sinc(v) * 0.5 (1 + cos(pi v /
    zeros)) at v = i / res, a Hann-windowed sinc with `zeros` zero crossings at `res` points each, computed in float64.  Entry 0 is exactly
    1, the entries at the other multiples of res and the last two exactly 0, so that a whole-sample shift is the identity."""
    _time_warp_dims(zeros, res)
    if (zeros, res) not in _TIME_WARP_HOST:
        import numpy as np
        v = np.arange(zeros * res + 2, dtype=np.float64) / res
        tab = np.sinc(v) * 0.5 * (1.0 + np.cos(np.pi * v / zeros))
        tab[res::res] = 0.0                      # the zero crossings, exactly
        tab[0] = 1.0
        tab[-2:] = 0.0
        _TIME_WARP_HOST[(zeros, res)] = torch.from_numpy(tab.astype(np.float32))
    return _TIME_WARP_HOST[(zeros, res)]


def _time_warp_table_on(zeros, res, device):
    key = (zeros, res, str(device))
    if key not in _TIME_WARP_DEV:
        _TIME_WARP_DEV[key] = time_warp_table(zeros, res).to(device)
    return _TIME_WARP_DEV[key]


def time_warp(x, params, table=None, adjoint=False, zeros=16, res=512):
    """One launch of wm_time_warp along the last axis of a contiguous fp32 CUDA tensor (all leading axes are rows):
    y[r][t] = sum_k W(p_r(t) - k) x[r][k] with p_r(t) = a t + off + d sinpi(2 frac(w t + phi)) from params, a (rows, 6) fp32 CUDA tensor of
    {a, off, d, w, phi, c} per row, and W the table's interpolated value at cutoff c (include/wm_hip.h has the definition).  table: the
    (zeros * res + 2,) fp32 half response, None for time_warp_table(zeros, res).  adjoint=True: the transposed map (the backward pass),
    defined for increasing p."""
    x = _chk(x, "x")
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError(f"x: needs at least one row of at least one sample, got shape {tuple(x.shape)}")
    n = x.shape[-1]
    rows = x.numel() // n
    _time_warp_dims(zeros, res)
    params = _chk(params, "params", 2)
    if tuple(params.shape) != (rows, 6):
        raise ValueError(f"params: expected ({rows}, 6), one {{a, off, d, w, phi, c}} per row, got shape {tuple(params.shape)}")
    table = _time_warp_table_on(zeros, res, x.device) if table is None else _chk(table, "table", 1)
    if table.shape[0] != zeros * res + 2:
        raise ValueError(f"table: expected zeros * res + 2 = {zeros * res + 2} values, got shape {tuple(table.shape)}")
    for t, name in ((params, "params"), (table, "table")):
        if t.device != x.device:
            raise ValueError(f"{name}: expected a tensor on {x.device}, got one on {t.device}")
    y = torch.empty_like(x)
    lib.wm_time_warp(_p(x), _p(params), _p(table), _p(y), rows, n, zeros, res, int(bool(adjoint)), _stream())
    return y


class TimeWarpFn(torch.autograd.Function):
    """y = W x per row (time_warp) on the tape.  Saved for the backward: params and the table alone; dx = W^T dy is the same launch with
    adjoint=True.  params and the table are CONSTANTS of the graph: no gradient flows to them (a speed is drawn, not trained)."""

    @staticmethod
    def forward(ctx, x, params, table, zeros, res):
        y = time_warp(x, params, table, zeros=zeros, res=res)
        ctx.save_for_backward(params, table)
        ctx.dims = (zeros, res)
        return y

    @staticmethod
    def backward(ctx, g):
        params, table = ctx.saved_tensors
        return time_warp(g.contiguous(), params, table, adjoint=True, zeros=ctx.dims[0], res=ctx.dims[1]), None, None, None, None


# ---------------------------------------------------------------------------------------------- pitch-preserving time stretch
# Waveform-similarity overlap-add (wm_wsola, csrc/wsola.hip): frames of the input copied to evenly spaced places of the output, each
# taken near its nominal place where it continues the one before best.  Given the chosen positions the map is a linear gather, so the
# backward pass is exact with the positions held constant.
WSOLA_MAX_N = 2 ** 30


def _wsola_dims(L, S):
    _chk_int(L, "L", 64, 1024)
    if L & (L - 1):
        raise ValueError(f"L: expected a power of two, got {L}")
    _chk_int(S, "S", 1, L // 2)


_WSOLA_HOST = {}         # L -> the rising half window (a CPU tensor)
_WSOLA_DEV = {}          # (L, device) -> the same on the device


def wsola_window(L=512):
    """The rising half of the frame's Hann window, an (L / 2,) fp32 CPU tensor (cached; do not write to it): 0.5 - 0.5 cos(pi j / Hs),
    Hs = L / 2, computed in float64.  Entry 0 is exactly 0, so a frame that continues its predecessor hands the samples on bit for bit."""
    _wsola_dims(L, 1)
    if L not in _WSOLA_HOST:
        import numpy as np
        hs = L // 2
        w = 0.5 - 0.5 * np.cos(np.pi * np.arange(hs, dtype=np.float64) / hs)
        w[0] = 0.0
        _WSOLA_HOST[L] = torch.from_numpy(w.astype(np.float32))
    return _WSOLA_HOST[L]


def _wsola_window_on(L, device):
    key = (L, str(device))
    if key not in _WSOLA_DEV:
        _WSOLA_DEV[key] = wsola_window(L).to(device)
    return _WSOLA_DEV[key]


def wsola_frames(n_out, L=512):
    """K, the frames of a row of n_out output samples: ceil(n_out / Hs) + 1"""
    return -(-n_out // (L // 2)) + 1


def wsola(x, rate, n_out=None, delta=None, adjoint=False, L=512, S=128):
    """One launch of wm_wsola along the last axis of a contiguous fp32 CUDA tensor (all leading axes are rows; include/wm_hip.h has the
    definition).  rate: (rows,) fp32 CUDA tensor, input samples consumed per output sample; a row whose rate is outside [1/4, 4] comes
    back as zeros.  n_out: the length of the result's last axis, None for that of x.
    delta=None: the search (mode 0); returns (y, delta), delta the (rows, K) int32 offsets of the chosen positions, K = wsola_frames(n_out, L).
    delta given: synthesis from these offsets (mode 1), clamped to [-S, S]; returns (y, delta).
    adjoint=True (delta is needed): x is the gradient of a result of x's length, and the transposed map of mode 1 comes back, dx with
    n_out samples a row -- here n_out is the FORWARD call's input length."""
    x = _chk(x, "x")
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError(f"x: needs at least one row of at least one sample, got shape {tuple(x.shape)}")
    n = x.shape[-1]
    rows = x.numel() // n
    _wsola_dims(L, S)
    n_res = _chk_int(n if n_out is None else n_out, "n_out", 1, WSOLA_MAX_N)
    if n > WSOLA_MAX_N or rows * max(n, n_res) > 2 ** 46:
        raise ValueError(f"rows = {rows}, n = {n}, n_out = {n_res}: a row may have 2^30 samples and a launch 2^46")
    rate = _chk(rate, "rate", 1)
    if rate.shape[0] != rows:
        raise ValueError(f"rate: expected ({rows},), one per row, got shape {tuple(rate.shape)}")
    if adjoint and delta is None:
        raise ValueError("delta: the adjoint needs the positions of the forward call")
    K = wsola_frames(n if adjoint else n_res, L)
    if delta is not None:
        delta = _chk(delta, "delta", 2, torch.int32)
        if tuple(delta.shape) != (rows, K):
            raise ValueError(f"delta: expected ({rows}, {K}), one offset per frame, got shape {tuple(delta.shape)}")
    for t, name in ((rate, "rate"), (delta, "delta")):
        if t is not None and t.device != x.device:
            raise ValueError(f"{name}: expected a tensor on {x.device}, got one on {t.device}")
    mode = 2 if adjoint else (0 if delta is None else 1)
    if delta is None:
        delta = torch.empty((rows, K), dtype=torch.int32, device=x.device)
    y = _f32(*x.shape[:-1], n_res, device=x.device)
    n_in, n_o = (n_res, n) if adjoint else (n, n_res)
    lib.wm_wsola(_p(x), _p(rate), _p(_wsola_window_on(L, x.device)), _p(y), _p(delta), rows, n_in, n_o, L, S, mode, _stream())
    return y if adjoint else (y, delta)


class WsolaFn(torch.autograd.Function):
    """y, delta = wsola(x, rate, n_out) on the tape.  Saved for the backward: delta and rate alone; dx is the mode-2 launch on them.  The
    positions are CONSTANTS of the graph: the map is differentiated as the linear gather it is once they are chosen, and no gradient
    flows to the rate (it is drawn, not trained)."""

    @staticmethod
    def forward(ctx, x, rate, n_out, L, S):
        y, delta = wsola(x, rate, n_out, L=L, S=S)
        ctx.save_for_backward(delta, rate)
        ctx.dims = (x.shape, L, S)
        ctx.mark_non_differentiable(delta)
        return y, delta

    @staticmethod
    def backward(ctx, g, _):
        delta, rate = ctx.saved_tensors
        shape, L, S = ctx.dims
        dx = wsola(g.contiguous(), rate, shape[-1], delta, adjoint=True, L=L, S=S)
        return dx.reshape(shape), None, None, None, None


# ---------------------------------------------------------------------------------------------- predictive speech-codec stand-in
# Per-frame linear prediction -> open-loop quantiser on the residual -> all-pole synthesis (wm_lpc_codec, csrc/lpc_codec.hip): the signal
# path ADPCM / CELP / AMR-WB / SILK share, as a step of the graph.  A stand-in, not a speech codec: no LSP interpolation, no pitch
# predictor, no noise feedback, no entropy coder; parity with a real one is unmeasured.
LPC_FRAMES = (160, 320, 640)
LPC_MAX_ORDER = 16
LPC_GRAD_MODES = ("straight_through", "dead_zone")
LPC_FLOOR_STEP = 2.0 ** -15

_LPC_HOST = {}           # (order, sample_rate) -> (lag, expand), CPU tensors
_LPC_DEV = {}            # (order, sample_rate, device) -> the same on the device


def _lpc_dims(frame, order):
    if isinstance(frame, bool) or not isinstance(frame, int) or frame not in LPC_FRAMES:
        raise ValueError(f"frame must be one of {LPC_FRAMES}, got {frame!r}")
    _chk_int(order, "order", 2, LPC_MAX_ORDER)


def lpc_tables(order=16, sample_rate=16000):
    """(lag, expand), fp32 CPU tensors (cached; do not write to them), evaluated in float64 and rounded once.  lag (order + 1,): the lag
    window the autocorrelation is multiplied by, exp(-0.5 (2 pi 60 k / sample_rate)^2) -- a 60 Hz Gaussian -- with lag[0] = 1 + 1e-4, the
    white-noise correction.  expand (order,): 0.994^k for k = 1 .. order, the bandwidth expansion of the coefficients."""
    _chk_int(order, "order", 2, LPC_MAX_ORDER)
    _chk_positive(sample_rate, "sample_rate")
    key = (order, float(sample_rate))
    if key not in _LPC_HOST:
        import numpy as np
        k = np.arange(order + 1, dtype=np.float64)
        lag = np.exp(-0.5 * (2.0 * np.pi * 60.0 * k / float(sample_rate)) ** 2)
        lag[0] = 1.0 + 1e-4
        expand = 0.994 ** k[1:]
        _LPC_HOST[key] = (torch.from_numpy(lag.astype(np.float32)), torch.from_numpy(expand.astype(np.float32)))
    return _LPC_HOST[key]


def _lpc_tables_on(order, sample_rate, device):
    key = (order, float(sample_rate), str(device))
    if key not in _LPC_DEV:
        _LPC_DEV[key] = tuple(t.to(device) for t in lpc_tables(order, sample_rate))
    return _LPC_DEV[key]


def lpc_frames(n, frame=320):
    """F = ceil(n / frame): the frames of a row of n samples"""
    return -(-int(n) // int(frame))


def lpc_codec(x, snr_db, *, frame=320, order=16, sample_rate=16000, floor_step=None, quantise=True, coeffs=None, coeffs_out=False,
              codes_out=False, mask_in=None, adjoint=False):
    """One launch of wm_lpc_codec along the last axis of a contiguous fp32 CUDA tensor (all leading axes are rows; include/wm_hip.h has the
    definition): per frame of `frame` samples an order-`order` predictor from the windowed autocorrelation (lpc_tables(order,
    sample_rate) are its lag window and bandwidth expansion), the residual quantised at the per-row SNR snr_db (a (rows,) fp32 CUDA
    tensor, values in [0, 60]; ignored with quantise=False, where None is allowed) but never finer than floor_step (None: 2^-15), and
    all-pole synthesis.  coeffs: a (rows, lpc_frames(n, frame), order) fp32 tensor that replaces the analysis.  mask_in: a (rows, n) int16
    tensor; the residual is set to 0 where it holds 0.  coeffs_out / codes_out: also return the coefficients the launch used / the int16
    codes (rows, n); the result is then the tuple (y[, coeffs][, codes]).  adjoint=True (needs coeffs, quantise=False): x is a gradient
    and the transpose of the linear map synthesis . mask . residual filter at these coefficients comes back.  A stand-in for a speech
    codec; parity with a real one is unmeasured."""
    x = _chk(x, "x")
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError(f"x: needs at least one row of at least one sample, got shape {tuple(x.shape)}")
    _lpc_dims(frame, order)
    if floor_step is None:
        floor_step = LPC_FLOOR_STEP
    _chk_positive(floor_step, "floor_step")
    if codes_out and not quantise:
        raise ValueError("codes_out needs quantise=True: the linear map has no codes")
    if adjoint and (coeffs is None or quantise or coeffs_out or codes_out):
        raise ValueError("adjoint: needs coeffs and quantise=False, and has neither coeffs_out nor codes_out")
    n = x.shape[-1]
    rows = x.numel() // n
    if n > 2 ** 34 or rows * n > 2 ** 46:
        raise ValueError(f"rows = {rows}, n = {n}: a row may have 2^34 samples and a launch 2^46")
    F = lpc_frames(n, frame)
    if snr_db is None and not quantise:
        snr_db = torch.zeros(rows, dtype=torch.float32, device=x.device)
    snr_db = _chk(snr_db, "snr_db", 1)
    if snr_db.shape[0] != rows:
        raise ValueError(f"snr_db: expected ({rows},), one per row, got shape {tuple(snr_db.shape)}")
    if coeffs is not None:
        coeffs = _chk(coeffs, "coeffs")
        if coeffs.numel() != rows * F * order or coeffs.shape[-1] != order:
            raise ValueError(f"coeffs: expected {rows} x {F} x {order} fp32 values, got shape {tuple(coeffs.shape)}")
    if mask_in is not None:
        mask_in = _chk(mask_in, "mask_in", None, torch.int16)
        if mask_in.numel() != rows * n:
            raise ValueError(f"mask_in: expected {rows} x {n} int16 values, got shape {tuple(mask_in.shape)}")
    for t, name in ((snr_db, "snr_db"), (coeffs, "coeffs"), (mask_in, "mask_in")):
        if t is not None and t.device != x.device:
            raise ValueError(f"{name}: expected a tensor on {x.device}, got one on {t.device}")
    lag, expand = _lpc_tables_on(order, sample_rate, x.device)
    y = torch.empty_like(x)
    used = torch.empty(rows, F, order, dtype=torch.float32, device=x.device) if coeffs_out else None
    codes = torch.empty(rows, n, dtype=torch.int16, device=x.device) if codes_out else None
    lib.wm_lpc_codec(_p(x), _p(y), _p(coeffs), _p(used), _p(codes), _p(mask_in), _p(snr_db), _p(lag), _p(expand), rows, n, frame, order,
                     float(floor_step), int(bool(quantise)), int(bool(adjoint)), _stream())
    out = (y,) + ((used,) if coeffs_out else ()) + ((codes,) if codes_out else ())
    return out if len(out) > 1 else y


class LpcCodecFn(torch.autograd.Function):
    """y = synthesis(Q(residual(x))) per row (lpc_codec) on the tape.  The coefficients and the steps follow x, and that dependence is
    NOT differentiated: they are constants of the backward pass, as the MDCT codec's steps and WSOLA's positions are.
      grad "straight_through": with the quantiser taken for the identity, synthesis inverts the residual filter exactly, so the map is the
                               identity and the gradient IS dy: no launch, nothing saved;
      grad "dead_zone":        residual samples whose forward code was 0 pass no gradient: the forward's coefficients and int16 codes
                               are saved, and dx is the adjoint launch at those coefficients with the codes as mask_in."""

    @staticmethod
    def forward(ctx, x, snr_db, frame, order, sample_rate, floor_step, grad):
        if grad not in LPC_GRAD_MODES:
            raise ValueError(f"grad must be one of {LPC_GRAD_MODES}, got {grad!r}")
        ctx.cfg = (frame, order, sample_rate, floor_step)
        ctx.dead = grad == "dead_zone" and ctx.needs_input_grad[0]
        if ctx.dead:
            y, coeffs, codes = lpc_codec(x, snr_db, frame=frame, order=order, sample_rate=sample_rate, floor_step=floor_step,
                                         coeffs_out=True, codes_out=True)
            ctx.save_for_backward(coeffs, codes)
            return y
        return lpc_codec(x, snr_db, frame=frame, order=order, sample_rate=sample_rate, floor_step=floor_step)

    @staticmethod
    def backward(ctx, g):
        if not ctx.dead:
            return g, None, None, None, None, None, None
        frame, order, sample_rate, floor_step = ctx.cfg
        coeffs, codes = ctx.saved_tensors
        dx = lpc_codec(g.contiguous(), None, frame=frame, order=order, sample_rate=sample_rate, floor_step=floor_step, quantise=False,
                       coeffs=coeffs, mask_in=codes, adjoint=True)
        return dx.reshape(g.shape), None, None, None, None, None, None


# ---------------------------------------------------------------------------------------------- STOI
# Short-time objective intelligibility of rows at 10 kHz (wm_stoi, csrc/stoi.hip; the definition is in include/wm_hip.h): the quality
# column of the evaluation side.  Nothing is differentiated: a measure, not a loss.
def stoi_plan(rows, n):
    """bytes of scratch one wm_stoi launch on (rows, n) needs"""
    import ctypes
    for v, name in ((rows, "rows"), (n, "n")):
        _chk_int(v, name, 1, math.inf, "a positive int")
    if n > 2 ** 34 or rows * n > 2 ** 46:
        raise ValueError(f"rows = {rows}, n = {n}: a row may have 2^34 samples and a launch 2^46")
    need = ctypes.c_longlong(0)
    lib.wm_stoi_plan(rows, n, ctypes.addressof(need), None)
    return need.value


def _stoi_rows(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise ValueError(f"{name}: expected dtype torch.float32, got {t.dtype}")
    if t.dim() == 3 and t.shape[1] == 1:
        rows = t.reshape(t.shape[0], t.shape[2])
    elif t.dim() == 2:
        rows = t
    elif t.dim() == 1:
        rows = t[None]
    else:
        raise ValueError(f"{name}: expected (B, 1, T), (C, N) or (N,), got shape {tuple(t.shape)}")
    if rows.shape[0] < 1 or rows.shape[1] < 1:
        raise ValueError(f"{name}: needs at least one row of at least one sample, got shape {tuple(t.shape)}")
    return rows.contiguous()


def stoi(x, y, sample_rate=16000):
    """STOI of every row of y (the processed signal) against the same row of x (the reference): float32 tensors of equal shape (B, 1, T),
    (C, N) or (N,) at `sample_rate`.  Returns (d (rows,) float32, kept (rows,) int32) on the inputs' device: the score and the number of
    frames that survived silent-frame removal.  CUDA tensors: one wm_stoi call, preceded by ONE resample_rows launch on x and y stacked
    unless sample_rate == 10000.  CPU tensors: the float64 restatement of quality.stoi_rows_host (after the host resampler)."""
    from .quality import STOI_RATE, stoi_rows_host
    rate = _rate(sample_rate, "sample_rate")
    xr, yr = _stoi_rows(x, "x"), _stoi_rows(y, "y")
    if x.shape != y.shape:
        raise ValueError(f"x and y: expected equal shapes, got {tuple(x.shape)} and {tuple(y.shape)}")
    if xr.device != yr.device:
        raise ValueError(f"x and y: expected one device, got {xr.device} and {yr.device}")
    rows = xr.shape[0]
    if not xr.is_cuda:
        if rate != STOI_RATE:
            from .inference import _resample_rows_host
            both = _resample_rows_host(torch.cat([xr, yr], dim=0), rate, STOI_RATE)
            xr, yr = both[:rows], both[rows:]
        return stoi_rows_host(xr, yr)
    if rate != STOI_RATE:
        both = resample_rows(torch.cat([xr, yr], dim=0), rate, STOI_RATE)
        xr, yr = both[:rows], both[rows:]
    n = xr.shape[1]
    d = _f32(rows, device=xr.device)
    kept = torch.empty(rows, dtype=torch.int32, device=xr.device)
    scratch = torch.empty(stoi_plan(rows, n) // 4, dtype=torch.float32, device=xr.device)
    lib.wm_stoi(_p(xr), _p(yr), _p(d), _p(kept), _p(scratch), rows, n, _stream())
    return d, kept


# ---------------------------------------------------------------------------------------------- splice attack and localisation
# wm_splice / wm_splice_bwd, wm_bce_masked_fwd / _bwd and wm_loc_score (csrc/splice.hip; the definitions are in include/wm_hip.h).  Labels
# travel as bit masks: (rows, ceil(n / 32)) int32 tensors, bit j of word w = sample 32 w + j, 1 = "still watermarked", tail bits zero.
SPLICE_MAX_SPANS = 8
SPLICE_MAX_N = 2 ** 24


def label_words(n):
    """words per row of a label mask over n samples"""
    return (int(n) + 31) // 32


def _lab(lab, rows, n, name="lab"):
    lab = _chk(lab, name, 2, torch.int32)
    if tuple(lab.shape) != (rows, label_words(n)):
        raise ValueError(f"{name}: expected a ({rows}, {label_words(n)}) int32 mask for {rows} rows of {n} samples, got shape {tuple(lab.shape)}")
    return lab


class SpliceFn(torch.autograd.Function):
    """wm_splice on the tape: spans of the watermarked rows `a` replaced by the clean rows `b` (as they are, silenced, or moved within the
    row), with the spans drawn in the kernel from (seed, draw, row0 + r).  cut = (max_spans, p_span, len_lo, len_hi, p_original,
    p_silence), the lengths in samples.  Returns (y, lab): y like a, lab the (rows, ceil(n / 32)) int32 label mask, not differentiable.
    Saved for the backward: lab alone.  da = wm_splice_bwd(dy, lab); b is data and gets no gradient."""

    @staticmethod
    def forward(ctx, a, b, cut, seed, draw, row0):
        a, b = _chk(a, "a"), _chk(b, "b")
        if a.shape != b.shape or a.device != b.device:
            raise ValueError(f"a and b: expected equal shapes on one device, got {tuple(a.shape)} on {a.device} and {tuple(b.shape)} on {b.device}")
        if a.dim() < 1 or a.numel() == 0:
            raise ValueError(f"a: needs at least one row of at least one sample, got shape {tuple(a.shape)}")
        n = a.shape[-1]
        rows = a.numel() // n
        max_spans, p_span, len_lo, len_hi, p_original, p_silence = cut
        y = torch.empty_like(a)
        lab = torch.empty(rows, label_words(n), dtype=torch.int32, device=a.device)
        lib.wm_splice(_p(a), _p(b), _p(y), _p(lab), rows, n, int(row0), _seed64(seed), int(draw), int(max_spans),
                      float(p_span), int(len_lo), int(len_hi), float(p_original), float(p_silence), _stream())
        ctx.save_for_backward(lab)
        ctx.mark_non_differentiable(lab)
        return y, lab

    @staticmethod
    def backward(ctx, g, _glab):
        (lab,) = ctx.saved_tensors
        g = _chk(g, "grad")
        n = g.shape[-1]
        da = torch.empty_like(g)
        lib.wm_splice_bwd(_p(g), _p(lab), _p(da), g.numel() // n, n, _stream())
        return da, None, None, None, None, None


def splice(a, b, *, max_spans=2, p_span=0.5, len_lo=800, len_hi=6400, p_original=1 / 3, p_silence=1 / 3, seed=0, draw=0, row0=0):
    """(y, lab) of one wm_splice call on contiguous fp32 CUDA tensors a (watermarked) and b (clean) of one shape, all leading axes rows;
    the lengths in samples.  Differentiable in a (ops.SpliceFn)."""
    return SpliceFn.apply(a, b, (max_spans, p_span, len_lo, len_hi, p_original, p_silence), seed, draw, row0)


class MaskedBCEFn(torch.autograd.Function):
    """(loc, bce) of wm_bce_masked_fwd: BCEFn against per-sample labels.  logits (2B, T, 1 + bits), message (B,) int64, lab the (B,
    ceil(T / 32)) int32 label mask of the watermarked half; the clean half has target 0 throughout.  The bit term averages over the
    samples whose label is 1 -- their number N1 is counted on the device and stays there for the backward (`count`, a device int64
    saved with logits, message and lab): no host sync."""

    @staticmethod
    def forward(ctx, logits, message, lab):
        logits = _chk(logits, "logits", 3)
        message = _chk(message, "message", 1, torch.int64)
        R, T, NO = logits.shape
        B = message.shape[0]
        if R != 2 * B:
            raise ValueError(f"logits must hold [watermarked; clean] = 2*B clips, got {R} for B={B}")
        lab = _lab(lab, B, T)
        dev = logits.device
        part = _f32(3 * R * ((T * NO + 4095) // 4096), device=dev)
        out = torch.zeros(2, dtype=torch.float32, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        lib.wm_bce_masked_fwd(_p(logits), _p(message), _p(lab), _p(part), _p(count), _p(out[0]), _p(out[1]), B, R, T, NO, _stream())
        ctx.save_for_backward(logits, message, lab, count)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_loc, g_bce):
        logits, message, lab, count = ctx.saved_tensors
        R, T, NO = logits.shape
        gl = g_loc.contiguous().float().reshape(1) if g_loc is not None else torch.zeros(1, device=logits.device)
        gb = g_bce.contiguous().float().reshape(1) if g_bce is not None else torch.zeros(1, device=logits.device)
        d = torch.empty_like(logits)
        lib.wm_bce_masked_bwd(_p(logits), _p(message), _p(lab), _p(count), _p(gl), _p(gb), _p(d), message.shape[0], R, T, NO, _stream())
        return d, None, None


def loc_threshold_logit(threshold):
    """log(p / (1 - p)) in float64 on the host: the logit the probability threshold p stands for; exactly 0.0 at p = 0.5"""
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not 0.0 <= threshold <= 1.0:
        raise ValueError(f"threshold: expected a probability in [0, 1], got {threshold!r}")
    p = float(threshold)
    if p == 0.5:
        return 0.0
    if p == 0.0:
        return -math.inf
    if p == 1.0:
        return math.inf
    return math.log(p / (1.0 - p))


def loc_counts(logits, lab, threshold=0.5, want_pred=False):
    """The per-sample prediction sigmoid(logits[r, t, 0]) > threshold, taken as logits[r, t, 0] > log(p / (1 - p)), against the label mask
    `lab` ((lab_rows, ceil(T / 32)) int32 with lab_rows <= R: rows behind it have label 0; None: every label is 1).  One wm_loc_score
    launch.  Returns counts (R, 4) int32 = {tp, fp, fn, tn} on the device, exact; with want_pred also pred (R, ceil(T / 32)) int32, the
    prediction in the mask layout.  NaN logits predict 0."""
    logits = _chk(logits, "logits", 3)
    R, T, NO = logits.shape
    if R < 1 or T < 1 or NO < 1:
        raise ValueError(f"logits: needs at least one row, one sample and one channel, got shape {tuple(logits.shape)}")
    thr = loc_threshold_logit(threshold)
    lab_rows = 0
    if lab is not None:
        lab = _chk(lab, "lab", 2, torch.int32)
        lab_rows = lab.shape[0]
        if lab_rows < 1 or lab_rows > R or lab.shape[1] != label_words(T):
            raise ValueError(f"lab: expected (at most {R}, {label_words(T)}) int32, got shape {tuple(lab.shape)}")
    counts = torch.empty(R, 4, dtype=torch.int32, device=logits.device)
    pred = torch.empty(R, label_words(T), dtype=torch.int32, device=logits.device) if want_pred else None
    lib.wm_loc_score(_p(logits), _p(lab), thr, _p(counts), _p(pred), R, T, NO, lab_rows, _stream())
    return (counts, pred) if want_pred else counts


# ---------------------------------------------------------------------------------------------- per-clip detection scores
# wm_clip_scores (csrc/clip_scores.hip; the definition is in include/wm_hip.h): everything an operating-point report needs of the
# Detector's logits, in one pass.  Nothing is differentiated: a measure, not a loss.
CLIP_SCORES_MAX_T = 2 ** 24
ClipScores = collections.namedtuple("ClipScores", "prob llr votes words biterr")


def clip_scores_plan(R, T, NO):
    """bytes of scratch one wm_clip_scores launch on (R, T, NO) logits needs"""
    import ctypes
    for v, name in ((R, "R"), (T, "T"), (NO, "NO")):
        _chk_int(v, name, 1, math.inf, "a positive int")
    if T > CLIP_SCORES_MAX_T or NO > 64 or R * T * NO > 2 ** 46:
        raise ValueError(f"R = {R}, T = {T}, NO = {NO}: a clip may have 2^24 samples and 64 channels, a launch 2^46 elements")
    need = ctypes.c_longlong(0)
    lib.wm_clip_scores_plan(R, T, NO, ctypes.addressof(need), None)
    return need.value


def clip_scores(logits, message=None, threshold=0.5):
    """Per-clip scores of the Detector's logits (R, T, NO) float32, channel 0 the detection logit and channels 1.. the message bits:
    ClipScores(prob, llr, votes, words, biterr) on the logits' device --
      prob (R,) float32         the mean over t of sigmoid(logits[:, t, 0]): the reference's per-clip score
      llr (R, NO) float32       the mean logit of every channel
      votes (R, NO) int32       exact: the samples with sigmoid(channel 0) > threshold (taken as logit > log(p / (1 - p)), as
                                loc_counts does), and for o >= 1 the samples with logit > 0; a NaN casts no vote
      words (R, 2) int64        the decoded message: [:, 0] the majority of the hard decisions (a tie is 0), [:, 1] the sign of the summed logits
      biterr (B, 2) int32       the wrong bits of words[:B] against `message` ((B,) int64, B <= R: the watermarked rows come first);
                                (0, 2) without a message
    CUDA tensors: one wm_clip_scores call, no host sync.  CPU tensors: the float64 restatement detection.clip_scores_host rounded to
    float32, the integers exact -- so that what is built on top runs without a GPU."""
    if not isinstance(logits, torch.Tensor):
        raise TypeError(f"logits: expected a tensor, got {type(logits).__name__}")
    if logits.dtype != torch.float32 or logits.dim() != 3:
        raise ValueError(f"logits: expected a float32 (R, T, NO) tensor, got {logits.dtype} with shape {tuple(logits.shape)}")
    R, T, NO = logits.shape
    if R < 1 or T < 1 or NO < 1 or NO > 64 or T > CLIP_SCORES_MAX_T or R * T * NO > 2 ** 46:
        raise ValueError(f"logits: needs at least one row, 1 .. 2^24 samples, 1 .. 64 channels and at most 2^46 elements, got shape {tuple(logits.shape)}")
    thr = loc_threshold_logit(threshold)
    B = 0
    if message is not None:
        if not isinstance(message, torch.Tensor) or message.dtype != torch.int64 or message.dim() != 1:
            raise ValueError("message: expected a (B,) int64 tensor")
        if message.device != logits.device:
            raise ValueError(f"logits and message: expected one device, got {logits.device} and {message.device}")
        B = message.shape[0]
        if B > R:
            raise ValueError(f"message: at most one per row of logits ({R}), got {B}")
    dev = logits.device
    if not logits.is_cuda:
        from .detection import clip_scores_host
        prob, llr, votes, words, biterr = clip_scores_host(logits.detach().numpy(), None if message is None else message.numpy(), thr)
        return ClipScores(torch.from_numpy(prob.astype("float32")), torch.from_numpy(llr.astype("float32")), torch.from_numpy(votes),
                          torch.from_numpy(words), torch.from_numpy(biterr))
    logits = logits.contiguous()
    message = None if message is None else message.contiguous()
    prob, llr = _f32(R, device=dev), _f32(R, NO, device=dev)
    votes = torch.empty(R, NO, dtype=torch.int32, device=dev)
    words = torch.empty(R, 2, dtype=torch.int64, device=dev)
    biterr = torch.empty(B, 2, dtype=torch.int32, device=dev)
    scratch = torch.empty(clip_scores_plan(R, T, NO) // 4, dtype=torch.int32, device=dev)
    lib.wm_clip_scores(_p(logits), _p(message) if B else None, thr, _p(prob), _p(llr), _p(votes), _p(words), _p(biterr) if B else None,
                       _p(scratch), B, R, T, NO, _stream())
    return ClipScores(prob, llr, votes, words, biterr)


# ---------------------------------------------------------------------------------------------- clip curation features
# wm_clip_features (csrc/clip_features.hip; the definition is in include/wm_hip.h): the speech / noise feature table and the silence
# measure of the reference's dataset scripts, one launch for all rows.  Nothing is differentiated: a measure, not a loss.
ClipFeaturesPlan = collections.namedtuple("ClipFeaturesPlan", "frames energy_frames lds_bytes")


def clip_features_plan(rows, n, sample_rate=16000):
    """ClipFeaturesPlan(frames, energy_frames, lds_bytes) of one wm_clip_features launch on (rows, n) at sample_rate: F = 1 + n // 512
    spectral frames per row, the 25-ms frames of energy_std, the LDS one workgroup takes.  ValueError where the launch would be refused."""
    import ctypes
    from .curate import check_shape
    _chk_int(rows, "rows", 1, 2 ** 40)
    _chk_int(n, "n", 1, math.inf, "a positive int")
    sr = check_shape(n, sample_rate)
    out = (ctypes.c_int * 3)()
    base = ctypes.addressof(out)
    lib.wm_clip_features_plan(rows, n, sr, base, base + 4, base + 8, None)
    return ClipFeaturesPlan(out[0], out[1], out[2])


def clip_features(x, sample_rate=16000, frames=False):
    """The curation features of every row of x: a float32 tensor (B, 1, T), (C, N) or (N,) at `sample_rate`, 400 .. 32768 samples a row.
    Returns (feat (rows, 16) float32, counts (rows, 4) int32) on x's device, and with frames=True also frames (rows, F, 4) float32 -- per
    spectral frame the centroid, the bandwidth, the roll-off bin and the zero-crossing count.  The columns of feat are curate.FEATURES
    (then three reserved zeros); counts holds the zero-crossing total, the speech score, the non-finite flag and the label (1 speech,
    0 noise, -1 non-finite).  CUDA tensors: ONE wm_clip_features launch, no host sync.  CPU tensors: the float64 restatement
    curate.clip_features_host rounded to float32, the integers exact."""
    from . import curate
    rows_t = _stoi_rows(x, "x")
    rows, n = rows_t.shape
    sr = curate.check_shape(n, sample_rate)
    if not rows_t.is_cuda:
        out = curate.clip_features_host(rows_t.detach().numpy(), sr, frames)
        res = (torch.from_numpy(out[0].astype("float32")), torch.from_numpy(out[1]))
        return res + (torch.from_numpy(out[2].astype("float32")),) if frames else res
    dev = rows_t.device
    F = clip_features_plan(rows, n, sr).frames
    tab = curate.tables_on(sr, dev)
    feat = _f32(rows, 16, device=dev)
    counts = torch.empty(rows, 4, dtype=torch.int32, device=dev)
    per = _f32(rows, F, 4, device=dev) if frames else None
    lib.wm_clip_features(_p(rows_t), _p(tab["sos"]), _p(tab["fb"]), _p(tab["klo"]), _p(tab["khi"]), _p(tab["dct"]), _p(feat), _p(counts),
                         _p(per), rows, n, sr, tab["warm"], _stream())
    return (feat, counts, per) if frames else (feat, counts)
