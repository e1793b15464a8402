"""The float64 yardsticks of the main16 LSTM kernels (csrc/lstm_fwd.hip, lstm_bwd.hip, lstm_grad.hip behind ops.LSTMFn) with the case
tables, the input builders and the tolerance rules, for tests/test_gpu_lstm_edges.py (GPU) and tests/test_lstm_yardstick_cpu.py (the
input conditions and the float32 restatements, without a GPU).  `import lstm_yardstick as Y`.  Nothing from the package.

References.  oracle.wm_oracle.lstm_forward in float64, differentiated by autograd; lstm_trace is the same loop, statement for statement
(the CPU file holds their outputs bit for bit against each other), that also returns what the kernels save for the backward: the gate
activations [B, T, 256] in the kernels' column order n' = unit * 4 + gate (csrc/lstm.hpp) and the cell states [B, T, 64].

A. The activation sweep: csrc/lstm.hpp's own claim about sigm (v_exp_f32 + v_rcp_f32) and tanh_s(z) = 2 sigm(2z) - 1, tested directly.
wm_lstm_fwd takes pre-activations xp [B, T, 256]; with h_0 = 0 its step 0 applies the gate functions to xp[:, 0] itself, so the saved
gates[:, 0] are sigm (i, f, o columns) and tanh_s (g columns) of chosen z.  Bounds, per element, from the operations themselves:
sigm(z) = v_rcp_f32(1 + v_exp_f32(-z log2 e)).  The product -z log2 e is rounded (U of the argument: |z| U of the exponential), v_exp_f32 and
v_rcp_f32 are accurate to 1 ulp (2 U; the CDNA instruction set reference), the sum 1 + e rounds once (U).  An error delta of e moves
sigma = 1 / (1 + e) by sigma (1 - sigma) delta, an error of the sum or the reciprocal by sigma times itself:
    d_sigm(z)      sigma (1 - sigma) (|z| + 2) U + 3 U sigma + 2^-126        (the last: a denormal result may be flushed)   <= 1.9e-7
    d_tanh(z)      2 d_sigm(2 z) + U |tanh z|                               (2 s - 1 fused: one rounding)                  <= 4.3e-7
    c_0 = i g      d_i |g| + |i| d_g + ulp32(c_0) / 2
    h_0 = o tanh_s(c_0)    d_o |tanh c_0| + |o| (d_tanh(c_0) + d_c) + ulp32(h_0) / 2          (|tanh'| <= 1)
csrc/lstm.hpp used to state "<= 3e-8 for every z" (SIGM_ABS_CLAIMED): that is the first term alone, with |z| O(1e-7) read as its
largest value; it leaves out the roundings of 1 + e and of the reciprocal, 3 U sigma = 1.8e-7 where sigma is near 1.  Correctly rounded
float32 arithmetic already misses 3e-8 + ulp32 / 2 (tests/test_lstm_yardstick_cpu.py shows it: 7.4e-8 against 6.0e-8 at z = 2.69), so
the header was wrong, not the function; the header now carries the bound above.  Measured on the MI355X: sigm 7.4e-8 at z = 2.69,
tanh_s 1.6e-7 at z = 1.21; the largest error / bound 0.72 (gates), 0.67 (c_0), 0.33 (h_0); finite for every z in +-1e4.

B. Everything behind the recurrence (routes by length, saturated gates, the saved tensors) is held by the project's rule
max(8 * e32, floor) (loss_yardstick.bar / held), e32 the distance of the float32 run of the same loop to the float64 one; floors
FWD_FLOOR = 1e-5 and GRAD_FLOOR = 2e-4, a tenth of test_gpu_parity.py's tolerances.  tests/test_lstm_yardstick_cpu.py asserts that no
case's bar rises above those tolerances themselves (a case that needed more would be badly conditioned, not the kernel wrong), and for
the saturated cases that they are what they claim.

Measured on 1 x MI355X (tests/test_gpu_lstm_edges.py prints every figure), the largest distance / bound:

    activation sweep            sigm / tanh_s 0.72, c_0 0.67, h_0 0.33
    ops.LSTMFn, T = 4 ... 68    h 0.04, gradients 0.003
    saved gates, cst            wm_lstm_fwd_fused (both builds) 0.035, wm_lstm_xproj + wm_lstm_fwd 0.042
    saturated gates             h 0.14, gradients 0.014
    zero x / all-zero           h 0.11, gradients 0.003; h, dx, dW_ih, dW_hh exactly 0 where they must be
"""
import functools

import numpy as np
import torch

from loss_yardstick import held, rel_err  # noqa: F401  (the rule; re-exported for the two test files)
from oracle import wm_oracle as O
from yardstick_common import U, ulp32

H = 64
FWD_FLOOR, GRAD_FLOOR = 1e-5, 2e-4
PARITY_FWD_TOL, PARITY_GRAD_TOL = 1e-4, 2e-3
GRAD_NAMES = ("dx", "dW_ih", "dW_hh", "db_ih", "db_hh")


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def uniform(*shape, seed=0, scale=1.0):
    return (torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1) * scale


# ------------------------------------------------------------------------------------------------------------ A. activation sweep
SIGM_ABS_CLAIMED = 3e-8                          # what csrc/lstm.hpp stated before: kept to show that float32 itself misses it
FTZ = 2.0 ** -126
SWEEP_B, SWEEP_T = 8, 4


def sweep_z(neg_zero=False):
    """float32: +-{0, 2^-126, 1e-20, 1e-6, 1e-3, 0.1 ... 20 in steps of 0.37, 44, 87, 88.8, 100, 1e4}: 128 values"""
    base = np.concatenate([[0.0, 2.0 ** -126, 1e-20, 1e-6, 1e-3], np.arange(0.1, 20.0, 0.37), [44.0, 87.0, 88.8, 100.0, 1e4]])
    z = np.concatenate([base, -base]).astype(np.float32)
    assert z.size == 128
    if neg_zero:
        z[z == 0] = -0.0
    return z


def sweep_xp(neg_zero=False):
    """xp [8, 4, 256] float32: at t = 0 gate q of slot s = b * 64 + unit holds z[((2 q + 1) s + 17 q) % 128] -- an odd multiplier, so
    every z stands four times in every gate's columns and the (i, g, o) of a unit are different combinations; t > 0: unit normal"""
    z = sweep_z(neg_zero)
    xp = rnd(SWEEP_B, SWEEP_T, 256, seed=7).numpy().copy()
    s = np.arange(SWEEP_B * H)
    xp[:, 0, :] = np.stack([z[((2 * q + 1) * s + 17 * q) % 128] for q in range(4)], axis=1).reshape(SWEEP_B, 256)
    return xp


def sigm64(z):
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def d_sigm(z, s=None):
    """the bound of sigm at z (s = sigma(z) in float64)"""
    s = sigm64(z) if s is None else s
    return s * (1.0 - s) * (np.abs(z) + 2.0) * U + 3.0 * U * s + FTZ


def d_tanh(z):
    return 2.0 * d_sigm(2.0 * np.asarray(z, dtype=np.float64)) + U * np.abs(np.tanh(z))


def sweep_ref(xp):
    """float64 {gates [8, 256] (activations of step 0, kernel column order), c [8, 64], h [8, 64]} with their bounds {.._bound}"""
    a = np.asarray(xp[:, 0, :], dtype=np.float64).reshape(-1, H, 4)
    i, f, o, g = sigm64(a[..., 0]), sigm64(a[..., 1]), sigm64(a[..., 3]), np.tanh(a[..., 2])
    c = i * g
    h = o * np.tanh(c)
    d_i, d_f, d_o = d_sigm(a[..., 0], i), d_sigm(a[..., 1], f), d_sigm(a[..., 3], o)
    d_g = d_tanh(a[..., 2])
    d_c = d_i * np.abs(g) + i * d_g + ulp32(c) / 2
    d_h = d_o * np.abs(np.tanh(c)) + o * (d_tanh(c) + d_c) + ulp32(h) / 2
    gates = np.stack([i, f, g, o], axis=2)
    gb = np.stack([d_i, d_f, d_g, d_o], axis=2)
    B = a.shape[0]
    return dict(gates=gates.reshape(B, 256), gates_bound=gb.reshape(B, 256), c=c, c_bound=d_c, h=h, h_bound=d_h, z=a.reshape(B, 256))


def sweep_restated(xp, defect=None):
    """the kernel's step 0 in numpy float32: sigm(z) = 1 / (1 + exp(-z)), tanh_s(z) = 2 sigm(2 z) - 1, c = i g, h = o tanh_s(c).
    defect: "tanh_1e-6" adds 1e-6 to tanh_s, "swap_if" takes the f column for i and the i column for f"""
    one, two = np.float32(1.0), np.float32(2.0)

    def sg(z):
        with np.errstate(over="ignore"):
            return one / (one + np.exp(-z, dtype=np.float32))

    def th(z):
        return two * sg(two * z) - one + (np.float32(1e-6) if defect == "tanh_1e-6" else np.float32(0.0))
    a = np.asarray(xp[:, 0, :], dtype=np.float32).reshape(-1, H, 4)
    qi, qf = (1, 0) if defect == "swap_if" else (0, 1)
    i, f, g, o = sg(a[..., qi]), sg(a[..., qf]), th(a[..., 2]), sg(a[..., 3])
    c = i * g
    h = o * th(c)
    return dict(gates=np.stack([i, f, g, o], axis=2).reshape(-1, 256), c=c, h=h)


# --------------------------------------------------------------------------------------------------- B. the recurrence: cases
# ops._lstm_fwd / _lstm_bwd choose the launch by T.  4: the only length on wm_lstm_xproj + wm_lstm_fwd by default; 8: the shortest
# wm_lstm_fwd_fused; 12, 28: less than one 32-step chunk, ragged 16-step groups; 32: a multiple of 32 below the wave-specialised BPTT's
# threshold; 60: the last length below it; 64: the first on it; 68: past it and no multiple of 32.
ROUTE_T = (4, 8, 12, 28, 32, 60, 64, 68)
ROUTE_B = (1, 3)
SAVED_T = (8, 36, 64)                            # the saved gates / cst of every forward entry point, through the C ABI
SATURATED = ((2, 36), (1, 96))
SATURATED_SEED = {(2, 36): 0, (1, 96): 0}        # of the weights; tests/test_lstm_yardstick_cpu.py asserts what the case claims
ZERO_X = (2, 36)
ALL_ZERO = (2, 36)
LAUNCHES = ("wm_lstm_xproj", "wm_lstm_fwd", "wm_lstm_fwd_fused", "wm_lstm_fwd_tail", "wm_lstm_bwd", "wm_lstm_bwd_fused", "wm_lstm_bwd_wgrad",
            "wm_lstm_bwd_wgrad_dx", "wm_lstm_dx", "wm_lstm_wgrad")


def expected_launches(T):
    """{entry point: calls} of one ops.LSTMFn forward + backward at the default switches"""
    fwd = ("wm_lstm_xproj", "wm_lstm_fwd") if T < 8 else ("wm_lstm_fwd_fused",)
    bwd = ("wm_lstm_bwd_wgrad", "wm_lstm_dx") if T % 32 == 0 and T >= 64 else ("wm_lstm_bwd", "wm_lstm_dx", "wm_lstm_wgrad")
    return {n: 1 for n in fwd + bwd}


def lstm_inputs(kind, B, T):
    """(x [B, 64, T], W_ih, W_hh [256, 64], b_ih, b_hh [256], dh [B, 64, T]) float32.
    "route": weights and biases uniform +-1/8, unit-variance x -- every gate in the linear part of its function, as test_gpu_parity.py's.
    "saturated": W uniform +-1, biases uniform +-4 with the forget gate's b_ih shifted by +4, x scaled by 3: pre-activations of
    several tens, cells that keep their state over the whole clip.  "zero_x": the route weights, x = 0.  "all_zero": x, weights and biases
    0: every sigm is 0.5 and every tanh_s 0, so h = 0 exactly, and so are dx, dW_ih and dW_hh; the biases' gradient is not (the g gate's
    da = dc i (1 - g^2) = dc / 2)."""
    if kind == "saturated":
        seed = 900 + 10 * SATURATED_SEED[(B, T)] + T
        wi, wh = uniform(256, 64, seed=seed), uniform(256, 64, seed=seed + 1)
        bi, bh = uniform(256, seed=seed + 2, scale=4.0), uniform(256, seed=seed + 3, scale=4.0)
        bi[H:2 * H] += 4.0
        x = rnd(B, 64, T, seed=seed + 4, scale=3.0)
    else:
        seed = 800 + 7 * B + T
        wi, wh = uniform(256, 64, seed=seed, scale=0.125), uniform(256, 64, seed=seed + 1, scale=0.125)
        bi, bh = uniform(256, seed=seed + 2, scale=0.125), uniform(256, seed=seed + 3, scale=0.125)
        x = rnd(B, 64, T, seed=seed + 4) if kind == "route" else torch.zeros(B, 64, T)
        if kind == "all_zero":
            wi, wh, bi, bh = (torch.zeros_like(t) for t in (wi, wh, bi, bh))
    return x, wi, wh, bi, bh, rnd(B, 64, T, seed=seed + 5)


def lstm_trace(x_bt, w_ih, w_hh, b_ih, b_hh, defect=None):
    """oracle.wm_oracle.lstm_forward, statement for statement, that also returns what the kernels save:
    (h [B, T, 64], gate activations [B, T, 256] with column unit * 4 + gate, cell states [B, T, 64]).
    defect (for the restatement): "swap_if" exchanges the i and f gates, "tanh_1e-6" adds 1e-6 to both tanh"""
    B, T, _ = x_bt.shape
    off = 1e-6 if defect == "tanh_1e-6" else 0.0
    xp = x_bt @ w_ih.t() + (b_ih + b_hh)
    h = x_bt.new_zeros(B, H)
    c = x_bt.new_zeros(B, H)
    whh_t = w_hh.t()
    outs, acts, cells = [], [], []
    for t in range(T):
        a = xp[:, t] + h @ whh_t
        i, f, g, o = a.split(H, dim=1)
        if defect == "swap_if":
            i, f = f, i
        if defect is None:
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
        else:
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * (torch.tanh(g) + off)
            h = torch.sigmoid(o) * (torch.tanh(c) + off)
        outs.append(h)
        acts.append(torch.stack([torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g) + off, torch.sigmoid(o)], dim=2).reshape(B, 4 * H))
        cells.append(c)
    return torch.stack(outs, dim=1), torch.stack(acts, dim=1).detach(), torch.stack(cells, dim=1).detach()


def _run(inputs, dtype, defect=None):
    x, wi, wh, bi, bh, gg = (t.to(dtype) for t in inputs)
    leaves = [t.clone().requires_grad_() for t in (x, wi, wh, bi, bh)]
    if defect is None:
        h = O.lstm_forward(leaves[0].permute(0, 2, 1), *leaves[1:]).permute(0, 2, 1)
        with torch.no_grad():
            _, gates, cst = lstm_trace(x.permute(0, 2, 1), wi, wh, bi, bh)
    else:
        h, gates, cst = lstm_trace(leaves[0].permute(0, 2, 1), *leaves[1:], defect=defect)
        h = h.permute(0, 2, 1)
    h.backward(gg)
    out = dict(h=h.detach(), gates=gates, cst=cst)
    out.update({n: t.grad for n, t in zip(GRAD_NAMES, leaves)})
    return out


@functools.lru_cache(maxsize=None)
def lstm_ref(kind, B, T):
    """(float64 reference, float32 reference) of a case: dicts of h [B, 64, T], gates, cst and the five gradients.  Computed once per
    case and shared; nobody writes to them."""
    inputs = lstm_inputs(kind, B, T)
    return _run(inputs, torch.float64), _run(inputs, torch.float32)


def lstm_defect(kind, B, T, defect):
    """the float32 run with a planted defect"""
    return _run(lstm_inputs(kind, B, T), torch.float32, defect)


def floor_of(name):
    return FWD_FLOOR if name in ("h", "gates", "cst") else GRAD_FLOOR


def saturation_share(gates64):
    """the share of gate activations outside [0.01, 0.99] (the g column: |tanh| > 0.98, the same distance from its ends)"""
    a = gates64.reshape(-1, H, 4)
    sig = a[..., [0, 1, 3]]
    out = ((sig < 0.01) | (sig > 0.99)).sum() + (a[..., 2].abs() > 0.98).sum()
    return float(out) / a.numel()
