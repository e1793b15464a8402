"""The step recipe of the reference's hot loop (train_one_epoch / validate_one_epoch / evaluate_model,
py/main16.py:238-278, :312-347, :377-403), expressed over the HIP modules.  Host glue only."""
from __future__ import annotations

from collections import OrderedDict

import torch

from . import losses as L, ops
from .masking import MaskingLoss

# py/main16.py:38-43
LOSS_WEIGHTS = OrderedDict(l1=1.0, mel=4.0, loud=20.0, loc=10.0, bce=1.0, hf=5.0)

_mel = L.MultiScaleMelLoss()
_loud = L.TFLoudnessLoss()
_mask = MaskingLoss()


def forward_losses(generator, detector, s, message, codec=None, tamper=None, masking=None):
    """delta -> post-processing -> detector on cat([s_w, s]) -> the six loss terms and both totals.
    `codec` (a codec.PcmCodec): the main15c graph -- s_w = codec(s + delta) is what the Detector, mel and loudness see.
    `tamper` (an attacks.Splice): the Detector sees cat([s_t, s]) with s_t, labels = tamper(s_w, s) -- the splice comes last, behind any
    codec -- and loc / bce are taken against the per-sample labels (losses.detection_losses_masked) behind the plain
    detector(x, input_grad_rows=B): the fused Detector tail hard-codes "row < B => 1" and is not used.  Mel, loudness, l1 and hf see the
    unspliced signals exactly as without it; `out` gains "labels" and "s_t".  None: the call as it was.
    `masking` (a float, the weight): a seventh term, out["mask"] = masking.MaskingLoss()(s, s_w) -- the mean number of dB by which
    s_w - s is above the masking threshold of s, s_w taken behind any codec like mel and loudness -- and total += masking * mask.
    raw_total and LOSS_WEIGHTS are as they were.  None: the call as it was, bit for bit."""
    B = s.shape[0]
    delta_raw = generator(s, message)                                  # :244
    delta = L.postprocess(delta_raw)                                   # :245-247
    s_w = s + delta                                                    # :248
    if codec is not None:
        s_w = codec(s_w)                                               # main15c: perceptual_postprocess(s + delta)
    if tamper is None:
        logits, loc, bce = L.detect_with_losses(detector, torch.cat([s_w, s], dim=0), message, input_grad_rows=s.shape[0])   # :249-264
    else:
        s_t, labels = tamper(s_w, s)
        logits = detector(torch.cat([s_t, s], dim=0), input_grad_rows=s.shape[0])
        loc, bce = L.detection_losses_masked(logits, message, labels)
    l1 = L.l1_to_zero(delta)                                           # :266
    mel = _mel(s, s_w)                                                 # :267
    loud = _loud(s, s_w)                                               # :268
    hf = L.high_freq_penalty(delta)                                    # :271
    raw = l1 + mel + loud + loc + bce                                  # :273
    w = LOSS_WEIGHTS
    total = w["l1"] * l1 + w["mel"] * mel + w["loud"] * loud + w["loc"] * loc + w["bce"] * bce + w["hf"] * hf   # :275-276
    out = OrderedDict(delta_raw=delta_raw, delta=delta, s_w=s_w, logits=logits, l1=l1, mel=mel, loud=loud, loc=loc,
                      bce=bce, hf=hf, raw_total=raw, total=total)
    if tamper is not None:
        out["labels"], out["s_t"] = labels, s_t
    if masking is not None:
        out["mask"] = _mask(s, s_w)
        total = total + float(masking) * out["mask"]
        out["total"] = total
    return total, out


def _train_step(forward_losses, generator, detector, optimizer, s, message, grad_sync, codec=None, tamper=None, masking=None):
    """the step around a model family's forward_losses: zero_grad, forward, backward, gradient sync, message-id check, update.
    `codec`, `tamper` and `masking` are handed to forward_losses only when given (a family without them keeps its signature)."""
    extra = {} if codec is None else {"codec": codec}
    if tamper is not None:
        extra["tamper"] = tamper
    if masking is not None:
        extra["masking"] = masking
    optimizer.zero_grad(set_to_none=not hasattr(optimizer, "flat"))
    if hasattr(grad_sync, "begin_step"):
        grad_sync.begin_step()
    try:
        with ops.index_check_mode():
            total, out = forward_losses(generator, detector, s, message, **extra)   # no mid-step sync for the message-id range check ...
        total.backward()
        if hasattr(optimizer, "finish_backward"):
            optimizer.finish_backward()
        if grad_sync is not None:
            grad_sync()
        # ... its flag (copied to pinned memory right after the lookup) has landed long before backward returns: read it here, so
        # that a bad id raises BEFORE the update, as nn.Embedding's IndexError does (py/main16.py:158), never one step late
        ops.check_message_ids(wait=True, what="this train_step's batch")
    except BaseException:
        ops.drop_pending_message_checks()        # a step that died half-way must not report its flag inside a later, valid step
        raise
    optimizer.step()
    return out


def train_step(generator, detector, optimizer, s, message, grad_sync=None, codec=None, tamper=None, masking=None):
    """One iteration of train_one_epoch's loop body (:242-278): zero_grad, forward, backward, optimizer step.
    `grad_sync` (optional callable) runs between backward and the update -- the data-parallel all-reduce.
    `codec` (a codec.PcmCodec): main15c's step, see forward_losses.  `tamper` (an attacks.Splice): the splice attack with per-sample
    labels, see forward_losses.  `masking` (a float): the weight of the masking loss as a seventh term, see forward_losses."""
    return _train_step(forward_losses, generator, detector, optimizer, s, message, grad_sync, codec, tamper, masking)


def _eval_reductions(logits, message, delta):
    """evaluate_model's per-clip reductions (:386-403) of the Detector's logits on cat([watermarked, clean]) (2B rows)"""
    B = delta.shape[0]
    probs = torch.sigmoid(logits[:, :, 0]).mean(dim=1)
    decoded = (torch.sigmoid(logits[:B, :, 1:]) > 0.5).float().mean(dim=1) > 0.5
    bits = ((message.unsqueeze(1) & (1 << torch.arange(logits.shape[-1] - 1, device=logits.device))) > 0)
    return OrderedDict(delta=delta, logits=logits, prob_watermarked=probs[:B], prob_clean=probs[B:],
                       bit_accuracy=(decoded == bits).float().mean(dim=1), delta_rms=torch.sqrt((delta ** 2).mean(dim=[1, 2])))


@torch.no_grad()
def eval_forward(generator, detector, s, message, codec=None, tamper=None):
    """evaluate_model's per-batch quantities (:383-403).  In eval mode BatchNorm uses running statistics, so the Detector's
    rows are independent: the clean half D(s) does not wait for the Generator -- it is queued for the side stream and released
    when the Generator reaches its latency-bound LSTM (B clips keep only B of the 256 CUs busy there), and the two halves are
    concatenated afterwards (bit-identical to the single 2B-row call).
    `codec` (a codec.PcmCodec): the Detector sees codec(s + delta), as in main15c's validate_one_epoch, on both branches; the processed
    signal is returned as "s_w".
    `tamper` (an attacks.Splice): the Detector's watermarked half is s_t, labels = tamper(s_w, s), the splice behind any codec; the
    reductions are the same, and "labels" and "s_t" are returned as well."""
    overlap = (not generator.training) and (not detector.training) and s.is_cuda
    box = {}
    if overlap:
        def clean_half():
            box["lg"] = detector(s)
        ops._on_side((s,), clean_half)                # queued: released on the side stream when the LSTM launch is reached
    delta = L.postprocess(generator(s, message))
    s_w = s + delta if codec is None else codec(s + delta)
    if tamper is not None:
        s_t, labels = tamper(s_w, s)
    else:
        s_t = s_w
    if overlap:
        lg_wm = detector(s_t)
        ops.join_side_stream()                        # (also releases the queue if the Generator had no LSTM call)
        box["lg"].record_stream(torch.cuda.current_stream())
        logits = torch.cat([lg_wm, box["lg"]], dim=0)
    else:
        logits = detector(torch.cat([s_t, s], dim=0))
    out = _eval_reductions(logits, message, delta)
    if codec is not None:
        out["s_w"] = s_w
    if tamper is not None:
        out["labels"], out["s_t"] = labels, s_t
    return out
