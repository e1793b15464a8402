"""Drop-in nn.Module mirrors of the reference's hot-path classes (py/main16.py:112-186).

Same class names, constructor signatures, sub-module names and state_dict layout (SURVEY.md
appendix A), so checkpoints, optimizers and callers of the reference keep working; the
forward/backward arithmetic is the HIP path in ops.py.  The torch.nn layers created in
__init__ are used as *parameter containers only* (this also reproduces the reference's
default initialisation bit-for-bit under the same seed) -- their own forward is never run.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops


class ResBlock(nn.Module):
    """py/main16.py:112-125."""

    def __init__(self, ch):
        super().__init__()
        if ch != 64:
            raise ValueError("the MI355X hot path is built for the reference's 64-channel ResBlock")
        self.block = nn.Sequential(
            nn.Conv1d(ch, ch, 3, padding=1),
            nn.BatchNorm1d(ch),
            nn.ReLU(),
            nn.Conv1d(ch, ch, 3, padding=1),
            nn.BatchNorm1d(ch),
        )
        self.relu = nn.ReLU()

    def forward(self, x):
        return ops.ResBlockFn.apply(x, *_rb_args(self), self.training)


def _rb_args(m):
    c1, n1, _, c2, n2 = m.block
    return ops.BlockParams(c1.weight, c1.bias, n1.weight, n1.bias, c2.weight, c2.bias, n2.weight, n2.bias,
                           n1.running_mean, n1.running_var, n1.num_batches_tracked, n2.running_mean, n2.running_var, n2.num_batches_tracked)


def _hooked(*modules):
    return any(m._forward_hooks or m._forward_pre_hooks for m in modules)


def resblock_pair(m1, m2, x):
    """m2(m1(x)) for two ResBlocks in a row (py/main16.py:135-136, :178-179).  In a training step on the fused path the pair is
    ONE tape node (ops.ResBlockPairFn: the second block's backward also does the first block's ReLU backward and BatchNorm sums);
    otherwise -- inference, no gradients wanted, odd clip lengths, any of the knobs off, forward hooks on the blocks -- two calls."""
    if m1.training and m2.training and not _hooked(m1, m2) and ops.pair_node_applies(x):
        return ops.ResBlockPairFn.apply(x, *_rb_args(m1), *_rb_args(m2), True)
    return m2(m1(x))


class _Stem(nn.Conv1d):
    def forward(self, x, grad_rows=None):
        return ops.StemFn.apply(x, self.weight, self.bias, grad_rows)


class _Head1(nn.Conv1d):
    def forward(self, x):
        return ops.Head1Fn.apply(x, self.weight, self.bias)


class Generator(nn.Module):
    """Encoder -> LSTM -> (+ message embedding) -> decoder, py/main16.py:128-162."""

    def __init__(self, message_bits=0):
        super().__init__()
        self.message_bits = message_bits
        self.encoder = nn.Sequential(_Stem(1, 64, 7, padding=3), ResBlock(64), ResBlock(64))
        self.lstm = nn.LSTM(64, 64, batch_first=True)
        if message_bits > 0:
            self.embedding = nn.Embedding(2 ** message_bits, 64)
        self.decoder = nn.Sequential(nn.ConvTranspose1d(64, 64, 7, padding=3), ResBlock(64), _Head1(64, 1, 1))

    def forward(self, s, message=None):
        stem, e1, e2 = self.encoder
        lstm = (self.lstm.weight_ih_l0, self.lstm.weight_hh_l0, self.lstm.bias_ih_l0, self.lstm.bias_hh_l0)
        fold = e1.training and e2.training and not _hooked(self.encoder, e1, e2, self.lstm)
        if fold and not _hooked(stem) and ops.stem_in_conv1_applies(s, lstm=True):
            # the stem's output is formed by encoder.1's conv1 launch; both tails ride in the kernels that read them next
            x = ops.StemEncoderLSTMFn.apply(s, stem.weight, stem.bias, *_rb_args(e1), *_rb_args(e2), *lstm)
        else:
            x = stem(s)                                                          # (B,64,T)
            if fold and ops.tail_in_consumer_applies(x, lstm=True):
                x = ops.EncoderLSTMFn.apply(x, *_rb_args(e1), *_rb_args(e2), *lstm)  # both tails ride in the kernels that read them next
            else:
                x = ops.LSTMFn.apply(resblock_pair(e1, e2, x), *lstm)
        vec = None
        if self.message_bits > 0 and message is not None:
            if message.dim() != 1 or message.shape[0] != s.shape[0]:
                raise ValueError(f"message must have shape ({s.shape[0]},), got {tuple(message.shape)}")
            vec = ops.EmbedFn.apply(self.embedding.weight, message.to(torch.int64))
        ct = self.decoder[0]
        x = ops.ConvT7Fn.apply(x, vec, ct.weight, ct.bias)
        rb, head = self.decoder[1], self.decoder[2]
        if rb.training and not _hooked(rb, head) and ops.tail_in_head_applies(x):
            return ops.ResBlockHead1Fn.apply(x, *_rb_args(rb), head.weight, head.bias)   # the block's tail rides in the head's kernel
        return head(rb(x))                                                      # delta (B,1,T)


class _HeadN(nn.Conv1d):
    def forward(self, x):
        return ops.HeadNFn.apply(x, self.weight, self.bias)


class Detector(nn.Module):
    """Sample-level logits (B,T,1+bits), py/main16.py:170-186."""

    def __init__(self, message_bits=0):
        super().__init__()
        self.message_bits = message_bits
        output_dim = 1 + message_bits
        self.model = nn.Sequential(_Stem(1, 64, kernel_size=7, padding=3), ResBlock(64), ResBlock(64),
                                   _HeadN(64, output_dim, kernel_size=1))

    def forward(self, x, input_grad_rows=None):
        """`input_grad_rows` (optional, not in the reference): only clips [0, input_grad_rows) get an input gradient --
        the train step feeds [watermarked; clean] (py/main16.py:249) and the clean half is data."""
        stem, m1, m2, head = self.model
        if m1.training and m2.training and not _hooked(stem, m1, m2) and ops.stem_in_conv1_applies(x):
            # the stem's output is formed by model.1's conv1 launch
            return head(ops.StemResBlockPairFn.apply(x, stem.weight, stem.bias, input_grad_rows, *_rb_args(m1), *_rb_args(m2), True))
        x = stem(x) if input_grad_rows is None else stem(x, input_grad_rows)
        return head(resblock_pair(m1, m2, x))

    def forward_with_losses(self, x, message, input_grad_rows=None):
        """(logits, loc, bce) = (self(x), *detection_losses(self(x), message)) as one tape node behind the stem (ops.DetectorTailFn), or
        None where that node does not apply: then the caller takes the two calls.  It applies in a training step on the fused path
        (resblock_pair's conditions), with no forward hooks from model.1 to the Detector itself and x = [watermarked; clean]."""
        m1, m2, head = self.model[1], self.model[2], self.model[3]
        ok = (m1.training and m2.training and not _hooked(self, self.model, m1, m2, head) and ops.tail_in_head_applies(x)
              and ops.pair_node_applies(x) and 1 <= head.weight.shape[0] <= 64 and isinstance(message, torch.Tensor) and message.is_cuda
              and message.dtype == torch.int64 and message.dim() == 1 and x.shape[0] == 2 * message.shape[0])
        if not ok:
            return None
        stem = self.model[0]
        if not _hooked(stem) and ops.stem_in_conv1_applies(x):                  # the stem's output is formed by model.1's conv1 launch
            return ops.StemDetectorTailFn.apply(x, stem.weight, stem.bias, input_grad_rows, message.contiguous(), *_rb_args(m1),
                                                *_rb_args(m2), head.weight, head.bias)
        x = stem(x) if input_grad_rows is None else stem(x, input_grad_rows)
        return ops.DetectorTailFn.apply(x, message.contiguous(), *_rb_args(m1), *_rb_args(m2), head.weight, head.bias)


def load_state_dict_strip_prefix(model, state_dict, prefix="_orig_mod."):
    """py/main16.py:707-712: accept checkpoints saved from torch.compile-wrapped models."""
    cleaned = {(k[len(prefix):] if k.startswith(prefix) else k): v for k, v in state_dict.items()}
    return model.load_state_dict(cleaned, strict=False)
