"""Spatial-reduction attention (sr_ratio > 1) restated on top of the CPU oracle (TEST INFRASTRUCTURE ONLY).

``oracle/segmm_oracle.py`` states the reference's path with ``sr_ratio = 1``.  This file adds the one thing a reduced layer changes
(reference encoder.py:23-31,84-102) -- in the form the engine computes it, so that the restatement is checked against the real
reference's fixtures (tests/golden/sr, tools/gen_golden_sr.py) and the engine against the restatement:

  p = (r - 1) // 2,  Ls = S // r  (must equal the conv length (S + 2p - r) // r + 1, and be >= 1)
  pack    A[b Ls + j, c r + t] = x[b, j r - p + t, c]  if 0 <= j r - p + t < S else 0        (masked tokens are NOT zeroed)
  reduce  Xsr = A . W2^T + bias,  W2 = cross_attn.sr.weight.view(d, r d)                     (the Conv1d, kernel_size == stride)
  mask    m_sr[b, j] = OR_{t < r} m[b, j r + t]                                              (NOT shifted by p)
  the key / value projections that read video tokens read Xsr; the queries read x; user side unchanged
  unpack  G[b, i, c] = res[b, i, c] + dA[b Ls + (i + p) // r, c r + (i + p) % r]  if (i + p) // r < Ls else res[b, i, c]

``pack_np`` / ``unpack_np`` / ``mask_pool_np`` are the numpy statements the kernels are compared with bit for bit; ``pack`` is the
differentiable torch form the model functions use.  ``reduced(sr)`` swaps the oracle's ``encoder_layer`` for the reduced one while
its ``model_forward`` / ``forward_backward`` / ``train_steps`` run, so everything around the layer stays the oracle's."""
import contextlib
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

from helpers import ROOT

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import segmm_oracle as O  # noqa: E402


def sr_len(S, r):
    """Ls, or ValueError where the conv length and the mask-pool length differ (the reference raises IndexError there)."""
    p = (r - 1) // 2
    Lc, Lm = (S + 2 * p - r) // r + 1 if S + 2 * p >= r else 0, S // r
    if Lc != Lm or Lm < 1:
        raise ValueError("S=%d, r=%d: conv length %d != mask-pool length %d" % (S, r, Lc, Lm))
    return Lm


# ------------------------------------------------------------------------------------------------ numpy statements of the kernels
def pack_np(x, r):
    """x [B, S, d] -> A [B Ls, r d]."""
    B, S, d = x.shape
    Ls, p = sr_len(S, r), (r - 1) // 2
    A = np.zeros((B, Ls, d, r), dtype=x.dtype)
    for j in range(Ls):
        for t in range(r):
            i = j * r - p + t
            if 0 <= i < S:
                A[:, j, :, t] = x[:, i, :]
    return A.reshape(B * Ls, d * r)


def unpack_np(dA, res, B, S, d, r):
    """dA [B Ls, r d], res [B, S, d] or None -> G [B, S, d]: one fp32 add per element (a copy where ``res`` is None)."""
    Ls, p = sr_len(S, r), (r - 1) // 2
    dA = dA.reshape(B, Ls, d, r)
    G = np.zeros((B, S, d), dtype=dA.dtype) if res is None else res.copy()
    for i in range(S):
        j, t = (i + p) // r, (i + p) % r
        if j < Ls:
            G[:, i, :] = dA[:, j, :, t] if res is None else res[:, i, :] + dA[:, j, :, t]
    return G


def mask_pool_np(m, r):
    """m [B, S] bool -> [B, Ls] bool: max_pool1d(kernel = stride = r), no padding."""
    B, S = m.shape
    Ls = sr_len(S, r)
    return m[:, :Ls * r].reshape(B, Ls, r).any(-1)


# ------------------------------------------------------------------------------------------------ the layer, on the oracle
def pack(x, r):
    """``pack_np`` in differentiable torch: x [B, S, d] -> [B, Ls, r d]."""
    B, S, d = x.shape
    Ls, p = sr_len(S, r), (r - 1) // 2
    xp = torch.cat([x.new_zeros(B, p, d), x, x.new_zeros(B, r, d)], 1)          # xp[:, i + p] = x[:, i]; zeros outside
    idx = (torch.arange(Ls)[:, None] * r + torch.arange(r)[None, :]).reshape(-1)          # (j r - p + t) + p
    return xp[:, idx].reshape(B, Ls, r, d).permute(0, 1, 3, 2).reshape(B, Ls, d * r)


def reduce_keys(sd, pre, vid, vid_mask, r):
    """(Xsr [B, Ls, d], m_sr [B, Ls]) of the attention block ``pre`` (``...cross_attn``)."""
    d = vid.shape[-1]
    W2 = sd[pre + ".sr.weight"].reshape(d, d * r)
    xsr = pack(vid, r) @ W2.t() + sd[pre + ".sr.bias"]
    m_sr = vid_mask[:, :sr_len(vid.shape[1], r) * r].reshape(vid.shape[0], -1, r).any(-1)
    return xsr, m_sr


def cross_attention(sd, pre, vid, vid_mask, usr, usr_mask, nhead, need_usr=True, drop=None, mode="joint", r=1):
    """``segmm_oracle.cross_attention`` with the video KEYS of a reduced layer: every key / value projection that reads video tokens
    reads (Xsr, m_sr); queries, the user side and the dropout call order are the oracle's."""
    if r == 1:
        return O.cross_attention(sd, pre, vid, vid_mask, usr, usr_mask, nhead, need_usr, drop, mode)
    B, Lv, d = vid.shape
    Lt = usr.shape[1]
    dh = d // nhead
    do = drop if drop is not None else (lambda t: t)
    _lin, _ln, attn_logits = O._lin, O._ln, O.attn_logits
    ksr, msr = reduce_keys(sd, pre, vid, vid_mask, r)
    vals, logits = [], []
    if mode != "cross":
        vals.append(_lin(sd, pre + ".v2v_proj.2", ksr))
        logits.append(attn_logits(sd, pre + ".v2v_proj", ksr, msr, vid, vid_mask, nhead))
    if mode != "self":
        vals.append(_lin(sd, pre + ".t2v_proj.2", usr))
        logits.append(attn_logits(sd, pre + ".t2v_proj", usr, usr_mask, vid, vid_mask, nhead))
    v_val = torch.cat(vals, 1)
    v_val = v_val.view(B, v_val.shape[1], nhead, dh)
    v_logits = do(torch.cat(logits, -1)) / math.sqrt(dh)
    if need_usr:
        if mode == "self":
            vals = [_lin(sd, pre + ".t2t_proj.2", usr)]
            logits = [attn_logits(sd, pre + ".t2t_proj", usr, usr_mask, usr, usr_mask, nhead)]
        else:
            vals = [_lin(sd, pre + ".v2t_proj.2", ksr)]
            logits = [attn_logits(sd, pre + ".v2t_proj", ksr, msr, usr, usr_mask, nhead)]
            if mode == "joint":
                vals.append(_lin(sd, pre + ".t2t_proj.2", usr))
                logits.append(attn_logits(sd, pre + ".t2t_proj", usr, usr_mask, usr, usr_mask, nhead))
        t_val = torch.cat(vals, 1)
        t_val = t_val.view(B, t_val.shape[1], nhead, dh)
        t_logits = do(torch.cat(logits, -1)) / math.sqrt(dh)
    vid_ = torch.einsum("bhqk,bkhd->bqhd", F.softmax(v_logits, -1), v_val).reshape(B, Lv, d)
    usr_out = None
    if need_usr:
        usr_ = torch.einsum("bhqk,bkhd->bqhd", F.softmax(t_logits, -1), t_val).reshape(B, Lt, d)
        usr_ = do(_lin(sd, pre + ".ff_usr", usr_))
        if mode != "self":
            usr_out = _ln(sd, pre + ".ln_usr", usr + usr_)
    vid_ = do(_lin(sd, pre + ".ff_vid", vid_))
    return _ln(sd, pre + ".ln_vid", vid + vid_), usr_out


def encoder_layer(sd, pre, usr, usr_mask, vid, vid_mask, nhead, need_usr=True, drop=None, mode="joint", r=1):
    """``segmm_oracle.encoder_layer`` around the reduced attention block."""
    do = drop if drop is not None else (lambda t: t)
    vid, usr_new = cross_attention(sd, pre + ".cross_attn", vid, vid_mask, usr, usr_mask, nhead, need_usr, drop, mode, r)
    vid = O._ln(sd, pre + ".ln_vid", vid + do(O.mlp_gelu(sd, pre + ".ff_vid", vid, drop)))
    if usr_new is not None:
        usr_new = O._ln(sd, pre + ".ln_usr", usr_new + do(O.mlp_gelu(sd, pre + ".ff_usr", usr_new, drop)))
    return vid, usr_new


@contextlib.contextmanager
def reduced(sr):
    """While open, the oracle's backbone runs layer i with ratio ``sr[i]`` (the layer index is the tail of its state-dict prefix)."""
    orig = O.encoder_layer

    def layer(sd, pre, usr, usr_mask, vid, vid_mask, nhead, need_usr=True, drop=None, mode="joint"):
        return encoder_layer(sd, pre, usr, usr_mask, vid, vid_mask, nhead, need_usr, drop, mode, r=int(sr[int(pre.rsplit(".", 1)[1])]))
    O.encoder_layer = layer
    try:
        yield
    finally:
        O.encoder_layer = orig


def model_forward(sd, cfg, inp, *a, **k):
    with reduced(cfg["sr"]):
        return O.model_forward(sd, cfg, inp, *a, **k)


def forward_backward(sd, cfg, inp, *a, **k):
    with reduced(cfg["sr"]):
        return O.forward_backward(sd, cfg, inp, *a, **k)


def train_steps(sd, cfg, inp, n_steps, *a, **k):
    with reduced(cfg["sr"]):
        return O.train_steps(sd, cfg, inp, n_steps, *a, **k)
