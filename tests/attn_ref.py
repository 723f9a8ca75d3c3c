"""The attention kernels (csrc/attention.h, attention16.h, attention_lds.h, attention_pl.h for head dims <= 64; attention_wide.h
for 96 and 128; attention_stream.h for every head dim: the last section), restated on the
host: a float64 statement of one side's forward and backward written from the definition in the header comment of
csrc/attention.h (no autograd, no kernel loops), a first-order error bound per output, the rule that says which kernel instance
serves a call (restated from capi.hip), fixed-seed inputs, an fp32 emulation in a fixed summation order and a list of planted
defects.  Shared by test_attn_ref_cpu.py (the yardstick shown sound without a GPU), test_attn_float64_gpu.py and
test_attn_wide_stream_float64_gpu.py.

The statement.  One side: two key blocks a, b, each with its own query projection, T = La + Lb real keys:
    raw    = [Qa Ka^T | Qb Kb^T]                     per (batch row, head)
    raw[~(mq (x) mk)] = -10000                       the fill
    logit  = raw * mult * scale                      mult: the dropout multiplier (0 or 1 / (1 - p)), fills included;
                                                     scale = 1 / sqrt(dh) as the fp32 number the kernels use
    m = max_k logit, inv = 1 / sum_k exp(logit - m), P = exp(logit - m) inv      over the REAL keys; a pad key has P = 0
    O = P [Va; Vb]           lse plane 0 = m, plane 1 = inv          D = rowsum(dO * O)
    dV = P^T dO    dP = dO V^T    dS = P o (dP - D)    dlogit = dS mult scale, 0 where the fill replaced the product
    dQa = dlogit_a Ka   dQb = dlogit_b Kb   dKa = dlogit_a^T Qa   dKb = dlogit_b^T Qb
The multipliers come in the kernels' own layout [B, H, Lq, La_p + Lb_p] (key blocks padded separately to multiples of 16).
A fill is a constant of the arithmetic, not a computed product: logit_xform (attention.h) demands that every kernel forms it
by the same two ROUNDED fp32 products, so it enters the statement as that fp32 value (``fill_logit``); everything else is float64.

Error bounds.  u = 2^-24.  A sum of n terms evaluated in fp32 along any tree whose longest chain of roundings is c has
|computed - exact| <= c u sum|terms| to first order (tests/rowops_ref.py).  Constants, each counted on the documented shape:

* a matrix-core product with reduction length n (v_mfma_f32_16x16x4_f32 chains, n / 4 instructions of 4 products; how an
  instruction orders its four adds is not documented, so the chain is taken as the longest possible): n adds and the rounding of
  the product:  c_dot(n) = n + 1.  Sums that continue across waves or key tiles in LDS (the fused backward's dQ) are chains over
  the same n terms and are covered by the same count.
* the fp16x3 and planes-in forms replace an fp32 operand x by hi + lo under a power-of-two scale s (tests/p32_ref.py):
  |hi + lo - x s| <= REL |x s| + ABS, and drop the lo lo partial product (<= 2^-22 |a b|: both lo terms are below 2^-11 of their
  operands).  Per product:  (n_split REL + 2^-22) sum|a b|  +  for every operand split inside the kernel  ABS / s sum|other|, with
  1 / s <= 2^-14 A, A an upper bound of the operand's magnitude (the tensor maximum for Q, K, V, dO; 1 for P, whose scale is
  the fixed 2^14; the kernels' own bound (dh max|dO| max|V| + max|D|) max(mult) scale for dS, attention16.h).  n_split counts the
  operands the kernel splits itself: both in the fp16x3 form; in the planes-in forms Q, K and V are the planes' own values
  (the statement is evaluated on hi + lo under the site scale), so only dO, P and dS count.
* logit:  eps_s = (err_prod(Q, K) + 2 u |raw|) mult scale: the two rounded products of logit_xform.  A fill has eps_s = 0 for the
  probabilities (see above; checked: a fill is either dropped -- logit exactly 0 --, has probability exactly 0, or sits in a row of
  equal logits, which is uniform whatever the value) and 2 u |fill logit| for the row maximum, which the float64 statement forms from the exact product.
* exp(x), x = logit - m <= 0, as exp2(x log2e):  the subtraction, the product and the fp32 constant log2e each move the
  argument by u |x|, the instruction is good to one ulp = 2 u:  (3 |x| + 2) u relative.
* probability, forward:  rho_k = eps_k + (3 |x_k| + 2) u + N,  N = sum_j p_j (eps_j + (3 |x_j| + 2) u) + (T + 3) u  the normaliser:
  the terms' own errors weighted by their share, a T-term sum (chain <= T), the division, the product e inv.  The row maximum
  cancels between numerator and denominator: both use the same computed number.  With the key tiles split over wave groups
  (staged forward, KSPLIT > 1) the groups' sums are rescaled by exp(m_group - m) and added: a second exp (its argument error is
  already inside 3 |x_k|: |l_k - m_g| + |m_g - m| = |x_k|), two more products, the groups' adds: + 8 u.
  backward: the kernels recompute exp(logit - m) from the SAVED m and inv:  rho_k = eps_k(backward form) + (3 |x_k| + 3) u + N(forward form).
* row statistics:  m: max of eps over the keys that can be the maximum;  inv: N + err(m) relative (the statement's sum is taken
  around the exact m, the kernel's around its own).
* O = P V:  sum_k p_k |v_k| (rho_k + c_dot(T) u) + the split terms.     D: (dh + 1) u sum|dO O| + sum|dO| bound(O of the forward form).
* dV = P^T dO:  sum_q p |dO| (rho + c_dot(Lq) u) + split terms.
* dS = p (dP - D):  p (err(dP) + err(D)) + rho p |dP - D| + 2 u |dS|  (the subtraction and the product), err(dP) = err_prod(dO, V).
  dlogit = dS mult scale: the kernels multiply by fac = mult scale formed once (1 rounding) in two products: + 3 u |dlogit|.
* dQ = dlogit K:  sum_k err(dlogit_k) |K_k| + c_dot(T_block) u sum_k |dlogit_k K_k| + split terms;  dK the same over the queries.
  The cancellation in dP - D is carried by err(dS), not by a constant.

Wide heads and the streamed kernels (csrc/attention_wide.h, attention_stream.h).  The statement above is the statement of every
built head dim (4 .. 128) and of the streamed kernels too; what follows extends its reach, not the statement.
* the direct forward, D, dQ and dK/dV instances at head dims 96 and 128 are the kernels of attention.h with more registers: the
  held-forward constants above hold as they stand (c_dot(dh) has dh = 96 | 128).
* streamed forward (online softmax over nt = Tp / 16 <= 32 key tiles; ``bounds_fwd(stream=nt)``).  Key k of tile t is evaluated as
  e_k = exp(logit_k - m_t') and then multiplied by every later rescale a_s = exp(m_(s-1) - m_s), s = t + 1 .. nt - 1.
  - arguments: every one is a difference of two COMPUTED logits, all <= 0, and the running maximum is monotone, so the magnitudes
    telescope: |logit_k - m_t'| + sum_s |m_(s-1) - m_s| = |x_k|.  The three argument roundings per exp therefore still sum to
    3 |x_k| u; what grows is the number of exp instructions on the path, one ulp (2 u) each: at most nt of them (its own and at
    most nt - 1 rescales; the first tile's a is the constant 0, not an exp):  ex_k = (3 |x_k| + 2 nt) u  instead of (3 |x_k| + 2) u.
  - the row sum: a lane adds its four keys of a tile (ts: 3 adds after the first term), then l = l a + ts (a product and an add,
    or one fused rounding), so the oldest term goes through 3 + 2 nt roundings; the two shuffles add 2; the division 1; the product
    O inv (it replaces e inv: the row is normalised after the product with V, not before) 1:
        N = sum_j p_j (eps_j + ex_j) + (2 nt + 7) u     instead of  ... + (T + 3) u.
    (The rescales multiply l and O by the same computed a, so their errors cancel in P; they are counted all the same, once in
    ex_k and once in the chain: the bound is an upper bound either way, and the planted 2^-11 defect stays 50 times above it.)
  - O: the accumulators are multiplied by a once per tile after the first, a rounding of the whole partial sum each:
        O:  sum_k p_k |v_k| (rho_k + c_dot(T) u) + (nt - 1) u sum_k p_k |v_k|.
    m is the largest computed logit, selected exactly: its bound does not move.  inv: N + err(m) as before.
* D.  attn_row_D (streamed dQ and attn_D_stream_kernel): a lane's dh / 4 products through a fused-multiply-add chain (dh / 4
  roundings), then two adds across the four lanes: dh / 4 + 2.  The wide fused kernel: a group of four products as
  (p0 + p1) + (p2 + p3) -- a product and two adds on the longest path: 3 -- then the dh / 4 partials in index order: dh / 4 + 3.
  attn_D_kernel: groups of four (<= 4 roundings) chained dh / 4 times.  All <= dh + 1 for dh >= 4: the (dh + 1) u term covers them.
* the wide fused backward takes a key block of more than 8 tiles in passes and carries a chunk's dQ partial sum from pass to
  pass through the fp32 dQ buffer.  A store and reload of an fp32 number is exact, and the sum continues where it stopped: the
  chain over the block's n keys stays within c_dot(n), like the narrow kernel's sums that continue across waves in LDS.
* a backward that consumes a STREAMED forward's O and lse (the streamed dQ, the dK/dV kernel above 192 padded keys, the fused
  backward behind a streamed forward) takes N and the bound of O from ``bounds_fwd(stream=nt)``: ``bounds_bwd`` takes the
  forward's bounds as an argument.
"""
import numpy as np

import p32_ref as P32

U = 2.0 ** -24
F = np.float32
FILL = -10000.0
LOLO = 2.0 ** -22

# the shapes of test_attn_float64_gpu.py: (B, H, dh, Lq, La, Lb), and the values of p each runs with
SHAPES = [(2, 2, 16, 1, 1, 20), (2, 2, 32, 20, 20, 1), (2, 2, 32, 20, 20, 12), (2, 3, 48, 40, 40, 100), (2, 2, 48, 100, 40, 100),
          (1, 2, 64, 49, 17, 30), (1, 2, 16, 112, 96, 96), (1, 1, 48, 33, 176, 16), (1, 2, 32, 48, 64, 16), (2, 2, 16, 8, 40, 8),
          (2, 2, 8, 7, 40, 7), (2, 4, 4, 33, 5, 3), (2, 2, 16, 40, 0, 100), (2, 2, 16, 40, 40, 0)]
P_HALF = {(2, 2, 32, 20, 20, 1), (2, 3, 48, 40, 40, 100)}          # config 3 and config 2: p = 0.5 as well


def drop_ps(shape):
    return (0.0, 0.1, 0.5) if shape in P_HALF else (0.0, 0.1)


def r16(x):
    return (x + 15) & ~15


def scale_of(dh):
    """1 / sqrt(dh) as attn_fill forms it: 1.0f / sqrtf((float)dh)"""
    return F(1.0) / np.sqrt(F(dh))


# ------------------------------------------------------------------ dispatch restated (capi.hip)
KNOBS = dict(ATT_FWD_PL=1, ATT_FWD_LDS=1, ATT_FWD_KSPLIT=1, ATT_STREAM=0, ATT_FUSED_LAUNCH=2, ATT_MERGE=1, ATT_WAVES=4, ATT_WAVES_PL=3)
SHAPE_KNOBS = dict(ATT_HPB_FWD=0, ATT_HPB_DQ=0, ATT_HPB_DKV=0)          # workgroup shape: heads per workgroup | tiles << 8
ATT_PL_MAXW, ATT_FUSED_QCHUNK, ATT_FUSED_MAXW, ATT_WIDE_MAXW = 7, 48, 12, 8


def _knobs(k):
    out = dict(KNOBS)
    out.update(SHAPE_KNOBS)
    out.update(k or {})
    return out


def _by_key_tiles(Tp):
    return 4 if Tp <= 64 else 10 if Tp <= 160 else 12


def _by_waves(nw):
    return 4 if nw <= 4 else 8 if nw <= 8 else 12


def fwd_lds_bytes(dh, La, Lb):
    ch = lambda rows: (rows * (dh // 4 + 1) + 63) & ~63
    return (2 * ch(r16(La)) + 2 * ch(r16(Lb))) * 16 + r16(La) + r16(Lb)


def fwd_pl_takes(dh, Lq, La, Lb, pin, knobs=None, masks_aligned=True):
    """attn_fwd_pl_takes"""
    k = _knobs(knobs)
    if dh % 16 != 0 or dh > 64 or k["ATT_FWD_PL"] == 0:
        return False
    nqt, T = (Lq + 15) // 16, La + Lb
    return bool(pin) and La % 4 == 0 and Lb % 4 == 0 and nqt <= ATT_PL_MAXW and T <= 192 and 2 * T * (dh // 4) * 16 <= 160 * 1024 and masks_aligned


def fwd_instance(dh, Lq, La, Lb, pin=False, knobs=None, f32_views=True):
    """attn_launch_fwd: the kernel instance of a forward call (head dims <= 64), or an error string starting with '!'."""
    k = _knobs(knobs)
    Tp, nqt = r16(La) + r16(Lb), (Lq + 15) // 16
    if fwd_pl_takes(dh, Lq, La, Lb, pin, k):
        T = La + Lb
        if dh == 48 and La == 40 and 128 < T <= 144:
            return "fwd_pl<48,9,40,hot>"
        return "fwd_pl<%d,%d>" % (dh, 4 if T <= 64 else 9 if T <= 144 else 12)
    if not f32_views:
        return "!no fp32 views"
    if Tp > 192 or k["ATT_STREAM"]:
        return "fwd_stream<%d>" % dh
    lds = k["ATT_FWD_LDS"]
    if dh >= 16 and (lds == 2 or (lds == 1 and nqt >= 4)) and nqt <= 8 and fwd_lds_bytes(dh, La, Lb) <= 80 * 1024:
        ksp = min(k["ATT_FWD_KSPLIT"], Tp // 16)
        if ksp < 1 or nqt * ksp > 12:
            ksp = 1
        return "fwd_lds<%d,%d>ksp%d" % (dh, _by_key_tiles(Tp), ksp)
    return "fwd<%d,%d>" % (dh, _by_key_tiles(Tp))


def fwd_ksplit(name):
    return int(name.rsplit("ksp", 1)[1]) if "ksp" in name else 1


def bwd_instance(dh, Lq, La, Lb, phase, mode=1, pin=False, knobs=None, f32_views=True):
    """attn_launch_bwd: the tuple of kernel instances one backward call launches (head dims <= 64)."""
    k = _knobs(knobs)
    Tp = r16(La) + r16(Lb)
    streamed = Tp > 192 or k["ATT_STREAM"]
    if phase == 1:
        return ("D_stream<%d>" % dh if streamed else "D<%d>" % dh,)
    if phase >= 4:
        nta, ntb = r16(La) // 16, r16(Lb) // 16
        if nta > ATT_FUSED_MAXW or ntb > ATT_FUSED_MAXW:
            return ("!more than 12 key tiles in a block",)
        small = 16 if Lq <= 16 else 32 if Lq <= 32 else ATT_FUSED_QCHUNK
        f16able = dh % 16 == 0 and dh <= 48
        if not pin and k["ATT_MERGE"] and phase == 4 and Lq <= 32 and nta > 0 and ntb > 0 and nta + ntb <= 4 and not (f16able and mode >= 2):
            return ("fused<%d,4,merged,%d>" % (dh, small),)
        fmode, out = k["ATT_FUSED_LAUNCH"], []
        one = Lq <= ATT_FUSED_QCHUNK
        for blk in range(2):
            if fmode == 1 and blk == 1:
                break
            if fmode != 1 and phase >= 5 and blk != phase - 5:
                continue
            nw = max(nta, ntb) if fmode == 1 else (nta if blk == 0 else ntb)
            if nw == 0:
                continue
            tag = "ab" if fmode == 1 else "ab"[blk]
            if f16able and pin:
                wc = k["ATT_WAVES_PL"] if 1 <= k["ATT_WAVES_PL"] <= 4 else 3
                nwp = wc if one and nw > wc else nw
                out.append("pl<%d,%d,%s>%s/w%d" % (dh, _by_waves(nwp), "one" if one else "chunks", tag, nwp))
                continue
            if f16able and mode >= (1 if one and Lq > 32 else 2):
                wc = k["ATT_WAVES"]
                nw16 = wc if one and wc >= 1 and nw > wc else nw
                out.append("fused16<%d,%d,%s>%s/w%d" % (dh, _by_waves(nw16), "one" if one else "chunks", tag, nw16))
                continue
            if not f32_views:
                return ("!no fp32 views",)
            q = "16" if small == 16 else "32" if small == 32 else "one" if one else "chunks"
            out.append("fused<%d,%d,%s>%s/w%d" % (dh, _by_waves(nw), q, tag, nw))
        return tuple(out)
    out = []
    if phase in (0, 2):
        out.append("dq_stream<%d>" % dh if streamed else "dq<%d,%d>" % (dh, _by_key_tiles(Tp)))
    if phase in (0, 3):
        Lq_p = r16(Lq)
        out.append("dkv<%d,%d>" % (dh, 3 if Lq_p == 48 else 1 if Lq_p == 16 else 0))
    return tuple(out)


def attn_shape(n, H, max_waves, knob, want_default=1):
    """attn_shape: (wq, hpb) of a one-wave-per-tile kernel with n row tiles per head; knob = heads | tiles << 8"""
    wq = n
    if n > 5:
        wq = next((w for w in (5, 4, 3) if n % w == 0), 4)
    wq = min(wq, max_waves)
    want = want_default
    if knob & 0xff:
        want = knob & 0xff
        if 0 < (knob >> 8) <= n and (knob >> 8) <= max_waves:
            wq = knob >> 8
    hpb = next((c for c in range(want, 0, -1) if H % c == 0 and c * wq <= max_waves), 1)
    return wq, hpb


def wide(dh):
    return dh > 64


def _bwd_waves(dh):
    return 4 if wide(dh) else 12          # att_bwd_threads / 64


def fwd_launch(H, dh, Lq, La, Lb, pin=False, knobs=None, f32_views=True):
    """attn_launch_fwd for every built head dim: the instance of ``fwd_instance`` (head dims 96 and 128: the direct or the streamed
    form only) and, for the kernels with a workgroup shape, '/wq<tiles>/hpb<heads>'."""
    k = _knobs(knobs)
    Tp, nqt = r16(La) + r16(Lb), (Lq + 15) // 16
    if wide(dh):
        if not f32_views:
            return "!no fp32 views"          # (wide heads never take the planes-in or the staged form)
        name = "fwd_stream<%d>" % dh if Tp > 192 or k["ATT_STREAM"] else "fwd<%d,%d>" % (dh, _by_key_tiles(Tp))
    else:
        name = fwd_instance(dh, Lq, La, Lb, pin=pin, knobs=k, f32_views=f32_views)
    if name.startswith("fwd_stream<"):
        return name + "/wq%d/hpb%d" % attn_shape(nqt, H, 4 if wide(dh) else 5, k["ATT_HPB_FWD"])
    if name.startswith("fwd<"):
        return name + "/wq%d/hpb%d" % attn_shape(nqt, H, 5, k["ATT_HPB_FWD"])
    return name


def bwd_launch(H, dh, Lq, La, Lb, phase, mode=1, pin=False, knobs=None, f32_views=True, repair=False):
    """attn_launch_bwd for every built head dim: the tuple of ``bwd_instance`` with the workgroup shape of the dQ and dK/dV kernels
    ('/wq<tiles>/hpb<heads>') and, for head dims 96 and 128, the wide fused kernel's launches
    'wide<dh,W,QCH>blocks/w<waves>/p<passes>'.  ``repair``: the repair launch (one launch for both blocks whatever the knob)."""
    k = _knobs(knobs)
    La_p, Lb_p = r16(La), r16(Lb)
    Tp, nta, ntb = La_p + Lb_p, La_p // 16, Lb_p // 16
    if phase >= 4 and Tp > 192:          # segmm_attn_bwd itself: the fused backward is entered with at most 192 padded keys in all
        return ("!more than 192 padded keys in the fused backward",)
    if phase >= 4 and wide(dh):
        if nta > ATT_FUSED_MAXW or ntb > ATT_FUSED_MAXW:
            return ("!more than 12 key tiles in a block",)
        if pin or not f32_views:
            return ("!wide heads take the fp32 views",)
        small = 16 if Lq <= 16 else 32 if Lq <= 32 else ATT_FUSED_QCHUNK
        if k["ATT_MERGE"] and phase == 4 and Lq <= 32 and nta > 0 and ntb > 0 and nta + ntb <= 4:
            return ("wide<%d,4,merged,%d>/w%d/p1" % (dh, small, nta + ntb),)
        fmode, out = (1 if repair else k["ATT_FUSED_LAUNCH"]), []
        one = Lq <= ATT_FUSED_QCHUNK
        for blk in range(2):
            if fmode == 1 and blk == 1:
                break
            if fmode != 1 and phase >= 5 and blk != phase - 5:
                continue
            nt_ = max(nta, ntb) if fmode == 1 else (nta if blk == 0 else ntb)
            if nt_ == 0:
                continue
            nw = min(nt_, ATT_WIDE_MAXW)
            q = "16" if small == 16 else "32" if small == 32 else "one" if one else "chunks"
            out.append("wide<%d,%d,%s>%s/w%d/p%d" % (dh, 4 if nw <= 4 else 8, q, "ab" if fmode == 1 else "ab"[blk], nw, -(-nt_ // nw)))
        return tuple(out)
    if wide(dh):
        streamed = Tp > 192 or k["ATT_STREAM"]
        names = []
        if phase == 1:
            names.append("D_stream<%d>" % dh if streamed else "D<%d>" % dh)
        if phase in (0, 2):
            names.append("dq_stream<%d>" % dh if streamed else "dq<%d,%d>" % (dh, _by_key_tiles(Tp)))
        if phase in (0, 3):
            names.append("dkv<%d,%d>" % (dh, 3 if r16(Lq) == 48 else 1 if r16(Lq) == 16 else 0))
    else:
        names = bwd_instance(dh, Lq, La, Lb, phase, mode=mode, pin=pin, knobs=k, f32_views=f32_views)
    out = []
    for n in names:
        if n.startswith("dq"):
            n += "/wq%d/hpb%d" % attn_shape((Lq + 15) // 16, H, _bwd_waves(dh), k["ATT_HPB_DQ"])
        elif n.startswith("dkv<"):
            wq, hpb = attn_shape(Tp // 16, H, _bwd_waves(dh), k["ATT_HPB_DKV"])
            if not k["ATT_HPB_DKV"]:
                wq = 2 if Tp // 16 >= 2 else 1          # (small workgroups; hpb was chosen before)
            n += "/wq%d/hpb%d" % (wq, hpb)
        out.append(n)
    return tuple(out)


def launch_field(name, key):
    """the integer behind '/<key>' in an instance string ('w', 'p', 'wq', 'hpb'); None when the instance has none"""
    for part in name.split("/")[1:]:
        if part.startswith(key) and part[len(key):].isdigit():
            return int(part[len(key):])
    return None


def rep_of(instances):
    """The operand representation ('f32', 'f16x3', 'planes') the bound of a backward call is taken for."""
    reps = {"planes" if n.startswith("pl<") else "f16x3" if n.startswith("fused16<") else "f32" for n in instances}
    assert len(reps) == 1, instances
    return reps.pop()


# ------------------------------------------------------------------ inputs
def batch_rows(shape):
    """The listed B rows with random masks, then three rows with set masks (block a masked, every key masked, fully valid)."""
    return shape[0] + 3


def make_masks(shape, seed):
    B0, H, dh, Lq, La, Lb = shape
    B = batch_rows(shape)
    r = np.random.RandomState(seed)
    mq, mka, mkb = r.rand(B, Lq) < 0.8, r.rand(B, La) < 0.8, r.rand(B, Lb) < 0.7
    mq[0, 0] = False                       # one masked query in a row that has valid ones (Lq = 1: the only query)
    mq[0, 1:2] = True
    if B0 > 1:
        mq[1, 0] = True
    mka[B0] = False                        # block a fully masked
    mka[B0 + 1] = False                    # every key of both blocks masked
    mkb[B0 + 1] = False
    mq[B0 + 2], mka[B0 + 2], mkb[B0 + 2] = True, True, True
    return mq, mka, mkb


def make_inputs(shape, seed=0):
    """Operands as the engine lays them out: Qa | Qb | Ka | Va column slices of Yv [B La, 4 d], Kb | Vb of Yu [B Lb, 2 d]; the
    queries in a buffer of their own when Lq != La.  Returns a dict of fp32 arrays and bool masks."""
    B0, H, dh, Lq, La, Lb = shape
    B, d = batch_rows(shape), H * dh
    r = np.random.RandomState(1000 + seed)
    Yv = (r.randn(B * max(La, 1), 4 * d) * 0.7).astype(F)
    Yu = (r.randn(B * max(Lb, 1), 2 * d) * 0.7).astype(F)
    Qs = Yv if Lq == La else (r.randn(B * Lq, 4 * d) * 0.7).astype(F)
    dO = r.randn(B * Lq, d).astype(F)
    mq, mka, mkb = make_masks(shape, seed + 7)
    return dict(shape=shape, B=B, Yv=Yv, Yu=Yu, Qs=Qs, dO=dO, mq=mq, mka=mka, mkb=mkb)


def numpy_mult(shape, p, seed):
    """A numpy draw of dropout multipliers in the kernels' layout (the CPU tests; the GPU tests export the kernels' own)."""
    B0, H, dh, Lq, La, Lb = shape
    Tp = r16(La) + r16(Lb)
    if p == 0.0:
        return np.ones((batch_rows(shape), H, Lq, Tp), F)
    keep = np.random.RandomState(seed).rand(batch_rows(shape), H, Lq, Tp) >= p
    return np.where(keep, F(1.0) / (F(1.0) - F(p)), F(0.0)).astype(F)


def operands(inp, Yv=None, Yu=None, Qs=None):
    """The six operands [B, L, d] (float64) cut from the fused buffers; other buffers (the values planes hold) may be given."""
    B0, H, dh, Lq, La, Lb = inp["shape"]
    B, d = inp["B"], H * dh
    Yv = inp["Yv"] if Yv is None else Yv
    Yu = inp["Yu"] if Yu is None else Yu
    Qs = inp["Qs"] if Qs is None else Qs
    cut = lambda Y, k, L: np.asarray(Y, np.float64).reshape(B, max(L, 1), -1)[:, :L, k * d:(k + 1) * d]
    return cut(Qs, 0, Lq), cut(Qs, 1, Lq), cut(Yv, 2, La), cut(Yv, 3, La), cut(Yu, 0, Lb), cut(Yu, 1, Lb)


def _heads(x, H):
    B, L, d = x.shape
    return x.reshape(B, L, H, d // H).transpose(0, 2, 1, 3)          # [B, H, L, dh]


def _unheads(x):
    B, H, L, dh = x.shape
    return x.transpose(0, 2, 1, 3).reshape(B, L, H * dh)


def real_keys(mult, La, Lb):
    """[.., La_p + Lb_p] -> [.., La + Lb]"""
    return np.concatenate([mult[..., :La], mult[..., r16(La):r16(La) + Lb]], -1)


# ------------------------------------------------------------------ the float64 statement
def fill_logit(mult32, dh):
    """logit_xform's value of a fill: two rounded fp32 products"""
    return (F(FILL) * mult32.astype(F)).astype(F) * scale_of(dh)


def statement(ops, mq, mka, mkb, H, mult, dO):
    """ops: (Qa, Qb, Ka, Va, Kb, Vb) [B, L, d]; mult [B, H, Lq, La_p + Lb_p] fp32; dO [B, Lq, d].  Returns a dict of float64 arrays:
    the outputs (O, m, inv, D, dQa, dQb, dKa, dVa, dKb, dVb in the tensors' own [B, L, d] / [B, H, Lq] shapes) and every intermediate
    the bounds need ([B, H, Lq, T] unless noted)."""
    Qa, Qb, Ka, Va, Kb, Vb = [_heads(np.asarray(t, np.float64), H) for t in ops]
    B, _, Lq, dh = Qa.shape
    La, Lb = Ka.shape[2], Kb.shape[2]
    scale = np.float64(scale_of(dh))
    m32 = real_keys(np.asarray(mult, F), La, Lb)
    mu = m32.astype(np.float64)
    raw = np.concatenate([Qa @ Ka.transpose(0, 1, 3, 2), Qb @ Kb.transpose(0, 1, 3, 2)], -1)
    absqk = np.concatenate([np.abs(Qa) @ np.abs(Ka).transpose(0, 1, 3, 2), np.abs(Qb) @ np.abs(Kb).transpose(0, 1, 3, 2)], -1)
    valid = (mq[:, :, None] & np.concatenate([mka, mkb], -1)[:, None, :])[:, None]
    valid = np.broadcast_to(valid, raw.shape)
    logit = np.where(valid, raw * mu * scale, fill_logit(m32, dh).astype(np.float64))
    m = logit.max(-1)
    x = logit - m[..., None]
    e = np.exp(x)
    inv = 1.0 / e.sum(-1)
    P = e * inv[..., None]
    V = np.concatenate([Va, Vb], 2)
    Oh = P @ V
    dOh = _heads(np.asarray(dO, np.float64).reshape(B, Lq, -1), H)
    D = (dOh * Oh).sum(-1)
    dV = P.transpose(0, 1, 3, 2) @ dOh
    dP = dOh @ V.transpose(0, 1, 3, 2)
    dS = P * (dP - D[..., None])
    dl = np.where(valid, dS * mu * scale, 0.0)
    dQa, dQb = dl[..., :La] @ Ka, dl[..., La:] @ Kb
    dKa, dKb = dl[..., :La].transpose(0, 1, 3, 2) @ Qa, dl[..., La:].transpose(0, 1, 3, 2) @ Qb
    # the rule the bounds rest on: a fill is dropped (exactly 0), has probability exactly 0, or its row is uniform
    rows_uniform = (logit == logit[..., :1]).all(-1)
    assert ((P == 0) | valid | (logit == 0) | rows_uniform[..., None]).all(), "a kept fill with a probability in a row that is not uniform"
    return dict(H=H, dh=dh, Lq=Lq, La=La, Lb=Lb, scale=scale, Qa=Qa, Qb=Qb, Ka=Ka, Kb=Kb, V=V, dOh=dOh, mu=mu, valid=valid, raw=raw,
                absqk=absqk, logit=logit, x=x, P=P, dP=dP, dS=dS, dl=dl, Oh=Oh,
                O=_unheads(Oh), m=m, inv=inv, D=D, dQa=_unheads(dQa), dQb=_unheads(dQb), dKa=_unheads(dKa), dVa=_unheads(dV[:, :, :La]),
                dKb=_unheads(dKb), dVb=_unheads(dV[:, :, La:]))


OUTPUTS_FWD = ("O", "m", "inv")
OUTPUTS_BWD = ("D", "dQa", "dQb", "dKa", "dVa", "dKb", "dVb")


# ------------------------------------------------------------------ bounds
def c_dot(n):
    return n + 1


def _split_terms(rep, sum_ab, a, b):
    """The representation part of one product's error.  a, b: (kernel splits it itself?, magnitude bound A, sum|other| array) per
    operand; rep 'f32': nothing."""
    if rep == "f32":
        return 0.0
    nsplit = int(a[0]) + int(b[0])
    e = (nsplit * P32.REL + LOLO) * sum_ab
    for on, A, other in (a, b):
        if on:
            e = e + P32.ABS * 2.0 ** -14 * A * other
    return e


def bounds_fwd(st, rep="f32", merge=False, stream=0):
    """Bounds of the forward outputs (same shapes as the statement's) and the pieces a backward bound needs.  ``stream``: the key
    tile count nt of a streamed (online softmax) forward, 0 for the held forms."""
    dh, T = st["dh"], st["La"] + st["Lb"]
    on = rep == "f16x3"                                    # Q, K, V split by the kernel itself?
    Av = float(np.abs(st["V"]).max()) if st["V"].size else 0.0
    eps = own_eps(st, rep)
    eps_m = np.where(st["valid"], eps, 2 * U * np.abs(st["logit"]))
    assert not (stream and (merge or rep != "f32")), "the streamed forward has fp32 operands and no key split"
    ex = (3 * np.abs(st["x"]) + (2 * stream if stream else 2)) * U
    P = st["P"]
    N = (P * (eps + ex)).sum(-1) + ((2 * stream + 7) if stream else (T + 3 + (8 if merge else 0))) * U
    rho = eps + ex + N[..., None]
    # keys that can be the computed maximum: within the two errors of the exact one
    cand = st["logit"] + eps_m >= (st["m"] - (eps_m * (st["x"] == 0)).max(-1))[..., None]
    b_m = (eps_m * cand).max(-1)
    b_inv = (N + b_m) * st["inv"]
    absV = np.abs(st["V"])
    pv = P @ absV
    b_O = (P * rho) @ absV + (c_dot(T) + max(stream - 1, 0)) * U * pv + _split_terms(rep, pv, (rep != "f32", 1.0, np.broadcast_to(absV.sum(2)[:, :, None, :], pv.shape)),
                                                              (on, Av, np.broadcast_to(P.sum(-1)[..., None], pv.shape)))
    return dict(O=_unheads(b_O), m=b_m, inv=b_inv, N=N, Oh=b_O)


def bounds_bwd(st, fwd, rep="f32"):
    """Bounds of the backward outputs for a backward of representation ``rep`` that consumes the O and lse of the forward whose
    bounds are ``fwd`` (bounds_fwd of that forward's form)."""
    dh, Lq, La, T = st["dh"], st["Lq"], st["La"], st["La"] + st["Lb"]
    fac = st["mu"] * st["scale"]
    on, f16 = rep == "f16x3", rep != "f32"
    amax = lambda t: float(np.abs(t).max()) if t.size else 0.0
    P, V, dOh = st["P"], st["V"], st["dOh"]
    absV, absdO = np.abs(V), np.abs(dOh)
    AdO, Av = amax(dOh), amax(V)
    eps = own_eps(st, rep)                                 # this form's recomputed logits
    rho = eps + (3 * np.abs(st["x"]) + 3) * U + fwd["N"][..., None]
    b_D = (dh + 1) * U * (absdO * np.abs(st["Oh"])).sum(-1) + (absdO * fwd["Oh"]).sum(-1)
    # dV = P^T dO
    pdo = P.transpose(0, 1, 3, 2) @ absdO
    b_dV = (P * rho).transpose(0, 1, 3, 2) @ absdO + c_dot(Lq) * U * pdo + _split_terms(
        rep, pdo, (f16, 1.0, np.broadcast_to(absdO.sum(2)[:, :, None, :], pdo.shape)), (f16, AdO, np.broadcast_to(P.sum(2)[..., None], pdo.shape)))
    # dP = dO V^T
    dov = absdO @ absV.transpose(0, 1, 3, 2)
    e_dP = c_dot(dh) * U * dov + _split_terms(rep, dov, (f16, AdO, np.broadcast_to(absV.sum(-1)[:, :, None, :], dov.shape)),
                                              (on, Av, np.broadcast_to(absdO.sum(-1)[..., None], dov.shape)))
    e_dS = P * (e_dP + b_D[..., None]) + rho * np.abs(st["dS"]) + 2 * U * np.abs(st["dS"])
    e_dl = np.where(st["valid"], e_dS * fac + 3 * U * np.abs(st["dl"]), 0.0)
    A_dS = (dh * AdO * Av + amax(st["D"])) * float(st["mu"].max()) * st["scale"]          # the kernels' own bound of |dS| (attention16.h)
    adl = np.abs(st["dl"])
    out = dict(D=b_D)
    for blk, sl, K, Q, Ak in (("a", slice(0, La), st["Ka"], st["Qa"], amax(st["Ka"])), ("b", slice(La, T), st["Kb"], st["Qb"], amax(st["Kb"]))):
        n = sl.stop - sl.start
        aK, aQ = np.abs(K), np.abs(Q)
        dlk = adl[..., sl] @ aK
        b_dQ = e_dl[..., sl] @ aK + c_dot(max(n, 1)) * U * dlk + _split_terms(
            rep, dlk, (f16, A_dS, np.broadcast_to(aK.sum(2)[:, :, None, :], dlk.shape)), (on, Ak, np.broadcast_to(adl[..., sl].sum(-1)[..., None], dlk.shape)))
        dlq = adl[..., sl].transpose(0, 1, 3, 2) @ aQ
        b_dK = e_dl[..., sl].transpose(0, 1, 3, 2) @ aQ + c_dot(Lq) * U * dlq + _split_terms(
            rep, dlq, (f16, A_dS, np.broadcast_to(aQ.sum(2)[:, :, None, :], dlq.shape)),
            (on, amax(Q), np.broadcast_to(adl[..., sl].sum(2)[..., None], dlq.shape)))
        out["dQ" + blk], out["dK" + blk], out["dV" + blk] = _unheads(b_dQ), _unheads(b_dK), _unheads(b_dV[:, :, sl])
    return out


def own_eps(st, rep):
    """eps_s of a form's logits (0 at fills), as bounds_fwd forms it"""
    dh = st["dh"]
    on = rep == "f16x3"
    amax = lambda t: float(np.abs(t).max()) if t.size else 0.0
    Aq, Ak = max(amax(st["Qa"]), amax(st["Qb"])), max(amax(st["Ka"]), amax(st["Kb"]))
    La = st["La"]
    sumq = np.concatenate([np.broadcast_to(np.abs(st["Qa"]).sum(-1)[..., None], st["raw"][..., :La].shape),
                           np.broadcast_to(np.abs(st["Qb"]).sum(-1)[..., None], st["raw"][..., La:].shape)], -1)
    sumk = np.concatenate([np.abs(st["Ka"]).sum(-1), np.abs(st["Kb"]).sum(-1)], -1)[:, :, None, :]
    e_raw = c_dot(dh) * U * st["absqk"] + _split_terms(rep, st["absqk"], (on, Aq, sumk), (on, Ak, sumq))
    return np.where(st["valid"], (e_raw + 2 * U * np.abs(st["raw"])) * st["mu"] * st["scale"], 0.0)


def ratio(got, want, bound):
    """max |got - want| / bound; an element whose bound is 0 must be met exactly"""
    err = np.abs(np.asarray(got, np.float64) - want)
    if err.size == 0:
        return 0.0
    if not np.isfinite(err).all():
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max())


# ------------------------------------------------------------------ fp32 emulation, fixed order, with planted defects
DEFECTS = ("pad_key_filled", "mult_b_unpadded", "drop_after_scale_fills_undropped", "dropped_masked_key_kept", "key_mask_shifted",
           "mq_ignored", "qb_for_qa", "D_without_dropped", "dlogit_without_mult", "dqa_takes_block_b", "head_offset", "inv_holds_sum",
           "lse_swapped", "dq_skips_last_tile", "p_rel_2^-11")


def _dot32(a, b):
    """sum over the last axis of a * b in fp32, products rounded, added in index order"""
    acc = np.zeros(np.broadcast_shapes(a.shape[:-1], b.shape[:-1]), F)
    for i in range(a.shape[-1]):
        acc = acc + a[..., i] * b[..., i]
    return acc


def _mm32(a, b):
    """a [.., M, n] @ b [.., n, N] in fp32, fixed order"""
    return _dot32(a[..., :, None, :], np.swapaxes(b, -1, -2)[..., None, :, :])


def emulate(inp, mult, defect=None):
    """Forward and backward in numpy fp32 on the fp32 operands of ``inp``: fp32 products and sums in index order, exp as
    exp2(x log2e) in fp32, the logit transform with each product rounded.  ``defect``: one of DEFECTS planted.  Returns the
    outputs under the statement's names."""
    B0, H, dh, Lq, La, Lb = inp["shape"]
    B = inp["B"]
    Qa, Qb, Ka, Va, Kb, Vb = [_heads(t.astype(F), H) for t in operands(inp)]
    dOh = _heads(inp["dO"].reshape(B, Lq, -1).astype(F), H)
    mq, mka, mkb = inp["mq"], inp["mka"], inp["mkb"]
    La_p, Lb_p = r16(La), r16(Lb)
    scale = scale_of(dh)
    mult = np.asarray(mult, F)
    if defect == "head_offset":                 # the head column offset h dh one head off (V of the next head)
        Va, Vb = np.roll(Va, -1, 1), np.roll(Vb, -1, 1)
    if defect == "key_mask_shifted":
        mka, mkb = np.roll(mka, 1, 1), np.roll(mkb, 1, 1)
    if defect == "mq_ignored":
        mq = np.ones_like(mq)
    boff = La if defect == "mult_b_unpadded" else La_p
    mu = np.concatenate([mult[..., :La], mult[..., boff:boff + Lb]], -1)
    if mu.shape[-1] < La + Lb:                  # (block b read past the end of a row: the next row's multipliers, here: ones)
        mu = np.concatenate([mu, np.ones(mu.shape[:-1] + (La + Lb - mu.shape[-1],), F)], -1)
    raw = np.concatenate([_mm32(Qb if defect == "qb_for_qa" else Qa, Ka.transpose(0, 1, 3, 2)), _mm32(Qb, Kb.transpose(0, 1, 3, 2))], -1)
    valid = np.broadcast_to((mq[:, :, None] & np.concatenate([mka, mkb], -1)[:, None, :])[:, None], raw.shape)
    filled = np.where(valid, raw, F(FILL))
    if defect == "drop_after_scale_fills_undropped":
        logit = np.where(valid, (raw * mu).astype(F) * scale, F(FILL) * scale)
    elif defect == "dropped_masked_key_kept":
        logit = np.where(valid, (raw * mu).astype(F) * scale, (F(FILL) * mu.max()).astype(F) * scale)
    else:
        logit = (filled * mu).astype(F) * scale
    logit = logit.astype(F)
    npad = (La_p - La) + (Lb_p - Lb) if defect == "pad_key_filled" else 0
    m = logit.max(-1)
    if npad:
        m = np.maximum(m, F(FILL) * scale)
    L2E = F(1.4426950408889634)
    ex = lambda x: np.exp2((x * L2E).astype(F)).astype(F)
    e = ex(logit - m[..., None])
    s = np.zeros(m.shape, F)
    for k in range(e.shape[-1]):
        s = s + e[..., k]
    for _ in range(npad):
        s = s + ex(F(FILL) * scale - m)
    inv = (F(1.0) / s).astype(F)
    P = (e * inv[..., None]).astype(F)
    if defect == "p_rel_2^-11":
        P = (P * F(1 + 2.0 ** -11)).astype(F)
    V = np.concatenate([Va, Vb], 2)
    Oh = _mm32(P, V)
    # backward: P recomputed from the saved statistics
    Pb = (ex(logit - m[..., None]) * inv[..., None]).astype(F)
    if defect == "p_rel_2^-11":
        Pb = (Pb * F(1 + 2.0 ** -11)).astype(F)
    dP = _mm32(dOh, V.transpose(0, 1, 3, 2))
    if defect == "D_without_dropped":
        D = _dot32(Pb * (mu != 0), dP)
    else:
        D = _dot32(dOh, Oh)
    dV = _mm32(Pb.transpose(0, 1, 3, 2), dOh)
    fac = (mu * scale).astype(F) if defect != "dlogit_without_mult" else np.broadcast_to(scale, mu.shape)
    dl = np.where(valid, ((Pb * (dP - D[..., None])).astype(F) * fac).astype(F), F(0))
    dla, dlb = dl[..., :La], dl[..., La:]
    if defect == "dq_skips_last_tile":
        dla, dlb = dla.copy(), dlb.copy()
        if Lb:
            dlb[..., 16 * ((Lb - 1) // 16):] = 0
        else:
            dla[..., 16 * ((La - 1) // 16):] = 0
    dQa, dQb = _mm32(dla, Ka), _mm32(dlb, Kb)
    if defect == "dqa_takes_block_b":
        dQa = dQa + _mm32(dl[..., La:], Kb)
    dKa, dKb = _mm32(dl[..., :La].transpose(0, 1, 3, 2), Qa), _mm32(dl[..., La:].transpose(0, 1, 3, 2), Qb)
    out = dict(O=_unheads(Oh), m=m, inv=inv, D=D, dQa=_unheads(dQa), dQb=_unheads(dQb), dKa=_unheads(dKa), dVa=_unheads(dV[:, :, :La]),
               dKb=_unheads(dKb), dVb=_unheads(dV[:, :, La:]))
    if defect == "inv_holds_sum":
        out["inv"] = s
    if defect == "lse_swapped":
        out["m"], out["inv"] = out["inv"], out["m"]
    return out


def ratios(out, st, bf, bb):
    """worst error / bound per output of an emulation or a kernel run"""
    r = {k: ratio(out[k], st[k], bf[k]) for k in OUTPUTS_FWD if k in out}
    r.update({k: ratio(out[k], st[k], bb[k]) for k in OUTPUTS_BWD if k in out})
    return r


# ------------------------------------------------------------------ wide heads and streamed forms: shapes, the dropout stream on the host
WIDE_DIMS = (96, 128)
STREAM_DIMS = (4, 8, 16, 32, 48, 64, 96, 128)


def wide_shapes(dh):
    """(shape, what it reaches) of test_attn_wide_stream_float64_gpu.py at a wide head dim"""
    return [(2, 2, dh, 1, 1, 20), (2, 2, dh, 20, 20, 12), (2, 2, dh, 20, 20, 1), (1, 2, dh, 40, 40, 100), (1, 2, dh, 49, 17, 30),
            (1, 2, dh, 100, 40, 100), (1, 1, dh, 33, 176, 16), (1, 1, dh, 52, 132, 16), (2, 2, dh, 40, 0, 100), (2, 2, dh, 40, 40, 0)]


WIDE_SHAPES = [s for dh in WIDE_DIMS for s in wide_shapes(dh)]
# ATT_STREAM = 1 at a small shape per built head dim
STREAM_SMALL = [(2, 4, 4, 33, 5, 3), (2, 2, 8, 7, 40, 7), (2, 2, 16, 1, 1, 20), (2, 2, 32, 20, 20, 12), (2, 3, 48, 40, 40, 100),
                (1, 2, 64, 49, 17, 30), (1, 2, 96, 40, 40, 100), (1, 2, 128, 40, 40, 100)]
# above 192 padded keys: streamed whatever the knob
STREAM_LONG = [(1, 2, 16, 17, 200, 9), (1, 1, 96, 17, 200, 9), (1, 1, 128, 17, 200, 9), (1, 2, 48, 40, 200, 0), (1, 1, 128, 17, 200, 0),
               (1, 2, 8, 7, 0, 208), (1, 1, 64, 33, 256, 256), (1, 1, 128, 33, 256, 256)]
# 11 + 2 tiles, Tp = 208: streamed forward, D and dQ; the fused backward REFUSES more than 192 padded keys (segmm_attn_bwd), so the
# streamed forward in front of the fused backward is reached at 11 + 1 tiles under ATT_STREAM = 1 (two passes at a wide head)
STREAM_FUSED = [(1, 2, 48, 33, 176, 32), (1, 2, 96, 33, 176, 32), (1, 2, 128, 33, 176, 32)]
STREAM_FUSED_RUN = [(1, 2, 48, 33, 176, 16), (1, 2, 96, 33, 176, 16), (1, 2, 128, 33, 176, 16)]
# the workgroup-shape knobs
HPB_SHAPES = [(2, 2, 32, 20, 20, 12), (2, 4, 4, 33, 5, 3), (2, 2, 96, 20, 20, 12), (1, 2, 16, 17, 200, 9)]
P_HALF_WIDE = {(1, 2, 96, 40, 40, 100), (1, 2, 128, 40, 40, 100)}
DROP_SEED, DROP_SITE = 11, 3          # the dropout stream of every GPU case; its preconditions are checked on the host stream below


def drop_ps_x(shape):
    return (0.0, 0.1, 0.5) if shape in P_HALF_WIDE else (0.0, 0.1)


def n_tiles(shape):
    return (r16(shape[4]) + r16(shape[5])) // 16


def hpb_value(kernel, shape, knobs=None):
    """The value of ATT_HPB_<kernel> ('FWD', 'DQ', 'DKV') that puts two heads in a workgroup at ``shape``: 2 where attn_shape takes it,
    otherwise 2 | tiles << 8 with the most tiles per head that still fit (the knob's own second field; the shape stays)."""
    B0, H, dh, Lq, La, Lb = shape
    for tiles in [0] + list(range(12, 0, -1)):
        v = 2 | (tiles << 8)
        k = dict(knobs or {})
        k["ATT_HPB_" + kernel] = v
        if kernel == "FWD":
            names = (fwd_launch(H, dh, Lq, La, Lb, knobs=k),)
        else:
            names = bwd_launch(H, dh, Lq, La, Lb, 2 if kernel == "DQ" else 3, knobs=k)
        if launch_field(names[0], "hpb") == 2 and (tiles == 0 or launch_field(names[0], "wq") == tiles):
            return v
    raise AssertionError("no value of ATT_HPB_%s gives two heads per workgroup at %s" % (kernel, shape))


def _mix32(x):
    x = x & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def host_mult(shape, p, seed=DROP_SEED, site=DROP_SITE):
    """The kernels' own dropout multipliers in their layout [B, H, Lq, La_p + Lb_p], restated from common.h (make_drop,
    drop_rand_quad, drop_apply4): element e of the site draws 16 bits of the two hashed words of its quad e >> 2; kept when they
    reach the threshold round(p 65536).  The GPU test asserts that the library's exported stream is this one."""
    B0, H, dh, Lq, La, Lb = shape
    Tp = r16(La) + r16(Lb)
    dims = (batch_rows(shape), H, Lq, Tp)
    if p == 0.0:
        return np.ones(dims, F)
    thresh = int(float(F(p)) * 65536.0 + 0.5)
    scale = F(65536.0 / (65536.0 - thresh))
    e = np.arange(int(np.prod(dims)), dtype=np.uint64)
    q = e >> np.uint64(2)
    k = np.uint64((seed & 0xFFFFFFFF) ^ ((site * 0x9E3779B9) & 0xFFFFFFFF)) ^ (((q >> np.uint64(32)) * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF))
    a = _mix32((q & np.uint64(0xFFFFFFFF)) ^ k)
    b = _mix32(a ^ np.uint64(((seed >> 32) & 0x7FFFFFFF) ^ 0x68E31DA4))
    lane = e & np.uint64(3)
    w = np.where(lane < 2, a, b)
    x = np.where((lane & np.uint64(1)) != 0, w >> np.uint64(16), w & np.uint64(0xFFFF))
    return np.where(x >= thresh, scale, F(0.0)).astype(F).reshape(dims)


# ------------------------------------------------------------------ fp32 emulation of the online order, with planted defects
# rescale_l_not_o: a multiplies the row sum but not the O accumulators.  max_follows_lower_tile: after a tile whose maximum is LOWER
# than the running one, m is left at that tile's maximum instead of max(m, tile) (e and a of the tile itself are right; the next
# rescale and the stored m are not).  odd_last_tile_dropped: the loop unrolled by two forgets the tail.  block_b_tile_not_rebased:
# block b's tile t read at rows 16 t of block b, not 16 (t - nta).  pad_key_a_in_rowsum: block a's pad keys are fills, not -inf.
# drop_index_T: the dropout index formed with T, not Tp.  carry_lost / carry_twice / pass2_owns_tile_w: the wide kernel's second pass
# starts dQ from zero / adds the carry twice / owns tile w again instead of w + nw.  head_offset_128_at_96: V's head column offset
# h 128 at dh = 96.  D_first_partials: the wide kernel's D over the first dh / 8 of its dh / 4 partials.  p_rel_2^-11: as in DEFECTS.
STREAM_DEFECTS = ("rescale_l_not_o", "max_follows_lower_tile", "odd_last_tile_dropped", "block_b_tile_not_rebased", "pad_key_a_in_rowsum",
                  "drop_index_T", "carry_lost", "carry_twice", "pass2_owns_tile_w", "head_offset_128_at_96", "D_first_partials",
                  "p_rel_2^-11")


def _row_frag_index(dh):
    """[4, dh / 4]: the head columns lane group g holds of a row fragment (frag_load: 16 i + 4 g + e, or contiguous below dh 16)"""
    KS = dh // 4
    if KS % 4 == 0:
        return np.array([[16 * i + 4 * g + e for i in range(KS // 4) for e in range(4)] for g in range(4)])
    return np.array([[KS * g + i for i in range(KS)] for g in range(4)])


def emulate_online(inp, mult, defect=None, passes=0, d_order="row"):
    """The streamed kernels' order in numpy fp32: the forward walks the padded key tiles (16 keys, key blocks padded separately, pad
    keys -inf) with the running maximum m, the rescale a (0 on the first tile), the per-lane partial row sums l (lane group g holds
    keys 4 g .. 4 g + 3 of every tile) and the unnormalised o; O = o inv at the end.  The backward recomputes P from the saved m and
    inv.  ``d_order``: 'row' attn_row_D (a lane group's products chained, then the groups), 'wide' the wide fused kernel's (groups of
    four products, then the dh / 4 partials in index order).  ``passes`` = nw > 0: dQ as the wide fused kernel accumulates it -- wave w
    of pass i owns tile w + i nw of its block, the waves add their tiles' partial products in turn to a sum that is stored as fp32
    between passes; 0: one chain over the block's keys (the streamed dQ kernel).  ``defect``: one of STREAM_DEFECTS."""
    B0, H, dh, Lq, La, Lb = inp["shape"]
    B = inp["B"]
    Qa, Qb, Ka, Va, Kb, Vb = [_heads(t.astype(F), H) for t in operands(inp)]
    if defect == "head_offset_128_at_96":          # head h's V at column h 128 of the slice's buffer, not h dh (zeros past the buffer)
        d = H * dh
        def off(Y, k, L):
            Y = np.concatenate([np.asarray(Y, F).reshape(B, max(L, 1), -1)[:, :L], np.zeros((B, L, 128 * H), F)], -1)
            return np.stack([Y[:, :, k * d + 128 * h:k * d + 128 * h + dh] for h in range(H)], 1)
        Va, Vb = off(inp["Yv"], 3, La), off(inp["Yu"], 1, Lb)
    dOh = _heads(inp["dO"].reshape(B, Lq, -1).astype(F), H)
    mq, mka, mkb = inp["mq"], inp["mka"], inp["mkb"]
    La_p, Lb_p = r16(La), r16(Lb)
    Tp, T, nta, nt = La_p + Lb_p, La + Lb, La_p // 16, (La_p + Lb_p) // 16
    scale = scale_of(dh)
    mult = np.asarray(mult, F)
    if defect == "drop_index_T":                   # the multiplier of (row, padded key jp) read at row T + jp of the stream
        flat = np.concatenate([mult.reshape(-1), np.ones(Tp, F)])
        rows = np.arange(B * H * Lq).reshape(B, H, Lq, 1)
        mult = flat[rows * T + np.arange(Tp)]
    pad = lambda x, L, Lp: np.concatenate([x, np.zeros(x.shape[:2] + (Lp - L,) + x.shape[3:], F)], 2)
    Kp, Vp = np.concatenate([pad(Ka, La, La_p), pad(Kb, Lb, Lb_p)], 2), np.concatenate([pad(Va, La, La_p), pad(Vb, Lb, Lb_p)], 2)
    if defect == "block_b_tile_not_rebased":       # block b's tile t read at rows 16 t of block b (past its end: zeros), not 16 (t - nta)
        z = np.zeros((B, H, Lb_p + La_p, dh), F)
        Kb2, Vb2 = z.copy(), z.copy()
        Kb2[:, :, :Lb], Vb2[:, :, :Lb] = Kb, Vb
        Kp, Vp = np.concatenate([Kp[:, :, :La_p], Kb2[:, :, La_p:]], 2), np.concatenate([Vp[:, :, :La_p], Vb2[:, :, La_p:]], 2)
    kflag = np.full((B, Tp), 2, np.uint8)          # 1 valid, 0 masked, 2 pad
    kflag[:, :La], kflag[:, La_p:La_p + Lb] = mka, mkb
    raw = np.concatenate([_mm32(Qa, Kp[:, :, :La_p].transpose(0, 1, 3, 2)), _mm32(Qb, Kp[:, :, La_p:].transpose(0, 1, 3, 2))], -1)
    valid = np.broadcast_to((mq[:, :, None] & (kflag == 1)[:, None, :])[:, None], raw.shape)
    logit = ((np.where(valid, raw, F(FILL)) * mult).astype(F) * scale).astype(F)
    is_pad = np.broadcast_to((kflag == 2)[:, None, None, :], raw.shape).copy()
    if defect == "pad_key_a_in_rowsum":
        is_pad[..., :La_p] = False
    logit = np.where(is_pad, F(-np.inf), logit)
    L2E = F(1.4426950408889634)
    ex = lambda x: np.exp2((x * L2E).astype(F)).astype(F)
    m = np.full((B, H, Lq), -np.inf, F)
    l = np.zeros((B, H, Lq, 4), F)
    o = np.zeros((B, H, Lq, dh), F)
    ntl = nt - 1 if defect == "odd_last_tile_dropped" and nt % 2 == 1 and nt > 1 else nt
    with np.errstate(invalid="ignore"):
        for t in range(ntl):
            lt = logit[..., 16 * t:16 * t + 16]
            tm = lt.max(-1)
            mn = np.maximum(m, tm)
            a = np.zeros_like(m) if t == 0 else ex(m - mn)
            m = tm if defect == "max_follows_lower_tile" else mn
            e = ex(lt - mn[..., None])
            ts, e4 = np.zeros_like(l), e.reshape(e.shape[:-1] + (4, 4))          # [.., lane group, key of the group]
            for r in range(4):
                ts = ts + e4[..., r]
            l = (l * a[..., None]).astype(F) + ts
            if defect != "rescale_l_not_o":
                o = (o * a[..., None]).astype(F)
            Vt = Vp[:, :, 16 * t:16 * t + 16]
            for k in range(16):
                o = o + e[..., k:k + 1] * Vt[:, :, None, k, :]
    ls = (l[..., 0] + l[..., 1]) + (l[..., 2] + l[..., 3])
    inv = (F(1.0) / ls).astype(F)
    Oh = (o * inv[..., None]).astype(F)
    if defect == "p_rel_2^-11":
        Oh = (Oh * F(1 + 2.0 ** -11)).astype(F)
    # backward: P recomputed from the saved statistics, real keys only
    real = np.concatenate([np.arange(La), La_p + np.arange(Lb)]).astype(int)
    lg, mu, vr = logit[..., real], mult[..., real], valid[..., real]
    Pb = (ex(lg - m[..., None]) * inv[..., None]).astype(F)
    if defect == "p_rel_2^-11":
        Pb = (Pb * F(1 + 2.0 ** -11)).astype(F)
    V, K = Vp[:, :, real], Kp[:, :, real]
    dP = _mm32(dOh, V.transpose(0, 1, 3, 2))
    prod = (dOh * Oh).astype(F)
    if d_order == "wide":
        parts = (prod[..., 0::4] + prod[..., 1::4]) + (prod[..., 2::4] + prod[..., 3::4])          # [.., dh / 4]
        npart = dh // 8 if defect == "D_first_partials" else dh // 4
        D = np.zeros(prod.shape[:-1], F)
        for j in range(npart):
            D = D + parts[..., j]
    else:
        idx = _row_frag_index(dh)
        Dg = np.zeros(prod.shape[:-1] + (4,), F)
        for c in range(idx.shape[1]):
            Dg = Dg + prod[..., idx[:, c]]
        D = (Dg[..., 0] + Dg[..., 1]) + (Dg[..., 2] + Dg[..., 3])
    dV = _mm32(Pb.transpose(0, 1, 3, 2), dOh)
    fac = (mu * scale).astype(F)
    dl = np.where(vr & (mu != 0), ((Pb * (dP - D[..., None])).astype(F) * fac).astype(F), F(0))

    def dq_block(dlb, Kb_, n):
        if not passes or n == 0:
            return _mm32(dlb, Kb_)
        ntb_ = (n + 15) // 16
        nw = min(ntb_, passes)
        acc = np.zeros(dlb.shape[:-1] + (dh,), F)
        for ps in range(-(-ntb_ // nw)):
            if ps > 0 and defect == "carry_lost":
                acc = np.zeros_like(acc)
            if ps > 0 and defect == "carry_twice":
                acc = acc + acc
            for w in range(nw):
                t = w if (ps > 0 and defect == "pass2_owns_tile_w") else w + ps * nw
                if w + ps * nw >= ntb_:
                    break
                acc = acc + _mm32(dlb[..., 16 * t:16 * t + 16], Kb_[:, :, 16 * t:16 * t + 16])
        return acc
    dQa, dQb = dq_block(dl[..., :La], K[:, :, :La], La), dq_block(dl[..., La:], K[:, :, La:], Lb)
    dKa, dKb = _mm32(dl[..., :La].transpose(0, 1, 3, 2), Qa), _mm32(dl[..., La:].transpose(0, 1, 3, 2), Qb)
    return dict(O=_unheads(Oh), m=m, inv=inv, D=D, dQa=_unheads(dQa), dQb=_unheads(dQb), dKa=_unheads(dKa), dVa=_unheads(dV[:, :, :La]),
                dKb=_unheads(dKb), dVb=_unheads(dV[:, :, La:]))
