"""The plane-operand GEMMs (segmm_gemm_p: csrc/gemm_planes.h, gemm_planes8.h, gemm_planes4.h, gemm_planes_epi.h, gemm_planes_tn.h,
splitk_reduce of gemm.h) restated on the host: a numpy float64 statement of the NT and TN forms written from the header comments and
the code, a first-order error bound per output element, the counter-based dropout stream of common.h, the rule that says which
kernel and which copy of the epilogue a launch takes (restated from segmm_gemm_p), the two tile maps, fixed-seed cases, an fp32
emulation of the kernel arithmetic and a list of planted defects.  Shared by test_gemm_ref_cpu.py (the yardstick shown sound
without a GPU) and test_gemm_float64_gpu.py.

Operands.  A plane operand IS the float64 number (hi + lo) / s its two fp16 terms hold under the site scale s (p32_ref.split /
unpack); an operand that takes the fp32 fallback (flag up, scale 0: consumer's rule p32_ref.planes_ok) is its fp32 copy split at
p32_ref.exact_scale of its recorded maxima -- what nt_slow_stage / slow_stage do.  Representation error is therefore no part of a
GEMM bound; only the omitted lo lo product is.

The NT statement, in the kernels' order (nt_epilogue, epi_strip_emit), for m < M, n < N:
    v = sum_k a[m, k] b[n, k]
    v *= row_scale[m]                                  (round-2 kernel only)
    v += bias[n]
    GELU:  aux[m, n] = v;  v = gelu(v) = v (1 + erf(v / sqrt 2)) / 2
    dGELU: v *= gelu'(aux[m, n]),  gelu'(x) = (1 + erf(x / sqrt 2)) / 2 + x exp(-x^2 / 2) / sqrt(2 pi)
    ReLU:  v = max(v, 0)           dReLU: v = aux[m, n] > 0 ? v : 0
    v *= mult(m N + n)                                 the dropout multiplier of ELEMENT m N + n (not m ldc + n)
    v += R[m mod res_period if res_period < M else m, n]          accumulate: R = the old C
outputs C[m, n] under ldc, aux under ldaux, planes = p32_ref.pack(fp32 v, c_scale) under ldc2, header hdr[0] = c_scale, hdr[1] per
p32_ref.overflow_flag, max over the AMAX_SLOTS partial maxima = max |v| over the elements that exist.  A REPAIR launch rewrites the
planes at the exact scale of the recorded maxima exactly when p32_ref.planes_ok calls the site unusable, and leaves the header.

The TN statement:  C[m, n] = sum_k A[k, m] B[k, n] (+ old C), colsum[m] = sum_k A[k, m] (+ old colsum), any K > 0 (token tails
are zero-filled by the buffer range check); split-K by the host's rule: ktiles = ceil(K / 32), splits = min(splits, ktiles),
tps = ceil(ktiles / splits), splits = ceil(ktiles / tps), slabs of tps * 32 tokens summed in slab order by splitk_reduce.

The dropout stream (common.h): make_drop quantises p to thresh = round(p 65536) (65535 at most) and rescales by the fp32 number
65536 / (65536 - thresh); the four elements 4 q .. 4 q + 3 of a site draw 16 bits each from (a, b) = drop_rand_quad(q):
k = seed_lo ^ site * 0x9E3779B9 ^ (q >> 32) * 0x85EBCA6B, a = mix32(lo32(q) ^ k), b = mix32(a ^ seed_hi ^ 0x68E31DA4); element e keeps
(multiplier = scale) iff its 16 bits >= thresh, elements 0, 1 from a (low, high half), 2, 3 from b.  A live seed (bit 63 of the seed
argument) XORs the step state's two seed words into (seed_lo, seed_hi).  The ``q >> 32`` word needs an element index of 2^34 or more
(a 64 GiB fp32 tensor): it cannot be reached at test sizes and is restated, not exercised.

Error bounds.  u = 2^-24.  A sum of n terms evaluated in fp32 along any tree whose longest chain of roundings is c has
|computed - exact| <= c u sum|terms| to first order (tests/rowops_ref.py).  Constants, each counted on the code:

* the accumulator: every k-tile of 32 adds the three products ah bl, al bh (bh al in the kernels' operand order), ah bh, each a matrix-core dot
  product of EXACT fp16 x fp16 terms (22 bits) added into the fp32 accumulator.  How an instruction orders its adds is not
  documented, so the chain is taken as the longest possible, one rounding per term:  c_acc = 3 K (NT; the same count for the 16x16x32
  and the 32x32x16 shapes: 32 terms per product and k-tile either way).  TN: c_acc = 3 * (tokens of the longest slab) and, for split-K,
  + (slabs - 1) adds of splitk_reduce, + 1 for accumulate (the old C is a term of the sum).  Column sums: two products (ah 1, al 1)
  per token: c = 2 * (slab tokens) + (slabs - 1) + 1.
* the lo lo omission:  |al bl| summed over k, charged EXACTLY (the statement holds both lo planes); it is at most
  attn_ref.LOLO sum|a b| = 2^-22 sum|a b| (|lo| <= 2^-11 |x s|, tests/p32_ref.py), the form attn_ref._split_terms uses.
* the two multiplications by 1 / sa, 1 / sb:  exact (powers of two, exponents clamped to +-60 by f16_scale_of): 0 roundings.
* row_scale, bias, the dropout multiplier, the residual add:  one rounding each, u |result| (the statement multiplies by the fp32
  number scale itself, so the quantisation of 1 / (1 - p) is no error).  ``c inv_ab + bias`` may contract into one fma: still one.
* erff:  the argument x * 0.70710678f carries the constant's and the product's rounding, 2 u |t| erf'(t); the function is charged
  ERF_ULPS = 4 ulp = 8 u |erf|, the figure of the HIP math API table for erff; 1 + erf one rounding; 0.5 x (.) one more (0.5 x exact).
  Together gelu_eval_err.  Nothing of this was raised after a measurement.
* gelu_erf_grad:  the cdf as above; the pdf 0.39894228f * __expf(-0.5 x x): x x one rounding, u y in the argument (y = x^2 / 2);
  __expf is exp2(arg * log2e): the product and the constant u y each, the exp2 instruction one ulp = 2 u (attn_ref's count
  (3 |x| + 2) u), the constant and its product 2 u:  (3 y + 4) u relative;  x pdf one rounding, cdf + x pdf one.  gelu_grad_eval_err.
* through an activation the incoming error e is carried by the derivative: |gelu'(v)| e + e^2 (|gelu''| < 2 everywhere, so the second
  order is covered, not dropped, where gelu' crosses 0); ReLU is 1-Lipschitz: e; dReLU and dropout SELECT on exact inputs (the aux
  tensor, the integer draw): e or exactly 0 -- nothing is excluded near a discontinuity, the share of unchecked elements is zero.
* GELU, second and tighter check: C against float64 gelu of the aux THE KERNEL WROTE (gelu_eval_err of that fp32 number, then the
  dropout and residual roundings): separates the GEMM error from the activation's.
* planes: bit equality with p32_ref.pack of the fp32 C the kernel wrote; without an fp32 C (planes only, repair) the unpacked
  (hi + lo) / s against float64 under  bound + P32.REL (|v| + bound) + P32.ABS / s,  p32_ref's representation term.
* the recorded maximum: bit equal to max |fp32 C| where C is written; else within the largest element bound of max |v|.
No constant was raised to make a kernel pass.  Measured worst ratios: profiles/gemm_float64/ratios.txt.  Those above one half
(C|aux 0.98, the row_scale form 0.90, TN with K = 1 0.68) are single final roundings held against their own u |result| -- an add
whose result is dominated by the residual or the bias has that rounding as its whole error and almost its whole bound -- and the
fp32 emulation below reaches the same figures; outputs that only pass the accumulator sit at 0.002 - 0.09.

The on-the-fly engines of segmm_gemm (ENGINE_F32, ENGINE_F16X3: the referees of test_planes_gpu.py) are held to the same statement
with their own operand terms; see the section before the emulation.
"""
import numpy as np

import p32_ref as P32
from assemble_ref import mix32
from attn_ref import LOLO, ratio          # noqa: F401  (LOLO: the closed form of the lo lo term, asserted against the exact one)

U = 2.0 ** -24
F = np.float32
M32 = 0xFFFFFFFF
EPI_NONE, EPI_GELU, EPI_DGELU, EPI_RELU, EPI_DRELU = 0, 1, 2, 3, 4
ERF_ULPS = 4
LIVE_SEED = 1 << 63
PBM, PBN, P4_BM, P4_BN, P4_NGROUP = 256, 256, 128, 256, 4
SEED, SITE = 0x1234567_89ABCDEF, 5          # the dropout stream of the GEMM cases (non-zero high word)
STEP_WORDS = 0x0BADC0DE_F00DFACE            # what the live-seed case hands to segmm_step_set


# ------------------------------------------------------------------ the dropout stream (common.h)
def make_drop(p, seed, site, step_seed=0):
    """DropCfg of make_drop(p, seed, site); with bit 63 of ``seed`` set, drop_live's XOR of the step state's seed words (what
    segmm_step_set(step_seed) stored: lo32, hi32 & 0x7fffffff) is applied as well."""
    p = F(p)
    t = float(p) * 65536.0 + 0.5
    thresh = 0 if p <= 0 else (65535 if t >= 65535.0 else int(t))
    scale = F(65536.0 / (65536.0 - thresh)) if p > 0 else F(1.0)
    lo, hi = seed & M32, (seed >> 32) & 0x7FFFFFFF
    if (seed >> 63) & 1:
        lo, hi = lo ^ (step_seed & M32), hi ^ ((step_seed >> 32) & 0x7FFFFFFF)
    return dict(p=p, thresh=thresh, scale=scale, seed_lo=lo, seed_hi=hi, site=site & M32, live=(seed >> 63) & 1)


def drop_rand_quad(d, q):
    """(a, b): the 64 random bits of the quads ``q`` (uint64 array), as uint64 arrays holding 32-bit values"""
    q = np.asarray(q, dtype=np.uint64)
    k = np.uint64(d["seed_lo"] ^ ((d["site"] * 0x9E3779B9) & M32)) ^ (((q >> np.uint64(32)) * np.uint64(0x85EBCA6B)) & np.uint64(M32))
    a = mix32((q & np.uint64(M32)) ^ k)
    b = mix32(a ^ np.uint64(d["seed_hi"] ^ 0x68E31DA4))
    return a, b


def drop_mult(d, elems):
    """fp32 multipliers (0 or scale) of the elements ``elems`` (integer array of element indices) of the site's stream"""
    e = np.asarray(elems, dtype=np.uint64)
    a, b = drop_rand_quad(d, e >> np.uint64(2))
    lane = e & np.uint64(3)
    w = np.where(lane < 2, a, b)
    x = np.where((lane & np.uint64(1)) != 0, w >> np.uint64(16), w & np.uint64(0xFFFF))
    return np.where(x >= np.uint64(d["thresh"]), d["scale"], F(0.0)).astype(F)


def nt_mult(d, M, N, ld=None):
    """multipliers of an [M, N] output: element m N + n (``ld``: a planted other stride)"""
    ld = N if ld is None else ld
    idx = np.arange(M, dtype=np.uint64)[:, None] * np.uint64(ld) + np.arange(N, dtype=np.uint64)[None, :]
    return drop_mult(d, idx)


# ------------------------------------------------------------------ dispatch restated (segmm_gemm_p)
KNOBS = dict(PL_VAR=4, PL_NJ=0, TN_VAR=8)


def _knobs(k):
    out = dict(KNOBS)
    out.update(k or {})
    return out


def nt_fits(L):
    """``fits`` of segmm_gemm_p: the launch can run on the round-3 / round-6 kernels (32-bit epilogue offsets, one extra operand)"""
    lim = 1 << 31
    M = L["M"]
    return (not L.get("row_scale") and M * L["ldc"] * 4 < lim and (not L.get("aux") or M * L["ldaux"] * 4 < lim)
            and (not L.get("residual") or min(L["res_period"], M) * L["ldr"] * 4 < lim)
            and (not L.get("c_planes") or M * L["ldc2"] * 2 < lim)
            and not (L.get("residual") and L["act"] in (EPI_DGELU, EPI_DRELU)))


def nt_nj(M, N, K, ncu=256, nj_knob=0):
    """tile width of gemm_pl_nt8 in 64-column units: the knob, or the cost model (fewest CU-rounds, near-ties to the widest)"""
    if 2 <= nj_knob <= 4:
        return nj_knob
    best, best_cost, bm = 4, 0.0, (M + PBM - 1) // PBM
    for nj in (4, 3, 2):
        tiles = bm * ((N + 64 * nj - 1) // (64 * nj))
        cost = float((tiles + ncu - 1) // ncu) * (15.0 + 11.4 * nj * (K / 768.0))
        if nj == 4 or cost < 0.93 * best_cost:
            best, best_cost = nj, cost
    return best


def nt_kernel(L, knobs=None, ncu=256):
    """The NT kernel of a launch L (dict: M, N, K, ldc, ldaux, ldr, ldc2, res_period, act and the flags row_scale, aux, residual,
    c_planes, repair, b_f32), or an error string starting with '!' where segmm_gemm_p refuses it."""
    k = _knobs(knobs)
    var = k["PL_VAR"]
    if var in (8, 4, 44):
        fits = nt_fits(L)
        if fits and (var == 44 or (var == 4 and L["K"] >= 768 and L["N"] >= 768)):
            return "gemm_pl_nt4"
        if fits:
            return "gemm_pl_nt8<%d>" % nt_nj(L["M"], L["N"], L["K"], ncu, k["PL_NJ"])
    if L.get("repair"):
        return "!repair needs gemm_pl_nt8 / gemm_pl_nt4"
    if L.get("b_f32"):
        return "!the round-2 kernel has no fp32 fallback for B"
    return "gemm_pl_nt"


def nt_tile(kernel):
    return {"gemm_pl_nt4": (P4_BM, P4_BN), "gemm_pl_nt": (PBM, PBN)}.get(kernel) or (PBM, 64 * int(kernel[-2]))


def nt_epilogue_copies(kernel, L, drop, planes_on):
    """The copies of the epilogue the tiles of a launch run: 'fast<E>' / 'fast<>' (nt_epilogue's unrolled loops), 'row<ACT,DROP,PLANES>'
    (its twelve rolled loops) or, on the round-2 kernel, 'strip' with '+row_scale' and '+res+dact' marking the two arms only it has.
    ``planes_on``: a plane output with a scale > 0."""
    if kernel == "gemm_pl_nt":
        tag = "strip"
        if L.get("row_scale"):
            tag += "+row_scale"
        if L.get("residual") and L["act"] in (EPI_DGELU, EPI_DRELU):
            tag += "+res+dact"
        return {tag}
    BM, BN = nt_tile(kernel)
    act = 2 if L["act"] in (EPI_GELU, EPI_DGELU) else 1 if L["act"] in (EPI_RELU, EPI_DRELU) else 0
    has_e = bool(L.get("residual")) or L["act"] in (EPI_DGELU, EPI_DRELU)
    out = set()
    for m0 in range(0, L["M"], BM):
        for n0 in range(0, L["N"], BN):
            full = m0 + BM <= L["M"] and n0 + BN <= L["N"]
            if full and L["act"] == EPI_NONE and not drop and not planes_on:
                out.add("fast<E>" if has_e else "fast<>")
            else:
                out.add("row<%d,%d,%d>" % (act, int(bool(drop)), int(bool(planes_on))))
    return out


def tn_plan(M, N, K, splits, ldc, accumulate, knobs=None):
    """(kernel, slabs, tokens per slab) of a TN launch"""
    k = _knobs(knobs)
    ktiles = (K + 31) // 32
    splits = max(1, min(splits, ktiles))
    residual = False
    if splits > 1:
        tps = (ktiles + splits - 1) // splits
        splits = (ktiles + tps - 1) // tps
    else:
        tps = ktiles
        residual = bool(accumulate)
    small_out = not residual and M * (N if splits > 1 else ldc) * 4 < (1 << 31)
    fits8 = M % PBM == 0 and N % PBN == 0 and small_out
    fits4 = M % P4_BM == 0 and N % P4_BN == 0 and small_out
    few = ((M + PBM - 1) // PBM) * ((N + PBN - 1) // PBN) <= 9 and M >= 768 and N >= 768
    var = k["TN_VAR"]
    tn4 = fits4 and (var == 4 or (var == 8 and (few or not fits8)))
    tn8 = not tn4 and fits8 and var in (8, 88, 4)
    return ("gemm_pl_tn4" if tn4 else "gemm_pl_tn8" if tn8 else "gemm_pl_tn"), splits, tps * 32


def xcd_remap(bid, nwg):
    """common.h: gives every XCD a contiguous chunk of logical workgroup ids"""
    q, r, x = nwg >> 3, nwg & 7, bid & 7
    return (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + (bid >> 3)


def nt4_tile(lb, nbm, nbn, gc=P4_NGROUP):
    """gemm_pl_nt4's grouped tile order: logical id -> (row tile, column tile)"""
    mt, nt = lb // nbn, lb % nbn
    if gc > 0 and nbn > gc:
        gsz = gc * nbm
        g, rem = lb // gsz, lb % gsz
        wdt = min(gc, nbn - g * gc)
        mt = rem // wdt
        nt = g * gc + (rem - mt * wdt)
    return mt, nt


# ------------------------------------------------------------------ operands
STATES = ("exact", "delay3", "delay6", "flag", "never")


def operand(x32, state="exact", site=None):
    """A plane operand of values x32 [R, C] in one of STATES.  ``site``: the fp32 tensor whose maxima the header records (a fused
    buffer the operand is a column slice of; default x32 itself).  Returns hi, lo (fp16, under the scale the KERNEL uses), s (that
    scale), hdr (the site header as the consumer finds it), fallback (the kernel reads the fp32 copy) and val = (hi + lo) / s."""
    x32 = np.asarray(x32, F)
    site = x32 if site is None else np.asarray(site, F)
    amax = P32.amax_of(site)
    se = P32.exact_scale(amax)
    hdr = np.zeros(P32.SITE_FLOATS, F)
    hdr[P32.SITE_HDR:] = P32.slot_fill(site)
    flag = False
    if state == "flag":
        hdr[0], flag = se, True
        hdr.view(np.uint32)[1] = 1
    elif state == "never":
        hdr[0] = 0.0
    else:
        hdr[0] = se / F({"exact": 1, "delay3": 8, "delay6": 64}[state])
    fallback = not P32.planes_ok(amax, hdr[0], flag)
    assert fallback == (state in ("flag", "never")), state
    s = se if fallback else hdr[0]
    hi, lo = P32.split(x32, s)
    val = (hi.astype(np.float64) + lo.astype(np.float64)) / np.float64(s)
    return dict(hi=hi, lo=lo, s=s, hdr=hdr, fallback=fallback, val=val, x32=x32)


def _terms(opA, opB, layout="nt"):
    """(a, b float64 values, sum of |terms| of the three products, exact sum of the omitted |lo lo| terms); NT: [M, K] x [N, K],
    NN: [M, K] x [K, N], TN: [K, M] x [K, N]"""
    sa, sb = np.float64(opA["s"]), np.float64(opB["s"])
    ah, al = opA["hi"].astype(np.float64) / sa, opA["lo"].astype(np.float64) / sa
    bh, bl = opB["hi"].astype(np.float64) / sb, opB["lo"].astype(np.float64) / sb
    if layout == "tn":
        ah, al = ah.T, al.T
    elif layout == "nt":
        bh, bl = bh.T, bl.T
    S = np.abs(ah) @ np.abs(bh) + np.abs(ah) @ np.abs(bl) + np.abs(al) @ np.abs(bh)
    lolo = np.abs(al) @ np.abs(bl)
    assert (lolo <= LOLO * 1.01 * (np.abs(ah + al) @ np.abs(bh + bl)) + 1e-300).all()
    return ah + al, bh + bl, S, lolo


# ------------------------------------------------------------------ activations in float64, and what their fp32 evaluation costs
def _erf(x):
    import torch
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x))).numpy()


def gelu(x):
    return 0.5 * x * (1.0 + _erf(x / np.sqrt(2.0)))


def gelu_grad(x):
    return 0.5 * (1.0 + _erf(x / np.sqrt(2.0))) + x * np.exp(-0.5 * x * x) / np.sqrt(2.0 * np.pi)


def _erf_parts(x):
    t = x / np.sqrt(2.0)
    er = _erf(t)
    e_erf = 2.0 / np.sqrt(np.pi) * np.exp(-t * t) * np.abs(t) * 2 * U + ERF_ULPS * 2 * U * np.abs(er)
    return er, e_erf + U * np.abs(1.0 + er)          # the error of (1 + erff(x * c)) as computed


def gelu_eval_err(x):
    """|gelu_erf(x) in fp32 - gelu(x)| for an exact fp32 x"""
    er, e1 = _erf_parts(x)
    return 0.5 * np.abs(x) * e1 + U * np.abs(0.5 * x * (1.0 + er))


def gelu_grad_eval_err(x):
    er, e1 = _erf_parts(x)
    y = 0.5 * x * x
    xpdf = np.abs(x) * np.exp(-y) / np.sqrt(2.0 * np.pi)
    return 0.5 * e1 + xpdf * (3 * y + 5) * U + U * np.abs(gelu_grad(x))


# ------------------------------------------------------------------ cases
def _f(name, **kw):
    f = dict(name=name, bias=False, res=None, acc=False, act=EPI_NONE, p=0.0, planes=False, write_c=True, hdr_only=False, row_scale=False,
             opa="exact", opb="exact", live=False, repair=None)
    f.update(kw)
    return f


_ACTS = (("none", EPI_NONE), ("relu", EPI_RELU), ("drelu", EPI_DRELU), ("gelu", EPI_GELU), ("dgelu", EPI_DGELU))
NT_FORMS = ([_f("plain"), _f("bias_res_full", bias=True, res="full"), _f("bias_res100_drop", bias=True, res=100, p=0.1),
             _f("bias_res7_drop", bias=True, res=7, p=0.1), _f("accumulate", acc=True)]
            + [_f("%s_p%g%s" % (an, p, "_planes" if pl else ""), bias=True, act=a, p=p, planes=pl)
               for an, a in _ACTS for p in (0.0, 0.1, 0.5) for pl in (False, True)]
            + [_f("gelu_res", bias=True, act=EPI_GELU, res="full"), _f("relu_res100", bias=True, act=EPI_RELU, res=100),
               _f("planes_only", bias=True, planes=True, write_c=False), _f("hdr_only", bias=True, hdr_only=True),
               _f("row_scale", bias=True, row_scale=True), _f("row_scale_gelu_drop_planes", bias=True, row_scale=True, act=EPI_GELU, p=0.1, planes=True),
               _f("res_dgelu", res="full", act=EPI_DGELU), _f("res100_drelu_drop", res=100, act=EPI_DRELU, p=0.1),
               _f("repair_exact", bias=True, planes=True, write_c=False, repair="exact"),
               _f("repair_window", bias=True, planes=True, write_c=False, repair="window"),
               _f("repair_overflow", bias=True, planes=True, write_c=False, repair="overflow"),
               _f("repair_small", bias=True, planes=True, write_c=False, repair="small"),
               _f("live_seed", bias=True, p=0.25, live=True),
               _f("a_flag", bias=True, opa="flag"), _f("b_flag", bias=True, opb="flag"), _f("never", opa="never", opb="never"),
               _f("delay3", bias=True, opa="delay3", opb="exact"), _f("delay6_res", res="full", opa="delay6", opb="delay3")])
NT_SHAPES = [(256, 256, 32), (256, 256, 64), (256, 256, 96), (256, 256, 128), (256, 256, 224), (130, 96, 64), (300, 448, 96), (300, 100, 32),
             (130, 1184, 32), (384, 1312, 32)]
NT_ARMS = (("default", {}), ("nt8<2>", dict(PL_VAR=8, PL_NJ=2)), ("nt8<3>", dict(PL_VAR=8, PL_NJ=3)), ("nt8<4>", dict(PL_VAR=8, PL_NJ=4)),
           ("nt4", dict(PL_VAR=44)), ("round2", dict(PL_VAR=1)))
REPAIR_SHIFT = dict(exact=0, window=-2, overflow=2, small=-17)          # log2 of (first launch's scale / exact scale of max |v|)


def nt_round2_only(form):
    """forms only the round-2 kernel takes, whatever PL_VAR says"""
    return form["row_scale"] or (form["res"] is not None and form["act"] in (EPI_DGELU, EPI_DRELU))


def nt_form_runs(form, shape, arm):
    """Does (form, shape) run under a kernel arm?  Plane outputs need N % 32 == 0 (SEGMM_REQUIRE); the round-2 kernel refuses a repair
    launch and an fp32 fallback for B (SEGMM_REQUIRE); the forms only it takes run under 'default' and 'round2' (under the other arms
    the launch would be the same round-2 launch once more)."""
    M, N, K = shape
    if (form["planes"] or form["repair"]) and N % 32:
        return False
    if nt_round2_only(form):
        return arm in ("default", "round2") and form["opb"] not in ("flag", "never")
    if arm == "round2" and (form["repair"] or form["opb"] in ("flag", "never")):
        return False
    return True


def nt_launch(form, shape):
    """the launch descriptor nt_kernel / nt_epilogue_copies take, with the strides the GPU test uses"""
    M, N, K = shape
    has_res = form["res"] is not None or form["acc"]
    return dict(M=M, N=N, K=K, ldc=N + 32, ldaux=N + 32, ldr=N + 32, ldc2=2 * N + 64,
                res_period=(M if form["acc"] or form["res"] == "full" else form["res"]) if has_res else 1,
                act=form["act"], row_scale=form["row_scale"], aux=form["act"] in (EPI_GELU, EPI_DGELU, EPI_DRELU), residual=has_res,
                c_planes=form["planes"], repair=bool(form["repair"]), b_f32=form["opb"] in ("flag", "never"))


_BASE = {}


def nt_base(shape):
    """fixed-seed inputs of a shape, shared by its forms and never modified"""
    if shape not in _BASE:
        M, N, K = shape
        r = np.random.RandomState(M * 7919 + N * 31 + K)
        A = r.randn(M, K).astype(F)
        A[::7] *= 3.0
        A[M - 1] *= 4.0          # the last row holds the large values: its copies in a ragged tile's masked rows must not reach the maximum
        B = (r.randn(N, K) * 0.1).astype(F)
        aux = r.randn(M, N).astype(F)
        aux[::3, ::5] = 0.0          # dReLU selects on aux > 0: zeros of both signs select nothing
        aux[1::3, ::5] = -0.0
        b = dict(A=A, B=B, bias=r.randn(N).astype(F), res_full=r.randn(M, N).astype(F), res100=r.randn(100, N).astype(F),
                 res7=r.randn(7, N).astype(F), aux=aux, cold=r.randn(M, N).astype(F), rs=(r.rand(M) * 1.5 - 0.5).astype(F))
        for v in b.values():
            v.setflags(write=False)
        _BASE[shape] = b
    return _BASE[shape]


_OPS = {}


def nt_operands(shape, form):
    key = (shape, form["opa"], form["opb"])
    if key not in _OPS:
        b = nt_base(shape)
        _OPS[key] = (operand(b["A"], form["opa"]), operand(b["B"], form["opb"]))
    return _OPS[key]


def nt_residual(form, shape):
    """(R as [M, N] rows already wrapped, the stored residual array or None)"""
    b, M = nt_base(shape), shape[0]
    if form["acc"]:
        return b["cold"], b["cold"]
    if form["res"] is None:
        return None, None
    R = b["res_full"] if form["res"] == "full" else b["res%d" % form["res"]]
    rows = np.arange(M) % R.shape[0] if R.shape[0] < M else np.arange(M)
    return R[rows], R


def nt_drop(form):
    if form["p"] <= 0:
        return None
    return make_drop(form["p"], SEED | (LIVE_SEED if form["live"] else 0), SITE, STEP_WORDS)


# ------------------------------------------------------------------ the float64 statement with its bounds
def _tail(v, e, mult, R):
    if mult is not None:
        v = v * mult
        e = e * mult + U * np.abs(v)
    if R is not None:
        v = v + R
        e = e + U * np.abs(v)
    return v, e


def nt_reference(form, shape, engine="planes"):
    """dict: C, bC (value and bound of the output element), aux, baux (GELU's pre-activation), mult, R, c_scale (the scale the GPU
    test and the emulation hand to a plane output: half the exact scale of max |C|; a repair form: shifted by REPAIR_SHIFT).
    ``engine``: 'planes' (segmm_gemm_p; the on-the-fly fp16x3 engine of segmm_gemm is the same statement on operands in state
    'exact': it splits the fp32 operands at the exact scale of their maxima) or 'f32' (segmm_gemm's fp32 matrix-core engine: the
    operands are the fp32 numbers, nothing is omitted, every product is rounded: c_acc = K + 1)."""
    M, N, K = shape
    b = nt_base(shape)
    if engine == "f32":
        a, bb = b["A"].astype(np.float64), b["B"].astype(np.float64).T
        v = a @ bb
        e = (K + 1) * U * (np.abs(a) @ np.abs(bb))
    else:
        opA, opB = nt_operands(shape, form)
        a, bb, S, lolo = _terms(opA, opB)
        v = a @ bb
        e = 3 * K * U * S + lolo
    if form["row_scale"]:
        rs = b["rs"].astype(np.float64)[:, None]
        v = v * rs
        e = e * np.abs(rs) + U * np.abs(v)
    if form["bias"]:
        v = v + b["bias"].astype(np.float64)[None, :]
        e = e + U * np.abs(v)
    aux = baux = None
    act = form["act"]
    auxin = b["aux"].astype(np.float64)
    if act == EPI_GELU:
        aux, baux = v, e
        e = np.abs(gelu_grad(v)) * e + e * e + gelu_eval_err(v)
        v = gelu(v)
    elif act == EPI_DGELU:
        gp = gelu_grad(auxin)
        e = np.abs(gp) * e + np.abs(v) * gelu_grad_eval_err(auxin)
        v = v * gp
        e = e + U * np.abs(v)
    elif act == EPI_RELU:
        v = np.maximum(v, 0.0)
    elif act == EPI_DRELU:
        sel = b["aux"] > 0
        v, e = np.where(sel, v, 0.0), np.where(sel, e, 0.0)
    d = nt_drop(form)
    mult = None if d is None else nt_mult(d, M, N).astype(np.float64)
    R, _ = nt_residual(form, shape)
    v, e = _tail(v, e, mult, None if R is None else R.astype(np.float64))
    se = P32.exact_scale(F(np.abs(v).max()))
    c_scale = F(se * F(2.0 ** REPAIR_SHIFT[form["repair"]])) if form["repair"] else F(se / F(2.0))
    return dict(C=v, bC=e, aux=aux, baux=baux, mult=mult, R=R, c_scale=c_scale)


def gelu_second_check(form, ref, aux32):
    """(value, bound) of C given the fp32 pre-activations the kernel wrote"""
    x = np.asarray(aux32, np.float64)
    return _tail(gelu(x), gelu_eval_err(x), ref["mult"], None if ref["R"] is None else ref["R"].astype(np.float64))


def judge_nt(form, ref, got):
    """``got``: C, aux (fp32 [M, N] or None), hi, lo (fp16 [M, N] unpacked from the plane region, or None), hdr (the site header after
    the launch, or None), for a repair form also hdr0 / hi0 / lo0 (header and planes after the FIRST launch) and C32 (the fp32 result
    of the same arithmetic with an fp32 C).  Returns (ratios: output -> worst error / bound, exact: name -> bool)."""
    ratios, exact = {}, {}
    C, bC = ref["C"], ref["bC"]
    s = ref["c_scale"]
    if got.get("C") is not None:
        ratios["C"] = ratio(got["C"], C, bC)
    if ref["aux"] is not None:
        ratios["aux"] = ratio(got["aux"], ref["aux"], ref["baux"])
        if got.get("C") is not None:
            want, bound = gelu_second_check(form, ref, got["aux"])
            ratios["C|aux"] = ratio(got["C"], want, bound)
    hdr = got.get("hdr")
    amax = flag = None
    if hdr is not None:
        amax = F(np.fmax.reduce(hdr[P32.SITE_HDR:]))
        flag = bool(hdr.view(np.uint32)[1] != 0)
        if got.get("C") is not None:
            exact["amax"] = bool(amax == np.abs(got["C"]).max())
        else:
            ratios["amax"] = ratio(amax, np.abs(C).max(), bC.max())
    if form["hdr_only"]:
        exact["hdr_untouched"] = bool(hdr[0] == 0 and not flag)
    if form["planes"]:
        exact["hdr_scale"] = bool(hdr[0] == s)
        exact["hdr_flag"] = flag == (not bool(amax * s < P32.F16_MAX))
        s_used = s
        if form["repair"]:
            unusable = not P32.planes_ok(amax, s, flag)
            exact["repair_verdict"] = unusable == (form["repair"] in ("overflow", "small"))
            exact["repair_header_kept"] = bool(np.array_equal(hdr.view(np.uint32), got["hdr0"].view(np.uint32)))
            if unusable:
                s_used = P32.exact_scale(amax)
                h, l = P32.split(got["C32"], s_used)
                exact["repair_rewritten"] = _same16(h, got["hi"]) and _same16(l, got["lo"])
            else:
                exact["repair_left_alone"] = _same16(got["hi0"], got["hi"]) and _same16(got["lo0"], got["lo"])
        if got.get("C") is not None:
            h, l = P32.split(got["C"], s)
            exact["planes"] = _same16(h, got["hi"]) and _same16(l, got["lo"])
        else:
            val = (got["hi"].astype(np.float64) + got["lo"].astype(np.float64)) / np.float64(s_used)
            ratios["planes"] = ratio(val, C, bC + P32.REL * (np.abs(C) + bC) + P32.ABS / np.float64(s_used))
    return ratios, exact


def _same16(a, b):
    return bool(np.array_equal(np.asarray(a).view(np.uint16), np.asarray(b).view(np.uint16)))


# ------------------------------------------------------------------ TN
TN_SHAPES = ([(256, 256, K) for K in (1, 8, 40, 200, 203)] + [(128, 256, K) for K in (1, 8, 40, 200, 203)]
             + [(256, 512, 40), (96, 64, 300), (32, 32, 8), (160, 288, 72)])
TN_ARMS = (("default", {}), ("tn4", dict(TN_VAR=4)), ("tn8", dict(TN_VAR=88)), ("round2", dict(TN_VAR=0)))
TN_FORMS = [dict(name="plain", acc=False, colsum=False, opa="exact", opb="exact"), dict(name="accumulate", acc=True, colsum=False, opa="exact", opb="exact"),
            dict(name="colsum", acc=False, colsum=True, opa="exact", opb="exact"), dict(name="colsum_acc", acc=True, colsum=True, opa="exact", opb="exact"),
            dict(name="a_flag_colsum", acc=False, colsum=True, opa="flag", opb="exact"), dict(name="never", acc=False, colsum=False, opa="never", opb="never")]


def tn_splits(K):
    """the split counts of a shape: 1, 2, 3 and one above the k-tile count, without those the host's rule maps to the same slabs"""
    ktiles, out, seen = (K + 31) // 32, [], set()
    for s in (1, 2, 3, ktiles + 1):
        plan = tn_plan(256, 256, K, s, 256, False)[1:]
        if plan not in seen:
            seen.add(plan)
            out.append(s)
    return out


def tn_base(shape):
    key = ("tn",) + shape
    if key not in _BASE:
        M, N, K = shape
        r = np.random.RandomState(M * 7919 + N * 31 + K + 1)
        A3 = (r.randn(K, 3 * M) * 0.01).astype(F)          # the fused [K][3 M] buffer; operand A is its middle third
        Bm = r.randn(K, N).astype(F)
        b = dict(A3=A3, A=np.ascontiguousarray(A3[:, M:2 * M]), B=Bm, cold=r.randn(M, N).astype(F), csold=r.randn(M).astype(F))
        for v in b.values():
            v.setflags(write=False)
        _BASE[key] = b
    return _BASE[key]


def tn_operands(shape, form):
    key = ("tn", shape, form["opa"], form["opb"])
    if key not in _OPS:
        b = tn_base(shape)
        _OPS[key] = (operand(b["A"], form["opa"], site=b["A3"]), operand(b["B"], form["opb"]))
    return _OPS[key]


def tn_reference(form, shape, splits):
    M, N, K = shape
    b = tn_base(shape)
    opA, opB = tn_operands(shape, form)
    a, bb, S, lolo = _terms(opA, opB, "tn")
    _, slabs, slab_tokens = tn_plan(M, N, K, splits, N + 32, form["acc"])
    n_tok = min(slab_tokens, K)
    C = a @ bb
    absC = S
    if form["acc"]:
        C = C + b["cold"]
        absC = absC + np.abs(b["cold"])
    bC = (3 * n_tok + (slabs - 1) + 1) * U * absC + lolo
    sa = np.float64(opA["s"])
    csh, csl = opA["hi"].astype(np.float64) / sa, opA["lo"].astype(np.float64) / sa
    cs = (csh + csl).sum(0)
    abscs = np.abs(csh).sum(0) + np.abs(csl).sum(0)
    if form["acc"]:
        cs = cs + b["csold"]
        abscs = abscs + np.abs(b["csold"])
    bcs = (2 * n_tok + (slabs - 1) + 1) * U * abscs
    return dict(C=C, bC=bC, colsum=cs, bcolsum=bcs)


def judge_tn(form, ref, got):
    r = {"C": ratio(got["C"], ref["C"], ref["bC"])}
    if form["colsum"]:
        r["colsum"] = ratio(got["colsum"], ref["colsum"], ref["bcolsum"])
    return r, {}


# ------------------------------------------------------------------ the on-the-fly engines of segmm_gemm (gemm.h, gemm_split.h)
# Same epilogue order (row_scale, bias, activation, dropout of element m N + n, residual row m mod res_period), tile 128 x 128 x 32,
# split-K by the same host rule.  ENGINE_F16X3 splits the fp32 operands itself at f16_scale_of of their maxima (= p32_ref.exact_scale)
# and adds lo hi + hi lo + hi hi per k16 step: the plane statement on operands in state 'exact'.  ENGINE_F32 multiplies the fp32
# numbers on v_mfma_f32_32x32x2_f32: c_acc = tokens + 1 (attn_ref.c_dot: every product rounded, every add).
ONFLY_ENGINES = ("f32", "f16x3")
ONFLY_NT_SHAPES = [(130, 96, 64), (300, 448, 96)]
ONFLY_FORMS = [f for f in NT_FORMS if not (f["planes"] or f["hdr_only"] or f["repair"]) and f["opa"] == "exact" and f["opb"] == "exact"]
ONFLY_PLAIN = (96, 48, 360)          # NN and TN, splits 1 and 2: a token tail (360 = 11 k-tiles + 8), one column tile narrower than 128


def plain_inputs(layout):
    key = ("plain", layout)
    if key not in _BASE:
        M, N, K = ONFLY_PLAIN
        r = np.random.RandomState(17 if layout == "nn" else 18)
        A = r.randn(*((M, K) if layout == "nn" else (K, M))).astype(F)
        A[::5] *= 3.0
        Bm = (r.randn(K, N) * 0.1).astype(F)
        A.setflags(write=False)
        Bm.setflags(write=False)
        _BASE[key] = (A, Bm)
    return _BASE[key]


def plain_plan(splits):
    ktiles = (ONFLY_PLAIN[2] + 31) // 32
    splits = max(1, min(splits, ktiles))
    tps = (ktiles + splits - 1) // splits
    return (ktiles + tps - 1) // tps, tps * 32


def plain_reference(layout, engine, splits):
    """C = A B (NN) or A^T B (TN) without an epilogue: (value, bound)"""
    M, N, K = ONFLY_PLAIN
    A, Bm = plain_inputs(layout)
    slabs, tok = plain_plan(splits)
    tok = min(tok, K)
    if engine == "f32":
        a, bb = A.astype(np.float64), Bm.astype(np.float64)
        a = a.T if layout == "tn" else a
        return a @ bb, (tok + 1 + (slabs - 1)) * U * (np.abs(a) @ np.abs(bb))
    a, bb, S, lolo = _terms(operand(A), operand(Bm), layout)
    return a @ bb, (3 * tok + (slabs - 1)) * U * S + lolo


def emulate_plain(layout, engine, splits):
    M, N, K = ONFLY_PLAIN
    A, Bm = plain_inputs(layout)
    slabs, tok = plain_plan(splits)
    C = None
    opA, opB = operand(A), operand(Bm)
    f = lambda x: x.astype(F)
    tr = (lambda x: x.T) if layout == "tn" else (lambda x: x)
    for z in range(slabs):
        k0, k1 = z * tok, min(K, (z + 1) * tok)
        if engine == "f32":
            part = tr(A)[:, k0:k1] @ Bm[k0:k1]
        else:
            part = _acc32(tr(f(opA["hi"])), tr(f(opA["lo"])), f(opB["hi"]), f(opB["lo"]), k0, k1, None) * (F(1.0) / opA["s"]) * (F(1.0) / opB["s"])
        C = part if C is None else (C + part).astype(F)
    return C


# ------------------------------------------------------------------ fp32 emulation of the kernel arithmetic, with planted defects
NT_DEFECTS = ("bias_after_activation", "residual_row_not_wrapped", "dropout_index_with_ldc", "dropout_after_residual", "aux_holds_post_activation",
              "dgelu_reads_c", "accumulate_ignored", "last_ktile_dropped", "hi_lo_dropped", "lo_hi_dropped", "tanh_gelu", "wrong_pdf_constant",
              "block4x4_transposed", "row_scale_after_bias", "plane_scale_x2", "planes_swapped", "amax_over_masked_rows", "flag_not_raised")
TN_DEFECTS = ("colsum_misses_token_tail", "slab_not_summed", "accumulate_ignored", "last_ktile_dropped", "hi_lo_dropped", "lo_hi_dropped")
DEFECTS = NT_DEFECTS + tuple(d for d in TN_DEFECTS if d not in NT_DEFECTS)


def _acc32(ah, al, bh, bl, k0, k1, defect):
    """fp32 accumulator over the k32 blocks of [k0, k1): al bh + ah bl + ah bh per block, the kernels' order; operands [rows, K] / [K, cols]"""
    acc = np.zeros((ah.shape[0], bh.shape[1]), F)
    blocks = list(range(k0, k1, 32))
    if defect == "last_ktile_dropped":
        blocks = blocks[:-1]
    for k in blocks:
        sl = slice(k, min(k + 32, k1))
        if defect != "lo_hi_dropped":
            acc = acc + al[:, sl] @ bh[sl]
        if defect != "hi_lo_dropped":
            acc = acc + ah[:, sl] @ bl[sl]
        acc = acc + ah[:, sl] @ bh[sl]
    return acc


def _erf32(x):
    return _erf(np.asarray(x, F)).astype(F)


def _gelu32(x, defect=None):
    if defect == "tanh_gelu":
        return F(0.5) * x * (F(1.0) + np.tanh(F(0.7978845608) * (x + F(0.044715) * x * x * x)).astype(F))
    return F(0.5) * x * (F(1.0) + _erf32(x * F(0.70710678118654752)))


def _gelu_grad32(x, defect=None):
    cdf = F(0.5) * (F(1.0) + _erf32(x * F(0.70710678118654752)))
    c = F(0.79788456080286536) if defect == "wrong_pdf_constant" else F(0.39894228040143268)
    return cdf + x * (c * np.exp(F(-0.5) * x * x).astype(F))


def emulate_nt(form, shape, ref, defect=None, engine="planes"):
    """The launch (for a repair form: first launch + repair launch) in numpy fp32.  Returns the ``got`` dict judge_nt takes."""
    M, N, K = shape
    b = nt_base(shape)
    opA, opB = nt_operands(shape, form)
    f = lambda x: x.astype(F)
    if engine == "f32":
        v = b["A"] @ b["B"].T
    else:
        acc = _acc32(f(opA["hi"]), f(opA["lo"]), f(opB["hi"]).T, f(opB["lo"]).T, 0, K, defect)
        v = acc * (F(1.0) / opA["s"]) * (F(1.0) / opB["s"])
    bias = b["bias"][None, :] if form["bias"] else F(0.0)
    rs = b["rs"][:, None]
    late_bias = defect == "bias_after_activation" and form["act"] != EPI_NONE
    if form["row_scale"] and defect != "row_scale_after_bias":
        v = v * rs
    if not late_bias:
        v = v + bias
    if form["row_scale"] and defect == "row_scale_after_bias":
        v = v * rs
    act, aux = form["act"], None
    if act == EPI_GELU:
        aux = v
        v = _gelu32(v, defect)
        if defect == "aux_holds_post_activation":
            aux = v
    elif act == EPI_DGELU:
        v = v * _gelu_grad32(v if defect == "dgelu_reads_c" else b["aux"], defect)
    elif act == EPI_RELU:
        v = np.maximum(v, F(0.0))
    elif act == EPI_DRELU:
        v = np.where(b["aux"] > 0, v, F(0.0))
    if late_bias:
        v = v + bias
    v = v.astype(F)
    d = nt_drop(form)
    mult = None if d is None else nt_mult(d, M, N, ld=N + 32 if defect == "dropout_index_with_ldc" else None)
    R, Rstore = nt_residual(form, shape)
    if R is not None and defect == "residual_row_not_wrapped" and Rstore.shape[0] < M:
        R = np.zeros((M, N), F)          # rows beyond the stored ones are outside the buffer view: they read as 0
        R[:Rstore.shape[0]] = Rstore
    if form["acc"] and defect == "accumulate_ignored":
        R = None
    ghost = v[M - 1:M] if mult is None else v[M - 1:M] * d["scale"]          # the last row once more, kept by some masked row's draw
    if defect == "dropout_after_residual" and mult is not None and R is not None:
        v = ((v + R).astype(F) * mult).astype(F)
    else:
        if mult is not None:
            v = (v * mult).astype(F)
        if R is not None:
            v = (v + R).astype(F)
    if defect == "block4x4_transposed" and M >= 24 and N >= 40:
        v = v.copy()
        v[16:20, 32:36] = v[16:20, 32:36].T.copy()
    got = dict(C=v if form["write_c"] else None, aux=aux, hi=None, lo=None, hdr=None)
    amax = F(np.abs(v).max())
    if defect == "amax_over_masked_rows" and M % 128:
        amax = max(amax, F(np.abs(ghost).max()))
    if form["planes"] or form["hdr_only"]:
        hdr = np.zeros(P32.SITE_FLOATS, F)
        hdr[P32.SITE_HDR] = amax
        got["hdr"] = hdr
    if form["planes"]:
        s = ref["c_scale"]
        hdr[0] = s
        flag = not bool(amax * s < P32.F16_MAX) and defect != "flag_not_raised"
        hdr.view(np.uint32)[1] = int(flag)
        sw = F(2.0) * s if defect == "plane_scale_x2" else s
        hi, lo = P32.split(v, sw)
        if form["repair"]:
            got.update(hdr0=hdr.copy(), hi0=hi, lo0=lo, C32=v)
            if not P32.planes_ok(amax, s, flag):
                se = P32.exact_scale(amax)
                hi, lo = P32.split(v, F(2.0) * se if defect == "plane_scale_x2" else se)
        got["hi"], got["lo"] = (lo, hi) if defect == "planes_swapped" else (hi, lo)
    return got


def emulate_tn(form, shape, splits, defect=None):
    M, N, K = shape
    b = tn_base(shape)
    opA, opB = tn_operands(shape, form)
    f = lambda x: x.astype(F)
    ah, al, bh, bl = f(opA["hi"]).T, f(opA["lo"]).T, f(opB["hi"]), f(opB["lo"])
    _, slabs, slab_tokens = tn_plan(M, N, K, splits, N + 32, form["acc"])
    inv_a = F(1.0) / opA["s"]
    inv_ab = inv_a * (F(1.0) / opB["s"])
    C = cs = None
    for z in range(slabs):
        k0, k1 = z * slab_tokens, min(K, (z + 1) * slab_tokens)
        if defect == "slab_not_summed" and slabs > 1 and z == slabs - 1:
            continue
        part = _acc32(ah, al, bh, bl, k0, k1, defect) * inv_ab
        kc = k0 + 32 * ((k1 - k0) // 32) if defect == "colsum_misses_token_tail" and z == slabs - 1 else k1
        pcs = np.zeros(M, F)
        for k in range(k0, kc, 32):          # the column sums: al . 1 + ah . 1 per k32 block
            sl = slice(k, min(k + 32, kc))
            pcs = pcs + al[:, sl].sum(1, dtype=F)
            pcs = pcs + ah[:, sl].sum(1, dtype=F)
        pcs = pcs * inv_a
        C = part if C is None else (C + part).astype(F)
        cs = pcs if cs is None else (cs + pcs).astype(F)
    if form["acc"] and defect != "accumulate_ignored":
        C, cs = (C + b["cold"]).astype(F), (cs + b["csold"]).astype(F)
    return dict(C=C, colsum=cs if form["colsum"] else None)


def rejected(ratios, exact):
    return any(not (r <= 1.0) for r in ratios.values()) or not all(exact.values())
