"""The ONE-PRODUCT plane GEMMs (segmm_gemm_pq with products = 1: gemm_pl_nt4<1>, gemm_pl_nt8<NJ, 1>, gemm_pl_tn4<1>, gemm_pl_tn8<1>)
restated on the host, on top of tests/gemm_ref.py and tests/p32_ref.py.  Nothing those two state is declared again: the dispatch
rule, the operand states, the dropout stream, the epilogue statement with its constants, the split-K plan, the judges and the
fixed-seed inputs are theirs.  Shared by test_gemm1_ref_cpu.py (the yardstick shown sound without a GPU) and test_gemm1_gpu.py.

Operands.  With one product an operand IS the float64 number hi / s: the fp16 rounding of x s, divided by the power of two s.  For
an operand that takes the fp32 fallback, hi is that of p32_ref.split at p32_ref.exact_scale of the recorded maxima (what
nt_slow_stage / tn_image_put stage; the kernel then multiplies with the same one-product mma).  That hi / s differs from x by up
to 2^-11 |x| is the user's trade and no part of a bound: the statement is about hi / s, so only evaluation error is left.

The statement.
    NT:  v[m, n] = sum_k a_hi[m, k] b_hi[n, k] / (s_a s_b),   then gemm_ref's epilogue statement, unchanged
    TN:  C[m, n] = sum_k a_hi[k, m] b_hi[k, n] / (s_a s_b) (+ old C) under gemm_ref.tn_plan's slabs;
         colsum[m] = sum_k a_hi[k, m] / s_a (+ old colsum)

Error bound: gemm_ref's, with two changes and no other.
  * The accumulator chain is counted at ONE product per term: c_acc = K (NT); (tokens of the longest slab) + (slabs - 1) +
    (1 if accumulate) for TN.  The column sums take one product (a_hi . 1) per token: the same count.
    (gemm_ref charges the TN forms "+ 1" whether or not the old C is a term; here the add is counted only where it happens, as the
    count above says.  At K = 1 without accumulate the bound is then u |a b| for a product that is exact in fp32: still sound.)
  * There is no lo lo term: nothing of the stated sum is omitted.
  Every epilogue constant is gemm_ref's; none is raised.

How gemm_ref's epilogue statement is reached without restating it.  gemm_ref.nt_reference takes its operand terms from
gemm_ref._terms and charges ``3 K u S + lolo``; gemm_ref.emulate_nt takes its accumulator from gemm_ref._acc32.  Under
``one_product()`` those two names are replaced, for the duration of the call, by the one-product operand terms (a_hi, b_hi, S / 3,
lolo = 0 -- so that the line reads K u S with S = sum |a_hi b_hi|; the division by three and the multiplication that undoes it cost
2^-53 relative) and the one-product accumulator.  Everything downstream -- bias, activation, dropout, residual, planes, header,
repair -- is then gemm_ref's own code on the one-product sum.  The TN statement has no epilogue and is written out here.

Why a launch that silently ran three products cannot pass at the test's shapes: the cross terms hi lo + lo hi it would add are about
2^-12.5 sqrt(2 K) of the products' RMS, the bound K 2^-24 of their absolute sum over K terms: worst element / bound ~ 2^12 / K^1.5
times a few sigma -- 177 at K = 32 down to 10 at K = 224 (test_gemm1_ref_cpu.py measures and asserts it at every shape).  Conversely
the one-product result fails gemm_ref's three-product bound (58 .. 3.4): at these widths the two statements cannot be confused.  The
margin shrinks as K^-1.5 (a worst-case chain bound against a random-sign error); it is of order one near K = 768, which no case uses.
"""
import contextlib

import numpy as np

import gemm_ref as G
import p32_ref as P32          # noqa: F401  (the operand format of the statement: hi is p32_ref.split's)

U, F = G.U, G.F

# ------------------------------------------------------------------ cases (test_gemm1_gpu.py)
NT_ARMS = (("nt4", dict(PL_VAR=44)), ("nt8<2>", dict(PL_VAR=8, PL_NJ=2)), ("nt8<3>", dict(PL_VAR=8, PL_NJ=3)), ("nt8<4>", dict(PL_VAR=8, PL_NJ=4)))
TN_ARMS = (("tn4", dict(TN_VAR=4)), ("tn8", dict(TN_VAR=88)))
# the smallest shapes at which the k-loops can still go wrong: the one-tile prologue with its zero-length requests (K = 32), two and
# three k-tiles, a full rotation of gemm_pl_nt4's three half-slots plus one (K = 128), seven k-tiles, a row tail with a narrow column
# tile, two row tiles with a tail and a second column tile of 192
NT_SHAPES = [(256, 256, 32), (256, 256, 64), (256, 256, 96), (256, 256, 128), (256, 256, 224), (130, 96, 64), (300, 448, 96)]
NT_FORMS = ([G._f("plain"), G._f("bias_gelu", bias=True, act=G.EPI_GELU), G._f("dgelu", bias=True, act=G.EPI_DGELU),
             G._f("bias_res100_drop_live", bias=True, res=100, p=0.1, live=True), G._f("accumulate", acc=True),
             G._f("planes", bias=True, planes=True)]
            + [G._f("repair_" + r, bias=True, planes=True, write_c=False, repair=r) for r in G.REPAIR_SHIFT]
            + [G._f("a_delay3", bias=True, opa="delay3"), G._f("b_delay3", bias=True, opb="delay3"),
               G._f("a_flag", bias=True, opa="flag"), G._f("b_flag", bias=True, opb="flag")])
# a form only the round-2 kernel takes, whatever the arm: held to the THREE-product statement (segmm_gemm_pq: products does not reach it)
NT_ROUND2_FORM = G._f("row_scale", bias=True, row_scale=True)
TN_SHAPES = [s for s in G.TN_SHAPES if s[:2] in ((256, 256), (128, 256)) and s[2] in (1, 8, 40, 200, 203)]
TN_FORMS = [f for f in G.TN_FORMS if f["name"] in ("plain", "accumulate", "colsum", "colsum_acc", "a_flag_colsum")]


def tn_splits(K):
    """split counts of a TN shape: 1 and gemm_ref.tn_splits(K), each once"""
    out = [1]
    for s in G.tn_splits(K):
        if s not in out:
            out.append(s)
    return out


# ------------------------------------------------------------------ the one-product terms and accumulator
DEFECTS = ("ran_three_products", "lo_of_a_added", "lo_of_b_added", "colsum_kept_lo", "last_ktile_dropped")


def _hi(op):
    return op["hi"].astype(np.float64) / np.float64(op["s"])


def _terms1(opA, opB, layout="nt"):
    """gemm_ref._terms for one product: (a_hi, b_hi, sum |a_hi b_hi| / 3, 0) -- see the module text for the 3"""
    a, b = _hi(opA), _hi(opB)
    if layout == "tn":
        a = a.T
    elif layout == "nt":
        b = b.T
    return a, b, (np.abs(a) @ np.abs(b)) / 3.0, np.zeros((a.shape[0], b.shape[1]))


def _acc32_1(ah, al, bh, bl, k0, k1, defect):
    """gemm_ref._acc32 for one product: ah bh per k32 block into the fp32 accumulator; the planted defects add what must not be there"""
    acc = np.zeros((ah.shape[0], bh.shape[1]), F)
    blocks = list(range(k0, k1, 32))
    if defect == "last_ktile_dropped":
        blocks = blocks[:-1]
    for k in blocks:
        sl = slice(k, min(k + 32, k1))
        if defect in ("ran_three_products", "lo_of_a_added"):
            acc = acc + al[:, sl] @ bh[sl]
        if defect in ("ran_three_products", "lo_of_b_added"):
            acc = acc + ah[:, sl] @ bl[sl]
        acc = acc + ah[:, sl] @ bh[sl]
    return acc


@contextlib.contextmanager
def one_product():
    """gemm_ref's reference and emulation on the one-product terms and accumulator (module text); restored on exit"""
    terms, acc = G._terms, G._acc32
    G._terms, G._acc32 = _terms1, _acc32_1
    try:
        yield
    finally:
        G._terms, G._acc32 = terms, acc


# ------------------------------------------------------------------ NT
def nt_reference(form, shape):
    """gemm_ref.nt_reference's dict for the one-product statement: the accumulator charged K u sum |a_hi b_hi|, nothing omitted,
    gemm_ref's epilogue statement and constants"""
    with one_product():
        return G.nt_reference(form, shape)


def emulate_nt(form, shape, ref, defect=None):
    """the launch in numpy fp32 with the one-product accumulator and gemm_ref's epilogue emulation"""
    with one_product():
        return G.emulate_nt(form, shape, ref, defect)


judge_nt = G.judge_nt


# ------------------------------------------------------------------ TN
def tn_reference(form, shape, splits):
    M, N, K = shape
    b = G.tn_base(shape)
    opA, opB = G.tn_operands(shape, form)
    a, bb = _hi(opA).T, _hi(opB)
    _, slabs, slab_tokens = G.tn_plan(M, N, K, splits, N + 32, form["acc"])
    chain = min(slab_tokens, K) + (slabs - 1) + int(bool(form["acc"]))
    C, absC = a @ bb, np.abs(a) @ np.abs(bb)
    cs, abscs = a.sum(1), np.abs(a).sum(1)
    if form["acc"]:
        C, absC = C + b["cold"], absC + np.abs(b["cold"])
        cs, abscs = cs + b["csold"], abscs + np.abs(b["csold"])
    return dict(C=C, bC=chain * U * absC, colsum=cs, bcolsum=chain * U * abscs)


def emulate_tn(form, shape, splits, defect=None):
    """gemm_ref.emulate_tn's arithmetic with one product per k32 block and the column sums a_hi . 1"""
    M, N, K = shape
    b = G.tn_base(shape)
    opA, opB = G.tn_operands(shape, form)
    f = lambda x: x.astype(F)
    ah, al, bh, bl = f(opA["hi"]).T, f(opA["lo"]).T, f(opB["hi"]), f(opB["lo"])
    _, slabs, slab_tokens = G.tn_plan(M, N, K, splits, N + 32, form["acc"])
    inv_a = F(1.0) / opA["s"]
    inv_ab = inv_a * (F(1.0) / opB["s"])
    C = cs = None
    for z in range(slabs):
        k0, k1 = z * slab_tokens, min(K, (z + 1) * slab_tokens)
        part = _acc32_1(ah, al, bh, bl, k0, k1, defect) * inv_ab
        pcs = np.zeros(M, F)
        for k in range(k0, k1, 32):
            sl = slice(k, min(k + 32, k1))
            if defect in ("colsum_kept_lo", "ran_three_products"):
                pcs = pcs + al[:, sl].sum(1, dtype=F)
            pcs = pcs + ah[:, sl].sum(1, dtype=F)
        pcs = pcs * inv_a
        C = part if C is None else (C + part).astype(F)
        cs = pcs if cs is None else (cs + pcs).astype(F)
    if form["acc"]:
        C, cs = (C + b["cold"]).astype(F), (cs + b["csold"]).astype(F)
    return dict(C=C, colsum=cs if form["colsum"] else None)


judge_tn = G.judge_tn
rejected = G.rejected
