"""The plane-operand GEMMs (segmm_gemm_p: gemm_pl_nt8<2|3|4>, gemm_pl_nt4, gemm_pl_nt, gemm_pl_tn4, gemm_pl_tn8, gemm_pl_tn,
splitk_reduce, the fourteen copies of nt_epilogue) against the float64 statement of tests/gemm_ref.py: every output element under the
first-order bound derived there (error / bound <= 1), bit equality where the statement says so (planes against p32_ref.pack of
the fp32 C the kernel wrote, header words, dropout masks, untouched margins).  No tolerance is a constant chosen in advance.

Buffers.  Every output goes into a buffer wider (ld = N + 32; planes 2 N + 64) and longer (M + 3 rows) than its region, filled with
a NaN pattern (planes: p32_ref.CANARY); afterwards everything outside the region is bit-identical and no NaN / canary is left inside.
Inputs use ld > N too: the residual, the aux tensor a d-activation reads, and the operands, which are column slices of wider plane
buffers built on the host by p32_ref (NT: columns [32, 32 + K) of [rows][K + 64]; TN: the middle third of a fused [K][3 M] buffer).
An operand whose planes are usable comes with an fp32 copy full of NaN, one that takes the fp32 fallback with planes full of
canaries: a kernel that reads the wrong one of the two fails.  The dropout masks of the statement come from gemm_ref.drop_mult,
the host statement of the stream, which test_dropout_stream holds segmm_dropout_mult to bit for bit.

Cases: gemm_ref.NT_SHAPES x NT_FORMS under each of NT_ARMS, TN_SHAPES x TN_FORMS x tn_splits under each of TN_ARMS; a test is one
(arm, shape) and walks the forms, the float64 reference is cached per (shape, form) across arms.  Departures from the full cross,
each a refusal of the library (SEGMM_REQUIRE) or a launch that would be run twice (gemm_ref.nt_form_runs):
  * a plane output or a repair launch needs N % 32 == 0: (300, 100, 32) runs the non-plane forms only;
  * the round-2 kernel refuses a repair launch and an fp32 fallback for B: the arm 'round2' skips the repair, b_flag and never forms;
  * row-scaled outputs and a residual together with a d-activation run on the round-2 kernel whatever PL_VAR says: those forms run
    under 'default' and 'round2' only;
  * a TN launch with more splits than k-tiles is clamped by the host: split counts that give the same slabs run once;
  * the on-the-fly engines have no plane output, header, repair launch or operand state: they run gemm_ref.ONFLY_FORMS, the
    NT forms without those.
The on-the-fly engines (segmm_gemm with ENGINE_F32 / ENGINE_F16X3; test_planes_gpu.py uses them as referee) come last and smaller:
the NT forms at (130, 96, 64) and (300, 448, 96), plain NN and TN at (96, 48, 360) with splits 1 and 2, same statement with their own
operand terms (gemm_ref.nt_reference(engine=...), plain_reference), operands again column slices of NaN-filled wider buffers.

Measured on the MI355X: every case passes, no kernel was changed and no constant raised.  Outputs that only pass the accumulator sit
at 0.002 - 0.09 of their bound; the lines above one half (C|aux 0.98, the row_scale form 0.90, TN at K = 1 0.68) are single final
roundings held against their own u |result| (profiles/README.md), and the CPU emulation reaches the same figures.

Run with ``pytest -m gpu -s`` to see the worst error / bound per (kernel, output); SEGMM_GEMM_RATIO_LOG=path writes them to a file
(profiles/gemm_float64/ratios.txt).  tests/test_gemm_ref_cpu.py shows without a GPU that the bounds accept a faithful fp32 emulation
and reject planted defects, and that this case list reaches every kernel and every epilogue copy."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as G      # noqa: E402
import p32_ref as P32      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN_BITS = 0x7FC0BEEF
RATIOS = {}
_REF = {}


def _abi():
    from segmminterest_amd import hipabi
    hipabi.lib()
    return hipabi


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    lines = ["%-46s worst error / bound %.3g" % ("%s %s" % k, v) for k, v in sorted(RATIOS.items())]
    print("\n" + "\n".join(lines))
    path = os.environ.get("SEGMM_GEMM_RATIO_LOG")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


@pytest.fixture
def knobs(request):
    """set the knobs of an arm; restored in a finalizer"""
    H = _abi()
    prev = []

    def set_(kn):
        for k, v in kn.items():
            prev.append((k, H.config_set(k, v)))
        return {k: H.knob(k) for k in G.KNOBS}

    def restore():
        for k, v in reversed(prev):
            H.config_set(k, v)
    request.addfinalizer(restore)
    return set_


# ------------------------------------------------------------------ buffers
def _nan_buf(rows, ld):
    return torch.full((rows, ld), NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)


def _wide(x, ld, rows=None):
    """x [R, C] in the top-left corner of a NaN-filled [rows, ld] buffer"""
    x = np.asarray(x, np.float32)
    buf = _nan_buf(x.shape[0] if rows is None else rows, ld)
    buf[:x.shape[0], :x.shape[1]] = _dev(x)
    return buf


def _dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)          # (a copy: the shared inputs are read-only arrays)


def _canary_buf(rows, ld2):
    return torch.full((rows, ld2), P32.CANARY, dtype=torch.int16, device=DEV).view(torch.float16)


def _region_f32(buf, M, N, what, written=True):
    """the [M, N] region of an output buffer, after checking that nothing outside it changed and no NaN is left inside"""
    a = buf.cpu().numpy()
    bits = a.view(np.uint32)
    out = np.ones(a.shape, bool)
    out[:M, :N] = not written
    assert (bits[out] == NAN_BITS).all(), "%s: %d words outside the documented region changed" % (what, int((bits[out] != NAN_BITS).sum()))
    if not written:
        return None
    assert not np.isnan(a[:M, :N]).any(), "%s: %d elements of the region never written" % (what, int(np.isnan(a[:M, :N]).sum()))
    return a[:M, :N].copy()


def _region_planes(pl, M, N, ld2, what, overflowed=False):
    raw = pl.cpu().view(torch.int16).numpy().view(np.uint16).reshape(-1)
    off = P32._offsets(M, N, ld2)
    inside = np.zeros(raw.shape, bool)
    inside[off] = True
    inside[off + 32] = True
    assert (raw[~inside] == P32.CANARY).all(), "%s: %d halves outside the plane region changed" % (what, int((raw[~inside] != P32.CANARY).sum()))
    # (planes written with a scale that is too large may hold 65504, the canary's own pattern: no such check on them)
    assert overflowed or (raw[inside] != P32.CANARY).all(), "%s: halves of the plane region never written" % what
    return raw[off].view(np.float16), raw[off + 32].view(np.float16)


def _operand_pt(H, op, rows, cols, ld2, p_off, wide32, ldf, f_off, with_f32):
    """The operand on the device: planes placed in a canary-filled [rows][ld2] buffer at half offset p_off (all canaries when the
    kernel must take the fp32 copy), header as the statement gives it, the fp32 copy (NaN when the planes are to be used)."""
    img = np.full(rows * ld2, P32.CANARY, np.uint16)
    if not op["fallback"]:
        off = P32._offsets(rows, cols, ld2) + p_off
        img[off] = op["hi"].view(np.uint16)
        img[off + 32] = op["lo"].view(np.uint16)
    planes = _dev(img.view(np.int16)).view(torch.float16)
    f32 = None
    if with_f32:
        f32 = _dev(wide32) if op["fallback"] else _nan_buf(wide32.shape[0], wide32.shape[1])
    return H.PT(planes, _dev(op["hdr"].copy()), rows, cols, ld2=ld2, p_off=p_off, f32=f32, ldf=ldf, f_off=f_off)


def _nt_operand(H, op, rows, K, with_f32):
    wide = np.full((rows, K + 64), np.float32(0.5), np.float32)
    wide[:, 32:32 + K] = op["x32"]
    return _operand_pt(H, op, rows, K, 2 * (K + 64), 64, wide, K + 64, 32, with_f32)


def _note(kernel, ratios):
    for k, r in ratios.items():
        RATIOS[(kernel, k)] = max(RATIOS.get((kernel, k), 0.0), r)


# ------------------------------------------------------------------ NT
def _nt_ref(form, shape):
    key = (shape, form["name"])
    if key not in _REF:
        _REF[key] = G.nt_reference(form, shape)
    return _REF[key]


def _nt_launch(H, form, shape, ref, planes, write_c=True, repair=False, c_scale=None, state=None):
    """one launch of the form; ``state``: the buffers of an earlier launch of the same case (a repair launch reuses planes and header)"""
    M, N, K = shape
    b = G.nt_base(shape)
    opA, opB = G.nt_operands(shape, form)
    st = state or {}
    if not st:
        st["pa"] = _nt_operand(H, opA, M, K, True)
        st["pb"] = _nt_operand(H, opB, N, K, opB["fallback"])
        st["C"] = _nan_buf(M + 3, N + 32)
        if form["acc"]:
            st["C"][:M, :N] = _dev(b["cold"])
        kw = {}
        if form["bias"]:
            kw["bias"] = _dev(b["bias"])
        if form["row_scale"]:
            kw["row_scale"] = _dev(b["rs"])
        if form["res"] is not None:
            _, stored = G.nt_residual(form, shape)
            kw.update(residual=_wide(stored, N + 32), ldr=N + 32, res_period=M if form["res"] == "full" else form["res"])
        if form["act"] == G.EPI_GELU:
            st["aux"] = _nan_buf(M + 3, N + 32)
        elif form["act"] in (G.EPI_DGELU, G.EPI_DRELU):
            st["aux"] = _wide(b["aux"], N + 32)
        if form["act"] != G.EPI_NONE and "aux" in st:
            kw.update(aux=st["aux"], ldaux=N + 32)
        if form["act"] != G.EPI_NONE:
            kw["activation"] = form["act"]
        if form["p"] > 0:
            kw.update(drop_p=form["p"], seed=G.SEED | (G.LIVE_SEED if form["live"] else 0), site=G.SITE)
        if form["acc"]:
            kw["accumulate"] = True
        st["kw"] = kw
        if planes:
            st["pl"] = _canary_buf(M + 3, 2 * N + 64)
            st["hdr"] = H.new_site(DEV)[0]
            st["sc"] = torch.tensor([float(c_scale)], dtype=torch.float32, device=DEV)
        if form["hdr_only"]:
            st["hdr"] = H.new_site(DEV)[0]
    kwp = {}
    if planes:
        kwp = dict(c_pt=H.PT(st["pl"], st["hdr"], M, N, ld2=2 * N + 64), c_scale_ptr=st["sc"].data_ptr())
    elif form["hdr_only"]:
        kwp = dict(c_hdr=st["hdr"])
    H.gemm_p(H.LAYOUT_NT, M, N, K, st["pa"], st["pb"], None if repair else st["C"], N + 32, write_c=write_c, repair=repair, **st["kw"], **kwp)
    torch.cuda.synchronize()
    return st


def _nt_case(H, form, shape, kernel):
    M, N, K = shape
    ref = _nt_ref(form, shape)
    what = "%s %s %s" % (kernel, shape, form["name"])
    if form["live"]:
        H.step_set(G.STEP_WORDS, 0)
    got = {}
    if form["repair"]:
        plain = dict(form, planes=False, repair=None, write_c=True)
        got["C32"] = _region_f32(_nt_launch(H, plain, shape, ref, False)["C"], M, N, what + " (fp32 launch)")
        st = _nt_launch(H, form, shape, ref, True, write_c=False, c_scale=ref["c_scale"])
        got["hdr0"] = st["hdr"].cpu().numpy().copy()
        got["hi0"], got["lo0"] = _region_planes(st["pl"], M, N, 2 * N + 64, what + " (first launch)", overflowed=form["repair"] == "overflow")
        _nt_launch(H, form, shape, ref, True, write_c=False, repair=True, state=st)
    else:
        st = _nt_launch(H, form, shape, ref, form["planes"], write_c=form["write_c"], c_scale=ref["c_scale"])
    got["C"] = _region_f32(st["C"], M, N, what + " C", written=form["write_c"])
    if form["act"] == G.EPI_GELU:
        got["aux"] = _region_f32(st["aux"], M, N, what + " aux")
    if form["planes"]:
        got["hi"], got["lo"] = _region_planes(st["pl"], M, N, 2 * N + 64, what + " planes")
    if "hdr" in st:
        got["hdr"] = st["hdr"].cpu().numpy().copy()
    if form["live"]:
        H.step_set(0, 0)
    ratios, exact = G.judge_nt(form, ref, got)
    _note(kernel, ratios)
    print("%-60s %s" % (what, " ".join("%s %.3g" % kv for kv in sorted(ratios.items()))))
    assert all(exact.values()), (what, exact)
    assert all(r <= 1.0 for r in ratios.values()), (what, ratios)


@pytest.mark.parametrize("shape", G.NT_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("arm", [a for a, _ in G.NT_ARMS])
def test_nt(arm, shape, knobs):
    H = _abi()
    live = knobs(dict(G.NT_ARMS)[arm])
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    ran = 0
    for form in G.NT_FORMS:
        if not G.nt_form_runs(form, shape, arm):
            continue
        kernel = G.nt_kernel(G.nt_launch(form, shape), live, ncu)
        assert not kernel.startswith("!"), (arm, shape, form["name"], kernel)
        if arm not in ("default",) and not G.nt_round2_only(form):
            assert kernel == {"round2": "gemm_pl_nt", "nt4": "gemm_pl_nt4"}.get(arm, "gemm_pl_" + arm), (arm, kernel)
        _nt_case(H, form, shape, kernel)
        ran += 1
    assert ran >= 20


# ------------------------------------------------------------------ TN
def _tn_case(H, form, shape, splits, kernel):
    M, N, K = shape
    b = G.tn_base(shape)
    opA, opB = G.tn_operands(shape, form)
    ref = G.tn_reference(form, shape, splits)
    what = "%s %s %s splits %d" % (kernel, shape, form["name"], splits)
    # A: the middle third of the fused [K][3 M] buffer (the fp32 copy has the same layout); B: [K][N] in a wider buffer
    img = np.full(K * 6 * M, P32.CANARY, np.uint16)
    if not opA["fallback"]:
        off = P32._offsets(K, M, 6 * M) + 2 * M
        img[off], img[off + 32] = opA["hi"].view(np.uint16), opA["lo"].view(np.uint16)
    a32 = _dev(b["A3"]) if opA["fallback"] else _nan_buf(K, 3 * M)
    pa = H.PT(_dev(img.view(np.int16)).view(torch.float16), _dev(opA["hdr"].copy()), K, M, ld2=6 * M, p_off=2 * M, f32=a32, ldf=3 * M, f_off=M)
    wideB = np.full((K, N + 32), np.float32(0.5), np.float32)
    wideB[:, :N] = b["B"]
    pb = _operand_pt(H, opB, K, N, 2 * N + 64, 0, wideB, N + 32, 0, opB["fallback"])
    C = _nan_buf(M + 3, N + 32)
    cs = _nan_buf(1, M + 3)
    if form["acc"]:
        C[:M, :N] = _dev(b["cold"])
        cs[0, :M] = _dev(b["csold"])
    nsl = max(1, min(splits, (K + 31) // 32))
    ws = _nan_buf(1, nsl * (M * N + M) + 64)
    H.gemm_p(H.LAYOUT_TN, M, N, K, pa, pb, C, N + 32, splits=splits, workspace=ws, accumulate=form["acc"], colsum_out=cs if form["colsum"] else None)
    torch.cuda.synchronize()
    got = dict(C=_region_f32(C, M, N, what + " C"))
    colsum = _region_f32(cs, 1, M, what + " colsum", written=form["colsum"] or form["acc"])
    if form["colsum"]:
        got["colsum"] = colsum[0]
    elif form["acc"]:
        assert np.array_equal(colsum[0], b["csold"]), what + ": column sums written without colsum_out"
    ratios, exact = G.judge_tn(form, ref, got)
    _note(kernel, ratios)
    print("%-60s %s" % (what, " ".join("%s %.3g" % kv for kv in sorted(ratios.items()))))
    assert all(r <= 1.0 for r in ratios.values()), (what, ratios)


@pytest.mark.parametrize("shape", G.TN_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("arm", [a for a, _ in G.TN_ARMS])
def test_tn(arm, shape, knobs):
    H = _abi()
    live = knobs(dict(G.TN_ARMS)[arm])
    M, N, K = shape
    for form in G.TN_FORMS:
        for splits in G.tn_splits(K):
            kernel, slabs, _ = G.tn_plan(M, N, K, splits, N + 32, form["acc"], live)
            _tn_case(H, form, shape, splits, kernel + ("+splitk_reduce" if slabs > 1 else ""))


# ------------------------------------------------------------------ the on-the-fly engines
def _slice32(x, c0, extra):
    """x [R, C] as columns [c0, c0 + C) of a NaN-filled [R, C + extra] buffer"""
    x = np.asarray(x, np.float32)
    buf = _nan_buf(x.shape[0], x.shape[1] + extra)
    buf[:, c0:c0 + x.shape[1]] = _dev(x)
    return buf


@pytest.mark.parametrize("shape", G.ONFLY_NT_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("engine", G.ONFLY_ENGINES)
def test_on_the_fly_nt(engine, shape):
    H = _abi()
    M, N, K = shape
    b = G.nt_base(shape)
    eng = {"f32": H.ENGINE_F32, "f16x3": H.ENGINE_F16X3}[engine]
    A, B = _slice32(b["A"], 32, 64), _slice32(b["B"], 32, 64)
    for form in G.ONFLY_FORMS:
        key = (shape, form["name"], "f32" if engine == "f32" else "planes")
        if key not in _REF:
            _REF[key] = G.nt_reference(form, shape, key[2])
        ref = _REF[key]
        what = "on the fly %s %s %s" % (engine, shape, form["name"])
        C = _nan_buf(M + 3, N + 32)
        kw, aux = {}, None
        if form["acc"]:
            C[:M, :N] = _dev(b["cold"])
            kw["accumulate"] = True
        if form["bias"]:
            kw["bias"] = _dev(b["bias"])
        if form["row_scale"]:
            kw["row_scale"] = _dev(b["rs"])
        if form["res"] is not None:
            _, stored = G.nt_residual(form, shape)
            kw.update(residual=_wide(stored, N + 32), ldr=N + 32, res_period=M if form["res"] == "full" else form["res"])
        if form["act"] == G.EPI_GELU:
            aux = _nan_buf(M + 3, N + 32)
        elif form["act"] in (G.EPI_DGELU, G.EPI_DRELU):
            aux = _wide(b["aux"], N + 32)
        if aux is not None:
            kw.update(aux=aux, ldaux=N + 32)
        if form["p"] > 0:
            kw.update(drop_p=form["p"], seed=G.SEED | (G.LIVE_SEED if form["live"] else 0), site=G.SITE)
        if form["live"]:
            H.step_set(G.STEP_WORDS, 0)
        H.gemm(H.LAYOUT_NT, M, N, K, A, K + 64, B, K + 64, C, N + 32, activation=form["act"], a_off=32, b_off=32, engine=eng, **kw)
        torch.cuda.synchronize()
        if form["live"]:
            H.step_set(0, 0)
        got = dict(C=_region_f32(C, M, N, what + " C"))
        if form["act"] == G.EPI_GELU:
            got["aux"] = _region_f32(aux, M, N, what + " aux")
        ratios, exact = G.judge_nt(form, ref, got)
        _note("on the fly " + engine, ratios)
        print("%-60s %s" % (what, " ".join("%s %.3g" % kv for kv in sorted(ratios.items()))))
        assert all(exact.values()) and all(r <= 1.0 for r in ratios.values()), (what, ratios, exact)


@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("layout", ["nn", "tn"])
@pytest.mark.parametrize("engine", G.ONFLY_ENGINES)
def test_on_the_fly_plain(engine, layout, splits):
    H = _abi()
    M, N, K = G.ONFLY_PLAIN
    A32, B32 = G.plain_inputs(layout)
    want, bound = G.plain_reference(layout, engine, splits)
    A, B = _slice32(A32, 0, 8), _slice32(B32, 0, 32)
    C = _nan_buf(M + 3, N + 32)
    ws = _nan_buf(1, splits * M * N + 64)
    H.gemm(H.LAYOUT_NN if layout == "nn" else H.LAYOUT_TN, M, N, K, A, A.shape[1], B, N + 32, C, N + 32, splits=splits, workspace=ws,
           engine={"f32": H.ENGINE_F32, "f16x3": H.ENGINE_F16X3}[engine])
    torch.cuda.synchronize()
    r = G.ratio(_region_f32(C, M, N, "on the fly %s %s splits %d" % (engine, layout, splits)), want, bound)
    _note("on the fly %s %s%s" % (engine, layout, "+splitk_reduce" if splits > 1 else ""), {"C": r})
    assert r <= 1.0, (engine, layout, splits, r)


# ------------------------------------------------------------------ the dropout stream
@pytest.mark.parametrize("p", [0.0, 0.1, 0.25, 0.5, 0.999])
def test_dropout_stream(p):
    """segmm_dropout_mult equals gemm_ref.drop_mult bit for bit (the output in a longer NaN-filled buffer), live seed included"""
    H = _abi()
    H.step_set(G.STEP_WORDS, 0)
    try:
        for seed in (0x1_00000000, 0x7FFFFFFF_FFFFFFFF, G.SEED, G.SEED | G.LIVE_SEED):
            for site in (0, 5, 1 << 31):
                for n in (1, 3, 4, 4097):
                    out = _nan_buf(1, n + 5)
                    H.dropout_mult(out, n, p, seed, site)
                    torch.cuda.synchronize()
                    got = _region_f32(out, 1, n, "dropout_mult p %g seed %x site %x n %d" % (p, seed, site, n))[0]
                    want = G.drop_mult(G.make_drop(p, seed, site, G.STEP_WORDS), np.arange(n))
                    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (p, hex(seed), site, n)
    finally:
        H.step_set(0, 0)
