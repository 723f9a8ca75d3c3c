"""Input features stored as float16 / bfloat16: the resident feature table (segmm_gather_l1_h) and host-fed batches (segmm_l1norm_h).

Both formats embed in fp32 exactly, and the 16-bit kernels are DEFINED as "the fp32 kernel applied to the exactly widened values" (same
columns per lane, summation order, wave reduction, true division, plane calls).  So nothing here has a tolerance of its own: every
output of a 16-bit launch -- rows, masks, reciprocal scales, planes, site headers, partial maxima, and through them losses and
parameters of whole training steps -- is compared BIT FOR BIT with the fp32 launch on ``x16.float()``; the one bound used is
rowops_ref.l1_bounds against float64, unchanged.  Output buffers are pre-filled with a recorded pattern and every element outside the
documented output region is compared afterwards, as in tests/test_rowops_gpu.py."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rowops_ref as R
from helpers import build_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
ELEMS = [torch.float16, torch.bfloat16]
DS = [4, 260, 768, 1536, 2052]          # one lane, 8-byte row | 520-byte pitch + a 4-column tail | V = 3 | V = 6 | the loop form
F16_MAX = 65504.0


def _abi():
    from segmminterest_amd import hipabi
    hipabi.lib()
    # a binding without the 16-bit entry points would hand a 16-bit buffer to a float32 kernel (twice the bytes read): stop before
    # any launch
    assert "segmm_l1norm_h" in hipabi.SIGNATURES and "segmm_gather_l1_h" in hipabi.SIGNATURES, "no 16-bit feature kernels in this library"
    return hipabi


@contextlib.contextmanager
def _knob(H, name, value):
    prev = H.config_set(name, value)
    try:
        yield
    finally:
        H.config_set(name, prev)


def _host(t):
    torch.cuda.synchronize()
    return t.detach().cpu()


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _pattern(n, seed):
    """the recorded random fill of an output buffer (tests/test_rowops_gpu.py)"""
    return torch.from_numpy(np.random.default_rng(1000 + seed).standard_normal(n).astype(F))


def _rows16(rows, D, seed, elem):
    """rowops_ref.l1_rows cast to ``elem`` on the CPU; from 5 rows on, rows 1 .. 4 are: all zeros | signed with -0.0 entries |
    alternating +- the largest finite fp16 value | fp16 subnormals (k 2^-24, k = 1 .. 1023, signed).  Every row sum is finite in fp32
    (at most 2052 x 65536)."""
    x = R.l1_rows(rows, D, seed)
    if rows >= 5:
        sign = np.where(np.arange(D) % 2 == 0, 1.0, -1.0).astype(F)
        x[1] = 0.0
        x[2] = R.signed_rows(1, D, seed + 7)[0]
        x[2, ::3] = -0.0
        x[3] = sign * F(F16_MAX)
        x[4] = sign * ((np.arange(D) % 1023 + 1) * 2.0 ** -24).astype(F)
    t = torch.from_numpy(x).to(elem)
    assert torch.isfinite(t.float()).all() and torch.isfinite(t.float().abs().sum(1)).all()
    if rows >= 5:
        assert bool((_bits(t[2, ::3]) == -32768).all())          # -0.0 survives the cast (0x8000)
        if elem == torch.float16:
            assert float(t[3, 0]) == F16_MAX and float(t[4, 0]) == 2.0 ** -24
    return t


def _po(H, rows, D, scale):
    hdr = H.new_site(DEV)[0]
    sc = torch.tensor([scale], dtype=torch.float32, device=DEV)
    pl = torch.zeros((rows, 2 * D), dtype=torch.float16, device=DEV)
    return H.PO(pl, 2 * D, hdr, sc.data_ptr()), pl, hdr, sc


# ------------------------------------------------------------------ 1. gather
N_LINES, G_ROWS = 23, 21


def _gather_run(H, table, idx, normalize, D, amax=False, planes=False):
    """-> dict of host tensors: out [rows, D], mask, guards checked; optional amax slots / planes + header"""
    n = G_ROWS * D
    o0, m0 = _pattern(n + 2 * D + 16, 3), torch.full((G_ROWS + 8,), 7, dtype=torch.uint8)
    od, md = o0.to(DEV), m0.to(DEV)
    res = {}
    slots = torch.zeros(H.AMAX_SLOTS, dtype=torch.float32, device=DEV) if amax else None
    po = pl = hdr = keep = None
    if planes:
        po, pl, hdr, keep = _po(H, G_ROWS, D, 2.0 ** 13)          # |out| <= 1 when normalised
    H.gather_l1(table, idx, normalize=normalize, out=od, mask=md, amax=slots, po=po)
    o, m = _host(od), _host(md)
    assert _same(o[n:], o0[n:]) and _same(m[G_ROWS:], m0[G_ROWS:])          # nothing outside the output region was written
    res["out"], res["mask"] = o[:n].reshape(G_ROWS, D), m[:G_ROWS]
    if amax:
        res["amax"] = _host(slots)
    if planes:
        res["planes"], res["hdr"] = _host(pl), _host(hdr)
    return res


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("elem", ELEMS, ids=["f16", "bf16"])
@pytest.mark.parametrize("D", DS)
def test_gather_16bit_equals_fp32_gather_of_the_widened_table(D, elem, normalize):
    H = _abi()
    t16 = _rows16(N_LINES, D, D, elem)
    wide = t16.float()
    idx = np.random.default_rng(D).integers(0, N_LINES, G_ROWS).astype(np.int64)
    idx[[0, 1, 2, 3, 4, 5, 6, 7, 8]] = [-1, N_LINES, 10 ** 9, 0, N_LINES - 1, 1, 2, 3, 4]
    ok = (idx >= 0) & (idx < N_LINES)
    idx_d = torch.from_numpy(idx.reshape(3, 7)).to(DEV)
    t16d, wided = t16.to(DEV), wide.to(DEV)
    got, want = _gather_run(H, t16d, idx_d, normalize, D), _gather_run(H, wided, idx_d, normalize, D)
    assert got["out"].dtype == torch.float32
    assert _same(got["out"], want["out"]) and _same(got["mask"], want["mask"])
    assert np.array_equal(got["mask"].numpy(), ok.astype(np.uint8))
    assert not _bits(got["out"][torch.from_numpy(~ok)]).any()          # +0.0 in every padded element
    g = wide.numpy()[idx[ok]]
    o = got["out"].numpy()[ok]
    if not normalize:
        assert np.array_equal(o.view(np.uint32), g.view(np.uint32))          # the widened table rows, signed zeros included
    else:
        _, _, y64 = R.l1_ref(g)
        with np.errstate(all="ignore"):
            r = R.ratio(np.abs(o.astype(np.float64) - y64), R.l1_bounds(g)[2])
        print("gather_l1_h D=%d %s: worst error / l1 bound = %.3g" % (D, elem, r))
        assert r <= 1.0
    a16, a32 = _gather_run(H, t16d, idx_d, normalize, D, amax=True), _gather_run(H, wided, idx_d, normalize, D, amax=True)
    assert _same(a16["amax"], a32["amax"]) and _same(a16["out"], want["out"]) and float(a32["amax"].max()) > 0
    if D % 32 == 0 and normalize:
        p16, p32 = _gather_run(H, t16d, idx_d, normalize, D, planes=True), _gather_run(H, wided, idx_d, normalize, D, planes=True)
        assert _same(p16["planes"], p32["planes"]) and _same(p16["hdr"], p32["hdr"]) and _same(p16["out"], want["out"])
        assert float(p32["hdr"][0]) == 2.0 ** 13 and bool(p32["planes"].any())


# ------------------------------------------------------------------ 2. L1 normalisation of a 16-bit x
def _l1_run(H, xd, rows, D, with_y, with_inv, planes=False):
    n = rows * D
    y0, i0 = _pattern(n + 2 * D + 16, 1), _pattern(rows + 5, 2)
    yd, idv = y0.to(DEV), i0.to(DEV)
    po = pl = hdr = keep = None
    if planes:
        po, pl, hdr, keep = _po(H, rows, D, 2.0 ** 14)
    H.l1norm(xd, yd if with_y else None, idv if with_inv else None, po=po)
    y, inv = _host(yd), _host(idv)
    assert _same(y[n:], y0[n:]) and _same(inv[rows:], i0[rows:])
    if not with_y:
        assert _same(y, y0)
    if not with_inv:
        assert _same(inv, i0)
    return dict(y=y[:n], inv=inv[:rows], planes=None if pl is None else _host(pl), hdr=None if hdr is None else _host(hdr))


@pytest.mark.parametrize("rows", [1, 5, 21])
@pytest.mark.parametrize("elem", ELEMS, ids=["f16", "bf16"])
@pytest.mark.parametrize("D", DS)
def test_l1norm_16bit_equals_fp32_l1norm_of_the_widened_rows(D, elem, rows):
    H = _abi()
    x16 = _rows16(rows, D, D + rows, elem).to(DEV)
    wide = x16.float()
    modes = [(True, True, False), (True, False, False), (False, True, False)]
    if D % 32 == 0:
        modes += [(False, False, True), (True, True, True)]          # planes only (y null), and planes next to y
    for with_y, with_inv, planes in modes:
        got = _l1_run(H, x16, rows, D, with_y, with_inv, planes)
        for reg in (1, 0):
            with _knob(H, "L1NORM_REG", reg):
                want = _l1_run(H, wide, rows, D, with_y, with_inv, planes)
            what = "D=%d rows=%d %s y=%d inv=%d planes=%d reg=%d" % (D, rows, elem, with_y, with_inv, planes, reg)
            assert _same(got["y"], want["y"]) and _same(got["inv"], want["inv"]), what
            if planes:
                assert _same(got["planes"], want["planes"]) and _same(got["hdr"], want["hdr"]), what
                assert bool(want["planes"].any()) and float(want["hdr"][0]) == 2.0 ** 14, what
    if rows >= 5:          # the special rows did what they are there for: the zero row gives 0 / 1e-6, the +-65504 row 1 / D
        y = _l1_run(H, x16, rows, D, True, True)
        assert not y["y"].reshape(rows, D)[1].any() and float(y["inv"][1]) == float(np.float32(1.0) / np.float32(1e-6))


# ------------------------------------------------------------------ 3. refusals
def test_refusals_launch_nothing():
    H = _abi()
    D, n = 8, 5
    idx = torch.zeros((3,), dtype=torch.int64, device=DEV)
    o0 = _pattern(3 * D + 16, 5)
    od = o0.to(DEV)
    base = torch.rand(n, D, device=DEV)
    wide2 = torch.rand(n, 2 * D, device=DEV)
    strided16, strided32 = wide2.half()[:, ::2], wide2[:, ::2]
    assert not strided16.is_contiguous() and not strided32.is_contiguous()
    for bad, word in ((base.double(), "float64"), (base.to(torch.int16), "int16"), (strided16, "float16"), (strided32, "float32")):
        with pytest.raises(RuntimeError, match=word):
            H.gather_l1(bad, idx, out=od)
        with pytest.raises(RuntimeError, match=word):
            H.l1norm(bad, od[:n * D].view(n, D))
    for elem in ELEMS:
        six = torch.rand(n, 6, device=DEV).to(elem)
        with pytest.raises(RuntimeError, match="D=6"):
            H.gather_l1(six, idx, out=od)
        with pytest.raises(RuntimeError, match="D=6"):
            H.l1norm(six, od[:n * 6].view(n, 6))
    # outputs stay float32: a 16-bit output buffer is refused as well
    with pytest.raises(RuntimeError, match="float32"):
        H.l1norm(base.half().to(DEV), torch.empty(n, D, dtype=torch.float16, device=DEV))
    # elem = 0 through the raw C entry points: an error return with a message, never a launch
    L = H.lib()
    t16 = base.half().to(DEV)
    rc = L.segmm_gather_l1_h(t16.data_ptr(), 0, n, D, idx.data_ptr(), 3, 1, od.data_ptr(), None, None, None, 0, None, None, H._stream())
    assert rc != 0 and b"elem" in L.segmm_last_error()
    rc = L.segmm_l1norm_h(t16.data_ptr(), 3, od.data_ptr(), None, n, D, None, None, 0, None, None, H._stream())
    assert rc != 0 and b"elem" in L.segmm_last_error()
    assert _same(_host(od), o0)          # nothing was launched: the output buffer still holds its pattern


# ------------------------------------------------------------------ 4. whole model, resident table
def _dataset():
    from test_assemble_gpu import _dataset as ds
    table, feats = ds()
    return table, feats.half()          # U[0, 1) features rounded to fp16 once; every trainer below sees these values


def _cfg(d=32):
    from test_assemble_gpu import D_E, LT_E, S_E
    return dict(N=2, h=4 if d == 32 else d // 16, S=S_E, d=d, D_in=D_E, Lt=LT_E, user="image", photo="image", loss_type_list=["interestBPR"],
                loss_weight={"interestBPR": 1.0, "mse": 1.0}, exposure_prob=[1.0] * S_E)


def _trainer(feats=None, d=32, user_feats=None, **kw):
    from segmminterest_amd.feature_store import ResidentFeatureTable
    from segmminterest_amd.trainer import Trainer
    torch.manual_seed(5)
    model = build_model(_cfg(d)).cuda()
    torch.manual_seed(11)
    ft = None if feats is None else ResidentFeatureTable(feats.to(DEV), None if user_feats is None else user_feats.to(DEV))
    return model, Trainer(model, lr=1e-3, feature_table=ft, **kw)


def _index_batches(n=4):
    from test_assemble_gpu import B_E, LT_E, S_E
    from segmminterest_amd import feature_store as FS
    table, feats16 = _dataset()
    db = FS.DeviceBatches(table.to(DEV), B_E, S_E, LT_E, seed=3, drop_last=True)
    batches = list(db(0))[:n]
    assert len(batches) == n
    return table, feats16, batches


def _steps(feats, batches, d=32, how="eager", user_feats=None, **kw):
    """three optimisation steps -> (losses, flat parameters)"""
    model, tr = _trainer(feats, d=d, user_feats=user_feats, **kw)
    losses = []
    if how == "eager":
        for b in batches[:3]:
            losses.append(tr.train_step(b)["loss"].detach().clone())
    elif how == "prefetch":
        for b, nb in zip(batches[:3], batches[1:4]):
            losses.append(tr.train_step(b, next_batch=nb)["loss"].detach().clone())
    else:          # "recorded": one eager warm-up step, the recorded step, then three replays on other batch objects
        losses.append(tr.record(batches[0], warmup=1)["loss"].detach().clone())
        for b in batches[1:4]:
            losses.append(tr.run_recorded(b)["loss"].detach().clone())
    torch.cuda.synchronize()
    assert all(torch.isfinite(x).all() for x in losses)
    return losses, model._store.flat.detach().clone()


def _equal_runs(a, b):
    assert len(a[0]) == len(b[0]) and all(torch.equal(x, y) for x, y in zip(a[0], b[0]))
    assert torch.equal(a[1], b[1]) and torch.isfinite(a[1]).all()


@pytest.mark.parametrize("case", ["d32", "d48_fp32_consumers", "bf16", "dropout_device_state", "prefetch", "recorded", "mixed_tables"])
def test_training_on_a_16bit_table_equals_training_on_the_widened_table(case):
    _abi()
    _, feats16, batches = _index_batches()
    kw, how, d, t16, user16 = {"dropout": False}, "eager", 32, feats16, None
    if case == "d48_fp32_consumers":
        d = 48          # (3 heads of 16) d_model % 32 != 0: the weight gradient reads the fp32 copy of the features (Trainer._plane_consumers_only)
    elif case == "bf16":
        t16 = feats16.float().bfloat16()
    elif case == "dropout_device_state":
        kw = {"dropout": True, "device_state": True}
    elif case == "prefetch":
        how = "prefetch"
    elif case == "recorded":
        kw, how = {"dropout": False, "device_state": True}, "recorded"
    elif case == "mixed_tables":
        user16 = feats16.float().bfloat16()          # photo table float16, user table bfloat16
    wide = t16.float()
    a = _steps(t16, batches, d=d, how=how, user_feats=user16, **kw)
    b = _steps(wide, batches, d=d, how=how, user_feats=None if user16 is None else user16.float(), **kw)
    _equal_runs(a, b)
    assert not torch.equal(a[0][0], a[0][-1])          # the steps moved the model


def test_fit_recorded_and_eager_on_a_16bit_table_equal_the_widened_table():
    from test_assemble_gpu import B_E, LT_E, S_E
    from segmminterest_amd import feature_store as FS
    _abi()
    table, feats16 = _dataset()
    dev = table.to(DEV)
    valid = list(FS.DeviceBatches(dev, 16, S_E, LT_E, shuffle=False)(0))
    ends = {}
    for name, feats in (("f16", feats16), ("wide", feats16.float())):
        for mode in ("eager", "recorded"):
            model, tr = _trainer(feats, device_state=True)
            db = FS.DeviceBatches(dev, B_E, S_E, LT_E, seed=3, drop_last=True)
            hist = tr.fit(db, valid, epochs=2, valid_step=100, permutation=0, recorded=(mode == "recorded"))
            assert hist["global_step"] == 8
            if mode == "recorded":
                assert tr.__dict__.get("_recorded") is not None
            ends[name, mode] = model._store.flat.detach().clone()
    ref = ends["wide", "eager"]
    assert torch.isfinite(ref).all() and all(torch.equal(v, ref) for v in ends.values())


# ------------------------------------------------------------------ 5. whole model, host-fed 16-bit batches
def _feature_batches(dtype, n=4):
    from test_assemble_gpu import B_E, D_E, LT_E, S_E
    from segmminterest_amd.synth import make_batch
    out = []
    for i in range(n):
        b = make_batch(B_E, S_E, LT_E, D_E, n_users=50, n_items=500, seed=40 + i)
        for k in ("user", "photo"):
            b[k] = b[k].half().to(dtype)          # rounded to fp16 once; float32: the widened values
        out.append({k: v.to(DEV) for k, v in b.items()})
    return out


@pytest.mark.parametrize("how", ["eager", "recorded"])
def test_host_fed_16bit_batches_equal_the_widened_batches(how):
    _abi()
    kw = {"dropout": False, "device_state": how == "recorded"}
    b16, b32 = _feature_batches(torch.float16), _feature_batches(torch.float32)
    assert b16[0]["user"].dtype == torch.float16 and torch.equal(b16[0]["photo"].float(), b32[0]["photo"])
    _equal_runs(_steps(None, b16, how=how, **kw), _steps(None, b32, how=how, **kw))


def test_a_recorded_step_refuses_a_batch_of_another_feature_dtype():
    _abi()
    b16, b32 = _feature_batches(torch.float16, 2), _feature_batches(torch.float32, 2)
    for rec, other in ((b32, b16), (b16, b32)):
        model, tr = _trainer(None, dropout=False, device_state=True)
        tr.record(rec[0], warmup=1)
        tr.run_recorded(rec[1])          # the recorded dtype replays onto another batch object
        flat = model._store.flat.detach().clone()
        with pytest.raises(RuntimeError, match="run_recorded"):
            tr.run_recorded(other[1])
        torch.cuda.synchronize()
        assert torch.equal(model._store.flat, flat)          # the refused call enqueued nothing


# ------------------------------------------------------------------ 6. evaluation
def _assert_same_tree(a, b, path=""):
    assert type(a) is type(b), path
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _assert_same_tree(a[k], b[k], "%s/%s" % (path, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _assert_same_tree(x, y, "%s[%d]" % (path, i))
    elif torch.is_tensor(a):
        assert _same(a, b), path
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), (path, a, b)


def test_validation_and_test_metrics_equal_on_the_16bit_and_the_widened_table():
    from test_assemble_gpu import LT_E, S_E
    from segmminterest_amd import feature_store as FS
    _abi()
    table, feats16 = _dataset()
    valid = list(FS.DeviceBatches(table.to(DEV), 16, S_E, LT_E, shuffle=False)(0))
    evals = ["JaccardSim", "LeaveMSE", "LeaveCTR", "LeaveCTR_view", "TOP_K", "ProbAUC"]
    res = []
    for feats in (feats16, feats16.float()):
        _, tr = _trainer(feats)
        res.append((tr.valid_model(valid, permutation=0), tr.test_model(valid, evals, top_k_permutation=0)["final"],
                    tr.test_model(valid, evals, top_k_permutation=0, device_metrics=True)["final"]))
    _assert_same_tree(res[0], res[1])
    assert len(res[0][0]) > 0 and all(np.isfinite(v) for v in res[0][0].values())


# ------------------------------------------------------------------ 7. from_memmap
def test_from_memmap_streams_and_converts_in_chunks(tmp_path):
    from segmminterest_amd.feature_store import ResidentFeatureTable
    _abi()
    a = np.random.default_rng(5).standard_normal((37, 64)).astype(F)
    path = str(tmp_path / "features.bin")
    a.tofile(path)
    t16 = ResidentFeatureTable.from_memmap(path, 37, 64, dtype=torch.float16, device=DEV, chunk_rows=16)          # 16 + 16 + 5 lines
    assert t16.tables["photo"].dtype == torch.float16 and t16.tables["user"] is t16.tables["photo"]
    assert _same(_host(t16.tables["photo"]), torch.from_numpy(a).half())
    tb = ResidentFeatureTable.from_memmap(path, 37, 64, dtype=torch.bfloat16, device=DEV, chunk_rows=16)
    assert _same(_host(tb.tables["photo"]), torch.from_numpy(a).bfloat16())
    t32 = ResidentFeatureTable.from_memmap(path, 37, 64, device=DEV, chunk_rows=16)
    assert t32.tables["photo"].dtype == torch.float32 and _same(_host(t32.tables["photo"]), torch.from_numpy(a))
    idx = torch.tensor([[0, 36, -1, 17]], device=DEV)
    out, mask = t16.gather("photo", idx)
    assert out.dtype == torch.float32 and mask.tolist() == [[True, True, False, True]]
    a[33, 7] = 1e6          # finite in float32 and bfloat16, not in float16
    a[35, 1] = -1e6
    a.tofile(path)
    with pytest.raises(ValueError, match=r"line 33\b"):
        ResidentFeatureTable.from_memmap(path, 37, 64, dtype=torch.float16, device=DEV, chunk_rows=16)
    ok = ResidentFeatureTable.from_memmap(path, 37, 64, dtype=torch.float32, device=DEV, chunk_rows=16)
    assert float(ok.tables["photo"][33, 7]) == 1e6
    with pytest.raises(RuntimeError, match="float64"):
        ResidentFeatureTable(torch.zeros(4, 8, dtype=torch.float64, device=DEV))
