"""The kernels that write the P32 plane format on the MI355X against its host statement (tests/p32_ref.py), bit for bit on the uint16
images: segmm_split_p32 (both modes), segmm_split_p32_transpose, the two device forms of the split against each other,
segmm_wsplit_p32 on hand-built descriptor tables, and the parameter store's weight planes before and after eager and recorded
training steps.  Every plane buffer is filled with a canary pattern first: what the format does not address must come back
untouched.  Run with ``pytest -m gpu``."""
import os
import struct
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import p32_ref as P      # noqa: E402
from helpers import MODEL_CASES, build_model, load_case      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 128          # canary halves in front of and behind every plane view
HUGE = 3e38          # fills what the kernels must not read: fmaxf would drop a NaN, this shows up as a wrong maximum / scale
SENT = 7.25          # header words 2 .. 7 belong to nobody here


def _abi():
    from segmminterest_amd import hipabi
    hipabi.lib()
    assert (hipabi.SITE_HDR, hipabi.AMAX_SLOTS) == (P.SITE_HDR, P.AMAX_SLOTS)
    return hipabi


def _canaries(n):
    return torch.full((n,), P.CANARY, dtype=torch.int16, device=DEV)


def _u16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16).reshape(-1)


def _canon(img):
    """A NaN term is a NaN term: its sign and payload are not part of the format (every pattern maps to 0x7E00)."""
    img = img.copy()
    img[((img & 0x7C00) == 0x7C00) & ((img & 0x03FF) != 0)] = 0x7E00
    return img


def _same_image(got, want, what, ld2=None):
    """Bit for bit, canaries included; on a mismatch name the first half that differs."""
    got, want = _canon(got), _canon(want)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(bad[0])
        where = "" if ld2 is None else " (row %d, half %d of the row)" % ((i - GUARD) // ld2, (i - GUARD) % ld2)
        raise AssertionError("%s: %d halves differ, first at %d%s: got 0x%04X, want 0x%04X" % (what, bad.size, i, where, got[i], want[i]))


def _guarded(img):
    return np.concatenate([np.full(GUARD, P.CANARY, np.uint16), img, np.full(GUARD, P.CANARY, np.uint16)])


def _f32_view(x2d, ld, x_off):
    """x2d inside a buffer of HUGE: leading offset, row stride ld, 64 floats behind the last row."""
    R, C = x2d.shape
    buf = np.full(x_off + R * ld + 64, HUGE, dtype=np.float32)
    v = buf[x_off:x_off + R * ld].reshape(R, ld)
    v[:, :C] = x2d
    return torch.from_numpy(buf).to(DEV)


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ inputs
_INPUTS = {}


def _values(kind, rows, cols):
    """(x [rows, cols] fp32, the scale a mode-1 call is given).  Built once per (kind, shape) and never modified."""
    key = (kind, rows, cols)
    if key in _INPUTS:
        return _INPUTS[key]
    n = rows * cols
    rng = np.random.RandomState(rows * 131 + cols)
    if kind == "normal":
        x = (rng.standard_normal(n) * 0.37).astype(np.float32)
        s = P.exact_scale(P.amax_of(x)) / np.float32(8.0)          # a delayed scale with head-room
    elif kind in ("log24", "log12"):
        x = np.resize(P.log_input(24 if kind == "log24" else 12), n).copy()          # element 0 is the maximum
        s = P.exact_scale(P.amax_of(x))
    elif kind == "zeros":
        x, s = np.zeros(n, dtype=np.float32), np.float32(2.0 ** 14)
    elif kind == "negzero":
        x = rng.standard_normal(n).astype(np.float32)
        x[::3] = -0.0
        s = P.exact_scale(P.amax_of(x))
    else:          # the maximum at an edge of the fp16 range under s = 4, or one NaN
        s = np.float32(4.0)
        name, m, _ = [b for b in P.flag_boundaries(s) if b[0] == kind][0]
        x = (rng.standard_normal(n) * 100.0 / s).astype(np.float32)
        x[(2 * n) // 3] = -m if kind == "above_hi_finite" else m
    x = x.reshape(rows, cols)
    x.setflags(write=False)
    _INPUTS[key] = (x, np.float32(s))
    return _INPUTS[key]


SHAPES = [(1, 32, 32, 0, 64), (3, 64, 80, 8, 2 * 64 + 64), (300, 96, 96, 0, 192),
          (4100, 512, 512, 0, 1024)]          # 4100 x 128 float4 groups > 2048 workgroups x 256: the grid-stride loop, slot keys past 255
KINDS = ["normal", "log24", "log12", "zeros", "negzero", "below", "at", "above_hi_finite", "nan"]


# ------------------------------------------------------------------ segmm_split_p32
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows,cols,ld,x_off,ld2", SHAPES)
@pytest.mark.parametrize("mode", [0, 1])
def test_split_p32_equals_the_host_split(mode, rows, cols, ld, x_off, ld2, kind):
    H = _abi()
    x, s1 = _values(kind, rows, cols)
    amax = P.amax_of(x)
    xd = _f32_view(x, ld, x_off)
    pl = _canaries(GUARD + rows * ld2 + GUARD)
    hdr = np.zeros(P.SITE_FLOATS, dtype=np.float32)
    hdr[2:P.SITE_HDR] = SENT
    if mode == 0:          # the maxima are complete when the pass runs; a stale flag and scale are overwritten
        hdr[0], hdr[1] = 3.0, 1.0
        hdr[P.SITE_HDR:] = P.slot_fill(x)
        s = P.exact_scale(amax)
    else:
        hdr[0] = s = s1
    hd = torch.from_numpy(hdr.copy()).to(DEV)
    H.split_p32(xd, rows, cols, ld, pl, ld2, hd, mode=mode, x_off=x_off, p_off=GUARD)
    torch.cuda.synchronize()
    got_h = hd.cpu().numpy()
    what = "split_p32 mode %d %dx%d %s" % (mode, rows, cols, kind)
    assert _bits(got_h[0]) == _bits(s), (what, got_h[0], s)
    assert np.array_equal(_bits(got_h[2:P.SITE_HDR]), _bits(hdr[2:P.SITE_HDR])), what
    slots = got_h[P.SITE_HDR:]
    if mode == 0:
        assert _bits(got_h[1]) == 0, what
        assert np.array_equal(_bits(slots), _bits(hdr[P.SITE_HDR:])), what
    else:
        assert bool(_bits(got_h[1]) != 0) is P.overflow_flag(x, s), (what, got_h[1])
        assert _bits(slots.max()) == _bits(amax) and (slots >= 0).all() and (slots <= amax).all(), (what, slots.max(), amax)
    want, _ = P.pack(x, s, ld2)
    got = _u16(pl)
    if kind == "nan":
        r, c = divmod(int(np.flatnonzero(np.isnan(x.reshape(-1)))[0]), cols)
        i = GUARD + r * ld2 + (c // 32) * 64 + c % 32
        print("%s: device NaN terms hi 0x%04X lo 0x%04X" % (what, got[i], got[i + 32]))
    _same_image(got, _guarded(want), what, ld2)
    if kind.startswith("log"):          # the per-element bound of the CPU test, on what the device wrote
        hi, lo = P.unpack(got[GUARD:GUARD + rows * ld2], rows, cols, ld2)
        p = x.astype(np.float64) * float(s)
        err = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - p)
        big = np.abs(p) >= P.KNEE
        assert (err[big] <= P.REL * np.abs(p[big])).all() and (err[~big] <= P.ABS).all(), what
        if kind == "log24" and rows * cols >= 4096:
            sub = (lo != 0) & (np.abs(lo.astype(np.float64)) < 2.0 ** -14)
            assert sub.mean() > 0.2, "no subnormal lo terms came back from the device"


# ------------------------------------------------------------------ segmm_split_p32_transpose
T_SHAPES = [(32, 32, 32, 64), (64, 40, 48, 2 * 64 + 64), (96, 160, 160, 192)]


def _transpose_planes(H, x, ld, ld2, s):
    R, C = x.shape
    xd = _f32_view(x, ld, 0)
    pl = _canaries(GUARD + C * ld2 + GUARD)
    hdr = np.zeros(P.SITE_FLOATS, dtype=np.float32)
    hdr[0], hdr[2:P.SITE_HDR] = s, SENT
    hd = torch.from_numpy(hdr.copy()).to(DEV)
    H.split_p32_transpose(xd, R, C, ld, pl, ld2, hd, p_off=GUARD)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(hd.cpu().numpy()), _bits(hdr)), "split_p32_transpose only reads the header"
    return _u16(pl)


@pytest.mark.parametrize("kind", ["normal", "log24", "negzero"])
@pytest.mark.parametrize("R,C,ld,ld2", T_SHAPES)
def test_split_p32_transpose_equals_the_host_split(R, C, ld, ld2, kind):
    H = _abi()
    x, s = _values(kind, R, C)
    got = _transpose_planes(H, x, ld, ld2, s)
    want, _ = P.pack_transposed(x, s, ld2)
    _same_image(got, _guarded(want), "split_p32_transpose %dx%d %s" % (R, C, kind), ld2)


@pytest.mark.parametrize("kind", ["normal", "log24", "negzero"])
def test_the_two_device_forms_of_the_split_agree(kind):
    """v_fma_mix (split_p32, every fused producer) against casts + fmaf (split_p32_transpose, the weight split): the forward and
    dgrad GEMMs multiply an operand made by one with an operand made by the other."""
    H = _abi()
    R, C = 96, 160
    x, s = _values(kind, R, C)
    a = _transpose_planes(H, x, C, 2 * R, s)
    xt = torch.from_numpy(np.ascontiguousarray(x.T)).to(DEV)
    pl = _canaries(GUARD + C * 2 * R + GUARD)
    hd = torch.zeros(P.SITE_FLOATS, device=DEV)
    hd[0] = float(s)
    H.split_p32(xt, C, R, R, pl, 2 * R, hd, mode=1, p_off=GUARD)
    torch.cuda.synchronize()
    b = _u16(pl)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, "split_p32_transpose and split_p32 differ in %d halves, first at %d: 0x%04X (casts + fmaf) vs 0x%04X (v_fma_mix)" % (
        bad.size, bad[0], a[bad[0]], b[bad[0]])
    if kind == "log24":
        lo = P.unpack(a[GUARD:-GUARD], C, R)[1]
        assert ((lo != 0) & (np.abs(lo.astype(np.float64)) < 2.0 ** -14)).mean() > 0.2


# ------------------------------------------------------------------ segmm_wsplit_p32
W_SHAPES = [(8, 32, 0), (72, 64, 0), (32, 96, 1), (96, 32, 1), (256, 128, 1), (1, 32, 0)]


def _table(shapes):
    """[(offset, R, C, transpose, first tile, tile columns)], the float count and the tile count: offsets rounded up to 32 floats
    with gaps of 32 .. 96 floats in front of every matrix."""
    recs, off, tile0 = [], 0, 0
    for i, (R, C, tr) in enumerate(shapes):
        off = ((off + 31) & ~31) + 32 * (1 + i % 3)
        recs.append((off, R, C, tr, tile0, C // 32))
        off += R * C
        tile0 += ((R + 31) // 32) * (C // 32)
    return recs, ((off + 31) & ~31) + 32, tile0


def _check_wsplit(recs, flat, whdr, wpl, wTpl, what):
    flat, whdr, wpl, wTpl = flat.cpu().numpy(), whdr.cpu().numpy(), _u16(wpl), _u16(wTpl)
    want, wantT = np.full(wpl.shape, P.CANARY, np.uint16), np.full(wTpl.shape, P.CANARY, np.uint16)
    for i, (off, R, C, tr, _, _) in enumerate(recs):
        W = flat[off:off + R * C].reshape(R, C)
        amax = P.amax_of(W)
        s = P.exact_scale(amax)
        h = whdr[i]
        w = "%s: matrix %d (%d x %d%s)" % (what, i, R, C, ", transposed too" if tr else "")
        assert _bits(h[0]) == _bits(s), (w, h[0], s)
        assert _bits(h[1]) == 0 and not _bits(h[2:P.SITE_HDR]).any(), w
        slots = h[P.SITE_HDR:]
        assert _bits(slots.max()) == _bits(amax) and (slots >= 0).all() and (slots <= amax).all(), (w, slots.max(), amax)
        if amax == 0:
            assert s == 1 and not _bits(slots).any(), w
        want[2 * off:2 * off + 2 * R * C] = P.pack(W, s)[0]
        if tr:
            wantT[2 * off:2 * off + 2 * R * C] = P.pack_transposed(W, s)[0]
    _same_image(wpl, want, what + ": W planes")
    _same_image(wTpl, wantT, what + ": W^T planes")


@pytest.mark.parametrize("shapes", [[(32, 32, 1)], W_SHAPES * 7], ids=["one_32x32", "42_mixed"])
def test_wsplit_p32_equals_the_host_split_and_keeps_no_stale_maxima(shapes):
    H = _abi()
    recs, n, n_tiles = _table(shapes)
    rng = np.random.RandomState(len(shapes))
    flat = np.full(n, HUGE, dtype=np.float32)
    zero = len(recs) // 2
    for i, (off, R, C, _, _, _) in enumerate(recs):
        mag = 10.0 ** rng.uniform(-6, 3)          # every header gets a scale of its own
        flat[off:off + R * C] = 0.0 if (i == zero and len(recs) > 1) else rng.standard_normal(R * C) * mag
        if i % 5 == 1:
            flat[off:off + R * C:3] = -0.0
    desc = torch.frombuffer(bytearray(b"".join(struct.pack("<qiiiii4x", *r) for r in recs)), dtype=torch.uint8).to(DEV)
    fd = torch.from_numpy(flat).to(DEV)
    whdr = torch.zeros((len(recs), P.SITE_FLOATS), device=DEV)
    wpl, wTpl = _canaries(2 * n), _canaries(2 * n)
    H.wsplit_p32(fd, desc, len(recs), n_tiles, whdr, wpl, wTpl)
    torch.cuda.synchronize()
    _check_wsplit(recs, fd, whdr, wpl, wTpl, "first call")
    # the optimizer has stepped: same headers, NOT zeroed in between; all weights 2^12 times smaller, another matrix all zero
    fd.mul_(2.0 ** -12)
    off, R, C = recs[0][:3]
    fd[off:off + R * C] = 0.0
    H.wsplit_p32(fd, desc, len(recs), n_tiles, whdr, wpl, wTpl)
    torch.cuda.synchronize()
    _check_wsplit(recs, fd, whdr, wpl, wTpl, "second call on the same headers")


# ------------------------------------------------------------------ the parameter store
def _check_store(st, flat, what):
    """The planes and headers ``st.wpt`` / ``st.wTpt`` address are the host split of the weights in ``flat`` (a host copy)."""
    assert len(st._wmats) > 0
    wpl, wTpl, whdr = _u16(st.wpl), _u16(st.wTpl), st.whdr.cpu().numpy()
    n_tr = 0
    for i, (name, off, R, C, tr) in enumerate(st._wmats):
        W = flat[off:off + R * C].reshape(R, C)
        amax = P.amax_of(W)
        s = P.exact_scale(amax)
        pt = st.wpt[name]
        w = "%s: %s (%d x %d)" % (what, name, R, C)
        assert pt.planes is st.wpl and (pt.rows, pt.cols) == (R, C) and pt.hdr.data_ptr() == st.whdr[i].data_ptr(), w
        h = pt.hdr.cpu().numpy()
        assert np.array_equal(_bits(h), _bits(whdr[i])), w
        assert _bits(h[0]) == _bits(s) and _bits(h[1]) == 0, (w, h[0], s)
        assert _bits(h[P.SITE_HDR:].max()) == _bits(amax), (w, h[P.SITE_HDR:].max(), amax)
        _same_image(wpl[pt.p_off:pt.p_off + R * pt.ld2], P.pack(W, s, pt.ld2)[0], w + " W planes")
        if tr:
            n_tr += 1
            ptT = st.wTpt[name]
            assert ptT.planes is st.wTpl and (ptT.rows, ptT.cols) == (C, R) and ptT.hdr.data_ptr() == st.whdr[i].data_ptr(), w
            _same_image(wTpl[ptT.p_off:ptT.p_off + C * ptT.ld2], P.pack_transposed(W, s, ptT.ld2)[0], w + " W^T planes")
        else:
            assert name not in st.wTpt, w
    assert n_tr > 0


@pytest.mark.parametrize("name", ["img_d32_N2", "id_d32_N2"])
def test_parameter_store_planes_are_the_split_of_the_weights_a_step_runs_on(name):
    """ParamStore._refresh_p32 (descriptor packing, p_off / ld2 / hdr of every PT) and the invariant around a step: a training step
    splits the weights it starts from -- eager, recorded and replayed alike, also when an evaluation pass had already made the
    planes current before record() -- and ``ensure()`` after a step leaves the split of the updated weights."""
    from segmminterest_amd import hipabi as H
    from segmminterest_amd.synth import make_batch
    from segmminterest_amd.trainer import Trainer
    if H.GEMM_ENGINE != H.ENGINE_F16X3P:
        pytest.skip("plane engine only")
    assert name in MODEL_CASES
    cfg, g, _, _ = load_case(name)
    model = build_model(cfg)
    model.load_state_dict(g["sd"])
    model = model.cuda()
    st = model._store
    tr = Trainer(model, lr=1e-2, weight_decay=1e-4, device_state=True, dropout=False)          # large lr: every step moves every weight's planes
    batches = [{k: v.to(DEV) for k, v in make_batch(16, cfg["S"], cfg["Lt"], cfg["D_in"], n_users=cfg.get("n_users") or 50,
                                                    n_items=cfg.get("n_items") or 500, seed=810 + i, features=cfg["D_in"] > 0).items()}
               for i in range(2)]

    def host_flat():
        torch.cuda.synchronize()
        return st.flat.detach().cpu().numpy().copy()

    st.ensure()
    _check_store(st, host_flat(), "fresh model")

    def step(fn, batch, what):
        before = host_flat()
        fn(batch)
        after = host_flat()
        moved = [n for (n, off, R, C, _) in st._wmats if not np.array_equal(before[off:off + R * C], after[off:off + R * C])]
        assert len(moved) > len(st._wmats) // 2, (what, "the step did not move the weights")
        _check_store(st, before, what)

    step(tr.train_step, batches[0], "eager step 1")
    step(tr.train_step, batches[1], "eager step 2")
    st.ensure()          # what an evaluation pass between two steps does: the planes follow the optimizer
    _check_store(st, host_flat(), "ensure() after a step")
    step(lambda b: tr.record(b, prev_batch=batches[1]), batches[0], "recorded step")          # planes current at record(): the split is recorded all the same
    step(tr.run_recorded, batches[1], "replay 1")
    step(tr.run_recorded, batches[0], "replay 2")
    st.ensure()
    _check_store(st, host_flat(), "ensure() after a replay")
