"""The embedding LayerNorm gradients as planes only (csrc/rowops.h layernorm_bwd_kernel with dx == NULL and its REPAIR form; library
knob DPRE_PLANES_ONLY; engine.BackboneRun.backward): everything is a statement about bits, so every check is bitwise.

Kernel level (through hipabi): the launch without dx leaves the planes, the site header, the maxima and the three partial buffers of
the launch with dx; after a wrong delayed scale, segmm_site_fixup + the repair launch leave the exact split of dx and touch nothing
else; a good site is left alone; the argument rules fail with the library's error.  Shapes: d = 64 (one float4 per lane) and 768
(three), sequences of 8 and 12 tokens, 6 sequences (every wave walks one row) and one grid whose waves walk 2 or 3 rows
(LN_BWD_PARTS = 64: 63 workgroups for 600 rows) -- the smallest at which a null dx, the per-position grid and the row tail can go
wrong.  Model level: three trainer steps with the knob at 0 and at 2, eager and recorded.  Run with ``pytest -m gpu``."""
import contextlib

import pytest
import torch

from helpers import build_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED, SITE_Y = 77, 5
# (d, period, rows, LN_BWD_PARTS)
SHAPES = [(64, 8, 48, 0), (64, 12, 72, 0), (768, 8, 48, 0), (768, 12, 72, 0), (768, 12, 600, 64)]


def _abi():
    from segmminterest_amd import hipabi
    hipabi.lib()
    return hipabi


@contextlib.contextmanager
def _knob(H, name, value):
    prev = H.config_set(name, value)
    try:
        yield
    finally:
        H.config_set(name, prev)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


_CASES = {}


def _case(H, d, period, rows, parts_knob, p):
    """Inputs, the forward's statistics, the fp32 launch's dx, its exact split (planes + header) and the fitting power-of-two scale;
    made once per shape and left unchanged."""
    key = (d, period, rows, parts_knob, p)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(d + 7 * period + rows)
    x = (torch.randn(rows, d, generator=g) * 1.5 + 0.3).to(DEV)
    dy = (torch.randn(rows, d, generator=g) * 0.02).to(DEV)
    gamma = (1 + 0.1 * torch.randn(d, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(d, generator=g)).to(DEV)
    y, mean, rstd = torch.empty(rows, d, device=DEV), torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    H.layernorm_fwd(x, gamma, beta, y, mean, rstd)
    with _knob(H, "LN_BWD_PARTS", parts_knob):
        parts = H.layernorm_bwd_pos_parts(rows, period, d)
        assert parts > 0 and (4 * parts) % period == 0
        if parts_knob:
            assert rows % (4 * parts) != 0 and rows > 8 * parts          # waves walk 2 or 3 rows
        dx = torch.empty(rows, d, device=DEV)
        pg, pb, pp = (torch.empty(n, d, device=DEV) for n in (parts, parts, 4 * parts))
        H.layernorm_bwd_pos(dy, x, mean, rstd, gamma, dx, None, pg, pb, pp, period, drop_y_p=p, drop_y_site=SITE_Y, seed=SEED)
    hdr = H.new_site(DEV)[0]
    H.absmax(dx, rows, d, d, out=hdr[H.SITE_HDR:])
    exact = torch.empty(rows, 2 * d, dtype=torch.float16, device=DEV)
    H.split_p32(dx, rows, d, d, exact, 2 * d, hdr, mode=0)
    fit = float(hdr[0])
    assert 2.0 ** 14 <= float(dx.abs().max()) * fit < 2.0 ** 15
    _CASES[key] = dict(x=x, dy=dy, gamma=gamma, mean=mean, rstd=rstd, parts=parts, dx=dx, exact=exact, fit=fit, part=(pg, pb, pp))
    return _CASES[key]


def _launch(H, c, d, period, parts_knob, p, scale, with_dx):
    """One per-position launch with a plane output written with ``scale``, the maxima folded into the site header as the engine
    does; every output pre-filled.  -> dict of the outputs."""
    rows, parts = c["x"].shape[0], c["parts"]
    sc = torch.full((1,), scale, device=DEV)
    hdr = H.new_site(DEV)[0]
    planes = torch.full((rows, 2 * d), 3.0, dtype=torch.float16, device=DEV)
    dx = torch.full((rows, d), -7.0, device=DEV)
    pg, pb, pp = (torch.full((n, d), 5.0, device=DEV) for n in (parts, parts, 4 * parts))
    po = H.PO(planes, 2 * d, hdr, sc.data_ptr())
    with _knob(H, "LN_BWD_PARTS", parts_knob):
        H.layernorm_bwd_pos(c["dy"], c["x"], c["mean"], c["rstd"], c["gamma"], dx if with_dx else None, None, pg, pb, pp, period,
                            drop_y_p=p, drop_y_site=SITE_Y, seed=SEED, amax=hdr[H.SITE_HDR:], po=po)
    torch.cuda.synchronize()
    return dict(sc=sc, hdr=hdr, planes=planes, dx=dx, pg=pg, pb=pb, pp=pp, po=po)


def _repair(H, c, o, period, parts_knob, p):
    with _knob(H, "LN_BWD_PARTS", parts_knob):
        H.layernorm_bwd_pos_repair(c["dy"], c["x"], c["mean"], c["rstd"], c["gamma"], period, o["po"], drop_y_p=p, drop_y_site=SITE_Y,
                                   seed=SEED)
    torch.cuda.synchronize()


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("d,period,rows,parts_knob", SHAPES)
def test_null_dx_leaves_the_same_bits(d, period, rows, parts_knob, p):
    """dx = None against today's launch: planes, header words, maxima slots and the three partial buffers bit for bit; the fp32
    launch's dx is the reference's; a sentinel-filled dx buffer that is passed nowhere stays untouched."""
    H = _abi()
    c = _case(H, d, period, rows, parts_knob, p)
    a = _launch(H, c, d, period, parts_knob, p, c["fit"], True)
    b = _launch(H, c, d, period, parts_knob, p, c["fit"], False)
    assert _same(a["dx"], c["dx"])
    assert float(a["hdr"][0]) == c["fit"] and float(a["hdr"][1]) == 0.0
    assert float(a["hdr"][H.SITE_HDR:].max()) == float(c["dx"].abs().max())
    assert _same(a["planes"], c["exact"])          # (the fitting scale is the exact one)
    for k in ("planes", "hdr", "pg", "pb", "pp"):
        assert _same(a[k], b[k]), k
    for k, r in zip(("pg", "pb", "pp"), c["part"]):
        assert _same(a[k], r), k
    assert bool((b["dx"] == -7.0).all())


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("off", [30, -30])
@pytest.mark.parametrize("d,period,rows,parts_knob", SHAPES)
def test_repair_rewrites_the_planes_with_the_exact_scale(d, period, rows, parts_knob, off, p):
    """A delayed scale 2^30 too large (overflow flag) or 2^-30 too small (maximum below the window): after the planes-only launch,
    site_fixup and the repair launch the planes are the exact split of the fp32 launch's dx, hdr[0] is that split's scale,
    hdr[2] != 0, and the partial buffers are the ones the first launch left."""
    H = _abi()
    c = _case(H, d, period, rows, parts_knob, p)
    o = _launch(H, c, d, period, parts_knob, p, c["fit"] * 2.0 ** off, False)
    assert (float(o["hdr"][1]) != 0.0) == (off > 0)
    assert not _same(o["planes"], c["exact"])
    before = {k: o[k].clone() for k in ("pg", "pb", "pp", "dx")}
    maxima = o["hdr"][H.SITE_HDR:].clone()
    stats = torch.zeros(8, device=DEV)
    H.site_fixup(o["hdr"], stats=stats)
    _repair(H, c, o, period, parts_knob, p)
    assert float(o["hdr"][0]) == c["fit"] and float(o["hdr"][2]) != 0.0 and float(o["hdr"][1]) == 0.0 and float(stats[0]) == 1.0
    assert _same(o["planes"], c["exact"])
    for k, r in zip(("pg", "pb", "pp"), c["part"]):
        assert _same(o[k], before[k]) and _same(o[k], r), k
    assert _same(o["dx"], before["dx"]) and _same(o["hdr"][H.SITE_HDR:], maxima)


@pytest.mark.parametrize("d,period,rows,parts_knob", SHAPES)
def test_repair_leaves_a_good_site_alone(d, period, rows, parts_knob):
    """A fitting scale: site_fixup leaves hdr[2] == 0 and the repair launch changes nothing -- shown on planes overwritten with a
    pattern between the two launches, which a repair pass that ran would replace."""
    H = _abi()
    c = _case(H, d, period, rows, parts_knob, 0.1)
    o = _launch(H, c, d, period, parts_knob, 0.1, c["fit"], False)
    assert _same(o["planes"], c["exact"])
    hdr0 = o["hdr"].clone()
    stats = torch.zeros(8, device=DEV)
    H.site_fixup(o["hdr"], stats=stats)
    assert float(o["hdr"][2]) == 0.0 and float(stats[0]) == 0.0 and _same(o["hdr"], hdr0)
    _repair(H, c, o, period, parts_knob, 0.1)
    assert _same(o["planes"], c["exact"])
    o["planes"].fill_(9.0)
    before = {k: o[k].clone() for k in ("pg", "pb", "pp", "dx", "hdr")}
    _repair(H, c, o, period, parts_knob, 0.1)
    assert bool((o["planes"] == 9.0).all())
    for k in before:
        assert _same(o[k], before[k]), k


def test_null_dx_argument_rules():
    """dx = None without a plane output, and dx = None next to dx_drop, fail with the library's error (no launch is made)."""
    H = _abi()
    d, period, rows = 64, 8, 48
    c = _case(H, d, period, rows, 0, 0.0)
    parts = c["parts"]
    pg, pb, pp = (torch.zeros(n, d, device=DEV) for n in (parts, parts, 4 * parts))
    with pytest.raises(RuntimeError, match="planes only"):
        H.layernorm_bwd_pos(c["dy"], c["x"], c["mean"], c["rstd"], c["gamma"], None, None, pg, pb, pp, period)
    with pytest.raises(RuntimeError, match="planes only"):
        H.layernorm_bwd(c["dy"], c["x"], c["mean"], c["rstd"], c["gamma"], None, None, pg, pb)
    sc = torch.full((1,), c["fit"], device=DEV)
    hdr = H.new_site(DEV)[0]
    planes = torch.zeros((rows, 2 * d), dtype=torch.float16, device=DEV)
    po = H.PO(planes, 2 * d, hdr, sc.data_ptr())
    dxd = torch.zeros(rows, d, device=DEV)
    with pytest.raises(RuntimeError, match="dx_drop"):
        H.layernorm_bwd_pos(c["dy"], c["x"], c["mean"], c["rstd"], c["gamma"], None, dxd, pg, pb, pp, period, po=po)
    po_noscale = H.PO(planes, 2 * d, hdr, None)
    with pytest.raises(RuntimeError, match="planes only"):
        H.layernorm_bwd_pos(c["dy"], c["x"], c["mean"], c["rstd"], c["gamma"], None, None, pg, pb, pp, period, po=po_noscale)
    torch.cuda.synchronize()
    assert not bool(planes.any()) and not bool(pg.any()) and not bool(dxd.any())


# ------------------------------------------------------------------ model level
def _trainer_case():
    from segmminterest_amd.synth import l1_normalize, make_batch
    B, S, Lt, D, N, h = 4, 8, 8, 64, 2, 4
    cfg = dict(N=N, h=h, S=S, d=D, D_in=D, Lt=Lt, user="image", photo="image", loss_type_list=["interestBPR"],
               loss_weight={"interestBPR": 1.0, "mse": 1.0}, exposure_prob=[1.0] * S)
    b = make_batch(B, S, Lt, D, seed=9)
    batch = dict(user=l1_normalize(b["user"]).to(DEV), photo=l1_normalize(b["photo"]).to(DEV), user_mask=b["user_mask"].to(DEV),
                 photo_mask=b["photo_mask"].to(DEV), label=b["label"].to(DEV), user_identity_id=b["user_identity_id"].to(DEV),
                 photo_identity_id=b["photo_identity_id"].to(DEV))
    return cfg, batch


def _three_steps(H, cfg, batch, knob, recorded):
    """Parameters and losses after three trainer steps (dropout 0.1, plane engine, delayed scales) that follow one calibrating
    step; ``recorded``: the three are replays of a recorded step.  Also -> whether the embedding sides ran planes only."""
    from segmminterest_amd import engine as E
    from segmminterest_amd.trainer import Trainer
    seen = []
    orig = E.H.layernorm_bwd_pos

    def spy(dy, x, mean, rstd, gamma, dx, *a, **k):
        seen.append(dx is None)
        return orig(dy, x, mean, rstd, gamma, dx, *a, **k)
    with _knob(H, "DPRE_PLANES_ONLY", knob):
        torch.manual_seed(5)
        model = build_model(cfg)
        tr = Trainer(model.cuda(), device_state=True)
        tr.normalize = lambda key, x, *a, **k: x             # already L1-normalised
        E.H.layernorm_bwd_pos = spy
        try:
            if recorded:
                tr.record(batch, warmup=1)
            else:
                for _ in range(2):
                    tr.train_step(batch)
            losses = [float((tr.run_recorded(batch) if recorded else tr.train_step(batch))["loss"].detach()) for _ in range(3)]
        finally:
            E.H.layernorm_bwd_pos = orig
        torch.cuda.synchronize()
    return model._store.flat.detach().clone(), losses, seen


def test_model_steps_bitwise_with_and_without_the_fp32_copy():
    """image / image, N = 2, d = 64, h = 4, B = 4, S = 8, Lt = 8, dropout 0.1: every parameter after three eager steps is bitwise
    the same with the knob at 0 and at 2, and a recorded step replayed three times leaves what the eager steps leave.  (At this
    shape the per-position grid is the plain grid -- 8 workgroups, one row per wave -- so knob 2 changes no summation order.)"""
    H = _abi()
    if H.GEMM_ENGINE != H.ENGINE_F16X3P:
        pytest.fail("the planes-only embedding gradients belong to the plane engine (SEGMM_GEMM unset or f16x3p)")
    cfg, batch = _trainer_case()
    p0, l0, s0 = _three_steps(H, cfg, batch, 0, False)
    p2, l2, s2 = _three_steps(H, cfg, batch, 2, False)
    pr, lr_, sr = _three_steps(H, cfg, batch, 2, True)
    assert not any(s0)          # knob 0: no per-position launch at this size, let alone one without dx
    assert s2[-2:] == [True, True] and sr and all(sr[-2:])          # both sides planes only once the sites are calibrated
    assert torch.isfinite(p0).all() and l0 == l2 == lr_
    assert _same(p0, p2)
    assert _same(p2, pr)
