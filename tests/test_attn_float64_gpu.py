"""Every form of the attention kernels for head dims <= 64 (csrc/attention.h, attention16.h, attention_lds.h, attention_pl.h)
against the float64 statement of tests/attn_ref.py, each output under the first-order bound derived there.  Operands are column
slices of fused projection buffers (the engine's layout); every output goes into a buffer wider and longer than its documented
region, pre-filled with a recorded pattern, and every word outside that region is compared bit for bit afterwards.

The cases are generated from (form, shape) pairs the restated dispatch rule (attn_ref.fwd_instance / bwd_instance) accepts; each
case carries the kernel instance it means to test and asserts that the rule, fed with the knobs read back from the library,
names it.  A knob variant whose launches are those of the default knobs at that shape is not generated a second time.
The planes-in forms need H dh % 32 == 0 (plane slices start at multiples of 32 columns): the two shapes of the list with
H dh = 144 and 48 run their planes-in cases with one head more (``_pl_shape``); the instances reached do not depend on H.

Run with ``pytest -m gpu -s`` to see the worst error / bound per (form, output); SEGMM_ATTN_RATIO_LOG=path writes them to a file.
tests/test_attn_ref_cpu.py shows without a GPU that the bounds accept a faithful fp32 emulation and reject planted defects."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as R      # noqa: E402
import p32_ref as P32      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED, SITE = 11, 3          # the dropout stream of every case; the preconditions on the multipliers are asserted for it
RATIOS = {}
KNOB_NAMES = ("ATT_FWD_PL", "ATT_FWD_LDS", "ATT_FWD_KSPLIT", "ATT_STREAM", "ATT_FUSED_LAUNCH", "ATT_MERGE", "ATT_WAVES", "ATT_WAVES_PL")


def _abi():
    from segmminterest_amd import hipabi
    hipabi.lib()
    return hipabi


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    lines = ["%-34s worst error / bound %.3g" % ("%s %s" % k, v) for k, v in sorted(RATIOS.items())]
    print("\n" + "\n".join(lines))
    path = os.environ.get("SEGMM_ATTN_RATIO_LOG")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


def _check(form, name, got, want, bound, what):
    r = R.ratio(got, want, bound)
    RATIOS[(form, name)] = max(RATIOS.get((form, name), 0.0), r)
    assert r <= 1.0, "%s %s %s: error / bound = %.4g" % (form, name, what, r)


class _Knobs:
    """Set knobs and the attention mode for a block; everything is restored on the way out."""

    def __init__(self, H, knobs, mode=None):
        self.H, self.knobs, self.mode, self.prev = H, knobs, mode, []

    def __enter__(self):
        self.prev_mode = self.H.attn_mode(-1)
        try:
            for k, v in self.knobs.items():
                self.prev.append((k, self.H.config_set(k, v)))
            if self.mode is not None:
                self.H.attn_mode(self.mode)
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        for k, v in reversed(self.prev):
            self.H.config_set(k, v)
        self.H.attn_mode(self.prev_mode)

    def live(self):
        """the knobs as the library holds them now, and the mode"""
        return {k: self.H.knob(k) for k in KNOB_NAMES}, self.H.attn_mode(-1)


# ------------------------------------------------------------------ inputs on the device, references (computed once, never modified)
def _pl_shape(shape):
    B0, H, dh, Lq, La, Lb = shape
    while (H * dh) % 32:
        H += 1
    return (B0, H, dh, Lq, La, Lb)


_DEVC, _REFC, _BNDC = {}, {}, {}


def _site_planes(H, x, rows, cols):
    """P32 planes + complete site header of x under the exact scale of its maxima (as test_planes_gpu._site_planes, mode 0)"""
    hdr = H.new_site(x.device)[0]
    pl = torch.empty((rows, 2 * cols), dtype=torch.float16, device=x.device)
    H.absmax(x, rows, cols, cols, out=hdr[H.SITE_HDR:])
    H.split_p32(x, rows, cols, cols, pl, 2 * cols, hdr, mode=0)
    return pl, hdr


def _held(pl, hdr, rows, cols):
    """the values the planes hold: hi + lo under the site scale"""
    v = pl.view(rows, cols // 32, 2, 32).double()
    return ((v[:, :, 0] + v[:, :, 1]) / float(hdr[0])).reshape(rows, cols).cpu().numpy()


def _dev(shape, planes=False):
    key = (shape, planes)
    if key not in _DEVC:
        H = _abi()
        inp = R.make_inputs(shape)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        dv = dict(inp=inp, Yv=t(inp["Yv"]), Yu=t(inp["Yu"]), dO=t(inp["dO"]), mq=t(inp["mq"]), mka=t(inp["mka"]), mkb=t(inp["mkb"]))
        dv["Qs"] = dv["Yv"] if inp["Qs"] is inp["Yv"] else t(inp["Qs"])
        if planes:
            d = shape[1] * shape[2]
            plv, hv = _site_planes(H, dv["Yv"], dv["Yv"].shape[0], 4 * d)
            plu, hu = _site_planes(H, dv["Yu"], dv["Yu"].shape[0], 2 * d)
            plq, hq = (plv, hv) if dv["Qs"] is dv["Yv"] else _site_planes(H, dv["Qs"], dv["Qs"].shape[0], 4 * d)
            dv["pin"] = dict(q=(plq, hq, 8 * d), a=(plv, hv, 8 * d), b=(plu, hu, 4 * d))
            hYv, hYu = _held(plv, hv, dv["Yv"].shape[0], 4 * d), _held(plu, hu, dv["Yu"].shape[0], 2 * d)
            dv["held"] = (hYv, hYu, hYv if dv["Qs"] is dv["Yv"] else _held(plq, hq, dv["Qs"].shape[0], 4 * d))
        _DEVC[key] = dv
    return _DEVC[key]


def _ref(shape, p, held=False):
    """The float64 statement under the kernels' own dropout stream; ``held``: on the values the input planes hold"""
    key = (shape, p, held)
    if key not in _REFC:
        H = _abi()
        B0, H_, dh, Lq, La, Lb = shape
        dv = _dev(shape, planes=held)
        inp = dv["inp"]
        n = inp["B"] * H_ * Lq * (R.r16(La) + R.r16(Lb))
        mult = torch.ones(n, device=DEV)
        if p > 0:
            H.dropout_mult(mult, n, p, SEED, SITE)
        mult = mult.cpu().numpy().reshape(inp["B"], H_, Lq, -1)
        ops = R.operands(inp, *dv["held"]) if held else R.operands(inp)
        st = R.statement(ops, inp["mq"], inp["mka"], inp["mkb"], H_, mult, inp["dO"])
        if p > 0:          # conditions on the inputs: the reference's quirk is exercised
            dropped = st["mu"] == 0
            thresh = int(float(np.float32(p)) * 65536.0 + 0.5)          # make_drop (common.h): p quantised to 16 bits
            assert set(np.unique(mult)) == {np.float32(0.0), np.float32(65536.0 / (65536.0 - thresh))}
            assert (dropped & ~st["valid"]).any(), "no masked key is dropped under seed %d" % SEED
            assert (dropped & ~inp["mq"][:, None, :, None]).any(), "no masked query row has a dropped key under seed %d" % SEED
        _REFC[key] = st
    return _REFC[key]


def _bounds_fwd(shape, p, held, rep, merge):
    key = ("f", shape, p, held, rep, merge)
    if key not in _BNDC:
        _BNDC[key] = R.bounds_fwd(_ref(shape, p, held), rep, merge)
    return _BNDC[key]


def _bounds_bwd(shape, p, held, fwd_key, rep):
    key = ("b", shape, p, held, fwd_key, rep)
    if key not in _BNDC:
        _BNDC[key] = R.bounds_bwd(_ref(shape, p, held), _bounds_fwd(shape, p, held, *fwd_key), rep)
    return _BNDC[key]


# ------------------------------------------------------------------ guarded output buffers
def _pattern(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, cols, generator=g) * 1000.0 + 3000.0).to(DEV)


class _Guarded:
    """An output buffer with a recorded pattern; ``written`` marks the documented output region."""

    def __init__(self, rows, cols, seed):
        self.t = _pattern(rows, cols, seed)
        self.before = self.t.clone()
        self.written = torch.zeros(rows, cols, dtype=torch.bool, device=DEV)

    def region(self, rows, c0, c1):
        self.written[:rows, c0:c1] = True
        return self

    def assert_outside_untouched(self, what):
        a, b = self.t.view(torch.int32), self.before.view(torch.int32)
        moved = (a != b) & ~self.written
        assert not bool(moved.any()), "%s: %d words outside the documented output region were written" % (what, int(moved.sum()))
        same = (a == b) & self.written          # (a documented word that kept the pattern was not stored)
        assert not bool(same.any()), "%s: %d words of the output region were never written" % (what, int(same.sum()))


def _views(dv, shape, with_f32=True):
    B0, H_, dh, Lq, La, Lb = shape
    d = H_ * dh
    t = (lambda x: x) if with_f32 else (lambda x: None)
    return ((t(dv["Qs"]), 0), (t(dv["Qs"]), d), 4 * d, (t(dv["Yv"]), 2 * d) if La else None, (t(dv["Yv"]), 3 * d) if La else None, 4 * d,
            (t(dv["Yu"]), 0) if Lb else None, (t(dv["Yu"]), d) if Lb else None, 2 * d)


def _masks(dv, shape):
    return dv["mq"], dv["mka"] if shape[4] else None, dv["mkb"] if shape[5] else None


def _run_fwd(H, shape, p, dv, pin, with_f32, amax=False, po=False):
    B0, H_, dh, Lq, La, Lb = shape
    B, d = dv["inp"]["B"], H_ * dh
    O = _Guarded(B * Lq + 3, d + 8, 1).region(B * Lq, 0, d)
    lse = _Guarded(1, 2 * B * H_ * Lq + 5, 2).region(1, 0, 2 * B * H_ * Lq)
    am = torch.zeros(H.AMAX_SLOTS, device=DEV) if amax else None
    pout = None
    if po:
        hdr = H.new_site(DEV)[0]
        sc = torch.tensor([2.0 ** 12], dtype=torch.float32, device=DEV)
        pl = torch.zeros((B * Lq, 2 * d), dtype=torch.float16, device=DEV)
        pout = (pl, hdr, sc, H.PO(pl, 2 * d, hdr, sc.data_ptr()))
    H.attn_fwd(dv["inp"]["B"], H_, dh, Lq, La, Lb, *_views(dv, shape, with_f32), *_masks(dv, shape), O.t, d + 8, lse.t,
               drop_p=p, seed=SEED, site=SITE, amax_o=am, po=pout[3] if po else None, pin=pin)
    torch.cuda.synchronize()
    return O, lse, am, pout


# ------------------------------------------------------------------ forward
FWD_FORMS = {          # name -> (knobs, pin, fp32 views)
    "default": ({}, False, True),
    "direct": ({"ATT_FWD_LDS": 0}, False, True),
    "staged_k1": ({"ATT_FWD_LDS": 2, "ATT_FWD_KSPLIT": 1}, False, True),
    "staged_k2": ({"ATT_FWD_LDS": 2, "ATT_FWD_KSPLIT": 2}, False, True),
    "staged_k3": ({"ATT_FWD_LDS": 2, "ATT_FWD_KSPLIT": 3}, False, True),
    "planes": ({}, True, True),
    "planes_only": ({}, True, False),
}


def _fwd_cases():
    out = []
    for shape0 in R.SHAPES:
        for form, (knobs, pin, f32) in FWD_FORMS.items():
            shape = _pl_shape(shape0) if pin else shape0
            inst = R.fwd_instance(*shape[2:], pin=pin, knobs=knobs, f32_views=f32)
            if form == "direct" and not inst.startswith("fwd<"):
                continue
            if form.startswith("staged") and not (inst.startswith("fwd_lds<") and inst.endswith("ksp" + form[-1])):
                continue          # no staged form here (head dim < 16, K / V over 80 KB), or the split is capped at this shape
            if pin and not inst.startswith("fwd_pl<"):
                continue
            for p in R.drop_ps(shape0):
                out.append(pytest.param(form, shape, p, inst, id="%s-%s-p%g" % (form, "x".join(map(str, shape)), p)))
    return out


@pytest.mark.parametrize("form,shape,p,inst", _fwd_cases())
def test_attention_forward_against_float64(form, shape, p, inst):
    H = _abi()
    B0, H_, dh, Lq, La, Lb = shape
    knobs, pin, f32 = FWD_FORMS[form]
    dv = _dev(shape, planes=pin)
    B, d = dv["inp"]["B"], H_ * dh
    with _Knobs(H, knobs) as kn:
        live, _ = kn.live()
        assert R.fwd_instance(dh, Lq, La, Lb, pin=pin, knobs=live, f32_views=f32) == inst
        O, lse, am, _ = _run_fwd(H, shape, p, dv, dv["pin"] if pin else None, f32, amax=True)
        # (with a plane output the maxima go to its site header: a run of its own)
        O2, lse2, _, po = _run_fwd(H, shape, p, dv, dv["pin"] if pin else None, f32, po=True) if d % 32 == 0 else (None, None, None, None)
    rep, merge = ("planes" if pin else "f32"), R.fwd_ksplit(inst) > 1
    st, bf = _ref(shape, p, held=pin), _bounds_fwd(shape, p, pin, rep, merge)
    what = "%s p=%g (%s)" % (shape, p, inst)
    O.assert_outside_untouched("O " + what)
    lse.assert_outside_untouched("lse " + what)
    Ok = O.t[:B * Lq, :d].cpu().numpy()
    l = lse.t[0, :2 * B * H_ * Lq].cpu().numpy().reshape(2, B, H_, Lq)
    tag = "fwd " + form
    _check(tag, "O", Ok.reshape(B, Lq, d), st["O"], bf["O"], what)
    _check(tag, "lse.max", l[0], st["m"], bf["m"], what)
    _check(tag, "lse.inv", l[1], st["inv"], bf["inv"], what)
    assert float(am.max()) == float(np.abs(Ok).max()), "amax_o " + what
    if po is not None:          # the plane output is the host split of the kernel's own fp32 O
        assert torch.equal(O2.t, O.t) and torch.equal(lse2.t, lse.t), "po run " + what
        want, _ = P32.pack(Ok, 2.0 ** 12)
        got = po[0].cpu().view(torch.int16).numpy().view(want.dtype).reshape(-1)
        assert (got == want).all() and float(po[1][0]) == 2.0 ** 12, "po " + what


# ------------------------------------------------------------------ backward
BWD_FORMS = {          # name -> (phases, mode, knobs, pin, fp32 views)
    "phase0": ((0,), None, {}, False, True),
    "phases123": ((1, 2, 3), None, {}, False, True),
    "fused_m0": ((4,), 0, {}, False, True),
    "fused_m1": ((4,), 1, {}, False, True),
    "fused_m2": ((4,), 2, {}, False, True),
    "merge0_m0": ((4,), 0, {"ATT_MERGE": 0}, False, True),
    "launch1_m0": ((4,), 0, {"ATT_FUSED_LAUNCH": 1}, False, True),
    "launch1_m2": ((4,), 2, {"ATT_FUSED_LAUNCH": 1}, False, True),
    "waves1_m2": ((4,), 2, {"ATT_WAVES": 1}, False, True),
    "phases56": ((5, 6), None, {}, False, True),
    "pl_w1": ((4,), None, {"ATT_WAVES_PL": 1}, True, True),
    "pl_w3": ((4,), None, {"ATT_WAVES_PL": 3}, True, True),
    "pl_only": ((4,), None, {}, True, False),
}
_BASE = {"merge0_m0": "fused_m0", "launch1_m0": "fused_m0", "launch1_m2": "fused_m2", "waves1_m2": "fused_m2", "pl_w1": "pl_w3"}


def _bwd_insts(shape, form):
    phases, mode, knobs, pin, f32 = BWD_FORMS[form]
    return tuple(R.bwd_instance(*shape[2:], ph, mode=1 if mode is None else mode, pin=pin, knobs=knobs, f32_views=f32) for ph in phases)


def _bwd_cases():
    out = []
    for shape0 in R.SHAPES:
        for form, (phases, mode, knobs, pin, f32) in BWD_FORMS.items():
            shape = _pl_shape(shape0) if pin else shape0
            if pin and not (shape[2] in (16, 32, 48) and R.fwd_pl_takes(*shape[2:], True)):
                continue
            insts = _bwd_insts(shape, form)
            if form in _BASE and insts == _bwd_insts(shape, _BASE[form]):
                continue          # the knob changes nothing at this shape: the base form's case is this one
            assert not any(n.startswith("!") for ph in insts for n in ph), (form, shape, insts)
            if pin:
                assert all(n.startswith("pl<") for ph in insts for n in ph), (form, shape, insts)
            for p in R.drop_ps(shape0):
                out.append(pytest.param(form, shape, p, insts, id="%s-%s-p%g" % (form, "x".join(map(str, shape)), p)))
    return out


@pytest.mark.parametrize("form,shape,p,insts", _bwd_cases())
def test_attention_backward_against_float64(form, shape, p, insts):
    H = _abi()
    B0, H_, dh, Lq, La, Lb = shape
    phases, mode, knobs, pin, f32 = BWD_FORMS[form]
    dv = _dev(shape, planes=pin)
    B, d = dv["inp"]["B"], H_ * dh
    # the forward that precedes this backward in the engine: default knobs; the planes-in forward in front of the planes-in backward
    fwd_inst = R.fwd_instance(dh, Lq, La, Lb, pin=pin, f32_views=f32)
    assert fwd_inst.startswith("fwd_pl<") == pin
    O, lse, _, _ = _run_fwd(H, shape, p, dv, dv["pin"] if pin else None, f32)
    fwd_key = ("planes" if pin else "f32", R.fwd_ksplit(fwd_inst) > 1)
    rep = R.rep_of([n for ph in insts for n in ph])
    st, bb = _ref(shape, p, held=pin), _bounds_bwd(shape, p, pin, fwd_key, rep)
    what = "%s p=%g %s" % (shape, p, insts)
    own_q = dv["Qs"] is not dv["Yv"]
    gYv = _Guarded(dv["Yv"].shape[0] + 2, 4 * d, 3)
    gYu = _Guarded(dv["Yu"].shape[0] + 2, 2 * d, 4)
    gQ = _Guarded(B * Lq + 2, 4 * d, 5) if own_q else gYv
    Dv = _Guarded(1, B * H_ * Lq + 5, 6)
    if La:
        gQ.region(B * Lq, 0, d)
        gYv.region(B * La, 2 * d, 4 * d)
    if Lb:
        gQ.region(B * Lq, d, 2 * d)
        gYu.region(B * Lb, 0, 2 * d)
    grads = ((gQ.t, 0) if La else None, (gQ.t, d) if Lb else None, 4 * d, (gYv.t, 2 * d) if La else None, (gYv.t, 3 * d) if La else None, 4 * d,
             (gYu.t, 0) if Lb else None, (gYu.t, d) if Lb else None, 2 * d)
    tag = "bwd " + form
    with _Knobs(H, knobs, mode) as kn:
        live, live_mode = kn.live()
        for ph, want in zip(phases, insts):
            assert R.bwd_instance(dh, Lq, La, Lb, ph, mode=live_mode, pin=pin, knobs=live, f32_views=f32) == want
            H.attn_bwd(B, H_, dh, Lq, La, Lb, *_views(dv, shape, f32), *_masks(dv, shape), lse.t, O.t, d + 8, dv["dO"], d, Dv.t, *grads,
                       drop_p=p, seed=SEED, site=SITE, phase=ph, pin=dv["pin"] if pin else None)
            torch.cuda.synchronize()
            if ph == 1:          # D alone, before the kernels that consume it
                Dv.region(1, 0, B * H_ * Lq)
                _check(tag, "D", Dv.t[0, :B * H_ * Lq].cpu().numpy().reshape(B, H_, Lq), st["D"], bb["D"], what)
    if phases == (0,):          # the whole backward stores D from its dQ kernel
        Dv.region(1, 0, B * H_ * Lq)
        _check(tag, "D", Dv.t[0, :B * H_ * Lq].cpu().numpy().reshape(B, H_, Lq), st["D"], bb["D"], what)
    Dv.assert_outside_untouched("Dvec " + what)          # (the fused backward forms D in LDS: it leaves Dvec alone altogether)
    for g_, nm in ((gQ, "dQ buffer"), (gYv, "dYv"), (gYu, "dYu")):
        g_.assert_outside_untouched(nm + " " + what)
    dq = gQ.t[:B * Lq].cpu().numpy().reshape(B, Lq, 4 * d)
    if La:
        yv = gYv.t[:B * La].cpu().numpy().reshape(B, La, 4 * d)
        _check(tag, "dQa", dq[..., :d], st["dQa"], bb["dQa"], what)
        _check(tag, "dKa", yv[..., 2 * d:3 * d], st["dKa"], bb["dKa"], what)
        _check(tag, "dVa", yv[..., 3 * d:], st["dVa"], bb["dVa"], what)
    if Lb:
        yu = gYu.t[:B * Lb].cpu().numpy().reshape(B, Lb, 2 * d)
        _check(tag, "dQb", dq[..., d:2 * d], st["dQb"], bb["dQb"], what)
        _check(tag, "dKb", yu[..., :d], st["dKb"], bb["dKb"], what)
        _check(tag, "dVb", yu[..., d:], st["dVb"], bb["dVb"], what)


def test_every_form_and_instance_of_the_list_is_present():
    """The generated cases reach every kernel family at least once, and the knobs are back at their defaults."""
    H = _abi()
    fw = {c.values[3].split("<")[0] for c in _fwd_cases()} | {"ksp%d" % R.fwd_ksplit(c.values[3]) for c in _fwd_cases()}
    assert {"fwd", "fwd_lds", "fwd_pl", "ksp1", "ksp2", "ksp3"} <= fw
    assert "fwd_pl<48,9,40,hot>" in {c.values[3] for c in _fwd_cases()}
    names = {n for c in _bwd_cases() for ph in c.values[3] for n in ph}
    fam = {n.split("<")[0] for n in names}
    assert {"D", "dq", "dkv", "fused", "fused16", "pl"} <= fam
    for piece in ("merged,16>", "merged,32>", ",16>a", ",32>a", ",one>", ",chunks>", ">ab/", "fused<48,12,one>a/w11", "fused<16,8,chunks>a/w6",
                  "fused16<48,4,one>b/w4", "fused16<48,4,one>b/w1", "pl<48,4,one>b/w3", "pl<48,4,one>b/w1", "pl<16,8,chunks>"):
        assert any(piece in n for n in names), piece
    assert {k: H.knob(k) for k in KNOB_NAMES} == R.KNOBS and H.attn_mode(-1) == 1
