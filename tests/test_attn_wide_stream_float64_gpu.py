"""The attention kernels the float64 statement did not reach: head dims 96 and 128 (the direct forward, D, dQ, dK/dV at four waves
per workgroup and attn_bwd_fused_wide_kernel, csrc/attention_wide.h), the streamed kernels of csrc/attention_stream.h at every built
head dim (ATT_STREAM = 1 at small shapes; above 192 padded keys by themselves, up to the 16 + 16 tiles they accept) and the
workgroup-shape knobs ATT_HPB_FWD / _DQ / _DKV.  Every output is held to the per-element first-order bound derived in
tests/attn_ref.py (the streamed forward under its own counted constants, ``bounds_fwd(stream=nt)``); the only pass criterion is
error / bound <= 1.

The machinery is that of test_attn_float64_gpu.py and is imported from there, not copied: operands as column slices of fused
buffers, guarded outputs (ld > width, spare rows, a recorded pattern, every word outside the documented region compared bit for
bit), the kernels' own dropout stream, three extra batch rows (block a masked, everything masked, fully valid) and the knob
context.  Each case carries the launches it means to reach -- with the workgroup shape and, for the wide fused kernel, the wave and
pass counts -- and asserts that the restated rule (attn_ref.fwd_launch / bwd_launch), fed the knobs read back from the library,
names them.  The dropout seed and site are attn_ref.DROP_SEED / DROP_SITE (11, 3), chosen once: tests/test_attn_ref_cpu.py checks
their preconditions at every p > 0 shape on the host restatement of the stream, and this module asserts that the library's
exported stream is that restatement.

Workgroup shape and bits.  attn_fwd_kernel, attn_fwd_stream_kernel, attn_bwd_dq_kernel, attn_bwd_dq_stream_kernel and
attn_bwd_dkv_kernel are one-wave-per-tile kernels: a wave derives (b, h, tile) from its place in the grid and the shape
(``wave / wq``, ``wave % wq``) and then works from global memory and its own registers alone; what the waves of a workgroup share
is the key-flag bytes and, in the dK/dV kernel, the per-head row statistics in LDS -- copies of inputs, no arithmetic.  The
arithmetic of a (head, tile) therefore does not depend on wq or hpb, and the ATT_HPB_* cases assert bit equality with the default
launch on top of the bounds, for all five kernels.

Run with ``pytest -m gpu -s`` to see the worst error / bound per (form, output); SEGMM_ATTN_RATIO_LOG=path writes them to a file
(profiles/attn_wide_stream_float64/ratios.txt is such a file)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as R      # noqa: E402
import p32_ref as P32      # noqa: E402
import test_attn_float64_gpu as G      # noqa: E402  (the shared machinery; its own cases are collected from its own file only)

pytestmark = pytest.mark.gpu
DEV = "cuda"
assert (G.SEED, G.SITE) == (R.DROP_SEED, R.DROP_SITE)
RATIOS = {}
ALL_KNOBS = G.KNOB_NAMES + tuple(R.SHAPE_KNOBS)
STREAM1 = {"ATT_STREAM": 1}


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
    print("%s %s %s: error / bound = %.4g" % (form, name, what, r))
    RATIOS[(form, name)] = max(RATIOS.get((form, name), 0.0), r)
    assert r <= 1.0, "%s %s %s: error / bound = %.4g" % (form, name, what, r)


class _Knobs(G._Knobs):
    def live(self):
        return {k: self.H.knob(k) for k in ALL_KNOBS}, self.H.attn_mode(-1)


def _streamed(shape, knobs):
    return R.n_tiles(shape) > 12 or bool(knobs.get("ATT_STREAM"))


_BND = {}


def _bounds(shape, p, stream_fwd, rep="f32"):
    """(forward bounds, backward bounds) for a backward of representation ``rep`` behind a held (0) or streamed forward"""
    nt = R.n_tiles(shape) if stream_fwd else 0
    kf = ("f", shape, p, nt)
    if kf not in _BND:
        _BND[kf] = R.bounds_fwd(G._ref(shape, p), stream=nt)
    kb = ("b", shape, p, nt, rep)
    if kb not in _BND:
        _BND[kb] = R.bounds_bwd(G._ref(shape, p), _BND[kf], rep)
    return _BND[kf], _BND[kb]


def _id(form, shape, p):
    return "%s-%s-p%g" % (form, "x".join(map(str, shape)), p)


# (shape, knobs) of every streamed case: ATT_STREAM = 1 up to 192 padded keys, the default knobs above
STREAMED = [(s, STREAM1) for s in R.STREAM_SMALL + R.STREAM_FUSED_RUN] + [(s, {}) for s in R.STREAM_LONG + R.STREAM_FUSED]


# ------------------------------------------------------------------ forward
def _fwd_cases():
    out = []
    for shape in R.WIDE_SHAPES:
        inst = R.fwd_launch(*shape[1:])
        assert inst.startswith("fwd<%d," % shape[2]), inst
        out += [pytest.param("direct", shape, p, {}, inst, id=_id("direct", shape, p)) for p in R.drop_ps_x(shape)]
    for shape, knobs in STREAMED:
        inst = R.fwd_launch(*shape[1:], knobs=knobs)
        assert inst.startswith("fwd_stream<%d>" % shape[2]), inst
        out += [pytest.param("stream", shape, p, knobs, inst, id=_id("stream", shape, p)) for p in R.drop_ps_x(shape)]
    return out


def _forward(H, shape, p, knobs, inst, po=True):
    """run the forward under ``knobs``; returns (O, lse guarded buffers, amax, plane output run or None)"""
    B0, H_, dh, Lq, La, Lb = shape
    dv = G._dev(shape)
    with _Knobs(H, knobs) as kn:
        live, _ = kn.live()
        assert R.fwd_launch(H_, dh, Lq, La, Lb, knobs=live) == inst
        O, lse, am, _ = G._run_fwd(H, shape, p, dv, None, True, amax=True)
        run2 = G._run_fwd(H, shape, p, dv, None, True, po=True) if po and (H_ * dh) % 32 == 0 else None
    return O, lse, am, run2


def _check_forward(tag, shape, p, inst, O, lse, am, run2, stream_fwd):
    B0, H_, dh, Lq, La, Lb = shape
    B, d = R.batch_rows(shape), H_ * dh
    st, (bf, _) = G._ref(shape, p), _bounds(shape, p, stream_fwd)
    what = "%s p=%g (%s)" % (shape, p, inst)
    O.assert_outside_untouched("O " + what)
    lse.assert_outside_untouched("lse " + what)
    Ok = O.t[:B * Lq, :d].cpu().numpy()
    l = lse.t[0, :2 * B * H_ * Lq].cpu().numpy().reshape(2, B, H_, Lq)
    _check(tag, "O", Ok.reshape(B, Lq, d), st["O"], bf["O"], what)
    _check(tag, "lse.max", l[0], st["m"], bf["m"], what)
    _check(tag, "lse.inv", l[1], st["inv"], bf["inv"], what)
    assert float(am.max()) == float(np.abs(Ok).max()), "amax_o " + what
    if run2 is not None:          # the plane output is the host split of the kernel's own fp32 O
        O2, lse2, _, po = run2
        assert torch.equal(O2.t, O.t) and torch.equal(lse2.t, lse.t), "po run " + what
        want, _ = P32.pack(Ok, 2.0 ** 12)
        got = po[0].cpu().view(torch.int16).numpy().view(want.dtype).reshape(-1)
        assert (got == want).all() and float(po[1][0]) == 2.0 ** 12, "po " + what


@pytest.mark.parametrize("form,shape,p,knobs,inst", _fwd_cases())
def test_wide_and_streamed_forward_against_float64(form, shape, p, knobs, inst):
    H = G._abi()
    O, lse, am, run2 = _forward(H, shape, p, knobs, inst)
    _check_forward("fwd " + form, shape, p, inst, O, lse, am, run2, form == "stream")


# ------------------------------------------------------------------ backward
BWD_FORMS = {          # name -> (phases, knobs)
    "phase0": ((0,), {}),
    "phases123": ((1, 2, 3), {}),
    "fused": ((4,), {}),
    "phases56": ((5, 6), {}),
    "launch1": ((4,), {"ATT_FUSED_LAUNCH": 1}),
    "merge0": ((4,), {"ATT_MERGE": 0}),
}
_BASE = {"launch1": "fused", "merge0": "fused"}


def _bwd_insts(shape, form, extra):
    phases, knobs = BWD_FORMS[form]
    return tuple(R.bwd_launch(*shape[1:], ph, knobs=dict(knobs, **extra)) for ph in phases)


def _bwd_cases():
    out = []
    for shape in R.WIDE_SHAPES:
        for form in BWD_FORMS:
            insts = _bwd_insts(shape, form, {})
            if form in _BASE and insts == _bwd_insts(shape, _BASE[form], {}):
                continue          # the knob changes nothing at this shape: the base form's case is this one
            assert not any(n.startswith("!") for ph in insts for n in ph), (form, shape, insts)
            out += [pytest.param(form, shape, p, {}, insts, id=_id(form, shape, p)) for p in R.drop_ps_x(shape)]
    for shape, extra in STREAMED:
        for form in ("phase0", "phases123") + (("fused",) if shape in R.STREAM_FUSED_RUN else ()):
            insts = _bwd_insts(shape, form, extra)
            assert not any(n.startswith("!") for ph in insts for n in ph), (form, shape, insts)
            if form != "fused":
                assert any(n.startswith("dq_stream<") for ph in insts for n in ph), insts
            tag = "stream_" + form
            out += [pytest.param(tag, shape, p, extra, insts, id=_id(tag, shape, p)) for p in R.drop_ps_x(shape)]
    return out


def _backward(H, shape, p, O, lse, phases, insts, knobs, tag=None, bb=None, what=""):
    """Run the phases under ``knobs`` into guarded buffers; with ``bb`` D is held to its bound where a phase stores it alone.
    Returns the outputs as numpy arrays (D None when no phase stores it) after the untouched-words checks."""
    B0, H_, dh, Lq, La, Lb = shape
    dv = G._dev(shape)
    B, d = R.batch_rows(shape), H_ * dh
    st = G._ref(shape, p)
    own_q = dv["Qs"] is not dv["Yv"]
    gYv = G._Guarded(dv["Yv"].shape[0] + 2, 4 * d, 3)
    gYu = G._Guarded(dv["Yu"].shape[0] + 2, 2 * d, 4)
    gQ = G._Guarded(B * Lq + 2, 4 * d, 5) if own_q else gYv
    Dv = G._Guarded(1, B * H_ * Lq + 5, 6)
    if La:
        gQ.region(B * Lq, 0, d)
        gYv.region(B * La, 2 * d, 4 * d)
    if Lb:
        gQ.region(B * Lq, d, 2 * d)
        gYu.region(B * Lb, 0, 2 * d)
    grads = ((gQ.t, 0) if La else None, (gQ.t, d) if Lb else None, 4 * d, (gYv.t, 2 * d) if La else None, (gYv.t, 3 * d) if La else None, 4 * d,
             (gYu.t, 0) if Lb else None, (gYu.t, d) if Lb else None, 2 * d)
    Dn = lambda: Dv.t[0, :B * H_ * Lq].cpu().numpy().reshape(B, H_, Lq)
    with _Knobs(H, knobs) as kn:
        live, live_mode = kn.live()
        for ph, want in zip(phases, insts):
            assert R.bwd_launch(H_, dh, Lq, La, Lb, ph, mode=live_mode, knobs=live) == want
            H.attn_bwd(B, H_, dh, Lq, La, Lb, *G._views(dv, shape), *G._masks(dv, shape), lse.t, O.t, d + 8, dv["dO"], d, Dv.t, *grads,
                       drop_p=p, seed=G.SEED, site=G.SITE, phase=ph)
            torch.cuda.synchronize()
            if ph == 1:          # D alone, before the kernels that consume it
                Dv.region(1, 0, B * H_ * Lq)
                if bb is not None:
                    _check(tag, "D", Dn(), st["D"], bb["D"], what)
    if phases == (0,):          # the whole backward stores D from its dQ kernel
        Dv.region(1, 0, B * H_ * Lq)
    Dv.assert_outside_untouched("Dvec " + what)          # (the fused backward forms D in LDS: it leaves Dvec alone altogether)
    for g_, nm in ((gQ, "dQ buffer"), (gYv, "dYv"), (gYu, "dYu")):
        g_.assert_outside_untouched(nm + " " + what)
    out = dict(D=Dn() if bool(Dv.written.any()) else None)
    dq = gQ.t[:B * Lq].cpu().numpy().reshape(B, Lq, 4 * d)
    if La:
        yv = gYv.t[:B * La].cpu().numpy().reshape(B, La, 4 * d)
        out.update(dQa=dq[..., :d], dKa=yv[..., 2 * d:3 * d], dVa=yv[..., 3 * d:])
    if Lb:
        yu = gYu.t[:B * Lb].cpu().numpy().reshape(B, Lb, 2 * d)
        out.update(dQb=dq[..., d:2 * d], dKb=yu[..., :d], dVb=yu[..., d:])
    return out


def _check_backward(tag, out, st, bb, what):
    for k in R.OUTPUTS_BWD:
        if out.get(k) is not None:
            _check(tag, k, out[k], st[k], bb[k], what)


@pytest.mark.parametrize("form,shape,p,knobs,insts", _bwd_cases())
def test_wide_and_streamed_backward_against_float64(form, shape, p, knobs, insts):
    H = G._abi()
    phases, fk = BWD_FORMS[form.replace("stream_", "")]
    knobs = dict(fk, **knobs)
    # the forward that precedes this backward in the engine: the same stream knob, otherwise default knobs
    fwd_knobs = {k: v for k, v in knobs.items() if k == "ATT_STREAM"}
    stream_fwd = _streamed(shape, fwd_knobs)
    fwd_inst = R.fwd_launch(*shape[1:], knobs=fwd_knobs)
    assert fwd_inst.startswith("fwd_stream<") == stream_fwd
    O, lse, _, _ = _forward(H, shape, p, fwd_knobs, fwd_inst, po=False)
    rep = R.rep_of([n for ph in insts for n in ph])
    st, (_, bb) = G._ref(shape, p), _bounds(shape, p, stream_fwd, rep)
    what = "%s p=%g %s" % (shape, p, insts)
    tag = "bwd " + form
    out = _backward(H, shape, p, O, lse, phases, insts, knobs, tag, bb, what)
    assert (out["D"] is not None) == (phases in ((0,), (1, 2, 3)))
    if phases == (1, 2, 3):
        out["D"] = None          # held to its bound above, alone
    _check_backward(tag, out, st, bb, what)


@pytest.mark.parametrize("shape,knobs", STREAMED, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "stream%d" % len(v))
def test_streamed_split_backward_gives_the_bits_of_the_whole_one(shape, knobs):
    """attention_stream.h: phases 1 + 2 + 3 (attn_D_stream_kernel, then dQ and dK/dV) give the D, dQ, dK and dV bits of phase 0"""
    H = G._abi()
    p = 0.1
    O, lse, _, _ = _forward(H, shape, p, knobs, R.fwd_launch(*shape[1:], knobs=knobs), po=False)
    whole = _backward(H, shape, p, O, lse, (0,), _bwd_insts(shape, "phase0", knobs), knobs)
    split = _backward(H, shape, p, O, lse, (1, 2, 3), _bwd_insts(shape, "phases123", knobs), knobs)
    assert "D_stream<%d>" % shape[2] in _bwd_insts(shape, "phases123", knobs)[0]
    for k, v in whole.items():
        assert v is not None and np.array_equal(v.view(np.int32), split[k].view(np.int32)), (k, shape)


# ------------------------------------------------------------------ the workgroup-shape knobs
def _hpb_cases():
    out = []
    for shape in R.HPB_SHAPES:
        for kernel in ("FWD", "DQ", "DKV"):
            values = [R.hpb_value(kernel, shape)]
            if shape == (2, 4, 4, 33, 5, 3):          # a heads,tiles value that changes wq as well: two tiles (dK/dV: one) per head
                values.append(2 | (1 if kernel == "DKV" else 2) << 8)
            for v in dict.fromkeys(values):
                out += [pytest.param(kernel, shape, p, v, id="%s=%d,%d-%s-p%g" % (kernel, v & 0xff, v >> 8, "x".join(map(str, shape)), p))
                        for p in (0.0, 0.1)]
    return out


@pytest.mark.parametrize("kernel,shape,p,value", _hpb_cases())
def test_two_heads_per_workgroup_against_float64_and_the_default_launch(kernel, shape, p, value):
    """ATT_HPB_FWD / _DQ / _DKV with two heads per workgroup (``wave / wq`` selects the head): the same bounds, and the bits of the
    default launch -- the arithmetic of a (head, tile) does not depend on the workgroup shape in any of the five kernels (module
    docstring)."""
    H = G._abi()
    B0, H_, dh, Lq, La, Lb = shape
    knobs = {"ATT_HPB_" + kernel: value}
    stream = _streamed(shape, {})
    fwd0 = R.fwd_launch(*shape[1:])
    O0, lse0, am0, _ = _forward(H, shape, p, {}, fwd0, po=False)
    st = G._ref(shape, p)
    what = "%s p=%g %s" % (shape, p, knobs)
    if kernel == "FWD":
        inst = R.fwd_launch(*shape[1:], knobs=knobs)
        assert R.launch_field(inst, "hpb") == 2 and R.launch_field(fwd0, "hpb") == 1, (inst, fwd0)
        if value >> 8:
            assert R.launch_field(inst, "wq") == value >> 8 != R.launch_field(fwd0, "wq"), (inst, fwd0)
        O, lse, am, run2 = _forward(H, shape, p, knobs, inst)
        _check_forward("hpb fwd" + ("_stream" if stream else ""), shape, p, inst, O, lse, am, run2, stream)
        assert torch.equal(O.t, O0.t) and torch.equal(lse.t, lse0.t) and float(am.max()) == float(am0.max()), "bits of the default launch " + what
        return
    phases = (1, 2, 3)
    insts0 = tuple(R.bwd_launch(*shape[1:], ph) for ph in phases)
    insts = tuple(R.bwd_launch(*shape[1:], ph, knobs=knobs) for ph in phases)
    mine, theirs = insts[1 if kernel == "DQ" else 2][0], insts0[1 if kernel == "DQ" else 2][0]
    assert R.launch_field(mine, "hpb") == 2 and R.launch_field(theirs, "hpb") == 1, (mine, theirs)
    assert mine.startswith(("dq_stream<" if stream else "dq<") if kernel == "DQ" else "dkv<")
    _, bb = _bounds(shape, p, stream)
    tag = "hpb " + mine.split("<")[0]
    out = _backward(H, shape, p, O0, lse0, phases, insts, knobs, tag, bb, what)
    ref = _backward(H, shape, p, O0, lse0, phases, insts0, {})
    _check_backward(tag, dict(out, D=None), st, bb, what)
    for k, v in ref.items():
        assert np.array_equal(v.view(np.int32), out[k].view(np.int32)), "bits of the default launch: %s %s" % (k, what)


@pytest.mark.parametrize("shape", R.STREAM_FUSED, ids=lambda s: "x".join(map(str, s)))
def test_the_fused_backward_refuses_more_than_192_padded_keys(shape):
    """11 + 2 key tiles: each block is within the fused kernels' 12 tiles, the call is refused all the same (segmm_attn_bwd), as the
    restated rule says; nothing is launched and no output word is written.  The streamed forward in front of the fused backward is
    the ``stream_fused`` form at 11 + 1 tiles under ATT_STREAM = 1."""
    H = G._abi()
    assert R.bwd_launch(*shape[1:], 4) == ("!more than 192 padded keys in the fused backward",)
    O, lse, _, _ = _forward(H, shape, 0.0, {}, R.fwd_launch(*shape[1:]), po=False)
    with pytest.raises(RuntimeError, match="at most 12 key tiles"):
        _backward(H, shape, 0.0, O, lse, (4,), (R.bwd_launch(*shape[1:], 4),), {})


# ------------------------------------------------------------------ the stream, the list, the knobs
def test_the_exported_dropout_stream_is_the_host_restatement():
    H = G._abi()
    for shape, p in (((1, 2, 16, 17, 200, 9), 0.1), ((1, 2, 128, 40, 40, 100), 0.5), ((2, 2, 96, 1, 1, 20), 0.1)):
        want = R.host_mult(shape, p)
        got = torch.ones(want.size, device=DEV)
        H.dropout_mult(got, want.size, p, R.DROP_SEED, R.DROP_SITE)
        assert np.array_equal(got.cpu().numpy(), want.reshape(-1)), (shape, p)


def test_every_instance_of_the_list_is_present():
    """The generated cases reach every kernel the module is about, no case is generated twice, and the knobs and the attention mode
    are back at their defaults."""
    H = G._abi()
    fw = {c.values[4].split("/")[0] for c in _fwd_cases()}
    assert {"fwd_stream<%d>" % dh for dh in R.STREAM_DIMS} <= fw
    assert any(n.startswith("fwd<96,") for n in fw) and any(n.startswith("fwd<128,") for n in fw)
    names = {n for c in _bwd_cases() for ph in c.values[4] for n in ph}
    for dh in R.STREAM_DIMS:
        assert "D_stream<%d>" % dh in names and any(n.startswith("dq_stream<%d>" % dh) for n in names), dh
    for dh in R.WIDE_DIMS:
        for piece in ("D<%d>", "dq<%d,", "dkv<%d,", "wide<%d,4,", "wide<%d,8,", "wide<%d,4,merged,16>", "wide<%d,4,merged,32>", "wide<%d,4,16>",
                      "wide<%d,4,32>", "wide<%d,8,one>", "wide<%d,8,chunks>", "wide<%d,8,one>a/w8/p2", "wide<%d,8,chunks>a/w8/p2", "wide<%d,8,one>ab/",
                      "wide<%d,8,one>b/w7/p1", "wide<%d,4,one>a/w3/p1"):
            assert any(n.startswith(piece % dh) for n in names), piece % dh
        # the streamed forward in front of the fused backward, two passes
        assert any(c.values[0] == "stream_fused" and c.values[4] == (("wide<%d,8,one>a/w8/p2" % dh, "wide<%d,4,one>b/w1/p1" % dh),) for c in _bwd_cases())
    assert any(c.values[0] == "stream_fused" and c.values[1][2] == 48 for c in _bwd_cases())
    assert any(R.launch_field(n, "wq") == 4 and n.startswith("dq<128,") for n in names)          # seven query tiles: a surplus wave
    assert max(R.n_tiles(c.values[1]) for c in _fwd_cases()) == 32
    assert {R.n_tiles(s) for s in R.STREAM_LONG} >= {13, 14, 32}
    hp = {(c.values[0], c.values[1]) for c in _hpb_cases()}
    assert hp == {(k, s) for k in ("FWD", "DQ", "DKV") for s in R.HPB_SHAPES}
    ids = [c.id for f in (_fwd_cases, _bwd_cases, _hpb_cases) for c in f()]
    assert len(ids) == len(set(ids))
    want = dict(R.KNOBS, **R.SHAPE_KNOBS)
    assert {k: H.knob(k) for k in ALL_KNOBS} == want and H.attn_mode(-1) == 1
