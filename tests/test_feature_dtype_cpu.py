"""The C ABI of the 16-bit input features (segmm_gather_l1_h, segmm_l1norm_h; SEGMM_ELEM_F16 / SEGMM_ELEM_BF16) as the binding sees
it: the two additive entry points are bound with the header's types, the ABI version did not move, both generated mirrors are
current, a recorded command round-trips with ``elem`` and ``D`` readable by name, and the dtype rules of the binding and of
ResidentFeatureTable refuse before anything touches a device.  No GPU."""
import ctypes
import importlib.util
import os

import pytest
import torch

from helpers import ROOT

_spec = importlib.util.spec_from_file_location("gen_cmd_dispatch", os.path.join(ROOT, "tools", "gen_cmd_dispatch.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

NEW = ("segmm_gather_l1_h", "segmm_l1norm_h")
TWIN = {"segmm_gather_l1_h": "segmm_gather_l1", "segmm_l1norm_h": "segmm_l1norm"}


def _header():
    return open(gen.HDR).read()


def test_the_two_entry_points_are_bound_with_the_headers_types():
    from segmminterest_amd import hipabi as H
    ct = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}
    protos = dict(gen.prototypes(_header()))
    L = H.lib()
    for name in NEW:
        assert name in H.SIGNATURES and name in H.PARAMS and name in protos
        ps = protos[name]
        want = [ctypes.c_void_p if (ty.endswith("*") or ty == "segmm_stream_t") else ct[ty] for ty, _ in ps]
        assert list(getattr(L, name).argtypes) == want == H.SIGNATURES[name]
        assert H.PARAMS[name] == tuple(p for _, p in ps)
        # (const uint16_t* input, int elem, ...) followed by the remaining arguments of the fp32 twin, types and names
        twin = protos[TWIN[name]]
        assert ps[0][0] == "const uint16_t*" and ps[1] == ("int", "elem") and ps[0][1] == twin[0][1]
        assert ps[2:] == twin[1:]
        assert name in H.op_ids() and TWIN[name] in H.op_ids()          # dispatchable: a recorded step can carry it


def test_abi_version_constants_and_mirrors():
    from segmminterest_amd import _abi, hipabi as H
    k = gen.constants(_header())
    assert H.ABI_VERSION == _abi.ABI_VERSION == k["SEGMM_ABI_VERSION"] == 30 == H.lib().segmm_abi_version()
    assert (k["SEGMM_ELEM_F16"], k["SEGMM_ELEM_BF16"]) == (1, 2)
    assert (_abi.CONSTANTS["SEGMM_ELEM_F16"], _abi.CONSTANTS["SEGMM_ELEM_BF16"]) == (H.ELEM_F16, H.ELEM_BF16) == (1, 2)
    assert H._ELEM == {torch.float16: 1, torch.bfloat16: 2}
    gen.check(_header(), {p: open(p).read() for p in (gen.OUT, gen.OUT_ABI)})          # both generated files are current
    inc = open(gen.OUT).read()
    for name in NEW:
        assert '"%s",' % name in inc and "return %s((const uint16_t*)a[0].p, (int)a[1].i," % name in inc


def test_a_recorded_gather_command_round_trips():
    from segmminterest_amd import hipabi as H

    def args(name, **kw):
        assert set(kw) <= set(H.PARAMS[name])
        return tuple(kw.get(p, None if ct is H._p else 0) for p, ct in zip(H.PARAMS[name], H.SIGNATURES[name]))

    rec = H.Recorder(111, 222)
    rec.mark(H.PHASE_STEP_BEGIN)
    rec.call("segmm_gather_l1_h", args("segmm_gather_l1_h", table=4096, elem=H.ELEM_BF16, n_lines=200000, D=768, idx=8192, rows=51200,
                                       normalize=1, out=12288, stream=111))
    rec.call("segmm_l1norm_h", args("segmm_l1norm_h", x=16384, elem=H.ELEM_F16, rows=20480, D=1024, stream=222))
    (ph, a), = rec.finish()
    assert ph.n_cmds == 2 and a[0].op == H.op_ids()["segmm_gather_l1_h"] and a[1].op == H.op_ids()["segmm_l1norm_h"]
    g = lambda p: H.cmd_arg(a[0], "segmm_gather_l1_h", p)
    assert (g("table"), g("elem"), g("n_lines"), g("D"), g("idx"), g("rows"), g("normalize"), g("out"), g("mask")) == (
        4096, 2, 200000, 768, 8192, 51200, 1, 12288, None) and a[0].stream == 0
    n = lambda p: H.cmd_arg(a[1], "segmm_l1norm_h", p)
    assert (n("x"), n("elem"), n("rows"), n("D"), n("y")) == (16384, 1, 20480, 1024, None) and a[1].stream == 1
    # the pointer slots a replay may re-base: table / idx / out of the gather, x of the normalisation -- never elem or D
    names = [[H.PARAMS[nm][k] for ci, k in rec.pslots[0] if ci == c] for c, nm in enumerate(("segmm_gather_l1_h", "segmm_l1norm_h"))]
    assert names == [["table", "idx", "out"], ["x"]]


def test_dtype_rules_refuse_on_the_host():
    """Checked before a device is touched: CPU tensors of a wrong dtype name the dtype and the accepted ones."""
    from segmminterest_amd import hipabi as H
    from segmminterest_amd.feature_store import ResidentFeatureTable
    for bad in (torch.zeros(4, 8, dtype=torch.float64), torch.zeros(4, 8, dtype=torch.int16)):
        with pytest.raises(RuntimeError, match=str(bad.dtype).replace(".", r"\.") + ".*float32.*float16.*bfloat16"):
            H._feat(bad, "x")
        with pytest.raises(RuntimeError, match="float32.*float16.*bfloat16"):
            ResidentFeatureTable(bad)
    with pytest.raises(RuntimeError, match="contiguous"):
        H._feat(torch.zeros(4, 16, dtype=torch.float16)[:, ::2], "x")
    assert [H._feat(torch.zeros(2, 4, dtype=d), "x") for d in (torch.float32, torch.float16, torch.bfloat16)] == [None, 1, 2]
    with pytest.raises(RuntimeError, match="HIP tensor"):
        ResidentFeatureTable(torch.zeros(4, 8, dtype=torch.float16))          # a host tensor is no resident table
