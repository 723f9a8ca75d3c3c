"""The ctypes binding's tables are generated from include/segmm_hip.h (tools/gen_cmd_dispatch.py -> segmminterest_amd/_abi.py):
the parser on synthetic header text, the bound argument TYPES against the real header, recorded arguments read back by
parameter name, and the staleness check of both generated files.  No GPU."""
import ctypes
import importlib.util
import os

import pytest

from helpers import ROOT

_spec = importlib.util.spec_from_file_location("gen_cmd_dispatch", os.path.join(ROOT, "tools", "gen_cmd_dispatch.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

SYNTH = """
/* int segmm_in_a_comment(int x); */
#define SEGMM_X (-2)
#define SEGMM_Y 7 /* trailing comment */
#define SEGMM_GUARD_H
enum { SEGMM_PHASE_A = 0, SEGMM_PHASE_B = 3 };
typedef struct {
    uint16_t *a, *b; int n; const float *p, *q;
    const float* r;      /* one declarator, star on the type */
} segmm_s_t;
int segmm_f(const float* x, int64_t n,
            float eps, uint64_t seed, uint32_t site, segmm_stream_t stream);
int segmm_g(void);
const char* segmm_not_an_int(void);
"""


def test_parser_on_synthetic_text():
    assert gen.prototypes(SYNTH) == [("segmm_f", [("const float*", "x"), ("int64_t", "n"), ("float", "eps"), ("uint64_t", "seed"),
                                                  ("uint32_t", "site"), ("segmm_stream_t", "stream")]),
                                     ("segmm_g", [])]
    assert [gen.type_code(ty) for ty, _ in gen.prototypes(SYNTH)[0][1]] == ["p", "i64", "f", "u64", "u32", "p"]
    assert gen.struct_fields(SYNTH, "segmm_s_t") == [("a", "p"), ("b", "p"), ("n", "i"), ("p", "p"), ("q", "p"), ("r", "p")]
    assert gen.constants(SYNTH) == {"SEGMM_X": -2, "SEGMM_Y": 7, "SEGMM_PHASE_A": 0, "SEGMM_PHASE_B": 3}


@pytest.mark.parametrize("text,call", [
    ("int segmm_f(double x, segmm_stream_t stream);", lambda t: gen.abi_py(t)),                      # a parameter type
    ("typedef struct { uint16_t v; } segmm_s_t;", lambda t: gen.struct_fields(t, "segmm_s_t")),      # a by-value field type
    ("typedef struct { int a[4]; } segmm_s_t;", lambda t: gen.struct_fields(t, "segmm_s_t")),        # a declarator form
    ("enum { SEGMM_PHASE_A };", lambda t: gen.constants(t)),                                         # an implicit enum value
])
def test_parser_refuses_what_it_does_not_handle(text, call):
    with pytest.raises(SystemExit, match="unhandled"):
        call("#define SEGMM_ABI_VERSION 1\ntypedef struct { int n; } segmm_attn_planes_t;\n" + text)


def _header():
    return open(gen.HDR).read()


def test_bound_argument_types_equal_the_header():
    """Types, not only names: what ctypes was told about every entry point equals what the header declares."""
    from segmminterest_amd import hipabi as H
    ct = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}
    protos = {n: ps for n, ps in gen.prototypes(_header()) if n != "segmm_abi_version"}          # (bound by hand, no arguments)
    assert set(protos) == set(H.SIGNATURES) == set(H.PARAMS)
    L = H.lib()
    for name, ps in protos.items():
        want = [ctypes.c_void_p if (ty.endswith("*") or ty == "segmm_stream_t") else ct[ty] for ty, _ in ps]
        assert list(getattr(L, name).argtypes) == want == H.SIGNATURES[name], name
        assert H.PARAMS[name] == tuple(p for _, p in ps) and len(H.PARAMS[name]) == len(H.SIGNATURES[name]), name
    assert L.segmm_abi_version() == H.ABI_VERSION == gen.constants(_header())["SEGMM_ABI_VERSION"]
    want = [(n, H._CTYPE[c]) for n, c in gen.struct_fields(_header(), "segmm_attn_planes_t")]
    assert H.AttnPlanes._fields_ == want and len(want) == 32
    k = gen.constants(_header())
    assert (H.CMD_MAX_ARGS, H.OP_FORK, H.OP_JOIN, H.SITE_HDR, H.AMAX_SLOTS, H.ATTN_PLANES_ONLY, H.ATTN_REPAIR) == tuple(
        k["SEGMM_" + n] for n in ("CMD_MAX_ARGS", "OP_FORK", "OP_JOIN", "SITE_HDR", "AMAX_SLOTS", "ATTN_PLANES_ONLY", "ATTN_REPAIR"))
    assert [getattr(H, "PHASE_" + e[len("segmm_"):].upper()) for e in H.PHASE_ENTRY] == list(range(k["SEGMM_PHASE_KINDS"]))


def test_recorded_arguments_read_back_by_name():
    """hipabi.cmd_arg reads the slot Recorder.call wrote, found by the header's parameter name."""
    from segmminterest_amd import hipabi as H
    protos = dict(gen.prototypes(_header()))

    def args(name, **kw):          # every argument 0 / null except the named ones; integer stand-ins for pointers, main stream 111
        assert set(kw) <= set(H.PARAMS[name])
        return tuple(kw.get(p, None if ct is H._p else 0) for p, ct in zip(H.PARAMS[name], H.SIGNATURES[name]))

    rec = H.Recorder(111, 222)
    rec.mark(H.PHASE_LAYER_BWD)
    rec.call("segmm_gemm_p", args("segmm_gemm_p", layout=2, M=77, N=5, K=9, write_c=3, drop_p=0.25, c_hdr=4096, stream=111))
    rec.call("segmm_attn_bwd", args("segmm_attn_bwd", B=16, H=4, dh=16, Lq=40, La=12, Lb=8, phase=5, planes=8192, seed=(1 << 63) | 9, stream=222))
    (ph, a), = rec.finish()
    g = lambda p: H.cmd_arg(a[0], "segmm_gemm_p", p)
    assert (g("layout"), g("M"), g("N"), g("K"), g("write_c"), g("drop_p"), g("c_hdr"), g("bias")) == (2, 77, 5, 9, 3, 0.25, 4096, None)
    slot = [p for _, p in protos["segmm_gemm_p"]].index("write_c")
    assert a[0].a[slot].i == 3 and [k for k in range(H.CMD_MAX_ARGS) if a[0].a[k].i == 3] == [slot]
    b = lambda p: H.cmd_arg(a[1], "segmm_attn_bwd", p)
    assert [b(p) for p in ("B", "H", "dh", "Lq", "La", "Lb", "phase", "planes")] == [16, 4, 16, 40, 12, 8, 5, 8192] and a[1].stream == 1
    assert b("seed") & ((1 << 64) - 1) == (1 << 63) | 9
    with pytest.raises(ValueError):
        H.cmd_arg(a[0], "segmm_gemm_p", "no_such_parameter")
    # the record-naming rules both the eager wrappers and the timed replay use
    assert H.gemm_record(g("layout"), g("M"), g("N"), g("K"), g("write_c")) is None          # bit 1: a repair launch
    assert H.gemm_record(2, 77, 5, 9, 1) == (12, 77, 5, 9) and H.gemm_record(2, 77, 5, 9) == (2, 77, 5, 9)
    assert H.attn_record(16, 4, 16, 40, 12, 8) == ("fwd", 16, 4, 16, 40, 12, 8)
    assert H.attn_record(16, 4, 16, 40, 12, 8, 0) == ("bwd", 16, 4, 16, 40, 12, 8) and H.attn_record(16, 4, 16, 40, 12, 8, 2)[0] == "bwd2"
    assert H.attn_record(16, 4, 16, 40, 12, 8, 5, H.AttnPlanes()) == ("bwd4", 16, 4, 16, 40, 12, 0)
    assert H.attn_record(16, 4, 16, 40, 12, 8, 6, H.AttnPlanes(flags=H.ATTN_REPAIR)) == ("bwd4r", 16, 4, 16, 40, 0, 8)


def test_check_reports_either_generated_file_as_stale():
    hdr = _header()
    current = {p: open(p).read() for p in (gen.OUT, gen.OUT_ABI)}
    assert "do not edit" in current[gen.OUT_ABI].splitlines()[0]
    gen.check(hdr, current)

    def stale(text, cur=current):
        assert text != hdr or cur is not current
        with pytest.raises(SystemExit) as e:
            gen.check(text, cur)
        assert e.value.code not in (None, 0)
        return str(e.value.code)

    # one argument more on a dispatchable entry point: both mirrors move; on another one: only the binding's data
    assert stale(hdr.replace("int segmm_fill_zero(", "int segmm_fill_zero(int extra, ")).startswith("cmd_dispatch.inc and _abi.py stale")
    assert stale(hdr.replace("int segmm_step_bind(", "int segmm_step_bind(int extra, ")).startswith("_abi.py stale")
    assert stale(hdr.replace("#define SEGMM_ABI_VERSION 30", "#define SEGMM_ABI_VERSION 31")).startswith("_abi.py stale")
    assert stale(hdr, {gen.OUT: current[gen.OUT]}).startswith("_abi.py stale")          # a missing file is stale
