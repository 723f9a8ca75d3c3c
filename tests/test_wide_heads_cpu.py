"""Wide attention heads (dh = 96, 128) without a GPU: what the C entry points accept and refuse before any launch.  The argument
checks of ``attn_fill`` run in a fixed order -- head dim, input planes, leading dims, alignment, then the 256-token limit -- so a
call that reaches the "at most 256" message has passed the width check."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _lib():
    from segmminterest_amd import hipabi as H
    return H, H.lib()


def _ptr():
    buf = (ctypes.c_double * 64)()
    return buf, (ctypes.addressof(buf) + 15) & ~15          # 16-byte aligned, never dereferenced: a check fails first


def _fwd(L, dh, Lq, p, pl=None):
    ld = 2 * dh
    return L.segmm_attn_fwd(2, 2, dh, Lq, 40, 10, p, p, ld, p, p, ld, p, p, ld, p, p, p, p, ld, p, 0.0, 0, 0, None, pl, None)


def _bwd(L, dh, Lq, p, phase, pl=None):
    ld = 2 * dh
    return L.segmm_attn_bwd(2, 2, dh, Lq, 40, 10, p, p, ld, p, p, ld, p, p, ld, p, p, p, p, p, ld, p, ld, p, p, p, ld, p, p, ld, p, p, ld,
                            0.0, 0, 0, None, None, None, phase, pl, None)


@pytest.mark.parametrize("dh", [96, 128])
def test_wide_head_dims_pass_the_width_check(dh):
    H, L = _lib()
    keep, p = _ptr()
    assert _fwd(L, dh, 257, p) != 0
    msg = L.segmm_last_error().decode()
    assert "at most 256" in msg and "Lq=257" in msg and "head dim" not in msg, msg
    for phase in (0, 2, 4):
        assert _bwd(L, dh, 257, p, phase) != 0
        msg = L.segmm_last_error().decode()
        assert "at most 256" in msg and "head dim" not in msg, msg


@pytest.mark.parametrize("dh", [80, 24])
def test_unbuilt_head_dims_are_refused_with_the_built_list(dh):
    H, L = _lib()
    keep, p = _ptr()
    assert _fwd(L, dh, 40, p) != 0
    msg = L.segmm_last_error().decode()
    assert "head dim %d not built" % dh in msg and "96" in msg and "128" in msg and "4,8,16,32,48,64,96,128" in msg, msg
    assert _bwd(L, dh, 40, p, 4) != 0
    assert "4,8,16,32,48,64,96,128" in L.segmm_last_error().decode()


def test_input_planes_are_refused_at_a_wide_head():
    H, L = _lib()
    keep, p = _ptr()
    pl = H.AttnPlanes()
    pl.qa_in = p
    assert _fwd(L, 96, 40, p, ctypes.byref(pl)) != 0
    msg = L.segmm_last_error().decode()
    assert "input planes are not built for wide heads" in msg and "96" in msg, msg
    assert _bwd(L, 96, 40, p, 4, ctypes.byref(pl)) != 0
    assert "input planes are not built for wide heads" in L.segmm_last_error().decode()
    assert _fwd(L, 48, 257, p, ctypes.byref(pl)) != 0          # (a built planes-in width still gets as far as the size check)
    assert "at most 256" in L.segmm_last_error().decode()


def test_abi_version_is_unchanged():
    H, L = _lib()
    assert L.segmm_abi_version() == H.ABI_VERSION == 30


def test_committed_resource_table_meets_the_scratch_condition():
    """profiles/attn_wide_heads_resources.txt (tools/attn_resource_table.py; ``--check`` recompiles and compares): every dh = 96 and
    dh = 128 instantiation on the default model path uses no more scratch per lane than the same kernel's dh = 64 instantiation,
    and the kernels taken only above 192 keys or under a knob use none."""
    import re
    rows = {}
    with open(os.path.join(ROOT, "profiles", "attn_wide_heads_resources.txt")) as f:
        for line in f:
            m = re.match(r"(\w+)<(\d+)((?:, \w+)*)>\s+(default|opt)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", line)
            if m:
                name = m.group(1).replace("_wide", "")
                rows[(name, int(m.group(2)), m.group(3))] = (m.group(4), int(m.group(7)))
    wide = [k for k in rows if k[1] in (96, 128)]
    assert len(wide) == 2 * 21 and sum(1 for k in rows if k[1] == 64) == 28
    for name, dh, rest in wide:
        path, scratch = rows[(name, dh, rest)]
        base = rows[(name, 64, rest)][1]
        assert scratch <= base, (name, dh, rest, scratch, base)
        if path == "opt":
            assert scratch == 0, (name, dh, rest, scratch)
