"""Segment counts above 64 without a GPU: the argument checks of segmm_loss_fwd_bwd / segmm_rand_perm_rows name the limit of 256
(every call below fails its check before anything is launched; neither entry point is called here with an accepted S), the ABI
version and the dispatch table are what they were, and the engine refuses more than 192 padded attention keys by itself."""
import ctypes
import os
import subprocess
import sys

import pytest

from helpers import ROOT


def _lib():
    from segmminterest_amd import hipabi
    return hipabi, hipabi.lib()


def _err(L, rc):
    assert rc != 0
    return L.segmm_last_error().decode()


@pytest.mark.parametrize("S", [257, 0, -1, 1 << 20])
def test_loss_refuses_s_outside_1_256(S):
    H, L = _lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)          # never dereferenced: the S check fails first
    coef, en = (ctypes.c_float * 9)(), (ctypes.c_int * 9)()
    msg = _err(L, L.segmm_loss_fwd_bwd(4, S, p, p, None, None, p, ctypes.cast(coef, ctypes.c_void_p), ctypes.cast(en, ctypes.c_void_p),
                                       0, 0, 0, p, p, p, 4, p, p, p, None))
    assert "256" in msg and "S=%d" % S in msg and "loss" in msg


@pytest.mark.parametrize("S", [257, 0, -3])
def test_rand_perm_rows_refuses_s_outside_1_256(S):
    H, L = _lib()
    buf = (ctypes.c_double * 64)()
    msg = _err(L, L.segmm_rand_perm_rows(ctypes.addressof(buf), 4, S, 1, 1, None))
    assert "256" in msg and "rand_perm_rows" in msg
    assert "rand_perm_rows" in _err(L, L.segmm_rand_perm_rows(None, 4, 40, 1, 1, None))


def test_abi_and_dispatch_table_unchanged():
    H, L = _lib()
    assert L.segmm_abi_version() == H.ABI_VERSION == 30
    assert len(H.SIGNATURES["segmm_loss_fwd_bwd"]) == 20 and len(H.SIGNATURES["segmm_rand_perm_rows"]) == 6
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_cmd_dispatch.py"), "--check"])


@pytest.mark.parametrize("S,Lt,N,abl,ok", [(80, 100, 3, "ours", True), (176, 16, 2, "ours", True), (160, 1, 2, "ours", True),
                                          (177, 16, 2, "ours", False), (200, 1, 2, "ours", False), (100, 100, 2, "ours", False),
                                          (97, 90, 2, "ours", False), (256, 100, 1, "ours", True), (256, 100, 3, "SelfMLP", True)])
def test_engine_refuses_more_than_192_padded_keys(S, Lt, N, abl, ok):
    """BackboneRun._require_attn_keys: pad16(S) + pad16(Lt) <= 192 wherever the pass runs an attention (no encoder layer with
    N = 1, none in the MLP ablations); (97, 90): 187 tokens, but 112 + 96 padded keys."""
    from segmminterest_amd import engine as E
    run = E.BackboneRun.__new__(E.BackboneRun)
    run.abl, run.N, run.mode = abl, N, "both"
    if ok:
        run._require_attn_keys(S, Lt)
    else:
        with pytest.raises(RuntimeError, match=r"> 192 not built .*pad16\(S\) \+ pad16\(Lt\) <= 192"):
            run._require_attn_keys(S, Lt)
