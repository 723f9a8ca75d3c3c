"""Streamed attention without a GPU: the engine's opt-in (``model_cfg.attn_stream``) widens ``_require_attn_keys`` to 256 per axis
and leaves the default refusal alone; the argument checks of segmm_attn_fwd / segmm_attn_bwd name the limit of 256 (every call
below fails its check before anything is launched); the ABI version and the dispatch table are what they were; the knob table
lists ATT_STREAM = 0."""
import argparse
import ctypes
import os
import subprocess
import sys

import pytest

from helpers import ROOT


def _lib():
    from segmminterest_amd import hipabi
    return hipabi, hipabi.lib()


def _bare_run(**attrs):
    from segmminterest_amd import engine as E
    run = E.BackboneRun.__new__(E.BackboneRun)
    run.abl, run.N, run.mode = "ours", 3, "both"
    for k, v in attrs.items():
        setattr(run, k, v)
    return run


@pytest.mark.parametrize("S,Lt", [(200, 1), (100, 100), (256, 100), (256, 256), (80, 100)])
def test_opt_in_accepts_up_to_256_per_axis(S, Lt):
    _bare_run(attn_stream=1)._require_attn_keys(S, Lt)


@pytest.mark.parametrize("S,Lt", [(257, 1), (40, 257)])
def test_opt_in_refuses_more_than_256(S, Lt):
    with pytest.raises(RuntimeError, match="256"):
        _bare_run(attn_stream=1)._require_attn_keys(S, Lt)


@pytest.mark.parametrize("attrs", [{}, {"attn_stream": 0}])
def test_without_the_opt_in_the_192_refusal_stays(attrs):
    run = _bare_run(**attrs)
    run._require_attn_keys(80, 100)
    for S, Lt in ((200, 1), (100, 100), (256, 100)):
        with pytest.raises(RuntimeError, match=r"> 192 not built .*pad16\(S\) \+ pad16\(Lt\) <= 192"):
            run._require_attn_keys(S, Lt)


def test_model_cfg_attn_stream_reaches_the_backbone():
    """``default_args(attn_stream=1)`` -> SegFormerX.attn_stream -> BackboneRun.attn_stream; absent means 0."""
    from segmminterest_amd import engine as E
    from segmminterest_amd.trainer import default_args, init_model
    for over, want in (({}, 0), ({"attn_stream": 1}, 1)):
        margs = default_args(num_layers_enc=2, d_model=32, nhead=2, input_type={"user": "image", "photo": "image"}, **over)
        model = init_model(margs, n_users=5, n_items=5, input_dim=32, max_vid_len=40, max_usr_len=10)
        bbs = [m for m in model.modules() if type(m).__name__ == "SegFormerX"]
        assert bbs and all(bb.attn_stream == want for bb in bbs)
        assert E.BackboneRun(None, bbs[0], "", 0).attn_stream == want
    assert not hasattr(argparse.Namespace(), "attn_stream")


@pytest.mark.parametrize("Lq,La,Lb", [(40, 257, 1), (40, 40, 257), (257, 40, 40)])
def test_attention_entry_points_refuse_more_than_256(Lq, La, Lb):
    H, L = _lib()
    buf = (ctypes.c_double * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15          # 16-byte aligned, never dereferenced: the size check fails first
    msg = L.segmm_attn_fwd(2, 2, 16, Lq, La, Lb, p, p, 32, p, p, 32, p, p, 32, p, p, p, p, 32, p, 0.0, 0, 0, None, None, None)
    assert msg != 0
    msg = L.segmm_last_error().decode()
    assert "256" in msg and "attn" in msg and "La=%d" % La in msg
    for phase in (0, 2, 4):
        rc = L.segmm_attn_bwd(2, 2, 16, Lq, La, Lb, p, p, 32, p, p, 32, p, p, 32, p, p, p, p, p, 32, p, 32, p, p, p, 32, p, p, 32, p, p, 32,
                              0.0, 0, 0, None, None, None, phase, None, None)
        assert rc != 0 and "256" in L.segmm_last_error().decode()


def test_abi_dispatch_table_and_knob_table():
    H, L = _lib()
    assert L.segmm_abi_version() == H.ABI_VERSION == 30
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_cmd_dispatch.py"), "--check"])
    dump = H.config_dump()
    assert dump["ATT_STREAM"][0] == 0 and "streamed" in dump["ATT_STREAM"][1]
