"""The weight average (Trainer(ema=...), segmm_ema_update / segmm_vec_swap), the parts that need no GPU: the host reference against the
float64 closed form, argument parsing and every refusal by name, the generated ABI tables and the two new exports."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import ema_ref as R
from helpers import ROOT

F = np.float32


@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("decay", [0.9, 0.999, 0.0])
def test_reference_against_float64_closed_form(decay, warmup):
    """Constant p over T = 50 steps: s_T = p + (s_0 - p) prod(1 - w_t).  Bound: T * 3 * 2^-24 * max(|s_0|, |p|) -- three roundings per
    step, each at most half an ulp (2^-24 relative) of a value no larger than max(|s_0|, |p|) (s stays between s_0 and p, p - s and its
    product with w <= 1 are no larger than 2 max and are counted in the 3), errors of earlier steps only shrink (factor 1 - w_t <= 1)."""
    T = 50
    rng = np.random.default_rng(11)
    for s0, p in zip(rng.standard_normal(64).astype(F) * F(3), rng.standard_normal(64).astype(F)):
        s = F(s0)
        for t in range(1, T + 1):
            s = R.update(s, p, decay, t, warmup)
        want = R.closed_form(s0, p, decay, T, warmup)
        bound = T * 3 * 2.0 ** -24 * max(abs(float(s0)), abs(float(p)))
        assert abs(float(s) - want) <= bound, (decay, warmup, float(s0), float(p), float(s), want, bound)


def test_reference_weights():
    assert R.weight(0.999) == F(1.0 - 0.999) and R.w_at(0.999, 1) == F(9.0 / 11.0) and R.w_at(0.9, 1000) == F(1.0 - 0.9)
    assert R.w_at(0.999, 1, warmup=False) == R.weight(0.999)
    # decay_t = min(decay, (1 + t) / (10 + t)) written as its complement
    for t in (1, 2, 9, 80, 1000, 10 ** 6):
        assert abs(float(R.w_at(0.999, t)) - (1.0 - min(0.999, (1.0 + t) / (10.0 + t)))) < 1e-7


def test_parse_ema_and_refusals_by_name():
    from segmminterest_amd.trainer import FusedAdamW, Trainer, WeightEMA, parse_ema
    assert parse_ema(None) is None
    assert parse_ema(0.99) == (0.99, True) and parse_ema(0) == (0.0, True)
    assert parse_ema({}) == (0.999, True) and parse_ema(dict(decay=0.9, warmup=False)) == (0.9, False)
    for bad in (1.0, -0.1, 1.5, float("nan"), "0.9", True, [0.9], dict(decay=1.0), dict(decay=None)):
        with pytest.raises(ValueError, match="ema: decay must be a float with 0 <= decay < 1"):
            parse_ema(bad)
    with pytest.raises(ValueError, match="ema: unknown key 'update_every'"):
        parse_ema(dict(decay=0.9, update_every=2))
    with pytest.raises(ValueError, match="ema: warmup must be a bool"):
        parse_ema(dict(warmup=1))
    # the constructors refuse before they touch the model
    with pytest.raises(ValueError, match="ema: decay"):
        Trainer(None, ema=1.0)
    with pytest.raises(ValueError, match="ema: unknown key 'beta'"):
        FusedAdamW(None, ema=dict(beta=0.9))
    assert FusedAdamW(None).ema is None
    e = FusedAdamW(None, ema=dict(decay=0.9, warmup=False)).ema
    assert isinstance(e, WeightEMA) and e.decay == 0.9 and e.warmup is False and e.shadow is None
    assert e.weight == float(R.weight(0.9)) and e.hyper() == (float(R.weight(0.9)), False)
    with pytest.raises(ValueError, match="ema: decay"):
        e.decay = 1.0
    e.decay = 0.5
    assert e.hyper() == (0.5, False)
    w = FusedAdamW(None, ema=0.999).ema
    assert [w.weight_at(t) for t in (1, 2, 9, 1000, 10 ** 6)] == [float(R.w_at(0.999, t)) for t in (1, 2, 9, 1000, 10 ** 6)]


def test_evaluation_entry_points_refuse_ema_without_one():
    from segmminterest_amd.trainer import Trainer, fit
    tr = Trainer.__new__(Trainer)
    tr.ema = None
    for who, call in (("valid_model", lambda: tr.valid_model([], ema=True)), ("test_model", lambda: tr.test_model([], [], ema=True)),
                      ("dump_logits", lambda: tr.dump_logits([], ema=True))):
        with pytest.raises(ValueError, match=r"%s\(ema=True\) needs Trainer\(ema=\.\.\.\)" % who):
            call()
    tr.device_state = False
    with pytest.raises(ValueError, match=r"fit\(ema_valid=True\) needs Trainer\(ema=\.\.\.\)"):
        fit(tr, [], [], 1, ema_valid=True)


def test_applied_refusals_by_name():
    from segmminterest_amd.trainer import FusedAdamW, Trainer
    e = FusedAdamW(None, ema=0.9).ema
    e.is_applied = True
    with pytest.raises(RuntimeError, match="nested applied"):
        with e.applied():
            pass
    tr = Trainer.__new__(Trainer)
    tr.ema, tr.device_state, tr.micro_batch = e, True, None
    tr.__dict__["_recorded"] = {}
    for who, call in (("train_step", lambda: tr.train_step({})), ("record", lambda: tr.record({})), ("run_recorded", lambda: tr.run_recorded({}))):
        with pytest.raises(RuntimeError, match=r"%s\(\) inside ema\.applied\(\)" % who):
            call()
    for call in (e.state_dict, lambda: e.load_state_dict({}), e.update):
        with pytest.raises(RuntimeError, match=r"ema\.applied\(\)"):
            call()


def test_load_checkpoint_refuses_a_file_without_model_ema(tmp_path):
    import torch
    from segmminterest_amd.trainer import CheckPointer, FusedAdamW

    class Opt:
        def state_dict(self):
            return {"k": 1}

        def load_state_dict(self, sd):
            self.got = sd

    class Ema:
        def state_dict(self):
            return {"w": torch.full((2, 2), 3.0)}

        def load_state_dict(self, sd):
            self.got = sd

    model = torch.nn.Linear(2, 2)
    ck = CheckPointer("main_metric", str(tmp_path), mode="max")
    ck.save_checkpoint(model, Opt(), 0, {"main_metric": 0.5})
    sd = ck.load_checkpoint(model, Opt())          # a file without the key loads as ever
    assert "model_ema" not in sd
    e = Ema()
    with pytest.raises(KeyError, match="model_ema"):
        ck.load_checkpoint(model, Opt(), ema=e)
    assert not hasattr(e, "got")
    ck.save_checkpoint(model, Opt(), 1, {"main_metric": 0.6}, ema=e)
    for mode in ("latest", "best"):
        e2, o2 = Ema(), Opt()
        sd = ck.load_checkpoint(model, o2, mode=mode, ema=e2)
        assert set(sd) == {"model", "optimizer", "num_epochs", "metrics", "model_ema"}
        assert torch.equal(e2.got["w"], torch.full((2, 2), 3.0)) and o2.got == {"k": 1}
    assert "model_ema" in ck.load_checkpoint(model, Opt())          # and is ignored without ema=
    assert FusedAdamW(None).ema is None


def test_generated_tables_are_current_and_list_the_exports():
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_cmd_dispatch.py"), "--check"])
    from segmminterest_amd import _abi, hipabi as H
    assert H.ABI_VERSION == 30 and _abi.ABI_VERSION == 30          # additive exports: the version stays
    P = _abi.PROTOTYPES
    assert P["segmm_ema_update"] == (("shadow", "p"), ("p", "p"), ("n", "i64"), ("weight", "f"), ("warmup", "i"), ("step", "i"), ("stream", "p"))
    assert P["segmm_vec_swap"] == (("a", "p"), ("b", "p"), ("n", "i64"), ("stream", "p"))
    hdr = open(os.path.join(ROOT, "include", "segmm_hip.h")).read()
    assert "#define SEGMM_ABI_VERSION 30" in hdr
    inc = open(os.path.join(ROOT, "segmminterest_amd", "csrc", "cmd_dispatch.inc")).read()
    assert '"segmm_ema_update",' in inc and '"segmm_vec_swap",' in inc


def test_library_exports_both_symbols_as_recordable_commands():
    from segmminterest_amd import hipabi as H
    L = ctypes.CDLL(H.LIB_PATH)
    assert hasattr(L, "segmm_ema_update") and hasattr(L, "segmm_vec_swap")
    L.segmm_abi_version.restype = ctypes.c_int
    assert L.segmm_abi_version() == 30
    L.segmm_cmd_op_name.restype = ctypes.c_char_p
    names = [L.segmm_cmd_op_name(i).decode() for i in range(L.segmm_cmd_op_count())]
    assert "segmm_ema_update" in names and "segmm_vec_swap" in names and names == sorted(names)
    assert "EMA_NT" in H.config_dump()
