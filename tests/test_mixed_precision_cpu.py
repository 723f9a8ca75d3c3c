"""``Trainer(mixed_precision=...)`` without a GPU: how the argument is resolved and refused, what the ParamStore hands the GEMM
helpers in a step pass and in an evaluation pass, which entry point ``hipabi.gemm_p`` calls at each product count (against a fake
library that notes the calls), and the new export's place in the generated ABI tables."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from segmminterest_amd import _abi, engine as E, hipabi as H, trainer as TR      # noqa: E402

ALL = dict(forward=True, dgrad=True, wgrad=True)


def test_argument_forms():
    assert E.resolve_mixed_precision(None) is None and E.resolve_mixed_precision(False) is None
    assert E.resolve_mixed_precision(True) == ALL and E.resolve_mixed_precision({}) == ALL
    assert E.resolve_mixed_precision(dict(wgrad=False)) == dict(forward=True, dgrad=True, wgrad=False)
    assert E.resolve_mixed_precision(dict(forward=1, dgrad=0, wgrad=0)) == dict(forward=True, dgrad=False, wgrad=False)
    # all False equals off
    assert E.resolve_mixed_precision(dict(forward=False, dgrad=False, wgrad=False)) is None


def test_unknown_keys_and_types_are_refused_by_name():
    with pytest.raises(ValueError, match="backward.*fwd|fwd.*backward") as e:
        E.resolve_mixed_precision(dict(fwd=True, backward=True, wgrad=True))
    assert "wgrad" in str(e.value)          # (the message lists the roles)
    for bad in (1, "fp16", [True], 0.5):
        with pytest.raises(TypeError, match="mixed_precision"):
            E.resolve_mixed_precision(bad)


@pytest.mark.parametrize("engine", ["f32", "bf16x6", "f16x3"])
def test_other_gemm_engines_are_refused_by_name(engine, monkeypatch):
    monkeypatch.setattr(H, "GEMM_ENGINE", {"f32": H.ENGINE_F32, "bf16x6": H.ENGINE_BF16X6, "f16x3": H.ENGINE_F16X3}[engine])
    with pytest.raises(RuntimeError, match="SEGMM_GEMM=%s" % engine):
        E.resolve_mixed_precision(True)
    # off stays off under any engine: nothing to refuse
    assert E.resolve_mixed_precision(None) is None and E.resolve_mixed_precision(dict(forward=False, dgrad=False, wgrad=False)) is None


def _bare_trainer():
    """a Trainer object around a bare store: only what the ``mixed_precision`` property touches"""
    st = types.SimpleNamespace(mixed_precision=None, in_train_step=False, products=dict(E.ALL_PRODUCTS))
    st.set_pass_products = types.MethodType(E.ParamStore.set_pass_products, st)
    t = TR.Trainer.__new__(TR.Trainer)
    t.model = types.SimpleNamespace(_store=st)
    return t, st


def test_trainer_property_returns_the_resolved_setting():
    t, st = _bare_trainer()
    assert t.mixed_precision is None
    t.mixed_precision = True
    assert t.mixed_precision == ALL and st.mixed_precision == ALL
    got = t.mixed_precision
    got["forward"] = False          # a copy: the store's setting is not edited through it
    assert st.mixed_precision == ALL
    t.mixed_precision = dict(dgrad=False)
    assert t.mixed_precision == dict(forward=True, dgrad=False, wgrad=True)
    t.mixed_precision = dict(forward=False, dgrad=False, wgrad=False)
    assert t.mixed_precision is None
    with pytest.raises(ValueError, match="bwd"):
        t.mixed_precision = dict(bwd=True)
    assert t.mixed_precision is None
    assert "mixed_precision" in TR.Trainer.__init__.__code__.co_varnames


def test_only_step_passes_take_the_setting():
    t, st = _bare_trainer()
    t.mixed_precision = dict(dgrad=False)
    st.set_pass_products(False)          # an evaluation pass (eval_step, valid_model, test_model, dump_logits, EMA-applied)
    assert st.products == dict(forward=3, dgrad=3, wgrad=3)
    st.set_pass_products(True)           # a pass of the optimisation step
    assert st.products == dict(forward=1, dgrad=3, wgrad=1)
    t.mixed_precision = None
    st.set_pass_products(True)
    assert st.products == dict(forward=3, dgrad=3, wgrad=3)


def test_the_setting_is_part_of_what_a_recording_is_checked_against():
    t, st = _bare_trainer()
    t.opt = types.SimpleNamespace(lr=1e-3, schedule=None, wd=0.0, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, group_table=lambda: ())
    t.ema = None
    off = t._hyper()
    t.mixed_precision = True
    on = t._hyper()
    t.mixed_precision = dict(wgrad=False)
    assert len({off, on, t._hyper()}) == 3
    t.mixed_precision = False
    assert t._hyper() == off


class _FakeLib:
    def __init__(self):
        self.calls = []

    def segmm_gemm_p(self, *a):
        self.calls.append(("segmm_gemm_p", a))
        return 0

    def segmm_gemm_pq(self, *a):
        self.calls.append(("segmm_gemm_pq", a))
        return 0


def test_gemm_p_picks_the_entry_point(monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(H, "lib", lambda: fake)
    monkeypatch.setattr(H, "_stream", lambda: 0x5EED)
    pl, hdr = torch.zeros(64, 128, dtype=torch.float16), torch.zeros(64)
    a, b, c = H.PT(pl, hdr, 64, 64), H.PT(pl, hdr, 64, 64), torch.zeros(64, 64)
    H.gemm_p(H.LAYOUT_NT, 64, 64, 64, a, b, c, 64)
    H.gemm_p(H.LAYOUT_NT, 64, 64, 64, a, b, c, 64, products=3)
    H.gemm_p(H.LAYOUT_NT, 64, 64, 64, a, b, c, 64, products=1)
    n_p = len(_abi.PROTOTYPES["segmm_gemm_p"])
    (n0, a0), (n1, a1), (n2, a2) = fake.calls
    # the default and products=3 are the call the binding has always made: same entry point, same arguments
    assert n0 == n1 == "segmm_gemm_p" and a0 == a1 and len(a0) == n_p and a0[-1] == 0x5EED
    assert n2 == "segmm_gemm_pq" and len(a2) == n_p + 1 and a2[:-2] == a0[:-1] and a2[-2:] == (1, 0x5EED)


def test_the_export_is_in_the_generated_tables():
    p, q = _abi.PROTOTYPES["segmm_gemm_p"], _abi.PROTOTYPES["segmm_gemm_pq"]
    assert q[:-2] == p[:-1] and q[-2] == ("products", "i") and q[-1] == p[-1] == ("stream", "p")
    inc = open(os.path.join(os.path.dirname(os.path.abspath(H.__file__)), "csrc", "cmd_dispatch.inc")).read()
    assert '"segmm_gemm_pq",' in inc and '"segmm_gemm_p",' in inc
    # no new knob and no new environment switch: the product count travels in the call
    src = open(os.path.join(os.path.dirname(os.path.abspath(H.__file__)), "csrc", "capi.hip")).read()
    assert "PRODUCTS" not in src and "SEGMM_MIXED" not in src
