"""Global-norm gradient clipping, the parts that need no GPU: the C entry points are exported, declared and recordable, they
validate their arguments without touching the device, and FusedAdamW / Trainer validate ``max_grad_norm``."""
import math

import pytest
import torch

from helpers import build_model, load_case

NEW = ("segmm_grad_norm", "segmm_adamw_scaled", "segmm_adamw_table_scaled")


def test_clip_entry_points_exported_and_dispatchable():
    from segmminterest_amd import hipabi as H
    L = H.lib()
    ops = H.op_ids()
    for n in NEW:
        assert n in H.SIGNATURES and hasattr(L, n), n
        assert n in ops, n          # segmm_run_phase can replay it from a recorded step
    assert L.segmm_abi_version() == H.ABI_VERSION == 30
    # the unscaled entry points keep their argument lists
    assert len(H.SIGNATURES["segmm_adamw"]) == 12 and len(H.SIGNATURES["segmm_adamw_table"]) == 17


def test_grad_norm_rejects_bad_arguments():
    from segmminterest_amd import hipabi as H
    L = H.lib()
    g, scratch, out2 = 4096, 8192, 16384          # never dereferenced: every call below fails its argument check first

    def err(rc):
        assert rc != 0
        return L.segmm_last_error().decode()

    assert "null" in err(L.segmm_grad_norm(None, 4, 1.0, scratch, out2, None))
    assert "null" in err(L.segmm_grad_norm(g, 4, 1.0, None, out2, None))
    assert "null" in err(L.segmm_grad_norm(g, 4, 1.0, scratch, None, None))
    assert "alignment" in err(L.segmm_grad_norm(g + 2, 4, 1.0, scratch, out2, None))
    assert "alignment" in err(L.segmm_grad_norm(g, 4, 1.0, scratch + 4, out2, None))
    assert "n=-1" in err(L.segmm_grad_norm(g, -1, 1.0, scratch, out2, None))
    for bad in (0.0, -1.0, float("nan"), -math.inf):
        assert "max_norm" in err(L.segmm_grad_norm(g, 4, bad, scratch, out2, None)), bad


def test_scaled_adamw_rejects_bad_arguments():
    from segmminterest_amd import hipabi as H
    L = H.lib()
    p, g, m, v, c = 4096, 8192, 12288, 16384, 20480
    hp = (1e-3, 0.9, 0.999, 1e-8, 1e-4)

    def err(rc):
        assert rc != 0
        return L.segmm_last_error().decode()

    assert "coef" in err(L.segmm_adamw_scaled(p, g, m, v, 8, *hp, 1, None, None))
    assert "pointer" in err(L.segmm_adamw_scaled(p, None, m, v, 8, *hp, 1, c, None))
    assert "alignment" in err(L.segmm_adamw_scaled(p + 4, g, m, v, 8, *hp, 1, c, None))
    assert "step=0" in err(L.segmm_adamw_scaled(p, g, m, v, 8, *hp, 0, c, None))
    ids, flags = 24576, 28672
    assert "coef" in err(L.segmm_adamw_table_scaled(p, g, m, v, 10, 8, ids, 3, flags, *hp, 1, None, None))
    assert "pointer" in err(L.segmm_adamw_table_scaled(p, None, m, v, 10, 8, ids, 3, flags, *hp, 1, c, None))
    assert "pointer" in err(L.segmm_adamw_table_scaled(p, g, m, v, 10, 8, None, 3, flags, *hp, 1, c, None))
    assert "width" in err(L.segmm_adamw_table_scaled(p, g, m, v, 10, 6, ids, 3, flags, *hp, 1, c, None))
    assert "sizes" in err(L.segmm_adamw_table_scaled(p, g, m, v, -1, 8, ids, 3, flags, *hp, 1, c, None))


def test_recorder_converts_clip_arguments():
    from segmminterest_amd import hipabi as H
    ops = H.op_ids()
    rec = H.Recorder(111, 222)
    rec.mark(H.PHASE_STEP_TAIL)
    rec.call("segmm_grad_norm", (4096, 1000003, 10.0, 8192, 12288, 111))
    rec.call("segmm_grad_norm", (4096, 7, math.inf, 8192, 12288, 111))
    rec.call("segmm_adamw_scaled", (4096, 8192, 0, None, 10, 1e-3, 0.9, 0.999, 1e-8, 1e-4, -1, 12292, 111))
    rec.call("segmm_adamw_table_scaled", (4096, 8192, 16384, 20480, 100, 8, 24576, 5, 28672, 1e-3, 0.9, 0.999, 1e-8, 1e-4, -1, 12292, 222))
    (ph, a), = rec.finish()
    assert ph.n_cmds == 4
    assert a[0].op == ops["segmm_grad_norm"] and a[0].stream == 0
    assert a[0].a[0].p == 4096 and a[0].a[1].i == 1000003 and a[0].a[2].f == 10.0 and a[0].a[3].p == 8192 and a[0].a[4].p == 12288
    assert a[1].a[2].f == math.inf
    assert a[2].op == ops["segmm_adamw_scaled"] and a[2].a[3].p is None and a[2].a[10].i == -1 and a[2].a[11].p == 12292
    assert a[3].op == ops["segmm_adamw_table_scaled"] and a[3].stream == 1 and a[3].a[5].i == 8 and a[3].a[15].p == 12292
    assert a[3].a[9].f == pytest.approx(1e-3) and a[3].a[14].i == -1


@pytest.mark.parametrize("bad", [0, 0.0, -1, -1e-3, float("nan"), -math.inf, "ten", [1.0]])
def test_max_grad_norm_validation(bad):
    from segmminterest_amd.trainer import FusedAdamW, Trainer
    cfg, _, _, _ = load_case("img_d32_N2")
    model = build_model(cfg)
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedAdamW(model, max_grad_norm=bad)
    with pytest.raises(ValueError, match="max_grad_norm"):
        Trainer(model, max_grad_norm=bad)


def test_max_grad_norm_accepted_values():
    from segmminterest_amd.trainer import FusedAdamW
    cfg, _, _, _ = load_case("img_d32_N2")
    model = build_model(cfg)
    assert FusedAdamW(model).max_grad_norm is None
    assert FusedAdamW(model, max_grad_norm=math.inf).max_grad_norm == math.inf
    assert FusedAdamW(model, max_grad_norm=10).max_grad_norm == 10.0
    assert FusedAdamW(model, max_grad_norm=torch.tensor(0.5)).max_grad_norm == 0.5
    assert FusedAdamW(model, max_grad_norm=10.0).grad_norm is None          # no step yet
