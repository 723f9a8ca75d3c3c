"""The host statement of lazy tables beside the weight average (tests/lazy_ema_ref.py): the protocol leaves p, m, v AND the shadow
equal in every bit to the dense update followed by the dense EMA update of every step, and every planted defect of order is caught
by that bitwise comparison -- which is what makes the bitwise GPU comparisons of tests/test_lazy_ema_gpu.py a test of the order of
the replayed lerps.  Inputs: warm-up on (w_t moves every step), 16 steps with a ring of 4, a row that is never listed, a row listed
twice in one step, and a data-parallel flavour in which the head catches up only a part of the step's rows."""
import numpy as np
import pytest

import ema_ref as E
import lazy_ema_ref as LE
import lazy_table_ref as L

F = np.float32
ROWS, WIDTH, STEPS, CAP, NEVER, DECAY = 23, 8, 16, 4, 5, 0.99
HP = dict(b1=0.9, b2=0.999, eps=1e-8, wd=1e-2)


def _bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def _case():
    rng = np.random.default_rng(17)
    p0 = (0.1 * rng.standard_normal((ROWS, WIDTH))).astype(F)
    m0 = (0.1 * rng.standard_normal((ROWS, WIDTH))).astype(F)
    v0 = (0.01 * rng.uniform(0.25, 1.0, size=(ROWS, WIDTH))).astype(F)
    rates = [F(1e-2 * (1.0 + 0.5 * np.cos(0.7 * k)) + 1e-4 * k) for k in range(STEPS)]
    id_lists, grads = [], []
    for k in range(STEPS):
        ids = rng.integers(0, ROWS, size=5)
        ids[ids == NEVER] = NEVER + 1
        ids = np.concatenate([ids, ids[:2], [-1, ROWS, -2 ** 40]])          # the first two ids are listed twice; ids outside the table
        id_lists.append(ids)
        grads.append(L.dense_grad(rng.standard_normal((ROWS, WIDTH)).astype(F), ids, ROWS))
    return p0, m0, v0, rates, id_lists, grads


def _want():
    p0, m0, v0, rates, id_lists, grads = _case()
    dense = L.dense_run(p0, m0, v0, grads, rates, HP)
    return dense, LE.dense_shadow(p0, dense, DECAY)


def _run(defect=None, own_part=None):
    p0, m0, v0, rates, id_lists, grads = _case()
    t = LE.LazyEmaTable(p0, m0, v0, CAP, HP, DECAY, defect=defect)
    for ids, g, lr in zip(id_lists, grads, rates):
        t.step(ids, g, lr, own_ids=None if own_part is None else ids[:own_part])
    t.flush()
    return t


def test_inputs_are_what_the_statement_needs():
    _, _, _, rates, id_lists, _ = _case()
    ws = [E.w_at(DECAY, t) for t in range(1, STEPS + 1)]
    assert STEPS >= 12 and CAP == 4
    assert len(set(float(w) for w in ws)) == STEPS and min(ws) > E.weight(DECAY)          # warm-up: another weight every step
    assert not any(NEVER in ids for ids in id_lists)
    assert all(len(ids) > len(set(ids.tolist())) for ids in id_lists)          # every step lists a row twice
    rows = [set(int(r) for r in ids if 0 <= r < ROWS) for ids in id_lists]
    gaps = [k - max(j for j in range(k) if r in rows[j]) for k in range(1, STEPS) for r in rows[k] if any(r in rows[j] for j in range(k))]
    assert max(gaps) >= 3          # some listed row replays a gap of more than one step (one_lerp / final_p / newest_w need it)


@pytest.mark.parametrize("own_part", [None, 3], ids=["single", "data_parallel"])
def test_protocol_equals_dense_adamw_and_dense_ema_bit_for_bit(own_part):
    dense, shadows = _want()
    p0, m0, v0, rates, id_lists, grads = _case()
    t = LE.LazyEmaTable(p0, m0, v0, CAP, HP, DECAY)
    for k, (ids, g, lr) in enumerate(zip(id_lists, grads, rates)):
        t.step(ids, g, lr, own_ids=None if own_part is None else ids[:own_part])
        assert t.pending <= CAP
        rows = sorted(set(int(r) for r in ids if 0 <= r < ROWS))          # the step's rows and their shadow are current after it
        for got, want in zip((t.p, t.m, t.v, t.shadow), dense[k] + (shadows[k],)):
            assert np.array_equal(_bits(got[rows]), _bits(want[rows])), k
    assert t.stamps[NEVER] < STEPS and not np.array_equal(_bits(t.shadow[NEVER]), _bits(shadows[-1][NEVER]))
    t.flush()
    assert t.n_flushes >= 3 and (t.stamps == STEPS).all()
    for name, got, want in zip(("p", "m", "v", "shadow"), (t.p, t.m, t.v, t.shadow), dense[-1] + (shadows[-1],)):
        assert np.array_equal(_bits(got), _bits(want)), name
    assert not np.array_equal(_bits(t.shadow), _bits(t.p))


@pytest.mark.parametrize("own_part", [None, 3], ids=["single", "data_parallel"])
@pytest.mark.parametrize("defect", LE.DEFECTS)
def test_planted_defects_are_rejected(defect, own_part):
    """Each defect leaves p, m, v alone (they are defects of the SHADOW's order) and is caught by the shadow's bits."""
    dense, shadows = _want()
    t = _run(defect, own_part)
    for got, want in zip((t.p, t.m, t.v), dense[-1]):
        assert np.array_equal(_bits(got), _bits(want)), defect
    assert not np.array_equal(_bits(t.shadow), _bits(shadows[-1])), defect
