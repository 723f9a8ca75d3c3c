"""The AdamW yardstick of tests/test_adamw_gpu.py, shown sound without a GPU (tests/adamw_ref.py): it accepts a faithful fp32
emulation of adamw_elem4 and rejects four planted defects; the float hyperparameters of the C ABI are harmless; and the host's
bias corrections are the numbers the device step state is compared with."""
import math
from decimal import Decimal, getcontext

import numpy as np
import pytest

import adamw_ref as A

F = np.float32


def test_yardstick_accepts_the_emulation_and_rejects_every_mutant():
    """Every regime of the GPU tests at its checkpoints: the unmutated emulation's E_p, E_m, E_v against R_abi stay within
    MARGIN x torch32's against R_true; each of the four mutants exceeds the margin in at least one regime and checkpoint (all of
    them in E_p: they leave m and v alone).  Anyone who loosens the margin until a mutant passes fails here."""
    worst = [0.0, 0.0, 0.0]
    caught = {m: [] for m in A.MUTANTS}
    for name in A.REGIMES:
        r, y = A.regime(name), A.yardstick(name)
        got = A.run(r, A.emul32)
        for t in r["checkpoints"]:
            ratios = y.ratios(got[t], t)
            assert max(ratios) <= A.MARGIN, (name, t, ratios)
            worst = [max(a, b) for a, b in zip(worst, ratios)]
        for mut in A.MUTANTS:
            bad = A.run(r, A.emul32, mutant=mut)
            for t in r["checkpoints"]:
                worst_of = max(y.ratios(bad[t], t))
                if worst_of > A.MARGIN:
                    caught[mut].append((name, t, float("%.3g" % worst_of)))
    print("worst emulation ratios (E_p, E_m, E_v):", worst)
    for mut, where in caught.items():
        print(mut, "rejected at", where)
        assert where, "mutant %s passes the yardstick in every regime" % mut
        # a margin raised to 4 (the most the yardstick's rule allows) would still reject it
        assert max(x for _, _, x in where) > 4.0, mut


def test_float_abi_is_harmless():
    """The C ABI takes the hyperparameters as float.  (1) The parameter trajectory does not care: |R_abi - R_true| in p stays below
    torch32's own E_p against R_true at every checkpoint of every regime (the bias corrections use the same rounded betas, so the
    rounding cancels between moment and correction).  (2) exp_avg_sq does: float32(0.999) = 0.999 + 1.2875e-8, so the factor
    1 - b2 in front of g^2 is 1.2875e-5 (relative) smaller than torch's.  Closed form: v_abi / v_true = (1 - b2') / (1 - b2) exactly
    at t = 1, (1 - b2'^t) / (1 - b2^t) for a constant gradient, and for any gradient history within
    (1 - b2') / (1 - b2) x [1, (b2' / b2)^(t-1)] -- that is -1.2875e-5 at t = 1 and between -1.2875e-5 and -8.9e-6 at t = 300 --
    a deviation a checkpoint exported through FusedAdamW.state_dict() carries into torch.optim.AdamW.  The decay factor is the
    same fp32 number on both paths."""
    for name in A.REGIMES:
        r, y = A.regime(name), A.yardstick(name)
        assert A.decay_factor(r["hp"]["lr"], r["hp"]["wd"], True) == A.decay_factor(r["hp"]["lr"], r["hp"]["wd"], False)
        for t in r["checkpoints"]:
            d = float(np.max(np.abs(y.r_abi[t][0] - y.r_true[t][0])))
            assert d < y.torch_err[t][0], (name, t, d, y.torch_err[t][0])
    b2 = A.HP["b2"]
    b2f = float(F(b2))
    c1 = (1.0 - b2f) / (1.0 - b2)
    assert abs((c1 - 1.0) + 1.2875e-5) < 1e-9
    r, y = A.regime("unit"), A.yardstick("unit")
    live = slice(A.ZEROS, None)
    for t in r["checkpoints"]:
        ratio = y.r_abi[t][2][live] / y.r_true[t][2][live]
        lo, hi = c1, c1 * (b2f / b2) ** (t - 1)
        tol = 4 * t * 2.0 ** -53          # float64 rounding of two t-step recurrences
        assert ratio.min() >= lo - tol and ratio.max() <= hi + tol, (t, ratio.min() - 1, ratio.max() - 1, lo - 1, hi - 1)
        if t == 1:
            assert np.max(np.abs(ratio - c1)) <= tol
        print("t = %d: exp_avg_sq of R_abi / R_true - 1 in [%.4e, %.4e]" % (t, ratio.min() - 1, ratio.max() - 1))
    # a constant gradient: v_t = g^2 (1 - b2^t) on both sides
    g = [np.full(8, 0.37, dtype=F)] * 300
    ck = (1, 3, 10, 300)
    va = A.ref64(np.zeros(8), g, abi_rounded=True, checkpoints=ck, **A.HP)
    vt = A.ref64(np.zeros(8), g, abi_rounded=False, checkpoints=ck, **A.HP)
    for t in ck:
        want = (1.0 - b2f ** t) / (1.0 - b2 ** t)
        # float64 rounding of that closed form: 1 - b2^t cancels, which costs a factor 1 / (1 - b2^t); the recurrences add t roundings
        assert np.max(np.abs(va[t][2] / vt[t][2] - want)) <= 8 * 2.0 ** -53 * (t + 1.0 / (1.0 - b2 ** t)), t


BC_STEPS = (1, 2, 10, 1000, 10 ** 6)


@pytest.mark.parametrize("b", [0.9, 0.999, 0.8, 0.99, 0.95, 0.9999])
def test_host_bias_corrections(b):
    """host_bc(b, t) = float32(1 - double(float32(b))^t) and float32(sqrt(that double)) -- capi.hip's adamw_flat, and what the
    device step state must return within an ulp -- against 60-digit decimal arithmetic: each is the correctly rounded fp32 value
    of the exact quantity, at t = 1 the exact fp32 difference 1.0f - b, and (1, 1) once b^t is below half an ulp of 1."""
    getcontext().prec = 60
    bf = float(F(b))
    for t in BC_STEPS:
        bc, bcs = A.host_bc(b, t)
        assert type(bc) is F and type(bcs) is F
        exact = Decimal(1) - Decimal(bf) ** t
        assert bc == F(float(exact)), (b, t)
        assert bcs == F(float(exact.sqrt())), (b, t)
        assert 0 < bc <= 1 and bc <= bcs <= 1
        if t == 1:
            assert bc == F(1.0) - F(b)
        if t * math.log(bf) < math.log(2.0 ** -26):
            assert bc == 1 and bcs == 1
    assert A.host_bc(b, 10 ** 6) == (F(1.0), F(1.0))
    assert all(A.host_bc(b, t)[0] < A.host_bc(b, u)[0] or A.host_bc(b, u)[0] == 1 for t, u in zip(BC_STEPS, BC_STEPS[1:]))
