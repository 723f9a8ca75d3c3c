"""The AdamW kernels and the device step state on the MI355X against float64 (tests/adamw_ref.py; tests/test_adamw_cpu.py shows
the yardstick sound).  Rule of every comparison: E_p, E_m, E_v of the kernel against R_abi (float64 with the hyperparameters as
the C ABI's floats) <= MARGIN = 3 x the same errors of torch.optim.AdamW (CPU, fp32) against R_true (float64 with the Python
doubles), same regime, same step.  The bit-for-bit identities between the five kernel variants are pinned elsewhere
(test_clip_gpu.py, test_eval_gpu.py, test_dp_gpu.py) and not repeated here.

Worst ratio (error against R_abi) / (torch's error against R_true) over the checkpoints, per regime and quantity.  The per-regime
figures below are those of the numpy-fp32 emulation of the kernel (adamw_ref.emul32, tests/test_adamw_cpu.py), which the device
reproduces bit for bit if its fp32 multiply, add, divide and square root are correctly rounded and nothing is contracted; all
tests of this file pass on an MI355X within the margin, but their per-regime ratios were not recorded from that run.  Every test
prints its ratios in lines that start with RATIO (pytest -s).

    regime         E_p    E_m    E_v
    unit          1.05   1.26   0.82
    eps           1.22   1.19   1.02
    decades       1.27   1.76   0.75
    decay         1.12   1.30   0.80
    betas_fast    1.43   1.30   1.13
    betas_slow    0.86   1.53   0.85
    late          1.00   1.25   1.04

Measured on an MI355X (E_p, worst parameter): FusedAdamW horizon 1.01 at step 20 and 1.06 at step 40; the step-20 state_dict
continued under torch.optim.AdamW 1.40 at step 40.

A ratio above 3 is a finding to be explained from the arithmetic, not a margin to be raised (adamw_ref.MARGIN; 4 at the most, with
the explanation next to this table, and test_adamw_cpu.py still rejecting all four mutants).
"""
import copy

import numpy as np
import pytest
import torch

import adamw_ref as A
from helpers import build_model, load_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
OFF, GUARD = 96, 32          # where the tests place a range inside its buffers, and the untouched floats checked around it


def _H():
    from segmminterest_amd import hipabi as H
    H.lib()
    return H


def _dev(x):
    return torch.from_numpy(np.array(x, dtype=F)).to(DEV)


def _bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def _report(what, ratios):
    print("RATIO %-44s E_p %5.2f  E_m %5.2f  E_v %5.2f" % ((what,) + tuple(ratios)))


def _check(what, ratios):
    _report(what, ratios)
    assert max(ratios) <= A.MARGIN, (what, ratios)


def _state(r, n=None):
    """Device (p, m, v) of regime dict ``r`` (its first n elements)."""
    z = np.zeros_like(r["p0"])
    return [_dev(x[:n]) for x in (r["p0"], z if r["m0"] is None else r["m0"], z if r["v0"] is None else r["v0"])]


def _grad_rows(r):
    """The gradients of ``r`` as rows of one device matrix whose row stride is a multiple of 4 floats (16-byte aligned rows)."""
    n = r["p0"].size
    g = np.zeros((len(r["grads"]), (n + 3) & ~3), dtype=F)
    for i, x in enumerate(r["grads"]):
        g[i, :n] = x
    return torch.from_numpy(g).to(DEV)


def _one_step(n, t, seed, steps=1):
    """A regime dict of ``steps`` steps from a non-trivial state at step count t - 1: p0 = 0 (p is the update), m0 ~ 0.1 N(0, 1),
    v0 = 0.01 U(0.25, 1), g ~ N(0, 1); G0 the smallest scale the state allows (adamw_ref.state_gmax)."""
    rng = np.random.default_rng([seed, n, t])
    m0 = (0.1 * rng.standard_normal(n)).astype(F)
    v0 = (0.01 * rng.uniform(0.25, 1.0, size=n)).astype(F)
    grads = tuple(rng.standard_normal(n).astype(F) for _ in range(steps))
    return dict(hp=dict(A.HP), p0=np.zeros(n, dtype=F), m0=m0, v0=v0, t0=t - 1, G0=A.state_gmax(m0, v0), grads=grads,
                checkpoints=tuple(range(t, t + steps)))


# ------------------------------------------------------------------------------------------------ 1. the flat kernel
@pytest.mark.parametrize("name", A.REGIMES)
def test_flat_kernel_against_float64(name):
    """segmm_adamw with a host step count over every regime of adamw_ref.regime (n = 4099, T = 300, compared at steps 1, 2, 3, 10,
    100, 300; ``late``: 20 steps from step 5000).  Elements whose gradient is always zero keep m = v = 0 exactly (adamw_ref.errors
    asserts it) and a p bit-equal to torch's."""
    H = _H()
    r, y = A.regime(name), A.yardstick(name)
    n, hp = r["p0"].size, r["hp"]
    p, m, v = _state(r)
    g = _grad_rows(r)
    worst = [0.0, 0.0, 0.0]
    for i in range(g.shape[0]):
        t = r["t0"] + i + 1
        H.adamw(p, g[i], m, v, n, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], t)
        if t in r["checkpoints"]:
            got = [x.cpu().numpy() for x in (p, m, v)]
            ratios = y.ratios(got, t)
            assert max(ratios) <= A.MARGIN, (name, t, ratios)
            worst = [max(a, b) for a, b in zip(worst, ratios)]
            assert np.array_equal(_bits(got[0][:A.ZEROS]), _bits(y.t32[t][0][:A.ZEROS])), (name, t)
    _report("flat " + name, worst)


# ------------------------------------------------------------------------------------------------ 2. sizes and neighbours
BIG = 4_194_304 + 4099          # more than 4096 blocks x 256 threads x 4 elements: the grid-stride loop makes a second lap


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, BIG])
def test_sizes_and_neighbours(n):
    """One step (t = 7) from a non-trivial state over n elements placed 96 floats into buffers with 32 guard floats checked on
    both sides, in p, g, m and v: the guards keep their bits.  Yardstick: torch's errors over a sample of max(n, 4099) elements of
    the same distribution, of which the kernel's n are the first -- the yardstick measures what fp32 does in the regime; the
    maximum over one to five elements would measure the luck of those elements instead."""
    H = _H()
    t = 7
    r = _one_step(max(n, A.N), t, 21)
    y = A.Yardstick(r)
    hp = r["hp"]
    rng = np.random.default_rng(5)
    size = OFF + ((n + 3) & ~3) + GUARD
    bufs, before = [], []
    for x in (r["p0"], r["grads"][0], r["m0"], r["v0"]):
        h = (1000.0 + 100.0 * rng.standard_normal(size)).astype(F)
        h[OFF:OFF + n] = x[:n]
        before.append(h)
        bufs.append(torch.from_numpy(h.copy()).to(DEV))
    p, g, m, v = bufs
    H.adamw(p, g, m, v, n, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], t, p_off=OFF)
    after = [x.cpu().numpy() for x in bufs]
    for name, a, b in zip("pgmv", after, before):
        assert np.array_equal(_bits(a[:OFF]), _bits(b[:OFF])) and np.array_equal(_bits(a[OFF + n:]), _bits(b[OFF + n:])), (n, name)
    assert np.array_equal(_bits(after[1]), _bits(before[1]))          # the gradient is read only
    _check("sizes n = %d" % n, y.ratios([after[i][OFF:OFF + n] for i in (0, 2, 3)], t, n=n))


# ------------------------------------------------------------------------------------------------ 3. non-finite and extreme gradients
SPECIAL = (np.inf, -np.inf, np.nan, 1e20, -1e20, 1e-30, -1e-30, 1e-38, -1e-38)
SPECIAL_AT = (65, 70, 75, 100, 101, 1022, 1025, 2050, 4098)          # inside float4 groups shared with ordinary elements; 4098: the tail


def test_non_finite_and_extreme_gradients():
    """3 steps over the ``unit`` regime's first gradients with nine elements' gradient replaced by inf, -inf, nan, +-1e20, +-1e-30,
    +-1e-38: the isnan / isinf / finite masks of p, m, v equal torch's (an inf gradient: p, m NaN from the second step and v inf;
    +-1e20: g^2 overflows fp32 but (1 - b2) g^2 = 1e37 does not, so v is finite and the element steps -- torch's addcmul order
    (1 - b2) g, then times g); every ordinary element is bit-equal to a run without the special ones; the +-1e-30 and +-1e-38
    elements (v = 0 in fp32, the update is lr m_hat / eps) match R_abi by the yardstick taken over those elements, with finite m
    and v >= 0.  Recorded, not asserted: whether the device keeps fp32 subnormals in m (m = 2.71e-39 after three steps of
    g = 1e-38; the test prints it).  hipcc's default kernel mode keeps them; a device that flushed them would give p = 0 there and
    fail the comparison with R_abi.  The comparison passes on an MI355X, so the device keeps them."""
    H = _H()
    base = A.regime("unit")
    hp, n, steps = base["hp"], base["p0"].size, 3
    grads = [np.array(g) for g in base["grads"][:steps]]
    special = [g.copy() for g in grads]
    for g in special:
        g[list(SPECIAL_AT)] = np.array(SPECIAL, dtype=F)
    r = dict(base, grads=tuple(special), checkpoints=(steps,))
    runs = []
    for gs in (special, grads):
        p, m, v = _state(base)
        for i, g in enumerate(gs):
            H.adamw(p, _dev(g), m, v, n, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], i + 1)
        runs.append([x.cpu().numpy() for x in (p, m, v)])
    got, plain = runs
    with np.errstate(all="ignore"):
        t32, r_abi, r_true = A.run(r, A.torch32)[steps], A.run(r, A.ref64, abi_rounded=True)[steps], A.run(r, A.ref64, abi_rounded=False)[steps]
    for name, a, b in zip("pmv", got, t32):
        for mask in (np.isnan, np.isinf, np.isfinite):
            assert np.array_equal(mask(a), mask(b)), (name, mask.__name__, a[list(SPECIAL_AT)], b[list(SPECIAL_AT)])
    ordinary = np.ones(n, dtype=bool)
    ordinary[list(SPECIAL_AT)] = False
    for name, a, b in zip("pmv", got, plain):
        assert np.array_equal(_bits(a[ordinary]), _bits(b[ordinary])), name
    for lo in (5, 7):          # the +-1e-30 pair, the +-1e-38 pair
        at = list(SPECIAL_AT[lo:lo + 2])
        e_k = float(np.max(np.abs(got[0][at].astype(np.float64) - r_abi[0][at])))
        e_t = float(np.max(np.abs(t32[0][at].astype(np.float64) - r_true[0][at])))
        print("RATIO tiny g = %g: E_p %.2f (kernel %.3e, torch %.3e)" % (SPECIAL[lo], e_k / e_t, e_k, e_t))
        assert e_k <= A.MARGIN * e_t, (SPECIAL[lo], e_k, e_t)
        assert np.isfinite(got[1][at]).all() and np.isfinite(got[2][at]).all() and (got[2][at] >= 0).all()
    print("subnormal m kept:", got[1][list(SPECIAL_AT[7:])], "float64:", r_abi[1][list(SPECIAL_AT[7:])])


# ------------------------------------------------------------------------------------------------ 4. the table kernels
@pytest.mark.parametrize("rows,width,n_ids", [(300, 4, 40), (200, 384, 30), (70_000, 64, 500), (300, 4, 0)])
def test_table_kernels_against_float64(rows, width, n_ids):
    """segmm_adamw_table, phase 0 then phase 1, for two steps (t = 7, 8) from a non-trivial state against the float64 dense update
    whose gradient is zero outside the listed rows.  width 384: the lane loop of adamw_table_rows_kernel iterates (96 float4 per
    row, 64 lanes); 70 000 x 64: 1 120 000 float4, past the 4096 x 256 threads of adamw_table_rest_kernel's capped grid.  The id
    list holds duplicates and ids outside the table; n_ids = 0: every row steps with g = 0 in phase 0 and phase 1 launches
    nothing.  The flags end at zero and the floats around the table keep their bits."""
    H = _H()
    n, t = rows * width, 7
    r = _one_step(n, t, 33, steps=2)
    rng = np.random.default_rng([rows, width])
    r["p0"] = (1e-3 * rng.standard_normal(n)).astype(F)
    hp = r["hp"]
    id_lists, grads = [], []
    for g in r["grads"]:
        ids = rng.integers(0, rows, size=n_ids)
        if n_ids:
            ids[:n_ids // 4] = ids[n_ids // 4:2 * (n_ids // 4)]          # duplicates
            ids = np.concatenate([ids[:n_ids // 2], [-1, rows, rows + 7, -2 ** 40], ids[n_ids // 2:]])          # ignored
        keep = np.zeros(rows, dtype=bool)
        keep[ids[(ids >= 0) & (ids < rows)]] = True
        g = np.where(np.repeat(keep, width), g, F(0.0))
        id_lists.append(torch.from_numpy(ids.astype(np.int64)).to(DEV))
        grads.append(g)
    r["grads"] = tuple(grads)
    y = A.Yardstick(r)
    size = OFF + n + GUARD
    bufs, before = [], []
    for x in (r["p0"], r["m0"], r["v0"]):
        h = (1000.0 + 100.0 * rng.standard_normal(size)).astype(F)
        h[OFF:OFF + n] = x
        before.append(h)
        bufs.append(torch.from_numpy(h.copy()).to(DEV))
    p, m, v = bufs
    flags = torch.zeros(rows, dtype=torch.int32, device=DEV)
    worst = [0.0, 0.0, 0.0]
    for i, (ids, g) in enumerate(zip(id_lists, grads)):
        gd = torch.zeros(size, device=DEV)
        gd[OFF:OFF + n] = _dev(g)
        args = (hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], t + i)
        H.adamw_table(p, None, m, v, OFF, rows, width, ids, flags, *args, 0)
        H.adamw_table(p, gd, m, v, OFF, rows, width, ids, flags, *args, 1)
        assert int(flags.abs().sum()) == 0
        after = [x.cpu().numpy() for x in bufs]
        ratios = y.ratios([a[OFF:OFF + n] for a in after], t + i)
        assert max(ratios) <= A.MARGIN, (rows, width, t + i, ratios)
        worst = [max(a, b) for a, b in zip(worst, ratios)]
    for name, a, b in zip("pmv", after, before):
        assert np.array_equal(_bits(a[:OFF]), _bits(b[:OFF])) and np.array_equal(_bits(a[OFF + n:]), _bits(b[OFF + n:])), name
    _report("table %d x %d, %d ids" % (rows, width, n_ids), worst)


# ------------------------------------------------------------------------------------------------ 5. the device step state
@pytest.fixture
def own_step_state():
    """A step state of the test's own, bound for the test.  The library has no getter for the binding, so what is restored is the
    library's default state (``step_bind(None)``): every trainer binds its own state again before it launches, and nothing is
    left pointing at this test's freed memory."""
    H = _H()
    state = torch.zeros((H.step_state_bytes() + 3) // 4, dtype=torch.int32, device=DEV)
    H.step_bind(state)
    try:
        yield state
    finally:
        torch.cuda.synchronize()
        H.step_bind(None)


STATE_STEPS = (0, 1, 2, 10, 1000, 10 ** 6)


def _ulp_close(got, want):
    return abs(float(got) - float(want)) <= float(np.spacing(F(want)))


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.95, 0.9999)])
def test_step_state_bias_corrections(own_step_state, betas):
    """step_set(seed, t) then step_get(): the step count, the seed, and the host formula float32(1 - double(float32(b))^t) and the
    float32 root of that double (test_adamw_cpu.py::test_host_bias_corrections) within one fp32 ulp; exactly (1, 1) at t = 0.
    step_set(t) followed by 7 step_advance calls gives the bits of step_set(t + 7)."""
    H = _H()
    b1, b2 = betas
    seed = 0x1234_5678_9ABC_DEF0 & (2 ** 63 - 1)
    for t in STATE_STEPS:
        H.step_set(seed, t, b1, b2)
        s, step, (bc1, bc2s) = H.step_get()
        assert (s, step) == (seed, t)
        if t == 0:
            assert (bc1, bc2s) == (1.0, 1.0)
            continue
        w1, w2 = A.host_bc(b1, t)[0], A.host_bc(b2, t)[1]
        print("t = %d: bc1 %r (host %r)  bc2_sqrt %r (host %r)" % (t, bc1, float(w1), bc2s, float(w2)))
        assert _ulp_close(bc1, w1) and _ulp_close(bc2s, w2), (t, bc1, float(w1), bc2s, float(w2))
    for t in (0, 1, 3, 1000):
        H.step_set(seed, t, b1, b2)
        for _ in range(7):
            H.step_advance(b1, b2)
        _, step, bc = H.step_get()
        H.step_set(seed, t + 7, b1, b2)
        _, step2, bc2 = H.step_get()
        assert step == step2 == t + 7 and bc == bc2, (t, bc, bc2)


def test_a_bound_step_state_outlives_its_owner():
    """The library holds the bare pointer of the bound state.  An owner that is dropped while its state is still bound (a trainer
    at the end of a test) must not hand the block back to the allocator: the next tensors of that size would take it, and a later
    caller's step_set / live dropout seed would write and read their data -- wrong dropout masks in whatever runs next with a live
    seed.  hipabi.step_bind keeps the tensor alive until something else is bound."""
    H = _H()
    n = (H.step_state_bytes() + 3) // 4
    seed = 0x0BAD_C0DE_F00D_FACE
    state = torch.zeros(n, dtype=torch.int32, device=DEV)
    ptr = state.data_ptr()
    H.step_bind(state)
    try:
        H.step_set(seed, 5)
        torch.cuda.synchronize()
        del state
        junk = [torch.full((n,), -1, dtype=torch.int32, device=DEV) for _ in range(8)]      # (a freed block of this size would be reused at once)
        assert all(j.data_ptr() != ptr for j in junk)
        torch.cuda.synchronize()
        got, step, _ = H.step_get()
        assert (got, step) == (seed, 5)
    finally:
        H.step_bind(None)
    assert H._STEP_BOUND is None


@pytest.mark.parametrize("t", [1, 2, 10, 1000])
def test_adamw_with_device_step_state(own_step_state, t):
    """segmm_adamw(step = -1) after step_set(t) against segmm_adamw(step = t): bit-identical whenever step_get returned the host's
    corrections bit for bit, and within the yardstick otherwise."""
    H = _H()
    r = _one_step(A.N, t, 44)
    y = A.Yardstick(r)
    hp, n = r["hp"], r["p0"].size
    g = _dev(r["grads"][0])
    H.step_set(3, t, hp["b1"], hp["b2"])
    _, _, bc = H.step_get()
    same = bc == (float(A.host_bc(hp["b1"], t)[0]), float(A.host_bc(hp["b2"], t)[1]))
    res = []
    for step in (-1, t):
        p, m, v = _state(r)
        H.adamw(p, g, m, v, n, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], step)
        res.append([x.cpu().numpy() for x in (p, m, v)])
    _check("device step state t = %d (corrections %s)" % (t, "equal" if same else "differ"), y.ratios(res[0], t))
    assert max(y.ratios(res[1], t)) <= A.MARGIN
    if same:
        for a, b in zip(*res):
            assert np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ 6. FusedAdamW over a horizon
HORIZON, HALF = 40, 20
TABLE = "backbone1.vid_proj.weight"


def _model(sd=None):
    cfg, g, nograd, _ = load_case("id_d32_N2")
    model = build_model(cfg)
    model.load_state_dict(g["sd"] if sd is None else sd)
    model = model.cuda()
    model.eval()
    return model, g, nograd


def _injected(shapes, step):
    """Seeded gradients of step ``step`` for every live parameter; on even steps the item table's gradient is zero outside the
    rows of ``ids`` (returned; None on odd steps)."""
    gen = torch.Generator().manual_seed(9000 + step)
    grads = {k: torch.randn(shape, generator=gen) for k, shape in shapes.items()}
    ids = None
    if step % 2 == 0:
        rows = shapes[TABLE][0]
        ids = torch.randint(0, rows, (12,), generator=gen)
        ids[:3] = ids[3:6]
        keep = torch.zeros(rows, dtype=torch.bool)
        keep[ids] = True
        grads[TABLE] = grads[TABLE] * keep[:, None]
    return grads, ids


def _fused_steps(model, opt, shapes, first, last):
    params = dict(model.named_parameters())
    for step in range(first, last + 1):
        grads, ids = _injected(shapes, step)
        if ids is not None:
            opt.table_early(TABLE, ids.to(DEV))
        for k, gr in grads.items():
            params[k].grad = gr.to(DEV)
        opt.step()
    return {k: params[k].detach().cpu().numpy().reshape(-1) for k in shapes}


def test_fused_adamw_over_a_horizon():
    """FusedAdamW on the smallest id-mode golden model for 40 steps of injected gradients (no forward or backward; on even steps
    the item table takes the two-pass update, table_early first) against torch.optim.AdamW on a CPU copy fed the same gradients:
    per parameter, E_p of the fused run against R_abi <= MARGIN x E_p of the torch run against R_true, at steps 20 and 40; dead
    parameters keep their bits.  The state_dict exported at step 20, loaded into a fresh torch.optim.AdamW (on a CPU copy of the
    step-20 parameters) and into a fresh FusedAdamW on a fresh model, continues to step 40 within the same bound."""
    from segmminterest_amd.trainer import FusedAdamW
    model, g, nograd = _model()
    lr, wd = 1e-3, 1e-4
    hp = dict(A.HP, lr=lr, wd=wd)
    opt = FusedAdamW(model, lr=lr, weight_decay=wd)
    st = opt._state()
    names = [k for k, _ in model.named_parameters()]
    shapes = {k: tuple(p.shape) for k, p in model.named_parameters() if k in st.live_names}
    dead = [k for k in names if k not in shapes]
    assert TABLE in shapes and dead and set(dead) <= set(nograd)
    start = {k: p.detach().cpu().clone() for k, p in model.named_parameters()}
    # torch on the CPU copy, and the two float64 recurrences, over the same gradients
    cpu = {k: torch.nn.Parameter(start[k].clone()) for k in names}
    topt = torch.optim.AdamW([cpu[k] for k in names], lr=lr, weight_decay=wd, foreach=False)
    all_grads = {k: [] for k in shapes}
    t32 = {}
    for step in range(1, HORIZON + 1):
        grads, _ = _injected(shapes, step)
        for k, gr in grads.items():
            cpu[k].grad = gr.clone()
            all_grads[k].append(gr.numpy().reshape(-1))
        topt.step()
        if step in (HALF, HORIZON):
            t32[step] = {k: cpu[k].detach().numpy().reshape(-1).copy() for k in shapes}
    ref = {k: [A.ref64(start[k].numpy().reshape(-1), all_grads[k], abi_rounded=a, checkpoints=(HALF, HORIZON), **hp) for a in (True, False)]
           for k in shapes}

    # a parameter of fewer than 32 elements (stage_mlp1.bias has one) is judged together with the rest of its module: the maximum
    # over one element is that element's luck on either side, not a yardstick (see test_sizes_and_neighbours)
    groups = {}
    for k, shape in shapes.items():
        small = int(np.prod(shape)) < 32
        groups[k] = [j for j in shapes if j.rsplit(".", 1)[0] == k.rsplit(".", 1)[0]] if small else [k]

    def check(what, got, step):
        worst = 0.0
        for k, members in groups.items():
            e_k = max(float(np.max(np.abs(got[j].astype(np.float64) - ref[j][0][step][0]))) for j in members)
            e_t = max(float(np.max(np.abs(t32[step][j].astype(np.float64) - ref[j][1][step][0]))) for j in members)
            assert e_k <= A.MARGIN * e_t, (what, step, k, e_k, e_t)
            worst = max(worst, e_k / e_t)
        print("RATIO %-44s E_p %5.2f" % ("%s, step %d" % (what, step), worst))

    check("FusedAdamW", _fused_steps(model, opt, shapes, 1, HALF), HALF)
    sd = opt.state_dict()
    sd_model = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    check("FusedAdamW", _fused_steps(model, opt, shapes, HALF + 1, HORIZON), HORIZON)
    for k, p in model.named_parameters():
        if k in dead:
            assert torch.equal(p.detach().cpu(), g["sd"][k]), k
    # the exported state under torch's optimizer
    cpu2 = {k: torch.nn.Parameter(sd_model[k].clone()) for k in names}
    topt2 = torch.optim.AdamW([cpu2[k] for k in names], lr=lr, weight_decay=wd, foreach=False)
    topt2.load_state_dict(copy.deepcopy(sd))          # torch keeps CPU tensors of a loaded state by reference and steps them in place
    for step in range(HALF + 1, HORIZON + 1):
        grads, _ = _injected(shapes, step)
        for k, gr in grads.items():
            cpu2[k].grad = gr.clone()
        topt2.step()
    check("torch.optim.AdamW resumed", {k: cpu2[k].detach().numpy().reshape(-1) for k in shapes}, HORIZON)
    # ... and under a fresh FusedAdamW
    model3, _, _ = _model(sd_model)
    opt3 = FusedAdamW(model3)
    opt3.load_state_dict(sd)
    assert opt3.step_count == HALF and (opt3.lr, opt3.wd) == (lr, wd)
    check("FusedAdamW resumed", _fused_steps(model3, opt3, shapes, HALF + 1, HORIZON), HORIZON)
