"""Learning-rate schedules in the device step state on the MI355X: the schedule the one-thread kernels evaluate against the float64
closed form (tests/lr_ref.py), the five AdamW kernel variants reading the rate from the state bit for bit as if it had been
passed, AdamW under a moving rate against float64 by the rule of tests/test_adamw_gpu.py, and the trainer: eager against recorded
steps, a rate that moves under a recording, constant schedule against none, resume from a checkpoint, reduce-on-plateau in fit, one
forced-collective rank.

Measured on an MI355X.  The device schedule: 0 of 40 advances differ from the host's fp32 value in each of the ten (kind, W)
cases -- the one-ulp allowance of test_device_schedule_against_float64 was not used; each case prints its count in a line that
starts with NONZERO (pytest -s).  AdamW under the device schedule, (error against R_abi) / (torch's error against R_true), printed
in lines that start with RATIO; the numpy-fp32 emulation of tests/test_lr_schedule_cpu.py gives the same figures except E_p 0.88
at step 1:

    step    E_p    E_m    E_v
    1      0.82   0.79   0.66
    2      0.85   1.06   0.79
    3      0.99   1.06   0.82
    10     0.91   1.01   0.53
    40     0.84   0.82   0.66

A ratio above adamw_ref.MARGIN = 3 is a finding to be explained from the arithmetic, not a margin to be raised.
"""
import copy
import multiprocessing as mp
import os
import sys

import numpy as np
import pytest
import torch

import adamw_ref as A
import lr_ref as L
from helpers import ROOT, build_model, load_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
OFF, GUARD = 96, 32          # the placement of tests/test_adamw_gpu.py: a range 96 floats into its buffers, 32 guard floats behind it
SEED = 0x1234_5678_9ABC_DEF0 & (2 ** 63 - 1)
HP = (A.HP["b1"], A.HP["b2"], A.HP["eps"], A.HP["wd"])


def _H():
    from segmminterest_amd import hipabi as H
    H.lib()
    return H


def _bits(x):
    return np.ascontiguousarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x).view(np.uint32)


@pytest.fixture
def own_step_state():
    """A zeroed step state of the test's own, bound for the test; the library's default state is bound again afterwards."""
    H = _H()
    state = torch.zeros((H.step_state_bytes() + 3) // 4, dtype=torch.int32, device=DEV)
    H.step_bind(state)
    try:
        yield state
    finally:
        torch.cuda.synchronize()
        H.step_bind(None)


# ------------------------------------------------------------------------------------------------ 1. the device schedule
ADVANCES = 40
NONZERO = {}          # test id -> advances (of 40) at which the device's rate was not the host's fp32 value


@pytest.mark.parametrize("W", [0, 5])
@pytest.mark.parametrize("kind", L.KINDS)
def test_device_schedule_against_float64(own_step_state, kind, W):
    """A fresh state, segmm_step_schedule (D = 30, eta_min 1e-5, gamma 0.97, step_size 7, start_factor 0.1), 40 advances through the
    hold region with segmm_step_get_lr after each: |lr_dev - fp32(lr_ref64_abi)| <= 1 fp32 ulp.  Expected 0; the ulp covers the
    device's double cos / pow differing from libm in the last bit next to an fp32 rounding boundary.  The count of non-zero
    differences is printed (NONZERO lines).  The installed schedule shows the rate of step 1 before any advance; step_set(seed, t)
    gives lr_t again and leaves the descriptor alone; step_set_base_lr rescales and the next advance continues from the new base."""
    H = _H()
    kw = dict(kind=kind, base_lr=1e-3, warmup_steps=W, start_factor=0.1, decay_steps=30, eta_min=1e-5, gamma=0.97, step_size=7)
    want = [F(L.lr_at(k, abi_rounded=True, **kw)) for k in range(ADVANCES + 2)]
    assert H.step_get_lr() == (0.0, 0.0)          # all zero: no schedule
    H.step_set(SEED, 0, *HP[:2])
    H.step_schedule(**kw)
    lr, base = H.step_get_lr()
    assert (F(lr), F(base)) == (want[0], F(1e-3))
    nonzero = []
    for t in range(1, ADVANCES + 1):
        H.step_advance(*HP[:2])
        lr = F(H.step_get_lr()[0])
        if lr != want[t - 1]:
            nonzero.append((t, float(lr), float(want[t - 1])))
        assert abs(float(lr) - float(want[t - 1])) <= float(np.spacing(want[t - 1])), (t, lr, want[t - 1])
    NONZERO["%s-W%d" % (kind, W)] = nonzero
    print("NONZERO %s W=%d: %d of %d advances %s" % (kind, W, len(nonzero), ADVANCES, nonzero))
    _, step, bc40 = H.step_get()
    assert step == ADVANCES
    for t in (1, 3, 17, ADVANCES, 0):
        H.step_set(SEED, t, *HP[:2])
        lr, base = H.step_get_lr()
        assert abs(lr - float(want[max(t - 1, 0)])) <= float(np.spacing(want[max(t - 1, 0)])) and F(base) == F(1e-3), (t, lr)
    H.step_set(SEED, ADVANCES, *HP[:2])
    assert H.step_get()[2] == bc40          # the bias corrections are what they were
    # a new base rate: the current step's rate at once, the following steps' from the advance
    H.step_set(SEED, 7, *HP[:2])
    half = dict(kw, base_lr=5e-4)
    H.step_set_base_lr(5e-4)
    for t in (7, 8, 9):
        lr, base = H.step_get_lr()
        w = F(L.lr_at(t - 1, abi_rounded=True, **half))
        assert abs(lr - float(w)) <= float(np.spacing(w)) and F(base) == F(5e-4), (t, lr, w)
        H.step_advance(*HP[:2])


# ------------------------------------------------------------------------------------------------ 2. the kernels use it bit for bit
COSINE = dict(kind="cosine", base_lr=1e-3, warmup_steps=5, start_factor=0.1, decay_steps=30, eta_min=1e-5)
ROWS, WIDTH = 37, 8


def _placed(rng, n, values=None, scale=1.0):
    """A host buffer of OFF + n (rounded up to 4) + GUARD floats around 1000 with ``values`` (default N(0, scale)) at OFF."""
    h = (1000.0 + 100.0 * rng.standard_normal(OFF + ((n + 3) & ~3) + GUARD)).astype(F)
    h[OFF:OFF + n] = (scale * rng.standard_normal(n)).astype(F) if values is None else values
    return h


@pytest.mark.parametrize("t", [2, 18, 40], ids=["warmup", "decay", "held"])
def test_kernels_read_the_state_rate_bit_for_bit(own_step_state, t):
    """At step t of a cosine schedule (W = 5, D = 30: t = 2 in the warm-up, 18 mid-decay, 40 held at eta_min) each of segmm_adamw,
    segmm_adamw_scaled, segmm_adamw_table phase 0, phase 1 and segmm_adamw_table_scaled runs twice on identical copies, step = -1
    in both: once with the sentinel lr = -1, once with the fp32 rate just read back from the state passed by value.  n = 4099 (the
    n & 3 tail) and a 37 x 8 table with duplicate and out-of-range ids, both 96 floats into buffers with 32 guard floats behind:
    p, m, v, the flags and everything around the range are bitwise equal after every launch, and the update is not a no-op."""
    H = _H()
    H.step_set(SEED, t, *HP[:2])
    H.step_schedule(**COSINE)
    lr_t = H.step_get_lr()[0]
    assert abs(lr_t - float(F(L.lr_at(t - 1, abi_rounded=True, **COSINE)))) <= float(np.spacing(F(lr_t))) and lr_t > 0
    rng = np.random.default_rng([7, t])
    coef = torch.tensor([0.37], dtype=torch.float32, device=DEV)

    def same(a, b, what):
        for name, x, y in zip(("p", "m", "v", "flags"), a, b):
            assert np.array_equal(_bits(x), _bits(y)), (what, name)

    # the flat kernel, unscaled and scaled
    n = A.N
    host = [_placed(rng, n), _placed(rng, n), _placed(rng, n, scale=0.1), _placed(rng, n, values=(0.01 * rng.uniform(0.25, 1.0, n)).astype(F))]
    for c in (None, coef):
        runs = []
        for lr in (H.LIVE_LR, lr_t):
            p, g, m, v = (torch.from_numpy(h.copy()).to(DEV) for h in host)
            H.adamw(p, g, m, v, n, lr, *HP, -1, p_off=OFF, coef=c)
            runs.append((p, m, v))
        same(runs[0], runs[1], "flat scaled" if c is not None else "flat")
        for x, h in zip(runs[0], (host[0], host[2], host[3])):
            got = x.cpu().numpy()
            assert np.array_equal(_bits(got[:OFF]), _bits(h[:OFF])) and np.array_equal(_bits(got[OFF + n:]), _bits(h[OFF + n:]))
        assert not np.array_equal(_bits(runs[0][0]), _bits(host[0]))
    # the table kernels: phase 0, then phase 1 unscaled / scaled
    nt = ROWS * WIDTH
    ids = rng.integers(0, ROWS, size=12)
    ids[:3] = ids[3:6]                                                        # duplicates
    ids = np.concatenate([ids[:6], [-1, ROWS, ROWS + 7, -2 ** 40], ids[6:]])          # ignored
    ids = torch.from_numpy(ids.astype(np.int64)).to(DEV)
    host = [_placed(rng, nt, scale=1e-3), _placed(rng, nt), _placed(rng, nt, scale=0.1),
            _placed(rng, nt, values=(0.01 * rng.uniform(0.25, 1.0, nt)).astype(F))]
    for c in (None, coef):
        runs = []
        for lr in (H.LIVE_LR, lr_t):
            p, g, m, v = (torch.from_numpy(h.copy()).to(DEV) for h in host)
            flags = torch.zeros(ROWS, dtype=torch.int32, device=DEV)
            H.adamw_table(p, None, m, v, OFF, ROWS, WIDTH, ids, flags, lr, *HP, -1, 0)
            after0 = tuple(x.clone() for x in (p, m, v, flags))
            H.adamw_table(p, g, m, v, OFF, ROWS, WIDTH, ids, flags, lr, *HP, -1, 1, coef=c)
            runs.append((after0, (p, m, v, flags)))
        same(runs[0][0], runs[1][0], "table phase 0")
        same(runs[0][1], runs[1][1], "table phase 1 scaled" if c is not None else "table phase 1")
        assert int(runs[0][0][3].sum()) > 0 and int(runs[0][1][3].abs().sum()) == 0          # rows were marked, then claimed
        for x, h in zip(runs[0][1], (host[0], host[2], host[3])):
            got = x.cpu().numpy()
            assert np.array_equal(_bits(got[:OFF]), _bits(h[:OFF])) and np.array_equal(_bits(got[OFF + nt:]), _bits(h[OFF + nt:]))
            assert not np.array_equal(_bits(got[OFF:OFF + nt]), _bits(h[OFF:OFF + nt]))


def test_sentinel_without_a_schedule_is_a_zero_rate(own_step_state):
    """A state without a schedule holds lr = 0: the sentinel then gives the step of lr = 0 passed by value (moments move, the
    parameter does not), never a step at a negative rate."""
    H = _H()
    H.step_set(SEED, 3, *HP[:2])
    rng = np.random.default_rng(11)
    host = [rng.standard_normal(64).astype(F) for _ in range(3)] + [rng.uniform(0.1, 1.0, 64).astype(F)]
    runs = []
    for lr in (H.LIVE_LR, 0.0):
        p, g, m, v = (torch.from_numpy(h.copy()).to(DEV) for h in host)
        H.adamw(p, g, m, v, 64, lr, *HP, -1)
        runs.append((p, m, v))
    for x, y in zip(*runs):
        assert np.array_equal(_bits(x), _bits(y))
    assert np.array_equal(_bits(runs[0][0]), _bits(host[0])) and not np.array_equal(_bits(runs[0][1]), _bits(host[2]))


# ------------------------------------------------------------------------------------------------ 3. against float64
def test_adamw_under_the_device_schedule_against_float64(own_step_state):
    """Regime ``unit`` (N = 4099) for 40 steps, every step segmm_step_advance then segmm_adamw(lr = -1, step = -1) under the cosine
    schedule with W = 5, D = 30 (lr_ref.MOVING): E_p, E_m, E_v against R_abi over torch's own errors against R_true (torch.optim.AdamW
    + torch's scheduler, held at the end of its decay) <= adamw_ref.MARGIN at steps 1, 2, 3, 10, 40 (RATIO lines)."""
    H = _H()
    y = L.moving_yardstick()
    r = A.regime("unit")
    n = r["p0"].size
    p, m, v = (torch.zeros(n, device=DEV) for _ in range(3))
    g = np.zeros((L.MOVING_STEPS, (n + 3) & ~3), dtype=F)
    for i in range(L.MOVING_STEPS):
        g[i, :n] = r["grads"][i]
    g = torch.from_numpy(g).to(DEV)
    H.step_set(SEED, 0, *HP[:2])
    H.step_schedule(**L.MOVING)
    worst = [0.0, 0.0, 0.0]
    for t in range(1, L.MOVING_STEPS + 1):
        H.step_advance(*HP[:2])
        H.adamw(p, g[t - 1], m, v, n, H.LIVE_LR, *HP, -1)
        if t in L.MOVING_CHECKPOINTS:
            ratios = y.ratios([x.cpu().numpy() for x in (p, m, v)], t)
            print("RATIO %-44s E_p %5.2f  E_m %5.2f  E_v %5.2f" % (("device schedule, step %d" % t,) + ratios))
            assert max(ratios) <= A.MARGIN, (t, ratios)
            worst = [max(a, b) for a, b in zip(worst, ratios)]
    print("RATIO %-44s E_p %5.2f  E_m %5.2f  E_v %5.2f" % (("device schedule, worst",) + tuple(worst)))


# ------------------------------------------------------------------------------------------------ 4 - 7. the trainer
LR = 1e-3
SCHED = dict(kind="cosine", warmup_steps=3, start_factor=0.1, decay_steps=8, eta_min=1e-5)


def _cfg(name="img_d32_N2", S=20):
    cfg, _, _, _ = load_case(name)
    return dict(cfg, S=S, exposure_prob=list(cfg["exposure_prob"])[:S])


def _batches(cfg, n=3, B=8):
    from segmminterest_amd.synth import make_batch
    return [{k: v.to(DEV) for k, v in make_batch(B, cfg["S"], cfg["Lt"], cfg["D_in"], n_users=cfg.get("n_users", 5) or 5,
                                                 n_items=cfg.get("n_items", 5) or 5, seed=400 + i).items()} for i in range(n)]


def _trainer(cfg, **kw):
    from segmminterest_amd.trainer import Trainer
    torch.manual_seed(5)
    model = build_model(cfg).to(DEV)
    return Trainer(model, lr=LR, dropout=False, device_state=True, **kw)


def _snap(tr):
    torch.cuda.synchronize()
    return tuple(x.detach().clone() for x in (tr.model._store.flat, tr.opt.m, tr.opt.v))


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _steps(tr, batches, first, last, recorded_from=None, between=None):
    """Steps first .. last on batches[(t - 1) % 3]; from step ``recorded_from`` on: record() (that step), then run_recorded.
    ``between`` = (t, fn): fn(tr) runs before step t."""
    for t in range(first, last + 1):
        b = batches[(t - 1) % len(batches)]
        if between is not None and between[0] == t:
            between[1](tr)
        if recorded_from is None or t < recorded_from:
            tr.train_step(b)
        elif t == recorded_from:
            tr.record(b, prev_batch=batches[(t - 2) % len(batches)])
        else:
            tr.run_recorded(b)


def test_trainer_eager_equals_recorded_under_a_schedule():
    """The tiny image model (d = 32, N = 2, S = 20, B = 8, dropout 0) under a cosine schedule with W = 3, D = 8: 12 train_steps
    against 4 eager steps + record() + 7 run_recorded() on the same batches -- parameters and both moments bitwise equal; the
    state's rate after step 12 is the reference's (held at eta_min: every operation behind it is exact or correctly rounded);
    current_lr() follows without a sync; and the recording holds as many commands as that of a trainer without a schedule."""
    cfg = _cfg()
    batches = _batches(cfg)
    eager = _trainer(cfg, lr_schedule=SCHED)
    seen = []
    for t in range(1, 13):
        seen.append(eager.opt.current_lr())
        eager.train_step(batches[(t - 1) % 3])
    want = [float(F(L.lr_at(k, base_lr=LR, abi_rounded=True, **SCHED))) for k in range(13)]
    assert seen == want[:12] and eager.opt.current_lr() == want[12]
    rec = _trainer(cfg, lr_schedule=SCHED)
    _steps(rec, batches, 1, 12, recorded_from=5)
    assert _equal(_snap(eager), _snap(rec))
    assert eager.opt.device_lr() == rec.opt.device_lr() == want[11]
    assert want[11] == want[12] and len(set(want[:11])) == 11          # the schedule moved on every step before the hold
    plain = _trainer(cfg)
    _steps(plain, batches, 1, 5, recorded_from=5)
    assert rec._recorded["n_cmds"] == plain._recorded["n_cmds"]          # no launch was added


def test_rate_moves_under_a_recording():
    """Constant schedule: record(), set_base_lr(lr / 2), run_recorded() -- no exception, and bitwise the eager trainer given the
    same call at the same point.  A trainer without a schedule still refuses a changed rate after record()."""
    cfg = _cfg()
    batches = _batches(cfg)
    halve = (6, lambda tr: tr.opt.set_base_lr(LR / 2))
    rec = _trainer(cfg, lr_schedule="constant")
    _steps(rec, batches, 1, 8, recorded_from=5, between=halve)
    eager = _trainer(cfg, lr_schedule="constant")
    _steps(eager, batches, 1, 8, between=halve)
    assert _equal(_snap(eager), _snap(rec))
    assert rec.opt.lr == LR / 2 and rec.opt.device_lr() == float(F(LR / 2)) == rec.opt.current_lr()
    stay = _trainer(cfg, lr_schedule="constant")
    _steps(stay, batches, 1, 8)
    assert not _equal(_snap(stay), _snap(eager))          # the halved rate was used
    plain = _trainer(cfg)
    _steps(plain, batches, 1, 5, recorded_from=5)
    plain.opt.lr = LR / 2
    with pytest.raises(RuntimeError, match="record\\(\\) again"):
        plain.run_recorded(batches[2])
    with pytest.raises(RuntimeError, match="needs an lr_schedule"):
        plain.opt.set_base_lr(LR / 2)


def test_constant_schedule_equals_no_schedule():
    """6 steps with lr_schedule="constant" (the kernels read the rate from the state) and without (it travels by value):
    bitwise equal parameters and moments."""
    cfg = _cfg()
    batches = _batches(cfg)
    a, b = _trainer(cfg, lr_schedule="constant"), _trainer(cfg)
    _steps(a, batches, 1, 6)
    _steps(b, batches, 1, 6)
    assert _equal(_snap(a), _snap(b))
    assert a.opt.state_dict()["param_groups"][0]["lr"] == float(F(LR)) and "segmm_lr_schedule" not in b.opt.state_dict()["param_groups"][0]


def test_resume_under_a_schedule():
    """6 steps, the model's and the optimizer's state_dict() into a fresh trainer (built with another rate and schedule), 6 more
    steps: bitwise the parameters and moments of 12 uninterrupted steps.  The saved dict carries the coming step's rate as "lr",
    the base rate as "initial_lr" and the descriptor, and loads into torch.optim.AdamW."""
    from segmminterest_amd.trainer import LRSchedule
    cfg = _cfg()
    batches = _batches(cfg)
    whole = _trainer(cfg, lr_schedule=SCHED)
    _steps(whole, batches, 1, 12)
    first = _trainer(cfg, lr_schedule=SCHED)
    _steps(first, batches, 1, 6)
    torch.cuda.synchronize()
    sd_model = {k: v.detach().cpu().clone() for k, v in first.model.state_dict().items()}
    sd_opt = first.opt.state_dict()
    group = sd_opt["param_groups"][0]
    assert group["lr"] == float(F(L.lr_at(6, base_lr=LR, abi_rounded=True, **SCHED))) and group["initial_lr"] == LR
    assert LRSchedule(**group["segmm_lr_schedule"]) == first.opt.schedule
    topt = torch.optim.AdamW(list(first.model.parameters()), lr=0.5)
    topt.load_state_dict(copy.deepcopy(sd_opt))
    assert topt.param_groups[0]["lr"] == group["lr"] and topt.param_groups[0]["segmm_lr_schedule"] == group["segmm_lr_schedule"]
    second = _trainer(cfg, lr_schedule="constant")
    second.opt.lr = 0.5
    second.model.load_state_dict(sd_model)
    second.opt.load_state_dict(sd_opt)
    assert second.opt.step_count == 6 and second.opt.lr == LR and second.opt.schedule == first.opt.schedule
    assert second.opt.device_lr() == first.opt.device_lr()          # the rate of step 6, the state's current step on both
    _steps(second, batches, 7, 12)
    assert _equal(_snap(whole), _snap(second))
    assert second.opt.device_lr() == whole.opt.device_lr()


def test_fit_reduces_on_plateau_under_recorded_steps():
    """fit(recorded=True, lr_plateau=...) on the tiny model, 12 steps with a validation every 2 and patience 0: the base rate ends
    where a PlateauLR fed the recorded history of the monitored metric ends (the validation before training is not fed), the
    device holds it, and no replayed step refused the moved rate."""
    from segmminterest_amd.trainer import PlateauLR
    cfg = _cfg()
    batches = _batches(cfg)
    tr = _trainer(cfg, lr_schedule="constant")
    kw = dict(factor=0.5, patience=0, min_lr=LR / 4)
    hist = tr.fit([batches[i % 3] for i in range(12)], batches[:1], epochs=1, valid_step=2, recorded=True, eager_steps=2, lr_plateau=kw)
    assert hist["global_step"] == 12 and len(hist["NDCG@5"]) == 7 and tr.__dict__.get("_recorded") is not None

    class Opt:
        lr = LR

        def set_base_lr(self, lr):
            self.lr = lr
    ref = PlateauLR(Opt(), mode="max", **kw)
    for x in hist["NDCG@5"][1:]:
        ref.step(x)
    print("monitored metric:", hist["NDCG@5"], "base rate:", tr.opt.lr)
    assert tr.opt.lr == ref.opt.lr and tr.opt.device_lr() == float(F(tr.opt.lr))


# ------------------------------------------------------------------------------------------------ 8. one forced-collective rank
def _run_rank(port, name, force, q):
    """One process on cuda:0: 4 eager steps + record() + 7 run_recorded() under the cosine schedule.  force: a one-rank RCCL
    process group with SEGMM_DP_FORCE=1, so every collective of the data-parallel step is really issued."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", SEGMM_DP_FORCE="1" if force else "0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from segmminterest_amd.trainer import DPComm
    torch.cuda.set_device(0)
    if force:
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        cfg = _cfg(name, S=40 if name.startswith("id") else 20)
        # (id mode: the dense all-reduce of the table gradients -- a SUM over one rank is the identity; the sparse row exchange
        # sums the same rows in another order)
        tr = _trainer(cfg, lr_schedule=SCHED, comm=DPComm(), sparse_tables=False)
        assert tr.comm.active == bool(force)
        _steps(tr, _batches(cfg), 1, 12, recorded_from=5)
        early = bool(tr.opt.__dict__.get("_table_flags"))
        q.put(tuple(x.cpu().numpy() for x in _snap(tr)) + (tr.opt.device_lr(), early))
    finally:
        if force:
            dist.destroy_process_group()


@pytest.mark.parametrize("name", ["img_d32_N2", "id_d32_N2"])
def test_forced_collective_rank_equals_single_process(name):
    """A single rank whose collectives are forced through RCCL against the plain single-process run, both 4 eager + record + 7
    replayed steps under the cosine schedule: parameters, moments and the state's rate bitwise equal.  In id mode the plain run
    updates the item table in two passes (table_early at the head of the step, on its own stream, reading the same step's rate)
    and the forced rank in one dense launch after its all-reduce."""
    ctx = mp.get_context("spawn")
    res = {}
    for force in (0, 1):
        q = ctx.Queue()
        p = ctx.Process(target=_run_rank, args=(29350 + os.getpid() % 200 + force + (7 if name.startswith("id") else 0), name, force, q))
        p.start()
        res[force] = q.get(timeout=300)
        p.join(timeout=60)
        assert p.exitcode == 0
    for a, b in zip(res[0][:3], res[1][:3]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert res[0][3] == res[1][3] == float(F(L.lr_at(11, base_lr=LR, abi_rounded=True, **SCHED)))
    assert res[0][4] == name.startswith("id") and not res[1][4]          # the two-pass table update ran in the plain id-mode run only
