"""Trainer(micro_batch=m): one optimizer step on a batch taken in micro-batches, with the gradient of the WHOLE batch's loss.

The yardstick is the unchanged plain step on the same rows; the tolerances are the project's own for partial-batch sums against the
whole batch (tests/test_dp_gpu.py: flat gradient 1e-4 max|g|, first loss 1e-5, second loss 3e-4, parameters rtol 1e-4 / atol
4.5e-3 after two AdamW steps), loss slots 1e-5 relative (floor: four fp32 roundings of the largest slot), logits the fixtures' 1e-4 absolute.  Where the arithmetic is the same
by construction (degenerate settings, two runs, eager against recorded, the add kernel against torch.add) equality is bitwise."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import lr_ref as L
from helpers import ROOT, build_model, load_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32


def _H():
    from segmminterest_amd import hipabi as H
    H.lib()
    return H


def _fully_watched(label):
    return (label == 0).sum(1) == 0          # no leave segment: every segment of the video is 1


def _batch(cfg, B=16, dev=DEV):
    """synth.make_batch(B, seed=21), rows stable-sorted so that the fully watched rows come first."""
    from segmminterest_amd.synth import make_batch
    b = make_batch(B, cfg["S"], cfg["Lt"], cfg["D_in"], n_users=cfg.get("n_users", 5) or 5, n_items=cfg.get("n_items", 5) or 5, seed=21)
    order = torch.sort((~_fully_watched(b["label"])).to(torch.int64), stable=True).indices
    b = {k: v[order].contiguous() for k, v in b.items()}
    return b if dev is None else {k: v.to(dev) for k, v in b.items()}


def _clone(batch):
    return {k: v.clone() for k, v in batch.items()}


def _trainer(name, **kw):
    from segmminterest_amd.trainer import Trainer
    cfg, g, _, _ = load_case(name)
    torch.manual_seed(5)
    model = build_model(cfg)
    model.load_state_dict(g["sd"])
    kw.setdefault("dropout", False)
    return Trainer(model.to(DEV), **kw)


def _two_steps(tr, batch, detached=False):
    """-> (loss-slot dicts of the two steps, logits of step 1, flat gradient of step 1, parameters after step 2)"""
    st = tr.model._store
    outs, logits, g1 = [], None, None
    for i in range(2):
        out = tr.train_step(_clone(batch))
        outs.append({k: float(v.detach()) for k, v in out.items() if k not in ("logits", "gt")})
        if i == 0:
            logits, g1 = out["logits"].detach().clone(), st.gflat.detach().clone()
            if detached:          # the micro-batched step's outputs: sums and copies written by launches, nothing of autograd's
                assert not any(v.requires_grad for v in out.values()) and out["gt"].shape[0] == out["logits"].shape[0]
    torch.cuda.synchronize()
    return outs, logits, g1, st.flat.detach().clone()


def _close(a, b, tol):
    return abs(a - b) <= tol * max(1.0, abs(a))


def _check_against_plain(got, want, B, S):
    (o, lg, g, p), (o0, lg0, g0, p0) = got, want
    n = min(g.numel(), g0.numel())
    err, top = float((g[:n] - g0[:n]).abs().max()), float(g0.abs().max())
    print("grad err %.3g of max|g| %.3g; loss %r vs %r" % (err, top, [x["loss"] for x in o], [x["loss"] for x in o0]))
    assert err <= 1e-4 * top, "summed micro-batch gradients != whole-batch gradient"
    assert list(o[0]) == list(o0[0])          # today's keys, today's order
    assert _close(o0[0]["loss"], o[0]["loss"], 1e-5), (o0[0], o[0])
    # every slot 1e-5 RELATIVE.  interestKL and hazard are differences of sums, so their rounding error follows the size of the terms,
    # not of the value: an absolute floor of 4 fp32 roundings (2^-22) of the step's largest slot
    floor = 2.0 ** -22 * max(abs(v) for v in o0[0].values())
    for k in o0[0]:
        print("  %-12s plain %.9g micro-batched %.9g" % (k, o0[0][k], o[0][k]))
        assert abs(o0[0][k] - o[0][k]) <= 1e-5 * abs(o0[0][k]) + floor, (k, o0[0][k], o[0][k])
    assert _close(o0[1]["loss"], o[1]["loss"], 3e-4), (o0[1], o[1])
    assert tuple(lg.shape) == (B, S) and float((lg - lg0).abs().max()) < 1e-4
    assert torch.allclose(p, p0, rtol=1e-4, atol=4.5e-3)


_PLAIN = {}


def _plain(name, B=16):
    """The plain trainer's two steps on the sorted batch: computed once, shared, left unchanged."""
    if (name, B) not in _PLAIN:
        cfg, _, _, _ = load_case(name)
        batch = _batch(cfg, B)
        if name == "id_d32_N2" and B == 16:
            batch["photo_identity_id"][0] = batch["photo_identity_id"][15]
        _PLAIN[(name, B)] = (cfg, batch, _two_steps(_trainer(name), batch))
    return _PLAIN[(name, B)]


# ------------------------------------------------------------------------------------------------ 1, 2: equivalence
@pytest.mark.parametrize("name", ["img_d32_N3_alllosses", "id_d32_N2", "both_fh2"])
def test_micro_batched_step_is_the_whole_batch_step(name):
    """16 rows in micro-batches of 4 against the plain step on the 16 rows, two steps from the same state.  Six of the 16 rows are
    fully watched and sorted to the front, so the micro-batches differ in composition: per-micro-batch normalisers (the BPR mean,
    the Σ/B losses, the mse double sums) would not give the batch's loss.  id_d32_N2: one item id occurs in micro-batches 0 and 3,
    so a scatter that overwrites, or a clear between micro-batches, loses a row gradient."""
    cfg, batch, want = _plain(name)
    assert int(_fully_watched(batch["label"]).sum()) == 6 and bool(_fully_watched(batch["label"])[:6].all())
    if name == "id_d32_N2":
        ids = batch["photo_identity_id"]
        assert int(ids[0]) == int(ids[15])
    tr = _trainer(name, micro_batch=4)
    got = _two_steps(tr, batch, detached=True)
    _check_against_plain(got, want, 16, cfg["S"])
    assert tr.opt.step_count == 2


def test_ragged_last_micro_batch():
    """B = 10, m = 4: micro-batches of 4, 4 and 2 rows."""
    cfg, batch, want = _plain("img_d32_N3_alllosses", 10)
    got = _two_steps(_trainer("img_d32_N3_alllosses", micro_batch=4), batch)
    _check_against_plain(got, want, 10, cfg["S"])


# ------------------------------------------------------------------------------------------------ 3: degenerate settings
@pytest.mark.parametrize("m", [16, 64])
def test_micro_batch_not_below_the_batch_is_the_plain_step(m):
    cfg, batch, (o0, lg0, g0, p0) = _plain("img_d32_N3_alllosses")
    o, lg, g, p = _two_steps(_trainer("img_d32_N3_alllosses", micro_batch=m), batch)
    assert o == o0 and torch.equal(lg, lg0) and torch.equal(g, g0) and torch.equal(p, p0)


def test_no_prefetch_of_a_batch_that_will_be_micro_batched():
    """A short batch takes the plain step; the input stage of a next batch the trainer will take in slices is not prefetched (the
    micro-batched step could not use it, and its buffers would be those of all 16 rows); a short next batch is, as ever."""
    cfg, batch, _ = _plain("img_d32_N3_alllosses")
    tr = _trainer("img_d32_N3_alllosses", micro_batch=4)
    b4, c4 = ({k: v[r:r + 4].clone() for k, v in batch.items()} for r in (0, 4))
    tr.train_step(b4, next_batch=batch)
    assert tr._pf is None
    tr.train_step(b4, next_batch=c4)
    assert tr._pf is not None and tr._pf["batch"] is c4


def test_parameter_hooks_are_refused_by_name():
    cfg, batch, _ = _plain("img_d32_N3_alllosses")
    tr = _trainer("img_d32_N3_alllosses", micro_batch=4)
    next(tr.model.parameters()).register_hook(lambda g: g)
    with pytest.raises(RuntimeError, match="micro_batch.*parameter hooks"):
        tr.train_step(_clone(batch))


def test_too_many_micro_batches_for_the_header_arena_are_refused_and_leave_the_step_state(monkeypatch):
    """device_state: every pass draws its site headers from the step's arena.  With the arena one row short of what k = 4 passes
    draw, the step is refused by name after pass 0 -- and the device step count, advanced at the head of the failed step, is put
    back: the same trainer then takes a k = 2 step (which fits) bitwise like a trainer that never failed."""
    from segmminterest_amd.engine import ParamStore
    H = _H()
    cfg, batch, _ = _plain("img_d32_N3_alllosses")
    probe = _trainer("img_d32_N3_alllosses", micro_batch=4, device_state=True)
    probe.train_step(_clone(batch))
    used = probe.model._store._arena_used          # rows the four passes of a first step draw
    assert 0 < used < ParamStore.HDR_RING_ROWS
    monkeypatch.setattr(ParamStore, "HDR_RING_ROWS", used - 1)
    tr = _trainer("img_d32_N3_alllosses", micro_batch=4, device_state=True)
    with pytest.raises(RuntimeError, match=r"micro_batch=4.*site headers.*%d rows" % (used - 1)):
        tr.train_step(_clone(batch))
    H.step_bind(tr._step_state)
    assert tr.opt.step_count == 0 and H.step_get()[1] == 0
    ref = _trainer("img_d32_N3_alllosses", micro_batch=8, device_state=True)
    tr.micro_batch = 8          # two passes: half the rows, they fit
    outs = [t.train_step(_clone(batch)) for t in (tr, ref)]
    torch.cuda.synchronize()
    assert float(outs[0]["loss"]) == float(outs[1]["loss"])
    assert torch.equal(tr.model._store.flat, ref.model._store.flat) and torch.equal(tr.opt.m, ref.opt.m) and torch.equal(tr.opt.v, ref.opt.v)
    for t in (tr, ref):
        H.step_bind(t._step_state)
        assert t.opt.step_count == 1 and H.step_get()[1] == 1


# ------------------------------------------------------------------------------------------------ 4: reproducibility, recording
def test_two_runs_are_bitwise_equal():
    cfg, batch, _ = _plain("img_d32_N3_alllosses")
    runs = []
    for _ in range(2):
        torch.manual_seed(77)
        runs.append(_two_steps(_trainer("img_d32_N3_alllosses", micro_batch=4, dropout=True), batch))
    (o, lg, g, p), (o2, lg2, g2, p2) = runs
    assert o == o2 and torch.equal(g, g2) and torch.equal(p, p2) and torch.equal(lg, lg2)


def _rotating(batch):
    return [batch] + [{k: v.roll(3 * i, 0).contiguous() for k, v in batch.items()} for i in (1, 2)]


@pytest.mark.parametrize("name", ["img_d32_N3_alllosses", "id_d32_N2"])
def test_recorded_micro_batched_steps_equal_eager_bitwise(name):
    """device_state: five eager micro-batched steps against two eager + record() + two run_recorded() on the same rotating
    batches, dropout on: parameters, both moments, every step's loss bitwise equal; the recording is k passes long but ONE optimizer
    step -- opt.step_count and the device step count advance by one per step."""
    H = _H()
    cfg, batch, _ = _plain(name)
    batches = _rotating(batch)
    res = []
    for recorded in (False, True):
        torch.manual_seed(11)
        tr = _trainer(name, micro_batch=4, dropout=True, device_state=True)
        losses = []
        for t in range(5):
            b = _clone(batches[t % 3])
            if not recorded or t < 2:
                out = tr.train_step(b)
            elif t == 2:
                out = tr.record(b, prev_batch=prev)
            else:
                out = tr.run_recorded(b)
            prev = b
            losses.append(float(out["loss"]))
            assert tuple(out["logits"].shape) == (16, cfg["S"])
            H.step_bind(tr._step_state)
            assert tr.opt.step_count == t + 1 and H.step_get()[1] == t + 1
        torch.cuda.synchronize()
        res.append((losses, tr.model._store.flat.detach().clone(), tr.opt.m.clone(), tr.opt.v.clone()))
        if recorded:
            names = {v: k for k, v in H.op_ids().items()}
            ops = [names.get(arr[i].op) for ph, arr in tr._recorded["phases"] if arr is not None for i in range(ph.n_cmds)]
            assert ops.count("segmm_step_advance") == 1 and ops.count("segmm_vec_add") >= 3 + 2 * 3          # gradient sums of 3 passes, loss sums
    (l0, p0, m0, v0), (l1, p1, m1, v1) = res
    assert l0 == l1, (l0, l1)
    assert torch.equal(p0, p1) and torch.equal(m0, m1) and torch.equal(v0, v1)


# ------------------------------------------------------------------------------------------------ 5: clipping and schedule
SCHED = dict(kind="cosine", warmup_steps=2, start_factor=0.1, decay_steps=6, eta_min=1e-5)
LR = 1e-3


@pytest.mark.parametrize("name", ["img_d32_N3_alllosses", "id_d32_N2"])
def test_clipping_and_schedule_are_per_optimizer_step(name):
    """max_grad_norm = 0.05 clips on both fixtures (measured whole-batch gradient norms at step 1: 2.527 on img_d32_N3_alllosses,
    0.6127 on id_d32_N2 -- clip coefficients 0.0198 and 0.0816), cosine schedule with a
    warm-up.  opt.grad_norm is the 2-norm of the SUMMED gradient -- within 1e-5 of the float64 norm of the plain whole-batch step's
    live gradient -- and the device rate moves once per step, whatever k is."""
    cfg, batch, (_, _, g0, _) = _plain(name)
    tr = _trainer(name, micro_batch=4, device_state=True, max_grad_norm=0.05, lr_schedule=SCHED, lr=LR)
    st = tr.model._store
    for t in range(1, 4):
        assert tr.opt.current_lr() == float(F(L.lr_at(t - 1, base_lr=LR, abi_rounded=True, **SCHED)))
        want = tr.opt.current_lr()
        tr.train_step(_clone(batch))
        lr_dev = tr.opt.device_lr()
        assert abs(lr_dev - want) <= float(np.spacing(F(want))), (t, lr_dev, want)
        if t == 1:
            norm64 = float(g0[:st.n_live].double().norm())
            got, coef = float(tr.opt.grad_norm), float(tr.opt._coef())
            print("%s: whole-batch gradient norm %.6g, micro-batched %.6g, clip coefficient %.4g" % (name, norm64, got, coef))
            assert norm64 > 0.05 and coef < 1.0          # the value clips
            assert abs(got - norm64) <= 1e-5 * norm64
    assert tr.opt.step_count == 3


# ------------------------------------------------------------------------------------------------ 6: dropout streams
@pytest.mark.parametrize("device_state", [True, False])
def test_micro_batches_of_one_step_draw_different_dropout(device_state):
    cfg, batch, _ = _plain("img_d32_N3_alllosses")
    b8 = {k: torch.cat([v[:4], v[:4]]).contiguous() for k, v in batch.items()}          # rows 4-7 are copies of rows 0-3
    for dropout in (False, True):
        torch.manual_seed(3)
        tr = _trainer("img_d32_N3_alllosses", micro_batch=4, dropout=dropout, device_state=device_state)
        lg = tr.train_step(_clone(b8))["logits"]
        assert tuple(lg.shape) == (8, cfg["S"])
        diff = float((lg[:4] - lg[4:8]).abs().max())
        print("dropout=%s device_state=%s: max |logits of pass 0 - logits of pass 1| = %.3g" % (dropout, device_state, diff))
        if dropout:          # other dropped elements move a logit by far more than the fixtures' logit tolerance
            assert diff > 1e-4
        else:
            assert torch.equal(lg[:4], lg[4:8])


# ------------------------------------------------------------------------------------------------ 7: the kernel
def _special(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g)
    sp = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1e-39, -3e-41, float("inf"), float("-inf"), float("nan"), 3.4e38, -3.4e38, 1.0], dtype=torch.float32)
    k = min(n, 4 * sp.numel())
    x[torch.randperm(n, generator=g)[:k]] = sp.repeat(4)[:k]
    return x


def _same_bits(got, want):
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(got.view(torch.int32)[~nan], want.view(torch.int32)[~nan])


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1023, 2 ** 20 + 3])
def test_vec_add_is_torch_add_bitwise(n):
    """Every combination of the three pointers' offsets from a 16-byte boundary (0 .. 3 floats each): the vector path where they
    agree, the dword path where they do not; head, tail and the elements around the output untouched."""
    H = _H()
    a, b = _special(n + 8, 1).to(DEV), _special(n + 8, 2).to(DEV)
    for oa, ob in itertools.product(range(4), repeat=2):
        want = torch.add(a[oa:oa + n], b[ob:ob + n])
        for oo in range(4):
            out = torch.full((n + 8,), 7.0, device=DEV)
            H.vec_add(out, a, b, n, oo, oa, ob)
            assert _same_bits(out[oo:oo + n], want), (n, oo, oa, ob)
            assert bool((out[:oo] == 7.0).all()) and bool((out[oo + n:] == 7.0).all()), (n, oo, oa, ob)
    for off, ob in itertools.product((0, 1), (0, 3)):          # out is exactly an operand
        want = torch.add(a[off:off + n], b[ob:ob + n])
        x = a.clone()
        H.vec_add(x, x, b, n, off, off, ob)
        assert _same_bits(x[off:off + n], want) and torch.equal(x[off + n:].view(torch.int32), a[off + n:].view(torch.int32))
        y = a.clone()
        H.vec_add(y, b, y, n, off, ob, off)
        assert _same_bits(y[off:off + n], want)


def test_vec_add_unrolled_loops_bitwise():
    """The size at which the production path runs: the launch is capped at 8 workgroups of 256 lanes per CU, so a lane takes the
    four-way unrolled loop only where more than 3 grid strides of work remain.  n = 5 x (8 CUs 256) vectors + 3 floats (10 x 2^20 + 3 on
    256 CUs) gives every lane of the 16-byte path one unrolled round and one single step, and every lane of the dword path five
    unrolled rounds; with the head, the tail and the guard elements.  Offsets that agree (0 and 1 float), offsets that do not, and
    both alias patterns on each path."""
    H = _H()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    stride = 8 * cus * 256
    n = 5 * stride * 4 + 3
    assert n // 4 > 4 * stride and n > 4 * stride          # both paths: unrolled rounds and a remainder
    a, b = _special(n + 8, 3).to(DEV), _special(n + 8, 4).to(DEV)
    for oo, oa, ob in ((0, 0, 0), (1, 1, 1), (3, 3, 3), (0, 1, 2), (2, 0, 0)):
        want = torch.add(a[oa:oa + n], b[ob:ob + n])
        out = torch.full((n + 8,), 7.0, device=DEV)
        H.vec_add(out, a, b, n, oo, oa, ob)
        assert _same_bits(out[oo:oo + n], want), (oo, oa, ob)
        assert bool((out[:oo] == 7.0).all()) and bool((out[oo + n:] == 7.0).all()), (oo, oa, ob)
        del out, want
    for off, ob in ((0, 0), (1, 1), (0, 3), (1, 2)):          # out is exactly an operand: 16-byte path (offsets agree) and dword path
        want = torch.add(a[off:off + n], b[ob:ob + n])
        x = a.clone()
        H.vec_add(x, x, b, n, off, off, ob)
        assert _same_bits(x[off:off + n], want), ("out is a", off, ob)
        assert torch.equal(x[:off].view(torch.int32), a[:off].view(torch.int32)) and torch.equal(x[off + n:].view(torch.int32), a[off + n:].view(torch.int32))
        y = a.clone()
        H.vec_add(y, b, y, n, off, ob, off)
        assert _same_bits(y[off:off + n], want), ("out is b", off, ob)
        del x, y, want


def test_vec_add_refuses_a_partial_overlap():
    H = _H()
    lib = H._lib_real()
    x, b = torch.arange(64, dtype=torch.float32, device=DEV), torch.ones(64, device=DEV)
    keep = x.clone()
    for args in ((x.data_ptr() + 4, x.data_ptr(), b.data_ptr()), (x.data_ptr(), b.data_ptr(), x.data_ptr() + 16),
                 (x.data_ptr(), x.data_ptr() + 60, b.data_ptr())):
        rc = lib.segmm_vec_add(*args, 16, H._stream())
        assert rc != 0 and "overlaps" in lib.segmm_last_error().decode()
    with pytest.raises(RuntimeError, match="segmm_vec_add.*overlaps"):
        H.vec_add(x, x, b, 16, 1, 0, 0)
    torch.cuda.synchronize()
    assert torch.equal(x, keep)          # nothing was written
    assert lib.segmm_vec_add(x.data_ptr(), x.data_ptr() + 64, b.data_ptr(), 16, H._stream()) == 0          # adjacent ranges are disjoint


# ------------------------------------------------------------------------------------------------ 8: memory
def test_activation_memory_is_that_of_a_micro_batch():
    """d = 128, N = 2, S = 40, Lt = 100, D_in = 128, B = 256: the peak of one step in micro-batches of 32 rows lies below the plain
    step's (the micro-batched trainer first, fresh trainers, each after reset_peak_memory_stats)."""
    from segmminterest_amd.synth import make_batch
    from segmminterest_amd.trainer import Trainer
    cfg = dict(S=40, N=2, d=128, h=4, user="image", photo="image", Lt=100, D_in=128, exposure_prob=[1.0] * 40,
               loss_type_list=["interestBPR"], loss_weight={"interestBPR": 1.0, "mse": 1.0})
    batch = {k: v.to(DEV) for k, v in make_batch(256, 40, 100, 128, seed=21).items()}
    peaks = []
    for m in (32, None):
        torch.manual_seed(5)
        tr = Trainer(build_model(cfg).to(DEV), dropout=False, micro_batch=m)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        tr.train_step(batch)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated())
        del tr
    print("peak bytes: micro_batch=32 %d, plain %d, ratio %.3f (allocated before the step: %d)" % (peaks[0], peaks[1], peaks[0] / peaks[1], base))
    assert peaks[0] < peaks[1]


# ------------------------------------------------------------------------------------------------ 9: data parallel
def _run_dp(rank, world, port, name, q):
    """world = 1: the plain step on the 16 rows; world = 2: gloo ranks sharing the GPU, 8 rows each in micro-batches of 4."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from segmminterest_amd.trainer import DPComm, Trainer, shard_rows
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        cfg, g, _, _ = load_case(name)
        torch.manual_seed(5)
        model = build_model(cfg)
        model.load_state_dict(g["sd"])
        model = model.cuda()
        tr = Trainer(model, comm=DPComm(), overlap=True, dropout=False, micro_batch=4 if world > 1 else None)
        full = _batch(cfg, 16, dev=None)
        s, e = shard_rows(16, world, rank)
        shard = {k: v[s:e].contiguous().cuda() for k, v in full.items()}
        losses, gflat = [], None
        for i in range(2):
            out = tr.train_step(shard)
            assert tuple(out["logits"].shape) == (e - s, cfg["S"])
            losses.append(float(tr.comm.sum_scalar(out["loss"].detach().clone())))
            if i == 0:
                gflat = model._store.gflat.detach().cpu().numpy().copy()
        assert tr.opt.step_count == 2
        if rank == 0:
            q.put((losses, gflat, {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}))
    finally:
        if world > 1:
            dist.destroy_process_group()


def _spawn(target, world, port, *args):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, world, port) + args + (q,)) for r in range(world)]
    for p in procs:
        p.start()
    res = q.get(timeout=240)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    return res


@pytest.mark.parametrize("name", ["img_d32_N3_alllosses", "id_d32_N2"])
def test_two_ranks_micro_batched_equal_single_plain_process(name):
    """Shard first, micro-batch second: label statistics gathered once for the rank's 8 rows, no collective inside a backward, one
    all-reduce of the summed gradient (id tables: the row exchange per micro-batch, accumulating)."""
    base = 29300 + (os.getpid() + (17 if name.startswith("id") else 0)) % 200
    (l1, g1, sd1), (l2, g2, sd2) = _spawn(_run_dp, 1, base, name), _spawn(_run_dp, 2, base + 1, name)
    g1, g2 = torch.from_numpy(g1), torch.from_numpy(g2)
    print("grad err %.3g of %.3g, losses %r / %r" % (float((g1 - g2).abs().max()), float(g1.abs().max()), l1, l2))
    assert float((g1 - g2).abs().max()) <= 1e-4 * float(g1.abs().max())
    assert _close(l1[0], l2[0], 1e-5) and _close(l1[1], l2[1], 3e-4), (l1, l2)
    for k in sd1:
        assert torch.allclose(torch.from_numpy(sd1[k]), torch.from_numpy(sd2[k]), rtol=1e-4, atol=4.5e-3), k


def _run_dp_recorded(rank, world, port, name, recorded, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from segmminterest_amd.trainer import DPComm, Trainer, shard_rows
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg, g, _, _ = load_case(name)
        torch.manual_seed(11)
        model = build_model(cfg)
        model.load_state_dict(g["sd"])
        model = model.cuda()
        tr = Trainer(model, comm=DPComm(), overlap=True, dropout=True, device_state=True, micro_batch=4)
        s, e = shard_rows(16, world, rank)
        shards = [{k: v[s:e].contiguous().cuda() for k, v in f.items()} for f in _rotating(_batch(cfg, 16, dev=None))]
        losses = []
        if recorded:
            tr.record(shards[0], warmup=2)
        else:
            for _ in range(3):          # what record(warmup=2) runs: two warm-up steps and the recorded one
                tr.train_step(shards[0])
        for t in range(4):
            out = tr.run_recorded(shards[t % 3]) if recorded else tr.train_step(shards[t % 3])
            losses.append(float(tr.comm.sum_scalar(out["loss"].detach().clone())))
        torch.cuda.synchronize()
        assert tr.opt.step_count == 7
        if rank == 0:
            q.put((losses, model._store.flat.detach().cpu().numpy(), tr.opt.m.cpu().numpy()))
    finally:
        dist.destroy_process_group()


def test_recorded_data_parallel_micro_batched_step_equals_eager():
    """Two gloo ranks, device_state, dropout on: the micro-batched data-parallel step replayed from its recording (the label
    statistics' all-gather, the one all-reduce and its wait as host actions) against the same steps enqueued from Python."""
    base = 29520 + os.getpid() % 60
    (l0, p0, m0), (l1, p1, m1) = (_spawn(_run_dp_recorded, 2, base + 2 * r, "img_d32_N3_alllosses", r) for r in (0, 1))
    assert l0 == l1, (l0, l1)
    assert (p0 == p1).all() and (m0 == m1).all()
