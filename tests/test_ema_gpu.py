"""The weight average on the MI355X: segmm_ema_update and segmm_vec_swap bit for bit against the host reference (tests/ema_ref.py), and
Trainer(ema=...) -- eager, recorded, micro-batched, id tables in one and two passes, the swap (logits, training continuity, recorded
validation), checkpoints and two ranks -- against a host replay of the reference on the per-step parameters."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import ema_ref as R
from helpers import ROOT, build_model, load_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32

SIZES = [0, 1, 3, 4, 5, 255, 256, 257, 1023, 1025, 4099, 70001]
PAD = 8          # floats behind the range that must stay untouched (a multiple of 4: every offset stays 16-byte aligned)


def _H():
    from segmminterest_amd import hipabi as H
    H.lib()
    return H


def _big_n():
    """More than four grid rounds of 16-byte vectors, plus 300 vectors, plus a 3-float tail: the lanes below 300 take the unrolled loop
    AND the single-vector loop, every other lane the unrolled loop alone, workgroup 0 the tail (8.4 M floats on 256 CUs)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return 4 * (4 * cus * 8 * 256 + 300) + 3


def _sizes():
    return SIZES + ["grid"]


@pytest.fixture
def step_state():
    """A zeroed device step state of the test's own, bound for the test; the library's default state is bound again afterwards."""
    H = _H()
    state = torch.zeros((H.step_state_bytes() + 3) // 4, dtype=torch.int32, device=DEV)
    H.step_bind(state)
    try:
        yield state
    finally:
        torch.cuda.synchronize()
        H.step_bind(None)


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("n", _sizes())
def test_ema_update_equals_the_reference_bitwise(n, step_state):
    """A chain of in-place updates on one shadow: with and without warm-up, t in {1, 2, 9, 1000} by value and as step = -1 against
    the bound step state set to the same count; after every launch the shadow equals the reference's (NaN lanes: NaN on both sides)
    and the PAD floats behind the range keep their bits.  Inputs carry +-0, denormals, +-inf and NaN in both operands."""
    H = _H()
    n = _big_n() if n == "grid" else n
    s_h, p_h = R.special_values(n, seed=n + 1)
    guard = np.full(PAD, 123.25, dtype=F)
    shadow = torch.from_numpy(np.concatenate([s_h, guard])).to(DEV)
    p = torch.from_numpy(np.concatenate([p_h, -guard])).to(DEV)
    want = s_h.copy()
    decay = 0.999
    for warmup in (True, False):
        for t in (1, 2, 9, 1000):
            for live in (False, True):
                if live:
                    H.step_set(99, t, 0.9, 0.999)
                H.ema_update(shadow, p, n, float(R.weight(decay)), warmup, -1 if live else t)
                want = R.update(want, p_h, decay, t, warmup)
                got = shadow.cpu().numpy()
                assert R.bits_equal_nan_aware(got[:n], want), (n, warmup, t, live)
                assert (got[n:].view(np.int32) == guard.view(np.int32)).all(), (n, warmup, t, live)
    assert (p.cpu().numpy()[:n].view(np.int32) == p_h.view(np.int32)).all()          # p is only read
    if n > 300:          # the chain did something, and the special lanes behave as IEEE says (inf - inf: every inf lane ends as NaN)
        assert not R.bits_equal_nan_aware(want, s_h)
        assert np.isnan(want).any() and np.isfinite(want).sum() > 0.9 * n


def test_ema_update_nontemporal_and_default_policy_give_the_same_bits():
    H = _H()
    n = 70001
    s_h, p_h = R.special_values(n, seed=5)
    outs = []
    prev = H.knob("EMA_NT")
    try:
        for nt in (1, 0):
            H.config_set("EMA_NT", nt)
            s = torch.from_numpy(s_h).to(DEV)
            H.ema_update(s, torch.from_numpy(p_h).to(DEV), n, 0.25, False, 1)
            outs.append(s.cpu().numpy())
    finally:
        H.config_set("EMA_NT", prev)
    assert R.bits_equal_nan_aware(outs[0], R.lerp(s_h, p_h, 0.25)) and (outs[0].view(np.int32) == outs[1].view(np.int32)).all()


def test_ema_update_and_vec_swap_refusals_name_the_reason():
    H = _H()
    x = torch.zeros(64, device=DEV)
    y = torch.ones(64, device=DEV)
    with pytest.raises(RuntimeError, match="segmm_ema_update.*16-byte aligned"):
        H.ema_update(x, y, 16, 0.5, False, 1, shadow_off=1)
    with pytest.raises(RuntimeError, match="segmm_ema_update.*16-byte aligned"):
        H.ema_update(x, y, 16, 0.5, False, 1, p_off=2)
    with pytest.raises(RuntimeError, match="segmm_ema_update.*overlap"):
        H.ema_update(x, x, 16, 0.5, False, 1, shadow_off=0, p_off=8)
    with pytest.raises(RuntimeError, match="segmm_ema_update.*overlap"):
        H.ema_update(x, x, 16, 0.5, False, 1)
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(RuntimeError, match="segmm_ema_update.*weight"):
            H.ema_update(x, y, 16, bad, False, 1)
    for bad in (0, -2):
        with pytest.raises(RuntimeError, match="segmm_ema_update.*step"):
            H.ema_update(x, y, 16, 0.5, True, bad)
    with pytest.raises(RuntimeError, match="segmm_vec_swap.*16-byte aligned"):
        H.vec_swap(x, y, 16, a_off=3)
    with pytest.raises(RuntimeError, match="segmm_vec_swap.*overlap"):
        H.vec_swap(x, x, 16, a_off=0, b_off=12)
    H.ema_update(x, x, 16, 0.5, False, 1, shadow_off=0, p_off=16)          # adjacent ranges are disjoint
    H.vec_swap(x, x, 16, a_off=16, b_off=32)
    torch.cuda.synchronize()
    assert not bool(x.any()) and bool((y == 1).all())          # nothing was written by a refused call


@pytest.mark.parametrize("n", _sizes())
def test_vec_swap_exchanges_exactly_and_twice_is_the_identity(n):
    H = _H()
    n = _big_n() if n == "grid" else n
    a_h, b_h = R.special_values(n, seed=n + 2)
    guard = np.full(PAD, 7.5, dtype=F)
    a = torch.from_numpy(np.concatenate([a_h, guard])).to(DEV)
    b = torch.from_numpy(np.concatenate([b_h, -guard])).to(DEV)
    a0, b0 = a.clone(), b.clone()
    H.vec_swap(a, b, n)
    assert _bits_equal(a[:n], b0[:n]) and _bits_equal(b[:n], a0[:n])
    assert _bits_equal(a[n:], a0[n:]) and _bits_equal(b[n:], b0[n:])
    H.vec_swap(a, b, n)
    assert _bits_equal(a, a0) and _bits_equal(b, b0)


# ------------------------------------------------------------------------------------------------ the trainer
def _cfg(name, S=8, Lt=4):
    cfg, g, _, _ = load_case(name)
    return dict(cfg, S=S, Lt=min(Lt, cfg["Lt"]), exposure_prob=list(cfg["exposure_prob"])[:S])


def _batches(cfg, n=3, B=4, dev=DEV, seed0=500):
    from segmminterest_amd.synth import make_batch
    out = [make_batch(B, cfg["S"], cfg["Lt"], cfg["D_in"], n_users=cfg.get("n_users", 5) or 5, n_items=cfg.get("n_items", 5) or 5, seed=seed0 + i)
           for i in range(n)]
    return out if dev is None else [{k: v.to(dev) for k, v in b.items()} for b in out]


def _trainer(cfg, **kw):
    from segmminterest_amd.trainer import Trainer
    torch.manual_seed(5)
    model = build_model(cfg).to(DEV)
    kw.setdefault("dropout", False)
    return Trainer(model, **kw)


def _live(tr):
    """The live range of the flat parameter buffer, on the host."""
    st = tr.model._store
    st.ensure()
    torch.cuda.synchronize()
    return st.flat[:st.n_live].detach().cpu().numpy().copy()


def _shadow(tr):
    torch.cuda.synchronize()
    return tr.ema.shadow.detach().cpu().numpy().copy()


def _snap(tr):
    torch.cuda.synchronize()
    return tuple(x.detach().clone() for x in (tr.model._store.flat, tr.opt.m, tr.opt.v) + ((tr.ema.shadow,) if tr.ema is not None else ()))


def _equal(a, b):
    return len(a) == len(b) and all(_bits_equal(x, y) for x, y in zip(a, b))


def _same_bits(a, b):
    return a.shape == b.shape and bool((a.view(np.int32) == b.view(np.int32)).all())


EMA = dict(decay=0.9, warmup=True)


# ---- 1. eager replay
@pytest.mark.parametrize("device_state", [False, True], ids=["by_value", "device_state"])
@pytest.mark.parametrize("case,ema", [("img_d32_N2", EMA), ("both_fh2", EMA), ("img_d32_N2", dict(decay=0.999, warmup=False))],
                         ids=["img", "both", "img_nowarm"])
def test_eager_steps_equal_the_host_replay_bitwise(case, ema, device_state):
    """Five eager steps; after each the shadow equals the reference replayed on the host over the per-step live range, seeded with
    the parameters before step 1 -- with the step count by value and from the device step state."""
    cfg = _cfg(case)
    batches = _batches(cfg)
    tr = _trainer(cfg, ema=ema, device_state=device_state)
    assert tr.ema is tr.opt.ema and tr.ema.shadow is None
    want = _live(tr)
    seed = want.copy()
    for t in range(1, 6):
        tr.train_step(batches[t % 3])
        p = _live(tr)
        want = R.update(want, p, ema["decay"], t, ema["warmup"])
        assert _same_bits(_shadow(tr), want), (case, t)
    assert not _same_bits(want, seed) and not _same_bits(want, p)          # an average: neither the seed nor the weights
    assert tr.ema.shadow.numel() == tr.model._store.n_live and tr.ema.shadow.dtype == torch.float32


def test_the_seed_is_taken_at_the_head_of_the_first_optimizer_step():
    """The shadow is read before any step (applied(), state_dict()), then other weights are loaded into the model: the average starts
    from the weights as they stand at the head of step 1, not from the ones the earlier read saw."""
    cfg = _cfg("img_d32_N2")
    batches = _batches(cfg)
    tr = _trainer(cfg, ema=EMA)
    first = _live(tr)
    with tr.ema.applied():
        pass
    assert _same_bits(_shadow(tr), first) and all(torch.equal(v, tr.model.state_dict()[k].cpu()) for k, v in tr.ema.state_dict().items())
    torch.manual_seed(7)
    tr.model.load_state_dict(build_model(cfg).state_dict())
    seed = _live(tr)
    assert not _same_bits(seed, first)
    tr.train_step(batches[0])
    assert _same_bits(_shadow(tr), R.update(seed, _live(tr), EMA["decay"], 1, True))


# ---- 2. nothing changes without an EMA, and the EMA does not disturb the step
def _recorded_ops(tr):
    H = _H()
    names = {v: k for k, v in H.op_ids().items()}
    return [[names.get(arr[i].op, arr[i].op) for i in range(ph.n_cmds)] for ph, arr in tr._recorded["phases"] if arr is not None]


def test_plain_step_launches_are_unchanged_and_the_twin_is_bit_identical():
    """Per phase of a recorded step, the trainer with an EMA has the command list of the trainer without one plus ONE segmm_ema_update,
    the last command of the tail; the trainer without one launches no EMA kernel (recorded commands and the profiled eager launches);
    parameters, m and v of the two are bit-equal after the same steps."""
    H = _H()
    cfg = _cfg("img_d32_N2")
    batches = _batches(cfg)
    plain, twin = _trainer(cfg, device_state=True), _trainer(cfg, device_state=True, ema=EMA)
    assert plain.ema is None and plain.opt.ema is None
    for tr in (plain, twin):
        tr.record(batches[0], warmup=2)
        tr.run_recorded(batches[1])
    a, b = _recorded_ops(plain), _recorded_ops(twin)
    assert len(a) == len(b) and a[:-1] == b[:-1]
    assert b[-1] == a[-1] + ["segmm_ema_update"]
    assert not any(op in ("segmm_ema_update", "segmm_vec_swap") for ph in a for op in ph)
    assert sum(ph.count("segmm_ema_update") for ph in b) == 1
    names = []
    for tr in (plain, twin):
        H.KERNEL_PROFILE = []
        try:
            tr.train_step(batches[2])
            torch.cuda.synchronize()
            names.append([e[0] for e in H.KERNEL_PROFILE])
        finally:
            H.KERNEL_PROFILE = None
    assert "ema_update" not in names[0] and names[1] == names[0] + ["ema_update"]
    sp, stw = _snap(plain), _snap(twin)
    assert _equal(sp, stw[:3]) and plain.opt.step_count == twin.opt.step_count == 5


# ---- 3. recorded and micro-batched
SCHED = dict(kind="cosine", warmup_steps=2, decay_steps=8, eta_min=1e-4)


@pytest.mark.parametrize("kw", [{}, {"lr_schedule": SCHED}, {"micro_batch": 2}], ids=["plain", "lr_schedule", "micro_batch"])
def test_recorded_steps_equal_the_eager_twin_bitwise(kw):
    """Six steps: all eager, against one eager + record() + four run_recorded(); shadow (and p, m, v) bit-equal, and the eager shadow is
    the host replay's -- one update per OPTIMIZER step under micro_batch=2 with B = 4.  run_recorded() after ema.decay changed is refused."""
    cfg = _cfg("img_d32_N2")
    batches = _batches(cfg)
    eager, rec = (_trainer(cfg, ema=EMA, device_state=True, **kw) for _ in range(2))
    want = _live(eager)
    for t in range(1, 7):
        eager.train_step(batches[(t - 1) % 3])
        want = R.update(want, _live(eager), EMA["decay"], t, True)
    assert _same_bits(_shadow(eager), want)
    for t in range(1, 7):
        b = batches[(t - 1) % 3]
        if t < 2:
            rec.train_step(b)
        elif t == 2:
            rec.record(b, warmup=0, prev_batch=batches[(t - 2) % 3])
        else:
            rec.run_recorded(b)
    assert _equal(_snap(eager), _snap(rec)) and rec.opt.step_count == 6
    ops = [op for ph in _recorded_ops(rec) for op in ph]
    assert ops.count("segmm_ema_update") == 1
    rec.ema.decay = 0.5
    with pytest.raises(RuntimeError, match="record\\(\\) again"):
        rec.run_recorded(batches[0])


# ---- 4. id mode: the two-pass table update and the dense one
def _id_run(two_pass, q=None):
    """4 steps of the id-mode model -> (shadow, seed, [live range after each step]) as numpy (and into ``q``)."""
    os.environ["SEGMM_TABLE_TWO_PASS"] = "1" if two_pass else "0"
    sys.path.insert(0, ROOT)
    cfg = _cfg("id_d32_N2")
    batches = _batches(cfg)
    tr = _trainer(cfg, lr=1e-3, weight_decay=1e-2, ema=EMA)
    assert tr.table_two_pass == two_pass
    seed = _live(tr)
    params = []
    for t in range(4):
        tr.train_step(batches[t % 3])
        params.append(_live(tr))
    if two_pass:
        assert tr.opt.__dict__.get("_table_flags")          # the early pass ran
    st = tr.model._store
    res = (_shadow(tr), seed, params, st.index["backbone1.vid_proj.weight"])
    if q is not None:
        q.put(res)
    return res


def _child(target, *args, timeout=240):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=target, args=args + (q,))
    p.start()
    res = q.get(timeout=timeout)
    p.join(60)
    assert p.exitcode == 0
    return res


def test_id_tables_two_pass_and_dense_shadows_equal_the_replay_on_all_rows():
    """The two-pass table update (untouched rows stepped at the head of the step, on the auxiliary stream) and the dense one
    (SEGMM_TABLE_TWO_PASS=0, read when the trainer is built: a child process) give bit-equal shadows, and both equal the host replay
    over the WHOLE live range -- the table's untouched rows included: seeded before the early pass, updated after the late one."""
    try:
        two = _id_run(True)
    finally:
        os.environ.pop("SEGMM_TABLE_TWO_PASS", None)
    dense = _child(_id_run, False)
    assert _same_bits(two[0], dense[0])
    for shadow, seed, params, (o, k) in (two, dense):
        want = R.replay(seed, params, EMA["decay"], True)
        assert _same_bits(shadow, want)
        moved = (params[-1][o:o + k] != seed[o:o + k])
        assert moved.mean() > 0.9          # weight decay moves the rows no batch touched, too
        assert not _same_bits(shadow[o:o + k], params[-1][o:o + k])


# ---- 5. / 6. / 7. the swap
def test_applied_logits_equal_a_model_that_loaded_the_ema_state_dict():
    from segmminterest_amd.trainer import Trainer
    cfg = _cfg("both_fh2")
    batches = _batches(cfg, n=4)
    tr = _trainer(cfg, ema=EMA)
    for t in range(3):
        tr.train_step(batches[t])
    plain = tr.eval_step(batches[3], mode="inference")["logits"].clone()
    sd = tr.ema.state_dict()
    assert list(sd) == list(tr.model.state_dict()) and all(sd[k].shape == v.shape for k, v in tr.model.state_dict().items())
    before = _snap(tr)
    with tr.ema.applied():
        with pytest.raises(RuntimeError, match="nested applied"):
            with tr.ema.applied():
                pass
        with pytest.raises(RuntimeError, match=r"train_step\(\) inside ema\.applied\(\)"):
            tr.train_step(batches[0])
        got = tr.eval_step(batches[3], mode="inference")["logits"].clone()
        assert all(torch.equal(v.cpu(), sd[k]) for k, v in tr.model.state_dict().items())          # the model IS the average now
    assert _equal(before, _snap(tr)) and not tr.ema.is_applied
    torch.manual_seed(99)
    other = build_model(cfg).to(DEV)
    other.load_state_dict(sd)
    want = Trainer(other, dropout=False).eval_step(batches[3], mode="inference")["logits"]
    assert _bits_equal(got, want)
    assert not torch.equal(got, plain)
    # the inverse: a fresh EMA that loads the dict holds the same shadow
    tr2 = _trainer(cfg, ema=EMA)
    tr2.ema.load_state_dict(sd)
    assert _bits_equal(tr2.ema.shadow, tr.ema.shadow)
    with pytest.raises(KeyError, match="ema.load_state_dict: no entry for the parameter"):
        tr2.ema.load_state_dict({})


@pytest.mark.parametrize("recorded", [False, True], ids=["eager", "recorded"])
def test_training_continues_bit_identically_after_a_swap(recorded):
    """Three steps, an evaluation inside applied(), three more steps -- against a twin that evaluated WITHOUT the swap: parameters
    bit-equal right after the exit and p, m, v and shadow bit-equal after the further steps.  Stale weight planes (the split of the
    averaged weights left behind) would show here."""
    cfg = _cfg("img_d32_N2")
    batches = _batches(cfg, n=4)
    runs = []
    for swap in (False, True):
        tr = _trainer(cfg, ema=EMA, device_state=recorded)
        for t in range(6):
            b = batches[t % 3]
            if not recorded or t < 1:
                tr.train_step(b)
            elif t == 1:
                tr.record(b, warmup=0, prev_batch=batches[(t - 1) % 3])
            else:
                tr.run_recorded(b)
            if t == 2:
                before = _snap(tr)
                v0 = tr.model._store.fused_version
                if swap:
                    with tr.ema.applied():
                        assert tr.model._store.fused_version == v0 + 1
                        tr.eval_step(batches[3], mode="inference")
                    assert tr.model._store.fused_version == v0 + 2
                else:
                    tr.eval_step(batches[3], mode="inference")
                assert _equal(before, _snap(tr))
        runs.append(_snap(tr))
    assert _equal(*runs)


def _check_rank_gaps(tr, batches, exposure):
    """Precondition of comparing the recorded pass's ranks with the eager pass's (torch's sigmoid against the library's): no
    candidate's interest within 1e-6 relative of the target's unless it is its exact tie (tests/test_valid_recorded_gpu.py)."""
    expo = torch.tensor(exposure, dtype=torch.float64)
    for bi, b in enumerate(batches):
        out = tr.eval_step(b, mode="train")
        lg, gt = out["logits"].cpu(), out["gt"].cpu()
        x = torch.sigmoid(lg.double()) * expo[: lg.shape[1]]
        vl = (gt == 1).sum(1)
        for row in torch.nonzero(vl < lg.shape[1]).reshape(-1).tolist():
            t = int(vl[row])
            gap = (x[row] - x[row, t]).abs() / x[row, t]
            same = (lg[row] == lg[row, t]) & (expo[: lg.shape[1]] == expo[t])
            bad = ~((gap > 1e-6) | ((gap == 0) & same))
            assert not bool(bad.any()), "batch %d row %d: a near-tie with the target interest -- pick another seed" % (bi, row)


def test_recorded_validation_on_the_averaged_weights_equals_the_eager_pass():
    cfg = _cfg("img_d32_N2")
    batches = _batches(cfg)
    valid = _batches(cfg, n=3, seed0=900)
    tr = _trainer(cfg, ema=EMA, lr=1e-2)
    for t in range(4):
        tr.train_step(batches[t % 3])
    with tr.ema.applied():
        _check_rank_gaps(tr, valid, cfg["exposure_prob"])
    _check_rank_gaps(tr, valid, cfg["exposure_prob"])
    before = _snap(tr)
    eager = tr.valid_model(valid, permutation=0, ema=True)
    rec1 = tr.valid_model(valid, permutation=0, ema=True, recorded=True)          # records one batch, replays two
    rec2 = tr.valid_model(valid, permutation=0, ema=True, recorded=True)          # three replays, on planes split again
    plain = tr.valid_model(valid, permutation=0)
    plain_rec = tr.valid_model(valid, permutation=0, recorded=True)               # the same recording, the trained weights' planes
    assert tr._valid_rec["n_replays"] == 8
    assert eager == rec1 == rec2 and plain == plain_rec
    assert eager["valid_loss"] != plain["valid_loss"]
    assert _equal(before, _snap(tr)) and not tr.ema.is_applied
    with pytest.raises(ValueError, match=r"valid_model\(ema=True\) needs Trainer\(ema=\.\.\.\)"):
        _trainer(cfg).valid_model(valid, ema=True)


# ---- 8. checkpoints
def test_fit_writes_model_ema_and_a_resumed_run_continues_bit_identically(tmp_path):
    from segmminterest_amd.trainer import CheckPointer, fit
    cfg = _cfg("img_d32_N2")
    train = _batches(cfg, n=6)
    valid = _batches(cfg, n=2, seed0=900)
    kw = dict(ema=EMA, device_state=True)
    whole = _trainer(cfg, **kw)
    ck = CheckPointer("main_metric", str(tmp_path), mode="max")
    hist = fit(whole, train, valid, epochs=1, valid_step=3, ckpt=ck, permutation=0, ema_valid=True)
    assert hist["global_step"] == 6 and len(hist["NDCG@5"]) == 3
    sd = torch.load(ck.ckpt_latest, map_location="cpu", weights_only=False)
    assert list(sd["model_ema"]) == list(sd["model"]) and all(sd["model_ema"][k].shape == v.shape for k, v in sd["model"].items())
    assert any(not torch.equal(sd["model_ema"][k], v) for k, v in sd["model"].items())
    # the validations of the loop ran on the averaged weights
    assert hist["valid_loss"][-1] == whole.valid_model(valid, permutation=0, ema=True)["valid_loss"]
    assert hist["valid_loss"][-1] != whole.valid_model(valid, permutation=0)["valid_loss"]
    # the reference's model loads the entry directly: its keys and shapes are the model's own
    torch.manual_seed(1)
    build_model(cfg).load_state_dict(sd["model_ema"])
    for t in range(2):
        whole.train_step(train[t])
    # resume from the checkpoint written after step 6
    second = _trainer(cfg, **kw)
    ck.load_checkpoint(second.model, second.opt, ema=second.ema)
    assert second.opt.step_count == 6
    for t in range(2):
        second.train_step(train[t])
    assert _equal(_snap(whole), _snap(second))
    # ... and the warm-up continued: the shadow is the replay from the loaded one at t = 7, 8 (not 1, 2)
    third = _trainer(cfg, **kw)
    ck.load_checkpoint(third.model, third.opt, ema=third.ema)
    s = _shadow(third)
    params = []
    for t in range(2):
        third.train_step(train[t])
        params.append(_live(third))
    assert _same_bits(_shadow(third), R.replay(s, params, EMA["decay"], True, t0=6))
    assert not _same_bits(_shadow(third), R.replay(s, params, EMA["decay"], True, t0=0))
    # a checkpoint written without an EMA is refused by name when one is to be restored, and loads as ever without
    ck2 = CheckPointer("main_metric", str(tmp_path / "noema"), mode="max")
    ck2.save_checkpoint(second.model, second.opt, 0, {"main_metric": 0.1})
    with pytest.raises(KeyError, match="model_ema"):
        ck2.load_checkpoint(second.model, second.opt, ema=second.ema)
    assert "model_ema" not in ck2.load_checkpoint(second.model, second.opt)


# ---- 9. two ranks
def _run_dp(rank, world, port, q):
    """Two gloo ranks sharing the GPU, 4 rows each of 8-row batches, three steps with an EMA."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from segmminterest_amd.trainer import DPComm, Trainer, shard_rows
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        cfg = _cfg("img_d32_N2")
        torch.manual_seed(5)
        model = build_model(cfg).cuda()
        tr = Trainer(model, lr=1e-3, weight_decay=1e-2, comm=DPComm(), overlap=True, dropout=False, ema=EMA)
        assert tr.comm.active
        s, e = shard_rows(8, world, rank)
        shards = [{k: v[s:e].contiguous().cuda() for k, v in b.items()} for b in _batches(cfg, n=3, B=8, dev=None)]
        seed = _live(tr)
        params = []
        for t in range(3):
            tr.train_step(shards[t])
            params.append(_live(tr))
        q.put((rank, _shadow(tr), seed, params))
    finally:
        dist.destroy_process_group()


def test_two_ranks_keep_the_same_shadow():
    """The per-bucket data-parallel tail: both ranks' shadows are bit-equal to each other and to the host replay over rank 0's
    per-step parameters (no collective carries the shadow)."""
    port = 29900 + os.getpid() % 90
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_run_dp, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(2):
        r = q.get(timeout=240)
        res[r[0]] = r[1:]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert _same_bits(res[0][0], res[1][0])
    shadow, seed, params = res[0]
    assert _same_bits(shadow, R.replay(seed, params, EMA["decay"], True))
    assert not _same_bits(shadow, params[-1])
