"""Trainer.dump_logits(recorded=True): the inference pass replayed from one recorded launch sequence whose tail is ONE
segmm_store_append into a preallocated DeviceLogitStore, against today's eager dump of the same trainer.  Keys and values are bit
copies of what the eager pass stores: every comparison is exact."""
import types

import numpy as np
import pytest
import torch

from helpers import build_model, load_case
from segmminterest_amd.bridge import DeviceLogitStore

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B, S, LT, D, N = 48, 40, 10, 32, 2
T0 = 1_700_000_000_000          # time_ms of the reference's logs: 41 bits


def _H():
    from segmminterest_amd import hipabi
    hipabi.lib()
    return hipabi


def _id_cfg():
    cfg, _, _, _ = load_case("id_d32_N2")          # id mode: d = 32, h = 4, N = 2, S = 40; the user is ONE id token
    return dict(cfg, n_items=500)


def _batches(kind, n, rows=B, seed0=100):
    from segmminterest_amd.synth import make_batch
    out = []
    for i in range(n):
        if kind == "image":
            b = make_batch(rows, S, LT, D, seed=seed0 + i)
        else:
            cfg = _id_cfg()
            b = make_batch(rows, cfg["S"], cfg["Lt"], cfg["D_in"], n_users=cfg["n_users"], n_items=cfg["n_items"], seed=seed0 + i)
        b["time_ms"] = b["time_ms"] + T0
        out.append({k: v.to(DEV) for k, v in b.items()})
    return out


def _trainer(kind, seed=3, **kw):
    from segmminterest_amd.trainer import Trainer, default_args, init_model
    torch.manual_seed(seed)
    if kind == "image":
        margs = default_args(num_layers_enc=N, d_model=D, nhead=4, input_type={"user": "image", "photo": "image"}, exposure_prob=[0.9] * S)
        model = init_model(margs, n_users=1, n_items=1, input_dim=D, max_vid_len=S, max_usr_len=LT).to(DEV)
    else:
        model = build_model(_id_cfg()).to(DEV)
    return Trainer(model, **kw)


def _splits(kind):
    """two splits of full batches plus a short last batch each; one key repeats across the splits (the later logits win)"""
    a = _batches(kind, 3) + _batches(kind, 1, rows=17, seed0=200)
    b = _batches(kind, 2, seed0=300) + _batches(kind, 1, rows=5, seed0=400)
    for k in ("user_id", "photo_id", "time_ms"):
        b[1][k] = b[1][k].clone()
        b[1][k][5] = a[0][k][2]
    return [a, b]


N_FULL, N_ROWS = 5, 5 * B + 17 + 5


def _same_store(x, y):
    (kx, vx), (ky, vy) = x._cat(), y._cat()
    return len(x) == len(y) and torch.equal(kx, ky) and torch.equal(vx.view(torch.int32), vy.view(torch.int32))


def _npz_bytes(store, path):
    store.to_store().save_binary(path)
    return open(path, "rb").read()


@pytest.mark.parametrize("kind", ("image", "id"))
def test_recorded_dump_equals_the_eager_dump_on_record_and_on_replay(kind, tmp_path):
    """First pass: one batch recorded, four replayed, the two short ones eager with the append tail; second pass: replays only."""
    _H()
    tr = _trainer(kind)
    splits = _splits(kind)
    want = tr.dump_logits(splits)
    assert len(want) == N_ROWS and want.capacity is None
    got1 = tr.dump_logits(splits, recorded=True)
    r = tr._dump_rec
    assert r["n_replays"] == N_FULL - 1 and r["spans"]["label"][0] == (B, S)
    got2 = tr.dump_logits(splits, recorded=True)
    assert tr._dump_rec is r and r["n_replays"] == 2 * N_FULL - 1
    for got in (got1, got2):
        assert isinstance(got, DeviceLogitStore) and got.capacity >= N_ROWS and _same_store(got, want)
    ref = _npz_bytes(want, tmp_path / "eager.npz")
    assert _npz_bytes(got1, tmp_path / "rec1.npz") == ref and _npz_bytes(got2, tmp_path / "rec2.npz") == ref
    assert got1.to_store().as_dict() == want.to_store().as_dict() and len(want.to_store().as_dict()) == N_ROWS - 1
    # finalize(on_device=True) on the recorded store answers like today's path on the eager store
    q = splits[0][0]
    u, it, t = q["user_id"][:8], torch.stack([q["photo_id"][:8], q["photo_id"][8:16]], 1), q["time_ms"][:8]
    w = got2.finalize(on_device=True).weights(u, it, t)
    assert torch.equal(w, want.finalize().weights(u, it, t)) and torch.equal(got2._index[0], want._index[0]) and torch.equal(got2._index[1], want._index[1])
    assert torch.equal(w[2, 0], tr.eval_step(splits[1][1], mode="inference")["logits"][5])          # the repeated key: the later batch's logits
    # a caller's store (preallocated, or a block list that the pass turns into tables) is appended to
    own = DeviceLogitStore(S=S, device=DEV, capacity=8)
    assert tr.dump_logits(splits, store=own, recorded=True) is own and _same_store(own, want) and own.capacity >= N_ROWS
    mixed = tr.dump_logits(splits[:1])
    assert tr.dump_logits(splits[1:], store=mixed, recorded=True) is mixed and _same_store(mixed, want)


def test_a_replayed_batch_enqueues_nothing_from_python(monkeypatch):
    """After the first pass: a pass over full batches is replays only -- the binding's per-launch door (hipabi.lib) is not passed
    once, the recording's command count covers the pass -- and the enqueue never synchronises."""
    H = _H()
    tr = _trainer("image")
    full = _batches("image", 4)
    want = tr.dump_logits([full])
    tr.dump_logits([full], recorded=True)
    r = tr._dump_rec
    names = {v: k for k, v in H.op_ids().items()}
    cmds = [names.get(arr[i].op) for ph, arr in r["phases"] if arr is not None for i in range(ph.n_cmds)]
    assert r["n_cmds"] == len(cmds) > 10 and cmds[0] == "segmm_fill_zero" and cmds[-1] == "segmm_store_append" and cmds.count("segmm_store_append") == 1
    assert r["n_replays"] == 3
    store = DeviceLogitStore(S=S, device=DEV, capacity=4 * B)          # (room for the pass: no growth copies)
    torch.cuda.synchronize()
    calls = []
    real = H.lib
    monkeypatch.setattr(H, "lib", lambda: (calls.append(1), real())[1])
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = tr.dump_logits([full], store=store, recorded=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert calls == [] and r["n_replays"] == 7 and len(got) == 4 * B
    monkeypatch.undo()
    assert _same_store(got, want)


def test_replays_never_write_buffers_the_trainer_has_let_go():
    """The trainer replaces its normalised-feature buffers when a batch of another shape comes by (the short last batch of a split);
    the recording holds the ones its commands name.  20 passes into fresh stores of three capacities -- whose tables the allocator
    places wherever memory has come free --, an eager full-shape forward and a device index build thrown in: every pass equals
    the eager dump."""
    _H()
    tr = _trainer("image")
    splits = _splits("image")
    want = tr.dump_logits(splits)
    tr.dump_logits(splits, recorded=True)
    held = tr._dump_rec["held"]
    full = {k: v for k, v in held[1].items() if v.shape[0] == B}          # (the other slot's entries are whatever batch came by last)
    assert held[0].shape == (B, S) and {k[0] for k in full} == {"user", "photo"}
    ptrs = {k: v.data_ptr() for k, v in full.items()}
    tr.eval_step(splits[0][3], mode="inference")
    tr.eval_step(splits[1][2], mode="inference")          # the short batches: both buffer sets of the trainer are replaced
    assert all(tr._norm[k] is not v and tr._norm[k].shape[0] != B for k, v in full.items())
    assert {k: v.data_ptr() for k, v in tr._dump_rec["held"][1].items() if k in ptrs} == ptrs
    for i in range(20):
        own = DeviceLogitStore(S=S, device=DEV, capacity=(8, 300, 1024)[i % 3])
        tr.dump_logits(splits, store=own, recorded=True)
        assert _same_store(own, want), i
        if i % 4 == 1:
            tr.eval_step(splits[1][1], mode="inference")
            own.finalize(on_device=True)


def test_a_train_step_between_two_recorded_passes_shows_in_the_second():
    _H()
    tr = _trainer("image", lr=1e-2, dropout=False)
    splits = _splits("image")
    first = tr.dump_logits(splits, recorded=True)
    for b in _batches("image", 2, seed0=500):
        tr.train_step(b)
    second = tr.dump_logits(splits, recorded=True)
    assert tr._dump_rec["n_replays"] == 2 * N_FULL - 1
    assert _same_store(second, tr.dump_logits(splits)) and not _same_store(second, first)
    assert torch.equal(second._cat()[0], first._cat()[0])          # the keys are the batches'


def test_ema_lazy_tables_and_a_recorded_training_step_interleave():
    """id mode, Trainer(ema=..., lazy_tables=dict(ema=True), device_state=True): eager steps, the recorded training step, recorded dumps
    of the trained and of the averaged weights between its replays -- each equal to the eager dump at the same point, and the
    training run equal to its twin that only ever dumped eagerly."""
    _H()
    train, splits = _batches("id", 6, seed0=700), _splits("id")

    def run(recorded):
        tr = _trainer("id", ema=dict(decay=0.9, warmup=True), lazy_tables=dict(flush_every=8, ema=True), device_state=True, dropout=False,
                      lr=1e-2, weight_decay=1e-2)
        dumps = []
        tr.train_step(train[0])
        tr.train_step(train[1])
        tr.record(train[2], warmup=0, prev_batch=train[1])
        dumps.append(tr.dump_logits(splits, ema=True, recorded=recorded))
        tr.run_recorded(train[3])
        dumps.append(tr.dump_logits(splits, recorded=recorded))
        dumps.append(tr.dump_logits(splits, ema=True, recorded=recorded))
        tr.run_recorded(train[4])
        tr.train_step(train[5])
        dumps.append(tr.dump_logits(splits, ema=True, recorded=recorded))
        tr.opt.flush_tables()
        torch.cuda.synchronize()
        return tr, dumps, (tr.model._store.flat.detach().clone(), tr.ema.shadow.detach().clone())

    (te, de, fe), (tg, dg, fg) = run(False), run(True)
    assert tg._dump_rec["n_replays"] == 4 * N_FULL - 1 and te.__dict__.get("_dump_rec") is None
    for i, (a, b) in enumerate(zip(de, dg)):
        assert _same_store(a, b), i
    assert not _same_store(dg[1], dg[2]) and not _same_store(dg[0], dg[2])          # averaged != trained weights; the weights moved
    assert torch.equal(fe[0].view(torch.int32), fg[0].view(torch.int32)) and torch.equal(fe[1].view(torch.int32), fg[1].view(torch.int32))
    with pytest.raises(ValueError, match=r"dump_logits\(ema=True\) needs Trainer\(ema=...\)"):
        _trainer("id").dump_logits(splits, ema=True, recorded=True)


def test_refusals_name_what_is_wrong():
    _H()
    tr = _trainer("image")
    batch = _batches("image", 1)[0]
    who = r"dump_logits\(recorded=True\)"
    with pytest.raises(RuntimeError, match=who + r": batch\['time_ms'\] is missing; the store's writer reads the three key columns"):
        tr.dump_logits([[{k: v for k, v in batch.items() if k != "time_ms"}]], recorded=True)
    with pytest.raises(RuntimeError, match=who + r": batch\['photo_id'\] is \(48,\) torch.int64 on cpu"):
        tr.dump_logits([[dict(batch, photo_id=batch["photo_id"].cpu())]], recorded=True)
    nc = dict(batch, photo=batch["photo"].transpose(0, 1).contiguous().transpose(0, 1))
    with pytest.raises(RuntimeError, match=who + r": batch\['photo'\] is not contiguous"):
        tr.dump_logits([[batch, nc]], recorded=True)
    assert tr._dump_rec["n_replays"] == 0          # (the first batch was recorded before the second was looked at: batches stream)
    comm, tr.comm = tr.comm, types.SimpleNamespace(active=True)
    with pytest.raises(RuntimeError, match=who + r" is not supported under data parallelism \(an active DPComm\)"):
        tr.dump_logits([[batch]], recorded=True)
    tr.comm = comm
    lb = _trainer("image")
    lb.model.bias_weight = torch.nn.Parameter(torch.zeros(1, S, device=DEV))          # (only looked at, never run)
    with pytest.raises(RuntimeError, match=who + ": the model has a learnable position bias"):
        lb.dump_logits([[batch]], recorded=True)
    got = tr.dump_logits([[batch]], recorded=True)          # and the trainer goes on working
    assert tr._dump_rec["n_replays"] == 1 and np.isfinite(got._cat()[1].cpu().numpy()).all()
