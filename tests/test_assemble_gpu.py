"""segmm_assemble_rows and feature_store.DeviceBatches on the MI355X: every output bit for bit against the numpy restatement of the
header (tests/assemble_ref.py -- which tests/test_assemble_cpu.py ties to IndexBatchBuilder and the reference's own dataset rows),
the shuffle / sharding rules, and a training step + a recorded fit over device-assembled batches."""
import numpy as np
import pytest
import torch

import assemble_ref as R
from helpers import build_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 20240607
_cache = {}


def _fs():
    from segmminterest_amd import feature_store as FS, hipabi as H
    H.lib()
    return FS, H


def _check(table, ids, S, Lt, seed, what=""):
    """Kernel == reference for the rows ``ids`` of the (host) table; returns the device outputs as numpy."""
    FS, H = _fs()
    dev = _cache.get(id(table))
    if dev is None:
        dev = _cache[id(table)] = (table, table.to(DEV))          # (keeps the host table alive: its id is the key)
    got = H.assemble_rows(dev[1].descriptor(), torch.tensor(list(ids), dtype=torch.int64, device=DEV), S, Lt, seed, FS.SITE_ASSEMBLE)
    got = [g.cpu().numpy() for g in got]
    ref = R.assemble(table, ids, S, Lt, seed, FS.SITE_ASSEMBLE)
    for name, g, r in zip(("photo_idx", "user_idx", "label", "cols"), got, ref):
        assert g.shape == r.shape and g.dtype == r.dtype == np.int64 and (g == r).all(), (what, name, np.argwhere(g != r)[:4])
    return got


def _fixture_table():
    FS, _ = _fs()
    if "fixture" not in _cache:
        _, rows, b = R.fixture()
        _cache["fixture"] = FS.InteractionTable.compile(b, rows)
    return _cache["fixture"]


@pytest.mark.parametrize("ids", [[3], [0, 1, 2, 3, 4], [0, 1, 3, 1, 3, 9, 4]])
def test_fixture_rows_bitwise(ids):
    """S = 40, Lt = 100 on the reference's fixture: B = 1, 5 and 7 (two repeated row ids, one out of range)."""
    photo, user, label, cols = _check(_fixture_table(), ids, 40, 100, SEED, "fixture")
    for b, r in enumerate(ids):
        if r == 9:
            assert (photo[b] == -1).all() and (user[b] == -1).all() and (label[b] == -2).all() and (cols[:, b] == 0).all()
        if r == 3:
            assert (user[b] >= 0).all() and len(set(photo[b][photo[b] >= 0].tolist())) == 4


def _synthetic(counts):
    FS, _ = _fs()
    key = ("syn",) + tuple(counts)
    if key not in _cache:
        _cache[key] = FS.InteractionTable.compile(R.synthetic_builder(3, 5), R.synthetic_rows(counts))
    return _cache[key]


@pytest.mark.parametrize("counts,instance", [((0, 5, 6, 64, 65, 1024), 1024), ((0, 5, 6, 64, 65, 1024, 1025, 4096), 4096)])
def test_synthetic_table_bitwise(counts, instance):
    """S = 3, Lt = 5: video frame counts 0, 1, 3, 4; user candidate counts 0, Lt, Lt + 1, 64, 65, the 1024-candidate instance's
    boundary, one past it (the 4096 instance) and the limit; a hole at frame 0, an unresolvable own frame, an empty history, a
    history switched off by history_lengths == 0; B not a multiple of the rows per workgroup (4 / 2)."""
    t = _synthetic(counts)
    assert t.max_cand == counts[-1] and (t.max_cand <= 1024) == (instance == 1024)
    n = t.n_rows
    assert t.row_info[:n, 1].tolist()[:4] == [0, 1, 3, 4] and n == len(counts) + 4
    ids = list(range(n)) + [n - 3]
    assert len(ids) % 4 and len(ids) % 2
    photo, user, _, _ = _check(t, ids, 3, 5, SEED, "synthetic")
    k = len(counts)
    assert (user[0] == -1).all() and (user[1] >= 0).all() and (photo[0] == -1).all() and (photo[3] >= 0).all()
    assert (user[k] >= 0).all() and (user[k + 1] >= 0).all() and (user[k + 2] >= 0).sum() == 4 and (user[k + 3] == -1).all()
    _check(t, ids[::-1], 3, 5, SEED + 1, "synthetic, another seed and order")


def test_history_longer_than_the_item_and_foreign_indices_bitwise():
    """A hand-edited table: watched-frame counts beyond the item's length are cut to it, an item / user index outside the table
    contributes nothing (the reference restates both; the compiled tables of the other tests never contain them)."""
    FS, _ = _fs()
    t0 = _synthetic((0, 5, 6, 64, 65, 1024))
    t = FS.InteractionTable().load_state_dict({k: (v.clone() if torch.is_tensor(v) else dict(v)) for k, v in t0.state_dict().items()})
    k = 6
    h0 = int(t.hist_ptr[k])
    assert t.hist_pair[h0].tolist()[1] == 6
    t.hist_pair[h0, 1] += 1000          # item 200 has 6 frames in the table
    t.hist_pair[h0 + 1, 1] = 7          # item 300: 2
    t.row_info[2, 1] = 9                # a video of "9 frames" whose item has 4
    photo, user, _, _ = _check(t, range(t.n_rows), 3, 5, SEED, "cut to the item's length")
    ref = _check(t0, range(t0.n_rows), 3, 5, SEED, "compiled")
    assert (user[k] == ref[1][k]).all() and (photo[2] >= 0).all()


def test_rows_do_not_depend_on_the_batch_and_undrawn_rows_not_on_the_seed():
    t = _fixture_table()
    together = _check(t, [3, 1, 0], 40, 100, SEED)
    for b, r in enumerate([3, 1, 0]):
        alone = _check(t, [r], 40, 100, SEED)
        assert all((alone[i][0] == together[i][b]).all() for i in range(3)) and (alone[3][:, 0] == together[3][:, b]).all(), r
    other = _check(t, [3, 1, 0], 40, 100, SEED + 12345)
    assert (other[1][0] != together[1][0]).any() and (other[0][1] != together[0][1]).any()          # rows 3 (user) and 1 (video) are drawn
    assert (other[0][2] == together[0][2]).all() and (other[1][2] == together[1][2]).all() and (other[0][0] == together[0][0]).all()


def test_device_draws_are_uniform():
    """The statistic of tests/test_assemble_cpu.py on the device's output (4096 rows share 8 candidates, cap 3, all counts within
    5 sd); the output equals the reference's bit for bit, so this passes where that did."""
    t = R.shared_candidates_table()
    _, user, _, _ = _check(t, range(4096), 1, 3, SEED, "shared candidates")
    R.uniformity(user)


def test_live_seed_is_refused():
    FS, H = _fs()
    t = _fixture_table().to(DEV)
    with pytest.raises(RuntimeError, match="assemble_rows.*bit 63"):
        H.assemble_rows(t.descriptor(), torch.zeros(2, dtype=torch.int64, device=DEV), 40, 100, H.LIVE_SEED | 3, FS.SITE_ASSEMBLE)


def test_device_batches_shuffle_and_shards():
    FS, _ = _fs()
    big = R.shared_candidates_table(9000).to(DEV)          # more than one workgroup's sort
    db = [FS.DeviceBatches(big, 16, 1, 3, seed=5, rank=r, world=4) for r in range(4)]
    p0, p1 = db[0].permutation(0), db[0].permutation(1)
    assert p0.dtype == torch.int64 and sorted(p0.tolist()) == list(range(9000)) and sorted(p1.tolist()) == list(range(9000))
    assert not torch.equal(p0, p1) and p0.tolist() != list(range(9000))
    assert all(torch.equal(d.permutation(0), p0) and torch.equal(d.permutation(1), p1) for d in db[1:])
    assert not torch.equal(FS.DeviceBatches(big, 16, 1, 3, seed=6).permutation(0), p0)
    assert torch.equal(FS.DeviceBatches(big, 16, 1, 3, shuffle=False).permutation(3), torch.arange(9000, device=DEV))
    # 100 rows whose time_ms column is the row number: which rows a rank's batch carries is readable from the batch
    _, rows, b = R.fixture()
    t = FS.InteractionTable.compile(b, [dict(rows[k % 5], time_ms=k) for k in range(100)]).to(DEV)
    for drop_last in (False, True):
        dbs = [FS.DeviceBatches(t, 8, 40, 100, seed=9, rank=r, world=4, drop_last=drop_last) for r in range(4)]
        perm = dbs[0].permutation(2).tolist()
        its = [list(d(2)) for d in dbs]
        assert all(len(x) == len(dbs[0]) == (3 if drop_last else 4) for x in its)
        for k in range(len(dbs[0])):
            shards = [its[r][k]["time_ms"].tolist() for r in range(4)]
            want = perm[32 * k:32 * (k + 1)]
            assert sum(shards, []) == want and [len(s) for s in shards] == ([8] * 4 if k < 3 else [1] * 4)
    one = FS.DeviceBatches(t, 8, 40, 100, shuffle=False)
    batches = list(one(0))
    assert [x["time_ms"].tolist() for x in batches] == [list(range(8 * k, min(8 * k + 8, 100))) for k in range(13)]
    bt = batches[-1]
    assert set(bt) == {"photo_idx", "user_idx", "photo_mask", "user_mask", "label", "photo_id", "photo_identity_id", "user_id", "user_identity_id",
                       "time_ms", "play_time", "duration"}
    assert all(v.is_cuda and v.is_contiguous() and v.shape[0] == 4 for v in bt.values())
    assert bt["photo_mask"].dtype == torch.bool and torch.equal(bt["user_mask"], bt["user_idx"] >= 0)
    # a row is resampled each epoch, identically on every rank
    e0, e1 = next(iter(dbs[0](0))), next(iter(FS.DeviceBatches(t, 8, 40, 100, seed=9, rank=2, world=4)(0)))
    again = FS.DeviceBatches(t, 100, 40, 100, shuffle=False, seed=9)
    a0, a1 = next(iter(again(0))), next(iter(again(1)))
    assert not torch.equal(a0["user_idx"][3], a1["user_idx"][3]) and torch.equal(a0["user_idx"][0], a1["user_idx"][0])
    for x in (e0, e1):          # whichever rank assembles row r in epoch 0 draws what the single-process loader drew
        for j, r in enumerate(x["time_ms"].tolist()):
            assert torch.equal(x["user_idx"][j], a0["user_idx"][r]) and torch.equal(x["photo_idx"][j], a0["photo_idx"][r])


# ------------------------------------------------------------------------------------------------ end to end, image mode
S_E, LT_E, D_E, B_E = 8, 10, 32, 8


def _dataset():
    """32 interactions over 12 items (3 .. 12 frames: some videos longer than S = 8) and 6 users (histories of 0 .. 3 items +
    1 .. 3 own frames: some user lists longer than Lt = 10); the features are a random [n_lines, 32] table."""
    FS, _ = _fs()
    g = np.random.RandomState(7)
    n_fr = {100 + i: int(g.randint(3, 13)) for i in range(12)}
    keys = ["%d-%d" % (p, f) for p, n in n_fr.items() for f in range(n) if not (p == 103 and f == 1)]          # one hole
    uid = {str(u): ["%d_%d" % (100 + int(g.randint(12)), 0) for _ in range(int(g.randint(1, 4)))] for u in range(1, 7)}
    b = FS.IndexBatchBuilder(FS.KeyIndex(keys), uid, {u: int(u) for u in uid}, {str(p): p - 99 for p in n_fr}, S=S_E, Lt=LT_E)
    rows = []
    for k in range(32):
        p = 100 + int(g.randint(12))
        if p == 103:
            p = 104
        n = n_fr[p]
        v = int(g.randint(0, n))
        hist = [100 + int(x) for x in g.randint(0, 12, size=int(g.randint(0, 4)))]
        rows.append(dict(user_id=1 + int(g.randint(6)), video_id=p, time_ms=k, duration_ms=5000 * n, playing_time=5000 * v,
                         label_1D=[1] * v + [0] + [-1] * (n - v - 1), history_items=hist, history_playing=[5000 * int(g.randint(1, 13)) for _ in hist]))
    table = FS.InteractionTable.compile(b, rows)
    feats = torch.rand(len(keys), D_E, generator=torch.Generator().manual_seed(3))
    return table, feats


def _trainer(feats, **kw):
    from segmminterest_amd.feature_store import ResidentFeatureTable
    from segmminterest_amd.trainer import Trainer
    cfg = dict(N=2, h=4, S=S_E, d=32, D_in=D_E, Lt=LT_E, user="image", photo="image", loss_type_list=["interestBPR"],
               loss_weight={"interestBPR": 1.0, "mse": 1.0}, exposure_prob=[1.0] * S_E)
    torch.manual_seed(5)
    model = build_model(cfg).cuda()
    torch.manual_seed(11)
    return model, Trainer(model, lr=1e-3, feature_table=ResidentFeatureTable(feats.to(DEV)), **kw)


def test_train_step_on_a_device_batch_equals_the_host_built_batch():
    FS, _ = _fs()
    table, feats = _dataset()
    assert table.max_cand > LT_E and int(table.row_info[:32, 1].max()) > S_E          # both draws occur
    db = FS.DeviceBatches(table.to(DEV), B_E, S_E, LT_E, seed=3, drop_last=True)
    batch = next(iter(db(0)))
    assert (batch["user_mask"].sum(1) == LT_E).any() and (batch["photo_mask"].sum(1) == S_E).any()
    host = {k: v.cpu().clone() for k, v in batch.items() if not k.endswith("_mask")}
    host["photo_mask"], host["user_mask"] = host["photo_idx"] >= 0, host["user_idx"] >= 0
    res = []
    for b in (batch, {k: v.to(DEV) for k, v in host.items()}):
        model, tr = _trainer(feats, dropout=False)
        out = [tr.train_step(b)["loss"].detach().clone() for _ in range(2)]
        res.append((out, model._store.flat.detach().clone()))
    assert all(torch.equal(a, b) for a, b in zip(res[0][0], res[1][0])) and torch.isfinite(res[0][0][1])
    assert torch.equal(res[0][1], res[1][1])


def test_fit_recorded_over_device_batches_equals_eager_fit():
    FS, _ = _fs()
    table, feats = _dataset()
    dev = table.to(DEV)
    valid = list(FS.DeviceBatches(dev, 16, S_E, LT_E, shuffle=False)(0))
    ends = {}
    for mode in ("eager", "recorded"):
        model, tr = _trainer(feats, device_state=True)
        db = FS.DeviceBatches(dev, B_E, S_E, LT_E, seed=3, drop_last=True)
        hist = tr.fit(db, valid, epochs=2, valid_step=100, permutation=0, recorded=(mode == "recorded"))
        assert hist["global_step"] == 8
        if mode == "recorded":
            assert tr.__dict__.get("_recorded") is not None
        ends[mode] = model._store.flat.detach().clone()
    assert torch.equal(ends["eager"], ends["recorded"]) and torch.isfinite(ends["eager"]).all()
