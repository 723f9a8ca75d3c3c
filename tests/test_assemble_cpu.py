"""Index batches from a compiled interaction table, without a GPU: InteractionTable.compile + the numpy restatement of
segmm_assemble_rows (tests/assemble_ref.py) against IndexBatchBuilder on the fixture the reference's own ``_getitem`` wrote
(tests/golden/io_dataloader.npz), the compile-time refusals, the uniformity of the reference's draws at a fixed seed, and the
argument checks of the C entry point (every call below fails its check before anything is launched)."""
import collections
import ctypes
import random

import numpy as np
import pytest
import torch

import assemble_ref as R
from segmminterest_amd.feature_store import SITE_ASSEMBLE, DeviceBatches, IndexBatchBuilder, InteractionTable

SEED = 20240607
COLS = ("photo_id", "photo_identity_id", "user_id", "user_identity_id", "time_ms", "play_time", "duration")
_cache = {}


def _fixture():
    if not _cache:
        z, rows, b = R.fixture()
        random.seed(int(z["seed"]))                  # init_seed of the reference (dataloader_SegMM.py:31-38)
        np.random.seed(int(z["seed"]))
        host = b.batch([b.row(r["user_id"], r["video_id"], r["time_ms"], r["duration_ms"], r["playing_time_x"], r["label_1D"],
                              r["history_items"], r["history_playing"], r["history_lengths"]) for r in rows])
        table = InteractionTable.compile(b, rows)
        _cache.update(z=z, rows=rows, b=b, host=host, table=table, ref=R.assemble(table, range(5), 40, 100, SEED, SITE_ASSEMBLE))
    return _cache


def test_compiled_table_layout():
    t = _fixture()["table"]
    assert (t.S, t.n_rows, t.n_users) == (40, 5, 4) and t.max_cand == 197
    assert t.item_ptr.dtype == t.own_ptr.dtype == t.hist_ptr.dtype == t.row_cols.dtype == torch.int64
    assert t.item_line.dtype == t.own_line.dtype == t.hist_pair.dtype == t.row_info.dtype == torch.int32 and t.label.dtype == torch.int8
    assert t.item_ptr.numel() == t.n_items + 1 and t.own_ptr.numel() == t.n_users + 1 and t.hist_ptr.tolist() == [0, 3, 3, 5, 33, 34]
    assert t.row_info[:5, 1].tolist() == [10, 47, 40, 4, 8] and int(t.row_info[0, 2]) == int(t.row_info[4, 2])      # the same user
    assert (t.own_line[:int(t.own_ptr[-1])] >= 0).all() and (t.item_line[:int(t.item_ptr[-1])] < 0).any()          # holes stay, in items only
    f = _fixture()
    own = lambda r: int(t.own_ptr[int(t.row_info[r, 2]) + 1] - t.own_ptr[int(t.row_info[r, 2])])
    assert all(own(r) < len(f["b"].user_input_dict[str(f["rows"][r]["user_id"])]) for r in (0, 2, 4))          # an unresolvable own frame each
    t2 = InteractionTable().load_state_dict(t.state_dict())
    assert all(torch.equal(getattr(t, k), getattr(t2, k)) for k in t.TENSORS) and (t2.S, t2.n_rows, t2.max_cand) == (40, 5, 197)


def test_undrawn_fixture_rows_equal_the_index_batch_builder_and_the_reference_dataset():
    f = _fixture()
    z, host, (photo, user, label, cols) = f["z"], f["host"], f["ref"]
    t = R.as_numpy(f["table"])
    table = torch.from_numpy(z["table"])
    counts = {r: tuple(len(c) for c in R.candidates(t, r)) for r in range(5)}
    assert (counts[0], counts[2], counts[3], counts[4]) == ((10, 9), (40, 6), (4, 197), (8, 4)) and counts[1][0] == 47 and counts[1][1] <= 100
    holes = lambda r: sum(int((t["item_line"][t["item_ptr"][i]:t["item_ptr"][i] + nf] < 0).sum()) for i, nf in t["hist_pair"][t["hist_ptr"][r]:t["hist_ptr"][r + 1]])
    assert holes(0) > 0 and holes(2) > 0          # rows 0 and 2 carry a history hole
    for r in (0, 2, 4):                           # no draw: 10 / 40 / 8 video frames <= 40, 9 / 6 / 4 user candidates <= 100
        assert photo[r].tolist() == host["photo_idx"][r].tolist() and user[r].tolist() == host["user_idx"][r].tolist(), r
        assert label[r].tolist() == host["label"][r].tolist(), r
        for key, idx, exp_f, exp_m in (("photo", photo, "exp_photo", "exp_photo_mask"), ("user", user, "exp_user", "exp_user_mask")):
            i = torch.from_numpy(idx[r])
            got = torch.where((i >= 0)[..., None], table[i.clamp(min=0)], torch.zeros(()))
            assert torch.equal(got, torch.from_numpy(z[exp_f][r])), (key, r)
            assert torch.equal(i >= 0, torch.from_numpy(z[exp_m][r])), (key, r)
        assert label[r].tolist() == z["exp_label"][r].astype(np.int64).tolist()
        for k, name in enumerate(COLS):
            assert int(cols[k, r]) == int(z["exp_" + name][r]) == int(host[name][r]), (name, r)


def test_drawn_fixture_rows_are_subsets_in_random_order():
    f = _fixture()
    photo, user, label, _ = f["ref"]
    t, rows, b = R.as_numpy(f["table"]), f["rows"], f["b"]
    video, _ = R.candidates(t, 1)                 # row 1: 47 video frames, S = 40
    assert len(video) == 47 and video == [b.line["105-%d" % k] for k in range(47)]
    got = photo[1].tolist()
    assert len(set(got)) == 40 and set(got) <= set(video) and got != sorted(got)
    assert label[1].tolist() == b._ints(rows[1]["label_1D"])[:40] == f["host"]["label"][1].tolist()
    r3 = rows[3]                                  # row 3: 197 user candidates, Lt = 100; the candidate list from the builder itself
    wide = IndexBatchBuilder(b.line, b.user_input_dict, b.user2id, b.item2id, S=40, Lt=4096)
    cand = wide.row(r3["user_id"], r3["video_id"], r3["time_ms"], r3["duration_ms"], r3["playing_time_x"], r3["label_1D"], r3["history_items"],
                    r3["history_playing"], r3["history_lengths"])["user_idx"]
    cand = cand[cand >= 0].tolist()
    assert len(cand) == 197 and cand == R.candidates(t, 3)[1]
    got = user[3].tolist()
    assert min(got) >= 0 and not (collections.Counter(got) - collections.Counter(cand))          # taken by position: a sub-multiset
    k = R.keys(SEED, SITE_ASSEMBLE, 3, R.STREAM_USER, 197)
    pos = sorted(range(197), key=lambda j: (int(k[j]), j))[:100]
    assert len(set(pos)) == 100 and got == [cand[j] for j in pos] and pos != sorted(pos)
    assert photo[3].tolist() == f["host"]["photo_idx"][3].tolist()                               # 4 frames: no draw on the video side


def test_draw_depends_on_seed_site_and_row_only():
    t = _fixture()["table"]
    a = R.assemble(t, [3, 1, 7, 1, -1], 40, 100, SEED, SITE_ASSEMBLE)
    ref = _fixture()["ref"]
    assert (a[0][1] == ref[0][1]).all() and (a[0][3] == a[0][1]).all() and (a[1][0] == ref[1][3]).all()
    for b in (2, 4):                              # out-of-range row ids: all padding
        assert (a[0][b] == -1).all() and (a[1][b] == -1).all() and (a[2][b] == -2).all() and (a[3][:, b] == 0).all()
    other = R.assemble(t, range(5), 40, 100, SEED + 1, SITE_ASSEMBLE)
    assert (other[0][1] != ref[0][1]).any() and (other[1][3] != ref[1][3]).any()
    for r in (0, 2, 4):
        assert (other[0][r] == ref[0][r]).all() and (other[1][r] == ref[1][r]).all()
    hi = R.assemble(t, [1], 40, 100, SEED + (1 << 40), SITE_ASSEMBLE)          # the high seed word matters too
    assert (hi[0][0] != ref[0][1]).any()


def test_compile_refuses_a_missing_video_frame_and_a_row_over_the_candidate_limit():
    f = _fixture()
    bad = dict(f["rows"][0], video_id=110, duration_ms=14000)          # frame 110-2 is not in the line map
    with pytest.raises(ValueError, match="No key in lineid dict: 110-2"):
        InteractionTable.compile(f["b"], [f["rows"][0], bad])
    b = R.synthetic_builder(3, 5, big=4100)
    ok = R.synthetic_rows([4096])
    assert InteractionTable.compile(b, ok).max_cand == 4096
    with pytest.raises(ValueError, match=r"row 1 has 1 video frames and 4097 user candidates.*SEGMM_ASSEMBLE_MAX_CAND = 4096"):
        InteractionTable.compile(b, R.synthetic_rows([5, 4097]))
    with pytest.raises(ValueError, match="S = 3"):
        DeviceBatches(InteractionTable.compile(b, ok), 4, 40, 5)


def test_rows_as_tuples_and_dicts_compile_alike():
    f = _fixture()
    tup = [(r["user_id"], r["video_id"], r["time_ms"], r["duration_ms"], r["playing_time_x"], r["label_1D"], r["history_items"],
            r["history_playing"], r["history_lengths"]) for r in f["rows"]]
    t2 = InteractionTable.compile(f["b"], tup)
    assert all(torch.equal(getattr(f["table"], k), getattr(t2, k)) for k in t2.TENSORS)


def test_reference_draws_are_uniform_at_the_committed_seed():
    """4096 rows share 8 candidates, cap 3: selection counts ~ Binomial(4096, 3/8) (sd 31.0), (candidate, position) counts ~
    Binomial(4096, 1/8) (sd 21.2); all 8 + 24 counts within 5 sd.  Fixed seed: deterministic.  (At SEED the reference's worst
    deviations are the two figures the helper prints.)"""
    u = np.stack([R.draw(np.arange(8), 3, SEED, SITE_ASSEMBLE, r, R.STREAM_USER) for r in range(4096)])
    R.uniformity(u)
    t = R.shared_candidates_table()
    assert (R.assemble(t, range(4096), 1, 3, SEED, SITE_ASSEMBLE)[1] == u).all()          # the table of the GPU test draws the same


# ---- the C entry point's argument checks (no launch)
def _lib():
    from segmminterest_amd import hipabi
    return hipabi, hipabi.lib()


def _call(L, H, table=True, S=40, Lt=100, seed=1, null=None):
    desc = H.ITable()                                # all-null descriptor: only reached after the scalar checks
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)                        # never dereferenced
    a = dict(row_ids=p, photo_idx=p, user_idx=p, label=p, cols=p)
    if null:
        a[null] = None
    rc = L.segmm_assemble_rows(ctypes.addressof(desc) if table else None, a["row_ids"], 4, S, Lt, seed, 1, a["photo_idx"], a["user_idx"], a["label"],
                               a["cols"], None)
    assert rc != 0
    return L.segmm_last_error().decode()


def test_assemble_rows_argument_checks_name_the_entry_point_and_the_limit():
    H, L = _lib()
    assert H.ASSEMBLE_MAX_CAND == 4096 and len(H.SIGNATURES["segmm_assemble_rows"]) == 12
    assert [n for n, _ in H.ITable._fields_][:3] == ["item_ptr", "item_line", "own_ptr"] and ctypes.sizeof(H.ITable) == 9 * 8 + 8 + 4 * 4
    for null in (None, "row_ids", "photo_idx", "user_idx", "label", "cols"):
        msg = _call(L, H, table=null is not None, null=null)
        assert "assemble_rows" in msg and "null pointer" in msg
    for S in (0, 257):
        msg = _call(L, H, S=S)
        assert "assemble_rows" in msg and "S = %d" % S in msg and "256" in msg
    for Lt in (0, 4097):
        msg = _call(L, H, Lt=Lt)
        assert "assemble_rows" in msg and "Lt = %d" % Lt in msg and "4096" in msg
    msg = _call(L, H, seed=(1 << 63) | 5)
    assert "assemble_rows" in msg and "bit 63" in msg and "step state" in msg
    assert "table descriptor" in _call(L, H)          # every scalar accepted: the empty descriptor is refused next
