"""The device logit store's host restatement (tests/store_ref.py) against what it replaces: LogitStore.weights on the reference
reader's fixture and on seeded random stores, the ClipRec fixture through the reference head, and the library's new exports."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import store_ref as R
from helpers import GOLDEN
from segmminterest_amd.bridge import LogitStore


def _host_store(batches, S):
    st = LogitStore(S=S)
    for b in batches or []:
        st.add_batch(*b)
    return st


def _ref_weights(clip, neg, user, item, time, id2user=None, id2item=None):
    """LogitStore.weights' answer from store_ref: (weights or None, miss)"""
    k, v = clip._cat()
    nk, nv = neg._cat() if neg is not None else (None, None)
    um, im = (R.dense_map(id2user) if id2user else None), (R.dense_map(id2item) if id2item else None)
    rowidx, miss = R.lookup(user, item, time, R.build_index(k), R.build_index(nk) if neg is not None else None, um, im)
    return R.weights(rowidx, v, nv, clip.S), miss


def _key_error_of(fn):
    with pytest.raises(KeyError) as e:
        fn()
    return e.value.args[0]


def reader_stores():
    d = json.load(open(os.path.join(GOLDEN, "io_reader.json")))

    def batch(m):
        ks = np.array([[int(x) for x in k.split("-")] for k in m], np.int64)
        return (ks[:, 0], ks[:, 1], ks[:, 2], np.array(list(m.values()), np.float32))
    return d["cases"], batch(d["clip_weight"]), batch(d["neg_weight"])


def test_reference_reproduces_logitstore_on_the_reader_fixture():
    cases, cb, nb = reader_stores()
    clip, neg = _host_store([cb], 40), _host_store([nb], 40)
    assert len(cases) == 8
    for c in cases:
        items = np.array([[c["item"]] + c["neg"]])
        maps = dict(id2user=c["id_maps"][0], id2item=c["id_maps"][1]) if c["id_maps"] else {}
        ng = neg if c["with_neg_file"] else None
        w, miss = _ref_weights(clip, ng, [c["user_id"]], items, [c["time"]], **maps)
        if c["error"]:
            assert miss[0] != R.MISS_NONE and miss[1] == R.MISS_NONE
            b, j = divmod(int(miss[0]), items.shape[1])
            msg = _key_error_of(lambda: clip.weights([c["user_id"]], items, [c["time"]], neg=ng, **maps))
            assert msg == "Inference, Key %d-%d-%d not found in clip_weight" % (c["user_id"], items[b, j], c["time"])
            continue
        assert miss.tolist() == [R.MISS_NONE] * 2
        want = clip.weights([c["user_id"]], items, [c["time"]], neg=ng, **maps).numpy()
        assert w.tobytes() == want.tobytes(), c


@pytest.mark.parametrize("seed,I,with_neg,drop", R.RANDOM_CASES)
def test_reference_reproduces_logitstore_on_random_stores(seed, I, with_neg, drop):
    c = R.random_case(seed, I, with_neg, drop_neg=drop)
    clip, neg = _host_store(c["batches"], 8), (_host_store(c["neg_batches"], 8) if with_neg else None)
    w, miss = _ref_weights(clip, neg, c["user"], c["item"], c["time"])
    first = clip._lookup(np.stack([c["user"], c["item"][:, 0], c["time"]], 1))
    assert (first >= 0).any() and (first < 0).sum() >= 2          # present and absent targets, duplicates among the stored keys
    assert len(clip.as_dict()) < len(clip._cat()[0])
    if drop:
        b, j = divmod(int(miss[0]), I)
        msg = _key_error_of(lambda: clip.weights(c["user"], c["item"], c["time"], neg=neg))
        assert msg == "Inference, Key %d-%d-%d not found in clip_weight" % (c["user"][b], c["item"][b, j], c["time"][b])
        return
    assert miss.tolist() == [R.MISS_NONE] * 2
    assert w.tobytes() == clip.weights(c["user"], c["item"], c["time"], neg=neg).numpy().tobytes()


def test_reference_flags_ids_outside_the_maps():
    c = R.random_case(3, 3, False)
    clip = _host_store(c["batches"], 8)
    k, _ = clip._cat()
    ident = np.arange(9, dtype=np.int64)
    im = ident.copy()
    im[c["item"][2, 1]] = -1                                   # a negative entry: item (2, 1) -- and whoever shares its id
    bad_items = np.argwhere(c["item"] == c["item"][2, 1])
    rowidx, miss = R.lookup(c["user"], c["item"], c["time"], R.build_index(k), None, np.arange(200, dtype=np.int64), im)
    assert miss[0] == R.MISS_NONE and miss[1] == bad_items[0][0] * 3 + bad_items[0][1]
    assert all(rowidx[b, j] == -1 for b, j in bad_items if j > 0)
    rowidx, miss = R.lookup(c["user"], c["item"], c["time"], R.build_index(k), None, ident, None)          # user 99 is outside [0, 9)
    assert miss[1] == 1 * 3 and (rowidx[1] == -1).all()
    with pytest.raises(KeyError):                              # LogitStore's dicts raise for the same ids
        clip.weights(c["user"], c["item"], c["time"], id2user={str(i): i for i in range(9)})


def test_cliprec_fixture_through_the_reference_head():
    """io_cliprec.npz with item 0 of each row in a target store and items 1, 2 in a negatives store (I = 3), within the 2e-5 of
    test_cliprec_fixture_is_the_weighted_masked_sum."""
    z = np.load(os.path.join(GOLDEN, "io_cliprec.npz"))
    cp, w, dur = z["clip_pred"], z["weight"], z["duration"]
    B, I, S = cp.shape
    assert I == 3
    vals, neg_vals = w[:, 0], w[:, 1:].reshape(-1, S)
    rowidx = np.stack([np.arange(B), -2 - 2 * np.arange(B), -2 - (2 * np.arange(B) + 1)], 1).astype(np.int32)
    ones = np.full((B, I), -1, np.int32)
    assert np.abs(R.head(cp, rowidx, vals, neg_vals, dur)[0] - z["pred_weighted_masked"]).max() <= 2e-5
    assert np.abs(R.head(cp, ones, vals, neg_vals, dur)[0] - z["pred_ones_masked"]).max() <= 2e-5
    assert np.abs(R.head(cp, rowidx, vals, neg_vals, None)[0] - z["pred_weighted_nomask"]).max() <= 2e-5
    g = np.random.RandomState(0).randn(B, I)
    mask = np.arange(S) < dur[..., None]
    assert np.array_equal(R.head_bwd(g, S, rowidx, vals, neg_vals, duration=dur), g[..., None] * w.astype(np.float64) * mask)


def test_library_exports_the_store_entry_points():
    from segmminterest_amd import _abi
    from segmminterest_amd import hipabi as H
    names = ("segmm_store_lookup", "segmm_store_head", "segmm_store_head_bwd")
    for n in names:
        assert n in _abi.PROTOTYPES and _abi.PROTOTYPES[n][-1] == ("stream", "p")
    L = ctypes.CDLL(H.LIB_PATH)
    for n in names:
        assert hasattr(L, n), n
    L.segmm_abi_version.restype = ctypes.c_int
    assert L.segmm_abi_version() == 30 == _abi.ABI_VERSION
    ops = {H.lib().segmm_cmd_op_name(i).decode() for i in range(H.lib().segmm_cmd_op_count())}
    assert set(names) <= ops          # flat arguments + a trailing stream: recordable like every other launch


def test_store_entry_points_refuse_bad_arguments_on_the_host():
    from segmminterest_amd import hipabi as H
    L = H.lib()
    assert L.segmm_store_head(None, None, None, 0, None, 0, None, 0, 0, None, None, None) != 0
    assert "store_head" in L.segmm_last_error().decode() and "S = 0" in L.segmm_last_error().decode()
    assert L.segmm_store_head_bwd(None, None, None, 0, None, 0, None, None, 0, 40, None, None) == 0          # rows == 0 launches nothing
    assert L.segmm_store_lookup(None, None, None, 0, 0, None, None, 0, None, None, -1, None, 0, None, 0, None, None, None) != 0
    assert "store_lookup" in L.segmm_last_error().decode()
    with pytest.raises(RuntimeError, match="device tensors"):
        H.store_head(torch.zeros(2, 3, 4), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(1, 4))
