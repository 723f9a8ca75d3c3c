"""The device-resident logit store on the MI355X: segmm_store_lookup's row indices and miss slots against tests/store_ref.py,
DeviceLogitStore.weights bit for bit against LogitStore.weights, segmm_store_head / _bwd against float64 and the ClipRec fixture,
the differentiable heads, and Trainer.dump_logits against the host store filled batch by batch."""
import json
import os

import numpy as np
import pytest
import torch

import store_ref as R
from helpers import GOLDEN
from segmminterest_amd.bridge import DeviceLogitStore, LogitStore, weighted_head

pytestmark = pytest.mark.gpu
DEV = "cuda"
T0 = 10 ** 12


def _H():
    from segmminterest_amd import hipabi
    hipabi.lib()
    return hipabi


def _stores(batches, S):
    """(DeviceLogitStore, LogitStore) fed the same batches, the device one from device tensors"""
    d, h = DeviceLogitStore(S=S, device=DEV), LogitStore(S=S)
    for b in batches or []:
        d.add_batch(*(torch.as_tensor(x).to(DEV) for x in b))
        h.add_batch(*b)
    return d, h


def _all_keys(batches):
    return np.concatenate([np.stack(b[:3], 1) for b in batches], 0) if batches else np.zeros((0, 3), np.int64)


def _key_error_of(fn):
    with pytest.raises(KeyError) as e:
        fn()
    return e.value.args[0]


def _bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


# ------------------------------------------------------------------ lookup
def _keyset(n, S=4):
    """n distinct keys in two batches plus re-added ones (the last occurrence wins): times near 10^12, neighbours that differ only
    in the first word (same item and time, users u and u + 1) and only in the third (same user and item, times t and t + 1)."""
    g = np.random.RandomState(100 + n)
    if n <= 3:
        ks = np.array([(5, 7, T0 + 1), (6, 7, T0 + 1), (6, 7, T0 + 2)][:n], np.int64).reshape(-1, 3)
    else:
        flat = g.choice(40 * 30 * 4, n, replace=False)
        ks = np.stack([1 + flat // 120, 1 + (flat // 4) % 30, T0 + flat % 4], 1).astype(np.int64)
    ks = ks[g.permutation(n)]
    h = n // 2
    batches = [tuple(ks[a:b, c].copy() for c in range(3)) + (g.randn(b - a, S).astype(np.float32),) for a, b in ((0, h), (h, n)) if b > a]
    if n:
        again = ks[g.randint(0, n, min(n, 5))]
        batches.append(tuple(again[:, c].copy() for c in range(3)) + (g.randn(len(again), S).astype(np.float32),))
    return batches


def _queries(batches, I, seed):
    """five query rows: the first key, the last key, one below the first, one above the last, one between two neighbours"""
    g = np.random.RandomState(seed)
    ks = R.build_index(_all_keys(batches))[0]
    if len(ks):
        mid = ks[len(ks) // 2]
        q = np.array([ks[0], ks[-1], (ks[0, 0] - 1, ks[0, 1], ks[0, 2]), (ks[-1, 0], ks[-1, 1], ks[-1, 2] + 1), (mid[0], mid[1], mid[2] + 10)], np.int64)
    else:
        q = np.array([(5, 7, T0 + k) for k in range(5)], np.int64)
    item = g.randint(1, 31, (5, I)).astype(np.int64)
    item[:, 0] = q[:, 1]
    return q[:, 0].copy(), item, q[:, 2].copy()


@pytest.mark.parametrize("n", [0, 1, 2, 3, 1000])
def test_lookup_equals_the_reference(n):
    batches = _keyset(n)
    dev, host = _stores(batches, 4)
    index = R.build_index(_all_keys(batches))
    assert len(index[0]) == n
    for I in (1, 2, 3, 70):
        user, item, time = _queries(batches, I, seed=n + I)
        # a negatives store that answers every (user, item j, time) of the batch -- without and with the last item of row 1
        nq = np.array([(user[b], item[b, j], time[b]) for b in range(5) for j in range(1, I)], np.int64).reshape(-1, 3)
        for drop in (False, True):
            if drop:
                nq = nq[~((nq == (user[1], item[1, -1], time[1])).all(1))]
            nb = [(nq[:, 0], nq[:, 1], nq[:, 2], np.zeros((len(nq), 4), np.float32))] if len(nq) else []
            ndev, nhost = _stores(nb, 4)
            nindex = R.build_index(nq)
            for neg, ni in ((None, None), (ndev, nindex)):
                for rows in ([slice(0, 5)] + [slice(b, b + 1) for b in range(5)]):          # B = 5 and B = 1
                    u, it, t = user[rows], item[rows], time[rows]
                    want, wmiss = R.lookup(u, it, t, index, ni)
                    got, miss = dev.lookup(u, it, t, neg=neg, check=False)
                    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (n, I, drop, rows)
                    assert miss.cpu().numpy().tolist() == wmiss.tolist(), (n, I, drop, rows)
                    if I == 2:          # the reference's len(item_ids) > 2: a negatives file is ignored
                        assert (want == want[:, :1]).all() and wmiss[0] == R.MISS_NONE
                    if wmiss[0] != R.MISS_NONE:
                        assert (_key_error_of(lambda: dev.lookup(u, it, t, neg=neg))
                                == _key_error_of(lambda: host.weights(u, it, t, neg=nhost)))
    if n >= 1:          # the first and the last key are found, the last added duplicate is the row that answers
        user, item, time = _queries(batches, 1, seed=0)
        r = dev.lookup(user, item, time).cpu().numpy()[:, 0]
        assert r[0] >= 0 and r[1] >= 0 and (r[2:] == -1).all()
        k = _all_keys(batches)
        assert (k[r[0]] == index[0][0]).all() and r[0] == max(i for i in range(len(k)) if (k[i] == index[0][0]).all())


def test_lookup_of_rows_of_300_items():
    """I > 128 takes the 256-thread workgroup, every thread more than one item: with and without a negatives index (one of its keys
    missing) and an item map with holes."""
    batches = _keyset(1000)
    dev, _ = _stores(batches, 4)
    index = R.build_index(_all_keys(batches))
    for I in (129, 300, 700):
        user, item, time = _queries(batches, I, seed=I)
        nq = np.array([(user[b], item[b, j], time[b]) for b in range(5) for j in range(1, I) if (b, item[b, j]) != (1, 5)], np.int64)          # row 1 misses item 5
        ndev, _ = _stores([(nq[:, 0], nq[:, 1], nq[:, 2], np.zeros((len(nq), 4), np.float32))], 4)
        im = np.arange(31, dtype=np.int64)
        im[[3, 17]] = -1
        for neg, ni in ((None, None), (ndev, R.build_index(nq))):
            for imap in (None, im):
                want, wmiss = R.lookup(user, item, time, index, ni, None, imap)
                got, miss = dev.lookup(user, item, time, neg=neg, check=False, id2item=None if imap is None else torch.from_numpy(imap).to(DEV))
                assert np.array_equal(got.cpu().numpy(), want) and miss.cpu().numpy().tolist() == wmiss.tolist(), (I, neg is None, imap is None)
        assert wmiss[0] != R.MISS_NONE and wmiss[1] != R.MISS_NONE and (want[:2] <= -2).any()


def test_lookup_with_dense_id_maps():
    c = R.random_case(3, 3, True)
    dev, host = _stores(c["batches"], 8)
    ndev, nhost = _stores(c["neg_batches"], 8)
    index, nindex = R.build_index(_all_keys(c["batches"])), R.build_index(_all_keys(c["neg_batches"]))
    ident = {str(i): i for i in range(9)}                     # user 99 of row 1 is outside it
    shifted = {str(i): i for i in range(9) if i != int(c["item"][2, 1])}          # no entry = a negative entry of the dense map
    for id2user, id2item in ((ident, None), (None, shifted), (ident, shifted), ({str(i): i for i in range(200)}, ident)):
        um = R.dense_map(id2user) if id2user else None
        im = R.dense_map(id2item) if id2item else None
        for neg, ni, nh in ((None, None, None), (ndev, nindex, nhost)):
            want, wmiss = R.lookup(c["user"], c["item"], c["time"], index, ni, um, im)
            got, miss = dev.lookup(c["user"], c["item"], c["time"], neg=neg, id2user=id2user, id2item=id2item, check=False)
            assert np.array_equal(got.cpu().numpy(), want) and miss.cpu().numpy().tolist() == wmiss.tolist()
            # the maps as device tensors give the same answer
            got2, miss2 = dev.lookup(c["user"], c["item"], c["time"], neg=neg, check=False,
                                     id2user=None if um is None else torch.from_numpy(um).to(DEV),
                                     id2item=None if im is None else torch.from_numpy(im).to(DEV))
            assert torch.equal(got, got2) and torch.equal(miss, miss2)
            if wmiss[1] != R.MISS_NONE:
                assert (_key_error_of(lambda: dev.lookup(c["user"], c["item"], c["time"], neg=neg, id2user=id2user, id2item=id2item))
                        == _key_error_of(lambda: host.weights(c["user"], c["item"], c["time"], neg=nh, id2user=id2user, id2item=id2item)))
            else:
                assert torch.equal(dev.lookup(c["user"], c["item"], c["time"], neg=neg, id2user=id2user, id2item=id2item), got)
    assert len(dev._maps) == 3          # the dicts were converted once each


# ------------------------------------------------------------------ materialised weights
def test_weights_are_logitstore_weights_on_the_reader_fixture():
    d = json.load(open(os.path.join(GOLDEN, "io_reader.json")))

    def batch(m):
        ks = np.array([[int(x) for x in k.split("-")] for k in m], np.int64)
        return (ks[:, 0], ks[:, 1], ks[:, 2], np.array(list(m.values()), np.float32))
    (clip, hclip), (neg, hneg) = _stores([batch(d["clip_weight"])], 40), _stores([batch(d["neg_weight"])], 40)
    assert len(d["cases"]) == 8
    for c in d["cases"]:
        items = np.array([[c["item"]] + c["neg"]])
        maps = dict(id2user=c["id_maps"][0], id2item=c["id_maps"][1]) if c["id_maps"] else {}
        args = ([c["user_id"]], items, [c["time"]])
        if c["error"]:
            assert (_key_error_of(lambda: clip.weights(*args, neg=neg if c["with_neg_file"] else None, **maps))
                    == _key_error_of(lambda: hclip.weights(*args, neg=hneg if c["with_neg_file"] else None, **maps)))
            continue
        got = clip.weights(*args, neg=neg if c["with_neg_file"] else None, **maps)
        want = hclip.weights(*args, neg=hneg if c["with_neg_file"] else None, **maps)
        assert got.is_cuda and got.shape == want.shape and _bits(got) == _bits(want), c


@pytest.mark.parametrize("seed,I,with_neg,drop", R.RANDOM_CASES)
def test_weights_are_logitstore_weights_on_random_stores(seed, I, with_neg, drop):
    c = R.random_case(seed, I, with_neg, drop_neg=drop)
    dev, host = _stores(c["batches"], 8)
    ndev, nhost = _stores(c["neg_batches"], 8) if with_neg else (None, None)
    if drop:
        assert (_key_error_of(lambda: dev.weights(c["user"], c["item"], c["time"], neg=ndev))
                == _key_error_of(lambda: host.weights(c["user"], c["item"], c["time"], neg=nhost)))
        return
    got = dev.weights(torch.from_numpy(c["user"]).to(DEV), torch.from_numpy(c["item"]), c["time"], neg=ndev)          # device, host tensor, numpy
    assert _bits(got) == _bits(host.weights(c["user"], c["item"], c["time"], neg=nhost))
    # round trip: the host store of the device store is the host store
    back = dev.to_store()
    assert back.as_dict() == host.as_dict() and np.array_equal(back._cat()[0], host._cat()[0]) and back._cat()[1].tobytes() == host._cat()[1].tobytes()
    again = DeviceLogitStore.from_store(host, device=DEV)
    assert _bits(again.weights(c["user"], c["item"], c["time"], neg=ndev)) == _bits(got)


def test_add_batch_refuses_a_wrong_segment_count():
    dev, host = DeviceLogitStore(S=40, device=DEV), LogitStore(S=40)
    args = (torch.ones(3, dtype=torch.int64), torch.ones(3, dtype=torch.int64), torch.ones(3, dtype=torch.int64), torch.zeros(3, 39))
    with pytest.raises(ValueError) as e1:
        dev.add_batch(*args)
    with pytest.raises(ValueError) as e2:
        host.add_batch(*args)
    assert e1.value.args == e2.value.args


# ------------------------------------------------------------------ head forward
@pytest.mark.parametrize("S", [1, 40, 64, 65, 130, 260])
@pytest.mark.parametrize("B,I", [(1, 1), (5, 3), (7, 37)])          # 1, 15 and 4 * 64 + 3 rows
def test_head_forward_within_the_fp32_bound(S, B, I):
    """S = 40, 64: 16-byte accesses, one round of chunks; 260: 16-byte accesses, several rounds; 1, 65: scalar accesses, 65 and 130 in
    several rounds."""
    H = _H()
    g = np.random.RandomState(S * 1000 + B * I)
    m, mn = 11, 5
    vals, neg_vals = g.randn(m, S).astype(np.float32), g.randn(mn, S).astype(np.float32)
    pred = g.randn(B, I, S).astype(np.float32)
    rowidx = g.choice(np.concatenate([[-1, -1], np.arange(m), -2 - np.arange(mn)]), (B, I)).astype(np.int32)          # mixed within a row
    dur = g.randint(0, S + 4, (B, I)).astype(np.int64)
    dur.reshape(-1)[0] = 0
    dur.reshape(-1)[-1] = S + 3
    d = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    for duration in (dur, None):
        want, bound = R.head(pred, rowidx, vals, neg_vals, duration)
        got, w = H.store_head(d(pred), d(rowidx), d(vals), d(neg_vals), d(duration), weight_out=True)
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        print("S=%d rows=%d mask=%s: max err / bound = %.3f" % (S, B * I, duration is not None, float((err / np.maximum(bound, 1e-300)).max())))
        assert (err <= bound).all()
        assert _bits(w) == R.weights(rowidx, vals, neg_vals).tobytes()
        again = H.store_head(d(pred), d(rowidx), d(vals), d(neg_vals), d(duration))
        assert _bits(again) == _bits(got)
    if B * I > 1:
        assert (R.head(pred, rowidx, vals, neg_vals, dur)[0].reshape(-1)[0] == 0) and float(got.reshape(-1)[0]) != 0.0


def test_head_with_bases_off_the_16_byte_grid():
    """S = 40 would take 16-byte accesses; a pred or a value matrix that starts 4 bytes off takes the scalar kernels (64 lanes per
    row, 40 of them busy).  Same bound forward, same bits backward."""
    H = _H()
    S, B, I, m, mn = 40, 7, 37, 11, 5
    g = np.random.RandomState(5)
    vals, neg_vals, pred = g.randn(m, S).astype(np.float32), g.randn(mn, S).astype(np.float32), g.randn(B, I, S).astype(np.float32)
    rowidx = g.choice(np.concatenate([[-1, -1], np.arange(m), -2 - np.arange(mn)]), (B, I)).astype(np.int32)
    dur = g.randint(0, S + 4, (B, I)).astype(np.int64)
    gout = g.randn(B, I).astype(np.float32)

    def off4(a):          # the same values in a contiguous device tensor whose first byte is 4 past an aligned address
        buf = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)
        t = buf[1:].view(a.shape)
        t.copy_(torch.from_numpy(a))
        assert t.is_contiguous() and t.data_ptr() % 16 == 4
        return t
    d = lambda a: torch.from_numpy(a).to(DEV)
    want, bound = R.head(pred, rowidx, vals, neg_vals, dur)
    wgrad = (torch.from_numpy(gout)[..., None] * torch.from_numpy(R.weights(rowidx, vals, neg_vals))) * torch.from_numpy((np.arange(S) < dur[..., None]).astype(np.float32))
    for p_, v_ in ((off4(pred), d(vals)), (d(pred), off4(vals)), (off4(pred), off4(vals))):
        got, w = H.store_head(p_, d(rowidx), v_, d(neg_vals), d(dur), weight_out=True)
        assert (np.abs(got.cpu().numpy().astype(np.float64) - want) <= bound).all()
        assert _bits(w) == R.weights(rowidx, vals, neg_vals).tobytes()
        assert _bits(H.store_head(p_, d(rowidx), v_, d(neg_vals), d(dur))) == _bits(got)
        assert _bits(H.store_head_bwd(d(gout), S, rowidx=d(rowidx), vals=v_, neg_vals=d(neg_vals), duration=d(dur))) == _bits(wgrad)
    wt = g.rand(B, I, S).astype(np.float32)
    wg2 = (torch.from_numpy(gout)[..., None] * torch.from_numpy(wt)) * torch.from_numpy((np.arange(S) < dur[..., None]).astype(np.float32))
    assert _bits(H.store_head_bwd(d(gout), S, weight=off4(wt), duration=d(dur))) == _bits(wg2)


def test_head_marks_a_row_index_outside_its_matrix():
    H = _H()
    S = 40
    vals, neg_vals = torch.randn(3, S, device=DEV), torch.randn(2, S, device=DEV)
    rowidx = torch.tensor([[0, 3, -3, -4, 2 ** 31 - 1, -2 ** 31, -1]], dtype=torch.int32, device=DEV)
    out, w = H.store_head(torch.ones(1, 7, S, device=DEV), rowidx, vals, neg_vals, weight_out=True)
    nan = torch.isnan(out.cpu())[0].tolist()
    assert nan == [False, True, False, True, True, True, False]
    assert torch.isnan(w.cpu()).all(-1)[0].tolist() == nan and torch.equal(w[0, 6].cpu(), torch.ones(S))
    out2 = H.store_head(torch.ones(1, 7, S, device=DEV), rowidx, vals, None)          # no negatives matrix at all
    assert torch.isnan(out2.cpu())[0].tolist() == [False, True, True, True, True, True, False]


def test_head_through_stores_built_from_the_cliprec_fixture():
    """Item 0 of each row in the target store, items 1 and 2 in a negatives store, I = 3; the 2e-5 of
    test_weighted_head_matches_cliprec_forward."""
    z = np.load(os.path.join(GOLDEN, "io_cliprec.npz"))
    cp, w, dur = z["clip_pred"], z["weight"], z["duration"]
    B, I, S = cp.shape
    assert I == 3
    user, time = np.arange(B, dtype=np.int64) + 1, T0 + np.arange(B, dtype=np.int64)
    item = (np.arange(B * I, dtype=np.int64) + 1).reshape(B, I)
    clip, _ = _stores([(user, item[:, 0], time, w[:, 0])], S)
    neg, _ = _stores([(np.repeat(user, 2), item[:, 1:].reshape(-1), np.repeat(time, 2), w[:, 1:].reshape(-1, S))], S)
    empty = DeviceLogitStore(S=S, device=DEV)
    pred = torch.from_numpy(cp).to(DEV)
    for got, ref in ((clip.head(pred, user, item, time, duration=dur, neg=neg), z["pred_weighted_masked"]),
                     (empty.head(pred, user, item, time, duration=dur, neg=neg), z["pred_ones_masked"]),
                     (clip.head(pred, user, item, time, neg=neg), z["pred_weighted_nomask"])):
        assert got.shape == (B, I) and float((got.cpu() - torch.from_numpy(ref)).abs().max()) <= 2e-5
    assert _bits(clip.weights(user, item, time, neg=neg)) == w.tobytes()
    # check=False: no exception for a missing negatives key, the miss slots come back with the output
    few, _ = _stores([(np.repeat(user, 2)[1:], item[:, 1:].reshape(-1)[1:], np.repeat(time, 2)[1:], w[:, 1:].reshape(-1, S)[1:])], S)
    out, miss = clip.head(pred, user, item, time, duration=dur, neg=few, check=False)
    assert miss.cpu().tolist() == [1, R.MISS_NONE] and out.shape == (B, I)
    with pytest.raises(KeyError):
        clip.head(pred, user, item, time, duration=dur, neg=few)


# ------------------------------------------------------------------ backward
@pytest.mark.parametrize("S", [40, 65])
def test_heads_are_differentiable_in_pred(S):
    H = _H()
    c = R.random_case(21, 3, True, S=S)
    dev, host = _stores(c["batches"], S)
    ndev, nhost = _stores(c["neg_batches"], S)
    B, I = c["item"].shape
    gen = torch.Generator().manual_seed(S)
    pred = torch.randn(B, I, S, generator=gen)
    g = torch.randn(B, I, generator=gen)
    dur = torch.randint(0, S + 3, (B, I), generator=gen)
    w = host.weights(c["user"], c["item"], c["time"], neg=nhost)
    assert (w != 1).any() and (w == 1).all(-1).any()
    for duration in (dur, None):
        mask = (torch.arange(S)[None, None, :] < duration[..., None]).float() if duration is not None else torch.ones(B, I, S)
        p = pred.to(DEV).requires_grad_(True)
        out = dev.head(p, c["user"], c["item"], c["time"], duration=duration, neg=ndev)
        (dp,) = torch.autograd.grad(out, p, g.to(DEV))
        assert _bits(dp) == _bits((g[..., None] * w) * mask)
        # weighted_head: an explicit weight, and none
        for weight in (torch.rand(B, I, S, generator=gen), None):
            p = pred.to(DEV).requires_grad_(True)
            wd, dd = (None if weight is None else weight.to(DEV)), (None if duration is None else duration.to(DEV))
            out = weighted_head(p, wd, dd)
            assert out.requires_grad and _bits(out) == _bits(H.segment_weighted_sum(pred.to(DEV), wd, dd))
            (dp,) = torch.autograd.grad(out, p, g.to(DEV))
            assert _bits(dp) == _bits((g[..., None] * (weight if weight is not None else torch.ones(B, I, S))) * mask)
    with torch.no_grad():
        assert not weighted_head(pred.to(DEV), None, None).requires_grad


# ------------------------------------------------------------------ the dump loop
def test_dump_logits_is_the_host_store_filled_batch_by_batch(tmp_path):
    """The small model of test_eval_gpu.test_valid_model_matches_host_metrics; two splits of two batches, a key repeated across
    batches (the later logits win)."""
    _H()
    from segmminterest_amd.synth import make_batch
    from segmminterest_amd.trainer import Trainer, default_args, init_model
    B, S, Lt, D, N = 48, 40, 10, 64, 2
    margs = default_args(num_layers_enc=N, d_model=D, nhead=4, input_type={"user": "image", "photo": "image"}, exposure_prob=[0.9] * S)
    torch.manual_seed(3)
    model = init_model(margs, n_users=1, n_items=1, input_dim=D, max_vid_len=S, max_usr_len=Lt).to(DEV)
    tr = Trainer(model)
    batches = [{k: v.to(DEV) for k, v in make_batch(B, S, Lt, D, seed=200 + i).items()} for i in range(4)]
    for k in ("user_id", "photo_id", "time_ms"):
        for i in range(4):
            batches[i][k] = batches[i][k].clone()
        batches[3][k][5] = batches[0][k][2]          # across splits
        batches[1][k][0] = batches[0][k][7]          # within a split
    splits = [batches[:2], batches[2:]]
    dev = tr.dump_logits(splits)
    assert isinstance(dev, DeviceLogitStore) and len(dev) == 4 * B and dev._vals[0].is_cuda
    host = LogitStore(S=S)
    for split in splits:
        for b in split:
            host.add_batch(b["user_id"], b["photo_id"], b["time_ms"], tr.eval_step(b, mode="inference")["logits"])
    back = dev.to_store()
    assert back.as_dict() == host.as_dict() and len(host.as_dict()) <= 4 * B - 2
    back.save_json(tmp_path / "dev.json")
    host.save_json(tmp_path / "host.json")
    assert open(tmp_path / "dev.json", "rb").read() == open(tmp_path / "host.json", "rb").read()
    # and the store answers for the repeated key with the later batch's logits
    b0, b3 = batches[0], batches[3]
    w = dev.weights(b0["user_id"][2:3], b0["photo_id"][2:3].reshape(1, 1), b0["time_ms"][2:3])
    assert _bits(w[0, 0]) == _bits(tr.eval_step(b3, mode="inference")["logits"][5])
