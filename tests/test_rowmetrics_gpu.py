"""The per-row metrics of the test phase on the device (csrc/evalops.h row_metrics_kernel / row_metrics_accumulate_kernel,
my_evaluation.row_metrics_device / RowMetricAccumulator, Trainer.test_model(device_metrics=True)) against the float64 restatement
of tests/test_rowmetrics_cpu.py, the reference's recorded values, the host path and a two-rank run."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from helpers import GOLDEN, ROOT, build_model, load_case
from test_rowmetrics_cpu import EPS, PER_ROW, bounds, make_case, ref_records

pytestmark = pytest.mark.gpu
DEV = "cuda"
INT_FIELDS = ("view_length", "duration", "top1", "group")
FLOAT_FIELDS = ("jaccard", "pred_view_length", "leave_ctr", "leave_ctr_view")
SUMS = ("n", "jaccard", "pred", "sq_err", "abs_err", "leave_ctr", "leave_ctr_view", "top1_sq_err", "top1_abs_err", "n_complete")


def _records(x, gt, photo_id=None, seen=None):
    from segmminterest_amd.my_evaluation import row_metrics_device
    return row_metrics_device(x, gt, photo_id=photo_id, seen=seen)


def _check_against(rec, ref, S, factor=1, rows=None):
    bd = bounds(S)
    for k in INT_FIELDS:
        assert rec[k].dtype == torch.int32
        got = rec[k].cpu().numpy()
        assert np.array_equal(got if rows is None else got[rows], ref[k] if rows is None else ref[k][rows]), k
    for k in FLOAT_FIELDS:
        assert rec[k].dtype == torch.float32
        got = rec[k].cpu().numpy().astype(np.float64)
        err = np.abs((got if rows is None else got[rows]) - (ref[k] if rows is None else ref[k][rows]))
        print(k, "max err", err.max() if err.size else 0.0, "bound", factor * bd[k])
        assert (err <= factor * bd[k]).all(), (k, err.max())


@pytest.mark.parametrize("c", [1.0, 8.0])
@pytest.mark.parametrize("B,S", [(64, 40), (513, 40), (37, 20), (5, 100), (1, 1)])
def test_records_against_float64(B, S, c):
    from segmminterest_amd import hipabi as H
    x, gt = make_case(B, S, c, seed=7 * B + S)
    ref = ref_records(x.numpy(), gt.numpy())
    if B >= 3:
        assert (ref["view_length"] == 0).any() and (ref["view_length"] == S).any()
    xd, gd = x.to(DEV), gt.to(DEV)
    rec = _records(xd, gd)
    assert set(rec) == set(INT_FIELDS + FLOAT_FIELDS) and all(v.shape == (B,) and v.is_cuda for v in rec.values())
    _check_against(rec, ref, S)
    # leave_ctr_view is 1 - the survival the AUC kernels see, bit for bit
    surv = H.survival(xd, gd)[0]
    k = torch.from_numpy(np.where(ref["view_length"] > 0, ref["view_length"] - 1, S - 1)).to(DEV)
    assert torch.equal(rec["leave_ctr_view"], 1 - surv[torch.arange(B, device=DEV), k])
    # a view whose row stride is not S gives the same records
    wide = torch.full((B, S + 7), 0.25, device=DEV)
    wide[:, :S] = xd
    view = wide[:, :S]
    assert view.stride(0) != S or B == 1
    rec2 = _records(view, gd)
    for name in rec:
        assert torch.equal(rec[name], rec2[name]), name


def test_records_of_the_reference_fixture():
    z = np.load(os.path.join(GOLDEN, "metrics_kat.npz"))
    x, gt = torch.from_numpy(z["interests"]), torch.from_numpy(z["gt"])
    S = x.shape[1]
    rec = {k: v.cpu().numpy() for k, v in _records(x.to(DEV), gt.to(DEV)).items()}
    assert np.array_equal(rec["top1"], z["min_indices"])
    rows, bd = z["meb_rows"], bounds(S)
    assert np.array_equal(rec["view_length"][rows].astype(np.float64), z["meb/view_lengths"])
    for name, key in (("JaccardSim", "jaccard"), ("LeaveMSE", "pred_view_length"), ("LeaveCTR", "leave_ctr"), ("LeaveCTR_view", "leave_ctr_view")):
        err = np.abs(rec[key][rows].astype(np.float64) - z["meb/" + name]).max()
        print(name, "max |device - fixture| =", err, "bound", 2 * bd[key])
        assert err <= 2 * bd[key], (name, err)


def _sums_of(recs):
    """float64 sums [3, F] of the device's own records (a list of host dicts), and sum |v| per entry."""
    tot, mag = np.zeros((3, len(SUMS))), np.zeros((3, len(SUMS)))
    for r in recs:
        r = {k: v.astype(np.float64) for k, v in r.items()}
        vl, pred, top1 = r["view_length"], r["pred_view_length"], r["top1"]
        cols = [np.ones_like(vl), r["jaccard"], pred, (pred - vl) ** 2, np.abs(pred - vl), r["leave_ctr"], r["leave_ctr_view"],
                (top1 - vl) ** 2, np.abs(top1 - vl), (vl == r["duration"]).astype(np.float64)]
        for g, sel in enumerate((np.ones(len(vl), dtype=bool), r["group"] == 1, r["group"] == 0)):
            for f, col in enumerate(cols):
                tot[g, f] += col[sel].sum()
                mag[g, f] += np.abs(col[sel]).sum()
    return tot, mag


def _three_adds(with_empty_row=False):
    from segmminterest_amd.my_evaluation import RowMetricAccumulator, seen_table
    seen_ids = set(range(0, 60, 3))
    seen = seen_table(seen_ids, DEV)
    acc = RowMetricAccumulator(DEV)
    recs, refs = [], []
    for i, (B, S) in enumerate([(64, 40), (513, 40), (37, 20)]):
        x, gt = make_case(B, S, 1.0 if i != 1 else 8.0, seed=100 + i)
        pid = torch.randint(-4, 75, (B,), generator=torch.Generator().manual_seed(i))          # ids below 0 and past the table (58) included
        if with_empty_row and i == 2:
            gt[5] = -2
            pid[5] = 3          # hot
        rec = _records(x.to(DEV), gt.to(DEV), photo_id=pid.to(DEV), seen=seen)
        acc.add(rec)
        recs.append({k: v.cpu().numpy() for k, v in rec.items()})
        refs.append(ref_records(x.numpy(), gt.numpy(), photo_id=pid.numpy(), seen=seen.cpu().numpy()))
    return acc, recs, refs


def test_accumulator_sums_partitions_and_repeats_bit_identically():
    acc, recs, refs = _three_adds()
    state = acc.state.cpu().numpy()
    assert acc.state.dtype == torch.float64 and state.shape == (3, len(SUMS))
    tot, mag = _sums_of(recs)
    n = sum(len(r["group"]) for r in recs)
    err = np.abs(state - tot)
    print("max err / bound", (err / np.maximum(n * 2.0 ** -52 * mag, 1e-300)).max())
    assert (err <= n * 2.0 ** -52 * mag).all(), err
    # the groups against the table, ids outside it cold
    want_cold = sum(int((r["group"] == 1).sum()) for r in refs)
    assert all(np.array_equal(a["group"], b["group"]) for a, b in zip(recs, refs))
    assert 0 < want_cold < n and any((r["group"] == 1).sum() > 0 for r in refs)
    assert state[0, 0] == n and state[1, 0] == want_cold and state[2, 0] == n - want_cold
    assert state[0, 9] == state[1, 9] + state[2, 9] == sum(int((r["view_length"] == r["duration"]).sum()) for r in refs)
    acc2, _, _ = _three_adds()
    assert torch.equal(acc.state, acc2.state)
    fin = acc.final(PER_ROW, "cold")
    assert abs(fin["JaccardSim"] - tot[1, 1] / tot[1, 0]) <= 1e-12 and acc.extras("hot")["rows"] == n - want_cold


def test_a_row_without_segments_makes_only_its_jaccard_sums_nan():
    acc, recs, _ = _three_adds(with_empty_row=True)
    assert recs[2]["duration"][5] == 0 and recs[2]["group"][5] == 0 and np.isnan(recs[2]["jaccard"][5])
    assert all(np.isfinite(recs[2][k][5]) for k in FLOAT_FIELDS if k != "jaccard")
    nan = torch.isnan(acc.state).cpu().numpy()
    want = np.zeros_like(nan)
    want[0, 1] = want[2, 1] = True          # sum of jaccard of all rows and of the hot rows
    assert np.array_equal(nan, want)


def _model_and_batches(n_batches):
    from segmminterest_amd.synth import make_batch
    cfg, g, _, _ = load_case("img_d32_N2")
    model = build_model(cfg)
    model.load_state_dict(g["sd"])
    sizes = [16] * (n_batches - 1) + [8]          # the last batch is short
    batches = [make_batch(b, cfg["S"], cfg["Lt"], cfg["D_in"], n_items=40, seed=300 + i) for i, b in enumerate(sizes)]
    train_videos = set(int(p) for p in batches[0]["photo_id"].tolist()) | {1000, 7}
    return cfg, model.cuda(), [{k: v.to(DEV) for k, v in b.items()} for b in batches], train_videos


EVALS = ["JaccardSim", "LeaveMSE", "LeaveCTR", "LeaveCTR_view", "TOP_K", "ProbAUC"]


def test_test_model_device_metrics_equal_the_host_path():
    from segmminterest_amd.trainer import Trainer
    cfg, model, batches, train_videos = _model_and_batches(3)
    S = cfg["S"]
    tr = Trainer(model)
    host = tr.test_model(batches, EVALS, top_k_permutation=0, train_videos=train_videos)
    dev = tr.test_model(batches, EVALS, top_k_permutation=0, train_videos=train_videos, device_metrics=True)
    assert set(dev) == set(host) | {"extras"}
    assert dev["cold_count_inter"] == host["cold_count_inter"] > 0 and dev["hot_count_inter"] == host["hot_count_inter"] >= 16
    bd = bounds(S)
    tol = {"JaccardSim": 2 * bd["jaccard"], "LeaveCTR": 2 * bd["leave_ctr"], "LeaveCTR_view": 2 * bd["leave_ctr_view"],
           "LeaveMSE": 2 * 2 * S * bd["pred_view_length"]}          # |a^2 - b^2| <= 2 S |a - b| for errors a, b of at most S
    for part in ("final", "cold_final", "hot_final"):
        assert set(dev[part]) == set(host[part]) and set(PER_ROW) | {"ProbAUC", "HR@1", "NDCG@10"} <= set(host[part]), part
        for k, v in host[part].items():
            if k in tol:
                print(part, k, "|device - host| =", abs(dev[part][k] - v), "bound", tol[k])
                assert abs(dev[part][k] - v) <= tol[k], (part, k, dev[part][k], v)
            else:          # batch-level metrics: the same kernels on the same rows
                assert np.isfinite(v) and dev[part][k] == v, (part, k, dev[part][k], v)
    assert not any(k in dev["results_list"] for k in PER_ROW) and dev["results_list"]["view_lengths"] == []
    gt = torch.cat([b["label"] for b in batches])
    n_rows = gt.shape[0]
    assert dev["extras"]["rows"] == n_rows == dev["cold_count_inter"] + dev["hot_count_inter"]
    assert dev["extras"]["view_complete"] == int(((gt == 1).sum(1) == (gt != -2).sum(1)).sum()) > 0


def _run_dp(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from segmminterest_amd.trainer import DPComm, Trainer
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        _, model, batches, train_videos = _model_and_batches(4)
        tr = Trainer(model, comm=DPComm())
        assert tr.comm.active
        res = tr.test_model(batches[rank::world], list(PER_ROW), top_k_permutation=0, train_videos=train_videos, device_metrics=True)
        q.put((rank, {k: res[k] for k in ("final", "cold_final", "hot_final", "extras", "cold_count_inter", "hot_count_inter")}))
    finally:
        dist.destroy_process_group()


def test_two_ranks_give_the_finals_of_all_rows():
    """Two gloo ranks sharing the GPU, each with half of the batches: after the one all-reduce of the accumulator both hold the
    finals of a single process over all batches (another summation order: n 2^-52 sum|v|, every term >= 0 so sum|v| = n |mean|)."""
    from segmminterest_amd.trainer import Trainer
    _, model, batches, train_videos = _model_and_batches(4)
    one = Trainer(model).test_model(batches, list(PER_ROW), top_k_permutation=0, train_videos=train_videos, device_metrics=True)
    n = one["extras"]["rows"]
    assert n == 56
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29480 + os.getpid() % 100
    procs = [ctx.Process(target=_run_dp, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=240) for _ in range(2))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert set(got) == {0, 1}
    for rank, res in got.items():
        assert res["extras"]["rows"] == n and res["extras"]["view_complete"] == one["extras"]["view_complete"]
        assert res["cold_count_inter"] == one["cold_count_inter"] and res["hot_count_inter"] == one["hot_count_inter"]
        for part in ("final", "cold_final", "hot_final"):
            assert set(res[part]) == set(one[part]) == set(PER_ROW)
            for k, v in one[part].items():
                assert abs(res[part][k] - v) <= n * 2.0 ** -52 * abs(v), (rank, part, k, res[part][k], v)
        for k in ("LeaveMAE", "TOP1MSE", "TOP1MAE"):
            assert abs(res["extras"][k] - one["extras"][k]) <= n * 2.0 ** -52 * abs(one["extras"][k]), (rank, k)
