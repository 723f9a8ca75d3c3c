"""The per-row metrics of the test phase without a GPU: argument checks of the two C entry points, the float64 restatement of the
record formulas (the yardstick of tests/test_rowmetrics_gpu.py) against the reference's recorded values and against the host
``main_eval_batch``, and ``RowMetricAccumulator.final`` / ``extras`` against ``compute_final_result``."""
import argparse
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN

EPS = 2.0 ** -23
PER_ROW = ("JaccardSim", "LeaveMSE", "LeaveCTR", "LeaveCTR_view")


def bounds(S):
    """Absolute bounds of the fp32 records against the float64 restatement.  The fp32 survival surv_t = exp(sum_{j <= t} log x_j)
    is off by at most (t + 4) eps absolutely (t + 1 roundings of the sum, log, exp and the product with s |ln s| <= 1 / e): the
    mean of such terms (jaccard) and surv_k (leave_ctr_view) stay within (S + 4) eps, the sum of up to S of them within
    S (S + 4) eps, 1 - interest[k] is one rounding."""
    return {"leave_ctr": EPS, "jaccard": (S + 4) * EPS, "leave_ctr_view": (S + 4) * EPS, "pred_view_length": S * (S + 4) * EPS}


def ref_records(interests, gt, photo_id=None, seen=None):
    """The six formulas of the per-row record in float64 numpy (interests [B, S] float32, gt [B, S] int64)."""
    x32 = np.asarray(interests, dtype=np.float32)
    gt = np.asarray(gt, dtype=np.int64)
    B, S = gt.shape
    x = x32.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        surv = np.exp(np.cumsum(np.log(x), axis=1))
    vl = (gt == 1).sum(1)
    dur = (gt != -2).sum(1)
    pos = np.arange(S)[None, :]
    k = np.where(vl > 0, vl - 1, S - 1)
    rows = np.arange(B)
    watched = pos < vl[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        jaccard = (np.where(watched, 1.0 - np.abs(gt - surv), 0.0).sum(1) + (dur - vl)) / dur
    group = np.zeros(B, dtype=np.int64)
    if seen is not None:
        pid = np.asarray(photo_id, dtype=np.int64).reshape(-1)
        seen = np.asarray(seen)
        inside = (pid >= 0) & (pid < len(seen))
        hot = np.zeros(B, dtype=bool)
        hot[inside] = seen[pid[inside]] != 0
        group = np.where(hot, 0, 1)
    return {"view_length": vl, "duration": dur, "top1": np.argmin(x32, axis=1) if B else np.zeros(0, dtype=np.int64), "group": group,
            "jaccard": jaccard, "pred_view_length": np.where(gt != -2, surv, 0.0).sum(1),
            "leave_ctr": 1.0 - x[rows, k], "leave_ctr_view": 1.0 - surv[rows, k]}


def make_case(B, S, c, seed):
    """interests = sigmoid(randn * c) * linspace(1, 0.6, S) (c = 8 reaches 1e-14: the survival underflows) and labels from
    synth.make_labels with a fully watched row and a row that leaves in the first segment forced in (B >= 3).  S == 1 is below
    make_labels' shortest video (2 segments): there the single cell is the leave segment."""
    from segmminterest_amd.synth import make_labels
    gen = torch.Generator().manual_seed(seed)
    if S >= 2:
        gt = make_labels(B, S, gen)[0]
        if B >= 3:
            gt[0] = 1
            gt[1] = torch.tensor([0] + [-1] * (S // 2) + [-2] * (S - 1 - S // 2))
    else:
        gt = torch.zeros((B, 1), dtype=torch.int64)
    x = torch.sigmoid(torch.randn(B, S, generator=gen) * c) * torch.linspace(1.0, 0.6, S)
    return x.float().contiguous(), gt.contiguous()


def host_lists(interests, gt):
    from segmminterest_amd import main_eval_batch
    args = argparse.Namespace(TOP_K_mask=0, TOP_K_permutation=0, draw_case=0)
    rl = {k: [] for k in PER_ROW + ("view_lengths",)}
    return main_eval_batch(args, interests, gt, (interests > 0.5).float(), rl, type="inference")


def test_entry_points_validate_arguments_without_a_gpu():
    """Null pointers and S = 0 are refused by both entry points before any GPU call, with a message naming the function."""
    from segmminterest_amd import hipabi
    L = hipabi.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    assert L.segmm_row_metrics(None, 4, p, None, None, 0, 2, 4, p, p, None) != 0 and b"row_metrics" in L.segmm_last_error()
    assert L.segmm_row_metrics(p, 4, None, None, None, 0, 2, 4, p, p, None) != 0 and b"row_metrics" in L.segmm_last_error()
    assert L.segmm_row_metrics(p, 4, p, None, None, 0, 2, 4, None, p, None) != 0 and b"row_metrics" in L.segmm_last_error()
    assert L.segmm_row_metrics(p, 4, p, None, None, 0, 2, 4, p, None, None) != 0 and b"row_metrics" in L.segmm_last_error()
    assert L.segmm_row_metrics(p, 4, p, None, None, 0, 2, 0, p, p, None) != 0 and b"row_metrics" in L.segmm_last_error()
    assert L.segmm_row_metrics(p, 4, p, None, None, 0, -1, 4, p, p, None) != 0 and b"row_metrics" in L.segmm_last_error()
    assert L.segmm_row_metrics(p, 4, p, None, p, 8, 2, 4, p, p, None) != 0 and b"row_metrics" in L.segmm_last_error()       # table without ids
    assert L.segmm_row_metrics(p, 4, p, None, None, 0, 0, 4, p, p, None) == 0          # B == 0 launches nothing
    for args in ((None, p, 2, 4, p), (p, None, 2, 4, p), (p, p, 2, 4, None), (p, p, 2, 0, p), (p, p, -1, 4, p)):
        assert L.segmm_row_metrics_accumulate(*args, None) != 0 and b"row_metrics_accumulate" in L.segmm_last_error(), args
    assert L.segmm_row_metrics_accumulate(p, p, 0, 4, p, None) == 0
    assert L.segmm_abi_version() == hipabi.ABI_VERSION == 30
    assert {"segmm_row_metrics", "segmm_row_metrics_accumulate"} <= set(hipabi.op_ids())


def test_restatement_reproduces_the_reference_fixture():
    """The float64 formulas against what the reference's main_eval_batch / TOP_K_leave(test=1) recorded (fp32 arithmetic: both
    sides err, twice the bound)."""
    z = np.load(os.path.join(GOLDEN, "metrics_kat.npz"))
    S = z["interests"].shape[1]
    r = ref_records(z["interests"], z["gt"])
    assert np.array_equal(r["top1"], z["min_indices"])
    assert {0, S} & set(r["view_length"].tolist()) == {0, S}          # the fixture has rows that leave at once and fully watched rows
    rows, bd = z["meb_rows"], bounds(S)
    assert np.array_equal(r["view_length"][rows].astype(np.float64), z["meb/view_lengths"])
    for name, key in (("JaccardSim", "jaccard"), ("LeaveMSE", "pred_view_length"), ("LeaveCTR", "leave_ctr"), ("LeaveCTR_view", "leave_ctr_view")):
        err = np.abs(r[key][rows] - z["meb/" + name]).max()
        print(name, "max |restatement - fixture| =", err, "bound", 2 * bd[key])
        assert err <= 2 * bd[key], (name, err)


@pytest.mark.parametrize("B,S,c", [(64, 40, 1.0), (64, 40, 8.0), (37, 20, 8.0), (5, 100, 1.0), (5, 100, 8.0)])
def test_restatement_agrees_with_the_host_main_eval_batch(B, S, c):
    """The host row loop on CPU tensors (fp32 survival, the yardstick of the reference) stays inside the bounds too -- every row,
    the rows that index [-1] (view_length 0) included."""
    if (B, S, c) == (64, 40, 1.0):
        z = np.load(os.path.join(GOLDEN, "metrics_kat.npz"))
        x, gt = torch.from_numpy(z["interests"]), torch.from_numpy(z["gt"])
    else:
        x, gt = make_case(B, S, c, seed=B + S)
    r, bd = ref_records(x.numpy(), gt.numpy()), bounds(S)
    assert (r["view_length"] == 0).any() and (r["view_length"] == r["duration"]).any()
    rl = host_lists(x, gt)
    assert np.array_equal(np.array(rl["view_lengths"]), r["view_length"].astype(np.float64))
    for name, key in (("JaccardSim", "jaccard"), ("LeaveMSE", "pred_view_length"), ("LeaveCTR", "leave_ctr"), ("LeaveCTR_view", "leave_ctr_view")):
        err = np.abs(r[key] - np.array(rl[name], dtype=np.float64)).max()
        print(name, "max |restatement - host| =", err, "bound", bd[key])
        assert err <= bd[key], (name, err)


def _filled(rng, n_cold, n_hot):
    """(state [3, F] float64 CPU tensor filled by hand, per-group dicts of the per-row lists it was summed from)."""
    from segmminterest_amd.hipabi import ROW_METRIC_SUMS
    assert ROW_METRIC_SUMS == ("n", "jaccard", "pred", "sq_err", "abs_err", "leave_ctr", "leave_ctr_view", "top1_sq_err", "top1_abs_err", "n_complete")
    n = n_cold + n_hot
    rows = dict(vl=rng.randint(0, 41, n).astype(np.float64), dur=rng.randint(1, 41, n).astype(np.float64), top1=rng.randint(0, 40, n).astype(np.float64),
                jaccard=rng.rand(n), pred=rng.rand(n) * 40, leave_ctr=rng.rand(n), leave_ctr_view=rng.rand(n))
    cold = np.arange(n) < n_cold
    state = torch.zeros((3, len(ROW_METRIC_SUMS)), dtype=torch.float64)
    lists = {}
    for g, sel in enumerate((np.ones(n, dtype=bool), cold, ~cold)):
        r = {k: v[sel] for k, v in rows.items()}
        state[g] = torch.tensor([sel.sum(), math.fsum(r["jaccard"]), math.fsum(r["pred"]), math.fsum((r["pred"] - r["vl"]) ** 2),
                                 math.fsum(np.abs(r["pred"] - r["vl"])), math.fsum(r["leave_ctr"]), math.fsum(r["leave_ctr_view"]),
                                 math.fsum((r["top1"] - r["vl"]) ** 2), math.fsum(np.abs(r["top1"] - r["vl"])), (r["vl"] == r["dur"]).sum()],
                                dtype=torch.float64)
        lists[("all", "cold", "hot")[g]] = r
    return state, lists


@pytest.mark.parametrize("n_cold,n_hot", [(7, 30), (0, 12)])
def test_accumulator_final_and_extras_equal_compute_final_result(n_cold, n_hot):
    from segmminterest_amd.my_evaluation import RowMetricAccumulator
    from segmminterest_amd.trainer import compute_final_result
    state, lists = _filled(np.random.RandomState(3), n_cold, n_hot)
    acc = RowMetricAccumulator("cpu")
    assert acc.state.dtype == torch.float64 and tuple(acc.state.shape) == tuple(state.shape) and float(acc.state.abs().sum()) == 0.0
    acc.state.copy_(state)
    for group, r in lists.items():
        got = acc.final(list(PER_ROW) + ["TOP_K", "ProbAUC"], group=group)
        ex = acc.extras(group)
        assert set(got) == set(PER_ROW) and set(ex) == {"LeaveMAE", "TOP1MSE", "TOP1MAE", "view_complete", "rows"}
        n = len(r["vl"])
        assert ex["rows"] == n and ex["view_complete"] == int((r["vl"] == r["dur"]).sum())
        if n == 0:          # an empty group: NaN, no exception
            assert all(math.isnan(v) for v in got.values()) and all(math.isnan(ex[k]) for k in ("LeaveMAE", "TOP1MSE", "TOP1MAE"))
            continue
        want = compute_final_result({"JaccardSim": r["jaccard"].tolist(), "LeaveMSE": r["pred"].tolist(), "view_lengths": r["vl"].tolist(),
                                     "LeaveCTR": r["leave_ctr"].tolist(), "LeaveCTR_view": r["leave_ctr_view"].tolist()})
        for k in PER_ROW:
            assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (group, k, got[k], want[k])
        assert abs(ex["LeaveMAE"] - np.abs(r["pred"] - r["vl"]).mean()) <= 1e-12 * ex["LeaveMAE"]
        assert abs(ex["TOP1MSE"] - ((r["top1"] - r["vl"]) ** 2).mean()) <= 1e-12 * ex["TOP1MSE"]
        assert abs(ex["TOP1MAE"] - np.abs(r["top1"] - r["vl"]).mean()) <= 1e-12 * ex["TOP1MAE"]
    assert acc.final(["LeaveMSE"]) == {"LeaveMSE": acc.final(PER_ROW, "all")["LeaveMSE"]}


def test_seen_table_marks_exactly_the_given_ids():
    from segmminterest_amd.my_evaluation import seen_table
    t = seen_table({3, 0, 11}, "cpu")
    assert t.dtype == torch.uint8 and t.tolist() == [1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1]
    assert seen_table(set(), "cpu").tolist() == [0]          # nothing seen: every row is cold
    with pytest.raises(ValueError):
        seen_table({-1, 2}, "cpu")
