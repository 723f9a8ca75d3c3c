"""The id tables' row lists across eager, short and recorded steps: the cases and the checks shared by test_id_rows_mixed_cpu.py,
test_id_rows_mixed_gpu.py and test_id_rows_mixed_dp_gpu.py.

The dense id-table gradient is never refilled: every step clears the rows the step BEFORE it scattered into it, by that step's id
list (engine._embed_bwd; a recorded step carries the list by address and its length by value).  The list crosses step boundaries,
so it is tested where step kinds change: full eager steps, short eager steps (8 and 5 rows), the recording step, replays and
validation passes, in three orders.

Batches: ``synth.make_batch`` with both id tensors (and their ``user_id`` / ``photo_id`` copies) overwritten from an explicit schedule
(:func:`ids_for`), so that ids recur, and fail to recur, by design.

Check 1 (:func:`stale_rows`, after every step): the non-zero rows of each table's slice of the flat gradient lie among the ids
stepped in this step -- a row an earlier step left behind shows at once, whatever AdamW makes of it later.
Check 2 (:func:`same_state`): losses, parameters and both moments equal, in every bit, those of a reference run that depends on no
row list: a fresh trainer with the same seeds, every step eager, ``hipabi.zero_rows`` replaced by a fill of the whole table
(:func:`dense_clears`).
Check 3 (:func:`guarded_replay`): a host-side guard around ``recording.replay`` that raises BEFORE anything is enqueued unless every
pointer slot is about to name a tensor of the recorded shape and dtype and every relocated ``segmm_zero_rows`` id list holds its
recorded count -- so no test of these modules ever launches a replay that reads outside a tensor."""
import contextlib

import numpy as np
import torch

FIXTURES = ("id_d32_N2", "both_fh2", "uimg_pid_fh2")          # d = 32, n_items = 200, n_users = 50
FULL, SHORT = 16, (8, 5)          # rows of a full batch; of the short ones (5: no multiple of 4)

# E eager full, e8 / e5 eager short, R record(batch, warmup=0, prev_batch=the batch before), P run_recorded, V valid_model
SEQUENCES = {
    "A": "E E R P P e8 P P e5 P E P".split(),
    "B": "E E R P e8 V P P V e5 E P".split(),
    "C": "E E R P e8 e8 R P P E e8 P".split(),          # the second R records the 8-row shape; the last e8 follows two 8-row replays
}
# data parallel: the first R is record(batch, warmup=0) -- one warm-up step on a copy of the batch, then the recorded one (the
# reference run steps that batch twice); 5-row batches do not shard evenly and stay out
DP_SEQUENCE = "R P P e8 P P e8 P E P".split()

# ---- the id schedule.  Row 0: a general id; row 1: its duplicate; rows 2, 3 (items) / row 2 (users): ids of this step alone, never
# seen again; row 4: on even steps the id that comes back two steps later and is absent in between; every other row: general ids,
# which overlap from step to step
ITEM_GENERAL, ITEM_ONCE, ITEM_BACK = 90, (150, 170), 120
USER_GENERAL, USER_ONCE, USER_BACK = 30, 38, 35


def ids_for(t, n):
    """(item ids, user ids) of step ``t`` with ``n`` rows, int64."""
    items = [1 + (7 * t + 3 * j) % ITEM_GENERAL for j in range(n)]
    users = [1 + (5 * t + 2 * j) % USER_GENERAL for j in range(n)]
    items[1], users[1] = items[0], users[0]
    items[2], items[3], users[2] = ITEM_ONCE[0] + t, ITEM_ONCE[1] + t, USER_ONCE + t
    if t % 2 == 0:
        items[4], users[4] = ITEM_BACK, USER_BACK
    return torch.tensor(items, dtype=torch.int64), torch.tensor(users, dtype=torch.int64)


def sizes(seq):
    """Rows of every step of ``seq`` (V steps on no batch of its own).  P replays the shape of the last R."""
    out, rec = [], None
    for i, tok in enumerate(seq):
        if tok == "V":
            continue
        if tok == "E":
            n = FULL
        elif tok[0] == "e":
            n = int(tok[1:])
        elif tok == "R":          # the shape of the batch before it (record(prev_batch=...)); a first R: a full batch
            n = rec = out[-1] if out else FULL
        else:
            n = rec
        out.append(n)
    return out


def make_batches(cfg, seq, seed=300):
    """One CPU batch per step of ``seq``, ids from the schedule."""
    from segmminterest_amd.synth import make_batch
    out = []
    for t, n in enumerate(sizes(seq)):
        b = make_batch(n, cfg["S"], cfg["Lt"], cfg["D_in"], n_users=cfg["n_users"], n_items=cfg["n_items"], seed=seed + t)
        items, users = ids_for(t, n)
        b["photo_identity_id"], b["photo_id"] = items, items.clone()
        b["user_identity_id"], b["user_id"] = users, users.clone()
        out.append(b)
    return out


def schedule_report(seq, n_items=200, n_users=50):
    """What the schedule of ``seq`` guarantees, as a dict of booleans / counts (test_id_rows_mixed_cpu.py asserts them)."""
    steps = [tuple(x.tolist() for x in ids_for(t, n)) + (n,) for t, n in enumerate(sizes(seq))]
    rep = dict(duplicates=True, covers=False, short_absent_items=[], short_absent_users=[], returns=False, never=False, in_range=True)
    for t, (items, users, n) in enumerate(steps):
        rep["duplicates"] &= len(set(items)) < n and len(set(users)) < n
        rep["covers"] |= len(set(items)) >= n_items or len(set(users)) >= n_users
        rep["in_range"] &= all(1 <= x <= n_items for x in items) and all(1 <= x <= n_users for x in users)
        if n < FULL and t + 1 < len(steps):
            for k, table in ((0, "short_absent_items"), (1, "short_absent_users")):
                absent = set(steps[t][k]) - set(steps[t + 1][k])
                rep[table].append(len(absent))
                later = [set(s[k]) for s in steps[t + 2:]]
                rep["returns"] |= any(a in s for a in absent for s in later)
                rep["never"] |= any(all(a not in s for s in later) for a in absent)
    return rep


# ---- check 1
def id_tables(model):
    """[(parameter name, start, end, rows, width, batch key of its ids)] of the live id-embedding tables in the flat gradient."""
    st = model._store
    mods = dict(model.named_modules())
    out = []
    for name in st.live_names:
        if name.endswith(("vid_proj.weight", "usr_proj.weight")) and isinstance(mods.get(name.rsplit(".", 1)[0]), torch.nn.Embedding):
            o, n = st.index[name]
            rows, width = st._params[name].shape
            out.append((name, o, o + n, rows, width, "photo_identity_id" if name.endswith("vid_proj.weight") else "user_identity_id"))
    assert sorted((s, e) for _, s, e, _, _, _ in out) == st.table_ranges()
    return out


def stale_rows(grad, ids):
    """Rows of the 2-D table gradient ``grad`` that hold a non-zero bit and are not among ``ids``."""
    g = np.ascontiguousarray(grad.detach().cpu().numpy() if torch.is_tensor(grad) else grad).view(np.int32)
    nz = np.flatnonzero((g != 0).any(axis=1))          # (bits, not values: -0.0 left behind is a row that was written)
    return sorted(set(nz.tolist()) - {int(x) for x in ids})


def check_rows(model, ids_by_key, what=""):
    """Check 1 on ``model`` (device synchronised by the caller): ``ids_by_key`` = {batch key: every id stepped in this step}."""
    st = model._store
    for name, s, e, rows, width, key in id_tables(model):
        bad = stale_rows(st.gflat[s:e].view(rows, width), ids_by_key[key])
        assert not bad, "%s: rows %s of the gradient of %s are non-zero, but this step's ids are %s" % (what, bad, name, sorted(set(ids_by_key[key])))


# ---- check 2
@contextlib.contextmanager
def dense_clears():
    """The reference run's patch: while open, ``hipabi.zero_rows(table, ids)`` fills the whole table with zeros -- no row list is read."""
    from segmminterest_amd import hipabi as H
    real = H.zero_rows

    def zero_rows(table, ids):
        H.fill_zero(table)
    H.zero_rows = zero_rows
    try:
        yield zero_rows
    finally:
        H.zero_rows = real


def snapshot(tr):
    """(parameters, m, v) as int32 numpy arrays; lazy tables flushed first."""
    tr.opt.flush_tables()
    torch.cuda.synchronize()
    return tuple(x.detach().cpu().numpy().view(np.int32).copy() for x in (tr.model._store.flat, tr.opt.m, tr.opt.v))


def same_state(got, want, what=""):
    """Check 2 on two results of :func:`run_sequence`: every loss, every validation and every snapshot, bit for bit."""
    assert got["losses"] == want["losses"], (what, got["losses"], want["losses"])
    assert got["valid"] == want["valid"], (what, got["valid"], want["valid"])
    assert len(got["snaps"]) == len(want["snaps"]) >= 1
    for k, (a, b) in enumerate(zip(got["snaps"], want["snaps"])):
        for name, x, y in zip(("parameters", "m", "v"), a, b):
            assert x.shape == y.shape and (x == y).all(), "%s: %s differ at snapshot %d (%d of %d words)" % (what, name, k, int((x != y).sum()), x.size)


# ---- check 3
class ReplayGuardError(AssertionError):
    pass


def check_replay(r, batch, prev):
    """Raises unless the replay of ``r`` on ``batch`` (lag-1 slots: ``prev``) stays inside the tensors it names."""
    from segmminterest_amd import hipabi as H
    spans = r["spans"]
    zr = H.op_ids()["segmm_zero_rows"]
    ids_slot = H.PARAMS["segmm_zero_rows"].index("ids")
    for arr, ci, ai, k, off, lag in r["relocs"]:
        src = prev if lag else batch
        t = src.get(k) if src is not None else None
        if not torch.is_tensor(t):
            raise ReplayGuardError("slot (%d, %d): no tensor %r in the %s batch" % (ci, ai, k, "previous" if lag else "current"))
        if (tuple(t.shape), t.dtype) != spans[k]:
            raise ReplayGuardError("slot (%d, %d) is about to name %s[%r] of %s %s; the recording holds %s %s"
                                   % (ci, ai, "prev" if lag else "batch", k, tuple(t.shape), t.dtype, spans[k][0], spans[k][1]))
        if arr[ci].op == zr and ai == ids_slot:
            n = int(H.cmd_arg(arr[ci], "segmm_zero_rows", "n"))
            if off + 8 * n > t.numel() * t.element_size():
                raise ReplayGuardError("segmm_zero_rows reads %d ids from byte %d of %s[%r], which holds %d bytes"
                                       % (n, off, "prev" if lag else "batch", k, t.numel() * t.element_size()))


def guarded_replay(real, log=None):
    """``recording.replay`` behind :func:`check_replay`: the check runs first and raises before ``real`` touches a slot or enqueues
    anything.  ``log``: a list that gets one entry per replay let through."""
    def replay(r, who, what, batch, prev=None, *a, **kw):
        check_replay(r, batch, prev)
        if log is not None:
            log.append(what)
        return real(r, who, what, batch, prev, *a, **kw)
    return replay


@contextlib.contextmanager
def replay_guard():
    """Check 3 active while open; yields the log of the replays it let through."""
    from segmminterest_amd import recording as R
    real, log = R.replay, []
    R.replay = guarded_replay(real, log)
    try:
        yield log
    finally:
        R.replay = real


# ---- one run of a sequence
def run_sequence(tr, seq, batches, valid_batch, mixed, all_ids=None, shard=None):
    """Steps ``tr`` through ``seq`` on ``batches`` (device batches, one per step; ``shard`` = the rank's own, data parallel);
    ``mixed`` = False: every R and P is an eager step.  Check 1 after every step (``all_ids(t)`` -> {batch key: ids of all ranks};
    default: the batch's own).  Returns losses (floats, in step order), validation results, snapshots after each V and at the end."""
    res = dict(losses=[], valid=[], snaps=[])
    own = shard if shard is not None else batches
    t = 0
    for i, tok in enumerate(seq):
        if tok == "V":
            res["valid"].append(tr.valid_model([valid_batch], permutation=0))
            res["snaps"].append(snapshot(tr))
            continue
        b = own[t]
        if not mixed or tok in ("E", "e8", "e5"):
            if tok == "R" and t == 0:          # (a first R steps its batch twice: the warm-up on a copy, then the recorded step)
                tr.train_step({k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()})
            out = tr.train_step(b)
        elif tok == "R":
            out = tr.record(b, warmup=0, prev_batch=own[t - 1]) if t else tr.record(b, warmup=0)
        else:
            out = tr.run_recorded(b)
        loss = out["loss"].detach().clone()
        if tr.comm.active:
            loss = tr.comm.sum_scalar(loss)
        torch.cuda.synchronize()
        res["losses"].append(float(loss))
        ids = all_ids(t) if all_ids is not None else {k: batches[t][k].reshape(-1).tolist() for k in ("photo_identity_id", "user_identity_id")}
        check_rows(tr.model, ids, "step %d (%s)" % (t, tok))
        t += 1
    res["snaps"].append(snapshot(tr))
    return res
