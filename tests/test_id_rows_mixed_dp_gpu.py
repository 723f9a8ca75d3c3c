"""Data parallel: the id tables' row lists across recorded steps, replays, eager short steps and eager full steps
(tests/id_rows_cases.py tells the cases and the three checks).  Under the sparse row exchange the list is the communicator's
persistent gathered-id buffer, which an eager step of another shape replaces (DPComm._pbuf) while the recording goes on naming
the one it was recorded with.

Spawned ranks on cuda:0 as in test_dp_gpu.py: two ranks over gloo (host-staged collectives), one forced rank over nccl.
id_d32_N2, Trainer(comm=DPComm(), overlap=True, dropout=True, device_state=True), sparse tables and
lazy_tables=dict(data_parallel=True); sequence ``R P P e8 P P e8 P E P``.  Every rank runs checks 1 (ids of all ranks, gathered by
the test) and 2 (against the reference run's arrays, made by ranks of their own with ``hipabi.zero_rows`` replaced) itself and
has check 3 around every replay; rank 0 returns numpy arrays.  Four cases: their time is process start-up."""
import os
import queue as queue_mod
import sys

import pytest
import torch
import torch.multiprocessing as mp

import id_rows_cases as C
from helpers import ROOT, build_model, load_case

pytestmark = pytest.mark.gpu
NAME = "id_d32_N2"
KW = {"sparse": {}, "lazy": dict(lazy_tables=dict(data_parallel=True))}


def _setup(rank, world, port, backend):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      SEGMM_DP_FORCE="1" if world == 1 else "0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    torch.cuda.set_device(0)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    return dist


def _trainer(variant):
    from segmminterest_amd.trainer import DPComm, Trainer
    cfg, g, _, _ = load_case(NAME)
    model = build_model(cfg)
    model.load_state_dict(g["sd"])
    model = model.cuda()
    torch.manual_seed(11)
    tr = Trainer(model, lr=1e-3, comm=DPComm(), overlap=True, dropout=True, device_state=True, **KW[variant])
    assert tr.comm.active and tr.sparse_tables
    return cfg, tr


def _shards(fulls, world, rank):
    from segmminterest_amd.trainer import shard_rows
    out = []
    for f in fulls:
        s, e = shard_rows(f["label"].shape[0], world, rank)
        out.append({k: (v[s:e].contiguous().cuda() if torch.is_tensor(v) else v) for k, v in f.items()})
    return out


def _seq_child(rank, world, port, backend, variant, ref, q):
    """One rank.  ``ref`` None: the reference run (every step eager, zero_rows -> a fill of the whole table, in this process only).
    Otherwise the mixed sequence behind the replay guard, compared with ``ref`` (rank 0's arrays of the reference run) right here."""
    dist = _setup(rank, world, port, backend)
    try:
        cfg, tr = _trainer(variant)
        fulls = C.make_batches(cfg, C.DP_SEQUENCE)
        shards = _shards(fulls, world, rank)

        def all_ids(t):          # the test gathers the ids itself: every rank's shard of step t, in rank order
            out = {}
            for key in ("photo_identity_id", "user_identity_id"):
                parts = [shards[t][key].reshape(-1).tolist()]
                if world > 1:
                    parts = [None] * world
                    dist.all_gather_object(parts, shards[t][key].reshape(-1).tolist())
                out[key] = [x for p in parts for x in p]
                assert out[key] == fulls[t][key].tolist()
            return out
        if ref is None:
            with C.dense_clears():
                res = C.run_sequence(tr, C.DP_SEQUENCE, fulls, None, mixed=False, all_ids=all_ids, shard=shards)
        else:
            with C.replay_guard() as log:
                res = C.run_sequence(tr, C.DP_SEQUENCE, fulls, None, mixed=True, all_ids=all_ids, shard=shards)
            assert log.count("step") == C.DP_SEQUENCE.count("P")
            C.same_state(res, ref, "rank %d" % rank)
        if rank == 0:
            q.put(res)          # floats and numpy arrays: no torch shared-memory handles
    finally:
        dist.destroy_process_group()


def _fit_child(rank, world, port, backend, recorded, q):
    dist = _setup(rank, world, port, backend)
    try:
        from segmminterest_amd.synth import make_batch
        cfg, tr = _trainer("sparse")
        train = _shards(C.make_batches(cfg, ["E"] * 7 + ["e8"]), world, rank)
        valid = _shards([make_batch(C.FULL, cfg["S"], cfg["Lt"], cfg["D_in"], n_users=cfg["n_users"], n_items=cfg["n_items"], seed=s) for s in (100, 101)],
                        world, rank)
        with C.replay_guard() as log:
            hist = tr.fit(train, valid, epochs=2, valid_step=3, main_metric="NDCG@5", permutation=0, recorded=bool(recorded))
        assert log.count("step") == (10 if recorded else 0)
        snap = C.snapshot(tr)
        if rank == 0:
            q.put((hist, snap))
    finally:
        dist.destroy_process_group()


def _spawn(target, world, port, args):
    """Rank 0's result; a rank that ends with an error ends the wait at once."""
    import time
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, world, port) + args + (q,)) for r in range(world)]
    for p in procs:
        p.start()
    res, t0 = None, time.monotonic()
    try:
        while res is None:
            try:
                res = q.get(timeout=0.5)
            except queue_mod.Empty:
                bad = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                assert not bad, "a rank failed (exit codes %s)" % bad
                assert time.monotonic() - t0 < 300, "no result from the ranks"
    finally:
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.kill()
                p.join()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return res


DP_CASES = [(2, "gloo", "sparse"), (2, "gloo", "lazy"), (1, "nccl", "sparse"), (1, "nccl", "lazy")]


@pytest.mark.parametrize("world,backend,variant", DP_CASES, ids=["%d-%s-%s" % c for c in DP_CASES])
def test_mixed_data_parallel_steps_clear_exactly_the_rows_last_scattered(world, backend, variant):
    port = 29100 + (os.getpid() + 7 * world + (3 if variant == "lazy" else 0)) % 150
    ref = _spawn(_seq_child, world, port, (backend, variant, None))
    assert len(set(ref["losses"])) == len(ref["losses"]) == len(C.DP_SEQUENCE)
    got = _spawn(_seq_child, world, port + 1, (backend, variant, ref))
    C.same_state(got, ref, "rank 0")


def test_data_parallel_fit_recorded_equals_fit_eager_in_id_mode():
    """Two gloo ranks, an epoch of 7 full batches and an 8-row one, twice: the short batch is stepped eagerly between replays."""
    port = 29260 + os.getpid() % 30
    (h_e, s_e), (h_r, s_r) = (_spawn(_fit_child, 2, port + rec, ("gloo", rec)) for rec in (0, 1))
    assert h_e["global_step"] == h_r["global_step"] == 16
    assert h_e == h_r
    for name, a, b in zip(("parameters", "m", "v"), s_e, s_r):
        assert (a == b).all(), name
