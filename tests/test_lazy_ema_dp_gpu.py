"""Lazy id tables beside the weight average under data parallelism (lazy_tables=dict(data_parallel=True, ema=True)), on the device:
two ranks, fresh child processes sharing the GPU over gloo, against the dense data-parallel EMA trainer ``Trainer(ema=...)`` on the
same shards.  After ``flush_tables()`` EVERY rank's parameters, moments and shadow equal the dense run's in every bit (int32 views);
before it the ranks hold the same table, shadow and stamps and rows were pending.  Eager and recorded."""
import os
import queue as queue_mod
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from helpers import ROOT, build_model, load_case

pytestmark = pytest.mark.gpu
TABLE = "backbone1.vid_proj.weight"
N_ITEMS, GLOBAL_B, DP_STEPS, FLUSH, WORLD = 97, 16, 14, 4, 2
EMA = dict(decay=0.99, warmup=True)
LAZY = dict(flush_every=FLUSH, data_parallel=True, ema=True)


def _cfg():
    cfg, _, _, _ = load_case("id_d32_N2")
    S = 20
    return dict(cfg, S=S, Lt=1, n_items=N_ITEMS, exposure_prob=list(cfg["exposure_prob"])[:S])


def _full_batches():
    """The 14 global batches (CPU): the item ids differ from step to step, drawn from the 97."""
    from segmminterest_amd.synth import make_batch
    cfg = _cfg()
    return [make_batch(GLOBAL_B, cfg["S"], cfg["Lt"], cfg["D_in"], n_users=cfg["n_users"], n_items=N_ITEMS, seed=5100 + i) for i in range(DP_STEPS)]


def _check_id_lists(record_at=None):
    """From the id lists alone: some step brings rank 0 an id that only the other rank holds and whose row is two or more steps behind
    -- the replay of AdamW steps and lerps inside lazy_rows_ema."""
    from segmminterest_amd.trainer import shard_rows
    stamps, flushed, far = {}, 0, False
    for k, b in enumerate(_full_batches()):
        T = k + 1
        if T - 1 - flushed >= FLUSH or T == record_at:
            stamps, flushed = {}, T - 1
        ids = b["photo_identity_id"].tolist()
        per_rank = [set(ids[s:e]) for s, e in (shard_rows(GLOBAL_B, WORLD, r) for r in range(WORLD))]
        far |= any(T - 1 - stamps.get(r, flushed) >= 2 for r in per_rank[1] - per_rank[0])
        for r in ids:
            stamps[r] = T
    return far


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _dp_child(rank, port, mode, q):
    """One rank on cuda:0: the dense data-parallel EMA trainer, then the lazy one, same seeds, same shards.  ``recorded``: device step
    state; the lazy run records step 3 and replays 4..14, the dense run stays eager."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(WORLD), SEGMM_DP_FORCE="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from segmminterest_amd.trainer import DPComm, Trainer, shard_rows
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    try:
        cfg = _cfg()
        s, e = shard_rows(GLOBAL_B, WORLD, rank)
        shards = [{k: v[s:e].contiguous().cuda() for k, v in f.items()} for f in _full_batches()]
        out = {}
        for kind in ("dense", "lazy"):
            torch.manual_seed(5)
            model = build_model(cfg).cuda()
            kw = dict(comm=DPComm(), overlap=True, dropout=False, weight_decay=1e-2, device_state=mode != "eager", ema=dict(EMA))
            if kind == "lazy":
                kw["lazy_tables"] = dict(LAZY)
            tr = Trainer(model, **kw)
            assert tr.comm.active and tr.sparse_tables
            pending = 0
            for t in range(1, DP_STEPS + 1):
                if kind == "dense" or mode == "eager" or t < 3:
                    tr.train_step(shards[t - 1])
                elif t == 3:
                    tr.record(shards[t - 1], warmup=0, prev_batch=shards[t - 2])
                else:
                    tr.run_recorded(shards[t - 1])
                pending = max(pending, tr.opt.tables_pending)
            torch.cuda.synchronize()
            st = model._store
            before = None
            if kind == "lazy":          # before the final flush: what this rank holds, for the comparison between ranks
                o, n = st.index[TABLE]
                before = (pending, tr.opt.tables_pending, [_bits(x[o:o + n]) for x in (st.flat, tr.opt.m, tr.opt.v, tr.ema.shadow)],
                          tr.opt._lazy[TABLE]["stamps"].cpu().numpy())
                tr.opt.flush_tables()
                torch.cuda.synchronize()
                assert tr.opt.tables_pending == 0 and bool((tr.opt._lazy[TABLE]["stamps"] == DP_STEPS).all())
            else:
                assert pending == 0 and not tr.opt._lazy
            out[kind] = (before, [_bits(x[:st.n_live]) for x in (st.flat, tr.opt.m, tr.opt.v, tr.ema.shadow)],
                         {k: _bits(v) for k, v in tr.ema.state_dict().items() if v.dtype == torch.float32})
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def _collect(procs, q, n_msgs, limit=300.0):
    """``n_msgs`` messages from the children; a child that ends with an error ends the wait at once."""
    import time
    got, t0 = [], time.monotonic()
    while len(got) < n_msgs:
        try:
            got.append(q.get(timeout=0.5))
        except queue_mod.Empty:
            bad = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
            assert not bad, "a rank failed (exit codes %s)" % bad
            assert time.monotonic() - t0 < limit, "no result from the ranks"
    return got


@pytest.mark.parametrize("mode", ["eager", "recorded"])
def test_trainer_data_parallel_lazy_ema_equals_dense_ema(mode):
    assert _check_id_lists(None if mode == "eager" else 3)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29600 + (os.getpid() + (5 if mode == "recorded" else 0)) % 250
    procs = [ctx.Process(target=_dp_child, args=(r, port, mode, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    try:
        msgs = dict(_collect(procs, q, WORLD))
    finally:
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.kill()
                p.join()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert sorted(msgs) == list(range(WORLD))
    names = ("p", "m", "v", "shadow")
    for r, out in msgs.items():
        pending_max, pending_end, held, stamps = out["lazy"][0]
        assert pending_max > 0 and pending_end > 0, "rank %d: nothing was ever pending" % r
        held0, stamps0 = msgs[0]["lazy"][0][2:]
        assert (stamps == stamps0).all() and int(stamps.min()) < DP_STEPS == int(stamps.max())
        for name, a, b in zip(names, held, held0):
            assert (a == b).all(), "rank %d holds another table %s than rank 0 before the flush" % (r, name)
        o_d, o_l = out["dense"], out["lazy"]
        for name, a, b in zip(names, o_d[1], o_l[1]):
            assert a.shape == b.shape and (a == b).all(), "rank %d: %s differs from the dense data-parallel EMA run" % (r, name)
        assert set(o_d[2]) == set(o_l[2]) and TABLE in o_d[2]
        for k in o_d[2]:
            assert (o_d[2][k] == o_l[2][k]).all(), "rank %d: ema.state_dict()[%s] differs" % (r, k)
        assert not (o_l[1][3] == o_l[1][0]).all()          # (the shadow is an average, not the weights)
