"""Lazy exact AdamW of the item-id table under data parallelism, on the device.  Every comparison is BITWISE (int32 views) and the
yardstick is code the project had before segmm_adamw_table_lazy_rows existed -- the four launches it fuses (catch-up, ring push,
phase 1, stamp), phase 0 + phase 1 of segmm_adamw_table_lrs, or the dense data-parallel Trainer -- never the new kernel.
tests/test_lazy_dp_cpu.py shows on the host that such a comparison rejects a wrong ring slot, a skipped step and a duplicate stepped
twice.

1. the kernel: 12 steps, ring of 4, a prefix of each list caught up ahead (the rank's own ids), the whole list through lazy_rows;
2. idempotence: a second lazy_rows at the same T reads and writes nothing (its gradient is NaN);
3. Trainer(lazy_tables=dict(flush_every=4, data_parallel=True)) against the dense trainer on 2 and 4 ranks sharing the GPU over gloo
   and through one forced RCCL rank, eager and recorded;
4. the refusals, and the single-process step launch for launch."""
import os
import queue as queue_mod
import sys
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from helpers import ROOT, build_model, load_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
OFF, GUARD = 96, 32          # where a table sits inside its buffers, and the untouched floats checked behind it
B1, B2, EPS = 0.9, 0.999, 1e-8
STEPS, CAP = 12, 4


def _H():
    from segmminterest_amd import hipabi as H
    H.lib()
    return H


def _i32(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return bool((_i32(a) == _i32(b)).all())


@pytest.fixture
def own_step_state():
    """A step state of the test's own, bound for the test; the library's default state is bound again afterwards."""
    H = _H()
    state = torch.zeros((H.step_state_bytes() + 3) // 4, dtype=torch.int32, device=DEV)
    H.step_bind(state)
    try:
        yield state
    finally:
        torch.cuda.synchronize()
        H.step_bind(None)


def _buffers(rows, width, seed):
    """p, m, v: a non-trivial table state at float OFF of buffers filled with other numbers."""
    g = torch.Generator().manual_seed(seed)
    n, size = rows * width, OFF + rows * width + GUARD
    out = []
    for k in range(3):
        h = 1000.0 + 100.0 * torch.randn(size, generator=g)
        t = torch.randn(n, generator=g)
        h[OFF:OFF + n] = (0.05 * t, 0.1 * t, 0.01 * (0.25 + 0.75 * torch.rand(n, generator=g)))[k]
        out.append(h)
    return out


def _id_lists(rows, n_ids, seed):
    """One id list per step (tests/test_lazy_tables_gpu.py's recipe): duplicates, ids outside the table; step 5 lists nothing; row 3
    is never listed.  On the host: the protocol is walked from these lists alone."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(STEPS):
        ids = torch.randint(0, rows, (n_ids,), generator=g)
        ids[ids == 3] = 4
        ids = torch.cat([ids[:n_ids // 2], ids[:n_ids // 4], torch.tensor([-1, rows, rows + 7, -2 ** 40]), ids[n_ids // 2:]])
        out.append((ids if k != 5 else ids[:0]).to(torch.int64))
    return out


def _own(ids):
    """The prefix of a step's list that plays the rank's own ids (caught up ahead of the forward)."""
    return ids[:(ids.numel() + 2) // 3]


def _gaps(id_lists, rows):
    """From the lists alone: for every step, {row: steps the row is behind T - 1 when lazy_rows reaches it} for the rows OUTSIDE the
    prefix, and the same for all rows -- the flush rule (CAP pending) and the stamps walked on the host."""
    stamps, flushed = [0] * rows, 0
    outside, every = [], []
    for k, ids in enumerate(id_lists):
        T = k + 1
        if T - 1 - flushed >= CAP:
            stamps, flushed = [T - 1] * rows, T - 1
        own = {int(r) for r in _own(ids) if 0 <= int(r) < rows}
        listed = {int(r) for r in ids if 0 <= int(r) < rows}
        every.append({r: T - 1 - stamps[r] for r in listed})
        outside.append({r: T - 1 - stamps[r] for r in listed - own})
        for r in listed:
            stamps[r] = T
    return outside, every


KERNEL_CASES = [(257, 8, "plain"), (300, 256, "plain"), (300, 384, "plain"), (300, 384, "scaled_nodecay"), (300, 384, "clip"),
                (257, 8, "state"), (300, 384, "state")]


@pytest.mark.parametrize("rows,width,variant", KERNEL_CASES, ids=["%dx%d-%s" % c for c in KERNEL_CASES])
def test_lazy_rows_equals_the_four_launches_and_the_dense_update_bitwise(rows, width, variant, own_step_state):
    """12 steps at a rate that changes every step, ring of 4, a flush whenever 4 steps are pending and at the end.  Three copies of one
    table: FUSED -- catch-up of the list's prefix (the own ids) to T - 1 without flags, the ring's entry of T, lazy_rows on the whole
    list; FOUR -- catch-up of the whole list with flags, the ring's entry, phase 1, the stamp; DENSE -- phase 0 + phase 1.  After every
    step FUSED and FOUR hold the same bits and stamps; at the end all three agree, every stamp is 12, the floats around the table are
    untouched.  Widths 8, 256, 384: width / 4 below, at and above one wave's 64 lanes; 41 + 4 list entries: no multiple of 4."""
    H = _H()
    n = rows * width
    scale, wd = (0.5, 0.0) if variant == "scaled_nodecay" else (1.0, 1e-2)
    coef = torch.tensor([0.37], device=DEV) if variant == "clip" else None
    live = variant == "state"
    host_lists = _id_lists(rows, 41, rows + width)
    outside, every = _gaps(host_lists, rows)
    # the lists make the run a test of the replay inside lazy_rows: rows the prefix did not catch up, two or more steps behind, and
    # a row that needs the whole ring but one slot
    assert any(gap >= 2 for step in outside for gap in step.values())
    assert any(gap == CAP - 1 for step in every for gap in step.values())
    assert any(len(ids) % 4 for ids in host_lists) and not any(3 in ids.tolist() for ids in host_lists)
    id_lists = [ids.to(DEV) for ids in host_lists]
    host = _buffers(rows, width, rows * 7 + width)
    fused, four, dense = ([h.clone().to(DEV) for h in host] for _ in range(3))
    gen = torch.Generator().manual_seed(11)
    st_f, st_4 = (torch.zeros(rows, dtype=torch.int32, device=DEV) for _ in range(2))
    hist_f, hist_4 = (torch.zeros((CAP, 4), device=DEV) for _ in range(2))
    flags_4, flags_d = (torch.zeros(rows, dtype=torch.int32, device=DEV) for _ in range(2))
    flushed = 0
    for k, ids in enumerate(id_lists):
        T = k + 1
        g = torch.zeros(OFF + n + GUARD)
        g[OFF:OFF + n] = torch.randn(n, generator=gen)
        g = g.to(DEV)
        lr = H.LIVE_LR if live else 1e-3 * (1.0 + 0.3 * k)
        step = -1 if live else T
        if T - 1 - flushed >= CAP:          # the flush rule: the ring holds the last CAP steps
            for bufs, stamps, hist in ((fused, st_f, hist_f), (four, st_4, hist_4)):
                H.adamw_table_catchup(*bufs, OFF, rows, width, None, stamps, hist, T - 1, scale, B1, B2, EPS, wd)
            flushed = T - 1
        if live:
            if k == 0:
                H.step_set(1234, 0, B1, B2)
                H.step_schedule("cosine", 2e-3, warmup_steps=2, start_factor=0.5, decay_steps=9, eta_min=1e-4)
            H.step_advance(B1, B2)
        target = -1 if live else T - 1
        H.adamw_table_lrs(dense[0], None, dense[1], dense[2], OFF, rows, width, ids, flags_d, lr, scale, B1, B2, EPS, wd, step, 0)
        H.adamw_table_lrs(dense[0], g, dense[1], dense[2], OFF, rows, width, ids, flags_d, lr, scale, B1, B2, EPS, wd, step, 1, coef=coef)
        H.adamw_table_catchup(*four, OFF, rows, width, ids, st_4, hist_4, target, scale, B1, B2, EPS, wd, relative=live, flags=flags_4)
        H.adamw_hist_push(hist_4, lr, B1, B2, step)
        H.adamw_table_lrs(four[0], g, four[1], four[2], OFF, rows, width, ids, flags_4, lr, scale, B1, B2, EPS, wd, step, 1, coef=coef)
        H.adamw_table_stamp(ids, rows, st_4, 0 if live else T, relative=live)
        H.adamw_table_catchup(*fused, OFF, rows, width, _own(ids), st_f, hist_f, target, scale, B1, B2, EPS, wd, relative=live)
        H.adamw_hist_push(hist_f, lr, B1, B2, step)
        H.adamw_table_lazy_rows(fused[0], g, fused[1], fused[2], OFF, rows, width, ids, st_f, hist_f, lr, scale, B1, B2, EPS, wd, step, coef=coef)
        torch.cuda.synchronize()
        assert bool((st_f == st_4).all()), "stamps differ from the four launches' after step %d" % T
        for name, a, b in zip("pmv", fused, four):
            assert _same(a, b), "%s differs from the four launches after step %d" % (name, T)
    assert int(st_f[3]) == flushed < STEPS          # the row never listed is behind until the flush
    H.adamw_table_catchup(*fused, OFF, rows, width, None, st_f, hist_f, STEPS, scale, B1, B2, EPS, wd)
    torch.cuda.synchronize()
    assert bool((st_f == STEPS).all()) and int(flags_d.abs().sum()) == 0
    for name, a, b, h in zip("pmv", fused, dense, host):
        assert _same(a[OFF:OFF + n], b[OFF:OFF + n]), "%s differs from the dense update" % name
        assert not _same(a[OFF:OFF + n], h[OFF:OFF + n].to(DEV))
        assert _same(a[:OFF], h[:OFF].to(DEV)) and _same(a[OFF + n:], h[OFF + n:].to(DEV)), "%s: floats around the table moved" % name


@pytest.mark.parametrize("width", [8, 256, 384])
def test_lazy_rows_is_idempotent_and_reads_no_unclaimed_row(width):
    """A second lazy_rows on the same list at the same T changes no bit of p, m, v or the stamps, although its gradient is NaN
    everywhere: a row that is not claimed is not read into the result.  (The first call moved every listed row.)"""
    H = _H()
    rows, T = 64, 3
    n = rows * width
    bufs = [h.to(DEV) for h in _buffers(rows, width, 5)]
    hist = torch.tensor([[0.0, 1.0, 1.0, 0.0], [1e-3, 0.1, 0.0316, 0.0], [2e-3, 0.19, 0.0447, 0.0], [3e-3, 0.271, 0.0547, 0.0]], device=DEV)
    stamps = (torch.arange(rows, dtype=torch.int32) % 3).to(DEV)          # 0, 1 or 2 steps taken: gaps 2, 1 and 0
    g = torch.zeros(OFF + n + GUARD)
    g[OFF:OFF + n] = torch.randn(n, generator=torch.Generator().manual_seed(3))
    g = g.to(DEV)
    listed = torch.arange(0, rows, 2)
    ids = torch.cat([listed, listed, torch.tensor([-5, rows])]).to(torch.int64).to(DEV)          # every other row, twice; two ids outside
    before = [b.clone() for b in bufs]
    H.adamw_table_lazy_rows(*bufs[:1], g, *bufs[1:], OFF, rows, width, ids, stamps, hist, 3e-3, 1.0, B1, B2, EPS, 1e-2, T)
    torch.cuda.synchronize()
    once, stamps_once = [b.clone() for b in bufs], stamps.clone()
    H.adamw_table_lazy_rows(*bufs[:1], torch.full_like(g, float("nan")), *bufs[1:], OFF, rows, width, ids, stamps, hist, 3e-3, 1.0, B1, B2, EPS,
                            1e-2, T)
    torch.cuda.synchronize()
    on = torch.zeros(rows, dtype=torch.bool, device=DEV)
    on[listed.to(DEV)] = True
    assert bool((stamps == stamps_once).all()) and bool((stamps[on] == T).all())
    assert bool((stamps[~on] == (torch.arange(rows, device=DEV)[~on] % 3)).all())
    for name, a, o, b in zip("pmv", bufs, once, before):
        assert _same(a, o), "%s: the second lazy_rows changed bits" % name
        assert not bool(torch.isnan(a[OFF:OFF + n]).any())
        ra, rb = a[OFF:OFF + n].view(rows, width), b[OFF:OFF + n].view(rows, width)
        assert _same(ra[~on], rb[~on]), "%s: a row outside the list was touched" % name
        assert not bool((_i32(ra[on]) == _i32(rb[on])).all(dim=1).any()), "%s: a listed row did not move" % name
        assert _same(a[:OFF], b[:OFF]) and _same(a[OFF + n:], b[OFF + n:])


# ------------------------------------------------------------------------------------------------ 3. the trainer, data parallel
TABLE = "backbone1.vid_proj.weight"
N_ITEMS, GLOBAL_B, DP_STEPS, FLUSH = 97, 16, 14, 4
LAZY_DP = dict(flush_every=FLUSH, data_parallel=True)
SCHED = dict(kind="cosine", warmup_steps=3, decay_steps=12, eta_min=1e-4)


def _cfg():
    cfg, _, _, _ = load_case("id_d32_N2")
    S = 20
    return dict(cfg, S=S, Lt=1, n_items=N_ITEMS, exposure_prob=list(cfg["exposure_prob"])[:S])


def _full_batches():
    """The 14 global batches (CPU): the item ids differ from step to step, drawn from the 97."""
    from segmminterest_amd.synth import make_batch
    cfg = _cfg()
    return [make_batch(GLOBAL_B, cfg["S"], cfg["Lt"], cfg["D_in"], n_users=cfg["n_users"], n_items=N_ITEMS, seed=4100 + i) for i in range(DP_STEPS)]


def _check_id_lists(world, record_at=None):
    """From the id lists alone (the flush rule and the stamps walked on the host; ``record_at``: record() flushes ahead of that step):
    some step has an id on two ranks, and some step brings rank 0 an id that only another rank holds and whose row is two or more
    steps behind -- the replay inside lazy_rows."""
    from segmminterest_amd.trainer import shard_rows
    stamps, flushed = {}, 0
    shared = far = False
    for k, b in enumerate(_full_batches()):
        T = k + 1
        if T - 1 - flushed >= FLUSH or T == record_at:
            stamps, flushed = {}, T - 1
        ids = b["photo_identity_id"].tolist()
        per_rank = [set(ids[s:e]) for s, e in (shard_rows(GLOBAL_B, world, r) for r in range(world))]
        shared |= any(per_rank[a] & per_rank[b_] for a in range(world) for b_ in range(a + 1, world))
        others = set().union(*per_rank[1:]) - per_rank[0] if world > 1 else set()
        far |= any(T - 1 - stamps.get(r, flushed) >= 2 for r in others)
        for r in ids:
            stamps[r] = T
    return shared, far


def _dp_child(rank, world, port, backend, mode, q):
    """One rank on cuda:0: the dense data-parallel trainer, then the lazy one, same seeds, same shards.  mode: ``eager``;
    ``recorded`` (device step state; the lazy run records step 3 and replays 4..14, the dense run stays eager); ``clipped``
    (recorded, with max_grad_norm, a cosine schedule and no_decay_groups)."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      SEGMM_DP_FORCE="1" if world == 1 else "0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from segmminterest_amd.trainer import DPComm, Trainer, no_decay_groups, shard_rows
    torch.cuda.set_device(0)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg = _cfg()
        s, e = shard_rows(GLOBAL_B, world, rank)
        shards = [{k: v[s:e].contiguous().cuda() for k, v in f.items()} for f in _full_batches()]
        out = {}
        for kind in ("dense", "lazy"):
            torch.manual_seed(5)
            model = build_model(cfg).cuda()
            kw = dict(comm=DPComm(), overlap=True, dropout=False, weight_decay=1e-2, device_state=mode != "eager")
            if mode == "clipped":
                kw.update(max_grad_norm=0.05, lr_schedule=SCHED, param_groups=no_decay_groups(model))
            if kind == "lazy":
                kw["lazy_tables"] = LAZY_DP
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
            if kind == "lazy":          # before the final flush: what this rank holds, for the comparison between ranks
                o, n = st.index[TABLE]
                q.put(("rank", rank, pending, tr.opt.tables_pending,
                       [x[o:o + n].detach().cpu().numpy().view(np.int32) for x in (st.flat, tr.opt.m, tr.opt.v)],
                       tr.opt._lazy[TABLE]["stamps"].cpu().numpy()))
                tr.opt.flush_tables()
                torch.cuda.synchronize()
                assert tr.opt.tables_pending == 0 and bool((tr.opt._lazy[TABLE]["stamps"] == DP_STEPS).all())
            else:
                assert pending == 0 and not tr.opt._lazy
            out[kind] = ({k: v.detach().cpu().numpy().view(np.int32) for k, v in model.state_dict().items() if v.dtype == torch.float32},
                         tr.opt.m.cpu().numpy().view(np.int32), tr.opt.v.cpu().numpy().view(np.int32))
        if rank == 0:
            q.put(("final", out))
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


DP_CASES = [(2, "gloo", "eager"), (2, "gloo", "clipped"), (4, "gloo", "eager"), (1, "nccl", "recorded")]


@pytest.mark.parametrize("world,backend,mode", DP_CASES, ids=["%d-%s-%s" % c for c in DP_CASES])
def test_trainer_data_parallel_lazy_equals_dense(world, backend, mode):
    """14 steps on a global batch of 16 over ``world`` ranks (gloo: the ranks share the GPU, collectives staged through the host;
    nccl: one forced RCCL rank), flush_every = 4: after ``flush_tables()`` the state dict and both moments of rank 0 equal the dense
    data-parallel trainer's in every bit.  Before that flush the ranks hold the same table, moments and stamps, and rows were
    pending (the run was not dense in disguise)."""
    shared, far = _check_id_lists(world, None if mode == "eager" else 3)
    if world > 1:
        assert shared and far
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29300 + (os.getpid() + 7 * world + (3 if mode == "clipped" else 0)) % 250
    procs = [ctx.Process(target=_dp_child, args=(r, world, port, backend, mode, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        msgs = _collect(procs, q, world + 1)
    finally:
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.kill()
                p.join()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    ranks = {m[1]: m[2:] for m in msgs if m[0] == "rank"}
    (final,) = [m[1] for m in msgs if m[0] == "final"]
    assert sorted(ranks) == list(range(world))
    for r, (pending_max, pending_end, pmv, stamps) in ranks.items():
        assert pending_max > 0 and pending_end > 0, "rank %d: nothing was ever pending" % r
        assert (stamps == ranks[0][3]).all() and int(stamps.min()) < DP_STEPS == int(stamps.max())
        for name, a, b in zip("pmv", pmv, ranks[0][2]):
            assert (a == b).all(), "rank %d holds another table %s than rank 0 before the flush" % (r, name)
    (sd_d, m_d, v_d), (sd_l, m_l, v_l) = final["dense"], final["lazy"]
    assert set(sd_d) == set(sd_l) and TABLE in sd_d
    for k in sd_d:
        assert (sd_d[k] == sd_l[k]).all(), "%s differs from the dense data-parallel run" % k
    assert (m_d == m_l).all() and (v_d == v_l).all()


# ------------------------------------------------------------------------------------------------ 4. refusals, the unchanged default
def test_refusals_and_the_unchanged_single_process_step(monkeypatch):
    from segmminterest_amd.synth import make_batch
    from segmminterest_amd.trainer import Trainer
    cfg = _cfg()
    model = build_model(cfg).to(DEV)
    active = types.SimpleNamespace(active=True)
    with pytest.raises(ValueError, match="DPComm"):
        Trainer(model, lazy_tables=True, comm=active)
    with pytest.raises(ValueError, match="DPComm.*data_parallel=True"):
        Trainer(model, lazy_tables=dict(flush_every=4), comm=active)
    for comm in (None, active):
        with pytest.raises(ValueError, match="data_parallel must be a bool"):
            Trainer(model, lazy_tables=dict(data_parallel=1), comm=comm)
    with pytest.raises(ValueError, match="micro_batch"):
        Trainer(model, lazy_tables=LAZY_DP, comm=active, micro_batch=8)
    with pytest.raises(ValueError, match="sparse_tables"):
        Trainer(model, lazy_tables=LAZY_DP, comm=active, sparse_tables=False)
    monkeypatch.setenv("SEGMM_SPARSE_TABLES", "0")
    with pytest.raises(ValueError, match="SEGMM_SPARSE_TABLES"):
        Trainer(model, lazy_tables=LAZY_DP, comm=active)
    monkeypatch.delenv("SEGMM_SPARSE_TABLES")
    with pytest.raises(ValueError, match="ema"):
        Trainer(model, lazy_tables=LAZY_DP, ema=0.99)
    # a single process: the key is accepted and changes nothing -- the recorded step holds the same commands, the run the same bits
    bs = [{k: v.to(DEV) for k, v in make_batch(8, cfg["S"], cfg["Lt"], cfg["D_in"], n_users=cfg["n_users"], n_items=N_ITEMS, seed=700 + i).items()}
          for i in range(7)]
    runs = []
    for lazy in (dict(flush_every=4), LAZY_DP):
        torch.manual_seed(5)
        tr = Trainer(build_model(cfg).to(DEV), dropout=False, device_state=True, lazy_tables=lazy)
        assert not tr._lazy_dp and tr.opt.lazy_data_parallel == bool(lazy.get("data_parallel"))
        tr.train_step(bs[0])
        tr.train_step(bs[1])
        tr.record(bs[2], warmup=0, prev_batch=bs[1])
        for b in bs[3:]:
            tr.run_recorded(b)
        assert TABLE in tr.opt._lazy and tr.opt.tables_pending > 0 and not tr.opt._lazy_tail
        ops = [(ph.kind, ph.backbone, ph.layer, [(arr[i].op, arr[i].stream) for i in range(ph.n_cmds)])
               for ph, arr in tr._recorded["phases"] if arr is not None]
        torch.cuda.synchronize()
        runs.append((ops, [x.detach().clone() for x in (tr.model._store.flat, tr.opt.m, tr.opt.v)]))
    names = _H().op_ids()
    used = {op for p in runs[0][0] for op, _ in p[3]}
    assert names["segmm_adamw_table_catchup"] in used and names["segmm_adamw_table_stamp"] in used
    assert names["segmm_adamw_table_lazy_rows"] not in used
    assert runs[0][0] == runs[1][0], "the recorded phases, entry points or stream slots differ"
    assert all(_same(a, b) for a, b in zip(runs[0][1], runs[1][1]))
