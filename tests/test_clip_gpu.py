"""Global-norm gradient clipping on the MI355X (FusedAdamW / Trainer ``max_grad_norm``): the norm kernel against float64, the
scaled AdamW bit for bit against AdamW on the pre-scaled gradient, the optimizer against torch's clip_grad_norm_ + AdamW, an
inactive clip bit-identical to no clip, the trainer against the CPU oracle, and the recorded and data-parallel steps."""
import math
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp

from helpers import ROOT, build_model, call_model, load_case

pytestmark = pytest.mark.gpu
DEV = "cuda"

sys.path.insert(0, os.path.join(ROOT, "oracle"))


def _torch_coef(norm, max_norm):
    """torch.nn.utils.clip_grad_norm_'s coefficient for an fp32 norm, evaluated by torch (fp32, CPU)."""
    return torch.clamp(max_norm / (torch.tensor(norm, dtype=torch.float32) + 1e-6), max=1.0)


def _bufs():
    from segmminterest_amd import hipabi as H
    return torch.zeros(H.GRAD_NORM_SCRATCH, dtype=torch.float64, device=DEV), torch.zeros(2, dtype=torch.float32, device=DEV)


# ------------------------------------------------------------------------------------------------ 1. the norm kernel
@pytest.mark.parametrize("kind", ["randn", "tiny", "huge", "zero"])
def test_grad_norm_kernel_vs_float64(kind):
    """segmm_grad_norm over ranges of any length and float offset: the 2-norm to 2^-22 relative of the float64 norm (data near
    1e-20 and 1e19: fp32 squares would underflow / overflow, the fp64 partials do not), the coefficient bit-equal to torch's
    fp32 formula evaluated on the returned norm, and bitwise the same outputs on a second run."""
    from segmminterest_amd import hipabi as H
    scratch, out2 = _bufs()
    gen = torch.Generator().manual_seed(7)
    for n in (1, 3, 4, 1_000_003, 6_400_000):
        for off in (0, 1):
            x = torch.randn(n + off, generator=gen)
            x = {"randn": x, "tiny": x * 1e-20, "huge": x * 1e19, "zero": torch.zeros_like(x)}[kind]
            xd = x.to(DEV)
            ref = float(torch.linalg.vector_norm(x[off:].double()))
            for m in (0.5 * ref if ref > 0 else 1.0, 1.0, math.inf):
                H.grad_norm(xd, n, m, scratch, out2, off=off)
                first = out2.cpu().clone()
                scratch.fill_(float("nan"))          # nothing of a previous call may leak into the next
                H.grad_norm(xd, n, m, scratch, out2, off=off)
                again = out2.cpu()
                assert torch.equal(first.view(torch.int32), again.view(torch.int32)), (n, off, m)
                t, c = float(first[0]), first[1]
                if ref == 0.0:
                    assert t == 0.0
                else:
                    assert abs(t - ref) <= 2.0 ** -22 * ref, (n, off, t, ref)
                want = torch.tensor(1.0) if m == math.inf else _torch_coef(t, m)
                assert torch.equal(c.view(torch.int32), want.view(torch.int32)), (n, off, m, float(c), float(want))


def test_grad_norm_kernel_non_finite():
    """One inf or one NaN element gives the norm torch computes (inf / NaN) and torch's coefficient (0 / NaN); max_norm = inf
    still gives coef = 1."""
    from segmminterest_amd import hipabi as H
    scratch, out2 = _bufs()
    for bad in (math.inf, -math.inf, math.nan):
        x = torch.randn(100_003, generator=torch.Generator().manual_seed(3))
        x[77_777] = bad
        p = torch.nn.Parameter(torch.zeros_like(x))
        p.grad = x.clone()
        tn = torch.nn.utils.clip_grad_norm_([p], 2.0)
        H.grad_norm(x.to(DEV), x.numel(), 2.0, scratch, out2)
        t, c = out2.cpu()
        want_c = _torch_coef(float(tn), 2.0)
        if math.isnan(bad):
            assert math.isnan(float(t)) and math.isnan(float(tn)) and math.isnan(float(c)) and math.isnan(float(want_c))
        else:
            assert float(t) == float(tn) == math.inf and float(c) == float(want_c) == 0.0
        H.grad_norm(x.to(DEV), x.numel(), math.inf, scratch, out2)
        assert float(out2[1]) == 1.0 and (math.isnan(float(out2[0])) if math.isnan(bad) else float(out2[0]) == math.inf)


# ------------------------------------------------------------------------------------------------ 2. the scaled AdamW
@pytest.mark.parametrize("c", [0.3712345, 1.0, 2.0 ** -30])
def test_scaled_adamw_is_adamw_on_the_scaled_gradient(c):
    """segmm_adamw_scaled(g, coef = &c) == segmm_adamw(fp32(g * c)) bit for bit (flat ranges with n % 4 != 0, steps 1 and 5);
    with c == 1 also == segmm_adamw(g)."""
    from segmminterest_amd import hipabi as H
    gen = torch.Generator().manual_seed(11)
    coef = torch.tensor([c], dtype=torch.float32, device=DEV)
    for n in (1, 7, 1001, 262_147):
        p0, g, m0 = (torch.randn(n, generator=gen).to(DEV) for _ in range(3))
        v0 = torch.rand(n, generator=gen).to(DEV) * 1e-3
        gs = g * coef          # fp32 product on the device: torch's g.mul_(clip_coef)
        for step in (1, 5):
            a = [t.clone() for t in (p0, m0, v0)]
            b = [t.clone() for t in (p0, m0, v0)]
            H.adamw(a[0], g, a[1], a[2], n, 1e-3, 0.9, 0.999, 1e-8, 1e-4, step, coef=coef)
            H.adamw(b[0], gs, b[1], b[2], n, 1e-3, 0.9, 0.999, 1e-8, 1e-4, step)
            for x, y in zip(a, b):
                assert torch.equal(x, y), (n, step)
            if c == 1.0:
                u = [t.clone() for t in (p0, m0, v0)]
                H.adamw(u[0], g, u[1], u[2], n, 1e-3, 0.9, 0.999, 1e-8, 1e-4, step)
                for x, y in zip(a, u):
                    assert torch.equal(x, y), (n, step)
            assert not torch.equal(a[0], p0)


@pytest.mark.parametrize("c", [0.3712345, 1.0])
def test_scaled_adamw_table_rows(c):
    """Phase 1 of the two-pass table update with a device-side scale == the unscaled phase 1 on fp32(g * c), bit for bit, for an
    id list with duplicates and ids outside the table; the flags end at zero."""
    from segmminterest_amd import hipabi as H
    gen = torch.Generator().manual_seed(5)
    rows, width = 300, 24
    n = rows * width
    coef = torch.tensor([c], dtype=torch.float32, device=DEV)
    ids = torch.tensor([5, 17, 5, -1, 299, 300, 0, 17, 17, 1000, 42], dtype=torch.int64, device=DEV)
    p0, m0 = (torch.randn(n, generator=gen).to(DEV) for _ in range(2))
    v0 = torch.rand(n, generator=gen).to(DEV) * 1e-3
    g = torch.zeros(rows, width)
    for r in (5, 17, 299, 0, 42):
        g[r] = torch.randn(width, generator=gen)
    g = g.view(-1).to(DEV)
    gs = g * coef
    res = []
    for scaled in (True, False):
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        flags = torch.zeros(rows, dtype=torch.int32, device=DEV)
        H.adamw_table(p, None, m, v, 0, rows, width, ids, flags, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 2, 0)
        H.adamw_table(p, g if scaled else gs, m, v, 0, rows, width, ids, flags, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 2, 1,
                      coef=coef if scaled else None)
        assert int(flags.abs().sum()) == 0
        res.append((p, m, v))
    for x, y in zip(*res):
        assert torch.equal(x, y)
    if c == 1.0:
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        flags = torch.zeros(rows, dtype=torch.int32, device=DEV)
        H.adamw_table(p, None, m, v, 0, rows, width, ids, flags, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 2, 0)
        H.adamw_table(p, g, m, v, 0, rows, width, ids, flags, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 2, 1)
        for x, y in zip(res[0], (p, m, v)):
            assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ 3. FusedAdamW vs torch
def _loaded(name):
    cfg, g, nograd, extra = load_case(name)
    model = build_model(cfg)
    model.load_state_dict(g["sd"])
    model = model.cuda()
    model.eval()
    return cfg, g, nograd, model


@pytest.mark.parametrize("name", ["img_d32_N2", "id_d32_N2", "both_fh2"])
def test_fused_adamw_clip_matches_torch_clip_and_adamw(name):
    """3 steps of call_model -> backward -> FusedAdamW(max_grad_norm=m).step() against torch.nn.utils.clip_grad_norm_ +
    torch.optim.AdamW in float64 on a copy of the parameters, fed the SAME gradients (the engine's), m = 0.25 x the first norm so
    that every step clips.  Tolerance: per step the fp32 kernel rounds the decayed weight and the update (a few units of 2^-24 of
    |p|), and the update lr * m_hat / (sqrt(v_hat) + eps) -- at most ~lr in magnitude -- carries the relative error of its fp32
    moments, bias corrections and coefficient (~10 roundings: ~1e-6 of lr): |p - p_ref| <= steps * (2^-20 |p_ref| + 1e-5 lr), a
    margin of ~4 over both.  The reported norm is
    torch's to 2^-20; ``.grad`` keeps the unclipped gradient."""
    from segmminterest_amd.trainer import FusedAdamW
    cfg, g, nograd, model = _loaded(name)
    lr, wd = 1e-3, 1e-4
    ref = None
    opt = None
    for step in range(1, 4):
        model.zero_grad(set_to_none=True)
        out = call_model(model, g["in"], "train", DEV)
        out["loss"].backward()
        live = [(k, p) for k, p in model.named_parameters() if p.grad is not None]
        grads = {k: p.grad.detach().clone() for k, p in live}
        if opt is None:
            norm0 = float(torch.sqrt(sum((gr.double() ** 2).sum() for gr in grads.values())))
            max_norm = 0.25 * norm0
            opt = FusedAdamW(model, lr=lr, weight_decay=wd, max_grad_norm=max_norm)
            ref = {k: p.detach().double().cpu().clone().requires_grad_(True) for k, p in live}
            topt = torch.optim.AdamW(list(ref.values()), lr=lr, weight_decay=wd, foreach=False)
        for k, gr in grads.items():
            ref[k].grad = gr.double().cpu()
        tn = float(torch.nn.utils.clip_grad_norm_(list(ref.values()), max_norm))
        topt.step()
        opt.step()
        got = float(opt.grad_norm)
        assert opt.grad_norm.dim() == 0 and opt.grad_norm.is_cuda
        assert abs(got - tn) <= 2.0 ** -20 * tn, (step, got, tn)
        assert tn > max_norm and float(opt._clip_out[1]) < 1.0          # the clip is active
        for k, p in live:
            assert torch.equal(p.grad, grads[k]), k          # the unclipped gradient
            want = ref[k].detach()
            err = (p.detach().double().cpu() - want).abs()
            lim = step * (2.0 ** -20 * want.abs() + 1e-5 * lr)
            assert bool((err <= lim).all()), (step, k, float((err - lim).max()))
    for k, p in model.named_parameters():
        if k in nograd:
            assert torch.equal(p.detach().cpu(), g["sd"][k]), k


# ------------------------------------------------------------------------------------------------ 4. an inactive clip is free
def _trainer_run(name, max_grad_norm, steps=3, **kw):
    from segmminterest_amd.synth import make_batch
    from segmminterest_amd.trainer import Trainer
    cfg, g, _, _ = load_case(name)
    torch.manual_seed(0)
    model = build_model(cfg)
    model.load_state_dict(g["sd"])
    model = model.cuda()
    tr = Trainer(model, dropout=False, max_grad_norm=max_grad_norm, **kw)
    batch = {k: v.to(DEV) for k, v in make_batch(16, cfg["S"], cfg["Lt"], cfg["D_in"], n_users=cfg.get("n_users", 5) or 5,
                                                  n_items=cfg.get("n_items", 5) or 5, seed=3).items()}
    norms = []
    for _ in range(steps):
        tr.train_step(batch)
        if tr.opt.grad_norm is not None:
            norms.append(tr.opt.grad_norm.clone())
    torch.cuda.synchronize()
    return model._store.flat.detach().clone(), tr.opt.m.clone(), [float(x) for x in norms], cfg, g, model


@pytest.mark.parametrize("name", ["img_d32_N2", "id_d32_N2"])
def test_inactive_clip_is_bit_identical_to_no_clip(name):
    """max_grad_norm = 1e30 (coef clamps to exactly 1) and = inf leave the parameters and moments bit-identical to
    max_grad_norm = None after 3 train_steps, and still report the norm."""
    p0, m0, n0, *_ = _trainer_run(name, None)
    assert n0 == []
    norms = {}
    for mg in (1e30, math.inf):
        p1, m1, norms[mg], *_ = _trainer_run(name, mg)
        assert torch.equal(p0, p1) and torch.equal(m0, m1), mg
        assert len(norms[mg]) == 3 and all(math.isfinite(x) and x > 0 for x in norms[mg]), norms[mg]
    assert norms[1e30] == norms[math.inf]


# ------------------------------------------------------------------------------------------------ 5. end to end vs the oracle
def test_trainer_clip_matches_oracle():
    """3 steps of Trainer(max_grad_norm=m) (active on every step) against oracle.forward_backward + a float64 clip +
    oracle.adamw_step, with the tolerance rule of test_fused_adamw_optimizer_matches_reference."""
    import segmm_oracle as O
    from segmminterest_amd.synth import l1_normalize, make_batch
    from segmminterest_amd.trainer import Trainer
    cfg, g, nograd, _ = load_case("img_d32_N2")
    model = build_model(cfg)
    model.load_state_dict(g["sd"])
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    b = make_batch(16, cfg["S"], cfg["Lt"], cfg["D_in"], seed=3)
    inp = dict(usr_image=l1_normalize(b["user"]), usr_id=b["user_identity_id"], usr_mask=b["user_mask"],
               vid_image=l1_normalize(b["photo"]), vid_id=b["photo_identity_id"], vid_mask=b["photo_mask"], gt=b["label"])
    names = [k for k, _ in model.named_parameters()]
    params = {k: v.clone() for k, v in sd.items()}
    mom = {k: torch.zeros_like(v) for k, v in params.items() if v.is_floating_point()}
    vel = {k: torch.zeros_like(v) for k, v in params.items() if v.is_floating_point()}
    max_norm, ref_norms, g1 = None, [], None
    for step in range(1, 4):
        _, grads = O.forward_backward(params, cfg, inp)
        grads = {k: grads[k].detach() for k in names if grads.get(k) is not None}
        norm = float(torch.sqrt(sum((x.double() ** 2).sum() for x in grads.values())))
        if max_norm is None:
            max_norm, g1 = 0.25 * norm, grads
        coef = min(1.0, max_norm / (norm + 1e-6))
        assert coef < 1.0
        ref_norms.append(norm)
        with torch.no_grad():
            O.adamw_step(params, {k: (x.double() * coef).float() for k, x in grads.items()}, mom, vel, step)
    model = model.cuda()
    tr = Trainer(model, dropout=False, max_grad_norm=max_norm)
    batch = {k: v.to(DEV) for k, v in b.items()}
    for step in range(3):
        tr.train_step(batch)
        got = float(tr.opt.grad_norm)
        assert abs(got - ref_norms[step]) <= 1e-3 * ref_norms[step], (step, got, ref_norms[step])
    for k, p in model.named_parameters():
        got = p.detach().cpu()
        if k in nograd or k not in g1:
            assert torch.equal(got, sd[k]), k
            continue
        gabs = g1[k].abs()
        solid = gabs > max(1e-5, 2e-3 * float(gabs.max()))
        err = (got - params[k]).abs()
        lim = torch.where(solid, torch.full_like(err, 1e-4), torch.full_like(err, 6.6e-3)) + 1e-4 * params[k].abs()
        assert bool((err <= lim).all()), (k, float(err.max()))


# ------------------------------------------------------------------------------------------------ 6. the recorded step
def _synth_cfg3():
    """BASELINE config 3's width in id mode (id / id, d = 512, h = 16, N = 4, S = 20, one user token), as test_dp_gpu builds it."""
    return dict(S=20, N=4, d=512, h=16, user="id", photo="id", Lt=1, D_in=4, n_users=200, n_items=1000, exposure_prob=[1.0] * 20,
                loss_type_list=["interestBPR"], loss_weight={"interestBPR": 1.0, "mse": 1.0})


@pytest.mark.parametrize("case", ["image", "synth_cfg3"])
def test_recorded_clip_step_equals_eager(case):
    """Trainer(device_state=True, max_grad_norm=m), clipping active: record() then run_recorded() on 3 rotating batches leaves
    parameters, moments and every step's norm bit-identical to the same steps taken by train_step."""
    from segmminterest_amd.synth import make_batch
    from segmminterest_amd.trainer import Trainer, default_args, init_model
    if case == "image":
        B, S, Lt, D, N, h = 32, 40, 10, 64, 2, 4
        margs = default_args(num_layers_enc=N, d_model=D, nhead=h, input_type={"user": "image", "photo": "image"}, exposure_prob=[1.0] * S)
        batches = [{k: v.to(DEV) for k, v in make_batch(B, S, Lt, D, seed=200 + i).items()} for i in range(3)]

        def fresh():
            return init_model(margs, n_users=50, n_items=500, input_dim=D, max_vid_len=S, max_usr_len=Lt).to(DEV)
    else:
        cfg = _synth_cfg3()
        batches = [{k: v.to(DEV) for k, v in make_batch(16, cfg["S"], cfg["Lt"], cfg["D_in"], n_users=cfg["n_users"], n_items=cfg["n_items"],
                                                        seed=300 + i).items()} for i in range(3)]

        def fresh():
            return build_model(cfg).to(DEV)
    max_norm = 1e-4

    def run(graph):
        torch.manual_seed(5)
        model = fresh()
        tr = Trainer(model, device_state=True, max_grad_norm=max_norm)
        if graph:
            tr.record(batches[0], warmup=2)
        else:
            for _ in range(3):
                tr.train_step(batches[0])
        norms = []
        for t in range(3):
            tr.run_recorded(batches[t % 3]) if graph else tr.train_step(batches[t % 3])
            norms.append(tr.opt._clip_out.clone())
        torch.cuda.synchronize()
        return model._store.flat.detach().clone(), tr.opt.m.clone(), torch.stack(norms)

    p_e, m_e, n_e = run(False)
    p_g, m_g, n_g = run(True)
    assert bool((n_e[:, 0] > max_norm).all()) and bool((n_e[:, 1] < 1.0).all()), n_e          # clipping active
    assert torch.equal(n_e, n_g)
    assert torch.equal(p_e, p_g) and torch.equal(m_e, m_g)


# ------------------------------------------------------------------------------------------------ 7. data parallel
def _batch16(cfg, seed=21):
    from segmminterest_amd.synth import make_batch
    return make_batch(16, cfg["S"], cfg["Lt"], cfg["D_in"], n_users=cfg.get("n_users", 5) or 5, n_items=cfg.get("n_items", 5) or 5, seed=seed)


def _run_dp(rank, world, port, name, recorded, max_norm, q):
    """``world`` gloo ranks sharing cuda:0 (world 1: a plain single-process trainer on the whole batch), dropout off, device state
    on.  2 steps (eager, or record(warmup=1): 1 eager + the recorded one), then 2 more (train_step or run_recorded)."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from segmminterest_amd.trainer import DPComm, Trainer, shard_rows
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        cfg, g, _, _ = load_case(name)
        torch.manual_seed(5)
        model = build_model(cfg)
        model.load_state_dict(g["sd"])
        model = model.cuda()
        tr = Trainer(model, comm=DPComm(), overlap=True, dropout=False, device_state=True, max_grad_norm=max_norm)
        assert tr.comm.active == (world > 1)
        s, e = shard_rows(16, world, rank)
        shards = [{k: v[s:e].contiguous().cuda() for k, v in _batch16(cfg, seed).items()} for seed in (21, 22)]
        norms = []
        if recorded:
            tr.record(shards[0], warmup=1)
            norms.append(tr.opt._clip_out.cpu())
        else:
            for _ in range(2):
                tr.train_step(shards[0])
                norms.append(tr.opt._clip_out.cpu())
        p2 = model._store.flat.detach().cpu().clone()
        sd2 = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
        for t in range(2):
            tr.run_recorded(shards[t]) if recorded else tr.train_step(shards[t])
            norms.append(tr.opt._clip_out.cpu())
        torch.cuda.synchronize()
        q.put((rank, [n.numpy() for n in norms], p2.numpy(), sd2, model._store.flat.detach().cpu().numpy(), tr.opt.m.cpu().numpy()))
    finally:
        if world > 1:
            dist.destroy_process_group()


def _spawn_dp(world, name, recorded, max_norm, port):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_run_dp, args=(r, world, port, name, recorded, max_norm, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        r = q.get(timeout=300)
        res[r[0]] = r[1:]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    return res


@pytest.mark.parametrize("name", ["img_d32_N3_alllosses", "id_d32_N2"])
def test_data_parallel_clip(name):
    """Two gloo ranks sharing the GPU, clipping active: every rank reports a bitwise-identical norm (each computes it from its own
    copy of the all-reduced gradient); after 2 steps the parameters equal a single-process run on the whole batch to the tolerance
    of test_two_ranks_equal_single_process; and the recorded data-parallel step is bit-identical to the eager one."""
    import numpy as np
    max_norm = 1e-4
    base = 29500 + os.getpid() % 200 + (7 if name.startswith("id") else 0)
    single = _spawn_dp(1, name, False, max_norm, base)[0]
    eager = _spawn_dp(2, name, False, max_norm, base + 211)
    rec = _spawn_dp(2, name, True, max_norm, base + 223)
    for run in (eager, rec):
        for a, b in zip(run[0][0], run[1][0]):
            assert a.view(np.int32).tolist() == b.view(np.int32).tolist(), (a, b)          # bitwise across ranks
        assert (run[1][1] == run[0][1]).all() and (run[1][3] == run[0][3]).all()          # identical replicas
    for n in eager[0][0]:
        assert n[0] > max_norm and n[1] < 1.0, n          # clipping active
    for a, b in zip(single[0][:2], eager[0][0][:2]):
        assert abs(float(a[0]) - float(b[0])) <= 1e-3 * float(a[0]), (a, b)
    for k in single[2]:
        assert np.allclose(single[2][k], eager[0][2][k], rtol=1e-4, atol=4.5e-3), k
    for r in (0, 1):
        # (the recorded run reports from its second step on: record() takes the first one eagerly)
        assert len(rec[r][0]) == len(eager[r][0]) - 1
        assert all(a.view(np.int32).tolist() == b.view(np.int32).tolist() for a, b in zip(eager[r][0][1:], rec[r][0]))
        assert (eager[r][1] == rec[r][1]).all() and (eager[r][3] == rec[r][3]).all() and (eager[r][4] == rec[r][4]).all()
