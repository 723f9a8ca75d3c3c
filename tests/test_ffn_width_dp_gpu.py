"""The data-parallel trainer at feed-forward widths that differ from d_model: test_dp_gpu.test_two_ranks_equal_single_process on
tests/golden/ffn/ff_img_d32_N3 (d = 32, N = 3, ff = [64, 96, 32]).  The rank body is test_dp_gpu._run itself; only the fixture
loader and the model builder are replaced by the ones that know ``ff_dim_lvls``.  Two gloo ranks share the one GPU; after 2 steps
their parameters must equal a single-process run on the whole batch: the buckets of the flat gradient buffer, cut from parameter
sizes, hold [ff, d], [d, ff] and [ff] tensors here."""
import os

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
NAME = "ff_img_d32_N3"


def _run(rank, world, port, q):
    import test_dp_gpu as T
    from ffn_cases import build_ff_model, load_ff_case

    def case(name):
        cfg, g, _, _ = load_ff_case(name)
        return cfg, g["sd"]
    T._case, T.build_model = case, build_ff_model
    T._run(rank, world, port, NAME, q)


def test_two_ranks_equal_single_process_at_ff_not_d():
    ctx = mp.get_context("spawn")
    results = {}
    for world in (1, 2):
        q = ctx.Queue()
        port = 29600 + (os.getpid() + world + 150) % 300
        procs = [ctx.Process(target=_run, args=(r, world, port, q)) for r in range(world)]
        for p in procs:
            p.start()
        res = q.get(timeout=240)
        for p in procs:
            p.join(60)
            assert p.exitcode == 0
        results[world] = res
    (l1, g1, sd1, vm1), (l2, g2, sd2, vm2) = results[1], results[2]
    assert tuple(sd1["backbone1.encoder.layers.1.ff_vid.layers.0.weight"].shape) == (96, 32)
    for k in vm1:
        if k == "valid_loss":
            assert abs(vm1[k] - vm2[k]) <= 3e-3 * max(1.0, abs(vm1[k])), (k, vm1[k], vm2[k])
        else:
            assert abs(vm1[k] - vm2[k]) <= 0.07, (k, vm1[k], vm2[k])
    g1, g2 = torch.from_numpy(g1), torch.from_numpy(g2)
    assert float((g1 - g2).abs().max()) <= 1e-4 * float(g1.abs().max()), "summed shard gradients != whole-batch gradients"
    assert abs(l1[0] - l2[0]) <= 1e-5 * max(1.0, abs(l1[0])), (l1, l2)
    assert abs(l1[1] - l2[1]) <= 3e-4 * max(1.0, abs(l1[1])), (l1, l2)
    for k in sd1:
        assert torch.allclose(torch.from_numpy(sd1[k]), torch.from_numpy(sd2[k]), rtol=1e-4, atol=4.5e-3), k
