"""The gloo world-2 check of test_dp_cpu.py on a model whose feed-forward widths differ from d_model: per-shard losses and
gradients normalised by the GLOBAL label statistics, reduced in two asynchronous buckets, sum to the single-process loss and
gradient.  The rank body is test_dp_cpu._rank_checks itself, unchanged; only the fixture it loads is replaced by
tests/golden/ffn/ff_img_d32_N3 (d = 32, N = 3, ff = [64, 96, 32]: layer 0 full at ff = 64, layer 1 video-side at ff = 96), so the
flat gradient the buckets cut holds [ff, d], [d, ff] and [ff] tensors.  What runs here is the collectives and the oracle; the
trainer's own bucket layout at ff != d is checked on the GPU (test_ffn_width_gpu.py)."""
import os

import torch.multiprocessing as mp


def _worker(rank, world, port, q):
    import test_dp_cpu as T
    from ffn_cases import load_ff_case
    T.load_case = lambda name: load_ff_case("ff_img_d32_N3")
    T._worker(rank, world, port, q)


def test_dp_world2_gloo_matches_single_process_at_ff_not_d():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() + 517) % 1000
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    loss, ref_loss, gerr, gmax = q.get(timeout=5)
    assert abs(loss - ref_loss) < 1e-4 * max(1.0, abs(ref_loss))
    assert gerr < 1e-4 * gmax
