"""bench.py --dump-outputs on the host: what dump_outputs writes for a model and a step's output dict."""
import importlib.util
import os

import numpy as np
import torch

from helpers import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_outputs_is_bounded_seeded_and_float32(tmp_path, monkeypatch):
    """Every floating output and every parameter lands as <name>.npy in float32; arrays that do not fit their share of the budget
    are a fixed sample of their elements (the same in every run), the rest are whole; the data stays within the budget."""
    from segmminterest_amd.trainer import default_args, init_model
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_BYTES", 256 << 10)          # small budget: the embedding and layer matrices get sampled
    S, d = 10, 64
    margs = default_args(num_layers_enc=2, d_model=d, nhead=4, input_type={"user": "image", "photo": "image"}, exposure_prob=[1.0] * S)
    torch.manual_seed(0)
    model = init_model(margs, n_users=10, n_items=10, input_dim=d, max_vid_len=S, max_usr_len=12)
    out = {"loss": torch.tensor(0.25), "interestBPR": torch.tensor(0.25), "logits": torch.randn(32, S),
           "gt": torch.zeros(32, S, dtype=torch.int64)}
    bench.dump_outputs(str(tmp_path / "a"), out, model)
    bench.dump_outputs(str(tmp_path / "b"), out, model)
    params = dict(model.named_parameters())
    names = sorted(f[:-4] for f in os.listdir(tmp_path / "a"))
    assert names == sorted(["loss", "interestBPR", "logits"] + ["param." + k for k in params])
    data, sampled = 0, 0
    for n in names:
        a, b = np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy"))
        assert a.dtype == np.float32 and np.array_equal(a, b), n
        ref = (params[n[6:]] if n.startswith("param.") else out[n]).detach().numpy()
        if a.shape == ref.shape:
            assert np.array_equal(a, ref), n
        else:
            sampled += 1
            assert a.ndim == 1 and a.size < ref.size and np.isin(a, ref.reshape(-1)).all(), n
        data += a.nbytes
    assert sampled > 0 and data <= bench.DUMP_BYTES
