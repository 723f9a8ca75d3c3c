"""CPU side of the recorded validation pass: the ABI mirror of segmm_valid_rows, the host finalisation of the pass's device tables,
the refusal under data parallelism."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def test_abi_mirror_lists_the_new_export_at_version_30():
    from segmminterest_amd import _abi
    from segmminterest_amd import hipabi as H
    assert _abi.ABI_VERSION == 30 and H.ABI_VERSION == 30
    assert H.PARAMS["segmm_valid_rows"] == ("logits", "ld", "exposure", "gt", "B", "S", "masked", "seq_valid", "permute", "seed", "site", "row0",
                                            "ranks", "interests", "perm_out", "stream")
    codes = [c for _, c in _abi.PROTOTYPES["segmm_valid_rows"]]
    assert codes == ["p", "i", "p", "p", "i", "i", "i", "i", "i", "u64", "u32", "i64", "p", "p", "p", "p"]
    assert _abi.CONSTANTS["SEGMM_PHASE_KINDS"] == 8
    inc = open(os.path.join(os.path.dirname(H.__file__), "csrc", "cmd_dispatch.inc")).read()
    assert '"segmm_valid_rows",' in inc and "return segmm_valid_rows(" in inc          # a recordable command
    assert callable(H.valid_rows) and callable(H.cmd_set_arg)


def test_cmd_set_arg_writes_the_slot_cmd_arg_reads():
    from segmminterest_amd import hipabi as H
    c = H.Cmd()
    H.cmd_set_arg(c, "segmm_valid_rows", "row0", 4711)
    H.cmd_set_arg(c, "segmm_valid_rows", "seed", (1 << 63) - 5)
    H.cmd_set_arg(c, "segmm_valid_rows", "ranks", 0x7F0000001000)
    assert H.cmd_arg(c, "segmm_valid_rows", "row0") == 4711 and H.cmd_arg(c, "segmm_valid_rows", "seed") == (1 << 63) - 5
    assert H.cmd_arg(c, "segmm_valid_rows", "ranks") == 0x7F0000001000 and H.cmd_arg(c, "segmm_valid_rows", "ld") == 0


def test_host_finalisation_is_the_arithmetic_of_valid_model():
    """ValidationAccumulator.finalize on synthetic tables == today's valid_model loop on the same per-batch values: per batch
    _evaluations(r[r > 0]) and float() of the float32 loss scalars, then sum / len over the batches."""
    from segmminterest_amd.my_evaluation import ValidationAccumulator, _evaluations
    rng = np.random.RandomState(3)
    rows = [48, 48, 17, 5]
    offsets = [0] + list(np.cumsum(rows))
    ranks = rng.randint(0, 41, size=offsets[-1]).astype(np.int32)          # 0 = invalid row
    ranks[offsets[3]:] = 0                                                 # a batch without one valid row
    scalars = rng.rand(len(rows), 13).astype(np.float32)
    metrics = ("valid_loss", "HR@1", "HR@3", "HR@5", "HR@10", "NDCG@1", "NDCG@3", "NDCG@5", "NDCG@10", "interestBPR", "mse", "loss", "nothing")
    slots = {"interestBPR": 0, "mse": 7, "mse2": 8, "loss": 12}
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got = ValidationAccumulator.finalize(ranks, scalars, offsets, metrics, slots)
            acc = {k: [] for k in metrics}
            for i in range(len(rows)):
                out = {"loss": torch.tensor(scalars[i, 12]), "interestBPR": torch.tensor(scalars[i, 0]), "mse": torch.tensor(scalars[i, 7]),
                       "mse2": torch.tensor(scalars[i, 8]), "gt": None, "logits": None}
                r = ranks[offsets[i]:offsets[i + 1]].astype(np.int64)
                ev = _evaluations(r[r > 0], verbose=False)
                for k in acc:
                    if k == "valid_loss":
                        acc[k].append(float(out["loss"].detach().clone()))
                    elif k in out and k not in ("gt", "logits"):
                        acc[k].append(float(out[k]))
                    elif k in ev:
                        acc[k].append(float(ev[k]))
            want = {k: (sum(v) / len(v) if v else float("nan")) for k, v in acc.items()}
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k] or (np.isnan(got[k]) and np.isnan(want[k])), k
    assert np.isnan(got["nothing"]) and np.isnan(got["HR@1"]) and got["valid_loss"] == sum(float(x) for x in scalars[:, 12]) / 4


def test_accumulator_lays_the_batches_out_at_disjoint_offsets():
    from segmminterest_amd.my_evaluation import ValidationAccumulator
    acc = ValidationAccumulator([48, 48, 17], torch.device("cpu"), ("valid_loss",))
    assert acc.offsets == [0, 48, 96, 113] and acc.ranks.shape == (113,) and acc.ranks.dtype == torch.int32
    assert acc.scalars.shape == (3, 13) and acc.scalars.dtype == torch.float32
    assert acc.rank_slice(2).data_ptr() == acc.ranks.data_ptr() + 4 * 96 and acc.rank_slice(2).numel() == 17


def test_recorded_validation_is_refused_under_data_parallelism():
    from segmminterest_amd.trainer import Trainer, default_args, init_model, fit
    margs = default_args(num_layers_enc=1, d_model=16, nhead=2, input_type={"user": "image", "photo": "image"}, exposure_prob=[1.0] * 4)
    model = init_model(margs, n_users=1, n_items=1, input_dim=16, max_vid_len=4, max_usr_len=2)
    tr = Trainer(model)
    tr.comm.active = True          # (a stub: what DPComm reports with more than one rank)
    with pytest.raises(RuntimeError, match=r"valid_model\(recorded=True\) is not supported under data parallelism"):
        tr.valid_model([], recorded=True)
    with pytest.raises(RuntimeError, match=r"recorded=True\) is not supported under data parallelism"):
        fit(tr, [], [], epochs=0, recorded_valid=True)


def test_pass_seeds_differ_by_pass_and_follow_the_model_seed():
    from segmminterest_amd.trainer import Trainer
    t = Trainer.__new__(Trainer)
    t._seed0 = 12345
    a, b = t._valid_seed(0), t._valid_seed(1)
    assert a != b and 0 <= a < (1 << 63) and 0 <= b < (1 << 63) and t._valid_seed(0) == a
    t._seed0 = 12346
    assert t._valid_seed(0) != a
