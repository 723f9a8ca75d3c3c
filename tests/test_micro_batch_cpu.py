"""Micro-batched steps (Trainer(micro_batch=m)), the parts that need no GPU: the new export of the C ABI, the argument check and
the row slicing."""
import ctypes
import math

import pytest
import torch

from helpers import ROOT  # noqa: F401  (puts the repository on sys.path)


def test_library_exports_vec_add_and_dispatches_it():
    from segmminterest_amd import _abi, hipabi as H
    assert H.ABI_VERSION == 30 and _abi.ABI_VERSION == 30          # an additive export: the version stays
    assert [p for p, _ in _abi.PROTOTYPES["segmm_vec_add"]] == ["out", "a", "b", "n", "stream"]
    assert [c for _, c in _abi.PROTOTYPES["segmm_vec_add"]] == ["p", "p", "p", "i64", "p"]
    assert list(_abi.PROTOTYPES)[-1] == "segmm_vec_add"          # placed after the existing exports
    L = ctypes.CDLL(H.LIB_PATH)
    assert hasattr(L, "segmm_vec_add")
    L.segmm_cmd_op_name.restype = ctypes.c_char_p
    names = [L.segmm_cmd_op_name(i).decode() for i in range(L.segmm_cmd_op_count())]
    assert "segmm_vec_add" in names and names == sorted(names)          # a recordable command


@pytest.mark.parametrize("bad", [0, -4, 2.0, "8", True])
def test_trainer_refuses_bad_micro_batch(bad):
    from segmminterest_amd.trainer import Trainer
    with pytest.raises(ValueError, match="micro_batch"):
        Trainer(None, micro_batch=bad)


@pytest.mark.parametrize("B", [1, 4, 10, 16])
def test_micro_slices_cover_every_row_once(B):
    from segmminterest_amd.synth import make_batch
    from segmminterest_amd.trainer import batch_rows, micro_slices
    m = 4
    batch = make_batch(B, 6, 5, 8, n_users=9, n_items=9, seed=3)
    batch["note"] = "passed along"
    assert batch_rows(batch) == B
    parts = micro_slices(batch, m)
    assert len(parts) == math.ceil(B / m)
    assert [batch_rows(p) for p in parts] == [min(m, B - r0) for r0 in range(0, B, m)]
    for k, v in batch.items():
        if not torch.is_tensor(v):
            assert all(p[k] is v for p in parts)
            continue
        r0 = 0
        for p in parts:
            s = p[k]
            assert s.is_contiguous() and s.data_ptr() == v.data_ptr() + r0 * v.stride(0) * v.element_size()          # a view, in row order
            assert torch.equal(s, v[r0:r0 + s.shape[0]])
            r0 += s.shape[0]
        assert r0 == B
