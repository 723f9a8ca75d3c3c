"""segmm_store_append on the MI355X: the store's writer as one launch -- bit copies of the batch's key columns and logits into rows
[row0, row0 + B) of preallocated tables, nothing outside them -- and the preallocated form of DeviceLogitStore that appends with it
and grows geometrically.  Everything is integers and bit copies: every comparison is exact."""
import pytest
import torch

from segmminterest_amd.bridge import DeviceLogitStore

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 7          # rows of the tables behind `capacity` that no call may touch


def _H():
    from segmminterest_amd import hipabi
    hipabi.lib()
    return hipabi


def _case(B, S, ld, seed, misalign):
    """key columns int64 [B] (any int64), logits float32 rows ld floats apart as random BIT patterns (NaNs and denormals included);
    ``misalign``: the logits start 4 bytes behind a 16-byte boundary."""
    gen = torch.Generator().manual_seed(seed)
    cols = [torch.randint(-2 ** 62, 2 ** 62, (B,), generator=gen, dtype=torch.int64).to(DEV) for _ in range(3)]
    flat = torch.randint(-2 ** 31, 2 ** 31 - 1, (B * ld + 8,), generator=gen, dtype=torch.int64).to(torch.int32).view(torch.float32).to(DEV)
    off = 1 if misalign else 0
    assert flat.data_ptr() % 16 == 0
    logits = flat[off:off + B * ld].view(B, ld)[:, :S]
    assert (logits.data_ptr() % 16 != 0) == bool(misalign)
    return cols, logits


@pytest.mark.parametrize("misalign", (False, True))
@pytest.mark.parametrize("row0", (0, 3))
@pytest.mark.parametrize("B,S,ld", [(1, 1, 1), (5, 40, 40), (130, 40, 48), (7, 41, 64), (3, 256, 256)])
def test_append_writes_its_rows_bit_for_bit_and_nothing_else(B, S, ld, row0, misalign):
    H = _H()
    cap = row0 + B + 2
    gen = torch.Generator().manual_seed(1)
    keys = torch.randint(-2 ** 62, 2 ** 62, (cap + GUARD, 3), generator=gen, dtype=torch.int64).to(DEV)          # the recorded pattern
    vals = torch.randint(-2 ** 31, 2 ** 31 - 1, (cap + GUARD, S), generator=gen, dtype=torch.int64).to(torch.int32).to(DEV)
    k0, v0 = keys.clone(), vals.clone()
    cols, logits = _case(B, S, ld, 10 * B + S, misalign)
    H.store_append(cols[0], cols[1], cols[2], logits, row0, keys[:cap], vals[:cap].view(torch.float32))
    want_k, want_v = k0.clone(), v0.clone()
    want_k[row0:row0 + B] = torch.stack(cols, 1)
    want_v[row0:row0 + B] = logits.contiguous().view(torch.int32)
    assert torch.equal(keys, want_k)
    assert torch.equal(vals, want_v)          # int32 views: NaN payloads compare as bits


def test_zero_rows_launch_nothing():
    H = _H()
    keys = torch.full((4, 3), 7, dtype=torch.int64, device=DEV)
    vals = torch.full((4, 5), 7.0, device=DEV)
    e = torch.zeros((0,), dtype=torch.int64, device=DEV)
    H.store_append(e, e, e, torch.zeros((0, 5), device=DEV), 4, keys, vals)
    assert bool((keys == 7).all()) and bool((vals == 7).all())


def _batches(S):
    out = []
    for i, B in enumerate((3, 3, 130)):
        cols, logits = _case(B, S, S + 8 * (i == 2), 50 + i, False)
        out.append((cols[0], cols[1], cols[2], logits))
    return out


@pytest.mark.parametrize("S", (40, 41))
def test_a_store_of_capacity_4_grows_and_equals_the_block_list_store(S):
    _H()
    grown, blocks = DeviceLogitStore(S=S, device=DEV, capacity=4), DeviceLogitStore(S=S, device=DEV)
    assert grown.capacity == 4 and blocks.capacity is None and len(grown) == 0 and grown._cat()[0].shape == (0, 3)
    caps = []
    for n, b in enumerate(_batches(S)):
        grown.append(*b)
        blocks.add_batch(*b)
        caps.append(grown.capacity)
        assert len(grown) == len(blocks) == (3, 6, 136)[n]
        # every reader sees exactly the rows appended so far
        (gk, gv), (bk, bv) = grown._cat(), blocks._cat()
        assert torch.equal(gk, bk) and torch.equal(gv.view(torch.int32), bv.view(torch.int32))
    assert caps == [4, 8, 136]          # geometric, or the batch when that is more
    hg, hb = grown.to_store()._cat(), blocks.to_store()._cat()
    assert (hg[0] == hb[0]).all() and (hg[1].view("int32") == hb[1].view("int32")).all()
    # add_batch keeps working on the preallocated form (host tensors, converted as it always did) ...
    extra = (torch.tensor([1, 2]), torch.tensor([3, 4]), torch.tensor([5, 6]), torch.arange(2 * S, dtype=torch.float32).reshape(2, S))
    grown.add_batch(*extra)
    blocks.add_batch(*extra)
    assert len(grown) == 138 and torch.equal(grown._cat()[0], blocks._cat()[0]) and torch.equal(grown._cat()[1][-2:], blocks._cat()[1][-2:])
    # ... reserve turns a block-list store into a preallocated one with the same rows, and the readers agree
    blocks.reserve(200)
    assert blocks.capacity == 200 and len(blocks) == 138 and torch.equal(blocks._cat()[0], grown._cat()[0])
    u, it, t = extra[0].to(DEV), extra[1].to(DEV).reshape(2, 1), extra[2].to(DEV)
    w = grown.finalize().weights(u, it, t)
    assert torch.equal(w, blocks.weights(u, it, t)) and torch.equal(w[:, 0].cpu(), extra[3])


def test_refusals_name_what_is_wrong():
    H = _H()
    L = H.lib()
    cols, logits = _case(5, 40, 40, 3, False)
    keys = torch.zeros((10, 3), dtype=torch.int64, device=DEV)
    vals = torch.zeros((10, 40), device=DEV)
    with pytest.raises(RuntimeError, match=r"store_append: rows \[6, 11\) overflow the capacity of 10 rows"):
        H.store_append(cols[0], cols[1], cols[2], logits, 6, keys, vals)
    with pytest.raises(RuntimeError, match=r"store_append: negative row0 \(-1\)"):
        H.store_append(cols[0], cols[1], cols[2], logits, -1, keys, vals)
    rc = L.segmm_store_append(cols[0].data_ptr(), cols[1].data_ptr(), None, logits.data_ptr(), 40, 5, 40, 0, 10, keys.data_ptr(), vals.data_ptr(), None)
    assert rc != 0 and "store_append: null pointer" in L.segmm_last_error().decode()
    torch.cuda.synchronize()
    assert not bool(keys.any()) and not bool(vals.any())          # a refused call wrote nothing
    with pytest.raises(RuntimeError, match="device tensors"):
        H.store_append(cols[0].cpu(), cols[1], cols[2], logits, 0, keys, vals)
    with pytest.raises(RuntimeError, match="user must be contiguous int64"):
        H.store_append(cols[0].int(), cols[1], cols[2], logits, 0, keys, vals)
    st = DeviceLogitStore(S=41, device=DEV, capacity=8)
    with pytest.raises(ValueError, match="store expects 41"):
        st.append(cols[0], cols[1], cols[2], logits)
