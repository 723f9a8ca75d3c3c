"""segmm_store_index on the MI355X: the index of a logit store built where the keys are -- sorted distinct (user, item, time) triples
in signed lexicographic order with the row of each key's LAST occurrence -- against bridge.LogitStore._build_index (numpy) on the same
keys, and DeviceLogitStore.finalize(on_device=True) under its consumers.  Integers only: every comparison is exact."""
import numpy as np
import pytest
import torch

from segmminterest_amd.bridge import DeviceLogitStore, LogitStore

pytestmark = pytest.mark.gpu
DEV = "cuda"
I64 = np.iinfo(np.int64)
# the issue's sizes (one chunk, the first global stride, several strides with a ragged tail) and the edges of the LDS chunk of 2048
SIZES = (0, 1, 2, 3, 2047, 2048, 2049, 8191, 8192, 8193, 16385, 131075)
KINDS = ("dup1", "dup50", "equal", "sorted", "reverse", "negative", "large", "pairs", "int64max")


def _H():
    from segmminterest_amd import hipabi
    hipabi.lib()
    return hipabi


def _lexsorted(k):
    return k[np.lexsort((k[:, 2], k[:, 1], k[:, 0]))]


def _keys(kind, n, seed=0):
    """int64 [n, 3] keys of one content kind"""
    rng = np.random.default_rng(1000 * seed + n)
    rnd = lambda m: rng.integers(I64.min, I64.max, (m, 3), dtype=np.int64, endpoint=True)
    if kind == "dup1":          # about 1 % of the rows repeat another row's key
        k = rnd(n)
        d = rng.random(n) < 0.01
        k[d] = k[rng.integers(0, max(n, 1), int(d.sum()))]
    elif kind == "dup50":          # keys from a pool of n / 2: about half the rows are repeats
        k = rnd(max(n // 2, 1))[rng.integers(0, max(n // 2, 1), n)]
    elif kind == "equal":
        k = np.repeat(rnd(1), n, 0)
    elif kind in ("sorted", "reverse"):
        k = _lexsorted(rnd(max(n // 2, 1))[rng.integers(0, max(n // 2, 1), n)])
        k = k[::-1].copy() if kind == "reverse" else k
    elif kind == "negative":          # small values of both signs in every column: ties in the leading columns decide further right
        k = rng.integers(-40, 40, (n, 3), dtype=np.int64)
    elif kind == "large":          # above 2^32 and 2^41 in each column, time_ms near 1.7e12 (41 bits)
        base = np.array([[2 ** 32, 2 ** 41, 1_700_000_000_000], [2 ** 41, 2 ** 32, 1_700_000_000_000], [2 ** 52, 2 ** 33, 2 ** 41 + 5]], np.int64)
        k = base[rng.integers(0, 3, n)] + rng.integers(0, 30, (n, 3), dtype=np.int64)
    elif kind == "pairs":          # pairs that differ only in the top word, only in the third column, only by sign
        x = 0x12345678
        pool = np.array([[x, 5, 9], [x + (1 << 32), 5, 9], [x + (3 << 32), 5, 9], [5, x, 9], [5, x + (1 << 32), 9], [5, 9, x], [5, 9, x + (1 << 32)],
                         [7, 7, 1], [7, 7, 2], [7, 7, -2], [x, 5, -9], [-x, 5, 9], [x, -5, 9], [-x, -5, -9], [(1 << 63) - 1, 0, 0], [-(1 << 62), 0, 0],
                         [0, 0, 0], [0, 0, -1], [0, -1, 0], [-1, 0, 0]], np.int64)
        k = pool[rng.integers(0, len(pool), n)]
    else:          # "int64max": a real key of (INT64_MAX,) * 3 -- what a sentinel padding would collide with -- beside its neighbours
        pool = np.array([[I64.max] * 3, [I64.max, I64.max, I64.max - 1], [I64.max, I64.max - 1, I64.max], [I64.min] * 3, [I64.min, I64.min, I64.min + 1],
                         [I64.max, I64.min, 0], [0, 0, 0], [-1, -1, -1]], np.int64)
        k = np.concatenate([pool[rng.integers(0, len(pool), n - n // 2)], rnd(n // 2)])[rng.permutation(n)] if n else pool[:0]
        if n:
            k[rng.integers(0, n)] = I64.max          # present at every size
    return np.ascontiguousarray(k.reshape(n, 3))


def _host_index(k):
    h = LogitStore(1)
    h._keys, h._vals = [k], [np.zeros((k.shape[0], 0), np.float32)]
    h._build_index()
    return h._index


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_index_equals_the_host_index(kind, n):
    H = _H()
    k = _keys(kind, n)
    ks, rows = _host_index(k)
    out_keys, out_rows, nu = H.store_index(torch.from_numpy(k).to(DEV))
    m = int(nu.item())
    print("%s n=%d: %d distinct keys (host %d)" % (kind, n, m, len(ks)))
    assert m == len(ks)
    assert np.array_equal(out_keys[:m].cpu().numpy(), ks)
    assert np.array_equal(out_rows[:m].cpu().numpy(), rows.astype(np.int32))
    if kind == "equal" and n:
        assert m == 1 and int(out_rows[0]) == n - 1          # the last occurrence
    if kind == "int64max" and n:
        assert (ks[-1] == I64.max).all()          # the pitfall key is in the index, as its last entry


def test_two_runs_give_identical_output_and_write_nothing_behind_n_unique():
    H = _H()
    n = 16385
    k = torch.from_numpy(_keys("dup50", n, seed=3)).to(DEV)
    runs = []
    for _ in range(2):
        ok = torch.full((n, 3), -77, dtype=torch.int64, device=DEV)
        orow = torch.full((n,), -77, dtype=torch.int32, device=DEV)
        H.store_index(k, out_keys=ok, out_rows=orow, n_unique=(nu := torch.full((1,), -77, dtype=torch.int64, device=DEV)))
        runs.append((ok, orow, nu))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    m = int(runs[0][2].item())
    assert 0 < m < n and bool((runs[0][0][m:] == -77).all()) and bool((runs[0][1][m:] == -77).all())
    # a caller's workspace: too small is refused by name, large enough gives the same index
    need = H.store_index_ws_bytes(n)
    with pytest.raises(RuntimeError, match="workspace of %d bytes" % need):
        H.store_index(k, ws=torch.empty(need - 1, dtype=torch.uint8, device=DEV))
    again = H.store_index(k, ws=torch.empty(need + 64, dtype=torch.uint8, device=DEV))
    assert torch.equal(again[0][:m], runs[0][0][:m]) and torch.equal(again[1][:m], runs[0][1][:m]) and int(again[2].item()) == m


def test_beyond_the_built_limit_is_refused_by_name():
    H = _H()
    with pytest.raises(RuntimeError, match=r"store_index_ws: n = %d keys .*finalize\(\) without on_device" % (H.STORE_INDEX_MAX + 1)):
        H.store_index_ws_bytes(H.STORE_INDEX_MAX + 1)


def _stores(n, S, seed):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 60, (n, 3), dtype=np.int64) + np.array([2 ** 33, 0, 1_700_000_000_000], np.int64)          # many repeats
    host = LogitStore(S)
    host._keys, host._vals = [k], [rng.standard_normal((n, S)).astype(np.float32)]
    return host, k


@pytest.mark.parametrize("with_neg", (False, True))
def test_lookup_and_head_on_a_device_built_index_equal_those_on_the_host_built_one(with_neg):
    _H()
    S, B, I = 40, 64, 4
    host, k = _stores(5000, S, 1)
    nhost, nk = _stores(9000, S, 2)
    rng = np.random.default_rng(5)
    pick = k[rng.integers(0, len(k), B)]
    user, time = pick[:, 0].copy(), pick[:, 2].copy()
    item = np.concatenate([pick[:, 1:2], rng.integers(0, 60, (B, I - 1), dtype=np.int64)], 1)
    user[::7] += 1000          # absent targets: rows of ones
    q = [torch.from_numpy(x).to(DEV) for x in (user, item, time)]
    pred = torch.randn(B, I, S, generator=torch.Generator().manual_seed(1)).to(DEV)
    got = []
    for on_device in (False, True):
        st = DeviceLogitStore.from_store(host, DEV).finalize(on_device=on_device)
        neg = DeviceLogitStore.from_store(nhost, DEV).finalize(on_device=on_device) if with_neg else None
        rowidx, miss = st.lookup(*q, neg=neg, check=False)
        out, miss2 = st.head(pred, *q, neg=neg, check=False)
        got.append((st._index[0], st._index[1], rowidx, miss, out, miss2))
    for a, b in zip(*got):
        assert torch.equal(a, b)
    rowidx = got[1][2]
    assert bool((rowidx == -1).any()) and bool((rowidx >= 0).any()) and bool((rowidx <= -2).any()) == with_neg
    # and the preallocated form builds its index over exactly the rows appended so far
    grown = DeviceLogitStore(S=S, device=DEV, capacity=8000)
    grown.add_batch(k[:, 0], k[:, 1], k[:, 2], host._vals[0])
    assert torch.equal(grown.finalize(on_device=True)._index[0], got[0][0]) and torch.equal(grown._index[1], got[0][1])


def test_an_empty_store_has_an_empty_index_on_the_device():
    _H()
    st = DeviceLogitStore(S=4, device=DEV).finalize(on_device=True)
    assert st._index[0].shape == (0, 3) and st._index[1].shape == (0,)
    st = DeviceLogitStore(S=4, device=DEV, capacity=16).finalize(on_device=True)
    assert st._index[0].shape == (0, 3) and len(st) == 0
