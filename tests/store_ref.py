"""segmm_store_lookup / segmm_store_head / segmm_store_head_bwd restated in numpy from the words of include/segmm_hip.h: the row
indices and the miss slots as integers, the head and its backward in float64.  Shared by test_store_cpu.py and test_store_gpu.py."""
import numpy as np

MISS_NONE = np.iinfo(np.int64).max


def build_index(keys):
    """keys int64 [m, 3] in insertion order -> (sorted unique keys [n, 3], rows int32 [n]); the last occurrence of a key wins."""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    best = {}
    for r, k in enumerate(keys.tolist()):
        best[tuple(k)] = r
    ks = sorted(best)          # python tuples of ints: lexicographic and signed
    return np.array(ks, np.int64).reshape(-1, 3), np.array([best[k] for k in ks], np.int32)


def _find(index, key):
    ks, rows = index
    lo, hi = 0, len(ks)
    while lo < hi:
        mid = (lo + hi) // 2
        if tuple(ks[mid].tolist()) < key:
            lo = mid + 1
        else:
            hi = mid
    return int(rows[lo]) if lo < len(ks) and tuple(ks[lo].tolist()) == key else -1


def _mapped(mp, x):
    """(ok, mapped id) of the dense id map ``mp`` (None = identity)"""
    if mp is None:
        return True, int(x)
    if x < 0 or x >= len(mp) or mp[x] < 0:
        return False, int(x)
    return True, int(mp[x])


def lookup(user, item, time, index, neg_index=None, user_map=None, item_map=None):
    """-> rowidx int32 [B, I], miss int64 [2]"""
    user, item, time = np.asarray(user, np.int64).reshape(-1), np.asarray(item, np.int64), np.asarray(time, np.int64).reshape(-1)
    B, I = item.shape
    rowidx = np.empty((B, I), np.int32)
    miss = [MISS_NONE, MISS_NONE]
    for b in range(B):
        uok, u = _mapped(user_map, int(user[b]))
        iok, i0 = _mapped(item_map, int(item[b, 0]))
        t = -1
        if uok and iok:
            t = _find(index, (u, i0, int(time[b])))
        else:
            miss[1] = min(miss[1], b * I)
        own = neg_index is not None and I > 2 and t >= 0
        rowidx[b, 0] = t
        for j in range(1, I):
            v = t
            if item_map is not None or own:
                ok, it = _mapped(item_map, int(item[b, j]))
                if not ok:
                    miss[1] = min(miss[1], b * I + j)
                    v = -1
                elif own:
                    r = _find(neg_index, (u, it, int(time[b])))
                    if r < 0:
                        miss[0] = min(miss[0], b * I + j)
                    v = -1 if r < 0 else -2 - r
            rowidx[b, j] = v
    return rowidx, np.array(miss, np.int64)


def weights(rowidx, vals, neg_vals=None, S=None):
    """w(b, i) float32 [..., S]: -1 ones, r >= 0 vals[r], r <= -2 neg_vals[-2 - r]; NaN for an index outside its matrix"""
    rowidx = np.asarray(rowidx)
    S = S if S is not None else vals.shape[1]
    out = np.ones(rowidx.shape + (S,), np.float32)
    for pos in np.ndindex(*rowidx.shape):
        r = int(rowidx[pos])
        if r >= 0:
            out[pos] = vals[r] if vals is not None and r < len(vals) else np.nan
        elif r <= -2:
            out[pos] = neg_vals[-2 - r] if neg_vals is not None and -2 - r < len(neg_vals) else np.nan
    return out


def _mask(shape, S, duration):
    if duration is None:
        return np.ones(tuple(shape) + (S,), np.float64)
    return (np.arange(S) < np.asarray(duration, np.int64)[..., None]).astype(np.float64)


def head(pred, rowidx, vals, neg_vals=None, duration=None):
    """-> (out float64 [...], bound float64 [...]): the sum in float64 and the issue's per-output bound for an fp32 kernel,
    (S + 2) * 2^-24 * sum_s |pred * w * mask| (one rounding per product, at most S for the sum)"""
    pred = np.asarray(pred, np.float64)
    S = pred.shape[-1]
    terms = pred * weights(rowidx, vals, neg_vals, S).astype(np.float64) * _mask(pred.shape[:-1], S, duration)
    return terms.sum(-1), (S + 2) * 2.0 ** -24 * np.abs(terms).sum(-1)


def head_bwd(g, S, rowidx=None, vals=None, neg_vals=None, weight=None, duration=None):
    """d pred float64 [..., S] = g * w * mask; w from rowidx, from ``weight``, or ones"""
    g = np.asarray(g, np.float64)
    w = weights(rowidx, vals, neg_vals, S) if rowidx is not None else weight if weight is not None else np.ones(g.shape + (S,))
    return g[..., None] * np.asarray(w, np.float64) * _mask(g.shape, S, duration)


# ------------------------------------------------------------------ inputs both test files use
def random_case(seed, I, with_neg, S=8, B=7, drop_neg=False):
    """A seeded store with duplicated keys over three batches (times near 10^12), queries of which some targets are absent, and --
    ``with_neg`` -- a negatives store that holds every queried (user, item j, time) (one of them left out with ``drop_neg``).
    -> dict(batches, neg_batches or None, user [B], item [B, I], time [B]); batches = [(user, photo, time, logits float32 [n, S])]"""
    g = np.random.RandomState(seed)

    def batch(n):
        return (g.randint(1, 7, n).astype(np.int64), g.randint(1, 9, n).astype(np.int64), (10 ** 12 + g.randint(0, 3, n)).astype(np.int64),
                g.randn(n, S).astype(np.float32))
    batches = [batch(12) for _ in range(3)]
    batches[2][0][:3], batches[2][1][:3], batches[2][2][:3] = batches[0][0][:3], batches[0][1][:3], batches[0][2][:3]          # duplicates: the later logits win
    ku, kp, kt = (np.concatenate([b[c] for b in batches]) for c in range(3))
    pick = g.randint(0, len(ku), B)
    user, time = ku[pick].copy(), kt[pick].copy()
    item = g.randint(1, 9, (B, I)).astype(np.int64)
    item[:, 0] = kp[pick]
    user[1] = 99                     # absent targets: an unknown user, a time that differs in the last word
    time[B - 1] += 7
    neg_batches = None
    if with_neg:
        q = [(user[b], item[b, j], time[b]) for b in range(B) for j in range(1, I)]
        q = q + q[:2]                # duplicated negatives keys too
        if drop_neg:                 # row 0's target is present: its item 2 goes missing from the negatives
            q = [x for x in q if x != (user[0], item[0, 2], time[0])]
        cols = [np.array([x[c] for x in q], np.int64).reshape(-1) for c in range(3)]
        neg_batches = [(cols[0], cols[1], cols[2], g.randn(len(q), S).astype(np.float32))] if q else []          # I == 1: an empty negatives store
    return dict(batches=batches, neg_batches=neg_batches, user=user, item=item, time=time)


RANDOM_CASES = [(11 + 5 * I + int(n), I, n, d) for I in (1, 2, 3) for n in (False, True) for d in (False,)] + [(40, 3, True, True)]


def dense_map(d):
    """the reference's str-keyed id dict as a dense int64 map (-1 = no entry)"""
    m = np.full((max(int(k) for k in d) + 1,), -1, np.int64)
    for k, v in d.items():
        m[int(k)] = int(v)
    return m
