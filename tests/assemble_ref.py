"""segmm_assemble_rows restated in numpy from the words of include/segmm_hip.h (candidate lists, draw rule, padding conventions):
the host reference the kernel is compared with, bit for bit.  uint32 arithmetic throughout; never called by product code."""
import numpy as np

M32 = 0xFFFFFFFF
STREAM_VIDEO, STREAM_USER = 0, 1


def mix32(x):
    """x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16  (mod 2^32), on uint64 arrays holding 32-bit values"""
    x = np.asarray(x, dtype=np.uint64) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return x


def keys(seed, site, r, stream, count):
    """The 32-bit keys of candidates j = 0 .. count-1 of global row r: counter q = (r << 13) | (stream << 12) | j,
    k = seed_lo ^ (site * 0x9E3779B9) ^ ((q >> 32) * 0x85EBCA6B), a = mix32((q & M32) ^ k), key = mix32(a ^ seed_hi ^ 0x68E31DA4)."""
    assert 0 <= seed < 1 << 63 and 0 <= count <= 4096
    seed_lo, seed_hi = seed & M32, (seed >> 32) & 0x7FFFFFFF
    q = (int(r) << 13) | (stream << 12)
    j = np.arange(count, dtype=np.uint64)
    q_lo, q_hi = (np.uint64(q & M32) | j), (q >> 32) & M32          # j < 2^12 sits below the stream bit: no carry
    k = (seed_lo ^ ((site * 0x9E3779B9) & M32) ^ ((q_hi * 0x85EBCA6B) & M32)) & M32
    a = mix32(q_lo ^ np.uint64(k))
    return mix32(a ^ np.uint64(seed_hi ^ 0x68E31DA4))


def draw(cands, cap, seed, site, r, stream):
    """cap slots: the candidates in order when they fit, else the cap smallest (key, j) pairs, each at its rank; -1 = padding."""
    out = np.full((cap,), -1, dtype=np.int64)
    cands = np.asarray(cands, dtype=np.int64)
    if len(cands) <= cap:
        out[:len(cands)] = cands
        return out
    k = keys(seed, site, r, stream, len(cands))
    order = np.lexsort((np.arange(len(cands)), k))          # by key, ties by j
    return cands[order[:cap]]


def candidates(t, r):
    """(video candidates, user candidates) of row r of the compiled table ``t`` (numpy views of its tensors)."""
    item, n, user, _ = (int(x) for x in t["row_info"][r])
    ip, il = t["item_ptr"], t["item_line"]
    n = min(max(n, 0), int(ip[item + 1] - ip[item]))
    video = il[ip[item]:ip[item] + n]
    cand = []
    for h in range(int(t["hist_ptr"][r]), int(t["hist_ptr"][r + 1])):
        it, nf = (int(x) for x in t["hist_pair"][h])
        c = min(max(nf, 0), int(ip[it + 1] - ip[it]))
        lines = il[ip[it]:ip[it] + c]
        cand += [int(x) for x in lines if x >= 0]          # holes skipped
    cand += [int(x) for x in t["own_line"][t["own_ptr"][user]:t["own_ptr"][user + 1]]]
    return [int(x) for x in video], cand


def as_numpy(table):
    return {k: getattr(table, k).cpu().numpy() for k in table.TENSORS}


def assemble(table, row_ids, S, Lt, seed, site, limit=4096):
    """(photo_idx [B, S], user_idx [B, Lt], label [B, S], cols [7, B]) int64 for the rows ``row_ids`` of an InteractionTable."""
    assert S == table.S
    t = as_numpy(table)
    B = len(row_ids)
    photo, user = np.full((B, S), -1, dtype=np.int64), np.full((B, Lt), -1, dtype=np.int64)
    label, cols = np.full((B, S), -2, dtype=np.int64), np.zeros((7, B), dtype=np.int64)
    for b, r in enumerate(int(x) for x in row_ids):
        if not 0 <= r < table.n_rows:
            continue          # all-padding slot
        video, cand = candidates(t, r)
        if len(video) > limit or len(cand) > limit:
            continue
        photo[b] = draw(video, S, seed, site, r, STREAM_VIDEO)
        user[b] = draw(cand, Lt, seed, site, r, STREAM_USER)
        label[b] = t["label"][r].astype(np.int64)
        cols[:, b] = t["row_cols"][r]
    return photo, user, label, cols


# ------------------------------------------------------------------ shared by tests/test_assemble_cpu.py and tests/test_assemble_gpu.py
def fixture():
    """(npz, its five rows, IndexBatchBuilder) of tests/golden/io_dataloader.npz, written by the reference's own _getitem."""
    import json
    import os
    from segmminterest_amd.feature_store import IndexBatchBuilder, KeyIndex
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "io_dataloader.npz"))
    rows = json.loads(str(z["rows"]))
    b = IndexBatchBuilder(KeyIndex([str(k) for k in z["keys"]]), json.loads(str(z["user_input_dict"])), json.loads(str(z["user2id"])),
                          json.loads(str(z["item2id"])))
    return z, rows, b


def synthetic_builder(S, Lt, big=4096):
    """An IndexBatchBuilder over a small made-up line map: item 100 has frames 0..3, item 200 frames 1..5 (a hole at frame 0),
    item 300 frames 0..1, item 400 frames 0..big-1; users: "1" no own frame, "2" three own frames and one unresolvable, "3" six."""
    from segmminterest_amd.feature_store import IndexBatchBuilder, KeyIndex
    keys = ["100-%d" % f for f in range(4)] + ["200-%d" % f for f in range(1, 6)] + ["300-0", "300-1"] + ["400-%d" % f for f in range(big)]
    keys += ["900-%d" % f for f in range(6)]
    uid = {"1": [], "2": ["900_0", "900_1", "901_0", "900_2"], "3": ["900_%d" % f for f in range(6)]}
    items = {str(i): i % 97 + 1 for i in (100, 200, 300, 400)}
    return IndexBatchBuilder(KeyIndex(keys), uid, {u: int(u) + 10 for u in uid}, items, S=S, Lt=Lt)


def synthetic_rows(user_counts):
    """Rows for :func:`synthetic_builder` at S = 3: video frame counts 0, 1, 3 (= S), 4 (= S + 1) in turn; user candidate counts
    ``user_counts`` as watched frames of item 400 (user "1": no own frames), then the special rows (see the comments)."""
    rows, durs = [], (0, 5000, 15000, 20000)
    for k, c in enumerate(user_counts):
        d = durs[k % 4]
        lab = [1] * (d // 5000)
        rows.append(dict(user_id=1, video_id=100, time_ms=1000 + k, duration_ms=d, playing_time=2500 * k, label_1D=lab,
                         history_items=[400] if c else [], history_playing=[5000 * c] if c else []))
    base = dict(video_id=100, time_ms=7, duration_ms=20000, playing_time=12000, label_1D=[1, 1, 0, -1])
    rows.append(dict(base, user_id=2, history_items=[200, 300], history_playing=[30000, 10000]))      # hole at frame 0; 5 + 2 + 3 own = 10
    rows.append(dict(base, user_id=3))                                                                # empty history, 6 own frames > Lt = 5
    rows.append(dict(base, user_id=2, history_items=[200], history_playing=[10000]))                  # frames 0 (hole), 1 + 3 own = 4 <= Lt
    rows.append(dict(base, user_id=1, history_items=[200, 400], history_playing=[5000, 20000], history_length=0))      # history_lengths == 0: no history
    return rows


def shared_candidates_table(n_rows=4096, n_cand=8):
    """n_rows rows that share one video and one user with n_cand own frames (no history): the uniformity statistic's table."""
    from segmminterest_amd.feature_store import IndexBatchBuilder, InteractionTable, KeyIndex
    b = IndexBatchBuilder(KeyIndex(["9-%d" % f for f in range(n_cand)] + ["1-0"]), {"5": ["9_%d" % f for f in range(n_cand)]}, {"5": 1}, {"1": 1},
                          S=1, Lt=3)
    row = dict(user_id=5, video_id=1, time_ms=0, duration_ms=1, playing_time=0, label_1D=[0])
    return InteractionTable.compile(b, [row] * n_rows)


def uniformity(user_idx, n_cand=8, cap=3, sigmas=5.0):
    """user_idx [n, cap] drawn from candidates 0 .. n_cand-1 (their lines): every candidate's selection count ~ Binomial(n, cap / n_cand)
    and every (candidate, position) count ~ Binomial(n, 1 / n_cand).  Returns the worst deviation in standard deviations of each
    and asserts both within ``sigmas``."""
    u = np.asarray(user_idx)
    n = u.shape[0]
    assert u.shape == (n, cap) and u.min() >= 0 and u.max() < n_cand
    assert all(len(set(r)) == cap for r in u.tolist())
    p = cap / n_cand
    sel = np.bincount(u.reshape(-1), minlength=n_cand)
    z_sel = np.abs(sel - n * p) / np.sqrt(n * p * (1 - p))
    pos = np.stack([np.bincount(u[:, c], minlength=n_cand) for c in range(cap)])
    q = 1.0 / n_cand
    z_pos = np.abs(pos - n * q) / np.sqrt(n * q * (1 - q))
    print("uniformity: worst selection deviation %.2f sd, worst (candidate, position) deviation %.2f sd" % (z_sel.max(), z_pos.max()))
    assert z_sel.max() <= sigmas and z_pos.max() <= sigmas, (sel, pos)
    return float(z_sel.max()), float(z_pos.max())
