"""Host reference of the weight average (segmm_ema_update, WeightEMA): a numpy float32 restatement, operation for operation.

    w_t = max(float32(1 - decay), float32(9.0 / (10.0 + t)))        (warm-up; without it w_t = float32(1 - decay))
    s   = s + (p - s) * w                                           each operation rounded to float32

Every operation is a correctly rounded IEEE operation on both sides (the device keeps fp32 denormals), so the kernel is compared
with this bit for bit.  The one thing IEEE leaves open is WHICH NaN an invalid operation returns: ``bits_equal_nan_aware`` compares
NaN lanes as "NaN on both sides" and every other lane as int32."""
import numpy as np

F = np.float32


def weight(decay):
    """The kernel's ``weight`` argument: float32(1 - decay), the subtraction in double."""
    return F(1.0 - float(decay))


def w_at(decay, t, warmup=True):
    w = weight(decay)
    if not warmup:
        return w
    wt = F(9.0 / (10.0 + float(int(t))))
    return wt if wt > w else w


def lerp(s, p, w):
    """One update of float32 arrays (or scalars): three rounded float32 operations."""
    s, p, w = np.asarray(s, dtype=F), np.asarray(p, dtype=F), F(w)
    with np.errstate(all="ignore"):
        d = (p - s).astype(F)
        dw = (d * w).astype(F)
        return (s + dw).astype(F)


def update(s, p, decay, t, warmup=True):
    return lerp(s, p, w_at(decay, t, warmup))


def replay(seed, params, decay, warmup=True, t0=0):
    """The shadow after optimizer steps t0 + 1 ... t0 + len(params): ``seed`` = the parameters before step t0 + 1 (or a loaded
    shadow), ``params[k]`` = the parameters after step t0 + k + 1."""
    s = np.array(seed, dtype=F)
    for k, p in enumerate(params):
        s = update(s, p, decay, t0 + k + 1, warmup)
    return s


def closed_form(s0, p, decay, T, warmup=True):
    """float64: constant p over T steps -> p + (s0 - p) prod_t (1 - w_t), w_t the float32 weights as doubles."""
    prod = 1.0
    for t in range(1, T + 1):
        prod *= 1.0 - float(w_at(decay, t, warmup))
    return float(p) + (float(s0) - float(p)) * prod


def bits_equal_nan_aware(a, b):
    a, b = np.asarray(a, dtype=F).reshape(-1), np.asarray(b, dtype=F).reshape(-1)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(np.int32)[~na] == b.view(np.int32)[~na]).all())


def special_values(n, seed):
    """(s, p) float32 arrays of n elements: normal draws with +-0, denormals, +-inf and NaN planted in both, at lanes that meet every
    pairing at least once when n allows it."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal(n).astype(F)
    p = (s + F(0.01) * rng.standard_normal(n).astype(F)).astype(F)
    spec = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -3e-39, np.inf, -np.inf, np.nan, 3.4e38, -3.4e38, 1.17549435e-38], dtype=F)
    k = len(spec)
    for j in range(min(n, k * k)):          # lane j: s gets spec[j % k], p gets spec[j // k]
        idx = (j * 7) % n if n > k * k * 7 else j
        s[idx] = spec[j % k]
        p[idx] = spec[(j // k) % k]
    return s, p
