"""What the AdamW / EMA entry points of the C ABI refuse, and that a refusal touches nothing.

Each of the 18 ``segmm_adamw*`` / ``segmm_ema_update*`` functions is called directly (ctypes, not the hipabi wrappers, whose own
pre-checks would answer first) with arguments that are valid but for ONE bad value.  The call returns -1, ``segmm_last_error`` starts
with the entry point's name and holds the reason's key words, and every buffer handed in holds the bits it held before.

Buffers: a table of 8 rows x width 8 (64 floats per buffer), a ring of cap = 4, 3 ids.  Nothing launches, so the sizes only have to
make the pointers real; each buffer has room behind it for the misaligned (+ 4 bytes) and overlapping (+ 16 bytes) pointers."""
import math

import pytest
import torch

from segmminterest_amd._abi import PROTOTYPES

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS, WIDTH, CAP, NIDS = 8, 8, 4, 3
N = ROWS * WIDTH
ROOM = N + 64          # floats per buffer: the table plus slack behind it

FLAT = ("segmm_adamw", "segmm_adamw_scaled", "segmm_adamw_guarded")
GROUPS = ("segmm_adamw_groups", "segmm_adamw_groups_guarded")
TABLE = ("segmm_adamw_table", "segmm_adamw_table_scaled", "segmm_adamw_table_lrs", "segmm_adamw_table_lrs_guarded")
PUSH = ("segmm_adamw_hist_push", "segmm_adamw_hist_push_ema")
CATCHUP = ("segmm_adamw_table_catchup", "segmm_adamw_table_catchup_ema")
LAZY_ROWS = ("segmm_adamw_table_lazy_rows", "segmm_adamw_table_lazy_rows_ema")
STAMP = ("segmm_adamw_table_stamp",)
EMA = ("segmm_ema_update", "segmm_ema_update_guarded")
ALL = FLAT + GROUPS + TABLE + PUSH + CATCHUP + LAZY_ROWS + STAMP + EMA
GUARDED = tuple(n for n in ALL if n.endswith("_guarded"))
SCALED = ("segmm_adamw_scaled", "segmm_adamw_table_scaled")          # the forms that insist on a coef


PARAMS = {n: tuple(p for p, _ in PROTOTYPES[n]) for n in ALL}          # entry point -> its parameter names, in order


def _H():
    from segmminterest_amd import hipabi as H
    H.lib()
    return H


class Bufs:
    """Every buffer an entry point can take, filled with values of its own, and a copy of their bits."""

    def __init__(self):
        gen = torch.Generator().manual_seed(20)
        self.f = {k: torch.randn(ROOM, generator=gen).to(DEV) for k in ("p", "g", "m", "v", "shadow")}
        self.f["hist"] = torch.rand(CAP * 4 + 16, generator=gen).to(DEV)
        self.f["coef"] = torch.full((4,), 0.5, device=DEV)
        self.f["seg_lr_scale"] = torch.ones(4, device=DEV)
        self.f["seg_weight_decay"] = torch.full((4,), 0.01, device=DEV)
        self.i = {"ids": torch.tensor([5, 0, 5], dtype=torch.int64, device=DEV), "seg_end": torch.tensor([N], dtype=torch.int64, device=DEV),
                  "stamps": torch.arange(ROWS, dtype=torch.int32, device=DEV), "flags": torch.zeros(ROWS, dtype=torch.int32, device=DEV)}
        self.all = {**self.f, **self.i}
        torch.cuda.synchronize()
        self.before = {k: t.clone() for k, t in self.all.items()}

    def ptr(self, name):
        return self.all[name].data_ptr()

    def unchanged(self):
        torch.cuda.synchronize()
        return [k for k, t in self.all.items() if not torch.equal(t.view(torch.uint8), self.before[k].view(torch.uint8))]


@pytest.fixture(scope="module")
def bufs():
    _H()
    return Bufs()


def _valid(name, b):
    """Arguments the entry point accepts (by parameter name), every pointer real."""
    a = {"n": N, "start": 0, "n_rows": ROWS, "width": WIDTH, "n_ids": NIDS, "n_seg": 1, "cap": CAP, "lr": 1e-3, "lr_scale": 1.0,
         "beta1": 0.9, "beta2": 0.999, "eps": 1e-8, "weight_decay": 0.01, "step": -1 if name in GUARDED else 1, "phase": 1,
         "target": 1, "relative": 0, "weight": 0.1, "warmup": 0, "ema_weight": 0.1, "ema_warmup": 0, "stream": None,
         "seg_frozen": None, "coef": b.ptr("coef") if name in SCALED else None}
    for k in ("p", "g", "m", "v", "shadow", "hist", "ids", "stamps", "flags", "seg_end", "seg_lr_scale", "seg_weight_decay"):
        a[k] = b.ptr(k)
    return a


def _refused(name, b, words, **bad):
    """Calls ``name`` with its valid arguments but for ``bad``; the refusal names the entry point and holds ``words``; no buffer moved."""
    L = _H()._lib_real()
    args = _valid(name, b)
    for k, val in bad.items():
        assert k in PARAMS[name], (name, k)
        args[k] = val(b) if callable(val) else val
    rc = getattr(L, name)(*[args[k] for k in PARAMS[name]])
    msg = L.segmm_last_error().decode()
    assert rc == -1, (name, bad, rc, msg)
    assert msg.startswith(name[len("segmm_"):] + ":"), (name, bad, msg)
    for w in words:
        assert w in msg, (name, bad, w, msg)
    assert b.unchanged() == [], (name, bad)


def _off(buf, nbytes):
    return lambda b: b.ptr(buf) + nbytes


BY_STEP = tuple(n for n in ALL if n not in GUARDED and n not in CATCHUP + STAMP)          # step >= 1 by value, or -1
WITH_LR = tuple(n for n in BY_STEP if n not in EMA)
LR_SCALE = ("segmm_adamw_table_lrs", "segmm_adamw_table_lrs_guarded") + CATCHUP + LAZY_ROWS
RING = CATCHUP + LAZY_ROWS


@pytest.mark.parametrize("name", BY_STEP)
def test_step_zero(bufs, name):
    _refused(name, bufs, ("step=0", ">= 1, or -1"), step=0)


@pytest.mark.parametrize("name", WITH_LR)
def test_negative_lr_by_value(bufs, name):
    _refused(name, bufs, ("lr=-1", "needs step == -1"), lr=-1.0, step=1)


@pytest.mark.parametrize("name", GUARDED)
def test_guarded_by_value(bufs, name):
    _refused(name, bufs, ("step=1", "the guarded form reads the live device-side step state"), step=1)


@pytest.mark.parametrize("name,which", [(n, w) for n in FLAT + GROUPS + TABLE + CATCHUP + LAZY_ROWS for w in "pgmv" if w in PARAMS[n]])
def test_misaligned_pgmv(bufs, name, which):
    words = ("pointer/alignment",)
    if which == "g" and name in TABLE and name != "segmm_adamw_table_scaled":
        words = ("phase 1", "needs g")          # the table step wants g in phase 1 only, and says so
    _refused(name, bufs, words, **{which: _off(which, 4)})


@pytest.mark.parametrize("name", PUSH + RING)
def test_misaligned_hist(bufs, name):
    _refused(name, bufs, ("pointer/alignment",), hist=_off("hist", 4))


@pytest.mark.parametrize("name", ("segmm_adamw_table_catchup_ema", "segmm_adamw_table_lazy_rows_ema"))
def test_shadow(bufs, name):
    _refused(name, bufs, ("shadow pointer/alignment",), shadow=_off("shadow", 4))
    _refused(name, bufs, ("shadow pointer/alignment",), shadow=None)
    _refused(name, bufs, ("shadow overlaps p", "disjoint"), shadow=_off("p", 16))


@pytest.mark.parametrize("name", EMA)
def test_ema_update_ranges(bufs, name):
    _refused(name, bufs, ("16-byte aligned",), shadow=_off("shadow", 4))
    _refused(name, bufs, ("16-byte aligned",), p=_off("p", 4))
    _refused(name, bufs, ("overlap", "disjoint"), shadow=_off("p", 16))


@pytest.mark.parametrize("name", LR_SCALE)
def test_lr_scale(bufs, name):
    _refused(name, bufs, ("lr_scale=-1", "finite, >= 0"), lr_scale=-1.0)
    _refused(name, bufs, ("lr_scale=inf", "finite, >= 0"), lr_scale=math.inf)


@pytest.mark.parametrize("name", TABLE + RING)
def test_width(bufs, name):
    _refused(name, bufs, ("width % 4",), width=6)


@pytest.mark.parametrize("name", PUSH + RING)
def test_cap_zero(bufs, name):
    _refused(name, bufs, ("cap=0 (>= 1)",) if name in PUSH else ("cap >= 1",), cap=0)


@pytest.mark.parametrize("name", CATCHUP + STAMP)
def test_target(bufs, name):
    _refused(name, bufs, ("target=2 (relative=1", "0 or -1 from the device-side step count"), relative=1, target=2)
    _refused(name, bufs, ("target=-1 (relative=0", ">= 0 by value"), relative=0, target=-1)


@pytest.mark.parametrize("name", ("segmm_adamw_table_lrs", "segmm_adamw_table_lrs_guarded"))
def test_coef_in_phase_0(bufs, name):
    _refused(name, bufs, ("a scaled update is phase 1 only",), phase=0, coef=lambda b: b.ptr("coef"))


@pytest.mark.parametrize("name", SCALED)
def test_scaled_needs_coef(bufs, name):
    _refused(name, bufs, ("null coef",), coef=None)


def test_catchup_flags_without_ids(bufs):
    _refused("segmm_adamw_table_catchup", bufs, ("flags mark LISTED rows",), ids=None, n_ids=0)


@pytest.mark.parametrize("name", EMA + ("segmm_adamw_hist_push_ema",))
def test_ema_weight(bufs, name):
    key = "ema_weight" if name == "segmm_adamw_hist_push_ema" else "weight"
    _refused(name, bufs, ("weight=0 ", "0 < weight <= 1"), **{key: 0.0})
    _refused(name, bufs, ("weight=1.5", "0 < weight <= 1"), **{key: 1.5})
