"""ctypes binding of ``libsegmm_hip.so`` (C ABI declared in ``include/segmm_hip.h``).

PyTorch is only plumbing here: it owns device memory and the HIP stream; every wrapper passes raw
device pointers, sizes and ``torch.cuda.current_stream()`` through the C ABI.  There is NO fallback:
if the shared library is missing or a call fails, a ``RuntimeError`` is raised (the product path
must never run on a silent eager/CPU substitute).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SEGMM_LIB") or os.path.join(_HERE, "libsegmm_hip.so")      # SEGMM_LIB: A/B builds of the kernels

_lib = None

_i, _i64, _f, _u64, _u32, _p = C.c_int, C.c_int64, C.c_float, C.c_uint64, C.c_uint32, C.c_void_p

# The mirror of include/segmm_hip.h comes from _abi.py, which tools/gen_cmd_dispatch.py generates from the header (build() refuses
# a stale one).  segmm_abi_version is left out of the tables: _lib_real binds it by hand, it gates everything else.
ABI_VERSION = _abi.ABI_VERSION
_CTYPE = {"i": _i, "i64": _i64, "f": _f, "u64": _u64, "u32": _u32, "p": _p}
_PROTOS = {n: ps for n, ps in _abi.PROTOTYPES.items() if n != "segmm_abi_version"}
SIGNATURES = {n: [_CTYPE[c] for _, c in ps] for n, ps in _PROTOS.items()}          # name -> argtypes
PARAMS = {n: tuple(p for p, _ in ps) for n, ps in _PROTOS.items()}                 # name -> parameter names


def lib():
    """The shared library (loaded once; raises if it has not been built) -- or, while a step is being recorded, a proxy that
    records every dispatchable call before making it."""
    L = _lib_real()
    rec = RECORDER
    if rec is not None:
        return _RecLib(L, rec)
    return L


def _lib_real():
    """Loads the shared library once; raises if it has not been built (``python -c 'import __graft_entry__ as g; g.build()'``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("segmminterest_amd: %s is missing -- build it with __graft_entry__.build() "
                           "(hipcc --offload-arch=gfx950); there is no fallback path" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    L.segmm_last_error.restype = C.c_char_p
    L.segmm_last_error.argtypes = []
    L.segmm_abi_version.restype = _i
    L.segmm_abi_version.argtypes = []
    L.segmm_cmd_op_name.restype = C.c_char_p
    L.segmm_cmd_op_name.argtypes = [_i]
    for name, at in SIGNATURES.items():
        fn = getattr(L, name)
        fn.argtypes = at
        fn.restype = _i
    if L.segmm_abi_version() != ABI_VERSION:
        raise RuntimeError("libsegmm_hip.so ABI %d != expected %d: rebuild" % (L.segmm_abi_version(), ABI_VERSION))
    _lib = L
    return L


# =============================================================================================== recorded launch sequences
# include/segmm_hip.h "Recorded launch sequences": the per-op calls of ONE eager training step are recorded (entry point, its
# arguments, the stream slot) and replayed every step from C by segmm_run_phase / the named phase entry points -- one
# foreign-function call per part of the step instead of one per kernel (+ the Python that sequences them).
_K = _abi.CONSTANTS
CMD_MAX_ARGS = _K["SEGMM_CMD_MAX_ARGS"]
OP_FORK, OP_JOIN = _K["SEGMM_OP_FORK"], _K["SEGMM_OP_JOIN"]
(PHASE_STEP_BEGIN, PHASE_EMBED_FWD, PHASE_LAYER_FWD, PHASE_HEAD_LOSS_FWD, PHASE_HEAD_LOSS_BWD, PHASE_LAYER_BWD, PHASE_EMBED_BWD,
 PHASE_STEP_TAIL) = (_K["SEGMM_PHASE_" + n] for n in ("STEP_BEGIN", "EMBED_FWD", "LAYER_FWD", "HEAD_LOSS_FWD", "HEAD_LOSS_BWD", "LAYER_BWD",
                                                      "EMBED_BWD", "STEP_TAIL"))
PHASE_ENTRY = ("segmm_step_begin", "segmm_embed_fwd", "segmm_layer_fwd", "segmm_head_loss_fwd", "segmm_head_loss_bwd",
               "segmm_layer_bwd", "segmm_embed_bwd", "segmm_step_tail")


class CmdArg(C.Union):
    _fields_ = [("i", C.c_int64), ("f", C.c_double), ("p", C.c_void_p)]


class Cmd(C.Structure):
    """segmm_cmd_t"""
    _fields_ = [("op", C.c_int32), ("stream", C.c_int32), ("a", CmdArg * CMD_MAX_ARGS)]


class Phase(C.Structure):
    """segmm_phase_t"""
    _fields_ = [("kind", C.c_int32), ("backbone", C.c_int32), ("layer", C.c_int32), ("n_cmds", C.c_int32), ("cmds", C.POINTER(Cmd))]


def _member(ct):
    """The segmm_arg_t member that carries an argument of ctypes type ``ct`` (what the generated dispatch switch reads it from)."""
    return "f" if ct is _f else "p" if ct is _p else "i"


def cmd_arg(c, name, param):
    """The value of parameter ``param`` (its name in the header) in the recorded command ``c`` of the entry point ``name``."""
    k = PARAMS[name].index(param)
    return getattr(c.a[k], _member(SIGNATURES[name][k]))


def cmd_set_arg(c, name, param, value):
    """Rewrites parameter ``param`` (its name in the header) of the recorded command ``c`` of the entry point ``name``: the slots of
    a replayed command that change from replay to replay, found by name -- never by matching addresses."""
    k = PARAMS[name].index(param)
    setattr(c.a[k], _member(SIGNATURES[name][k]), value)


_op_ids = None


def op_ids():
    """{entry point name: op id} of the library's dispatch table (segmm_cmd_op_name)."""
    global _op_ids
    if _op_ids is None:
        L = lib()
        _op_ids = {L.segmm_cmd_op_name(i).decode(): i for i in range(L.segmm_cmd_op_count())}
    return _op_ids


RECORDER = None          # a Recorder while Trainer.record() runs its one eager step


class Recorder:
    """Collects the C-ABI calls of one eager step, split into phases by :func:`mark`."""

    def __init__(self, main_stream: int, side_stream: int, aux_stream: int = 0):
        self.streams = {int(main_stream): 0, int(side_stream): 1}
        if aux_stream:
            self.streams[int(aux_stream)] = 2
        self.phases = []          # [kind, backbone, layer, [(op, slot, [(field, value)])]]
        self.keep = []            # host structs / arrays the recorded pointer arguments name
        self.pslots = {}          # finish(): index in its result -> [(command, argument slot)] of the pointer arguments
        self.ops = op_ids()

    def mark(self, kind, backbone=0, layer=0):
        self.phases.append([int(kind), int(backbone), int(layer), []])

    def _cmds(self):
        if not self.phases or callable(self.phases[-1]):
            raise RuntimeError("recorder: a launch before the first phase marker")
        return self.phases[-1][3]

    def pseudo(self, op, slot=1):
        self._cmds().append((op, slot, []))

    def callback(self, fn):
        """A host action between launches (a data-parallel collective, a wait for one): replayed by calling ``fn`` again at the
        same point of the launch order.  The launches that follow continue the current phase in a new fragment."""
        last = self.phases[-1] if self.phases else [PHASE_STEP_BEGIN, 0, 0, []]
        self.phases.append(fn)
        self.phases.append([last[0], last[1], last[2], []])

    def call(self, name, args):
        at = SIGNATURES[name]
        if len(args) != len(at) or at[-1] is not _p:
            raise RuntimeError("recorder: %s called with %d arguments" % (name, len(args)))
        slot = self.streams.get(int(args[-1] or 0))
        if slot is None:
            raise RuntimeError("recorder: %s was enqueued on a stream that is neither the step's main, side nor auxiliary stream; this "
                               "launch sequence cannot be replayed (prefetch / third-stream knobs must be off)" % name)
        vals = []
        for ct, v in zip(at[:-1], args[:-1]):
            fld = _member(ct)
            if fld == "f":
                vals.append(("f", float(v)))
            elif fld == "p":
                if v is None:
                    vals.append(("p", None))
                elif isinstance(v, int):
                    vals.append(("p", v or None))
                else:          # byref(struct) / cast(array) / ctypes instance: a host object that must outlive the replay
                    obj = getattr(v, "_obj", v)
                    self.keep.append((v, obj))
                    addr = v.value if isinstance(v, C.c_void_p) else C.addressof(obj)
                    vals.append(("p", addr))
            else:
                iv = int(v)
                vals.append(("i", iv - (1 << 64) if iv >= (1 << 63) else iv))
        self._cmds().append((self.ops[name], slot, vals))

    def finish(self):
        """-> list of (Phase struct, Cmd array); the arrays are referenced by the Phase structs (keep both)."""
        out = []
        for item in self.phases:
            if callable(item):
                out.append((item, None))
                continue
            kind, bb, layer, cmds = item
            if not cmds:          # (an empty fragment behind a callback)
                continue
            arr = (Cmd * max(len(cmds), 1))()
            pslots = []          # (command, argument slot) of every non-null POINTER argument: what a replay may re-base
            for ci, (c, (op, slot, vals)) in enumerate(zip(arr, cmds)):
                c.op, c.stream = op, slot
                for k, (fld, v) in enumerate(vals):
                    setattr(c.a[k], fld, v)
                    if fld == "p" and v:
                        pslots.append((ci, k))
            self.pslots[len(out)] = pslots
            ph = Phase(kind=kind, backbone=bb, layer=layer, n_cmds=len(cmds), cmds=C.cast(arr, C.POINTER(Cmd)))
            out.append((ph, arr))
        return out


class _RecLib:
    """``lib()`` while recording: every dispatchable entry point is recorded, then executed."""

    def __init__(self, real, rec):
        self._real, self._rec = real, rec

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        rec = self._rec
        if name not in rec.ops:
            return fn

        def call(*args):
            rec.call(name, args)
            return fn(*args)
        return call


def torch_fallback(what):
    """A torch kernel (dtype / layout conversion, sort, copy) is about to run inside the step: fine in an eager step, fatal
    while the step is being recorded -- the launch would be missing from the replay, which would keep using the record-time
    result without any error."""
    if RECORDER is not None:
        raise RuntimeError("record(): %s runs a torch kernel inside the step; a recorded step would silently drop it "
                           "(pass bool masks, int64 ids / labels and contiguous float32 / float16 / bfloat16 / 8-bit features, at most %d ids per table lookup)" % (what, ARGSORT_MAX))


def mark(kind, backbone=0, layer=0):
    """Phase boundary of the step (no-op unless a step is being recorded)."""
    if RECORDER is not None:
        RECORDER.mark(kind, backbone, layer)


def host_action(fn):
    """Run ``fn()`` now; while a step is being recorded, also note it as a host action of the step (Recorder.callback)."""
    if RECORDER is not None:
        RECORDER.callback(fn)
    return fn()


def stream_table(streams, events):
    """(ctypes array of hipStream_t, count, ctypes array of hipEvent_t) for :func:`run_phase`: ``streams`` = raw handles of the main,
    side (and auxiliary) stream, ``events`` = two raw event handles per non-main stream."""
    sa = (C.c_void_p * len(streams))(*[int(x) for x in streams])
    ea = (C.c_void_p * max(len(events), 1))(*[int(x) for x in events])
    return sa, len(streams), ea


def run_phase(phase: "Phase", table):
    L = _lib_real()
    sa, n, ea = table
    _check(getattr(L, PHASE_ENTRY[phase.kind])(C.addressof(phase), sa, n, ea), PHASE_ENTRY[phase.kind])


def fill_zero(t: torch.Tensor):
    """``t.zero_()`` through the C ABI (a recordable command; contiguous tensors only)."""
    if not t.is_contiguous():
        raise RuntimeError("fill_zero: non-contiguous view")
    if t.numel():
        _check(lib().segmm_fill_zero(t.data_ptr(), t.numel() * t.element_size(), _stream()), "segmm_fill_zero")


def copy_bytes(dst: torch.Tensor, src: torch.Tensor):
    """``dst.copy_(src)`` of same-sized contiguous tensors through the C ABI (a recordable, re-basable command)."""
    nb = src.numel() * src.element_size()
    if not (dst.is_contiguous() and src.is_contiguous()) or dst.numel() * dst.element_size() != nb:
        raise RuntimeError("copy_bytes: contiguous tensors of the same byte size")
    if nb:
        _check(lib().segmm_copy_bytes(dst.data_ptr(), src.data_ptr(), nb, _stream()), "segmm_copy_bytes")


def vec_add(out: torch.Tensor, a: torch.Tensor, b: torch.Tensor, n=None, out_off=0, a_off=0, b_off=0):
    """segmm_vec_add: ``out[out_off + i] = a[a_off + i] + b[b_off + i]`` for i < n (default: all of ``out``) over contiguous float32
    tensors, offsets in floats like ``adamw``'s ``p_off``.  ``out`` may be exactly an operand; a partial overlap is refused by the
    library.  A recordable, re-basable command."""
    for t, name in ((out, "out"), (a, "a"), (b, "b")):
        _f32c(t, "vec_add: " + name)
    _dev(out, a, b)
    n = out.numel() - out_off if n is None else int(n)
    if n < 0 or min(out_off, a_off, b_off) < 0 or out_off + n > out.numel() or a_off + n > a.numel() or b_off + n > b.numel():
        raise RuntimeError("vec_add: %d elements from offsets %d / %d / %d do not fit tensors of %d / %d / %d"
                           % (n, out_off, a_off, b_off, out.numel(), a.numel(), b.numel()))
    with _kprof("vec_add", 12 * n):
        _check(lib().segmm_vec_add(out.data_ptr() + 4 * out_off, a.data_ptr() + 4 * a_off, b.data_ptr() + 4 * b_off, n, _stream()), "segmm_vec_add")


def ema_update(shadow: torch.Tensor, p: torch.Tensor, n, weight, warmup, step, shadow_off=0, p_off=0, guard=False):
    """segmm_ema_update: ``shadow[i] += (p[i] - shadow[i]) * w`` for i < n over contiguous float32 tensors (offsets in floats), three
    rounded fp32 operations per element.  ``w`` = ``weight`` or, with ``warmup``, max(weight, fp32(9 / (10 + t))), t = ``step`` (>= 1)
    or, with step = -1, the bound device step state's count.  16-byte aligned, disjoint ranges.  A recordable command.
    ``guard``: segmm_ema_update_guarded (step = -1): nothing is written in a step the non-finite guard skipped."""
    _f32c(shadow, "ema_update: shadow")
    _f32c(p, "ema_update: p")
    _dev(shadow, p)
    n = int(n)
    if n < 0 or min(shadow_off, p_off) < 0 or shadow_off + n > shadow.numel() or p_off + n > p.numel():
        raise RuntimeError("ema_update: %d elements from offsets %d / %d do not fit tensors of %d / %d" % (n, shadow_off, p_off, shadow.numel(), p.numel()))
    with _kprof("ema_update", 12 * n):
        fn = "segmm_ema_update_guarded" if guard else "segmm_ema_update"
        _check(getattr(lib(), fn)(shadow.data_ptr() + 4 * shadow_off, p.data_ptr() + 4 * p_off, n, float(weight), int(bool(warmup)), int(step),
                                  _stream()), fn)


def vec_swap(a: torch.Tensor, b: torch.Tensor, n=None, a_off=0, b_off=0):
    """segmm_vec_swap: ``a[a_off + i] <-> b[b_off + i]`` for i < n (default: all of ``a``) over contiguous float32 tensors; 16-byte
    aligned, disjoint ranges.  A recordable command."""
    _f32c(a, "vec_swap: a")
    _f32c(b, "vec_swap: b")
    _dev(a, b)
    n = a.numel() - a_off if n is None else int(n)
    if n < 0 or min(a_off, b_off) < 0 or a_off + n > a.numel() or b_off + n > b.numel():
        raise RuntimeError("vec_swap: %d elements from offsets %d / %d do not fit tensors of %d / %d" % (n, a_off, b_off, a.numel(), b.numel()))
    with _kprof("vec_swap", 16 * n):
        _check(lib().segmm_vec_swap(a.data_ptr() + 4 * a_off, b.data_ptr() + 4 * b_off, n, _stream()), "segmm_vec_swap")


def _check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (what, rc, _lib_real().segmm_last_error().decode()))


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """hipStream_t of torch's current stream on the current device (the raw-handle query: no Stream object per launch)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("segmminterest_amd kernels need device tensors (got %s); no CPU fallback" % t.device)


def _f32c(t, name="tensor"):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError("%s must be contiguous float32 (got %s, contiguous=%s)" % (name, t.dtype, t.is_contiguous()))
    return t


GEMM_PROFILE = None       # bench.py sets this to a list to time every GEMM launch with HIP events
ATTN_PROFILE = None       # ... and every attention launch: (kind, B, H, dh, Lq, La, Lb, event0, event1)
KERNEL_PROFILE = None     # ... and selected HBM-bound launches: (name, algorithmic bytes, event0, event1)


def gemm_record(layout, M, N, K, write_c=None):
    """What a GEMM_PROFILE entry of one GEMM launch starts with, or None for a launch that is not timed.  ``write_c``: that argument
    of segmm_gemm_p (None: a launch of segmm_gemm / _x / _h).  A plane-engine launch is listed under 10 + layout (bench.py's
    per-shape table); its repair launch (write_c bit 1) does no work normally: not a GEMM of the roofline."""
    if write_c is None:
        return (layout, M, N, K)
    return None if write_c & 2 else (10 + layout, M, N, K)


def attn_record(B, H, dh, Lq, La, Lb, phase=None, planes=None):
    """What an ATTN_PROFILE entry of one attention launch starts with.  ``phase`` / ``planes`` (an AttnPlanes or None): those
    arguments of segmm_attn_bwd; ``phase=None``: a forward launch."""
    if phase is None:
        return ("fwd", B, H, dh, Lq, La, Lb)
    repair = planes is not None and (planes.flags & ATTN_REPAIR)
    kind = "bwd" if phase == 0 else "bwd4r" if repair else "bwd4" if phase >= 4 else "bwd%d" % phase
    # (phase 5 / 6 = one key block of the fused backward: its FLOPs are the block's; a repair launch does no work normally)
    return (kind, B, H, dh, Lq, 0 if phase == 6 else La, 0 if phase == 5 else Lb)


class _kprof:
    """``with _kprof(name, nbytes):`` -- HIP events around a launch when bench.py asked for them (KERNEL_PROFILE is a list)."""

    def __init__(self, name, nbytes):
        self.name, self.nbytes = name, nbytes

    def __enter__(self):
        self.on = KERNEL_PROFILE is not None
        if self.on:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *exc):
        if self.on:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            KERNEL_PROFILE.append((self.name, self.nbytes, self.e0, e1))


def attn_peak_tflops():
    """Dense MFMA peak of the instruction the attention kernels use (roofline denominator of bench.py)."""
    return 157.3          # v_mfma_f32_16x16x4_f32 (exact fp32 products)


ATTN_PIN_CALLS = 0          # attention calls that were handed input planes (bench.py names the kernels it measured by this)


def attn_kernel_name():
    if ATTN_PIN_CALLS:
        return ("attn_fwd_pl_kernel + attn_bwd_pl_kernel (csrc/attention_pl.h): Q / K / V read from the projection GEMMs' P32 planes "
                "(forward: K / V by LDS-DMA into a conflict-free rotated image, 9 key tiles over both key blocks; backward: dQ + dK + dV in "
                "one kernel per key block, row fragments straight to registers, K^T read back transposed from LDS), 3 x "
                "v_mfma_f32_16x16x16_f16 per product, O / dQ / dK / dV written as planes (the backward: planes only + a repair launch)")
    return ("attn_fwd (v_mfma_f32_16x16x4_f32, exact fp32 products) + attn_bwd_fused16 / attn_bwd_fused (dQ + dK + dV in one kernel per key "
            "block, S and dP computed once: 10 dh Lq T FLOP instead of 14; fp16x3 products -- 3 x v_mfma_f32_16x16x16_f16 -- for single-chunk "
            "launches with more than 32 queries, exact fp32 products otherwise)")
ENGINE_F32, ENGINE_BF16X6, ENGINE_F16X3, ENGINE_F16X3P = 0, 1, 2, 3
# default engine of gemm(): the scaled two-term fp16 split on the fp16 matrix cores (22-bit operands, three exact
# partial products, fp32 accumulation: measured error vs fp64 at or below the f32-MFMA kernel's on every layout).
# SEGMM_GEMM=bf16x6 selects the exact 3-way bf16 split (six products), SEGMM_GEMM=f32 the f32-input MFMA kernel
# (A/B and parity cross-checks)
# "f16x3p" (default): the same fp16x3 arithmetic with operands PRE-SPLIT into fp16 planes by their producers and staged by
# LDS-DMA (gemm_p / csrc/gemm_planes.h); raw gemm() calls under it run the on-the-fly fp16x3 kernel.
GEMM_ENGINE = {"f32": 0, "bf16x6": 1, "f16x3": 2, "f16x3p": 3}[os.environ.get("SEGMM_GEMM", "f16x3p")]
AMAX_SLOTS = _K["SEGMM_AMAX_SLOTS"]          # partial maxima per tensor written by the fused producers (SEGMM_AMAX_SLOTS)
AMAX_PARTS = 1024         # ... and by the stand-alone absmax() pass
LAYOUT_NT, LAYOUT_NN, LAYOUT_TN = 0, 1, 2
ACT_NONE, ACT_GELU, ACT_DGELU, ACT_RELU, ACT_DRELU = 0, 1, 2, 3, 4


class PO:
    """Plane output of a producer kernel: (planes tensor, element offset, ld2, site header, device address of the delayed scale)."""
    __slots__ = ("planes", "p_off", "ld2", "hdr", "scale_ptr")

    def __init__(self, planes, ld2, hdr, scale_ptr, p_off=0):
        self.planes, self.ld2, self.hdr, self.scale_ptr, self.p_off = planes, ld2, hdr, scale_ptr, p_off

    def args(self):
        return (self.planes.data_ptr() + 2 * self.p_off, self.ld2, self.hdr.data_ptr(), self.scale_ptr)


_NO_PO = (None, 0, None, None)


def _po(po):
    return _NO_PO if po is None else po.args()


ELEM_F16, ELEM_BF16 = _K["SEGMM_ELEM_F16"], _K["SEGMM_ELEM_BF16"]
_ELEM = {torch.float16: ELEM_F16, torch.bfloat16: ELEM_BF16}          # 16-bit input features -> the ``elem`` code of the _h entry points
ELEM_E4M3, ELEM_E5M2, ELEM_I8 = _K["SEGMM_ELEM_E4M3"], _K["SEGMM_ELEM_E5M2"], _K["SEGMM_ELEM_I8"]
# 8-bit input features -> the ``elem`` code of the _b entry points (OCP fp8 / bf8 and int8; uint8 is NOT a feature dtype: features are
# signed, and a mask buffer must not pass for a table)
_ELEM8 = {torch.float8_e4m3fn: ELEM_E4M3, torch.float8_e5m2: ELEM_E5M2, torch.int8: ELEM_I8}
FEATURE_DTYPES = (torch.float32, torch.float16, torch.bfloat16) + tuple(_ELEM8)
FEATURE_DTYPE_NAMES = ("torch.float32, torch.float16 or torch.bfloat16, or 8-bit: torch.float8_e4m3fn, torch.float8_e5m2 or torch.int8 "
                       "(not torch.uint8: features are signed)")


def _feat(t, name):
    """The ``elem`` code of an input feature tensor (None: float32; 1, 2: the _h forms; 3, 4, 5: the _b forms); refuses every other
    dtype and non-contiguous views."""
    if t.dtype not in FEATURE_DTYPES:
        raise RuntimeError("%s is %s; input features are %s" % (name, t.dtype, FEATURE_DTYPE_NAMES))
    if not t.is_contiguous():
        raise RuntimeError("%s (%s) must be contiguous" % (name, t.dtype))
    return _ELEM.get(t.dtype, _ELEM8.get(t.dtype))


def l1norm(x, out=None, inv_scale=None, amax=None, po=None):
    """``x``: float32, or float16 / bfloat16, or float8_e4m3fn / float8_e5m2 / int8 (widened exactly in the kernel: the float32 result
    on the widened ``x``, bit for bit); ``out`` / ``inv_scale``: float32.  ``amax``: optional zeroed [AMAX_SLOTS] vector that receives the partial maxima of |out|
    (fp16x3 GEMM operand); ``po``: optional plane output (PO)."""
    _dev(x)
    elem = _feat(x, "l1norm: x")
    for t, name in ((out, "out"), (inv_scale, "inv_scale")):
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError("l1norm: %s must be float32 whatever x is (got %s)" % (name, t.dtype))
    D = x.shape[-1]
    rows = x.numel() // D
    if elem is None:
        _check(lib().segmm_l1norm(_ptr(x), _ptr(out), _ptr(inv_scale), rows, D, _ptr(amax), *_po(po), _stream()), "segmm_l1norm")
    elif x.dtype in _ELEM:
        _check(lib().segmm_l1norm_h(_ptr(x), elem, _ptr(out), _ptr(inv_scale), rows, D, _ptr(amax), *_po(po), _stream()), "segmm_l1norm_h")
    else:
        _check(lib().segmm_l1norm_b(_ptr(x), elem, _ptr(out), _ptr(inv_scale), rows, D, _ptr(amax), *_po(po), _stream()), "segmm_l1norm_b")


def quantize_rows(x, dtype, out=None, scale_out=None):
    """float32 rows ``x`` [..., D] -> 8-bit codes of ``dtype`` (float8_e4m3fn / float8_e5m2 / int8), one wave per row: each row is
    scaled by a power of two (fp8: max|x| lands in [128, 256) / [16384, 32768)) or by 127 / max|x| (int8) and rounded to nearest even;
    a row whose max|x| is under 2^-100 or not finite gives zero codes.  ``scale_out``: optional float32 [rows], the factor per row (0
    for such a row).  The scale is not needed by the readers: L1 normalisation cancels it (segmm_quantize_rows in the header)."""
    _dev(x)
    if dtype not in _ELEM8:
        raise RuntimeError("quantize_rows: dtype %s; the 8-bit feature dtypes are torch.float8_e4m3fn, torch.float8_e5m2 and torch.int8" % (dtype,))
    if x.dtype != torch.float32 or not x.is_contiguous() or x.dim() < 1:
        raise RuntimeError("quantize_rows: x must be a contiguous float32 tensor (got %s, contiguous=%s)" % (x.dtype, x.is_contiguous()))
    D = x.shape[-1]
    rows = x.numel() // D if D else 0
    if out is None:
        out = torch.empty(x.shape, dtype=dtype, device=x.device)
    if out.dtype != dtype or out.shape != x.shape or not out.is_contiguous() or out.device != x.device:
        raise RuntimeError("quantize_rows: out must be a contiguous %s tensor of x's shape on x's device" % (dtype,))
    if scale_out is not None and (scale_out.dtype != torch.float32 or scale_out.numel() != rows or not scale_out.is_contiguous()
                                  or scale_out.device != x.device):
        raise RuntimeError("quantize_rows: scale_out must be a contiguous float32 tensor of one element per row on x's device")
    _check(lib().segmm_quantize_rows(_ptr(x), rows, D, _ELEM8[dtype], _ptr(out), _ptr(scale_out), _stream()), "segmm_quantize_rows")
    return out


def gemm(layout, M, N, K, A, lda, B, ldb, Cout, ldc, bias=None, row_scale=None, residual=None, ldr=0, res_period=0,
         activation=0, aux=None, ldaux=0, drop_p=0.0, seed=0, site=0, splits=1, workspace=None, accumulate=False,
         a_off=0, b_off=0, c_off=0, engine=None, a_planes=None, b_planes=None, nplanes=3, a_amax=None, b_amax=None, c_amax=None):
    """Raw strided GEMM; ``*_off`` are element offsets into the tensors (column slices of fused buffers).
    ``a_planes`` / ``b_planes`` = (16-bit planes tensor [nplanes, ...], element offset): pre-split operand (NT only).
    ``a_amax`` / ``b_amax`` (fp16x3 engine): float32 vectors of partial maxima of |A| / |B|; computed here with
    :func:`absmax` when the caller has none.  ``c_amax``: zeroed [AMAX_SLOTS] vector that receives the partial
    maxima of |C| (ignored by the other engines: nothing consumes it there)."""
    _dev(Cout)
    es = 4
    prof = GEMM_PROFILE
    if prof is not None:          # bench.py: HIP events on the launch stream around the dominant kernel
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
    eng = GEMM_ENGINE if engine is None else int(engine)
    if eng == ENGINE_F16X3P:
        eng = ENGINE_F16X3
    # the arguments segmm_gemm / _x / _h share (a null fp32 operand is refused by the library unless its planes are given)
    head = (layout, M, N, K, None if A is None else A.data_ptr() + a_off * es, lda, None if B is None else B.data_ptr() + b_off * es, ldb,
            Cout.data_ptr() + c_off * es, ldc, _ptr(bias), _ptr(row_scale), _ptr(residual), ldr, res_period, activation, _ptr(aux), ldaux,
            float(drop_p), int(seed), int(site), int(splits), _ptr(workspace), int(bool(accumulate)))
    planes = (None if a_planes is None else a_planes[0].data_ptr() + 2 * a_planes[1], 0 if a_planes is None else a_planes[0].stride(0),
              None if b_planes is None else b_planes[0].data_ptr() + 2 * b_planes[1], 0 if b_planes is None else b_planes[0].stride(0))
    if eng == ENGINE_F16X3:
        if a_amax is None:
            if a_planes is not None:
                raise RuntimeError("pre-split fp16 planes need the partial maxima they were made with")
            a_amax = absmax(A, K if layout == LAYOUT_TN else M, M if layout == LAYOUT_TN else K, lda, off=a_off)
        if b_amax is None:
            if b_planes is not None:
                raise RuntimeError("pre-split fp16 planes need the partial maxima they were made with")
            b_amax = absmax(B, N if layout == LAYOUT_NT else K, K if layout == LAYOUT_NT else N, ldb, off=b_off)
        _check(lib().segmm_gemm_h(*head, *planes, a_amax.data_ptr(), a_amax.numel(), b_amax.data_ptr(), b_amax.numel(), _ptr(c_amax),
                                  _stream()), "segmm_gemm_h")
    elif a_planes is None and b_planes is None and nplanes == 3:
        _check(lib().segmm_gemm(*head, eng, _stream()), "segmm_gemm")
    else:
        if eng != ENGINE_BF16X6:
            raise RuntimeError("pre-split operands / nplanes=2 need the bf16x6 engine")
        _check(lib().segmm_gemm_x(*head, *planes, int(nplanes), _stream()), "segmm_gemm_x")
    if prof is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        prof.append(gemm_record(layout, M, N, K) + (e0, e1))


SITE_HDR = _K["SEGMM_SITE_HDR"]          # floats in front of the partial maxima of a plane tensor's site header
SITE_FLOATS = SITE_HDR + AMAX_SLOTS


class PT:
    """A GEMM operand as its producer leaves it: P32 fp16 planes (``planes`` [rows, 2 * cols] halves, or a wider buffer
    with ``p_off`` / ``ld2`` selecting a column slice), the site header ``hdr`` ([SITE_FLOATS] floats: scale, overflow flag,
    partial maxima) and -- optionally -- the fp32 copy ``f32`` (``f_off`` / ``ldf``) that consumers fall back to."""
    __slots__ = ("planes", "p_off", "ld2", "hdr", "f32", "f_off", "ldf", "rows", "cols")

    def __init__(self, planes, hdr, rows, cols, ld2=None, p_off=0, f32=None, ldf=None, f_off=0):
        self.planes, self.hdr, self.rows, self.cols = planes, hdr, rows, cols
        self.ld2 = 2 * cols if ld2 is None else ld2
        self.p_off = p_off
        self.f32, self.ldf, self.f_off = f32, (cols if ldf is None else ldf), f_off

    def cols_slice(self, c0, ncols):
        """Columns [c0, c0 + ncols) of the same rows (c0, ncols multiples of 32)."""
        return PT(self.planes, self.hdr, self.rows, ncols, self.ld2, self.p_off + 2 * c0, self.f32, self.ldf, self.f_off + c0)

    def pptr(self):
        return self.planes.data_ptr() + 2 * self.p_off

    def fptr(self):
        return None if self.f32 is None else self.f32.data_ptr() + 4 * self.f_off


def new_site(device, n=1):
    """Zeroed site headers [n, SITE_FLOATS]."""
    return torch.zeros((n, SITE_FLOATS), dtype=torch.float32, device=device)


def split_p32(x, rows, cols, ld, planes, ld2, hdr, mode=0, x_off=0, p_off=0):
    """fp32 view -> P32 planes; mode 0: exact scale from the header's (complete) partial maxima; 1: scale hdr[0] as given."""
    _check(lib().segmm_split_p32(x.data_ptr() + 4 * x_off, rows, cols, ld, planes.data_ptr() + 2 * p_off, ld2, hdr.data_ptr(), int(mode),
                                 _stream()), "segmm_split_p32")


def split_p32_transpose(x, R, Cc, ld, planes, ld2, hdr, x_off=0, p_off=0):
    _check(lib().segmm_split_p32_transpose(x.data_ptr() + 4 * x_off, R, Cc, ld, planes.data_ptr() + 2 * p_off, ld2, hdr.data_ptr(),
                                           _stream()), "segmm_split_p32_transpose")


def wsplit_p32(flat, desc, n_mats, n_tiles, hdr, wpl, wTpl):
    """Absmax + exact P32 split (+ transposed split) of every weight matrix described in ``desc`` (see segmm_wsplit_p32)."""
    _check(lib().segmm_wsplit_p32(flat.data_ptr(), desc.data_ptr(), int(n_mats), int(n_tiles), hdr.data_ptr(), wpl.data_ptr(),
                                  wTpl.data_ptr(), _stream()), "segmm_wsplit_p32")


def to_planes(x, rows, cols, ld=None, x_off=0, keep_f32=True):
    """Stand-alone adapter: absmax pass + exact split pass -> PT (tests, external inputs, first use of a site)."""
    ld = cols if ld is None else ld
    hdr = new_site(x.device)[0]
    absmax(x, rows, cols, ld, off=x_off, out=hdr[SITE_HDR:])
    planes = torch.empty((rows, 2 * cols), dtype=torch.float16, device=x.device)
    split_p32(x, rows, cols, ld, planes, 2 * cols, hdr, mode=0, x_off=x_off)
    return PT(planes, hdr, rows, cols, f32=x if keep_f32 else None, ldf=ld, f_off=x_off)


def gemm_p(layout, M, N, K, A: "PT", B: "PT", Cout, ldc, c_pt: "PT" = None, write_c=True, bias=None, row_scale=None, residual=None,
           ldr=0, res_period=0, activation=0, aux=None, ldaux=0, drop_p=0.0, seed=0, site=0, splits=1, workspace=None,
           accumulate=False, c_off=0, c_hdr=None, c_scale_ptr=None, colsum_out=None, repair=False, products=3):
    """Plane-operand GEMM (segmm_gemm_p).  ``c_pt``: optional plane output (its hdr[0] holds the scale to write with);
    ``c_hdr``: site header that only receives the partial maxima of |C| (no plane output).  ``repair``: the REPAIR launch of a
    planes-only NT output (``Cout=None, write_c=False``): same arguments, workgroups leave at once unless the output site's planes
    are unusable under the recorded scale, in which case they are rewritten with the exact scale of the recorded maxima.
    ``products``: 3 calls ``segmm_gemm_p`` (hl + lh + hh, fp32-accurate) exactly as before the argument existed; 1 calls
    ``segmm_gemm_pq`` with one product (hi . hi: fp16 operands, fp32 accumulate); anything else is the library's error."""
    wc = int(bool(write_c)) | (2 if repair else 0)
    head = gemm_record(layout, M, N, K, wc)
    prof = GEMM_PROFILE if head is not None else None
    if prof is not None:
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
    args = (layout, M, N, K, A.pptr(), A.ld2, A.hdr.data_ptr(), A.fptr(), A.ldf, B.pptr(), B.ld2, B.hdr.data_ptr(),
            B.fptr(), B.ldf, None if Cout is None else Cout.data_ptr() + 4 * c_off, ldc,
            None if c_pt is None else c_pt.pptr(), 0 if c_pt is None else c_pt.ld2,
            (None if c_hdr is None else c_hdr.data_ptr()) if c_pt is None else c_pt.hdr.data_ptr(), c_scale_ptr,
            wc, _ptr(bias), _ptr(row_scale), _ptr(residual),
            ldr, res_period, activation, _ptr(aux), ldaux, float(drop_p), int(seed), int(site), int(splits),
            _ptr(workspace), int(bool(accumulate)), _ptr(colsum_out))
    if products == 3:          # the default trainer's recorded sequences stay command for command what they were
        _check(lib().segmm_gemm_p(*args, _stream()), "segmm_gemm_p")
    else:
        _check(lib().segmm_gemm_pq(*args, int(products), _stream()), "segmm_gemm_pq")
    if prof is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        prof.append(head + (e0, e1))


def scales_update(arena, site_idx, n_rows, site_scale, stats, target=12, gain=None, gmax=None):
    _check(lib().segmm_scales_update(arena.data_ptr(), site_idx.data_ptr(), int(n_rows), site_scale.data_ptr(), stats.data_ptr(), int(target),
                                     _ptr(gain), _ptr(gmax), _stream()), "segmm_scales_update")


LIVE_SEED = 1 << 63          # dropout seed argument bit: XOR the device-side step words into the seed (segmm_step_advance)


def step_state_bytes():
    return int(lib().segmm_step_state_bytes())


def step_bind(state):
    """``segmm_step_bind``: the device-side step state (a caller-owned device tensor of step_state_bytes() bytes, or None: the
    library's own default state) that the launches which follow use -- the pointer travels in their arguments.
    The library holds the bare pointer, so the tensor is kept alive here for as long as it is bound: an owner that goes away
    without unbinding (a trainer that is dropped) must not hand the block back to the allocator, where the next tensor of that
    size would take it and ``step_set`` / a live dropout seed of a later caller would write and read somebody else's data."""
    global _STEP_BOUND
    _check(_lib_real().segmm_step_bind(None if state is None else state.data_ptr()), "segmm_step_bind")
    _STEP_BOUND = state


_STEP_BOUND = None          # the tensor behind the library's bound step-state pointer (None: the library's default state)


def step_set(seed, step, beta1=0.9, beta2=0.999):
    _check(lib().segmm_step_set(int(seed) & (2 ** 63 - 1), int(step), float(beta1), float(beta2), _stream()), "segmm_step_set")


def step_advance(beta1=0.9, beta2=0.999):
    _check(lib().segmm_step_advance(float(beta1), float(beta2), _stream()), "segmm_step_advance")


# ---- the non-finite guard (include/segmm_hip.h "THE NON-FINITE GUARD"): two words of the step state, skip and skipped
STEP_SKIP_WORD = _K["SEGMM_STEP_SKIP_WORD"]          # int32 index of ``skip`` in the step state; ``skipped`` is the word behind it


def step_advance_guarded(beta1=0.9, beta2=0.999):
    """segmm_step_advance_guarded: :func:`step_advance` with the bias corrections of the applied index; clears the verdict."""
    _check(lib().segmm_step_advance_guarded(float(beta1), float(beta2), _stream()), "segmm_step_advance_guarded")


def step_guard(out2):
    """segmm_step_guard: the verdict of the step from ``out2`` = the {norm, coef} :func:`grad_norm` wrote on this stream."""
    if out2.dtype != torch.float32 or out2.numel() < 2:
        raise RuntimeError("step_guard: out2 must be the two float32 of grad_norm")
    _check(lib().segmm_step_guard(out2.data_ptr(), _stream()), "segmm_step_guard")


def step_set_skipped(skipped):
    _check(lib().segmm_step_set_skipped(int(skipped), _stream()), "segmm_step_set_skipped")


def step_get_skipped():
    """(skip, skipped) of the device-side step state: the last step's verdict and the count of skipped steps; synchronises."""
    out = (C.c_uint32 * 2)()
    _check(_lib_real().segmm_step_get_skipped(C.addressof(out), C.addressof(out) + 4, _stream()), "segmm_step_get_skipped")
    return int(out[0]), int(out[1])


def step_get():
    """(seed words, step count, (bc1, sqrt(bc2))) of the device-side step state; synchronises the stream."""
    import ctypes
    seed, step, bc = ctypes.c_uint64(0), ctypes.c_int(0), (ctypes.c_float * 2)()
    _check(lib().segmm_step_get(ctypes.addressof(seed), ctypes.addressof(step), ctypes.addressof(bc), _stream()), "segmm_step_get")
    return int(seed.value), int(step.value), (float(bc[0]), float(bc[1]))


LIVE_LR = float(_K["SEGMM_LIVE_LR"])          # lr argument of the AdamW entry points: the device step state's rate (needs step = -1)
LR_KINDS = {n: _K["SEGMM_LR_" + n.upper()] for n in ("constant", "cosine", "linear", "step", "exp")}


def step_schedule(kind, base_lr, warmup_steps=0, start_factor=1.0, decay_steps=1, eta_min=0.0, gamma=1.0, step_size=1):
    """``segmm_step_schedule``: installs a learning-rate schedule (``kind``: a key of LR_KINDS or its number) in the bound step
    state and sets the state's rate for its current step count."""
    _check(lib().segmm_step_schedule(int(LR_KINDS.get(kind, kind)), float(base_lr), int(warmup_steps), float(start_factor), int(decay_steps),
                                     float(eta_min), float(gamma), int(step_size), _stream()), "segmm_step_schedule")


def step_set_base_lr(base_lr):
    _check(lib().segmm_step_set_base_lr(float(base_lr), _stream()), "segmm_step_set_base_lr")


def step_get_lr():
    """(lr of the state's current step, base_lr) of the device-side step state; synchronises the stream."""
    out = (C.c_float * 2)()
    _check(_lib_real().segmm_step_get_lr(C.addressof(out), C.addressof(out) + 4, _stream()), "segmm_step_get_lr")
    return float(out[0]), float(out[1])


def config_set(name, value):
    """``segmm_config_set``: set the tuning knob ``name`` (without the SEGMM_ prefix; see :func:`config_dump`); returns the previous value."""
    _KNOBS.clear()
    r = int(lib().segmm_config_set(name.encode(), int(value)))
    if r < 0 and name not in config_dump():
        _check(r, "segmm_config_set")
    return r


_KNOBS = {}


def knob(name):
    """Current value of one tuning knob (cached; ``config_set`` drops the cache)."""
    if not _KNOBS:
        _KNOBS.update({k: v[0] for k, v in config_dump().items()})
    return _KNOBS[name]


def config_dump():
    """{knob name: (value, doc)} of the library's tuning table (``segmm_config_dump``)."""
    n = int(lib().segmm_config_dump(None, 0)) + 1
    buf = C.create_string_buffer(n)
    lib().segmm_config_dump(buf, n)
    out = {}
    for ln in buf.value.decode().splitlines():
        k, rest = ln.split("=", 1)
        v, doc = rest.split("#", 1)
        out[k.replace("SEGMM_", "", 1)] = (int(v), doc.strip())
    return out


def attn_mode(mode=-1):
    """``segmm_attn_mode``: 0 exact-fp32 attention kernels, 1 fp16x3 where faster (default), 2 fp16x3 wherever built;
    returns the previous mode, ``mode < 0`` only queries."""
    return int(lib().segmm_attn_mode(int(mode)))


def mfma_sustained_tflops(ms_target=25.0):
    """Diagnostic: sustained fp16 matrix-core rate (TFLOP/s) of this GPU on random operand bits, registers only
    (``segmm_probe_mfma_rate``: 256 workgroups x 8 waves, the plane GEMM's accumulator order).  bench.py reports it beside
    the datasheet peak: the power management clocks a random-data MFMA stream down, so no real-data GEMM can reach the
    datasheet figure on this part."""
    import ctypes
    scratch = torch.zeros(1, dtype=torch.float32, device="cuda")
    fl = ctypes.c_double(0.0)
    iters = 4000

    def run(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _check(lib().segmm_probe_mfma_rate(256, int(n), scratch.data_ptr(), ctypes.addressof(fl), _stream()), "segmm_probe_mfma_rate")
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    ms = run(iters)                                   # warm-up + calibration
    iters = max(1000, int(iters * ms_target / max(ms, 1e-3)))
    ms = run(iters)
    return fl.value / (ms * 1e-3) * 1e-12


def absmax(x, rows, cols, ld, off=0, out=None):
    """Partial maxima of |x| over the [rows, cols] view (row stride ld) starting ``off`` elements into x."""
    if out is None:
        out = torch.empty(AMAX_PARTS, dtype=torch.float32, device=x.device)
    _check(lib().segmm_absmax(x.data_ptr() + 4 * off, rows, cols, ld, out.data_ptr(), out.numel(), _stream()), "segmm_absmax")
    return out


def split2h(x, planes, n, amax, x_off=0, p_off=0):
    """planes[0/1, p_off + i] = fp16 hi / lo of x.flat[x_off + i] * s(amax); planes is a [2, size] 16-bit tensor."""
    _check(lib().segmm_split2h(x.data_ptr() + 4 * x_off, planes.data_ptr() + 2 * p_off, n, planes.stride(0),
                               amax.data_ptr(), amax.numel(), _stream()), "segmm_split2h")


def split2h_transpose(x, R, Cc, ld, planes, amax, x_off=0, p_off=0):
    """planes[0/1, p_off + c*R + r] = fp16 hi / lo of x.flat[x_off + r*ld + c] * s(amax)."""
    _check(lib().segmm_split2h_transpose(x.data_ptr() + 4 * x_off, R, Cc, ld, planes.data_ptr() + 2 * p_off, planes.stride(0),
                                         amax.data_ptr(), amax.numel(), _stream()), "segmm_split2h_transpose")


def split3(x, planes, n, x_off=0, p_off=0):
    """planes[p, p_off + i] = p-th bf16 term of x.flat[x_off + i]; planes is a [3, size] bf16 tensor."""
    _check(lib().segmm_split3(x.data_ptr() + 4 * x_off, planes.data_ptr() + 2 * p_off, n, planes.stride(0), _stream()), "segmm_split3")


def split3_transpose(x, R, Cc, ld, planes, x_off=0, p_off=0):
    """planes[p, p_off + c*R + r] = p-th bf16 term of x.flat[x_off + r*ld + c]."""
    _check(lib().segmm_split3_transpose(x.data_ptr() + 4 * x_off, R, Cc, ld, planes.data_ptr() + 2 * p_off, planes.stride(0),
                                        _stream()), "segmm_split3_transpose")


def layernorm_fwd(x, gamma, beta, y, mean, rstd, eps=1e-12, drop_p=0.0, seed=0, site=0, amax=None, po=None):
    _dev(x, y)
    d = x.shape[-1]
    _check(lib().segmm_layernorm_fwd(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(mean), _ptr(rstd),
                                     x.numel() // d, d, eps, float(drop_p), int(seed), int(site), _ptr(amax), *_po(po), _stream()),
           "segmm_layernorm_fwd")


def layernorm_fwd_dot(x, gamma, beta, y, mean, rstd, dot_w, dot_b, dot_out, eps=1e-12, drop_p=0.0, seed=0, site=0, amax=None, po=None):
    """layernorm_fwd that also leaves dot_out[row] = y[row, :] . dot_w (+ dot_b[0])."""
    _dev(x, y)
    d = x.shape[-1]
    _check(lib().segmm_layernorm_fwd_dot(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(mean), _ptr(rstd),
                                         x.numel() // d, d, eps, float(drop_p), int(seed), int(site), _ptr(amax), *_po(po),
                                         _ptr(dot_w), _ptr(dot_b), _ptr(dot_out), _stream()),
           "segmm_layernorm_fwd_dot")


def layernorm_bwd_parts(rows, d):
    return lib().segmm_layernorm_bwd_parts(rows, d)


def layernorm_bwd(dy, x, mean, rstd, gamma, dx, dx_drop, part_dgamma, part_dbeta, drop_y_p=0.0, drop_y_site=0,
                  drop_b_p=0.0, drop_b_site=0, seed=0, amax=None, part_dsum=None, po=None):
    _dev(dy, x, dx)
    d = x.shape[-1]
    _check(lib().segmm_layernorm_bwd(_ptr(dy), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(dx), _ptr(dx_drop),
                                     _ptr(part_dgamma), _ptr(part_dbeta), _ptr(part_dsum), x.numel() // d, d, float(drop_y_p),
                                     int(drop_y_site), float(drop_b_p), int(drop_b_site), int(seed), _ptr(amax), *_po(po), _stream()),
           "segmm_layernorm_bwd")


def layernorm_bwd_outer(dy_row, dy_col, x, mean, rstd, gamma, dx, dx_drop, part_dgamma, part_dbeta, drop_y_p=0.0, drop_y_site=0,
                        drop_b_p=0.0, drop_b_site=0, seed=0, amax=None, part_dsum=None, po=None):
    """layernorm_bwd with the incoming gradient dy[row, c] = dy_row[row] * dy_col[c] formed inside the launch."""
    _dev(dy_row, x, dx)
    d = x.shape[-1]
    _check(lib().segmm_layernorm_bwd_outer(_ptr(dy_row), _ptr(dy_col), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(dx), _ptr(dx_drop),
                                           _ptr(part_dgamma), _ptr(part_dbeta), _ptr(part_dsum), x.numel() // d, d, float(drop_y_p),
                                           int(drop_y_site), float(drop_b_p), int(drop_b_site), int(seed), _ptr(amax), *_po(po), _stream()),
           "segmm_layernorm_bwd_outer")


def layernorm_bwd_pos_parts(rows, period, d):
    return lib().segmm_layernorm_bwd_pos_parts(rows, period, d)


def layernorm_bwd_pos(dy, x, mean, rstd, gamma, dx, dx_drop, part_dgamma, part_dbeta, part_pos, period, drop_y_p=0.0, drop_y_site=0,
                      drop_b_p=0.0, drop_b_site=0, seed=0, amax=None, part_dsum=None, po=None):
    """LayerNorm backward on the per-position grid: also leaves the per-wave sums of dx in ``part_pos`` [4 * parts, d].
    ``dx=None`` (with ``po``, no ``dx_drop``): planes only -- no fp32 dx is stored; see :func:`layernorm_bwd_pos_repair`."""
    _dev(dy, x, dx)
    d = x.shape[-1]
    _check(lib().segmm_layernorm_bwd_pos(_ptr(dy), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(dx), _ptr(dx_drop),
                                         _ptr(part_dgamma), _ptr(part_dbeta), _ptr(part_dsum), x.numel() // d, d, float(drop_y_p),
                                         int(drop_y_site), float(drop_b_p), int(drop_b_site), int(seed), _ptr(amax), *_po(po),
                                         _ptr(part_pos), int(period), _stream()),
           "segmm_layernorm_bwd_pos")


def layernorm_bwd_pos_repair(dy, x, mean, rstd, gamma, period, po, drop_y_p=0.0, drop_y_site=0, seed=0):
    """The REPAIR launch of a planes-only ``layernorm_bwd_pos`` (``dx=None``), after :func:`site_fixup`: leaves at once when the
    site's planes are usable (hdr[2] == 0), else rewrites the planes -- and nothing else -- with the exact scale in hdr[0]."""
    _dev(dy, x)
    d = x.shape[-1]
    _check(lib().segmm_layernorm_bwd_pos_repair(_ptr(dy), _ptr(x), _ptr(mean), _ptr(rstd), _ptr(gamma), None, None, None, None, None,
                                                x.numel() // d, d, float(drop_y_p), int(drop_y_site), 0.0, 0, int(seed), None, *_po(po),
                                                None, int(period), _stream()),
           "segmm_layernorm_bwd_pos_repair")


def colsum_pos(part, period, out):
    """out[s, :] = sum of the rows p = s (mod period) of ``part`` [P, d]."""
    _dev(part, out)
    _check(lib().segmm_colsum_pos(_ptr(part), part.shape[0], int(period), part.shape[1], _ptr(out), _stream()), "segmm_colsum_pos")


def colsum_chunks(M):
    return lib().segmm_colsum_chunks(M)


def colsum(X, ld, M, N, out, workspace, w=None, accumulate=False, x_off=0, out_off=0):
    _dev(X, out, workspace)
    _check(lib().segmm_colsum(X.data_ptr() + 4 * x_off, ld, _ptr(w), M, N, out.data_ptr() + 4 * out_off,
                              int(bool(accumulate)), _ptr(workspace), _stream()), "segmm_colsum")


class AttnPlanes(C.Structure):
    """segmm_attn_planes_t"""
    _fields_ = [(n, _CTYPE[c]) for n, c in _abi.ATTN_PLANES_FIELDS]


ATTN_PLANES_ONLY, ATTN_REPAIR = _K["SEGMM_ATTN_PLANES_ONLY"], _K["SEGMM_ATTN_REPAIR"]


def site_fixup(*hdrs, stats=None):
    """Between planes-only producers and their repair launches: judge each site (hdr[2] = needs repair, hdr[0] = the exact
    scale to repair with); ``stats[0]`` counts the repaired sites."""
    h = [None if x is None else x.data_ptr() for x in hdrs] + [None] * 4
    _check(lib().segmm_site_fixup(h[0], h[1], h[2], h[3], _ptr(stats), _stream()), "segmm_site_fixup")


def _fill_pin(pl, pin, Qa, Qb, Ka, Va, Kb, Vb):
    """Input-plane fields of a segmm_attn_planes_t from ``pin = dict(q=(planes, hdr, ld2), a=..., b=...)`` and the (tensor,
    column offset) pairs of the fp32 views (only the offsets are used: 2 fp16 per column)."""
    def PP(side, x):
        return None if (x is None or pin.get(side) is None) else pin[side][0].data_ptr() + 4 * x[1]
    pl.qa_in, pl.qb_in = PP("q", Qa if Qa is not None else Qb), PP("q", Qb if Qb is not None else Qa)
    pl.ldq2_in, pl.hdr_q_in = pin["q"][2], pin["q"][1].data_ptr()
    if pin.get("a") is not None and Ka is not None:
        pl.ka_in, pl.va_in, pl.ldka2_in, pl.hdr_ka_in = PP("a", Ka), PP("a", Va), pin["a"][2], pin["a"][1].data_ptr()
    if pin.get("b") is not None and Kb is not None:
        pl.kb_in, pl.vb_in, pl.ldkb2_in, pl.hdr_kb_in = PP("b", Kb), PP("b", Vb), pin["b"][2], pin["b"][1].data_ptr()


def attn_fwd(B, H, dh, Lq, La, Lb, Qa, Qb, ldq, Ka, Va, ldka, Kb, Vb, ldkb, mq, mka, mkb, O, ldo, lse,
             drop_p=0.0, seed=0, site=0, amax_o=None, po=None, pin=None):
    """Q*/K*/V* are (tensor, element_offset) pairs: column slices of the fused projection buffers.  A key block may be
    empty (La == 0 or Lb == 0, its pairs None): the CrossAtt / SelfAtt ablations attend to one block only.
    ``pin`` (optional): the INPUT planes of the same slices, ``dict(q=(planes, hdr, ld2), a=(planes, hdr, ld2), b=...)`` --
    the P32 plane tensors of the buffers the query views / the key block a views / the key block b views slice (planes
    [rows, ld2] fp16) with their site headers; the planes-in forward (csrc/attention_pl.h) then runs where the shape qualifies."""
    def P(x):
        return 0 if (x is None or x[0] is None) else x[0].data_ptr() + 4 * x[1]
    prof = ATTN_PROFILE
    if prof is not None:
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
    pl = None
    if po is not None:
        a = po.args()
        pl = AttnPlanes(o=a[0], ldo2=a[1], hdr_o=a[2], sin_o=a[3])
    if pin is not None:
        pl = pl if pl is not None else AttnPlanes()
        _fill_pin(pl, pin, Qa, Qb, Ka, Va, Kb, Vb)
    if pl is not None:
        pl = C.byref(pl)
    _check(lib().segmm_attn_fwd(B, H, dh, Lq, La, Lb, P(Qa), P(Qb), ldq, P(Ka), P(Va), ldka, P(Kb), P(Vb), ldkb,
                                _ptr(mq), _ptr(mka), _ptr(mkb), _ptr(O), ldo, _ptr(lse), float(drop_p), int(seed),
                                int(site), _ptr(amax_o), pl, _stream()), "segmm_attn_fwd")
    if prof is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        prof.append(attn_record(B, H, dh, Lq, La, Lb) + (e0, e1))


def attn_bwd(B, H, dh, Lq, La, Lb, Qa, Qb, ldq, Ka, Va, ldka, Kb, Vb, ldkb, mq, mka, mkb, lse, O, ldo, dO, lddo, Dvec,
             dQa, dQb, lddq, dKa, dVa, lddka, dKb, dVb, lddkb, drop_p=0.0, seed=0, site=0, amax_q=None, amax_ka=None,
             amax_kb=None, phase=0, planes=None, pin=None):
    """``phase``: 0 whole backward; 1 Dvec only; 2 dQ only; 3 dK/dV only (2 and 3 may run concurrently after 1).
    ``pin`` (fused backward, phase >= 4): the INPUT planes of Q / K / V like attn_fwd's; the Q / K / V pairs then only name
    column offsets and their tensors may be None (a caller whose projection GEMMs write planes only): ``(None, offset)``."""
    def P(x):
        return 0 if (x is None or x[0] is None) else x[0].data_ptr() + 4 * x[1]
    if pin is not None:
        global ATTN_PIN_CALLS
        ATTN_PIN_CALLS += 1
        planes = planes if planes is not None else AttnPlanes()
        _fill_pin(planes, pin, Qa, Qb, Ka, Va, Kb, Vb)
    prof = ATTN_PROFILE
    if prof is not None:
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
    _check(lib().segmm_attn_bwd(B, H, dh, Lq, La, Lb, P(Qa), P(Qb), ldq, P(Ka), P(Va), ldka, P(Kb), P(Vb), ldkb,
                                _ptr(mq), _ptr(mka), _ptr(mkb), _ptr(lse), _ptr(O), ldo, _ptr(dO), lddo, _ptr(Dvec), P(dQa),
                                P(dQb), lddq, P(dKa), P(dVa), lddka, P(dKb), P(dVb), lddkb, float(drop_p), int(seed),
                                int(site), _ptr(amax_q), _ptr(amax_ka), _ptr(amax_kb), int(phase),
                                None if planes is None else C.byref(planes), _stream()), "segmm_attn_bwd")
    if prof is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        prof.append(attn_record(B, H, dh, Lq, La, Lb, phase, planes) + (e0, e1))


ARGSORT_MAX = 8192


def label_stats_unpack(gathered, G, B, v_all, v2_all, norms):
    """``segmm_label_stats_unpack``: G gathered records [v | v2 | norms] -> v_all, v2_all [G * B], norms summed in rank order."""
    _check(lib().segmm_label_stats_unpack(gathered.data_ptr(), int(G), int(B), v_all.data_ptr(), v2_all.data_ptr(), norms.data_ptr(), _stream()),
           "segmm_label_stats_unpack")


def argsort_ws_words(n):
    """64-bit words of workspace ``argsort_ids`` needs for ``n`` ids (0 up to ARGSORT_MAX: one workgroup sorts in LDS)."""
    if n <= ARGSORT_MAX:
        return 0
    w = 2 * ARGSORT_MAX
    while w < n:
        w <<= 1
    return w


def argsort_ids(ids, out=None, ws=None):
    """Stable argsort of int64 ids as int32 (``torch.argsort(ids, stable=True)`` is five ATen launches): one launch up to
    ARGSORT_MAX ids; beyond, the multi-workgroup bitonic network over ``ws`` (int64 tensor of ``argsort_ws_words(n)`` words;
    allocated here when not given -- a recorded step passes a persistent one)."""
    n = ids.numel()
    if out is None:
        out = torch.empty((n,), dtype=torch.int32, device=ids.device)
    if n <= ARGSORT_MAX:
        _check(lib().segmm_argsort_ids(ids.data_ptr(), int(n), out.data_ptr(), _stream()), "segmm_argsort_ids")
        return out
    need = argsort_ws_words(n)
    if ws is None:
        ws = torch.empty((need,), dtype=torch.int64, device=ids.device)
    if ws.numel() < need or ws.dtype != torch.int64:
        raise RuntimeError("argsort_ids: %d ids need %d int64 words of workspace" % (n, need))
    _check(lib().segmm_argsort_ids_ws(ids.data_ptr(), int(n), out.data_ptr(), ws.data_ptr(), _stream()), "segmm_argsort_ids_ws")
    return out


def zero_rows(table, ids):
    """table[ids, :] = 0 (2-D float32 table, int64 ids; ids outside the table are skipped), one launch."""
    ids = ids.reshape(-1)
    _check(lib().segmm_zero_rows(table.data_ptr(), int(table.shape[1]), ids.data_ptr(), int(ids.numel()), int(table.shape[0]), _stream()),
           "segmm_zero_rows")


def loss_finish(parts, B, coef, losses, total, dlogits=None, site_scale=None, gain=None, n_sites=0, gmax=None, target=7):
    """losses[12] = column sums of parts[B, 12]; total[0] = coef . losses (one launch).  With ``dlogits``: also the step's
    max |d loss / d logits| and the loss-relative delayed scales of the backward sites (segmm_loss_finish)."""
    _check(lib().segmm_loss_finish(_ptr(parts), int(B), _ptr(coef), _ptr(losses), _ptr(total), _ptr(dlogits),
                                   0 if dlogits is None else int(dlogits.numel()), _ptr(site_scale), _ptr(gain), int(n_sites), _ptr(gmax),
                                   int(target), _stream()), "segmm_loss_finish")


def rowdot(x, ld, w, bias, out, rows, d, accumulate=False, x_off=0, w_off=0):
    _check(lib().segmm_rowdot(x.data_ptr() + 4 * x_off, ld, w.data_ptr() + 4 * w_off, _ptr(bias), _ptr(out), rows, d,
                              int(bool(accumulate)), _stream()), "segmm_rowdot")


def rowscale_bcast(g, w, dx, ld, rows, d, accumulate=False, w_off=0, dx_off=0):
    _check(lib().segmm_rowscale_bcast(_ptr(g), w.data_ptr() + 4 * w_off, dx.data_ptr() + 4 * dx_off, ld, rows, d,
                                      int(bool(accumulate)), _stream()), "segmm_rowscale_bcast")


def rowdot_pair(a, lda, b, ldb, out, rows, d, accumulate=False, a_off=0, b_off=0):
    _check(lib().segmm_rowdot_pair(a.data_ptr() + 4 * a_off, lda, b.data_ptr() + 4 * b_off, ldb, _ptr(out), rows, d,
                                   int(bool(accumulate)), _stream()), "segmm_rowdot_pair")


def rowscale_mat(g, X, ldx, out, ldo, rows, d, accumulate=False):
    _check(lib().segmm_rowscale_mat(_ptr(g), _ptr(X), ldx, _ptr(out), ldo, rows, d, int(bool(accumulate)), _stream()),
           "segmm_rowscale_mat")


def vecsum(v, n, out, accumulate=False):
    _check(lib().segmm_vecsum(_ptr(v), n, _ptr(out), int(bool(accumulate)), _stream()), "segmm_vecsum")


def embed_id_vid(item_id, table, dhalf, frame_w, frame_b, pe, out, B, S, frame_pos=None):
    _check(lib().segmm_embed_id_vid(_ptr(item_id), _ptr(table), dhalf, _ptr(frame_w), _ptr(frame_b), _ptr(pe),
                                    _ptr(frame_pos), _ptr(out), B, S, table.shape[0], _stream()), "segmm_embed_id_vid")


def embed_id_usr(user_id, table, d, pe, out, B):
    _check(lib().segmm_embed_id_usr(_ptr(user_id), _ptr(table), d, _ptr(pe), _ptr(out), B, table.shape[0], _stream()),
           "segmm_embed_id_usr")


def embed_id_bwd(dpre, tokens_per_row, ld, col0, width, order, ids, dtable, B):
    _check(lib().segmm_embed_id_bwd(_ptr(dpre), tokens_per_row, ld, col0, width, _ptr(order), _ptr(ids), _ptr(dtable),
                                    B, dtable.shape[0], _stream()), "segmm_embed_id_bwd")


def pe_grad(dpre, ld, B, S, d, dpe, accumulate=False):
    _check(lib().segmm_pe_grad(_ptr(dpre), ld, B, S, d, _ptr(dpe), int(bool(accumulate)), _stream()), "segmm_pe_grad")


def label_stats(gt, B, S, rewritten, v, v2, norms):
    _check(lib().segmm_label_stats(_ptr(gt), B, S, int(rewritten), _ptr(v), _ptr(v2), _ptr(norms), _stream()),
           "segmm_label_stats")


def loss_fwd_bwd(B, S, logits, gt, bias_w, bias_b, exposure, coef, enabled, rew_ce, rew_kl, use_mask, norms, v_all,
                 v2_all, Bg, logits_out, dlogits, parts):
    coef_a = (C.c_float * 9)(*[float(c) for c in coef])
    en_a = (C.c_int * 9)(*[int(e) for e in enabled])
    _check(lib().segmm_loss_fwd_bwd(B, S, _ptr(logits), _ptr(gt), _ptr(bias_w), _ptr(bias_b), _ptr(exposure),
                                    C.cast(coef_a, C.c_void_p), C.cast(en_a, C.c_void_p), int(rew_ce), int(rew_kl),
                                    int(use_mask), _ptr(norms), _ptr(v_all), _ptr(v2_all), Bg, _ptr(logits_out),
                                    _ptr(dlogits), _ptr(parts), _stream()), "segmm_loss_fwd_bwd")


def adamw(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, p_off=0, coef=None, guard=False):
    """segmm_adamw over [p_off, p_off + n) of the flat buffers; ``coef``: a device float the gradient is multiplied by first
    (segmm_adamw_scaled, the clip coefficient of :func:`grad_norm`).  ``guard``: segmm_adamw_guarded (step = -1), with or without
    ``coef``: nothing is read or written in a step the non-finite guard skipped."""
    with _kprof("adamw", 28 * int(n)):
        if guard:
            _check(lib().segmm_adamw_guarded(p.data_ptr() + 4 * p_off, g.data_ptr() + 4 * p_off, m.data_ptr() + 4 * p_off, v.data_ptr() + 4 * p_off, n,
                                             lr, beta1, beta2, eps, weight_decay, step, _ptr(coef), _stream()), "segmm_adamw_guarded")
        else:
            _adamw(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, p_off, coef)


def adamw_table(p, g, m, v, off, n_rows, width, ids, flags, lr, beta1, beta2, eps, weight_decay, step, phase, coef=None):
    """segmm_adamw_table on the table that starts ``off`` floats into the flat buffers (phase 0: rows without a gradient, g = 0;
    phase 1: the rows listed in ``ids``, their gradient multiplied by the device float ``coef`` first when one is given)."""
    with _kprof("adamw", (24 if phase == 0 else 28) * int(n_rows if phase == 0 else ids.numel()) * int(width)):
        args = (p.data_ptr() + 4 * off, None if g is None else g.data_ptr() + 4 * off, m.data_ptr() + 4 * off, v.data_ptr() + 4 * off,
                int(n_rows), int(width), ids.data_ptr(), ids.numel(), flags.data_ptr(), float(lr), float(beta1), float(beta2), float(eps),
                float(weight_decay), int(step))
        if coef is None:
            _check(lib().segmm_adamw_table(*args, int(phase), _stream()), "segmm_adamw_table")
        else:
            if phase != 1:
                raise RuntimeError("adamw_table: a scaled update is phase 1 only (phase 0 has g = 0)")
            _check(lib().segmm_adamw_table_scaled(*args, coef.data_ptr(), _stream()), "segmm_adamw_table_scaled")


def _adamw(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, p_off=0, coef=None):
    args = (p.data_ptr() + 4 * p_off, g.data_ptr() + 4 * p_off, m.data_ptr() + 4 * p_off, v.data_ptr() + 4 * p_off, n, lr, beta1, beta2,
            eps, weight_decay, step)
    if coef is None:
        _check(lib().segmm_adamw(*args, _stream()), "segmm_adamw")
    else:
        _check(lib().segmm_adamw_scaled(*args, coef.data_ptr(), _stream()), "segmm_adamw_scaled")


def _segs(segs):
    """The segment table of a grouped optimizer, (ends int64, lr_scale float32, weight_decay float32, frozen uint8): equally long,
    contiguous device tensors -> their pointers and the segment count.  ``frozen`` may be None: no segment is frozen."""
    ends, scale, wd, frozen = segs
    n_seg = ends.numel()
    given = [t for t in segs if t is not None]
    if (ends.dtype, scale.dtype, wd.dtype) != (torch.int64, torch.float32, torch.float32) or (frozen is not None and frozen.dtype != torch.uint8) \
            or n_seg < 1 or not all(t.numel() == n_seg and t.is_contiguous() for t in given):
        raise RuntimeError("segment table: int64 ends, float32 lr_scale, float32 weight_decay, uint8 frozen (or None), one entry per segment")
    _dev(*given)
    return ends.data_ptr(), scale.data_ptr(), wd.data_ptr(), _ptr(frozen), n_seg


def adamw_groups(p, g, m, v, start, n, segs, lr, beta1, beta2, eps, step, coef=None, guard=False):
    """segmm_adamw_groups over [start, start + n) of the flat buffers, ``segs`` = (ends, lr_scale, weight_decay, frozen) the
    segment table (:func:`_segs`; ends counted from the buffers' first element); ``coef`` and ``guard`` (segmm_adamw_groups_guarded)
    as in :func:`adamw`."""
    start, n = int(start), int(n)
    if start < 0 or start % 4 or n < 0 or start + n > min(p.numel(), g.numel(), m.numel(), v.numel()):
        raise RuntimeError("adamw_groups: range [%d, %d) (start a multiple of 4) outside buffers of %d / %d / %d / %d elements"
                           % (start, start + n, p.numel(), g.numel(), m.numel(), v.numel()))
    e, s, w, f, n_seg = _segs(segs)
    with _kprof("adamw", 28 * n):
        fn = "segmm_adamw_groups_guarded" if guard else "segmm_adamw_groups"
        _check(getattr(lib(), fn)(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), start, n, e, s, w, f, n_seg, float(lr), float(beta1),
                                  float(beta2), float(eps), int(step), _ptr(coef), _stream()), fn)


def adamw_table_lrs(p, g, m, v, off, n_rows, width, ids, flags, lr, lr_scale, beta1, beta2, eps, weight_decay, step, phase, coef=None, guard=False):
    """segmm_adamw_table_lrs: :func:`adamw_table` at the rate fp32(lr * lr_scale).  ``guard``: segmm_adamw_table_lrs_guarded (step = -1)."""
    with _kprof("adamw", (24 if phase == 0 else 28) * int(n_rows if phase == 0 else ids.numel()) * int(width)):
        fn = "segmm_adamw_table_lrs_guarded" if guard else "segmm_adamw_table_lrs"
        _check(getattr(lib(), fn)(p.data_ptr() + 4 * off, None if g is None else g.data_ptr() + 4 * off, m.data_ptr() + 4 * off,
                                  v.data_ptr() + 4 * off, int(n_rows), int(width), ids.data_ptr(), ids.numel(), flags.data_ptr(), float(lr),
                                  float(lr_scale), float(beta1), float(beta2), float(eps), float(weight_decay), int(step), int(phase),
                                  _ptr(coef), _stream()), fn)


# ---- lazy exact AdamW of an id table (include/segmm_hip.h "Lazy exact AdamW"): stamps int32 [n_rows], hist float32 [cap, 4]
def _lazy_state(stamps, hist, n_rows):
    if stamps.dtype != torch.int32 or not stamps.is_contiguous() or stamps.numel() != int(n_rows):
        raise RuntimeError("lazy table: stamps must be %d contiguous int32 (got %s x %d)" % (n_rows, stamps.dtype, stamps.numel()))
    if hist is not None and (hist.dtype != torch.float32 or not hist.is_contiguous() or hist.dim() != 2 or hist.shape[1] != 4 or hist.shape[0] < 1):
        raise RuntimeError("lazy table: the history ring must be contiguous float32 [cap, 4]")
    _dev(stamps, hist)


def adamw_hist_push(hist, lr, beta1, beta2, step):
    """segmm_adamw_hist_push: the entry of ``step`` (>= 1, or -1: the bound device step state's count, with ``lr`` = LIVE_LR its rate
    too) into slot step % cap of the ring ``hist`` (float32 [cap, 4])."""
    if hist.dtype != torch.float32 or not hist.is_contiguous() or hist.dim() != 2 or hist.shape[1] != 4:
        raise RuntimeError("adamw_hist_push: the history ring must be contiguous float32 [cap, 4]")
    _dev(hist)
    _check(lib().segmm_adamw_hist_push(hist.data_ptr(), hist.shape[0], float(lr), float(beta1), float(beta2), int(step), _stream()),
           "segmm_adamw_hist_push")


def adamw_table_catchup(p, m, v, off, n_rows, width, ids, stamps, hist, target, lr_scale, beta1, beta2, eps, weight_decay, relative=False,
                        flags=None):
    """segmm_adamw_table_catchup on the table that starts ``off`` floats into the flat buffers: the rows listed in ``ids`` (None: every
    row, the flush) replay their missed g = 0 steps up to ``target`` (``relative``: the bound device step count plus ``target``, 0 or
    -1); ``flags``: the listed rows are marked for the phase 1 that follows."""
    n_rows, width = int(n_rows), int(width)
    _lazy_state(stamps, hist, n_rows)
    if off < 0 or off + n_rows * width > min(p.numel(), m.numel(), v.numel()):
        raise RuntimeError("adamw_table_catchup: a table of %d x %d at float %d does not fit buffers of %d / %d / %d elements"
                           % (n_rows, width, off, p.numel(), m.numel(), v.numel()))
    if flags is not None and (ids is None or flags.numel() != n_rows or flags.dtype != torch.int32):
        raise RuntimeError("adamw_table_catchup: flags are %d int32 and go with an id list" % n_rows)
    if ids is not None and (ids.dtype != torch.int64 or not ids.is_contiguous()):
        raise RuntimeError("adamw_table_catchup: ids must be contiguous int64")
    if ids is not None and ids.numel() == 0:          # an empty list (torch hands out a null pointer for it, the C ABI's flush) lists nothing
        return
    _check(lib().segmm_adamw_table_catchup(p.data_ptr() + 4 * off, m.data_ptr() + 4 * off, v.data_ptr() + 4 * off, n_rows, width, _ptr(ids),
                                           0 if ids is None else ids.numel(), stamps.data_ptr(), _ptr(flags), hist.data_ptr(), hist.shape[0],
                                           int(target), int(bool(relative)), float(lr_scale), float(beta1), float(beta2), float(eps),
                                           float(weight_decay), _stream()), "segmm_adamw_table_catchup")


def adamw_table_stamp(ids, n_rows, stamps, target, relative=False):
    """segmm_adamw_table_stamp: the listed rows' stamps become at least ``target``; ``ids`` None: every stamp is set to it."""
    _lazy_state(stamps, None, n_rows)
    if ids is not None and (ids.dtype != torch.int64 or not ids.is_contiguous()):
        raise RuntimeError("adamw_table_stamp: ids must be contiguous int64")
    if ids is not None and ids.numel() == 0:          # (a null pointer in the C ABI means every row)
        return
    _check(lib().segmm_adamw_table_stamp(_ptr(ids), 0 if ids is None else ids.numel(), int(n_rows), stamps.data_ptr(), int(target),
                                         int(bool(relative)), _stream()), "segmm_adamw_table_stamp")


def adamw_table_lazy_rows(p, g, m, v, off, n_rows, width, ids, stamps, hist, lr, lr_scale, beta1, beta2, eps, weight_decay, step, coef=None):
    """segmm_adamw_table_lazy_rows on the table that starts ``off`` floats into the flat buffers: every row listed in ``ids`` (all
    ranks' ids of a data-parallel step) whose stamp is below T = ``step`` (>= 1, or -1: the bound device step state's count) replays
    its missed g = 0 steps up to T - 1 from the ring, takes step T with its row of ``g`` (times ``coef[0]``) and is stamped T."""
    n_rows, width = int(n_rows), int(width)
    _lazy_state(stamps, hist, n_rows)
    if hist is None:
        raise RuntimeError("adamw_table_lazy_rows: needs the history ring")
    if off < 0 or off + n_rows * width > min(p.numel(), g.numel(), m.numel(), v.numel()):
        raise RuntimeError("adamw_table_lazy_rows: a table of %d x %d at float %d does not fit buffers of %d / %d / %d / %d elements"
                           % (n_rows, width, off, p.numel(), g.numel(), m.numel(), v.numel()))
    if ids is None or ids.dtype != torch.int64 or not ids.is_contiguous():
        raise RuntimeError("adamw_table_lazy_rows: ids must be contiguous int64 (the gathered list of the step)")
    _dev(p, g, m, v, ids, coef)
    if ids.numel() == 0:
        return
    _check(lib().segmm_adamw_table_lazy_rows(p.data_ptr() + 4 * off, g.data_ptr() + 4 * off, m.data_ptr() + 4 * off, v.data_ptr() + 4 * off,
                                             n_rows, width, ids.data_ptr(), ids.numel(), stamps.data_ptr(), hist.data_ptr(), hist.shape[0],
                                             float(lr), float(lr_scale), float(beta1), float(beta2), float(eps), float(weight_decay), int(step),
                                             _ptr(coef), _stream()), "segmm_adamw_table_lazy_rows")


# ---- the same with the EMA shadow of the table replayed beside the rows (include/segmm_hip.h): ``shadow`` is the flat shadow tensor,
# the table's shadow rows start ``shadow_off`` floats into it
def adamw_hist_push_ema(hist, lr, beta1, beta2, step, ema_weight, ema_warmup):
    """segmm_adamw_hist_push_ema: :func:`adamw_hist_push`, and the entry's fourth float is the w of
    ``ema_update(weight=ema_weight, warmup=ema_warmup, step=step)``."""
    if hist.dtype != torch.float32 or not hist.is_contiguous() or hist.dim() != 2 or hist.shape[1] != 4:
        raise RuntimeError("adamw_hist_push_ema: the history ring must be contiguous float32 [cap, 4]")
    _dev(hist)
    _check(lib().segmm_adamw_hist_push_ema(hist.data_ptr(), hist.shape[0], float(lr), float(beta1), float(beta2), int(step), float(ema_weight),
                                           int(bool(ema_warmup)), _stream()), "segmm_adamw_hist_push_ema")


def _lazy_shadow(who, shadow, shadow_off, n_rows, width):
    _f32c(shadow, who + ": shadow")
    _dev(shadow)
    if shadow_off < 0 or shadow_off + n_rows * width > shadow.numel():
        raise RuntimeError("%s: the shadow of a table of %d x %d at float %d does not fit a tensor of %d elements"
                           % (who, n_rows, width, shadow_off, shadow.numel()))


def adamw_table_catchup_ema(p, m, v, shadow, off, shadow_off, n_rows, width, ids, stamps, hist, target, lr_scale, beta1, beta2, eps, weight_decay,
                            relative=False):
    """segmm_adamw_table_catchup_ema: :func:`adamw_table_catchup` (no flags) whose replay also averages the rows' shadow, step by
    step, with the weights the ring holds."""
    n_rows, width = int(n_rows), int(width)
    _lazy_state(stamps, hist, n_rows)
    if hist is None:
        raise RuntimeError("adamw_table_catchup_ema: needs the history ring")
    if off < 0 or off + n_rows * width > min(p.numel(), m.numel(), v.numel()):
        raise RuntimeError("adamw_table_catchup_ema: a table of %d x %d at float %d does not fit buffers of %d / %d / %d elements"
                           % (n_rows, width, off, p.numel(), m.numel(), v.numel()))
    _lazy_shadow("adamw_table_catchup_ema", shadow, shadow_off, n_rows, width)
    if ids is not None and (ids.dtype != torch.int64 or not ids.is_contiguous()):
        raise RuntimeError("adamw_table_catchup_ema: ids must be contiguous int64")
    _dev(p, m, v, ids)
    if ids is not None and ids.numel() == 0:          # an empty list (torch hands out a null pointer for it, the C ABI's flush) lists nothing
        return
    _check(lib().segmm_adamw_table_catchup_ema(p.data_ptr() + 4 * off, m.data_ptr() + 4 * off, v.data_ptr() + 4 * off,
                                               shadow.data_ptr() + 4 * shadow_off, n_rows, width, _ptr(ids), 0 if ids is None else ids.numel(),
                                               stamps.data_ptr(), hist.data_ptr(), hist.shape[0], int(target), int(bool(relative)), float(lr_scale),
                                               float(beta1), float(beta2), float(eps), float(weight_decay), _stream()),
           "segmm_adamw_table_catchup_ema")


def adamw_table_lazy_rows_ema(p, g, m, v, shadow, off, shadow_off, n_rows, width, ids, stamps, hist, lr, lr_scale, beta1, beta2, eps, weight_decay,
                              step, coef=None):
    """segmm_adamw_table_lazy_rows_ema: :func:`adamw_table_lazy_rows` that also averages the rows' shadow -- through the replayed
    steps and, with the weight :func:`adamw_hist_push_ema` has just written for it, through step T."""
    n_rows, width = int(n_rows), int(width)
    _lazy_state(stamps, hist, n_rows)
    if hist is None:
        raise RuntimeError("adamw_table_lazy_rows_ema: needs the history ring")
    if off < 0 or off + n_rows * width > min(p.numel(), g.numel(), m.numel(), v.numel()):
        raise RuntimeError("adamw_table_lazy_rows_ema: a table of %d x %d at float %d does not fit buffers of %d / %d / %d / %d elements"
                           % (n_rows, width, off, p.numel(), g.numel(), m.numel(), v.numel()))
    _lazy_shadow("adamw_table_lazy_rows_ema", shadow, shadow_off, n_rows, width)
    if ids is None or ids.dtype != torch.int64 or not ids.is_contiguous():
        raise RuntimeError("adamw_table_lazy_rows_ema: ids must be contiguous int64 (the id list of the step)")
    _dev(p, g, m, v, ids, coef)
    if ids.numel() == 0:
        return
    _check(lib().segmm_adamw_table_lazy_rows_ema(p.data_ptr() + 4 * off, g.data_ptr() + 4 * off, m.data_ptr() + 4 * off, v.data_ptr() + 4 * off,
                                                 shadow.data_ptr() + 4 * shadow_off, n_rows, width, ids.data_ptr(), ids.numel(), stamps.data_ptr(),
                                                 hist.data_ptr(), hist.shape[0], float(lr), float(lr_scale), float(beta1), float(beta2), float(eps),
                                                 float(weight_decay), int(step), _ptr(coef), _stream()), "segmm_adamw_table_lazy_rows_ema")


GRAD_NORM_SCRATCH = 1024         # fp64 partials segmm_grad_norm may write


def grad_norm_groups(g, n, segs, max_norm, scratch, out2):
    """segmm_grad_norm_groups: :func:`grad_norm` over g[0, n) without the elements of the frozen segments of ``segs``."""
    if scratch.dtype != torch.float64 or scratch.numel() < GRAD_NORM_SCRATCH or out2.dtype != torch.float32 or out2.numel() < 2:
        raise RuntimeError("grad_norm_groups: scratch must be %d float64, out2 two float32" % GRAD_NORM_SCRATCH)
    if n < 0 or n > g.numel():
        raise RuntimeError("grad_norm_groups: %d elements of a tensor of %d" % (n, g.numel()))
    e, _, _, f, n_seg = _segs(segs)
    if f is None:
        raise RuntimeError("grad_norm_groups: no frozen flags (without a frozen segment call grad_norm)")
    with _kprof("grad_norm", 4 * int(n)):
        _check(lib().segmm_grad_norm_groups(g.data_ptr(), int(n), e, f, n_seg, float(max_norm), scratch.data_ptr(), out2.data_ptr(), _stream()),
               "segmm_grad_norm_groups")


def grad_norm(g, n, max_norm, scratch, out2, off=0):
    """segmm_grad_norm over g[off, off + n): out2 (two device floats) = {2-norm, clip coefficient for ``max_norm``};
    ``scratch``: GRAD_NORM_SCRATCH float64 on the device."""
    if scratch.dtype != torch.float64 or scratch.numel() < GRAD_NORM_SCRATCH or out2.dtype != torch.float32 or out2.numel() < 2:
        raise RuntimeError("grad_norm: scratch must be %d float64, out2 two float32" % GRAD_NORM_SCRATCH)
    if off < 0 or n < 0 or off + n > g.numel():
        raise RuntimeError("grad_norm: range [%d, %d) outside a tensor of %d elements" % (off, off + n, g.numel()))
    with _kprof("grad_norm", 4 * int(n)):
        _check(lib().segmm_grad_norm(g.data_ptr() + 4 * off, int(n), float(max_norm), scratch.data_ptr(), out2.data_ptr(), _stream()),
               "segmm_grad_norm")


def bias_grad(dl, B, S, gbw, gbb):
    _check(lib().segmm_bias_grad(_ptr(dl), int(B), int(S), _ptr(gbw), _ptr(gbb), _stream()), "segmm_bias_grad")


def focal_relabel(gt):
    _check(lib().segmm_focal_relabel(_ptr(gt), gt.numel(), _stream()), "segmm_focal_relabel")


def rand_uniform(out, seed, site):
    _check(lib().segmm_rand_uniform(_ptr(out), out.numel(), int(seed), int(site), _stream()), "segmm_rand_uniform")


def rand_ids(out, lo, hi, seed, site):
    _check(lib().segmm_rand_ids(_ptr(out), out.numel(), int(lo), int(hi), int(seed), int(site), _stream()), "segmm_rand_ids")


def rand_perm_rows(out, rows, S, seed, site):
    _check(lib().segmm_rand_perm_rows(_ptr(out), int(rows), int(S), int(seed), int(site), _stream()), "segmm_rand_perm_rows")


def dropout_mult(out, n, p, seed, site):
    _check(lib().segmm_dropout_mult(_ptr(out), n, float(p), int(seed), int(site), _stream()), "segmm_dropout_mult")


# ------------------------------------------------------------------ evaluation, gather, SegRec head
def rank_leave(x, gt, perm=None, masked=False, seq_valid=None):
    """(ranks int32 [B], hist int32 [S+1]) of the leave segment; see segmm_rank_leave in include/segmm_hip.h."""
    _dev(x, gt)
    B, S = gt.shape
    if x.dtype != torch.float32 or x.stride(-1) != 1 or gt.dtype != torch.int64 or not gt.is_contiguous():
        raise RuntimeError("rank_leave: x float32 with unit inner stride, gt contiguous int64")
    if perm is not None and (perm.dtype != torch.int32 or not perm.is_contiguous() or perm.shape != gt.shape):
        raise RuntimeError("rank_leave: perm must be a contiguous int32 [B, S] tensor")
    ranks = torch.empty(B, dtype=torch.int32, device=x.device)
    hist = torch.zeros(S + 1, dtype=torch.int32, device=x.device)
    _check(lib().segmm_rank_leave(_ptr(x), x.stride(0), _ptr(gt), _ptr(perm), B, S, int(bool(masked)),
                                  S if seq_valid is None else int(seq_valid), _ptr(ranks), _ptr(hist), _stream()), "segmm_rank_leave")
    return ranks, hist


SEED_MASK = (1 << 63) - 1          # the seed bits below LIVE_SEED


def valid_rows(logits, exposure, gt, ranks=None, masked=False, seq_valid=None, permute=False, seed=0, site=0, row0=0,
               interests=None, perm_out=None):
    """The tail of a validation batch in one launch (segmm_valid_rows in include/segmm_hip.h): ranks int32 [B] of the leave segment
    under interests = sigmoid(logits) * exposure, the candidates shuffled (``permute``) by a permutation drawn in the kernel for
    (seed, site, row0 + b).  ``ranks`` (written in place: a slice of a pass's table) or a fresh tensor is returned; ``interests``
    float32 [B, S] / ``perm_out`` int32 [B, S]: optional outputs (tests)."""
    _dev(logits, exposure, gt)
    if gt.dim() != 2 or gt.dtype != torch.int64 or not gt.is_contiguous():
        raise RuntimeError("valid_rows: gt must be a contiguous int64 [B, S] tensor")
    B, S = gt.shape
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.shape != gt.shape or (S > 1 and logits.stride(1) != 1):
        raise RuntimeError("valid_rows: logits must be float32 [B, S] with unit inner stride")
    if exposure is not None and (exposure.dtype != torch.float32 or not exposure.is_contiguous() or exposure.numel() < S):
        raise RuntimeError("valid_rows: exposure must be a contiguous float32 tensor of at least S elements")
    if ranks is None:
        ranks = torch.empty(B, dtype=torch.int32, device=gt.device)
    if ranks.dtype != torch.int32 or not ranks.is_contiguous() or ranks.numel() != B:
        raise RuntimeError("valid_rows: ranks must be a contiguous int32 [B] tensor")
    for t, dt, nm in ((interests, torch.float32, "interests"), (perm_out, torch.int32, "perm_out")):
        if t is not None and (t.dtype != dt or not t.is_contiguous() or t.shape != gt.shape):
            raise RuntimeError("valid_rows: %s must be a contiguous %s [B, S] tensor" % (nm, str(dt).replace("torch.", "")))
    if B == 0:          # (an empty tensor has no address to pass)
        return ranks
    _check(lib().segmm_valid_rows(_ptr(logits), logits.stride(0) if B > 1 else max(logits.stride(0), S), _ptr(exposure), _ptr(gt), B, S,
                                  int(bool(masked)), S if seq_valid is None else int(seq_valid), int(bool(permute)), int(seed) & SEED_MASK,
                                  int(site), int(row0), _ptr(ranks), _ptr(interests), _ptr(perm_out), _stream()), "segmm_valid_rows")
    return ranks


def auc_counts(score, label, seg_off):
    """int64 [n_seg, 3] = (U2, npos, nneg) per segment; label int8 (1 / 0 / other = ignored)."""
    _dev(score, label, seg_off)
    if score.dtype != torch.float32 or label.dtype != torch.int8 or seg_off.dtype != torch.int64:
        raise RuntimeError("auc_counts: score float32, label int8, seg_off int64")
    n_seg = seg_off.numel() - 1
    out = torch.zeros((max(n_seg, 0), 3), dtype=torch.int64, device=score.device)
    _check(lib().segmm_auc_counts(_ptr(score.contiguous()), _ptr(label.contiguous()), _ptr(seg_off.contiguous()), n_seg, _ptr(out),
                                  _stream()), "segmm_auc_counts")
    return out


def survival(interest, gt):
    """(surv float32 [B, S], label int8 [B, S]) for ProbAUC."""
    _dev(interest, gt)
    B, S = gt.shape
    surv = torch.empty((B, S), dtype=torch.float32, device=interest.device)
    label = torch.empty((B, S), dtype=torch.int8, device=interest.device)
    _check(lib().segmm_survival(_ptr(interest), interest.stride(0), _ptr(gt.contiguous()), _ptr(surv), _ptr(label), B, S, _stream()),
           "segmm_survival")
    return surv, label


ROW_METRIC_INT_FIELDS = ("view_length", "duration", "top1", "group")
ROW_METRIC_FLOAT_FIELDS = ("jaccard", "pred_view_length", "leave_ctr", "leave_ctr_view")
ROW_METRIC_SUMS = ("n", "jaccard", "pred", "sq_err", "abs_err", "leave_ctr", "leave_ctr_view", "top1_sq_err", "top1_abs_err", "n_complete")


def row_metrics(interest, gt, photo_id=None, seen=None):
    """(irec int32 [4, B], frec float32 [4, B]): the per-row records of the test phase; see segmm_row_metrics in include/segmm_hip.h."""
    _dev(interest, gt)
    B, S = gt.shape
    if interest.dtype != torch.float32 or interest.stride(-1) != 1 or gt.dtype != torch.int64 or not gt.is_contiguous():
        raise RuntimeError("row_metrics: interest float32 with unit inner stride, gt contiguous int64")
    if (photo_id is None) != (seen is None):
        raise RuntimeError("row_metrics: photo_id and seen go together")
    if seen is not None:
        _dev(photo_id, seen)
        if photo_id.dtype != torch.int64 or not photo_id.is_contiguous() or photo_id.numel() != B or seen.dtype != torch.uint8 or not seen.is_contiguous():
            raise RuntimeError("row_metrics: photo_id contiguous int64 [B], seen contiguous uint8")
    irec = torch.empty((len(ROW_METRIC_INT_FIELDS), B), dtype=torch.int32, device=interest.device)
    frec = torch.empty((len(ROW_METRIC_FLOAT_FIELDS), B), dtype=torch.float32, device=interest.device)
    _check(lib().segmm_row_metrics(_ptr(interest), interest.stride(0), _ptr(gt), _ptr(photo_id),
                                   _ptr(seen), 0 if seen is None else seen.numel(), B, S, _ptr(irec), _ptr(frec), _stream()),
           "segmm_row_metrics")
    return irec, frec


def row_metrics_accumulate(irec, frec, acc, S):
    """acc float64 [3, 10] (all / cold / hot rows) += the sums of the records; see segmm_row_metrics_accumulate."""
    _dev(irec, frec, acc)
    B = irec.shape[1]
    if (irec.dtype != torch.int32 or frec.dtype != torch.float32 or not irec.is_contiguous() or not frec.is_contiguous() or frec.shape[1] != B
            or acc.dtype != torch.float64 or not acc.is_contiguous() or tuple(acc.shape) != (3, len(ROW_METRIC_SUMS))):
        raise RuntimeError("row_metrics_accumulate: irec int32 [4, B], frec float32 [4, B], acc contiguous float64 [3, 10]")
    _check(lib().segmm_row_metrics_accumulate(_ptr(irec), _ptr(frec), B, int(S), _ptr(acc), _stream()), "segmm_row_metrics_accumulate")


def gather_l1(table, idx, normalize=True, out=None, mask=None, amax=None, po=None):
    """out[..., :] = (L1-normalised) table[idx[...]], mask[...] = idx in range; idx int64 of any shape.  ``table``: float32, or
    float16 / bfloat16, or float8_e4m3fn / float8_e5m2 / int8 (widened exactly in the kernel: the float32 result on the widened table,
    bit for bit); ``out``: float32."""
    _dev(table, idx)
    elem = _feat(table, "gather_l1: table")
    if table.dim() != 2:
        raise RuntimeError("gather_l1: table must be [n_lines, D] (got %s)" % (tuple(table.shape),))
    if out is not None and out.dtype != torch.float32:
        raise RuntimeError("gather_l1: out must be float32 whatever the table is (got %s)" % out.dtype)
    D = table.shape[1]
    rows = idx.numel()
    if out is None:
        out = torch.empty(tuple(idx.shape) + (D,), dtype=torch.float32, device=table.device)
    if mask is None:
        mask = torch.empty(tuple(idx.shape), dtype=torch.uint8, device=table.device)
    if elem is None:
        with _kprof("gather_l1", rows * (8 * D + 9)):
            _check(lib().segmm_gather_l1(_ptr(table), table.shape[0], D, _ptr(idx.contiguous()), rows, int(bool(normalize)),
                                         _ptr(out), _ptr(mask), _ptr(amax), *_po(po), _stream()), "segmm_gather_l1")
    elif table.dtype in _ELEM:          # a 16-bit table: 2 D bytes read, 4 D written per row
        with _kprof("gather_l1", rows * (6 * D + 9)):
            _check(lib().segmm_gather_l1_h(_ptr(table), elem, table.shape[0], D, _ptr(idx.contiguous()), rows, int(bool(normalize)),
                                           _ptr(out), _ptr(mask), _ptr(amax), *_po(po), _stream()), "segmm_gather_l1_h")
    else:          # an 8-bit table: D bytes read, 4 D written per row
        with _kprof("gather_l1", rows * (5 * D + 9)):
            _check(lib().segmm_gather_l1_b(_ptr(table), elem, table.shape[0], D, _ptr(idx.contiguous()), rows, int(bool(normalize)),
                                           _ptr(out), _ptr(mask), _ptr(amax), *_po(po), _stream()), "segmm_gather_l1_b")
    return out, mask.view(torch.bool)


class ITable(C.Structure):
    """segmm_itable_t: the compiled interaction table as device pointers + counts (feature_store.InteractionTable.descriptor)"""
    _fields_ = [(n, _CTYPE[c]) for n, c in _abi.STRUCT_FIELDS["segmm_itable_t"]]


ASSEMBLE_MAX_CAND = _K["SEGMM_ASSEMBLE_MAX_CAND"]          # candidates (video frames / user list) a row may have, and the largest Lt
ASSEMBLE_COLS = ("photo_id", "photo_identity_id", "user_id", "user_identity_id", "time_ms", "play_time", "duration")


def assemble_rows(desc: "ITable", row_ids, S, Lt, seed, site):
    """``segmm_assemble_rows``: row_ids int64 [B] (device) -> photo_idx [B, S], user_idx [B, Lt] (-1 = padding), label [B, S] and
    the seven scalar columns as cols [7, B] (ASSEMBLE_COLS order), all int64, fresh tensors.  ``desc``: the table's descriptor,
    whose tensors the caller keeps alive."""
    _dev(row_ids)
    if row_ids.dtype != torch.int64 or row_ids.dim() != 1 or not row_ids.is_contiguous():
        raise RuntimeError("assemble_rows: row_ids must be a contiguous int64 vector")
    B, dev = row_ids.numel(), row_ids.device
    photo = torch.empty((B, int(S)), dtype=torch.int64, device=dev)
    user = torch.empty((B, int(Lt)), dtype=torch.int64, device=dev)
    label = torch.empty((B, int(S)), dtype=torch.int64, device=dev)
    cols = torch.empty((len(ASSEMBLE_COLS), B), dtype=torch.int64, device=dev)
    _check(lib().segmm_assemble_rows(C.addressof(desc), row_ids.data_ptr(), B, int(S), int(Lt), int(seed), int(site), photo.data_ptr(),
                                     user.data_ptr(), label.data_ptr(), cols.data_ptr(), _stream()), "segmm_assemble_rows")
    return photo, user, label, cols


def segment_weighted_sum(pred, weight=None, duration=None):
    """sum_seg pred * weight * (seg < duration) over the last axis."""
    _dev(pred)
    S = pred.shape[-1]
    rows = pred.numel() // S
    out = torch.empty(pred.shape[:-1], dtype=torch.float32, device=pred.device)
    _check(lib().segmm_segment_weighted_sum(_ptr(_f32c(pred, "pred")), _ptr(None if weight is None else _f32c(weight, "weight")),
                                            _ptr(None if duration is None else duration.contiguous()), rows, S, _ptr(out), _stream()),
           "segmm_segment_weighted_sum")
    return out


STORE_MISS_NONE = (1 << 63) - 1          # what both slots of store_lookup's ``miss`` hold when nothing was missed


def _i64c(t, name, shape=None):
    if t.dtype != torch.int64 or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise RuntimeError("%s must be contiguous int64%s (got %s %s, contiguous=%s)"
                           % (name, "" if shape is None else " " + str(list(shape)), t.dtype, list(t.shape), t.is_contiguous()))
    return t


def _store_index(keys, rows, name):
    """(keys, rows, n) of one index of ``segmm_store_lookup`` after the argument checks; ``(None, None, n)`` for an empty one."""
    _dev(keys, rows)
    n = keys.shape[0]
    _i64c(keys, name + " keys", (n, 3))
    if rows.dtype != torch.int32 or not rows.is_contiguous() or tuple(rows.shape) != (n,):
        raise RuntimeError("%s rows must be contiguous int32 [%d]" % (name, n))
    return (keys, rows, n) if n else (None, None, 0)


def store_lookup(user, item, time, keys, rows, neg_keys=None, neg_rows=None, user_map=None, item_map=None, miss=None):
    """``segmm_store_lookup``: user [B], item [B, I] (column 0 = the target), time [B] (device int64) against the target index
    (keys int64 [n, 3], rows int32 [n]) and, when given, the negatives index and the dense id maps -> (rowidx int32 [B, I], miss
    int64 [2]).  miss[0] / miss[1]: the first flat index b * I + j whose negatives key / whose id was missing, STORE_MISS_NONE when
    none was.  Never synchronises."""
    _dev(user, item, time, user_map, item_map)
    if item.dim() != 2:
        raise RuntimeError("store_lookup: item must be [B, I]")
    B, I = item.shape
    _i64c(user, "store_lookup: user", (B,)), _i64c(item, "store_lookup: item"), _i64c(time, "store_lookup: time", (B,))
    keys, rows, n = _store_index(keys, rows, "store_lookup: target")
    if (neg_keys is None) != (neg_rows is None):
        raise RuntimeError("store_lookup: neg_keys and neg_rows go together")
    nk, nr, nn = _store_index(neg_keys, neg_rows, "store_lookup: negatives") if neg_keys is not None else (None, None, -1)
    for mp, nm in ((user_map, "user_map"), (item_map, "item_map")):
        if mp is not None:
            _i64c(mp, "store_lookup: " + nm, (mp.numel(),))
    rowidx = torch.empty((B, I), dtype=torch.int32, device=item.device)
    if miss is None:
        miss = torch.full((2,), STORE_MISS_NONE, dtype=torch.int64, device=item.device)
    else:
        _dev(miss), _i64c(miss, "store_lookup: miss", (2,))
    _check(lib().segmm_store_lookup(_ptr(user), _ptr(item), _ptr(time), B, I, _ptr(keys), _ptr(rows), n, _ptr(nk), _ptr(nr), nn,
                                    _ptr(user_map), 0 if user_map is None else user_map.numel(), _ptr(item_map),
                                    0 if item_map is None else item_map.numel(), _ptr(rowidx), _ptr(miss), _stream()), "segmm_store_lookup")
    return rowidx, miss


def _store_vals(vals, S, name):
    """(pointer, rows) of a value matrix [m, S]; a missing or empty one is (None, 0): an index into it gives NaN weights"""
    if vals is None or vals.shape[0] == 0:
        return None, 0
    _dev(vals)
    if vals.dim() != 2 or vals.shape[1] != S:
        raise RuntimeError("%s must be [m, %d] (got %s)" % (name, S, list(vals.shape)))
    return _ptr(_f32c(vals, name)), vals.shape[0]


def _store_rows(rowidx, duration, shape, what):
    _dev(rowidx, duration)
    if rowidx is not None and (rowidx.dtype != torch.int32 or not rowidx.is_contiguous() or tuple(rowidx.shape) != tuple(shape)):
        raise RuntimeError("%s: rowidx must be contiguous int32 %s" % (what, list(shape)))
    if duration is not None:
        _i64c(duration, what + ": duration", shape)


def store_head(pred, rowidx, vals, neg_vals=None, duration=None, weight_out=False):
    """``segmm_store_head``: out[..., i] = sum_s pred[..., i, s] * w(rowidx[..., i])[s] * (s < duration[..., i]); rowidx -1 = ones,
    r >= 0 = vals[r], r <= -2 = neg_vals[-2 - r].  ``weight_out=True``: returns (out, weights [..., S]) as well.  ``pred=None``: only
    the weights, of ``vals``' segment count."""
    _dev(pred, rowidx)
    if pred is None:
        if vals is None:
            raise RuntimeError("store_head: without pred the segment count comes from vals")
        S, shape, weight_out = vals.shape[1], tuple(rowidx.shape), True
    else:
        S, shape = pred.shape[-1], tuple(pred.shape[:-1])
        _f32c(pred, "store_head: pred")
    _store_rows(rowidx, duration, shape, "store_head")
    vp, m = _store_vals(vals, S, "store_head: vals")
    ngp, mn = _store_vals(neg_vals, S, "store_head: neg_vals")
    out = None if pred is None else torch.empty(shape, dtype=torch.float32, device=rowidx.device)
    w = torch.empty(shape + (S,), dtype=torch.float32, device=rowidx.device) if weight_out else None
    rows = rowidx.numel()
    with _kprof("store_head", rows * (4 * S * ((pred is not None) + (w is not None)) + 8 + 8 * (duration is not None))):
        _check(lib().segmm_store_head(_ptr(pred), _ptr(rowidx), vp, m, ngp, mn, _ptr(duration), rows, S, _ptr(out), _ptr(w), _stream()),
               "segmm_store_head")
    return w if pred is None else (out, w) if weight_out else out


def store_head_bwd(g, S, rowidx=None, vals=None, neg_vals=None, weight=None, duration=None):
    """``segmm_store_head_bwd``: dpred[..., i, s] = (g[..., i] * w[s]) * (s < duration[..., i]) with w from rowidx + the value
    matrices, from an explicit ``weight`` [..., S], or ones."""
    _dev(g, weight)
    shape, S = tuple(g.shape), int(S)
    _f32c(g, "store_head_bwd: g")
    if rowidx is not None and weight is not None:
        raise RuntimeError("store_head_bwd: rowidx and an explicit weight exclude each other")
    _store_rows(rowidx, duration, shape, "store_head_bwd")
    if weight is not None and (tuple(weight.shape) != shape + (S,) or weight.dtype != torch.float32 or not weight.is_contiguous()):
        raise RuntimeError("store_head_bwd: weight must be contiguous float32 %s" % list(shape + (S,)))
    vp, m = _store_vals(vals, S, "store_head_bwd: vals")
    ngp, mn = _store_vals(neg_vals, S, "store_head_bwd: neg_vals")
    dpred = torch.empty(shape + (S,), dtype=torch.float32, device=g.device)
    _check(lib().segmm_store_head_bwd(_ptr(g), _ptr(rowidx), vp, m, ngp, mn, _ptr(weight), _ptr(duration), g.numel(), S, _ptr(dpred),
                                      _stream()), "segmm_store_head_bwd")
    return dpred


def store_append(user, photo, time_ms, logits, row0, keys, vals):
    """``segmm_store_append``: the batch's key columns (device int64 [B] each) and its logits (float32 [B, S], rows ``logits.stride(0)``
    floats apart) into rows [row0, row0 + B) of the tables keys (int64 [capacity, 3]) / vals (float32 [capacity, S]).  One launch, a
    recordable command; an overflow is refused by the library."""
    _dev(user, photo, time_ms, logits, keys, vals)
    if (logits.dim() != 2 or logits.dtype != torch.float32 or logits.shape[1] < 1 or (logits.shape[1] > 1 and logits.stride(1) != 1)
            or (logits.shape[0] > 1 and logits.stride(0) < logits.shape[1])):
        raise RuntimeError("store_append: logits must be float32 [B, S] with unit column stride and a row stride >= S (got %s %s, strides %s)"
                           % (logits.dtype, list(logits.shape), list(logits.stride())))
    B, S = logits.shape
    ld = logits.stride(0) if B > 1 else S
    for t, nm in ((user, "user"), (photo, "photo"), (time_ms, "time_ms")):
        _i64c(t, "store_append: " + nm, (B,))
    cap = keys.shape[0]
    _i64c(keys, "store_append: keys", (cap, 3))
    if vals.dtype != torch.float32 or not vals.is_contiguous() or tuple(vals.shape) != (cap, S):
        raise RuntimeError("store_append: vals must be contiguous float32 [%d, %d] (got %s %s)" % (cap, S, vals.dtype, list(vals.shape)))
    if B == 0:          # (an empty batch has no addresses to pass: nothing is launched)
        if not 0 <= int(row0) <= cap:
            raise RuntimeError("store_append: row0 = %d outside the capacity of %d rows" % (row0, cap))
        return
    with _kprof("store_append", B * (8 * S + 48)):
        _check(lib().segmm_store_append(_ptr(user), _ptr(photo), _ptr(time_ms), _ptr(logits), int(ld), int(B), int(S), int(row0), int(cap), _ptr(keys),
                                        _ptr(vals), _stream()), "segmm_store_append")


STORE_INDEX_MAX = _K["SEGMM_STORE_INDEX_MAX"]          # keys segmm_store_index is built for


def store_index_ws_bytes(n):
    """Bytes of workspace ``segmm_store_index`` needs for ``n`` keys (refused by name beyond STORE_INDEX_MAX)."""
    nb = _i64(0)
    _check(_lib_real().segmm_store_index_ws(C.byref(nb), int(n)), "segmm_store_index_ws")
    return int(nb.value)


def store_index(keys, ws=None, out_keys=None, out_rows=None, n_unique=None):
    """``segmm_store_index``: keys (device int64 [n, 3], unsorted, duplicates allowed) -> (out_keys int64 [n, 3], out_rows int32 [n],
    n_unique int64 [1]) on the device: the first n_unique entries are the index ``segmm_store_lookup`` takes (sorted unique keys, the
    row of each key's last occurrence).  Never synchronises; ``ws``: a uint8 tensor of ``store_index_ws_bytes(n)`` bytes (allocated
    here when not given)."""
    _dev(keys)
    n = keys.shape[0]
    _i64c(keys, "store_index: keys", (n, 3))
    need = store_index_ws_bytes(n)
    if ws is None:
        ws = torch.empty((need,), dtype=torch.uint8, device=keys.device)
    if ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.numel() < need:
        raise RuntimeError("store_index: %d keys need a contiguous uint8 workspace of %d bytes" % (n, need))
    if out_keys is None:
        out_keys = torch.empty((n, 3), dtype=torch.int64, device=keys.device)
    if out_rows is None:
        out_rows = torch.empty((n,), dtype=torch.int32, device=keys.device)
    if n_unique is None:
        n_unique = torch.empty((1,), dtype=torch.int64, device=keys.device)
    _i64c(out_keys, "store_index: out_keys", (n, 3)), _i64c(n_unique, "store_index: n_unique", (1,))
    if out_rows.dtype != torch.int32 or not out_rows.is_contiguous() or tuple(out_rows.shape) != (n,):
        raise RuntimeError("store_index: out_rows must be contiguous int32 [%d]" % n)
    _dev(ws, out_keys, out_rows, n_unique)
    with _kprof("store_index", 56 * n):
        _check(lib().segmm_store_index(_ptr(keys) if n else None, n, _ptr(ws) if n else None, ws.numel(), _ptr(out_keys) if n else None,
                                       _ptr(out_rows) if n else None, _ptr(n_unique), _stream()), "segmm_store_index")
    return out_keys, out_rows, n_unique


def pool_tokens(U, Lu, V, Lv, out, B, d, bins):
    """AdaptiveAvgPool1d(bins) over the tokens of cat(U[B,Lu,d], V[B,Lv,d]) (CrossMLP ablation)."""
    _dev(U, V, out)
    _check(lib().segmm_pool_tokens(_ptr(U), Lu, _ptr(V), Lv, _ptr(out), B, d, bins, _stream()), "segmm_pool_tokens")


def pool_tokens_bwd(dOut, dU, Lu, dV, Lv, B, d, bins):
    _dev(dOut, dU, dV)
    _check(lib().segmm_pool_tokens_bwd(_ptr(dOut), _ptr(dU), Lu, _ptr(dV), Lv, B, d, bins, _stream()), "segmm_pool_tokens_bwd")


def sr_len(S, r):
    """Reduced key length of ``S`` video segments under sr_ratio ``r`` (encoder.py:23-31,84-102): the conv length
    (S + 2p - r) // r + 1, p = (r - 1) // 2, must equal the mask-pool length S // r and be >= 1 -- the reference raises where they
    differ; refused here, by name."""
    S, r = int(S), int(r)
    if not 2 <= r <= 8:
        raise NotImplementedError("sr_ratio = %d is not built (1, or 2 <= sr_ratio <= 8)" % r)
    p = (r - 1) // 2
    Lc, Lm = ((S + 2 * p - r) // r + 1 if S + 2 * p >= r else 0), S // r
    if Lc != Lm or Lm < 1:
        raise RuntimeError("S=%d video segments with sr_ratio=%d: the reducing conv gives %d keys and the mask pool %d (the reference "
                           "fails there too; r = 4 and 8 need S %% r in {0, 1})" % (S, r, Lc, Lm))
    return Lm


def sr_pack(x, ldx, m, A, m_sr, amax, B, S, d, r):
    """A[b Ls + j, c r + t] = x[b, j r - p + t, c] (0 outside the sequence) + partial maxima of |A| + pooled mask m_sr (csrc/srops.h)."""
    _dev(x, A)
    _check(lib().segmm_sr_pack(_ptr(x), ldx, _ptr(m), _ptr(A), _ptr(m_sr), _ptr(amax), B, S, d, r, _stream()), "segmm_sr_pack")


def sr_unpack(dA, res, G, B, S, d, r):
    """G[b, i, c] = res[b, i, c] + dA[b Ls + (i + p) // r, c r + (i + p) % r] (rows in no window: res, or 0); ``res`` may be None."""
    _dev(dA, G)
    _check(lib().segmm_sr_unpack(_ptr(dA), _ptr(res), _ptr(G), B, S, d, r, _stream()), "segmm_sr_unpack")


def colsum3(Xs, ld, M, N, outs, ws):
    """Column sums of up to three same-shaped [M, N] matrices in one launch pair; ws: 3 * colsum_chunks(M) * N floats."""
    X = list(Xs) + [None] * (3 - len(Xs))
    O = list(outs) + [None] * (3 - len(outs))
    _check(lib().segmm_colsum3(_ptr(X[0]), _ptr(X[1]), _ptr(X[2]), ld, M, N, _ptr(O[0]), _ptr(O[1]), _ptr(O[2]), _ptr(ws), _stream()),
           "segmm_colsum3")
