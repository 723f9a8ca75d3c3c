"""Record a launch sequence once, replay it with the batch's pointers re-based: the one statement of the mechanism behind
``Trainer.record`` / ``run_recorded`` (the training step) and ``valid_model(recorded=True)`` (a validation batch).

A recording is a plain dict: ``phases`` ([(Phase, Cmd array) | (host action, None)], ``Recorder.finish``), ``keep`` and ``pool`` (what
the recorded pointers name: host structs, the private memory pool of the recorded run), ``relocs`` ([(Cmd array, command, argument
slot, batch key, byte offset, lag)]: the pointer slots that name a batch tensor; lag 1 = the PREVIOUS batch's), ``spans``
(:func:`batch_shapes` of the recorded batch), ``main`` / ``events`` / ``table`` (the stream it replays on, the stream table of
``hipabi.run_phase``), ``n_cmds`` and, made on the first replay, ``reloc_keys`` (the (batch key, lag) pairs of ``relocs``: the
tensors :func:`check_shapes` looks at before every replay).  Its owner adds what only it knows (the step: ``prev_batch`` -- None
behind a step that was no replay of it --, ``tab_keys``, ``hdr_cleared`` / ``hdr_used``, ``hyper``, ``out``; the validation batch:
its named tail commands, ``cfg``, ``n_replays``)."""
from __future__ import annotations

import contextlib
import ctypes

import torch

from . import hipabi as H


def batch_shapes(batch):
    """``{key: (shape, dtype)}`` over the non-empty tensors of a batch: what a recording is valid for."""
    return {k: (tuple(v.shape), v.dtype) for k, v in batch.items() if torch.is_tensor(v) and v.numel()}


@contextlib.contextmanager
def capture(st, side, aux=0):
    """The context a launch sequence is recorded in, on the current stream: every C-ABI call of the body is noted by an
    ``H.Recorder`` (``side`` / ``aux``: the raw handles of the store's other streams, 0 = none) while it runs, and the body's
    allocations come from a private memory pool (``ParamStore.rec_pool``).  The device is idle when the body starts and when the
    context is left; ``H.RECORDER`` is cleared however the body ends.  Yields what :func:`finish` takes."""
    torch.cuda.synchronize()
    main = H._stream()
    pool = torch.cuda.MemPool()
    rec = H.Recorder(main, side, aux)
    H.RECORDER = rec
    try:
        with st.rec_pool(pool):
            yield dict(rec=rec, pool=pool, streams=[main, side] + ([aux] if aux else []))
    finally:
        H.RECORDER = None
    torch.cuda.synchronize()


def relocations(phases, pslots, batches):
    """The relocation table of recorded ``phases``: one ``(arr, ci, ai, key, offset, lag)`` per pointer slot that falls inside a
    tensor of ``batches[lag]`` (the current batch is searched before the previous one)."""
    spans = [[(k, v.data_ptr(), v.numel() * v.element_size()) for k, v in b.items() if torch.is_tensor(v) and v.numel()] for b in batches]
    relocs = []
    for pi, (ph, arr) in enumerate(phases):
        if arr is None:
            continue
        # only the slots recorded as POINTER arguments (Recorder.pslots): an integer / float slot -- a seed, a byte count, the
        # bit pattern of lr -- that happens to fall inside a batch tensor's address range must never be rewritten
        for ci, ai in pslots[pi]:
            pv = arr[ci].a[ai].p
            hit = next(((k, pv - base, lag) for lag, sp in enumerate(spans) for k, base, nb in sp if base <= pv < base + nb), None)
            if hit is not None:
                relocs.append((arr, ci, ai) + hit)
    return relocs


def finish(cap, batches):
    """The recording of a left :func:`capture` context ``cap``.  ``batches``: ``(batch,)``, or ``(batch, previous batch)`` for a
    sequence that also names tensors of the batch before it -- every recorded pointer into one of them is re-based per replay."""
    rec, streams = cap["rec"], cap["streams"]
    phases = rec.finish()
    evs = tuple(torch.cuda.Event() for _ in range(4))
    for e in evs:
        e.record()
    return dict(phases=phases, keep=rec.keep, pool=cap["pool"], relocs=relocations(phases, rec.pslots, batches), spans=batch_shapes(batches[0]),
                main=streams[0], events=evs, table=H.stream_table(streams, [e.cuda_event for e in evs[:2 * (len(streams) - 1)]]),
                n_cmds=sum(ph.n_cmds for ph, a in phases if a is not None))


def rebase(r, batch, prev=None):
    """Points the recorded commands at the tensors of ``batch`` (lag-1 slots: at those of ``prev``)."""
    for arr, ci, ai, k, off, lag in r["relocs"]:
        arr[ci].a[ai].p = (prev if lag else batch)[k].data_ptr() + off


def check_shapes(r, who, what, batch, prev=None):
    """Refuses a replay one of whose pointer slots would name a tensor of another shape or dtype than the recorded one: every
    recorded count, stride and byte size travels by value, so such a launch reads or writes outside the tensor.  Looks at the
    tensor each slot is about to name -- ``prev`` for lag 1, ``batch`` for lag 0 -- and at nothing else of the batches."""
    spans = r.get("spans")
    if spans is None:
        return
    keys = r.get("reloc_keys")
    if keys is None:
        keys = r["reloc_keys"] = sorted({(k, lag) for _, _, _, k, _, lag in r["relocs"]})
    for k, lag in keys:
        src = prev if lag else batch
        v = src.get(k) if src is not None else None
        if not torch.is_tensor(v) or (tuple(v.shape), v.dtype) != spans[k] or not v.is_contiguous():
            got = "missing" if not torch.is_tensor(v) else "%s %s" % (tuple(v.shape), v.dtype)
            raise RuntimeError("%s: %s[%r] is %s, the %s was recorded for %s %s" % (who, "the previous batch" if lag else "batch", k, got, what,
                                                                                   spans[k][0], spans[k][1]))


def replay(r, who, what, batch, prev=None, timed=None, before=None):
    """Enqueues the recording ``r`` on ``batch``: refuses a current stream other than the recorded one (``who`` / ``what``: the
    caller and "step" / "validation batch" in the message) and a tensor of another shape behind a pointer slot
    (:func:`check_shapes`) BEFORE anything of ``r`` is touched, re-bases the batch pointers, then one C call per phase.
    ``before``: launches of the caller's that belong ahead of the first phase, enqueued once the checks have passed.
    ``timed``: see ``Trainer.run_recorded``."""
    if H._stream() != r["main"]:
        raise RuntimeError("%s: the current stream is not the stream the %s was recorded on" % (who, what))
    check_shapes(r, who, what, batch, prev)
    if before is not None:
        before()
    rebase(r, batch, prev)
    table = r["table"]
    if timed is not None:
        return _replay_timed(r, table, timed)
    for ph, arr in r["phases"]:
        if arr is None:
            ph()          # a host action of the step (data-parallel collective / wait), at its place in the launch order
        else:
            H.run_phase(ph, table)


def _replay_timed(r, table, timed):
    streams = r.get("timed_streams")
    if streams is None:
        streams = r["timed_streams"] = [torch.cuda.current_stream()] + [torch.cuda.ExternalStream(int(h)) for h in list(table[0])[1:]]
    for item in timed_plan(r):
        if item[0] == "host":
            item[1]()
        elif item[0] == "run":
            H.run_phase(item[1], table)
        else:
            _, ph1, slot, (fam, head) = item
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(streams[slot])
            H.run_phase(ph1, table)
            e1.record(streams[slot])
            timed[0 if fam == "gemm" else 1].append(head + (e0, e1))


def timed_plan(r):
    """The recorded phases cut at every GEMM / attention command (bench.py's timed replay): [("host", fn) | ("run", Phase) |
    ("timed", Phase of ONE command, stream slot, record)], record = the tuple hipabi's GEMM_PROFILE / ATTN_PROFILE entries
    start with.  The sub-phases alias the recorded command arrays (the per-step re-basing of batch pointers reaches them)."""
    plan = r.get("timed_plan")
    if plan is not None:
        return plan
    names = {v: k for k, v in H.op_ids().items()}
    plan = []
    for ph, arr in r["phases"]:
        if arr is None:
            plan.append(("host", ph))
            continue
        def sub(lo, hi, ph=ph, arr=arr):
            return H.Phase(kind=ph.kind, backbone=ph.backbone, layer=ph.layer, n_cmds=hi - lo,
                           cmds=ctypes.cast(ctypes.byref(arr, lo * ctypes.sizeof(H.Cmd)), ctypes.POINTER(H.Cmd)))
        lo = 0
        for ci in range(ph.n_cmds):
            c = arr[ci]
            nm = names.get(c.op)
            def args(*params, c=c, nm=nm):          # the command's arguments, by the header's parameter names
                return [H.cmd_arg(c, nm, p) for p in params]
            rec = None
            if nm in ("segmm_gemm", "segmm_gemm_h"):
                rec = ("gemm", H.gemm_record(*args("layout", "M", "N", "K")))
            elif nm == "segmm_gemm_p":
                rec = ("gemm", H.gemm_record(*args("layout", "M", "N", "K", "write_c")))
            elif nm == "segmm_attn_fwd":
                rec = ("attn", H.attn_record(*args("B", "H", "dh", "Lq", "La", "Lb")))
            elif nm == "segmm_attn_bwd":
                planes, = args("planes")
                rec = ("attn", H.attn_record(*args("B", "H", "dh", "Lq", "La", "Lb", "phase"), H.AttnPlanes.from_address(planes) if planes else None))
            if rec is None or rec[1] is None:          # (gemm_record: a repair launch is not timed)
                continue
            if ci > lo:
                plan.append(("run", sub(lo, ci)))
            plan.append(("timed", sub(ci, ci + 1), c.stream, rec))
            lo = ci + 1
        if ph.n_cmds > lo:
            plan.append(("run", sub(lo, ph.n_cmds)))
    r["timed_plan"] = plan
    return plan
