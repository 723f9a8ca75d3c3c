"""Capture / relocation / replay of a recorded launch sequence (segmminterest_amd/recording.py), the parts that need no GPU: the
relocation table over a recorder's pointer slots, ``rebase``, ``batch_shapes``, the refusal of a wrong stream -- and the facade of
names ``trainer.py`` keeps after its split."""
import ctypes

import pytest
import torch

LABEL_B, PHOTO_B = 4 * 3 * 8, 4 * 3 * 8 * 4          # bytes of label int64 [4, 3] and photo float32 [4, 3, 8]


def _batch(buf, at):
    """{label, photo} as views of the byte buffer ``buf`` from byte ``at``: a gap behind each tensor, so that one past the end of a
    tensor is inside nothing."""
    return {"label": buf[at:at + LABEL_B].view(torch.int64).view(4, 3), "photo": buf[at + 128:at + 128 + PHOTO_B].view(torch.float32).view(4, 3, 8)}


def _record(batch, prev, outside):
    """Two fragments with a host action between them -> (phases, pslots, the expected relocations as (phase, command, slot, key,
    offset, lag), the host action's call counter)."""
    from segmminterest_amd import hipabi as H
    lab, pho, plab = batch["label"].data_ptr(), batch["photo"].data_ptr(), prev["label"].data_ptr()
    calls = []
    rec = H.Recorder(111, 222)
    rec.mark(H.PHASE_STEP_BEGIN)
    rec.call("segmm_copy_bytes", (outside, pho, 16, 111))                      # the base of a current-batch tensor; dst outside all
    rec.call("segmm_copy_bytes", (lab + 40, outside + 64, 8, 222))             # an interior byte
    rec.call("segmm_fill_zero", (pho + PHOTO_B - 1, 1, 111))                   # the last byte ...
    rec.call("segmm_fill_zero", (pho + PHOTO_B, 1, 111))                       # ... and one past the end: not relocated
    rec.callback(lambda: calls.append(1))
    rec.call("segmm_copy_bytes", (outside, plab + 8, 8, 111))                  # inside a previous-batch tensor
    rec.call("segmm_fill_zero", (outside, pho + 4, 111))                       # INTEGER slots (bytes, n) whose value lies inside a
    rec.call("segmm_vec_add", (outside, outside + 64, outside + 128, lab + 16, 222))          # batch tensor's address range
    phases = rec.finish()
    assert [a is None for _, a in phases] == [False, True, False] and phases[0][0].n_cmds == 4 and phases[2][0].n_cmds == 3
    assert phases[2][1][1].a[1].i == pho + 4 and phases[2][1][2].a[3].i == lab + 16
    want = [(0, 0, 1, "photo", 0, 0), (0, 1, 0, "label", 40, 0), (0, 2, 0, "photo", PHOTO_B - 1, 0), (2, 0, 1, "label", 8, 1)]
    return phases, rec.pslots, want, calls


def _image(phases, relocs=()):
    """bytes of every command array, the slots listed in ``relocs`` zeroed."""
    from segmminterest_amd import hipabi as H
    out = []
    for _, arr in phases:
        if arr is None:
            continue
        b = bytearray(bytes(arr))
        for a, ci, ai, *_ in relocs:
            if a is arr:
                o = ci * ctypes.sizeof(H.Cmd) + H.Cmd.a.offset + ai * ctypes.sizeof(H.CmdArg)
                b[o:o + 8] = bytes(8)
        out.append(bytes(b))
    return out


def test_relocations_list_exactly_the_pointer_slots_inside_the_batches_and_rebase_moves_only_them():
    from segmminterest_amd import recording as R
    buf = torch.zeros(4096, dtype=torch.uint8)
    batch, prev, outside = _batch(buf, 0), _batch(buf, 1024), buf.data_ptr() + 3072
    phases, pslots, want, _ = _record(batch, prev, outside)
    relocs = R.relocations(phases, pslots, (batch, prev))
    index = {id(arr): pi for pi, (_, arr) in enumerate(phases) if arr is not None}
    assert [(index[id(arr)], ci, ai, k, off, lag) for arr, ci, ai, k, off, lag in relocs] == want
    for arr, ci, ai, k, off, lag in relocs:
        assert arr[ci].a[ai].p == (prev if lag else batch)[k].data_ptr() + off
    # a validation recording relocates against its batch alone: the same entries, the previous batch's gone, every lag 0
    assert [(index[id(r[0])],) + r[1:] for r in R.relocations(phases, pslots, (batch,))] == want[:3]

    before, masked = _image(phases), _image(phases, relocs)
    buf2 = torch.zeros(4096, dtype=torch.uint8)
    new, new_prev = _batch(buf2, 2048), _batch(buf2, 512)
    r = {"relocs": relocs}
    R.rebase(r, new, new_prev)
    for arr, ci, ai, k, off, lag in relocs:
        assert arr[ci].a[ai].p == (new_prev if lag else new)[k].data_ptr() + off
    assert _image(phases) != before and _image(phases, relocs) == masked          # every other slot of every command: byte for byte
    R.rebase(r, batch, prev)
    assert _image(phases) == before


def test_batch_shapes_is_the_rule_a_recording_stores():
    from segmminterest_amd.recording import batch_shapes
    batch = {"label": torch.zeros(4, 3, dtype=torch.int64), "photo": torch.zeros(4, 3, 8), "user": torch.zeros(0, 5), "name": "x", "n": 3,
             "photo_mask": torch.ones(4, 3, dtype=torch.bool)}
    assert batch_shapes(batch) == {"label": ((4, 3), torch.int64), "photo": ((4, 3, 8), torch.float32), "photo_mask": ((4, 3), torch.bool)}
    assert list(batch_shapes(batch)) == ["label", "photo", "photo_mask"]          # the batch's own key order
    assert batch_shapes({}) == {} and batch_shapes({"user": torch.zeros(0)}) == {}


def test_replay_refuses_a_wrong_stream_before_it_touches_the_recording(monkeypatch):
    from segmminterest_amd import hipabi as H
    from segmminterest_amd import recording as R
    buf = torch.zeros(4096, dtype=torch.uint8)
    batch, prev, outside = _batch(buf, 0), _batch(buf, 1024), buf.data_ptr() + 3072
    phases, pslots, _, calls = _record(batch, prev, outside)
    r = dict(phases=[p for p in phases if p[1] is None], relocs=R.relocations(phases, pslots, (batch, prev)), main=111, table=None, prev_batch=prev)
    before = _image(phases)
    new = _batch(torch.zeros(4096, dtype=torch.uint8), 0)
    monkeypatch.setattr(H, "_stream", lambda: 222)
    with pytest.raises(RuntimeError, match=r"^run_recorded\(\): the current stream is not the stream the step was recorded on$"):
        R.replay(r, "run_recorded()", "step", new, r["prev_batch"])
    with pytest.raises(RuntimeError, match=r"^valid_model\(recorded=True\): the current stream is not the stream the validation batch was recorded on$"):
        R.replay(r, "valid_model(recorded=True)", "validation batch", new)
    assert _image(phases) == before and r["prev_batch"] is prev and not calls
    # on the recorded stream: the slots move, the host action runs at its place (this recording keeps no launches: no device)
    monkeypatch.setattr(H, "_stream", lambda: 111)
    R.replay(r, "run_recorded()", "step", new, r["prev_batch"])
    assert calls == [1] and _image(phases) != before
    assert all(arr[ci].a[ai].p == (prev if lag else new)[k].data_ptr() + off for arr, ci, ai, k, off, lag in r["relocs"])


PUBLIC = {"trainer": ("init_model", "default_args", "batch_rows", "micro_slices", "Trainer"),
          "optim": ("GROUP_KEYS", "resolve_param_groups", "group_segments", "no_decay_groups", "LRSchedule", "PlateauLR", "parse_ema", "WeightEMA",
                    "FusedAdamW"),
          "dp": ("DPComm", "shard_rows"),
          "loop": ("early_stop_reached", "compute_final_result", "fit", "CheckPointer")}


def test_trainer_module_re_exports_every_public_name():
    import importlib
    facade = importlib.import_module("segmminterest_amd.trainer")
    for home, names in PUBLIC.items():
        mod = importlib.import_module("segmminterest_amd." + home)
        for n in names:
            assert getattr(facade, n) is getattr(mod, n), n
            assert not callable(getattr(mod, n)) or getattr(mod, n).__module__ == mod.__name__, n          # defined there, not passed on
    assert sum(len(v) for v in PUBLIC.values()) == 20
    for n in ("valid_model", "valid_enqueue", "test_model", "dump_logits", "eval_step", "fit", "record", "run_recorded", "train_step"):
        assert callable(getattr(facade.Trainer, n)), n
    # an optimizer state dict carries the schedule as a plain dict, never an instance: no checkpoint names a class by module path
    import dataclasses
    assert dataclasses.asdict(facade.LRSchedule(kind="exp", gamma=0.5)) == dict(kind="exp", warmup_steps=0, start_factor=1.0 / 3, decay_steps=0,
                                                                                  eta_min=0.0, gamma=0.5, step_size=1)
