"""The parts of tests/id_rows_cases.py that need no GPU: the id schedule keeps its promises, check 1 sees a planted stale row, check 3
refuses a planted short previous tensor and a planted over-long count (hand-built command arrays, as in test_recording_cpu.py) and
lets the recorded arrangement through, the reference run's patch really replaces ``hipabi.zero_rows`` -- and the library's own
host check (``recording.check_shapes``, which ``run_recorded`` passes before it launches) refuses the same short tensor."""
import pytest
import torch

import id_rows_cases as C

def test_the_id_schedule_meets_its_conditions():
    from segmminterest_amd.dp import shard_rows
    for name, seq in list(C.SEQUENCES.items()) + [("DP", C.DP_SEQUENCE)]:
        sz = C.sizes(seq)
        assert len(sz) == len([t for t in seq if t != "V"]) and set(sz) <= {C.FULL} | set(C.SHORT)
        rep = C.schedule_report(seq)
        assert rep["duplicates"], name                                           # every batch, both tables
        assert rep["in_range"] and not rep["covers"], name                        # no batch covers a table's whole id range
        assert rep["short_absent_items"] and min(rep["short_absent_items"]) >= 2, (name, rep)
        assert rep["short_absent_users"] and min(rep["short_absent_users"]) >= 1, (name, rep)
        assert rep["returns"] and rep["never"], (name, rep)
    assert C.sizes(C.SEQUENCES["A"]) == [16, 16, 16, 16, 16, 8, 16, 16, 5, 16, 16, 16]
    assert C.sizes(C.SEQUENCES["B"]) == [16, 16, 16, 16, 8, 16, 16, 5, 16, 16]
    assert C.sizes(C.SEQUENCES["C"]) == [16, 16, 16, 16, 8, 8, 8, 8, 8, 16, 8, 8]
    assert C.sizes(C.DP_SEQUENCE) == [16, 16, 16, 8, 16, 16, 8, 16, 16, 16]
    assert 5 in C.sizes(C.SEQUENCES["A"]) and 5 % 4
    # data parallel: 16 and 8 rows shard evenly over two ranks, the ranks' shards tile the batch in order
    for n in (16, 8):
        assert [shard_rows(n, 2, r) for r in range(2)] == [(0, n // 2), (n // 2, n)]
        assert shard_rows(n, 1, 0) == (0, n)
    # the returning id of a short batch is absent from the next step and present two steps later (sequence A, step 8)
    assert C.ITEM_BACK in C.ids_for(8, 5)[0].tolist() and C.ITEM_BACK not in C.ids_for(9, 16)[0].tolist() and C.ITEM_BACK in C.ids_for(10, 16)[0].tolist()


def test_make_batches_overwrites_both_id_tensors_and_their_copies():
    cfg = dict(S=6, Lt=1, D_in=0, n_users=50, n_items=200)
    bs = C.make_batches(cfg, C.SEQUENCES["A"])
    assert [b["label"].shape[0] for b in bs] == C.sizes(C.SEQUENCES["A"])
    for t, b in enumerate(bs):
        items, users = C.ids_for(t, b["label"].shape[0])
        for key, want in (("photo_identity_id", items), ("photo_id", items), ("user_identity_id", users), ("user_id", users)):
            assert b[key].dtype == torch.int64 and torch.equal(b[key], want), (t, key)
        assert b["photo_id"].data_ptr() != b["photo_identity_id"].data_ptr()


def test_check_1_rejects_a_planted_stale_row():
    g = torch.zeros(201, 16)
    ids = [3, 3, 7, 150]
    for i in ids:
        g[i] = 1.0
    assert C.stale_rows(g, ids) == []
    g[7] = 0.0          # (a listed row may be all zero: dropout, a masked row)
    assert C.stale_rows(g, ids) == []
    g[42, 5] = 1e-30
    assert C.stale_rows(g, ids) == [42]
    g[42, 5] = -0.0          # a row that was written, even with a zero of the other sign
    assert C.stale_rows(g, ids) == [42]
    g[42, 5] = 0.0
    g[200, 15] = float("nan")
    assert C.stale_rows(g.numpy(), ids) == [200]


def _ids_batch(buf, at, rows=16):
    return {"photo_identity_id": buf[at:at + 8 * rows].view(torch.int64), "label": buf[at + 256:at + 256 + 8 * rows * 3].view(torch.int64).view(rows, 3)}


def _recording(batch, prev, outside, n, ids_off=0):
    """A recording of three commands: a copy from the current batch's labels, a ``segmm_zero_rows`` of ``n`` ids that names the
    PREVIOUS batch's item ids (lag 1), one that names a buffer outside every batch (the data-parallel arrangement)."""
    from segmminterest_amd import hipabi as H
    from segmminterest_amd import recording as R
    rec = H.Recorder(111, 222)
    rec.mark(H.PHASE_STEP_BEGIN)
    rec.call("segmm_copy_bytes", (outside, batch["label"].data_ptr(), 16, 111))
    rec.call("segmm_zero_rows", (outside + 512, 16, prev["photo_identity_id"].data_ptr() + ids_off, n, 201, 111))
    rec.call("segmm_zero_rows", (outside + 512, 16, outside + 1024, 4 * n, 201, 111))
    phases = rec.finish()
    relocs = R.relocations(phases, rec.pslots, (batch, prev))
    assert [(ci, ai, k, off, lag) for _, ci, ai, k, off, lag in relocs] == [(0, 1, "label", 0, 0), (1, 2, "photo_identity_id", ids_off, 1)]
    return dict(phases=[], keep_phases=phases, relocs=relocs, spans=R.batch_shapes(batch), main=111, table=None)


def test_check_3_rejects_a_short_previous_tensor_and_an_overlong_count_and_accepts_the_recorded_arrangement(monkeypatch):
    from segmminterest_amd import hipabi as H
    from segmminterest_amd import recording as R
    buf = torch.zeros(8192, dtype=torch.uint8)
    batch, prev, outside = _ids_batch(buf, 0), _ids_batch(buf, 1024), buf.data_ptr() + 4096
    r = _recording(batch, prev, outside, 16)
    new, new_prev = _ids_batch(buf, 2048), _ids_batch(buf, 3072)
    short = _ids_batch(torch.zeros(2048, dtype=torch.uint8), 0, rows=8)
    C.check_replay(r, new, new_prev)          # the recorded arrangement: another batch pair of the recorded shapes
    C.check_replay(r, batch, prev)
    with pytest.raises(C.ReplayGuardError, match=r"prev\['photo_identity_id'\] of \(8,\)"):
        C.check_replay(r, new, short)          # the short batch of an eager step as "the previous batch"
    with pytest.raises(C.ReplayGuardError, match=r"batch\['label'\] of \(8, 3\)"):
        C.check_replay(r, short, new_prev)
    with pytest.raises(C.ReplayGuardError, match="no tensor"):
        C.check_replay(r, new, None)
    # the recorded count longer than the tensor it is read from: same shapes, n = 17 (and n = 16 from byte 8)
    with pytest.raises(C.ReplayGuardError, match=r"reads 17 ids from byte 0 .* holds 128 bytes"):
        C.check_replay(_recording(batch, prev, outside, 17), new, new_prev)
    with pytest.raises(C.ReplayGuardError, match=r"reads 16 ids from byte 8 "):
        C.check_replay(_recording(batch, prev, outside, 16, ids_off=8), new, new_prev)
    C.check_replay(_recording(batch, prev, outside, 15, ids_off=8), new, new_prev)
    # the guard wraps replay, checks first and calls through: a refused replay moves no slot and reaches nothing behind it
    calls, log = [], []
    guarded = C.guarded_replay(lambda *a, **kw: calls.append(a), log)
    image = bytes(r["keep_phases"][0][1])
    with pytest.raises(C.ReplayGuardError):
        guarded(r, "run_recorded()", "step", new, short)
    assert not calls and not log and bytes(r["keep_phases"][0][1]) == image
    guarded(r, "run_recorded()", "step", new, new_prev)
    assert len(calls) == 1 and log == ["step"]
    # ... and the library's own check, which run_recorded passes before its first launch, refuses the same tensors
    monkeypatch.setattr(H, "_stream", lambda: 111)
    before = []
    with pytest.raises(RuntimeError, match=r"^run_recorded\(\): the previous batch\['photo_identity_id'\] is \(8,\) torch.int64, the step was recorded "
                                           r"for \(16,\) torch.int64$"):
        R.replay(r, "run_recorded()", "step", new, short, before=lambda: before.append(1))
    with pytest.raises(RuntimeError, match=r"^run_recorded\(\): batch\['label'\] is \(8, 3\) torch.int64"):
        R.replay(r, "run_recorded()", "step", short, new_prev, before=lambda: before.append(1))
    assert not before and bytes(r["keep_phases"][0][1]) == image
    R.replay(r, "run_recorded()", "step", new, new_prev, before=lambda: before.append(1))
    assert before == [1] and bytes(r["keep_phases"][0][1]) != image
    c = r["keep_phases"][0][1][1]
    assert H.cmd_arg(c, "segmm_zero_rows", "ids") == new_prev["photo_identity_id"].data_ptr() and H.cmd_arg(c, "segmm_zero_rows", "n") == 16


def test_the_reference_patch_replaces_zero_rows(monkeypatch):
    from segmminterest_amd import engine as E
    from segmminterest_amd import hipabi as H
    real = H.zero_rows
    filled = []
    monkeypatch.setattr(H, "fill_zero", lambda t: filled.append(t))
    table = torch.zeros(5, 4)
    with C.dense_clears() as patched:
        assert H.zero_rows is patched is not real and E.H.zero_rows is patched          # the name engine._embed_bwd calls
        H.zero_rows(table, torch.tensor([1, 2]))
        assert len(filled) == 1 and filled[0] is table
    assert H.zero_rows is real
    with pytest.raises(ZeroDivisionError):
        with C.dense_clears():
            1 / 0
    assert H.zero_rows is real


def test_the_replay_guard_is_installed_and_removed():
    from segmminterest_amd import recording as R
    real = R.replay
    with C.replay_guard() as log:
        assert R.replay is not real and log == []
    assert R.replay is real
