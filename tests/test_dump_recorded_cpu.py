"""The store's writer, its device index build and the recorded dump, the parts that need no GPU: the three C entry points are
declared, exported and (the two launches) dispatchable under ABI version 30, the generated tables are not stale, and the host-side
argument checks of the entry points answer by name without touching a device."""
import ctypes
import os
import subprocess
import sys

from helpers import ROOT

NEW = ("segmm_store_append", "segmm_store_index_ws", "segmm_store_index")


def _L():
    from segmminterest_amd import hipabi as H
    return H, H.lib()


def test_new_entry_points_declared_exported_and_dispatchable():
    from segmminterest_amd import _abi
    H, L = _L()
    names = [L.segmm_cmd_op_name(i).decode() for i in range(L.segmm_cmd_op_count())]
    for n in ("segmm_store_append", "segmm_store_index"):
        assert n in _abi.PROTOTYPES and _abi.PROTOTYPES[n][-1] == ("stream", "p"), n
        assert n in names and hasattr(L, n), n          # segmm_run_phase can replay it from a recorded command
    ws = _abi.PROTOTYPES["segmm_store_index_ws"]
    assert ws == (("ws_bytes", "p"), ("n", "i64")) and "segmm_store_index_ws" not in names and hasattr(L, "segmm_store_index_ws")
    assert [p for p, _ in _abi.PROTOTYPES["segmm_store_append"]] == ["user", "photo", "time_ms", "logits", "ld", "B", "S", "row0", "capacity",
                                                                     "keys", "vals", "stream"]
    assert [p for p, _ in _abi.PROTOTYPES["segmm_store_index"]] == ["keys", "n", "ws", "ws_bytes", "out_keys", "out_rows", "n_unique", "stream"]
    assert L.segmm_abi_version() == H.ABI_VERSION == _abi.ABI_VERSION == 30
    # the entry points that existed keep their argument lists
    assert len(H.SIGNATURES["segmm_store_lookup"]) == 18 and len(H.SIGNATURES["segmm_store_head"]) == 12 and len(H.SIGNATURES["segmm_copy_bytes"]) == 4


def test_generated_tables_are_not_stale():
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_cmd_dispatch.py"), "--check"])


def test_store_append_refuses_bad_arguments_by_name():
    _, L = _L()
    u, p, t, lg, k, v = 4096, 8192, 12288, 16384, 20480, 24576          # never dereferenced: every call fails its argument check first

    def err(rc):
        assert rc != 0
        return L.segmm_last_error().decode()

    assert "overflow the capacity" in err(L.segmm_store_append(u, p, t, lg, 40, 5, 40, 6, 10, k, v, None))
    assert "overflow the capacity" in err(L.segmm_store_append(u, p, t, lg, 40, 5, 40, 2 ** 62, 10, k, v, None))
    assert "overflow the capacity" in err(L.segmm_store_append(u, p, t, lg, 40, 5, 40, 0, 4, k, v, None))
    assert "negative row0" in err(L.segmm_store_append(u, p, t, lg, 40, 5, 40, -1, 10, k, v, None))
    for args in ((None, p, t, lg, k, v), (u, None, t, lg, k, v), (u, p, None, lg, k, v), (u, p, t, None, k, v), (u, p, t, lg, None, v),
                 (u, p, t, lg, k, None)):
        assert "null pointer" in err(L.segmm_store_append(*args[:4], 40, 5, 40, 0, 10, *args[4:], None)), args
    assert "ld >= S" in err(L.segmm_store_append(u, p, t, lg, 39, 5, 40, 0, 10, k, v, None))
    assert "S >= 1" in err(L.segmm_store_append(u, p, t, lg, 1, 5, 0, 0, 10, k, v, None))
    assert "alignment" in err(L.segmm_store_append(u + 4, p, t, lg, 40, 5, 40, 0, 10, k, v, None))
    assert "alignment" in err(L.segmm_store_append(u, p, t, lg + 2, 40, 5, 40, 0, 10, k, v, None))
    # B == 0 inside the capacity: accepted, nothing launched (no device is touched)
    assert L.segmm_store_append(u, p, t, lg, 40, 0, 40, 10, 10, k, v, None) == 0


def test_store_index_refuses_bad_arguments_by_name():
    H, L = _L()
    keys, ws, ok, orow, nu = 4096, 8192, 12288, 16384, 20480
    nb = ctypes.c_int64(-1)

    def err(rc):
        assert rc != 0
        return L.segmm_last_error().decode()

    # the workspace helper: 0 bytes for no keys, 28 bytes a padded tuple + 4 per 1024 of them, a power of two of at least 2048 tuples
    assert L.segmm_store_index_ws(ctypes.byref(nb), 0) == 0 and nb.value == 0
    for n, np2 in ((1, 2048), (2048, 2048), (2049, 4096), (131075, 262144), (2 ** 24, 2 ** 24)):
        assert L.segmm_store_index_ws(ctypes.byref(nb), n) == 0 and nb.value == np2 * 28 + (np2 // 1024) * 4, n
    assert H.STORE_INDEX_MAX == 2 ** 24
    for n in (-1, 2 ** 24 + 1):
        msg = err(L.segmm_store_index_ws(ctypes.byref(nb), n))
        assert "store_index_ws" in msg and "finalize() without on_device" in msg
        msg = err(L.segmm_store_index(keys, n, ws, 1 << 40, ok, orow, nu, None))
        assert "store_index: n = %d" % n in msg and "finalize() without on_device" in msg
    assert "null pointer" in err(L.segmm_store_index_ws(None, 4))
    assert "n_unique" in err(L.segmm_store_index(keys, 4, ws, 1 << 20, ok, orow, None, None))
    for args in ((None, ws, ok, orow), (keys, None, ok, orow), (keys, ws, None, orow), (keys, ws, ok, None)):
        assert "null pointer" in err(L.segmm_store_index(args[0], 4, args[1], 1 << 20, args[2], args[3], nu, None)), args
    assert "alignment" in err(L.segmm_store_index(keys + 4, 4, ws, 1 << 20, ok, orow, nu, None))
    assert "alignment" in err(L.segmm_store_index(keys, 4, ws + 8, 1 << 20, ok, orow, nu, None))
    assert "need a workspace of %d bytes" % (2048 * 28 + 8) in err(L.segmm_store_index(keys, 4, ws, 2048 * 28, ok, orow, nu, None))


def test_recorder_takes_the_append_command_and_its_named_slots():
    """What dump_logits(recorded=True) rewrites per replay is found by parameter name in the recorded command."""
    H, _ = _L()
    rec = H.Recorder(111, 222)
    rec.mark(H.PHASE_STEP_TAIL)
    rec.call("segmm_store_append", (4096, 8192, 12288, 16384, 40, 5, 40, 7, 100, 20480, 24576, 111))
    (ph, arr), = rec.finish()
    c = arr[0]
    assert ph.n_cmds == 1 and c.op == H.op_ids()["segmm_store_append"] and c.stream == 0
    assert [H.cmd_arg(c, "segmm_store_append", p) for p in ("ld", "B", "S", "row0", "capacity", "keys", "vals")] == [40, 5, 40, 7, 100, 20480, 24576]
    assert rec.pslots[0] == [(0, 0), (0, 1), (0, 2), (0, 3), (0, 9), (0, 10)]          # row0 / capacity are integers: never re-based
    H.cmd_set_arg(c, "segmm_store_append", "row0", 2 ** 40)
    H.cmd_set_arg(c, "segmm_store_append", "keys", 28672)
    assert H.cmd_arg(c, "segmm_store_append", "row0") == 2 ** 40 and H.cmd_arg(c, "segmm_store_append", "keys") == 28672


def test_dump_logits_recorded_refusals_need_no_device():
    """The keyword exists and the refusals that come before any launch are worded by name."""
    import inspect

    import pytest
    import torch

    from segmminterest_amd.bridge import DeviceLogitStore
    from segmminterest_amd.eval_passes import EvalPasses
    assert inspect.signature(EvalPasses.dump_logits).parameters["recorded"].default is False
    assert inspect.signature(DeviceLogitStore.finalize).parameters["on_device"].default is False
    assert inspect.signature(DeviceLogitStore.__init__).parameters["capacity"].default is None

    class _Comm:
        active = True

    class _Tr(EvalPasses):
        comm, ema = _Comm(), None

    with pytest.raises(RuntimeError, match=r"dump_logits\(recorded=True\) is not supported under data parallelism \(an active DPComm\)"):
        _Tr().dump_logits([[]], recorded=True)
    st = DeviceLogitStore(S=4, device="cpu")
    with pytest.raises(RuntimeError, match="no preallocated tables"):
        st.append(torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), torch.zeros(1, 4))
