"""bench.py on the GPU: --steps sets the number of timed steps, --dump-outputs writes what the last of them computed, and --full
adds its legs without changing either."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import ROOT

TOY_SHAPE = ["--dim", "64", "--heads", "4", "--lt", "12", "--batch", "32", "--batches", "2", "--warmup", "1"]
TOY = TOY_SHAPE + ["--no-cpu-baseline", "--no-f32-engine", "--no-host-fed", "--no-probe", "--no-index-leg"]
FULL_ONLY = {"roofline", "roofline_attention", "value_index_input", "index_input", "cpu_baseline", "value_f32_engine", "host_fed"}


def _bench(out_dir, *extra, base=TOY):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + base + list(extra) + ["--dump-outputs", str(out_dir)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.count("\n") == 1, p.stdout
    return json.loads(p.stdout), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


@pytest.mark.gpu
def test_bench_steps_are_the_timed_steps_and_the_dump_is_the_last_one(tmp_path):
    """The same 4 timed steps in one window or in two leave bitwise the same outputs and parameters (seeded inputs, ordered
    reductions); a fifth timed step moves the parameters.  loss.npy is the loss the line reports for the last timed step."""
    r4, a = _bench(tmp_path / "a", "--steps", "4")
    r4w, b = _bench(tmp_path / "b", "--steps", "4", "--windows", "2")
    r5, c = _bench(tmp_path / "c", "--steps", "5")
    assert (r4["steps"], r4["windows"], r4w["windows"], r5["steps"]) == (4, 1, 2, 5)
    assert {"loss", "logits"} <= set(a) and any(k.startswith("param.") for k in a)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64e6
    assert float(a["loss"]) == pytest.approx(r4["config"]["final_loss"], abs=1e-6)
    assert a.keys() == b.keys() == c.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert any(not np.array_equal(a[k], c[k]) for k in a if k.startswith("param."))


@pytest.mark.gpu
def test_bench_full_adds_its_legs_and_leaves_the_timed_steps_alone(tmp_path):
    """A plain run prints none of the --full fields; --full (every leg on) prints them, and its last timed step computed bitwise
    what the plain run's did: the event pairs ride on steps a plain run takes too, and the legs run after the dump."""
    plain, a = _bench(tmp_path / "plain", "--steps", "3", base=TOY_SHAPE)
    full, b = _bench(tmp_path / "full", "--steps", "3", "--full", base=TOY_SHAPE)
    assert not FULL_ONLY & set(plain) and plain["config"]["replicas_identical"] is None
    assert FULL_ONLY <= set(full), sorted(FULL_ONLY - set(full))
    assert full["roofline"]["launches"] > 0 and full["cpu_baseline"]["value"] > 0
    assert plain["config"]["final_loss"] == full["config"]["final_loss"]
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
