"""``bench.py --dump-outputs DIR`` without a GPU: the single-GPU job on the host-emulated kernel library (``--cpu-emulator``) writes
what its last timed step computed as float32 ``.npy`` files, the same arrays on every run with the same arguments, and ``--steps``
is the number of timed steps the line's ``ms_per_step`` is taken over."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("params_online", "params_target", "adam_exp_avg", "adam_exp_avg_sq", "loss", "grad_norm", "priority")


def _run(out_dir, steps):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import simlib
    env = dict(os.environ, MORL_HIP_LIB=simlib.build_sim(), MORL_LAZY_MIN_ROWS="0", MORL_BF_MIN_ROWS="0", OMP_NUM_THREADS="1")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--cpu-emulator", "--steps", str(steps), "--warmup", "1",
           "--batch", "8", "--weights", "4", "--buffer-fill", "200", "--no-cpu-baseline", "--no-ramp-record",
           "--no-sustained-record", "--no-exact-record", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {n: np.load(os.path.join(out_dir, n + ".npy")) for n in NAMES}


def test_dump_outputs_are_the_last_timed_step_and_repeat(tmp_path):
    d1, o1 = _run(tmp_path / "a", 2)
    d2, o2 = _run(tmp_path / "b", 2)
    d3, o3 = _run(tmp_path / "c", 3)
    assert d1["steps"] == 2 and d3["steps"] == 3 and d1["ms_per_step"] > 0 and d3["ms_per_step"] > 0
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in NAMES)
    for n in NAMES:
        assert o1[n].dtype == np.float32 and o1[n].size > 0, n
        assert np.array_equal(o1[n], o2[n]), n                      # same arguments: same inputs, same outputs
    assert sum(v.nbytes for v in o1.values()) <= 64 << 20
    assert o1["params_online"].shape == o1["adam_exp_avg"].shape == o1["params_target"].shape
    assert o1["priority"].shape == (8,)
    assert float(o1["loss"][0]) == d1["last_loss"]                 # the loss the line reports is the dumped step's
    assert np.all(np.isfinite(o1["params_online"])) and np.all(o1["priority"] > 0)
    # one more timed step moved the parameters on
    assert not np.array_equal(o1["params_online"], o3["params_online"])
