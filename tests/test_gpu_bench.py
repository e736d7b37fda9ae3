"""bench.py --gpus 1 at a test size: a plain run times exactly --steps steps, prints only the line of the timed steps and, with
--dump-outputs, writes what the last step computed -- the same files from run to run (the inputs are seeded); --full still
adds the side measurements."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--workload", "configs1", "--mbp", "5", "--warmup", "1"]
SIDE = ("kernels", "one_shot", "roofline_by_kernel", "cpu_baseline", "end_to_end", "repeat_rich", "other_k")


def _bench(args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1"] + args, cwd=REPO, env=env,
                         capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_dumps_what_the_step_computed(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    d1 = _bench(SMALL + ["--steps", "3", "--dump-outputs", str(a)])
    d2 = _bench(SMALL + ["--steps", "2", "--dump-outputs", str(b)])
    assert d1["steps"] == 3 and d2["steps"] == 2
    # the library's own count over the timed region (reset before it): candidates / --steps is the same for 3 and 2 steps of the
    # same seeded input only if each run timed as many steps as it was told
    c1, c2 = d1["fallbacks"]["candidates_per_step"], d2["fallbacks"]["candidates_per_step"]
    assert c1 == c2 > 0, (c1, c2)
    for d in (d1, d2):
        assert d["unit"] == "Gbp/s" and d["higher_is_better"] is True and d["dtype"] == "u64" and "Gbp/s" in d["metric"]
        assert d["value"] > 0 and d["ms_per_step"] > 0 and not any(k in d for k in SIDE)
    files = sorted(os.listdir(a))
    assert files and files == sorted(os.listdir(b))
    assert sum(os.path.getsize(a / f) for f in files) <= 64 << 20
    for f in files:
        x, y = np.load(a / f), np.load(b / f)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), f
    counts = np.load(a / "counts.npy").astype(np.int64).tolist()
    c = d1["config"]
    assert sum(counts[:-2]) == c["minimizers"] and counts[-2:] == [c["vertices"], c["edges"]] and c["edges"] > 0


@pytest.mark.gpu
def test_full_run_keeps_the_side_measurements():
    d = _bench(SMALL + ["--steps", "2", "--full", "--cpu-seconds", "2"])
    assert d["steps"] == 2 and d["value"] > 0
    for k in ("kernels", "one_shot", "roofline_by_kernel", "cpu_baseline", "end_to_end"):
        assert d.get(k), k
    assert d["parity_counts_match_cpu"] is True   # (5 Mbp: the CPU baseline sketches the whole workload)
