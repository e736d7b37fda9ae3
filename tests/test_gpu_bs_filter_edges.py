"""GPU tests of the bit-sliced ring filter's compare at the ends of its range and of record borders at the borders of its geometry:

  * the generated kernel against the direct ring formula (the standalone binary of tests/test_gpu_bs.py) at the thresholds next
    to the ends: tt = 1, and tt = 2^14 - 2, from which on every sum passes ([-2, tt] is then the whole range; a stream generated
    with --carry-in compares St + 1 with min(tt + 1, 2^14 - 1) there -- the binary states the set of the stream it was built with);
  * one sketch through the k = 32 route against the CPU oracle on three records of about 200 kbp whose borders fall on a chunk
    border of the filter (65 536 positions), inside a strip (16 positions into its 32) and on a lane border (1024 positions):
    records start on multiples of 16 bases in the packed assembly.
"""
import os
import random
import subprocess

import pytest

from tests.test_gpu_scale_paths import _check

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("tt", [1, 16382])
def test_filter_kernel_at_the_thresholds_next_to_the_ends(tt):
    exe = os.path.join(REPO, "ntjoin_amd", "bin", "bs_check")
    assert os.path.exists(exe), "ntjoin_amd/bin/bs_check missing: run __graft_entry__.build()"
    r = subprocess.run([exe, "1", str(tt)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "verify: ok" in r.stdout


def _border_records():
    """record 0 ends five bases short of the first chunk border, so record 1 (two chunks and 777 bases) starts on it; record 2
    then starts 16 positions into a strip and ends on a lane border"""
    rng = random.Random(2032)
    lengths = [65536 - 5, 131072 + 777, 2288]
    off, offs = 0, []
    for n in lengths:
        offs.append(off)
        off += (n + 15) // 16 * 16
    assert offs[1] == 65536 and offs[2] % 32 == 16 and (offs[2] + lengths[2]) % 1024 == 0 and (offs[2] + lengths[2]) % 65536 != 0
    return [(f"r{i}", "".join(rng.choice("ACGT") for _ in range(n))) for i, n in enumerate(lengths)]


@pytest.mark.parametrize("w", [150, 1000])
def test_record_borders_on_strip_lane_and_chunk_borders(oracle, w):
    saved = {k: os.environ.pop(k, None) for k in ("MXG_BS", "MXG_BS_SELECT", "MXG_SPARSE_S")}
    try:
        recs = _border_records()
        st = _check(oracle, recs, 32, w)
    finally:
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v
    assert st["bs_filter_bases"] == sum(len(s) for _, s in recs), "the k = 32 route did not run"
    assert st["candidates"] > 0
