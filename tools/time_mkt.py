"""time the --mkt statistics (csrc/mk.hip): python tools/time_mkt.py
  (1) mxg_mk_stats on one run of 2^24 random values        (2) on 2^20 runs of random length 2..64
  (3) mxg_path_segments_mk after find_paths on a configs[2]-shaped pair (3 Gbp reference of 24 records + derived target, w=1000)
Each number is the best of 5 calls of the C entry point (host arrays in, results on the host: (1) and (2) include the copy of
the values to the device).  A CPU count in numpy (vectorised bottom-up merge, O(n log^2 n)) is printed beside (1)."""
import ctypes as C
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from ntjoin_amd import synth  # noqa: E402
from ntjoin_amd.engine import MxEngine  # noqa: E402


def best_ms(fn, reps=5):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return min(out)


def cpu_merge_count(x):
    x = np.asarray(x, dtype=np.int64)
    n = len(x)
    size = 1 << (n - 1).bit_length()
    big = int(x.max()) + 1
    a = np.concatenate([x, np.full(size - n, big, dtype=np.int64)])
    s, w = 0, 1
    while w < size:
        blocks = a.reshape(-1, 2, w)
        rows = np.arange(len(blocks), dtype=np.int64)[:, None]
        left = (blocks[:, 0, :] + rows * (big + 1)).ravel()
        right = blocks[:, 1, :] + rows * (big + 1)
        lb = np.searchsorted(left, right, "left") - rows * w
        ub = np.searchsorted(left, right, "right") - rows * w
        s += int((lb - (w - ub)).sum())
        a = np.sort(blocks.reshape(-1, 2 * w), axis=1).ravel()
        w *= 2
    return s - n * (size - n)


def call(eng, x, first, s, t):
    rc = eng._lib.mxg_mk_stats(eng._h, x.ctypes.data, first.ctypes.data, len(first) - 1, s.ctypes.data, t.ctypes.data)
    assert rc == 0, eng._lib.mxg_last_error(eng._h)


rng = np.random.default_rng(1)
with MxEngine(k=32, w=1000) as eng:
    x = rng.integers(0, 2 ** 32, size=1 << 24, dtype=np.uint64).astype(np.uint32)
    first = np.array([0, len(x)], dtype=np.uint64)
    s, t = np.zeros(1, np.int64), np.zeros(1, np.uint64)
    ms = best_ms(lambda: call(eng, x, first, s, t))
    t0 = time.perf_counter()
    s_cpu = cpu_merge_count(x)
    ms_cpu = (time.perf_counter() - t0) * 1e3
    assert int(s[0]) == s_cpu
    print(f"one run of 2^24 random values: mxg_mk_stats {ms:.2f} ms (s = {int(s[0])}); CPU numpy merge count {ms_cpu:.0f} ms")

    lens = rng.integers(2, 65, size=1 << 20)
    first = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    x = rng.integers(0, 2 ** 32, size=int(first[-1]), dtype=np.uint64).astype(np.uint32)
    s, t = np.zeros(len(lens), np.int64), np.zeros(len(lens), np.uint64)
    ms = best_ms(lambda: call(eng, x, first, s, t))
    print(f"2^20 runs of 2..64 values ({len(x)} values): mxg_mk_stats {ms:.2f} ms")

with MxEngine(k=32, w=1000) as eng:
    cfg = synth.genome_config(3_000_000_000, 24, seed=1, min_len=3000, max_len=600_000)
    keep = []
    for which, name, weight in (("ref", "ref", 2.0), ("tgt", "tgt", 1.0)):
        segs, n_words = cfg[which + "_segs"], cfg[which + "_words"]
        d = synth.fill_device(segs, n_words, cfg["seed"], cfg["sub_seed"], synth.SUB_PER_65536 if which == "tgt" else 0)
        eng.add_packed_device(name, weight, d.data_ptr(), segs[:, 0], segs[:, 2], keepalive=d)
    eng.sketch(-2)
    eng.build_graph()
    found = eng.find_paths(2)
    seg = eng.path_segments(1)
    ps, pt, pn = C.POINTER(C.c_int64)(), C.POINTER(C.c_uint64)(), C.c_uint64()
    ms = best_ms(lambda: eng._lib.mxg_path_segments_mk(eng._h, 1, C.byref(ps), C.byref(pt), C.byref(pn)))
    mk = eng.path_segments_mk(1)
    n = seg["n"].astype(np.int64)
    not_mono = int(((seg["inc"] != n - 1) & (seg["dec"] != n - 1) & (n > 1)).sum())
    print(f"configs[2] pair, -n 2: {len(found)} paths, {int(n.sum())} path vertices, {len(n)} runs (longest {int(n.max())}, "
          f"{not_mono} not strictly monotone): mxg_path_segments_mk {ms:.2f} ms")
