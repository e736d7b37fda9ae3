"""bench.py without a GPU: the launcher of `python bench.py --gpus N` (ranks started, failures reported, no JSON line from a failed
run) and the helpers that read the committed profiles."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _clean_env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(extra)
    return env


def test_own_launcher_reports_a_failed_rank():
    """no GPU here: every rank ends with "bench.py needs a GPU"; the launcher must come back with a non-zero status, say which
    rank failed, and print no JSON line"""
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "1"], cwd=REPO, env=_clean_env(),
                         capture_output=True, text=True, timeout=300)
    import torch
    if torch.cuda.is_available():   # (on a GPU box this test has nothing to say: tests/test_gpu_dist2.py runs the launcher for real)
        return
    assert out.returncode != 0
    assert "ended with status" in out.stderr and "needs a GPU" in out.stderr
    assert not [ln for ln in out.stdout.splitlines() if ln.startswith("{")]


def test_rank_count_must_match():
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "4", "--steps", "1"], cwd=REPO,
                         env=_clean_env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"), capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "must agree" in (out.stderr + out.stdout)


def test_committed_profiles_are_readable():
    """what bench.py quotes from profiles/<round>/: the kernel stats name the step's kernels (largest first) and the slice kernel's
    PMC summary has the fields the valu_by_kernel entry is made of"""
    sys.path.insert(0, REPO)
    import bench
    rows, path = bench.committed_kernel_stats("configs2")
    if rows is None:   # (no profile of this round committed yet)
        assert not os.path.exists(path)
        return
    names = [r[0] for r in rows]
    assert any(n.startswith("k_hash_bs") for n in names) and any(n.startswith("k_bs_select") for n in names)
    assert rows == sorted(rows, key=lambda r: -r[1]) and not any(n.startswith("k_synth") for n in names)
    sp = os.path.join(REPO, "profiles", bench.PROFILE_ROUND, "configs2_select_pmc.json")
    if os.path.exists(sp):
        pj = json.load(open(sp))
        assert pj["per_slice"]["valu"] > 0 and pj["per_slice"]["salu"] > 0 and pj["slices_per_launch"] > 0
        m = bench.select_valu_model(0.5, pj["slices_per_launch"])
        assert m is not None and ("stale" in m or 0 < m["frac_of_issue_bound"] < 1.5)


def test_scaling_fields_quote_the_same_workload_on_one_gpu():
    """the N-GPU line's efficiency = value / (N x the committed one-GPU line of the SAME workload and size); another size: no figure"""
    sys.path.insert(0, REPO)
    import bench
    f = bench.scaling_fields("configs2", 1000, 2, 3000.0, 5993199554.0)
    one = f["one_gpu_same_workload"]
    assert one and one["from"].startswith("profiles/r0") and one["from"].endswith("bench_configs2.json") and one["value"] > 1000
    assert abs(f["efficiency"] - 3000.0 / (2 * one["value"])) < 1e-3
    g = bench.scaling_fields("configs2", 1000, 2, 30.0, 1.0e7)   # (a test-sized run: no committed line of that size)
    assert g["efficiency"] is None and g["one_gpu_same_workload"] is None and "python bench.py --workload configs2" in g["efficiency_is"]


def test_own_launcher_stops_a_run_that_outlives_its_budget(tmp_path):
    """the launcher's wall-clock budget, without a GPU: a stand-in rank program that sleeps; rc 124, the ranks named, their stderr shown"""
    sys.path.insert(0, REPO)
    import bench
    prog = tmp_path / "sleeper.py"
    prog.write_text("import os, sys, time\nprint('rank', os.environ['RANK'], 'sleeping', file=sys.stderr, flush=True)\ntime.sleep(600)\n")
    code = ("import sys, os\nsys.path.insert(0, %r)\nimport bench\nbench.__file__ = %r\nsys.argv = ['bench.py']\n"
            "os.environ['MXG_BENCH_BUDGET_S'] = '3'\nsys.exit(bench.launch_ranks(2))\n") % (REPO, str(prog))
    out = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=_clean_env(), capture_output=True, text=True, timeout=120)
    assert out.returncode == 124, out.stderr[-2000:]
    assert "still running after 3 s" in out.stderr and "[rank 1] rank 1 sleeping" in out.stderr and "[rank 0] rank 0 sleeping" in out.stderr


def test_exchange_beside_sketches_timeline():
    """the dry run's model of an exchange per assembly on one communication stream: an exchange starts when its assembly is sketched
    and the exchange in front of it has ended"""
    import bench
    f = bench.exchange_beside_sketches
    assert f([1.0, 1.0], [0.5, 0.5]) == 2.5                 # each hides under the next sketch; the last one is exposed
    assert f([1.0, 1.0], [3.0, 0.5]) == 4.5                 # the first is still travelling when the second is ready
    assert f([0.5, 0.5, 0.5, 0.5], [0.2] * 4) == 2.2        # four assemblies: only the last exchange shows
    assert f([1.0], [0.7]) == 1.7 and f([], []) == 0.0
    # never better than everything behind the sketches, never worse than that either
    import itertools
    for sk, se in itertools.product([[0.3, 0.9, 0.1], [1.0, 1.0, 1.0]], [[0.5, 0.1, 0.8], [2.0, 2.0, 2.0]]):
        assert max(sum(sk) + se[-1], sk[0] + sum(se)) - 1e-12 <= f(sk, se) <= sum(sk) + sum(se) + 1e-12


class _FakeEngine:
    """what dump_outputs reads of an MxEngine after a step: get_sketch per assembly, get_graph (seeded arrays of bench-like sizes)"""

    def __init__(self, seed, n_mx=(300_000, 250_000), nv=200_000, ne=190_000):
        import numpy as np
        rng = np.random.default_rng(seed)
        self.sk = []
        for n in n_mx:
            rec_first = np.concatenate([[0], np.sort(rng.integers(0, n, 999)), [n]]).astype(np.uint64)
            self.sk.append({"out_hash": rng.integers(0, 2**64 - 1, n, dtype=np.uint64, endpoint=True),
                            "pos": rng.integers(0, 2**28, n, dtype=np.uint32), "record": rng.integers(0, 1000, n, dtype=np.uint32),
                            "forward": rng.integers(0, 2, n, dtype=np.uint8), "record_first": rec_first})
        A = len(n_mx)
        self.g = {"n_assemblies": A, "vertex_hash": rng.integers(0, 2**64 - 1, nv, dtype=np.uint64, endpoint=True),
                  "vertex_pos": rng.integers(0, 2**28, (A, nv), dtype=np.uint32), "vertex_record": rng.integers(0, 1000, (A, nv), dtype=np.uint32),
                  "edge_u": rng.integers(0, nv, ne, dtype=np.uint32), "edge_v": rng.integers(0, nv, ne, dtype=np.uint32),
                  "edge_support": rng.integers(1, 4, ne, dtype=np.uint32), "edge_weight": rng.random(ne) * 3}

    @property
    def n_assemblies(self):   # (a property, as MxEngine's)
        return len(self.sk)

    def get_sketch(self, a):
        return self.sk[a]

    def get_graph(self):
        return self.g


def test_dump_outputs_float_files_exact_sampled_and_repeatable(tmp_path):
    """--dump-outputs: float32/float64 .npy files only, under 64 MB together, the same files for the same outputs, sampled arrays
    taken at the written indices, and 64-bit hashes exact through their two halves"""
    import numpy as np
    sys.path.insert(0, REPO)
    import bench
    # (eight assemblies: more columns than DUMP_SAMPLE entries each fit in 64 MB, the sample shrinks)
    for n_mx in ((300_000, 250_000), (300_000,) * 4, (120_000,) * 8):
        eng = _FakeEngine(7, n_mx)
        d1, d2 = tmp_path / f"a{len(n_mx)}", tmp_path / f"b{len(n_mx)}"
        names = bench.dump_outputs(eng, str(d1))
        assert names == bench.dump_outputs(_FakeEngine(7, n_mx), str(d2))
        files = sorted(os.listdir(d1))
        assert files == sorted(n + ".npy" for n in names) and "counts.npy" in files
        total = 0
        for f in files:
            a, b = np.load(d1 / f), np.load(d2 / f)
            assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), f
            total += os.path.getsize(d1 / f)
        assert total <= 64 << 20
        c = np.load(d1 / "counts.npy")
        assert c.tolist() == list(n_mx) + [200_000, 190_000]
        idx = np.load(d1 / "sketch0_index.npy").astype(np.int64)
        assert 0 < len(idx) < n_mx[0] and np.all(np.diff(idx) > 0)
        assert (len(idx) < bench.DUMP_SAMPLE) == (len(n_mx) == 8) and len(np.load(d1 / "graph_edge_index.npy")) == len(idx)
        h = eng.sk[0]["out_hash"][idx]
        hi, lo = np.load(d1 / "sketch0_hash_hi.npy"), np.load(d1 / "sketch0_hash_lo.npy")
        assert np.array_equal((hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64), h)
        assert np.array_equal(np.load(d1 / "sketch0_pos.npy"), eng.sk[0]["pos"][idx].astype(np.float64))
        assert np.load(d1 / "graph_vertex_pos.npy").shape == (len(n_mx), len(np.load(d1 / "graph_vertex_index.npy")))
        assert np.array_equal(np.load(d1 / "sketch0_record_first.npy"), eng.sk[0]["record_first"].astype(np.float64))   # (short: whole)
    # other outputs, other files
    bench.dump_outputs(_FakeEngine(8), str(tmp_path / "c"))
    assert not np.array_equal(np.load(tmp_path / "c" / "sketch0_hash_lo.npy"), np.load(tmp_path / "a2" / "sketch0_hash_lo.npy"))


def test_plain_and_full_options():
    """--full and --dump-outputs are options of bench.py; --dump-outputs is refused where there is no one-GPU step to dump"""
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--help"], cwd=REPO, env=_clean_env(),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--full" in out.stdout and "--dump-outputs" in out.stdout
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--dump-outputs", "x"], cwd=REPO,
                         env=_clean_env(), capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "--dump-outputs" in out.stderr and not os.path.exists(os.path.join(REPO, "x"))
