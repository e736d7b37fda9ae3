"""GPU tests of the BGZF writer: text deflated on the device into BGZF members (ntjoin_amd/csrc/bgzf_deflate.hip, the coder of
bgzf_deflate.h), through mxg_bgzf_write and through mxg_write_scaffolds with MXG_SCAF_BGZF.

The witness that the device deflated a file is the line "[mxg] bgzf_deflate members=... bytes_in=... bytes_out=... stored=... ms=..."
that MXG_DEBUG_IO=1 prints when, and only when, it did.  What a file must be: byte for byte the file the stand-alone CPU program
(tests/_bgzf_deflate_host.py: the same header compiled for the host) writes for the same text and payload size, and a gzip file of
the text.

 1. mxg_bgzf_write at text sizes around one, two and three members, over the payload kinds of tests/test_bgzf_deflate_cpu.py;
 2. MXG_BGZF_PAYLOAD 1, 7, 255, 256, 4096 on a 20 kB text: a thread's share is 255 bytes, so these put partial words at thread
    borders, payloads shorter than one share and members of one symbol through the kernel;
 3. the scaffold cases of tests/test_gpu_scaffolds.py with MXG_SCAF_BGZF: the decompressed files, the BED, the strips and the counts
    are the plain call's; small windows and small members give the bytes of one window;
 4. the compressed scaffolds go back in through add_fasta on the device inflate route and sketch to the same minimizers;
 5. without the flag nothing changes and no witness line appears;
 6. the compressed file into a FIFO, in several windows: the bytes of the regular file."""
import glob
import gzip
import os
import random
import re

import numpy as np
import pytest

from ntjoin_amd.engine import MxEngine
from tests import _bgzf, _bgzf_deflate_host as host, _fifo, _oracle, _scaffold_cases as cases
from tests.test_bgzf_deflate_cpu import P_MAX, check_file, deep_text, fibonacci_text

pytestmark = pytest.mark.gpu

WITNESS = re.compile(r"\[mxg\] bgzf_deflate members=(\d+) bytes_in=(\d+) bytes_out=(\d+) stored=(\d+) ms=[0-9.]+\n")
INFLATE = re.compile(r"\[mxg\] bgzf_inflate members=(\d+) bytes_in=(\d+) bytes_out=(\d+) ms=[0-9.]+\n")
NAMES = ("MXG_DEBUG_IO", "MXG_BGZF_PAYLOAD", "MXG_SCAF_WIN", "MXG_HOST_INGEST")
SIZES = [0, 1, P_MAX - 1, P_MAX, P_MAX + 1, 2 * P_MAX, 3 * P_MAX + 17]
GOLDENS = sorted(glob.glob(os.path.join(cases.GOLDEN, "scaffolds", "*.json")))


@pytest.fixture
def env():
    saved = {k: os.environ.get(k) for k in NAMES}
    for k in NAMES:
        os.environ.pop(k, None)
    os.environ["MXG_DEBUG_IO"] = "1"
    yield os.environ
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host.build(tmp_path_factory.mktemp("bgzf_deflate_host"), ["-O2"])


@pytest.fixture(scope="module")
def kinds():
    "the CPU test's payload kinds, each long enough for the largest size (made once, never changed)"
    rng = random.Random(7)
    need = max(SIZES)

    def cycled(b):
        return (b * (need // len(b) + 1))[:need]
    return {"same": b"N" * need,
            "acgt": bytes(rng.choice(b"ACGT") for _ in range(need)),
            "fasta": _bgzf.shapes_fasta()[300_000:300_000 + need],   # (upper case, then lower case: two codes in a member)
            "all256": cycled(bytes(range(256))),
            "random": rng.randbytes(need),
            "fibonacci": cycled(fibonacci_text()),
            "deep": cycled(deep_text())}


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


def write_and_check(eng, capfd, program, tmp_path, name, text, payload):
    "mxg_bgzf_write of `text` -> the file's bytes, checked against the CPU program's file, gzip and the witness line"
    path = str(tmp_path / (name + ".dev.gz"))
    capfd.readouterr()
    eng.bgzf_write(text, path)
    err = capfd.readouterr().err
    got = read(path)
    want, info = host.deflate(program, payload, text, tmp_path, name)
    assert got == want, (name, len(text), payload, len(got), len(want))
    assert gzip.decompress(got) == text, name
    m = WITNESS.search(err)
    assert m, err
    assert [int(g) for g in m.groups()] == [info["members"], len(text), len(got), info["stored"]], (name, m.group(0), info)
    return got, info


@pytest.mark.parametrize("size", SIZES)
def test_bgzf_write_equals_the_cpu_program(size, env, capfd, program, kinds, tmp_path):
    with MxEngine(k=32, w=100) as eng:
        for name, text in kinds.items():
            got, info = write_and_check(eng, capfd, program, tmp_path, name, text[:size], P_MAX)
            if size and (name in ("random", "all256") or size == 1):   # eight bits a byte, or a header larger than the text
                assert info["stored"] == info["members"], (name, info)
            elif size:                                                  # (a last member of 1 or 17 bytes may be a stored one)
                assert info["stored"] <= (1 if size % P_MAX in (1, 17) else 0), (name, info)
            else:
                assert got == _bgzf.EOF_MARKER
        assert "MXG_BGZF_PAYLOAD" not in eng.knobs()


@pytest.mark.parametrize("payload", [1, 7, 255, 256, 4096])
def test_small_payloads(payload, env, capfd, program, tmp_path):
    text = _bgzf.shapes_fasta()[325_000:345_000]   # 20 kB: the end of a record, a header line, lower case
    env["MXG_BGZF_PAYLOAD"] = str(payload)
    with MxEngine(k=32, w=100) as eng:
        got, info = write_and_check(eng, capfd, program, tmp_path, f"p{payload}", text, payload)
        assert f"MXG_BGZF_PAYLOAD={payload}" in eng.knobs()
    check_file(got, text, payload, f"p{payload}")
    assert info["members"] == (len(text) + payload - 1) // payload


def scaffold_inputs(kind, which, tmp_path):
    "-> (records, paths, overlap_gap, fold, FASTA path) of a fuzz seed or a golden of tests/test_gpu_scaffolds.py"
    if kind == "fuzz":
        case = cases.fuzz_case(which)
        fasta = str(tmp_path / "t.fa")
        cases.write_fasta(fasta, case["records"], case["width"], case["final_newline"])
        return case["records"], case["paths"], case["overlap_gap"], case["fold"], fasta
    doc, fasta = cases.load_golden(which)
    return _oracle.read_fasta(fasta), cases.golden_nodes(doc), doc["meta"]["overlap_gap"] if doc["meta"]["overlap"] else None, False, fasta


def scaffolds(eng, a, records, paths, out, overlap_gap, fold, bgzf):
    index = {rid: r for r, (rid, _) in enumerate(records)}
    rows, first = cases.rows_of(paths, index)
    names = [str(out) + s for s in (".assigned.fa", ".unassigned.fa", ".bed")]
    res = eng.write_scaffolds(a, rows, first, overlap_gap=overlap_gap, fold_case=fold, assigned=names[0], unassigned=names[1], bed=names[2],
                              bgzf=bgzf)
    lead_u, tail_u = eng.scaffold_strips()
    return ([read(n) for n in names], (res["lead_strip"].tolist(), res["tail_strip"].tolist(), res["n_unassigned"], lead_u.tolist(), tail_u.tolist()))


SCAF_CASES = [("fuzz", s) for s in cases.FUZZ_SEEDS] + [("golden", g) for g in GOLDENS]
SCAF_IDS = [f"fuzz{s}" for s in cases.FUZZ_SEEDS] + [os.path.basename(g)[:-5] for g in GOLDENS]


@pytest.mark.parametrize("kind,which", SCAF_CASES, ids=SCAF_IDS)
def test_scaffolds_compressed_equal_plain(kind, which, env, capfd, program, tmp_path):
    records, paths, gap, fold, fasta = scaffold_inputs(kind, which, tmp_path)
    k, w = (15, 10) if kind == "fuzz" else (32, 100)
    with MxEngine(k=k, w=w) as eng:
        a = eng.add_fasta("t", 1.0, fasta)
        capfd.readouterr()
        plain, res_plain = scaffolds(eng, a, records, paths, tmp_path / "plain", gap, fold, False)
        assert not WITNESS.search(capfd.readouterr().err)           # the plain route: no deflate
        comp, res_comp = scaffolds(eng, a, records, paths, tmp_path / "comp", gap, fold, True)
        lines = WITNESS.findall(capfd.readouterr().err)
        again, _ = scaffolds(eng, a, records, paths, tmp_path / "again", gap, fold, False)
    assert again == plain                                           # ... and unchanged by the compressed call before it
    assert res_comp == res_plain and comp[2] == plain[2]            # strips, counts, the BED
    assert len(lines) == 2                                          # one line per FASTA
    for f in (0, 1):
        assert gzip.decompress(comp[f]) == plain[f]
        want, info = host.deflate(program, P_MAX, plain[f], tmp_path, f"want{f}")
        assert comp[f] == want
        assert [int(g) for g in lines[f]] == [info["members"], len(plain[f]), len(comp[f]), info["stored"]]
    # many windows of many members: the same bytes as one window at that payload size
    env["MXG_BGZF_PAYLOAD"] = "1000"
    got = []
    for win in ("8192", None):
        if win:
            env["MXG_SCAF_WIN"] = win
        else:
            env.pop("MXG_SCAF_WIN", None)
        with MxEngine(k=k, w=w) as eng:
            a = eng.add_fasta("t", 1.0, fasta)
            files, res = scaffolds(eng, a, records, paths, tmp_path / f"w{win}", gap, fold, True)
            assert "MXG_BGZF_PAYLOAD=1000" in eng.knobs() and (win is None or f"MXG_SCAF_WIN={win}" in eng.knobs())
        assert res == res_plain and files[2] == plain[2]
        got.append(files[:2])
    assert got[0] == got[1]
    for f in (0, 1):
        want, _ = host.deflate(program, 1000, plain[f], tmp_path, f"want1000_{f}")
        assert got[0][f] == want


def test_a_fifo_takes_the_compressed_windows_in_order(env, tmp_path):
    """the assigned FASTA with MXG_SCAF_BGZF into a FIFO (no offsets: the windows' members and the end-of-file marker are written in
    order at the descriptor's own position): the bytes of the same call into a regular file.  Members of 4096 bytes make a window of
    one emit tile a whole number of members, so the knob gives the fuzz case's assigned file three windows."""
    records, paths, gap, fold, fasta = scaffold_inputs("fuzz", 46, tmp_path)
    index = {rid: r for r, (rid, _) in enumerate(records)}
    rows, first = cases.rows_of(paths, index)
    env["MXG_BGZF_PAYLOAD"] = "4096"
    env["MXG_SCAF_WIN"] = str(cases.TILE)
    with MxEngine(k=15, w=10) as eng:
        a = eng.add_fasta("t", 1.0, fasta)
        plain, _ = scaffolds(eng, a, records, paths, tmp_path / "plain", gap, fold, False)
        want, _ = scaffolds(eng, a, records, paths, tmp_path / "comp", gap, fold, True)
        assert len(plain[0]) > 2 * cases.TILE and gzip.decompress(want[0]) == plain[0]  # three windows
        assert "MXG_BGZF_PAYLOAD=4096" in eng.knobs() and f"MXG_SCAF_WIN={cases.TILE}" in eng.knobs()
        names = [str(tmp_path / f) for f in ("f.assigned.fa.gz", "f.unassigned.fa.gz", "f.bed")]
        with _fifo.fifo_reader(names[0], len(want[0])) as drain:
            eng.write_scaffolds(a, rows, first, overlap_gap=gap, fold_case=fold, assigned=names[0], unassigned=names[1], bed=names[2], bgzf=True)
            assert drain() == want[0]
        assert [read(n) for n in names[1:]] == want[1:]


def test_round_trip_through_the_device_inflate_route(env, capfd, tmp_path):
    "the compressed assigned file is the next round's target: inflated on the device, the same minimizers as the plain file"
    records, paths, gap, fold, fasta = scaffold_inputs("fuzz", 13, tmp_path)
    with MxEngine(k=15, w=10) as eng:
        a = eng.add_fasta("t", 1.0, fasta)
        plain, _ = scaffolds(eng, a, records, paths, tmp_path / "plain", gap, fold, False)
        scaffolds(eng, a, records, paths, tmp_path / "comp", gap, fold, True)
    assert len(plain[0]) > 40_000
    gz = str(tmp_path / "comp.assigned.fa.gz")
    os.rename(str(tmp_path / "comp.assigned.fa"), gz)
    sk = []
    for path in (str(tmp_path / "plain.assigned.fa"), gz):
        capfd.readouterr()
        with MxEngine(k=15, w=10) as eng:
            a = eng.add_fasta("x", 1.0, path)
            err = capfd.readouterr().err
            eng.sketch()
            s = eng.get_sketch(a)
            sk.append({key: np.array(s[key]).copy() for key in ("out_hash", "pos", "record_first")})
        m = INFLATE.search(err)
        assert bool(m) == path.endswith(".gz"), err
        if m:
            assert int(m.group(3)) == len(plain[0])
    assert len(sk[0]["out_hash"]) > 100
    for key in sk[0]:
        assert np.array_equal(sk[0][key], sk[1][key]), key
