"""GPU tests of the file route: FASTA text classified and packed ON THE DEVICE (ntjoin_amd/csrc/ingest.hip) and the TSV text
formatted ON THE DEVICE, against (a) the CPU oracle's own FASTA -> TSV driver (byte-identical files) and (b) the host parser /
host writer of the library (MXG_HOST_INGEST=1 / MXG_HOST_TSV=1).  Shapes that stress the text handling: CRLF line ends
(also across the 4 MiB read buffer of the host parser and across the device's 4096-byte tiles), lower case, N-runs,
IUPAC codes, ragged line lengths, no final newline, '>' inside header lines, empty records, thousands of tiny records.
The device parser's buffer of validity events at and beyond its capacity (MXG_INGEST_EV_CAP): files with a known number of changes
on both sides of the limit, a record with an invalid base every 50 to 200 bases, and the invalid-base intervals the overlap stage
reads behind the device parser, the host parser and the overflow's way to the host parser.

Which parser ran: neither mxg_stats nor mxg_knobs says so (knobs() lists MXG_INGEST_EV_CAP once the device parser has come as far
as its events, whether it then kept the file or handed it over).  The witness used here is the line "[mxg] load_fasta_device ..."
that MXG_DEBUG_IO=1 prints to stderr when, and only when, the device parser finished the file."""
import os
import random
import subprocess

import numpy as np
import pytest

from ntjoin_amd.engine import MxEngine
from tests import _oracle
from tests.conftest import BIN_DIR, REPO

pytestmark = pytest.mark.gpu


def _write_fasta(path, recs, width=60, eol="\n", ragged=None, final_newline=True):
    rng = random.Random(7)
    with open(path, "w", newline="") as fh:
        for i, (hdr, seq) in enumerate(recs):
            fh.write(">" + hdr + eol)
            p = 0
            while p < len(seq):
                wd = rng.randint(1, 2 * width) if ragged else width
                last = p + wd >= len(seq) and i == len(recs) - 1
                fh.write(seq[p:p + wd] + ("" if last and not final_newline else eol))
                p += wd


def _seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _messy_records(seed):
    rng = random.Random(seed)
    recs = [("chr1 some comment > with a bracket", _seq(rng, 150_000)),
            ("lower", _seq(rng, 40_000).lower()),
            ("mixed\tcase", "".join(c.lower() if rng.random() < 0.3 else c for c in _seq(rng, 60_000))),
            ("empty", ""),
            ("tiny", "ACGTACGTAC"),
            ("withN", _seq(rng, 30_000) + "N" * 700 + _seq(rng, 25_000) + "n" * 3 + _seq(rng, 9_000)),
            ("iupac", _seq(rng, 20_000) + "RYKM" + _seq(rng, 20_000) + "-" + _seq(rng, 5_000)),
            ("rna", _seq(rng, 30_000, "ACGU")),
            ("startsN", "NNNN" + _seq(rng, 12_000) + "NN")]
    recs += [(f"frag{i}", _seq(rng, rng.randint(20, 2500))) for i in range(300)]
    recs.append(("last", _seq(rng, 70_000)))
    # an invalid base (N or an IUPAC letter, either case) every 50 to 200 bases over 300 kbp: about 2400 of them, twice as many
    # changes between valid and invalid inside the device parser's tiles (a generator of its own: the records above stay as they were)
    rng2 = random.Random(seed + 1000)
    s, p = list(_seq(rng2, 300_000)), 0
    while True:
        p += rng2.randint(50, 200)
        if p >= len(s):
            break
        s[p] = rng2.choice("NnRYKMSWBDHVrykm")
    recs.append(("scattered", "".join(s)))
    return recs


def _tsv_by_engine(fa, k, w, out, **env):
    saved = {k_: os.environ.get(k_) for k_ in env}
    os.environ.update(env)
    try:
        with MxEngine(k=k, w=w, threads=3) as eng:
            eng.add_fasta("x", 1.0, fa)
            eng.sketch()
            eng.write_tsv(0, out, with_pos=True, with_strand=False, with_seq=True)
            st = eng.stats()
    finally:
        for k_, v in saved.items():
            if v is None:
                os.environ.pop(k_, None)
            else:
                os.environ[k_] = v
    return st


@pytest.mark.parametrize("eol,ragged,final_nl", [("\n", False, True), ("\r\n", False, True), ("\n", True, False), ("\r\n", True, True)])
@pytest.mark.parametrize("k,w", [(32, 100), (15, 10)])
def test_device_route_equals_oracle_and_host_route(tmp_path, eol, ragged, final_nl, k, w):
    orc = _oracle.load()
    fa = str(tmp_path / "messy.fa")
    _write_fasta(fa, _messy_records(3), width=70, eol=eol, ragged=ragged, final_newline=final_nl)
    want = str(tmp_path / "oracle.tsv")
    orc.fasta_to_tsv(fa, want, k, w)
    dev, host = str(tmp_path / "dev.tsv"), str(tmp_path / "host.tsv")
    st_dev = _tsv_by_engine(fa, k, w, dev)
    st_host = _tsv_by_engine(fa, k, w, host, MXG_HOST_INGEST="1", MXG_HOST_TSV="1")
    assert open(dev, "rb").read() == open(want, "rb").read()
    assert open(host, "rb").read() == open(want, "rb").read()
    assert st_dev["bases"] == st_host["bases"] and st_dev["kmers"] == st_host["kmers"] and st_dev["minimizers"] > 500


def test_crlf_across_buffer_and_tile_borders(tmp_path):
    """a CRLF FASTA larger than the host parser's 4 MiB read buffer, with a line length that walks the "\\r\\n" pair over
    every alignment (a pair cut by the buffer border left the '\\r' in the sequence)"""
    orc = _oracle.load()
    rng = random.Random(5)
    recs = [("a", _seq(rng, 5_300_000)), ("b", _seq(rng, 3_100_000))]
    lf, crlf = str(tmp_path / "lf.fa"), str(tmp_path / "crlf.fa")
    _write_fasta(lf, recs, width=61)
    _write_fasta(crlf, recs, width=61, eol="\r\n")
    want = str(tmp_path / "want.tsv")
    orc.fasta_to_tsv(lf, want, 32, 1000)
    for tag, env in (("dev", {}), ("host", {"MXG_HOST_INGEST": "1", "MXG_HOST_TSV": "1"})):
        out = str(tmp_path / f"{tag}.tsv")
        _tsv_by_engine(crlf, 32, 1000, out, **env)
        assert open(out, "rb").read() == open(want, "rb").read(), tag


def test_cli_threads_and_strand_column(tmp_path):
    """`indexlr -t N` (reference ntJoin:205 passes -t $(t)): same bytes for any thread count, and with --strand / without --seq"""
    orc = _oracle.load()
    fa = str(tmp_path / "m.fa")
    _write_fasta(fa, _messy_records(9), width=80)
    exe = os.path.join(BIN_DIR, "indexlr")
    want = str(tmp_path / "want.tsv")
    orc.fasta_to_tsv(fa, want, 32, 100)
    for t in ("1", "4", "48"):
        out = subprocess.run([exe, "--seq", "--long", "--pos", "-k32", "-w100", f"-t{t}", fa], capture_output=True, check=True).stdout
        assert out == open(want, "rb").read(), t
    want2 = str(tmp_path / "want2.tsv")
    orc.fasta_to_tsv(fa, want2, 32, 100, pos=True, strand=True, seq=False)
    out = subprocess.run([exe, "--pos", "--strand", "-k", "32", "-w", "100", "-t", "2", "-o", str(tmp_path / "o.tsv"), fa], check=True)
    assert open(tmp_path / "o.tsv", "rb").read() == open(want2, "rb").read()


def test_tsv_of_packed_device_assembly_is_formatted_on_the_device(tmp_path, oracle):
    """no text anywhere (bases born packed in HBM): the k-mer column is decoded from the packed bases; several output windows"""
    from ntjoin_amd import synth
    cfg = synth.genome_config(40_000_000, 5, seed=4, min_len=2000, max_len=200_000)
    with MxEngine(k=32, w=20) as eng:   # w=20: ~4 M minimizers, > 250 MB of TSV text = several 64 MiB windows
        segs = cfg["tgt_segs"]
        d = synth.fill_device(segs, cfg["tgt_words"], cfg["seed"], cfg["sub_seed"], synth.SUB_PER_65536)
        eng.add_packed_device("t", 1.0, d.data_ptr(), segs[:, 0], segs[:, 2], keepalive=d)
        eng.sketch()
        out = str(tmp_path / "t.tsv")
        eng.write_tsv(0, out)
        sk = eng.get_sketch(0)
    assert os.path.getsize(out) > 3 * (64 << 20)
    first = sk["record_first"]
    with open(out, "rb") as fh:
        for r, line in enumerate(fh):
            rid, _, rest = line.rstrip(b"\n").partition(b"\t")
            assert rid == str(r).encode()
            lo, hi = int(first[r]), int(first[r + 1])
            if r % 97 == 0 or r < 3:   # every field of these records, the k-mers against the generator's numpy mirror
                ents = rest.split(b" ") if rest else []
                assert len(ents) == hi - lo
                codes = synth.segment_codes(segs[r], cfg["seed"], cfg["sub_seed"], synth.SUB_PER_65536)
                seq = synth.to_ascii(codes)
                for e, i in zip(ents, range(lo, hi)):
                    hsh, pos, kmer = e.split(b":")
                    assert int(hsh) == int(sk["out_hash"][i]) and int(pos) == int(sk["pos"][i])
                    assert kmer == seq[int(pos):int(pos) + 32]
            else:
                assert rest.count(b" ") + (1 if rest else 0) == hi - lo
    assert r == len(segs) - 1


def test_gzip_fasta_input(tmp_path):
    """`.gz` input (indexlr reads both; SURVEY.md 8b B1 lists it as optional): same TSV as the plain file, through the CLI and
    through the sub-record split loader"""
    import gzip
    orc = _oracle.load()
    fa = str(tmp_path / "m.fa")
    _write_fasta(fa, _messy_records(11), width=60)
    gz = fa + ".gz"
    with open(fa, "rb") as src, gzip.open(gz, "wb") as dst:
        dst.write(src.read())
    want = str(tmp_path / "want.tsv")
    orc.fasta_to_tsv(fa, want, 32, 100)
    exe = os.path.join(BIN_DIR, "indexlr")
    out = subprocess.run([exe, "--seq", "--long", "--pos", "-k32", "-w100", "-t2", gz], capture_output=True, check=True).stdout
    assert out == open(want, "rb").read()
    parts = []
    for s in range(3):
        with MxEngine(k=32, w=100) as eng:
            eng.add_fasta_split("x", 1.0, gz, s, 3)
            eng.sketch()
            parts.append(eng.get_sketch(0))
    with MxEngine(k=32, w=100) as eng:
        eng.add_fasta("x", 1.0, fa)
        eng.sketch()
        whole = eng.get_sketch(0)
    for key in ("out_hash", "pos", "record"):
        assert np.array_equal(np.concatenate([p[key] for p in parts]), whole[key]), key


def test_fuzz_fasta_text_three_ways(tmp_path):
    """random FASTA text -- line widths from 1 up, LF or CRLF, with or without the final line end, empty and tiny records next to
    records of several device tiles, lower case, N runs and IUPAC letters at random places, header lines with blanks, tabs and
    '>' -- through the device route, the host route and the oracle's own FASTA -> TSV driver: three byte-identical files"""
    orc = _oracle.load()
    trials = int(os.environ.get("MXG_FUZZ_TRIALS", "25"))
    rng = random.Random(int(os.environ.get("MXG_FUZZ_SEED", "99")))
    for t in range(trials):
        k, w = rng.choice([(32, 100), (32, 300), (32, 1000), (15, 10), (21, 50)])
        recs = []
        for i in range(rng.choice([1, 2, 5, 40, 400])):
            n = rng.choice([0, 1, k - 1, k, k + w - 2, k + w - 1, 200, 4095, 4096, 4097, 9000, 70000])
            alphabet = rng.choice(["ACGT", "ACGT", "ACGTacgt", "ACGTN", "ACGTRYKMn-", "ACGU", "A", "AC"])
            s = [rng.choice(alphabet) for _ in range(n)]
            if n > 3000 and rng.random() < 0.4:
                a = rng.randrange(n - 2000)
                s[a:a + rng.choice([1, 31, 32, 700, 1900])] = rng.choice("Nn") * len(s[a:a + rng.choice([1, 31, 32, 700, 1900])])
            hdr = rng.choice([f"r{i}", f"r{i} a comment", f"r{i}\twith tab", f"r{i} > bracket", f"{i}"])
            recs.append((hdr, "".join(s)))
        fa = str(tmp_path / f"f{t}.fa")
        eol = rng.choice(["\n", "\r\n"])
        width = rng.choice([1, 7, 60, 61, 80, 4096, 100000])
        _write_fasta(fa, recs, width=width, eol=eol, ragged=rng.random() < 0.3, final_newline=rng.random() < 0.7)
        want = str(tmp_path / f"want{t}.tsv")
        orc.fasta_to_tsv(fa, want, k, w)
        for tag, env in (("dev", {}), ("host", {"MXG_HOST_INGEST": "1", "MXG_HOST_TSV": "1"})):
            out = str(tmp_path / f"{tag}{t}.tsv")
            _tsv_by_engine(fa, k, w, out, **env)
            assert open(out, "rb").read() == open(want, "rb").read(), (t, tag, k, w, width, repr(eol), len(recs))


# ---------------------------------------------------------------------------------------------------------------
# the device parser's validity events at their capacity (MXG_INGEST_EV_CAP)
# ---------------------------------------------------------------------------------------------------------------
DEVICE_LINE = "[mxg] load_fasta_device"


@pytest.fixture
def ingest_env():
    names = ("MXG_INGEST_EV_CAP", "MXG_HOST_INGEST", "MXG_HOST_TSV", "MXG_DEBUG_IO")
    saved = {k: os.environ.get(k) for k in names}
    for k in names:
        os.environ.pop(k, None)
    os.environ["MXG_DEBUG_IO"] = "1"
    yield os.environ
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _set(env, name, value):
    if value is None:
        env.pop(name, None)
    else:
        env[name] = str(value)


# one record inside one 4096-byte tile of the file (header at offset 0, under 4000 bytes in all): every change between valid and
# invalid bases behind the record's first base is one event of that tile
KNOWN_EVENTS = {
    2: lambda a, b, c: a + "N" + b + c,                       # ACGT... N ACGT...
    3: lambda a, b, c: a + "NNN" + b + c + "RY",              # ... and an invalid end
    4: lambda a, b, c: a + "n" + b + "K" * 40 + c,            # two islands
}


@pytest.mark.parametrize("changes", sorted(KNOWN_EVENTS))
@pytest.mark.parametrize("k,w", [(15, 10), (32, 50)])
def test_event_buffer_on_both_sides_of_its_capacity(tmp_path, ingest_env, capfd, changes, k, w):
    """capacities 1 .. 5 on files with two, three and four changes: the device parser keeps the file iff its events fit
    (n_ev <= capacity), else the host parser takes it; the TSV is the oracle's, byte for byte, either way"""
    orc = _oracle.load()
    rng = random.Random(changes)
    seq = KNOWN_EVENTS[changes](_seq(rng, 1200), _seq(rng, 900), _seq(rng, 1100))
    fa = str(tmp_path / "one_tile.fa")
    _write_fasta(fa, [("r", seq)], width=70)
    assert os.path.getsize(fa) < 4000
    want = str(tmp_path / "want.tsv")
    orc.fasta_to_tsv(fa, want, k, w)
    assert os.path.getsize(want) > 1000
    for cap in (1, 2, 3, 4, 5):
        ingest_env["MXG_INGEST_EV_CAP"] = str(cap)
        capfd.readouterr()
        out = str(tmp_path / f"cap{cap}.tsv")
        with MxEngine(k=k, w=w, threads=3) as eng:
            eng.add_fasta("x", 1.0, fa)
            err = capfd.readouterr().err
            assert f"MXG_INGEST_EV_CAP={cap}" in eng.knobs().split()   # (the device parser came as far as its events)
            eng.sketch()
            eng.write_tsv(0, out, with_pos=True, with_strand=False, with_seq=True)
        assert (DEVICE_LINE in err) == (changes <= cap), (changes, cap, err)
        assert open(out, "rb").read() == open(want, "rb").read(), (changes, cap)


@pytest.mark.parametrize("eol", ["\n", "\r\n"])
@pytest.mark.parametrize("k,w", [(32, 100), (15, 10)])
def test_scattered_invalid_bases_overflow_the_event_buffer(tmp_path, ingest_env, capfd, eol, k, w):
    """thousands of events (the `scattered` record of _messy_records) against a buffer of 1, of 64 and the default: through
    add_fasta, add_fasta_split (three parts whose concatenation is the whole) and the indexlr CLI; LF and CRLF"""
    orc = _oracle.load()
    fa = str(tmp_path / "messy.fa")
    _write_fasta(fa, _messy_records(21), width=70, eol=eol)
    want = str(tmp_path / "oracle.tsv")
    orc.fasta_to_tsv(fa, want, k, w)
    want_bytes = open(want, "rb").read()
    exe = os.path.join(BIN_DIR, "indexlr")
    for cap in (1, 64, None):
        _set(ingest_env, "MXG_INGEST_EV_CAP", cap)
        capfd.readouterr()
        out = str(tmp_path / f"cap{cap}.tsv")
        with MxEngine(k=k, w=w, threads=3) as eng:
            eng.add_fasta("x", 1.0, fa)
            err = capfd.readouterr().err
            eng.sketch()
            eng.write_tsv(0, out, with_pos=True, with_strand=False, with_seq=True)
            whole = {key: v.copy() for key, v in eng.get_sketch(0).items() if key in ("out_hash", "pos", "record")}
        assert (DEVICE_LINE in err) == (cap is None), (cap, err)
        assert open(out, "rb").read() == want_bytes, cap
        parts = []
        for s in range(3):
            with MxEngine(k=k, w=w) as eng:
                eng.add_fasta_split("x", 1.0, fa, s, 3)
                eng.sketch()
                parts.append({key: v.copy() for key, v in eng.get_sketch(0).items() if key in ("out_hash", "pos", "record")})
        for key in ("out_hash", "pos", "record"):
            assert np.array_equal(np.concatenate([p[key] for p in parts]), whole[key]), (cap, key)
        r = subprocess.run([exe, "--seq", "--long", "--pos", f"-k{k}", f"-w{w}", "-t3", fa], capture_output=True, check=True)
        assert r.stdout == want_bytes, cap
        assert (DEVICE_LINE in r.stderr.decode()) == (cap is None), cap


def test_invalid_base_intervals_agree_on_every_ingest_route(tmp_path, ingest_env, capfd):
    """mxg_overlap_cuts reads the invalid-base intervals every text ingest route fills: paths whose junctions overlap, N islands near
    the overlapping ends among them (tests/_overlap_cases.py), behind the device parser, behind the host parser (MXG_HOST_INGEST=1)
    and behind the device parser's overflow (one event of room): the same cut points, those of tests/_overlap_restatement.py"""
    from tests._overlap_cases import fasta_text, make_synth
    from tests.test_gpu_overlap import check_against_restatement
    records, paths = make_synth(seed=20261017, n_paths=60)
    n_islands = sum(1 for _, s in records for i, ch in enumerate(s) if ch == "N" and i and s[i - 1] != "N")
    assert n_islands >= 8, n_islands
    fa = str(tmp_path / "paths.fa")
    with open(fa, "w", encoding="ascii") as fh:
        fh.write(fasta_text(records))
    results = []
    for tag, knobs, device in (("device", {}, True), ("host", {"MXG_HOST_INGEST": "1"}, False), ("overflow", {"MXG_INGEST_EV_CAP": "1"}, False)):
        for name in ("MXG_HOST_INGEST", "MXG_INGEST_EV_CAP"):
            _set(ingest_env, name, knobs.get(name))
        capfd.readouterr()
        with MxEngine(k=32, w=100) as eng:   # (the handle's k and w are not the call's)
            a = eng.add_fasta("t", 1.0, fa)
            err = capfd.readouterr().err
            assert (DEVICE_LINE in err) == device, (tag, err)
            got = check_against_restatement(eng, a, records, paths, 15, 10)
            results.append({key: v.copy() for key, v in got.items()})
    assert results[0]["cut_found"].sum() > 20
    for res in results[1:]:
        for key in ("start_adjust", "end_adjust", "cut_found"):
            assert np.array_equal(res[key], results[0][key]), key
