"""GPU tests of the BGZF route of the file ingest: a `bgzip`-compressed FASTA is uploaded as it is, inflated by k_bgzf_inflate
(ntjoin_amd/csrc/bgzf.hip, the decoder of bgzf_inflate.h), its header lines found by kernels (ingest.hip), and from there on
treated like the text of a plain file.

The witness that the device inflated a file is the line "[mxg] bgzf_inflate members=... bytes_in=... bytes_out=... ms=..." that
MXG_DEBUG_IO=1 prints when, and only when, it did.  What the TSV must be: the TSV of the uncompressed file, and the TSV of the same
`.gz` through the host parser and zlib (MXG_HOST_INGEST=1); both are compared.  k = 32, w = 100.

 1. text shapes x member sizes: the borders of the members fall everywhere in the text (every byte, inside header lines, between
    a line end and the next '>', at the ingest tile's 4096), with and without the end marker, empty members in between;
 2. decoder shapes: stored, fixed, dynamic blocks, several blocks per member, long overlapping copies, distances near 32 768;
 3. what is not BGZF stays with the host parser (no witness line), with the same TSV;
 4. damaged files end as they do through the host parser, and the handle goes on working;
 5. the command-line surfaces."""
import gzip
import os
import re
import subprocess
import sys
import zlib

import pytest

from ntjoin_amd.engine import MxEngine, MxError
from tests import _bgzf
from tests.conftest import BIN_DIR, GOLDEN, REPO

pytestmark = pytest.mark.gpu

K, W = 32, 100
WITNESS = re.compile(r"\[mxg\] bgzf_inflate members=(\d+) bytes_in=(\d+) bytes_out=(\d+) ms=[0-9.]+\n")
PARSER_LINE = "[mxg] load_fasta_device"
NAMES = ("MXG_HOST_INGEST", "MXG_HOST_TSV", "MXG_DEBUG_IO", "MXG_INGEST_EV_CAP")


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


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


def _tsv(eng, path, out):
    a = eng.add_fasta(os.path.basename(out), 1.0, path)
    eng.sketch()
    eng.write_tsv(a, out, with_pos=True, with_strand=False, with_seq=True)
    return _read(out)


def _run(env, capfd, path, out, host=False):
    """-> (TSV bytes, stderr of the load) through the device route, or through the host parser"""
    if host:
        env["MXG_HOST_INGEST"] = "1"
    else:
        env.pop("MXG_HOST_INGEST", None)
    capfd.readouterr()
    try:
        with MxEngine(k=K, w=W, threads=3) as eng:
            a = eng.add_fasta("x", 1.0, path)
            err = capfd.readouterr().err
            eng.sketch()
            eng.write_tsv(a, out, with_pos=True, with_strand=False, with_seq=True)
    finally:
        env.pop("MXG_HOST_INGEST", None)
    return _read(out), err


class Text:
    """a FASTA text, its plain file and that file's TSV (made once per module, never changed)"""

    def __init__(self, d, name, text):
        self.text, self.fa = text, str(d / (name + ".fa"))
        with open(self.fa, "wb") as fh:
            fh.write(text)
        with MxEngine(k=K, w=W, threads=3) as eng:
            self.want = _tsv(eng, self.fa, str(d / (name + ".want.tsv")))


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    t = Text(tmp_path_factory.mktemp("bgzf_shapes"), "shapes", _bgzf.shapes_fasta())
    assert 900_000 < len(t.text) < 1_300_000 and t.want.count(b"\n") > 300 and len(t.want) > 500_000
    return t


@pytest.fixture(scope="module")
def decoder(tmp_path_factory):
    t = Text(tmp_path_factory.mktemp("bgzf_decoder"), "decoder", _bgzf.decoder_fasta())
    assert len(t.want) > 200_000
    return t


def _positive(env, capfd, tmp_path, gz, want, text_len, members=None):
    got, err = _run(env, capfd, gz, str(tmp_path / "dev.tsv"))
    m = WITNESS.search(err)
    assert m, err                                    # the device inflated the file ...
    assert PARSER_LINE in err, err                   # ... and the device parser kept it
    assert int(m.group(2)) == os.path.getsize(gz) and int(m.group(3)) == text_len, m.group(0)
    if members is not None:
        assert int(m.group(1)) == members, m.group(0)
    assert got == want
    host, err = _run(env, capfd, gz, str(tmp_path / "host.tsv"), host=True)
    assert not WITNESS.search(err) and PARSER_LINE not in err, err
    assert host == want


def _size_for_border(text, offset):
    """a member size s <= 65280 and a header line whose '>' sits at q with (q + offset) a multiple of s: a member ends `offset`
    bytes behind that '>'"""
    for m in re.finditer(rb"\n>", text):
        q = m.start() + 1 + offset
        for n in range(-(-q // 65280), q // 1000 + 1):
            if q % n == 0:
                return q // n, m.start() + 1
    raise AssertionError("no such size")


SIZES = ["1", "100", "4096", "65280", "cycle", "border_at_header", "border_in_header"]


@pytest.mark.parametrize("eof", [True, False], ids=["eof", "no_eof"])
@pytest.mark.parametrize("size", SIZES)
def test_text_shapes_by_member_size(tmp_path, env, capfd, shapes, size, eof):
    text = shapes.text
    if size == "cycle":
        sizes = (0, 1, 65280, 7, 0, 30000)
    elif size == "border_at_header":       # ... '\n' | '>' ...
        s, q = _size_for_border(text, 0)
        assert text[q - 1:q + 1] == b"\n>" and q % s == 0
        sizes = s
    elif size == "border_in_header":       # ... '>fr' | 'ag12' ...
        s, q = _size_for_border(text, 3)
        assert text[q] == ord(">") and b"\n" not in text[q:q + 5] and (q + 3) % s == 0
        sizes = s
    else:
        sizes = int(size)
    gz = _bgzf.write_bgzf(str(tmp_path / "shapes.fa.gz"), text, sizes, eof=eof)
    members = -(-len(text) // sizes) if isinstance(sizes, int) else None   # (the non-empty ones)
    _positive(env, capfd, tmp_path, gz, shapes.want, len(text), members)


def test_two_files_concatenated(tmp_path, env, capfd, shapes):
    """an end marker in the middle of the file"""
    cut = shapes.text.index(b"\n>frag100") + 1
    gz = str(tmp_path / "two.fa.gz")
    with open(gz, "wb") as fh:
        fh.write(_bgzf.bgzf_bytes(shapes.text[:cut], 30000) + _bgzf.bgzf_bytes(shapes.text[cut:], 50000))
    _positive(env, capfd, tmp_path, gz, shapes.want, len(shapes.text))


@pytest.mark.parametrize("n", [1, 4096, 65536])
def test_text_sizes(tmp_path, env, capfd, shapes, n):
    """one byte; exactly the ingest tile; exactly the largest member"""
    text = shapes.text[:n]
    fa = str(tmp_path / "t.fa")
    with open(fa, "wb") as fh:
        fh.write(text)
    want, err = _run(env, capfd, fa, str(tmp_path / "want.tsv"))
    assert PARSER_LINE in err and not WITNESS.search(err)
    assert n < 4096 or len(want) > 100
    gz = _bgzf.write_bgzf(str(tmp_path / "t.fa.gz"), text, 65536)
    _positive(env, capfd, tmp_path, gz, want, n, members=1)


DECODER_SHAPES = {"level0": dict(level=0), "fixed": dict(strategy=zlib.Z_FIXED), "huffman_only": dict(strategy=zlib.Z_HUFFMAN_ONLY),
                  "rle": dict(strategy=zlib.Z_RLE), "level1": dict(level=1), "level9": dict(level=9), "flush5000": dict(flush_every=5000),
                  "default": dict()}


@pytest.mark.parametrize("shape", sorted(DECODER_SHAPES))
def test_decoder_shapes(tmp_path, env, capfd, decoder, shape):
    """members of 60 000 bytes (matches as long and as far back as zlib finds them), the random bytes of the first header line in a
    member of their own: stored, whatever the level"""
    sizes = [_bgzf.RND_AT, _bgzf.RND_LEN] + [60000] * 40
    gz = _bgzf.write_bgzf(str(tmp_path / "decoder.fa.gz"), decoder.text, sizes, **DECODER_SHAPES[shape])
    rnd = decoder.text[_bgzf.RND_AT:_bgzf.RND_AT + _bgzf.RND_LEN]
    if shape == "default":   # (a stored block inside a default-level file)
        assert _bgzf.first_block_type(_bgzf.member(rnd)) == 0
    _positive(env, capfd, tmp_path, gz, decoder.want, len(decoder.text))


def _not_bgzf(shapes):
    text = shapes.text
    good = _bgzf.bgzf_bytes(text, 60000, eof=False)
    tail = b">appended\n" + b"ACGTTGCA" * 40 + b"\n"
    return {"gzip_open": (None, text),
            "plain_member_appended": (_bgzf.bgzf_bytes(text + b"\n", 60000) + gzip.compress(tail), text + b"\n" + tail),
            "fname_in_one_member": (_bgzf.member(text[:50000]) + _bgzf.member(text[50000:90000], fname=b"x.fa") +
                                    _bgzf.bgzf_bytes(text[90000:], 60000), text),
            "eof_marker_only": (_bgzf.EOF_MARKER, b"")}


@pytest.mark.parametrize("case", ["gzip_open", "plain_member_appended", "fname_in_one_member", "eof_marker_only"])
def test_routes_that_stay_as_they_are(tmp_path, env, capfd, shapes, case):
    data, text = _not_bgzf(shapes)[case]
    gz, fa = str(tmp_path / "x.fa.gz"), str(tmp_path / "x.fa")
    if data is None:
        with gzip.open(gz, "wb") as fh:
            fh.write(text)
    else:
        with open(gz, "wb") as fh:
            fh.write(data)
    with open(fa, "wb") as fh:
        fh.write(text)
    want, _ = _run(env, capfd, fa, str(tmp_path / "want.tsv"))
    if text == shapes.text:
        assert want == shapes.want
    got, err = _run(env, capfd, gz, str(tmp_path / "got.tsv"))
    assert not WITNESS.search(err) and PARSER_LINE not in err, err   # zlib on the host, as before
    assert got == want
    assert (len(want) == 0) == (case == "eof_marker_only")


def _damaged(text):
    """three files with one thing wrong each, and the member sizes they were written with"""
    stored = _bgzf.split_payloads(text, 60000)
    ms = [_bgzf.member(p, level=0 if i == 2 else 6) for i, p in enumerate(stored)]
    flip = bytearray(b"".join(ms) + _bgzf.EOF_MARKER)
    at = len(ms[0]) + len(ms[1]) + 18 + 5 + 1000      # a text byte of the stored member (behind its block's five bytes)
    assert flip[at] == stored[2][1000]
    flip[at] ^= 0x01
    good = [_bgzf.member(p) for p in stored]
    isize = bytearray(b"".join(good) + _bgzf.EOF_MARKER)
    at = len(good[0]) + len(good[1]) - 4
    isize[at:at + 4] = (len(stored[1]) + 1).to_bytes(4, "little")
    cut = (b"".join(good))[:-10]                      # (no end marker: the last member itself is cut)
    return {"crc_of_a_stored_member": bytes(flip), "isize_raised_by_one": bytes(isize), "last_member_cut_by_10": cut}


@pytest.mark.parametrize("case", ["crc_of_a_stored_member", "isize_raised_by_one", "last_member_cut_by_10"])
def test_damaged_files_end_as_they_do_on_the_host(tmp_path, env, capfd, shapes, case):
    """These expect a clean error.  The file's structure is valid in the first two (the walk accepts it, the kernel runs and a
    member's status -- CRC, size -- sends the file to zlib); the third is refused by the walk."""
    bad = str(tmp_path / "bad.fa.gz")
    with open(bad, "wb") as fh:
        fh.write(_damaged(shapes.text)[case])
    good = _bgzf.write_bgzf(str(tmp_path / "good.fa.gz"), shapes.text, 60000)

    def outcome(host):
        if host:
            env["MXG_HOST_INGEST"] = "1"
        capfd.readouterr()
        try:
            with MxEngine(k=K, w=W, threads=3) as eng:
                try:
                    a = eng.add_fasta("bad", 1.0, bad)
                    eng.sketch()
                    eng.write_tsv(a, str(tmp_path / "bad.tsv"), with_pos=True, with_strand=False, with_seq=True)
                    res = ("no error", _read(tmp_path / "bad.tsv"))
                except Exception as exc:   # noqa: BLE001 -- whatever it is, it has to be the same both ways
                    res = (type(exc).__name__, getattr(exc, "code", None))
                err = capfd.readouterr().err
                # the same handle, the intact file
                tsv = _tsv(eng, good, str(tmp_path / "good.tsv"))
                err_good = capfd.readouterr().err
        finally:
            env.pop("MXG_HOST_INGEST", None)
        return res, err, tsv, err_good

    dev, err, tsv, err_good = outcome(False)
    assert not WITNESS.search(err) and PARSER_LINE not in err, err    # the device did not keep the damaged file
    assert tsv == shapes.want and WITNESS.search(err_good), err_good
    host, _, tsv, _ = outcome(True)    # (a handle reads a knob once: this one stays with the host parser for the intact file too)
    assert tsv == shapes.want
    assert dev == host
    if case != "last_member_cut_by_10":
        assert dev[0] == MxError.__name__ and dev[1] is not None, dev


# ---- through the surfaces -------------------------------------------------------------------------------------------------
FASTA = os.path.join(GOLDEN, "fasta")
CHILD_ENV = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""), MXG_DEBUG_IO="1", MXG_NO_DETACH="1")
for _name in ("MXG_HOST_INGEST", "MXG_HOST_TSV"):
    CHILD_ENV.pop(_name, None)
LIMIT = ["timeout", "-k", "10", "120"]


def _child(words, cwd=None):
    res = subprocess.run(LIMIT + words, cwd=cwd, env=CHILD_ENV, capture_output=True, check=False)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    return res


def test_indexlr_prints_the_plain_file_s_bytes(tmp_path, shapes):
    gz = _bgzf.write_bgzf(str(tmp_path / "shapes.fa.gz"), shapes.text, 65280)
    exe = os.path.join(BIN_DIR, "indexlr")
    res = _child([exe, "--seq", "--long", "--pos", f"-k{K}", f"-w{W}", "-t2", gz])
    assert WITNESS.search(res.stderr.decode()), res.stderr
    assert res.stdout == shapes.want
    assert _child([exe, "--seq", "--long", "--pos", f"-k{K}", f"-w{W}", "-t2", shapes.fa]).stdout == shapes.want


def _two_dirs(tmp_path):
    """the f-f fixture's target and reference as plain copies and, under the same names, as BGZF files (the route is chosen by the
    file's bytes, not by its name: every output then carries the same names)"""
    dirs = {}
    for tag in ("plain", "bgzf"):
        d = tmp_path / tag
        d.mkdir()
        for src, name in (("scaf.f-f.fa", "scaf.f-f.fa"), ("ref.fa", "ref.fa")):
            data = _read(os.path.join(FASTA, src))
            with open(d / name, "wb") as fh:
                fh.write(data if tag == "plain" else _bgzf.bgzf_bytes(data, 1500))
        dirs[tag] = d
    return dirs


def test_mxgraph_on_bgzf_target_and_reference(tmp_path):
    dirs = _two_dirs(tmp_path)
    exe = os.path.join(BIN_DIR, "mxgraph")
    for tag, d in dirs.items():
        res = _child([exe, "-k32", "-w1000", "-t4", "-p", "out", "-s", "scaf.f-f.fa", "-r", "2", "ref.fa"], cwd=d)
        assert len(WITNESS.findall(res.stderr.decode())) == (2 if tag == "bgzf" else 0), res.stderr
    for name in ("out.mx.dot", "scaf.f-f.fa.k32.w1000.tsv", "ref.fa.k32.w1000.tsv"):
        assert _read(dirs["bgzf"] / name) == _read(dirs["plain"] / name), name
        assert len(_read(dirs["plain"] / name)) > 100, name


def test_assemble_on_bgzf_target_and_reference(tmp_path):
    dirs = _two_dirs(tmp_path)
    for tag, d in dirs.items():
        res = _child([sys.executable, "-m", "ntjoin_amd.assemble", "-p", "f-f_test", "-n", "1", "-s", "scaf.f-f.fa.k32.w1000.tsv", "-l", "1", "-r", "2",
                      "-k", "32", "--agp", "--overlap", "ref.fa.k32.w1000.tsv"], cwd=d)
        assert len(WITNESS.findall(res.stderr.decode())) == (2 if tag == "bgzf" else 0), res.stderr
    names = ["f-f_test.path", "f-f_test.agp", "f-f_test.scaf.f-f.fa.k32.w1000.tsv.unassigned.bed",
             "scaf.f-f.fa.k32.w1000.n1.assigned.scaffolds.fa", "scaf.f-f.fa.k32.w1000.n1.unassigned.scaffolds.fa"]
    for name in names:
        assert _read(dirs["bgzf"] / name) == _read(dirs["plain"] / name), name
    assert len(_read(dirs["plain"] / "f-f_test.path")) > 20 and len(_read(dirs["plain"] / names[3])) > 1000
