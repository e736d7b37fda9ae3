"""GPU tests of mxg_add_assembly_text_device and mxg_assembly_text (csrc/ingest.hip): for FASTA texts uploaded as
bytes, the assembly made from the text in device memory equals the assembly mxg_add_assembly_fasta makes of a file with those
bytes -- ids, lengths, sketch arrays, TSV bytes, .fai bytes and the assembly report; the handoff from a handle of one w to a handle
of another; the refusals."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from ntjoin_amd import capi
from ntjoin_amd.engine import MxEngine, MxError
from tests import _bgzf, _fai_cases as fc
from tests._devmem import download, upload
from tests.conftest import REPO

pytestmark = pytest.mark.gpu

TILE = fc.TILE


def _exact(rng, n_bytes, name="x", width=61):
    "one record whose file has exactly n_bytes"
    for n in range(n_bytes, 0, -1):
        t = fc.header(name) + fc.fold(fc.seq(rng, n), width)
        if len(t) == n_bytes:
            return t
        if len(t) < n_bytes:
            break
    return fc.header(name + "p" * (n_bytes - len(t))) + fc.fold(fc.seq(rng, n), width)


def _texts():
    rng = random.Random(77)
    out = {}
    for n in (4095, 4096, 4097):
        out["bytes_%d" % n] = _exact(rng, n)
        assert len(out["bytes_%d" % n]) == n
    t = fc.header("a") + fc.fold(fc.seq(rng, 4000), 60)
    t = t[:TILE - 10]
    t = t[:t.rfind("\n") + 1]
    t += "A" * (TILE - 10 - len(t) - 1) + "\n"
    assert len(t) == TILE - 10
    out["header_across_tile_border"] = t + fc.header("across_the_border", " a comment") + fc.fold(fc.seq(rng, 700), 60)
    out["bracket_in_header"] = fc.header("id1", " a > inside") + fc.fold(fc.seq(rng, 300), 60) + fc.header("id2>x") + fc.fold(fc.seq(rng, 90), 60)
    out["crlf"] = "".join(fc.header("r%d" % i, eol="\r\n") + fc.fold(fc.seq(rng, n), 70, "\r\n") for i, n in enumerate((500, 4096, 9000)))
    out["empty_record"] = fc.header("e0") + fc.header("a") + fc.fold(fc.seq(rng, 600), 60) + fc.header("e1") + fc.header("b") + fc.fold(fc.seq(rng, 200), 60) + ">e2"
    s = fc.seq(rng, 5000)
    out["lower_and_iupac"] = fc.header("l") + fc.fold(s.lower(), 60) + fc.header("i") + fc.fold(s[:900] + "RYKMSWBDHVrykm-" + s[900:2000] + "U" + s[2000:], 60)
    body = fc.seq(rng, TILE - 300).replace("N", "A").replace("n", "a")
    out["n_run_across_tile_border"] = fc.header("n") + body + "N" * 600 + body[:500] + "\n"
    out["one_record_of_three_tiles"] = fc.header("three") + fc.fold(fc.seq(rng, 2 * TILE + 100), 80)
    out["no_final_line_end"] = fc.header("a") + fc.fold(fc.seq(rng, 333), 60, end=False)
    out["zero_bytes"] = ""
    out = {k: v.encode("latin-1") for k, v in out.items()}
    shapes = fc.shapes()
    for name in ("split_crlf", "offsets_lf", "zero_crlf_noeol", "headers", "single_lf_noeol", "trailing_lf"):
        out["fai_" + name] = shapes[name]
    return out


TEXTS = _texts()
BIG = _bgzf.shapes_fasta()


def facts(eng, a, td, tag, fai=True):
    "everything the issue compares, of assembly a"
    eng.sketch(a)
    sk = eng.get_sketch(a)
    tsv = os.path.join(td, tag + ".tsv")
    eng.write_tsv(a, tsv)
    out = {"ids": eng.record_ids(a, eng.n_records(a)), "lengths": eng.record_lengths(a),
           "sketch": {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in sk.items()},
           "tsv": open(tsv, "rb").read()}
    rep = eng.assembly_report(a)
    out["report"] = {k: (sorted(v.tolist()) if isinstance(v, np.ndarray) else v) for k, v in rep.items()}
    if fai:
        p = os.path.join(td, tag + ".fai")
        eng.write_fai(a, p)
        out["fai"] = open(p, "rb").read()
    return out


def both_routes(text, k, w, td):
    fa = os.path.join(td, "t.fa")
    with open(fa, "wb") as fh:
        fh.write(text)
    with MxEngine(k=k, w=w) as ef, MxEngine(k=k, w=w) as et:
        af = ef.add_fasta("t", 1.0, fa)
        d = upload(text)
        at = et.add_text_device("t", 1.0, d.data_ptr(), len(text))
        del d   # the source may go as soon as the call has returned
        torch.cuda.empty_cache()
        made = []
        for eng, a in ((ef, af), (et, at)):   # (samtools refuses ragged records; the file route hands an empty file to the host parser)
            try:
                eng.write_fai(a, os.path.join(td, "probe.fai"))
                made.append(True)
            except MxError as e:
                assert e.code == capi.MXG_EINVAL
                made.append(False)
        assert made[0] == made[1] or not text
        fai = all(made)
        want, got = facts(ef, af, td, "file", fai), facts(et, at, td, "text", fai)
        if text:
            addr, n = et.assembly_text(at)
            assert n == len(text) and download(addr, n) == text
    return want, got


@pytest.mark.parametrize("name", sorted(TEXTS))
@pytest.mark.parametrize("k,w", [(15, 10), (21, 40)])
def test_text_in_device_memory_equals_the_file(name, k, w, tmp_path):
    want, got = both_routes(TEXTS[name], k, w, str(tmp_path))
    for key in want:
        assert got[key] == want[key], key
    assert bool(want["ids"]) == (name != "zero_bytes")


def test_k32_on_a_megabyte_of_every_shape(tmp_path):
    "CRLF, lower case, N runs of 700, IUPAC, a '>' inside a header, empty records, 300 tiny records, no final line end; the k = 32 route"
    want, got = both_routes(BIG, 32, 100, str(tmp_path))
    for key in want:
        assert got[key] == want[key], key
    assert len(want["sketch"]["out_hash"]) > 1000


def test_handoff_between_handles_of_different_w(tmp_path):
    "A (w = 100) loads a file; B (w = 50) takes A's text; A is closed before B sketches; B equals a fresh handle's add_fasta at w = 50"
    fa = os.path.join(str(tmp_path), "t.fa")
    with open(fa, "wb") as fh:
        fh.write(BIG)
    a = MxEngine(k=32, w=100)
    b = MxEngine(k=32, w=50)
    try:
        ia = a.add_fasta("t", 1.0, fa)
        addr, n = a.assembly_text(ia)
        assert n == len(BIG)
        ib = b.add_text_device("t", 1.0, addr, n)
        a.close()
        got = facts(b, ib, str(tmp_path), "handoff")
    finally:
        a.close()
        b.close()
    with MxEngine(k=32, w=50) as c:
        want = facts(c, c.add_fasta("t", 1.0, fa), str(tmp_path), "fresh")
    for key in want:
        assert got[key] == want[key], key


def test_assembly_text_needs_text_on_the_device(tmp_path):
    fa = os.path.join(str(tmp_path), "t.fa")
    with open(fa, "wb") as fh:
        fh.write(TEXTS["crlf"])
    with MxEngine(k=15, w=10) as eng:
        a = eng.add_fasta("t", 1.0, fa)
        eng.sketch(a)
        tsv = os.path.join(str(tmp_path), "t.tsv")
        eng.write_tsv(a, tsv)
        b = eng.add_tsv("from_tsv", 1.0, tsv)
        with pytest.raises(MxError, match="does not hold") as err:
            eng.assembly_text(b)
        assert err.value.code == capi.MXG_EINVAL
        with pytest.raises(MxError) as err:
            eng.assembly_text(7)
        assert err.value.code == capi.MXG_EINVAL
        with pytest.raises(MxError) as err:
            eng.add_text_device("t", 1.0, 0, 10)   # (the name is in use, and the text is null)
        assert err.value.code == capi.MXG_EINVAL
        with pytest.raises(MxError) as err:
            eng.add_text_device("null", 1.0, 0, 10)
        assert err.value.code == capi.MXG_EINVAL
        assert eng.assembly_text(a)[1] == len(TEXTS["crlf"])


_EV_CAP_CHILD = r"""
import sys
import torch
from ntjoin_amd import capi
from ntjoin_amd.engine import MxEngine, MxError
text = open(sys.argv[1], "rb").read()
d = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
torch.cuda.synchronize()
with MxEngine(k=15, w=10) as eng:
    try:
        eng.add_text_device("t", 1.0, d.data_ptr(), len(text))
        sys.exit("accepted")
    except MxError as e:
        assert e.code == capi.MXG_ELIMIT and "MXG_INGEST_EV_CAP" in str(e), (e.code, str(e))
    assert eng.n_assemblies == 0
    a = eng.add_fasta("t", 1.0, sys.argv[1])   # the host parser takes the file, and the name is free again
    eng.sketch(a)
    assert eng.n_records(a) == 1 and len(eng.get_sketch(a)["out_hash"]) > 0
print("OK")
"""


def test_more_validity_events_than_the_route_records_is_elimit(tmp_path):
    "MXG_INGEST_EV_CAP=1 (read once per handle from the environment: a child process) and a text of several N runs"
    rng = random.Random(5)
    text = ">n\n" + "".join("ACGT"[rng.randrange(4)] * 1 for _ in range(300))
    text = text[:80] + "NNN" + text[80:150] + "NN" + text[150:220] + "N" + text[220:] + "\n"
    fa = tmp_path / "n.fa"
    fa.write_text(text)
    script = tmp_path / "child.py"
    script.write_text(_EV_CAP_CHILD)
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, str(script), str(fa)], capture_output=True, text=True, cwd=REPO,
                       env=dict(os.environ, MXG_INGEST_EV_CAP="1", PYTHONPATH=REPO))
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
