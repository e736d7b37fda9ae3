"""GPU tests of k_bgzf_inflate (ntjoin_amd/csrc/bgzf.hip) on DEFLATE that zlib never writes and on members that are wrong in one
chosen place: the files of tests/_deflate_craft.py, every one checked against zlib's inflate as it is made, and every one decoded by
the stand-alone CPU program of tests/test_bgzf_craft_cpu.py through the kernel's own source, sink and table types, under the
sanitizers, before it reaches a device.

Legal files (the named cases at the four alignments of the text, the seeded generator's file): the witness line of
tests/test_gpu_bgzf.py is there with zlib's byte count and the number of non-empty members; the inflated text, read back from the
device (MxEngine.assembly_text, tests/_devmem.download), is zlib's text byte for byte; the TSV (k = 32, w = 100, --seq) is the plain
file's and the host route's.  The member whose literal/length set is the end-of-block code alone stays on the device too.

Malformed files, one member each, through ONE engine: no witness line and no parser line, the outcome (exception type and code)
is the host route's for the same file, and afterwards the same handle loads a legal file."""
import os

import pytest

from ntjoin_amd.engine import MxEngine
from tests import _deflate_craft as dc
from tests._devmem import download
from tests.test_gpu_bgzf import K, PARSER_LINE, W, WITNESS, _read, _run, env  # noqa: F401 -- env is a fixture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def generated():
    return dc.legal_members(dc.GENERATOR_SEED, dc.GENERATOR_N, dc.GENERATOR_BIG)[0]


def _members(name, generated):
    if name == "generated":
        return generated
    if name == "eob_only":
        return dc.named_members(0)[:1] + dc.case_eob_only()
    return dc.named_members(int(name[-1]))


def _device(capfd, gz, out):
    """-> (TSV, stderr of the load, the text as it lies in device memory) through the device route"""
    capfd.readouterr()
    with MxEngine(k=K, w=W, threads=3) as eng:
        a = eng.add_fasta("x", 1.0, gz)
        err = capfd.readouterr().err
        addr, n = eng.assembly_text(a)
        text = download(addr, n)
        eng.sketch()
        eng.write_tsv(a, out, with_pos=True, with_strand=False, with_seq=True)
    return _read(out), err, text


def _legal(tmp_path, env, capfd, members):
    data, text, n_members = dc.file_of(members)
    gz, fa = str(tmp_path / "craft.fa.gz"), str(tmp_path / "craft.fa")
    with open(gz, "wb") as fh:
        fh.write(data)
    with open(fa, "wb") as fh:
        fh.write(text)
    got, err, dev_text = _device(capfd, gz, str(tmp_path / "dev.tsv"))
    m = WITNESS.search(err)
    assert m, err                                    # the device inflated the file ...
    assert PARSER_LINE in err, err                   # ... and the device parser kept it
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (n_members, len(data), len(text)), m.group(0)
    assert len(dev_text) == len(text)
    assert dev_text == text                          # zlib's text, byte for byte
    want, err = _run(env, capfd, fa, str(tmp_path / "want.tsv"))
    assert PARSER_LINE in err and not WITNESS.search(err), err
    assert got == want
    host, err = _run(env, capfd, gz, str(tmp_path / "host.tsv"), host=True)
    assert not WITNESS.search(err) and PARSER_LINE not in err, err
    assert host == want
    return want


@pytest.mark.parametrize("name", ["named0", "named1", "named2", "named3", "generated"])
def test_legal_deflate_that_zlib_never_writes(tmp_path, env, capfd, generated, name):
    want = _legal(tmp_path, env, capfd, _members(name, generated))
    assert len(want) > 1000                          # (there are minimizers to compare)


def test_end_of_block_only_set_stays_on_the_device(tmp_path, env, capfd):
    """a literal/length set of one code of one bit is incomplete, and zlib takes it: without the same exception in
    bgzf_dynamic_tables the member ends with BGZF_CODE_LENGTHS and the whole file goes to the host -- no witness line"""
    _legal(tmp_path, env, capfd, _members("eob_only", None))


def test_malformed_members_end_as_they_do_on_the_host(tmp_path, env, capfd):
    table = dc.malformed()
    paths = {}
    for name, (data, _, _) in table.items():
        paths[name] = str(tmp_path / (name + ".fa.gz"))
        with open(paths[name], "wb") as fh:
            fh.write(data)
    data, text, n_members = dc.file_of(dc.named_members(0))
    good = str(tmp_path / "good.fa.gz")
    with open(good, "wb") as fh:
        fh.write(data)

    def outcomes(host):
        if host:
            env["MXG_HOST_INGEST"] = "1"
        res, errs = {}, {}
        capfd.readouterr()
        try:
            with MxEngine(k=K, w=W, threads=3) as eng:
                for name, path in paths.items():
                    tsv = str(tmp_path / (name + ".tsv"))
                    try:
                        a = eng.add_fasta(name, 1.0, path)
                        eng.sketch()
                        eng.write_tsv(a, tsv, with_pos=True, with_strand=False, with_seq=True)
                        res[name] = ("no error", _read(tsv))
                    except Exception as exc:   # noqa: BLE001 -- whatever it is, it has to be the same both ways
                        res[name] = (type(exc).__name__, getattr(exc, "code", None))
                    errs[name] = capfd.readouterr().err
                # the same handle, a legal file
                a = eng.add_fasta("good", 1.0, good)
                err_good = capfd.readouterr().err
                addr, n = (eng.assembly_text(a) if not host else (0, 0))
                good_text = download(addr, n) if not host else None
                eng.sketch()
                eng.write_tsv(a, str(tmp_path / "good.tsv"), with_pos=True, with_strand=False, with_seq=True)
        finally:
            env.pop("MXG_HOST_INGEST", None)
        return res, errs, err_good, good_text, _read(tmp_path / "good.tsv")

    dev, errs, err_good, good_text, good_tsv = outcomes(False)
    for name, err in errs.items():
        assert not WITNESS.search(err) and PARSER_LINE not in err, (name, err)    # the device did not keep the file
    m = WITNESS.search(err_good)
    assert m and int(m.group(1)) == n_members and int(m.group(3)) == len(text), err_good
    assert good_text == text
    host, _, _, _, host_tsv = outcomes(True)
    assert good_tsv == host_tsv and len(good_tsv) > 1000
    for name in table:
        assert dev[name] == host[name], name
    refused = [name for name, (_, outcome, _) in table.items() if outcome == dc.REFUSED and name != "isize_65537"]
    assert len(refused) == 5 and all(dev[name][0] == "no error" for name in refused)   # (legal gzip, not BGZF: zlib reads them)
    assert all(dev[name][0] != "no error" for name in table if name not in refused)
    assert os.path.getsize(paths["block_type_3"]) < 400
