"""CPU tests of the FASTA index route: the restatement of mxg_write_fai's contract (tests/_fai_restatement.py) against the two
`samtools faidx` outputs the reference records (tests/golden/fai/); the code of the device route (ntjoin_amd/csrc/fai_scan.h) run on
the host by tools/fai_check.cpp, built plainly and with AddressSanitizer + UndefinedBehaviorSanitizer (the runtime linked into the
program; nothing is preloaded), against the restatement on every shape and every refusal of tests/_fai_cases.py, and on the texts
that put one long record on the tile and round borders of the scan over the work items, each of which must come out wrong under the
fault of that scan it is listed for (fai_check FASTA FAULT); the way back from a row to the bases; ntjoin_amd.fai's concatenation; --fai on the command line and in `ntJoin-mx scaffold`; the exported symbols."""
import os
import random
import re
import shutil
import struct
import subprocess

import pytest

from ntjoin_amd import fai as fai_mod
from ntjoin_amd.run import parse_arguments
from tests import _fai_cases, _fai_restatement as R
from tests.conftest import GOLDEN, REPO

CSRC = os.path.join(REPO, "ntjoin_amd", "csrc")
GOLDEN_FAI = {"ref.fa": b"test\t4330\t6\t4330\t4331\n", "scaf.f-f.fa": b"1_f\t1981\t5\t1981\t1982\n2_f\t2329\t1992\t2329\t2330\n"}


def _golden(name):
    with open(os.path.join(GOLDEN, "fasta", name), "rb") as fh:
        text = fh.read()
    with open(os.path.join(GOLDEN, "fai", name + ".fai"), "rb") as fh:
        return text, fh.read()


@pytest.mark.parametrize("name", sorted(GOLDEN_FAI))
def test_restatement_reproduces_samtools(name):
    text, want = _golden(name)
    assert want == GOLDEN_FAI[name]  # (the recorded files are what the issue quotes)
    assert R.fai_bytes(text) == want


def _sanitizer_flags(cxx, td):
    probe = td / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    for static in (["-static-libasan", "-static-libubsan"], ["-static-libsan"]):
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] + static
        exe = td / "probe"
        if subprocess.run([cxx] + flags + [str(probe), "-o", str(exe)], capture_output=True).returncode == 0 and \
                subprocess.run([str(exe)], capture_output=True).returncode == 0:
            return flags
    return None


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    td = tmp_path_factory.mktemp("fai_check_" + request.param)
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    extra = []
    if request.param == "sanitized":
        extra = _sanitizer_flags(cxx, td)
        if extra is None:
            pytest.skip("the host compiler has no AddressSanitizer runtime to link")
    return _compile(cxx, td, extra)


def _compile(cxx, td, extra):
    out = td / "fai_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror"] + extra + ["-I", CSRC, os.path.join(REPO, "tools", "fai_check.cpp"),
                                                                                 "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def plain_exe(tmp_path_factory):
    "the plain build alone, for the runs with a fault switched on"
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    return _compile(cxx, tmp_path_factory.mktemp("fai_check_faults"), [])


def _run(exe, text, tmp_path, fault=None):
    fa = tmp_path / "x.fa"
    fa.write_bytes(text)
    return subprocess.run([exe, str(fa)] + ([fault] if fault else []), capture_output=True, timeout=120)


def check_fetch(rows, text, seed=1, tries=12):
    "faidx's formula through every row returns the record's bases"
    rng = random.Random(seed)
    recs = {}
    for name, lo, se in R.records(text):
        recs.setdefault(name, (lo, se))
    for row in rows:
        bases = R.bases_of(text, *recs[row[0]])
        assert len(bases) == row[1]
        if not bases:
            continue
        spans = [(0, len(bases)), (len(bases) - 1, len(bases))] if len(bases) < 20000 else []
        for _ in range(tries):
            lo = rng.randrange(len(bases))
            spans.append((lo, min(len(bases), lo + rng.randint(1, 300))))
        for lo, hi in spans:
            assert R.fetch(row, text, lo, hi) == bases[lo:hi], (row, lo, hi)


SHAPES = _fai_cases.shapes()
REFUSALS = _fai_cases.refusals()


def test_host_program_on_the_goldens(exe, tmp_path):
    for name in sorted(os.listdir(os.path.join(GOLDEN, "fasta"))):
        with open(os.path.join(GOLDEN, "fasta", name), "rb") as fh:
            text = fh.read()
        r = _run(exe, text, tmp_path)
        assert r.returncode == 0, (name, r.stdout, r.stderr)
        assert r.stdout == R.fai_bytes(text), name


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_host_program_equals_restatement_on_shapes(exe, tmp_path, name):
    text = SHAPES[name]
    want = R.fai_bytes(text)
    r = _run(exe, text, tmp_path)
    assert r.returncode == 0, (r.stdout[:300], r.stderr[:2000])
    assert r.stdout == want
    check_fetch(R.parse(want), text)


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_host_program_refuses_what_the_restatement_refuses(exe, tmp_path, name):
    text, bad = REFUSALS[name]
    with pytest.raises(R.Refused) as err:
        R.index(text)
    assert err.value.name == bad
    r = _run(exe, text, tmp_path)
    assert r.returncode == 3, (r.stdout[:300], r.stderr[:2000])
    word = r.stdout.decode().split()
    assert word[0] == "refused" and int(word[1]) == err.value.record and word[2] == bad


def test_host_program_drops_later_records_of_a_name(exe, tmp_path):
    text = _fai_cases.duplicates()
    rows, dropped = R.index(text)
    assert [r[0] for r in rows] == ["a", "b", "c"] and dropped == ["a", "b", "a"]
    r = _run(exe, text, tmp_path)
    assert r.returncode == 0 and r.stdout == R.format_rows(rows)
    assert r.stderr.decode().count("duplicate") == 3


def test_random_foldings_agree(exe, tmp_path):
    "records of random widths, line ends and last lines, glued into one file"
    rng = random.Random(5)
    text = ""
    for i in range(60):
        eol = rng.choice(["\n", "\r\n"])
        n, w = rng.choice([0, 1, 59, 4095, 4096, 4097, rng.randint(1, 14000)]), rng.choice([1, 7, 60, 61, 4094, 4096, rng.randint(1, 5000)])
        text += _fai_cases.header("r%d" % i, rng.choice(["", " d", "\tt"]), eol) + _fai_cases.fold(_fai_cases.seq(rng, n), w, eol)
    text = text.encode()
    r = _run(exe, text, tmp_path)
    assert r.returncode == 0 and r.stdout == R.fai_bytes(text)
    check_fetch(R.parse(r.stdout), text, tries=4)


# ---- the carries of the scan over the work items
B = _fai_cases.ITEMS_ROUND
# the faults tools/fai_check.cpp can switch on, and the cases that are there to show each.  A case stands where it does for the
# faults it is listed under; under each of them the program's answer must differ from the restatement's.
#   tile                  items 255 | 256: the first-level border.  The scan of the tiles' totals gives it excl[1] = the total of tile
#                         0 in its first round, where the carry is empty: only a thread that takes its own value (inclusive) shows.
#   last_of_round         "long" on items B - 1 | B: excl[256] is the round carry itself, written by thread 0.
#   first_of_round        "long" begins on item B: nothing of round 0 may reach it (rows_plain: the record in front leaks into it).
#   across                "long" on tiles 254 .. 257: excl[257] = combine(carry, sh[0]) needs the carry through thread 1.
#   second_round          the same over the border of rounds 1 and 2: the carry there is a carry folded onto a carry, and with the
#                         plain operator it drags round 0 along.
#   exact_round_plus_one  257 tiles: a second round of one tile with one item (the partial-round guards; a loop over whole rounds).
#   refusal_*             the offence's place travels in the summary: without the carry the verdict names another byte.
CARRY_FAULTS = {
    "tile": ("inclusive",),
    "last_of_round": ("nocarry", "nocarry_t0", "early"),
    "first_of_round": ("rows_plain",),
    "across": ("nocarry", "nocarry_rest", "early"),
    "second_round": ("nocarry_rest", "early", "plain"),
    "exact_round_plus_one": ("nocarry_t0", "rounds"),
    "refusal_behind": ("nocarry_rest",),
    "refusal_in_front": ("nocarry_rest", "early"),
}
# and what a case must NOT show, which says that it stands on the place it names: thread 0 against the others; a file of exactly
# 256 tiles has no second round, so no fault of the carry and no dropped partial round touches it (the other half of "exact").
CARRY_BLIND = {
    "last_of_round": ("nocarry_rest",),
    "across": ("nocarry_t0",),
    "exact_round": ("nocarry", "early", "rounds"),
    # No case can show `restart` (the carry restarted from the round's total instead of folded onto the carry before).  The two
    # differ only where a whole round holds no record's first item, for the total of a round that holds one forgets what is in
    # front of it anyway: one record over 65 536 items of 4 096 bytes, 256 MB of text.  second_round is the only case that reads a
    # carry made of two rounds, and it comes out right under it.
    "second_round": ("restart",),
}
_WANT = {}


def carry_want(name):
    "(exit status, stdout) the restatement asks of the host program; computed once per case"
    if name not in _WANT:
        text = _fai_cases.carry_case(name)
        try:
            _WANT[name] = (0, R.fai_bytes(text))
            assert not _fai_cases.CARRIES[name][1]
        except R.Refused as err:
            assert _fai_cases.CARRIES[name][1] and err.name == "long"
            _WANT[name] = (3, ("refused %d long %d\n" % (err.record, err.offset)).encode())
    return _WANT[name]


def carry_place(name):
    "(items in front of 'long', items of 'long', items of the text) by the cutting rule"
    text = _fai_cases.carry_case(name)
    items = _fai_cases.items_of(text)
    at = [rec[0] for rec in R.records(text)].index("long")
    return sum(items[:at]), items[at], sum(items)


def test_items_of_states_the_cutting_rule():
    t = _fai_cases
    pad = t.padded_header(0, "a", 4090)  # (the text of "a" begins 6 bytes in front of a border of the file's tiles)
    text = (pad + "ACGTAC\n" + ">b\n" + ">c\nAC\n" + t.padded_header(len(pad) + 17, "d", 4095) + "A" * 4098 + "\n>e").encode()
    assert t.items_of(text) == [2, 0, 1, 3, 0]
    assert t.items_of(b"") == [] and t.items_of(b">a") == [0] and t.items_of(b">a\n") == [0] and t.items_of(b">a\nA") == [1]


@pytest.mark.parametrize("name", sorted(_fai_cases.CARRIES))
def test_carry_cases_stand_where_they_say(name):
    kw = _fai_cases.CARRIES[name][0]
    at, span, total = carry_place(name)
    assert (at, span) == (kw["at"], kw["span"])
    if name.startswith("exact"):
        assert total == at + span == (B if name == "exact_round" else B + 1)
    text = _fai_cases.carry_case(name)
    items = _fai_cases.items_of(text)
    front = items[:[rec[0] for rec in R.records(text)].index("long")]
    assert 0 in front and (2 in front or at < 4096 // 8) and b"\r\n" in text and front[-1] == 1


@pytest.mark.parametrize("name", sorted(_fai_cases.CARRIES))
def test_host_program_on_the_carries(exe, tmp_path, name):
    r = _run(exe, _fai_cases.carry_case(name), tmp_path)
    assert (r.returncode, r.stdout) == carry_want(name), (r.stdout[-300:], r.stderr[:2000])


@pytest.mark.parametrize("name,fault", [(n, f) for n in sorted(CARRY_FAULTS) for f in CARRY_FAULTS[n]])
def test_every_carry_case_shows_its_faults(plain_exe, tmp_path, name, fault):
    r = _run(plain_exe, _fai_cases.carry_case(name), tmp_path, fault)
    assert r.returncode in (0, 3), r.stderr[:2000]
    assert (r.returncode, r.stdout) != carry_want(name)


@pytest.mark.parametrize("name,fault", [(n, f) for n in sorted(CARRY_BLIND) for f in CARRY_BLIND[n]])
def test_what_a_carry_case_cannot_show(plain_exe, tmp_path, name, fault):
    r = _run(plain_exe, _fai_cases.carry_case(name), tmp_path, fault)
    assert (r.returncode, r.stdout) == carry_want(name)


def test_host_program_knows_its_faults(plain_exe, tmp_path):
    assert _run(plain_exe, b">a\nAC\n", tmp_path, "no_such_fault").returncode == 2
    assert sorted({f for fs in list(CARRY_FAULTS.values()) + list(CARRY_BLIND.values()) for f in fs}) == sorted(
        ["nocarry", "nocarry_t0", "nocarry_rest", "early", "plain", "restart", "inclusive", "rounds", "rows_plain"])


# ---- ntjoin_amd.fai
def test_cat_fai_moves_the_offsets(tmp_path):
    a, b, out = tmp_path / "a.fai", tmp_path / "b.fai", tmp_path / "all.fai"
    a.write_bytes(b"ntJoin0\t10\t9\t10\t11\nntJoin1\t5\t29\t5\t6\n")
    b.write_bytes(b"x:0-7\t7\t7\t7\t8\ny z:3-4\t1\t24\t1\t2\n")
    fai_mod.cat_fai(str(a), 35, str(b), str(out))
    assert out.read_bytes() == b"ntJoin0\t10\t9\t10\t11\nntJoin1\t5\t29\t5\t6\nx:0-7\t7\t42\t7\t8\ny z:3-4\t1\t59\t1\t2\n"
    fai_mod.cat_fai(str(b), 1 << 40, str(a), str(out))
    assert out.read_bytes().splitlines()[2] == b"ntJoin0\t10\t%d\t10\t11" % ((1 << 40) + 9)


def test_cat_gzi_adds_the_pair_of_the_seam(tmp_path):
    a, b, out = tmp_path / "a.gzi", tmp_path / "b.gzi", tmp_path / "all.gzi"
    fai_mod.write_gzi(str(a), [(100, 65280), (190, 130560)])
    fai_mod.write_gzi(str(b), [(77, 65280)])
    fai_mod.cat_gzi(str(a), 300, 140000, str(b), 70000, str(out))
    assert fai_mod.read_gzi(str(out)) == [(100, 65280), (190, 130560), (272, 140000), (349, 205280)]
    assert out.read_bytes()[:8] == struct.pack("<Q", 4)
    fai_mod.write_gzi(str(b), [])
    fai_mod.cat_gzi(str(a), 300, 140000, str(b), 0, str(out))  # (an unassigned part without text: its file is the end marker)
    assert fai_mod.read_gzi(str(out)) == [(100, 65280), (190, 130560)]
    fai_mod.write_gzi(str(a), [])
    fai_mod.write_gzi(str(b), [(77, 65280)])
    fai_mod.cat_gzi(str(a), 28, 0, str(b), 70000, str(out))  # (no scaffold at all: the second part's first member is the file's first)
    assert fai_mod.read_gzi(str(out)) == [(77, 65280)]
    assert R.parse_gzi(R.gzi_bytes([(0, 0), (77, 65280)])) == [(77, 65280)]


def test_cat_files_from_the_command_line(tmp_path):
    from tests import _bgzf
    first, second = b">ntJoin0\nACGTACGTAC\n>ntJoin1\nGGGCC\n", b">x:0-7\nTTTTTTT\n"
    for gz in (False, True):
        ext = ".fa.gz" if gz else ".fa"
        names = [str(tmp_path / (n + ext)) for n in ("assigned", "unassigned", "all")]
        for name, text in zip(names, (first, second)):
            if gz:
                blob, members = _bgzf_with_members(_bgzf, text, 8)
                with open(name + ".gzi", "wb") as fh:
                    fh.write(R.gzi_bytes(members))
            else:
                blob = text
            with open(name, "wb") as fh:
                fh.write(blob)
            with open(name + ".fai", "wb") as fh:
                fh.write(R.fai_bytes(text))
        subprocess.run(["python3", "-m", "ntjoin_amd.fai", "cat"] + names, check=True, cwd=REPO, timeout=60)
        with open(names[2] + ".fai", "rb") as fh:
            assert fh.read() == R.fai_bytes(first + second)
        if gz:
            with open(names[0], "rb") as f0, open(names[1], "rb") as f1:
                whole = f0.read()[:-28] + f1.read()
            _, members = _bgzf_members_of(whole)
            assert fai_mod.read_gzi(names[2] + ".gzi") == members[1:]
            assert fai_mod.bgzf_text_bytes(names[0]) == len(first)


def _bgzf_with_members(_bgzf, text, payload):
    blob = _bgzf.bgzf_bytes(text, payload)
    return blob, _bgzf_members_of(blob)[1]


def _bgzf_members_of(blob):
    "-> (text bytes, [(compressed offset, text offset)] of the members that hold text), by the members' own headers"
    at, text, out = 0, 0, []
    while at < len(blob):
        assert blob[at:at + 4] == b"\x1f\x8b\x08\x04"
        (xlen,) = struct.unpack_from("<H", blob, at + 10)
        assert blob[at + 12:at + 14] == b"BC" and xlen == 6
        (bsize,) = struct.unpack_from("<H", blob, at + 16)
        (isize,) = struct.unpack_from("<I", blob, at + bsize + 1 - 4)
        if isize:
            out.append((at, text))
        text += isize
        at += bsize + 1
    return text, out


# ---- surfaces
ARGV = ["-s", "t.fa.k32.w100.tsv", "-r", "2", "-k", "32", "r.fa.k32.w100.tsv"]


def test_fai_is_a_store_true_flag_off_by_default():
    assert parse_arguments(ARGV).fai is False
    assert parse_arguments(["--fai"] + ARGV).fai is True
    assert parse_arguments(ARGV + ["--fai", "--gz"]).fai is True


def dry(*words):
    return subprocess.run(["make", "-n", "-f", os.path.join(REPO, "ntJoin-mx"), "scaffold", "target=t.fa", "references=r.fa", "reference_weights=2",
                           "k=32", "w=100", *words], capture_output=True, text=True, check=True, timeout=60).stdout


def test_make_variable_adds_the_flag_and_the_helper():
    plain, on, both = dry(), dry("fai=True"), dry("fai=True", "gz=True")
    assert dry("fai=False") == plain and "--fai" not in plain and "ntjoin_amd.fai" not in plain and ".fai" not in plain
    # without fai=True the recipe is what it was: the scaffolder's line and the concatenation
    assert len(plain.strip().split("\n")) == 3 and plain.rstrip().endswith("> t.fa.k32.w100.n1.all.scaffolds.fa")
    assert on.replace(" --fai", "").startswith(plain) and " --fai " in on
    base = "t.fa.k32.w100.n1."
    assert f"-m ntjoin_amd.fai cat {base}assigned.scaffolds.fa {base}unassigned.scaffolds.fa {base}all.scaffolds.fa\n" in on
    assert " --gz --fai " in both
    assert f"-m ntjoin_amd.fai cat {base}assigned.scaffolds.fa.gz {base}unassigned.scaffolds.fa.gz {base}all.scaffolds.fa.gz\n" in both
    assert both.index("head -c -28") < both.index("ntjoin_amd.fai cat")


def test_the_new_symbols_are_declared_and_exported():
    with open(os.path.join(REPO, "include", "ntjoin_mx.h"), encoding="utf-8") as fh:
        header = fh.read()
    assert re.search(r"int mxg_write_fai\(mxg_handle \*h, int assembly, const char \*fai_path, const char \*gzi_path\);", header)
    assert re.search(r"#define MXG_SCAF_FAI 0x4u", header)
    assert "ntJoin:152-153, 207-208" in header
    from ntjoin_amd import capi
    assert capi.SCAF_FAI == 0x4
    lib = capi.load()
    assert lib.mxg_write_fai is not None
