"""GPU tests of scaffolding rounds in one process (`python -m ntjoin_amd.assemble --rounds_w`, `ntJoin-mx scaffold rounds_w=`;
ntjoin_amd/rounds.py) on a seeded synthetic input: long contigs that the first round (w = 1000) joins, and contigs of
fewer than 1000 k-mers that only the second round's smaller w can place.  The reference is the chain: two separate runs with `cat`
between them.  With --rounds_keep the process leaves the chain's files, every one byte for byte; without it the last round's files
and every round's .path / .agp, and no intermediate FASTA; <p>.rounds.agp applied to the original target reproduces every record
of the final scaffolds.  Every run is a child process under a time limit of its own."""
import gzip
import os
import random
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
LIMIT = ["timeout", "-k", "10", "120"]
K, W1, W2, N = 32, 1000, 100, 1
P = "run"
COMP = str.maketrans("ACGTUNMRWSYKVHDBacgtunmrwsykvhdb", "TGCAANKYWSRMBDHVtgcaankywsrmbdhv")   # bin/ntjoin_utils.py:145-150


def rc(s):
    return s[::-1].translate(COMP)


def fold(s, width=60):
    return "\n".join(s[p:p + width] for p in range(0, len(s), width)) + "\n"


def write_inputs(d):
    rng = random.Random(2024)
    ref = "".join(rng.choice("ACGT") for _ in range(44_000))
    contigs = [("ctgA", ref[0:8000]), ("ctgB", rc(ref[8100:16000])), ("ctgC", ref[16100:24000]),
               ("small1", ref[24100:25000]), ("small2", rc(ref[25100:26000])),          # 900 bases: fewer than w = 1000 k-mers
               ("ctgD", ref[26100:34000].lower()), ("small3", rc(ref[34100:35000])), ("small4", ref[35100:36000]),
               ("ctgE", rc(ref[36100:43900]))]
    order = [4, 0, 8, 3, 2, 6, 5, 1, 7]
    with open(os.path.join(d, "ref.fa"), "w") as fh:
        fh.write(">chr\n" + fold(ref, 70))
    with open(os.path.join(d, "tgt.fa"), "w") as fh:
        for i in order:
            fh.write(">" + contigs[i][0] + " a comment\n" + fold(contigs[i][1]))


def child(cwd, words):
    res = subprocess.run(LIMIT + words, cwd=cwd, env=ENV, capture_output=True, text=True, check=False)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-3000:])
    return res


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


def assemble(cwd, prefix, target, w, opts):
    child(cwd, [sys.executable, "-m", "ntjoin_amd.assemble", "-p", prefix, "-n", str(N), "-s", f"{target}.k{K}.w{w}.tsv", "-l", "1", "-r", "2",
                "-k", str(K), "--agp"] + opts + [f"ref.fa.k{K}.w{w}.tsv"])


def all_name(target, w, gz):
    return f"{target}.k{K}.w{w}.n{N}.all.scaffolds" + (".fa.gz" if gz else ".fa")


def cat_all(cwd, target, w, gz):
    "what `ntJoin-mx scaffold` does behind the run"
    stem = f"{target}.k{K}.w{w}.n{N}"
    ext = ".fa.gz" if gz else ".fa"
    a, u = read(os.path.join(cwd, stem + ".assigned.scaffolds" + ext)), read(os.path.join(cwd, stem + ".unassigned.scaffolds" + ext))
    with open(os.path.join(cwd, all_name(target, w, gz)), "wb") as fh:
        fh.write((a[:-28] if gz else a) + u)


@pytest.fixture(scope="module")
def chains(tmp_path_factory):
    "the chain of two separate runs per option set -> {key: directory}; made once"
    made = {}

    def get(overlap, gz=False):
        key = (overlap, gz)
        if key not in made:
            d = str(tmp_path_factory.mktemp("chain"))
            write_inputs(d)
            opts = (["--overlap"] if overlap else []) + (["--gz"] if gz else [])
            assemble(d, P, "tgt.fa", W1, opts)
            cat_all(d, "tgt.fa", W1, gz)
            t2 = all_name("tgt.fa", W1, gz)
            assemble(d, P + ".round2", t2, W2, opts)
            check_chain_joins(d)
            made[key] = d
        return made[key]
    return get


def check_chain_joins(d):
    "the second round joins something the first could not: a path of two or more nodes with an ntJoin<p> of round 1 and a '-' node"
    lines = read(os.path.join(d, P + ".round2.path")).decode().splitlines()[1:]
    good = 0
    for line in lines:
        nodes = re.findall(r"(\S+)([+-]):\d+-\d+", line.split("\t")[1])
        if len(nodes) >= 2 and any(re.fullmatch(r"ntJoin\d+", name) for name, _ in nodes) and any(ori == "-" for _, ori in nodes):
            good += 1
    assert good >= 1, lines
    first = read(os.path.join(d, P + ".path")).decode().splitlines()[1:]
    assert any(len(line.split("\t")[1].split()) >= 3 for line in first), first   # round 1 joined long contigs


def rounds_dir(tmp_path, overlap, keep, gz=False):
    d = str(tmp_path)
    write_inputs(d)
    opts = (["--overlap"] if overlap else []) + (["--gz"] if gz else []) + ["--rounds_w", str(W2)] + (["--rounds_keep"] if keep else [])
    assemble(d, P, "tgt.fa", W1, opts)
    return d


def fasta_records(data):
    out = []
    for block in data.decode().split(">")[1:]:
        head, _, body = block.partition("\n")
        out.append((head.split()[0] if head.split() else "", body.replace("\n", "").replace("\r", "")))
    return out


def check_rounds_agp(d, gz=False):
    "a small applier: <p>.rounds.agp over the original target gives every record of the final all.scaffolds file, names and bytes"
    contigs = dict(fasta_records(read(os.path.join(d, "tgt.fa"))))
    t2 = all_name("tgt.fa", W1, gz)
    stem = f"{t2}.k{K}.w{W2}.n{N}"
    ext = ".fa.gz" if gz else ".fa"
    final = b""
    for kind in ("assigned", "unassigned"):
        data = read(os.path.join(d, f"{stem}.{kind}.scaffolds{ext}"))
        final += gzip.decompress(data) if gz else data
    built, order, expect_at, expect_part, last_kind = {}, [], {}, {}, {}
    for line in read(os.path.join(d, P + ".rounds.agp")).decode().splitlines():
        obj, lo, hi, part, kind, c6, c7, c8, c9 = line.split("\t")
        if obj not in built:
            built[obj], expect_at[obj], expect_part[obj] = [], 1, 1
            order.append(obj)
        assert int(lo) == expect_at[obj] and int(part) == expect_part[obj], line
        if kind == "N":
            assert (c7, c8, c9) == ("scaffold", "yes", "align_genus"), line
            assert last_kind.get(obj) != "N", "two gap lines in a row: " + line
            text = "N" * int(c6)
        else:
            assert kind == "W" and c9 in "+-", line
            text = contigs[c6][int(c7) - 1:int(c8)]
            text = rc(text) if c9 == "-" else text
        assert int(hi) - int(lo) + 1 == len(text), line
        built[obj].append(text)
        last_kind[obj] = kind
        expect_at[obj] += len(text)
        expect_part[obj] += 1
    want = fasta_records(final)
    assert [(obj, "".join(built[obj])) for obj in order] == want
    assert len(want) >= 2 and any(name.startswith("ntJoin") for name, _ in want)
    # the composition went through both rounds: some object holds contigs that only the second round placed, and a '-' component
    agp = read(os.path.join(d, P + ".rounds.agp")).decode()
    assert re.search(r"^ntJoin\d+\t.*\tW\tsmall\d\t", agp, re.M) and re.search(r"\tW\tctg[A-E]\t\d+\t\d+\t-$", agp, re.M)


@pytest.mark.parametrize("overlap", [False, True], ids=["overlap_off", "overlap_on"])
def test_rounds_keep_leaves_the_chains_files(overlap, chains, tmp_path):
    chain = chains(overlap)
    d = rounds_dir(tmp_path, overlap, keep=True)
    names = sorted(os.listdir(chain))
    assert f"ref.fa.k{K}.w{W2}.tsv" in names and all_name("tgt.fa", W1, False) in names
    for name in names:
        assert os.path.exists(os.path.join(d, name)), name
        assert read(os.path.join(d, name)) == read(os.path.join(chain, name)), name
    assert sorted(set(os.listdir(d)) - set(names)) == [P + ".rounds.agp"]
    check_rounds_agp(d)


@pytest.mark.parametrize("overlap", [False, True], ids=["overlap_off", "overlap_on"])
def test_rounds_without_keep_leave_no_intermediate_fasta(overlap, chains, tmp_path):
    chain = chains(overlap)
    d = rounds_dir(tmp_path, overlap, keep=False)
    t2 = all_name("tgt.fa", W1, False)
    stem2 = f"{t2}.k{K}.w{W2}.n{N}"
    must = [P + ".path", P + ".agp", P + ".round2.path", P + ".round2.agp", P + ".round2.mx.dot", stem2 + ".assigned.scaffolds.fa",
            stem2 + ".unassigned.scaffolds.fa", f"{P}.round2.{t2}.k{K}.w{W2}.tsv.unassigned.bed", f"{t2}.k{K}.w{W2}.tsv", f"ref.fa.k{K}.w{W2}.tsv",
            P + ".rounds.agp"]
    have = sorted(os.listdir(d))
    for name in must:
        assert name in have, name
    for name in have:
        if name != P + ".rounds.agp":
            assert read(os.path.join(d, name)) == read(os.path.join(chain, name)), name
    stem1 = f"tgt.fa.k{K}.w{W1}.n{N}"
    for name in (t2, stem1 + ".assigned.scaffolds.fa", stem1 + ".unassigned.scaffolds.fa", P + ".mx.dot", f"{P}.tgt.fa.k{K}.w{W1}.tsv.unassigned.bed"):
        assert name not in have, name
    assert not [name for name in have if name.endswith(".tmp")]
    check_rounds_agp(d)


def test_make_front_end(chains, tmp_path):
    chain = chains(False)
    d = str(tmp_path)
    write_inputs(d)
    child(d, ["make", "-f", os.path.join(REPO, "ntJoin-mx"), "scaffold", "target=tgt.fa", "references=ref.fa", "reference_weights=2", f"k={K}",
              f"w={W1}", f"n={N}", "prefix=" + P, "agp=True", "overlap=False", f"rounds_w={W2}"])
    t2 = all_name("tgt.fa", W1, False)
    stem2 = f"{t2}.k{K}.w{W2}.n{N}"
    for name in (P + ".path", P + ".agp", P + ".round2.path", P + ".round2.agp", stem2 + ".assigned.scaffolds.fa", stem2 + ".unassigned.scaffolds.fa"):
        assert read(os.path.join(d, name)) == read(os.path.join(chain, name)), name
    assert read(os.path.join(d, stem2 + ".all.scaffolds.fa")) == read(os.path.join(chain, stem2 + ".assigned.scaffolds.fa")) + \
        read(os.path.join(chain, stem2 + ".unassigned.scaffolds.fa"))
    assert not os.path.exists(os.path.join(d, t2))
    check_rounds_agp(d)


def test_gz_once(chains, tmp_path):
    chain = chains(False, gz=True)
    d = rounds_dir(tmp_path, False, keep=True, gz=True)
    for name in sorted(os.listdir(chain)):
        assert read(os.path.join(d, name)) == read(os.path.join(chain, name)), name
    check_rounds_agp(d, gz=True)


def test_bad_rounds_w_is_refused(tmp_path):
    write_inputs(str(tmp_path))
    res = subprocess.run(LIMIT + [sys.executable, "-m", "ntjoin_amd.assemble", "-p", P, "-s", f"tgt.fa.k{K}.w{W1}.tsv", "-r", "2", "-k", str(K),
                                  "--rounds_w", "100 x", f"ref.fa.k{K}.w{W1}.tsv"], cwd=str(tmp_path), env=ENV, capture_output=True, text=True, check=False)
    assert res.returncode == 1 and "--rounds_w" in res.stdout
