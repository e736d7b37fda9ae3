#!/usr/bin/env python3
"""
Counterpart of the reference's bin/ntjoin_assemble.py as bin/ntjoin_run.py drives it: the whole scaffolder in one process on
one handle.  Same command line as ntjoin_amd.run (its parser, imported): the references' sketches FILES, the target's sketch
-s, all named <fasta>.k<k>.w<w>.tsv as ntJoin's makefile names them.

The target is always sketched from <fasta> (the scaffolds are cut from its text) and its TSV written as a by-product; a
reference is loaded from its TSV when that file exists and sketched from <fasta> otherwise.  Then Ntjoin.scaffold():
graph -> find_paths -> format_paths -> adjust_paths -> trim_overlaps (--overlap) -> print_scaffolds.  Written, under the
reference's names: <p>.mx.dot, <p>.path, <p>.agp (--agp), <fasta>.k<k>.w<w>.n<n>.assigned.scaffolds.fa,
...unassigned.scaffolds.fa and <p>.<target tsv>.unassigned.bed.  -t and --btllib_t are accepted and unused.
--fai: also <fasta>.fai of the target and of every reference sketched from FASTA in this run (what the reference's `%.fai: %` rule
makes with `samtools faidx`, ntJoin:152-153, 207-208), <fasta>.gzi of a BGZF input, and the .fai (with --gz: and .gzi) of the two
scaffold files; a reference loaded from its TSV gets a line on stderr instead.
--report (--report_min_gap, --report_min_len): also <p>.report.tsv -- records, bases, base composition, N gaps, N50 and the like at
scaffold and at contig level, one row per input read from FASTA in this run and per scaffold file (assigned, unassigned, all),
computed on the GPU from the text the handle holds and from the scaffold files on their way out (ntjoin_amd/report.py).
--synteny (--synteny_max_gap, --synteny_min_anchors, --synteny_min_span): also <p>.synteny.paf -- the maximal collinear runs of shared
unique minimizers between the scaffolds (the records of the assigned, then of the unassigned file) and every reference, one PAF line
per run, computed on the GPU from the graph; a reference loaded from its TSV needs <fasta>.fai for its lengths, or is left out.
--assess (--assess_merge_gap, --assess_max_indel, --assess_join_indel): also <p>.assess.tsv and <p>.breakpoints.bed -- the target and
the scaffolds against every reference: the blocks of --synteny_* merged into chains, aligned and covered bases, NA50 / NGA50 / NG50,
and the breakpoints by kind, each blamed on a join the scaffolder made or on a contig; computed on the GPU (ntjoin_amd/report.py).
--identity (--identity_max_seg): also <p>.identity.tsv -- the target and the scaffolds against every reference: the edit distances of
the stretches between neighbouring minimizers of the blocks of --synteny_*, summed, and edits per 100 kbp; with --synteny the PAF lines
carry al:i, NM:i and dv:f; computed on the GPU.  A reference loaded from its TSV has no text in the handle and is left out.
--lift a.bed [b.bed ...] (--lift_whole_only): also <p>.<a>.lifted.bed and <p>.<a>.unlifted.bed per file -- the BED features of the
target's records in scaffold coordinates, carried through the scaffolds' piece table on the GPU: one line per piece a feature lands
in, column 4 on unchanged, the strand flipped on a reversed piece; what is not lifted whole also goes to the unlifted file behind its
reason.  The list of files ends at the next option.  With --rounds_w: once, behind the last round, from the first target's contigs.
--rounds_w "500 250" (--rounds_keep): further rounds with these window sizes in the same process, the scaffolds of a round being the
target of the next without a file between them, and <p>.rounds.agp over the contigs of the first target (ntjoin_amd/rounds.py).
"""
import os
import re
import sys

from .run import parse_arguments, set_weights

TSV_NAME = re.compile(r"^(.+)\.k(\d+)\.w(\d+)\.tsv$")


def fail(message):
    "one line on stdout and exit status 1, as the reference reports a bad command line (bin/ntjoin_assemble.py:788-797)"
    sys.stdout.write("ERROR: " + message + "\n")
    sys.exit(1)


def derive_names(args):
    "-> ({tsv name: fasta name} for -s and every FILES entry, w); ends the run when a name does not carry this run's k and one w"
    fasta, ws = {}, set()
    for tsv in [args.s] + list(args.FILES):
        match = TSV_NAME.match(tsv)
        if not match:
            fail(f"{tsv!r} is not named <fasta>.k<k>.w<w>.tsv")
        if int(match.group(2)) != args.k:
            fail(f"{tsv!r} names k={int(match.group(2))} but -k is {args.k}")
        fasta[tsv] = match.group(1)
        ws.add(int(match.group(3)))
    if len(ws) != 1:
        fail(f"the sketches name different window sizes (w = {sorted(ws)}); one run has one w")
    return fasta, ws.pop()


def sources(args, fasta):
    "-> {tsv name: fasta to sketch}: the target always, a reference only when its TSV does not exist yet"
    sketch = {}
    if not os.path.exists(fasta[args.s]):
        fail(f"the target FASTA {fasta[args.s]!r} does not exist (the scaffolds are cut from its text)")
    sketch[args.s] = fasta[args.s]
    for tsv in args.FILES:
        if os.path.exists(tsv):
            continue
        if not os.path.exists(fasta[tsv]):
            fail(f"neither the sketch {tsv!r} nor the FASTA {fasta[tsv]!r} exists")
        sketch[tsv] = fasta[tsv]
    return sketch


def main(argv=None):
    args = parse_arguments(argv)
    fasta, w = derive_names(args)
    sketch = sources(args, fasta)
    weights = set_weights(args)
    from . import rounds
    try:
        rounds_w = rounds.parse_rounds_w(args.rounds_w)
    except ValueError:
        fail(f"--rounds_w {args.rounds_w!r}: window sizes are positive integers, blank-separated")
    if rounds_w:
        rounds.run_rounds(args, fasta, w, weights, rounds_w, keep_files=args.rounds_keep)
        return 0
    from .ntjoin import Ntjoin  # (behind the checks: importing it loads the library)
    nj = Ntjoin(args, fasta=sketch, w=w)
    nj.weights_list = weights
    try:
        nj.load_minimizers_scaffold()
        nj.scaffold()
    finally:
        nj.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
