#!/usr/bin/env python3
"""
Counterpart of the reference's bin/ntjoin_run.py (argument surface: reference bin/ntjoin_run.py:10-60) for the
hot path only: load the minimizer TSVs (references in CLI order, then the target -s), run the graph stage on the
GPU and write <prefix>.mx.dot, exactly the state the reference has after `make_minimizer_graph()`
(reference bin/ntjoin_assemble.py:751-757).  Everything downstream (path finding, scaffolding, AGP) stays the
reference's Python and is out of scope here; flags that only matter downstream are accepted and ignored.
"""
import argparse
import sys

from .ntjoin import Ntjoin


def parse_arguments(argv=None):
    """same flag names, defaults and required-ness as the reference's parser (bin/ntjoin_run.py:10-60), so that its Makefile
    recipe runs unchanged; the descriptions are ours"""
    parser = argparse.ArgumentParser(description="ntJoin hot path on MI355X: minimizer TSVs -> <prefix>.mx.dot")
    parser.add_argument("FILES", nargs="+", help="sketches of the reference assemblies (indexlr TSVs), in the order their weights are given")
    parser.add_argument("-s", required=True, help="sketch (indexlr TSV) of the assembly to be scaffolded")
    parser.add_argument("-l", required=False, default=1, type=float, help="edge weight contributed by the target assembly (default 1)")
    parser.add_argument("-r", required=True, type=str, help="one edge weight per reference, blank-separated inside one quoted argument")
    parser.add_argument("-p", default="out", type=str, required=False, help="prefix of the files written (default: out)")
    parser.add_argument("-n", default=1, type=int, help="edges lighter than this are dropped downstream (default 1; not used by the graph build)")
    parser.add_argument("-k", required=True, type=int, help="the k the sketches were computed with")
    parser.add_argument("-g", required=False, default=20, type=int, help="downstream only: smallest gap written between joined pieces")
    parser.add_argument("-G", required=False, default=0, type=int, help="downstream only: largest gap allowed, 0 = unlimited")
    # flags of the stages behind the graph build: accepted so that the reference's command line parses, otherwise unused here
    parser.add_argument("--mkt", action="store_true")
    parser.add_argument("-m", type=int, default=90, required=False)
    parser.add_argument("-t", type=int, default=1)
    parser.add_argument("--agp", action="store_true")
    parser.add_argument("--no_cut", action="store_true")
    parser.add_argument("--overlap", action="store_true")
    parser.add_argument("--overlap_gap", type=int, default=20)
    parser.add_argument("--overlap_k", type=int, default=15)
    parser.add_argument("--overlap_w", type=int, default=10)
    parser.add_argument("--btllib_t", type=int, default=4)
    # ours (the reference has no such flag): the scaffold FASTA files as BGZF, ...scaffolds.fa.gz (ntjoin_amd.assemble)
    parser.add_argument("--gz", action="store_true", default=False)
    # ours: <fasta>.fai of the target, of every reference read from FASTA and of the scaffold files, .gzi for the BGZF ones
    # (what the reference's `%.fai: %` rule makes with samtools faidx, ntJoin:152-153, 207-208; ntjoin_amd.assemble)
    parser.add_argument("--fai", action="store_true", default=False)
    # ours: <prefix>.report.tsv -- contiguity, base composition and N gaps of the inputs read from FASTA and of the scaffold files,
    # computed on the GPU (the alignment-free part of the reference's `analysis` target, ntJoin:158-161, 244-252; ntjoin_amd.assemble)
    parser.add_argument("--report", action="store_true", default=False)
    parser.add_argument("--report_min_gap", type=int, default=10, help="an N run of at least this many bases is a gap [10]")
    parser.add_argument("--report_min_len", type=int, default=500, help="N50 and the like are taken over lengths of at least this [500]")
    # ours: scaffolding rounds in one process (ntjoin_amd/rounds.py): one more round per window size listed, the scaffolds of a round
    # being the target of the next without a file between them; --rounds_keep: every round leaves every file the chain of runs would
    parser.add_argument("--rounds_w", type=str, default=None, help="window sizes of further rounds, blank-separated inside one quoted argument")
    parser.add_argument("--rounds_keep", action="store_true", default=False)
    # ours: <prefix>.synteny.paf -- the maximal collinear runs of shared unique minimizers between the scaffolds and every reference, as
    # PAF for a dot-plot viewer, computed on the GPU from the graph (the alignment-free answer to what the reference's `analysis` target
    # runs minimap2 for, ntJoin:158-161, 238-242; ntjoin_amd.assemble)
    parser.add_argument("--synteny", action="store_true", default=False)
    parser.add_argument("--synteny_max_gap", type=int, default=100000,
                        help="largest distance between neighbouring anchors of a block, 0 = none [100000: QUAST's --scaffold-gap-max-size in ntJoin:247]")
    parser.add_argument("--synteny_min_anchors", type=int, default=3, help="smallest number of minimizers of a block, at least 2 [3]")
    parser.add_argument("--synteny_min_span", type=int, default=0, help="smallest extent of a block on the scaffold [0]")
    # ours: <prefix>.assess.tsv and <prefix>.breakpoints.bed -- the target and the scaffolds against every reference: the blocks above
    # merged into chains, aligned and covered bases, NA50 / NGA50 / NG50 and the breakpoints by kind, each blamed on a join or on a
    # contig; computed on the GPU (what the reference's `analysis` target runs QUAST for, ntJoin:243-252; ntjoin_amd.assemble).  The
    # blocks are made with the --synteny_* parameters
    parser.add_argument("--assess", action="store_true", default=False)
    parser.add_argument("--assess_merge_gap", type=int, default=100000,
                        help="largest gap between blocks of a chain, 0 = none [100000: QUAST's --scaffold-gap-max-size in ntJoin:247]")
    parser.add_argument("--assess_max_indel", type=int, default=1000,
                        help="largest difference of the two gaps between blocks of a chain inside a contig, 0 = none [1000: QUAST's --extensive-mis-size]")
    parser.add_argument("--assess_join_indel", type=int, default=100000, help="the same across a join of the scaffolder, 0 = none [100000]")
    # ours: <prefix>.identity.tsv -- how similar the target and the scaffolds are to every reference inside the blocks above: banded
    # edit distances of the stretches between neighbouring minimizers of a block, summed (QUAST's mismatches and indels per 100 kbp;
    # with --synteny the PAF lines also carry al:i, NM:i and dv:f); computed on the GPU (ntjoin_amd.assemble).  The blocks are made
    # with the --synteny_* parameters
    parser.add_argument("--identity", action="store_true", default=False)
    parser.add_argument("--identity_max_seg", type=int, default=10000,
                        help="stretches longer than this on either assembly are counted, not aligned, at least 1 [10000]")
    # ours: BED files over the target's records lifted onto the scaffolds, <prefix>.<name>.lifted.bed and <prefix>.<name>.unlifted.bed
    # for <name>.bed: cuts, reverse complements, trimmed overlaps and the rounds' renaming followed through the scaffolds' piece table
    # on the GPU (ntjoin_amd.assemble).  Another option, or the end of the command line, ends the list of files
    parser.add_argument("--lift", nargs="+", default=[], metavar="BED", help="BED files of features on the target's records to lift onto the scaffolds")
    parser.add_argument("--lift_whole_only", action="store_true", default=False,
                        help="lift only the features that land whole in one piece; the others go to the unlifted file alone")
    parser.add_argument("-v", "--version", action="version", version="ntjoin_amd hot path (ntJoin v1.1.5 compatible)")
    return parser.parse_args(argv)


def set_weights(args):
    """-r as a list of floats, one per reference TSV; a count mismatch ends the run with status 1, as in the reference
    (bin/ntjoin_assemble.py:788-797: same condition, same exit status)"""
    weights = [float(tok) for tok in args.r.split()]
    if len(weights) == len(args.FILES):
        return weights
    sys.stdout.write(f"ERROR: -r lists {len(weights)} weight(s) but {len(args.FILES)} reference sketch file(s) were given; "
                     "there must be exactly one weight per reference, in the same order.\n")
    sys.exit(1)


def main(argv=None):
    args = parse_arguments(argv)
    nj = Ntjoin(args)
    nj.weights_list = set_weights(args)
    try:
        nj.load_minimizers_scaffold()
        nj.make_minimizer_graph(materialize=False)
    finally:
        nj.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
