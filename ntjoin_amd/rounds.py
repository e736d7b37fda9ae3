#!/usr/bin/env python3
"""
Scaffolding rounds in one process.  ntJoin is run in rounds: the all.scaffolds.fa of one run is the target of the
next, usually with a smaller w.  `python -m ntjoin_amd.assemble ... --rounds_w "500 250"` runs the round the TSV names declare and
then one more per entry, with the same k, n and options, under the names of the chain of separate runs the user would have typed:

    round i >= 2:  target T_i = T_{i-1}.k<k>.w<w_{i-1}>.n<n>.all.scaffolds.fa (.fa.gz with --gz), prefix <p>.round<i>

A round is a new handle (a handle has one w).  Between two rounds no file is read: the next target is the text the scaffold stage
left in device memory (MXG_SCAF_KEEP -> mxg_add_assembly_text_device), a reference whose TSV of the new w does not exist comes from
the text the old handle holds (mxg_assembly_text), and the old handle is closed as soon as the new one has taken its texts.  If the
device route refuses a text (MXG_ELIMIT, MXG_ENOMEM) the files of the round before are written and the target is read from T_i.
The last round writes everything a single run writes; an earlier round its .path and, with --agp, its .agp -- with --rounds_keep
every file the chain would leave.  <p>.rounds.agp spells every record of the last round's scaffolds over the records of the
original target: the rounds' piece tables (mxg_scaffold_pieces) composed on the device (mxg_compose_pieces), formatted here.
--synteny: the last round's scaffolds against the references, <p>.round<i>.synteny.paf beside that round's other files.
--assess: likewise, the last round's target and scaffolds: <p>.round<i>.assess.tsv and <p>.round<i>.breakpoints.bed.
--identity: likewise: <p>.round<i>.identity.tsv.
--lift: the BED files lie on the contigs of the first target and are lifted once, behind the last round, through the composed table
onto the last round's scaffolds: <p>.round<i>.<name>.lifted.bed and <p>.round<i>.<name>.unlifted.bed.

    python -m ntjoin_amd.rounds last_out TARGET K W N GZ W2 [W3 ...]   prints T_last.k<k>.w<w_last>.n<n> (for the make front-end)
"""
import copy
import os
import shutil
import sys

BGZF_EOF = 28   # bytes of the end marker behind a BGZF file


def chain(target_fa, k, w, n, rounds_w, gz):
    "-> [(target FASTA, w)] of every round, under the chain's names"
    out, fa = [], target_fa
    for wi in [w] + list(rounds_w):
        out.append((fa, wi))
        fa = f"{fa}.k{k}.w{wi}.n{n}.all.scaffolds" + (".fa.gz" if gz else ".fa")
    return out


def parse_rounds_w(text):
    ws = [int(tok) for tok in (text or "").split()]
    if any(w < 1 for w in ws):
        raise ValueError("--rounds_w: window sizes are positive integers")
    return ws


def write_all(files, gz):
    "the `all` file of a round as `ntJoin-mx scaffold` makes it: assigned, then unassigned (BGZF: one chain, one end marker)"
    out = files["assigned"].replace(".assigned.scaffolds.", ".all.scaffolds.")
    with open(out, "wb") as dst:
        with open(files["assigned"], "rb") as src:
            shutil.copyfileobj(src, dst)
        if gz:
            dst.seek(-BGZF_EOF, os.SEEK_END)
            dst.truncate()
        with open(files["unassigned"], "rb") as src:
            shutil.copyfileobj(src, dst)
    return out


def write_rounds_agp(path, pieces, first, ids, contig_ids):
    "_write_agp's lines for a piece table: W lines with 1-based inclusive component coordinates, N lines for the gaps"
    from . import capi
    rows = pieces.tolist()
    with open(path, "w", encoding="utf-8") as fh:
        for r, name in enumerate(ids):
            at = 1
            for part, (rec, start, end, kind) in enumerate(rows[int(first[r]):int(first[r + 1])], start=1):
                n = end - start
                if kind == capi.PIECE_GAP:
                    cols = (name, at, at + n - 1, part, "N", n, "scaffold", "yes", "align_genus")
                else:
                    cols = (name, at, at + n - 1, part, "W", contig_ids[rec], start + 1, end, "-" if kind == capi.PIECE_REV else "+")
                fh.write("\t".join(str(c) for c in cols) + "\n")
                at += n


def run_rounds(args, fasta, w, weights, rounds_w, keep_files=False):
    """fasta: {tsv name: FASTA} of round 1 as ntjoin_amd.assemble derives it.  Returns the files of every round, by kind."""
    from . import capi
    from .assemble import fail
    from .engine import MxError
    from .ntjoin import Ntjoin
    k, n, gz = int(args.k), int(args.n), bool(getattr(args, "gz", False))
    refs = [fasta[tsv] for tsv in args.FILES]
    rounds = chain(fasta[args.s], k, w, n, rounds_w, gz)
    prev, prov, contig_ids, contig_len, all_files = None, None, None, None, []
    try:
        for i, (target_fa, wi) in enumerate(rounds, start=1):
            last = i == len(rounds)
            full = last or keep_files
            a = copy.copy(args)
            a.p = args.p if i == 1 else f"{args.p}.round{i}"
            a.s = f"{target_fa}.k{k}.w{wi}.tsv"
            a.FILES = [f"{ref}.k{k}.w{wi}.tsv" for ref in refs]
            sketch, texts, no_tsv = {}, {}, set()
            if i == 1:
                if not os.path.exists(target_fa):
                    fail(f"the target FASTA {target_fa!r} does not exist (the scaffolds are cut from its text)")
                sketch[a.s] = target_fa
            else:
                sketch[a.s] = target_fa
                # (--gz --fai: the .gzi of a target is made of its BGZF file, where the chain's files are kept)
                if not (gz and getattr(args, "fai", False) and os.path.exists(target_fa)):
                    addr, n_bytes, _ = prev._engine.scaffold_text()
                    texts[a.s] = (addr, n_bytes)
                if not full:
                    no_tsv.add(a.s)   # (an intermediate target's TSV is one of the chain's files, not a checkpoint anybody reads)
            for r, (tsv, ref) in enumerate(zip(a.FILES, refs)):
                if os.path.exists(tsv):
                    continue
                if prev is not None:
                    try:
                        texts[tsv] = prev._engine.assembly_text(r)
                    except MxError as err:
                        if err.code != capi.MXG_EINVAL:
                            raise
                if tsv not in texts and not os.path.exists(ref):
                    fail(f"neither the sketch {tsv!r} nor the FASTA {ref!r} exists")
                sketch[tsv] = ref
            nj = Ntjoin(a, fasta=sketch, w=wi, device_text=texts, no_tsv=no_tsv)
            try:
                nj.weights_list = list(weights)
                try:
                    nj.load_minimizers_scaffold()
                except MxError as err:
                    if i == 1 or err.code not in (capi.MXG_ELIMIT, capi.MXG_ENOMEM):
                        raise
                    # the device route refuses a text: the files of the round before, and everything from files
                    print(f"ntjoin_amd: round {i}: {err}; reading {target_fa} from a file instead", file=sys.stderr)
                    nj.close()
                    if not os.path.exists(target_fa):
                        write_all(prev.print_scaffolds(**prev._last_print), gz)
                    nj = Ntjoin(a, fasta=sketch, w=wi, no_tsv=no_tsv)
                    nj.weights_list = list(weights)
                    nj.load_minimizers_scaffold()
                if prev is not None:
                    prev.close()
                    prev = None
                if i == 1:
                    tgt = len(nj._order) - 1
                    contig_ids = nj._engine.record_ids(tgt, nj._engine.n_records(tgt))
                    contig_len = nj._engine.record_lengths(tgt)
                # (lift=[]: the BED files are about the contigs of round 1, not about this round's target)
                files = nj.scaffold(keep=True, quiet=not full, lift=[], **({} if last else {"synteny": False, "assess": False, "identity": False}))
                if full and not last:
                    files["all"] = write_all(files, gz)
                pieces, first, ids = nj._engine.scaffold_pieces()
                if prov is not None:
                    pieces, first = nj._engine.compose_pieces(pieces, first, prov[0], prov[1])
                prov = (pieces, first)
                all_files.append(files)
            except BaseException:
                nj.close()
                raise
            prev = nj
        agp = args.p + ".rounds.agp"
        write_rounds_agp(agp, prov[0], prov[1], ids, contig_ids)
        all_files[-1]["rounds_agp"] = agp
        if getattr(args, "lift", None):
            all_files[-1].update(prev.lift_beds(args.lift, whole_only=bool(getattr(args, "lift_whole_only", False)),
                                                table=(prov[0], prov[1], ids, contig_ids, contig_len)))
    finally:
        if prev is not None:
            prev.close()
    return all_files


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) >= 7 and argv[0] == "last_out":
        target, k, w, n, gz = argv[1], int(argv[2]), int(argv[3]), int(argv[4]), argv[5] == "True"
        ws = [int(x) for x in argv[6:]]
        print(f"{chain(target, k, w, n, ws, gz)[-1][0]}.k{k}.w{ws[-1]}.n{n}")
        return 0
    sys.stderr.write(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main())
