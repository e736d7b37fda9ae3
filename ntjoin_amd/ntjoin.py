"""
Counterpart of the reference's `Ntjoin` base class for the hot path only (reference bin/ntjoin.py:
load_minimizers :178-186, make_minimizer_graph :189-204, print_graph :25-67) plus the target-loading step of
NtjoinScaffolder.load_minimizers_scaffold (reference bin/ntjoin_assemble.py:799-807).

Fused: all assemblies live in ONE engine handle; sketches stay in HBM between load and graph build; the
`.mx.dot` is written by the library.  `args` carries the same attributes the reference reads:
    args.FILES  reference minimizer TSVs (CLI order)      args.s  target TSV        args.l  target weight
    args.p      output prefix                               args.k  k-mer size
Instead of TSVs the engine can sketch FASTA directly: pass fasta={tsv_name: fasta_path} and the TSVs are
WRITTEN (checkpoint files, ntJoin:202 `.SECONDARY`) rather than read.
"""
import datetime
import math
import os
import re
import sys

import numpy as np

from . import capi
from .engine import MxEngine, MxError
from .ntjoin_utils import MxGraph, sketch_views
from .report import ASSESS_COLUMNS, COLUMNS as REPORT_COLUMNS, IDENTITY_COLUMNS, assess_row, breakpoint_lines, identity_row, row as report_row

COLOURS = ["red", "green", "blue", "purple", "orange", "turquoise", "pink", "yellow", "orchid", "salmon"]

MK_Z975 = 1.959963984540054  # scipy.stats.norm.ppf(0.975): original_test's threshold on |z| at alpha = 0.05
_SQRT1_2 = 0.7071067811865476
def lift_outputs(prefix, bed):
    "the two files --lift makes of the BED file `bed`: <prefix>.<basename without a trailing .bed>.lifted.bed and ...unlifted.bed"
    stem = os.path.basename(str(bed))
    if stem.endswith(".bed"):
        stem = stem[:-4]
    return f"{prefix}.{stem}.lifted.bed", f"{prefix}.{stem}.unlifted.bed"


SYNTENY_DEFAULTS = dict(max_gap=100000, min_anchors=3, min_span=0)  # write_synteny's and write_assess's, of the blocks call


def _norm_cdf(a):
    "the standard normal CDF as scipy.special.ndtr (what norm.cdf evaluates) forms it, on math.erf / math.erfc"
    x = a * _SQRT1_2
    z = abs(x)
    if z < _SQRT1_2:
        return 0.5 + 0.5 * math.erf(x)
    y = 0.5 * math.erfc(z)
    return 1.0 - y if x > 0 else y


def mk_orientation(n, s, tie_term):
    """--mkt decision of determine_orientation (reference bin/ntjoin_assemble.py:37-40) for a run of n positions with
    Mann-Kendall score s and tie term sum t(t-1)(2t+5): pymannkendall.original_test's z, p and h, then '+' / '-' when
    h and p <= 0.05, else '?'.  (p is kept as the reference computes it: near |z| = 1.96 it can exceed 0.05 while h holds.)"""
    n, s, tie_term = int(n), int(s), int(tie_term)
    var = (n * (n - 1) * (2 * n + 5) - tie_term) / 18
    if s > 0:
        z = (s - 1) / math.sqrt(var)
    elif s < 0:
        z = (s + 1) / math.sqrt(var)
    else:
        z = 0.0
    p = 2 * (1 - _norm_cdf(abs(z)))
    h = abs(z) > MK_Z975
    if h and p <= 0.05:
        return "+" if z > 0 else "-"
    return "?"


class Ntjoin:
    "ntJoin hot path: minimizer sketches -> minimizer graph, on the GPU"

    def __init__(self, args, fasta=None, w=None, variant="v2", device_text=None, no_tsv=()):
        self.list_mx_info = {}  # assembly -> {mx: (contig, position)}
        self.list_mxs = {}      # assembly -> [lists of mx]
        self._graph = None
        self._graph_pending = False
        self.args = args
        self.weights = {}
        self.weights_list = []
        self._fasta = dict(fasta or {})
        if self._fasta and w is None:
            # (w is only unused on the TSV route; sketching with a default of 1 would write a huge, wrong checkpoint file)
            raise ValueError("Ntjoin(fasta=...): the window size w must be given when assemblies are sketched from FASTA")
        self._engine = MxEngine(k=int(getattr(args, "k", 32)), w=int(w if w is not None else 1), variant=variant)
        self._order = []
        # rounds (ntjoin_amd/rounds.py): {tsv name: (device address, bytes)} of FASTA texts that lie in device memory already -- the
        # assembly named in `fasta` is then loaded from that text, not from its file -- and the names whose TSV is not to be written
        self._device_text = dict(device_text or {})
        self._no_tsv = set(no_tsv)
        self._last_print = None

    def close(self):
        self._engine.close()

    @property
    def graph(self):
        if self._graph is None and getattr(self, "_graph_pending", False):
            g = self._engine.get_graph()
            self._graph = MxGraph.from_arrays(g["vertex_hash"], g["edge_u"], g["edge_v"], g["edge_support"], g["edge_weight"],
                                              self._order)
            self._graph_pending = False
        return self._graph

    @graph.setter
    def graph(self, value):
        self._graph = value
        self._graph_pending = False

    # -- loading (reference order: refs in FILES order, then target) --------------------------------------
    def _add(self, assembly, weight):
        if assembly in self._fasta:
            if assembly in self._device_text:
                a = self._engine.add_text_device(assembly, weight, *self._device_text[assembly])
            else:
                a = self._engine.add_fasta(assembly, weight, self._fasta[assembly])
            self._engine.sketch(a)
            if assembly not in self._no_tsv:
                self._engine.write_tsv(a, assembly, with_pos=True, with_strand=False, with_seq=True)
        else:
            print(datetime.datetime.today(), ": Reading minimizers", assembly, file=sys.stdout)
            a = self._engine.add_tsv(assembly, weight, assembly)
        self._order.append(assembly)
        self.weights[assembly] = weight
        return a

    def load_minimizers(self, repeat_bf=False):
        "Load in minimizers for ntJoin scaffolding mode"
        if repeat_bf:
            raise NotImplementedError("repeat_bf is never supplied on ntJoin's own path")
        for assembly in self.args.FILES:
            self._add(assembly, float(self.weights_list.pop(0)))

    def load_minimizers_scaffold(self):
        "Load in minimizers for ntJoin scaffolding mode (references, then the target)"
        self.load_minimizers()
        self._add(self.args.s, float(self.args.l))

    # -- graph ----------------------------------------------------------------------------------------------
    def make_minimizer_graph(self, materialize=True):
        "Run ntJoin graph stage"
        print(datetime.datetime.today(), ": Generating minimizer graph ...\n")
        weight_str = "\n".join([f"{assembly}: {asm_weight}" for assembly, asm_weight in self.weights.items()])
        print("\nWeights of assemblies:\n", weight_str, "\n", sep="", flush=True)
        print(datetime.datetime.today(), ": Filtering minimizers", file=sys.stdout)
        print(datetime.datetime.today(), ": Building graph", file=sys.stdout)
        eng = self._engine
        eng.build_graph()
        if not materialize:
            # only the .mx.dot is wanted (ntjoin_amd.run): the library writes it from its own arrays; no Python object
            # per vertex or edge is made (4.5 M vertices at 3 Gbp + 3 Gbp: seconds of str() and dict inserts) unless
            # somebody asks for self.graph afterwards (then: the array-backed container, built on first use)
            self._graph = None
            self._graph_pending = True
            self.print_graph(None)
            return
        g = eng.get_graph()
        if materialize == "views":
            # array-backed state for genome-scale inputs: same objects to index and iterate, no per-minimizer Python work
            self.graph = MxGraph.from_arrays(g["vertex_hash"], g["edge_u"], g["edge_v"], g["edge_support"], g["edge_weight"],
                                             self._order)
            for a, assembly in enumerate(self._order):
                sk = eng.get_sketch(a)
                uniq = (eng.get_mx_flags(a) & capi.MX_UNIQUE) != 0
                self.list_mx_info[assembly], self.list_mxs[assembly] = sketch_views(sk, uniq)
            self.print_graph(self.graph)
            return
        names = [str(h) for h in g["vertex_hash"].tolist()]
        support = [[self._order[b] for b in range(len(self._order)) if m >> b & 1] for m in g["edge_support"].tolist()]
        self.graph = MxGraph(names, zip(g["edge_u"].tolist(), g["edge_v"].tolist()), support,
                             g["edge_weight"].tolist())
        if materialize:
            # the state later stages of the reference read
            for a, assembly in enumerate(self._order):
                sk = eng.get_sketch(a)
                flags = eng.get_mx_flags(a)
                ids = sk["record_ids"]
                uniq = (flags & capi.MX_UNIQUE) != 0
                self.list_mx_info[assembly] = {
                    str(h): (ids[r], int(p)) for h, p, r in
                    zip(sk["out_hash"][uniq].tolist(), sk["pos"][uniq].tolist(), sk["record"][uniq].tolist())}
                first = sk["record_first"]
                lists = []
                for r in range(len(ids)):
                    lo, hi = int(first[r]), int(first[r + 1])
                    if hi > lo:
                        lists.append([str(x) for x in sk["out_hash"][lo:hi][uniq[lo:hi]].tolist()])
                self.list_mxs[assembly] = lists
        self.print_graph(self.graph)

    def find_paths(self):
        "Finds paths through the minimizer graph (global filter with args.n, branch filtering, linear paths)"
        print(datetime.datetime.today(), ": Finding paths", file=sys.stdout)
        found = self._engine.find_paths(int(getattr(self.args, "n", 1)))
        self._found = found
        by_comp = {}
        for comp, verts in found:
            by_comp.setdefault(comp, []).append(([self.graph.names[v] for v in verts], None))
        n_comp = self._engine.n_components
        print("\nTotal number of components in graph:", n_comp, "\n", sep=" ", file=sys.stdout, flush=True)
        # one list per component, as the reference returns (components without an accepted path give [])
        return list(by_comp.values()) + [[] for _ in range(n_comp - len(by_comp))]

    # -- what the scaffolder derives from the paths (reference bin/ntjoin_assemble.py) -----------------------------
    def find_mx_min_max(self, target):
        "Given the target assembly, find the min/max position of its graph-vertex minimizers per contig (:688-702)"
        a = self._order.index(target)
        ids = self._engine.record_ids(a, self._engine.n_records(a))
        return {ids[r]: e for r, e in enumerate(self._engine.mx_extremes(a)) if e is not None}

    @staticmethod
    def determine_orientation(n, inc, dec, m=90):
        "orientation of a run of n minimizers with inc / dec increasing / decreasing consecutive pairs (:30-50, no --mkt)"
        if n > 1:
            if dec == 0 and inc == n - 1:
                return "+"
            if inc == 0 and dec == n - 1:
                return "-"
            positive = inc / float(n - 1) * 100
            if positive >= m:
                return "+"
            if 100 - positive >= m:
                return "-"
        return "?"

    @staticmethod
    def _orientation_mkt(n, inc, dec, s, tie_term):
        "determine_orientation with --mkt: the strictly monotone checks first, then the Mann-Kendall test (:32-40)"
        if n > 1:
            if dec == 0 and inc == n - 1:
                return "+"
            if inc == 0 and dec == n - 1:
                return "-"
            return mk_orientation(n, s, tie_term)
        return "?"

    NO_LENGTHS = ("format_paths: the target was loaded from a minimizer TSV, which holds no contig lengths; "
                  "pass lengths={contig: length}")

    def format_paths(self, lengths=None, g=20, G=0, m=90, mkt=False):
        """format_path (:175-218) for every path of the last find_paths() and the target assembly: one list per path of
        [contig, ori, start, end, contig_size, first_mx, terminal_mx, gap_size, raw_gap_size].  Runs, orientations (the m rule,
        or with mkt=True the Mann-Kendall test), coordinates and the gap estimates of calculate_gap_size (:67-113) are the
        library's (mxg_format_paths: one call for all paths, from what the graph and path stages left on the device); only the
        rows are made here, with the minimizer hashes of the nodes' endpoints.  An engine without the call goes the host route
        (_format_paths_host)."""
        eng = self._engine
        if not hasattr(eng, "format_paths"):
            return self._format_paths_host(lengths, g, G, m, mkt)
        tgt = len(self._order) - 1
        ids = eng.record_ids(tgt, eng.n_records(tgt))
        lens = None if lengths is None else [lengths.get(c, 0) for c in ids]
        try:
            nodes = eng.format_paths(tgt, g=g, G=G, m=m, mkt=mkt, lengths=lens)
        except MxError as err:
            nodes = getattr(err, "nodes", None)
            if nodes is None:
                if lengths is None and err.code == capi.MXG_EINVAL and ids and not any(eng.record_lengths(tgt)):
                    raise ValueError(self.NO_LENGTHS) from None
                raise
            self._need_lengths(nodes, ids, lengths)
            # the view is filled: the error is the negative overhang, whose message names the first such path and node
            where = re.search(r"path (\d+) node (\d+)", str(err))
            if not where:
                raise
            path = self._node_rows(nodes, ids)[int(where.group(1))]
            u, v = path[int(where.group(2))], path[int(where.group(2)) + 1]
            raise ValueError(f"Gap distance estimation less than 0 between {u} and {v}") from None
        self._need_lengths(nodes, ids, lengths)
        return self._node_rows(nodes, ids)

    @staticmethod
    def _need_lengths(nodes, ids, lengths):
        "KeyError, as lengths[contig] of the host route gives, for a contig of some node that lengths does not hold"
        if lengths is not None:
            for r in np.unique(nodes["record"]).tolist():
                if ids[r] not in lengths:
                    raise KeyError(ids[r])

    def _node_rows(self, nodes, ids):
        "the rows of format_paths from the arrays of MxEngine.format_paths: one list per path"
        first_mx = self._engine.vertex_hashes(nodes["first_vertex"])
        terminal_mx = self._engine.vertex_hashes(nodes["terminal_vertex"])
        rows = [list(r) for r in zip(
            [ids[r] for r in nodes["record"].tolist()], ["-" if r else "+" for r in nodes["reverse"].tolist()],
            nodes["start"].tolist(), nodes["end"].tolist(), nodes["contig_size"].tolist(), map(str, first_mx.tolist()),
            map(str, terminal_mx.tolist()), nodes["gap_size"].tolist(), nodes["raw_gap_size"].tolist())]
        at = nodes["node_first"].tolist()
        return [rows[lo:hi] for lo, hi in zip(at, at[1:])]

    def _format_paths_host(self, lengths=None, g=20, G=0, m=90, mkt=False):
        """format_path (:175-218) for every path of the last find_paths() and the target assembly: one list per path of
        [contig, ori, start, end, contig_size, first_mx, terminal_mx, gap_size, raw_gap_size].  The per-minimizer work
        (grouping by contig, min/max, orientation tallies) is the library's (mxg_path_segments, mxg_mx_extremes); the
        gap estimate between two oriented runs (calculate_gap_size :68-112) reads a handful of graph entries here.
        mkt=True (ntJoin --mkt): a run that is not strictly monotone is decided by the Mann-Kendall test (mk_orientation on
        the library's mxg_path_segments_mk) instead of the m percentage rule."""
        eng, k = self._engine, int(getattr(self.args, "k", 32))
        tgt = len(self._order) - 1
        ids = eng.record_ids(tgt, eng.n_records(tgt))
        if lengths is None:
            lens = eng.record_lengths(tgt)
            if ids and not any(lens):
                # a target loaded from its TSV carries no record lengths (the reference takes them from the FASTA index,
                # calc_end_coord / scaffolds[ctg].length): silently using 0 would put every contig end at 0
                raise ValueError("format_paths: the target was loaded from a minimizer TSV, which holds no contig lengths; "
                                 "pass lengths={contig: length}")
            lengths = dict(zip(ids, lens))
        ext = eng.mx_extremes(tgt)
        seg = eng.path_segments(tgt)
        gr = eng.get_graph()
        vpos, names = gr["vertex_pos"], self.graph.names
        masks = {(min(u, v), max(u, v)): int(s) for u, v, s in
                 zip(gr["edge_u"].tolist(), gr["edge_v"].tolist(), gr["edge_support"].tolist())}
        offsets, at = [], 0
        for _comp, verts in self._found:
            offsets.append(at)
            at += len(verts)
        out = [[] for _ in self._found]
        kept = [[] for _ in self._found]
        cols = [seg[c].tolist() for c in ("path", "record", "first", "n", "min_pos", "max_pos", "inc", "dec")]
        if mkt:
            mk = eng.path_segments_mk(tgt)
            oris = [self._orientation_mkt(n, inc, dec, s, t) for n, inc, dec, s, t in
                    zip(cols[3], cols[6], cols[7], mk["s"].tolist(), mk["tie_term"].tolist())]
        for i, (p, rec, first, n, mn, mx, inc, dec) in enumerate(zip(*cols)):
            ori = oris[i] if mkt else self.determine_orientation(n, inc, dec, m)
            if ori == "?":
                continue
            ctg, verts, lo = ids[rec], self._found[p][1], first - offsets[p]
            start = 0 if mn == ext[rec][0] else mn
            end = lengths[ctg] if mx == ext[rec][1] else mx + k
            out[p].append([ctg, ori, start, end, lengths[ctg], names[verts[lo]], names[verts[lo + n - 1]], 0, 0])
            kept[p].append((lo, lo + n - 1))
        for p, nodes in enumerate(out):
            verts = self._found[p][1]
            for i in range(len(nodes) - 1):
                u, v = nodes[i], nodes[i + 1]
                iu, iv = kept[p][i][1], kept[p][i + 1][0]
                common = -1
                for a_, b_ in zip(verts[iu:iv], verts[iu + 1:iv + 1]):
                    common &= masks[(min(a_, b_), max(a_, b_))]
                sup = [b for b in range(len(self._order)) if common >> b & 1]
                if not sup:
                    u[7], u[8] = g, g
                    continue
                um, vm = verts[iu], verts[iv]
                dists = [abs(int(vpos[b][vm]) - int(vpos[b][um])) for b in sup]
                mean_dist = int(sum(dists) / len(dists)) - k
                upos, vpos_t = int(vpos[tgt][um]), int(vpos[tgt][vm])
                a_over = (u[3] - upos - k) if u[1] == "+" else (upos - u[2])
                b_over = (vpos_t - v[2]) if v[1] == "+" else (v[3] - vpos_t - k)
                if a_over < 0 or b_over < 0:
                    raise ValueError(f"Gap distance estimation less than 0 between {u} and {v}")
                gap = max(mean_dist - a_over - b_over, g)
                if G > 0:
                    gap = min(gap, G)
                u[7], u[8] = gap, mean_dist - a_over - b_over
        return out

    def adjust_paths(self, paths, no_cut=False, G=0):
        """What main_scaffolder does to the paths between format_path and the scaffolds (:775-784 and :549-553) for paths as
        format_paths() returns them: relocated pieces of one contig merged (merge_relocations :126-172, before and after the rest),
        with no_cut whole contigs instead of cut ones (adjust_paths :266-305; G clamps the gaps it accumulates), regions of one
        contig that overlap resolved (tally_intersecting_segments :661-686, remove_overlapping_regions :451-466), the last
        oriented node's gap zeroed.  One library call for all paths (mxg_adjust_paths); rows of the same shape come back, one list
        per input path (a path may come back with one node or none), ready for trim_overlaps and print_scaffolds.  Where the
        reference raises KeyError (two nodes with the same contig, start and end, one of which merges) MxError names the node."""
        flat = [nd for path in paths for nd in path]
        index, tags = {}, {}
        nodes = np.zeros(len(flat), dtype=MxEngine.ADJUST_NODE)
        nodes["record"] = [index.setdefault(nd[0], len(index)) for nd in flat]
        nodes["ori"] = ["+-?".index(nd[1]) for nd in flat]
        for col, name in ((2, "start"), (3, "end"), (4, "contig_size"), (7, "gap_size"), (8, "raw_gap_size")):
            nodes[name] = [nd[col] for nd in flat]
        for col, name in ((5, "first_mx"), (6, "terminal_mx")):  # opaque to the library: any hashable tag
            nodes[name] = [tags.setdefault(nd[col], len(tags)) for nd in flat]
        first = np.cumsum([0] + [len(path) for path in paths]).astype(np.uint64)
        res = self._engine.adjust_paths(nodes, first, no_cut=no_cut, G=G)
        contigs, tag_of, nd = list(index), list(tags), res["nodes"]
        rows = [[contigs[r], "+-?"[o], s, e, size, tag_of[f], tag_of[t], gap, raw] for r, o, s, e, size, f, t, gap, raw in zip(
            nd["record"].tolist(), nd["ori"].tolist(), nd["start"].tolist(), nd["end"].tolist(), nd["contig_size"].tolist(),
            nd["first_mx"].tolist(), nd["terminal_mx"].tolist(), nd["gap_size"].tolist(), nd["raw_gap_size"].tolist())]
        at = res["node_first"].tolist()
        return [rows[lo:hi] for lo, hi in zip(at, at[1:])]

    def scaffold(self, lengths=None, keep=False, quiet=False, synteny=None, assess=None, identity=None, lift=None):
        """main_scaffolder (:751-786) behind load_minimizers_scaffold in one handle: make_minimizer_graph -> find_paths ->
        format_paths -> adjust_paths -> trim_overlaps (when args.overlap) -> print_scaffolds.  Read from args, with ntJoin's
        defaults where one is missing: n, g, G, m, mkt, no_cut, overlap, overlap_k, overlap_w, overlap_gap, agp, gz, fai, report,
        report_min_gap, report_min_len, synteny, synteny_max_gap, synteny_min_anchors, synteny_min_span, assess, assess_merge_gap,
        assess_max_indel, assess_join_indel.  Returns what print_scaffolds returns (the written files by kind).  With args.fai the inputs read from FASTA get their <fasta>.fai first
        (write_input_indexes); with args.report <prefix>.report.tsv is written ("report": write_report); with args.synteny
        <prefix>.synteny.paf ("synteny": write_synteny; synteny=False leaves it out whatever args says: an earlier round of
        ntjoin_amd/rounds.py); with args.assess <prefix>.assess.tsv and <prefix>.breakpoints.bed ("assess", "breakpoints":
        write_assess, with the blocks parameters of --synteny_*; assess=False leaves them out likewise); with args.identity
        <prefix>.identity.tsv ("identity": write_identity, args.identity_max_seg; identity=False leaves it out likewise).  keep / quiet:
        print_scaffolds' (a round of ntjoin_amd/rounds.py); a quiet round writes no .mx.dot, no index, no report, no PAF and no
        assessment either.  With args.lift (BED files over the target's records) every one of them is lifted onto the scaffolds
        ("lifted", "unlifted": lists of files, lift_outputs' names; args.lift_whole_only); lift=[...] names the files instead, and
        lift=[] lifts nothing whatever args says (ntjoin_amd/rounds.py lifts once, behind the last round)."""
        opt = lambda name, dflt: dflt if getattr(self.args, name, None) is None else getattr(self.args, name)  # noqa: E731
        if quiet:
            opt = lambda name, dflt, _opt=opt: False if name in ("fai", "report") else _opt(name, dflt)  # noqa: E731
        self._quiet = bool(quiet)
        if opt("fai", False):
            self.write_input_indexes()
        report = bool(opt("report", False))
        if report:
            self._engine.set_report_params(int(opt("report_min_gap", 10)), int(opt("report_min_len", 500)))
            report_rows = self.input_reports()
        self.make_minimizer_graph(materialize=False)
        self.find_paths()
        G = int(opt("G", 0))
        paths = self.format_paths(lengths, g=int(opt("g", 20)), G=G, m=opt("m", 90), mkt=bool(opt("mkt", False)))
        paths = self.adjust_paths(paths, no_cut=bool(opt("no_cut", False)), G=G)
        cuts = self.trim_overlaps(paths, opt("overlap_k", 15), opt("overlap_w", 10)) if opt("overlap", False) else None
        syn = asz = None
        blocks_kw = dict(max_gap=int(opt("synteny_max_gap", 100000)), min_anchors=int(opt("synteny_min_anchors", 3)),
                         min_span=int(opt("synteny_min_span", 0)))
        if (bool(opt("synteny", False)) if synteny is None else synteny) and not quiet:
            syn = blocks_kw
        if (bool(opt("assess", False)) if assess is None else assess) and not quiet:
            asz = dict(blocks_kw, merge_gap=int(opt("assess_merge_gap", 100000)), max_indel=int(opt("assess_max_indel", 1000)),
                       join_indel=int(opt("assess_join_indel", 100000)))
        idy = None
        if (bool(opt("identity", False)) if identity is None else identity) and not quiet:
            idy = dict(blocks_kw, max_seg=int(opt("identity_max_seg", 10000)))
        beds = list(opt("lift", None) or []) if lift is None else list(lift)
        files = self.print_scaffolds(paths, cuts, n=int(opt("n", 1)), agp=bool(opt("agp", False)), overlap_gap=int(opt("overlap_gap", 20)),
                                     gz=bool(opt("gz", False)), fai=bool(opt("fai", False)), report=report, keep=keep, quiet=quiet,
                                     **({"lift": beds, "lift_whole_only": bool(opt("lift_whole_only", False))} if beds and not quiet else {}),
                                     **({"synteny": syn} if syn else {}), **({"assess": asz} if asz else {}), **({"identity": idy} if idy else {}))
        if report:
            files["report"] = self.write_report(report_rows, files)
        return files

    def input_reports(self):
        """(fasta, report) of every loaded assembly that was read from FASTA, references in command-line order, then the target
        (MxEngine.assembly_report).  An assembly loaded from its TSV has no text in the handle: one line on stderr and no entry."""
        rows = []
        for a, assembly in enumerate(self._order):
            fasta = self._fasta.get(assembly)
            if fasta is None:
                print(f"ntjoin_amd: {assembly} was loaded from its TSV: the report has no row for it", file=sys.stderr)
                continue
            rows.append((fasta, self._engine.assembly_report(a)))
        return rows

    def write_report(self, input_rows, files):
        """<prefix>.report.tsv: a header line, then one line per file -- the inputs (input_reports), the assigned, the unassigned and
        the `all` scaffolds file (named as `ntJoin-mx scaffold` names it) of the last print_scaffolds(report=True).  Returns its name."""
        rows = list(input_rows)
        for which in ("assigned", "unassigned"):
            rows.append((files[which], self._engine.scaffold_report(which)))
        rows.append((files["assigned"].replace(".assigned.scaffolds.", ".all.scaffolds."), self._engine.scaffold_report("all")))
        out = self.args.p + ".report.tsv"
        with open(out, "w", encoding="utf-8") as fh:
            fh.write("\t".join(REPORT_COLUMNS) + "\n")
            for name, rep in rows:
                fh.write(report_row(name, rep) + "\n")
        return out

    def write_input_indexes(self):
        """<fasta>.fai of every loaded assembly that was read from FASTA (the reference's `%.fai: %` rule, ntJoin:152-153, 207-208:
        `$(target).fai` and one per reference) from the text the handle holds, and <fasta>.gzi of a BGZF input.  An assembly loaded
        from its TSV has no text in the handle: one line on stderr, and the run goes on.  Returns the files written."""
        written = []
        for a, assembly in enumerate(self._order):
            fasta = self._fasta.get(assembly)
            if fasta is None:
                print(f"ntjoin_amd: {assembly} was loaded from its TSV: no FASTA index is written for it", file=sys.stderr)
                continue
            gzip_magic = False   # (text that came from device memory never was compressed: ntjoin_amd/rounds.py)
            if assembly not in self._device_text:
                with open(fasta, "rb") as fh:
                    gzip_magic = fh.read(2) == b"\x1f\x8b"
            try:
                self._engine.write_fai(a, fasta + ".fai", gzi=fasta + ".gzi" if gzip_magic else None)
            except MxError as err:
                if err.code != capi.MXG_EINVAL or "does not hold the file's text" not in str(err) and "did not come from a BGZF" not in str(err):
                    raise
                # (plain gzip, or a file the device parser left to the host's: the text is not in HBM)
                print(f"ntjoin_amd: no FASTA index is written for {fasta}: {err}", file=sys.stderr)
                continue
            written += [fasta + ".fai"] + ([fasta + ".gzi"] if gzip_magic else [])
        return written

    def trim_overlaps(self, paths, overlap_k=None, overlap_w=None):
        """The cut points of the reference's overlap stage (adjust_for_trimming, bin/ntjoin_assemble.py:468-516, and
        merge_overlapping, bin/ntjoin_overlap.py:20-88) for paths as format_paths() returns them.  Nodes of orientation '?'
        and paths left with fewer than two nodes are dropped, as print_scaffolds does (:558-575); per input path the list of
        (start_adjust, end_adjust) of its kept nodes comes back ([] for a dropped path; 0 = no adjustment).  k and w
        default to args.overlap_k / args.overlap_w, then 15 / 10 (ntJoin:39)."""
        k = int(overlap_k if overlap_k is not None else getattr(self.args, "overlap_k", None) or 15)
        w = int(overlap_w if overlap_w is not None else getattr(self.args, "overlap_w", None) or 10)
        eng, tgt = self._engine, len(self._order) - 1
        if tgt < 0:
            raise ValueError("trim_overlaps: no target assembly has been loaded")
        if self._order[tgt] not in self._fasta:
            raise ValueError("trim_overlaps: the target was loaded from a minimizer TSV, which holds no bases; the overlap stage "
                             "sketches the segments' ends, so the target must come from FASTA (Ntjoin(fasta={target: path}))")
        index = {rid: r for r, rid in enumerate(eng.record_ids(tgt, eng.n_records(tgt)))}
        rows, first, kept = [], [0], []
        for path in paths:
            nodes = [nd for nd in path if nd[1] != "?"]
            if len(nodes) < 2:
                kept.append(0)
                continue
            for i, nd in enumerate(nodes):
                if nd[0] not in index:
                    raise ValueError(f"trim_overlaps: path {len(kept)} node {i}: the target holds no contig {nd[0]!r}")
                rows.append((index[nd[0]], nd[2], nd[3], nd[8], nd[1] == "-"))
            first.append(len(rows))
            kept.append(len(nodes))
        if not rows:
            return [[] for _ in paths]
        res = eng.overlap_cuts(tgt, rows, first, k=k, w=w)
        sa, ea = res["start_adjust"].tolist(), res["end_adjust"].tolist()
        out, at = [], 0
        for n in kept:
            out.append(list(zip(sa[at:at + n], ea[at:at + n])))
            at += n
        return out

    @staticmethod
    def _path_coords(ori, start, end, start_adjust, end_adjust):
        "get_adjusted_start / get_adjusted_end of the reference's PathNode (bin/path_node.py:41-61)"
        length = end - start
        end_adj = length if end_adjust == 0 else end_adjust
        if ori == "+":
            return start + start_adjust, end - (length - end_adj)
        return start + (length - end_adj), end - start_adjust

    @staticmethod
    def _write_agp(fh, scaffold_id, path_str):
        "write_agp (:346-376): one W line per contig component and one N line per gap of the path string"
        at, part = 1, 1
        for comp in path_str.split():
            ctg = re.search(r"(\S+)([\+\-])\:(\d+)-(\d+)", comp)
            gap = re.search(r"(\d+)N", comp)
            if ctg:
                c_start, c_end = int(ctg.group(3)) + 1, int(ctg.group(4))
                n = c_end - c_start + 1
                cols = (scaffold_id, at, at + n - 1, part, "W", ctg.group(1), c_start, c_end, ctg.group(2))
            elif gap:
                n = int(gap.group(1))
                cols = (scaffold_id, at, at + n - 1, part, "N", n, "scaffold", "yes", "align_genus")
            else:
                raise ValueError("Path string is not formatted correctly: " + path_str)
            fh.write("\t".join(str(c) for c in cols) + "\n")
            at += n
            part += 1

    def _write_agp_unassigned(self, agp_fh, bed):
        """write_agp_unassigned (:379-404) for every unassigned interval that is not N throughout (= every record of the unassigned
        FASTA): `id:start-end  1  len  1  W  id  start  end  +`, the coordinates moved by the N/n stripped from either end.  The
        intervals are the BED's lines; the strip counts are the library's, kept from the call that wrote the files."""
        leads, tails = (x.tolist() for x in self._engine.scaffold_strips())
        with open(bed, encoding="utf-8") as fh:
            for line, lead, tail in zip(fh, leads, tails):
                ctg, lo, hi = line.rstrip("\n").split("\t")
                n = int(hi) - int(lo) - lead - tail
                if n <= 0:
                    continue
                start = int(lo) + 1 + lead
                agp_fh.write("\t".join(str(c) for c in (f"{ctg}:{lo}-{hi}", 1, n, 1, "W", ctg, start, start + n - 1, "+")) + "\n")

    def _write_path_host(self, files, assembly_fa, kept, leads, tails):
        """The .path file and, when files names one, the AGP as a per-node loop on the host (:605-610, write_agp, write_agp_unassigned):
        what print_scaffolds did before mxg_write_paths, kept for the inputs the library refuses.  kept = per written path its
        (nodes, cuts), leads / tails = the strips mxg_write_scaffolds returned."""
        agp_fh = None
        if "agp" in files:
            agp_fh = open(files["agp"], "w", encoding="utf-8")  # pylint: disable=consider-using-with
        try:
            with open(files["path"], "w", encoding="utf-8") as fh:
                fh.write(assembly_fa + "\n")
                for ct, ((nodes, cuts), lead, tail) in enumerate(zip(kept, leads, tails)):
                    coords = [[nd[1], nd[2], nd[3]] for nd in nodes]
                    for c, strip, left in ((coords[0], lead, True), (coords[-1], tail, False)):  # join_sequences :413-436
                        if strip:
                            if (c[0] == "+") == left:
                                c[1] += strip
                            else:
                                c[2] -= strip
                    parts = []
                    for nd, (ori, start, end), (sa, ea) in zip(nodes, coords, cuts):
                        a_start, a_end = self._path_coords(ori, start, end, sa, ea)
                        parts.append(f"{nd[0]}{ori}:{a_start}-{a_end} {nd[7]}N")
                    path_str = re.sub(r"\s+\d+N$", "", " ".join(parts))
                    fh.write(f"ntJoin{ct}\t{path_str}\n")
                    if agp_fh:
                        self._write_agp(agp_fh, f"ntJoin{ct}", path_str)
            if agp_fh:
                self._write_agp_unassigned(agp_fh, files["bed"])
        finally:
            if agp_fh:
                agp_fh.close()

    def print_scaffolds(self, paths, adjust=None, n=1, agp=False, overlap_gap=20, gz=False, fai=False, report=False, keep=False, quiet=False,
                        synteny=None, assess=None, identity=None, lift=None, lift_whole_only=False):
        """print_scaffolds (:580-613) and print_unassigned (:628-658) for paths as format_paths() returns them; adjust = what
        trim_overlaps(paths) returns, or None when the overlap stage is off.  Nodes of orientation '?' and paths left with fewer
        than two nodes are dropped (:585-594), the last kept node's gap is zeroed (check_terminal_node_gap_zero :441-448), and the
        library cuts the sequences from the text it holds (mxg_write_scaffolds): the target FASTA is not read again and no
        bedtools runs.  Written: <fasta>.k<k>.w<w>.n<n>.assigned.scaffolds.fa, ...unassigned.scaffolds.fa,
        <p>.<target tsv>.unassigned.bed, <p>.path and, with agp=True, <p>.agp.  gz=True: the two FASTA files are BGZF files
        (`bgzip`'s format, deflated on the device) named ...scaffolds.fa.gz.  fai=True: beside either FASTA its .fai ("assigned_fai",
        "unassigned_fai") and, with gz, its .gzi ("assigned_gzi", "unassigned_gzi").  report=True: either FASTA goes through the report's
        passes on its way out (MxEngine.scaffold_report hands the reports out; no file more).  keep=True: the text of both FASTA files
        also stays in device memory (MXG_SCAF_KEEP: MxEngine.scaffold_text, scaffold_pieces).  quiet=True (with keep): only <p>.path
        and, with agp, <p>.agp are written -- an earlier round of ntjoin_amd/rounds.py.  synteny=dict(max_gap, min_anchors, min_span)
        (or True for the defaults): also <p>.synteny.paf ("synteny": write_synteny), which needs the scaffolds' piece table and so
        turns keep on.  assess=dict(merge_gap, max_indel, join_indel, max_gap, min_anchors, min_span) (or True for the defaults): also
        <p>.assess.tsv and <p>.breakpoints.bed ("assess", "breakpoints": write_assess); it turns keep on as well, and with synteny the
        scaffolds' blocks are computed once for both, so the two must then name the same max_gap, min_anchors and min_span (ValueError
        otherwise, before anything is written).  lift=[BED files over the target's records]: every one of them is lifted onto the
        scaffolds ("lifted", "unlifted": lists of files, lift_outputs' names; lift_bed); it turns keep on as synteny= does.  Returns
        the file names by kind."""
        if synteny and assess:
            given = [{key: (arg if isinstance(arg, dict) else {}).get(key, default) for key, default in SYNTENY_DEFAULTS.items()}
                     for arg in (synteny, assess)]
            if given[0] != given[1]:
                raise ValueError(f"print_scaffolds: synteny= and assess= share one blocks call and must agree on its parameters: {given[0]} "
                                 f"against {given[1]}")
        if identity and (synteny or assess):
            given = [{key: (arg if isinstance(arg, dict) else {}).get(key, default) for key, default in SYNTENY_DEFAULTS.items()}
                     for arg in (identity, synteny or assess)]
            if given[0] != given[1]:
                raise ValueError(f"print_scaffolds: identity= shares one blocks call with synteny= and assess= and must agree on its parameters: "
                                 f"{given[0]} against {given[1]}")
        self._last_print = dict(paths=paths, adjust=adjust, n=n, agp=agp, overlap_gap=overlap_gap, gz=gz, fai=fai, report=report)
        if (synteny or assess or identity or lift) and not quiet:
            keep = True
        eng, tgt = self._engine, len(self._order) - 1
        if tgt < 0:
            raise ValueError("print_scaffolds: no target assembly has been loaded")
        target = self._order[tgt]
        if target not in self._fasta:
            raise ValueError("print_scaffolds: the target was loaded from a minimizer TSV, which holds no sequence; the scaffolds are "
                             "cut from the FASTA's text, so the target must come from FASTA (Ntjoin(fasta={target: path}))")
        match = re.search(r"^(\S+)(.k\d+.w\d+)\.tsv", target)
        if not match:
            raise ValueError(f"print_scaffolds: the target {target!r} is not named <fasta>.k<k>.w<w>.tsv")
        assembly_fa, params = match.group(1), match.group(2)
        if adjust is not None and len(adjust) != len(paths):
            raise ValueError("print_scaffolds: adjust needs one list per path, as trim_overlaps(paths) returns")
        index = {rid: r for r, rid in enumerate(eng.record_ids(tgt, eng.n_records(tgt)))}
        rows, first, kept = [], [0], []
        for p, path in enumerate(paths):
            nodes = [list(nd) for nd in path if nd[1] != "?"]
            if len(nodes) < 2:
                continue
            cuts = list(adjust[p]) if adjust is not None else [(0, 0)] * len(nodes)
            if len(cuts) != len(nodes):
                raise ValueError(f"print_scaffolds: path {p}: {len(cuts)} adjustments for {len(nodes)} oriented nodes")
            nodes[-1][7] = 0
            for i, (nd, (sa, ea)) in enumerate(zip(nodes, cuts)):
                if nd[0] not in index:
                    raise ValueError(f"print_scaffolds: path {p} node {i}: the target holds no contig {nd[0]!r}")
                rows.append((index[nd[0]], nd[2], nd[3], nd[7], sa, ea, nd[1] == "-"))
            first.append(len(rows))
            kept.append((nodes, cuts))
        prefix = assembly_fa + params + ".n" + str(n)
        ext = ".fa.gz" if gz else ".fa"
        files = {"assigned": prefix + ".assigned.scaffolds" + ext, "unassigned": prefix + ".unassigned.scaffolds" + ext,
                 "bed": self.args.p + "." + target + ".unassigned.bed", "path": self.args.p + ".path"}
        print(datetime.datetime.today(), ": Printing output scaffolds", file=sys.stdout)
        if quiet:
            # (the BED is what the host loop below reads the AGP's unassigned lines from, should the library refuse the paths: kept
            # under a name of its own until the .path is written)
            bed_tmp = files["bed"] + ".tmp"
            res = eng.write_scaffolds(tgt, rows, first, overlap_gap=overlap_gap if adjust is not None else None, bed=bed_tmp, keep=True)
            files = {"path": files["path"], "bed": bed_tmp}
            fai = False
        else:
            res = eng.write_scaffolds(tgt, rows, first, overlap_gap=overlap_gap if adjust is not None else None,
                                      assigned=files["assigned"], unassigned=files["unassigned"], bed=files["bed"], bgzf=bool(gz),
                                      **({"fai": True} if fai else {}), **({"report": True} if report else {}), **({"keep": True} if keep else {}))
        self._lift_prepared = False
        if lift and not quiet:
            files.update(self.lift_beds(lift, whole_only=lift_whole_only))
        if identity and not quiet:   # (one pass over the references for the table, the PAF and the assessment)
            idy = identity if isinstance(identity, dict) else {}
            files.update(self._synteny_files({key: idy.get(key, default) for key, default in SYNTENY_DEFAULTS.items()}, paf=bool(synteny),
                                             assess=None if not assess else {key: (assess if isinstance(assess, dict) else {}).get(key, default)
                                                                              for key, default in (("merge_gap", 100000), ("max_indel", 1000),
                                                                                                   ("join_indel", 100000))},
                                             scaffolds_name=files["assigned"].replace(".assigned.scaffolds.", ".all.scaffolds."),
                                             identity=dict(max_seg=idy.get("max_seg", 10000))))
        elif assess and not quiet:
            files.update(self.write_assess(**(assess if isinstance(assess, dict) else {}), paf=bool(synteny),
                                           scaffolds_name=files["assigned"].replace(".assigned.scaffolds.", ".all.scaffolds.")))
        elif synteny and not quiet:
            files["synteny"] = self.write_synteny(**(synteny if isinstance(synteny, dict) else {}))
        if fai:
            for kind in ("assigned", "unassigned"):
                files[kind + "_fai"] = files[kind] + ".fai"
                if gz:
                    files[kind + "_gzi"] = files[kind] + ".gzi"
        if agp:
            files["agp"] = self.args.p + ".agp"
        lead, tail = res["lead_strip"], res["tail_strip"]
        if hasattr(eng, "write_paths"):
            try:
                eng.write_paths(tgt, rows, first, lead_strip=lead, tail_strip=tail, first_line=assembly_fa, path=files["path"],
                                agp=files.get("agp"), agp_unassigned=agp)
                return self._quiet_files(files) if quiet else files
            except MxError as err:
                # a cut that leaves a node's interval empty or inverted: the library refuses it and has written nothing; such paths
                # keep the text the host loop gives them
                if err.code != capi.MXG_EINVAL or "empty or inverted" not in str(err):
                    raise
        self._write_path_host(files, assembly_fa, kept, lead.tolist(), tail.tolist())
        return self._quiet_files(files) if quiet else files

    def lift_prepare(self, table=None):
        """The index the lifts below go through (MxEngine.lift_prepare), kept until the next print_scaffolds: of the table and ids of
        scaffold_pieces() over the target's record ids and lengths, or of table=(pieces, first, ids, source_ids, source_length) --
        the rounds' composed one (ntjoin_amd/rounds.py)."""
        eng, tgt = self._engine, len(self._order) - 1
        if table is None:
            pieces, first, ids = eng.scaffold_pieces()
            table = (pieces, first, ids, eng.record_ids(tgt, eng.n_records(tgt)), eng.record_lengths(tgt))
        pieces, first, ids, source_ids, source_length = table
        self._lift_prepared = False
        eng.lift_prepare(pieces, first, source_length)
        self._lift_names = (list(source_ids), list(ids))
        self._lift_prepared = True

    def lift_bed(self, bed, lifted, unlifted=None, whole_only=False):
        """The features of the BED file `bed`, which lie on the target's records, lifted onto the scaffolds the last
        print_scaffolds(keep=True) left: `lifted` gets one line per part, `unlifted` what was not lifted whole, with the reason
        (lift_prepare, once per print_scaffolds; MxEngine.lift_bed).  Returns MxEngine.lift_bed's counts."""
        if not getattr(self, "_lift_prepared", False):
            self.lift_prepare()
        source_ids, ids = self._lift_names
        return self._engine.lift_bed(bed, source_ids, ids, lifted, unlifted, whole_only=whole_only)

    def lift_beds(self, beds, whole_only=False, table=None):
        "lift_bed for every file of `beds`, under lift_outputs' names (table: lift_prepare's) -> {'lifted': [files], 'unlifted': [files]}"
        if table is not None:
            self.lift_prepare(table)
        files = {"lifted": [], "unlifted": []}
        for bed in beds:
            lifted, unlifted = lift_outputs(self.args.p, bed)
            st = self.lift_bed(bed, lifted, unlifted, whole_only=whole_only)
            print(f"ntjoin_amd: {bed}: {st['features']} features, {st['whole']} lifted whole, {st['split']} split, {st['partial']} partially "
                  f"deleted, {st['lost']} deleted, {st['invalid']} invalid, {st['unknown']} on unknown records", file=sys.stderr)
            files["lifted"].append(lifted)
            files["unlifted"].append(unlifted)
        return files

    def write_synteny(self, max_gap=100000, min_anchors=3, min_span=0):
        """<prefix>.synteny.paf: the synteny blocks (MxEngine.synteny_blocks) of the scaffolds the last print_scaffolds(keep=True) left
        -- the records of the assigned file, then those of the unassigned file, under their names there -- against every reference,
        in command-line order, one PAF line per block (MxEngine.write_synteny_paf).  A reference loaded from its TSV has no record
        lengths in the handle: they are read from <fasta>.fai when that file exists, else the reference is left out with one line on
        stderr.  Returns the file's name."""
        return self._synteny_files(dict(max_gap=max_gap, min_anchors=min_anchors, min_span=min_span), paf=True)["synteny"]

    def write_assess(self, merge_gap=100000, max_indel=1000, join_indel=100000, max_gap=100000, min_anchors=3, min_span=0, paf=False,
                     scaffolds_name="scaffolds"):
        """<prefix>.assess.tsv and <prefix>.breakpoints.bed: for every reference, in command-line order, the target as loaded and then
        the scaffolds the last print_scaffolds(keep=True) left (write_synteny's records) are assessed against it -- one
        MxEngine.synteny_blocks (max_gap, min_anchors, min_span) and one MxEngine.synteny_assess (merge_gap, max_indel, join_indel)
        each.  The TSV has a header line and one row per (query, reference) (ntjoin_amd/report.py: assess_row); the BED holds the
        scaffolds' breakpoints (breakpoint_lines).  paf=True: the scaffolds' blocks are also written to <prefix>.synteny.paf, as
        write_synteny does.  A reference loaded from its TSV is treated as write_synteny treats it.  Returns the files by kind."""
        return self._synteny_files(dict(max_gap=max_gap, min_anchors=min_anchors, min_span=min_span), paf=paf,
                                   assess=dict(merge_gap=merge_gap, max_indel=max_indel, join_indel=join_indel), scaffolds_name=scaffolds_name)

    def write_identity(self, max_seg=10000, max_gap=100000, min_anchors=3, min_span=0, paf=False, scaffolds_name="scaffolds"):
        """<prefix>.identity.tsv: for every reference, in command-line order, the target as loaded and then the scaffolds the last
        print_scaffolds(keep=True) left get one row each: one MxEngine.synteny_blocks (max_gap, min_anchors, min_span) and one
        MxEngine.synteny_identity (max_seg), a header line first (ntjoin_amd/report.py: identity_row).  paf=True: the scaffolds' blocks
        are also written to <prefix>.synteny.paf with the identity tags.  A reference loaded from its TSV has no text in the handle:
        one line on stderr and no rows.  Returns the files by kind."""
        return self._synteny_files(dict(max_gap=max_gap, min_anchors=min_anchors, min_span=min_span), paf=paf, scaffolds_name=scaffolds_name,
                                   identity=dict(max_seg=max_seg))

    def _synteny_files(self, blocks_kw, paf, assess=None, scaffolds_name="scaffolds", identity=None):
        """write_synteny, write_assess and write_identity: one pass over the references, the scaffolds' blocks computed once for the PAF,
        the assessment and the identity table"""
        eng, tgt = self._engine, len(self._order) - 1
        pieces, first, ids = eng.scaffold_pieces()
        files = {}
        if paf:
            files["synteny"] = self.args.p + ".synteny.paf"
            with open(files["synteny"], "wb"):
                pass   # (every reference's lines are appended)
        rows, bed, idy_rows = [], [], []
        if assess is not None or identity is not None:
            target_ids = eng.record_ids(tgt, eng.n_records(tgt))
            target_name = self._fasta.get(self._order[tgt], self._order[tgt])
        for a, assembly in enumerate(self._order[:tgt]):
            lengths = None
            idy = identity if assembly in self._fasta else None   # (the reference's text is what its bases are read from)
            if identity is not None and idy is None:
                print(f"ntjoin_amd: {assembly} was loaded from its TSV and the handle holds no text of it: the identity table has no rows for it",
                      file=sys.stderr)
                if not paf and assess is None:
                    continue
            if assembly not in self._fasta:
                lengths = self._fai_lengths(a, assembly)
                if lengths is None:
                    what = ("the synteny PAF has no lines" if paf else "") + (" and " if paf and assess is not None else "") + \
                        ("the assessment has no rows" if assess is not None else "")
                    print(f"ntjoin_amd: {assembly} was loaded from its TSV and its FASTA has no .fai: {what} for it", file=sys.stderr)
                    continue
            if assess is not None or idy is not None:
                match = re.search(r"^(.+)\.k\d+\.w\d+\.tsv$", assembly)
                ref_name = self._fasta.get(assembly) or (match.group(1) if match else assembly)
                blk = eng.synteny_blocks(tgt, a, subject_length=lengths, **blocks_kw)
                if assess is not None:
                    rows.append(assess_row(target_name, ref_name, len(target_ids), blk["n_anchors_total"], eng.synteny_assess(**assess)))
                if idy is not None:
                    idy_rows.append(identity_row(target_name, ref_name, eng.synteny_identity(**idy)))
            blk = eng.synteny_blocks(tgt, a, pieces=pieces, first=first, subject_length=lengths, **blocks_kw)
            if idy is not None:
                idy_rows.append(identity_row(scaffolds_name, ref_name, eng.synteny_identity(**idy)))
            if paf:
                eng.write_synteny_paf(files["synteny"], query_names=ids, append=True, identity=idy is not None)
            if assess is not None:
                res = eng.synteny_assess(**assess)
                rows.append(assess_row(scaffolds_name, ref_name, len(ids), blk["n_anchors_total"], res))
                bed += breakpoint_lines(res, ids, ref_name, eng.record_ids(a, eng.n_records(a)))
        if assess is not None:
            files["assess"], files["breakpoints"] = self.args.p + ".assess.tsv", self.args.p + ".breakpoints.bed"
            with open(files["assess"], "w", encoding="utf-8") as fh:
                fh.write("\t".join(ASSESS_COLUMNS) + "\n")
                for row in rows:
                    fh.write(row + "\n")
            with open(files["breakpoints"], "w", encoding="utf-8") as fh:
                fh.writelines(bed)
        if identity is not None:
            files["identity"] = self.args.p + ".identity.tsv"
            with open(files["identity"], "w", encoding="utf-8") as fh:
                fh.write("\t".join(IDENTITY_COLUMNS) + "\n")
                for row in idy_rows:
                    fh.write(row + "\n")
        return files

    def _fai_lengths(self, a, assembly):
        "the lengths of assembly a's records from <fasta>.fai (the TSV being named <fasta>.k<k>.w<w>.tsv), or None"
        match = re.search(r"^(.+)\.k\d+\.w\d+\.tsv$", assembly)
        if not match or not os.path.exists(match.group(1) + ".fai"):
            return None
        known = {}
        with open(match.group(1) + ".fai", encoding="utf-8") as fh:
            for line in fh:
                cols = line.rstrip("\n").split("\t")
                if len(cols) >= 2 and cols[1].isdigit():
                    known.setdefault(cols[0], int(cols[1]))
        ids = self._engine.record_ids(a, self._engine.n_records(a))
        return [known[rid] for rid in ids] if all(rid in known for rid in ids) else None

    @staticmethod
    def _quiet_files(files):
        os.remove(files.pop("bed"))
        return files

    def print_graph(self, graph, out_prefix=None):
        "Prints the minimizer graph in dot format"
        out_graph = (self.args.p + ".mx.dot") if out_prefix is None else (out_prefix + "mx.dot")
        if getattr(self, "_quiet", False):
            return
        print(datetime.datetime.today(), ": Printing graph", out_graph, sep=" ", file=sys.stdout)
        self._engine.write_dot(out_graph)
        list_files = list(self._order)
        colours = COLOURS if len(list_files) <= len(COLOURS) else ["red"] * len(list_files)
        print("\nfile_name\tnumber\tcolour")
        for i, filename in enumerate(list_files):
            print(filename, i, colours[i], sep="\t")
        print("", flush=True)
