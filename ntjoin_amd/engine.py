"""
MxEngine -- Python face of one libntjoin_mx handle (one k, w, hash variant, one GPU).

Order of use mirrors the reference pipeline:
    eng = MxEngine(k=32, w=1000)
    eng.add_fasta("ref.fa.k32.w1000.tsv", 2.0, "ref.fa")        # references first, CLI order
    eng.add_fasta("scaf.fa.k32.w1000.tsv", 1.0, "scaf.fa")      # target last
    eng.sketch()                                                # = indexlr              ntJoin:204-205
    eng.write_tsv(0, "ref.fa.k32.w1000.tsv")
    eng.build_graph()                                           # = read_minimizers' uniqueness + filter_minimizers + build_graph
    eng.write_dot("prefix.mx.dot")                              # = Ntjoin.print_graph   bin/ntjoin.py:25-62
All arrays returned are numpy COPIES (the library owns its buffers), hence picklable.
"""
import ctypes as C
import os

import numpy as np

from . import capi


class MxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libntjoin_mx error {code}: {msg}")
        self.code = code


def _np(ptr, n, dtype):
    if n == 0:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(ptr, shape=(int(n),)).astype(dtype, copy=True)


class MxEngine:
    def __init__(self, k=32, w=1000, variant="v2", device=-1, stream=None, dense_only=False, drop_seq=False,
                 timing=False, cand_per_window=0, timing_fine=False, threads=0, one_shot=False):
        self._lib = capi.load()
        self._h = C.c_void_p()
        cfg = capi.Config()
        cfg.struct_size = C.sizeof(capi.Config)
        cfg.k, cfg.w = int(k), int(w)
        cfg.variant = capi.VARIANT_V1_MIN if str(variant).lower() in ("v1", "min", "1") else capi.VARIANT_V2_SUM
        cfg.device = int(device)
        cfg.flags = ((capi.FLAG_DENSE_ONLY if dense_only else 0) | (capi.FLAG_DROP_SEQ if drop_seq else 0) |
                     (capi.FLAG_TIMING if timing else 0) | (capi.FLAG_TIMING_FINE if timing_fine else 0) |
                     (capi.FLAG_ONE_SHOT if one_shot else 0))
        cfg.stream = C.c_void_p(stream) if stream else None
        cfg.cand_per_window = int(cand_per_window)
        cfg.host_threads = int(threads)
        rc = self._lib.mxg_create(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            raise MxError(rc, (self._lib.mxg_last_error(None) or b"").decode())
        self.k, self.w = int(k), int(w)
        self._keep = []  # objects that must outlive the handle (borrowed device buffers)

    # -- plumbing -------------------------------------------------------------------------------------
    def _check(self, rc):
        if rc < 0:
            raise MxError(rc, (self._lib.mxg_last_error(self._h) or b"").decode())
        return rc

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.mxg_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- assemblies -------------------------------------------------------------------------------------
    def add_fasta(self, name, weight, fasta_path):
        return self._check(self._lib.mxg_add_assembly_fasta(self._h, str(name).encode(), float(weight),
                                                            str(fasta_path).encode()))

    def add_text_device(self, name, weight, d_text, n_bytes):
        """mxg_add_assembly_text_device: FASTA text that lies in device memory already (d_text: an address, e.g. assembly_text()'s
        or a torch tensor's data_ptr()) is copied device to device and loaded as add_fasta loads a file with those bytes; the
        source may go as soon as the call returns"""
        return self._check(self._lib.mxg_add_assembly_text_device(self._h, str(name).encode(), float(weight), C.c_void_p(int(d_text) or None),
                                                                  int(n_bytes)))

    def assembly_text(self, a):
        """mxg_assembly_text: (device address, bytes) of the FASTA text of an assembly that the device ingest route loaded; the
        memory is the handle's"""
        p, n = C.c_void_p(), C.c_uint64()
        self._check(self._lib.mxg_assembly_text(self._h, int(a), C.byref(p), C.byref(n)))
        return int(p.value or 0), int(n.value)

    def add_fasta_shard(self, name, weight, fasta_path, shard, n_shards):
        """every record is registered (global indices) but only shard `shard` of `n_shards` is packed and sketched"""
        return self._check(self._lib.mxg_add_assembly_fasta_shard(self._h, str(name).encode(), float(weight),
                                                                  str(fasta_path).encode(), int(shard), int(n_shards)))

    def add_fasta_split(self, name, weight, fasta_path, shard, n_shards):
        """as add_fasta_shard, but the shards are equal BASE ranges: long records are sketched in pieces (with a halo) and the
        rank-ordered concatenation of the shards' sketches is the sketch of the whole file"""
        return self._check(self._lib.mxg_add_assembly_fasta_split(self._h, str(name).encode(), float(weight),
                                                                  str(fasta_path).encode(), int(shard), int(n_shards)))

    def assembly_continues(self, a):
        """split load: does this handle's first record continue a record begun on the shard before?"""
        rc = self._lib.mxg_assembly_continues(self._h, int(a))
        if rc < 0:
            raise ValueError("mxg_assembly_continues: bad arguments")
        return bool(rc)

    def xchg_pack(self, d_slot, head_bytes, caps):
        cc = np.ascontiguousarray(caps, dtype=np.uint64)
        return self._check(self._lib.mxg_xchg_pack(self._h, C.c_void_p(int(d_slot)), int(head_bytes),
                                                   cc.ctypes.data_as(C.POINTER(C.c_uint64))))

    def sketch_pack(self, d_slot, head_bytes, caps):
        """sketch every assembly and pack the sketches into the exchange slot without a host sync (finish with sketch_finish)"""
        cc = np.ascontiguousarray(caps, dtype=np.uint64)
        return self._check(self._lib.mxg_sketch_pack(self._h, C.c_void_p(int(d_slot)), int(head_bytes),
                                                     cc.ctypes.data_as(C.POINTER(C.c_uint64))))

    def sketch_pack_parts(self, d_parts, caps, rcaps):
        """sketch every assembly; each one's sketch is packed into its own buffer (d_parts[a]: 64-byte header + 12 * caps[a] bytes of
        hashes and positions + 4 * rcaps[a] bytes: the records' first entries) right behind its last kernel --
        part_packed_wait(a, stream) then lets a communication stream send it while the next assembly is sketched (finish with
        sketch_finish)"""
        cc = np.ascontiguousarray(caps, dtype=np.uint64)
        rc_ = np.ascontiguousarray(rcaps, dtype=np.uint64)
        pp = (C.c_void_p * len(d_parts))(*[int(x) for x in d_parts])
        return self._check(self._lib.mxg_sketch_pack_parts(self._h, pp, cc.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                           rc_.ctypes.data_as(C.POINTER(C.c_uint64))))

    def part_packed_wait(self, a, stream):
        """make `stream` (a raw hipStream_t) wait until assembly a's part is packed"""
        return self._check(self._lib.mxg_part_packed_wait(self._h, int(a), C.c_void_p(int(stream))))

    def xchg_unpack_graph_parts(self, d_all_parts, world, caps, rcaps, rec_offsets):
        """-> False when some rank's sketch did not fit its part (nothing usable), True: sketches unpacked + graph built"""
        cc = np.ascontiguousarray(caps, dtype=np.uint64)
        rc_ = np.ascontiguousarray(rcaps, dtype=np.uint64)
        ro = np.ascontiguousarray(rec_offsets, dtype=np.uint64)
        pp = (C.c_void_p * len(d_all_parts))(*[int(x) for x in d_all_parts])
        rc = self._lib.mxg_xchg_unpack_graph_parts(self._h, pp, int(world), cc.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                   rc_.ctypes.data_as(C.POINTER(C.c_uint64)), ro.ctypes.data_as(C.POINTER(C.c_uint64)))
        if rc == 1:
            return False
        self._check(rc)
        return True

    def sketch_finish(self):
        return self._check(self._lib.mxg_sketch_finish(self._h))

    def xchg_unpack_graph(self, d_all, world, slot_bytes, head_bytes, caps, rec_offsets):
        """-> False when some rank's sketch did not fit its slot (nothing usable), True: sketches unpacked + graph built"""
        cc = np.ascontiguousarray(caps, dtype=np.uint64)
        ro = np.ascontiguousarray(rec_offsets, dtype=np.uint64)
        rc = self._lib.mxg_xchg_unpack_graph(self._h, C.c_void_p(int(d_all)), int(world), int(slot_bytes), int(head_bytes),
                                             cc.ctypes.data_as(C.POINTER(C.c_uint64)), ro.ctypes.data_as(C.POINTER(C.c_uint64)))
        if rc == 1:
            return False
        self._check(rc)
        return True

    def assembly_shard(self, a):
        lo, hi = C.c_uint64(), C.c_uint64()
        self._check(self._lib.mxg_assembly_shard(self._h, int(a), C.byref(lo), C.byref(hi)))
        return int(lo.value), int(hi.value)

    def add_records(self, name, weight, records):
        """records: iterable of (id, sequence str/bytes)."""
        ids, seqs = [], []
        for rid, s in records:
            ids.append(str(rid).encode())
            seqs.append(s.encode("ascii") if isinstance(s, str) else bytes(s))
        blob = b"".join(seqs)
        offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
        if seqs:
            offs[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
        arr_ids = (C.c_char_p * max(len(ids), 1))(*ids)
        buf = C.create_string_buffer(blob, len(blob) + 1)
        return self._check(self._lib.mxg_add_assembly_buffers(
            self._h, str(name).encode(), float(weight), C.cast(buf, C.c_void_p),
            offs.ctypes.data_as(C.POINTER(C.c_uint64)), arr_ids, len(seqs)))

    def add_packed_device(self, name, weight, d_ptr, rec_start, rec_len, ids=None, keepalive=None):
        """2-bit packed bases already in HBM (see include/ntjoin_mx.h); d_ptr is borrowed."""
        rs = np.ascontiguousarray(rec_start, dtype=np.uint64)
        rl = np.ascontiguousarray(rec_len, dtype=np.uint64)
        arr_ids = None
        if ids is not None:
            arr_ids = (C.c_char_p * len(ids))(*[str(i).encode() for i in ids])
        if keepalive is not None:
            self._keep.append(keepalive)
        return self._check(self._lib.mxg_add_assembly_packed_device(
            self._h, str(name).encode(), float(weight), C.c_void_p(int(d_ptr)),
            rs.ctypes.data_as(C.POINTER(C.c_uint64)), rl.ctypes.data_as(C.POINTER(C.c_uint64)), arr_ids, len(rs)))

    def plan_split(self, lengths, shard, n_shards):
        """pieces of shard `shard` of `n_shards` for N-free records of the given lengths -> (lo, hi, drop) arrays"""
        ln = np.ascontiguousarray(lengths, dtype=np.uint64)
        lo, hi = np.zeros(len(ln), dtype=np.uint64), np.zeros(len(ln), dtype=np.uint64)
        drop = np.zeros(len(ln), dtype=np.uint8)
        rc = self._lib.mxg_plan_split(ln.ctypes.data, len(ln), int(shard), int(n_shards), self.k, self.w, lo.ctypes.data, hi.ctypes.data,
                                      drop.ctypes.data)
        if rc != 0:
            raise ValueError("mxg_plan_split: bad arguments")
        return lo, hi, drop

    def add_packed_device_pieces(self, name, weight, d_ptr, rec_start, rec_len, lo, hi, drop, ids=None, keepalive=None):
        """sub-record shard of 2-bit packed bases in HBM (see include/ntjoin_mx.h); d_ptr is borrowed"""
        arrs = [np.ascontiguousarray(x, dtype=np.uint64) for x in (rec_start, rec_len, lo, hi)]
        dr = np.ascontiguousarray(drop, dtype=np.uint8)
        arr_ids = None
        if ids is not None:
            arr_ids = (C.c_char_p * len(ids))(*[str(i).encode() for i in ids])
        if keepalive is not None:
            self._keep.append(keepalive)
        return self._check(self._lib.mxg_add_assembly_packed_device_pieces(
            self._h, str(name).encode(), float(weight), C.c_void_p(int(d_ptr)), arrs[0].ctypes.data, arrs[1].ctypes.data,
            arrs[2].ctypes.data, arrs[3].ctypes.data, dr.ctypes.data, arr_ids, len(arrs[0])))

    def add_tsv(self, name, weight, tsv_path):
        return self._check(self._lib.mxg_add_assembly_tsv(self._h, str(name).encode(), float(weight),
                                                          str(tsv_path).encode()))

    def add_bin(self, name, weight, bin_path):
        """a sketch from the binary side-car written by write_sketch_bin (no text parsing)"""
        rc = self._lib.mxg_add_assembly_bin(self._h, str(name).encode(), float(weight), str(bin_path).encode())
        if rc < 0:
            msg = (self._lib.mxg_last_error(self._h) or b"").decode()
            if "cannot open" in msg:
                raise FileNotFoundError(msg)
            raise MxError(rc, msg)
        return rc

    def write_sketch_bin(self, a, path):
        self._check(self._lib.mxg_write_sketch_bin(self._h, int(a), str(path).encode()))

    def add_minimizers(self, name, weight, out_hash, pos, record, record_ids):
        hh = np.ascontiguousarray(out_hash, dtype=np.uint64)
        pp = np.ascontiguousarray(pos, dtype=np.uint32)
        rr = np.ascontiguousarray(record, dtype=np.uint32)
        ids = (C.c_char_p * max(len(record_ids), 1))(*[str(i).encode() for i in record_ids])
        return self._check(self._lib.mxg_add_assembly_minimizers(
            self._h, str(name).encode(), float(weight), hh.ctypes.data, pp.ctypes.data, rr.ctypes.data,
            len(hh), ids, len(record_ids)))

    @property
    def n_assemblies(self):
        return self._lib.mxg_num_assemblies(self._h)

    def assembly_name(self, a):
        return self._lib.mxg_assembly_name(self._h, a).decode()

    def n_records(self, a):
        return int(self._lib.mxg_num_records(self._h, int(a)))

    def assembly_weight(self, a):
        return float(self._lib.mxg_assembly_weight(self._h, int(a)))

    def record_ids(self, a, n_records):
        return [self._lib.mxg_record_id(self._h, a, r).decode() for r in range(int(n_records))]

    def record_lengths(self, a):
        return [int(self._lib.mxg_record_length(self._h, int(a), r)) for r in range(self.n_records(a))]

    # -- sketch stage -------------------------------------------------------------------------------------
    def sketch(self, assembly=-1):
        self._check(self._lib.mxg_sketch(self._h, int(assembly)))

    def sketch_graph(self):
        """sketch every assembly and build the graph in one call (one host sync in the common case)"""
        self._check(self._lib.mxg_sketch_graph(self._h))

    def get_sketch(self, a):
        v = capi.SketchView()
        self._check(self._lib.mxg_get_sketch(self._h, int(a), C.byref(v)))
        return {"out_hash": _np(v.out_hash, v.n, np.uint64), "pos": _np(v.pos, v.n, np.uint32),
                "record": _np(v.record, v.n, np.uint32), "forward": _np(v.forward, v.n, np.uint8),
                "record_first": _np(v.record_first, v.n_records + 1, np.uint64),
                "record_ids": self.record_ids(a, v.n_records)}

    def get_sketch_device(self, a):
        v = capi.SketchDView()
        self._check(self._lib.mxg_get_sketch_device(self._h, int(a), C.byref(v)))
        return {"n": int(v.n), "out_hash": v.out_hash or 0, "pos": v.pos or 0, "record": v.record or 0,
                "forward": v.forward or 0}

    def compute_strands(self, a):
        self._check(self._lib.mxg_compute_strands(self._h, int(a)))

    def sketch_size(self, a):
        v = capi.SketchDView()
        self._check(self._lib.mxg_get_sketch_device(self._h, int(a), C.byref(v)))
        return int(v.n)

    def pack_sketch_device(self, a, d_buf, nmax):
        self._check(self._lib.mxg_pack_sketch_device(self._h, int(a), C.c_void_p(int(d_buf)), int(nmax)))

    def set_sketch_gathered(self, a, d_allbuf, nmax, counts, rec_offsets):
        cc = np.ascontiguousarray(counts, dtype=np.uint64)
        ro = np.ascontiguousarray(rec_offsets, dtype=np.uint64)
        self._check(self._lib.mxg_set_sketch_gathered(self._h, int(a), C.c_void_p(int(d_allbuf)), len(cc), int(nmax),
                                                      cc.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                      ro.ctypes.data_as(C.POINTER(C.c_uint64))))

    def set_sketch_gathered_strided(self, a, d_allbuf, stride_bytes, nmax, counts, rec_offsets):
        """like set_sketch_gathered, rank r's packed buffer at d_allbuf + r * stride_bytes"""
        cc = np.ascontiguousarray(counts, dtype=np.uint64)
        ro = np.ascontiguousarray(rec_offsets, dtype=np.uint64)
        self._check(self._lib.mxg_set_sketch_gathered_strided(self._h, int(a), C.c_void_p(int(d_allbuf)), len(cc),
                                                              int(stride_bytes), int(nmax),
                                                              cc.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                              ro.ctypes.data_as(C.POINTER(C.c_uint64))))

    def set_sketch_device(self, a, d_hash, d_pos, d_record, d_forward, n):
        self._check(self._lib.mxg_set_sketch_device(self._h, int(a), C.c_void_p(int(d_hash)), C.c_void_p(int(d_pos)),
                                                    C.c_void_p(int(d_record)),
                                                    C.c_void_p(int(d_forward)) if d_forward else None, int(n)))

    def write_tsv(self, a, path, with_pos=True, with_strand=False, with_seq=True):
        self._check(self._lib.mxg_write_tsv(self._h, int(a), str(path).encode(), int(with_pos), int(with_strand),
                                            int(with_seq)))

    # -- graph stage ----------------------------------------------------------------------------------------
    def build_graph(self):
        self._check(self._lib.mxg_build_graph(self._h))

    def get_mx_flags(self, a):
        p = C.POINTER(C.c_uint8)()
        n = C.c_uint64()
        self._check(self._lib.mxg_get_mx_flags(self._h, int(a), C.byref(p), C.byref(n)))
        return _np(p, n.value, np.uint8)

    def get_graph(self):
        g = capi.GraphView()
        self._check(self._lib.mxg_get_graph(self._h, C.byref(g)))
        A, nv, ne = int(g.n_assemblies), int(g.n_vertices), int(g.n_edges)
        return {"n_assemblies": A,
                "vertex_hash": _np(g.vertex_hash, nv, np.uint64),
                "vertex_pos": _np(g.vertex_pos, A * nv, np.uint32).reshape(A, nv),
                "vertex_record": _np(g.vertex_record, A * nv, np.uint32).reshape(A, nv),
                "edge_u": _np(g.edge_u, ne, np.uint32), "edge_v": _np(g.edge_v, ne, np.uint32),
                "edge_support": _np(g.edge_support, ne, np.uint32),
                "edge_weight": _np(g.edge_weight, ne, np.float64)}

    def vertex_hashes(self, vertices):
        """mxg_vertex_hashes: the minimizer hashes (u64) of the given graph vertices, gathered on the device: the graph's host
        mirror (get_graph) is not made for them"""
        idx = np.ascontiguousarray(vertices, dtype=np.uint32)
        out = np.zeros(len(idx), dtype=np.uint64)
        self._check(self._lib.mxg_vertex_hashes(self._h, idx.ctypes.data, len(idx), out.ctypes.data))
        return out

    def find_paths(self, n=1):
        """linear paths through the graph (ntJoin's -n = minimum edge weight): list of (component id, [vertex indices])"""
        v = capi.PathsView()
        self._check(self._lib.mxg_find_paths(self._h, int(n), C.byref(v)))
        npaths = int(v.n_paths)
        first = _np(v.path_first, npaths + 1, np.uint64)
        verts = _np(v.path_vertex, int(first[-1]) if npaths else 0, np.uint32)
        comp = _np(v.path_component, npaths, np.uint32)
        self.n_components = int(v.n_components)
        return [(int(comp[i]), verts[int(first[i]):int(first[i + 1])].tolist()) for i in range(npaths)]

    def path_segments(self, a):
        """runs of consecutive path vertices on the same record of assembly a (after find_paths): dict of arrays
        path, record, first (offset into the concatenated paths), n, min_pos, max_pos, inc, dec"""
        v = capi.SegmentsView()
        self._check(self._lib.mxg_path_segments(self._h, int(a), C.byref(v)))
        n = int(v.n_segments)
        st = _np(v.seg_stat, 5 * n, np.uint32).reshape(n, 5)
        return {"path": _np(v.seg_path, n, np.uint32), "record": _np(v.seg_record, n, np.uint32),
                "first": _np(v.seg_first, n, np.uint32), "n": st[:, 0], "min_pos": st[:, 1], "max_pos": st[:, 2],
                "inc": st[:, 3], "dec": st[:, 4]}

    def path_segments_mk(self, a):
        """Mann-Kendall statistics of the runs of the last path_segments(a), aligned with them (--mkt): dict of arrays
        s (int64: sum over i < j of sign(x_j - x_i)) and tie_term (uint64: sum over groups of t equal positions of
        t(t-1)(2t+5))"""
        s, t, n = C.POINTER(C.c_int64)(), C.POINTER(C.c_uint64)(), C.c_uint64()
        self._check(self._lib.mxg_path_segments_mk(self._h, int(a), C.byref(s), C.byref(t), C.byref(n)))
        return {"s": _np(s, n.value, np.int64), "tie_term": _np(t, n.value, np.uint64)}

    def format_paths(self, a, g=20, G=0, m=90, mkt=False, lengths=None):
        """mxg_format_paths: nodes, orientations and gap sizes of all paths of the last find_paths for assembly a, as a dict of
        arrays: node_first u64[n_paths + 1], and per node record, start, end, contig_size, first_vertex, terminal_vertex,
        segment (u32), reverse (u8: 0 '+', 1 '-'), gap_size, raw_gap_size (i64, to the next node of the path).  lengths = one
        length per record of the assembly (None: those the handle holds).  A negative overhang ("Gap distance estimation less
        than 0") raises MxError with the arrays as its .nodes."""
        p = capi.FormatParams()
        p.struct_size, p.g, p.G, p.m, p.mkt = C.sizeof(capi.FormatParams), int(g), int(G), float(m), int(bool(mkt))
        ln = None
        if lengths is not None:
            ln = np.ascontiguousarray(lengths, dtype=np.uint32)
            if ln.ndim != 1 or (0 <= int(a) < self.n_assemblies and len(ln) != self.n_records(a)):
                raise ValueError("format_paths: lengths needs one entry per record of the assembly")
        v = capi.PathNodesView()
        rc = self._lib.mxg_format_paths(self._h, int(a), C.byref(p), None if ln is None else ln.ctypes.data, C.byref(v))
        if rc < 0:
            err = MxError(rc, (self._lib.mxg_last_error(self._h) or b"").decode())
            # the one error that fills the view is the negative overhang (include/ntjoin_mx.h): no other leaves node_first set
            err.nodes = self._path_nodes(v) if rc == capi.MXG_EINVAL and v.node_first else None
            raise err
        return self._path_nodes(v)

    @staticmethod
    def _path_nodes(v):
        n = int(v.n_nodes)
        out = {"node_first": _np(v.node_first, int(v.n_paths) + 1, np.uint64), "reverse": _np(v.reverse, n, np.uint8),
               "gap_size": _np(v.gap_size, n, np.int64), "raw_gap_size": _np(v.raw_gap_size, n, np.int64)}
        for name in ("record", "start", "end", "contig_size", "first_vertex", "terminal_vertex", "segment"):
            out[name] = _np(getattr(v, name), n, np.uint32)
        return out

    def mk_stats(self, values, run_first):
        """the same statistics of caller-given runs: run r = values[run_first[r]:run_first[r + 1]] -> (s int64, tie_term uint64)"""
        x = np.ascontiguousarray(values, dtype=np.uint32)
        rf = np.ascontiguousarray(run_first, dtype=np.uint64)
        if rf.ndim != 1 or len(rf) == 0 or int(rf[-1]) > len(x):
            raise ValueError("mk_stats: run_first needs n_runs + 1 offsets, the last one at most len(values)")
        n_runs = len(rf) - 1
        s, t = np.zeros(n_runs, dtype=np.int64), np.zeros(n_runs, dtype=np.uint64)
        self._check(self._lib.mxg_mk_stats(self._h, x.ctypes.data, rf.ctypes.data, n_runs, s.ctypes.data, t.ctypes.data))
        return s, t

    OVERLAP_NODE = np.dtype([("record", "<u4"), ("start", "<u4"), ("end", "<u4"), ("raw_gap", "<i4"), ("reverse", "u1"),
                             ("pad", "u1", (3,))])

    def overlap_cuts(self, assembly, nodes, path_first, k=15, w=10):
        """mxg_overlap_cuts: nodes = array of OVERLAP_NODE (or rows (record, start, end, raw_gap, reverse)), path_first = n_paths + 1
        offsets -> dict(start_adjust u32[n], end_adjust u32[n], cut_found bool[n]: the junction behind node i got a cut)"""
        if not (isinstance(nodes, np.ndarray) and nodes.dtype == self.OVERLAP_NODE):
            rows = np.asarray(nodes, dtype=np.int64).reshape(-1, 5)
            nodes = np.zeros(len(rows), dtype=self.OVERLAP_NODE)
            for j, name in enumerate(("record", "start", "end", "raw_gap", "reverse")):
                nodes[name] = rows[:, j]
        nodes = np.ascontiguousarray(nodes)
        pf = np.ascontiguousarray(path_first, dtype=np.uint64)
        if len(pf) < 1 or int(pf[-1]) != len(nodes):
            raise ValueError("overlap_cuts: path_first needs n_paths + 1 offsets, the last one len(nodes)")
        n = len(nodes)
        sa, ea, cf = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8)
        self._check(self._lib.mxg_overlap_cuts(self._h, int(assembly), int(k), int(w), nodes.ctypes.data, pf.ctypes.data, len(pf) - 1,
                                               sa.ctypes.data, ea.ctypes.data, cf.ctypes.data))
        return {"start_adjust": sa, "end_adjust": ea, "cut_found": cf.astype(bool)}

    ADJUST_NODE = np.dtype([("record", "<u4"), ("start", "<u4"), ("end", "<u4"), ("contig_size", "<u4"), ("first_mx", "<u8"),
                            ("terminal_mx", "<u8"), ("gap_size", "<i8"), ("raw_gap_size", "<i8"), ("ori", "u1"), ("pad", "u1", (7,))])

    def adjust_paths(self, nodes, path_first, no_cut=False, G=0):
        """mxg_adjust_paths: nodes = array of ADJUST_NODE (ori: 0 '+', 1 '-', 2 '?'), path_first = n_paths + 1 offsets -> dict(nodes:
        the adjusted paths' nodes (ADJUST_NODE), node_first u64[n_paths + 1], source u64[n]: the input node every output node is).
        Merged relocations, --no_cut and the overlapping regions of all paths in the reference's order (include/ntjoin_mx.h)."""
        nodes = np.ascontiguousarray(nodes, dtype=self.ADJUST_NODE)
        pf = np.ascontiguousarray(path_first, dtype=np.uint64)
        if pf.ndim != 1 or len(pf) < 1 or int(pf[0]) != 0 or int(pf[-1]) != len(nodes):
            raise ValueError("adjust_paths: path_first needs n_paths + 1 offsets, the first one 0 and the last one len(nodes)")
        p = capi.AdjustParams()
        p.struct_size, p.no_cut, p.G = C.sizeof(capi.AdjustParams), int(bool(no_cut)), int(G)
        v = capi.AdjustedView()
        self._check(self._lib.mxg_adjust_paths(self._h, nodes.ctypes.data, pf.ctypes.data, len(pf) - 1, C.byref(p), C.byref(v)))
        n = int(v.n_nodes)
        out = np.zeros(n, dtype=self.ADJUST_NODE)
        if n:
            C.memmove(out.ctypes.data, v.nodes, n * self.ADJUST_NODE.itemsize)
        return {"nodes": out, "node_first": _np(v.node_first, int(v.n_paths) + 1, np.uint64), "source": _np(v.source, n, np.uint64)}

    SEQ_PIECE = np.dtype([("record", "<u4"), ("start", "<u4"), ("end", "<u4"), ("kind", "<u4")])

    def compose_pieces(self, outer, outer_first, inner, inner_first):
        """mxg_compose_pieces: two piece tables (arrays of SEQ_PIECE or rows (record, start, end, kind), kind = capi.PIECE_FWD /
        PIECE_REV / PIECE_GAP, and n_records + 1 offsets each); outer's records index inner's -> (pieces, first): outer's records
        spelled over whatever inner refers to, neighbouring gaps joined (include/ntjoin_mx.h)."""
        def table(pieces, first):
            a = np.asarray(pieces)
            if a.dtype != self.SEQ_PIECE:
                rows = np.asarray(pieces, dtype=np.uint32).reshape(-1, 4)
                a = np.zeros(len(rows), dtype=self.SEQ_PIECE)
                for c, name in enumerate(self.SEQ_PIECE.names):
                    a[name] = rows[:, c]
            f = np.ascontiguousarray(first, dtype=np.uint64)
            if f.ndim != 1 or len(f) < 1 or int(f[-1]) != len(a):
                raise ValueError("compose_pieces: a table needs n_records + 1 offsets, the last one the number of its pieces")
            return np.ascontiguousarray(a), f
        op, of = table(outer, outer_first)
        ip, jf = table(inner, inner_first)
        pp, pf = C.c_void_p(), C.POINTER(C.c_uint64)()
        self._check(self._lib.mxg_compose_pieces(self._h, op.ctypes.data, of.ctypes.data, len(of) - 1, ip.ctypes.data, jf.ctypes.data,
                                                 len(jf) - 1, C.byref(pp), C.byref(pf)))
        first = _np(pf, len(of), np.uint64)
        out = np.zeros(int(first[-1]), dtype=self.SEQ_PIECE)
        if len(out):
            C.memmove(out.ctypes.data, pp, len(out) * self.SEQ_PIECE.itemsize)
        return out, first

    LIFT_PART = np.dtype([("s_record", "<u4"), ("s_start", "<u4"), ("s_end", "<u4"), ("src_start", "<u4"), ("reverse", "u1")])

    def lift_prepare(self, pieces, first, source_length):
        """mxg_lift_prepare: the index of a piece table (SEQ_PIECE or rows, and n_records + 1 offsets) over source records of the
        lengths source_length, built on the device and kept by the handle until the next lift_prepare (include/ntjoin_mx.h)"""
        pc = np.asarray(pieces)
        if pc.dtype != self.SEQ_PIECE:
            rows = np.asarray(pieces, dtype=np.uint32).reshape(-1, 4)
            pc = np.zeros(len(rows), dtype=self.SEQ_PIECE)
            for c, name in enumerate(self.SEQ_PIECE.names):
                pc[name] = rows[:, c]
        pc = np.ascontiguousarray(pc)
        pf = np.ascontiguousarray(first, dtype=np.uint64)
        if pf.ndim != 1 or len(pf) < 1 or int(pf[-1]) != len(pc):
            raise ValueError("lift_prepare: a table needs n_records + 1 offsets, the last one the number of its pieces")
        sl = np.ascontiguousarray(source_length, dtype=np.uint32)
        if sl.ndim != 1:
            raise ValueError("lift_prepare: source_length needs one entry per source record")
        self._lift_shape = None
        self._check(self._lib.mxg_lift_prepare(self._h, pc.ctypes.data, pf.ctypes.data, len(pf) - 1, sl.ctypes.data, len(sl)))
        self._lift_shape = (len(sl), len(pf) - 1)

    def lift_intervals(self, record, start, end, whole_only=False):
        """mxg_lift_intervals: the features (record[i], start[i], end[i]) of the source records through the prepared index ->
        (status: u8 per feature (capi.LIFT_*), part_first: u64[n + 1], parts: array of LIFT_PART); whole_only: a feature that is not
        WHOLE keeps its status and gives no parts"""
        r, a, b = (np.ascontiguousarray(x, dtype=np.uint32) for x in (record, start, end))
        if r.ndim != 1 or r.shape != a.shape or r.shape != b.shape:
            raise ValueError("lift_intervals: record, start and end need one entry per feature each")
        v = capi.LiftView()
        self._check(self._lib.mxg_lift_intervals(self._h, r.ctypes.data, a.ctypes.data, b.ctypes.data, len(r),
                                                 capi.LIFT_WHOLE_ONLY if whole_only else 0, C.byref(v)))
        n, n_parts = int(v.n_features), int(v.n_parts)
        parts = np.zeros(n_parts, dtype=self.LIFT_PART)
        for name in ("s_record", "s_start", "s_end", "src_start"):
            parts[name] = _np(getattr(v, name), n_parts, np.uint32)
        parts["reverse"] = _np(v.reverse, n_parts, np.uint8)
        return _np(v.status, n, np.uint8), _np(v.part_first, n + 1, np.uint64), parts

    def lift_bed(self, bed, source_names, scaffold_names, lifted, unlifted=None, whole_only=False):
        """mxg_lift_bed: the features of the BED file `bed`, named by source_names (one per source record of the prepared index),
        lifted into `lifted` with the records named by scaffold_names (one per record of the table), formatted on the device;
        `unlifted`: what was not lifted whole, with the reason -> dict of capi.LIFT_STATS_FIELDS"""
        shape = getattr(self, "_lift_shape", None)
        if shape is not None and (len(source_names), len(scaffold_names)) != shape:
            raise ValueError(f"lift_bed: {len(source_names)} source names and {len(scaffold_names)} scaffold names for an index of "
                             f"{shape[0]} source records and {shape[1]} records")
        src = (C.c_char_p * max(len(source_names), 1))(*[str(i).encode() for i in source_names])
        dst = (C.c_char_p * max(len(scaffold_names), 1))(*[str(i).encode() for i in scaffold_names])
        st = capi.LiftStats()
        self._check(self._lib.mxg_lift_bed(self._h, os.fsencode(str(bed)), src, dst, os.fsencode(str(lifted)),
                                           None if unlifted is None else os.fsencode(str(unlifted)), capi.LIFT_WHOLE_ONLY if whole_only else 0,
                                           C.byref(st)))
        return {name: int(getattr(st, name)) for name in capi.LIFT_STATS_FIELDS}

    SCAFFOLD_NODE = np.dtype([("record", "<u4"), ("start", "<u4"), ("end", "<u4"), ("gap_size", "<u4"), ("start_adjust", "<u4"),
                              ("end_adjust", "<u4"), ("reverse", "u1"), ("pad", "u1", (3,))])

    def write_scaffolds(self, assembly, rows, path_first, overlap_gap=None, fold_case=False, assigned=None, unassigned=None, bed=None,
                        bgzf=False, fai=False, report=False, keep=False):
        """mxg_write_scaffolds: rows = array of SCAFFOLD_NODE (or rows (record, start, end, gap_size, start_adjust, end_adjust,
        reverse)), path_first = n_paths + 1 offsets; overlap_gap=None: the overlap stage is off (the adjustments are not read).
        Writes the scaffold FASTA `assigned` and, when named, the unassigned FASTA and BED -> dict(lead_strip u32[n_paths],
        tail_strip u32[n_paths]: N/n stripped from the scaffolds' ends, n_unassigned: records in the unassigned FASTA).
        bgzf=True: the two FASTA files are BGZF files of the same bytes, deflated on the device (MXG_SCAF_BGZF); fai=True: beside
        either FASTA its <name>.fai and, with bgzf, its <name>.gzi (MXG_SCAF_FAI); report=True: the windows of either FASTA go through
        the report's passes on their way out (MXG_SCAF_REPORT; scaffold_report() hands the reports out); keep=True: the bytes of both
        FASTA files, one behind the other, stay in device memory (MXG_SCAF_KEEP; scaffold_text(), scaffold_pieces()), and no file
        need be named"""
        if assigned is None and not keep:
            raise ValueError("write_scaffolds: assigned= names the scaffold FASTA to write")
        nodes = self._scaffold_nodes(rows)
        pf = np.ascontiguousarray(path_first, dtype=np.uint64)
        if len(pf) < 1 or int(pf[0]) != 0 or int(pf[-1]) != len(nodes):
            raise ValueError("write_scaffolds: path_first needs n_paths + 1 offsets, the first one 0 and the last one len(nodes)")
        n_paths = len(pf) - 1
        lead, tail = np.zeros(n_paths, dtype=np.uint32), np.zeros(n_paths, dtype=np.uint32)
        n_un = C.c_uint64(0)
        enc = lambda p: None if p is None else os.fsencode(str(p))  # noqa: E731
        self._check(self._lib.mxg_write_scaffolds(self._h, int(assembly), nodes.ctypes.data, pf.ctypes.data, n_paths,
                                                  -1 if overlap_gap is None else int(overlap_gap),
                                                  (capi.SCAF_FOLD_CASE if fold_case else 0) | (capi.SCAF_BGZF if bgzf else 0) | (capi.SCAF_FAI if fai else 0) |
                                                  (capi.SCAF_REPORT if report else 0) | (capi.SCAF_KEEP if keep else 0),
                                                  enc(assigned), enc(unassigned), enc(bed),
                                                  lead.ctypes.data, tail.ctypes.data, C.byref(n_un)))
        return {"lead_strip": lead, "tail_strip": tail, "n_unassigned": int(n_un.value)}

    def scaffold_text(self):
        """mxg_scaffold_text: (device address, bytes, records) of the text the last write_scaffolds(keep=True) left in device memory"""
        p, n, r = C.c_void_p(), C.c_uint64(), C.c_uint64()
        self._check(self._lib.mxg_scaffold_text(self._h, C.byref(p), C.byref(n), C.byref(r)))
        return int(p.value or 0), int(n.value), int(r.value)

    def scaffold_pieces(self):
        """mxg_scaffold_pieces: what the records of the kept text are made of -> (pieces: array of SEQ_PIECE over the records of the
        assembly the scaffolds were cut from, first: u64[n_records + 1], ids: the records' names)"""
        pp, pf, n = C.c_void_p(), C.POINTER(C.c_uint64)(), C.c_uint64()
        self._check(self._lib.mxg_scaffold_pieces(self._h, C.byref(pp), C.byref(pf), C.byref(n)))
        first = _np(pf, int(n.value) + 1, np.uint64)
        out = np.zeros(int(first[-1]), dtype=self.SEQ_PIECE)
        if len(out):
            C.memmove(out.ctypes.data, pp, len(out) * self.SEQ_PIECE.itemsize)
        return out, first, [self._lib.mxg_scaffold_record_id(self._h, r).decode() for r in range(int(n.value))]

    SYNTENY_FIELDS = ("n_anchors", "q_record", "q_start", "q_end", "s_record", "s_start", "s_end")

    def synteny_blocks(self, q, s, max_gap=100000, min_anchors=3, min_span=0, pieces=None, first=None, query_length=None,
                       subject_length=None):
        """mxg_synteny_blocks: the maximal collinear runs of graph vertices between query assembly q and subject assembly s
        (include/ntjoin_mx.h) -> dict(n_blocks, n_anchors_total, n_links, and per kept block n_anchors, q_record, q_start, q_end,
        s_record, s_start, s_end (u32), reverse (u8)).  pieces / first: a piece table over the records of q (SEQ_PIECE or rows, and
        n_records + 1 offsets; scaffold_pieces() gives the scaffolds'); query_length / subject_length: one length per record of q / s
        where the handle holds none (minimizer input)."""
        p = capi.SyntenyParams()
        p.struct_size, p.max_gap, p.min_anchors, p.min_span = C.sizeof(capi.SyntenyParams), int(max_gap), int(min_anchors), int(min_span)
        pc = pf = None
        if pieces is not None:
            pc = np.asarray(pieces)
            if pc.dtype != self.SEQ_PIECE:
                rows = np.asarray(pieces, dtype=np.uint32).reshape(-1, 4)
                pc = np.zeros(len(rows), dtype=self.SEQ_PIECE)
                for c, name in enumerate(self.SEQ_PIECE.names):
                    pc[name] = rows[:, c]
            pc = np.ascontiguousarray(pc)
            pf = np.ascontiguousarray(first, dtype=np.uint64)
            if pf.ndim != 1 or len(pf) < 1 or int(pf[-1]) != len(pc):
                raise ValueError("synteny_blocks: a table needs n_records + 1 offsets, the last one the number of its pieces")

        def lengths(ln, a, what):
            if ln is None:
                return None
            ln = np.ascontiguousarray(ln, dtype=np.uint32)
            if ln.ndim != 1 or (0 <= int(a) < self.n_assemblies and len(ln) != self.n_records(a)):
                raise ValueError(f"synteny_blocks: {what}_length needs one entry per record of the assembly")
            return ln
        ql, sl = lengths(query_length, q, "query"), lengths(subject_length, s, "subject")
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        v = capi.SyntenyView()
        self._check(self._lib.mxg_synteny_blocks(self._h, int(q), int(s), C.byref(p), ptr(pc), ptr(pf), 0 if pf is None else len(pf) - 1, ptr(ql), ptr(sl), C.byref(v)))
        self._syn_records = self.n_records(q) if pf is None else len(pf) - 1
        n = int(v.n_blocks)
        out = {"n_blocks": n, "n_anchors_total": int(v.n_anchors_total), "n_links": int(v.n_links), "reverse": _np(v.reverse, n, np.uint8)}
        for name in self.SYNTENY_FIELDS:
            out[name] = _np(getattr(v, name), n, np.uint32)
        return out

    def write_synteny_paf(self, path, query_names=None, append=False, identity=False):
        """mxg_write_synteny_paf_ex: the blocks of the last synteny_blocks() as PAF lines, formatted on the device; query_names = one name
        per query record (None: the handle's record ids of q -- not for a query that went through a piece table); append=True adds
        the lines to what `path` holds already; identity=True: every line also carries al:i, NM:i and dv:f of the last
        synteny_identity() (MXG_PAF_IDENTITY)"""
        names = None
        if query_names is not None:
            if len(query_names) != getattr(self, "_syn_records", len(query_names)):
                raise ValueError(f"write_synteny_paf: {len(query_names)} names for {self._syn_records} query records")
            names = (C.c_char_p * max(len(query_names), 1))(*[str(i).encode() for i in query_names])
        self._check(self._lib.mxg_write_synteny_paf_ex(self._h, names, os.fsencode(str(path)), int(bool(append)), capi.PAF_IDENTITY if identity else 0))

    def synteny_identity(self, max_seg=capi.IDY_DEFAULT_MAX_SEG):
        """mxg_synteny_identity: the banded edit distances of the segments between the anchors of the kept blocks of the last
        synteny_blocks() (include/ntjoin_mx.h) -> dict(the summary: n_blocks, n_segments, n_aligned, n_skip_len, n_skip_shift, n_skip_n,
        n_saturated, block_q, aligned_q, aligned_s, edits; blocks: dict of u64 arrays by capi.IDENTITY_BLOCK_FIELDS)"""
        p = capi.IdentityParams()
        p.struct_size, p.max_seg = C.sizeof(capi.IdentityParams), int(max_seg)
        v = capi.IdentityView()
        self._check(self._lib.mxg_synteny_identity(self._h, C.byref(p), C.byref(v)))
        out = {name: int(getattr(v, name)) for name in capi.IDENTITY_SUM_FIELDS}
        out["blocks"] = {name: _np(getattr(v, "blk_" + name), out["n_blocks"], np.uint64) for name in capi.IDENTITY_BLOCK_FIELDS}
        return out

    def synteny_assess(self, merge_gap=100000, max_indel=1000, join_indel=100000):
        """mxg_synteny_assess: the kept blocks of the last synteny_blocks() merged into chains, the breakpoints between the chains and
        the summary (include/ntjoin_mx.h) -> dict(n_blocks, n_chains, n_breakpoints, breakpoints: {(kind, at_join): count} with kind in
        capi.BP_*, query_bases, subject_bases, aligned_query, chained_subject, covered_subject, na / nga / ng: dict(n50, l50, n75, l75,
        n90, l90), chains: dict of u32 arrays by capi.ASSESS_CHAIN_FIELDS, bps: dict of u32 arrays by capi.ASSESS_BP_FIELDS)."""
        p = capi.AssessParams()
        p.struct_size, p.merge_gap, p.max_indel, p.join_indel = C.sizeof(capi.AssessParams), int(merge_gap), int(max_indel), int(join_indel)
        v = capi.AssessView()
        self._check(self._lib.mxg_synteny_assess(self._h, C.byref(p), C.byref(v)))
        out = {name: int(getattr(v, name)) for name in ("n_blocks", "n_chains", "n_breakpoints", "query_bases", "subject_bases", "aligned_query",
                                                        "chained_subject", "covered_subject")}
        out["breakpoints"] = {(kind, j): int(v.breakpoints[kind][j]) for kind in range(3) for j in range(2)}
        for which in ("na", "nga", "ng"):
            out[which] = {name: int(getattr(getattr(v, which), name)) for name, _ in capi.Nx._fields_}
        out["chains"] = {name: _np(getattr(v, "chain_" + name), out["n_chains"], np.uint32) for name in capi.ASSESS_CHAIN_FIELDS}
        out["bps"] = {name: _np(getattr(v, "bp_" + name), out["n_breakpoints"], np.uint32) for name in capi.ASSESS_BP_FIELDS}
        return out

    IDENTITY_SEG = np.dtype([(name, "<u4") for name in ("q_record", "q_start", "lq", "s_record", "s_start", "ls", "reverse", "pad")])

    def identity_segments(self, q_text, s_text, segs, max_seg=capi.IDY_DEFAULT_MAX_SEG):
        """mxg_identity_segments: the banded edit distance of explicit segments over two texts the handle holds on the device
        (include/ntjoin_mx.h).  q_text / s_text: an assembly index or capi.TEXT_SCAFFOLDS (the text write_scaffolds(keep=True) left);
        segs: array of IDENTITY_SEG, or rows (q_record, q_start, lq, s_record, s_start, ls, reverse) -> dict(edits u32[n], status
        u32[n]: capi.IDY_ALIGNED .. IDY_SKIP_N, saturated bool[n])"""
        sg = np.asarray(segs)
        if sg.dtype != self.IDENTITY_SEG:
            rows = np.asarray(segs, dtype=np.uint32).reshape(-1, 7)
            sg = np.zeros(len(rows), dtype=self.IDENTITY_SEG)
            for c, name in enumerate(self.IDENTITY_SEG.names[:7]):
                sg[name] = rows[:, c]
        sg = np.ascontiguousarray(sg)
        n = len(sg)
        edits, status = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        self._check(self._lib.mxg_identity_segments(self._h, int(q_text), int(s_text), sg.ctypes.data if n else None, n, int(max_seg),
                                                    edits.ctypes.data if n else None, status.ctypes.data if n else None))
        return {"edits": edits, "status": status & capi.IDY_STATUS_MASK, "saturated": (status & capi.IDY_SATURATED) != 0}

    def write_fai(self, assembly, path, gzi=None):
        """mxg_write_fai: the index `samtools faidx` makes of the assembly's FASTA, from the text the handle holds, written to `path`;
        gzi= names the .gzi to write for an assembly that came from a BGZF file"""
        enc = lambda p: None if p is None else os.fsencode(str(p))  # noqa: E731
        self._check(self._lib.mxg_write_fai(self._h, int(assembly), enc(path), enc(gzi)))

    def set_report_params(self, min_gap=10, min_len=500):
        """mxg_set_report_params: a gap is an N run of at least min_gap bases (0 is refused); the contiguity blocks are taken over the
        lengths of at least min_len"""
        self._check(self._lib.mxg_set_report_params(self._h, int(min_gap), int(min_len)))

    @staticmethod
    def _report_dict(rep):
        block = lambda b: {name: int(getattr(b, name)) for name, _ in capi.Contiguity._fields_}  # noqa: E731
        out = {name: int(getattr(rep, name)) for name in ("min_gap", "min_len", "n_records", "bases", "a", "c", "g", "t", "n", "other", "lower",
                                                          "n_gaps", "gap_bases", "max_gap")}
        out["scaffold"], out["contig"] = block(rep.scaffold), block(rep.contig)
        out["gap_len"] = _np(rep.gap_len, out["n_gaps"], np.uint64)
        out["contig_len"] = _np(rep.contig_len, out["contig"]["n"], np.uint64)
        return out

    def assembly_report(self, assembly):
        """mxg_assembly_report: contiguity, base composition and N gaps of a loaded assembly, from the text the handle holds -> a dict:
        min_gap, min_len, n_records, bases, a, c, g, t, n, other, lower, n_gaps, gap_bases, max_gap, scaffold / contig (dicts: n, n_min,
        sum, min, max, n50, l50, n75, l75, n90, l90) and gap_len / contig_len (u64 arrays, copies, in no particular order)"""
        rep = capi.SeqReport(struct_size=C.sizeof(capi.SeqReport))
        self._check(self._lib.mxg_assembly_report(self._h, int(assembly), C.byref(rep)))
        return self._report_dict(rep)

    def scaffold_report(self, which="all"):
        """mxg_scaffold_report: the report of a file the last write_scaffolds(report=True) wrote; which = "assigned", "unassigned" or
        "all" (the file that holds both) -> a dict as assembly_report returns"""
        code = {"assigned": capi.REPORT_ASSIGNED, "unassigned": capi.REPORT_UNASSIGNED, "all": capi.REPORT_ALL}.get(which, which)
        rep = capi.SeqReport(struct_size=C.sizeof(capi.SeqReport))
        self._check(self._lib.mxg_scaffold_report(self._h, int(code), C.byref(rep)))
        return self._report_dict(rep)

    def bgzf_write(self, data, path):
        """mxg_bgzf_write: the bytes of `data` (bytes, bytearray, or a contiguous uint8 array) written to `path` as a BGZF file,
        deflated on the device"""
        buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
        self._check(self._lib.mxg_bgzf_write(self._h, buf.ctypes.data if buf.size else None, int(buf.size), os.fsencode(str(path))))

    def _scaffold_nodes(self, rows):
        "rows (record, start, end, gap_size, start_adjust, end_adjust, reverse), or an array of SCAFFOLD_NODE -> that array"
        nodes = rows
        if not (isinstance(nodes, np.ndarray) and nodes.dtype == self.SCAFFOLD_NODE):
            arr = np.asarray(rows, dtype=np.int64).reshape(-1, 7)
            nodes = np.zeros(len(arr), dtype=self.SCAFFOLD_NODE)
            for j, name in enumerate(("record", "start", "end", "gap_size", "start_adjust", "end_adjust", "reverse")):
                nodes[name] = arr[:, j]
        return np.ascontiguousarray(nodes)

    def write_paths(self, assembly, rows, path_first, lead_strip=None, tail_strip=None, first_line="", path=None, agp=None,
                    agp_unassigned=False):
        """mxg_write_paths: the .path file `path` (line 1 = first_line, then one line per path) and, when named, the AGP `agp` of the
        paths, formatted on the device.  rows / path_first as write_scaffolds takes them, lead_strip / tail_strip = what it
        returned (None: no strips); agp_unassigned=True appends the AGP lines of the unassigned intervals the handle's last
        write_scaffolds left behind."""
        if path is None:
            raise ValueError("write_paths: path= names the .path file to write")
        nodes = self._scaffold_nodes(rows)
        pf = np.ascontiguousarray(path_first, dtype=np.uint64)
        if pf.ndim != 1 or len(pf) < 1:
            raise ValueError("write_paths: path_first needs n_paths + 1 offsets")
        n_paths = len(pf) - 1
        if len(pf) and int(pf[-1]) > len(nodes):
            raise ValueError("write_paths: path_first reaches beyond the nodes")
        strips = []
        for name, s in (("lead_strip", lead_strip), ("tail_strip", tail_strip)):
            if s is not None:
                s = np.ascontiguousarray(s, dtype=np.uint32)
                if s.shape != (n_paths,):
                    raise ValueError(f"write_paths: {name} needs one entry per path")
            strips.append(s)
        enc = lambda p: None if p is None else os.fsencode(str(p))  # noqa: E731
        self._check(self._lib.mxg_write_paths(self._h, int(assembly), nodes.ctypes.data if len(nodes) else None, pf.ctypes.data, n_paths,
                                              None if strips[0] is None else strips[0].ctypes.data,
                                              None if strips[1] is None else strips[1].ctypes.data, str(first_line).encode("utf-8"),
                                              enc(path), enc(agp), capi.PATHS_AGP_UNASSIGNED if agp_unassigned else 0))

    def scaffold_strips(self):
        """mxg_scaffold_strips: (lead u32[n], tail u32[n]) = N/n stripped from either end of every unassigned interval (the BED's
        lines, in order) by the last write_scaffolds"""
        lead, tail, n = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.c_uint64()
        self._check(self._lib.mxg_scaffold_strips(self._h, C.byref(lead), C.byref(tail), C.byref(n)))
        return _np(lead, n.value, np.uint32), _np(tail, n.value, np.uint32)

    def write_outputs(self, dot_path, tsv_paths, with_pos=True, with_strand=False, with_seq=True):
        """mxg_write_outputs: the .mx.dot and the TSVs of the assemblies (None: none for that assembly) in one call"""
        arr = (C.c_char_p * max(len(tsv_paths), 1))(*[None if p is None else os.fsencode(str(p)) for p in tsv_paths])
        self._check(self._lib.mxg_write_outputs(self._h, os.fsencode(str(dot_path)), arr, int(with_pos), int(with_strand), int(with_seq)))

    def mx_extremes(self, a):
        """per record of assembly a: (min, max) position over its graph vertices; None for records without one"""
        mn, mx, n = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.c_uint64()
        self._check(self._lib.mxg_mx_extremes(self._h, int(a), C.byref(mn), C.byref(mx), C.byref(n)))
        lo, hi = _np(mn, n.value, np.uint32), _np(mx, n.value, np.uint32)
        return [None if l > h_ else (int(l), int(h_)) for l, h_ in zip(lo.tolist(), hi.tolist())]

    def dot_part_format(self, part, n_parts):
        """format part `part` of `n_parts` of the .mx.dot into memory -> (vertex segment bytes, edge segment bytes)"""
        b = (C.c_uint64 * 2)()
        self._check(self._lib.mxg_dot_part_format(self._h, int(part), int(n_parts), b))
        return int(b[0]), int(b[1])

    def dot_part_write(self, path, v_off, e_off, first, last):
        self._check(self._lib.mxg_dot_part_write(self._h, str(path).encode(), int(v_off), int(e_off), int(bool(first)), int(bool(last))))

    def write_dot(self, path):
        self._check(self._lib.mxg_write_dot(self._h, str(path).encode()))

    # -- stats ------------------------------------------------------------------------------------------------
    def stats(self):
        s = capi.Stats()
        s.struct_size = C.sizeof(capi.Stats)
        self._check(self._lib.mxg_get_stats(self._h, C.byref(s)))
        return {f: getattr(s, f) for f, _ in capi.Stats._fields_ if f not in ("struct_size", "reserved")}

    def knobs(self):
        """the MXG_* environment knobs this handle has read and found set: 'NAME=value ...' (parsed once per handle)"""
        buf = C.create_string_buffer(4096)
        self._lib.mxg_knobs(self._h, buf, 4096)
        return buf.value.decode()

    def reset_timers(self):
        self._check(self._lib.mxg_reset_timers(self._h))
