"""tests/_assess_cases.py's cover_case at any size and on two subject records, as numpy arrays and with its kept blocks in closed form
(the manner of tests/_synteny_scale.py): what puts the assessment's running maximum of (s_record << 32) | s_end -- the largest
subject end in front of every chain, which decides covered_subject -- on its carries.  tests/test_cover_scale_cpu.py pins the closed
form against the restatements at small sizes; tests/test_gpu_assess.py runs it with the second record's long chain at sorted place
1023 (the last of tile 0) and 262 143 (the last of the first round of k_pt_max_tiles).  No GPU, no library.

For subject record r (0, 1) with m = m_r:
  query record 2 r      one chain of chain_blocks(m) blocks of two anchors, block b at 200 b on the query and 1000 + 200 b on the
                        subject: collinear and 118 apart on both, so one chain over s [1000, chain_end(m))
  query record 2 r + 1  m single blocks of two anchors, block j at 200 j on the query and chain_end(m) - 83 - 4 j on the subject: inside
                        the chain's interval, from its far end inwards (on odd places: the chain's anchors lie on even ones).  The subject
                        falls while the query rises, so no two join: m chains
In (s_record, s_start) order the chains are: record 0's long one, its singles from the last to the first, record 1's long one (place
m0 + 1), its singles.  Every single lies under its record's long chain: covered_subject is the two long spans, and a single that
sees another maximum in front of it -- none, or record 0's -- adds bases of its own to it."""
import numpy as np

K, STEP, SPAN, STRIDE, MAX_GAP = 32, 50, 82, 200, 100
ODD = 0x9E3779B97F4A7C15   # (an odd multiplier is a bijection of the 64-bit words: distinct hashes)
QUERY_NAMES, SUBJECT_NAMES = ["long0", "singles0", "long1", "singles1"], ["chr1", "chr2"]
CARRY_CASES = [(1022, 1500), (262142, 1500)]   # (m0, m1): record 1's long chain on place 1023 and 262 143, its singles over one more tile border


def chain_blocks(m):
    return (4 * m + STRIDE - 1) // STRIDE + 1


def chain_end(m):
    return 1000 + STRIDE * (chain_blocks(m) - 1) + SPAN


def blocks_of(m0, m1):
    "the kept blocks in the query's order, by _synteny_restatement.FIELDS, as int64 arrays"
    q_record, q_start, s_record, s_start = [], [], [], []
    for r, m in enumerate((m0, m1)):
        b, j = np.arange(chain_blocks(m), dtype=np.int64), np.arange(m, dtype=np.int64)
        q_record += [np.full(len(b), 2 * r), np.full(m, 2 * r + 1)]
        q_start += [STRIDE * b, STRIDE * j]
        s_record += [np.full(len(b) + m, r)]
        s_start += [1000 + STRIDE * b, chain_end(m) - 83 - 4 * j]
    q_record, q_start, s_record, s_start = (np.concatenate(x).astype(np.int64) for x in (q_record, q_start, s_record, s_start))
    n = len(q_start)
    return dict(n_anchors=np.full(n, 2, dtype=np.int64), q_record=q_record, q_start=q_start, q_end=q_start + SPAN, s_record=s_record,
                s_start=s_start, s_end=s_start + SPAN, reverse=np.zeros(n, dtype=np.int64))


def sorted_chains(m0, m1):
    "-> (place key, cover word) of the m0 + m1 + 2 chains in (s_record, s_start) order, as uint64: what the running maximum runs over"
    key, word = [], []
    for r, m in enumerate((m0, m1)):
        start = np.concatenate([[1000], chain_end(m) - 83 - 4 * np.arange(m - 1, -1, -1, dtype=np.int64)])
        end = np.concatenate([[chain_end(m)], start[1:] + SPAN])
        key.append((r << 32) + start)
        word.append((r << 32) + end)
    return np.concatenate(key).astype(np.uint64), np.concatenate(word).astype(np.uint64)


def covered(key, word, before):
    """covered_subject from the chains' place keys and cover words and, for every chain, the running maximum of the cover words in
    front of it: ntjoin_amd/csrc/assess.h, as_uncovered, summed"""
    s_record, s_start, s_end = (key >> 32).astype(np.int64), (key & 0xFFFFFFFF).astype(np.int64), (word & 0xFFFFFFFF).astype(np.int64)
    b_record, b_end = (before >> 32).astype(np.int64), (before & 0xFFFFFFFF).astype(np.int64)
    start = np.where((before != 0) & (b_record == s_record) & (b_end > s_start), b_end, s_start)
    return int(np.maximum(s_end - start, 0).sum())


def cover_scale_case(m0, m1):
    """-> dict in the manner of _synteny_scale.scale_case: anchors (qrec, qpos, srec, spos in the query's order), asms (subject first),
    lengths (per assembly), expect (the kept blocks), n_anchors_total, n_links, and of the assessment n_chains, covered_subject,
    chained_subject"""
    expect = blocks_of(m0, m1)
    n = len(expect["q_start"])
    step = np.tile(np.array([0, STEP], dtype=np.int64), n)
    qrec, qpos = np.repeat(expect["q_record"], 2), np.repeat(expect["q_start"], 2) + step
    srec, spos = np.repeat(expect["s_record"], 2), np.repeat(expect["s_start"], 2) + step
    with np.errstate(over="ignore"):
        hsh = (np.arange(1, 2 * n + 1, dtype=np.uint64) * np.uint64(ODD)).astype(np.uint64)

    def assembly(rec, pos, names):
        order = np.lexsort((pos, rec))
        return dict(hash=hsh[order], pos=pos[order].astype(np.uint32), record=rec[order].astype(np.uint32), names=names)

    def lengths(rec, pos, n_rec):
        out = np.full(n_rec, K + 100, dtype=np.int64)
        np.maximum.at(out, rec, pos + K + 100)
        return out.astype(np.uint32)

    spans = [chain_end(m) - 1000 for m in (m0, m1)]
    return dict(k=K, max_gap=MAX_GAP, min_anchors=2, anchors=(qrec, qpos, srec, spos),
                asms=[assembly(srec, spos, SUBJECT_NAMES), assembly(qrec, qpos, QUERY_NAMES)],
                lengths=[lengths(srec, spos, len(SUBJECT_NAMES)), lengths(qrec, qpos, len(QUERY_NAMES))],
                expect=expect, n_anchors_total=2 * n, n_links=n, n_chains=m0 + m1 + 2, covered_subject=sum(spans),
                chained_subject=sum(spans) + SPAN * (m0 + m1))
