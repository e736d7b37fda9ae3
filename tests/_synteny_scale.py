"""A two-assembly synteny input of any size as numpy arrays, with its blocks written down in closed form: B blocks of 17 anchors each
(tests/test_gpu_primitives.py runs it at 4.46 M anchors, past the second pass of the 32-bit scans and the second round of the 64-bit
scan; tests/test_synteny_scale_cpu.py checks the closed form against tests/_synteny_restatement.py at B = 300).  No GPU, no library.

Block b (0 <= b < B), anchor j (0 <= j < 17), k = 32:
  query    record qrec(b): the blocks in three contiguous thirds; inside its record the block is number bl = b - (first block of the
           record); position STRIDE * bl + STEP * j
  subject  record (b // 5) % 2; position STRIDE * b + STEP * j, or STRIDE * b + STEP * (16 - j) where b is odd (the block runs backwards)
STEP = 40 is below max_gap = 100, and the last anchor of a block and the first of the next one are STRIDE - 16 * STEP = 160 apart on
the query and 800 on the subject, above it, or a record changes: every block is one maximal run of 16 links.  Neighbouring blocks differ
in direction, so no two join into a chain whatever the merge gap.
"""
import numpy as np

K, PER, STEP, STRIDE, MAX_GAP = 32, 17, 40, 800, 100
ODD = 0x9E3779B97F4A7C15   # (an odd multiplier is a bijection of the 64-bit words: distinct hashes)
QUERY_NAMES, SUBJECT_NAMES = ["scaffold_a", "b", "scaffold_number_three"], ["chr1", "chromosome_two"]


def scale_case(n_blocks):
    """-> dict: anchors (qrec, qpos, srec, spos: arrays in the query's order), asms (subject first: dict(hash, pos, record, names), sorted
    by record and position as a sketch is), lengths (per assembly), expect (the kept blocks by _synteny_restatement.FIELDS, as arrays),
    n_anchors_total, n_links"""
    B = int(n_blocks)
    b = np.repeat(np.arange(B, dtype=np.int64), PER)
    j = np.tile(np.arange(PER, dtype=np.int64), B)
    bounds = np.array([0, B // 3, 2 * B // 3, B], dtype=np.int64)
    qrec_b = np.searchsorted(bounds, np.arange(B, dtype=np.int64), side="right") - 1
    bl_b = np.arange(B, dtype=np.int64) - bounds[qrec_b]
    srec_b = (np.arange(B, dtype=np.int64) // 5) % 2
    odd_b = np.arange(B, dtype=np.int64) % 2
    qrec, qpos = qrec_b[b], STRIDE * bl_b[b] + STEP * j
    srec, spos = srec_b[b], STRIDE * b + STEP * np.where(odd_b[b] == 1, PER - 1 - j, j)
    assert qpos.max(initial=0) < 2 ** 32 - 1000 and spos.max(initial=0) < 2 ** 32 - 1000
    with np.errstate(over="ignore"):
        hsh = (np.arange(1, B * PER + 1, dtype=np.uint64) * np.uint64(ODD)).astype(np.uint64)

    def assembly(rec, pos, names):
        order = np.lexsort((pos, rec))
        return dict(hash=hsh[order], pos=pos[order].astype(np.uint32), record=rec[order].astype(np.uint32), names=names)

    def lengths(rec, pos, n_rec):
        out = np.full(n_rec, K + 100, dtype=np.int64)
        np.maximum.at(out, rec, pos + K + 100)
        return out.astype(np.uint32)

    span = STEP * (PER - 1) + K
    ar = np.arange(B, dtype=np.int64)
    expect = dict(n_anchors=np.full(B, PER), q_record=qrec_b, q_start=STRIDE * bl_b, q_end=STRIDE * bl_b + span, s_record=srec_b,
                  s_start=STRIDE * ar, s_end=STRIDE * ar + span, reverse=odd_b)
    return dict(k=K, max_gap=MAX_GAP, min_anchors=2, anchors=(qrec, qpos, srec, spos),
                asms=[assembly(srec, spos, SUBJECT_NAMES), assembly(qrec, qpos, QUERY_NAMES)],
                lengths=[lengths(srec, spos, len(SUBJECT_NAMES)), lengths(qrec, qpos, len(QUERY_NAMES))],
                expect=expect, n_anchors_total=B * PER, n_links=B * (PER - 1))
