#!/usr/bin/env python3
"""
The index of two FASTA files written one behind the other, from the indexes of the two (host only; no library is loaded).

`ntJoin-mx scaffold` makes <...>.all.scaffolds.fa as the assigned file followed by the unassigned one, and with gz=True as the
assigned BGZF file without its 28-byte end marker followed by the unassigned one.  With fai=True either part has its .fai (and
.gzi) from the run that wrote it, so the index of the whole is a matter of offsets:

    cat_fai(first_fai, first_text_bytes, second_fai, out)
        the first index, then the second with every OFFSET moved by the (uncompressed) size of the first file
    cat_gzi(first_gzi, first_file_bytes, first_text_bytes, second_gzi, second_text_bytes, out)
        the first .gzi, then a pair for the second part's first member (it is no longer the first of the file), then the second
        .gzi with the compressed offsets moved by the first file's size less its end marker and the text offsets by its text
    python -m ntjoin_amd.fai cat FIRST.fa[.gz] SECOND.fa[.gz] ALL.fa[.gz]
        ALL.fa[.gz].fai from FIRST.fa[.gz].fai and SECOND.fa[.gz].fai and, when FIRST.fa.gz.gzi exists, ALL.fa.gz.gzi
"""
import os
import struct
import sys

BGZF_EOF_BYTES = 28


def cat_fai(first_fai, first_text_bytes, second_fai, out):
    with open(first_fai, "rb") as fh:
        lines = fh.read().splitlines(keepends=True)
    with open(second_fai, "rb") as fh:
        for line in fh.read().splitlines(keepends=True):
            f = line.split(b"\t")
            f[2] = b"%d" % (int(f[2]) + int(first_text_bytes))
            lines.append(b"\t".join(f))
    with open(out, "wb") as fh:
        fh.writelines(lines)


def read_gzi(path):
    with open(path, "rb") as fh:
        b = fh.read()
    (n,) = struct.unpack_from("<Q", b, 0)
    if len(b) != 8 + 16 * n:
        raise ValueError(f"{path}: {len(b)} bytes do not hold {n} pairs")
    return [struct.unpack_from("<QQ", b, 8 + 16 * i) for i in range(n)]


def write_gzi(path, pairs):
    with open(path, "wb") as fh:
        fh.write(struct.pack("<Q", len(pairs)) + b"".join(struct.pack("<QQ", c, u) for c, u in pairs))


def cat_gzi(first_gzi, first_file_bytes, first_text_bytes, second_gzi, second_text_bytes, out):
    shift_c, shift_u = int(first_file_bytes) - BGZF_EOF_BYTES, int(first_text_bytes)
    pairs = list(read_gzi(first_gzi))
    if int(second_text_bytes) > 0 and shift_u > 0:  # (a first part without text: the second's first member is the file's first)
        pairs.append((shift_c, shift_u))
    pairs += [(c + shift_c, u + shift_u) for c, u in read_gzi(second_gzi)]
    write_gzi(out, pairs)


def bgzf_text_bytes(path):
    "the bytes of text of a BGZF file: the ISIZE of its members added up (their headers say where the next one starts)"
    total, at, size = 0, 0, os.path.getsize(path)
    with open(path, "rb") as fh:
        while at < size:
            fh.seek(at)
            head = fh.read(12)
            if len(head) < 12 or head[:4] != b"\x1f\x8b\x08\x04":
                raise ValueError(f"{path}: no BGZF member at byte {at}")
            (xlen,) = struct.unpack_from("<H", head, 10)
            extra, bsize, q = fh.read(xlen), None, 0
            while q + 4 <= len(extra):
                (slen,) = struct.unpack_from("<H", extra, q + 2)
                if extra[q:q + 2] == b"BC" and slen == 2:
                    (bsize,) = struct.unpack_from("<H", extra, q + 4)
                q += 4 + slen
            if bsize is None:
                raise ValueError(f"{path}: the member at byte {at} has no BSIZE")
            fh.seek(at + bsize + 1 - 4)
            total += struct.unpack("<I", fh.read(4))[0]
            at += bsize + 1
    return total


def cat_files(first, second, out):
    "the indexes of `out` = `first` followed by `second` (FASTA names; their .fai, and for BGZF files their .gzi, lie beside them)"
    gz = os.path.exists(first + ".gzi")
    text = bgzf_text_bytes if gz else os.path.getsize
    first_text = text(first)
    cat_fai(first + ".fai", first_text, second + ".fai", out + ".fai")
    if gz:
        cat_gzi(first + ".gzi", os.path.getsize(first), first_text, second + ".gzi", text(second), out + ".gzi")


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 4 or argv[0] != "cat":
        sys.stderr.write("usage: python -m ntjoin_amd.fai cat FIRST.fa[.gz] SECOND.fa[.gz] ALL.fa[.gz]\n")
        return 2
    cat_files(*argv[1:])
    return 0


if __name__ == "__main__":
    sys.exit(main())
