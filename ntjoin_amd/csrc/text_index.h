// text_index.h -- the FASTA text in HBM as the device ingest leaves it (ingest.hip): the work items (tiles of the file cut at
// record borders), the byte classes, and the lookup from a base of a record to its byte in the text.  Shared by the TSV writer
// (ingest.hip: the k-mer column) and the scaffold writer (scaffold.hip: every text piece of the output).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "bisect.h"

namespace mxg {

constexpr uint32_t ING_TILE = 4096;  // text bytes per work item: one aligned tile of the file, cut at record borders

struct IngItem {
    uint64_t lo;   // first text byte
    uint32_t len;  // bytes (all inside one tile)
    uint32_t rec;  // record
};

// byte class: 0..3 = A C G T(U) (either case), 4 = any other base character (invalid), 5 = line break (not a base)
__device__ __forceinline__ uint32_t byte_class(uint32_t b)
{
    if (b == '\n' || b == '\r') return 5u;
    const uint32_t u = b & 0xDFu;  // upper case
    return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : (u == 'T' || u == 'U') ? 3u : 4u;
}

// the tile index of an assembly's text: what Assembly::d_text, d_ing_items, d_ing_pbase, d_ing_sub, d_ing_item0 hold
struct TextIndex {
    const unsigned char *text;
    const IngItem *items;
    const uint64_t *item_pbase;  // packed base index of every item's first base
    const uint16_t *item_sub;    // bases in each of an item's 16 sub-tiles of 256 bytes
    const uint64_t *rec_item0;   // [n_rec + 1] first item of every record
    const uint64_t *rec_base;    // [n_rec] packed base offset of record r
};

// text offset of base `pos` of record r: the tile by binary search over the tiles' first base indices, the 256-byte
// sub-tile by its 16 counts, then a scan over at most 256 bytes
__device__ __forceinline__ uint64_t text_of_base(const TextIndex &p, uint32_t r, uint32_t pos)
{
    const uint64_t want = p.rec_base[r] + pos;
    const uint64_t lo = last_le(p.item_pbase, p.rec_item0[r], p.rec_item0[r + 1], want);
    const IngItem it = p.items[lo];
    uint32_t local = (uint32_t)(want - p.item_pbase[lo]);
    const uint64_t tile = it.lo & ~(uint64_t)(ING_TILE - 1);
    uint32_t s = 0;
    for (; s < 15; ++s) {
        const uint32_t c = p.item_sub[lo * 16u + s];
        if (local < c) break;
        local -= c;
    }
    uint64_t a = tile + 256u * s;
    if (a < it.lo) a = it.lo;
    for (;; ++a) {  // (the base is there: the counts say so)
        const uint32_t c = byte_class(p.text[a]);
        if (c != 5u) {
            if (local == 0) return a;
            --local;
        }
    }
}

}  // namespace mxg
