// graph_rank.h -- "is v next to u in assembly b" from rank arrays, as plain C++ (host tests and the rank variants of the edge kernels
// in graph.hip share it).
//
// Every vertex occurs exactly once in every assembly's filtered list (a shared minimizer is unique in each assembly).  With
// rank_b[v] = the place of vertex v in assembly b's list and rec_b[r] = the record of place r, v is the successor or the
// predecessor of u in b (consecutive surviving minimizers of the same contig) exactly when their places differ by one and both
// lie in one record.  Assembly 0's vertex ids ARE its places, so rank_0 is the identity and needs no array.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GRK_HD __host__ __device__ inline
#else
#define GRK_HD inline
#endif

namespace mxg {

// places that differ by one (places are < 2^32 / A: r + 1 does not wrap)
GRK_HD bool rank_adjacent(uint32_t ru, uint32_t rv) { return ru + 1u == rv || rv + 1u == ru; }

// v is a neighbour of u in an assembly where they sit at places ru and rv, in records rec_u and rec_v
GRK_HD bool rank_neighbours(uint32_t ru, uint32_t rv, uint32_t rec_u, uint32_t rec_v) { return rank_adjacent(ru, rv) && rec_u == rec_v; }

// Where the two records of a pair of places are fetched from in a row of `stride` places: the lower place and the one behind it if
// `wanted` and the places differ by one -- else place 0 twice (a load that is not needed reads a word that exists, and is
// dropped).  Returns whether the records are worth comparing.  (Both places are held against the row: the ranks of an attempt
// whose join failed, to be redone over the global table, may hold anything, and nothing beyond the row is read.)
GRK_HD bool rank_fetch(bool wanted, uint32_t ru, uint32_t rv, uint32_t stride, uint32_t &lo, uint32_t &hi)
{
    const bool f = wanted && rank_adjacent(ru, rv) && ru < stride && rv < stride;
    lo = f ? (ru < rv ? ru : rv) : 0u;
    hi = f ? (ru < rv ? rv : ru) : 0u;
    return f;
}

// Items first .. first + n - 1 of an array of n_items = rows x stride items, of whose rows the first `count` places are used (the
// rows are strided by an upper bound of the count): true iff none of them is used -- the run begins beyond the count of its row
// and ends before the next row begins.  (A run that begins beyond the array is unused.)
GRK_HD bool rank_items_unused(uint32_t first, uint32_t n, uint32_t n_items, uint32_t stride, uint32_t count)
{
    if (first >= n_items || n == 0u || count == 0u) return true;
    const uint32_t last = (uint32_t)((uint64_t)first + n <= n_items ? first + n - 1u : n_items - 1u);
    const uint32_t a = first / stride;
    return first - a * stride >= count && last / stride == a;
}

// The support mask of the pair (u, v): bit b set iff v is a neighbour of u in assembly b.
// rank_of(b, vertex) -> place of the vertex in assembly b; rec_at(b, place) -> record of that place in assembly b.
template <class RankOf, class RecAt>
GRK_HD uint32_t rank_support_mask(uint32_t n_asm, uint32_t u, uint32_t v, RankOf rank_of, RecAt rec_at)
{
    uint32_t m = 0;
    for (uint32_t b = 0; b < n_asm; ++b) {
        const uint32_t ru = rank_of(b, u), rv = rank_of(b, v);
        if (rank_adjacent(ru, rv) && rec_at(b, ru) == rec_at(b, rv)) m |= 1u << b;
    }
    return m;
}

// the pair is assembly a's edge iff a is its first supporter: the lowest set bit of the mask
GRK_HD bool rank_first_supporter(uint32_t mask, uint32_t a) { return mask != 0u && (uint32_t)__builtin_ctz(mask) == a; }

// The flag byte of item (a, r) whose pair has this mask: 0 = no edge of a's; up to eight assemblies the byte IS the mask, beyond
// that it only says "edge" and the mask is looked up again.
GRK_HD uint8_t rank_edge_flag(uint32_t mask, uint32_t a, uint32_t n_asm)
{
    if (!rank_first_supporter(mask, a)) return 0;
    return n_asm <= 8u ? (uint8_t)mask : (uint8_t)1;
}

}  // namespace mxg
