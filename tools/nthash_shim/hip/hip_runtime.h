// Host stand-in for <hip/hip_runtime.h>, for tools/nthash_check.cpp only: what ntjoin_amd/csrc/nthash_dev.h needs to compile
// as plain C++ (tests/test_nthash_cpu.py copies that header beside this directory's files and compiles it unchanged).
#pragma once
#include <cstdint>

#define __device__
#define __forceinline__ inline
#ifndef __restrict__
#define __restrict__
#endif

struct uint4 {
    uint32_t x, y, z, w;
};
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
inline uint32_t min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// v_alignbit_b32: the low 32 bits of (hi:lo) >> (sh & 31)
inline uint32_t mxg_shim_alignbit(uint32_t hi, uint32_t lo, uint32_t sh)
{
    return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (sh & 31u));
}
#define __builtin_amdgcn_alignbit(hi, lo, sh) mxg_shim_alignbit(hi, lo, sh)
