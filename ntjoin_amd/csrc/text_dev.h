// text_dev.h -- text formed on the device: decimal digits, and the two sinks a formatter runs over.  A formatter written once
// against the sink interface (ch, lit, bytes, num) runs twice: over CountSink to learn its length, over WinSink to store the bytes
// that fall into the window at hand -- the two passes cannot disagree about a length.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mxg {

__device__ __forceinline__ uint32_t dec_digits(uint64_t v)
{
    uint32_t d = 1;
    while (v >= 10u) {
        v /= 10u;
        ++d;
    }
    return d;
}

struct CountSink {
    uint64_t n = 0;  // bytes so far
    __device__ __forceinline__ void ch(char) { ++n; }
    __device__ __forceinline__ void bytes(const char *, uint64_t len) { n += len; }
    __device__ __forceinline__ void lit(const char *, uint32_t len) { n += len; }
    __device__ __forceinline__ void num(uint64_t v) { n += dec_digits(v); }
};

struct WinSink {
    uint64_t pos, lo, hi;  // the next byte's offset in the file; the window
    char *out;             // the window's image
    __device__ __forceinline__ void put(uint64_t at, char c)
    {
        if (at >= lo && at < hi) out[at - lo] = c;
    }
    __device__ __forceinline__ void ch(char c) { put(pos++, c); }
    __device__ __forceinline__ void bytes(const char *src, uint64_t len)
    {
        const uint64_t a = max(pos, lo), b = min(pos + len, hi);  // (the part inside the window)
        for (uint64_t u = a; u < b; ++u) out[u - lo] = src[u - pos];
        pos += len;
    }
    __device__ __forceinline__ void lit(const char *s, uint32_t len) { bytes(s, len); }
    // from the last digit to the first, each through the window check (no buffer of digits: it may live in scratch)
    __device__ __forceinline__ void num(uint64_t v)
    {
        const uint32_t d = dec_digits(v);
        const uint64_t at = pos;
        for (uint32_t u = 0; u < d; ++u) {
            put(at + d - 1u - u, (char)('0' + (uint32_t)(v % 10u)));
            v /= 10u;
        }
        pos = at + d;
    }
};

}  // namespace mxg
