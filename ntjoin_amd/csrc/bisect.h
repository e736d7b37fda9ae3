// bisect.h -- the two bisection loops of the project; every search over a sorted array or a monotone predicate, on the device
// and on the host, is one of them.  Includes nothing of the project; compiles for host and device and with a plain C++ compiler
// (tools/bisect_check.cpp).  Index types are unsigned; lo <= hi; both midpoints are lo + (hi - lo) / 2, which cannot wrap.
#pragma once

#if defined(__HIPCC__)
#define BIS_HD __host__ __device__ inline __attribute__((always_inline))  // (__forceinline__ spelled out: no HIP header needed)
#else
#define BIS_HD inline
#endif

namespace mxg {

// "the owner": pred is true, then false, over (lo, hi).  The last index where it holds; pred(lo) is taken for granted and never
// evaluated, so lo comes back when pred holds nowhere behind it and whenever hi <= lo + 1 (an empty range included).
template <class I, class P>
BIS_HD I last_where(I lo, I hi, P pred)
{
    while (hi - lo > 1) {
        const I mid = lo + ((hi - lo) >> 1);
        if (pred(mid)) lo = mid; else hi = mid;
    }
    return lo;
}

// "the first": pred is false, then true, over [lo, hi).  The first index where it holds; hi when it holds nowhere.
template <class I, class P>
BIS_HD I first_where(I lo, I hi, P pred)
{
    while (lo < hi) {
        const I mid = lo + ((hi - lo) >> 1);
        if (pred(mid)) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// the same over a rising array: the last i in [lo, hi) with arr[i] <= x (arr[lo] is not read), the first i in [lo, hi) with
// arr[i] >= x, and the first with arr[i] > x
template <class T, class I, class K>
BIS_HD I last_le(const T *arr, I lo, I hi, K x)
{
    return last_where(lo, hi, [&](I i) { return arr[i] <= x; });
}
template <class T, class I, class K>
BIS_HD I first_ge(const T *arr, I lo, I hi, K x)
{
    return first_where(lo, hi, [&](I i) { return arr[i] >= x; });
}
template <class T, class I, class K>
BIS_HD I first_gt(const T *arr, I lo, I hi, K x)
{
    return first_where(lo, hi, [&](I i) { return arr[i] > x; });
}

}  // namespace mxg
