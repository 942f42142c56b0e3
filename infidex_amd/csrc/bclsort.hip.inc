// ArraySortHelper<T>.IntrospectiveSort with a Comparison<T> (the .NET 8 BCL's Array.Sort(T[], Comparison<T>)), as ResultProcessor.ApplyBoosts /
// ApplySort call it (Scoring/ResultProcessor.cs:116, 135-138).  The sort is unstable: above 16 elements it reorders elements that compare equal, so the
// rows a query returns depend on this exact sequence of compares and swaps, not only on the key.  Restated from the published dotnet/runtime sources
// like BclSort in csrc/host/query.h (PARITY UNPINNED: the BCL is not in the reference's sources).
//
// Plain C++ behind BCL_FN: compiled into k_postproc (postproc.hip.inc) and, unchanged, into a host model that checks it against the oracle's restatement
// (tests/models/bclsort_model.cpp, tests/test_bclsort_model.py).  The sequence is reached through an accessor S, so the device can keep it in lanes:
//   int  S::get(int i) / void S::set(int i, int v)     element i of the sequence (elements are ints: row indices)
//   int  S::cmp(int a, int b)                           the Comparison: < 0, 0, > 0
//   int  S::fget(int i) / void S::fset(int i, int v)    slot i of the pending-range stack (BCL_MAX_FRAMES slots)
// The recursion of IntroSort becomes that explicit stack.  Pending ranges are disjoint, so the order they are sorted in does not change the result;
// the depths on the stack strictly decrease from bottom to top, so it never holds more than depthLimit + 1 = 2 * (log2 n + 1) + 1 ranges (15 for n <= 64).
// Two entry points over the same sequence: bcl_introsort for n <= BCL_MAX_N (k_postproc: frames in lanes, 10-bit length) and bcl_introsort_wide for
// n <= BCL_WIDE_MAX_N (k_postproc_wide: frames in LDS, 11-bit length, 23 of BCL_WIDE_MAX_FRAMES slots at n = 1024).
#pragma once
#ifndef BCL_FN
#define BCL_FN __device__ __forceinline__
#endif
#ifndef BCL_BRANCH
#define BCL_BRANCH(which)          // host model: counts the insertion (0), partition (1) and heapsort (2) branches
#endif
#define BCL_MAX_N 64               // sequences of at most 64 elements (a frame packs lo / length / depth into 10 bits each)
#define BCL_MAX_FRAMES 16
#define BCL_WIDE_MAX_N 1024         // the wide entry point: lo in 10 bits, length in 11, depth (<= 22) above them
#define BCL_WIDE_MAX_FRAMES 24
#define BCL_SMALL 16               // IntrosortSizeThreshold

// float.CompareTo(float): NaN is less than every number and equal to NaN; -0 == +0
BCL_FN int bcl_cmp_float(float a, float b) {
    if (a < b) return -1;
    if (a > b) return 1;
    if (a == b) return 0;
    const bool na = a != a, nb = b != b;
    return na ? (nb ? 0 : -1) : 1;
}
BCL_FN int bcl_cmp_u32(uint32_t a, uint32_t b) { return a < b ? -1 : (a > b ? 1 : 0); }

template <class S> BCL_FN void bcl_swap(S& s, int i, int j) { const int a = s.get(i), b = s.get(j); s.set(i, b); s.set(j, a); }
template <class S> BCL_FN void bcl_swap_if_greater(S& s, int i, int j) { if (s.cmp(s.get(i), s.get(j)) > 0) bcl_swap(s, i, j); }

template <class S> BCL_FN void bcl_insertion(S& s, int lo, int n) {
    for (int i = 0; i < n - 1; i++) {
        const int t = s.get(lo + i + 1);
        int j = i;
        while (j >= 0 && s.cmp(t, s.get(lo + j)) < 0) { s.set(lo + j + 1, s.get(lo + j)); j--; }
        s.set(lo + j + 1, t);
    }
}
template <class S> BCL_FN void bcl_down_heap(S& s, int lo, int i, int n) {
    const int d = s.get(lo + i - 1);
    while (i <= n / 2) {
        int c = 2 * i;
        if (c < n && s.cmp(s.get(lo + c - 1), s.get(lo + c)) < 0) c++;
        if (!(s.cmp(d, s.get(lo + c - 1)) < 0)) break;
        s.set(lo + i - 1, s.get(lo + c - 1));
        i = c;
    }
    s.set(lo + i - 1, d);
}
template <class S> BCL_FN void bcl_heapsort(S& s, int lo, int n) {
    for (int i = n / 2; i >= 1; i--) bcl_down_heap(s, lo, i, n);
    for (int i = n; i > 1; i--) { bcl_swap(s, lo, lo + i - 1); bcl_down_heap(s, lo, 1, i - 1); }
}
// PickPivotAndPartition.  The scans stop at the pivot parked at hi - 1 and at element 0 (<= pivot after the median of three) for any consistent
// comparison; the explicit bounds only keep an inconsistent one inside the range and never change the result of a consistent one.
template <class S> BCL_FN int bcl_partition(S& s, int lo, int n) {
    const int hi = n - 1, mid = hi >> 1;
    bcl_swap_if_greater(s, lo, lo + mid); bcl_swap_if_greater(s, lo, lo + hi); bcl_swap_if_greater(s, lo + mid, lo + hi);
    const int pivot = s.get(lo + mid);
    bcl_swap(s, lo + mid, lo + hi - 1);
    int l = 0, r = hi - 1;
    while (l < r) {
        while (l < hi - 1 && s.cmp(s.get(lo + ++l), pivot) < 0) {}
        while (r > 0 && s.cmp(pivot, s.get(lo + --r)) < 0) {}
        if (l >= r) break;
        bcl_swap(s, lo + l, lo + r);
    }
    if (l != hi - 1) bcl_swap(s, lo + l, lo + hi - 1);
    return l;
}
// Array.Sort(keys[0..n), comparison); a frame packs lo (10 bits) / length (NBITS bits) / depth, the stack holds MAXF frames
template <class S, int NBITS, int MAXF> BCL_FN void bcl_introsort_frames(S& s, int n) {
    if (n < 2) return;
    int lg = 0;
    for (unsigned x = (unsigned)n; x >>= 1;) lg++;
    int sp = 0;
    s.fset(sp++, 0 | (n << 10) | ((2 * (lg + 1)) << (10 + NBITS)));
    while (sp > 0) {
        const int f = s.fget(--sp);
        const int lo = f & 1023;
        int part = (f >> 10) & ((1 << NBITS) - 1), depth = f >> (10 + NBITS);
        while (part > 1) {
            if (part <= BCL_SMALL) {
                BCL_BRANCH(0);
                if (part == 2) bcl_swap_if_greater(s, lo, lo + 1);
                else if (part == 3) { bcl_swap_if_greater(s, lo, lo + 1); bcl_swap_if_greater(s, lo, lo + 2); bcl_swap_if_greater(s, lo + 1, lo + 2); }
                else bcl_insertion(s, lo, part);
                break;
            }
            if (depth == 0) { BCL_BRANCH(2); bcl_heapsort(s, lo, part); break; }
            depth--;
            BCL_BRANCH(1);
            const int p = bcl_partition(s, lo, part);
            if (part - (p + 1) > 1 && sp < MAXF) s.fset(sp++, (lo + p + 1) | ((part - (p + 1)) << 10) | (depth << (10 + NBITS)));     // IntroSort(keys[(p+1)..part), depth)
            part = p;
        }
    }
}
// n <= BCL_MAX_N
template <class S> BCL_FN void bcl_introsort(S& s, int n) { bcl_introsort_frames<S, 10, BCL_MAX_FRAMES>(s, n); }
// n <= BCL_WIDE_MAX_N
template <class S> BCL_FN void bcl_introsort_wide(S& s, int n) { bcl_introsort_frames<S, 11, BCL_WIDE_MAX_FRAMES>(s, n); }
