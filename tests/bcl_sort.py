"""Test-side restatement of ResultProcessor.ApplyBoosts / ApplySort (Scoring/ResultProcessor.cs:75-141, 180-201) for the boost / sort-by tests.

`introsort` is a Python port of ArraySortHelper<T>.IntrospectiveSort with a Comparison<T> (Array.Sort, unstable above 16 elements), written after
oracle/dotnet.hpp's IntroSorter; tests/test_bclsort_model.py holds it to the host build of the device's sort on random tie-heavy inputs."""
import math

import numpy as np


def introsort(a, cmp):
    """Sorts the list a in place as Array.Sort(a, cmp) does; cmp(x, y) -> int."""
    def swap_if_greater(i, j):
        if cmp(a[i], a[j]) > 0:
            a[i], a[j] = a[j], a[i]

    def insertion(lo, n):
        for i in range(n - 1):
            t = a[lo + i + 1]
            j = i
            while j >= 0 and cmp(t, a[lo + j]) < 0:
                a[lo + j + 1] = a[lo + j]
                j -= 1
            a[lo + j + 1] = t

    def down_heap(lo, i, n):
        d = a[lo + i - 1]
        while i <= n // 2:
            c = 2 * i
            if c < n and cmp(a[lo + c - 1], a[lo + c]) < 0:
                c += 1
            if not cmp(d, a[lo + c - 1]) < 0:
                break
            a[lo + i - 1] = a[lo + c - 1]
            i = c
        a[lo + i - 1] = d

    def heapsort(lo, n):
        for i in range(n // 2, 0, -1):
            down_heap(lo, i, n)
        for i in range(n, 1, -1):
            a[lo], a[lo + i - 1] = a[lo + i - 1], a[lo]
            down_heap(lo, 1, i - 1)

    def partition(lo, n):
        hi = n - 1
        mid = hi >> 1
        swap_if_greater(lo, lo + mid); swap_if_greater(lo, lo + hi); swap_if_greater(lo + mid, lo + hi)
        pivot = a[lo + mid]
        a[lo + mid], a[lo + hi - 1] = a[lo + hi - 1], a[lo + mid]
        left, right = 0, hi - 1
        while left < right:
            left += 1
            while cmp(a[lo + left], pivot) < 0:
                left += 1
            right -= 1
            while cmp(pivot, a[lo + right]) < 0:
                right -= 1
            if left >= right:
                break
            a[lo + left], a[lo + right] = a[lo + right], a[lo + left]
        if left != hi - 1:
            a[lo + left], a[lo + hi - 1] = a[lo + hi - 1], a[lo + left]
        return left

    def intro(lo, n, depth):
        while n > 1:
            if n <= 16:
                if n == 2:
                    swap_if_greater(lo, lo + 1)
                elif n == 3:
                    swap_if_greater(lo, lo + 1); swap_if_greater(lo, lo + 2); swap_if_greater(lo + 1, lo + 2)
                else:
                    insertion(lo, n)
                return
            if depth == 0:
                heapsort(lo, n)
                return
            depth -= 1
            p = partition(lo, n)
            intro(lo + p + 1, n - (p + 1), depth)
            n = p

    if len(a) >= 2:
        intro(0, len(a), 2 * (len(a).bit_length() - 1 + 1))
    return a


def cmp_float(x, y):
    """float.CompareTo: NaN lowest, NaN == NaN, -0 == +0."""
    if x < y:
        return -1
    if x > y:
        return 1
    if x == y:
        return 0
    return (0 if math.isnan(y) else -1) if math.isnan(x) else 1


def cmp_values(a, b):
    """ResultProcessor.CompareValues on sort keys that are None (null) or mutually comparable keys of one column."""
    if a is None:
        return 0 if b is None else -1
    if b is None:
        return 1
    return -1 if a < b else (1 if a > b else 0)


def apply_boosts(rows, boost_hits):
    """rows: [(key, score (fp32 value), tie)]; boost_hits[i]: [strength of every non-null boost whose filter row i's document satisfies].
    Score + totalBoost in fp32, then Array.Sort by score descending (always, once a non-null boost exists)."""
    out = []
    for (k, s, t), hits in zip(rows, boost_hits):
        tb = sum(hits)
        out.append((k, float(np.float32(s) + np.float32(tb)) if tb > 0 else s, t))       # fp32 add (numpy float32 arithmetic rounds once)
    return introsort(out, lambda a, b: cmp_float(b[1], a[1]))


def apply_sort(rows, sort_keys, ascending):
    """sort_keys[i]: the sort value of row i (None = null).  Array.Sort over (row, value) with CompareValues (ascending) or its mirror."""
    pairs = list(zip(rows, sort_keys))
    if ascending:
        introsort(pairs, lambda a, b: cmp_values(a[1], b[1]))
    else:
        introsort(pairs, lambda a, b: cmp_values(b[1], a[1]))
    return [r for r, _ in pairs]


def double_key(x):
    """double.CompareTo as a key: NaN lowest (all NaNs equal), -0 == +0."""
    return (0, 0.0) if math.isnan(x) else (1, x + 0.0)


def string_key(s):
    """The current-culture string comparer, read as OrdinalIgnoreCase then ordinal (PARITY UNPINNED; ASCII upper-casing suffices for the test data)."""
    up = "".join(c.upper() if "a" <= c <= "z" else c for c in s)
    return (up.encode("utf-16-be"), s.encode("utf-8"))
