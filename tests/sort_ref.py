"""Reference for the listing sort (include/s3imph.h section 5f), in pure Python and independent of
the code under test: Python compares ``bytes`` as unsigned bytes with a proper prefix first —
Go's string <, which sort.Slice in SortPrefixRows uses (pkg/extsort/types.go:160-164) — and
``sorted`` is stable."""
import numpy as np

NONE = (1 << 64) - 1


def sort_order(keys) -> np.ndarray:
    """order[j] = the input index of the j-th key in sorted order; equal keys in input order."""
    keys = [bytes(k) for k in keys]
    return np.array(sorted(range(len(keys)), key=lambda i: keys[i]), np.uint32)


def first_unsorted(keys) -> int:
    """Smallest i with keys[i] < keys[i - 1], or 2^64 - 1 for sorted input."""
    for i in range(1, len(keys)):
        if bytes(keys[i]) < bytes(keys[i - 1]):
            return i
    return NONE


def n_equal(keys) -> int:
    """Neighbours of the sorted order that hold equal keys."""
    s = sorted(bytes(k) for k in keys)
    return sum(1 for a, b in zip(s, s[1:]) if a == b)


def info(keys) -> dict:
    """What s3imph_sort_info must report, rounds apart (reported, not contractual)."""
    return {"n_objects": len(keys), "key_bytes": sum(len(k) for k in keys), "first_unsorted": first_unsorted(keys),
            "n_equal": n_equal(keys)}
