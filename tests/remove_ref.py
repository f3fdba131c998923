"""The reference of every remove_ids assertion (tests only): include/haconvdr.h's "removing rows" restated in numpy.
remove_ids(ids) is faiss's IndexFlat::remove_ids(IDSelectorBatch(ids)): the named rows go, the survivors keep their bits and
order and are renumbered densely from 0."""
import numpy as np


def removed_rows(ids):
    """the distinct rows a call names: sorted, -1 (padding) dropped"""
    ids = np.asarray(ids, np.int64).reshape(-1)
    return np.unique(ids[ids >= 0])


def removed(x, ids):
    """the rows (or any per-row array) that are left, in their order"""
    return np.delete(np.asarray(x), removed_rows(ids), axis=0)


def renumber(I, ids):
    """row numbers of the index before the call -> of the index after it: old - #removed below old; -1 stays -1.  (A removed row
    has no new number: the callers never pass one.)"""
    I = np.asarray(I, np.int64)
    return np.where(I < 0, -1, I - np.searchsorted(removed_rows(ids), I, side="left"))


def src_map(rem, new_rows):
    """compact_rows_kernel's source row of every destination row j < new_rows (csrc/remove.inc): src(j) = j + t, t the smallest
    index in [0, R] with rem[t] - t > j (R when there is none), found by the kernel's own binary search.  rem: sorted, no duplicates."""
    rem = np.asarray(rem, np.int64)
    R = len(rem)
    out = np.empty(new_rows, np.int64)
    for j in range(new_rows):
        lo, hi = 0, R
        while lo < hi:
            mid = lo + ((hi - lo) >> 1)
            if rem[mid] - mid > j:
                hi = mid
            else:
                lo = mid + 1
        out[j] = j + lo
    return out
