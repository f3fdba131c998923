"""Test double (tests only) for the fourth hook of haconvdr_amd.sharded.ShardedSearcher, beside tests/doubles.py: a numpy
stand-in for the HIP filter kernel (hac_filter_keys_device), restating its contract from include/haconvdr.h."""
import numpy as np
import torch

CALLS = []          # (kin, e, k) of every call: the worker asserts that exclude=None never gets here


def filter(keys, exclude_pos, k):
    """keys int64(uint64 bits) [nq, kin], sorted lists, 0 = empty; exclude_pos int64 [nq, e] global positions, a value < 0 or
    > 0xFFFFFFFF is padding -> [nq, k]: per query the first k keys whose position is not excluded, in order, then 0."""
    a = keys.numpy().view(np.uint64)
    ex = np.asarray(exclude_pos.numpy(), np.int64)
    CALLS.append((a.shape[1], ex.shape[1], k))
    out = np.zeros((a.shape[0], k), np.uint64)
    for i in range(a.shape[0]):
        pos = (np.uint64(0xFFFFFFFF) - (a[i] & np.uint64(0xFFFFFFFF))).astype(np.int64)
        banned = ex[i][(ex[i] >= 0) & (ex[i] <= 0xFFFFFFFF)]
        kept = a[i][(a[i] != 0) & ~np.isin(pos, banned)][:k]
        out[i, :len(kept)] = kept
    return torch.from_numpy(out.view(np.int64))
