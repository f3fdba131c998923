"""The reference of every search_masked assertion (tests only): include/haconvdr.h's masked(q, M, k) restated over the CPU
oracle's canonical scores (rank_ref.canon_scores).  I is compared as integers, D by bits."""
import numpy as np

from tests import rank_ref

FMAX = np.finfo(np.float32).max


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def resolve_mask_of(n_masks, nq, mask_of):
    """the mask of each query, int64 [nq]: mask_of, or (None) mask 0 with one mask and mask i with nq masks"""
    if mask_of is not None:
        return np.asarray(mask_of, np.int64).reshape(nq)
    assert n_masks in (1, nq), (n_masks, nq)
    return np.zeros(nq, np.int64) if n_masks == 1 else np.arange(nq, dtype=np.int64)


def masked_from_scores(S, masks, mask_of, k):
    """S float32 [nq, n] canonical scores, masks bool [n] or [n_masks, n], mask_of int64 [nq] or None -> (D float32 [nq, k],
    I int64 [nq, k]): per query the first k of { r : masks[mask_of[i], r], S[i, r] not NaN } by (score desc, row asc), padded
    with -FLT_MAX / -1.  A mask_of entry outside [0, n_masks) selects nothing (the device forms' rule)."""
    S = np.asarray(S, np.float32)
    nq, n = S.shape
    masks = np.asarray(masks, np.bool_).reshape(-1, n)
    mo = resolve_mask_of(len(masks), nq, mask_of)
    D = np.full((nq, k), -FMAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    for i in range(nq):
        if not 0 <= mo[i] < len(masks):
            continue
        rows = np.flatnonzero(masks[mo[i]] & ~np.isnan(S[i])).astype(np.int64)
        order = np.lexsort((rows, -S[i, rows].astype(np.float64)))          # score desc, then row asc (float64 holds -FLT_MAX .. +-Inf exactly)
        rows = rows[order][:k]
        D[i, :len(rows)], I[i, :len(rows)] = S[i, rows], rows
    return D, I


def masked(oracle, x, q, masks, mask_of, k):
    return masked_from_scores(rank_ref.canon_scores(oracle, x, q), masks, mask_of, k)


def assert_same(got, want, what=""):
    (gD, gI), (wD, wI) = got, want
    gD, gI = np.asarray(gD), np.asarray(gI)
    assert gD.dtype == np.float32 and gI.dtype == np.int64, (what, gD.dtype, gI.dtype)
    np.testing.assert_array_equal(gI, wI, err_msg=f"{what}: I")
    np.testing.assert_array_equal(bits(gD), bits(wD), err_msg=f"{what}: D bits")
