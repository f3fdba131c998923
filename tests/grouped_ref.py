"""The reference of every search_grouped assertion (tests only): include/haconvdr.h's grouped(q, g, k) restated over the CPU
oracle's canonical scores (rank_ref.canon_scores).  I and G are compared as integers, D by bits."""
import numpy as np

from tests import rank_ref

FMAX = np.finfo(np.float32).max
LABEL_END = 2 ** 32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def grouped_from_scores(S, group_of, k):
    """S float32 [nq, n] canonical scores, group_of int64 [n] -> (D float32 [nq, k], I int64 [nq, k], G int64 [nq, k]): per
    query the rows whose score is not NaN in the order (score desc, row asc), reduced to the first occurrence of every label
    and cut at k; padded with -FLT_MAX / -1 / -1.  A row whose label lies outside [0, 2^32) is in no list (the device form's
    rule; the host form refuses such labels)."""
    S = np.asarray(S, np.float32)
    nq, n = S.shape
    g = np.asarray(group_of, np.int64).reshape(n)
    legal = (g >= 0) & (g < LABEL_END)
    D = np.full((nq, k), -FMAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    G = np.full((nq, k), -1, np.int64)
    for i in range(nq):
        rows = np.flatnonzero(legal & ~np.isnan(S[i])).astype(np.int64)
        rows = rows[np.lexsort((rows, -S[i, rows].astype(np.float64)))]      # score desc, then row asc (float64 holds -FLT_MAX .. +-Inf exactly)
        first = np.sort(np.unique(g[rows], return_index=True)[1])            # the first occurrence of every label, in list order
        rows = rows[first][:k]
        D[i, :len(rows)], I[i, :len(rows)], G[i, :len(rows)] = S[i, rows], rows, g[rows]
    return D, I, G


def grouped(oracle, x, q, group_of, k):
    return grouped_from_scores(rank_ref.canon_scores(oracle, x, q), group_of, k)


def assert_same(got, want, what=""):
    """(D, I) or (D, I, G) against the reference's (D, I, G)"""
    gD, gI = np.asarray(got[0]), np.asarray(got[1])
    assert gD.dtype == np.float32 and gI.dtype == np.int64, (what, gD.dtype, gI.dtype)
    np.testing.assert_array_equal(gI, want[1], err_msg=f"{what}: I")
    np.testing.assert_array_equal(bits(gD), bits(want[0]), err_msg=f"{what}: D bits")
    if len(got) > 2:
        gG = np.asarray(got[2])
        assert gG.dtype == np.int64, (what, gG.dtype)
        np.testing.assert_array_equal(gG, want[2], err_msg=f"{what}: G")
