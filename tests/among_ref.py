"""The reference of every search_among assertion (tests only): include/haconvdr.h's among(q, c, k) restated over the CPU
oracle's canonical scores (rank_ref.canon_scores).  I is compared as integers, D by bits."""
import numpy as np

from tests import rank_ref

FMAX = np.finfo(np.float32).max


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def among_from_scores(S, cand, k):
    """S float32 [nq, n] canonical scores, cand int64 [nq, m] -> (D float32 [nq, k], I int64 [nq, k]): per query the first k of
    { r in set(cand[i]), 0 <= r < n, S[i, r] not NaN } by (score desc, row asc), padded with -FLT_MAX / -1."""
    S = np.asarray(S, np.float32)
    cand = np.asarray(cand, np.int64).reshape(S.shape[0], -1)
    nq, n = S.shape
    D = np.full((nq, k), -FMAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    for i in range(nq):
        rows = np.unique(cand[i][(cand[i] >= 0) & (cand[i] < n)])          # a set, ascending
        rows = rows[~np.isnan(S[i, rows])]
        order = np.lexsort((rows, -S[i, rows].astype(np.float64)))          # score desc, then row asc (float64 holds -FLT_MAX .. +-Inf exactly)
        rows = rows[order][:k]
        D[i, :len(rows)], I[i, :len(rows)] = S[i, rows], rows
    return D, I


def among(oracle, x, q, cand, k):
    return among_from_scores(rank_ref.canon_scores(oracle, x, q), cand, k)


def assert_same(got, want, what=""):
    (gD, gI), (wD, wI) = got, want
    gD, gI = np.asarray(gD), np.asarray(gI)
    assert gD.dtype == np.float32 and gI.dtype == np.int64, (what, gD.dtype, gI.dtype)
    np.testing.assert_array_equal(gI, wI, err_msg=f"{what}: I")
    np.testing.assert_array_equal(bits(gD), bits(wD), err_msg=f"{what}: D bits")
