"""The reference of every range-search assertion (tests only): include/haconvdr.h's range(q, r) restated over the CPU
oracle's canonical scores.  lims and I are integers, D is compared by its bits."""
import numpy as np

from tests import rank_ref


def range_from_scores(S, radius):
    """S float32 [nq, n] (rank_ref.canon_scores), radius float32 [nq] (or a scalar) -> (lims int64 [nq + 1], D float32 [total],
    I int64 [total]): per query the rows with S > r and S not NaN, ordered by (-S, row)."""
    S = np.asarray(S, np.float32)
    nq = S.shape[0]
    radius = np.broadcast_to(np.asarray(radius, np.float32), (nq,))
    lims = np.zeros(nq + 1, np.int64)
    Ds, Is = [], []
    for i in range(nq):
        with np.errstate(invalid="ignore"):
            rows = np.flatnonzero(~np.isnan(S[i]) & (S[i] > radius[i])).astype(np.int64)
        rows = rows[np.lexsort((rows, -S[i][rows].astype(np.float64)))]         # (score desc, row asc); float64 negation is exact
        Ds.append(S[i][rows])
        Is.append(rows)
        lims[i + 1] = lims[i] + len(rows)
    return lims, np.concatenate(Ds).astype(np.float32) if Ds else np.zeros(0, np.float32), np.concatenate(Is) if Is else np.zeros(0, np.int64)


def range_search(oracle, x, q, radius):
    return range_from_scores(rank_ref.canon_scores(oracle, x, q), radius)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(got, want, what=""):
    """(lims, D, I) against the reference: lims and I equal, D equal bit for bit"""
    np.testing.assert_array_equal(got[0], want[0], err_msg=what + ": lims")
    np.testing.assert_array_equal(got[2], want[2], err_msg=what + ": I")
    np.testing.assert_array_equal(bits(got[1]), bits(want[1]), err_msg=what + ": bits of D")
