"""The reference of every rank assertion (tests only): include/haconvdr.h's count_ahead / rank_ids restated over the CPU
oracle's canonical scores.  Integer results, compared by equality."""
import numpy as np


def canon(scores):
    """make_key's "+ 0.0f": -0.0 -> +0.0, everything else unchanged."""
    return (np.asarray(scores, np.float32) + np.float32(0.0)).astype(np.float32)


def canon_scores(oracle, x, q):
    """S[i][r] = canonical score of (q[i], row r), float32 [nq, n]."""
    return canon(oracle.ip_scores(x, q))


def count_ahead_row(S_row, s_ref, bound):
    """count_ahead for one query: S_row float32 [n], s_ref float32 [m], bound int64 [m] -> int64 [m]."""
    S_row = np.asarray(S_row, np.float32)
    s_ref = canon(s_ref)
    bound = np.asarray(bound, np.int64)
    n = len(S_row)
    rows = np.arange(n, dtype=np.int64)
    ok = ~np.isnan(S_row)
    with np.errstate(invalid="ignore"):
        ahead = ok[None, :] & ((S_row[None, :] > s_ref[:, None]) | ((S_row[None, :] == s_ref[:, None]) & (rows[None, :] < bound[:, None])))
    out = ahead.sum(axis=1).astype(np.int64)
    out[np.isnan(s_ref) | (bound < 0)] = -1
    return out


def count_ahead(S, ref_scores, ref_bounds):
    """S float32 [nq, n] (canon_scores), ref_scores float32 [nq, m], ref_bounds int64 [nq, m] -> int64 [nq, m]."""
    ref_scores, ref_bounds = np.asarray(ref_scores, np.float32), np.asarray(ref_bounds, np.int64)
    return np.stack([count_ahead_row(S[i], ref_scores[i], ref_bounds[i]) for i in range(len(S))]).reshape(ref_bounds.shape)


def rank_ids_from_scores(S, ids):
    """rank_ids over precomputed canonical scores: ids int64 [nq, m], -1 for an id outside [0, n) and for a NaN-scored row."""
    ids = np.asarray(ids, np.int64)
    n = S.shape[1]
    inside = (ids >= 0) & (ids < n)
    own = np.take_along_axis(S, np.where(inside, ids, 0), 1) if n else np.zeros(ids.shape, np.float32)
    own = np.where(inside, own, np.float32(np.nan)).astype(np.float32)
    return count_ahead(S, own, np.where(inside, ids, -1))


def rank_ids(oracle, x, q, ids):
    return rank_ids_from_scores(canon_scores(oracle, x, q), ids)
