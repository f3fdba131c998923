"""The reference of every entries_at / search_at assertion (tests only): include/haconvdr.h's entry_at(q, t) restated over the
CPU oracle's canonical scores (rank_ref.canon_scores) -- the unbounded list of after_ref, indexed and padded.  I is compared as
integers, D by bits (after_ref.assert_same)."""
import numpy as np

from tests import after_ref, rank_ref

FMAX = after_ref.FMAX


def entries_at_from_scores(S, ranks):
    """S float32 [nq, n] canonical scores, ranks int64 [nq, m] (any values) -> (D float32 [nq, m], I int64 [nq, m]): the entry at
    each rank of the query's unbounded list, -FLT_MAX / -1 where the rank lies outside it"""
    ranks = np.asarray(ranks, np.int64)
    D = np.full(ranks.shape, -FMAX, np.float32)
    I = np.full(ranks.shape, -1, np.int64)
    for i, (scores, rows) in enumerate(after_ref.unbounded(S)):
        ok = (ranks[i] >= 0) & (ranks[i] < len(rows))
        at = ranks[i][ok]
        D[i, ok], I[i, ok] = scores[at], rows[at]
    return D, I


def entry_keys_from_scores(S, ranks, pos_base=0):
    """the keys form: uint64 [nq, m], after_ref.pack(score, pos_base + row) of every entry, 0 where the rank is outside the list"""
    D, I = entries_at_from_scores(S, ranks)
    keys = after_ref.pack(D, np.where(I >= 0, I + pos_base, 0))
    return np.where(I >= 0, keys, np.uint64(0)).astype(np.uint64)


def list_len(S):
    """|L(q)| of every query: the rows whose score is not NaN, int64 [nq]"""
    return (~np.isnan(np.asarray(S, np.float32))).sum(axis=1).astype(np.int64)


def search_at_from_scores(S, start, k):
    """the entries [start, start + k) of the unbounded search: start int64 [nq] >= 0 -> (D [nq, k], I [nq, k])"""
    start = np.asarray(start, np.int64)
    return entries_at_from_scores(S, start[:, None] + np.arange(k, dtype=np.int64)[None, :])


def passes(pos_base, ntotal, bits=8):
    """the documented number of passes over the rows of one tile of pairs: the 32 / bits score digits and the position digits in
    which two rows of the index can differ"""
    return 32 // bits + -(-int(pos_base ^ (pos_base + ntotal - 1)).bit_length() // bits)


def entries_at(oracle, x, q, ranks):
    return entries_at_from_scores(rank_ref.canon_scores(oracle, x, q), ranks)
