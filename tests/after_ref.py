"""The reference of every search_after assertion (tests only): include/haconvdr.h's after(q, s_ref, b, k) restated over the CPU
oracle's canonical scores (rank_ref.canon_scores).  I is compared as integers, D by bits."""
import numpy as np

from tests import rank_ref

FMAX = np.finfo(np.float32).max
START = -2                       # HAC_AFTER_START
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ordered(S_row):
    """the rows of one query whose score is not NaN, by (score desc, row asc)"""
    rows = np.flatnonzero(~np.isnan(S_row)).astype(np.int64)
    return rows[np.lexsort((rows, -S_row[rows].astype(np.float64)))]       # (float64 holds -FLT_MAX .. +-Inf exactly)


def _pad(S, lists, k):
    nq = len(lists)
    D = np.full((nq, k), -FMAX, np.float32)
    I = np.full((nq, k), -1, np.int64)
    for i, rows in enumerate(lists):
        rows = rows[:k]
        D[i, :len(rows)], I[i, :len(rows)] = S[i, rows], rows
    return D, I


def eligible(S_row, s_ref, b):
    """bool [n]: the rows behind the cursor (s_ref, b), by the definition's float comparisons"""
    s_ref, b = np.float32(s_ref) + np.float32(0.0), int(b)
    n = len(S_row)
    if b == START:
        return ~np.isnan(S_row)
    if b < 0 or np.isnan(s_ref):                                           # -1: an exhausted list; below -2: the device forms' empty list
        return np.zeros(n, np.bool_)
    with np.errstate(invalid="ignore"):
        return ~np.isnan(S_row) & ((S_row < s_ref) | ((S_row == s_ref) & (np.arange(n) > b)))


def after_from_scores(S, after_scores, after_rows, k):
    """S float32 [nq, n] canonical scores, cursors (after_scores float32 [nq], after_rows int64 [nq]) or (None, None) = every
    query from the start -> (D float32 [nq, k], I int64 [nq, k])."""
    S = np.asarray(S, np.float32)
    nq = len(S)
    if after_rows is None:
        after_scores, after_rows = np.zeros(nq, np.float32), np.full(nq, START, np.int64)
    lists = []
    for i in range(nq):
        order = _ordered(S[i])
        lists.append(order[eligible(S[i], after_scores[i], after_rows[i])[order]])
    return _pad(S, lists, k)


def pack(score, pos):
    """make_key on the host: float32 scores (not NaN), positions in [0, 2^32) -> uint64 keys"""
    s = (np.asarray(score, np.float32) + np.float32(0.0)).astype(np.float32)
    b = np.ascontiguousarray(s).view(np.uint32)
    o = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint64)
    return (o << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(pos).astype(np.uint64))


def cursor_keys(scores, rows, pos_base=0):
    """the rule of after_bounds_kernel, element by element in Python integers -> int64 view of the uint64 keys"""
    scores, rows = np.asarray(scores, np.float32), np.asarray(rows, np.int64)
    out = np.zeros(rows.shape, np.uint64)
    for at in np.ndindex(rows.shape):
        s, r = np.float32(scores[at]), int(rows[at])
        if r == START:
            out[at] = ALL_ONES
        elif r < 0 or np.isnan(s):
            out[at] = 0
        else:
            out[at] = (int(pack(s, 0).reshape(-1)[0]) >> 32 << 32) + (0xFFFFFFFF - min(r + pos_base, 0xFFFFFFFF))
    return out.view(np.int64)


def after_from_keys(S, after_keys, pos_base, k):
    """S float32 [nq, n], after_keys [nq] (int64 or uint64 view; None = the start) -> the uint64 KEYS [nq, k] (0 = padding) of
    the rows r with pack(S[i, r], pos_base + r) < after_keys[i], by key descending"""
    S = np.asarray(S, np.float32)
    nq, n = S.shape
    bound = np.full(nq, ALL_ONES) if after_keys is None else np.ascontiguousarray(after_keys).view(np.uint64)
    out = np.zeros((nq, k), np.uint64)
    for i in range(nq):
        rows = np.flatnonzero(~np.isnan(S[i]))
        keys = pack(S[i, rows], rows + pos_base)
        keys = np.sort(keys[keys < bound[i]])[::-1][:k]
        out[i, :len(keys)] = keys
    return out


def unpack(keys, pos_base=0):
    """uint64 keys -> (D float32, I int64 rows = position - pos_base; padding -FLT_MAX / -1)"""
    k = np.ascontiguousarray(keys).view(np.uint64)
    o = (k >> np.uint64(32)).astype(np.uint32)
    D = np.where(o & np.uint32(0x80000000), o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32).view(np.float32).copy()
    I = (np.uint64(0xFFFFFFFF) - (k & np.uint64(0xFFFFFFFF))).astype(np.int64) - pos_base
    D[k == 0], I[k == 0] = -FMAX, -1
    return D, I


def unbounded(S):
    """per query the whole list of an unbounded search: (scores float32 [m_i], rows int64 [m_i]) for every query"""
    S = np.asarray(S, np.float32)
    return [(S[i, o], o) for i, o in ((i, _ordered(S[i])) for i in range(len(S)))]


def after(oracle, x, q, after_scores, after_rows, k):
    return after_from_scores(rank_ref.canon_scores(oracle, x, q), after_scores, after_rows, k)


def assert_same(got, want, what=""):
    (gD, gI), (wD, wI) = got, want
    gD, gI = np.asarray(gD), np.asarray(gI)
    assert gD.dtype == np.float32 and gI.dtype == np.int64, (what, gD.dtype, gI.dtype)
    np.testing.assert_array_equal(gI, wI, err_msg=f"{what}: I")
    np.testing.assert_array_equal(bits(gD), bits(wD), err_msg=f"{what}: D bits")
