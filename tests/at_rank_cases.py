"""Inputs of the entries_at / search_at GPU tests (tests only, numpy only), kept apart from them so that
tests/test_index_at_rank.py can prove on the CPU that the inputs show what they are for: that the tie runs span the position
digit edges, that the hostile corpus holds NaN-, +-Inf- and -FLT_MAX-scoring rows, that the grid corpus puts adjacent floats,
+-0, +-Inf, -FLT_MAX and denormals into one ranking."""
import numpy as np

from haconvdr_amd import synth
from tests.test_index_rank_gpu import hostile_queries
from tests.test_index_rows_gpu import hostile_corpus
from tests.test_search_plans_gpu import _cuts

FMAX = np.finfo(np.float32).max

# ---- 1. every rank of a hostile corpus
HOSTILE_N, HOSTILE_DS, HOSTILE_NQS = 1000, (32, 96, 768), (1, 3, 17)
ROW_PINF, ROW_NINF, ROW_NFMAX = 20, 40, 60     # planted rows: their scores for query 2


def _nfmax_row(u):
    """A row whose k-ordered fmaf chain against u ends at exactly -FLT_MAX: components -FLT_MAX * sign(u_j) while the sum of
    |u_j| stays below 1 (the chain stays finite), then one component chosen so that the last step rounds to -FLT_MAX; the rest
    0.  The chain is emulated in float64 (the product of two floats is exact there) to choose among neighbouring floats; the
    CPU test checks the result against the oracle."""
    d = len(u)
    row = np.zeros(d, np.float32)
    t, A, J = np.float32(0), 0.0, 0
    while J < d and A + abs(float(u[J])) < 1.0:
        row[J] = -FMAX * np.sign(u[J])
        t = np.float32(np.float64(row[J]) * np.float64(u[J]) + np.float64(t))
        A += abs(float(u[J]))
        J += 1
    assert J < d and u[J] != 0, "the query's components do not sum to 1"
    c = np.float32((np.float64(FMAX) + np.float64(t)) / abs(np.float64(u[J])))
    for step in range(64):
        for cand in (c,) if step == 0 else (lo, hi):
            if np.isfinite(cand) and np.float32(np.float64(t) - np.float64(cand) * abs(np.float64(u[J]))) == -FMAX:
                row[J] = -cand * np.sign(u[J])
                return row
        lo, hi = (np.nextafter(c, np.float32(0)), np.nextafter(c, np.float32(np.inf))) if step == 0 else (
            np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(np.inf)))
    raise AssertionError("no component value rounds the chain to -FLT_MAX")


_HOSTILE = {}


def hostile_case(d):
    """(x [1000, d], q [17, d]): hostile_corpus (every tenth row raw words: NaN scores; denormals, -0.0, +-Inf words) with
    hostile_queries (query 0 all zero, query 3 = -query 2) and three planted rows following query 2: ROW_PINF / ROW_NINF
    (+-FLT_MAX in every component) score +Inf / -Inf for it, ROW_NFMAX exactly -FLT_MAX -- a real entry, not padding.  Built
    once per d; nobody writes to it."""
    if d not in _HOSTILE:
        x = hostile_corpus(0xD10 + d, HOSTILE_N, d)
        q = hostile_queries(0xD11 + d, max(HOSTILE_NQS), d)
        sign = np.where(q[2] >= 0, np.float32(1), np.float32(-1))
        x[ROW_PINF] = FMAX * sign
        x[ROW_NINF] = -FMAX * sign
        x[ROW_NFMAX] = _nfmax_row(q[2])
        x.setflags(write=False)
        q.setflags(write=False)
        _HOSTILE[d] = (x, q)
    return _HOSTILE[d]


def hostile_queries_of(q17, nq):
    """nq = 1: the all-zero query on its own; otherwise the first nq (zero query, the planted rows' query 2, the negated pair)"""
    return q17[:nq]


def all_ranks(nq, n):
    """ranks -2 .. n + 2 for every query: both ends of the list, every entry, the first padding slots"""
    return np.tile(np.arange(-2, n + 3, dtype=np.int64), (nq, 1))


# ---- 2. ties decided by position digits
TIE_D, TIE_N = 32, 66000
# 255 -> 256 crosses the first position byte (8-bit digits); 65 535 -> 65 536 changes bits 0 .. 16 (11-bit digits cut at 11 and 22:
# a digit edge of either width); then both ends of the list and the first padding slots
TIE_RANKS = (254, 255, 256, 257, 65534, 65535, 65536, 65537, 0, TIE_N - 1, TIE_N, -1)
RUN = 300                                         # rows per run of identical rows: no multiple of 64


def tie_zero_case():
    """(x [66000, 32] unit-ish rows, q [1, 32] all zero): every score is a +0 tie, the entry at rank t is row t -- the whole
    ranking is decided by position digits"""
    x = synth.embeddings(0xD20, TIE_N, TIE_D)
    return x, np.zeros((1, TIE_D), np.float32)


def tie_dup_case():
    """(x [66000, 32], q [2, 32]): 16 distinct grid-valued rows, row r = base[(r // 300) % 16] -- runs of 300 identical rows,
    which straddle the 64-row groups and the two segment edges of _index's three adds (_cuts: inside a run), the same row
    again every 4800 rows; integer queries: 16 distinct scores per query, each shared by ~4125 rows"""
    rng = np.random.default_rng(0xD21)
    base = (rng.integers(-8, 9, (16, TIE_D)) / 8.0).astype(np.float32)
    x = base[(np.arange(TIE_N) // RUN) % 16]
    q = rng.integers(-2, 3, (2, TIE_D)).astype(np.float32)
    return np.ascontiguousarray(x), q


def tie_dup_rows():
    """the rows whose entries the duplicate case asks for: both sides of each segment edge (inside a run of identical rows), of
    a 64-row group edge and of the position byte edges 256 and 65 536 inside runs"""
    c1, c2 = _cuts(TIE_N)
    edges = (c1, c2, 64 * 100, 256 * 7, 65536)
    for e in edges:
        assert e % RUN not in (0, 1, RUN - 1), e            # the rows e - 2 .. e + 1 lie in one run
    return np.array([e + o for e in edges for o in (-2, -1, 0, 1)], np.int64)


# ---- 3. score digit edges
GRID_D, GRID_N = 32, 300


def grid_values():
    """float32: runs of adjacent floats on the 1/8 grid (2^20 + k/8, ulp 1/8; 2^21 - 1/8 | 2^21: every lower score digit rolls
    over), +-0, +-Inf, +-FLT_MAX, the largest and the smallest denormal of either sign, a NaN"""
    v = [np.inf, FMAX, 2.0 ** 21, 2.0 ** 21 - 0.125] + [2.0 ** 20 + k / 8.0 for k in range(8)] + [0.125, 0.0, -0.0, -0.125]
    v += [-(2.0 ** 20 + k / 8.0) for k in range(8)] + [-(2.0 ** 21 - 0.125), -(2.0 ** 21), -FMAX, -np.inf, np.nan]
    v = np.array(v, np.float32)
    den = np.array([0x007FFFFF, 0x00000001, 0x80000001, 0x807FFFFF], np.uint32).view(np.float32)
    return np.concatenate([v, den])


def grid_case():
    """(x [300, 32], q [3, 32]): x[r, 0] = grid_values()[7 r mod 33] (7 and 33 coprime: every value in 9 or 10 scattered rows), the
    other components 0; queries e0, -e0 and all zero: the scores are the values themselves, their negation, and a +-0 tie (NaN
    where the value is +-Inf or NaN)"""
    v = grid_values()
    assert len(v) == 33
    x = np.zeros((GRID_N, GRID_D), np.float32)
    x[:, 0] = v[(7 * np.arange(GRID_N)) % len(v)]
    q = np.zeros((3, GRID_D), np.float32)
    q[0, 0], q[1, 0] = 1.0, -1.0
    return x, q


# ---- 7. search_at
AT_D, AT_N, AT_NQ = 96, 6000, 7
AT_KS = (1, 100, 2048)


def at_case():
    """(x [6000, 96], q [7, 96]) hostile rows and queries: every list ends before the rows do (NaN-scoring rows)"""
    return hostile_corpus(0xD70, AT_N, AT_D), hostile_queries(0xD71, AT_NQ, AT_D)


def at_starts(L):
    """one start per query: 0, 1, 2047, 3000, |L| - 1, |L|, |L| + 5 of the query's own list length L [7]"""
    L = np.asarray(L, np.int64)
    return np.array([0, 1, 2047, 3000, L[4] - 1, L[5], L[6] + 5], np.int64)
