"""Inputs of the search_after GPU tests (tests only, numpy only), kept apart from them so that tests/test_index_after.py can
prove on the CPU that the inputs show what they are for: that the tie corpus puts page boundaries inside runs of equal scores,
that the hostile corpus has NaN-scoring and -Inf-scoring rows, that per-query depths give every query of a tile its own bound."""
import numpy as np

from tests import masked_cases
from tests.test_index_among_gpu import _tie_corpus
from tests.test_index_rank_gpu import hostile_queries
from tests.test_index_rows_gpu import hostile_corpus

D, N, NQ = masked_cases.D, masked_cases.N, masked_cases.NQ   # 96 x 5000 (79 groups, the last of 8 rows), 37 queries
K_MAX = 2048
START_KS, START_NQS = (1, 10, 100, 2047, 2048), (1, 16, 17, 37)
CURSOR_JS, CURSOR_KS = (0, 1, 99, 2046, 2047), (1, 100, 2048)
PAGE_KS = (1000, 2048)
TIE_D, TIE_N, TIE_NQ, TIE_SEED = 96, 1000, 6, 0xC62
TIE_PAGE_KS = (7, 100)
HOSTILE_D, HOSTILE_N, HOSTILE_NQ = 96, 5000, 6
FMAX = np.finfo(np.float32).max


def base_case():
    """masked_cases' shared case: (x float32 [N, D], q float32 [NQ, D]) Gaussian"""
    return masked_cases.base_case()


def per_query_depths(nq=NQ):
    """int64 [nq]: the position j of each query's cursor in its own search(q, 2048) list -- all different inside every tile of
    16 (and of 4), from the first entry to the last"""
    j = (np.arange(nq) * 131 + 7) % K_MAX
    j[0], j[nq - 1] = 0, K_MAX - 1
    return j.astype(np.int64)


def tie_case():
    """(x [1000, 96], q [6, 96]): 16 distinct grid-valued rows repeated, integer queries, query 0 all zero -- at most 16 distinct
    scores per query, each shared by 62 or 63 rows"""
    return _tie_corpus(TIE_D, TIE_N, TIE_NQ, TIE_SEED)


def hostile_case():
    """(x [5000, 96], q [6, 96]): hostile_corpus (every tenth row raw words: NaN scores, and now and then a sum that overflows
    to +-Inf; denormals, -0.0, +-Inf words) with four planted rows of +-FLT_MAX whose signs follow query 2: they score +Inf
    (rows 20, 21) and -Inf (rows 40, 4001) for query 2 and the opposite for query 3 = -query 2, whatever the raw words do;
    query 0 is all zero (every score a +-0 tie, or NaN)"""
    x = hostile_corpus(0xC70, HOSTILE_N, HOSTILE_D)
    q = hostile_queries(0xC71, HOSTILE_NQ, HOSTILE_D)
    sign = np.where(q[2] >= 0, np.float32(1), np.float32(-1))
    x[20] = x[21] = FMAX * sign
    x[40] = x[4001] = -FMAX * sign
    return x, q
