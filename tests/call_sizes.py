"""Inputs for the rank, count and range calls past one query chunk and one merge pair (tests only, numpy only): what
tests/test_index_call_sizes_gpu.py runs and tests/test_index_call_sizes.py proves to be what it is for.

1. seam(d, nq, oracle): nq in SEAM_NQ queries over 300 hostile rows.  rows_host.inc sends queries out in launches of
   QUERY_CHUNK and gives every launch offsets of its own into the caller's arrays; a wrong offset returns the plausible result
   of ANOTHER query, so every query i >= 1024 differs from queries i - 1024 and i - 2048 in its radius, its list, its ids,
   its reference scores and its ranks.  Special queries and radii stand on both sides of every seam (SPECIALS).
2. offsets_lengths(nq, N): list lengths that make range_offsets_kernel's 256 threads walk runs of ceil(nq / 256) queries.
3. merge_sets / tie_case: segments of 0 .. 4 merge passes in one call, and tie runs across sorted blocks and merge tiles.
Lengths are planted on _adversarial's corpus (scores strictly increase with the row) through the radius alone."""
import numpy as np

from haconvdr_amd import synth
from tests import range_ref, rank_ref
from tests.test_index_range_gpu import _score_at
from tests.test_index_rank_gpu import hostile_queries
from tests.test_index_rows_gpu import hostile_corpus
from tests.test_search_plans_gpu import _adversarial

QUERY_CHUNK = 1024              # DeviceIndex::QUERY_CHUNK of haconvdr_amd/csrc/flat_ip.hip
OFFSET_THREADS = 256            # RANGE_THREADS of csrc/range.inc: range_offsets_kernel's one workgroup
SORT_N = 4096                   # RANGE_SORT_N of csrc/range.inc (the GPU file reads it from the plan and compares)
FMAX = np.finfo(np.float32).max
INF = np.float32(np.inf)
NAN = np.float32(np.nan)

# ---------------------------------------------------------------------------------------------------------------------
# 1. the query-chunk seam
SEAM_N = 300
SEAM_NQ = (1024, 1025, 1041, 2049)
SEAM_D = (32, 96)
TIE_ROWS = (41, 120, 257)       # three identical rows: they tie for every query, the bound alone orders them
NAN_ROW = 3                     # hostile_corpus plants +-Inf and NaNs there: its score is NaN for every query
# query -> what stands there (positions at or behind nq do not exist).  The launches are [0, 1024), [1024, 2048), [2048, ..):
# 1024 and 2048 are the launches of ONE query (QT = 1) at nq = 1025 and 2049, so their lists are not empty.
SPECIALS = {
    1022: "radius +Inf: empty",
    1023: "a NaN query (one NaN component, radius -FLT_MAX): every score NaN, empty, every rank -1",
    1024: "the all-zero query, radius -Inf: every row that does not score NaN, one tie in row order",
    1025: "the negation of query 1026, radius = its best score: empty by strictness",
    1026: "radius NaN: empty",
    2047: "radius -Inf: every row that scores neither NaN nor -Inf",
    2048: "the negation of query 2047, radius at one of its scores",
}   # (no two of the empty ones are 1024 or 2048 apart: an empty list tells nothing about whose it is)
_SEAM = {}


def launches(nq):
    """[(first query, queries)] of the launches of a call of nq queries"""
    return [(off, min(QUERY_CHUNK, nq - off)) for off in range(0, nq, QUERY_CHUNK)]


def last_launch_plan(nq):
    """(QT, T) the plan text must show: the last launch's"""
    n = launches(nq)[-1][1]
    qt = min(16, n)
    return qt, (n + qt - 1) // qt


def rank_table(S):
    """T[i][r] = position of row r in the unbounded search of query i (score desc, row asc), -1 for a NaN score: by sorting,
    where rank_ref counts"""
    nq, n = S.shape
    T = np.full((nq, n), -1, np.int64)
    rows = np.arange(n)
    for i in range(nq):
        ok = rows[~np.isnan(S[i])]
        order = ok[np.lexsort((ok, -S[i][ok].astype(np.float64)))]
        T[i, order] = np.arange(len(order))
    return T


def _seam_ids(S, T, m, seed):
    """ids int64 [nq, m] drawn per query among the rows that do not score NaN, then in the second and third launch: -1 and the
    NaN row in chosen slots, the three tied rows wherever they fit, and -- last -- an id moved on wherever a query's ranks
    equal those of the query one or two launches before it."""
    nq, n = S.shape
    u = synth.uniform_u32(seed, nq * m).astype(np.int64).reshape(nq, m)
    ids = np.zeros((nq, m), np.int64)
    ok = [np.flatnonzero(~np.isnan(S[i])) for i in range(nq)]
    for i in range(nq):
        if len(ok[i]):
            ids[i] = ok[i][u[i] % len(ok[i])]
    fixed = np.zeros((nq, m), bool)
    for i in range(QUERY_CHUNK, nq):
        c = i % m
        if i % 5 == 0:
            ids[i, c], fixed[i, c] = -1, True
        elif i % 7 == 0:
            ids[i, c], fixed[i, c] = NAN_ROW, True
        elif i % 3 == 0 or i in SPECIALS:                  # (1024 and 2048 are multiples of neither 5 nor 7)
            for t, row in enumerate(TIE_ROWS[:m] if m > 1 else TIE_ROWS[1:2]):
                ids[i, (c + t) % m], fixed[i, (c + t) % m] = row, i in SPECIALS
    if nq > 2048 and m > len(TIE_ROWS) + 2:                # the third launch's one query: -1, the NaN row and the tie in one row
        for c, what in (((2048 + 3) % m, NAN_ROW), ((2048 + m - 1) % m, -1)):
            ids[2048, c], fixed[2048, c] = what, True

    def ranks(i):
        return np.where(ids[i] >= 0, T[i, np.clip(ids[i], 0, None)], -1)

    for i in range(QUERY_CHUNK, nq):
        free = np.flatnonzero(~fixed[i])
        for _ in range(n):
            if not any(np.array_equal(ranks(i), ranks(j)) for j in (i - QUERY_CHUNK, i - 2 * QUERY_CHUNK) if j >= 0):
                break
            if not len(free) or not len(ok[i]):
                break                                       # (nothing to move: test_index_call_sizes.py says whether it matters)
            c = free[0]
            ids[i, c] = ok[i][(np.searchsorted(ok[i], ids[i, c]) + 1) % len(ok[i])]
    return ids


def seam(d, nq, oracle):
    """The seam case of (d, nq), computed once and left unchanged: x [300, d], q [nq, d], S canonical scores, radius [nq],
    want = the range reference, table = rank_table(S), ids / ranks / own = {m: ...} for the m asked through seam_rank()."""
    key = (d, nq)
    if key in _SEAM:
        return _SEAM[key]
    seed = 0x7C0 + 16 * d + SEAM_NQ.index(nq)
    x = hostile_corpus(seed, SEAM_N, d)
    x[list(TIE_ROWS[1:])] = x[TIE_ROWS[0]]
    q = hostile_queries(seed + 2, nq, d)
    has = lambda i: i < nq
    q[0] = -q[1]                                           # (hostile_queries' zero query would share its scores with query 1024)
    if has(1023):
        q[1023:1024].view(np.uint32)[0, 7] = 0x7FC00001
    if has(1024):
        q[1024] = 0.0
    if has(1026):
        q[1025] = -q[1026]
    if has(2048):
        q[2048] = -q[2047]
    S = rank_ref.canon_scores(oracle, x, q)
    radius = np.zeros(nq, np.float32)
    for i in range(nq):
        radius[i] = -INF if np.isnan(S[i]).all() else _score_at(S[i], 5 + i % 41)
    for i, r in ((1022, INF), (1023, -FMAX), (1024, -INF), (1026, NAN), (2047, -INF)):
        if has(i):
            radius[i] = r
    if has(1026):
        radius[1025] = _score_at(S[1025], 0)
    case = {"d": d, "nq": nq, "x": x, "q": q, "S": S, "radius": radius, "want": range_ref.range_from_scores(S, radius),
            "table": rank_table(S), "ids": {}, "ranks": {}, "own": {}, "seed": seed}
    _SEAM[key] = case
    return case


def seam_rank(case, m):
    """(ids [nq, m], the ranks rank_ref gives them, the ids' own canonical scores: NaN where the id is -1)"""
    if m not in case["ids"]:
        ids = _seam_ids(case["S"], case["table"], m, case["seed"] + 5 + m)
        case["ids"][m] = ids
        case["ranks"][m] = rank_ref.rank_ids_from_scores(case["S"], ids)
        own = np.take_along_axis(case["S"], np.clip(ids, 0, None), 1)
        case["own"][m] = np.where(ids >= 0, own, NAN).astype(np.float32)
    return case["ids"][m], case["ranks"][m], case["own"][m]


def lists(want, i):
    """(D, I) of query i in a range reference"""
    lo, hi = want[0][i], want[0][i + 1]
    return want[1][lo:hi], want[2][lo:hi]


def moved_by_a_launch(case, by=QUERY_CHUNK):
    """What a launch that forgot its offset would return: queries `by`.. answered with the scores AND radii of queries 0.."""
    S, radius = case["S"].copy(), case["radius"].copy()
    S[by:], radius[by:] = case["S"][:len(S) - by], case["radius"][:len(S) - by]
    return range_ref.range_from_scores(S, radius)


def assert_scores(got, want, what=""):
    """score_ids against the oracle: the NaN mask, and every other word bit for bit (a NaN's payload is the hardware's)"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=what + ": NaN mask")
    np.testing.assert_array_equal(np.where(nan, np.uint32(0), got.view(np.uint32)), np.where(nan, np.uint32(0), want.view(np.uint32)), err_msg=what)


# ---------------------------------------------------------------------------------------------------------------------
# 2. and 3.: lengths planted on the adversarial corpus
def planted(d, n, nq, seed, oracle):
    """(x, q, S) of _adversarial: S[i] strictly increases with the row for every query"""
    x, q = _adversarial(d, n, nq, seed)
    return x, q, rank_ref.canon_scores(oracle, x, q)


def radii_for_lengths(S, lengths):
    """the radius that gives query i exactly lengths[i] rows: the score of the row at descending position lengths[i], +Inf
    for an empty list"""
    n = S.shape[1]
    lengths = np.asarray(lengths, np.int64)
    assert (lengths >= 0).all() and (lengths < n).all()
    r = S[np.arange(len(lengths)), n - 1 - lengths].astype(np.float32)
    r[lengths == 0] = INF
    return r


OFFSETS_NQ = (255, 256, 257, 511, 513, 1000)
OFFSETS_LAST_EMPTY = (256, 511, 1000)


def offsets_lengths(nq, N):
    """Planned list lengths for range_offsets_kernel at nq queries (N = RANGE_SORT_N).  per = ceil(nq / 256) queries per thread:
    threads 1, 2 and 5 (and every thread behind ceil(nq / per)) have an empty run; thread 7's run is empty but for its first and
    last query; thread 9's run starts with N and N + 1 keys (blk + 1, blk + 2), another N + 1, N pair straddles nq / 2."""
    per = -(-nq // OFFSET_THREADS)
    L = 1 + (np.arange(nq, dtype=np.int64) * 7) % 13
    for t in (1, 2, 5, 7):
        L[t * per:(t + 1) * per] = 0
    L[7 * per], L[8 * per - 1] = 3, 5
    L[9 * per], L[9 * per + 1] = N, N + 1
    L[nq // 2], L[nq // 2 + 1] = N + 1, N
    L[nq - 1] = 0 if nq in OFFSETS_LAST_EMPTY else 2
    return L


def runs(nq):
    """[(lo, hi)] the run of queries of each of range_offsets_kernel's threads"""
    per = -(-nq // OFFSET_THREADS)
    return [(min(nq, t * per), min(nq, t * per + per)) for t in range(OFFSET_THREADS)]


def merge_sets(N):
    """name -> (segment lengths of one call, extra room in the tensor form's cap)"""
    first = (4 * N + 1, 1, 2 * N, 0, 5 * N, N - 1)
    return {"0 to 3 passes side by side": (first, 0), "4 passes, 8N meets 1": ((8 * N + 1, 3 * N + 5), 0),
            "more passes than any segment needs": (first, 20 * N)}


def passes_of(keys, N):
    """merge passes that sort `keys` keys out of blocks of N: ceil(log2(ceil(keys / N)))"""
    return max(0, -(-keys // N) - 1).bit_length()


def tie_case(d, N, oracle):
    """16 distinct grid-valued rows interleaved over 5N + 70 rows, integer queries: every score is exact and shared by about
    N / 3 rows.  -> (x, q, S, radius): radii on shared score values, lists of about 4N + 1400, N + 1400 and 1400 rows and
    an empty one."""
    n, nq = 5 * N + 70, 4
    base = ((synth.uniform_u32(0x7E0, 16 * d) % np.uint32(17)).astype(np.float32).reshape(16, d) - 8.0) / 8.0
    x = base[np.arange(n) % 16]
    q = (synth.uniform_u32(0x7E1, nq * d) % np.uint32(9)).astype(np.float32).reshape(nq, d) - 4.0
    S = rank_ref.canon_scores(oracle, x, q)
    radius = np.array([_score_at(S[i], pos) for i, pos in enumerate((4 * N + 1400, N + 1400, 1400, 0))], np.float32)
    return x, q, S, radius


def workspace_case(d, N, oracle):
    """One corpus of 8N + 70 rows and 1025 queries for calls of very different (nq, cap) on one index: big = the deepest merge
    set on the first two queries, small = 1025 short lists (every 50th empty), ids [1025, 2] with their ranks."""
    nq, n = QUERY_CHUNK + 1, 8 * N + 70
    x, q, S = planted(d, n, nq, 0x7DC, oracle)
    big_r = radii_for_lengths(S[:2], merge_sets(N)["4 passes, 8N meets 1"][0])
    L = 5 + np.arange(nq, dtype=np.int64) % 41
    L[7::50] = 0
    small_r = radii_for_lengths(S, L)
    ids = (synth.uniform_u32(0x7DD, nq * 2) % np.uint32(n)).astype(np.int64).reshape(nq, 2)
    ids[QUERY_CHUNK, 1] = -1
    return {"x": x, "q": q, "n": n, "big_r": big_r, "big": range_ref.range_from_scores(S[:2], big_r), "small_r": small_r,
            "small": range_ref.range_from_scores(S, small_r), "L": L, "ids": ids, "ranks": rank_ref.rank_ids_from_scores(S, ids)}
