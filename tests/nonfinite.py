"""Hostile QUERIES for the search routes (tests only, numpy only): Gaussian batches (cases.search_case_inputs) with special
queries planted where the kernels' tiles meet, and the corpus each kind needs to show what it is for.

Where: index 0, the last query of the first 16-query tile (15), the first of the second tile (16), the last query, and for
nq >= 48 the whole tile 32 .. 47 -- every planted query shares a scan16 tile, a scanq NQ tile and a 1024-query chunk with
untouched Gaussian neighbours.  queries() returns the positions; base() is the same batch before the planting, i.e. the
batch "with the special queries replaced by Gaussian ones".

The kinds, and the canonical score (k-ordered fp32 fmaf chain) each gives against rows(kind, ...):
  nan_all         every component NaN: every score NaN, the list is all padding.
  nan_one         ONE NaN component (NAN_COMP), planted by bit pattern, both sign bits (0x7FC00001 / 0xFFC00000 in turn):
                  every score NaN.
  inf_one         +Inf in component INF_A.  Rows hold exact 0.0 there in a planted tenth (Inf * 0 = NaN), a positive value in
                  every 47th row and a negative one elsewhere: a list of k = 100 is the +Inf ties in row order (between k / 2
                  and k of them at n = 3001 and 4000), then -Inf ties in row order, the NaN rows never.
  inf_pair        +Inf in INF_A and -Inf in comp_b(d): +Inf where x[a] > 0 > x[b] (every 47th row), -Inf where x[a] < 0 < x[b],
                  NaN where either is 0 (the planted tenth, Inf * 0) or both are positive (every 7th row, Inf - Inf).
  overflow_order  q[0] = 3e38, q[d-1] = -3e38, the rest Gaussian.  Three rows of four have x[0], x[d-1] >= 2: the chain
                  overflows to +Inf at k = 0 and STAYS there -- fmaf does not round the product, so the finite -6e38.. of
                  k = d-1 cannot undo it -- while the sum in any order that does not begin with k = 0 (or in float64) is
                  finite, -Inf or NaN.  Every fourth row has x[0] = x[d-1] = 0.5: the accumulator sits at 1.5e38, absorbs
                  every Gaussian product on the way and ends at exactly 0 -- a run of ties behind the +Inf run; a sum that
                  keeps the two large terms in different accumulators returns the Gaussian part instead.
  near_max        q[0] = 1e38, q[d-1] = 1e37 against rows with x[0] in [1, 3.4): finite scores between 1e38 and FLT_MAX =
                  3.4028e38, and a few rows whose chain overflows in its LAST step only.
  denormal        a Gaussian query times 1e-39 (every component subnormal) against Gaussian rows / 16: every product and
                  every score is subnormal or zero; a kernel that flushes denormals returns zeros.
Row counts are never a multiple of 64."""
import numpy as np

from haconvdr_amd import synth
from tests.golden import cases

KINDS = ("nan_all", "nan_one", "inf_one", "inf_pair", "overflow_order", "near_max", "denormal")
NAN_KINDS = ("nan_all", "nan_one")
INF_KINDS = ("inf_one", "inf_pair")
NAN_BITS = (0x7FC00001, 0xFFC00000)          # a positive quiet NaN with a payload, the negative default NaN
NAN_COMP = 7
INF_A = 5
FMAX = np.finfo(np.float32).max
TINY = np.finfo(np.float32).tiny             # the smallest normal number


def comp_b(d):
    return d - 3


def positions(nq, extra=()):
    """The planted positions of a batch of nq queries, ascending (extra: more of them, e.g. a chunk edge)."""
    pos = {0, 15, 16, nq - 1} | set(int(p) for p in extra)
    if nq >= 48:
        pos |= set(range(32, 48))
    return sorted(p for p in pos if 0 <= p < nq)


def base(d, nq, seed):
    """The Gaussian batch the special queries are planted into."""
    return cases.search_case_inputs("gauss", seed, 1, nq, d=d)[1]


def _plant(kind, q, i, nth):
    d = q.shape[1]
    if kind == "nan_all":
        q[i, :] = np.nan
    elif kind == "nan_one":
        q[i:i + 1].view(np.uint32)[0, NAN_COMP] = NAN_BITS[nth % 2]
    elif kind == "inf_one":
        q[i, INF_A] = np.inf
    elif kind == "inf_pair":
        q[i, INF_A] = np.inf
        q[i, comp_b(d)] = -np.inf
    elif kind == "overflow_order":
        q[i, 0] = 3e38
        q[i, d - 1] = -3e38
    elif kind == "near_max":
        q[i, 0] = 1e38
        q[i, d - 1] = 1e37
    elif kind == "denormal":
        q[i] = q[i] * np.float32(1e-39)
    else:
        raise ValueError(kind)


def queries(kind, d, nq, seed, extra=()):
    """-> (q float32 [nq, d], planted positions): base(d, nq, seed) with a query of `kind` at every position."""
    q = base(d, nq, seed).copy()
    pos = positions(nq, extra)
    with np.errstate(all="ignore"):
        for nth, i in enumerate(pos):
            _plant(kind, q, i, nth)
    return q, pos


def _inf_columns(kind, x):
    n, d = x.shape
    r = np.arange(n)
    zero, up = r % 10 == 3, r % 47 == 5       # a tenth of the rows: Inf * 0 = NaN; every 47th: the +Inf run, shorter than k = 100
    mag = np.abs(x[:, [INF_A, comp_b(d)]]) + np.float32(0.125)
    a = np.where(up, mag[:, 0], -mag[:, 0])
    if kind == "inf_pair":
        both = r % 7 == 2                     # +Inf and -Inf meet in one chain: NaN
        a = np.where(both, mag[:, 0], a)
        x[:, comp_b(d)] = np.where(zero, 0.0, np.where(up & ~both, -mag[:, 1], mag[:, 1]))
    x[:, INF_A] = np.where(zero, 0.0, a)


def rows(kind, d, n, seed):
    """The corpus of `kind`: Gaussian, float32 [n, d], with the columns the kind's special components meet prepared."""
    assert n % 64, "row counts are never a multiple of 64"
    x = cases.search_case_inputs("gauss", seed + 3, n, 1, d=d)[0]
    r = np.arange(n)
    if kind in INF_KINDS:
        _inf_columns(kind, x)
    elif kind == "overflow_order":
        cancel = r % 4 == 3
        for c in (0, d - 1):
            x[:, c] = np.where(cancel, np.float32(0.5), np.float32(2.0) + np.abs(x[:, c]))
    elif kind == "near_max":
        u = synth.uniform_u32(seed + 7, n).astype(np.float64) / 2.0 ** 32
        x[:, 0] = (1.0 + 2.4 * u).astype(np.float32)
    elif kind == "denormal":
        x = x * np.float32(1.0 / 16.0)
    return np.ascontiguousarray(x, np.float32)


def case(kind, d, n, nq, seed, extra=()):
    """-> (x, q, planted positions, base batch)."""
    q, pos = queries(kind, d, nq, seed, extra)
    return rows(kind, d, n, seed), q, pos, base(d, nq, seed)
