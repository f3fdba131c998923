"""The inputs of tests/test_search_nonfinite_queries_gpu.py do what they are for -- proved on the CPU oracle alone
(oracle.ip_scores, oracle.flat_ip_search), at the shapes the GPU file uses -- and its comparison helper rejects references
altered in the ways a wrong kernel would alter a result."""
import numpy as np
import pytest

from tests import nonfinite, rank_ref
from tests.test_search_nonfinite_queries_gpu import assert_same_bits

FMAX = np.finfo(np.float32).max
N, K = 3001, 100
SHAPES = [(768, 17), (96, 17), (768, 64)]


def _case(kind, d, nq):
    return nonfinite.case(kind, d, N, nq, 0x4E00 + d + nq)


def test_positions():
    assert nonfinite.positions(1) == [0]
    assert nonfinite.positions(16) == [0, 15]
    assert nonfinite.positions(17) == [0, 15, 16]
    assert nonfinite.positions(40) == [0, 15, 16, 39]
    assert nonfinite.positions(64) == [0, 15, 16] + list(range(32, 48)) + [63]
    assert nonfinite.positions(1030, (1023, 1024)) == [0, 15, 16] + list(range(32, 48)) + [1023, 1024, 1029]


@pytest.mark.parametrize("kind", nonfinite.KINDS)
@pytest.mark.parametrize("d,nq", SHAPES)
def test_neighbours_are_untouched_gaussian_queries(d, nq, kind):
    x, q, pos, qb = _case(kind, d, nq)
    assert x.shape == (N, d) and N % 64 and q.shape == qb.shape == (nq, d) and x.dtype == q.dtype == np.float32
    keep = np.setdiff1d(np.arange(nq), pos)
    assert {1, 14} <= set(keep.tolist()) and (nq <= 17 or 17 in keep)
    np.testing.assert_array_equal(q[keep].view(np.uint32), qb[keep].view(np.uint32))
    assert np.isfinite(qb).all() and np.all(np.abs((qb * qb).sum(1) - d) < 1e-2 * d)      # row-standardised Gaussian vectors
    for i in pos:
        assert not np.array_equal(q[i].view(np.uint32), qb[i].view(np.uint32))
    # every planted query has an untouched neighbour in its own 16-query tile, or fills the tile (32 .. 47) between two that do
    for i in pos:
        tile = set(range(16 * (i // 16), min(nq, 16 * (i // 16) + 16)))
        assert (tile - set(pos)) or tile == set(range(32, 48)) or len(tile) == 1, i


@pytest.mark.parametrize("kind", nonfinite.NAN_KINDS)
@pytest.mark.parametrize("d,nq", SHAPES)
def test_nan_queries_score_nan_everywhere(d, nq, kind, oracle):
    x, q, pos, _ = _case(kind, d, nq)
    S = oracle.ip_scores(x, q)
    D, I = oracle.flat_ip_search(x, q, K)
    assert np.isnan(S[pos]).all() and np.all(D[pos] == -FMAX) and np.all(I[pos] == -1)
    keep = np.setdiff1d(np.arange(nq), pos)
    assert np.isfinite(S[keep]).all() and np.all(I[keep] >= 0)
    if kind == "nan_one":                     # planted by bit pattern: one NaN component, both sign bits
        words = q[pos].view(np.uint32)
        assert set(words[:, nonfinite.NAN_COMP].tolist()) == set(nonfinite.NAN_BITS[:max(1, min(2, len(pos)))])
        assert np.isnan(q[pos]).sum(1).tolist() == [1] * len(pos)


@pytest.mark.parametrize("kind", nonfinite.INF_KINDS)
@pytest.mark.parametrize("d,nq", SHAPES)
def test_inf_queries_tie_at_both_infinities_and_skip_the_nan_rows(d, nq, kind, oracle):
    x, q, pos, _ = _case(kind, d, nq)
    S = oracle.ip_scores(x, q)[pos]
    n_pos, n_neg, n_nan = (S == np.inf).sum(1), (S == -np.inf).sum(1), np.isnan(S).sum(1)
    assert np.all(n_pos >= K // 2) and np.all(n_neg >= K // 2) and np.all(n_nan >= 16), (n_pos, n_neg, n_nan)
    assert np.all(n_pos + n_neg + n_nan == N) and np.all(n_pos < K)        # a list of K crosses from the +Inf run into the -Inf run
    planted = np.arange(N) % 10 == 3
    assert np.isnan(S[:, planted]).all()      # Inf * 0
    # k beyond the +Inf run: the list goes on into the -Inf rows, both runs in row order, and holds no NaN-scored row
    k = int(n_pos.max()) + 40
    D, I = oracle.flat_ip_search(x, q[pos], k)
    for i in range(len(pos)):
        want = np.concatenate([np.flatnonzero(S[i] == np.inf), np.flatnonzero(S[i] == -np.inf)])[:k]
        assert len(want) == k
        np.testing.assert_array_equal(I[i], want)
        assert np.all(D[i, :n_pos[i]] == np.inf) and np.all(D[i, n_pos[i]:] == -np.inf)
        assert not np.isnan(S[i][I[i]]).any()


@pytest.mark.parametrize("d,nq", SHAPES)
def test_overflow_order_tells_the_ordered_chain_from_every_other_sum(d, nq, oracle):
    """The ordered chain overflows at k = 0 and stays +Inf (fmaf does not round its product: the finite -6e38.. of k = d-1
    cannot bring it back), where the float64 sum is finite and the reversed chain -Inf; on the cancelling rows it is exactly
    0: 1.5e38 absorbs every Gaussian product on the way."""
    x, q, pos, _ = _case("overflow_order", d, nq)
    S = oracle.ip_scores(x, q[pos])
    R = oracle.ip_scores(x[:, ::-1], q[pos][:, ::-1])                    # the same products, summed from k = d-1 down
    with np.errstate(all="ignore"):
        F = q[pos].astype(np.float64) @ x.astype(np.float64).T
    assert np.isfinite(F).all()
    ordered_only = ~np.isfinite(S) & np.isfinite(F)
    assert np.all(ordered_only.sum(1) >= N // 4)
    big = np.arange(N) % 4 != 3
    assert np.all(S[:, big] == np.inf) and np.all(R[:, big] == -np.inf)
    assert np.all(S[:, ~big] == 0.0)


@pytest.mark.parametrize("d,nq", SHAPES)
def test_near_max_scores_are_finite_and_infinite_among_the_top_k(d, nq, oracle):
    x, q, pos, _ = _case("near_max", d, nq)
    D, I = oracle.flat_ip_search(x, q[pos], K)
    S = oracle.ip_scores(x, q[pos])
    assert not np.isnan(S).any()
    for i in range(len(pos)):
        assert 0 < (D[i] == np.inf).sum() < K and np.isfinite(D[i]).sum() > 0
        assert np.all(D[i][np.isfinite(D[i])] > 0.9 * FMAX)
        # a few rows overflow in the LAST step only: without k = d-1 their chain is finite
        late = oracle.ip_scores(x[I[i][D[i] == np.inf]][:, :d - 32], q[pos[i]:pos[i] + 1, :d - 32])
        assert np.isfinite(late).all()


@pytest.mark.parametrize("d,nq", SHAPES)
def test_denormal_queries_score_subnormal(d, nq, oracle):
    x, q, pos, _ = _case("denormal", d, nq)
    assert np.all(np.abs(q[pos]) < nonfinite.TINY) and np.all((q[pos] != 0).mean(1) > 0.99)
    D, I = oracle.flat_ip_search(x, q[pos], K)
    sub = (np.abs(D) < nonfinite.TINY) & (D != 0)
    assert np.all(sub.sum(1) >= K // 2), sub.sum(1)
    assert np.all(I >= 0) and np.all(D[:, 0] > D[:, -1])


# ---------------------------------------------------------------------------------------------------------------------
def _rejects(D, I, oD, oI):
    for args in ((D, I, oD, oI), (oD, oI, D, I)):                        # as the reference, and as the result under test
        with pytest.raises(AssertionError):
            assert_same_bits(*args)


def test_assertions_reject_mutated_references(oracle):
    d, nq = 96, 17
    # the helper accepts the reference itself
    x, q, pos, _ = _case("inf_one", d, nq)
    D, I = oracle.flat_ip_search(x, q, K)
    assert_same_bits(D, I, D.copy(), I.copy())
    S = oracle.ip_scores(x, q)
    sp, healthy = pos[0], 1
    assert np.all(D[sp, :10] == np.inf) and D[sp, -1] == -np.inf and np.all(np.diff(I[sp, :10]) > 0)
    # a NaN-scored row admitted
    mD, mI = D.copy(), I.copy()
    nan_row = int(np.flatnonzero(np.isnan(S[sp]))[0])
    mD[sp, 5], mI[sp, 5] = np.nan, nan_row
    _rejects(D, I, mD, mI)
    mD[sp, 5] = np.inf                        # ... or under the score of its neighbours
    _rejects(D, I, mD, mI)
    # an Inf tie broken by row descending
    mD, mI = D.copy(), I.copy()
    mI[sp, :10] = mI[sp, :10][::-1]
    _rejects(D, I, mD, mI)
    # a healthy tile-mate's last entry dropped
    mD, mI = D.copy(), I.copy()
    mD[healthy, -1], mI[healthy, -1] = -FMAX, -1
    _rejects(D, I, mD, mI)
    # an overflow_order score replaced by the reordered sum
    x, q, pos, _ = _case("overflow_order", d, nq)
    D, I = oracle.flat_ip_search(x, q, K)
    sp = pos[0]
    R = oracle.ip_scores(x[:, ::-1], q[:, ::-1])
    mD = D.copy()
    mD[sp, 0] = R[sp, I[sp, 0]]
    assert D[sp, 0] == np.inf and mD[sp, 0] == -np.inf
    _rejects(D, I, mD, I)
    with np.errstate(all="ignore"):
        mD[sp, 0] = np.float32(q[sp].astype(np.float64) @ x[I[sp, 0]].astype(np.float64))
    assert np.isfinite(mD[sp, 0])
    _rejects(D, I, mD, I)
    # a denormal score flushed to 0
    x, q, pos, _ = _case("denormal", d, nq)
    D, I = oracle.flat_ip_search(x, q, K)
    sp = pos[0]
    mD = D.copy()
    assert 0 < abs(mD[sp, 3]) < nonfinite.TINY
    mD[sp, 3] = 0.0
    _rejects(D, I, mD, I)
    mD = np.where(np.abs(D) < nonfinite.TINY, np.float32(0.0), D)       # every subnormal flushed: the order is still "sorted"
    _rejects(D, I, mD, I)
    # the sign of a zero is the one thing the helper canonicalises: the reference's -0.0 is the result's +0.0
    assert_same_bits(np.zeros((1, 1), np.float32), np.zeros((1, 1), np.int64), -np.zeros((1, 1), np.float32), np.zeros((1, 1), np.int64))
    assert rank_ref.canon(np.float32(-0.0)).view(np.uint32) == 0
