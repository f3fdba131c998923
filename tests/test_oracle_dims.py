"""The CPU oracle at d % 64 == 32, before the GPU is compared with it (tests/test_search_plans_gpu.py).  With "grid"
inputs (multiples of 1/8 in [-2, 2]) every partial sum is exact in fp32, so the k-ordered fmaf chain must equal a float64
matrix product exactly, and the ranking must be the stable (score desc, row asc) order of those products.  CPU only."""
import numpy as np
import pytest

from tests.golden import cases


@pytest.mark.parametrize("d", [32, 96, 992])
def test_oracle_is_exact_on_grid_inputs_at_other_dimensions(d, oracle):
    n, nq, k = 777, 9, 120
    x, q, _ = cases.search_case_inputs("grid", 4000 + d, n, nq, d=d)
    ref = q.astype(np.float64) @ x.astype(np.float64).T
    # |partial sums| <= 4 * d in units of 1/64: below 2^24 units, hence exact in fp32 (and in float64)
    assert 4 * d * 64 < 2 ** 24 and np.all(ref * 64 == np.round(ref * 64))
    s = oracle.ip_scores(x, q)
    assert s.dtype == np.float32
    np.testing.assert_array_equal(s.astype(np.float64), ref)
    for kk in (1, k, n, n + 5):
        D, I = oracle.flat_ip_search(x, q, kk)
        m = min(kk, n)
        for i in range(nq):
            order = np.lexsort((np.arange(n), -ref[i]))[:m]           # score desc, row asc; stable
            np.testing.assert_array_equal(I[i, :m], order)
            np.testing.assert_array_equal(D[i, :m].astype(np.float64), ref[i, order])
        assert np.all(I[:, m:] == -1) and np.all(D[:, m:] == -np.finfo(np.float32).max)
    assert len(np.unique(ref[0])) < n                                  # the grid does produce ties: the row order is exercised
