"""The exact fp32 top-k kernels (scan16_kernel, scanq_kernel<NT,W>, threshold seeding, tile_rows_kernel) at the plan,
dimension and k edges the rest of the suite does not reach: d % 64 == 32, scan16 with a reduced query tile over several
tiles, scanq with a single slack slot (C == k + 1), every scanq<NT,W> instantiation away from d = 768, and seeding on
hostile rows.  Every search goes through FlatIPIndex (the C ABI) with the prefilter off, is compared bit for bit (ids AND
scores, every query) with oracle.flat_ip_search, must leave the index's status word clean, and asserts on the parsed
plan text that it ran the kernel configuration it was written for: a planner change that moves a case off its edge
fails the test instead of silently taking the coverage away.

Row counts are not multiples of 64 (a partial last group) and rows arrive in three add() calls cut off the group grid
(several segments), except where a case needs an exact count (the seeding boundary 16 320 / 16 321, the 2048-row
single-slot ascending case)."""
import re

import numpy as np
import pytest

from tests.golden import cases

pytestmark = pytest.mark.gpu

FMAX = np.finfo(np.float32).max

_PLAN16 = re.compile(r"^scan16_kernel<W=(?P<W>\d+)> grid=\((?P<P>\d+),(?P<T>\d+)\) QT=(?P<QT>\d+) C=(?P<C>\d+) "
                     r"lds=(?P<lds>\d+) seed=(?P<seed>[01])$")
_PLANQ = re.compile(r"^scanq_kernel<NT=(?P<NT>\d+),W=(?P<W>\d+)> grid=\((?P<P>\d+),(?P<T>\d+)\) NQ=(?P<QT>\d+) C=(?P<C>\d+) "
                    r"lds=(?P<lds>\d+) seed=(?P<seed>[01])$")


def parse_plan(text):
    """hac_index_last_plan of an exact search -> {"kernel": "scan16" | "scanq", "NT", "W", "P", "T", "QT", "C", "seed"}
    (QT: queries per workgroup, scanq's NQ; T: query tiles = grid.y; NT is 0 for scan16).  Anything else, the prefilter's
    "split: ..." included, is a failure of the test that asked."""
    for kernel, rx in (("scan16", _PLAN16), ("scanq", _PLANQ)):
        m = rx.match(text)
        if m:
            f = {name: int(v) for name, v in m.groupdict().items()}
            f.setdefault("NT", 0)
            f["kernel"] = kernel
            return f
    raise AssertionError("not the plan of an exact scan: %r" % text)


def _seed(d, n, nq, k, salt=0):
    """One seed per (d, n, nq, k); search_case_inputs uses seed, seed + 1 and seed + 2, hence the stride of 4."""
    return ((((d * 32768 + n) * 256 + nq) * 4096 + k) * 64 + salt) * 4


def _cuts(n):
    c1, c2 = n // 3, (2 * n) // 3
    while c1 % 64 == 0:
        c1 += 1
    while c2 % 64 == 0 or c2 <= c1:
        c2 += 1
    return c1, c2


def _index(d, x, devices=(0,), **options):
    """A fresh index, prefilter off unless told otherwise, the rows in three adds whose cuts are off the 64-row grid."""
    from haconvdr_amd.index import FlatIPIndex
    idx = FlatIPIndex(d, devices=devices)
    idx.set_option("split", "0")
    for name, value in options.items():
        idx.set_option(name, value)
    n = len(x)
    if n >= 3:
        c1, c2 = _cuts(n)
        assert c1 % 64 and c2 % 64 and 0 < c1 < c2 < n
        idx.add(x[:c1])
        idx.add(x[c1:c2])
        idx.add(x[c2:])
    else:
        idx.add(x)
    assert idx.ntotal == n
    return idx


def _search_checked(idx, x, q, k, oracle):
    """search + status + oracle bits for every query -> (plan fields, D, I)."""
    D, I = idx.search(q, k)
    idx.check_status()                                   # a poisoned tile must never pass as an empty list
    plan = parse_plan(idx.last_plan())
    oD, oI = oracle.flat_ip_search(x, q, k)
    np.testing.assert_array_equal(I, oI)
    np.testing.assert_array_equal(D, oD)
    return plan, D, I


def _tiles(nq, qt):
    return (nq + qt - 1) // qt


def _adversarial(d, n, nq, seed):
    """test_adversarial_ascending_scores' construction at any d: every row beats everything before it for every query, so
    thresholds never filter and the candidate lists overflow every round."""
    base = cases.search_case_inputs("gauss", seed, 1, nq, d=d)[1]
    x = np.zeros((n, d), np.float32)
    x[:, 0] = (np.arange(n, dtype=np.float32) + 1.0) / 64.0          # exactly representable, increasing
    q = np.zeros_like(base)
    q[:, 0] = np.abs(base[:, 0]) + 1.0
    return x, q


# ---------------------------------------------------------------------------------------------------------------------
# A. d % 64 == 32: K4 % 16 == 8, so scan16_kernel for every query count and never the prefilter.  d = 32 is NB = K4 / PF
# = 1: the chunk loop of scan16_kernel runs zero times, only its tail.
D32 = [32, 96, 160, 736, 992]


@pytest.mark.parametrize("k", [1, 100])
@pytest.mark.parametrize("nq", [1, 16, 17, 50])
@pytest.mark.parametrize("d", D32)
def test_d_32_mod_64_takes_scan16(d, nq, k, oracle):
    n = 3001
    x, q, _ = cases.search_case_inputs("gauss", _seed(d, n, nq, k), n, nq, d=d)
    idx = _index(d, x)
    plan, _, _ = _search_checked(idx, x, q, k, oracle)
    assert plan["kernel"] == "scan16" and plan["QT"] == min(16, nq) and plan["seed"] == 0, plan
    assert plan["T"] == _tiles(nq, 16), plan             # nq = 17, 50: two and four tiles, the last one partial


@pytest.mark.parametrize("d", D32)
def test_d_32_mod_64_seeded(d, oracle):
    """n = 16 449 rows = 258 groups: sample_scores_kernel (LDS K4 * 256 bytes) / kth_select_kernel seed the thresholds."""
    n, nq, k = 16449, 20, 10
    x, q, _ = cases.search_case_inputs("gauss", _seed(d, n, nq, k), n, nq, d=d)
    idx = _index(d, x)
    plan, _, _ = _search_checked(idx, x, q, k, oracle)
    assert plan["kernel"] == "scan16" and plan["T"] == 2 and plan["seed"] == 1, plan


def test_d96_prefilter_is_refused_same_bits(oracle):
    d, n, nq, k = 96, 3001, 50, 100
    x, q, _ = cases.search_case_inputs("gauss", _seed(d, n, nq, k, 1), n, nq, d=d)
    idx = _index(d, x)
    _, D0, I0 = _search_checked(idx, x, q, k, oracle)
    idx.set_option("split", "1")
    plan, D1, I1 = _search_checked(idx, x, q, k, oracle)
    assert not idx.last_plan().startswith("split:") and plan["kernel"] == "scan16" and plan["T"] == 4, plan
    np.testing.assert_array_equal(I1, I0)
    np.testing.assert_array_equal(D1, D0)


def test_d96_three_shards_in_process(oracle):
    from haconvdr_amd.index import FlatIPIndex
    d, n, nq, k = 96, 3001, 17, 100
    x, q, _ = cases.search_case_inputs("dup", _seed(d, n, nq, k, 2), n, nq, d=d)
    idx = FlatIPIndex(d, devices=(0, 0, 0))
    idx.set_option("split", "0")
    idx.add(x[:1000])
    idx.add(x[1000:1001])                                # a one-row add: two shards get nothing from it
    idx.add(x[1001:])
    assert idx.ntotal == n
    plan, _, _ = _search_checked(idx, x, q, k, oracle)   # (the plan text is shard 0's)
    assert plan["kernel"] == "scan16" and plan["T"] == 2, plan


def test_d96_keys_with_pos_base_merge_and_id_map(oracle):
    import torch
    from haconvdr_amd.index import merge_keys, keys_to_results
    d, n, nq, k = 96, 3001, 17, 100
    x, q, ids = cases.search_case_inputs("dup", _seed(d, n, nq, k, 3), n, nq, d=d)
    half = 1501
    h1, h2 = _index(d, x[:half]), _index(d, x[half:])
    qd = torch.from_numpy(q).cuda()
    k1 = h1.search_keys_tensor(qd, k, pos_base=0)
    k2 = h2.search_keys_tensor(qd, k, pos_base=half)
    torch.cuda.synchronize()
    for h in (h1, h2):
        h.check_status()
        plan = parse_plan(h.last_plan())
        assert plan["kernel"] == "scan16" and plan["T"] == 2, plan
    D, I = keys_to_results(merge_keys(torch.stack([k1, k2])), id_map=torch.from_numpy(ids).cuda())
    oD, oI = oracle.flat_ip_search(x, q, k)
    np.testing.assert_array_equal(I.cpu().numpy(), ids[oI])
    np.testing.assert_array_equal(D.cpu().numpy(), oD)


def test_d96_k_larger_than_n_is_padded(oracle):
    d, n, nq, k = 96, 70, 17, 100
    x, q, _ = cases.search_case_inputs("gauss", _seed(d, n, nq, k, 4), n, nq, d=d)
    idx = _index(d, x)
    plan, D, I = _search_checked(idx, x, q, k, oracle)
    assert plan["kernel"] == "scan16" and plan["T"] == 2, plan
    assert np.all(I[:, n:] == -1) and np.all(D[:, n:] == -FMAX) and np.all(I[:, :n] >= 0)


def test_d96_ties_row_ascending(oracle):
    d = 96
    x = np.zeros((5001, d), np.float32)
    x[:, 0] = 1.0
    x[100:110, 1] = 1.0
    x[4000:4010, 1] = 1.0
    q = np.zeros((3, d), np.float32)
    q[0, 0], q[0, 1] = 1.0, 0.5
    q[2, 0] = -1.0
    idx = _index(d, x)
    plan, D, I = _search_checked(idx, x, q, 120, oracle)
    assert plan["kernel"] == "scan16", plan
    assert list(I[0, :20]) == list(range(100, 110)) + list(range(4000, 4010))
    assert list(I[1]) == list(range(120))                # all-zero query: every score ties at 0


# ---------------------------------------------------------------------------------------------------------------------
# B. scan16 with a reduced query tile: k >= 512 drops scanq (its LDS no longer fits), and K4 * 16 + C * 8 bytes per
# query no longer fit 16 times, so QT < 16 over several tiles.  ldsQ is [K4][QTr]: a wrong query stride or candidate base
# shows only with QTr < 16 on a tile that is not the first.
B_CASES = [(768, 9, 2048), (768, 40, 1000), (768, 33, 512), (1024, 7, 2048), (992, 21, 700), (64, 50, 2048)]


def _assert_reduced_tile(plan, nq):
    assert plan["kernel"] == "scan16" and plan["QT"] < 16 and plan["T"] >= 2, plan
    assert plan["T"] == _tiles(nq, plan["QT"]), plan


@pytest.mark.parametrize("d,nq,k", B_CASES)
def test_scan16_reduced_query_tile(d, nq, k, oracle):
    n = 5003
    x, q, _ = cases.search_case_inputs("gauss", _seed(d, n, nq, k), n, nq, d=d)
    idx = _index(d, x)
    plan, _, _ = _search_checked(idx, x, q, k, oracle)
    _assert_reduced_tile(plan, nq)


@pytest.mark.parametrize("order", ["ascending", "descending"])
@pytest.mark.parametrize("d,nq,k", [(768, 40, 1000), (1024, 7, 2048)])
def test_scan16_reduced_query_tile_adversarial(d, nq, k, order, oracle):
    """Every round overflows hw = C - 256 (ascending) or nothing after the first rounds passes (descending): compaction
    carries the result."""
    n = 5003
    x, q = _adversarial(d, n, nq, _seed(d, n, nq, k, 1))
    if order == "descending":
        x = x[::-1].copy()
    idx = _index(d, x)
    plan, _, _ = _search_checked(idx, x, q, k, oracle)
    _assert_reduced_tile(plan, nq)


def test_scan16_reduced_query_tile_fewer_rows_than_k(oracle):
    d, n, nq, k = 768, 300, 33, 512
    x, q, _ = cases.search_case_inputs("gauss", _seed(d, n, nq, k), n, nq, d=d)
    idx = _index(d, x)
    plan, D, I = _search_checked(idx, x, q, k, oracle)
    _assert_reduced_tile(plan, nq)
    assert np.all(I[:, n:] == -1) and np.all(D[:, n:] == -FMAX) and np.all(I[:, :n] >= 0)   # padded tails in every tile


# ---------------------------------------------------------------------------------------------------------------------
# C. scanq with exactly one slack slot: C = max(32, next_pow2(k + 1)) = k + 1 and hw = (C + k) / 2 = k for k = 2^m - 1,
# so a compacted list has room for a single key and a round needs up to W * 64 + 1 passes (bound: W * 64 + 4).
C_CASES = [(31, 40, "8"), (63, 40, "8"), (63, 40, "4"), (127, 40, "8"), (255, 40, "8"), (255, 40, "4"), (511, 40, "8"),
           (511, 20, "8")]       # k = 511: only NT = 1 fits


def _assert_one_slack_slot(plan, k, nq, waves):
    assert plan["kernel"] == "scanq" and plan["C"] == k + 1 and plan["W"] == int(waves), plan
    assert plan["T"] == _tiles(nq, 32 * plan["NT"]), plan


@pytest.mark.parametrize("k,nq,waves", C_CASES)
def test_scanq_one_slack_slot_gauss(k, nq, waves, oracle):
    d, n = 768, 6001
    x, q, _ = cases.search_case_inputs("gauss", _seed(d, n, nq, k, int(waves)), n, nq, d=d)
    idx = _index(d, x, scanq_waves=waves)
    plan, _, _ = _search_checked(idx, x, q, k, oracle)
    _assert_one_slack_slot(plan, k, nq, waves)


@pytest.mark.parametrize("order", ["ascending", "descending"])
@pytest.mark.parametrize("k,nq,waves", C_CASES)
def test_scanq_one_slack_slot_adversarial(k, nq, waves, order, oracle):
    """Ascending rows: every pass of a round places one key per query and compacts."""
    d, n = 768, (6000 if k <= 255 else 2048)
    x, q = _adversarial(d, n, nq, _seed(d, n, nq, k, int(waves)))
    if order == "descending":
        x = x[::-1].copy()
    idx = _index(d, x, scanq_waves=waves)
    plan, _, _ = _search_checked(idx, x, q, k, oracle)
    _assert_one_slack_slot(plan, k, nq, waves)


@pytest.mark.parametrize("k,nq,waves", C_CASES)
def test_scanq_one_slack_slot_all_ties(k, nq, waves, oracle):
    """Every score of a query equals its threshold: nothing is ever filtered, the earliest rows must survive."""
    d, n = 768, 3001
    x = np.ones((n, d), np.float32)
    q = np.zeros((nq, d), np.float32)
    q[:, 3] = np.linspace(-2, 2, nq).astype(np.float32)
    idx = _index(d, x, scanq_waves=waves)
    plan, _, I = _search_checked(idx, x, q, k, oracle)
    _assert_one_slack_slot(plan, k, nq, waves)
    assert np.all(I == np.arange(k)[None, :])


# ---------------------------------------------------------------------------------------------------------------------
# D. every scanq<NT, W> instantiation away from d = 768.  NS = K4 / 16 query slices go through a double-buffered LDS
# image: d = 64 is one slice, the kernel restages the slice it is reading.  nq = 130 gives several tiles with a partial
# last one for every NT (128 + 2 at NT = 4).
def _assert_scanq(plan, nt, waves, nq):
    assert plan["kernel"] == "scanq" and plan["NT"] == int(nt) and plan["W"] == int(waves), plan
    assert plan["QT"] == 32 * int(nt) and plan["T"] == _tiles(nq, 32 * int(nt)) and plan["T"] >= 2 and nq % plan["QT"], plan


@pytest.mark.parametrize("waves", ["4", "8"])
@pytest.mark.parametrize("nt", ["1", "2", "3", "4"])
@pytest.mark.parametrize("d", [64, 128, 448, 1024])
def test_scanq_instantiations_k10(d, nt, waves, oracle):
    n, nq, k = 4099, 130, 10
    x, q, _ = cases.search_case_inputs("gauss", _seed(d, n, nq, k, 4 * int(nt) + int(waves) // 8), n, nq, d=d)
    idx = _index(d, x, scanq_nt=nt, scanq_waves=waves)
    plan, _, _ = _search_checked(idx, x, q, k, oracle)
    _assert_scanq(plan, nt, waves, nq)
    assert plan["C"] == 32, plan


@pytest.mark.parametrize("waves", ["4", "8"])
@pytest.mark.parametrize("nt", ["1", "2", "3"])          # C = 128: NT = 4 no longer fits the LDS
@pytest.mark.parametrize("d", [64, 128, 448, 768, 1024])
def test_scanq_instantiations_k100(d, nt, waves, oracle):
    n, nq, k = 4099, 130, 100
    x, q, _ = cases.search_case_inputs("gauss", _seed(d, n, nq, k, 4 * int(nt) + int(waves) // 8), n, nq, d=d)
    idx = _index(d, x, scanq_nt=nt, scanq_waves=waves)
    plan, _, _ = _search_checked(idx, x, q, k, oracle)
    _assert_scanq(plan, nt, waves, nq)
    assert plan["C"] == 128, plan


def test_scanq_grid_rounding_switch_changes_no_bit(oracle):
    """scan_no_p8 = "1" (P not rounded down to a multiple of 8) against "0": another split of the rows over workgroups."""
    d, n, nq, k = 768, 4099, 130, 100
    x, q, _ = cases.search_case_inputs("gauss", _seed(d, n, nq, k, 31), n, nq, d=d)
    idx = _index(d, x)
    plan0, D0, I0 = _search_checked(idx, x, q, k, oracle)
    idx.set_option("scan_no_p8", "1")
    plan1, D1, I1 = _search_checked(idx, x, q, k, oracle)
    assert plan0["kernel"] == plan1["kernel"] == "scanq" and plan0["T"] == plan1["T"] >= 2, (plan0, plan1)
    assert {f: v for f, v in plan0.items() if f != "P"} == {f: v for f, v in plan1.items() if f != "P"}, (plan0, plan1)
    np.testing.assert_array_equal(I1, I0)
    np.testing.assert_array_equal(D1, D0)


@pytest.mark.parametrize("order", ["ascending", "descending"])
@pytest.mark.parametrize("d", [64, 1024])
def test_scanq_nt4_w4_adversarial(d, order, oracle):
    n, nq, k = 4099, 130, 10
    x, q = _adversarial(d, n, nq, _seed(d, n, nq, k, 32))
    if order == "descending":
        x = x[::-1].copy()
    idx = _index(d, x, scanq_nt="4", scanq_waves="4")
    plan, _, _ = _search_checked(idx, x, q, k, oracle)
    _assert_scanq(plan, "4", "4", nq)


# ---------------------------------------------------------------------------------------------------------------------
# E. threshold seeding as a true lower bound.  Seeding turns on at G >= 4 * max(64, G / 64, (k + 1) / 2) groups and samples
# every (G / n_sample)-th group: at the sizes below that is groups 0, 4, 8, ...  A seed that is too high silently shortens
# or corrupts a list.
def _hostile_rows(x):
    """Mutates x in place -> the rows that hold a NaN.
      * 36 rows of the sampled groups 0, 4 and 8, times four, repeated 300 times each elsewhere in the corpus (rows 1024 ...
        11 823, sampled and unsampled groups alike).  The copies outscore the other rows, so for every query the quarter
        maxima of the sample repeat a few values: the seed threshold sits on a score that 300 rows share inside and outside
        the sample, for small k on the true k-th score itself, and the earliest of the tied rows must come back.  (Every row
        of every sampled group 300 times over does not fit the row budget.)
      * NaN entries in rows of the sampled groups 0, 4 and 8, +Inf entries in two rows, a -0.0 row and a 0.0 row."""
    n, d = x.shape
    src = np.concatenate([g * 64 + np.arange(12) * 5 for g in (0, 4, 8)])
    x[1024:1024 + 300 * len(src)] = 4.0 * np.tile(x[src], (300, 1))
    nan_rows = [5, 4 * 64 + 17, 8 * 64 + 63]
    x[nan_rows[0], 5] = np.nan
    x[nan_rows[1], d - 1] = np.nan
    x[nan_rows[2], :] = np.nan
    x[12 * 64 + 1, 3] = np.inf                           # (group 12 is a sampled group)
    x[n - 2, d - 2] = np.inf
    x[77] = -0.0
    x[78] = 0.0
    return nan_rows


@pytest.mark.parametrize("k", [10, 127])
@pytest.mark.parametrize("nq", [5, 40])
@pytest.mark.parametrize("d", [96, 768, 1024])
@pytest.mark.parametrize("n", [16449, 20011])
def test_seed_is_a_true_lower_bound_on_hostile_rows(n, d, nq, k, oracle):
    x, q, _ = cases.search_case_inputs("gauss", _seed(d, n, nq, k), n, nq, d=d)
    nan_rows = _hostile_rows(x)
    idx = _index(d, x)
    plan, _, I = _search_checked(idx, x, q, k, oracle)
    assert plan["seed"] == 1, plan
    assert plan["kernel"] == ("scanq" if nq > 16 and d % 64 == 0 else "scan16"), plan
    assert not np.isin(I, nan_rows).any()                # NaN rows are never returned
    assert np.all(I >= 0)


@pytest.mark.parametrize("d", [96, 768])
def test_seeding_boundary_255_and_256_groups(d, oracle):
    """n = 16 320 is 255 groups: no seeding.  One more row is 256 groups: seeded.  Same queries, same oracle."""
    nq, k = 20, 10
    x, q, _ = cases.search_case_inputs("gauss", _seed(d, 16321, nq, k), 16321, nq, d=d)
    for n, seeded in ((16320, 0), (16321, 1)):
        idx = _index(d, x[:n])
        plan, _, _ = _search_checked(idx, x[:n], q, k, oracle)
        assert plan["seed"] == seeded, plan
