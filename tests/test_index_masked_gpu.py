"""search_masked: hac_index_search_masked* (mask_groups_kernel of csrc/masked.inc and scan16_masked_kernel of csrc/scan16_filter.inc) through FlatIPIndex,
i.e. the C ABI.

Every assertion is equality of I and of the bits of D with tests/masked_ref.py, the definition of include/haconvdr.h restated
over the CPU oracle's canonical scores.  Indexes are built like _index() of tests/test_search_plans_gpu.py: three adds cut off
the 64-row grid, so the rows straddle segments and the last group is partial (5000 rows: 79 groups, the last of 8 rows), with
the prefilter off.  Every case checks the host form and the tensor form and leaves the status word clean.  What the inputs
are good for is proved on the CPU in tests/test_index_masked.py."""
import re

import numpy as np
import pytest

from haconvdr_amd import synth
from tests import masked_cases, masked_ref, nonfinite, rank_ref
from tests.golden import cases
from tests.test_index_among_gpu import _tie_corpus
from tests.test_index_rank_gpu import hostile_queries
from tests.test_index_rows_gpu import hostile_corpus
from tests.test_search_plans_gpu import _index

pytestmark = pytest.mark.gpu

HAC_ERR_INVALID, HAC_ERR_UNSUPPORTED = 1, 4
MAX_K = 2048
D, N, NQ = masked_cases.D, masked_cases.N, masked_cases.NQ
_PLAN = re.compile(r"^mask_groups_kernel grid=\((?P<gx>\d+),(?P<gt>\d+)\) scan16_masked_kernel<W=(?P<W>\d+)> grid=\((?P<P>\d+),(?P<T>\d+)\) "
                   r"QT=(?P<QT>\d+) C=(?P<C>\d+) lds=(?P<lds>\d+) launches=(?P<launches>\d+)$")


def parse_plan(text):
    m = _PLAN.match(text)
    assert m, "not the plan of a search inside a bitmap: %r" % text
    return {k: int(v) for k, v in m.groupdict().items()}


def expected_tile(d, k, nq):
    """(QT, C, lds) by make_plan's scan16 arithmetic: C candidate slots per query, as many queries as 160 KiB of LDS hold, <= 16"""
    C = 1 << (k + 256 - 1).bit_length()
    per_q = (d // 4) * 16 + C * 8
    QT = min(16, (160 * 1024 - 128) // per_q, nq)
    return QT, C, per_q * QT + 128


def _cuda(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _words(masks, ntotal):
    """bool masks -> packed int64 [n_masks, W]; packed words pass through"""
    from haconvdr_amd.index import pack_mask
    a = np.asarray(masks)
    w = pack_mask(a) if a.dtype == np.bool_ else a.view(np.int64)
    return w.reshape((w.shape[0] if w.ndim == 2 else 1, (ntotal + 63) // 64))


def tensor_form(idx, q, masks, mask_of, k, id_map=None):
    """(D, I) of search_masked_tensor as ndarrays"""
    import torch
    D, I = idx.search_masked_tensor(_cuda(q, np.float32), k, _cuda(_words(masks, idx.ntotal), np.int64),
                                    None if mask_of is None else _cuda(mask_of, np.int64), id_map=id_map)
    torch.cuda.synchronize()
    return D.cpu().numpy(), I.cpu().numpy()


def both_forms(idx, q, masks, mask_of, k, want, what=""):
    """host form and tensor form against the reference; the status word stays clean"""
    masked_ref.assert_same(idx.search_masked(q, k, masks, mask_of), want, f"{what} host form")
    masked_ref.assert_same(tensor_form(idx, q, masks, mask_of, k), want, f"{what} tensor form")
    idx.check_status()


_BASE = {}


def _base(oracle):
    """the shared case: rows, queries and their canonical scores, computed once and never changed"""
    if not _BASE:
        x, q = masked_cases.base_case()
        S = rank_ref.canon_scores(oracle, x, q)
        S.setflags(write=False)
        _BASE["case"] = (x, q, S)
    return _BASE["case"]


# ---------------------------------------------------------------------------------------------------------------------
# 1. an all-ones mask is search
@pytest.mark.parametrize("k", [1, 10, 100, 2047, 2048])
def test_all_ones_mask_is_search(k, oracle):
    x, q, S = _base(oracle)
    idx = _index(D, x)
    ones = np.ones(N, np.bool_)
    for nq in (1, 16, 17, 37):
        want = masked_ref.masked_from_scores(S[:nq], ones, None, k)
        masked_ref.assert_same(idx.search(q[:nq], k), want, f"search k={k} nq={nq}")
        both_forms(idx, q[:nq], ones, None, k, want, f"k={k} nq={nq}")
        plan = parse_plan(idx.last_plan())
        QT, C, lds = expected_tile(D, k, nq)
        tiles = -(-nq // QT)
        assert (plan["QT"], plan["C"], plan["lds"], plan["T"], plan["gt"], plan["launches"], plan["W"]) == (QT, C, lds, tiles, tiles, 1, 4), plan
        assert plan["gx"] == 1 and 1 <= plan["P"] <= 20, plan             # 79 groups: one block of 256 lists them, at most 20 streams of 4 waves
    assert expected_tile(D, 2048, 37)[0] == 4 and expected_tile(D, 100, 37)[0] == 16


# ---------------------------------------------------------------------------------------------------------------------
# 2. mask edges
def test_mask_edges(oracle):
    x, q, S = _base(oracle)
    q, S = q[:5], S[:5]
    idx = _index(D, x)
    r = np.arange(N)
    half = masked_cases.random_masks(0xA40, 1, N, 2)[0]
    edges = {
        "all zeros": np.zeros(N, np.bool_),
        "row 0": r == 0, "row n-1": r == N - 1, "row 63": r == 63, "row 64": r == 64,
        "one whole group": (r >= 128) & (r < 192),
        "the last, partial group": r >= N - 8,
        "every 64th row": r % 64 == 17,
        "density 1/2": half, "its complement": ~half,
        "density 1/64": masked_cases.random_masks(0xA41, 1, N, 64)[0],
        "density 1/1000": masked_cases.random_masks(0xA42, 1, N, 1000)[0],
    }
    assert 1 <= edges["density 1/1000"].sum() < 10 and 40 < edges["density 1/64"].sum() < 120
    for name, mask in edges.items():
        for k in (1, 10, 100):
            want = masked_ref.masked_from_scores(S, mask, None, k)
            assert (want[1][:, :min(k, int(mask.sum()))] >= 0).all() and (want[1][:, int(mask.sum()):] == -1).all()    # k beyond the selected rows: padding
            both_forms(idx, q, mask, None, k, want, f"{name} k={k}")
    # a mask and its complement together are the search
    k = 50
    a, b = idx.search_masked(q, k, half), idx.search_masked(q, k, ~half)
    sD, sI = idx.search(q, k)
    for i in range(len(q)):
        both = np.concatenate([a[1][i], b[1][i]])
        sc = np.concatenate([a[0][i], b[0][i]])
        order = np.lexsort((both, -sc.astype(np.float64)))[:k]
        np.testing.assert_array_equal(both[order], sI[i])
    # only bits at or above ntotal in the last word: an empty list (packed words: a bool mask cannot say this)
    words = np.zeros((N + 63) // 64, np.int64)
    words[-1] = np.int64(-1) << np.int64(N % 64)
    empty = masked_ref.masked_from_scores(S, np.zeros(N, np.bool_), None, 7)
    both_forms(idx, q, words, None, 7, empty, "bits past ntotal only")
    words[-1] = -1                                                         # ... and with the 8 real rows of the last group
    both_forms(idx, q, words, None, 20, masked_ref.masked_from_scores(S, r >= N - 8, None, 20), "last word all ones")
    # nq == 0: HAC_OK, nothing touched
    import torch
    D0, I0 = idx.search_masked(np.zeros((0, D), np.float32), 7, half)
    assert D0.shape == I0.shape == (0, 7)
    D0, I0 = idx.search_masked_tensor(torch.zeros((0, D), device="cuda"), 7, _cuda(_words(half, N), np.int64))
    assert tuple(D0.shape) == tuple(I0.shape) == (0, 7)
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 3. which mask a query uses
@pytest.mark.parametrize("k", [10, 2048])
def test_which_mask_a_query_uses(k, oracle):
    x, q, S = _base(oracle)
    idx = _index(D, x)
    QT = expected_tile(D, k, NQ)[0]
    assert QT == (16 if k == 10 else 4)
    # a mask per query, mask_of null
    per_query = masked_cases.per_query_masks()
    both_forms(idx, q, per_query, None, k, masked_ref.masked_from_scores(S, per_query, None, k), "a mask per query")
    plan = parse_plan(idx.last_plan())
    assert plan["QT"] == QT and plan["T"] == -(-NQ // QT) and plan["launches"] == 1, plan
    # 37 queries over 5 masks: three tiles at QT = 16, the last partial
    grouped, mask_of = masked_cases.grouped_masks()
    both_forms(idx, q, grouped, mask_of, k, masked_ref.masked_from_scores(S, grouped, mask_of, k), "five masks")
    # one mask for all
    both_forms(idx, q, grouped[2], None, k, masked_ref.masked_from_scores(S, grouped[2], None, k), "one mask")
    # a tile whose queries' masks are pairwise disjoint
    disjoint = masked_cases.disjoint_masks()
    both_forms(idx, q[:16], disjoint, None, k, masked_ref.masked_from_scores(S[:16], disjoint, None, k), "disjoint masks")
    perm = (np.arange(16) * 5) % 16
    both_forms(idx, q[:16], disjoint, perm, k, masked_ref.masked_from_scores(S[:16], disjoint, perm, k), "disjoint masks, permuted")


def test_mask_of_out_of_range(oracle):
    import torch
    from haconvdr_amd import _lib
    from haconvdr_amd.index import _f32p, _i64p
    import ctypes
    x, q, S = _base(oracle)
    idx = _index(D, x)
    k = 10
    grouped, mask_of = masked_cases.grouped_masks()
    wild = mask_of.copy()
    wild[3], wild[16], wild[36], wild[20] = -1, 5, np.iinfo(np.int64).min, 2 ** 40
    want = masked_ref.masked_from_scores(S, grouped, wild, k)
    assert all((want[1][i] == -1).all() for i in (3, 16, 36, 20)) and (want[1][[0, 4, 17, 35], 0] >= 0).all()
    masked_ref.assert_same(tensor_form(idx, q, grouped, wild, k), want, "mask_of outside [0, n_masks): empty lists, tensor form")
    keys = idx.search_masked_keys_tensor(_cuda(q, np.float32), k, _cuda(_words(grouped, N), np.int64), _cuda(wild, np.int64))
    torch.cuda.synchronize()
    assert (keys.cpu().numpy()[[3, 16, 36, 20]] == 0).all()
    # the host form refuses, names the query and writes nothing
    Dh = np.full((NQ, k), np.float32(-123.5))
    Ih = np.full((NQ, k), -99, np.int64)
    w = _words(grouped, N)
    for at, bad in ((16, 5), (3, -1)):
        one = mask_of.copy()
        one[at] = bad
        with pytest.raises(_lib.HacError) as err:
            _lib.check(_lib.lib().hac_index_search_masked(idx._h, _f32p(q), NQ, k, w.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 5, w.shape[1],
                                                          _i64p(one), _f32p(Dh), _i64p(Ih)))
        assert err.value.code == HAC_ERR_INVALID and f"query {at}" in str(err.value) and f"{bad}" in str(err.value), str(err.value)
        with pytest.raises(_lib.HacError) as err:
            idx.search_masked(q, k, grouped, one)
        assert err.value.code == HAC_ERR_INVALID and f"query {at}" in str(err.value)
    assert (Dh == np.float32(-123.5)).all() and (Ih == -99).all()
    # a null mask_of with neither one mask nor nq of them, k out of range, no mask: the library's own checks (the C ABI called directly)
    qt, wt = _cuda(q, np.float32), _cuda(w, np.int64)
    L = _lib.lib()
    for nq_, k_, n_masks_ in ((NQ, k, 5), (NQ, 0, 1), (NQ, MAX_K + 1, 1), (NQ, k, 0)):
        assert L.hac_index_search_masked_device(idx._h, qt.data_ptr(), nq_, k_, wt.data_ptr(), n_masks_, w.shape[1], None, None, None, None, None) == HAC_ERR_INVALID
        assert L.hac_index_search_masked(idx._h, _f32p(q), nq_, k_, w.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), n_masks_, w.shape[1], None,
                                         _f32p(Dh), _i64p(Ih)) == HAC_ERR_INVALID
    # argument mistakes on real CUDA tensors: ValueError before the library is called
    mt = _cuda(mask_of, np.int64)
    for args in ((qt, 0, wt, mt), (qt, MAX_K + 1, wt, mt), (qt, k, wt, None), (qt, k, wt[:, :-1], mt), (qt, k, wt[0], None), (qt, k, wt.to(torch.int32), mt),
                 (qt, k, wt.cpu(), mt), (qt, k, wt, mt[:-1]), (qt, k, wt, mt.to(torch.int32)), (qt, k, wt, mt.cpu()), (qt, k, _cuda(grouped, np.bool_), mt)):
        with pytest.raises(ValueError):
            idx.search_masked_tensor(*args)
    masked_ref.assert_same(tensor_form(idx, q, grouped, mask_of, k), masked_ref.masked_from_scores(S, grouped, mask_of, k), "after the refused calls")
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 4. compaction and thresholds: one workgroup walks every group (masked_p = 1), k = 10
def _p1_and_auto(x, q, masks, mask_of, k, want, what):
    idx = _index(D, x, masked_p="1")
    both_forms(idx, q, masks, mask_of, k, want, f"{what} masked_p=1")
    plan = parse_plan(idx.last_plan())
    assert plan["P"] == 1 and plan["C"] == 512, plan                       # 20 rounds of 4 groups; a buffer compacts past 256 of its 512 slots
    idx.set_option("masked_p", "auto")
    both_forms(idx, q, masks, mask_of, k, want, f"{what} masked_p=auto")
    assert parse_plan(idx.last_plan())["P"] > 1
    idx.set_option("masked_p", "3")
    both_forms(idx, q, masks, mask_of, k, want, f"{what} masked_p=3")
    assert parse_plan(idx.last_plan())["P"] == 3


def test_compaction_under_a_dense_mask(oracle):
    x, q, S = _base(oracle)
    ones = np.ones(N, np.bool_)
    _p1_and_auto(x, q[:16], ones, None, 10, masked_ref.masked_from_scores(S[:16], ones, None, 10), "dense")
    half = masked_cases.per_query_masks()[:16]
    _p1_and_auto(x, q[:16], half, None, 10, masked_ref.masked_from_scores(S[:16], half, None, 10), "a mask per query")


@pytest.mark.parametrize("ascending", [True, False])
def test_compaction_with_scores_monotone_in_the_row(ascending, oracle):
    x, q = masked_cases.monotone_case(ascending)
    S = rank_ref.canon_scores(oracle, x, q)
    for name, mask in (("dense", np.ones(N, np.bool_)), ("every third row", np.arange(N) % 3 == 1)):
        want = masked_ref.masked_from_scores(S, mask, None, 10)
        _p1_and_auto(x, q, mask, None, 10, want, f"ascending={ascending} {name}")


def test_high_scorers_deselected(oracle):
    x, q, S = _base(oracle)
    q, S = q[:5], S[:5]
    masks = masked_cases.deselected_half(S)
    want = masked_ref.masked_from_scores(S, masks, None, 10)
    _p1_and_auto(x, q, masks, None, 10, want, "the lower-scoring half")


def test_set_option_values():
    from haconvdr_amd import _lib
    idx = _index(D, synth.embeddings(0xA50, 100, D))
    for name, bad in (("masked_p", "0"), ("masked_p", "4097"), ("masked_p", "x"), ("debug_masked_tiles", "-1"), ("debug_masked_tiles", "many")):
        with pytest.raises(_lib.HacError) as err:
            idx.set_option(name, bad)
        assert err.value.code == HAC_ERR_INVALID
    for name, good in (("masked_p", "1"), ("masked_p", "4096"), ("masked_p", "auto"), ("debug_masked_tiles", "2"), ("debug_masked_tiles", "0")):
        idx.set_option(name, good)


# ---------------------------------------------------------------------------------------------------------------------
# 5. ties
def test_ties_with_mask_boundaries_inside_runs_of_equal_scores(oracle):
    d, n, nq = 96, 1000, 6
    x, q = _tie_corpus(d, n, nq, 0xA60)
    S = rank_ref.canon_scores(oracle, x, q)
    assert all(len(np.unique(S[i])) <= 16 for i in range(nq))
    idx = _index(d, x)
    r = np.arange(n)
    masks = np.stack([(r >= 100) & (r < 517), r % 3 != 0, (r % 16 == 5) | (r % 16 == 6), masked_cases.random_masks(0xA61, 1, n, 2)[0]])
    mask_of = np.array([0, 1, 2, 3, 0, 1])
    for k in (37, 300):
        want = masked_ref.masked_from_scores(S, masks, mask_of, k)
        wD, wI = want
        named = wI >= 0
        same = (np.diff(wD, axis=1) == 0) & named[:, 1:]
        assert same.sum() > nq * min(k, 100) // 2 and (np.diff(wI, axis=1)[same] > 0).all()          # equal scores ascend by row
        both_forms(idx, q, masks, mask_of, k, want, f"ties k={k}")
    full = masked_ref.masked_from_scores(S, masks, mask_of, 38)[0]
    assert sum(full[i, 36] == full[i, 37] for i in range(nq)) >= nq - 1                               # the cut at 37 falls inside a tie
    np.testing.assert_array_equal(masked_ref.masked_from_scores(S[:1], masks[0], None, 417)[1][0], np.arange(100, 517))    # the zero query: row order


# ---------------------------------------------------------------------------------------------------------------------
# 6. launch cuts
@pytest.mark.parametrize("k", [10, 2048])
def test_launch_cuts(k, oracle):
    x, q, S = _base(oracle)
    idx = _index(D, x, debug_masked_tiles="2")
    QT = expected_tile(D, k, NQ)[0]
    tiles = -(-NQ // QT)
    per_query = masked_cases.per_query_masks()
    want = masked_ref.masked_from_scores(S, per_query, None, k)
    both_forms(idx, q, per_query, None, k, want, "a mask per query across the cut")
    plan = parse_plan(idx.last_plan())
    assert plan["T"] == plan["gt"] == 2 and plan["launches"] == -(-tiles // 2) and plan["launches"] >= 2, plan
    grouped, mask_of = masked_cases.grouped_masks()
    both_forms(idx, q, grouped, mask_of, k, masked_ref.masked_from_scores(S, grouped, mask_of, k), "mask_of across the cut")
    idx.set_option("debug_masked_tiles", "1")
    both_forms(idx, q, per_query, None, k, want, "one tile per launch")
    assert parse_plan(idx.last_plan())["launches"] == tiles
    idx.set_option("debug_masked_tiles", "0")
    both_forms(idx, q, per_query, None, k, want, "one launch")
    assert parse_plan(idx.last_plan())["launches"] == 1


# ---------------------------------------------------------------------------------------------------------------------
# 7. non-finite queries and hostile rows
@pytest.mark.parametrize("kind", nonfinite.KINDS)
def test_nonfinite_queries(kind, oracle):
    d, n, nq, k = 96, 3001, 33, 100
    x, q, pos, _ = nonfinite.case(kind, d, n, nq, 0xA70)
    with np.errstate(all="ignore"):
        S = rank_ref.canon_scores(oracle, x, q)
    masks = masked_cases.random_masks(0xA71, 3, n, 2)
    mask_of = (np.arange(nq) % 3).astype(np.int64)
    want = masked_ref.masked_from_scores(S, masks, mask_of, k)
    if kind in nonfinite.NAN_KINDS:
        assert all((want[1][i] == -1).all() for i in pos)                 # a NaN query: padding only
    if kind in nonfinite.INF_KINDS:
        assert all(np.isinf(want[0][i]).any() for i in pos)               # +-Inf are ordinary scores
    healthy = [i for i in range(nq) if i not in pos]
    assert (want[1][healthy] >= 0).all()
    idx = _index(d, x)
    both_forms(idx, q, masks, mask_of, k, want, kind)


@pytest.mark.parametrize("d", [32, 96, 160])
def test_dimensions_on_hostile_rows(d, oracle):
    n, nq = 1000, 17
    x = hostile_corpus(0xA80 + d, n, d)
    q = hostile_queries(0xA81 + d, nq, d)
    with np.errstate(all="ignore"):
        S = rank_ref.canon_scores(oracle, x, q)
    masks = masked_cases.random_masks(0xA82 + d, nq, n, 2)
    masks[:, 3:403:10] = True                                             # forty of the raw-word rows: NaN scores among the selected
    assert np.isnan(S[masks]).any()
    idx = _index(d, x)
    for k in (1, 100, 600):
        want = masked_ref.masked_from_scores(S, masks, None, k)
        assert not np.isnan(want[0]).any()
        both_forms(idx, q, masks, None, k, want, f"d={d} k={k}")


# ---------------------------------------------------------------------------------------------------------------------
# 8. index lifetime
def test_after_remove_and_after_reset(oracle):
    from haconvdr_amd import _lib
    from haconvdr_amd.index import pack_mask
    d, n, nq, k = 96, 1000, 5, 50
    x = synth.embeddings(0xA90, n, d)
    q = synth.embeddings(0xA91, nq, d)
    idx = _index(d, x)
    mask = masked_cases.random_masks(0xA92, 1, n, 3)[0]
    both_forms(idx, q, mask, None, k, masked_ref.masked(oracle, x, q, mask, None, k), "as built")
    old_words = pack_mask(mask)
    gone = np.arange(100, 900, 7)
    assert idx.remove_ids(gone) == len(gone)
    left = np.delete(x, gone, 0)
    # a mask packed before the removal has stale words: refused by the Python check and by the library
    assert len(old_words) != (len(left) + 63) // 64
    with pytest.raises(ValueError):
        idx.search_masked(q, k, old_words)
    import ctypes
    from haconvdr_amd.index import _f32p, _i64p
    Dh, Ih = np.zeros((nq, k), np.float32), np.zeros((nq, k), np.int64)
    rc = _lib.lib().hac_index_search_masked(idx._h, _f32p(q), nq, k, old_words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 1, len(old_words), None,
                                            _f32p(Dh), _i64p(Ih))
    assert rc == HAC_ERR_INVALID and "words=" in _lib.lib().hac_last_error().decode()
    rc = _lib.lib().hac_index_search_masked_device(idx._h, _cuda(q, np.float32).data_ptr(), nq, k, _cuda(old_words, np.int64).data_ptr(), 1, len(old_words),
                                                   None, None, None, None, None)
    assert rc == HAC_ERR_INVALID
    kept = np.delete(mask, gone)                                           # the mask repacked for the rows that are left
    both_forms(idx, q, kept, None, k, masked_ref.masked(oracle, left, q, kept, None, k), "after remove_ids")
    # reset() and a smaller add(): the stale rows behind the new ntotal are never returned, whatever the last word says
    idx.reset()
    small = synth.embeddings(0xA93, 130, d)
    idx.add(small)
    words = np.full(3, -1, np.int64)                                       # all ones, the 62 bits past row 129 too
    want = masked_ref.masked(oracle, small, q, np.ones(130, np.bool_), None, 200)
    assert (want[1][:, :130] >= 0).all() and (want[1][:, 130:] == -1).all()
    both_forms(idx, q, words, None, 200, want, "after reset and a smaller add")
    idx.reset()                                                            # an empty index: padding only, words == 0
    both_forms(idx, q, np.zeros((1, 0), np.int64), None, 4, (np.full((nq, 4), -masked_ref.FMAX, np.float32), np.full((nq, 4), -1, np.int64)), "empty index")


# ---------------------------------------------------------------------------------------------------------------------
# 9. the keys form
def test_keys_form_feeds_merge_keys_and_keys_to_results(oracle):
    """Two indexes hold the two halves of a corpus; each searches under its slice of the masks with pos_base = its first row:
    merged, the keys are those of one index over the whole corpus."""
    import torch
    from haconvdr_amd.index import keys_to_results, merge_keys
    d, n, nq, k = 96, 1501, 7, 60
    x, q, ids = cases.search_case_inputs("dup", 0xAA0, n, nq, d=d)        # row r and row r + 750 are twins: ties cross the cut
    cut = 751
    r = np.arange(n)
    masks = np.stack([(r % 750) % 3 != 1, (r >= cut - 40) & (r < cut + 25)])
    mask_of = (np.arange(nq) % 2).astype(np.int64)
    lo, hi = _index(d, x[:cut]), _index(d, x[cut:])
    qt, mt = _cuda(q, np.float32), _cuda(mask_of, np.int64)
    k_lo = lo.search_masked_keys_tensor(qt, k, _cuda(_words(masks[:, :cut], cut), np.int64), mt, pos_base=0)
    k_hi = hi.search_masked_keys_tensor(qt, k, _cuda(_words(masks[:, cut:], n - cut), np.int64), mt, pos_base=cut)
    Dm, Im = keys_to_results(merge_keys(torch.stack([k_lo, k_hi])), id_map=_cuda(ids, np.int64))
    torch.cuda.synchronize()
    wD, wI = masked_ref.masked(oracle, x, q, masks, mask_of, k)
    assert any(wD[i, j] == wD[i, j + 1] and wI[i, j] < cut <= wI[i, j + 1] for i in range(nq) for j in range(k - 1))
    masked_ref.assert_same((Dm.cpu().numpy(), Im.cpu().numpy()), (wD, ids[wI]), "two shards merged")
    # id_map through the tensor form of one index
    whole = _index(d, x)
    masked_ref.assert_same(tensor_form(whole, q, masks, mask_of, k, id_map=_cuda(ids, np.int64)), (wD, ids[wI]), "id_map")
    for i in (lo, hi, whole):
        i.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 10. several shards in one process
@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)])
def test_multi_device_index(devices, oracle):
    from haconvdr_amd import _lib
    d, n, nq, k = 96, 1501, 9, 80
    x, q, _ = cases.search_case_inputs("dup", 0xAB0, n, nq, d=d)          # twins 750 rows apart: they land on different shards
    idx = _index(d, x, devices=devices)
    S = rank_ref.canon_scores(oracle, x, q)
    r = np.arange(n)
    S_ = len(devices)
    # the rows at the edges of every shard's share of every add: the three adds are cut at c1, c2, each dealt to the shards in
    # contiguous pieces -- every multiple of a piece's length near a cut is covered by a band of rows around it
    from tests.test_search_plans_gpu import _cuts
    c1, c2 = _cuts(n)
    edges = np.zeros(n, np.bool_)
    for a, b in ((0, c1), (c1, c2), (c2, n)):
        per = -(-(b - a) // S_)
        for s in range(S_ + 1):
            e = min(b, a + s * per)
            edges[max(0, e - 2):min(n, e + 2)] = True
    masks = np.stack([(r % 750) % 3 != 1, edges, ~edges, masked_cases.random_masks(0xAB1, 1, n, 64)[0], np.ones(n, np.bool_)])
    mask_of = (np.arange(nq) % 5).astype(np.int64)
    for kk in (1, k, 700):
        want = masked_ref.masked_from_scores(S, masks, mask_of, kk)
        masked_ref.assert_same(idx.search_masked(q, kk, masks, mask_of), want, f"{S_} shards k={kk}")
    assert any(want[0][i, j] == want[0][i, j + 1] for i in range(nq) for j in range(40))
    assert (want[1][1, int(edges.sum()):] == -1).all() and (want[1][1, :int(edges.sum())] >= 0).all()    # every edge row found, none twice
    masked_ref.assert_same(idx.search_masked(q, 5, masks[4]), masked_ref.masked_from_scores(S, masks[4], None, 5), "one mask")
    masked_ref.assert_same(idx.search(q, 5), masked_ref.masked_from_scores(S, masks[4], None, 5), "search")
    bad = mask_of.copy()
    bad[4] = 5
    with pytest.raises(_lib.HacError) as err:
        idx.search_masked(q, k, masks, bad)
    assert err.value.code == HAC_ERR_INVALID and "query 4" in str(err.value)
    qt, wt, mt = _cuda(q, np.float32), _cuda(_words(masks, n), np.int64), _cuda(mask_of, np.int64)
    for call in (lambda: idx.search_masked_tensor(qt, k, wt, mt), lambda: idx.search_masked_keys_tensor(qt, k, wt, mt)):
        with pytest.raises(_lib.HacError) as err:
            call()
        assert err.value.code == HAC_ERR_UNSUPPORTED
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 11. captured into a graph
def test_captured_into_a_graph_replays_on_new_masks(oracle):
    import torch
    d, n, nq, k = 96, 1000, 17, 64
    x = hostile_corpus(0xAC0, n, d)
    qs = [hostile_queries(0xAC1 + r, nq, d) for r in range(2)]
    masks = [masked_cases.random_masks(0xAC3 + r, 4, n, 2 + 30 * r) for r in range(2)]       # dense, then selective: other group lists
    ofs = [((np.arange(nq) * (r + 1)) % 4).astype(np.int64) for r in range(2)]
    for o in ofs:
        o[5] = -1                                                          # a query without a mask in every replay
    with np.errstate(all="ignore"):
        wants = [masked_ref.masked(oracle, x, qs[r], masks[r], ofs[r], k) for r in range(2)]
    idx = _index(d, x)
    qt, wt, mt = _cuda(qs[0], np.float32), _cuda(_words(masks[0], n), np.int64), _cuda(ofs[0], np.int64)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()                            # a single stream: no parallel branches in the graph
    replayed = []
    with torch.cuda.stream(side):
        eager = idx.search_masked_tensor(qt, k, wt, mt)   # the largest shape once: workspaces and the segment table exist
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            Dg, Ig = idx.search_masked_tensor(qt, k, wt, mt)
        for r in (1, 0, 1):
            qt.copy_(torch.from_numpy(qs[r]))
            wt.copy_(torch.from_numpy(_words(masks[r], n)))
            mt.copy_(torch.from_numpy(ofs[r]))
            Dg.zero_()
            Ig.fill_(-7)
            g.replay()
            side.synchronize()
            replayed.append((r, Dg.cpu().numpy(), Ig.cpu().numpy()))
    torch.cuda.synchronize()
    masked_ref.assert_same((eager[0].cpu().numpy(), eager[1].cpu().numpy()), wants[0], "eager")
    for r, Dr, Ir in replayed:
        masked_ref.assert_same((Dr, Ir), wants[r], f"replay on contents {r}")
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 12. determinism
def test_two_identical_calls_return_identical_bytes():
    import torch
    d, n, nq, k = 96, 3000, 40, 300
    x, q = _tie_corpus(d, n, nq, 0xAD0)
    idx = _index(d, x)
    masks = masked_cases.random_masks(0xAD1, nq, n, 2)
    qt, wt = _cuda(q, np.float32), _cuda(_words(masks, n), np.int64)
    a = idx.search_masked_tensor(qt, k, wt)
    b = idx.search_masked_tensor(qt, k, wt)
    ka = idx.search_masked_keys_tensor(qt, k, wt, pos_base=5)
    kb = idx.search_masked_keys_tensor(qt, k, wt, pos_base=5)
    torch.cuda.synchronize()
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(ka, kb)
    h1, h2 = idx.search_masked(q, k, masks), idx.search_masked(q, k, masks)
    assert h1[0].tobytes() == h2[0].tobytes() and h1[1].tobytes() == h2[1].tobytes()
    masked_ref.assert_same(h1, (a[0].cpu().numpy(), a[1].cpu().numpy()), "host form vs tensor form")
    # pack_mask of a CUDA tensor gives the words pack_mask of the ndarray gives
    from haconvdr_amd.index import pack_mask
    assert torch.equal(pack_mask(torch.from_numpy(masks).cuda()).cpu(), torch.from_numpy(pack_mask(masks)))
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 13. the host form across its staging chunks.  The sizes follow from the host code: a chunk's queries (4d bytes and 8 of
# mask_of each) and the distinct masks they name (8 * ceil(shard rows / 64) bytes each) fit 64 MiB, and a chunk uploads only
# the masks it names, renumbered from 0.  d = 1024 (the widest row: the fewest queries per chunk), 200 hostile rows on two
# shards of one device, so the slice of every mask and the remap take part.
SEAM_BYTES, SEAM_D, SEAM_N, SEAM_NQ, SEAM_K = 64 << 20, 1024, 200, 16385, 5
_SEAM = {}


def seam_case(oracle):
    """(x [200, 1024] hostile, q [16385, 1024], their canonical scores): computed once, shared by the chunk-seam cases of
    search_masked and search_grouped, never changed"""
    if not _SEAM:
        x = hostile_corpus(0xAE0, SEAM_N, SEAM_D)
        q = hostile_queries(0xAE1, SEAM_NQ, SEAM_D)
        with np.errstate(all="ignore"):
            S = rank_ref.canon_scores(oracle, x, q)
        for a in (x, q, S):
            a.setflags(write=False)
        _SEAM["case"] = (x, q, S)
    return _SEAM["case"]


def shard_rows(n, shards):
    """the rows of every shard of _index(d, x, devices=(0,) * shards): each of the three adds is dealt in contiguous pieces"""
    from tests.test_search_plans_gpu import _cuts
    c1, c2 = _cuts(n)
    return [sum(m // shards + (s < m % shards) for m in (c1, c2 - c1, n - c2)) for s in range(shards)]


def _seam_mask_bytes():
    words = {-(-rows // 64) for rows in shard_rows(SEAM_N, 2)}
    assert len(words) == 1                                                 # both shards cut their chunks at the same query
    return 8 * words.pop()


@pytest.mark.parametrize("past", [0, 1])
def test_host_form_across_a_chunk_of_shared_masks(past, oracle):
    x, q, S = seam_case(oracle)
    m_bytes = _seam_mask_bytes()
    cut = (SEAM_BYTES - 3 * m_bytes) // (4 * SEAM_D + 8)                   # the largest n with n * (4d + 8) + 3 * m_bytes <= 64 MiB
    assert cut * (4 * SEAM_D + 8) + 3 * m_bytes <= SEAM_BYTES < (cut + 1) * (4 * SEAM_D + 8) + 3 * m_bytes and cut + 1 <= SEAM_NQ
    nq = cut + past
    r = np.arange(SEAM_N)
    masks = np.stack([r % 3 == 0, r % 3 == 1, r % 3 == 2])               # pairwise disjoint: an answer from the wrong mask shares no row
    mask_of = (np.arange(nq) % 2).astype(np.int64)
    mask_of[cut:] = 2                                                      # the second chunk names mask 2 alone: its local mask 0
    want = masked_ref.masked_from_scores(S[:nq], masks, mask_of, SEAM_K)
    assert (want[1][4:, 0] >= 0).all() and all((want[1][i][want[1][i] >= 0] % 3 == mask_of[i]).all() for i in (1, 2, cut - 1, nq - 1))
    idx = _index(SEAM_D, x, devices=(0, 0))
    masked_ref.assert_same(idx.search_masked(q[:nq], SEAM_K, masks, mask_of), want, f"{nq} queries, the cut at {cut}")
    plan = parse_plan(idx.last_plan())
    assert (plan["QT"] == 1) == (past == 1), plan                          # the last chunk held one query, or a full tile's
    idx.check_status()


def test_host_form_across_a_chunk_of_a_mask_per_query(oracle):
    x, q, S = seam_case(oracle)
    m_bytes = _seam_mask_bytes()
    cut = SEAM_BYTES // (4 * SEAM_D + 8 + m_bytes)                         # every query brings a new mask
    nq = cut + 1
    assert nq <= SEAM_NQ
    masks = masked_cases.random_masks(0xAE2, nq, SEAM_N, 2)
    want = masked_ref.masked_from_scores(S[:nq], masks, None, SEAM_K)
    assert (want[1][4:, 0] >= 0).all()
    idx = _index(SEAM_D, x, devices=(0, 0))
    masked_ref.assert_same(idx.search_masked(q[:nq], SEAM_K, masks), want, f"{nq} queries and masks, the cut at {cut}")
    assert parse_plan(idx.last_plan())["QT"] == 1
    idx.check_status()
