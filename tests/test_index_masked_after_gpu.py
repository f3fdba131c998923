"""search_masked behind a cursor: hac_index_search_masked_after* (scan16_masked_after_kernel of csrc/scan16_filter.inc behind
mask_groups_kernel and after_bounds_kernel) through FlatIPIndex, i.e. the C ABI.

Every assertion is equality of I and of the bits of D (or of the packed keys) with tests/masked_after_ref.py, the definition of
include/haconvdr.h restated over the CPU oracle's canonical scores.  Indexes are built like _index() of
tests/test_search_plans_gpu.py: three adds cut off the 64-row grid, the prefilter off.  Every case leaves the status word clean.
What the inputs are good for is proved on the CPU in tests/test_index_masked_after.py."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests import after_cases, after_ref, index_lifetime, masked_after_cases, masked_after_ref, masked_cases, masked_ref, nonfinite, rank_ref
from tests.test_index_among_gpu import _tie_corpus
from tests.test_index_masked_gpu import _cuda, _words, expected_tile
from tests.test_search_plans_gpu import _cuts, _index

pytestmark = pytest.mark.gpu

HAC_ERR_INVALID, HAC_ERR_UNSUPPORTED = 1, 4
MAX_K = 2048
D, N, NQ = masked_after_cases.D, masked_after_cases.N, masked_after_cases.NQ
FMAX = after_ref.FMAX
_PLAN = re.compile(r"^mask_groups_kernel grid=\((?P<gx>\d+),(?P<gt>\d+)\) scan16_masked_after_kernel<W=(?P<W>\d+)> grid=\((?P<P>\d+),(?P<T>\d+)\) "
                   r"QT=(?P<QT>\d+) C=(?P<C>\d+) lds=(?P<lds>\d+) launches=(?P<launches>\d+)$")
_CASES = {}


def parse_plan(text):
    m = _PLAN.match(text)
    assert m, "not the plan of a search inside a bitmap, behind a cursor: %r" % text
    return {k: int(v) for k, v in m.groupdict().items()}


def scores(name, oracle):
    """(x, q, S) of a shared input, computed once and never changed"""
    if name not in _CASES:
        x, q = {"base": after_cases.base_case, "tie": after_cases.tie_case, "hostile": after_cases.hostile_case,
                "descending": lambda: masked_cases.monotone_case(False), "ascending": lambda: masked_cases.monotone_case(True)}[name]()
        with np.errstate(all="ignore"):
            S = rank_ref.canon_scores(oracle, x, q)
        S.setflags(write=False)
        _CASES[name] = (x, q, S)
    return _CASES[name]


def tensor_form(idx, q, masks, mask_of, after, k, id_map=None):
    """(D, I) of search_masked_tensor(after=) as ndarrays; after None goes in as a start cursor (row -2), so that the call takes
    the cursor entry point"""
    import torch
    nq = len(q)
    sc, rw = (np.zeros(nq, np.float32), np.full(nq, after_ref.START, np.int64)) if after is None else after
    Dt, It = idx.search_masked_tensor(_cuda(q, np.float32), k, _cuda(_words(masks, idx.ntotal), np.int64), None if mask_of is None else _cuda(mask_of, np.int64),
                                      id_map=id_map, after=(_cuda(sc, np.float32), _cuda(rw, np.int64)))
    torch.cuda.synchronize()
    return Dt.cpu().numpy(), It.cpu().numpy()


def keys_form(idx, q, masks, mask_of, after_keys, k, pos_base=0):
    """the uint64 keys of search_masked_keys_tensor(after_keys=); None goes in as all-ones keys"""
    import torch
    ak = np.full(len(q), -1, np.int64) if after_keys is None else np.ascontiguousarray(after_keys).view(np.int64)
    keys = idx.search_masked_keys_tensor(_cuda(q, np.float32), k, _cuda(_words(masks, idx.ntotal), np.int64), None if mask_of is None else _cuda(mask_of, np.int64),
                                         pos_base=pos_base, after_keys=_cuda(ak, np.int64))
    torch.cuda.synchronize()
    return keys.cpu().numpy().view(np.uint64)


def host_form(idx, q, masks, mask_of, after, k):
    nq = len(q)
    return idx.search_masked(q, k, masks, mask_of, after=(np.zeros(nq, np.float32), np.full(nq, after_ref.START, np.int64)) if after is None else after)


def all_forms(idx, q, masks, mask_of, after, k, want, what=""):
    """host, tensor and keys form against the reference; the status word stays clean"""
    masked_after_ref.assert_same(host_form(idx, q, masks, mask_of, after, k), want, f"{what} host form")
    masked_after_ref.assert_same(tensor_form(idx, q, masks, mask_of, after, k), want, f"{what} tensor form")
    ak = None if after is None else after_ref.cursor_keys(after[0], after[1])
    masked_after_ref.assert_same(after_ref.unpack(keys_form(idx, q, masks, mask_of, ak, k)), want, f"{what} keys form")
    idx.check_status()


def want_of(S, masks, mask_of, after, k):
    return masked_after_ref.from_scores(S, masks, mask_of, None if after is None else after[0], None if after is None else after[1], k)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the base case: cursors from a search's own list, every query of a tile at a depth of its own
@pytest.mark.parametrize("k", [10, 2048])
def test_per_query_cursors_under_per_query_masks(k, oracle):
    x, q, S = scores("base", oracle)
    idx = _index(D, x)
    sD, sI = idx.search(q, MAX_K)
    j = after_cases.per_query_depths()
    after = (np.ascontiguousarray(sD[np.arange(NQ), j]), np.ascontiguousarray(sI[np.arange(NQ), j]))
    ref = masked_after_cases.own_depth_cursors(S)
    np.testing.assert_array_equal(after[1], ref[1])
    np.testing.assert_array_equal(after_ref.bits(after[0]), after_ref.bits(ref[0]))
    per_query = masked_cases.per_query_masks()
    all_forms(idx, q, per_query, None, after, k, want_of(S, per_query, None, after, k), "a mask per query")
    plan = parse_plan(idx.last_plan())
    QT, C, lds = expected_tile(D, k, NQ)
    tiles = -(-NQ // QT)
    assert QT == (16 if k == 10 else 4)
    assert (plan["QT"], plan["C"], plan["lds"], plan["T"], plan["gt"], plan["launches"], plan["W"]) == (QT, C, lds, tiles, tiles, 1, 4), plan
    grouped, mask_of = masked_cases.grouped_masks()
    all_forms(idx, q, grouped, mask_of, after, k, want_of(S, grouped, mask_of, after, k), "five masks")
    all_forms(idx, q, grouped[2], None, after, k, want_of(S, grouped[2], None, after, k), "one mask")


@pytest.mark.parametrize("k", masked_after_cases.K_EDGES)
def test_all_ones_mask_is_search_after_and_start_cursor_is_search_masked(k, oracle):
    x, q, S = scores("base", oracle)
    idx = _index(D, x)
    ones = np.ones(N, np.bool_)
    after = masked_after_cases.own_depth_cursors(S)
    # an all-ones mask: search_after, its reference and its kernel's own output
    want = after_ref.after_from_scores(S, after[0], after[1], k)
    parent = idx.search_after(q, k, after)
    assert "scan16_after_kernel" in idx.last_plan()
    after_ref.assert_same(parent, want, f"search_after k={k}")
    all_forms(idx, q, ones, None, after, k, want, f"all ones k={k}")
    all_forms(idx, q, np.tile(ones, (3, 1)), (np.arange(NQ) % 3).astype(np.int64), after, k, want, f"three all-ones masks k={k}")
    # the start cursor -- row -2, all-ones keys, None -- : search_masked, its reference and its kernel's own output
    per_query = masked_cases.per_query_masks()
    want = masked_ref.masked_from_scores(S, per_query, None, k)
    parent = idx.search_masked(q, k, per_query)
    assert "scan16_masked_kernel" in idx.last_plan()
    masked_ref.assert_same(parent, want, f"search_masked k={k}")
    all_forms(idx, q, per_query, None, None, k, want, f"start k={k}")
    assert "scan16_masked_after_kernel" in idx.last_plan()
    import torch
    from haconvdr_amd import _lib
    qt, wt = _cuda(q, np.float32), _cuda(_words(per_query, N), np.int64)
    keys = torch.zeros((NQ, k), dtype=torch.int64, device="cuda")
    Dt, It = torch.zeros((NQ, k), device="cuda"), torch.zeros((NQ, k), dtype=torch.int64, device="cuda")
    L = _lib.lib()
    _lib.check(L.hac_index_search_masked_after_keys_device(idx._h, qt.data_ptr(), NQ, k, wt.data_ptr(), NQ, wt.shape[1], None, None, keys.data_ptr(), 0, None))
    _lib.check(L.hac_index_search_masked_after_device(idx._h, qt.data_ptr(), NQ, k, wt.data_ptr(), NQ, wt.shape[1], None, None, None, Dt.data_ptr(), It.data_ptr(),
                                                      None, None))
    torch.cuda.synchronize()
    masked_ref.assert_same(after_ref.unpack(keys.cpu().numpy()), want, "null after_keys_dev")
    masked_ref.assert_same((Dt.cpu().numpy(), It.cpu().numpy()), want, "null cursor pointers, device form")
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 2. paging
def _chain(idx, q, S, masks, mask_of, k, what):
    """pages chained through (D[:, -1], I[:, -1]) to the end of the masked set and one page beyond -> (D, I) of all pages"""
    longest = max(len(rows) for _, rows in masked_after_ref.unbounded(S, masks, mask_of))
    after, Ds, Is = None, [], []
    for page in range(longest // k + 2):
        want = want_of(S, masks, mask_of, after, k)
        got = host_form(idx, q, masks, mask_of, after, k) if page % 2 else tensor_form(idx, q, masks, mask_of, after, k)
        masked_after_ref.assert_same(got, want, f"{what} page {page}")
        Ds.append(got[0])
        Is.append(got[1])
        after = (got[0][:, -1].copy(), got[1][:, -1].copy())
    assert (Is[-1] == -1).all() and (Ds[-1] == -FMAX).all()               # behind a padding cursor: padding
    idx.check_status()
    return np.concatenate(Ds, 1), np.concatenate(Is, 1)


def _assert_whole_list(Dc, Ic, S, masks, mask_of, idx, q):
    whole = masked_after_ref.unbounded(S, masks, mask_of)
    for i, (sc, rows) in enumerate(whole):
        m = len(rows)
        np.testing.assert_array_equal(Ic[i, :m], rows)                     # nothing twice, nothing missing, in order
        np.testing.assert_array_equal(after_ref.bits(Dc[i, :m]), after_ref.bits(sc))
        assert (Ic[i, m:] == -1).all()
    # rank_ids of the pages' entries is consistent with their order: ranks ascend strictly along every list
    ranks = idx.rank_ids(q, np.ascontiguousarray(Ic[:, :256]))
    for i, (sc, rows) in enumerate(whole):
        m = min(256, len(rows))
        assert (np.diff(ranks[i, :m]) > 0).all() and (ranks[i, :m] >= 0).all() and (ranks[i, m:] == -1).all()


def test_pages_chained_over_hostile_rows(oracle):
    x, q, S = scores("hostile", oracle)
    n = S.shape[1]
    idx = _index(after_cases.HOSTILE_D, x)
    masks = masked_cases.random_masks(0xD40, 3, n, 4)
    for r in (20, 21, 40, 4001, 3, 13, 23, 33):                            # +-Inf-, NaN-scoring rows selected by some masks, deselected by others
        masks[:, r] = np.arange(3) % 2 == r % 2
    masks[2, 60:64] = masks[2, 64:70] = True
    mask_of = (np.arange(len(q)) % 3).astype(np.int64)
    sel = masks[mask_of]
    assert (sel & np.isnan(S)).any() and (sel & (S == -np.inf)).any() and (~sel & (S == -np.inf)).any() and (sel & (S == np.inf)).any()
    Dc, Ic = _chain(idx, q, S, masks, mask_of, 500, "hostile")
    _assert_whole_list(Dc, Ic, S, masks, mask_of, idx, q)


def test_pages_chained_inside_runs_of_equal_scores_partly_deselected(oracle):
    x, q, S = scores("tie", oracle)
    n = S.shape[1]
    idx = _index(after_cases.TIE_D, x)
    r = np.arange(n)
    masks = np.stack([r % 3 != 0, (r % 16 == 5) | (r % 16 == 6) | (r % 16 == 11), masked_cases.random_masks(0xD41, 1, n, 2)[0]])
    mask_of = (np.arange(len(q)) % 3).astype(np.int64)
    for k in (7, 100):
        Dc, Ic = _chain(idx, q, S, masks, mask_of, k, f"tie k={k}")
        _assert_whole_list(Dc, Ic, S, masks, mask_of, idx, q)
        inside = sum(int(Dc[i, p - 1] == Dc[i, p] and Ic[i, p] >= 0) for i in range(len(q)) for p in range(k, Dc.shape[1], k))
        assert inside >= 0.8 * sum(len(rows) // k for _, rows in masked_after_ref.unbounded(S, masks, mask_of))   # page boundaries inside runs of equal scores
    # the run the boundary falls into is partly deselected: some row between two neighbours of a page seam is left out
    whole = masked_after_ref.unbounded(S, masks, mask_of)
    assert any(whole[i][1][p] - whole[i][1][p - 1] > 1 and whole[i][0][p] == whole[i][0][p - 1] for i in range(len(q)) for p in range(100, len(whole[i][1]), 100))


def test_cursor_edges_mixed_inside_one_tile(oracle):
    x, q6, S6 = scores("hostile", oracle)
    pick, masks, sc, rw = masked_after_cases.edge_case(S6)
    q, S = q6[pick], S6[pick]
    idx = _index(after_cases.HOSTILE_D, x)
    for k in (1, 40, 300):
        all_forms(idx, q, masks, None, (sc, rw), k, want_of(S, masks, None, (sc, rw), k), f"edges k={k}")
    assert parse_plan(idx.last_plan())["T"] == 1
    # a row below -2: the device forms answer with an empty list, next to healthy neighbours
    wild = rw.copy()
    wild[12], wild[13] = -3, np.iinfo(np.int64).min
    want = want_of(S, masks, None, (sc, wild), 40)
    assert (want[1][12:14] == -1).all() and (want[1][14:, 0] >= 0).all()
    masked_after_ref.assert_same(tensor_form(idx, q, masks, None, (sc, wild), 40), want, "rows below -2: empty lists, tensor form")
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 3. empty tiles
@pytest.mark.parametrize("k", [10, 2048])
def test_a_tile_whose_masks_select_nothing(k, oracle):
    x, q, S = scores("base", oracle)
    idx = _index(D, x)
    masks, mask_of = masked_after_cases.empty_tile_masks()
    live = masked_after_cases.own_depth_cursors(S)
    for name, after in (("a live cursor", live), ("the start", None)):
        want = want_of(S, masks, mask_of, after, k)
        assert (want[1][16:32] == -1).all() and (want[1][:16, 0] >= 0).all() and (want[1][32:, 0] >= 0).all()
        all_forms(idx, q, masks, mask_of, after, k, want, name)
    # every tile empty
    none = np.zeros(N, np.bool_)
    all_forms(idx, q, none, None, live, k, want_of(S, none, None, live, k), "no row selected")
    # a mask selecting only rows ahead of the cursor: all padding
    ahead = masked_after_cases.rows_ahead_masks(S, 60, 50)
    c60 = masked_after_cases.cursors_at(S, np.full(NQ, 60))
    want = want_of(S, ahead, None, c60, k)
    assert (want[1] == -1).all()
    all_forms(idx, q, ahead, None, c60, k, want, "rows ahead of the cursor only")


# ---------------------------------------------------------------------------------------------------------------------
# 4. thresholds: one workgroup walks every group through its compactions (masked_p = 1), then other plans, identical bytes
@pytest.mark.parametrize("ascending", [False, True])
def test_thresholds_come_from_eligible_rows_only(ascending, oracle):
    x, q, S = scores("ascending" if ascending else "descending", oracle)
    _, _, mask = masked_after_cases.threshold_case(ascending)
    after = masked_after_cases.threshold_cursors(S)
    idx = _index(D, x, masked_p="1")
    for k in masked_after_cases.THRESHOLD_KS:
        want = want_of(S, mask, None, after, k)
        assert (want[1] >= 0).all()
        by_plan = {}
        for p in ("1", "auto", "7"):
            idx.set_option("masked_p", p)
            all_forms(idx, q, mask, None, after, k, want, f"ascending={ascending} k={k} masked_p={p}")
            plan = parse_plan(idx.last_plan())
            assert plan["C"] == 512 and (plan["P"] == 1 if p == "1" else plan["P"] == 7 if p == "7" else plan["P"] > 1), plan
            by_plan[p] = keys_form(idx, q, mask, None, after_ref.cursor_keys(*after), k).tobytes()
        assert by_plan["1"] == by_plan["auto"] == by_plan["7"]


# ---------------------------------------------------------------------------------------------------------------------
# 5. launch cuts
@pytest.mark.parametrize("k", [10, 2048])
def test_launch_cuts_with_per_query_masks_and_cursors(k, oracle):
    x, q, S = scores("base", oracle)
    idx = _index(D, x)
    QT = expected_tile(D, k, NQ)[0]
    tiles = -(-NQ // QT)
    per_query = masked_cases.per_query_masks()
    after = masked_after_cases.own_depth_cursors(S)
    ak = after_ref.cursor_keys(*after)
    want = want_of(S, per_query, None, after, k)
    all_forms(idx, q, per_query, None, after, k, want, "one launch")
    assert parse_plan(idx.last_plan())["launches"] == 1
    single = keys_form(idx, q, per_query, None, ak, k).tobytes()
    grouped, mask_of = masked_cases.grouped_masks()
    for cut in (2, 1):
        idx.set_option("debug_masked_tiles", str(cut))
        all_forms(idx, q, per_query, None, after, k, want, f"{cut} tiles per launch")
        plan = parse_plan(idx.last_plan())
        assert plan["T"] == plan["gt"] == cut and plan["launches"] == -(-tiles // cut) and plan["launches"] >= 2, plan
        assert keys_form(idx, q, per_query, None, ak, k).tobytes() == single
        all_forms(idx, q, grouped, mask_of, after, k, want_of(S, grouped, mask_of, after, k), f"mask_of across the cut, {cut} tiles per launch")


def test_more_queries_than_one_query_chunk(oracle):
    x, q, masks, mask_of, depths = masked_after_cases.chunk_case()
    with np.errstate(all="ignore"):
        S = rank_ref.canon_scores(oracle, x, q)
    after = masked_after_cases.cursors_at(S, depths)
    k = masked_after_cases.CHUNK_K
    idx = _index(D, x)
    want = want_of(S, masks, mask_of, after, k)
    all_forms(idx, q, masks, mask_of, after, k, want, "1030 queries")
    plan = parse_plan(idx.last_plan())
    assert plan["launches"] == 2 and plan["T"] == 64 and plan["QT"] == 16, plan
    per_query = masked_cases.random_masks(0xD50, len(q), len(x), 3)         # query i uses mask i: the second launch starts at mask 1024
    all_forms(idx, q, per_query, None, after, k, want_of(S, per_query, None, after, k), "1030 masks")


# ---------------------------------------------------------------------------------------------------------------------
# 6. plan and dimension edges
def test_k_2048_at_d_768(oracle):
    from tests.golden import cases
    n, nq, k = 2500, 9, 2048
    x, q, _ = cases.search_case_inputs("gauss", 0xD60, n, nq, d=768)
    S = rank_ref.canon_scores(oracle, x, q)
    idx = _index(768, x)
    masks = masked_cases.random_masks(0xD61, nq, n, 2)
    masks[:, 1000:1700] = True                                             # lists longer than a page behind the cursor: the page is full
    after = masked_after_cases.cursors_at(S, (np.arange(nq) * 29) % 200)
    want = want_of(S, masks, None, after, k)
    all_forms(idx, q, masks, None, after, k, want, "k=2048 d=768")
    plan = parse_plan(idx.last_plan())
    assert plan["QT"] == 4 and plan["C"] == 4096 and plan["T"] == 3, plan
    assert (want[1][:, 900] >= 0).all()


@pytest.mark.parametrize("d, n, nq", [(32, 200, 3), (96, 1000, 17), (160, 1000, 17)])
def test_dimension_edges(d, n, nq, oracle):
    """d = 32: K4 == PF, the zero-trip edge of scan16_group_mfma; d = 96 and 160: d % 64 == 32"""
    from tests.test_index_rank_gpu import hostile_queries
    from tests.test_index_rows_gpu import hostile_corpus
    x = hostile_corpus(0xD70 + d, n, d)
    q = hostile_queries(0xD71 + d, nq, d)
    with np.errstate(all="ignore"):
        S = rank_ref.canon_scores(oracle, x, q)
    masks = masked_cases.random_masks(0xD72 + d, nq, n, 2)
    masks[:, 3:n:10] = True                                                # raw-word rows: NaN scores among the selected
    idx = _index(d, x)
    after = masked_after_cases.cursors_at(S, (np.arange(nq) * 13) % 60)
    for k in (1, 50):
        all_forms(idx, q, masks, None, after, k, want_of(S, masks, None, after, k), f"d={d} k={k}")
        all_forms(idx, q, masks, None, None, k, want_of(S, masks, None, None, k), f"d={d} k={k} start")


# ---------------------------------------------------------------------------------------------------------------------
# 7. the keys form
@pytest.mark.parametrize("pos_base", [0, 2 ** 24 - 300, 2 ** 32 - 1 - 1000])
def test_keys_form_in_the_position_space_of_pos_base(pos_base, oracle):
    import torch
    x, q, S = scores("tie", oracle)
    nq, n = S.shape
    assert pos_base + n <= 2 ** 32 - 1 and (pos_base == 0 or pos_base + n == 2 ** 32 - 1 or pos_base < 2 ** 24 < pos_base + n)
    idx = _index(after_cases.TIE_D, x)
    r = np.arange(n)
    masks = np.stack([r % 3 != 1, masked_cases.random_masks(0xD80, 1, n, 2)[0]])
    mask_of = (np.arange(nq) % 2).astype(np.int64)
    k = 61
    cursor = None
    for page in range(4):                                                  # the last column fed back as after_keys
        want = masked_after_ref.from_keys(S, masks, mask_of, cursor, pos_base, k)
        got = keys_form(idx, q, masks, mask_of, cursor, k, pos_base)
        np.testing.assert_array_equal(got, want, err_msg=f"pos_base={pos_base} page {page}")
        cursor = got[:, -1].copy()
    whole = masked_after_ref.unbounded(S, masks, mask_of)
    for i in range(nq):
        np.testing.assert_array_equal(after_ref.unpack(want, pos_base)[1][i], whole[i][1][3 * k:4 * k])
    # a (score, row) cursor packed in that space
    from haconvdr_amd.index import cursor_keys
    sc, rw = masked_after_cases.cursors_at(S, np.full(nq, 200))
    ck = cursor_keys(sc, rw, pos_base)
    np.testing.assert_array_equal(keys_form(idx, q, masks, mask_of, ck, k, pos_base), masked_after_ref.from_keys(S, masks, mask_of, ck, pos_base, k))
    # positions past 32 bits are refused
    if pos_base + n == 2 ** 32 - 1:
        from haconvdr_amd import _lib
        with pytest.raises(_lib.HacError):
            idx.search_masked_keys_tensor(_cuda(q, np.float32), k, _cuda(_words(masks, n), np.int64), _cuda(mask_of, np.int64), pos_base=pos_base + 1,
                                          after_keys=_cuda(ck, np.int64))
        torch.cuda.synchronize()
    idx.check_status()


def test_keys_form_feeds_merge_keys_and_id_map(oracle):
    """two indexes hold the two halves of a corpus, each under its slice of the masks with pos_base = its first row and the same
    cursor: merged, the keys are those of one index over the whole corpus, and their last column is the next page's cursor"""
    import torch
    from haconvdr_amd.index import keys_to_results, merge_keys
    from tests.golden import cases
    d, n, nq, k = 96, 1501, 7, 60
    x, q, ids = cases.search_case_inputs("dup", 0xD90, n, nq, d=d)        # row r and row r + 750 are twins: ties cross the cut
    cut = 751
    S = rank_ref.canon_scores(oracle, x, q)
    r = np.arange(n)
    masks = np.stack([(r % 750) % 3 != 1, (r >= cut - 200) & (r < cut + 180)])
    mask_of = (np.arange(nq) % 2).astype(np.int64)
    lo, hi, one = _index(d, x[:cut]), _index(d, x[cut:]), _index(d, x)
    qt, mt, idt = _cuda(q, np.float32), _cuda(mask_of, np.int64), _cuda(ids, np.int64)
    w_lo, w_hi = _cuda(_words(masks[:, :cut], cut), np.int64), _cuda(_words(masks[:, cut:], n - cut), np.int64)
    cursor = torch.full((nq,), -1, dtype=torch.int64, device="cuda")
    for page in range(3):
        k_lo = lo.search_masked_keys_tensor(qt, k, w_lo, mt, pos_base=0, after_keys=cursor)
        k_hi = hi.search_masked_keys_tensor(qt, k, w_hi, mt, pos_base=cut, after_keys=cursor)
        merged = merge_keys(torch.stack([k_lo, k_hi]))
        Dm, Im = keys_to_results(merged, id_map=idt)
        torch.cuda.synchronize()
        want = masked_after_ref.from_keys(S, masks, mask_of, cursor.cpu().numpy(), 0, k)
        np.testing.assert_array_equal(merged.cpu().numpy().view(np.uint64), want)
        wD, wI = after_ref.unpack(want)
        masked_after_ref.assert_same((Dm.cpu().numpy(), Im.cpu().numpy()), (wD, np.where(wI >= 0, ids[np.maximum(wI, 0)], -1)), f"two shards merged, page {page}")
        cursor = merged[:, -1].contiguous()
    # id_map through the tensor form: it remaps the result, the cursor rows stay the index's own rows
    after = masked_after_cases.cursors_at(S, np.full(nq, 40))
    wD, wI = want_of(S, masks, mask_of, after, k)
    masked_after_ref.assert_same(tensor_form(one, q, masks, mask_of, after, k, id_map=idt), (wD, np.where(wI >= 0, ids[np.maximum(wI, 0)], -1)), "id_map")
    for i in (lo, hi, one):
        i.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 8. non-finite queries
@pytest.mark.parametrize("kind", nonfinite.KINDS)
def test_nonfinite_queries(kind, oracle):
    d, n, nq, k = 96, 3001, 33, 100
    x, q, pos, base = nonfinite.case(kind, d, n, nq, 0xDA0)
    with np.errstate(all="ignore"):
        S = rank_ref.canon_scores(oracle, x, q)
        Sb = rank_ref.canon_scores(oracle, x, base)
    masks = masked_cases.random_masks(0xDA1, 3, n, 2)
    mask_of = (np.arange(nq) % 3).astype(np.int64)
    after = masked_after_cases.cursors_at(Sb, (np.arange(nq) * 17) % 300)  # cursors from the healthy batch's lists: finite scores, real rows
    want = want_of(S, masks, mask_of, after, k)
    if kind in nonfinite.NAN_KINDS:
        assert all((want[1][i] == -1).all() for i in pos)                 # a NaN query: padding only
    healthy = [i for i in range(nq) if i not in pos]
    assert (want[1][healthy] >= 0).all()
    idx = _index(d, x)
    all_forms(idx, q, masks, mask_of, after, k, want, kind)
    all_forms(idx, q, masks, mask_of, None, k, want_of(S, masks, mask_of, None, k), f"{kind} start")


# ---------------------------------------------------------------------------------------------------------------------
# 9. index lifetimes
def test_after_reset_and_a_smaller_add_no_stale_row_of_the_last_group(oracle):
    n2 = index_lifetime.B_N2[0]
    x1, x2, _, q, _ = index_lifetime.case_b(n2)                            # life 1: hostile rows at [n2, n2 + 200); life 2: n2 = 257 rows
    q = q[:9]
    idx = _index(768, x1)
    ones1 = np.ones(len(x1), np.bool_)
    with np.errstate(all="ignore"):
        S1 = rank_ref.canon_scores(oracle, x1, q)
    a1 = masked_after_cases.cursors_at(S1, np.full(len(q), 5))
    all_forms(idx, q, ones1, None, a1, 20, want_of(S1, ones1, None, a1, 20), "life 1")
    idx.reset()
    idx.add(x2)
    assert idx.ntotal == n2 and n2 % 64 == 1
    S2 = rank_ref.canon_scores(oracle, x2, q)
    words = np.full((n2 + 63) // 64, -1, np.int64)                         # all ones, the 63 bits past row 256 too
    for depth in (0, 200):
        a2 = masked_after_cases.cursors_at(S2, np.full(len(q), depth))
        want = want_of(S2, np.ones(n2, np.bool_), None, a2, 300)
        assert (want[1][:, :n2 - 1 - depth] >= 0).all() and (want[1][:, n2 - 1 - depth:] == -1).all()
        all_forms(idx, q, words, None, a2, 300, want, f"after reset and a smaller add, depth {depth}")
    all_forms(idx, q, words, None, None, 300, want_of(S2, np.ones(n2, np.bool_), None, None, 300), "after reset, the start")
    idx.reset()                                                            # an empty index: padding only, words == 0
    pad = (np.full((len(q), 4), -FMAX, np.float32), np.full((len(q), 4), -1, np.int64))
    all_forms(idx, q, np.zeros((1, 0), np.int64), None, a2, 4, pad, "empty index")


def test_after_remove_ids_a_mask_of_the_old_length_is_refused(oracle):
    import ctypes
    from haconvdr_amd import _lib, synth
    from haconvdr_amd.index import _f32p, _i64p, pack_mask
    d, n, nq, k = 96, 1000, 5, 50
    x = synth.embeddings(0xDB0, n, d)
    q = synth.embeddings(0xDB1, nq, d)
    idx = _index(d, x)
    mask = masked_cases.random_masks(0xDB2, 1, n, 3)[0]
    S = rank_ref.canon_scores(oracle, x, q)
    after = masked_after_cases.cursors_at(S, np.full(nq, 30))
    all_forms(idx, q, mask, None, after, k, want_of(S, mask, None, after, k), "as built")
    old_words = pack_mask(mask)
    gone = np.arange(100, 900, 7)
    assert idx.remove_ids(gone) == len(gone)
    left = np.delete(x, gone, 0)
    assert len(old_words) != (len(left) + 63) // 64
    with pytest.raises(ValueError):
        idx.search_masked(q, k, old_words, after=after)
    Dh, Ih = np.full((nq, k), np.float32(-123.5)), np.full((nq, k), -99, np.int64)
    L = _lib.lib()
    rc = L.hac_index_search_masked_after(idx._h, _f32p(q), nq, k, old_words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 1, len(old_words), None,
                                         _f32p(after[0]), _i64p(after[1]), _f32p(Dh), _i64p(Ih))
    assert rc == HAC_ERR_INVALID and "words=" in L.hac_last_error().decode() and (Dh == np.float32(-123.5)).all() and (Ih == -99).all()
    qt, wt = _cuda(q, np.float32), _cuda(old_words, np.int64)
    assert L.hac_index_search_masked_after_device(idx._h, qt.data_ptr(), nq, k, wt.data_ptr(), 1, len(old_words), None, None, None, None, None, None,
                                                  None) == HAC_ERR_INVALID
    assert L.hac_index_search_masked_after_keys_device(idx._h, qt.data_ptr(), nq, k, wt.data_ptr(), 1, len(old_words), None, None, None, 0, None) == HAC_ERR_INVALID
    kept = np.delete(mask, gone)                                           # a fresh mask, and cursors in the new numbering
    Sl = rank_ref.canon_scores(oracle, left, q)
    after = masked_after_cases.cursors_at(Sl, np.full(nq, 30))
    all_forms(idx, q, kept, None, after, k, want_of(Sl, kept, None, after, k), "after remove_ids")


def test_errors(oracle):
    import ctypes
    import torch
    from haconvdr_amd import _lib
    from haconvdr_amd.index import _f32p, _i64p
    x, q, S = scores("base", oracle)
    idx = _index(D, x)
    k = 10
    L = _lib.lib()
    grouped, mask_of = masked_cases.grouped_masks()
    w = _words(grouped, N)
    wp = w.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    sc, rows = np.zeros(NQ, np.float32), np.arange(NQ, dtype=np.int64)
    Dh, Ih = np.full((NQ, k), np.float32(-123.5)), np.full((NQ, k), -99, np.int64)
    null_f, null_i = ctypes.POINTER(ctypes.c_float)(), ctypes.POINTER(ctypes.c_int64)()
    # the host form refuses, names the query and writes nothing: a mask_of entry outside [0, n_masks), a cursor row below -2,
    # one cursor pointer without the other
    for at, bad in ((16, 5), (3, -1)):
        one = mask_of.copy()
        one[at] = bad
        with pytest.raises(_lib.HacError) as err:
            idx.search_masked(q, k, grouped, one, after=(sc, rows))
        assert err.value.code == HAC_ERR_INVALID and f"query {at}" in str(err.value) and f"{bad}" in str(err.value), str(err.value)
    for at, bad in ((16, -3), (3, np.iinfo(np.int64).min)):
        one = rows.copy()
        one[at] = bad
        with pytest.raises(_lib.HacError) as err:
            _lib.check(L.hac_index_search_masked_after(idx._h, _f32p(q), NQ, k, wp, 5, w.shape[1], _i64p(mask_of), _f32p(sc), _i64p(one), _f32p(Dh), _i64p(Ih)))
        assert err.value.code == HAC_ERR_INVALID and f"query {at}" in str(err.value) and f"{bad}" in str(err.value), str(err.value)
    assert L.hac_index_search_masked_after(idx._h, _f32p(q), NQ, k, wp, 5, w.shape[1], _i64p(mask_of), _f32p(sc), null_i, _f32p(Dh), _i64p(Ih)) == HAC_ERR_INVALID
    assert L.hac_index_search_masked_after(idx._h, _f32p(q), NQ, k, wp, 5, w.shape[1], _i64p(mask_of), null_f, _i64p(rows), _f32p(Dh), _i64p(Ih)) == HAC_ERR_INVALID
    for k_, n_masks_ in ((0, 5), (MAX_K + 1, 5), (k, 0)):
        assert L.hac_index_search_masked_after(idx._h, _f32p(q), NQ, k_, wp, n_masks_, w.shape[1], _i64p(mask_of), null_f, null_i, _f32p(Dh),
                                               _i64p(Ih)) == HAC_ERR_INVALID
    assert L.hac_index_search_masked_after(idx._h, _f32p(q), NQ, k, wp, 5, w.shape[1], null_i, null_f, null_i, _f32p(Dh), _i64p(Ih)) == HAC_ERR_INVALID
    assert (Dh == np.float32(-123.5)).all() and (Ih == -99).all()
    # the device forms give such queries an empty list and no error
    wild_of, wild_rows = mask_of.copy(), rows.copy()
    wild_of[3], wild_of[20] = -1, 5
    wild_rows[16], wild_rows[36] = -3, -1000
    want = want_of(S, grouped, wild_of, (sc, wild_rows), k)
    assert all((want[1][i] == -1).all() for i in (3, 20, 16, 36)) and (want[1][[0, 4, 17, 35], 0] >= 0).all()
    masked_after_ref.assert_same(tensor_form(idx, q, grouped, wild_of, (sc, wild_rows), k), want, "device form")
    qt, wt, mt, st, rt = _cuda(q, np.float32), _cuda(w, np.int64), _cuda(mask_of, np.int64), _cuda(sc, np.float32), _cuda(rows, np.int64)
    out_d, out_i = torch.empty((NQ, k), device="cuda"), torch.empty((NQ, k), dtype=torch.int64, device="cuda")
    assert L.hac_index_search_masked_after_device(idx._h, qt.data_ptr(), NQ, k, wt.data_ptr(), 5, w.shape[1], mt.data_ptr(), st.data_ptr(), None, out_d.data_ptr(),
                                                  out_i.data_ptr(), None, None) == HAC_ERR_INVALID
    # argument mistakes on real CUDA tensors: ValueError before the library is called
    for args, kw in (((qt, 0, wt, mt), dict(after=(st, rt))), ((qt, k, wt[:, :-1], mt), dict(after=(st, rt))), ((qt, k, wt, mt[:-1]), dict(after=(st, rt))),
                     ((qt, k, wt, mt), dict(after=(st[:-1], rt))), ((qt, k, wt, mt), dict(after=(st, rt.int()))), ((qt, k, wt, mt), dict(after=(st.double(), rt))),
                     ((qt, k, wt, mt), dict(after=(st.cpu(), rt))), ((qt, k, wt, mt), dict(after=(st,))), ((qt, k, wt, None), dict(after=(st, rt)))):
        with pytest.raises(ValueError):
            idx.search_masked_tensor(*args, **kw)
    for args, kw in (((qt, k, wt, mt), dict(after_keys=rt[:-1])), ((qt, k, wt, mt), dict(after_keys=rt.int())), ((qt, k, wt, mt), dict(after_keys=rt.cpu())),
                     ((qt, k, wt, mt), dict(after_keys=rt, pos_base=-1)), ((qt, k, wt, mt), dict(after_keys=rt, pos_base=2 ** 32)),
                     ((qt, MAX_K + 1, wt, mt), dict(after_keys=rt))):
        with pytest.raises(ValueError):
            idx.search_masked_keys_tensor(*args, **kw)
    after = masked_after_cases.own_depth_cursors(S)
    all_forms(idx, q, grouped, mask_of, after, k, want_of(S, grouped, mask_of, after, k), "after the refused calls")
    # nq == 0: HAC_OK, nothing touched
    D0, I0 = idx.search_masked(np.zeros((0, D), np.float32), 7, grouped[0], after=(np.zeros(0, np.float32), np.zeros(0, np.int64)))
    assert D0.shape == I0.shape == (0, 7)
    assert tuple(idx.search_masked_keys_tensor(torch.zeros((0, D), device="cuda"), 7, wt[:1], after_keys=torch.zeros(0, dtype=torch.int64, device="cuda")).shape) == (0, 7)
    # the device forms on a multi-device index
    two = _index(D, x[:500], devices=(0, 0))
    w2 = _cuda(_words(grouped[:, :500], 500), np.int64)
    for call in (lambda: two.search_masked_tensor(qt, k, w2, mt, after=(st, rt)), lambda: two.search_masked_keys_tensor(qt, k, w2, mt, after_keys=rt)):
        with pytest.raises(_lib.HacError) as err:
            call()
        assert err.value.code == HAC_ERR_UNSUPPORTED
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 10. several shards in one process
def test_two_shards_on_one_gpu(oracle):
    x, q, S = scores("tie", oracle)
    nq, n = S.shape
    idx = _index(after_cases.TIE_D, x, devices=(0, 0))
    one = _index(after_cases.TIE_D, x)
    r = np.arange(n)
    c1, c2 = _cuts(n)
    edges = set()
    for a, b in ((0, c1), (c1, c2), (c2, n)):
        per = -(-(b - a) // 2)
        for s in range(3):
            e = min(b, a + s * per)
            edges.update(t for t in (e - 2, e - 1, e, e + 1) if 0 <= t < n)
    band = np.zeros(n, np.bool_)
    band[sorted(edges)] = True
    masks = np.stack([r % 3 != 1, band, ~band, masked_cases.random_masks(0xDC0, 1, n, 2)[0]])
    mask_of = (np.arange(nq) % 4).astype(np.int64)
    # pages chained across the shards: every score's run spans both, the masks are sliced span by span
    for k in (7, 100):
        after = None
        for page in range(4):
            want = want_of(S, masks, mask_of, after, k)
            got = host_form(idx, q, masks, mask_of, after, k)
            masked_after_ref.assert_same(got, want, f"two shards k={k} page {page}")
            masked_after_ref.assert_same(host_form(one, q, masks, mask_of, after, k), got, f"one device k={k} page {page}")
            after = (want[0][:, -1].copy(), want[1][:, -1].copy())
    # cursor rows on the first shard, on the second, on every span edge, at and above ntotal
    rows = np.array(sorted(edges) + [n, n + 7, 2 ** 32, 2 ** 40], np.int64)
    whole = after_ref.unbounded(S)
    for qi in (1, 0):
        qs, Ss = np.repeat(q[qi:qi + 1], len(rows), 0), np.repeat(S[qi:qi + 1], len(rows), 0)
        for m in (0, 2):
            top = (np.full(len(rows), whole[qi][0][0], np.float32), rows)
            masked_after_ref.assert_same(idx.search_masked(qs, 70, masks[m], after=top), want_of(Ss, masks[m], None, top, 70), f"query {qi}: edge rows at the best score")
            own = (np.where(rows < n, S[qi, np.minimum(rows, n - 1)], whole[qi][0][500]).astype(np.float32), rows)
            got = idx.search_masked(qs, 70, masks[m], after=own)
            masked_after_ref.assert_same(got, want_of(Ss, masks[m], None, own, 70), f"query {qi}: edge rows at their own score")
            masked_after_ref.assert_same(one.search_masked(qs, 70, masks[m], after=own), got, "one device")
    # exhausted, start, NaN and +-Inf cursors on both shards alike
    sc = np.array([0, 0, np.nan, np.inf, -np.inf, -0.0], np.float32)
    rw = np.array([-1, -2, 4, 0, 0, 998], np.int64)
    want = want_of(S, masks, mask_of, (sc, rw), 30)
    assert (want[1][0] == -1).all() and (want[1][2] == -1).all() and (want[1][4] == -1).all() and (want[1][3] >= 0).all()
    masked_after_ref.assert_same(idx.search_masked(q, 30, masks, mask_of, after=(sc, rw)), want, "special cursors")
    # search_after's own results through the function the two host calls now share
    a = masked_after_cases.cursors_at(S, np.full(nq, 123))
    after_ref.assert_same(idx.search_after(q, 50, a), after_ref.after_from_scores(S, a[0], a[1], 50), "search_after on two shards")
    from haconvdr_amd import _lib
    bad = mask_of.copy()
    bad[4] = 4
    with pytest.raises(_lib.HacError) as err:
        idx.search_masked(q, 10, masks, bad, after=(sc, rw))
    assert err.value.code == HAC_ERR_INVALID and "query 4" in str(err.value)
    idx.check_status()
    one.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 11. captured into a graph
def test_captured_into_a_graph_replays_on_the_previous_pages_last_column(oracle):
    import torch
    x, q, S = scores("hostile", oracle)
    nq, n, k = len(q), S.shape[1], 64
    idx = _index(after_cases.HOSTILE_D, x)
    masks = masked_cases.random_masks(0xDD0, 2, n, 2)
    mask_of = (np.arange(nq) % 2).astype(np.int64)
    qt, wt, mt = _cuda(q, np.float32), _cuda(_words(masks, n), np.int64), _cuda(mask_of, np.int64)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()                            # a single stream: no parallel branches in the graph
    pages = []
    with torch.cuda.stream(side):
        first = idx.search_masked_keys_tensor(qt, k, wt, mt, after_keys=torch.full((nq,), -1, dtype=torch.int64, device="cuda"))   # the largest shape once, eagerly
        cursor = first[:, -1].clone()
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            keys = idx.search_masked_keys_tensor(qt, k, wt, mt, after_keys=cursor)
        for _ in range(3):
            keys.zero_()
            g.replay()
            side.synchronize()
            pages.append(keys.cpu().numpy().view(np.uint64).copy())
            cursor.copy_(keys[:, -1])
    torch.cuda.synchronize()
    want = masked_after_ref.from_keys(S, masks, mask_of, None, 0, 4 * k)
    np.testing.assert_array_equal(first.cpu().numpy().view(np.uint64), want[:, :k])
    for p, got in enumerate(pages):
        np.testing.assert_array_equal(got, want[:, (p + 1) * k:(p + 2) * k], err_msg=f"replay {p}: page {p + 2}")
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 12. ResidentCorpus and ShardedSearcher
def test_resident_corpus_search_deep_and_behind_within(tmp_path, oracle):
    from haconvdr_amd.passages import write_embedding_block
    from haconvdr_amd.search import ResidentCorpus
    from tests.golden import cases
    n, nq, depth = 5200, 5, 2300
    x, q, _ = cases.search_case_inputs("gauss", 0xDE0, n, nq)
    ids = (np.arange(n, dtype=np.int64) * 7 + 11)[::-1].copy()
    for b, (lo, hi) in enumerate(((0, 1800), (1800, 3600), (3600, n))):
        write_embedding_block(str(tmp_path), b, x[lo:hi], ids[lo:hi])
    rc = ResidentCorpus(str(tmp_path), passage_block_num=10)
    S = rank_ref.canon_scores(oracle, x, q)
    r = np.arange(n)
    two = np.stack([r % 2 == 0, r % 7 == 3])
    of = np.array([0, 1, 0, 1, 0])
    whole = masked_after_ref.unbounded(S, two, of)
    Dd, Id = rc.search_deep(q, depth, page=1024, within=two, within_of=of)
    assert Dd.shape == Id.shape == (nq, depth) and depth > MAX_K
    for i in range(nq):
        m = min(depth, len(whole[i][1]))
        np.testing.assert_array_equal(Id[i, :m], ids[whole[i][1][:m]])
        np.testing.assert_array_equal(Dd[i, :m], whole[i][0][:m].astype(np.float64))
        assert (Id[i, m:] == -1).all() and (Dd[i, m:] == np.float64(-FMAX)).all()
    assert len(whole[0][1]) > depth > len(whole[1][1])
    unmasked = after_ref.unbounded(S)
    at = np.array([0, 17, 2500, n - 1, 3])
    gold_rows = np.array([unmasked[i][1][at[i]] for i in range(nq)])
    Db, Ib = rc.behind(q, ids[gold_rows], 25, within=two, within_of=of)
    wD, wI = masked_after_ref.from_scores(S, two, of, S[np.arange(nq), gold_rows], gold_rows, 25)
    np.testing.assert_array_equal(Ib, np.where(wI >= 0, ids[np.maximum(wI, 0)], -1))
    np.testing.assert_array_equal(Db, wD.astype(np.float64))
    assert (Ib[3] == -1).all() and (Ib[0] >= 0).all()
    rc.index.check_status()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_search_masked_after_across_ranks_sharing_the_gpu(world):
    """`world` processes (tests/_gloo_worker_masked_after.py hip) each hold one contiguous shard of the tie corpus on the GPU,
    search their rows under their slice of the masks behind the same global-position cursor with pos_base = their shard's first
    row, all-gather the keys over gloo and merge on the device; each rank compares with the reference over the whole corpus."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_gloo_worker_masked_after.py")
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, script, "hip"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    try:
        outs = [p.communicate(timeout=300)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
        assert "OK" in o
