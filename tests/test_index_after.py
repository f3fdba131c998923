"""search_after, the parts that need no GPU: the C-ABI surface of the three entry points, the resource lines of
scan16_after_kernel, the identities of include/haconvdr.h ("search behind a cursor") proved over the oracle on the inputs of
tests/test_index_after_gpu.py (against masked_ref, range_ref and rank_ref), index.cursor_keys against the reference's packing,
proofs that those inputs show what they are for, the argument checks of the Python mirrors (ValueError before the library is
called, no handle needed), ResidentCorpus.search_deep / behind over a stand-in index, and ShardedSearcher.search_after over
gloo worlds of 2 and 3 ranks with a test double."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests import after_cases, after_ref, masked_ref, range_ref, rank_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("hac_index_search_after", "hac_index_search_after_device", "hac_index_search_after_keys_device")
FMAX = after_ref.FMAX
_CASES = {}


def scores(name, oracle):
    """(x, q, S) of the GPU tests' inputs, computed once and never changed"""
    if name not in _CASES:
        x, q = {"base": after_cases.base_case, "tie": after_cases.tie_case, "hostile": after_cases.hostile_case}[name]()
        with np.errstate(all="ignore"):
            S = rank_ref.canon_scores(oracle, x, q)
        S.setflags(write=False)
        _CASES[name] = (x, q, S)
    return _CASES[name]


# ---------------------------------------------------------------------------------------------------------------------
# 5. symbols, 6. registers
def test_new_entry_points_are_declared_listed_and_exported():
    from haconvdr_amd import _lib, index
    hdr = open(os.path.join(ROOT, "include", "haconvdr.h")).read()
    assert "search behind a cursor" in hdr and re.search(r"#define HAC_AFTER_START \(-2\)", hdr)
    assert _lib.HAC_AFTER_START == index.AFTER_START == after_ref.START == -2
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(hac_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()                      # dlopen only; nothing is computed
    for sym in NEW_SYMBOLS:
        assert sym in declared, sym
        assert sym in _lib.EXPORTED_SYMBOLS, sym
        f = getattr(L, sym)
        assert f.argtypes is not None and f.restype is not None, sym
        params = re.search(r"\b%s\s*\(([^)]*)\)" % sym, hdr).group(1)
        assert len(params.split(",")) == len(f.argtypes), sym
    assert [len(getattr(L, sym).argtypes) for sym in NEW_SYMBOLS] == [8, 10, 8]


def test_after_kernel_keeps_everything_in_registers():
    path = os.path.join(ROOT, "haconvdr_amd", "csrc", "flat_ip.resources.txt")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(path)])
    blocks = re.split(r"remark: Function Name: ", open(path).read())
    for kernel in ("scan16_after_kernel", "after_bounds_kernel"):
        mine = [b for b in blocks if re.search(r"\d+%s[A-Z]" % kernel, b.split("\n", 1)[0])]
        assert len(mine) == 1, (kernel, [b.split("\n", 1)[0] for b in mine])
        assert int(re.search(r"VGPRs: (\d+)", mine[0]).group(1)) <= 256, kernel
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", mine[0]).group(1)) == 0, kernel
        assert int(re.search(r"VGPRs Spill: (\d+)", mine[0]).group(1)) == 0, kernel


# ---------------------------------------------------------------------------------------------------------------------
# 1. the identities, on the GPU tests' inputs
def test_start_cursor_is_search(oracle):
    x, q, S = scores("base", oracle)
    for k in after_cases.START_KS:
        want = oracle.flat_ip_search(x, q, k)
        after_ref.assert_same(after_ref.after_from_scores(S, None, None, k), want, f"null cursors k={k}")
        after_ref.assert_same(after_ref.after_from_scores(S, np.full(len(q), np.nan, np.float32), np.full(len(q), -2, np.int64), k), want,
                              f"row -2 k={k}: the score is not read")
        after_ref.assert_same(after_ref.unpack(after_ref.after_from_keys(S, None, 0, k)), want, f"keys form k={k}")


def test_cursor_from_a_list_continues_it(oracle):
    x, q, S = scores("base", oracle)
    K = after_cases.K_MAX
    sD, sI = oracle.flat_ip_search(x, q, K)
    whole = after_ref.unbounded(S)
    for j in after_cases.CURSOR_JS:
        for k in after_cases.CURSOR_KS:
            D, I = after_ref.after_from_scores(S, sD[:, j], sI[:, j], k)
            fits = min(k, K - (j + 1))
            np.testing.assert_array_equal(I[:, :fits], sI[:, j + 1:j + 1 + fits])
            np.testing.assert_array_equal(after_ref.bits(D[:, :fits]), after_ref.bits(sD[:, j + 1:j + 1 + fits]))
            for i in range(len(q)):                                        # beyond K: the unbounded search goes on
                np.testing.assert_array_equal(I[i], whole[i][1][j + 1:j + 1 + k])
            # the key form of the same cursor: the last column of a sorted key list is the next page's cursor
            keys = after_ref.after_from_keys(S, after_ref.pack(sD[:, j], sI[:, j]), 0, k)
            after_ref.assert_same(after_ref.unpack(keys), (D, I), f"keys form j={j} k={k}")


def test_float_definition_is_the_key_comparison(oracle):
    """the two statements of the definition agree wherever both apply: (s < s_ref or (s == s_ref and r > b)) over non-NaN
    scores, and make_key(s, r) < make_key(s_ref, b) -- on hostile scores (+-Inf, +-0, denormals) and on long ties"""
    for name in ("hostile", "tie"):
        x, q, S = scores(name, oracle)
        n = S.shape[1]
        rng = np.random.default_rng(0xC01)
        for trial in range(6):
            rows = rng.integers(0, n, len(q))
            sc = S[np.arange(len(q)), rows].copy()
            if trial == 1:
                sc = -sc                                                    # scores no row may have; -0.0 for the zero query
            if trial == 2:
                rows = rows + n                                            # rows the index does not hold
            ok = ~np.isnan(sc)
            D, I = after_ref.after_from_scores(S[ok], sc[ok], rows[ok], 50)
            keys = after_ref.after_from_keys(S[ok], after_ref.cursor_keys(sc[ok], rows[ok]), 0, 50)
            after_ref.assert_same(after_ref.unpack(keys), (D, I), f"{name} trial {trial}")


@pytest.mark.parametrize("name, k", [("hostile", 1000), ("hostile", 2048), ("tie", 7), ("tie", 100)])
def test_chained_pages_are_the_unbounded_search(name, k, oracle):
    x, q, S = scores(name, oracle)
    nq, n = S.shape
    lims, rD, rI = range_ref.range_from_scores(S, np.float32(-np.inf))
    cursor = (None, None)
    pages = []
    for _ in range(n // k + 2):
        D, I = after_ref.after_from_scores(S, cursor[0], cursor[1], k)
        pages.append((D, I))
        cursor = (D[:, -1].copy(), I[:, -1].copy())
    assert (pages[-1][1] == -1).all() and (pages[-1][0] == -FMAX).all()   # the page after the end: padding only
    D, I = np.concatenate([p[0] for p in pages], 1), np.concatenate([p[1] for p in pages], 1)
    whole = after_ref.unbounded(S)
    for i in range(nq):
        m = int((~np.isnan(S[i])).sum())
        assert (I[i, :m] >= 0).all() and (I[i, m:] == -1).all() and len(set(I[i, :m].tolist())) == m      # every scored row once, then padding
        assert not np.isnan(S[i, I[i, :m]]).any()
        np.testing.assert_array_equal(I[i, :m], whole[i][1])
        np.testing.assert_array_equal(after_ref.bits(D[i, :m]), after_ref.bits(whole[i][0]))
        # range_search(q, -inf), then the rows scoring -Inf (which no radius admits)
        head = rI[lims[i]:lims[i + 1]]
        low = np.flatnonzero(S[i] == -np.inf)
        np.testing.assert_array_equal(I[i, :m], np.concatenate([head, low]))
        np.testing.assert_array_equal(after_ref.bits(D[i, :len(head)]), after_ref.bits(rD[lims[i]:lims[i + 1]]))


def test_ranks_of_a_page_follow_the_cursor(oracle):
    for name in ("hostile", "tie"):
        x, q, S = scores(name, oracle)
        nq = len(q)
        whole = after_ref.unbounded(S)
        for j, k in ((0, 5), (61, 100), (900, 64)):
            sc = np.array([whole[i][0][j] for i in range(nq)], np.float32)
            rw = np.array([whole[i][1][j] for i in range(nq)], np.int64)
            D, I = after_ref.after_from_scores(S, sc, rw, k)
            at = rank_ref.rank_ids_from_scores(S, rw[:, None])[:, 0]
            np.testing.assert_array_equal(at, j)
            np.testing.assert_array_equal(rank_ref.rank_ids_from_scores(S, I), at[:, None] + 1 + np.arange(k)[None, :])


def test_after_is_search_masked_under_the_mask_of_the_eligible_rows(oracle):
    for name in ("base", "hostile", "tie"):
        x, q, S = scores(name, oracle)
        nq, n = S.shape
        whole = after_ref.unbounded(S)
        for j, k in ((0, 10), (300, 100), (900, 2048)):
            sc = np.array([whole[i][0][j] for i in range(nq)], np.float32)
            rw = np.array([whole[i][1][j] for i in range(nq)], np.int64)
            bound = after_ref.cursor_keys(sc, rw).view(np.uint64)
            with np.errstate(invalid="ignore"):
                masks = np.stack([after_ref.pack(np.where(np.isnan(S[i]), 0, S[i]), np.arange(n)) < bound[i] for i in range(nq)])
            after_ref.assert_same(after_ref.after_from_scores(S, sc, rw, k), masked_ref.masked_from_scores(S, masks, None, k), f"{name} j={j} k={k}")


def test_ahead_the_cursor_row_and_behind_add_up(oracle):
    for name in ("hostile", "tie"):
        x, q, S = scores(name, oracle)
        nq, n = S.shape
        scored = (~np.isnan(S)).sum(axis=1)
        rng = np.random.default_rng(0xC02)
        for trial in range(4):
            rows = rng.integers(0, n, nq)
            sc = S[np.arange(nq), rows].copy()
            if trial == 1:
                rows = rows + 3                                            # the cursor row no longer scores s_ref (mostly)
            if trial == 2:
                rows[:] = n + 5
            keep = ~np.isnan(sc)
            ahead = rank_ref.count_ahead(S, sc[:, None], rows[:, None])[:, 0]
            behind = (after_ref.after_from_scores(S, sc, rows, n)[1] >= 0).sum(axis=1)
            own = np.array([rows[i] < n and S[i, min(rows[i], n - 1)] == sc[i] for i in range(nq)])
            np.testing.assert_array_equal((ahead + own + behind)[keep], scored[keep])
            assert (behind[~keep] == 0).all()                              # a NaN cursor score: an empty list


def test_cursor_edges(oracle):
    x, q, S = scores("hostile", oracle)
    nq, n = S.shape
    k = 9
    empty = (np.full((nq, k), -FMAX, np.float32), np.full((nq, k), -1, np.int64))
    for sc in (np.float32(np.nan), np.float32(-FMAX), np.float32(np.inf), np.float32(0)):
        after_ref.assert_same(after_ref.after_from_scores(S, np.full(nq, sc), np.full(nq, -1, np.int64), k), empty, f"row -1 at {sc}")
    after_ref.assert_same(after_ref.after_from_scores(S, np.full(nq, np.nan, np.float32), np.zeros(nq, np.int64), k), empty, "a NaN score")
    after_ref.assert_same(after_ref.after_from_scores(S, np.zeros(nq, np.float32), np.full(nq, -3, np.int64), k), empty, "row -3: the device forms' rule")
    # taken literally, a padding cursor (-FLT_MAX, -1) would list the rows scoring -Inf again: the -1 rule is needed
    low = np.flatnonzero(S[2] == -np.inf)
    with np.errstate(invalid="ignore"):
        assert (S[2] < np.float32(-FMAX)).sum() == len(low) >= 2 and {40, 4001} <= set(low.tolist()) and low[0] > 0
    # (-Inf, 0): the -Inf rows, all behind row 0; (-Inf, one of them): those behind it; (-Inf, the last, ntotal, 2^32): nothing
    for b, rows in ((0, low), (40, low[low > 40]), (low[-2], low[-1:]), (low[-1], low[:0]), (n, low[:0]), (2 ** 32, low[:0])):
        I = after_ref.after_from_scores(S[2:3], np.array([-np.inf], np.float32), np.array([b], np.int64), 40)[1][0]
        assert I[:len(rows)].tolist() == rows.tolist() and (I[len(rows):] == -1).all(), b
    # (+Inf, 20) where row 20 scores +Inf: the +Inf rows behind row 20, row 21 first, then everything else
    assert S[2, 20] == S[2, 21] == np.inf and S[3, 40] == np.inf
    D, I = after_ref.after_from_scores(S[2:3], np.array([np.inf], np.float32), np.array([20], np.int64), 40)
    high = np.flatnonzero(S[2] == np.inf)
    behind = high[high > 20]
    assert I[0, 0] == 21 and I[0, :len(behind)].tolist() == behind.tolist() and np.isfinite(D[0, len(behind):]).all()
    # -0.0 and +0.0 cursors are one cursor
    a = after_ref.after_from_scores(S, np.full(nq, -0.0, np.float32), np.full(nq, 7, np.int64), k)
    b = after_ref.after_from_scores(S, np.full(nq, 0.0, np.float32), np.full(nq, 7, np.int64), k)
    after_ref.assert_same(a, b, "-0.0 against +0.0")
    assert (a[1][0] > 7).all() and (a[0][0] == 0).all()                    # the zero query: every scored row ties at +0.0


# ---------------------------------------------------------------------------------------------------------------------
# 2. key packing
def test_cursor_keys_packs_like_the_reference(oracle):
    import torch
    from haconvdr_amd.index import cursor_keys
    sc = np.array([0.0, -0.0, 1.5, -1.5, np.inf, -np.inf, np.nan, FMAX, -FMAX, 1e-45, -1e-45, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0, np.nan, 2.0], np.float32)
    rw = np.array([0, 0, 7, 7, 5, 5, 5, 1, 1, 2, 2, -1, -2, -3, 2 ** 32 - 2, 2 ** 32 - 1, 2 ** 40, -2, np.iinfo(np.int64).max], np.int64)
    for base in (0, 1000, 2 ** 32 - 1):
        want = after_ref.cursor_keys(sc, rw, base)
        got = cursor_keys(sc, rw, base)
        assert got.dtype == np.int64 and got.shape == sc.shape
        np.testing.assert_array_equal(got, want, err_msg=f"ndarray base={base}")
        t = cursor_keys(torch.from_numpy(sc), torch.from_numpy(rw), base)            # a CPU tensor takes the path CUDA tensors take
        assert t.dtype == torch.int64
        np.testing.assert_array_equal(t.numpy(), want, err_msg=f"tensor base={base}")
    w = after_ref.cursor_keys(sc, rw).view(np.uint64)
    assert w[0] == w[1] and w[6] == 0 and w[11] == 0 and w[13] == 0 and w[12] == w[17] == after_ref.ALL_ONES
    assert w[15] == w[16] == w[18] - (w[18] >> np.uint64(32) << np.uint64(32)) + (w[15] >> np.uint64(32) << np.uint64(32))    # rows >= 2^32 - 1: low word 0
    assert (w[15] & np.uint64(0xFFFFFFFF)) == 0 and (w[14] & np.uint64(0xFFFFFFFF)) == 1
    assert w[4] > w[7] > w[2] > w[9] > w[0] > w[10] > w[3] > w[8] > w[5] > 0        # key order is score order
    # 2-D shapes pass through
    np.testing.assert_array_equal(cursor_keys(sc[:18].reshape(3, 6), rw[:18].reshape(3, 6)), after_ref.cursor_keys(sc[:18], rw[:18]).reshape(3, 6))
    # the cursor of (D[:, -1], I[:, -1]) is the last column of the oracle's key list, padding included
    x, q, S = scores("tie", oracle)
    for k in (7, 100, 1001):
        D, I = oracle.flat_ip_search(x, q, k)
        keys = after_ref.after_from_keys(S, None, 0, k)
        np.testing.assert_array_equal(cursor_keys(D[:, -1].copy(), I[:, -1].copy()).view(np.uint64), keys[:, -1])
    assert (keys[:, -1] == 0).all()
    for bad in ((sc.astype(np.float64), rw), (sc, rw.astype(np.float32)), (sc[:-1], rw), (torch.from_numpy(sc), rw)):
        with pytest.raises(ValueError):
            cursor_keys(*bad)
    for bad_base in (-1, 2 ** 32, 1.0, True):
        with pytest.raises(ValueError):
            cursor_keys(sc, rw, bad_base)


# ---------------------------------------------------------------------------------------------------------------------
# 3. what the GPU tests' inputs show
def test_tie_corpus_puts_page_boundaries_inside_runs_of_equal_scores(oracle):
    """A query's list is at most 16 runs of equal scores, 62 or 63 rows each (1000 = 62 * 16 + 8).  Pages of 100: every boundary
    lies inside a run.  Pages of 7: a run end that is a multiple of 7 cannot be avoided -- the run ends are 63 a + 62 b, and
    b, the 62-row runs so far, passes 7 on its way to 8 -- so a few boundaries coincide with a run end (the other edge: a page
    that ends with its run) and all the others, at least 97 %, lie inside one.  The zero query is one run of 1000."""
    x, q, S = scores("tie", oracle)
    n = S.shape[1]
    assert all(len(np.unique(S[i])) <= 16 for i in range(len(q))) and (S[0] == 0).all()
    whole = after_ref.unbounded(S)
    at_run_end = {k: sum(int(whole[i][0][p - 1] != whole[i][0][p]) for i in range(len(q)) for p in range(k, n, k)) for k in after_cases.TIE_PAGE_KS}
    boundaries = {k: len(q) * len(range(k, n, k)) for k in after_cases.TIE_PAGE_KS}
    assert at_run_end[100] == 0 and boundaries[100] == 54
    assert 1 <= at_run_end[7] <= 15 * (len(q) - 1) and at_run_end[7] <= 0.03 * boundaries[7]
    assert all(whole[0][0][p - 1] == whole[0][0][p] for p in range(1, n))


def test_hostile_corpus_has_nan_and_minus_inf_scores(oracle):
    x, q, S = scores("hostile", oracle)
    assert np.isnan(S).any(axis=1).all() and np.isnan(S).sum(axis=1).min() >= 100
    for i, (up, down) in ((2, ((20, 21), (40, 4001))), (3, ((40, 4001), (20, 21)))):
        assert (S[i, list(up)] == np.inf).all() and (S[i, list(down)] == -np.inf).all()
    assert ((np.abs(x.view(np.uint32)) & 0x7F800000) == 0).any()
    assert (~np.isnan(S)).sum(axis=1).min() > 2 * 2048                     # pages of 2048: at least two full ones and a partial one


def test_per_query_depths_give_every_query_of_a_tile_a_bound_of_its_own(oracle):
    x, q, S = scores("base", oracle)
    j = after_cases.per_query_depths()
    assert j.min() == 0 and j.max() == after_cases.K_MAX - 1
    for QT in (16, 4):
        for t0 in range(0, len(q), QT):
            assert len(set(j[t0:t0 + QT].tolist())) == len(j[t0:t0 + QT])
    sD, sI = oracle.flat_ip_search(x, q, after_cases.K_MAX)
    bounds = after_ref.cursor_keys(sD[np.arange(len(q)), j], sI[np.arange(len(q)), j])
    assert len(set(bounds.tolist())) == len(q)
    # a scan that tested one bound per tile would answer differently for every other query of the tile
    own = after_ref.after_from_scores(S, sD[np.arange(len(q)), j], sI[np.arange(len(q)), j], 10)[1]
    first = after_ref.after_from_scores(S[1:16], np.repeat(sD[0, j[0]], 15), np.repeat(sI[0, j[0]], 15), 10)[1]
    assert (own[1:16] != first).any(axis=1).all()


# ---------------------------------------------------------------------------------------------------------------------
# 4. argument checks (no handle, no library call)
def test_after_args_pass_good_arguments_through():
    from haconvdr_amd import index
    q, k, s, r = index._after_args(np.zeros((3, 96), np.float64), np.int64(10), None, 96)
    assert q.dtype == np.float32 and k == 10 and s is None and r is None
    q, k, s, r = index._after_args(np.zeros((3, 96)), 2048, (np.array([1, np.nan, -np.inf], np.float32), np.array([5, -1, -2], np.int32)), 96)
    assert s.dtype == np.float32 and r.dtype == np.int64 and r.tolist() == [5, -1, -2] and s.flags.c_contiguous and r.flags.c_contiguous
    q, k, s, r = index._after_args(np.zeros((0, 96)), 1, [np.zeros(0, np.float32), np.zeros(0, np.int64)], 96)
    assert q.shape == (0, 96) and s.shape == r.shape == (0,)
    assert index._after_args(np.zeros((1, 96)), 1, (np.zeros(1, np.float32), np.array([2 ** 40])), 96)[3].tolist() == [2 ** 40]


@pytest.mark.parametrize("q, k, after", [
    (np.zeros((3, 96)), 10, (np.zeros(3, np.float64), np.zeros(3, np.int64))),       # scores that are not float32
    (np.zeros((3, 96)), 10, (np.zeros(3, np.int64), np.zeros(3, np.int64))),
    (np.zeros((3, 96)), 10, (np.zeros(2, np.float32), np.zeros(3, np.int64))),       # one score per query
    (np.zeros((3, 96)), 10, (np.zeros((3, 1), np.float32), np.zeros(3, np.int64))),
    (np.zeros((3, 96)), 10, (np.zeros(3, np.float32), np.zeros(3, np.float32))),     # float rows
    (np.zeros((3, 96)), 10, (np.zeros(3, np.float32), np.zeros(4, np.int64))),       # one row per query
    (np.zeros((3, 96)), 10, (np.zeros(3, np.float32), np.zeros((1, 3), np.int64))),
    (np.zeros((3, 96)), 10, (np.zeros(3, np.float32), np.array([0, -3, 0]))),        # a row below -2
    (np.zeros((3, 96)), 10, (np.zeros(3, np.float32), np.array([0, 0, np.iinfo(np.int64).min]))),
    (np.zeros((3, 96)), 10, (np.zeros(3, np.float32),)),                             # not a pair
    (np.zeros((3, 96)), 10, np.zeros((2, 3), np.float32)),
    (np.zeros((3, 96)), 0, None),                                                    # k
    (np.zeros((3, 96)), 2049, None),
    (np.zeros((3, 96)), 2.0, None),
    (np.zeros((3, 95)), 10, None),                                                   # wrong dimension
])
def test_after_args_raise_value_error(q, k, after):
    from haconvdr_amd import index
    with pytest.raises(ValueError):
        index._after_args(q, k, after, 96)


def test_python_mirrors_raise_before_the_library_is_called(monkeypatch):
    """every ValueError of search_after / search_after_tensor / search_after_keys_tensor comes before _lib.lib() is touched"""
    import torch
    from haconvdr_amd import _lib, index

    def never():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", never)
    idx = index.FlatIPIndex.__new__(index.FlatIPIndex)
    idx.d, idx.devices = 96, (0,)
    with pytest.raises(ValueError) as err:
        idx.search_after(np.zeros((3, 96), np.float32), 10, (np.zeros(3, np.float32), np.array([0, -3, 0])))
    assert "query 1" in str(err.value) and "-3" in str(err.value)
    with pytest.raises(ValueError):
        idx.search_after(np.zeros((3, 96), np.float32), 0)
    # the tensor forms hand raw device pointers to kernels: a CPU tensor or an ndarray never gets there
    qt = torch.zeros(3, 96)
    for call in (lambda: idx.search_after_tensor(qt, 10), lambda: idx.search_after_keys_tensor(qt, 10),
                 lambda: idx.search_after_tensor(np.zeros((3, 96), np.float32), 10, (np.zeros(3, np.float32), np.zeros(3, np.int64))),
                 lambda: index._after_keys_args_tensor(qt, 10, torch.zeros(3, dtype=torch.int64), 0, 96),
                 lambda: index._after_args_tensor(qt, 10, (torch.zeros(3), torch.zeros(3, dtype=torch.int64)), None, 96)):
        with pytest.raises(ValueError):
            call()
    idx._h = None                                                          # (__del__ finds nothing to destroy)
    # (shape, dtype, device and k mistakes on real CUDA tensors: tests/test_index_after_gpu.py)


def test_sharded_searcher_checks_cursors_before_any_hook_runs():
    import torch
    from haconvdr_amd.sharded import ShardedSearcher

    def never(*a):
        raise AssertionError("a hook ran")
    s = ShardedSearcher(None, 0, local_keys=never, merge=never, to_results=never, filter=never, n_local=10, local_after_keys=never)
    for bad in (torch.zeros((3, 1), dtype=torch.int64), torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), torch.zeros(3)):
        with pytest.raises(ValueError):
            s.search_after(torch.zeros(3, 96), 10, bad)


# ---------------------------------------------------------------------------------------------------------------------
# ResidentCorpus over a stand-in index
class _StandInIndex:
    """the calls of FlatIPIndex that search_deep and behind make, over the oracle's canonical scores, on CPU tensors"""

    def __init__(self, oracle, x):
        self.oracle, self.x, self.calls = oracle, x, []

    @property
    def ntotal(self):
        return len(self.x)

    def _S(self, q):
        with np.errstate(all="ignore"):
            return rank_ref.canon_scores(self.oracle, self.x, np.asarray(q, np.float32))

    def search_keys_tensor(self, q, k, pos_base=0, stream=None):
        import torch
        self.calls.append(("search_keys", int(k)))
        return torch.from_numpy(after_ref.after_from_keys(self._S(q.numpy()), None, pos_base, k).view(np.int64))

    def search_after_keys_tensor(self, q, k, after_keys=None, pos_base=0, stream=None):
        import torch
        self.calls.append(("search_after_keys", int(k)))
        return torch.from_numpy(after_ref.after_from_keys(self._S(q.numpy()), after_keys.numpy(), pos_base, k).view(np.int64))

    def score_ids(self, q, ids):
        S = self._S(q)
        return np.where(ids >= 0, np.take_along_axis(S, np.maximum(ids, 0), 1), np.float32(-FMAX)).astype(np.float32)

    def search_after(self, q, k, after=None):
        self.calls.append(("search_after", int(k)))
        return after_ref.after_from_scores(self._S(q), after[0], after[1], k)


def test_resident_corpus_search_deep_and_behind(oracle, monkeypatch):
    import torch
    from haconvdr_amd import index as index_mod
    from haconvdr_amd.search import ResidentCorpus
    from tests import doubles
    x, q = after_cases.hostile_case()
    x, q = x[:700].copy(), q[:4]
    x[40] = x[21]                                                          # (row 4001 is gone: keep two rows on the -Inf side too)
    x[41] = -x[21]
    n = len(x)
    pids = np.arange(n, dtype=np.int64) * 7 + 11
    monkeypatch.setattr(index_mod, "keys_to_results", lambda keys, id_map=None, stream=None: tuple(
        torch.from_numpy(a) for a in doubles.to_results(keys, None if id_map is None else id_map.numpy())))
    rc = ResidentCorpus.__new__(ResidentCorpus)
    rc.index, rc._ids, rc._lookup = _StandInIndex(oracle, x), pids, None
    rc.dev, rc.id_map = torch.device("cpu"), torch.from_numpy(pids)
    with np.errstate(all="ignore"):
        S = rank_ref.canon_scores(oracle, x, q)
    whole = after_ref.unbounded(S)
    assert (S[2] == -np.inf).any() and np.isnan(S).any()
    for depth, page, calls in ((650, 256, [("search_keys", 256), ("search_after_keys", 256), ("search_after_keys", 138)]),
                               (800, 300, [("search_keys", 300), ("search_after_keys", 300), ("search_after_keys", 200)]),
                               (5, 1024, [("search_keys", 5)])):
        rc.index.calls.clear()
        D, I = rc.search_deep(torch.from_numpy(q) if depth == 5 else q, depth, page=page)
        assert rc.index.calls == calls and D.dtype == np.float64 and I.dtype == np.int64 and D.shape == I.shape == (len(q), depth)
        for i in range(len(q)):
            m = min(depth, len(whole[i][1]))
            np.testing.assert_array_equal(I[i, :m], pids[whole[i][1][:m]])
            np.testing.assert_array_equal(D[i, :m], whole[i][0][:m].astype(np.float64))
            assert (I[i, m:] == -1).all() and (D[i, m:] == np.float64(-FMAX)).all()
    for bad in (dict(depth=0), dict(depth=10, page=0), dict(depth=10, page=2049), dict(depth=2.0)):
        with pytest.raises(ValueError):
            rc.search_deep(q, **bad)
    # behind: the rows right behind the named passage; an absent passage and a NaN-scored one give empty lists
    gold = np.array([pids[100], 5, pids[3], pids[whole[3][1][-1]]])         # query 1: no block holds 5; query 2: row 3 scores NaN; query 3: the last row
    assert np.isnan(S[2, 3])
    D, I = rc.behind(q, gold, 12)
    assert D.dtype == np.float64 and I.dtype == np.int64 and D.shape == I.shape == (4, 12)
    at = int(np.flatnonzero(whole[0][1] == 100)[0])
    np.testing.assert_array_equal(I[0], pids[whole[0][1][at + 1:at + 13]])
    np.testing.assert_array_equal(D[0], whole[0][0][at + 1:at + 13].astype(np.float64))
    assert (I[1:] == -1).all() and (D[1:] == np.float64(-FMAX)).all()
    with pytest.raises(ValueError):
        rc.behind(q, gold[:, None], 12)


# ---------------------------------------------------------------------------------------------------------------------
# 7. ShardedSearcher.search_after over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_after_double_restates_the_contract(oracle):
    import torch
    from tests import doubles, doubles_after
    x = np.array([[1.0] * 32, [2.0] * 32, [1.0] * 32, [np.nan] * 32, [3.0] * 32, [1.0] * 32], np.float32)
    q = torch.ones((1, 32))
    hook = doubles_after.make_local_after_keys(oracle, x)
    D, pos = doubles.unpack_keys(hook(q, 4, None, 100).numpy())
    assert pos.tolist() == [[104, 101, 100, 102]] and D[0].tolist() == [96.0, 64.0, 32.0, 32.0]
    cursor = torch.from_numpy(after_ref.cursor_keys(np.array([32.0], np.float32), np.array([100])))     # global position 100 = local row 0
    D, pos = doubles.unpack_keys(hook(q, 4, cursor, 100).numpy())
    assert pos.tolist() == [[102, 105, -1, -1]]
    assert doubles_after.CALLS == [(4, False, 100), (4, True, 100)]
    doubles_after.CALLS.clear()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_search_after_gloo(world):
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="2")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_gloo_worker_after.py"), "double"], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
        assert "OK" in o
