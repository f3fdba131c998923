"""search_after: hac_index_search_after* (after_bounds_kernel of csrc/after.inc and scan16_after_kernel of csrc/scan16_filter.inc) through FlatIPIndex,
i.e. the C ABI.

Every assertion is equality of I and of the bits of D with tests/after_ref.py, the definition of include/haconvdr.h restated
over the CPU oracle's canonical scores.  Indexes are built like _index() of tests/test_search_plans_gpu.py: three adds cut off
the 64-row grid, so the rows straddle segments and the last group is partial (5000 rows: 79 groups, the last of 8 rows), with
the prefilter off.  Every case checks the host form and the tensor form and leaves the status word clean.  What the inputs
are good for, and the identities the cases lean on, are proved on the CPU in tests/test_index_after.py."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

from haconvdr_amd import synth
from tests import after_cases, after_ref, nonfinite, rank_ref
from tests.golden import cases
from tests.test_index_masked_gpu import expected_tile
from tests.test_search_plans_gpu import _cuts, _index

pytestmark = pytest.mark.gpu

HAC_ERR_INVALID, HAC_ERR_UNSUPPORTED = 1, 4
MAX_K = 2048
FMAX = after_ref.FMAX
D, N, NQ = after_cases.D, after_cases.N, after_cases.NQ
_PLAN = re.compile(r"^scan16_after_kernel<W=(?P<W>\d+)> grid=\((?P<P>\d+),(?P<T>\d+)\) QT=(?P<QT>\d+) C=(?P<C>\d+) lds=(?P<lds>\d+) launches=(?P<launches>\d+)$")


def parse_plan(text):
    m = _PLAN.match(text)
    assert m, "not the plan of a search behind a cursor: %r" % text
    return {k: int(v) for k, v in m.groupdict().items()}


def _cuda(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _after_cuda(after):
    return None if after is None else (_cuda(after[0], np.float32), _cuda(after[1], np.int64))


def tensor_form(idx, q, after, k, id_map=None):
    """(D, I) of search_after_tensor as ndarrays"""
    import torch
    Dt, It = idx.search_after_tensor(_cuda(q, np.float32), k, _after_cuda(after), id_map=id_map)
    torch.cuda.synchronize()
    return Dt.cpu().numpy(), It.cpu().numpy()


def keys_form(idx, q, after_keys, k, pos_base=0):
    """the uint64 keys of search_after_keys_tensor as an ndarray"""
    import torch
    keys = idx.search_after_keys_tensor(_cuda(q, np.float32), k, None if after_keys is None else _cuda(np.asarray(after_keys).view(np.int64), np.int64),
                                        pos_base=pos_base)
    torch.cuda.synchronize()
    return keys.cpu().numpy().view(np.uint64)


def both_forms(idx, q, after, k, want, what=""):
    """host form and tensor form against the reference; the status word stays clean"""
    after_ref.assert_same(idx.search_after(q, k, after), want, f"{what} host form")
    after_ref.assert_same(tensor_form(idx, q, after, k), want, f"{what} tensor form")
    idx.check_status()


def want_of(S, after, k):
    return after_ref.after_from_scores(S, None if after is None else after[0], None if after is None else after[1], k)


_CASES = {}


def scores(name, oracle):
    """(x, q, S) of a shared case: rows, queries and their canonical scores, computed once and never changed"""
    if name not in _CASES:
        x, q = {"base": after_cases.base_case, "tie": after_cases.tie_case, "hostile": after_cases.hostile_case}[name]()
        with np.errstate(all="ignore"):
            S = rank_ref.canon_scores(oracle, x, q)
        S.setflags(write=False)
        _CASES[name] = (x, q, S)
    return _CASES[name]


# ---------------------------------------------------------------------------------------------------------------------
# 1. a start cursor is search
@pytest.mark.parametrize("k", after_cases.START_KS)
def test_start_cursor_is_search(k, oracle):
    x, q, S = scores("base", oracle)
    idx = _index(D, x)
    for nq in after_cases.START_NQS:
        want = want_of(S[:nq], None, k)
        after_ref.assert_same(idx.search(q[:nq], k), want, f"search k={k} nq={nq}")
        both_forms(idx, q[:nq], None, k, want, f"null cursors k={k} nq={nq}")
        plan = parse_plan(idx.last_plan())
        QT, C, lds = expected_tile(D, k, nq)
        assert (plan["QT"], plan["C"], plan["lds"], plan["T"], plan["launches"], plan["W"]) == (QT, C, lds, -(-nq // QT), 1, 4), plan
        assert 1 <= plan["P"] <= 20, plan                                  # 79 groups: at most 20 streams of 4 waves
        start = (np.full(nq, np.nan, np.float32), np.full(nq, -2, np.int64))      # row -2: the score is not read
        both_forms(idx, q[:nq], start, k, want, f"row -2 k={k} nq={nq}")
        after_ref.assert_same(after_ref.unpack(keys_form(idx, q[:nq], None, k)), want, f"keys form k={k} nq={nq}")
    assert expected_tile(D, 2048, 37)[0] == 4 and expected_tile(D, 100, 37)[0] == 16


# ---------------------------------------------------------------------------------------------------------------------
# 2. a cursor from a search's own list
@pytest.mark.parametrize("k", after_cases.CURSOR_KS)
def test_cursor_from_a_searchs_own_list(k, oracle):
    x, q, S = scores("base", oracle)
    idx = _index(D, x)
    K = after_cases.K_MAX
    sD, sI = idx.search(q, K)
    after_ref.assert_same((sD, sI), want_of(S, None, K), "search at K")
    for j in after_cases.CURSOR_JS:
        after = (sD[:, j].copy(), sI[:, j].copy())
        want = want_of(S, after, k)
        both_forms(idx, q, after, k, want, f"j={j} k={k}")
        fits = min(k, K - (j + 1))
        np.testing.assert_array_equal(want[1][:, :fits], sI[:, j + 1:j + 1 + fits])
        np.testing.assert_array_equal(after_ref.bits(want[0][:, :fits]), after_ref.bits(sD[:, j + 1:j + 1 + fits]))
    # every query of a tile at a depth of its own
    j = after_cases.per_query_depths()
    after = (sD[np.arange(NQ), j].copy(), sI[np.arange(NQ), j].copy())
    both_forms(idx, q, after, k, want_of(S, after, k), f"per-query depths k={k}")


# ---------------------------------------------------------------------------------------------------------------------
# 3. paging to the end
@pytest.mark.parametrize("k", after_cases.PAGE_KS)
def test_paging_to_the_end(k, oracle):
    x, q, S = scores("hostile", oracle)
    nq, n = S.shape
    idx = _index(after_cases.HOSTILE_D, x)
    whole = after_ref.unbounded(S)
    after, pages, offset = None, [], 0
    for _ in range(n // k + 2):
        want = want_of(S, after, k)
        both_forms(idx, q, after, k, want, f"page at {offset}")
        Dp, Ip = idx.search_after(q, k, after)
        ranks = idx.rank_ids(q, Ip)                                        # rank_ids of a page: offset + j; -1 in padding
        np.testing.assert_array_equal(ranks, np.where(Ip >= 0, offset + np.arange(k)[None, :], -1))
        pages.append((Dp, Ip))
        after = (Dp[:, -1].copy(), Ip[:, -1].copy())                       # the last entry, padding or not, is the next cursor
        offset += k
    assert (pages[-1][1] == -1).all() and (pages[-1][0] == -FMAX).all()     # the page after the end
    Dc, Ic = np.concatenate([p[0] for p in pages], 1), np.concatenate([p[1] for p in pages], 1)
    for i in range(nq):
        m = len(whole[i][1])
        np.testing.assert_array_equal(Ic[i, :m], whole[i][1])
        np.testing.assert_array_equal(after_ref.bits(Dc[i, :m]), after_ref.bits(whole[i][0]))
        assert (Ic[i, m:] == -1).all()
    assert any(np.isneginf(whole[i][0][-1]) for i in range(nq)) and all(len(whole[i][1]) < n for i in range(nq))   # -Inf rows last, NaN rows never


# ---------------------------------------------------------------------------------------------------------------------
# 4. ties
def test_ties(oracle):
    x, q, S = scores("tie", oracle)
    nq, n = S.shape
    idx = _index(after_cases.TIE_D, x)
    whole = after_ref.unbounded(S)
    for k in after_cases.TIE_PAGE_KS:                                      # pages whose boundaries fall inside runs of equal scores
        after, offset = None, 0
        for _ in range(5 if k == 7 else n // k + 1):
            want = want_of(S, after, k)
            both_forms(idx, q, after, k, want, f"k={k} page at {offset}")
            for i in range(nq):
                np.testing.assert_array_equal(want[1][i][want[1][i] >= 0], whole[i][1][offset:offset + k])
            after = (want[0][:, -1].copy(), want[1][:, -1].copy())
            offset += k
    # cursors at every row of one tie run: the run of query 1's best score
    run = whole[1][1][whole[1][0] == whole[1][0][0]]
    assert 60 <= len(run) <= 130
    qs = np.repeat(q[1:2], len(run), 0)
    after = (np.full(len(run), whole[1][0][0], np.float32), run.astype(np.int64))
    want = want_of(np.repeat(S[1:2], len(run), 0), after, 70)
    assert all(want[1][t, 0] == (run[t + 1] if t + 1 < len(run) else whole[1][1][len(run)]) for t in range(len(run)))
    both_forms(idx, qs, after, 70, want, "every row of a run")
    # cursor rows the index does not hold at the cursor's score: between two rows of the run, ntotal, 2^32; a score no row has
    s1 = whole[1][0][0]
    between = np.setdiff1d(np.arange(run[0], run[-1]), run)[:2]
    rows = np.array([between[0], between[1], n, 2 ** 32, 2 ** 32 - 1, 2 ** 40, 0], np.int64)
    sc = np.array([s1] * 6 + [(np.float32(s1) + whole[1][0][len(run)]) / 2], np.float32)
    assert sc[-1] not in S[1]
    qs = np.repeat(q[1:2], len(rows), 0)
    want = want_of(np.repeat(S[1:2], len(rows), 0), (sc, rows), 20)
    assert want[1][0, 0] in run and want[1][2, 0] == want[1][3, 0] == want[1][6, 0] == whole[1][1][len(run)]
    both_forms(idx, qs, (sc, rows), 20, want, "rows and a score the index does not hold")
    # -0.0 and +0.0 cursors: one cursor (the zero query scores +0.0 everywhere)
    for k in (7, 100):
        a = (np.full(nq, -0.0, np.float32), np.full(nq, 500, np.int64))
        b = (np.full(nq, 0.0, np.float32), np.full(nq, 500, np.int64))
        want = want_of(S, b, k)
        assert want[1][0].tolist() == list(range(501, 501 + k))
        both_forms(idx, q, a, k, want, f"-0.0 k={k}")
        both_forms(idx, q, b, k, want, f"+0.0 k={k}")


# ---------------------------------------------------------------------------------------------------------------------
# 5. cursor edges
def test_cursor_edges(oracle):
    x, q, S = scores("hostile", oracle)
    nq, n = S.shape
    idx = _index(after_cases.HOSTILE_D, x)
    k = 40
    empty = (np.full((nq, k), -FMAX, np.float32), np.full((nq, k), -1, np.int64))
    both_forms(idx, q, (np.full(nq, np.nan, np.float32), np.zeros(nq, np.int64)), k, empty, "a NaN score")
    for sc in (np.nan, -FMAX, np.inf, 0.0):
        both_forms(idx, q, (np.full(nq, sc, np.float32), np.full(nq, -1, np.int64)), k, empty, f"row -1 at {sc}")
    # (-FLT_MAX, -1) as a padded page gives it
    last = idx.search_after(q, k, (np.full(nq, -np.inf, np.float32), np.full(nq, n, np.int64)))
    assert (last[1] == -1).all() and (last[0] == -FMAX).all()
    both_forms(idx, q, (last[0][:, -1].copy(), last[1][:, -1].copy()), k, empty, "the cursor of a padded page")
    # mixed in one tile: a start, an exhausted list, a NaN, -Inf and +Inf cursors next to an ordinary one
    low, high = np.flatnonzero(S[2] == -np.inf), np.flatnonzero(S[2] == np.inf)
    qs = q[[2, 2, 2, 2, 2, 2, 2, 3, 1]]
    Ss = S[[2, 2, 2, 2, 2, 2, 2, 3, 1]]
    sc = np.array([0, 0, np.nan, -np.inf, -np.inf, np.inf, np.inf, np.inf, 0.25], np.float32)
    rows = np.array([-2, -1, 5, 0, 40, 20, n, 40, 17], np.int64)
    want = want_of(Ss, (sc, rows), k)
    assert want[1][3][:len(low)].tolist() == low.tolist() and (want[1][3][len(low):] == -1).all()          # (-Inf, 0): the -Inf rows behind row 0 only
    assert want[1][4][:len(low) - 1].tolist() == low[low > 40].tolist()
    assert want[1][5][0] == 21 and want[0][5][0] == np.inf and want[1][7][0] == low[low > 40][0]                       # (+Inf, row) where the row scores +Inf
    assert np.isfinite(want[0][6][0]) and (want[1][1] == -1).all() and (want[1][2] == -1).all() and (want[1][0] >= 0).all()
    both_forms(idx, qs, (sc, rows), k, want, "edges in one tile")


# ---------------------------------------------------------------------------------------------------------------------
# 6. row streams and launch cuts
@pytest.mark.parametrize("k", [10, 2048])
def test_row_streams_and_launch_cuts(k, oracle):
    x, q, S = scores("base", oracle)
    sD, sI = want_of(S, None, after_cases.K_MAX)
    j = after_cases.per_query_depths()
    after = (sD[np.arange(NQ), j].copy(), sI[np.arange(NQ), j].copy())
    want = want_of(S, after, k)
    QT = expected_tile(D, k, NQ)[0]
    assert QT == (16 if k == 10 else 4)
    tiles = -(-NQ // QT)
    idx = _index(D, x, after_p="1")
    results = []
    for p, cut in (("1", "0"), ("auto", "0"), ("3", "0"), ("auto", "1"), ("1", "2"), ("4096", "0")):
        idx.set_option("after_p", p)
        idx.set_option("debug_after_tiles", cut)
        both_forms(idx, q, after, k, want, f"after_p={p} debug_after_tiles={cut}")
        plan = parse_plan(idx.last_plan())
        assert plan["QT"] == QT and plan["C"] == (512 if k == 10 else 4096), plan
        if p == "1":
            assert plan["P"] == 1, plan                                    # one workgroup walks every group: 20 rounds of 4, compactions past C - 256 slots
        elif p == "3":
            assert plan["P"] == 3, plan
        else:
            assert 1 < plan["P"] <= 20, plan
        per = int(cut) or tiles
        assert plan["T"] == min(per, tiles) and plan["launches"] == -(-tiles // per), plan
        keys = keys_form(idx, q, after_ref.cursor_keys(*after), k)
        results.append(keys.tobytes())
        after_ref.assert_same(after_ref.unpack(keys), want, f"keys form after_p={p}")
    assert len(set(results)) == 1                                          # identical bytes on every plan
    # the start cursor under one row stream: every row is eligible, the buffers compact throughout
    idx.set_option("after_p", "1")
    both_forms(idx, q, None, k, want_of(S, None, k), "start, after_p=1")


def test_set_option_values():
    from haconvdr_amd import _lib
    idx = _index(D, synth.embeddings(0xC50, 100, D))
    for name, bad in (("after_p", "0"), ("after_p", "4097"), ("after_p", "x"), ("debug_after_tiles", "-1"), ("debug_after_tiles", "many")):
        with pytest.raises(_lib.HacError) as err:
            idx.set_option(name, bad)
        assert err.value.code == HAC_ERR_INVALID
    for name, good in (("after_p", "1"), ("after_p", "4096"), ("after_p", "auto"), ("debug_after_tiles", "2"), ("debug_after_tiles", "0")):
        idx.set_option(name, good)


# ---------------------------------------------------------------------------------------------------------------------
# 7. non-finite queries next to healthy ones
@pytest.mark.parametrize("kind", nonfinite.KINDS)
def test_nonfinite_queries(kind, oracle):
    d, n, nq, k = 96, 3001, 33, 100
    x, q, pos, _ = nonfinite.case(kind, d, n, nq, 0xC80)
    with np.errstate(all="ignore"):
        S = rank_ref.canon_scores(oracle, x, q)
    first = want_of(S, None, k)
    healthy = [i for i in range(nq) if i not in pos]
    assert (first[1][healthy] >= 0).all()
    if kind in nonfinite.NAN_KINDS:
        assert all((first[1][i] == -1).all() for i in pos)                 # a NaN query: padding only, and its padding cursor stays exhausted
    idx = _index(d, x)
    both_forms(idx, q, None, k, first, f"{kind} page 1")
    after = (first[0][:, -1].copy(), first[1][:, -1].copy())
    second = want_of(S, after, k)
    assert (second[1][healthy] >= 0).all()
    both_forms(idx, q, after, k, second, f"{kind} page 2")
    mid = (first[0][:, 40].copy(), first[1][:, 40].copy())
    both_forms(idx, q, mid, k, want_of(S, mid, k), f"{kind} from entry 40")


# ---------------------------------------------------------------------------------------------------------------------
# 8. index lifetime
def test_after_remove_after_reset_and_without_rows_or_queries(oracle):
    import torch
    d, n, nq, k = 96, 1000, 5, 50
    x = synth.embeddings(0xC90, n, d)
    q = synth.embeddings(0xC91, nq, d)
    idx = _index(d, x)
    S = rank_ref.canon_scores(oracle, x, q)
    page = want_of(S, None, k)
    after = (page[0][:, -1].copy(), page[1][:, -1].copy())
    both_forms(idx, q, after, k, want_of(S, after, k), "as built")
    gone = np.arange(100, 900, 7)
    assert idx.remove_ids(gone) == len(gone)
    left = np.delete(x, gone, 0)
    Sl = rank_ref.canon_scores(oracle, left, q)
    for a in (None, after, (after[0], np.full(nq, len(left) - 1, np.int64))):          # (the old cursor: a score and a row number, whatever is there now)
        both_forms(idx, q, a, k, want_of(Sl, a, k), "after remove_ids")
    # reset() and a smaller add(): the stale rows behind the new ntotal are never returned
    idx.reset()
    small = synth.embeddings(0xC93, 130, d)
    idx.add(small)
    Ss = rank_ref.canon_scores(oracle, small, q)
    want = want_of(Ss, None, 200)
    assert (want[1][:, :130] >= 0).all() and (want[1][:, 130:] == -1).all()
    both_forms(idx, q, None, 200, want, "after reset and a smaller add")
    a = (want[0][:, 99].copy(), want[1][:, 99].copy())
    want = want_of(Ss, a, 200)
    assert (want[1][:, :30] >= 0).all() and (want[1][:, 30:] == -1).all()
    both_forms(idx, q, a, 200, want, "after reset, behind entry 99")
    # nq == 0: HAC_OK, nothing touched
    D0, I0 = idx.search_after(np.zeros((0, d), np.float32), 7)
    assert D0.shape == I0.shape == (0, 7)
    D0, I0 = idx.search_after_tensor(torch.zeros((0, d), device="cuda"), 7, (torch.zeros(0, device="cuda"), torch.zeros(0, dtype=torch.int64, device="cuda")))
    assert tuple(D0.shape) == tuple(I0.shape) == (0, 7)
    assert tuple(idx.search_after_keys_tensor(torch.zeros((0, d), device="cuda"), 7).shape) == (0, 7)
    # an empty index: padding only
    idx.reset()
    pad = (np.full((nq, 4), -FMAX, np.float32), np.full((nq, 4), -1, np.int64))
    both_forms(idx, q, None, 4, pad, "empty index, start")
    both_forms(idx, q, (np.zeros(nq, np.float32), np.zeros(nq, np.int64)), 4, pad, "empty index, a cursor")
    assert (keys_form(idx, q, None, 4) == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 9. errors
def test_errors(oracle):
    import ctypes
    import torch
    from haconvdr_amd import _lib
    from haconvdr_amd.index import _f32p, _i64p
    x, q, S = scores("base", oracle)
    idx = _index(D, x)
    k = 10
    L = _lib.lib()
    sc = np.zeros(NQ, np.float32)
    rows = np.arange(NQ, dtype=np.int64)
    # a row below -2: the host form refuses, names the query and writes nothing ...
    Dh = np.full((NQ, k), np.float32(-123.5))
    Ih = np.full((NQ, k), -99, np.int64)
    for at, bad in ((16, -3), (3, np.iinfo(np.int64).min)):
        one = rows.copy()
        one[at] = bad
        with pytest.raises(_lib.HacError) as err:
            _lib.check(L.hac_index_search_after(idx._h, _f32p(q), NQ, k, _f32p(sc), _i64p(one), _f32p(Dh), _i64p(Ih)))
        assert err.value.code == HAC_ERR_INVALID and f"query {at}" in str(err.value) and f"{bad}" in str(err.value), str(err.value)
        with pytest.raises(ValueError):
            idx.search_after(q, k, (sc, one))
    assert (Dh == np.float32(-123.5)).all() and (Ih == -99).all()
    # ... in the device forms that query gets an empty list and no error
    wild = rows.copy()
    wild[3], wild[16], wild[36] = -3, np.iinfo(np.int64).min, -1000
    want = want_of(S, (sc, wild), k)
    assert all((want[1][i] == -1).all() for i in (3, 16, 36)) and (want[1][[0, 4, 17, 35], 0] >= 0).all()
    after_ref.assert_same(tensor_form(idx, q, (sc, wild), k), want, "rows below -2: empty lists, tensor form")
    # k outside [1, 2048]; only one cursor pointer: the library's own checks (the C ABI called directly)
    qt, st, rt = _cuda(q, np.float32), _cuda(sc, np.float32), _cuda(rows, np.int64)
    out_d, out_i = torch.empty((NQ, k), device="cuda"), torch.empty((NQ, k), dtype=torch.int64, device="cuda")
    null_f, null_i = ctypes.POINTER(ctypes.c_float)(), ctypes.POINTER(ctypes.c_int64)()
    for k_ in (0, MAX_K + 1, -1):
        assert L.hac_index_search_after(idx._h, _f32p(q), NQ, k_, null_f, null_i, _f32p(Dh), _i64p(Ih)) == HAC_ERR_INVALID
        assert L.hac_index_search_after_device(idx._h, qt.data_ptr(), NQ, k_, None, None, out_d.data_ptr(), out_i.data_ptr(), None, None) == HAC_ERR_INVALID
        assert L.hac_index_search_after_keys_device(idx._h, qt.data_ptr(), NQ, k_, None, out_i.data_ptr(), 0, None) == HAC_ERR_INVALID
    assert L.hac_index_search_after(idx._h, _f32p(q), NQ, k, _f32p(sc), null_i, _f32p(Dh), _i64p(Ih)) == HAC_ERR_INVALID
    assert L.hac_index_search_after(idx._h, _f32p(q), NQ, k, null_f, _i64p(rows), _f32p(Dh), _i64p(Ih)) == HAC_ERR_INVALID
    assert L.hac_index_search_after_device(idx._h, qt.data_ptr(), NQ, k, st.data_ptr(), None, out_d.data_ptr(), out_i.data_ptr(), None, None) == HAC_ERR_INVALID
    assert L.hac_index_search_after_device(idx._h, qt.data_ptr(), NQ, k, None, rt.data_ptr(), out_d.data_ptr(), out_i.data_ptr(), None, None) == HAC_ERR_INVALID
    assert (Dh == np.float32(-123.5)).all() and (Ih == -99).all()
    # argument mistakes on real CUDA tensors: ValueError before the library is called
    for args in ((qt, 0, (st, rt)), (qt, MAX_K + 1, (st, rt)), (qt, k, (st[:-1], rt)), (qt, k, (st, rt[:-1])), (qt, k, (st.double(), rt)), (qt, k, (st, rt.int())),
                 (qt, k, (st.cpu(), rt)), (qt, k, (st, rt.cpu())), (qt, k, (st,)), (qt, k, st), (qt[:, :-1], k, (st, rt)), (qt, k, (st[:, None], rt))):
        with pytest.raises(ValueError):
            idx.search_after_tensor(*args)
    for args in ((qt, k, rt[:-1]), (qt, k, rt.int()), (qt, k, rt.cpu()), (qt, k, rt[:, None]), (qt, 0, rt), (qt, k, rt, -1), (qt, k, rt, 2 ** 32)):
        with pytest.raises(ValueError):
            idx.search_after_keys_tensor(*args)
    with pytest.raises(ValueError):
        idx.search_after_tensor(qt, k, (st, rt), id_map=rt.cpu())
    both_forms(idx, q, (sc, rows), k, want_of(S, (sc, rows), k), "after the refused calls")
    # the device forms on a multi-device index
    two = _index(D, x[:500], devices=(0, 0))
    for call in (lambda: two.search_after_tensor(qt, k), lambda: two.search_after_tensor(qt, k, (st, rt)), lambda: two.search_after_keys_tensor(qt, k, rt)):
        with pytest.raises(_lib.HacError) as err:
            call()
        assert err.value.code == HAC_ERR_UNSUPPORTED
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 10. the keys form
def test_keys_form_pages_through_merge_keys_and_keys_to_results(oracle):
    """Two indexes hold the two halves of a corpus and search with pos_base = their first row: merged, the keys are those of
    one index over the whole corpus, and the merged list's last column is the cursor both halves take for the next page."""
    import torch
    from haconvdr_amd.index import cursor_keys, keys_to_results, merge_keys
    d, n, nq, k = 96, 1501, 7, 61
    x, q, ids = cases.search_case_inputs("dup", 0xCA0, n, nq, d=d)        # row r and row r + 750 are twins: ties cross the cut
    cut = 751
    S = rank_ref.canon_scores(oracle, x, q)
    whole = after_ref.unbounded(S)
    lo, hi, one = _index(d, x[:cut]), _index(d, x[cut:]), _index(d, x)
    qt, idt = _cuda(q, np.float32), _cuda(ids, np.int64)
    cursor, crossed = None, False
    for page in range(4):
        k_lo = lo.search_after_keys_tensor(qt, k, cursor, pos_base=0)
        k_hi = hi.search_after_keys_tensor(qt, k, cursor, pos_base=cut)
        merged = merge_keys(torch.stack([k_lo, k_hi]))
        Dm, Im = keys_to_results(merged, id_map=idt)
        torch.cuda.synchronize()
        want = after_ref.after_from_keys(S, None if cursor is None else cursor.cpu().numpy(), 0, k)
        np.testing.assert_array_equal(merged.cpu().numpy().view(np.uint64), want)
        wD, wI = after_ref.unpack(want)
        after_ref.assert_same((Dm.cpu().numpy(), Im.cpu().numpy()), (wD, ids[wI]), f"two shards merged, page {page}")
        for i in range(nq):
            np.testing.assert_array_equal(wI[i], whole[i][1][page * k:(page + 1) * k])
        crossed = crossed or any(wD[i, -1] == whole[i][0][(page + 1) * k] and wI[i, -1] < cut <= whole[i][1][(page + 1) * k] for i in range(nq))
        # the whole index from the same cursor: its own keys form, and a cursor taken from search_keys_tensor's last column
        np.testing.assert_array_equal(keys_form(one, q, None if cursor is None else cursor.cpu().numpy(), k), want)
        if page == 0:
            first = one.search_keys_tensor(qt, k)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(first.cpu().numpy().view(np.uint64), want)
            np.testing.assert_array_equal(merged[:, -1].cpu().numpy(), first[:, -1].cpu().numpy())
        cursor = merged[:, -1].contiguous()
    assert crossed                                                         # a page ended between two twins on different shards
    # pos_base != 0 on one index: the keys, and a cursor, live in that position space
    base = 1000
    c = cursor_keys(_cuda(whole_scores(whole, 30), np.float32), _cuda(whole_rows(whole, 30), np.int64), pos_base=base)
    got = one.search_after_keys_tensor(qt, k, c, pos_base=base)
    torch.cuda.synchronize()
    want = after_ref.after_from_keys(S, after_ref.cursor_keys(whole_scores(whole, 30), whole_rows(whole, 30), base), base, k)
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint64), want)
    wD, wI = after_ref.unpack(want, base)
    for i in range(nq):
        np.testing.assert_array_equal(wI[i], whole[i][1][31:31 + k])
    # id_map through the tensor form: it remaps the result, the cursor rows stay the index's own rows
    after = (whole_scores(whole, 30), whole_rows(whole, 30))
    wD, wI = want_of(S, after, k)
    after_ref.assert_same(tensor_form(one, q, after, k, id_map=idt), (wD, ids[wI]), "id_map")
    for i in (lo, hi, one):
        i.check_status()


def whole_scores(whole, j):
    return np.array([w[0][j] for w in whole], np.float32)


def whole_rows(whole, j):
    return np.array([w[1][j] for w in whole], np.int64)


def test_resident_corpus_search_deep_and_behind(tmp_path, oracle):
    from haconvdr_amd.passages import write_embedding_block
    from haconvdr_amd.search import ResidentCorpus
    n, nq, depth = 5200, 5, 5000
    x, q, _ = cases.search_case_inputs("gauss", 0xCB0, n, nq)
    ids = (np.arange(n, dtype=np.int64) * 7 + 11)[::-1].copy()            # distinct ids: rows_of names one row
    for b, (lo, hi) in enumerate(((0, 1800), (1800, 3600), (3600, n))):
        write_embedding_block(str(tmp_path), b, x[lo:hi], ids[lo:hi])
    rc = ResidentCorpus(str(tmp_path), passage_block_num=10)
    assert rc.ntotal == n and depth > MAX_K
    S = rank_ref.canon_scores(oracle, x, q)
    whole = after_ref.unbounded(S)
    Dd, Id = rc.search_deep(q, depth, page=1024)
    assert Dd.dtype == np.float64 and Id.dtype == np.int64 and Dd.shape == Id.shape == (nq, depth)
    for i in range(nq):
        np.testing.assert_array_equal(Id[i], ids[whole[i][1][:depth]])
        np.testing.assert_array_equal(Dd[i], whole[i][0][:depth].astype(np.float64))
    Dd, Id = rc.search_deep(q, n + 100, page=2048)                          # past the end: padding
    assert (Id[:, n:] == -1).all() and (Dd[:, n:] == np.float64(-FMAX)).all()
    for i in range(nq):
        np.testing.assert_array_equal(Id[i, :n], ids[whole[i][1]])
    # behind: the rows right behind the named passage
    at = np.array([0, 17, 2500, n - 1, 3])
    gold = np.array([ids[whole[i][1][at[i]]] for i in range(nq)])
    gold[4] = ids.max() + 1                                                # no block holds it
    Db, Ib = rc.behind(q, gold, 25)
    for i in range(4):
        m = min(25, n - 1 - at[i])
        np.testing.assert_array_equal(Ib[i, :m], ids[whole[i][1][at[i] + 1:at[i] + 1 + m]])
        np.testing.assert_array_equal(Db[i, :m], whole[i][0][at[i] + 1:at[i] + 1 + m].astype(np.float64))
        assert (Ib[i, m:] == -1).all()
    assert (Ib[4] == -1).all() and (Ib[3] == -1).all() and (Db[4] == np.float64(-FMAX)).all()
    rc.index.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 11. captured into a graph
def test_captured_into_a_graph_replays_on_new_cursors(oracle):
    import torch
    x, q, S = scores("hostile", oracle)
    nq, k = len(q), 64
    idx = _index(after_cases.HOSTILE_D, x)
    qt = _cuda(q, np.float32)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()                            # a single stream: no parallel branches in the graph
    pages = []
    with torch.cuda.stream(side):
        first = idx.search_after_keys_tensor(qt, k)       # the largest shape once: workspaces and the segment table exist
        cursor = first[:, -1].clone()
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            keys = idx.search_after_keys_tensor(qt, k, cursor)
        for _ in range(3):
            keys.zero_()
            g.replay()
            side.synchronize()
            pages.append(keys.cpu().numpy().view(np.uint64).copy())
            cursor.copy_(keys[:, -1])
    torch.cuda.synchronize()
    want = after_ref.after_from_keys(S, None, 0, 4 * k)
    np.testing.assert_array_equal(first.cpu().numpy().view(np.uint64), want[:, :k])
    for p, got in enumerate(pages):
        np.testing.assert_array_equal(got, want[:, (p + 1) * k:(p + 2) * k], err_msg=f"replay {p}: page {p + 2}")
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 12. several shards
@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)])
def test_multi_device_index(devices, oracle):
    x, q, S = scores("tie", oracle)
    nq, n = S.shape
    idx = _index(after_cases.TIE_D, x, devices=devices)
    whole = after_ref.unbounded(S)
    after_ref.assert_same(idx.search_after(q, 50), want_of(S, None, 50), "start")
    # pages chained across the shards: every score's run spans all of them
    for k in (7, 100):
        after, offset = None, 0
        for _ in range(4):
            want = want_of(S, after, k)
            after_ref.assert_same(idx.search_after(q, k, after), want, f"{len(devices)} shards k={k} page at {offset}")
            after = (want[0][:, -1].copy(), want[1][:, -1].copy())
            offset += k
    # cursor rows at the edges of every shard's share of every add, at the best score's run and at the query's own score there
    c1, c2 = _cuts(n)
    S_ = len(devices)
    edges = set()
    for a, b in ((0, c1), (c1, c2), (c2, n)):
        per = -(-(b - a) // S_)
        for s in range(S_ + 1):
            e = min(b, a + s * per)
            edges.update(r for r in (e - 2, e - 1, e, e + 1) if 0 <= r < n)
    edges = np.array(sorted(edges) + [n, n + 7, 2 ** 32, 2 ** 40], np.int64)
    for qi in (1, 0):
        qs = np.repeat(q[qi:qi + 1], len(edges), 0)
        Ss = np.repeat(S[qi:qi + 1], len(edges), 0)
        top = (np.full(len(edges), whole[qi][0][0], np.float32), edges)
        after_ref.assert_same(idx.search_after(qs, 70, top), want_of(Ss, top, 70), f"query {qi}: edge rows at the best score")
        own = (np.where(edges < n, S[qi, np.minimum(edges, n - 1)], whole[qi][0][500]).astype(np.float32), edges)
        after_ref.assert_same(idx.search_after(qs, 70, own), want_of(Ss, own, 70), f"query {qi}: edge rows at their own score")
    # exhausted, start, NaN and +-Inf cursors on every shard alike
    sc = np.array([0, 0, np.nan, np.inf, -np.inf, -0.0], np.float32)
    rows = np.array([-1, -2, 4, 0, 0, 998], np.int64)
    want = want_of(S, (sc, rows), 30)
    assert (want[1][0] == -1).all() and (want[1][2] == -1).all() and (want[1][4] == -1).all() and want[1][3].tolist() == whole[3][1][:30].tolist()
    after_ref.assert_same(idx.search_after(q, 30, (sc, rows)), want, "special cursors")
    idx.check_status()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_search_after_across_ranks_sharing_the_gpu(world):
    """`world` processes (tests/_gloo_worker_after.py hip) each hold one contiguous shard of the tie corpus on the GPU, search
    behind the same global-position cursor with pos_base = their shard's first row, all-gather the keys over gloo and merge on
    the device; each rank compares with the reference over the whole corpus."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_gloo_worker_after.py")
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
