"""search_grouped: hac_index_search_grouped* (scan16_grouped_kernel and grouped_select_kernel of csrc/grouped.inc) through
FlatIPIndex, i.e. the C ABI.

Every assertion is equality of I, G and of the bits of D with tests/grouped_ref.py, the definition of include/haconvdr.h
restated over the CPU oracle's canonical scores.  Indexes are built like _index() of tests/test_search_plans_gpu.py: three adds
cut off the 64-row grid, so the rows straddle segments and the last group is partial (5000 rows: 79 groups, the last of 8
rows), with the prefilter off.  Every case checks the host form and the tensor form and leaves the status word clean.  What the
inputs are good for is proved on the CPU in tests/test_index_grouped.py."""
import ctypes
import re

import numpy as np
import pytest

from haconvdr_amd import synth
from tests import grouped_cases, grouped_ref, masked_cases, nonfinite, rank_ref
from tests.test_index_among_gpu import _tie_corpus
from tests.test_index_rank_gpu import hostile_queries
from tests.test_index_rows_gpu import hostile_corpus
from tests.test_search_plans_gpu import _cuts, _index

pytestmark = pytest.mark.gpu

HAC_ERR_INVALID, HAC_ERR_UNSUPPORTED = 1, 4
MAX_K = grouped_cases.MAX_K
D, N, NQ = grouped_cases.D, grouped_cases.N, grouped_cases.NQ
_PLAN = re.compile(r"^scan16_grouped_kernel<W=(?P<W>\d+)> grid=\((?P<P>\d+),(?P<T>\d+)\) QT=(?P<QT>\d+) C=(?P<C>\d+) lds=(?P<lds>\d+) "
                   r"grouped_select_kernel n_in=(?P<n_in>\d+) launches=(?P<launches>\d+)$")


def parse_plan(text):
    m = _PLAN.match(text)
    assert m, "not the plan of a search by group: %r" % text
    return {k: int(v) for k, v in m.groupdict().items()}


def _cuda(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def tensor_form(idx, q, labels, k, id_map=None):
    """(D, I, G) of search_grouped_tensor as ndarrays"""
    import torch
    D, I, G = idx.search_grouped_tensor(_cuda(q, np.float32), k, _cuda(labels, np.int64), id_map=id_map, return_groups=True)
    torch.cuda.synchronize()
    return D.cpu().numpy(), I.cpu().numpy(), G.cpu().numpy()


def both_forms(idx, q, labels, k, want, what=""):
    """host form (with and without G) and tensor form against the reference; the status word stays clean"""
    grouped_ref.assert_same(idx.search_grouped(q, k, labels, return_groups=True), want, f"{what} host form")
    grouped_ref.assert_same(idx.search_grouped(q, k, labels), want, f"{what} host form without G")
    grouped_ref.assert_same(tensor_form(idx, q, labels, k), want, f"{what} tensor form")
    idx.check_status()


_BASE = {}


def _base(oracle):
    """the shared case: rows, queries and their canonical scores, computed once and never changed"""
    if "case" not in _BASE:
        x, q = masked_cases.base_case()
        S = rank_ref.canon_scores(oracle, x, q)
        S.setflags(write=False)
        _BASE["case"] = (x, q, S)
    return _BASE["case"]


def _giant(oracle):
    if "giant" not in _BASE:
        x, q, labels = grouped_cases.giant_case()
        S = rank_ref.canon_scores(oracle, x, q)
        S.setflags(write=False)
        _BASE["giant"] = (x, q, labels, S)
    return _BASE["giant"]


# ---------------------------------------------------------------------------------------------------------------------
# 1. distinct labels against search; one label
@pytest.mark.parametrize("k", [1, 10, 100, 2047, 2048])
def test_distinct_labels_are_search(k, oracle):
    x, q, S = _base(oracle)
    idx = _index(D, x)
    labels = np.arange(N, dtype=np.int64)
    want = grouped_ref.grouped_from_scores(S, labels, k)
    grouped_ref.assert_same(idx.search(q, k), want, f"search k={k}")
    both_forms(idx, q, labels, k, want, f"arange labels k={k}")
    plan = parse_plan(idx.last_plan())
    QT, C, lds = grouped_cases.plan_tile(D, k, NQ)
    assert (plan["QT"], plan["C"], plan["lds"], plan["T"], plan["launches"], plan["W"]) == (QT, C, lds, -(-NQ // QT), 1, 4), plan
    assert 1 <= plan["P"] <= 20 and plan["n_in"] == plan["P"] * k, plan      # 79 groups: at most 20 streams of 4 waves
    # the same labels, spread over the 32 bits
    wide = labels * 858993 + 7
    assert wide.max() < 2 ** 32 and wide.max() > 2 ** 31
    grouped_ref.assert_same(idx.search_grouped(q, k, wide)[:2], want, "wide labels")


def test_one_label_is_the_best_row_and_padding(oracle):
    x, q, S = _base(oracle)
    idx = _index(D, x)
    for k in (1, 9):
        D1, I1 = idx.search(q, 1)
        for lab in (0, 77, 2 ** 32 - 1):
            labels = np.full(N, lab, np.int64)
            want = grouped_ref.grouped_from_scores(S, labels, k)
            assert (want[1][:, :1] == I1).all() and (want[1][:, 1:] == -1).all() and (want[2][:, 0] == lab).all()
            both_forms(idx, q, labels, k, want, f"one label {lab} k={k}")


# ---------------------------------------------------------------------------------------------------------------------
# 2. a giant group leads every list: no threshold before k distinct groups, every compaction shrinks to a handful
@pytest.mark.parametrize("k", [10, 100])
def test_giant_group(k, oracle):
    x, q, labels, S = _giant(oracle)
    want = grouped_ref.grouped_from_scores(S, labels, k)
    assert (want[2][:, 0] == 0).all() and (want[1] >= 0).all()
    idx = _index(D, x, grouped_p="1")
    both_forms(idx, q, labels, k, want, f"giant k={k} grouped_p=1")
    plan = parse_plan(idx.last_plan())
    assert plan["P"] == 1 and plan["C"] == 512 and plan["n_in"] == k, plan       # one workgroup walks every compaction: 20 rounds of 4 groups
    one = tensor_form(idx, q, labels, k)
    idx.set_option("grouped_p", "auto")
    both_forms(idx, q, labels, k, want, f"giant k={k} grouped_p=auto")
    assert parse_plan(idx.last_plan())["P"] > 1
    auto = tensor_form(idx, q, labels, k)
    for a, b in zip(one, auto):
        assert a.tobytes() == b.tobytes()
    idx.set_option("grouped_p", "3")
    both_forms(idx, q, labels, k, want, f"giant k={k} grouped_p=3")
    assert parse_plan(idx.last_plan())["P"] == 3


def test_set_option_values():
    from haconvdr_amd import _lib
    idx = _index(D, synth.embeddings(0xB50, 100, D))
    for name, bad in (("grouped_p", "0"), ("grouped_p", "4097"), ("grouped_p", "x"), ("debug_grouped_tiles", "-1"), ("debug_grouped_tiles", "many")):
        with pytest.raises(_lib.HacError) as err:
            idx.set_option(name, bad)
        assert err.value.code == HAC_ERR_INVALID
    for name, good in (("grouped_p", "1"), ("grouped_p", "4096"), ("grouped_p", "auto"), ("debug_grouped_tiles", "2"), ("debug_grouped_tiles", "0")):
        idx.set_option(name, good)


# ---------------------------------------------------------------------------------------------------------------------
# 3. interleaving: k at the label count's edges
@pytest.mark.parametrize("name", ["r % 7", "r // 3", "permuted r // 5"])
def test_interleaved_groups_and_k_at_the_label_count(name, oracle):
    x, q, S = _base(oracle)
    q, S = q[:17], S[:17]
    labels = grouped_cases.interleaved_labels()[name]
    n_labels = len(np.unique(labels))
    idx = _index(D, x)
    for k in (n_labels - 1, n_labels, n_labels + 1):
        want = grouped_ref.grouped_from_scores(S, labels, k)
        assert (want[1][:, :min(k, n_labels)] >= 0).all() and (want[1][:, n_labels:] == -1).all()      # the padding starts where the labels end
        both_forms(idx, q, labels, k, want, f"{name} k={k}")
    idx.set_option("grouped_p", "1")
    k = min(n_labels, 50)
    both_forms(idx, q, labels, k, grouped_ref.grouped_from_scores(S, labels, k), f"{name} k={k} grouped_p=1")


# ---------------------------------------------------------------------------------------------------------------------
# 4. ties
def test_ties_inside_and_across_groups(oracle):
    d, n, nq = 96, 1000, 6
    x, q = _tie_corpus(d, n, nq, 0xB60)
    S = rank_ref.canon_scores(oracle, x, q)
    idx = _index(d, x)
    r = np.arange(n, dtype=np.int64)
    # a group of identical rows: its representative is its lowest row
    inside = r % 16
    want = grouped_ref.grouped_from_scores(S, inside, 20)
    assert (np.sort(want[1][:, :16], axis=1) == np.arange(16)).all() and (want[1][:, 16:] == -1).all()
    both_forms(idx, q, inside, 20, want, "identical rows inside a group")
    # groups of four different rows: dozens of groups tie, ordered by their representative's row
    across = r // 4
    for k in (37, 250):
        want = grouped_ref.grouped_from_scores(S, across, k)
        same = np.diff(want[0], axis=1) == 0
        assert same.sum() > nq * min(k, 100) // 2 and (np.diff(want[1], axis=1)[same] > 0).all()
        both_forms(idx, q, across, k, want, f"ties across groups k={k}")
    # a grid-valued corpus: whole runs of groups tie at the k-th score
    x, q, g = grouped_cases.grid_tie_corpus(96, 1200, 6, 0xB40)
    S = rank_ref.canon_scores(oracle, x, q)
    idx = _index(96, x)
    for k in (37, 150, 300, 301):
        both_forms(idx, q, g, k, grouped_ref.grouped_from_scores(S, g, k), f"grid ties k={k}")
    idx.set_option("grouped_p", "1")
    both_forms(idx, q, g, 37, grouped_ref.grouped_from_scores(S, g, 37), "grid ties k=37 grouped_p=1")


# ---------------------------------------------------------------------------------------------------------------------
# 5. label edges
def test_label_edges(oracle):
    from haconvdr_amd import _lib
    from haconvdr_amd.index import _f32p, _i64p
    x, q, S = _base(oracle)
    q, S = q[:9], S[:9]
    idx = _index(D, x)
    e = grouped_cases.edge_labels()
    for k in (5, 11, 12):
        want = grouped_ref.grouped_from_scores(S, e, k)
        assert (want[2][:, :min(k, 11)] >= 0).all()
        both_forms(idx, q, e, k, want, f"edge labels k={k}")
    # out of range: the host form refuses, names the first offending row and writes nothing
    best = grouped_ref.grouped_from_scores(S, e, 11)[1]
    Dh = np.full((9, 11), np.float32(-123.5))
    Ih = np.full((9, 11), -99, np.int64)
    Gh = np.full((9, 11), -98, np.int64)
    for at, bad in ((int(best[0, 0]), -1), (int(best[0, 1]), 2 ** 32), (N - 1, np.iinfo(np.int64).min)):
        wild = e.copy()
        wild[at] = bad
        wild[N - 1] = bad if at == N - 1 else 2 ** 40                      # a later offender too: the FIRST is named
        rc = _lib.lib().hac_index_search_grouped(idx._h, _f32p(q), 9, 11, _i64p(wild), N, _f32p(Dh), _i64p(Ih), _i64p(Gh))
        msg = _lib.lib().hac_last_error().decode()
        assert rc == HAC_ERR_INVALID and f"group_of[{at}]" in msg and str(bad) in msg, msg
        with pytest.raises(_lib.HacError) as err:
            idx.search_grouped(q, 11, wild)
        assert err.value.code == HAC_ERR_INVALID and f"group_of[{at}]" in str(err.value)
    assert (Dh == np.float32(-123.5)).all() and (Ih == -99).all() and (Gh == -98).all()
    # the tensor form cannot look: those rows are in no list, and a group that loses its best row is represented by its next
    wild = e.copy()
    lost = [int(best[i, 0]) for i in range(9)] + [int(best[0, 1])]
    wild[lost[::2]] = -1
    wild[lost[1::2]] = 2 ** 32
    wild[7::50] = np.iinfo(np.int64).min
    wild[8::50] = 2 ** 63 - 1
    for k in (3, 11, 12):
        want = grouped_ref.grouped_from_scores(S, wild, k)
        assert not np.isin(want[1], lost).any() and (want[2][:, :min(k, 11)] >= 0).all() and (want[2] < 2 ** 32).all()
        grouped_ref.assert_same(tensor_form(idx, q, wild, k), want, f"labels out of range, tensor form k={k}")
    idx.set_option("grouped_p", "1")
    grouped_ref.assert_same(tensor_form(idx, q, wild, 3), grouped_ref.grouped_from_scores(S, wild, 3), "labels out of range, one row stream")
    nowhere = np.full(N, -5, np.int64)                                     # no legal label at all: padding only
    grouped_ref.assert_same(tensor_form(idx, q, nowhere, 4), grouped_ref.grouped_from_scores(S, nowhere, 4), "no legal label")
    # the library's own argument checks (the C ABI called directly), then ValueErrors on real CUDA tensors
    import torch
    qt, gt = _cuda(q, np.float32), _cuda(e, np.int64)
    L = _lib.lib()
    for nq_, k_, n_ in ((9, 0, N), (9, MAX_K + 1, N), (9, 5, N - 1), (9, 5, N + 64), (-1, 5, N)):
        assert L.hac_index_search_grouped_device(idx._h, qt.data_ptr(), nq_, k_, gt.data_ptr(), n_, None, None, None, None, None) == HAC_ERR_INVALID
        assert L.hac_index_search_grouped(idx._h, _f32p(q), nq_, k_, _i64p(e), n_, _f32p(Dh), _i64p(Ih), None) == HAC_ERR_INVALID
    assert "one label per row" in L.hac_last_error().decode() or "bad arguments" in L.hac_last_error().decode()
    for args in ((qt, 0, gt), (qt, MAX_K + 1, gt), (qt, 5, gt[:-1]), (qt, 5, gt.reshape(50, 100)), (qt, 5, gt.to(torch.int32)), (qt, 5, gt.double()),
                 (qt, 5, gt.cpu()), (qt.cpu(), 5, gt), (qt[:, :-1], 5, gt)):
        with pytest.raises(ValueError):
            idx.search_grouped_tensor(*args)
    with pytest.raises(ValueError):
        idx.search_grouped_tensor(qt, 5, gt, id_map=gt.cpu())
    for args in ((q, 5, e.astype(np.float32)), (q, 5, e[:-1]), (q, 5, e.reshape(50, 100)), (q, 0, e), (q, MAX_K + 1, e)):
        with pytest.raises(ValueError):
            idx.search_grouped(*args)
    D0, I0, G0 = idx.search_grouped(np.zeros((0, D), np.float32), 7, e, return_groups=True)      # nq == 0: HAC_OK, nothing touched
    assert D0.shape == I0.shape == G0.shape == (0, 7)
    D0, I0 = idx.search_grouped_tensor(torch.zeros((0, D), device="cuda"), 7, gt)
    assert tuple(D0.shape) == tuple(I0.shape) == (0, 7)
    both_forms(idx, q, e, 11, grouped_ref.grouped_from_scores(S, e, 11), "after the refused calls")


# ---------------------------------------------------------------------------------------------------------------------
# 6. tiles and launches
def _forty(oracle):
    if "forty" not in _BASE:
        x = _base(oracle)[0]
        q = synth.embeddings(0xB70, 40, D)
        _BASE["forty"] = (q, rank_ref.canon_scores(oracle, x, q))
    return _BASE["forty"]


@pytest.mark.parametrize("k", [10, 1000, 2048])
def test_tiles_and_launches(k, oracle):
    x = _base(oracle)[0]
    q, S = _forty(oracle)
    labels = grouped_cases.interleaved_labels()["r // 3"]
    idx = _index(D, x)
    for nq in (1, 15, 16, 17, 40):
        want = grouped_ref.grouped_from_scores(S[:nq], labels, k)
        both_forms(idx, q[:nq], labels, k, want, f"nq={nq} k={k}")
        plan = parse_plan(idx.last_plan())
        QT, C, lds = grouped_cases.plan_tile(D, k, nq)
        assert (plan["QT"], plan["C"], plan["lds"], plan["T"], plan["launches"]) == (QT, C, lds, -(-nq // QT), 1), plan
    QT = grouped_cases.plan_tile(D, k, 40)[0]
    assert QT == {10: 16, 1000: 5, 2048: 2}[k]                             # the scratch arrays take LDS: QT < 16 at large k
    want = grouped_ref.grouped_from_scores(S, labels, k)
    whole = tensor_form(idx, q, labels, k)
    idx.set_option("debug_grouped_tiles", "1")                             # a launch per tile
    both_forms(idx, q, labels, k, want, f"one tile per launch k={k}")
    plan = parse_plan(idx.last_plan())
    assert plan["T"] == 1 and plan["launches"] == -(-40 // QT), plan
    cut = tensor_form(idx, q, labels, k)
    for a, b in zip(whole, cut):
        assert a.tobytes() == b.tobytes()
    idx.set_option("debug_grouped_tiles", "2")
    both_forms(idx, q[:17], labels, k, grouped_ref.grouped_from_scores(S[:17], labels, k), f"two tiles per launch k={k}")
    assert parse_plan(idx.last_plan())["launches"] == -(-(-(-17 // min(QT, 17))) // 2)


# ---------------------------------------------------------------------------------------------------------------------
# 7. non-finite queries and hostile rows
@pytest.mark.parametrize("kind", nonfinite.KINDS)
def test_nonfinite_queries(kind, oracle):
    d, n, nq, k = 96, 3001, 33, 100
    x, q, pos, _ = nonfinite.case(kind, d, n, nq, 0xB80)
    with np.errstate(all="ignore"):
        S = rank_ref.canon_scores(oracle, x, q)
    labels = (np.arange(n, dtype=np.int64) * 7) % 431
    want = grouped_ref.grouped_from_scores(S, labels, k)
    if kind in nonfinite.NAN_KINDS:
        assert all((want[1][i] == -1).all() for i in pos)                 # a NaN query: padding only
    if kind in nonfinite.INF_KINDS:
        assert all(np.isinf(want[0][i]).any() for i in pos)               # +-Inf are ordinary scores
    healthy = [i for i in range(nq) if i not in pos]
    assert (want[1][healthy] >= 0).all()
    idx = _index(d, x)
    both_forms(idx, q, labels, k, want, kind)


@pytest.mark.parametrize("d", [32, 96, 160])
def test_nan_rows_as_only_and_as_best_members(d, oracle):
    n, nq = 1000, 17
    x = hostile_corpus(0xB90 + d, n, d)
    q = hostile_queries(0xB91 + d, nq, d)
    with np.errstate(all="ignore"):
        S = rank_ref.canon_scores(oracle, x, q)
    nan_rows = np.flatnonzero(np.isnan(S[1:]).all(axis=0))                 # NaN under every query but the zero query's Inf * 0 as well
    nan_rows = nan_rows[np.isnan(S[0, nan_rows])]
    assert len(nan_rows) >= 8
    labels = np.arange(n, dtype=np.int64) // 2 + 1000                      # pairs (2j, 2j + 1)
    alone = nan_rows[0::2]
    labels[alone] = 5000 + np.arange(len(alone))                           # NaN rows as their group's only members: the group is absent
    shared = nan_rows[1::2]                                                # NaN rows with a partner: the partner represents the group
    for k in (1, 100, 600):
        want = grouped_ref.grouped_from_scores(S, labels, k)
        assert not np.isnan(want[0]).any() and not np.isin(want[2], labels[alone]).any() and not np.isin(want[1], nan_rows).any()
        both_forms(_index(d, x), q, labels, k, want, f"d={d} k={k}")
    full = grouped_ref.grouped_from_scores(S, labels, 600)
    partners = [r ^ 1 for r in shared if labels[r ^ 1] == labels[r] and not np.isnan(S[2, r ^ 1])]
    assert len(partners) >= 2 and np.isin(partners, full[1][2]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 8. index lifetime
def test_after_remove_and_after_reset(oracle):
    from haconvdr_amd import _lib
    from haconvdr_amd.index import _f32p, _i64p
    d, n, nq, k = 96, 1000, 5, 50
    x = synth.embeddings(0xBA0, n, d)
    q = synth.embeddings(0xBA1, nq, d)
    idx = _index(d, x)
    labels = (np.arange(n, dtype=np.int64) * 13) % 211
    both_forms(idx, q, labels, k, grouped_ref.grouped(oracle, x, q, labels, k), "as built")
    gone = np.arange(100, 900, 7)
    assert idx.remove_ids(gone) == len(gone)
    left = np.delete(x, gone, 0)
    # labels of the old length are refused, by the Python check and by the library, on both forms
    with pytest.raises(ValueError):
        idx.search_grouped(q, k, labels)
    with pytest.raises(ValueError):
        idx.search_grouped_tensor(_cuda(q, np.float32), k, _cuda(labels, np.int64))
    Dh, Ih = np.zeros((nq, k), np.float32), np.zeros((nq, k), np.int64)
    rc = _lib.lib().hac_index_search_grouped(idx._h, _f32p(q), nq, k, _i64p(labels), n, _f32p(Dh), _i64p(Ih), None)
    assert rc == HAC_ERR_INVALID and "n_labels=" in _lib.lib().hac_last_error().decode()
    rc = _lib.lib().hac_index_search_grouped_device(idx._h, _cuda(q, np.float32).data_ptr(), nq, k, _cuda(labels, np.int64).data_ptr(), n, None, None, None, None, None)
    assert rc == HAC_ERR_INVALID
    kept = np.delete(labels, gone)
    both_forms(idx, q, kept, k, grouped_ref.grouped(oracle, left, q, kept, k), "after remove_ids")
    # reset() and a smaller add(): the stale rows behind the new ntotal are in no group
    idx.reset()
    small = synth.embeddings(0xBA3, 130, d)
    idx.add(small)
    few = np.arange(130, dtype=np.int64) % 100
    want = grouped_ref.grouped(oracle, small, q, few, 200)
    assert (want[1][:, :100] >= 0).all() and (want[1][:, 100:] == -1).all()
    both_forms(idx, q, few, 200, want, "after reset and a smaller add")
    idx.reset()                                                            # an empty index: padding only, no labels
    none = np.zeros(0, np.int64)
    empty = (np.full((nq, 4), -grouped_ref.FMAX, np.float32), np.full((nq, 4), -1, np.int64), np.full((nq, 4), -1, np.int64))
    both_forms(idx, q, none, 4, empty, "empty index")


# ---------------------------------------------------------------------------------------------------------------------
# 9. id_map, return_groups, capture
def test_id_map_groups_and_capture(oracle):
    import torch
    d, n, nq, k = 96, 1000, 17, 64
    x = hostile_corpus(0xBC0, n, d)
    qs = [hostile_queries(0xBC1 + r, nq, d) for r in range(2)]
    labels = [(np.arange(n, dtype=np.int64) * (3 + 4 * r)) % (97 + 300 * r) + 2 ** 31 * r for r in range(2)]     # few large groups, then many small ones
    ids = (np.arange(n, dtype=np.int64) * 7919) % 100003 + 10 ** 10       # external ids: nothing like a row or a label
    with np.errstate(all="ignore"):
        wants = [grouped_ref.grouped(oracle, x, qs[r], labels[r], k) for r in range(2)]
    idx = _index(d, x)
    qt, gt, it = _cuda(qs[0], np.float32), _cuda(labels[0], np.int64), _cuda(ids, np.int64)
    Dm, Im, Gm = tensor_form(idx, qs[0], labels[0], k, id_map=it)
    wD, wI, wG = wants[0]
    grouped_ref.assert_same((Dm, Im, Gm), (wD, np.where(wI >= 0, ids[wI], -1), wG), "I = id_map[row], G the row's own label")
    D2, I2 = idx.search_grouped_tensor(qt, k, gt, id_map=it)               # without G
    torch.cuda.synchronize()
    grouped_ref.assert_same((D2.cpu().numpy(), I2.cpu().numpy()), (wD, np.where(wI >= 0, ids[wI], -1), wG), "id_map, no G")
    side = torch.cuda.Stream()                            # a single stream: no parallel branches in the graph
    replayed = []
    with torch.cuda.stream(side):
        eager = idx.search_grouped_tensor(qt, k, gt, return_groups=True)   # the largest shape once: workspaces and the segment table exist
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            Dg, Ig, Gg = idx.search_grouped_tensor(qt, k, gt, return_groups=True)
        for r in (1, 0):
            qt.copy_(torch.from_numpy(qs[r]))
            gt.copy_(torch.from_numpy(labels[r]))
            Dg.zero_()
            Ig.fill_(-7)
            Gg.fill_(-7)
            g.replay()
            side.synchronize()
            replayed.append((r, Dg.cpu().numpy(), Ig.cpu().numpy(), Gg.cpu().numpy()))
    torch.cuda.synchronize()
    grouped_ref.assert_same(tuple(t.cpu().numpy() for t in eager), wants[0], "eager")
    for r, Dr, Ir, Gr in replayed:
        grouped_ref.assert_same((Dr, Ir, Gr), wants[r], f"replay on contents {r}")
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 10. several shards in one process
def _multi_device(devices, oracle):
    from haconvdr_amd import _lib
    d, n, nq = 96, 1501, 9
    x = synth.embeddings(0xBD0, n, d)
    q = synth.embeddings(0xBD1, nq, d)
    S = rank_ref.canon_scores(oracle, x, q)
    idx = _index(d, x, devices=devices)
    r = np.arange(n, dtype=np.int64)
    c1, c2 = _cuts(n)
    per = -(-c1 // len(devices))
    across = r % 50                                                        # every group has rows on every shard, in every add
    edge = np.where((r >= per - 3) & (r < per + 3), 2 ** 32 - 1, r + 1)    # one group split across the first shard boundary, singletons else
    for name, labels in (("r % 50", across), ("split at the shard boundary", edge), ("r // 3", r // 3)):
        n_labels = len(np.unique(labels))
        for k in (1, 49, 50, 51, 400):
            want = grouped_ref.grouped_from_scores(S, labels, k)
            grouped_ref.assert_same(idx.search_grouped(q, k, labels, return_groups=True), want, f"{len(devices)} shards {name} k={k} of {n_labels}")
    grouped_ref.assert_same(idx.search(q, 5), grouped_ref.grouped_from_scores(S, r, 5), "search")
    wild = across.copy()
    wild[700] = -1
    with pytest.raises(_lib.HacError) as err:
        idx.search_grouped(q, 5, wild)
    assert err.value.code == HAC_ERR_INVALID and "group_of[700]" in str(err.value)
    with pytest.raises(_lib.HacError) as err:
        idx.search_grouped_tensor(_cuda(q, np.float32), 5, _cuda(across, np.int64))
    assert err.value.code == HAC_ERR_UNSUPPORTED
    idx.check_status()


@pytest.mark.parametrize("shards", [2, 3])
def test_several_shards_on_one_device(shards, oracle):
    _multi_device((0,) * shards, oracle)


def test_several_devices(oracle):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    _multi_device((0, 1), oracle)


# ---------------------------------------------------------------------------------------------------------------------
# 11. determinism, and the resident corpus's distinct passages
def test_two_identical_calls_return_identical_bytes():
    import torch
    d, n, nq, k = 96, 3000, 40, 300
    x, q = _tie_corpus(d, n, nq, 0xBE0)
    idx = _index(d, x)
    labels = (np.arange(n, dtype=np.int64) * 11) % 700
    qt, gt = _cuda(q, np.float32), _cuda(labels, np.int64)
    a = idx.search_grouped_tensor(qt, k, gt, return_groups=True)
    b = idx.search_grouped_tensor(qt, k, gt, return_groups=True)
    torch.cuda.synchronize()
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[2], b[2])
    h1, h2 = idx.search_grouped(q, k, labels, True), idx.search_grouped(q, k, labels, True)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(h1, h2))
    grouped_ref.assert_same(h1, tuple(t.cpu().numpy() for t in a), "host form vs tensor form")
    idx.check_status()


def test_resident_corpus_distinct_passages(oracle):
    """ResidentCorpus.search_distinct over a real index: the labels live on the device, I comes back through id_map"""
    import torch
    from haconvdr_amd.search import ResidentCorpus
    n, d, nq, k = 1000, 96, 9, 100
    x = synth.embeddings(0xBF0, n, d)
    q = synth.embeddings(0xBF1, nq, d)
    x[600:] = x[:400]                                                      # the second block repeats four hundred passages, bit for bit
    pids = np.arange(n, dtype=np.int64) * 5 + 3
    pids[600:] = pids[:400]
    rc = ResidentCorpus.__new__(ResidentCorpus)
    rc.index, rc._ids, rc._lookup = _index(d, x), pids, None
    rc.dev = torch.device("cuda", 0)
    rc.id_map = torch.from_numpy(pids).to(rc.dev)
    S = rank_ref.canon_scores(oracle, x, q)
    wD, wI, _ = grouped_ref.grouped_from_scores(S, pids, k)
    D, I = rc.search_distinct(q, k)
    assert D.dtype == np.float64 and all(len(set(I[i].tolist())) == k for i in range(nq))
    grouped_ref.assert_same((D.astype(np.float32), I), (wD, pids[wI], None), "distinct passages")
    assert (wI < 600).all()                                                # twins tie: the lower row represents the passage
    sI = rc.search(q, k)[1]
    assert all(len(set(sI[i].tolist())) < k for i in range(nq))            # the plain search repeats passage ids inside its top 100
    page_of = np.arange(pids.max() + 1, dtype=np.int64) // 50              # pages of ten passages
    wD, wI, _ = grouped_ref.grouped_from_scores(S, page_of[pids], 60)
    D, I = rc.search_distinct(torch.from_numpy(q).cuda(), 60, group_of=page_of)
    grouped_ref.assert_same((D.astype(np.float32), I), (wD, pids[wI], None), "distinct pages")
    assert rc.remove(pids[:10]) == 20                                      # the default labels are renewed with the rows
    left = np.delete(np.arange(n), np.concatenate([np.arange(10), np.arange(600, 610)]))
    wD, wI, _ = grouped_ref.grouped_from_scores(S[:, left], pids[left], k)
    D, I = rc.search_distinct(q, k)
    grouped_ref.assert_same((D.astype(np.float32), I), (wD, pids[left][wI], None), "after remove")
    rc.index.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 12. the host form across its staging chunks: the queries go 64 MiB // 4d at a time through the pinned slab.  d = 1024 (the
# widest row: the fewest queries per chunk), 200 hostile rows on two shards of one device, so the slice of the labels and the
# remap take part; the case and its scores are those of tests/test_index_masked_gpu.py's section 13.
@pytest.mark.parametrize("past", [0, 1])
def test_host_form_across_a_query_chunk(past, oracle):
    from tests.test_index_masked_gpu import SEAM_BYTES, SEAM_D, SEAM_K, SEAM_N, SEAM_NQ, seam_case
    x, q, S = seam_case(oracle)
    chunk = SEAM_BYTES // (4 * SEAM_D)
    assert chunk == 16384 and chunk + 1 == SEAM_NQ
    nq = chunk + past
    labels = (np.arange(SEAM_N, dtype=np.int64) * 7) % 23                  # every group has rows on both shards
    want = grouped_ref.grouped_from_scores(S[:nq], labels, SEAM_K)
    assert (want[1][4:] >= 0).all()
    idx = _index(SEAM_D, x, devices=(0, 0))
    grouped_ref.assert_same(idx.search_grouped(q[:nq], SEAM_K, labels, return_groups=True), want, f"{nq} queries, chunks of {chunk}")
    plan = parse_plan(idx.last_plan())
    assert (plan["QT"] == 1) == (past == 1), plan                          # the last chunk held one query, or a full tile's
    idx.check_status()
