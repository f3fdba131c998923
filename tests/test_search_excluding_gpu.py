"""Exact top-k with per-query excluded rows: hac_index_search_excluding*, hac_filter_keys_device and their Python mirrors
(FlatIPIndex.search_excluding / search_excluding_tensor, index.filter_keys, ResidentCorpus.search(exclude=)).

Every comparison is bitwise, ids and scores, every query and every position, against two independent host expectations
(tests/excluding.py): (a) the oracle's top-(k + e) filtered in numpy, and (b) the oracle's top-k over the corpus with the
excluded rows deleted -- (b) does not assume that the answer lies inside the top-(k + e); that (a) == (b) is what proves it.
Indexes are built like those of tests/test_search_plans_gpu.py (three adds off the 64-row grid, a partial last group) and
the status word is clean after every search."""
import ctypes

import numpy as np
import pytest

from haconvdr_amd import synth
from tests import excluding
from tests.excluding import FMAX
from tests.golden import cases
from tests.test_search_plans_gpu import _index, _seed, parse_plan

pytestmark = pytest.mark.gpu


def _same(got, want, what):
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"{what}: ids")
    np.testing.assert_array_equal(np.asarray(got[0], np.float32).view(np.uint32), want[0].view(np.uint32), err_msg=f"{what}: scores")


def _excl(idx, q, k, E):
    out = idx.search_excluding(q, k, E)
    idx.check_status()
    return out


def _excl_tensor(idx, q, k, E, id_map=None):
    import torch
    D, I = idx.search_excluding_tensor(torch.from_numpy(q).cuda(), k, torch.from_numpy(np.ascontiguousarray(E, np.int64)).cuda(),
                                       id_map=None if id_map is None else torch.from_numpy(id_map).cuda())
    torch.cuda.synchronize()
    idx.check_status()
    return D.cpu().numpy(), I.cpu().numpy()


_CORPUS = {}


def _corpus(d):
    """(x, q, index with the prefilter off) for n = 1000, nq = 9: built once per dimension and left unchanged."""
    if d not in _CORPUS:
        n, nq = 1000, 9
        x, q, _ = cases.search_case_inputs("gauss", _seed(d, n, nq, 0, 7), n, nq, d=d)
        _CORPUS[d] = (x, q, _index(d, x))
    return _CORPUS[d]


# ---------------------------------------------------------------------------------------------------------------------
# 1. two independent expectations
@pytest.mark.parametrize("k, e", [(1, 1), (10, 3), (100, 7)])
@pytest.mark.parametrize("d", [64, 96, 768])
def test_excluding_equals_both_expectations(d, k, e, oracle):
    x, q, idx = _corpus(d)
    plain = oracle.flat_ip_search(x, q, k)
    for name, E in excluding.exclusion_sets(oracle, x, q, k, e).items():
        a = excluding.filtered_topk(oracle, x, q, k, E)
        b = excluding.deleted_topk(oracle, x, q, k, E)
        _same(a, b, f"{name}: the two expectations")
        _same(_excl(idx, q, k, E), a, name)
        if name in ("outside top-(k+e)", "e = 0"):               # nothing of the top-(k + e) named: search itself, bit for bit
            _same(a, plain, f"{name}: expectation vs plain search")
            got = idx.search(q, k)
            idx.check_status()
            _same(_excl(idx, q, k, E), got, f"{name}: vs search")
        elif name == "own top-e":                                # the whole list shifts by e
            assert not np.isin(a[1][:, 0], E).any() and not np.array_equal(a[1], plain[1])


# ---------------------------------------------------------------------------------------------------------------------
# 2. ties
def test_second_twin_takes_the_place_of_an_excluded_first_twin(oracle):
    """Rows 2j and 2j + 1 are identical and grid-valued (multiples of 1/8): they tie exactly and sit next to each other in
    every list, so the top-2e is e whole pairs.  Without the first twins the second twins lead, in the same (row) order."""
    d, pairs, nq, k, e = 64, 100, 6, 10, 5
    x = np.repeat(cases.grid_vectors(0x71E5, pairs, d), 2, axis=0)
    q = cases.grid_vectors(0x71E6, nq, d)
    idx = _index(d, x)
    _, top = oracle.flat_ip_search(x, q, k + e)
    assert (top[:, 0:2 * e:2] % 2 == 0).all() and (top[:, 1:2 * e:2] == top[:, 0:2 * e:2] + 1).all()
    E = top[:, 0:2 * e:2].copy()
    D, I = _excl(idx, q, k, E)
    np.testing.assert_array_equal(I[:, :e], E + 1)
    np.testing.assert_array_equal(I[:, e:], top[:, 2 * e:k + e])
    a = excluding.filtered_topk(oracle, x, q, k, E)
    _same(a, excluding.deleted_topk(oracle, x, q, k, E), "the two expectations")
    _same((D, I), a, "twins")
    _same(_excl_tensor(idx, q, k, E), a, "twins, tensor form")


# ---------------------------------------------------------------------------------------------------------------------
# 3. short corpora
@pytest.mark.parametrize("n, k, e", [(50, 10, 45), (5, 10, 2)])
def test_short_corpora_pad(n, k, e, oracle):
    d, nq = 64, 5
    x, q, _ = cases.search_case_inputs("gauss", _seed(d, n, nq, k, 3), n, nq, d=d)
    idx = _index(d, x)
    order = np.argsort(synth.uniform_u32(0x5407 + n, n), kind="stable").astype(np.int64)
    E = np.stack([np.roll(order, i)[:e] for i in range(nq)])            # e distinct rows, another set for every query
    assert all(len(set(r)) == e for r in E.tolist())
    a = excluding.filtered_topk(oracle, x, q, k, E)
    _same(a, excluding.deleted_topk(oracle, x, q, k, E), "the two expectations")
    got = _excl(idx, q, k, E)
    _same(got, a, "host form")
    left = n - e
    assert (got[1][:, :left] >= 0).all() and (got[1][:, left:] == -1).all() and (got[0][:, left:] == -FMAX).all()
    _same(_excl_tensor(idx, q, k, E), a, "tensor form")
    mapped = np.where(a[1] >= 0, order[np.clip(a[1], 0, None)], -1)      # id_map: a permutation of the rows; -1 stays -1
    _same(_excl_tensor(idx, q, k, E, id_map=order), (a[0], mapped), "tensor form with id_map")


# ---------------------------------------------------------------------------------------------------------------------
# 4. route edges: every route decision is made for k' = k + e
@pytest.mark.parametrize("form", ["host", "tensor"])
def test_route_is_decided_for_k_plus_e(form, oracle):
    d, k = 768, 100
    x, q, idx = _corpus(d)                                       # n = 1000
    _, top = oracle.flat_ip_search(x, q, k + 2 * 93)
    call = _excl if form == "host" else _excl_tensor
    idx.set_option("split", "1")
    try:
        for e, prefilter in ((92, True), (93, False)):
            E = top[:, 0:2 * e:2].copy()
            got = call(idx, q, k, E)
            plan = idx.last_plan()
            if prefilter:
                assert plan.startswith("split:"), (e, plan)     # k' = 192: the last k the prefilter takes
            else:
                parse_plan(plan)                                 # k' = 193: an exact scan's plan text, or this raises
            _same(got, excluding.filtered_topk(oracle, x, q, k, E), f"e = {e}")
    finally:
        idx.set_option("split", "0")                             # the corpus is shared


# ---------------------------------------------------------------------------------------------------------------------
# 5. ceiling
def test_ceiling_k_plus_e(oracle):
    from haconvdr_amd import _lib
    d, n, nq, k = 64, 2200, 3, 2000
    x, q, _ = cases.search_case_inputs("gauss", _seed(d, n, nq, k, 5), n, nq, d=d)
    idx = _index(d, x)
    _, top = oracle.flat_ip_search(x, q, 2 * 49)
    E = top[:, 0:96:2].copy()                                            # e = 48: k' = 2048
    _same(_excl(idx, q, k, E), excluding.filtered_topk(oracle, x, q, k, E), "k' = 2048")
    E49 = np.ascontiguousarray(top[:, 0:98:2])
    D, I = np.empty((nq, k), np.float32), np.empty((nq, k), np.int64)
    with pytest.raises(_lib.HacError) as err:                            # the C ABI itself, not the Python check before it
        _lib.check(_lib.lib().hac_index_search_excluding(idx._h, q.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), nq, k,
                                                         E49.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 49,
                                                         D.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                         I.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
    assert err.value.code == _lib.HAC_ERR_INVALID
    assert all(s in str(err.value) for s in ("2000", "49", "2048")), str(err.value)
    with pytest.raises(ValueError):
        idx.search_excluding(q, k, E49)
    import torch
    with pytest.raises(ValueError):
        idx.search_excluding_tensor(torch.from_numpy(q).cuda(), k, torch.from_numpy(E49).cuda())
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 6. ids outside the index
def test_ids_outside_the_index(oracle):
    from haconvdr_amd._lib import HAC_ERR_INVALID, HacError
    d, k, e = 96, 10, 3
    x, q, idx = _corpus(d)
    n = len(x)
    _, top = oracle.flat_ip_search(x, q, e)
    for bad in (n, -2):
        E = top.copy()
        E[4, 1] = bad
        with pytest.raises(HacError) as err:
            idx.search_excluding(q, k, E)
        assert err.value.code == HAC_ERR_INVALID
        msg = str(err.value)
        assert f"id {bad} " in msg and "query 4" in msg and "column 1" in msg, msg
        without = E.copy()
        without[4, 1] = -1
        want = excluding.filtered_topk(oracle, x, q, k, without)
        _same(_excl_tensor(idx, q, k, E), want, f"tensor form ignores {bad}")
        _same(_excl(idx, q, k, without), want, "host form, -1 in its place")


# ---------------------------------------------------------------------------------------------------------------------
# 7. every entry agrees
def test_every_entry_agrees(oracle):
    import torch
    from haconvdr_amd.index import filter_keys, keys_to_results, merge_keys
    d, k, e = 768, 10, 3
    x, q, idx = _corpus(d)
    n = len(x)
    E = excluding.exclusion_sets(oracle, x, q, k, e)["duplicates and holes"]
    E[0] = [int(v) for v in oracle.flat_ip_search(x, q[:1], e)[1][0]]    # and one list without holes
    want = excluding.filtered_topk(oracle, x, q, k, E)
    _same(_excl(idx, q, k, E), want, "search_excluding")
    _same(_excl_tensor(idx, q, k, E), want, "search_excluding_tensor")
    perm = np.argsort(synth.uniform_u32(0xE7, n), kind="stable").astype(np.int64)               # row -> external id: a permutation
    mapped = (want[0], perm[want[1]])
    _same(_excl_tensor(idx, q, k, E, id_map=perm), mapped, "search_excluding_tensor with id_map")
    qt, Et = torch.from_numpy(q).cuda(), torch.from_numpy(E).cuda()
    keys = idx.search_keys_tensor(qt, k + e)
    D, I = keys_to_results(filter_keys(keys, Et, k))
    torch.cuda.synchronize()
    idx.check_status()
    _same((D.cpu().numpy(), I.cpu().numpy()), want, "search_keys_tensor -> filter_keys -> keys_to_results")
    # two shards emulated on one GPU: each half in an index of its own, global positions by pos_base, merged, then filtered
    h = 487
    halves = [(_index(d, x[:h]), 0), (_index(d, x[h:]), h)]
    lists = torch.stack([ix.search_keys_tensor(qt, k + e, pos_base=base) for ix, base in halves])
    D2, I2 = keys_to_results(filter_keys(merge_keys(lists), Et, k))
    torch.cuda.synchronize()
    for ix, _ in halves:
        ix.check_status()
    _same((D2.cpu().numpy(), I2.cpu().numpy()), want, "two shards: search_keys -> merge_keys -> filter_keys")


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)])
def test_host_form_on_a_multi_device_index(devices, oracle):
    """Several shards (here on one GPU): they search k + e, are remapped to insertion order and merged at k + e, the filter runs
    once.  The device form has no multi-device form."""
    import torch
    from haconvdr_amd._lib import HAC_ERR_UNSUPPORTED, HacError
    d = 768
    x, q, _ = _corpus(d)
    idx = _index(d, x, devices=devices)
    for k, e in ((10, 3), (100, 7)):
        sets = excluding.exclusion_sets(oracle, x, q, k, e)
        for name, E in sets.items():
            _same(_excl(idx, q, k, E), excluding.filtered_topk(oracle, x, q, k, E), f"{name}, k = {k}")
    with pytest.raises(HacError) as err:
        idx.search_excluding_tensor(torch.from_numpy(q).cuda(), 10, torch.from_numpy(sets["own top-e"]).cuda())
    assert err.value.code == HAC_ERR_UNSUPPORTED


def test_filter_keys_alone():
    """The kernel on keys it did not make: positions up to 0xFFFFFFFF, padding above and below, an empty tail, kin on both
    sides of a multiple of 64, kout < kin survivors and kout > survivors, more exclusions than one chunk of 64."""
    import torch
    from haconvdr_amd.index import filter_keys
    from tests import doubles, doubles_filter
    nq = 5
    for kin, e, k in ((1, 1, 1), (64, 3, 64), (65, 70, 40), (200, 129, 200), (2048, 2047, 100)):
        fill = max(1, kin - 7)
        pos = np.full((nq, kin), -1, np.int64)
        sc = np.zeros((nq, kin), np.float32)
        for i in range(nq):
            p = np.unique(synth.uniform_u32(0xF17 + 31 * i + kin, 2 * kin).astype(np.int64))[:fill]
            p[-1] = 0xFFFFFFFF
            p[0] = 0
            pos[i, :len(p)] = p[np.argsort(synth.uniform_u32(0xF18 + i, len(p)), kind="stable")]
            sc[i, :len(p)] = (len(p) // 2 - np.arange(len(p))) * 0.125 * (i + 1)       # strictly descending, both signs and 0
        keys = doubles.pack_keys(sc, pos)
        u = keys.view(np.uint64)
        assert (u[:, :-1] >= u[:, 1:]).all() and (u[:, :fill] != 0).all() and (u[:, fill:] == 0).all()
        ex = np.full((nq, e), -1, np.int64)
        for j in range(e):
            ex[:, j] = (pos[:, (5 * j) % kin], -7, 2 ** 32 + pos[:, j % kin] % 1000, pos[:, (5 * j) % kin])[j % 4]
        ex[1, 0], ex[2, 0] = 0xFFFFFFFF, 0
        got = filter_keys(torch.from_numpy(keys).cuda(), torch.from_numpy(ex).cuda(), k)
        torch.cuda.synchronize()
        want = doubles_filter.filter(torch.from_numpy(keys), torch.from_numpy(ex), k)
        np.testing.assert_array_equal(got.cpu().numpy(), want.numpy(), err_msg=str((kin, e, k)))
        if e >= 2:
            assert (want.numpy() != keys[:, :k]).any()           # the exclusions bite


# ---------------------------------------------------------------------------------------------------------------------
# 8. capture
def test_search_excluding_tensor_is_graph_capturable(oracle):
    """One warm call, then search_excluding_tensor captured on a side stream (as tests/test_index_rows_gpu.py captures its
    calls) and replayed with new exclusion contents copied into the same tensor."""
    import torch
    d, k, e = 768, 10, 3
    x, q, idx = _corpus(d)
    _, top = oracle.flat_ip_search(x, q, 2 * e)
    Es = [top[:, :e].copy(), top[:, 0:2 * e:2].copy()]
    Es[1][2, 1] = -1
    qt, Et = torch.from_numpy(q).cuda(), torch.from_numpy(Es[0]).cuda()
    side = torch.cuda.Stream()
    eager, replayed = [], []
    with torch.cuda.stream(side):
        for r in range(2):                                       # warm-up at the captured shape
            Et.copy_(torch.from_numpy(Es[r]))
            D0, I0 = idx.search_excluding_tensor(qt, k, Et)
            side.synchronize()
            eager.append((D0.cpu().numpy(), I0.cpu().numpy()))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            D1, I1 = idx.search_excluding_tensor(qt, k, Et)
        for r in range(2):
            Et.copy_(torch.from_numpy(Es[r]))
            D1.zero_()
            I1.zero_()
            g.replay()
            side.synchronize()
            replayed.append((D1.cpu().numpy(), I1.cpu().numpy()))
    torch.cuda.synchronize()
    for r in range(2):
        _same(replayed[r], eager[r], f"replay {r} vs eager")
        _same(replayed[r], excluding.filtered_topk(oracle, x, q, k, Es[r]), f"replay {r} vs the expectation")
    assert not np.array_equal(replayed[0][1], replayed[1][1])
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 9. ResidentCorpus: exclusions by external passage id
def test_resident_corpus_excludes_every_row_of_an_id(tmp_path, oracle):
    from haconvdr_amd.passages import write_embedding_block
    from haconvdr_amd.search import ResidentCorpus
    d, n0, n1, nq, topN = 768, 150, 101, 4, 10
    x = synth.embeddings(0xE8C0, n0 + n1, d)
    q = synth.embeddings(0xE8C1, nq, d)
    ext = np.arange(n0 + n1, dtype=np.int64) * 7 + 1000
    _, top = oracle.flat_ip_search(x, q, 40)
    r0 = int(top[0, 0])                                                  # query 0's best row ...
    r1 = int(next(r for r in top[0, 1:] if (r < n0) != (r0 < n0)))       # ... and the best one the other block holds
    ext[r1] = ext[r0]                                                    # one external id, a row of each block
    write_embedding_block(str(tmp_path), 0, x[:n0], ext[:n0])
    write_embedding_block(str(tmp_path), 1, x[n0:], ext[n0:])
    rc = ResidentCorpus(str(tmp_path), 2)
    D0, I0 = rc.search(q, topN)
    assert ext[r0] in I0[0]
    shared, absent = int(ext[r0]), 999                                   # 999: held by no block
    excl = np.array([[shared, -1], [absent, shared], [absent, -1], [-1, -1]], np.int64)
    D, I = rc.search(q, topN, exclude=excl)
    rc.index.check_status()
    assert D.dtype == D0.dtype and I.dtype == I0.dtype and D.shape == D0.shape and I.shape == I0.shape
    rows = np.array([[r0, r1], [r0, r1], [-1, -1], [-1, -1]], np.int64)
    wD, wI = excluding.filtered_topk(oracle, x, q, topN, rows)
    _same(excluding.deleted_topk(oracle, x, q, topN, rows), (wD, wI), "the two expectations")
    np.testing.assert_array_equal(I, ext[wI])
    np.testing.assert_array_equal(D, wD.astype(np.float64))
    assert shared not in I[0] and shared not in I[1]                     # both rows gone, the list still full
    np.testing.assert_array_equal(I[2:], I0[2:])                         # an id no block holds changes nothing
    np.testing.assert_array_equal(D[2:], D0[2:])
    D2, I2 = rc.search(q, topN, exclude=np.full((nq, 1), absent, np.int64))
    np.testing.assert_array_equal(I2, I0)
    np.testing.assert_array_equal(D2, D0)
