"""search_masked behind a cursor, the parts that need no GPU: the C-ABI surface of the three entry points, the resource lines of
scan16_masked_after_kernel, the identities of include/haconvdr.h ("search inside a bitmap, behind a cursor") proved over the
oracle (tests/masked_after_ref.py against after_ref, masked_ref and range_ref), the argument checks of the Python mirrors
(ValueError before the library is called, no handle needed), ResidentCorpus.search_deep(within=) / behind(within=) over a
stand-in index, ShardedSearcher.search_masked_after over two gloo ranks with a test double, and proofs that the inputs of
tests/test_index_masked_after_gpu.py show what they are for."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests import after_cases, after_ref, masked_after_cases, masked_after_ref, masked_cases, masked_ref, range_ref, rank_ref
from tests.test_index_masked import _tie_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("hac_index_search_masked_after", "hac_index_search_masked_after_device", "hac_index_search_masked_after_keys_device")
FMAX = after_ref.FMAX
_CASES = {}


@pytest.fixture(autouse=True)
def _the_calls_exist():
    """the identities and the inputs proved here belong to calls that must exist: on a tree without them nothing in this file passes"""
    from haconvdr_amd import _lib
    assert set(NEW_SYMBOLS) <= set(_lib.EXPORTED_SYMBOLS)


def scores(name, oracle):
    """(x, q, S) of a shared input, computed once and never changed"""
    if name not in _CASES:
        if name == "small tie":
            x, q, S = _tie_case(oracle)
        else:
            x, q = {"base": after_cases.base_case, "tie": after_cases.tie_case, "hostile": after_cases.hostile_case,
                    "descending": lambda: masked_cases.monotone_case(False), "ascending": lambda: masked_cases.monotone_case(True)}[name]()
            with np.errstate(all="ignore"):
                S = rank_ref.canon_scores(oracle, x, q)
        S.setflags(write=False)
        _CASES[name] = (x, q, S)
    return _CASES[name]


def some_masks(name, S):
    """(masks bool [5, n], mask_of int64 [nq]) for the identity tests: densities 1/2 .. 1/64, with the rows the case is about
    (NaN-, +-Inf-, FLT_MAX-scoring) selected by some masks and deselected by others"""
    nq, n = S.shape
    masks = np.stack([masked_cases.random_masks(0xE00 + m, 1, n, (2, 3, 5, 64, 2)[m])[0] for m in range(5)])
    special = {"small tie": [37, 200], "hostile": [20, 21, 40, 4001, 3, 13, 23]}.get(name, [])
    for r in special:
        masks[:, r] = np.arange(5) % 2 == r % 2
    return masks, ((np.arange(nq) * 3) % 5).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# symbols, registers
def test_new_entry_points_are_declared_listed_and_exported():
    from haconvdr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "haconvdr.h")).read()
    assert "search inside a bitmap, behind a cursor" in hdr
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
    # (search_masked's three forms with the cursor's arguments: 10 + 2, 12 + 2, 11 + 1)
    assert [len(getattr(L, sym).argtypes) for sym in NEW_SYMBOLS] == [12, 14, 12]


def test_masked_after_kernel_uses_no_scratch_and_spills_nothing():
    path = os.path.join(ROOT, "haconvdr_amd", "csrc", "flat_ip.resources.txt")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(path)])
    blocks = re.split(r"remark: Function Name: ", open(path).read())
    kernel = "scan16_masked_after_kernel"
    mine = [b for b in blocks if re.search(r"\d+%s[A-Z]" % kernel, b.split("\n", 1)[0])]
    assert len(mine) == 1, [b.split("\n", 1)[0] for b in mine]
    assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", mine[0]).group(1)) == 0
    assert int(re.search(r"VGPRs Spill: (\d+)", mine[0]).group(1)) == 0
    assert int(re.search(r"SGPRs Spill: (\d+)", mine[0]).group(1)) == 0
    assert int(re.search(r"VGPRs: (\d+)", mine[0]).group(1)) <= 256
    # the parents keep their one block each: every kernel is a `__global__` function of its own (they call one shared body)
    for parent in ("scan16_masked_kernel", "scan16_after_kernel", "mask_groups_kernel", "after_bounds_kernel"):
        assert len([b for b in blocks if re.search(r"\d+%s[A-Z]" % parent, b.split("\n", 1)[0])]) == 1, parent


# ---------------------------------------------------------------------------------------------------------------------
# the identities of the header, over the oracle
@pytest.mark.parametrize("name", ["small tie", "hostile"])
def test_all_ones_mask_is_search_after(name, oracle):
    x, q, S = scores(name, oracle)
    nq, n = S.shape
    ones = np.ones(n, np.bool_)
    sc, rw = masked_after_cases.cursors_at(S, (np.arange(nq) * 41 + 3) % 300)
    for k in (1, 40, n):
        want = after_ref.after_from_scores(S, sc, rw, k)
        masked_after_ref.assert_same(masked_after_ref.from_scores(S, ones, None, sc, rw, k), want, f"one mask k={k}")
        masked_after_ref.assert_same(masked_after_ref.from_scores(S, np.tile(ones, (nq, 1)), None, sc, rw, k), want, f"a mask per query k={k}")
        keys = masked_after_ref.from_keys(S, ones, None, after_ref.cursor_keys(sc, rw, 1000), 1000, k)
        masked_after_ref.assert_same(after_ref.unpack(keys, 1000), want, f"keys form k={k}")


@pytest.mark.parametrize("name", ["small tie", "hostile"])
def test_start_cursor_is_search_masked(name, oracle):
    x, q, S = scores(name, oracle)
    nq, n = S.shape
    masks, mask_of = some_masks(name, S)
    for k in (1, 40, n):
        want = masked_ref.masked_from_scores(S, masks, mask_of, k)
        masked_after_ref.assert_same(masked_after_ref.from_scores(S, masks, mask_of, None, None, k), want, f"null cursors k={k}")
        masked_after_ref.assert_same(masked_after_ref.from_scores(S, masks, mask_of, np.full(nq, np.nan, np.float32), np.full(nq, -2, np.int64), k), want,
                                     f"row -2 k={k}: the score is not read")
        for after_keys in (None, np.full(nq, -1, np.int64)):
            masked_after_ref.assert_same(after_ref.unpack(masked_after_ref.from_keys(S, masks, mask_of, after_keys, 0, k)), want, f"keys form k={k}")
    # a mask_of entry outside [0, n_masks): nothing selected, whatever the cursor (the device forms' rule)
    wild = mask_of.copy()
    wild[1], wild[2] = -1, 5
    I = masked_after_ref.from_scores(S, masks, wild, None, None, 4)[1]
    assert (I[1:3] == -1).all() and (I[0] >= 0).all()


@pytest.mark.parametrize("name, k", [("small tie", 7), ("small tie", 64), ("hostile", 100), ("hostile", 1000)])
def test_chained_pages_are_the_unbounded_masked_list(name, k, oracle):
    x, q, S = scores(name, oracle)
    nq, n = S.shape
    masks, mask_of = some_masks(name, S)
    lims, rD, rI = range_ref.range_from_scores(S, np.float32(-np.inf))
    cursor, pages = (None, None), []
    for _ in range(int(masks.sum(axis=1).max()) // k + 2):
        D, I = masked_after_ref.from_scores(S, masks, mask_of, cursor[0], cursor[1], k)
        pages.append((D, I))
        cursor = (D[:, -1].copy(), I[:, -1].copy())
    assert (pages[-1][1] == -1).all() and (pages[-1][0] == -FMAX).all()   # the page after the end, behind a padding cursor: padding only
    D, I = np.concatenate([p[0] for p in pages], 1), np.concatenate([p[1] for p in pages], 1)
    saw_low = saw_tie_across_pages = False
    for i in range(nq):
        sel = masks[mask_of[i]]
        m = int((sel & ~np.isnan(S[i])).sum())
        assert (I[i, :m] >= 0).all() and (I[i, m:] == -1).all() and len(set(I[i, :m].tolist())) == m      # every selected scored row once, then padding
        assert sel[I[i, :m]].all()
        # range_search(q, -inf) filtered by the mask, then the selected rows scoring -Inf (which no radius admits)
        rows, sc = rI[lims[i]:lims[i + 1]], rD[lims[i]:lims[i + 1]]
        low = np.flatnonzero(sel & (S[i] == -np.inf))
        np.testing.assert_array_equal(I[i, :m], np.concatenate([rows[sel[rows]], low]))
        np.testing.assert_array_equal(after_ref.bits(D[i, :m - len(low)]), after_ref.bits(sc[sel[rows]]))
        saw_low |= len(low) > 0
        # ties are continued by row across page boundaries
        for p in range(k, m, k):
            if D[i, p - 1] == D[i, p]:
                saw_tie_across_pages = True
                assert I[i, p - 1] < I[i, p]
    assert saw_tie_across_pages and (saw_low or name != "hostile")


@pytest.mark.parametrize("name", ["small tie", "hostile"])
def test_the_cursor_row_need_not_be_selected_and_need_not_exist(name, oracle):
    x, q, S = scores(name, oracle)
    nq, n = S.shape
    masks, mask_of = some_masks(name, S)
    k = 25
    for depth in (0, 17, 150):
        whole = after_ref.unbounded(S)
        # the first row at or behind `depth` of the unmasked list that the query's mask leaves out
        rw = np.array([next(int(r) for r in whole[i][1][depth:] if not masks[mask_of[i], r]) for i in range(nq)], np.int64)
        sc = S[np.arange(nq), rw].astype(np.float32)
        D, I = masked_after_ref.from_scores(S, masks, mask_of, sc, rw, k)
        full = masked_after_ref.unbounded(S, masks, mask_of)
        for i in range(nq):
            # ... the list goes on with the selected rows behind it, exactly where the masked list passes that key
            at = int((after_ref.pack(full[i][0], full[i][1]) > after_ref.pack(sc[i], rw[i])).sum())
            m = min(k, len(full[i][1]) - at)
            np.testing.assert_array_equal(I[i, :m], full[i][1][at:at + m])
            assert (I[i, m:] == -1).all() and rw[i] not in I[i]
        # a row the index does not hold: n + 5 ties nothing from behind; with a score no row has, the same list as any row gives
        absent = masked_after_ref.from_scores(S, masks, mask_of, sc, np.full(nq, n + 5), k)
        for i in range(nq):
            at = int((full[i][0].astype(np.float64) >= np.float64(sc[i])).sum())
            np.testing.assert_array_equal(absent[1][i, :min(k, len(full[i][1]) - at)], full[i][1][at:at + k])
        between = np.nextafter(sc, np.float32(np.inf))
        ok = np.isfinite(between) & ~(S == between[:, None]).any(axis=1)
        assert ok.any()
        a = masked_after_ref.from_scores(S[ok], masks, mask_of[ok], between[ok], np.zeros(int(ok.sum()), np.int64), k)
        b = masked_after_ref.from_scores(S[ok], masks, mask_of[ok], between[ok], np.full(int(ok.sum()), 2 ** 40), k)
        masked_after_ref.assert_same(a, b, "a score no row has: the row does not matter")


# ---------------------------------------------------------------------------------------------------------------------
# argument checks (no handle, no library call)
def test_python_mirrors_raise_before_the_library_is_called(monkeypatch):
    import torch
    from haconvdr_amd import _lib, index

    def never():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", never)
    idx = index.FlatIPIndex.__new__(index.FlatIPIndex)
    idx.d, idx.devices = 96, (0,)
    monkeypatch.setattr(index.FlatIPIndex, "ntotal", property(lambda self: 130))
    q = np.zeros((3, 96), np.float32)
    mask = np.ones(130, np.bool_)
    good = (np.zeros(3, np.float32), np.array([0, -1, -2]))
    with pytest.raises(ValueError) as err:
        idx.search_masked(q, 10, mask, None, after=(np.zeros(3, np.float32), np.array([0, -3, 0])))
    assert "query 1" in str(err.value) and "-3" in str(err.value) and "search_masked" in str(err.value)
    for bad in (dict(masks=mask[:-1], after=good), dict(masks=np.ones((2, 130), np.bool_), after=good), dict(masks=mask, mask_of=np.zeros(2, np.int64), after=good),
                dict(masks=mask, after=(np.zeros(3, np.float64), np.zeros(3, np.int64))), dict(masks=mask, after=(np.zeros(2, np.float32), np.zeros(3, np.int64))),
                dict(masks=mask, after=(np.zeros(3, np.float32), np.zeros(3, np.float32))), dict(masks=mask, after=(np.zeros(3, np.float32),)),
                dict(masks=mask, after=np.zeros(3, np.float32)), dict(masks=mask, after=good, k=0), dict(masks=mask, after=good, k=2049)):
        kw = dict(k=10, mask_of=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            idx.search_masked(q, kw["k"], kw["masks"], kw["mask_of"], after=kw["after"])
    # the tensor forms hand raw device pointers to kernels: a CPU tensor or an ndarray never gets there
    qt, wt = torch.zeros(3, 96), torch.zeros((1, 3), dtype=torch.int64)
    cur = (torch.zeros(3), torch.zeros(3, dtype=torch.int64))
    for call in (lambda: idx.search_masked_tensor(qt, 10, wt, after=cur), lambda: idx.search_masked_keys_tensor(qt, 10, wt, after_keys=torch.zeros(3, dtype=torch.int64)),
                 lambda: idx.search_masked_tensor(q, 10, wt, after=good)):
        with pytest.raises(ValueError):
            call()
    idx._h = None                                                          # (__del__ finds nothing to destroy)
    # (shape, dtype, device and k mistakes on real CUDA tensors: tests/test_index_masked_after_gpu.py)


def test_sharded_searcher_checks_masks_and_cursors_before_any_hook_runs():
    import torch
    from haconvdr_amd.sharded import ShardedSearcher

    def never(*a):
        raise AssertionError("a hook ran")
    s = ShardedSearcher(None, 0, local_keys=never, merge=never, to_results=never, filter=never, n_local=10, local_masked_keys=never, local_after_keys=never,
                        local_masked_after_keys=never)
    q, w = torch.zeros(3, 96), torch.zeros((1, 1), dtype=torch.int64)
    for masks, mask_of, cursor in ((w[0], None, None), (w.to(torch.int32), None, None), (torch.zeros((2, 1), dtype=torch.int64), None, None),
                                   (w, torch.zeros(2, dtype=torch.int64), None), (w, None, torch.zeros((3, 1), dtype=torch.int64)),
                                   (w, None, torch.zeros(2, dtype=torch.int64)), (w, None, torch.zeros(3, dtype=torch.int32)), (w, None, torch.zeros(3))):
        with pytest.raises(ValueError):
            s.search_masked_after(q, 10, masks, mask_of, cursor)


# ---------------------------------------------------------------------------------------------------------------------
# ResidentCorpus over a stand-in index
class _StandInIndex:
    """the calls of FlatIPIndex that search_deep(within=) and behind(within=) make, over the oracle's canonical scores, on CPU
    tensors"""

    def __init__(self, oracle, x):
        self.oracle, self.x, self.calls = oracle, x, []

    @property
    def ntotal(self):
        return len(self.x)

    def _S(self, q):
        with np.errstate(all="ignore"):
            return rank_ref.canon_scores(self.oracle, self.x, np.asarray(q, np.float32))

    def search_masked_keys_tensor(self, q, k, masks, mask_of=None, pos_base=0, stream=None, after_keys=None):
        import torch
        from haconvdr_amd.index import unpack_mask
        self.calls.append(("search_masked_keys", int(k), tuple(masks.shape), after_keys is not None))
        keys = masked_after_ref.from_keys(self._S(q.numpy()), unpack_mask(masks.numpy(), len(self.x)), None if mask_of is None else mask_of.numpy(),
                                          None if after_keys is None else after_keys.numpy(), pos_base, k)
        return torch.from_numpy(keys.view(np.int64))

    def score_ids(self, q, ids):
        S = self._S(q)
        return np.where(ids >= 0, np.take_along_axis(S, np.maximum(ids, 0), 1), np.float32(-FMAX)).astype(np.float32)

    def search_masked(self, q, k, masks, mask_of=None, after=None):
        from haconvdr_amd.index import unpack_mask
        self.calls.append(("search_masked", int(k), tuple(np.asarray(masks).shape), after is not None))
        return masked_after_ref.from_scores(self._S(q), unpack_mask(masks, len(self.x)), mask_of, after[0], after[1], k)


def test_resident_corpus_search_deep_and_behind_within(oracle, monkeypatch):
    import torch
    from haconvdr_amd import index as index_mod
    from haconvdr_amd.search import ResidentCorpus
    from tests import doubles
    x, q = after_cases.hostile_case()
    x, q = x[:700].copy(), q[:4]
    x[40] = x[21]
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
    r = np.arange(n)
    two = np.stack([r % 3 != 1, r % 5 == 2])
    of = np.array([0, 1, 1, 0])
    whole = masked_after_ref.unbounded(S, two, of)
    assert len(whole[0][1]) > 400 > 140 >= len(whole[1][1]) > 100
    for depth, page, calls in ((420, 128, [(128, False), (128, True), (128, True), (36, True)]), (5, 1024, [(5, False)])):
        rc.index.calls.clear()
        D, I = rc.search_deep(torch.from_numpy(q) if depth == 5 else q, depth, page=page, within=two, within_of=of)
        assert rc.index.calls == [("search_masked_keys", k, (2, 11), cur) for k, cur in calls]
        assert D.dtype == np.float64 and I.dtype == np.int64 and D.shape == I.shape == (len(q), depth)
        for i in range(len(q)):
            m = min(depth, len(whole[i][1]))
            np.testing.assert_array_equal(I[i, :m], pids[whole[i][1][:m]])
            np.testing.assert_array_equal(D[i, :m], whole[i][0][:m].astype(np.float64))
            assert (I[i, m:] == -1).all() and (D[i, m:] == np.float64(-FMAX)).all()
    # one mask for all, no within_of; packed words pass through
    from haconvdr_amd.index import pack_mask
    D1, I1 = rc.search_deep(q, 300, page=256, within=pack_mask(two[1]))
    one = masked_after_ref.unbounded(S, two[1], None)
    for i in range(len(q)):
        m = len(one[i][1])
        np.testing.assert_array_equal(I1[i, :m], pids[one[i][1]])
        assert (I1[i, m:] == -1).all()
    calls = len(rc.index.calls)
    for bad in (dict(within_of=of), dict(within=two), dict(within=two[:, :-1], within_of=of), dict(within=two, within_of=np.array([0, 1, 2, 0])),
                dict(within=two, within_of=of[:-1])):
        with pytest.raises(ValueError):
            rc.search_deep(q, 10, **bad)
        with pytest.raises(ValueError):
            rc.behind(q, pids[:4], 3, **bad)
    assert len(rc.index.calls) == calls
    # behind(within=): the selected rows right behind the named passage, which need not be selected itself
    unmasked = after_ref.unbounded(S)
    gold_row = np.array([100, -1, 3, int(unmasked[3][1][50])])            # query 0: row 100 is deselected (100 % 3 == 1); query 2: row 3 scores NaN
    assert not two[0, 100] and np.isnan(S[2, 3])
    gold = np.where(gold_row >= 0, pids[np.maximum(gold_row, 0)], 5)       # query 1: no block holds passage 5
    rc.index.calls.clear()
    D, I = rc.behind(q, gold, 12, within=two, within_of=of)
    assert rc.index.calls == [("search_masked", 12, (2, 11), True)]
    assert D.dtype == np.float64 and I.dtype == np.int64 and D.shape == I.shape == (4, 12)
    wD, wI = masked_after_ref.from_scores(S, two, of, S[np.arange(4), np.maximum(gold_row, 0)], gold_row, 12)
    np.testing.assert_array_equal(I, np.where(wI >= 0, pids[np.maximum(wI, 0)], -1))
    np.testing.assert_array_equal(D, wD.astype(np.float64))
    assert (I[0] >= 0).all() and (I[1:3] == -1).all() and (I[3] >= 0).all() and pids[100] not in I[0]
    # search(exclude=, within=) keeps raising
    with pytest.raises(ValueError):
        rc.search(q, 9, within=two[0], exclude=np.zeros((4, 1), np.int64))


# ---------------------------------------------------------------------------------------------------------------------
# ShardedSearcher.search_masked_after over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_masked_after_double_restates_the_contract(oracle):
    import torch
    from haconvdr_amd.index import pack_mask
    from tests import doubles, doubles_masked_after
    x = np.array([[1.0] * 32, [2.0] * 32, [1.0] * 32, [np.nan] * 32, [3.0] * 32, [1.0] * 32], np.float32)
    q = torch.ones((1, 32))
    masks = torch.from_numpy(pack_mask(np.array([[True, True, True, True, False, True]])))
    hook = doubles_masked_after.make_local_masked_after_keys(oracle, x)
    D, pos = doubles.unpack_keys(hook(q, 4, masks, None, None, 100).numpy())
    assert pos.tolist() == [[101, 100, 102, 105]] and D[0].tolist() == [64.0, 32.0, 32.0, 32.0]
    cursor = torch.from_numpy(after_ref.cursor_keys(np.array([96.0], np.float32), np.array([104])))      # global position 104: the deselected row
    D, pos = doubles.unpack_keys(hook(q, 2, masks, None, cursor, 100).numpy())
    assert pos.tolist() == [[101, 100]]
    cursor = torch.from_numpy(after_ref.cursor_keys(np.array([32.0], np.float32), np.array([100])))
    D, pos = doubles.unpack_keys(hook(q, 4, masks, None, cursor, 100).numpy())
    assert pos.tolist() == [[102, 105, -1, -1]]
    assert doubles_masked_after.CALLS == [(4, 1, 1, False, 100), (2, 1, 1, True, 100), (4, 1, 1, True, 100)]
    doubles_masked_after.CALLS.clear()


def test_sharded_search_masked_after_gloo():
    world, port = 2, _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="2")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_gloo_worker_masked_after.py"), "double"], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
        assert "OK" in o


# ---------------------------------------------------------------------------------------------------------------------
# proofs about the inputs of tests/test_index_masked_after_gpu.py
@pytest.mark.parametrize("ascending", [False, True])
def test_threshold_cases_tell_select_then_filter_from_eligibility_before_append(ascending, oracle):
    """masked_p = 1 walks every group in row order.  A kernel that kept the best high_water(k) keys of ALL rows, or of the
    SELECTED rows whatever the cursor says, and applied the missing test afterwards would return a different list for every
    query: the cursor stands behind ~3000 rows, so the 256 best of either set lie ahead of it and nothing is left.  Keeping the
    best 256 of the rows BEHIND the cursor whatever the mask says and masking afterwards leaves two rows of three, more than k:
    at this density that variant returns the right list here, and the base case's one-in-six masks are what tell it apart."""
    x, q, S = scores("ascending" if ascending else "descending", oracle)
    _, _, mask = masked_after_cases.threshold_case(ascending)
    sc, rw = masked_after_cases.threshold_cursors(S)
    assert (~mask).sum() == -(-len(mask) // 3) and len(set(zip(sc.tolist(), rw.tolist()))) == len(q)
    assert not mask[rw].all() and mask[rw].any()                          # some cursor rows are deselected, some selected
    ahead = np.array([(~after_ref.eligible(S[i], sc[i], rw[i])).sum() for i in range(len(q))])
    assert (ahead > 2900).all() and (ahead < 3100).all()
    for k in masked_after_cases.THRESHOLD_KS:
        assert masked_after_cases.high_water(k) == 256
        own = masked_after_ref.from_scores(S, mask, None, sc, rw, k)[1]
        assert (own >= 0).all()
        for first in ("all", "selected"):
            wrong = masked_after_cases.select_then_filter(S, mask, sc, rw, k, first)
            assert (wrong != own).any(axis=1).all() and (wrong == -1).all(), (k, first)
        np.testing.assert_array_equal(masked_after_cases.select_then_filter(S, mask, sc, rw, k, "behind"), own)
    # the same list in ascending row order, or descending: what a compaction keeps is the newest rows, or the oldest
    steps = np.diff(own, axis=1)
    assert ((steps < 0) if ascending else (steps > 0)).all()


def test_base_case_tells_masking_after_the_cursor_cut_from_eligibility_before_append(oracle):
    x, q, S = scores("base", oracle)
    per_query = masked_cases.per_query_masks()
    sc, rw = masked_after_cases.own_depth_cursors(S)
    k = 100                     # (only: at k = 2048 the 3840 kept keys are more than the 5000-row case leaves behind most cursors)
    own = masked_after_ref.from_scores(S, per_query, None, sc, rw, k)[1]
    hw = masked_after_cases.high_water(k)
    differ = 0
    for i in range(len(q)):
        wrong = masked_after_cases.select_then_filter(S[i:i + 1], per_query[i], sc[i:i + 1], rw[i:i + 1], k, "behind")[0]
        differ += int((wrong != own[i]).any())
        if i % 5 == 4:                                                     # density 1/6: fewer than k of the hw kept rows are selected
            assert (wrong != own[i]).any() and hw / 6 < k, (k, i)
    assert differ >= len(q) // 5


def test_tile_cases_tell_the_lanes_own_mask_and_bound_from_its_neighbours(oracle):
    """per-query masks and per-query depths inside every tile: a kernel that tested the tile's OR of masks, or the bound of the
    query one lane (or one launch) away, answers differently"""
    x, q, S = scores("base", oracle)
    nq = len(q)
    sc, rw = masked_after_cases.own_depth_cursors(S)
    bounds = after_ref.cursor_keys(sc, rw)
    assert len(set(bounds.tolist())) == nq
    per_query = masked_cases.per_query_masks()
    grouped, mask_of = masked_cases.grouped_masks()
    for name, masks, mo in (("a mask per query", per_query, np.arange(nq)), ("five masks", grouped, mask_of)):
        for k, QT in ((10, 16), (2048, 4)):
            own = masked_after_ref.from_scores(S, masks, mo, sc, rw, k)[1]
            union = masked_after_ref.from_scores(S, masked_cases.union_of_tile(masks, mo, QT), None, sc, rw, k)[1]
            assert (own != union).any(axis=1).sum() >= (nq - 1 if name == "a mask per query" and QT == 16 else nq // 2), (name, k)
            for shift in (1, QT):                                          # the neighbour's bound; the bound a tile (a launch of one tile) before
                other = masked_after_ref.from_keys(S, masks, mo, np.roll(bounds, shift), 0, k)
                # (two cursors 48 entries apart in score can have no SELECTED row between them under a one-in-six mask: then, and
                # only then, the lists agree -- one query of the 37 at most)
                dense = np.ones(nq, np.bool_) if name == "a mask per query" else np.isin(mo, [0, 2, 4])      # (five masks: not the 1/64 and 1/1000 ones)
                assert (after_ref.unpack(other)[1] != own).any(axis=1)[dense].sum() >= dense.sum() - 1 and dense.sum() > nq // 2, (name, k, shift)
    # more than QUERY_CHUNK queries: the queries of the second launch stand elsewhere than those a launch before them
    cx, cq, cmasks, cmo, depths = masked_after_cases.chunk_case()
    C = masked_after_cases.QUERY_CHUNK
    assert len(cq) > C and (depths[C:] != depths[:len(cq) - C]).all() and (cmo[C:] != cmo[:len(cq) - C]).any()
    with np.errstate(all="ignore"):
        cS = rank_ref.canon_scores(oracle, cx, cq[C:])
    csc, crw = masked_after_cases.cursors_at(cS, depths[C:])
    own = masked_after_ref.from_scores(cS, cmasks, cmo[C:], csc, crw, masked_after_cases.CHUNK_K)[1]
    with np.errstate(all="ignore"):
        S0 = rank_ref.canon_scores(oracle, cx, cq[:len(cq) - C])
    s0, r0 = masked_after_cases.cursors_at(S0, depths[:len(cq) - C])
    first_launch = masked_after_ref.from_scores(cS, cmasks, cmo[C:], s0, r0, masked_after_cases.CHUNK_K)[1]
    assert (own != first_launch).any(axis=1).all() and (own[:, 0] >= 0).all()


def test_edge_and_empty_tile_cases_hold_what_they_name(oracle):
    x, q, S = scores("hostile", oracle)
    n = S.shape[1]
    pick, masks, sc, rw = masked_after_cases.edge_case(S)
    St = S[pick]
    D, I = masked_after_ref.from_scores(St, masks, None, sc, rw, 40)
    assert (I[[1, 4]] == -1).all()                                         # a NaN score, an exhausted list
    masked_after_ref.assert_same((D[0:1], I[0:1]), (D[6:7], I[6:7]), "-0.0 against +0.0")
    assert (I[0] > 7).all() and (D[0] == 0).all()
    assert St[2, 20] == np.inf and I[2, 0] == 21 and St[3, 20] == -np.inf
    low = np.flatnonzero(masks[3] & (St[3] == -np.inf))
    assert I[3, :len(low[low > 20])].tolist() == low[low > 20].tolist() and (I[3, len(low[low > 20]):] == -1).all() and len(low[low > 20]) >= 1
    assert (St[5, I[5][I[5] >= 0]] < sc[5]).all()                          # a row >= ntotal: no row tying the score
    assert not masks[:, 640:1280].any() and 640 <= rw[7] < 1280 and (I[7] >= 0).all()
    assert np.isfinite(D[8]).all() and (St[8] == np.inf).any()             # behind 2^32: no +Inf row
    masked_after_ref.assert_same((D[9:10], I[9:10]), masked_ref.masked_from_scores(St[9:10], masks[9], None, 40), "the start")
    assert not np.isnan(D).any() and len(set(rw[12:].tolist())) >= 2
    # empty tiles: the queries 16 .. 31 select nothing; their neighbours do
    bx, bq, bS = scores("base", oracle)
    emasks, emo = masked_after_cases.empty_tile_masks()
    assert not emasks[emo[16:32]].any() and emasks[emo[:16]].any(axis=1).all() and emasks[emo[32:]].any(axis=1).all()
    bsc, brw = masked_after_cases.own_depth_cursors(bS)
    I = masked_after_ref.from_scores(bS, emasks, emo, bsc, brw, 10)[1]
    assert (I[16:32] == -1).all() and (I[:16, 0] >= 0).all()
    # rows ahead of the cursor only: padding, although the mask selects 50 rows
    ahead = masked_after_cases.rows_ahead_masks(bS, 60, 50)
    c60 = masked_after_cases.cursors_at(bS, np.full(len(bq), 60))
    assert (ahead.sum(axis=1) == 50).all() and (masked_after_ref.from_scores(bS, ahead, None, c60[0], c60[1], 10)[1] == -1).all()
    assert (masked_after_ref.from_scores(bS, ahead, None, None, None, 10)[1] >= 0).all()
