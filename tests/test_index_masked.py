"""search_masked, the parts that need no GPU: the C-ABI surface of the three entry points, the resource lines of the two kernels
of csrc/masked.inc, the reference of tests/masked_ref.py against the oracle's search, among_ref, tests/excluding.py and
range_ref (the four identities of include/haconvdr.h), pack_mask / unpack_mask / range_mask, the argument checks of the Python
mirrors (ValueError before the library is called, no handle needed), ResidentCorpus.rows_mask / first_rows_mask /
search(within=) over a stand-in index, ShardedSearcher.search_masked over two gloo ranks, and proofs that the inputs of
tests/test_index_masked_gpu.py show what they are for."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests import among_ref, excluding, masked_cases, masked_ref, range_ref, rank_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("hac_index_search_masked", "hac_index_search_masked_device", "hac_index_search_masked_keys_device")
MASKED_KERNELS = ("mask_groups_kernel", "scan16_masked_kernel")


def test_new_entry_points_are_declared_listed_and_exported():
    from haconvdr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "haconvdr.h")).read()
    assert "search inside a bitmap" in hdr
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
    # (the keys form has the device form's arguments with keys_dev, pos_base in place of D_dev, I_dev, id_map_dev: 12 - 1)
    assert [len(getattr(L, sym).argtypes) for sym in NEW_SYMBOLS] == [10, 12, 11]


def test_masked_kernels_use_no_scratch_and_spill_nothing():
    path = os.path.join(ROOT, "haconvdr_amd", "csrc", "flat_ip.resources.txt")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(path)])
    blocks = re.split(r"remark: Function Name: ", open(path).read())
    for kernel in MASKED_KERNELS:
        mine = [b for b in blocks if re.search(r"\d+%s[A-Z]" % kernel, b.split("\n", 1)[0])]
        assert len(mine) == 1, (kernel, [b.split("\n", 1)[0] for b in mine])
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", mine[0]).group(1)) == 0, kernel
        assert int(re.search(r"VGPRs Spill: (\d+)", mine[0]).group(1)) == 0, kernel
        assert int(re.search(r"SGPRs Spill: (\d+)", mine[0]).group(1)) == 0, kernel


# ---------------------------------------------------------------------------------------------------------------------
# the reference itself
def _tie_case(oracle):
    """tests/test_index_among.py::_tie_case: 400 x 32, grid-valued rows of which many repeat, integer queries (exact scores, long
    ties), one NaN row, one FLT_MAX row, a zero query"""
    from haconvdr_amd import synth
    n, d, nq = 400, 32, 7
    base = ((synth.uniform_u32(0x7A0, 24 * d) % np.uint32(17)).astype(np.float32).reshape(24, d) - 8.0) / 8.0
    x = base[(synth.uniform_u32(0x7A1, n) % np.uint32(24)).astype(np.int64)]
    x[37, 3] = np.nan
    x[200] = np.finfo(np.float32).max
    q = (synth.uniform_u32(0x7A2, nq * d) % np.uint32(9)).astype(np.float32).reshape(nq, d) - 4.0
    q[0] = 0.0
    return x, q, rank_ref.canon_scores(oracle, x, q)


def test_reference_holds_the_four_identities(oracle):
    x, q, S = _tie_case(oracle)
    nq, n = S.shape
    assert np.isnan(S[1:, 37]).all() and any(len(np.unique(S[i][~np.isnan(S[i])])) < 60 for i in range(nq))
    ones = np.ones(n, np.bool_)
    # 1. an all-ones mask gives search(q, k); k beyond the rows that have a score: padding
    for k in (1, 40, 399, 400):
        want = oracle.flat_ip_search(x, q, k)
        masked_ref.assert_same(masked_ref.masked_from_scores(S, ones, None, k), want, f"all ones k={k}")
        masked_ref.assert_same(masked_ref.masked_from_scores(S, np.tile(ones, (nq, 1)), None, k), want, f"a mask per query k={k}")
    # 2. the mask of a set S gives search_among(q, k, S), per query
    rng = np.random.default_rng(0xB00)
    for m, k in ((1, 3), (50, 20), (50, 50), (300, 51)):
        cand = np.stack([rng.choice(n, m, replace=False) for _ in range(nq)]).astype(np.int64)
        cand[0, 0], cand[1, 0] = 37, 200                                  # the NaN row and the FLT_MAX row named once each
        masks = np.zeros((nq, n), np.bool_)
        np.put_along_axis(masks, cand, True, 1)
        masked_ref.assert_same(masked_ref.masked_from_scores(S, masks, None, k), among_ref.among_from_scores(S, cand, k), f"among m={m} k={k}")
    # 3. the complement of E gives search_excluding(q, k, E), both of its references
    for e, k in ((9, 30), (60, 388)):
        E = np.stack([rng.choice(n, e, replace=False) for _ in range(nq)]).astype(np.int64)
        E[0, 0], E[1, 1] = 37, 200
        masks = np.ones((nq, n), np.bool_)
        np.put_along_axis(masks, E, False, 1)
        got = masked_ref.masked_from_scores(S, masks, None, k)
        masked_ref.assert_same(got, excluding.filtered_topk(oracle, x, q, k, E), f"e={e}")
        masked_ref.assert_same(got, excluding.deleted_topk(oracle, x, q, k, E), f"e={e}, rows deleted")
    # 4. masked(q, M, k) is range_search(q, -inf) filtered by M, cut at k -- then, if there is room, the selected rows that score
    # -Inf, which no radius admits (the comparison is strict) and every search lists last
    lims, rD, rI = range_ref.range_from_scores(S, np.float32(-np.inf))
    five = masked_cases.random_masks(0xB01, 5, n, 3)
    mask_of = (np.arange(nq) % 5).astype(np.int64)
    for k in (1, 17, 200):
        D, I = masked_ref.masked_from_scores(S, five, mask_of, k)
        for i in range(nq):
            rows, sc = rI[lims[i]:lims[i + 1]], rD[lims[i]:lims[i + 1]]
            keep = five[mask_of[i]][rows]
            m = min(k, int(keep.sum()))
            np.testing.assert_array_equal(I[i, :m], rows[keep][:m])
            np.testing.assert_array_equal(masked_ref.bits(D[i, :m]), masked_ref.bits(sc[keep][:m]))
            low = np.flatnonzero(five[mask_of[i]] & (S[i] == -np.inf))[:k - m]
            np.testing.assert_array_equal(I[i, m:m + len(low)], low)
            assert (I[i, m + len(low):] == -1).all() and (D[i, m + len(low):] == -masked_ref.FMAX).all()
    assert (S[:, 200] == -np.inf).any() and five[:, 200].any()
    # the tie rule and the padding rules on their own
    D, I = masked_ref.masked_from_scores(S[:1], np.isin(np.arange(n), [300, 7, 150, 399, 37]), None, 6)
    assert I.tolist() == [[7, 150, 300, 399, -1, -1]]                     # the zero query: every score +0.0, row 37 NaN
    D, I = masked_ref.masked_from_scores(S, np.zeros(n, np.bool_), None, 4)
    assert (I == -1).all() and (D == -masked_ref.FMAX).all()
    D, I = masked_ref.masked_from_scores(S, five, np.array([0, -1, 5, 1, 2, 3, 4]), 4)       # outside [0, n_masks): nothing selected
    assert (I[1:3] == -1).all() and (I[[0, 3, 4, 5, 6]] >= 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# pack_mask / unpack_mask / range_mask
@pytest.mark.parametrize("ntotal", [1, 63, 64, 65, 4097])
def test_pack_mask_round_trip(ntotal):
    import torch
    from haconvdr_amd.index import mask_words, pack_mask, unpack_mask
    m = masked_cases.random_masks(0xB10 + ntotal, 3, ntotal, 2)
    m[0, :] = True                                                        # every bit, bit 63 of every whole word included
    m[1, :] = False
    m[1, min(63, ntotal - 1)] = True                                      # bit 63 alone (or the last row)
    w = pack_mask(m)
    W = mask_words(ntotal)
    assert W == -(-ntotal // 64) and w.dtype == np.int64 and w.shape == (3, W) and w.flags.c_contiguous
    want = np.zeros((3, W * 8), np.uint8)
    pb = np.packbits(m, axis=1, bitorder="little")
    want[:, :pb.shape[1]] = pb
    assert w.view(np.uint8).reshape(3, -1).tobytes() == want.tobytes()    # faiss's bitmap bytes, zero padded to whole words
    if ntotal >= 64:
        assert w[0, 0] == -1 and w[1, 0] == np.iinfo(np.int64).min        # bit 63 makes a negative word
    np.testing.assert_array_equal(unpack_mask(w, ntotal), m)
    np.testing.assert_array_equal(unpack_mask(w.view(np.uint64), ntotal), m)
    np.testing.assert_array_equal(pack_mask(m[2]), w[2])                  # one mask: [W]
    np.testing.assert_array_equal(unpack_mask(w[2], ntotal), m[2])
    # a CPU tensor goes through torch's own arithmetic (the path CUDA tensors take) and gives the same words
    tw = pack_mask(torch.from_numpy(m))
    assert tw.dtype == torch.int64 and tuple(tw.shape) == (3, W)
    np.testing.assert_array_equal(tw.numpy(), w)
    np.testing.assert_array_equal(unpack_mask(tw, ntotal), m)
    # bits past ntotal are dropped by unpack_mask
    dirty = w.copy()
    if ntotal % 64:
        dirty[:, -1] |= np.int64(-1) << np.int64(ntotal % 64)
        assert not np.array_equal(dirty, w)
    np.testing.assert_array_equal(unpack_mask(dirty, ntotal), m)


def test_pack_mask_refuses_what_is_not_a_bool_mask():
    from haconvdr_amd.index import pack_mask, unpack_mask
    for bad in (np.zeros(5, np.uint8), np.zeros((2, 2, 2), np.bool_), np.zeros((), np.bool_)):
        with pytest.raises(ValueError):
            pack_mask(bad)
    for bad, n in ((np.zeros(2, np.int64), 64), (np.zeros(1, np.int32), 64), (np.zeros((1, 1, 1), np.int64), 64)):
        with pytest.raises(ValueError):
            unpack_mask(bad, n)


def test_range_mask():
    from haconvdr_amd.index import range_mask, unpack_mask
    for n, lo, hi in ((200, 0, 200), (200, 63, 65), (200, 64, 128), (200, 199, 200), (200, 50, 50), (200, 70, 60), (200, -5, 10), (200, 190, 500),
                      (64, 0, 64), (1, 0, 1), (0, 0, 0)):
        w = range_mask(n, lo, hi)
        want = np.zeros(n, np.bool_)
        want[max(lo, 0):max(hi, 0)] = True
        assert w.dtype == np.int64 and w.shape == ((n + 63) // 64,)
        np.testing.assert_array_equal(unpack_mask(w, n), want)
    for bad in ((200.0, 0, 1), (200, 0.5, 1), (200, 0, True), (-1, 0, 0)):
        with pytest.raises(ValueError):
            range_mask(*bad)


# ---------------------------------------------------------------------------------------------------------------------
# argument checks (no handle)
def test_masked_args_pass_good_arguments_through():
    from haconvdr_amd import index
    n = 130
    q, k, w, mo = index._masked_args(np.zeros((3, 96), np.float64), np.int64(10), np.ones(n, np.bool_), None, 96, n)
    assert q.dtype == np.float32 and k == 10 and w.dtype == np.int64 and w.shape == (1, 3) and w.flags.c_contiguous and mo is None
    assert w.tolist() == [[-1, -1, 3]]
    assert index._masked_args(np.zeros((3, 96)), 2048, np.ones((3, n), np.bool_), None, 96, n)[2].shape == (3, 3)       # a mask per query
    q, k, w, mo = index._masked_args(np.zeros((3, 96)), 7, np.zeros((2, 3), np.uint64), np.array([1, 0, 1], np.int32), 96, n)
    assert w.dtype == np.int64 and w.shape == (2, 3) and mo.dtype == np.int64 and mo.tolist() == [1, 0, 1]
    assert index._masked_args(np.zeros((3, 96)), 7, np.zeros(3, np.int64), None, 96, n)[2].shape == (1, 3)              # packed, one mask
    assert index._masked_args(np.zeros((0, 96)), 7, np.ones(n, np.bool_), None, 96, n)[0].shape == (0, 96)
    assert index._masked_args(np.zeros((2, 96)), 7, np.ones((1, 0), np.bool_), None, 96, 0)[2].shape == (1, 0)          # an empty index


@pytest.mark.parametrize("q, k, masks, mask_of", [
    (np.zeros((3, 96)), 10, np.ones(129, np.bool_), None),                 # a bool mask of another length
    (np.zeros((3, 96)), 10, np.ones((3, 131), np.bool_), None),
    (np.zeros((3, 96)), 10, np.zeros(2, np.int64), None),                  # packed with too few words (a stale mask)
    (np.zeros((3, 96)), 10, np.zeros((3, 4), np.uint64), None),
    (np.zeros((3, 96)), 10, np.zeros((3, 3), np.int32), None),             # words of another width
    (np.zeros((3, 96)), 10, np.zeros((3, 3), np.float32), None),
    (np.zeros((3, 96)), 10, np.ones((1, 1, 130), np.bool_), None),         # three dimensions
    (np.zeros((3, 96)), 10, np.ones((), np.bool_), None),
    (np.zeros((3, 96)), 10, np.ones((0, 130), np.bool_), None),            # no mask
    (np.zeros((3, 96)), 10, np.ones((2, 130), np.bool_), None),            # two masks, three queries, no mask_of
    (np.zeros((3, 96)), 10, np.ones((2, 130), np.bool_), np.zeros(2, np.int64)),       # mask_of of another length
    (np.zeros((3, 96)), 10, np.ones((2, 130), np.bool_), np.zeros((3, 1), np.int64)),
    (np.zeros((3, 96)), 10, np.ones((2, 130), np.bool_), np.zeros(3, np.float32)),     # float mask_of
    (np.zeros((3, 96)), 0, np.ones(130, np.bool_), None),                  # k = 0
    (np.zeros((3, 96)), 2049, np.ones(130, np.bool_), None),               # k = 2049
    (np.zeros((3, 96)), 2.0, np.ones(130, np.bool_), None),
    (np.zeros((3, 95)), 10, np.ones(130, np.bool_), None),                 # wrong dimension
])
def test_masked_args_raise_value_error(q, k, masks, mask_of):
    from haconvdr_amd import index
    with pytest.raises(ValueError):
        index._masked_args(q, k, masks, mask_of, 96, 130)


def test_tensor_checks_refuse_host_tensors():
    """The tensor forms hand raw device pointers to kernels: a CPU tensor or an ndarray must never get there."""
    import torch
    from haconvdr_amd import index
    with pytest.raises(ValueError):
        index._masked_args_tensor(torch.zeros(3, 96), 10, torch.zeros(1, 3, dtype=torch.int64), None, None, 96, 130)
    with pytest.raises(ValueError):
        index._masked_args_tensor(np.zeros((3, 96), np.float32), 10, np.zeros((1, 3), np.int64), None, None, 96, 130)
    # (shape, dtype, k and mask_of mistakes on real CUDA tensors: tests/test_index_masked_gpu.py)


def test_sharded_searcher_checks_masks_before_any_hook_runs():
    import torch
    from haconvdr_amd.sharded import ShardedSearcher

    def never(*a):
        raise AssertionError("a hook ran")
    s = ShardedSearcher(None, 0, local_keys=never, merge=never, to_results=never, filter=never, n_local=10, local_masked_keys=never)
    good = torch.zeros((3, 1), dtype=torch.int64)
    for masks, mask_of in ((good[0], None), (good.to(torch.int32), None), (good[:2], None), (good, torch.zeros(2, dtype=torch.int64)),
                           (good, torch.zeros(3, dtype=torch.int32)), (good, torch.zeros((3, 1), dtype=torch.int64))):
        with pytest.raises(ValueError):
            s.search_masked(torch.zeros(3, 96), 10, masks, mask_of)


# ---------------------------------------------------------------------------------------------------------------------
# ResidentCorpus over a stand-in index
class _StandInIndex:
    """search_masked_tensor of FlatIPIndex over the oracle's canonical scores, on CPU tensors"""

    def __init__(self, oracle, x):
        self.oracle, self.x, self.calls = oracle, x, []

    @property
    def ntotal(self):
        return len(self.x)

    def search_masked_tensor(self, q, k, masks, mask_of=None, id_map=None, stream=None):
        import torch
        from haconvdr_amd.index import unpack_mask
        self.calls.append((int(k), tuple(masks.shape), None if mask_of is None else tuple(mask_of.shape)))
        D, I = masked_ref.masked(self.oracle, self.x, q.numpy(), unpack_mask(masks, len(self.x)), None if mask_of is None else mask_of.numpy(), k)
        if id_map is not None:
            I = np.where(I >= 0, id_map.numpy()[np.clip(I, 0, None)], -1)
        return torch.from_numpy(D), torch.from_numpy(I)

    def remove_ids(self, rows):
        self.x = np.delete(self.x, rows, 0)
        return len(rows)


def test_resident_corpus_masks_and_search_within(oracle):
    import torch
    from haconvdr_amd import synth
    from haconvdr_amd.search import ResidentCorpus
    n, d, nq, k = 300, 32, 4, 60
    x = synth.embeddings(0xB20, n, d)
    x[250:] = x[:50]                                                      # the second block repeats fifty passages, bit for bit
    q = synth.embeddings(0xB21, nq, d)
    pids = np.arange(n, dtype=np.int64) * 7 + 11                          # row -> passage id ...
    pids[250:] = pids[:50]                                                # ... the first 50 ids carried by two rows each
    rc = ResidentCorpus.__new__(ResidentCorpus)
    rc.index, rc._ids, rc._lookup = _StandInIndex(oracle, x), pids, None
    rc.dev, rc.id_map = torch.device("cpu"), torch.from_numpy(pids)
    S = rank_ref.canon_scores(oracle, x, q)
    # rows_mask: every row that carries one of the ids, an absent id and -1 ignored, any shape
    m = rc.rows_mask(np.array([[pids[3], pids[100]], [5, -1]]))
    assert m.dtype == np.bool_ and m.shape == (n,) and np.flatnonzero(m).tolist() == [3, 100, 253]
    assert not rc.rows_mask(np.zeros(0, np.int64)).any()
    with pytest.raises(ValueError):
        rc.rows_mask(np.array([1.0]))
    # first_rows_mask: the first row of each id
    first = rc.first_rows_mask()
    assert first.dtype == np.bool_ and first[:250].all() and not first[250:].any()
    # searching within it: no passage id twice, lists full; the plain search repeats ids
    D, I = rc.search(q, k, within=first)
    assert D.dtype == np.float64 and I.dtype == np.int64 and D.shape == I.shape == (nq, k)
    wD, wI = masked_ref.masked_from_scores(S, first, None, k)
    np.testing.assert_array_equal(I, pids[wI])
    np.testing.assert_array_equal(D, wD.astype(np.float64))
    assert all(len(set(I[i].tolist())) == k for i in range(nq))
    plain = pids[oracle.flat_ip_search(x, q, k)[1]]
    assert any(len(set(plain[i].tolist())) < k for i in range(nq))
    # masks per query through within_of; packed words are taken as they are
    from haconvdr_amd.index import pack_mask
    two = np.stack([rc.rows_mask(pids[:120]), ~rc.rows_mask(pids[:120])])
    of = np.array([0, 1, 1, 0])
    for within in (two, pack_mask(two)):
        D, I = rc.search(torch.from_numpy(q), 9, within=within, within_of=of)
        wD, wI = masked_ref.masked_from_scores(S, two, of, 9)
        np.testing.assert_array_equal(I, pids[wI])
        np.testing.assert_array_equal(D, wD.astype(np.float64))
    assert rc.index.calls[-1] == (9, (2, 5), (nq,))
    # mistakes
    calls = len(rc.index.calls)
    for kw in (dict(within=first, exclude=np.zeros((nq, 1), np.int64)), dict(within_of=of), dict(within=two), dict(within=first[:-1]),
               dict(within=two, within_of=np.array([0, 1, 2, 0])), dict(within=two, within_of=of[:-1])):
        with pytest.raises(ValueError):
            rc.search(q, 9, **kw)
    assert len(rc.index.calls) == calls
    # nothing is cached across remove(): the masks describe the rows as they are now
    assert rc.remove([pids[0], pids[10]]) == 4
    assert rc.ntotal == n - 4 and rc.first_rows_mask().shape == (n - 4,) and int(rc.first_rows_mask().sum()) == 248
    assert np.flatnonzero(rc.rows_mask([pids[1]])).tolist() == [0, 248]
    with pytest.raises(ValueError):
        rc.search(q, 9, within=first)                                     # a mask from before the removal


# ---------------------------------------------------------------------------------------------------------------------
# ShardedSearcher.search_masked over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_masked_double_restates_the_contract(oracle):
    import torch
    from haconvdr_amd.index import pack_mask
    from tests import doubles, doubles_masked
    x = np.array([[1.0] * 32, [2.0] * 32, [1.0] * 32, [np.nan] * 32, [3.0] * 32], np.float32)
    q = np.ones((1, 32), np.float32)
    masks = torch.from_numpy(pack_mask(np.array([[True, True, True, True, False]])))
    keys = doubles_masked.make_local_masked_keys(oracle, x)(torch.from_numpy(q), 4, masks, None, 100)
    D, pos = doubles.unpack_keys(keys.numpy())
    assert pos.tolist() == [[101, 100, 102, -1]] and D[0, :3].tolist() == [64.0, 32.0, 32.0]
    assert doubles_masked.CALLS == [(4, 1, 1, 100)]
    doubles_masked.CALLS.clear()


def test_sharded_search_masked_gloo(oracle):
    world, port = 2, _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="2")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_gloo_worker_masked.py")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
        assert "OK" in o


# ---------------------------------------------------------------------------------------------------------------------
# proofs about the inputs of tests/test_index_masked_gpu.py
def test_per_query_masks_differ_from_their_tiles_union(oracle):
    """A scan that tested the OR of its tile's masks instead of the lane's own query's mask would pass a test whose masks
    agree inside a tile: in every per-query-mask case some query's top-k under the union differs from its own."""
    x, q = masked_cases.base_case()
    S = rank_ref.canon_scores(oracle, x, q)
    nq = len(q)
    per_query = masked_cases.per_query_masks()
    grouped, mask_of = masked_cases.grouped_masks()
    disjoint = masked_cases.disjoint_masks()
    for name, masks, mo, rows in (("a mask per query", per_query, np.arange(nq), slice(0, nq)), ("five masks", grouped, mask_of, slice(0, nq)),
                                  ("disjoint", disjoint, np.arange(16), slice(0, 16))):
        for k, QT in ((10, 16), (2048, 4)):
            own = masked_ref.masked_from_scores(S[rows], masks, mo, k)[1]
            union = masked_ref.masked_from_scores(S[rows], masked_cases.union_of_tile(masks, mo, QT), None, k)[1]
            differ = (own != union).any(axis=1)
            assert differ.any(), (name, k)
            if name != "five masks" and QT == 16:                        # (at QT = 4 the 37th query is alone in its tile)
                assert differ.all(), (name, k)
    assert (disjoint.sum(axis=0) == 1).all()                               # pairwise disjoint, together every row
    assert len(set(mask_of[:16].tolist())) == 5 and all(len(set(mask_of[t:t + 4].tolist())) >= 2 for t in range(0, 36, 4))


def test_deselected_rows_are_the_unmasked_answer(oracle):
    x, q = masked_cases.base_case()
    q = q[:5]
    S = rank_ref.canon_scores(oracle, x, q)
    masks = masked_cases.deselected_half(S)
    k = 10
    top = oracle.flat_ip_search(x, q, k)[1]
    own = masked_ref.masked_from_scores(S, masks, None, k)[1]
    assert (own >= 0).all()
    for i in range(len(q)):
        assert not set(top[i].tolist()) & set(own[i].tolist())
        assert not masks[i][top[i]].any()
    assert abs(int(masks[0].sum()) - len(x) // 2) <= 1


def test_monotone_cases_are_monotone(oracle):
    for ascending in (True, False):
        x, q = masked_cases.monotone_case(ascending)
        S = rank_ref.canon_scores(oracle, x, q).astype(np.float64)
        steps = np.diff(S, axis=1)
        assert ((steps > 0) if ascending else (steps < 0)).mean() > 0.99
