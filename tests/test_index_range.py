"""Range search, the parts that need no GPU: the C-ABI surface of the two entry points, the resource lines of the range_*
kernels, the reference of tests/range_ref.py against the oracle's search and rank_ref's counts (the three identities of
include/haconvdr.h), the argument checks of the Python mirrors (ValueError before the library is called, no handle needed) and
ResidentCorpus.range_search / ahead_of over a stand-in index."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import range_ref, rank_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("hac_index_range_search", "hac_index_range_search_device")
RANGE_KERNELS = ("range_emit_kernel", "range_offsets_kernel", "range_scatter_kernel", "range_sort_kernel", "range_merge_kernel",
                 "range_results_kernel")


def test_new_entry_points_are_declared_listed_and_exported():
    from haconvdr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "haconvdr.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(hac_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()                      # dlopen only; nothing is computed
    for sym in NEW_SYMBOLS:
        assert sym in declared, sym
        assert sym in _lib.EXPORTED_SYMBOLS, sym
        f = getattr(L, sym)
        assert f.argtypes is not None and f.restype is not None, sym
    assert len(L.hac_index_range_search.argtypes) == 8 and len(L.hac_index_range_search_device.argtypes) == 10


def test_range_kernels_use_no_scratch():
    path = os.path.join(ROOT, "haconvdr_amd", "csrc", "flat_ip.resources.txt")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(path)])
    blocks = re.split(r"remark: Function Name: ", open(path).read())
    named = [b for b in blocks if re.search(r"\d+range_[a-z_]+kernel", b.split("\n", 1)[0])]
    assert len(named) == len(RANGE_KERNELS), [b.split("\n", 1)[0] for b in named]
    for kernel in RANGE_KERNELS:
        mine = [b for b in named if kernel in b.split("\n", 1)[0]]
        assert len(mine) == 1, kernel
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", mine[0]).group(1)) == 0, kernel
        assert int(re.search(r"VGPRs Spill: (\d+)", mine[0]).group(1)) == 0, kernel
        assert int(re.search(r"SGPRs Spill: (\d+)", mine[0]).group(1)) == 0, kernel


# ---------------------------------------------------------------------------------------------------------------------
# the reference itself
def _tie_case(oracle):
    """400 x 32, grid-valued rows of which many repeat, integer queries: exact scores, long ties; one NaN row, one Inf row"""
    from haconvdr_amd import synth
    n, d, nq = 400, 32, 7
    base = ((synth.uniform_u32(0x5A0, 24 * d) % np.uint32(17)).astype(np.float32).reshape(24, d) - 8.0) / 8.0
    x = base[(synth.uniform_u32(0x5A1, n) % np.uint32(24)).astype(np.int64)]
    x[37, 3] = np.nan
    x[200] = np.finfo(np.float32).max
    q = (synth.uniform_u32(0x5A2, nq * d) % np.uint32(9)).astype(np.float32).reshape(nq, d) - 4.0
    q[0] = 0.0
    return x, q, rank_ref.canon_scores(oracle, x, q)


def test_reference_holds_the_three_identities(oracle):
    x, q, S = _tie_case(oracle)
    n, nq = S.shape[1], S.shape[0]
    oD, oI = oracle.flat_ip_search(x, q, n)                         # the unbounded search: NaN rows are padding at the end
    assert np.isnan(S[1:, 37]).all() and any(len(np.unique(S[i][~np.isnan(S[i])])) < 60 for i in range(nq))
    for pos in (0, 1, 17, 150, 390):
        radius = oD[:, pos].copy()                                   # a score dozens of rows share
        radius[0] = -0.0 if pos % 2 else 0.0                         # the zero query: every score +-0
        lims, D, I = range_ref.range_from_scores(S, radius)
        np.testing.assert_array_equal(np.diff(lims), rank_ref.count_ahead(S, radius[:, None], np.zeros((nq, 1), np.int64))[:, 0])
        assert lims[1] == 0
        ranks = rank_ref.rank_ids_from_scores(S, np.zeros((nq, 0), np.int64))
        for i in range(nq):
            m = lims[i + 1] - lims[i]
            seg = slice(lims[i], lims[i + 1])
            for k in (1, 100, n):
                keep = oD[i, :k] > radius[i]
                take = min(k, m)
                assert keep.sum() == take and keep[:take].all()
                np.testing.assert_array_equal(oI[i, :k][keep], I[seg][:take])
                np.testing.assert_array_equal(range_ref.bits(oD[i, :k][keep]), range_ref.bits(D[seg][:take]))
            ranks = rank_ref.rank_ids_from_scores(S[i:i + 1], I[seg][None, :])
            np.testing.assert_array_equal(ranks[0], np.arange(m))
    # the radius rules
    inf = np.float32(np.inf)
    assert range_ref.range_from_scores(S, np.float32(np.nan))[0][-1] == 0 and range_ref.range_from_scores(S, inf)[0][-1] == 0
    lims = range_ref.range_from_scores(S, -inf)[0]
    np.testing.assert_array_equal(np.diff(lims), (~np.isnan(S) & ~np.isneginf(S)).sum(1))
    lims, D, I = range_ref.range_from_scores(S[:1], np.float32(-1e-30))      # the zero query: every non-NaN row, in row order
    np.testing.assert_array_equal(I, np.flatnonzero(~np.isnan(S[0])))


# ---------------------------------------------------------------------------------------------------------------------
# argument checks (no handle)
def test_range_args_pass_good_arguments_through():
    from haconvdr_amd import index
    q, r = index._range_args(np.zeros((3, 96), np.float64), 0.5, 96)
    assert q.dtype == np.float32 and r.dtype == np.float32 and r.shape == (3,) and (r == 0.5).all()
    q, r = index._range_args(np.zeros((3, 96)), np.array([1.0, np.nan, -np.inf]), 96)
    assert r.dtype == np.float32 and r.flags.c_contiguous and np.isnan(r[1]) and np.isneginf(r[2])
    assert index._range_args(np.zeros((3, 96)), np.arange(6)[::2], 96)[1].tolist() == [0.0, 2.0, 4.0]
    assert index._range_args(np.zeros((0, 96)), 1, 96)[1].shape == (0,)
    assert index._as_cap(0, "t") == 0 and index._as_cap(np.int64(7), "t") == 7


@pytest.mark.parametrize("q, radius", [
    (np.zeros((3, 96)), np.zeros(2)),                   # one per query
    (np.zeros((3, 96)), np.zeros((3, 1))),
    (np.zeros((3, 96)), np.zeros((1, 3))),
    (np.zeros((3, 96)), np.array(["a", "b", "c"])),
    (np.zeros((3, 96)), np.zeros(3, np.complex64)),
    (np.zeros((3, 96)), None),
    (np.zeros((3, 95)), 0.0),                           # wrong dimension
    (np.zeros(96), 0.0),
])
def test_range_args_raise_value_error(q, radius):
    from haconvdr_amd import index
    with pytest.raises(ValueError):
        index._range_args(q, radius, 96)


@pytest.mark.parametrize("cap", [-1, 1.0, 10.5, None, True, "7"])
def test_cap_must_be_a_non_negative_integer(cap):
    from haconvdr_amd import index
    with pytest.raises(ValueError):
        index._as_cap(cap, "range_search_tensor")


def test_tensor_checks_refuse_host_tensors():
    """The tensor form hands raw device pointers to kernels: a CPU tensor or an ndarray must never get there."""
    import torch
    from haconvdr_amd import index
    with pytest.raises(ValueError):
        index._range_args_tensor(torch.zeros(3, 96), torch.zeros(3), 10, None, 96)
    with pytest.raises(ValueError):
        index._range_args_tensor(np.zeros((3, 96), np.float32), np.zeros(3, np.float32), 10, None, 96)


# ---------------------------------------------------------------------------------------------------------------------
# ResidentCorpus over a stand-in index
class _StandInIndex:
    """range_search / score_ids of FlatIPIndex over the oracle's canonical scores"""

    def __init__(self, oracle, x):
        self.oracle, self.x, self.calls = oracle, x, []

    def range_search(self, q, radius):
        from haconvdr_amd import index
        q, radius = index._range_args(q, radius, self.x.shape[1])
        self.calls.append(radius.copy())
        return range_ref.range_search(self.oracle, self.x, q, radius)

    def score_ids(self, q, ids):
        S = rank_ref.canon_scores(self.oracle, self.x, np.asarray(q, np.float32))
        inside = ids >= 0
        got = np.take_along_axis(S, np.where(inside, ids, 0), 1)
        return np.where(inside, got, -np.finfo(np.float32).max).astype(np.float32)


def test_resident_corpus_maps_rows_to_passage_ids(oracle):
    from haconvdr_amd import synth
    from haconvdr_amd.search import ResidentCorpus
    n, d, nq = 300, 32, 5
    x = synth.embeddings(0x5B0, n, d)
    q = synth.embeddings(0x5B1, nq, d)
    pids = (np.arange(n, dtype=np.int64) * 7 + 11)[np.argsort(synth.uniform_u32(0x5B2, n), kind="stable")]    # row -> passage id
    rc = ResidentCorpus.__new__(ResidentCorpus)
    rc.index, rc._ids, rc._lookup = _StandInIndex(oracle, x), pids, None
    S = rank_ref.canon_scores(oracle, x, q)
    lims, D, I = rc.range_search(q, 0.05)
    want = range_ref.range_from_scores(S, np.float32(0.05))
    assert 0 < want[0][-1] < nq * n and D.dtype == np.float64 and I.dtype == np.int64
    np.testing.assert_array_equal(lims, want[0])
    np.testing.assert_array_equal(I, pids[want[2]])
    np.testing.assert_array_equal(D, want[1].astype(np.float64))
    # ahead_of: the rows scoring above each query's gold passage; absent passage -> empty
    full = oracle.flat_ip_search(x, q, n)[1]
    gold_rows = np.array([full[0, 0], full[1, 40], full[2, n - 1], full[3, 7], 0], np.int64)
    gold = pids[gold_rows]
    gold[4] = 5                                                       # no row carries it (ids are 11 mod 7 == 4)
    lims, D, I = rc.ahead_of(q, gold)
    np.testing.assert_array_equal(np.diff(lims), [0, 40, n - 1, 7, 0])
    for i in range(4):
        np.testing.assert_array_equal(I[lims[i]:lims[i + 1]], pids[full[i, :lims[i + 1] - lims[i]]])
    assert np.isposinf(rc.index.calls[-1][4]) and rc.index.calls[-1].dtype == np.float32
    with pytest.raises(ValueError):
        rc.ahead_of(q, gold[:, None])
