"""search_among, the parts that need no GPU: the C-ABI surface of the three entry points, the resource lines of the among_*
kernels, the reference of tests/among_ref.py against the oracle's search, rank_ref's scores and tests/excluding.py (the three
identities of include/haconvdr.h), the argument checks of the Python mirrors (ValueError before the library is called, no
handle needed), ResidentCorpus.rerank over a stand-in index and ShardedSearcher.search_among over two gloo ranks."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests import among_ref, excluding, rank_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("hac_index_search_among", "hac_index_search_among_device", "hac_index_search_among_keys_device")
AMONG_KERNELS = ("among_keys_kernel", "among_select_kernel")


def test_new_entry_points_are_declared_listed_and_exported():
    from haconvdr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "haconvdr.h")).read()
    assert re.search(r"#define\s+HAC_MAX_AMONG\s+4096\b", hdr) and _lib.HAC_MAX_AMONG == 4096
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(hac_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()                      # dlopen only; nothing is computed
    for sym in NEW_SYMBOLS:
        assert sym in declared, sym
        assert sym in _lib.EXPORTED_SYMBOLS, sym
        f = getattr(L, sym)
        assert f.argtypes is not None and f.restype is not None, sym
    assert [len(getattr(L, sym).argtypes) for sym in NEW_SYMBOLS] == [8, 10, 9]


def test_among_kernels_use_no_scratch():
    path = os.path.join(ROOT, "haconvdr_amd", "csrc", "flat_ip.resources.txt")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(path)])
    blocks = re.split(r"remark: Function Name: ", open(path).read())
    named = [b for b in blocks if re.search(r"\d+among_[a-z_]+kernel", b.split("\n", 1)[0])]
    assert len(named) == len(AMONG_KERNELS), [b.split("\n", 1)[0] for b in named]
    for kernel in AMONG_KERNELS:
        mine = [b for b in named if kernel in b.split("\n", 1)[0]]
        assert len(mine) == 1, kernel
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", mine[0]).group(1)) == 0, kernel
        assert int(re.search(r"VGPRs Spill: (\d+)", mine[0]).group(1)) == 0, kernel
        assert int(re.search(r"SGPRs Spill: (\d+)", mine[0]).group(1)) == 0, kernel


# ---------------------------------------------------------------------------------------------------------------------
# the reference itself
def _tie_case(oracle):
    """tests/test_index_range.py::_tie_case's shape: 400 x 32, grid-valued rows of which many repeat, integer queries (exact
    scores, long ties), one NaN row, one FLT_MAX row, a zero query"""
    from haconvdr_amd import synth
    n, d, nq = 400, 32, 7
    base = ((synth.uniform_u32(0x7A0, 24 * d) % np.uint32(17)).astype(np.float32).reshape(24, d) - 8.0) / 8.0
    x = base[(synth.uniform_u32(0x7A1, n) % np.uint32(24)).astype(np.int64)]
    x[37, 3] = np.nan
    x[200] = np.finfo(np.float32).max
    q = (synth.uniform_u32(0x7A2, nq * d) % np.uint32(9)).astype(np.float32).reshape(nq, d) - 4.0
    q[0] = 0.0
    return x, q, rank_ref.canon_scores(oracle, x, q)


def _shuffled(rows, seed, repeats, pads):
    """per query: the rows of rows[i] (>= 0 only) permuted, `repeats` of them named a second time and `pads` slots of -1 mixed in"""
    rng = np.random.default_rng(seed)
    out = []
    for r in rows:
        r = r[r >= 0]
        c = np.concatenate([r, rng.choice(r, repeats) if len(r) else r[:0], np.full(pads, -1, np.int64)])
        out.append(rng.permutation(c))
    w = max(len(c) for c in out)
    return np.stack([np.concatenate([c, np.full(w - len(c), -1, np.int64)]) for c in out]).astype(np.int64)


def test_reference_holds_the_three_identities(oracle):
    x, q, S = _tie_case(oracle)
    nq, n = S.shape
    assert np.isnan(S[1:, 37]).all() and any(len(np.unique(S[i][~np.isnan(S[i])])) < 60 for i in range(nq))
    # 1. among(q, shuffled I of search(q, k'), k) == search(q, k) for k <= k', and beyond k' the tail is padding
    for kp in (1, 40, 150):
        oD, oI = oracle.flat_ip_search(x, q, kp)
        cand = _shuffled(oI, 0x7B0 + kp, repeats=kp // 2 + 1, pads=5)
        m = kp                                                            # distinct candidates per query
        for k in sorted({1, max(1, m - 1), m, m + 1}):
            D, I = among_ref.among_from_scores(S, cand, k)
            kk = min(k, m)
            np.testing.assert_array_equal(I[:, :kk], oI[:, :kk])
            np.testing.assert_array_equal(among_ref.bits(D[:, :kk]), among_ref.bits(oD[:, :kk]))
            assert (I[:, kk:] == -1).all() and (D[:, kk:] == -among_ref.FMAX).all()
            # 2. D has the bits of the canonical scores of the rows I names
            named = I >= 0
            own = np.take_along_axis(S, np.where(named, I, 0), 1)
            np.testing.assert_array_equal(among_ref.bits(D)[named], among_ref.bits(own)[named])
            assert not np.isnan(D).any()
    # 3. with E the complement of set(c): among(q, c, k) == search_excluding(q, k, E), the NaN row on either side
    for e, k in ((9, 30), (60, 388)):
        rng = np.random.default_rng(0x7C0 + e)
        E = np.stack([rng.choice(n, e, replace=False) for _ in range(nq)]).astype(np.int64)
        E[0, 0], E[1, 1] = 37, 200                                        # the NaN row excluded once, the FLT_MAX row once
        comp = [np.setdiff1d(np.arange(n), E[i]) for i in range(nq)]
        cand = _shuffled(comp, 0x7C1 + e, repeats=17, pads=3)
        assert cand.shape[1] >= n - e + 20                                # (E may name a row twice)
        got = among_ref.among_from_scores(S, cand, k)
        want = excluding.filtered_topk(oracle, x, q, k, E)
        among_ref.assert_same(got, want, f"e={e}")
        among_ref.assert_same(got, excluding.deleted_topk(oracle, x, q, k, E), f"e={e}, rows deleted")
    # the tie rule and the set rule on their own: every candidate the same row; a tie ascends by row
    D, I = among_ref.among_from_scores(S, np.full((nq, 9), 5, np.int64), 3)
    assert (I[:, 0] == 5).all() and (I[:, 1:] == -1).all()
    D, I = among_ref.among_from_scores(S[:1], np.array([[300, 7, -1, 150, 7, 399, 37, 400, -9]], np.int64), 6)
    assert I.tolist() == [[7, 150, 300, 399, -1, -1]]                     # the zero query: every score +0.0 (row 37: NaN, 400 and -9: outside)
    D, I = among_ref.among_from_scores(S, np.zeros((nq, 0), np.int64), 4)
    assert (I == -1).all() and (D == -among_ref.FMAX).all()


# ---------------------------------------------------------------------------------------------------------------------
# argument checks (no handle)
def test_among_args_pass_good_arguments_through():
    from haconvdr_amd import index
    q, k, c = index._among_args(np.zeros((3, 96), np.float64), np.int64(10), np.zeros((3, 5), np.int32), 96)
    assert q.dtype == np.float32 and c.dtype == np.int64 and c.flags.c_contiguous and c.shape == (3, 5) and k == 10
    assert index._among_args(np.zeros((3, 96)), 2048, np.zeros((3, 4096), np.int64), 96)[2].shape == (3, 4096)    # both ceilings
    assert index._among_args(np.zeros((3, 96)), 7, np.zeros((3, 0), np.int64), 96)[2].shape == (3, 0)
    assert index._among_args(np.zeros((3, 96)), 7, np.full((3, 2), -1), 96)[1] == 7                                # k may exceed m
    assert index._among_args(np.zeros((0, 96)), 7, np.zeros((0, 4), np.int64), 96)[0].shape == (0, 96)


@pytest.mark.parametrize("q, k, cand", [
    (np.zeros((3, 96)), 10, np.zeros((3, 5), np.float32)),       # float ids
    (np.zeros((3, 96)), 10, np.zeros(5, np.int64)),              # wrong rank: one list, not one per query
    (np.zeros((3, 96)), 10, np.zeros((3, 5, 1), np.int64)),
    (np.zeros((3, 96)), 10, np.zeros((2, 5), np.int64)),         # nq mismatch
    (np.zeros((3, 96)), 10, np.zeros((3, 4097), np.int64)),      # m = 4097
    (np.zeros((3, 96)), 0, np.zeros((3, 5), np.int64)),          # k = 0
    (np.zeros((3, 96)), 2049, np.zeros((3, 5), np.int64)),       # k = 2049
    (np.zeros((3, 96)), 2.0, np.zeros((3, 5), np.int64)),
    (np.zeros((3, 95)), 10, np.zeros((3, 5), np.int64)),         # wrong dimension
    (np.zeros((3, 96)), 10, np.array([[2 ** 63] * 2] * 3, np.uint64)),
])
def test_among_args_raise_value_error(q, k, cand):
    from haconvdr_amd import index
    with pytest.raises(ValueError):
        index._among_args(q, k, cand, 96)


def test_tensor_checks_refuse_host_tensors():
    """The tensor forms hand raw device pointers to kernels: a CPU tensor or an ndarray must never get there."""
    import torch
    from haconvdr_amd import index
    with pytest.raises(ValueError):
        index._among_args_tensor(torch.zeros(3, 96), 10, torch.zeros(3, 5, dtype=torch.int64), None, 96)
    with pytest.raises(ValueError):
        index._among_args_tensor(np.zeros((3, 96), np.float32), 10, np.zeros((3, 5), np.int64), None, 96)
    # (shape, dtype, k and m mistakes on real CUDA tensors: tests/test_index_among_gpu.py)


def test_sharded_searcher_checks_cand_before_any_hook_runs():
    import torch
    from haconvdr_amd.sharded import ShardedSearcher

    def never(*a):
        raise AssertionError("a hook ran")
    s = ShardedSearcher(None, 0, local_keys=never, merge=never, to_results=never, filter=never, n_local=10, local_among_keys=never)
    for bad in (torch.zeros(5, dtype=torch.int64), torch.zeros((2, 5), dtype=torch.int64), torch.zeros((3, 5), dtype=torch.int32)):
        with pytest.raises(ValueError):
            s.search_among(torch.zeros(3, 96), 10, bad)


# ---------------------------------------------------------------------------------------------------------------------
# ResidentCorpus.rerank over a stand-in index
class _StandInIndex:
    """search_among_tensor of FlatIPIndex over the oracle's canonical scores, on CPU tensors"""

    def __init__(self, oracle, x):
        self.oracle, self.x, self.calls = oracle, x, []

    def search_among_tensor(self, q, k, cand, id_map=None, stream=None):
        import torch
        self.calls.append((int(k), tuple(cand.shape)))
        D, I = among_ref.among(self.oracle, self.x, q.numpy(), cand.numpy(), k)
        if id_map is not None:
            I = np.where(I >= 0, id_map.numpy()[np.clip(I, 0, None)], -1)
        return torch.from_numpy(D), torch.from_numpy(I)


def test_resident_corpus_rerank_ranks_every_row_of_an_id(oracle):
    import torch
    from haconvdr_amd import _lib, synth
    from haconvdr_amd.search import ResidentCorpus
    n, d, nq = 300, 32, 4
    x = synth.embeddings(0x7D0, n, d)
    q = synth.embeddings(0x7D1, nq, d)
    pids = np.arange(n, dtype=np.int64) * 7 + 11                          # row -> passage id ...
    pids[250:] = pids[:50]                                                # ... the first 50 ids carried by two rows each
    rc = ResidentCorpus.__new__(ResidentCorpus)
    rc.index, rc._ids, rc._lookup = _StandInIndex(oracle, x), pids, None
    rc.dev, rc.id_map = torch.device("cpu"), torch.from_numpy(pids)
    S = rank_ref.canon_scores(oracle, x, q)
    run = np.array([[pids[3], pids[100], 5, -1, pids[120], pids[100]],   # 5: an id no block holds (ids are 4 mod 7)
                    [pids[10], pids[20], pids[30], -1, -1, -1],
                    [5, 12, -1, -1, -1, -1],
                    [pids[299], pids[150], pids[151], pids[152], -1, pids[150]]], np.int64)   # row 299 carries row 49's id
    rows = [[3, 253, 100, 120], [10, 260, 20, 270, 30, 280], [], [49, 299, 150, 151, 152]]
    D, I = rc.rerank(q, run, 5)
    assert D.dtype == np.float64 and I.dtype == np.int64 and D.shape == I.shape == (nq, 5)
    for i in range(nq):
        r = np.array(rows[i], np.int64)
        order = r[np.lexsort((r, -S[i, r].astype(np.float64)))][:5] if len(r) else r
        np.testing.assert_array_equal(I[i, :len(order)], pids[order])
        np.testing.assert_array_equal(D[i, :len(order)], S[i, order].astype(np.float64))
        assert (I[i, len(order):] == -1).all() and (D[i, len(order):] == -float(among_ref.FMAX)).all()
    assert sorted(I[0, :4].tolist()) == sorted([pids[3], pids[3], pids[100], pids[120]])      # both rows of id pids[3], pids[100] once per row
    assert (I[2] == -1).all()
    assert rc.index.calls == [(5, (nq, 6))]                              # the widest row list: 6 rows
    # a CUDA-free tensor of queries goes the same way
    D2, I2 = rc.rerank(torch.from_numpy(q), run, 5)
    assert np.array_equal(D, D2) and np.array_equal(I, I2)
    # too wide a list: every id names two rows
    wide = np.tile(pids[:50], (nq, _lib.HAC_MAX_AMONG // 100 + 1))
    assert wide.shape[1] * 2 > _lib.HAC_MAX_AMONG >= wide.shape[1]
    with pytest.raises(ValueError):
        rc.rerank(q, wide, 5)
    for bad in (run[:-1], run[0], run.astype(np.float32)):
        with pytest.raises(ValueError):
            rc.rerank(q, bad, 5)
    assert len(rc.index.calls) == 2


# ---------------------------------------------------------------------------------------------------------------------
# ShardedSearcher.search_among over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_among_double_restates_the_contract(oracle):
    import torch
    from tests import doubles, doubles_among
    x = np.array([[1.0] * 32, [2.0] * 32, [1.0] * 32, [np.nan] * 32], np.float32)
    q = np.ones((1, 32), np.float32)
    keys = doubles_among.make_local_among_keys(oracle, x)(torch.from_numpy(q), 4, torch.tensor([[2, 0, 3, 1, 2, -1, 9]]), 100)
    D, pos = doubles.unpack_keys(keys.numpy())
    assert pos.tolist() == [[101, 100, 102, -1]] and D[0, :3].tolist() == [64.0, 32.0, 32.0]
    assert doubles_among.CALLS == [(4, 7, 100)]
    doubles_among.CALLS.clear()


def test_sharded_search_among_gloo(oracle):
    world, port = 2, _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="2")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_gloo_worker_among.py")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
        assert "OK" in o
