"""search_excluding, the parts that need no GPU: the C-ABI surface of the three new entry points, the argument checks of the
Python mirrors (ValueError before the library is called, factored so that they run without a handle, like those of
tests/test_index_rows.py), ResidentCorpus's id -> rows expansion as a pure function, and ShardedSearcher's exclude= over
two gloo ranks with numpy doubles."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("hac_filter_keys_device", "hac_index_search_excluding", "hac_index_search_excluding_device")


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


def test_filter_kernel_uses_no_scratch():
    path = os.path.join(ROOT, "haconvdr_amd", "csrc", "flat_ip.resources.txt")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(path)])
    blocks = [b for b in re.split(r"remark: Function Name: ", open(path).read()) if "filter_keys_kernel" in b.split("\n", 1)[0]]
    assert len(blocks) == 1
    assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blocks[0]).group(1)) == 0
    assert int(re.search(r"VGPRs Spill: (\d+)", blocks[0]).group(1)) == 0


# ---------------------------------------------------------------------------------------------------------------------
# argument checks (no handle)
def test_exclude_args_pass_good_arguments_through():
    from haconvdr_amd import index
    q, k, ex = index._exclude_args(np.zeros((3, 96), np.float64), np.int64(10), np.zeros((3, 5), np.int32), 96)
    assert q.dtype == np.float32 and ex.dtype == np.int64 and ex.shape == (3, 5) and k == 10
    q, k, ex = index._exclude_args(np.zeros((3, 96)), 2000, np.zeros((3, 48), np.int64), 96)      # k + e == HAC_MAX_K
    assert k + ex.shape[1] == 2048
    assert index._exclude_args(np.zeros((3, 96)), 7, np.zeros((3, 0), np.int64), 96)[2].shape == (3, 0)
    assert index._exclude_args(np.zeros((0, 96)), 7, np.zeros((0, 4), np.int64), 96)[0].shape == (0, 96)


@pytest.mark.parametrize("q, k, exclude", [
    (np.zeros((3, 96)), 10, np.zeros((3, 5), np.float32)),       # float ids
    (np.zeros((3, 96)), 10, np.zeros(5, np.int64)),              # one list, not one per query
    (np.zeros((3, 96)), 10, np.zeros((3, 5, 1), np.int64)),
    (np.zeros((3, 96)), 10, np.zeros((2, 5), np.int64)),         # exclude.shape[0] != nq
    (np.zeros((3, 96)), 2000, np.zeros((3, 49), np.int64)),      # k + e > HAC_MAX_K
    (np.zeros((3, 96)), 1, np.zeros((3, 2048), np.int64)),
    (np.zeros((3, 96)), 0, np.zeros((3, 5), np.int64)),
    (np.zeros((3, 96)), 2.0, np.zeros((3, 5), np.int64)),
    (np.zeros((3, 95)), 10, np.zeros((3, 5), np.int64)),         # wrong dimension
    (np.zeros(96), 10, np.zeros((1, 5), np.int64)),
    (np.zeros((3, 96)), 10, np.array([[2 ** 63] * 2] * 3, np.uint64)),
])
def test_exclude_args_raise_value_error(q, k, exclude):
    from haconvdr_amd import index
    with pytest.raises(ValueError):
        index._exclude_args(q, k, exclude, 96)


def test_tensor_checks_refuse_host_tensors():
    """The tensor forms hand raw device pointers to kernels: a CPU tensor or an ndarray must never get there."""
    import torch
    from haconvdr_amd import index
    with pytest.raises(ValueError):
        index._exclude_args_tensor(torch.zeros(3, 96), 10, torch.zeros(3, 5, dtype=torch.int64), 96)
    with pytest.raises(ValueError):
        index._filter_args(torch.zeros(3, 13, dtype=torch.int64), torch.zeros(3, 3, dtype=torch.int64), 10)
    with pytest.raises(ValueError):
        index._filter_args(np.zeros((3, 13), np.int64), np.zeros((3, 3), np.int64), 10)
    # (shape and dtype mistakes on real CUDA tensors are the same helpers' checks: tests/test_index_rows_gpu.py)


def test_sharded_searcher_checks_the_exclude_shape_before_any_hook_runs():
    import torch
    from haconvdr_amd.sharded import ShardedSearcher

    def never(*a):
        raise AssertionError("a hook ran")
    s = ShardedSearcher(None, 0, local_keys=never, merge=never, to_results=never, filter=never)
    for bad in (torch.zeros(5, dtype=torch.int64), torch.zeros((2, 5), dtype=torch.int64)):
        with pytest.raises(ValueError):
            s.search(torch.zeros(3, 96), 10, exclude=bad)


# ---------------------------------------------------------------------------------------------------------------------
# ResidentCorpus: external ids -> the rows that carry them
def _lookup(ids):
    order = np.argsort(ids, kind="stable")
    return ids[order], order.astype(np.int64)


def test_rows_carrying_expands_every_row_of_an_id():
    from haconvdr_amd.search import rows_carrying
    ids = np.array([50, 70, 50, 90, 70, 50, -1, 10], np.int64)          # 50 on three rows, 70 on two; -1 is an id a row may carry
    lk = _lookup(ids)
    rows = rows_carrying(*lk, np.array([[50, -1, 90], [1000, -1, -1], [70, 70, 50], [10, 60, 90]], np.int64))
    assert rows.dtype == np.int64 and rows.shape == (4, 7)               # the widest list: 2 + 2 + 3 rows
    assert [sorted(r[r >= 0].tolist()) for r in rows] == [[0, 2, 3, 5], [], [0, 1, 1, 2, 4, 4, 5], [3, 7]]
    for r in rows:                                                       # the rows first, the padding behind them
        m = int((r >= 0).sum())
        assert (r[:m] >= 0).all() and (r[m:] == -1).all()
    assert 6 not in rows                                                 # -1 in the list is padding, never "the row whose id is -1"
    # brute force over random lists
    rng = np.random.default_rng(5)
    ids = rng.integers(0, 40, 300)
    lk = _lookup(ids)
    ex = rng.integers(-1, 60, (17, 9))
    rows = rows_carrying(*lk, ex)
    for i in range(len(ex)):
        want = sorted(r for v in ex[i] if v != -1 for r in np.nonzero(ids == v)[0].tolist())
        assert sorted(rows[i][rows[i] >= 0].tolist()) == want
    assert rows.shape[1] == max(sum(int((ids == v).sum()) for v in ex[i] if v != -1) for i in range(len(ex)))


def test_rows_carrying_edges():
    from haconvdr_amd.search import rows_carrying
    lk = _lookup(np.array([5, 6, 7], np.int64))
    assert rows_carrying(*lk, np.zeros((4, 0), np.int64)).shape == (4, 0)
    assert rows_carrying(*lk, np.full((4, 3), -1, np.int64)).shape == (4, 0)
    assert rows_carrying(*lk, np.array([[4], [8]], np.int64)).shape == (2, 0)          # ids no block holds
    assert rows_carrying(*lk, np.zeros((0, 3), np.int64)).shape == (0, 0)
    assert rows_carrying(*lk, np.array([[7]], np.int32)).tolist() == [[2]]
    assert rows_carrying(*_lookup(np.zeros(0, np.int64)), np.array([[7]], np.int64)).shape == (1, 0)
    for bad in (np.array([[1.0]]), np.array([1, 2]), np.array([["a"]])):
        with pytest.raises(ValueError):
            rows_carrying(*lk, bad)


# ---------------------------------------------------------------------------------------------------------------------
# ShardedSearcher(exclude=) over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_filter_double_restates_the_contract():
    import torch
    from tests import doubles, doubles_filter
    D = np.array([[9.0, 8.0, 7.0, 6.0, 0.0, 0.0]], np.float32)
    pos = np.array([[4, 0xFFFFFFFF, 0, 11, -1, -1]], np.int64)
    keys = torch.from_numpy(doubles.pack_keys(D, pos))
    ex = torch.tensor([[0xFFFFFFFF, -1, 11, 11, 2 ** 32 + 4, -5]])
    out = doubles_filter.filter(keys, ex, 3)
    d2, p2 = doubles.unpack_keys(out.numpy())
    assert p2.tolist() == [[4, 0, -1]] and d2[0, :2].tolist() == [9.0, 7.0]
    doubles_filter.CALLS.clear()


def test_sharded_search_excluding_gloo(oracle):
    world, port = 2, _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="2")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_gloo_worker_excluding.py")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
        assert "OK" in o
