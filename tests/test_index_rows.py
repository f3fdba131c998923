"""Rows by id (reconstruct / score_ids), the parts that need no GPU: the C-ABI surface of the five new entry points, the
resource report of their kernels, and the argument checks of the Python mirrors, which raise ValueError before the library
is called and are therefore factored so that they can be called without a handle."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("hac_index_reconstruct", "hac_index_reconstruct_ids", "hac_index_reconstruct_device", "hac_index_score_ids",
               "hac_index_score_ids_device")
NEW_KERNELS = ("untile_range_kernel", "rows_by_id_kernel", "score_ids_kernel")


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
        assert f is not None and f.argtypes is not None and f.restype is not None, sym


def _resource_blocks():
    path = os.path.join(ROOT, "haconvdr_amd", "csrc", "flat_ip.resources.txt")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(path)])
    return re.split(r"remark: Function Name: ", open(path).read())


def test_rows_by_id_kernels_use_no_scratch():
    """The three kernels keep everything in registers: a scratch access between the loads of the rows in flight would be a
    full drain of them.  (Occupancy is theirs to choose; 0 bytes of scratch and no spill is the contract.)"""
    seen = set()
    for b in _resource_blocks():
        head = b.split("\n", 1)[0]
        for k in NEW_KERNELS:
            if k in head:
                seen.add(k)
                assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b[:200]
                assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, b[:200]
                assert int(re.search(r"SGPRs Spill: (\d+)", b).group(1)) == 0, b[:200]
    assert seen == set(NEW_KERNELS), seen


def test_rescore_kernel_keeps_its_registers():
    """score_ids_kernel carries its own copy of the chain loop so that rescore_kernel compiles as before: 94 VGPRs, no scratch."""
    blocks = [b for b in _resource_blocks() if "rescore_kernel" in b.split("\n", 1)[0]]
    assert len(blocks) == 1
    b = blocks[0]
    assert int(re.search(r"VGPRs: (\d+)", b).group(1)) == 94, b[:400]
    assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b[:400]
    assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, b[:400]


# ---------------------------------------------------------------------------------------------------------------------
# argument checks (no handle)
@pytest.mark.parametrize("ids, ndim", [
    ([1.0, 2.0], 1),                                  # float ids
    (np.zeros((2, 2), np.int64), 1),                  # a matrix where a list is expected
    (np.zeros(3, np.int64), 2),                       # a list where a matrix is expected
    (np.array(["a"]), 1),
    (np.array([2 ** 63], np.uint64), 1),              # does not fit int64
    (np.zeros(3, np.int64), 0),                       # reconstruct(i) takes one id
])
def test_ids_check_raises_value_error(ids, ndim):
    from haconvdr_amd import index
    with pytest.raises(ValueError):
        index._as_ids(ids, ndim, "test")


def test_ids_check_accepts_every_integer_dtype():
    from haconvdr_amd import index
    for dt in (np.int8, np.int32, np.int64, np.uint32, np.uint64):
        a = index._as_ids(np.array([3, 1, 2], dt), 1, "test")
        assert a.dtype == np.int64 and a.flags.c_contiguous and a.tolist() == [3, 1, 2]
    a = index._as_ids(np.arange(12, dtype=np.int64).reshape(3, 4)[:, ::2], 2, "test")      # a strided view is copied
    assert a.flags.c_contiguous and a.shape == (3, 2)
    assert index._as_ids(np.int32(7), 0, "test").reshape(1).tolist() == [7]
    assert index._as_ids(-1, 0, "test").reshape(1).tolist() == [-1]


@pytest.mark.parametrize("i0, n", [(0.5, 1), (0, 1.0), ("0", 1), (True, 1), (0, False)])
def test_range_check_raises_value_error(i0, n):
    from haconvdr_amd import index
    with pytest.raises(ValueError):
        index._as_range(i0, n, "test")


def test_range_check_passes_integers_through():
    from haconvdr_amd import index
    assert index._as_range(np.int64(5), None, "test") == (5, None)
    assert index._as_range(0, np.int32(7), "test") == (0, 7)
    assert index._as_range(-3, -1, "test") == (-3, -1)      # (what is outside the index is the library's to refuse)


def test_score_args_check():
    from haconvdr_amd import index
    q = np.zeros((3, 96), np.float64)
    ids = np.zeros((3, 5), np.int32)
    qq, ii = index._pair_args(q, ids, 96, "score_ids")
    assert qq.dtype == np.float32 and ii.dtype == np.int64 and qq.shape == (3, 96) and ii.shape == (3, 5)
    for bad_q, bad_ids in ((np.zeros((3, 95)), ids),                       # wrong dimension
                           (np.zeros(96), ids),                            # one query must still be [1, d]
                           (q, np.zeros((2, 5), np.int64)),                # a list per query
                           (q, np.zeros(5, np.int64)),
                           (q, np.zeros((3, 5), np.float32)),
                           (np.zeros((3, 96), np.complex64), ids),
                           (np.zeros((3, 96), object), ids)):
        with pytest.raises(ValueError):
            index._pair_args(bad_q, bad_ids, 96, "score_ids")


@pytest.mark.parametrize("k", [0, -1, 2049, 1.5, "10", True])
def test_k_check_raises_value_error(k):
    from haconvdr_amd import index
    with pytest.raises(ValueError):
        index._as_k(k, "test")
    assert index._as_k(np.int64(10), "test") == 10 and index._as_k(2048, "test") == 2048


def test_tensor_checks_refuse_host_tensors_and_wrong_dtypes():
    """The tensor forms hand raw device pointers to kernels: a CPU tensor, a wrong dtype or a wrong rank must never get there."""
    import torch
    from haconvdr_amd import index
    with pytest.raises(ValueError):
        index._ids_tensor(torch.zeros(4, dtype=torch.int64), 1, "test")                    # not on the GPU
    with pytest.raises(ValueError):
        index._ids_tensor(np.zeros(4, np.int64), 1, "test")                                # not a tensor
    with pytest.raises(ValueError):
        index._queries_tensor(torch.zeros(2, 96), 96, "test")
    with pytest.raises(ValueError):
        index._pair_args_tensor(torch.zeros(2, 96), torch.zeros(2, 3, dtype=torch.int64), 96, "score_ids_tensor")
    # (dtype and rank mistakes on real CUDA tensors: tests/test_index_rows_gpu.py)
