"""The argument checks of haconvdr_amd/index.py, table-driven: no handle, no library, no GPU.

Every host call that takes an integer array goes through index._int_array; every tensor call hands its tensors to
index._tensor_arg.  The table below names each per-call check, the argument it owns and the shapes it allows, and asks the
same of all of them: every integer dtype comes out as C-contiguous int64 with its values, and a float dtype, a wrong rank, a
wrong length and a uint64 above 2^63 - 1 raise ValueError.  (The same mistakes on CUDA tensors, method by method:
tests/test_index_tensor_checks_gpu.py.)"""
import numpy as np
import pytest

from haconvdr_amd import index

D, NQ, NTOTAL = 96, 3, 130
Q = np.zeros((NQ, D), np.float32)
INT_DTYPES = [np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64]
ZEROS = np.zeros(NQ, np.float32)
MASKS = np.ones((2, NTOTAL), np.bool_)

# name -> (call(array) -> the int64 array the check returns, allowed shapes, a shape of the wrong rank, a shape of the wrong
#          length or None where the check fixes none)
HOST_CHECKS = {
    "_int_array(ndim=2)": (lambda a: index._int_array(a, "a", "x", ndim=2), [(NQ, 4), (NQ, 0), (0, 4)], (NQ,), None),
    "_int_array(shape=(3, None))": (lambda a: index._int_array(a, "a", "x", shape=(NQ, None)), [(NQ, 4), (NQ, 0)], (NQ,), (2, 4)),
    "_int_array(shape=(130,))": (lambda a: index._int_array(a, "a", "x", shape=(NTOTAL,)), [(NTOTAL,)], (NTOTAL, 1), (NTOTAL + 1,)),
    "_as_ids(0)": (lambda a: index._as_ids(a, 0, "x"), [()], (1,), None),
    "_as_ids(1)": (lambda a: index._as_ids(a, 1, "x"), [(5,), (0,)], (5, 1), None),
    "_as_ids(2)": (lambda a: index._as_ids(a, 2, "x"), [(NQ, 4)], (4,), None),
    "_remove_args": (lambda a: index._remove_args(a, NTOTAL), [(5,), (0,)], (5, 1), None),
    "_pair_args": (lambda a: index._pair_args(Q, a, D, "x")[1], [(NQ, 4), (NQ, 0)], (NQ,), (2, 4)),
    "_rank_args": (lambda a: index._rank_args(Q, a, D)[1], [(NQ, 4), (NQ, 0)], (NQ,), (2, 4)),
    "_exclude_args": (lambda a: index._exclude_args(Q, 10, a, D)[2], [(NQ, 4), (NQ, 0)], (NQ,), (2, 4)),
    "_among_args": (lambda a: index._among_args(Q, 10, a, D)[2], [(NQ, 4), (NQ, 0)], (NQ,), (2, 4)),
    "_as_masks(mask_of)": (lambda a: index._as_masks(MASKS, a, NQ, NTOTAL, "x")[1], [(NQ,)], (NQ, 1), (2,)),
    "_masked_args(mask_of)": (lambda a: index._masked_args(Q, 10, MASKS, a, D, NTOTAL)[3], [(NQ,)], (NQ, 1), (2,)),
    "_grouped_args": (lambda a: index._grouped_args(Q, 10, a, D, NTOTAL)[2], [(NTOTAL,)], (NTOTAL, 1), (NTOTAL - 1,)),
    "_after_args(rows)": (lambda a: index._after_args(Q, 10, (ZEROS, a), D)[3], [(NQ,)], (NQ, 1), (4,)),
    "_as_start": (lambda a: index._as_start(a, NQ, "x"), [(NQ,), ()], (NQ, 1), (2,)),   # (a scalar start: one for every query)
}


def _values(shape, dtype):
    """0 and 1 only: a row, a rank, a label, a mask number and a start of every check above"""
    return (np.arange(int(np.prod(shape))) % 2).astype(dtype).reshape(shape)


@pytest.mark.parametrize("name", list(HOST_CHECKS))
def test_every_integer_dtype_comes_out_as_contiguous_int64(name):
    call, shapes, _, _ = HOST_CHECKS[name]
    for shape in shapes:
        # (a scalar id comes out as [1], np.ascontiguousarray's way with zero dimensions: reconstruct reshapes to that anyway)
        want = np.broadcast_to(_values(shape, np.int64), (NQ,)) if name == "_as_start" else np.atleast_1d(_values(shape, np.int64))
        for dtype in INT_DTYPES:
            out = call(_values(shape, dtype))
            assert out.dtype == np.int64 and out.flags.c_contiguous and out.shape == want.shape, (shape, dtype)
            np.testing.assert_array_equal(out, want)
        if want.size:                                                            # (an empty python list has no integer dtype)
            out = call(_values(shape, np.int64).tolist())
            assert out.dtype == np.int64 and out.flags.c_contiguous and np.array_equal(out, want), shape
        if shape and name != "_as_start":
            strided = np.repeat(_values(shape, np.int64), 2, axis=-1)[..., ::2]   # right dtype, not contiguous
            assert not strided.flags.c_contiguous or strided.size <= 1
            out = call(strided)
            assert out.dtype == np.int64 and out.flags.c_contiguous and np.array_equal(out, want), shape
            ready = _values(shape, np.int64)                                     # nothing to convert: no copy
            assert ready.size == 0 or call(ready).ctypes.data == ready.ctypes.data, shape
    big = np.full(shapes[0], 2 ** 63 - 1, np.uint64)                             # the largest uint64 that int64 holds
    assert (call(big) == 2 ** 63 - 1).all()


@pytest.mark.parametrize("mistake", ["float dtype", "wrong rank", "wrong length", "uint64 above 2^63 - 1"])
@pytest.mark.parametrize("name", list(HOST_CHECKS))
def test_a_mistake_in_an_integer_array_raises_value_error(name, mistake):
    call, shapes, wrong_rank, wrong_length = HOST_CHECKS[name]
    if mistake == "wrong length" and wrong_length is None:
        return                                                                   # (the check fixes no length: any is accepted above)
    bad = {"float dtype": lambda: _values(shapes[0], np.float32),
           "wrong rank": lambda: _values(wrong_rank, np.int64),
           "wrong length": lambda: _values(wrong_length, np.int64),
           "uint64 above 2^63 - 1": lambda: np.full(shapes[0], 2 ** 63, np.uint64)}[mistake]()
    with pytest.raises(ValueError):
        call(bad)
    if mistake == "float dtype":
        with pytest.raises(ValueError):
            call(_values(shapes[0], np.float64))


def test_the_shape_rule_of_both_primitives():
    """None in `shape` is any length; `ndim` asks for the rank alone; the hint ends the message"""
    assert index._int_array(np.zeros((3, 7), np.int16), "a", "x", shape=(None, 7)).shape == (3, 7)
    assert index._int_array(np.zeros((0, 7), np.int16), "a", "x", shape=(None, 7)).shape == (0, 7)
    assert index._int_array(np.zeros((2, 2, 2), np.uint8), "a", "x").shape == (2, 2, 2)          # nothing asked of the shape
    for bad in (np.zeros((3, 6), np.int64), np.zeros(7, np.int64), np.zeros((3, 7, 1), np.int64)):
        with pytest.raises(ValueError, match=r"call: arg must have shape \[\*, 7\].*\(the hint\)$"):
            index._int_array(bad, "arg", "call", shape=(None, 7), hint="(the hint)")
    with pytest.raises(ValueError, match=r"call: arg must have 2 dimension\(s\), got shape \(7,\)$"):
        index._int_array(np.zeros(7, np.int64), "arg", "call", ndim=2)


# ---- the tensor forms: no ndarray and no CPU tensor passes, whichever argument it is ----------------------------------
def _tensor_checks():
    """name -> (call(**tensors), the tensor arguments with dtype name and shape); q is a float32 [3, 96] everywhere"""
    W = index.mask_words(NTOTAL)
    i64, f32 = "int64", "float32"
    return {
        "_ids_tensor": (lambda ids: index._ids_tensor(ids, 2, "x"), {"ids": (i64, (NQ, 4))}),
        "_queries_tensor": (lambda q: index._queries_tensor(q, D, "x"), {}),
        "_check_id_map_tensor": (lambda q, id_map: index._check_id_map_tensor(id_map, q, "x"), {"id_map": (i64, (NTOTAL,))}),
        "_pair_args_tensor": (lambda q, ids: index._pair_args_tensor(q, ids, D, "x"), {"ids": (i64, (NQ, 4))}),
        "_count_args_tensor": (lambda q, ref_scores, ref_bounds: index._count_args_tensor(q, ref_scores, ref_bounds, D),
                               {"ref_scores": (f32, (NQ, 4)), "ref_bounds": (i64, (NQ, 4))}),
        "_range_args_tensor": (lambda q, radius, id_map: index._range_args_tensor(q, radius, 10, id_map, D),
                               {"radius": (f32, (NQ,)), "id_map": (i64, (NTOTAL,))}),
        "_exclude_args_tensor": (lambda q, exclude: index._exclude_args_tensor(q, 10, exclude, D), {"exclude": (i64, (NQ, 4))}),
        "_among_args_tensor": (lambda q, cand, id_map: index._among_args_tensor(q, 10, cand, id_map, D),
                               {"cand": (i64, (NQ, 4)), "id_map": (i64, (NTOTAL,))}),
        "_masked_args_tensor": (lambda q, masks, mask_of, id_map: index._masked_args_tensor(q, 10, masks, mask_of, id_map, D, NTOTAL),
                                {"masks": (i64, (2, W)), "mask_of": (i64, (NQ,)), "id_map": (i64, (NTOTAL,))}),
        "_grouped_args_tensor": (lambda q, group_of, id_map: index._grouped_args_tensor(q, 10, group_of, id_map, D, NTOTAL),
                                 {"group_of": (i64, (NTOTAL,)), "id_map": (i64, (NTOTAL,))}),
        "_after_args_tensor": (lambda q, scores, rows, id_map: index._after_args_tensor(q, 10, (scores, rows), id_map, D),
                               {"scores": (f32, (NQ,)), "rows": (i64, (NQ,)), "id_map": (i64, (NTOTAL,))}),
        "_after_keys_args_tensor": (lambda q, after_keys: index._after_keys_args_tensor(q, 10, after_keys, 0, D), {"after_keys": (i64, (NQ,))}),
        "_rank_args_tensor": (lambda q, ranks: index._rank_args_tensor(q, ranks, D), {"ranks": (i64, (NQ, 4))}),
        "_start_tensor": (lambda q, start: index._start_tensor(start, q, "x"), {"start": (i64, (NQ,))}),
        "_filter_args": (lambda keys, exclude_pos: index._filter_args(keys, exclude_pos, 2), {"keys": (i64, (NQ, 8)), "exclude_pos": (i64, (NQ, 4))}),
    }


TENSOR_CHECKS = _tensor_checks()


def _host_tensors(name, as_ndarray):
    import torch
    _, args = TENSOR_CHECKS[name]
    made = {} if name in ("_ids_tensor", "_filter_args") else {"q": torch.zeros(NQ, D)}
    made.update({arg: torch.zeros(shape, dtype=getattr(torch, dtype)) for arg, (dtype, shape) in args.items()})
    return {arg: t.numpy() for arg, t in made.items()} if as_ndarray else made


@pytest.mark.parametrize("as_ndarray", [False, True], ids=["cpu tensor", "ndarray"])
@pytest.mark.parametrize("name", list(TENSOR_CHECKS))
def test_no_host_memory_passes_a_tensor_check(name, as_ndarray):
    """The tensor forms hand raw device pointers to kernels: a CPU tensor or an ndarray must never get there."""
    with pytest.raises(ValueError):
        TENSOR_CHECKS[name][0](**_host_tensors(name, as_ndarray))


@pytest.mark.parametrize("as_ndarray", [False, True], ids=["cpu tensor", "ndarray"])
@pytest.mark.parametrize("name, arg", [(name, arg) for name, (_, args) in TENSOR_CHECKS.items() for arg in args])
def test_every_tensor_argument_is_refused_by_name(monkeypatch, name, arg, as_ndarray):
    """... not only the first of a call: with the check of q taken out (this machine has no CUDA tensor to pass it), every
    later argument is still refused, by the one check that owns the words "must be a CUDA tensor", under its own name"""
    monkeypatch.setattr(index, "_queries_tensor", lambda q, d, what: q)
    tensors = _host_tensors(name, False)
    for other in TENSOR_CHECKS[name][1]:
        if other != arg:
            tensors[other] = _Passes(tensors[other])
    if as_ndarray:
        tensors[arg] = tensors[arg].numpy()
    shown = {"scores": "cursor scores", "rows": "cursor rows", "ref_bounds": "ids"}.get(arg, arg)
    with pytest.raises(ValueError, match=f"{shown} must be a CUDA tensor"):
        TENSOR_CHECKS[name][0](**tensors)


def _Passes(t):
    """a CPU tensor that says it is a CUDA tensor: the stand-in for the arguments that are not under test"""
    import torch

    class Passes(torch.Tensor):
        is_cuda = True
    return t.as_subclass(Passes)


def test_tensor_arg_itself():
    import torch
    for bad in (np.zeros(3, np.int64), torch.zeros(3, dtype=torch.int64), [0, 1, 2], 3, None):
        with pytest.raises(ValueError, match="call: arg must be a CUDA tensor.*\\(the hint\\)$"):
            index._tensor_arg(bad, "arg", "call", dtype="int64", hint="(the hint)")
    assert index._tensor_arg(None, "arg", "call", dtype="int64", optional=True) is None
    with pytest.raises(ValueError):
        index._tensor_arg(torch.zeros(3, dtype=torch.int64), "arg", "call", dtype="int64", optional=True)   # optional: None, nothing else


def test_null_pointers():
    """_f32p / _i64p / _devp of None: the null pointer of their type, what the C ABI reads as "argument absent" """
    import ctypes
    assert not index._f32p(None) and isinstance(index._f32p(None), ctypes.POINTER(ctypes.c_float))
    assert not index._i64p(None) and isinstance(index._i64p(None), ctypes.POINTER(ctypes.c_int64))
    assert index._devp(None).value is None
    a = np.arange(3, dtype=np.int64)
    assert index._i64p(a)[2] == 2 and ctypes.addressof(index._i64p(a).contents) == a.ctypes.data
