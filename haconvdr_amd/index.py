"""Index seam of the reference, host-side mirror.

``build_index(args)`` stands where ``build_faiss_index(args)`` does in
src/test_HAConvDR_topiocqa.py:39-71 and returns an object with the three calls
``search_one_by_one_with_faiss`` makes on it (:98 add, :102 search, :122 reset),
with the same argument meaning, result dtypes and error behaviour (exceptions
propagate).  All arithmetic runs in the gfx950 HIP kernels of libhaconvdr.so.
"""
import ctypes

import numpy as np

from . import _lib


def _stream_ptr(stream):
    if stream is None:
        import torch
        stream = torch.cuda.current_stream()
    return ctypes.c_void_p(getattr(stream, "cuda_stream", stream))


def _keep_alive(stream, *tensors):
    """The kernels read the tensors asynchronously on ``stream`` (a torch stream, a raw hipStream_t or None = the
    current stream): tell the caching allocator, or it may hand the memory out again too early."""
    import torch
    if stream is None:
        stream = torch.cuda.current_stream()
    elif not hasattr(stream, "cuda_stream"):
        stream = torch.cuda.ExternalStream(int(stream))
    for t in tensors:
        t.record_stream(stream)


def _on_stream(stream):
    """Context in which torch's own kernels run on ``stream`` (a torch stream, a raw hipStream_t or None = the current stream)."""
    import contextlib
    import torch
    if stream is None:
        return contextlib.nullcontext()
    return torch.cuda.stream(stream if hasattr(stream, "cuda_stream") else torch.cuda.ExternalStream(int(stream)))


# ---- the pointers the C ABI takes: of a float32 / int64 ndarray, of a CUDA tensor (None: null)
def _f32p(a):
    return ctypes.POINTER(ctypes.c_float)() if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _i64p(a):
    return ctypes.POINTER(ctypes.c_int64)() if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def _devp(t):
    return ctypes.c_void_p() if t is None else ctypes.c_void_p(t.data_ptr())


def _host_results(shape):
    """(D float32, I int64) of a host search"""
    return np.empty(shape, np.float32), np.empty(shape, np.int64)


def _device_results(shape, device):
    import torch
    return torch.empty(shape, dtype=torch.float32, device=device), torch.empty(shape, dtype=torch.int64, device=device)


def _device_i64(shape, device):
    """the int64 CUDA tensor a call fills: packed keys [.., k], ranks, counts, labels, lims"""
    import torch
    return torch.empty(shape, dtype=torch.int64, device=device)


# ---- argument checks: no handle needed, a mistake raises ValueError before the library is called.  Two primitives, one per
# form -- _int_array for what the host calls take, _tensor_arg for what the tensor calls take -- and the per-call checks below,
# which compose them.  A message names the call (`what`) and the argument and says what it got.
def _check_shape(got, name, what, ndim, shape, hint):
    """shape: the wanted shape, None = any length; or ndim: the wanted rank."""
    got = tuple(got)
    if shape is not None:
        if len(got) != len(shape) or any(w is not None and w != g for w, g in zip(shape, got)):
            want = ", ".join("*" if w is None else str(w) for w in shape)
            raise ValueError(f"{what}: {name} must have shape [{want}], got {got} {hint}".rstrip())
    elif ndim is not None and len(got) != ndim:
        raise ValueError(f"{what}: {name} must have {ndim} dimension(s), got shape {got} {hint}".rstrip())


def _int_array(a, name, what, *, ndim=None, shape=None, hint=""):
    """a -> contiguous int64 ndarray of the wanted rank or shape; integers only (a float id is a mistake, not a row), and
    a uint64 only where int64 holds its values."""
    a = np.asarray(a)
    if a.dtype.kind not in "iu":
        raise ValueError(f"{what}: {name} must be integers, got dtype {a.dtype}")
    _check_shape(a.shape, name, what, ndim, shape, hint)
    if a.dtype == np.uint64 and a.size and int(a.max()) > np.iinfo(np.int64).max:
        raise ValueError(f"{what}: {name}: {int(a.max())} does not fit int64")
    return np.ascontiguousarray(a, dtype=np.int64)


def _tensor_arg(t, name, what, *, dtype, ndim=None, shape=None, like=None, optional=False, hint=""):
    """t -> t.contiguous() (t itself where it is contiguous: no allocation inside a capture), after the checks every tensor
    form owes the kernels, which get a raw device pointer: a CUDA tensor, of torch's dtype named `dtype` (None: any), of the
    wanted rank or shape, on the device of `like`.  optional: None passes through."""
    import torch
    if t is None and optional:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        got = f"a tensor on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{what}: {name} must be a CUDA tensor, got {got} {hint}".rstrip())
    if dtype is not None and t.dtype != getattr(torch, dtype):
        raise ValueError(f"{what}: {name} must be {dtype}, got {t.dtype} {hint}".rstrip())
    _check_shape(t.shape, name, what, ndim, shape, hint)
    if like is not None and t.device != like.device:
        raise ValueError(f"{what}: {name} on {t.device} but the tensor it goes with (q, or the keys) on {like.device}")
    return t.contiguous()


def _as_ids(ids, ndim, what):
    return _int_array(ids, "ids", what, ndim=ndim)


def _remove_args(ids, ntotal, what="remove_ids"):
    """ids of remove_ids -> contiguous int64 [n]: an integer array of one dimension (-1 = padding, duplicates allowed), or a
    boolean mask of shape [ntotal] (True = the row goes), which becomes its indices."""
    a = np.asarray(ids)
    if a.dtype == np.bool_:
        if a.shape != (ntotal,):
            raise ValueError(f"{what}: a mask must have shape ({ntotal},), one entry per row, got {a.shape}")
        return np.flatnonzero(a).astype(np.int64)
    return _as_ids(a, 1, what)


def _as_range(i0, n, what):
    """(i0, n) of reconstruct_n as python ints; n may be None (= up to ntotal, resolved by the caller)."""
    for name, v in (("i0", i0), ("n", n)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer))):
            raise ValueError(f"{what}: {name} must be an integer, got {v!r}")
    return int(i0), (None if n is None else int(n))


def _as_queries(q, d, what):
    a = np.asarray(q)
    if a.dtype.kind not in "fiu" or a.ndim != 2 or a.shape[1] != d:
        raise ValueError(f"{what} expects [nq, {d}] float32, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a, dtype=np.float32)


def _pair_args(q, ids, d, what):
    """(q float32 [nq, d], ids int64 [nq, m]) of score_ids / rank_ids."""
    q = _as_queries(q, d, what)
    return q, _int_array(ids, "ids", what, shape=(q.shape[0], None), hint="(one list per query)")


def _as_k(k, what):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= _lib.HAC_MAX_K:
        raise ValueError(f"{what}: k must be an integer in [1, {_lib.HAC_MAX_K}], got {k!r}")
    return int(k)


def _ids_tensor(ids, ndim, what):
    return _tensor_arg(ids, "ids", what, dtype="int64", ndim=ndim)


def _queries_tensor(q, d, what):
    q = _tensor_arg(q, "q", what, dtype=None)
    if not q.dtype.is_floating_point or q.dim() != 2 or q.shape[1] != d:
        raise ValueError(f"{what} expects [nq, {d}] float32, got {q.dtype} {tuple(q.shape)}")
    return q.float()


def _check_id_map_tensor(id_map, q, what):
    return _tensor_arg(id_map, "id_map", what, dtype="int64", ndim=1, like=q, optional=True, hint="(int64 CUDA [ntotal], or None)")


def _pair_args_tensor(q, ids, d, what):
    """(q float32 CUDA [nq, d], ids int64 CUDA [nq, m]) of score_ids_tensor / rank_ids_tensor / count_ahead_tensor."""
    q = _queries_tensor(q, d, what)
    return q, _tensor_arg(ids, "ids", what, dtype="int64", shape=(q.shape[0], None), like=q, hint="(one list per query)")


def _count_args_tensor(q, ref_scores, ref_bounds, d, what="count_ahead_tensor"):
    """(q float32 CUDA [nq, d], ref_scores float32 CUDA [nq, m], ref_bounds int64 CUDA [nq, m]) of count_ahead_tensor."""
    q, ref_bounds = _pair_args_tensor(q, ref_bounds, d, what)
    ref_scores = _tensor_arg(ref_scores, "ref_scores", what, dtype="float32", shape=tuple(ref_bounds.shape), like=q,
                             hint="(the bits a search returns, one per entry of ref_bounds)")
    return q, ref_scores, ref_bounds


def _as_radius(radius, nq, what):
    """radius of range_search -> contiguous float32 [nq]: a real scalar (faiss's form, one radius for every query) or one
    value per query.  float64 values are rounded to float32, the precision the scores are compared in."""
    a = np.asarray(radius)
    if a.dtype.kind not in "fiu":
        raise ValueError(f"{what}: radius must be real numbers, got dtype {a.dtype}")
    if a.ndim == 0:
        return np.full(nq, a, dtype=np.float32)
    if a.shape != (nq,):
        raise ValueError(f"{what}: {nq} queries but radius of shape {a.shape} (a scalar, or one per query)")
    return np.ascontiguousarray(a, dtype=np.float32)


def _as_cap(cap, what):
    if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or int(cap) < 0:
        raise ValueError(f"{what}: cap must be an integer >= 0 (results), got {cap!r}")
    return int(cap)


def _range_args(q, radius, d, what="range_search"):
    """(q float32 [nq, d], radius float32 [nq]) of range_search / range_count."""
    q = _as_queries(q, d, what)
    return q, _as_radius(radius, q.shape[0], what)


def _range_args_tensor(q, radius, cap, id_map, d, what="range_search_tensor"):
    """(q float32 CUDA [nq, d], radius float32 CUDA [nq], cap, id_map int64 CUDA [ntotal] or None) of range_search_tensor."""
    q = _queries_tensor(q, d, what)
    radius = _tensor_arg(radius, "radius", what, dtype="float32", shape=(q.shape[0],), like=q,
                         hint="(one per query, in the precision the scores are compared in)")
    return q, radius, _as_cap(cap, what), _check_id_map_tensor(id_map, q, what)


def _check_exclude_shape(nq, k, shape, what):
    if shape[0] != nq:
        raise ValueError(f"{what}: {nq} queries but exclude of shape {tuple(shape)} (one list per query)")
    if k + shape[1] > _lib.HAC_MAX_K:
        raise ValueError(f"{what}: k + e = {k} + {shape[1]} exceeds {_lib.HAC_MAX_K} (the search runs at k + e)")


def _exclude_args(q, k, exclude, d, what="search_excluding"):
    """(q float32 [nq, d], k, exclude int64 [nq, e]) of search_excluding."""
    q = _as_queries(q, d, what)
    k = _as_k(k, what)
    exclude = _int_array(exclude, "exclude", what, ndim=2)
    _check_exclude_shape(q.shape[0], k, exclude.shape, what)
    return q, k, exclude


def _exclude_args_tensor(q, k, exclude, d, what="search_excluding_tensor"):
    q = _queries_tensor(q, d, what)
    k = _as_k(k, what)
    exclude = _tensor_arg(exclude, "exclude", what, dtype="int64", ndim=2, like=q)
    _check_exclude_shape(q.shape[0], k, exclude.shape, what)
    return q, k, exclude


def _check_among_shape(nq, shape, what):
    if shape[0] != nq:
        raise ValueError(f"{what}: {nq} queries but cand of shape {tuple(shape)} (one list per query)")
    if shape[1] > _lib.HAC_MAX_AMONG:
        raise ValueError(f"{what}: m = {shape[1]} candidates per query exceed {_lib.HAC_MAX_AMONG} (one LDS sort block)")


def _among_args(q, k, cand, d, what="search_among"):
    """(q float32 [nq, d], k, cand int64 [nq, m]) of search_among."""
    q = _as_queries(q, d, what)
    k = _as_k(k, what)
    cand = _int_array(cand, "cand", what, ndim=2)
    _check_among_shape(q.shape[0], cand.shape, what)
    return q, k, cand


def _among_args_tensor(q, k, cand, id_map, d, what="search_among_tensor"):
    """(q float32 CUDA [nq, d], k, cand int64 CUDA [nq, m], id_map int64 CUDA [ntotal] or None) of search_among*_tensor."""
    q = _queries_tensor(q, d, what)
    k = _as_k(k, what)
    cand = _tensor_arg(cand, "cand", what, dtype="int64", ndim=2, like=q)
    _check_among_shape(q.shape[0], cand.shape, what)
    return q, k, cand, _check_id_map_tensor(id_map, q, what)


# ---- bitmaps of search_masked (include/haconvdr.h, "search inside a bitmap"): row r is bit r & 63 of word r >> 6
def mask_words(ntotal):
    """words per mask of an index of ntotal rows"""
    return (int(ntotal) + 63) // 64


def pack_mask(mask):
    """bool [ntotal] or [n_masks, ntotal] (ndarray or CUDA tensor) -> the packed words as int64 [W] or [n_masks, W], W =
    ceil(ntotal / 64), of the same kind; int64 is the view torch can hold: a word with bit 63 set is negative.  The bytes are
    np.packbits(mask, bitorder="little"), faiss's IDSelectorBitmap bitmap, zero padded to whole words."""
    if isinstance(mask, np.ndarray) or not hasattr(mask, "is_cuda"):
        a = np.asarray(mask)
        if a.dtype != np.bool_ or a.ndim not in (1, 2):
            raise ValueError(f"pack_mask: needs bool [ntotal] or [n_masks, ntotal], got {a.dtype} {a.shape}")
        W = mask_words(a.shape[-1])
        padded = np.zeros(a.shape[:-1] + (W * 64,), np.bool_)
        padded[..., :a.shape[-1]] = a
        return np.packbits(padded, axis=-1, bitorder="little").view("<u8").view(np.int64).reshape(a.shape[:-1] + (W,))
    import torch
    if mask.dtype != torch.bool or mask.dim() not in (1, 2):
        raise ValueError(f"pack_mask: needs bool [ntotal] or [n_masks, ntotal], got {mask.dtype} {tuple(mask.shape)}")
    n = mask.shape[-1]
    W = mask_words(n)
    padded = torch.zeros(tuple(mask.shape[:-1]) + (W * 64,), dtype=torch.int64, device=mask.device)
    padded[..., :n] = mask
    # bit b of a word: the sum of distinct powers of two cannot carry; 1 << 63 wraps to the sign bit, as the word wants
    weights = torch.ones(64, dtype=torch.int64, device=mask.device) << torch.arange(64, dtype=torch.int64, device=mask.device)
    return (padded.reshape(tuple(mask.shape[:-1]) + (W, 64)) * weights).sum(dim=-1)


def unpack_mask(words, ntotal):
    """pack_mask's inverse: int64 / uint64 words [W] or [n_masks, W] (ndarray or tensor) -> bool [ntotal] or [n_masks, ntotal]
    ndarray; bits at or above ntotal are dropped."""
    a = words.cpu().numpy() if hasattr(words, "is_cuda") else np.asarray(words)
    if a.dtype not in (np.int64, np.uint64) or a.ndim not in (1, 2) or a.shape[-1] != mask_words(ntotal):
        raise ValueError(f"unpack_mask: needs int64 / uint64 [.., {mask_words(ntotal)}] for {ntotal} rows, got {a.dtype} {a.shape}")
    b = np.ascontiguousarray(a).view(np.uint64).astype("<u8").view(np.uint8)
    return np.unpackbits(b, axis=-1, bitorder="little")[..., :int(ntotal)].astype(np.bool_)


def range_mask(ntotal, lo, hi):
    """The packed mask int64 [W] of the rows [lo, hi) (clipped to [0, ntotal)): faiss's IDSelectorRange."""
    for name, v in (("ntotal", ntotal), ("lo", lo), ("hi", hi)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"range_mask: {name} must be an integer, got {v!r}")
    if ntotal < 0:
        raise ValueError(f"range_mask: ntotal = {ntotal} is negative")
    m = np.zeros(int(ntotal), np.bool_)
    m[max(0, int(lo)):max(0, int(hi))] = True
    return pack_mask(m)


def _check_mask_of(mask_of_shape, n_masks, nq, what):
    if mask_of_shape is None:
        if n_masks != 1 and n_masks != nq:
            raise ValueError(f"{what}: {n_masks} masks for {nq} queries and no mask_of: needs one mask, one per query, or mask_of")
    elif tuple(mask_of_shape) != (nq,):
        raise ValueError(f"{what}: {nq} queries but mask_of of shape {tuple(mask_of_shape)} (one entry per query)")


def _as_masks(masks, mask_of, nq, ntotal, what):
    """(words int64 [n_masks, W], mask_of int64 [nq] or None) of nq queries over ntotal rows.  masks: bool [ntotal] or
    [n_masks, ntotal], or packed uint64 / int64 [W] or [n_masks, W]."""
    a = np.asarray(masks)
    if a.ndim not in (1, 2):
        raise ValueError(f"{what}: masks must have 1 or 2 dimensions, got shape {a.shape}")
    if a.dtype == np.bool_:
        if a.shape[-1] != ntotal:
            raise ValueError(f"{what}: a bool mask needs one entry per row, {ntotal}, got shape {a.shape}")
        a = pack_mask(a)
    elif a.dtype in (np.int64, np.uint64):
        if a.shape[-1] != mask_words(ntotal):
            raise ValueError(f"{what}: packed masks need {mask_words(ntotal)} words for {ntotal} rows, got shape {a.shape} "
                             "(packed before an add or a remove?)")
    else:
        raise ValueError(f"{what}: masks must be bool, or packed uint64 / int64 words, got dtype {a.dtype}")
    a = np.ascontiguousarray(a.reshape((a.shape[0] if a.ndim == 2 else 1, a.shape[-1]))).view(np.int64)
    if a.shape[0] < 1:
        raise ValueError(f"{what}: needs at least one mask")
    if mask_of is not None:
        mask_of = _int_array(mask_of, "mask_of", what, ndim=1)   # (its values: the library refuses one outside [0, n_masks), as it refuses ids)
    _check_mask_of(None if mask_of is None else mask_of.shape, a.shape[0], nq, what)
    return a, mask_of


def _masked_args(q, k, masks, mask_of, d, ntotal, what="search_masked"):
    """(q float32 [nq, d], k, words int64 [n_masks, W], mask_of int64 [nq] or None) of search_masked."""
    q = _as_queries(q, d, what)
    k = _as_k(k, what)
    words, mask_of = _as_masks(masks, mask_of, q.shape[0], ntotal, what)
    return q, k, words, mask_of


def _masked_args_tensor(q, k, masks, mask_of, id_map, d, ntotal, what="search_masked_tensor"):
    """(q float32 CUDA [nq, d], k, masks int64 CUDA [n_masks, W], mask_of int64 CUDA [nq] or None, id_map) of search_masked*_tensor."""
    q = _queries_tensor(q, d, what)
    k = _as_k(k, what)
    masks = _tensor_arg(masks, "masks", what, dtype="int64", shape=(None, mask_words(ntotal)), like=q,
                        hint=f"(pack_mask of a bool tensor: packed words [n_masks >= 1, W] for {ntotal} rows; packed before an add or a remove?)")
    if masks.shape[0] < 1:
        raise ValueError(f"{what}: needs at least one mask")
    mask_of = _tensor_arg(mask_of, "mask_of", what, dtype="int64", like=q, optional=True)
    _check_mask_of(None if mask_of is None else mask_of.shape, masks.shape[0], q.shape[0], what)
    return q, k, masks, mask_of, _check_id_map_tensor(id_map, q, what)


# ---- labels of search_grouped (include/haconvdr.h, "search by group"): one int64 label in [0, 2^32) per row
_LABELS_HINT = "(one label per row of the index; labels made before an add or a remove?)"


def _grouped_args(q, k, group_of, d, ntotal, what="search_grouped"):
    """(q float32 [nq, d], k, group_of int64 [ntotal]) of search_grouped.  The values are the library's to check: it names the
    first row whose label lies outside [0, 2^32)."""
    q = _as_queries(q, d, what)
    k = _as_k(k, what)
    return q, k, _int_array(group_of, "group_of", what, shape=(ntotal,), hint=_LABELS_HINT)


def _grouped_args_tensor(q, k, group_of, id_map, d, ntotal, what="search_grouped_tensor"):
    """(q float32 CUDA [nq, d], k, group_of int64 CUDA [ntotal], id_map int64 CUDA [ntotal] or None) of search_grouped_tensor."""
    q = _queries_tensor(q, d, what)
    k = _as_k(k, what)
    group_of = _tensor_arg(group_of, "group_of", what, dtype="int64", shape=(ntotal,), like=q, hint=_LABELS_HINT)
    return q, k, group_of, _check_id_map_tensor(id_map, q, what)


# ---- cursors of search_after (include/haconvdr.h, "search behind a cursor"): a (score, row) pair per query, or a packed key
AFTER_START = _lib.HAC_AFTER_START   # the cursor row that starts a query from the start


def cursor_keys(scores, rows, pos_base=0):
    """(scores float32 [..], rows int64 [..]) cursors -> their packed keys as int64 (the view of uint64 torch can hold) of the
    same shape and kind (ndarray or CUDA tensor), in the position space of pos_base: search_after_keys_tensor's after_keys.  The
    rule of after_bounds_kernel: a NaN score, row -1 (a padding slot) and a row below -2 give 0, the exhausted list; row
    AFTER_START gives all-ones, the start; otherwise ord(score + 0.0) << 32 | 2^32 - 1 - min(pos_base + row, 2^32 - 1)."""
    pos_base = _as_pos_base(pos_base, "cursor_keys")
    if hasattr(scores, "is_cuda") or hasattr(rows, "is_cuda"):
        import torch
        if not (isinstance(scores, torch.Tensor) and isinstance(rows, torch.Tensor)) or scores.device != rows.device:
            raise ValueError("cursor_keys: scores and rows must be tensors on one device (or both ndarrays)")
        if scores.dtype != torch.float32 or rows.dtype != torch.int64 or tuple(scores.shape) != tuple(rows.shape):
            raise ValueError(f"cursor_keys: needs float32 scores and int64 rows of one shape, got {scores.dtype} {tuple(scores.shape)} "
                             f"and {rows.dtype} {tuple(rows.shape)}")
        s = scores.contiguous() + 0.0                                          # -0.0 -> +0.0
        b = s.view(torch.int32).to(torch.int64)                               # the bits, sign-extended
        hi = torch.where(b < 0, ~b, b - 0x80000000)                           # ord(score) as a SIGNED 32-bit value: hi << 32 stays inside int64
        pos = torch.clamp(torch.clamp(rows, min=0) + pos_base, max=0xFFFFFFFF)    # (rows up to 2^63 - 1: clamp first)
        pos = torch.where(rows >= 0xFFFFFFFF, torch.full_like(rows, 0xFFFFFFFF), pos)
        keys = hi * (1 << 32) + (0xFFFFFFFF - pos)
        keys = torch.where((rows < 0) | torch.isnan(s), torch.zeros_like(keys), keys)
        return torch.where(rows == AFTER_START, torch.full_like(keys, -1), keys)
    s = np.asarray(scores)
    r = np.asarray(rows)
    if s.dtype != np.float32 or r.dtype.kind not in "iu" or s.shape != r.shape:
        raise ValueError(f"cursor_keys: needs float32 scores and integer rows of one shape, got {s.dtype} {s.shape} and {r.dtype} {r.shape}")
    r = r.astype(np.int64)
    s = (s + np.float32(0.0)).astype(np.float32)                              # -0.0 -> +0.0
    b = np.ascontiguousarray(s).view(np.uint32)
    ord_ = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint64)
    pos = np.where(r >= 0xFFFFFFFF, 0xFFFFFFFF, np.minimum(np.maximum(r, 0) + pos_base, 0xFFFFFFFF)).astype(np.uint64)
    keys = (ord_ << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - pos)
    keys = np.where((r < 0) | np.isnan(s), np.uint64(0), keys)
    keys = np.where(r == AFTER_START, np.uint64(0xFFFFFFFFFFFFFFFF), keys)
    return keys.astype(np.uint64).view(np.int64)


_CURSOR_HINT = "(one per query; the scores are the bits a search returns)"


def _cursor(after, nq, what):
    """after of search_after / search_masked(after=) -> (scores float32 [nq], rows int64 [nq]), or (None, None) for None."""
    if after is None:
        return None, None
    if not isinstance(after, (tuple, list)) or len(after) != 2:
        raise ValueError(f"{what}: after must be None or a pair (scores [nq], rows [nq])")
    scores = np.asarray(after[0])
    if scores.dtype != np.float32 or scores.shape != (nq,):
        raise ValueError(f"{what}: cursor scores must be float32 [{nq}], got {scores.dtype} {scores.shape} {_CURSOR_HINT}")
    rows = _int_array(after[1], "cursor rows", what, shape=(nq,), hint=_CURSOR_HINT)
    if rows.size and int(rows.min()) < AFTER_START:
        at = int(np.flatnonzero(rows < AFTER_START)[0])
        raise ValueError(f"{what}: cursor row {int(rows[at])} of query {at} is below {AFTER_START} (a row, -1 = an exhausted list, "
                         f"{AFTER_START} = the start)")
    return np.ascontiguousarray(scores), rows


def _cursor_tensor(after, q, what):
    """after of search_after_tensor / search_masked_tensor(after=) -> (scores float32 CUDA [nq], rows int64 CUDA [nq]), or
    (None, None) for None.  The rows' values are the device's to read: one below -2 gives that query an empty list."""
    if after is None:
        return None, None
    if not isinstance(after, (tuple, list)) or len(after) != 2:
        raise ValueError(f"{what}: after must be None or a pair (scores [nq], rows [nq])")
    return (_tensor_arg(after[0], "cursor scores", what, dtype="float32", shape=(q.shape[0],), like=q, hint=_CURSOR_HINT),
            _tensor_arg(after[1], "cursor rows", what, dtype="int64", shape=(q.shape[0],), like=q, hint=_CURSOR_HINT))


def _cursor_keys_tensor(after_keys, q, what):
    """after_keys of search_after_keys_tensor / search_masked_keys_tensor(after_keys=) -> int64 CUDA [nq], or None."""
    return _tensor_arg(after_keys, "after_keys", what, dtype="int64", shape=(q.shape[0],), like=q, optional=True,
                       hint="(one per query: cursor_keys, or the last column of a key list, the int64 view of the packed uint64 keys)")


def _after_args(q, k, after, d, what="search_after"):
    """(q float32 [nq, d], k, scores float32 [nq] or None, rows int64 [nq] or None) of search_after; after: None (every query
    from the start) or a pair (scores [nq] float32 -- the bits a search returned --, rows [nq] integers >= -2)."""
    q = _as_queries(q, d, what)
    return (q, _as_k(k, what), *_cursor(after, q.shape[0], what))


def _after_args_tensor(q, k, after, id_map, d, what="search_after_tensor"):
    """(q float32 CUDA [nq, d], k, scores float32 CUDA [nq] or None, rows int64 CUDA [nq] or None, id_map) of
    search_after_tensor."""
    q = _queries_tensor(q, d, what)
    k = _as_k(k, what)
    id_map = _check_id_map_tensor(id_map, q, what)
    return (q, k, *_cursor_tensor(after, q, what), id_map)


def _as_pos_base(pos_base, what):
    if isinstance(pos_base, bool) or not isinstance(pos_base, (int, np.integer)) or not 0 <= int(pos_base) <= 0xFFFFFFFF:
        raise ValueError(f"{what}: pos_base must be an integer in [0, 2^32), got {pos_base!r}")
    return int(pos_base)


def _after_keys_args_tensor(q, k, after_keys, pos_base, d, what="search_after_keys_tensor"):
    """(q float32 CUDA [nq, d], k, after_keys int64 CUDA [nq] or None, pos_base) of search_after_keys_tensor."""
    q = _queries_tensor(q, d, what)
    k = _as_k(k, what)
    pos_base = _as_pos_base(pos_base, what)
    return q, k, _cursor_keys_tensor(after_keys, q, what), pos_base


# ---- ranks of entries_at / search_at (include/haconvdr.h, "entry at a rank"): values, not ids -- any integer is allowed
def _rank_args(q, ranks, d, what="entries_at"):
    """(q float32 [nq, d], ranks int64 [nq, m]) of entries_at."""
    q = _as_queries(q, d, what)
    return q, _int_array(ranks, "ranks", what, shape=(q.shape[0], None), hint="(one list per query)")


def _rank_args_tensor(q, ranks, d, what="entries_at_tensor"):
    """(q float32 CUDA [nq, d], ranks int64 CUDA [nq, m]) of entries_at_tensor / entry_keys_at_tensor."""
    q = _queries_tensor(q, d, what)
    return q, _tensor_arg(ranks, "ranks", what, dtype="int64", shape=(q.shape[0], None), like=q, hint="(one list per query)")


def _as_start(start, nq, what):
    """start of search_at -> contiguous int64 [nq]: an integer (one start for every query) or one per query, all >= 0."""
    if isinstance(start, bool):
        raise ValueError(f"{what}: start must be an integer or int64 [nq], got {start!r}")
    a = np.asarray(start)
    if a.ndim == 0 and a.dtype.kind in "iu":
        a = np.full(nq, a)
    a = _int_array(a, "start", what, shape=(nq,), hint="(an integer, or one per query)")
    if a.size and int(a.min()) < 0:
        at = int(np.flatnonzero(a < 0)[0])
        raise ValueError(f"{what}: start {int(a[at])} of query {at} is negative (a rank of the unbounded search, >= 0)")
    return a


def _start_tensor(start, q, what):
    """start of search_at*_tensor -> int64 CUDA [nq]: an integer >= 0, or an int64 CUDA tensor [nq] on q's device (its values
    are the device's to read: a negative one gives that query an empty list)."""
    import torch
    nq = q.shape[0]
    if isinstance(start, bool) or not isinstance(start, (int, np.integer)):
        return _tensor_arg(start, "start", what, dtype="int64", shape=(nq,), like=q, hint="(an integer >= 0, or an int64 CUDA tensor [nq])")
    if int(start) < 0:
        raise ValueError(f"{what}: start must be an integer >= 0 or an int64 CUDA tensor [nq], got {start!r}")
    return torch.full((nq,), int(start), dtype=torch.int64, device=q.device)


def _filter_args(keys, exclude_pos, k, what="filter_keys"):
    """(keys int64 CUDA [nq, kin], exclude_pos int64 CUDA [nq, e], k in [1, kin]) of filter_keys."""
    keys = _tensor_arg(keys, "keys", what, dtype="int64", ndim=2)
    exclude_pos = _tensor_arg(exclude_pos, "exclude_pos", what, dtype="int64", ndim=2, like=keys)
    k = _as_k(k, what)
    if keys.shape[1] > _lib.HAC_MAX_K or k > keys.shape[1]:
        raise ValueError(f"{what}: needs k = {k} <= kin = {keys.shape[1]} <= {_lib.HAC_MAX_K}")
    if exclude_pos.shape[0] != keys.shape[0] or exclude_pos.shape[1] >= _lib.HAC_MAX_K:
        raise ValueError(f"{what}: keys of shape {tuple(keys.shape)} but exclude_pos of shape {tuple(exclude_pos.shape)} "
                         f"(one list of fewer than {_lib.HAC_MAX_K} positions per query)")
    return keys, exclude_pos, k


class FlatIPIndex:
    """faiss.IndexFlatIP(d) drop-in: exact fp32 inner product, results ordered by
    (score desc, row asc), padded with -FLT_MAX / -1.

    devices: HIP ordinals.  One device is the normal case (one process per GPU);
    several reproduce faiss's in-process ``shard=True`` clone (:55-66)."""

    def __init__(self, d=768, devices=(0,)):
        self.d = int(d)
        self.devices = tuple(int(x) for x in devices)
        self._h = ctypes.c_void_p()
        arr = (ctypes.c_int * len(self.devices))(*self.devices)
        _lib.check(_lib.lib().hac_index_create(self.d, arr, len(self.devices), ctypes.byref(self._h)))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                _lib.lib().hac_index_destroy(h)
            except Exception:
                pass

    # ---- the three calls of the reference ---------------------------------
    def add(self, x):
        """index.add(passage_embedding): float32 [n, d]; copied before return."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.d:
            raise ValueError(f"add expects [n, {self.d}] float32, got {x.shape}")
        _lib.check(_lib.lib().hac_index_add(self._h, _f32p(x), x.shape[0]))

    def search(self, q, k):
        """D, I = index.search(query_embeddings, topN) -> float32 [nq,k], int64 [nq,k]."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.d:
            raise ValueError(f"search expects [nq, {self.d}] float32, got {q.shape}")
        k = int(k)
        D, I = _host_results((q.shape[0], k))
        _lib.check(_lib.lib().hac_index_search(self._h, _f32p(q), q.shape[0], k, _f32p(D), _i64p(I)))
        return D, I

    def search_excluding(self, q, k, exclude):
        """search(q, k) over (rows minus the query's excluded rows): exclude int64 [nq, e] row ids, -1 = padding, duplicates
        allowed; any other id outside [0, ntotal) raises HacError.  The search runs at k + e <= HAC_MAX_K (include/haconvdr.h);
        faiss: SearchParameters(sel=IDSelectorNot(IDSelectorBatch(ids))), one selector per query."""
        q, k, exclude = _exclude_args(q, k, exclude, self.d)
        D, I = _host_results((q.shape[0], k))
        _lib.check(_lib.lib().hac_index_search_excluding(self._h, _f32p(q), q.shape[0], k, _i64p(exclude), exclude.shape[1], _f32p(D), _i64p(I)))
        return D, I

    def search_among(self, q, k, cand):
        """search(q, k) over the query's candidate rows only: cand int64 [nq, m] row ids, a set (a row named twice appears once),
        -1 = padding anywhere in the list; any other id outside [0, ntotal) raises HacError.  m <= HAC_MAX_AMONG; k may exceed m
        (the tail is padding).  Rows whose score is NaN are in no list (include/haconvdr.h, "search among named rows");
        faiss: SearchParameters(sel=IDSelectorBatch(ids)), one selector per query."""
        q, k, cand = _among_args(q, k, cand, self.d)
        D, I = _host_results((q.shape[0], k))
        _lib.check(_lib.lib().hac_index_search_among(self._h, _f32p(q), q.shape[0], k, _i64p(cand), cand.shape[1], _f32p(D), _i64p(I)))
        return D, I

    def search_masked(self, q, k, masks, mask_of=None, after=None):
        """search(q, k) over the rows a bitmap selects: masks bool [ntotal] or [n_masks, ntotal], or packed uint64 / int64
        [W] or [n_masks, W] (pack_mask; W = ceil(ntotal / 64)); mask_of int64 [nq] names each query's mask and may be None with
        one mask (every query uses it) or nq masks (query i uses mask i); an entry outside [0, n_masks) raises HacError.  Rows
        whose score is NaN are in no list; k may exceed the selected rows (the tail is padding).  Any number of rows may be
        selected (include/haconvdr.h, "search inside a bitmap"); faiss: SearchParameters(sel=IDSelectorBitmap(n, bitmap)),
        IDSelectorRange (range_mask), IDSelectorNot (~mask).
        after: None, or search_after's cursor pair (scores float32 [nq], rows int64 [nq]): the next page of the SELECTED rows,
        those behind each query's cursor, e.g. (D[:, -1], I[:, -1]) of the page before under the same masks.  The cursor row need
        not be selected and need not exist; row -1 gives padding, AFTER_START the start, a row below -2 raises ValueError
        (include/haconvdr.h, "search inside a bitmap, behind a cursor")."""
        q, k, words, mask_of = _masked_args(q, k, masks, mask_of, self.d, self.ntotal)
        scores, rows = _cursor(after, q.shape[0], "search_masked")
        D, I = _host_results((q.shape[0], k))
        head = (self._h, _f32p(q), q.shape[0], k, words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), words.shape[0], words.shape[1], _i64p(mask_of))
        if after is None:
            _lib.check(_lib.lib().hac_index_search_masked(*head, _f32p(D), _i64p(I)))
        else:
            _lib.check(_lib.lib().hac_index_search_masked_after(*head, _f32p(scores), _i64p(rows), _f32p(D), _i64p(I)))
        return D, I

    def search_grouped(self, q, k, group_of, return_groups=False):
        """The k best GROUPS of rows per query, each by its best row: group_of int64 [ntotal] labels in [0, 2^32), one per row
        (a label outside that range raises HacError naming the row).  -> (D, I), the score and row of each group's
        representative ordered by (score desc, row asc), padded with -FLT_MAX / -1 when fewer than k labels occur; with
        return_groups also G = group_of[I] (-1 in padding).  Exact however many rows a group has (include/haconvdr.h,
        "search by group"); the labels are uploaded on every call.  faiss: grouped search (IDGrouper)."""
        q, k, group_of = _grouped_args(q, k, group_of, self.d, self.ntotal)
        D, I = _host_results((q.shape[0], k))
        G = np.empty((q.shape[0], k), np.int64) if return_groups else None
        _lib.check(_lib.lib().hac_index_search_grouped(self._h, _f32p(q), q.shape[0], k, _i64p(group_of), group_of.shape[0], _f32p(D), _i64p(I), _i64p(G)))
        return (D, I, G) if return_groups else (D, I)

    def search_after(self, q, k, after=None):
        """The next page: search(q, k) over the rows BEHIND each query's cursor in the order (score desc, row asc).  after: None
        (every query from the start: search(q, k)) or a pair (scores float32 [nq], rows int64 [nq]), e.g. (D[:, -1], I[:, -1])
        of the page before.  Row r is listed iff its score is not NaN and lies below the cursor's, or equals it with r > the
        cursor row; the cursor row need not exist.  Row -1 (a padding slot: the list had ended) and a NaN score give an empty
        list, row AFTER_START the start; a row below -2 raises ValueError.  No ceiling at HAC_MAX_K on the depth, and a page
        costs the same at any depth (include/haconvdr.h, "search behind a cursor")."""
        q, k, scores, rows = _after_args(q, k, after, self.d)
        D, I = _host_results((q.shape[0], k))
        _lib.check(_lib.lib().hac_index_search_after(self._h, _f32p(q), q.shape[0], k, _f32p(scores), _i64p(rows), _f32p(D), _i64p(I)))
        return D, I

    def reset(self):
        _lib.check(_lib.lib().hac_index_reset(self._h))

    def remove_ids(self, ids):
        """index.remove_ids(ids) -> the number of rows removed.  ids: int64 [n] row ids (-1 = padding, duplicates allowed; any
        other id outside [0, ntotal) raises HacError and changes nothing) or a boolean mask [ntotal].  The surviving rows keep
        their bits and order and are renumbered densely from 0 (row j of np.delete(x, ids, axis=0)); in place on the device,
        synchronous (include/haconvdr.h, "removing rows")."""
        ids = _remove_args(ids, self.ntotal)
        removed = ctypes.c_int64(0)
        _lib.check(_lib.lib().hac_index_remove_ids(self._h, _i64p(ids), ids.shape[0], ctypes.byref(removed)))
        return int(removed.value)

    @property
    def ntotal(self):
        return int(_lib.lib().hac_index_ntotal(self._h))

    # ---- the faiss read-back calls and exact scores of named rows (include/haconvdr.h, "rows by id") -------------
    def reconstruct_n(self, i0=0, n=None):
        """index.reconstruct_n(i0, n) -> float32 [n, d], the rows as they were added, bit for bit (n=None: up to ntotal)."""
        i0, n = _as_range(i0, n, "reconstruct_n")
        if n is None:
            n = self.ntotal - i0
        out = np.empty((max(n, 0), self.d), np.float32)
        _lib.check(_lib.lib().hac_index_reconstruct(self._h, i0, n, _f32p(out)))
        return out

    def reconstruct_batch(self, ids):
        """index.reconstruct_batch(ids): int64 [n] -> float32 [n, d].  An id of -1 (a padding slot of a search) gives a row
        of all-ones words, the NaN faiss writes there; any other id outside [0, ntotal) raises HacError."""
        ids = _as_ids(ids, 1, "reconstruct_batch")
        out = np.empty((ids.shape[0], self.d), np.float32)
        _lib.check(_lib.lib().hac_index_reconstruct_ids(self._h, _i64p(ids), ids.shape[0], _f32p(out)))
        return out

    def reconstruct(self, i):
        """index.reconstruct(i) -> float32 [d]."""
        return self.reconstruct_batch(_as_ids(i, 0, "reconstruct").reshape(1))[0]

    def search_and_reconstruct(self, q, k):
        """D, I, R = index.search_and_reconstruct(q, k): R float32 [nq, k, d] holds the rows I names (all-ones where I is -1)."""
        q = _as_queries(q, self.d, "search_and_reconstruct")
        D, I = self.search(q, _as_k(k, "search_and_reconstruct"))
        return D, I, self.reconstruct_batch(I.reshape(-1)).reshape(I.shape[0], I.shape[1], self.d)

    def score_ids(self, q, ids):
        """Exact scores of named rows: q float32 [nq, d], ids int64 [nq, m] -> float32 [nq, m], the canonical score of every
        (q[i], row ids[i, j]) -- the bits a search returns for that pair.  -1 scores -FLT_MAX; NaN scores stay NaN."""
        q, ids = _pair_args(q, ids, self.d, "score_ids")
        D = np.empty(ids.shape, np.float32)
        _lib.check(_lib.lib().hac_index_score_ids(self._h, _f32p(q), q.shape[0], _i64p(ids), ids.shape[1], _f32p(D)))
        return D

    def rank_ids(self, q, ids):
        """Exact corpus rank of named rows: q float32 [nq, d], ids int64 [nq, m] -> int64 [nq, m], the 0-based position row
        ids[i, j] takes in an unbounded search of q[i] (order: score desc, row asc) -- no ceiling at HAC_MAX_K, and
        rank_ids(q, I)[i, j] == j for the I of any search.  -1 for the id -1 and for a row whose score is NaN (no search
        returns it); any other id outside [0, ntotal) raises HacError.  One pass over the rows per (16 queries, 8 ids)."""
        q, ids = _pair_args(q, ids, self.d, "rank_ids")
        R = np.empty(ids.shape, np.int64)
        _lib.check(_lib.lib().hac_index_rank_ids(self._h, _f32p(q), q.shape[0], _i64p(ids), ids.shape[1], _i64p(R)))
        return R

    # ---- entry at a rank (include/haconvdr.h, "entry at a rank") -------------
    def entries_at(self, q, ranks):
        """What sits at a rank: q float32 [nq, d], ranks int64 [nq, m] -> (D float32, I int64) of ranks.shape, the entry at
        0-based position ranks[i, j] of an unbounded search of q[i] (order: score desc, row asc) -- rank_ids' inverse, with no
        ceiling at HAC_MAX_K and at a cost that does not grow with the rank.  Ranks are values, not ids: any rank outside the
        list (negative, or at or beyond the number of rows whose score is not NaN) gives padding, -FLT_MAX / -1, never an error.
        entries_at(q, arange(k)) == search(q, k).  Single-device indexes only.  One pass over the rows per key digit (5 - 8) and
        16 (query, rank) pairs."""
        q, ranks = _rank_args(q, ranks, self.d)
        D, I = _host_results(ranks.shape)
        _lib.check(_lib.lib().hac_index_entries_at(self._h, _f32p(q), q.shape[0], _i64p(ranks), ranks.shape[1], _f32p(D), _i64p(I)))
        return D, I

    def search_at(self, q, k, start):
        """The entries [start, start + k) of the unbounded search: (D float32 [nq, k], I int64 [nq, k]).  start: an integer or
        int64 [nq], >= 0 (ValueError otherwise).  It is search_after behind entries_at(q, start - 1); a query with start == 0 gets
        the start cursor (search(q, k)), a start at or past the end gives padding only.  One entries_at of one rank per query
        plus one page, whatever the depth."""
        q = _as_queries(q, self.d, "search_at")
        k = _as_k(k, "search_at")
        start = _as_start(start, q.shape[0], "search_at")
        Dc, Ic = self.entries_at(q, (start - 1)[:, None])
        rows = np.where(start == 0, AFTER_START, Ic[:, 0]).astype(np.int64)   # (-1 from a start past the end: the exhausted list)
        return self.search_after(q, k, (np.ascontiguousarray(Dc[:, 0]), rows))

    # ---- range search (include/haconvdr.h, "range search") ------------------
    RANGE_FIRST_CAP = 1024   # results per query the first call of range_search makes room for

    def _range_call(self, q, radius, cap):
        lims = np.empty(q.shape[0] + 1, np.int64)
        D, I = _host_results((cap,))
        _lib.check(_lib.lib().hac_index_range_search(self._h, _f32p(q), q.shape[0], _f32p(radius), cap, _i64p(lims),
                                                     _f32p(D if cap else None), _i64p(I if cap else None)))
        return lims, D, I

    def range_search(self, q, radius):
        """lims, D, I = index.range_search(q, radius): every row whose score is STRICTLY above the query's radius (a scalar, or
        float32 [nq]).  lims int64 [nq + 1]; query i owns D[lims[i]:lims[i+1]] (float32) and I[lims[i]:lims[i+1]] (int64 rows),
        ordered by (score desc, row asc) -- the head of an unbounded search of q[i] (faiss leaves the order open).  NaN scores
        are in no list; a NaN or +Inf radius gives an empty list.  At most two library calls: the first makes room for
        RANGE_FIRST_CAP results per query, the second, only if that overflowed, for exactly lims[nq]."""
        q, radius = _range_args(q, radius, self.d)
        lims, D, I = self._range_call(q, radius, self.RANGE_FIRST_CAP * q.shape[0])
        total = int(lims[-1])
        if total > D.shape[0]:
            lims, D, I = self._range_call(q, radius, total)
        return lims, D[:total], I[:total]

    def range_count(self, q, radius):
        """len of every list range_search(q, radius) returns, int64 [nq], without the lists (the cap = 0 form: one pass over the
        rows per 16 queries, no sort).  Equals count_ahead(q, radius, 0)."""
        q, radius = _range_args(q, radius, self.d, "range_count")
        return np.diff(self._range_call(q, radius, 0)[0])

    def range_search_tensor(self, q, radius, cap, id_map=None, stream=None):
        """q float32 CUDA [nq, d], radius float32 CUDA [nq], cap = room for results -> (lims int64 [nq + 1], D float32 [cap],
        I int64 [cap]) CUDA tensors; no host sync.  lims is always exact.  If lims[nq] <= cap, D and I are filled in
        [0, lims[nq]) and untouched behind; otherwise their contents are unspecified: compare lims[nq] with cap and call again.
        id_map: optional int64 CUDA [ntotal], I = id_map[row].  Capturable after one call of the largest (nq, cap)."""
        q, radius, cap, id_map = _range_args_tensor(q, radius, cap, id_map, self.d)
        lims = _device_i64((q.shape[0] + 1,), q.device)
        D, I = _device_results((cap,), q.device)
        _lib.check(_lib.lib().hac_index_range_search_device(self._h, _devp(q), q.shape[0], _devp(radius), cap, _devp(lims), _devp(D if cap else None),
                                                            _devp(I if cap else None), _devp(id_map), _stream_ptr(stream)))
        _keep_alive(stream, q, radius, lims, D, I, *(() if id_map is None else (id_map,)))
        return lims, D, I

    # ---- device-resident variants (torch tensors on the index's GPU) -------
    def add_tensor(self, x, stream=None):
        """x: torch float32 CUDA tensor [n, d], contiguous.  Enqueued on ``stream`` (default: torch's current
        stream).  The host API (``add`` / ``search``) runs on the index's own stream: synchronize the stream used
        here before mixing in host-API calls."""
        assert x.is_cuda and x.dtype.is_floating_point and x.dim() == 2 and x.shape[1] == self.d
        x = x.contiguous().float()
        _lib.check(_lib.lib().hac_index_add_device(self._h, _devp(x), x.shape[0], _stream_ptr(stream)))
        _keep_alive(stream, x)

    def search_tensor(self, q, k, id_map=None, stream=None):
        """q: torch float32 CUDA [nq, d] -> (D float32 [nq,k], I int64 [nq,k]) CUDA tensors,
        enqueued on the current stream (no host sync).  id_map: optional int64 CUDA
        tensor [ntotal], fuses ``passage_embedding2id[I]`` (:110)."""
        assert q.is_cuda and q.dim() == 2 and q.shape[1] == self.d
        q = q.contiguous().float()
        id_map = _check_id_map_tensor(id_map, q, "search_tensor")
        D, I = _device_results((q.shape[0], k), q.device)
        _lib.check(_lib.lib().hac_index_search_device(self._h, _devp(q), q.shape[0], int(k), _devp(D), _devp(I), _devp(id_map), _stream_ptr(stream)))
        _keep_alive(stream, q, D, I, *(() if id_map is None else (id_map,)))
        return D, I

    def search_excluding_tensor(self, q, k, exclude, id_map=None, stream=None):
        """search_tensor over (rows minus the query's excluded rows): exclude int64 CUDA [nq, e] ROW ids (not id_map's), any id
        outside [0, ntotal) is ignored.  No host sync; capturable after one call of the largest (nq, k + e)."""
        q, k, exclude = _exclude_args_tensor(q, k, exclude, self.d)
        id_map = _check_id_map_tensor(id_map, q, "search_excluding_tensor")
        D, I = _device_results((q.shape[0], k), q.device)
        _lib.check(_lib.lib().hac_index_search_excluding_device(self._h, _devp(q), q.shape[0], k, _devp(exclude), exclude.shape[1], _devp(D), _devp(I),
                                                                _devp(id_map), _stream_ptr(stream)))
        _keep_alive(stream, q, exclude, D, I, *(() if id_map is None else (id_map,)))
        return D, I

    def search_among_tensor(self, q, k, cand, id_map=None, stream=None):
        """search_tensor over the query's candidate rows only: cand int64 CUDA [nq, m] ROW ids (not id_map's), a set; any id
        outside [0, ntotal), -1 included, is ignored.  id_map: optional int64 CUDA [ntotal], I = id_map[row].  No host sync;
        capturable after one call of the largest (nq, m, k)."""
        q, k, cand, id_map = _among_args_tensor(q, k, cand, id_map, self.d)
        D, I = _device_results((q.shape[0], k), q.device)
        _lib.check(_lib.lib().hac_index_search_among_device(self._h, _devp(q), q.shape[0], k, _devp(cand), cand.shape[1], _devp(D), _devp(I),
                                                            _devp(id_map), _stream_ptr(stream)))
        _keep_alive(stream, q, cand, D, I, *(() if id_map is None else (id_map,)))
        return D, I

    def search_among_keys_tensor(self, q, k, cand, pos_base=0, stream=None):
        """search_among_tensor's sorted packed keys (int64 view of uint64) [nq, k], positions pos_base + row: the unit exchanged
        between shards (merge_keys, keys_to_results)."""
        q, k, cand, _ = _among_args_tensor(q, k, cand, None, self.d, "search_among_keys_tensor")
        pos_base = _as_pos_base(pos_base, "search_among_keys_tensor")
        keys = _device_i64((q.shape[0], k), q.device)
        _lib.check(_lib.lib().hac_index_search_among_keys_device(self._h, _devp(q), q.shape[0], k, _devp(cand), cand.shape[1], _devp(keys),
                                                                 pos_base, _stream_ptr(stream)))
        _keep_alive(stream, q, cand, keys)
        return keys

    def search_masked_tensor(self, q, k, masks, mask_of=None, id_map=None, stream=None, after=None):
        """search_tensor over the rows a bitmap selects: masks packed int64 CUDA [n_masks, W] (pack_mask of a bool CUDA tensor),
        mask_of int64 CUDA [nq] or None (one mask, or one per query); a query whose mask_of entry is outside [0, n_masks) gets
        an empty list and no error.  id_map: optional int64 CUDA [ntotal], I = id_map[row].  after: None, or search_after_tensor's
        cursor pair (scores float32 CUDA [nq], rows int64 CUDA [nq]) -- the selected rows behind each query's cursor; a cursor
        row below -2 gives an empty list, and id_map remaps the result only.  No host sync; capturable after one call of the
        largest (nq, k, n_masks)."""
        q, k, masks, mask_of, id_map = _masked_args_tensor(q, k, masks, mask_of, id_map, self.d, self.ntotal)
        scores, rows = _cursor_tensor(after, q, "search_masked_tensor")
        D, I = _device_results((q.shape[0], k), q.device)
        head = (self._h, _devp(q), q.shape[0], k, _devp(masks), masks.shape[0], masks.shape[1], _devp(mask_of))
        tail = (_devp(D), _devp(I), _devp(id_map), _stream_ptr(stream))
        if after is None:
            _lib.check(_lib.lib().hac_index_search_masked_device(*head, *tail))
        else:
            _lib.check(_lib.lib().hac_index_search_masked_after_device(*head, _devp(scores), _devp(rows), *tail))
        _keep_alive(stream, q, masks, D, I, *(t for t in (scores, rows, mask_of, id_map) if t is not None))
        return D, I

    def search_masked_keys_tensor(self, q, k, masks, mask_of=None, pos_base=0, stream=None, after_keys=None):
        """search_masked_tensor's sorted packed keys (int64 view of uint64) [nq, k], positions pos_base + row: the unit exchanged
        between shards (merge_keys, keys_to_results).  after_keys: None, or int64 CUDA [nq] packed cursors in the same position
        space, as search_after_keys_tensor takes them (cursor_keys, or the last column of the page before; 0 = an exhausted
        list, -1 = the start): the selected rows whose key lies below the query's cursor."""
        q, k, masks, mask_of, _ = _masked_args_tensor(q, k, masks, mask_of, None, self.d, self.ntotal, "search_masked_keys_tensor")
        if after_keys is not None:   # (without a cursor pos_base goes to the library as it is, as in search_keys_tensor)
            pos_base = _as_pos_base(pos_base, "search_masked_keys_tensor")
            after_keys = _cursor_keys_tensor(after_keys, q, "search_masked_keys_tensor")
        keys = _device_i64((q.shape[0], k), q.device)
        head = (self._h, _devp(q), q.shape[0], k, _devp(masks), masks.shape[0], masks.shape[1], _devp(mask_of))
        tail = (_devp(keys), int(pos_base), _stream_ptr(stream))
        if after_keys is None:
            _lib.check(_lib.lib().hac_index_search_masked_keys_device(*head, *tail))
        else:
            _lib.check(_lib.lib().hac_index_search_masked_after_keys_device(*head, _devp(after_keys), *tail))
        _keep_alive(stream, q, masks, keys, *(t for t in (after_keys, mask_of) if t is not None))
        return keys

    def search_grouped_tensor(self, q, k, group_of, id_map=None, return_groups=False, stream=None):
        """search_grouped on the device: group_of int64 CUDA [ntotal]; a row whose label lies outside [0, 2^32) is in no list and
        raises nothing.  id_map: optional int64 CUDA [ntotal], I = id_map[row]; G (with return_groups) stays the row's own label.
        No host sync; capturable after one call of the largest (nq, k)."""
        q, k, group_of, id_map = _grouped_args_tensor(q, k, group_of, id_map, self.d, self.ntotal)
        D, I = _device_results((q.shape[0], k), q.device)
        G = _device_i64((q.shape[0], k), q.device) if return_groups else None
        _lib.check(_lib.lib().hac_index_search_grouped_device(self._h, _devp(q), q.shape[0], k, _devp(group_of), group_of.shape[0], _devp(D), _devp(I),
                                                              _devp(G), _devp(id_map), _stream_ptr(stream)))
        _keep_alive(stream, q, group_of, D, I, *(t for t in (G, id_map) if t is not None))
        return (D, I, G) if return_groups else (D, I)

    def search_after_tensor(self, q, k, after=None, id_map=None, stream=None):
        """search_after on the device: after None or (scores float32 CUDA [nq], rows int64 CUDA [nq]); a query whose cursor row
        is below -2 gets an empty list and no error.  id_map: optional int64 CUDA [ntotal], I = id_map[row] -- it remaps the
        result only: cursor rows are the index's own rows, so a caller that maps ids pages with search_after_keys_tensor.  No
        host sync; capturable after one call of the largest (nq, k)."""
        q, k, scores, rows, id_map = _after_args_tensor(q, k, after, id_map, self.d)
        D, I = _device_results((q.shape[0], k), q.device)
        _lib.check(_lib.lib().hac_index_search_after_device(self._h, _devp(q), q.shape[0], k, _devp(scores), _devp(rows), _devp(D), _devp(I),
                                                            _devp(id_map), _stream_ptr(stream)))
        _keep_alive(stream, q, D, I, *(t for t in (scores, rows, id_map) if t is not None))
        return D, I

    def search_after_keys_tensor(self, q, k, after_keys=None, pos_base=0, stream=None):
        """search_after_tensor's sorted packed keys (int64 view of uint64) [nq, k], positions pos_base + row: the unit exchanged
        between shards (merge_keys, keys_to_results).  after_keys: int64 CUDA [nq] packed cursors in the same position space
        (cursor_keys, or the last column of any sorted key list: search_keys_tensor's, a merged list's, this call's own); 0 = an
        exhausted list, -1 (all-ones) = the start; None starts every query from the start."""
        q, k, after_keys, pos_base = _after_keys_args_tensor(q, k, after_keys, pos_base, self.d)
        keys = _device_i64((q.shape[0], k), q.device)
        _lib.check(_lib.lib().hac_index_search_after_keys_device(self._h, _devp(q), q.shape[0], k, _devp(after_keys), _devp(keys), pos_base,
                                                                 _stream_ptr(stream)))
        _keep_alive(stream, q, keys, *(() if after_keys is None else (after_keys,)))
        return keys

    def entries_at_tensor(self, q, ranks, id_map=None, stream=None):
        """entries_at on the device: q float32 CUDA [nq, d], ranks int64 CUDA [nq, m] -> (D float32, I int64) CUDA of
        ranks.shape.  id_map: optional int64 CUDA [ntotal], I = id_map[row].  No host sync; the launches depend on (nq, m) and
        the index's size only; capturable after one call of the largest (nq, m)."""
        q, ranks = _rank_args_tensor(q, ranks, self.d)
        id_map = _check_id_map_tensor(id_map, q, "entries_at_tensor")
        D, I = _device_results(tuple(ranks.shape), q.device)
        _lib.check(_lib.lib().hac_index_entries_at_device(self._h, _devp(q), q.shape[0], _devp(ranks), ranks.shape[1], _devp(D), _devp(I), _devp(id_map),
                                                          _stream_ptr(stream)))
        _keep_alive(stream, q, ranks, D, I, *(() if id_map is None else (id_map,)))
        return D, I

    def entry_keys_at_tensor(self, q, ranks, pos_base=0, stream=None):
        """entries_at_tensor's packed keys (int64 view of uint64) of ranks.shape, positions pos_base + row, 0 = padding: the key
        space of search_keys_tensor and of search_after_keys_tensor's cursors, so a column of it is the cursor of the page
        behind those entries."""
        q, ranks = _rank_args_tensor(q, ranks, self.d, "entry_keys_at_tensor")
        pos_base = _as_pos_base(pos_base, "entry_keys_at_tensor")
        keys = _device_i64(tuple(ranks.shape), q.device)
        _lib.check(_lib.lib().hac_index_entries_at_keys_device(self._h, _devp(q), q.shape[0], _devp(ranks), ranks.shape[1], _devp(keys), pos_base,
                                                               _stream_ptr(stream)))
        _keep_alive(stream, q, ranks, keys)
        return keys

    def search_at_keys_tensor(self, q, k, start, pos_base=0, stream=None):
        """search_at's sorted packed keys (int64 view of uint64) [nq, k], positions pos_base + row, composed on the device:
        the cursor is where(start == 0, the start, entry_keys_at_tensor(q, start - 1)), fed to search_after_keys_tensor.
        start: an integer >= 0 or int64 CUDA [nq] (a negative entry gives that query an empty list).  No host sync."""
        import torch
        q = _queries_tensor(q, self.d, "search_at_keys_tensor")
        k = _as_k(k, "search_at_keys_tensor")
        with _on_stream(stream):   # (torch's own kernels between the two library calls go where those go)
            start = _start_tensor(start, q, "search_at_keys_tensor")
            cursor = self.entry_keys_at_tensor(q, (start - 1)[:, None], pos_base, stream)[:, 0]
            cursor = torch.where(start == 0, torch.full_like(cursor, -1), cursor).contiguous()
        return self.search_after_keys_tensor(q, k, cursor, pos_base, stream)

    def search_at_tensor(self, q, k, start, id_map=None, stream=None):
        """search_at on the device -> (D float32 [nq, k], I int64 [nq, k]) CUDA tensors; id_map: optional int64 CUDA [ntotal],
        I = id_map[row].  No host sync."""
        q = _queries_tensor(q, self.d, "search_at_tensor")
        id_map = _check_id_map_tensor(id_map, q, "search_at_tensor")
        keys = self.search_at_keys_tensor(q, k, start, 0, stream)
        return keys_to_results(keys, id_map, stream)

    def search_keys_tensor(self, q, k, pos_base=0, stream=None):
        """Packed top-k keys (int64 view of uint64) [nq, k]; the unit exchanged between shards."""
        import torch
        q = q.contiguous().float()
        keys = torch.empty((q.shape[0], k), dtype=torch.int64, device=q.device)
        _lib.check(_lib.lib().hac_index_search_keys_device(self._h, _devp(q), q.shape[0], int(k), _devp(keys), int(pos_base), _stream_ptr(stream)))
        _keep_alive(stream, q, keys)
        return keys

    def reconstruct_tensor(self, ids=None, i0=0, n=None, stream=None):
        """ids: int64 CUDA tensor [n] -> float32 CUDA [n, d]; ids=None: the rows [i0, i0 + n) (n=None: up to ntotal).
        Enqueued on ``stream`` (default: torch's current stream), no host sync.  Any id outside [0, ntotal), -1 included,
        gives a row of all-ones words and no error."""
        import torch
        if ids is None:
            i0, n = _as_range(i0, n, "reconstruct_tensor")
            if n is None:
                n = self.ntotal - i0
            dev = torch.device("cuda", self.devices[0])
        else:
            ids = _ids_tensor(ids, 1, "reconstruct_tensor")
            i0, n, dev = 0, ids.shape[0], ids.device
        out = torch.empty((max(n, 0), self.d), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().hac_index_reconstruct_device(self._h, _devp(ids), i0, n, _devp(out), _stream_ptr(stream)))
        _keep_alive(stream, out, *(() if ids is None else (ids,)))
        return out

    def score_ids_tensor(self, q, ids, stream=None):
        """q: float32 CUDA [nq, d], ids: int64 CUDA [nq, m] -> float32 CUDA [nq, m]; no host sync.  Any id outside
        [0, ntotal), -1 included, scores -FLT_MAX."""
        import torch
        q, ids = _pair_args_tensor(q, ids, self.d, "score_ids_tensor")
        D = torch.empty(tuple(ids.shape), dtype=torch.float32, device=q.device)
        _lib.check(_lib.lib().hac_index_score_ids_device(self._h, _devp(q), q.shape[0], _devp(ids), ids.shape[1], _devp(D), _stream_ptr(stream)))
        _keep_alive(stream, q, ids, D)
        return D

    def rank_ids_tensor(self, q, ids, stream=None):
        """q: float32 CUDA [nq, d], ids: int64 CUDA [nq, m] -> int64 CUDA [nq, m], rank_ids without a host sync.  Any id outside
        [0, ntotal), -1 included, ranks -1.  Capturable after one call of the largest (nq, m)."""
        q, ids = _pair_args_tensor(q, ids, self.d, "rank_ids_tensor")
        R = _device_i64(tuple(ids.shape), q.device)
        _lib.check(_lib.lib().hac_index_rank_ids_device(self._h, _devp(q), q.shape[0], _devp(ids), ids.shape[1], _devp(R), _stream_ptr(stream)))
        _keep_alive(stream, q, ids, R)
        return R

    def count_ahead_tensor(self, q, ref_scores, ref_bounds, stream=None):
        """The primitive behind rank_ids, the one corpus shards add up: per (query i, slot j) the number of this index's rows r
        whose score is not NaN and beats (ref_scores[i, j], ref_bounds[i, j]): s > s_ref, or s == s_ref and r < bound.
        q float32 CUDA [nq, d], ref_scores float32 CUDA [nq, m], ref_bounds int64 CUDA [nq, m] -> int64 CUDA [nq, m]; -1 for a
        NaN reference score or a negative bound; a bound above ntotal behaves like ntotal.  No host sync."""
        q, ref_scores, ref_bounds = _count_args_tensor(q, ref_scores, ref_bounds, self.d)
        C = _device_i64(tuple(ref_bounds.shape), q.device)
        _lib.check(_lib.lib().hac_index_count_ahead_device(self._h, _devp(q), q.shape[0], _devp(ref_scores), _devp(ref_bounds), ref_bounds.shape[1],
                                                           _devp(C), _stream_ptr(stream)))
        _keep_alive(stream, q, ref_scores, ref_bounds, C)
        return C

    def search_and_reconstruct_tensor(self, q, k, stream=None):
        """search_tensor, then reconstruct_tensor on its I, on one stream -> (D [nq,k], I [nq,k], R [nq,k,d])."""
        q = _queries_tensor(q, self.d, "search_and_reconstruct_tensor")
        D, I = self.search_tensor(q, _as_k(k, "search_and_reconstruct_tensor"), stream=stream)
        return D, I, self.reconstruct_tensor(I.reshape(-1), stream=stream).reshape(I.shape[0], I.shape[1], self.d)

    def set_option(self, name, value):
        """Tuning / test switch of this handle (include/haconvdr.h: hac_index_set_option), e.g.
        ``set_option("split", "0")`` = exact fp32 kernels only."""
        _lib.check(_lib.lib().hac_index_set_option(self._h, str(name).encode(), str(value).encode()))

    def set_profiling(self, on=True):
        _lib.check(_lib.lib().hac_index_set_profiling(self._h, int(bool(on))))

    def last_plan(self):
        return _lib.lib().hac_index_last_plan(self._h).decode()

    def check_status(self):
        """Raise HacError (code HAC_ERR_INTERNAL) if a scan of a search enqueued so far gave up at its pass bound
        (hac_index_last_status).  The host API reports this itself; after ``search_tensor`` / ``search_keys_tensor``
        synchronize the stream you searched on, then call this.  Reading clears the error word."""
        _lib.check(_lib.lib().hac_index_last_status(self._h))

    def profile_drain(self, cap=4096):
        """Durations (ms) of the main scan kernel of every search since the last drain."""
        buf = (ctypes.c_float * cap)()
        n = ctypes.c_int()
        _lib.check(_lib.lib().hac_index_profile_drain(self._h, buf, cap, ctypes.byref(n)))
        return [float(buf[i]) for i in range(n.value)]


def merge_keys(lists, stream=None):
    """lists: int64(uint64) CUDA tensor [L, nq, k] of per-shard sorted keys -> [nq, k]."""
    import torch
    L, nq, k = lists.shape
    lists = lists.contiguous()
    out = torch.empty((nq, k), dtype=torch.int64, device=lists.device)
    _lib.check(_lib.lib().hac_merge_keys_device(lists.device.index or 0, _devp(lists), L, nq, k, _devp(out), _stream_ptr(stream)))
    return out


def filter_keys(keys, exclude_pos, k, stream=None):
    """keys [nq, kin] sorted per-query lists, exclude_pos int64 CUDA [nq, e] global positions (< 0 or > 0xFFFFFFFF = padding)
    -> [nq, k]: each query's first k keys whose position is not excluded, in order, the rest 0."""
    keys, exclude_pos, k = _filter_args(keys, exclude_pos, k)
    out = _device_i64((keys.shape[0], k), keys.device)
    _lib.check(_lib.lib().hac_filter_keys_device(keys.device.index or 0, _devp(keys), keys.shape[0], keys.shape[1], _devp(exclude_pos),
                                                 exclude_pos.shape[1], k, _devp(out), _stream_ptr(stream)))
    _keep_alive(stream, keys, exclude_pos, out)
    return out


def keys_to_results(keys, id_map=None, stream=None):
    """keys [nq,k] -> (D float32, I int64); id_map optional int64 CUDA tensor (position -> id)."""
    keys = keys.contiguous()
    D, I = _device_results(keys.shape, keys.device)
    _lib.check(_lib.lib().hac_keys_to_results_device(keys.device.index or 0, _devp(keys), keys.numel(), _devp(id_map), _devp(D), _devp(I),
                                                     _stream_ptr(stream)))
    return D, I


def build_index(args):
    """Mirror of build_faiss_index(args) (src/test_HAConvDR_topiocqa.py:39-71).

    ``args.n_gpu`` devices hold contiguous shards of every added block; the reference's
    CPU branch (``use_gpu`` false, :68-69) has no counterpart here — this package is
    the GPU path and refuses to run without one."""
    n_gpu = max(1, int(getattr(args, "n_gpu", 1)))
    return FlatIPIndex(768, devices=tuple(range(n_gpu)))
