"""ctypes binding of haconvdr_amd/csrc/libhaconvdr.so (C ABI: include/haconvdr.h).

There is no CPU fallback.  If the HIP library has not been built, or no MI355X is
visible, the first call raises — loudly — instead of computing anything on the host.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# HAC_LIBRARY_PATH: development only (A/B runs of kernel variants built beside the tree); the product is the in-tree library
LIB_PATH = os.environ.get("HAC_LIBRARY_PATH") or os.path.join(_HERE, "csrc", "libhaconvdr.so")
_LIB = None

HAC_MAX_K = 2048
HAC_MAX_AMONG = 4096   # include/haconvdr.h: candidates per query of search_among
HAC_AFTER_START = -2   # include/haconvdr.h: the cursor row of search_after that starts a query from the start
HAC_ERR_INVALID = 1    # include/haconvdr.h: a bad argument
HAC_ERR_UNSUPPORTED = 4
HAC_ERR_INTERNAL = 5   # include/haconvdr.h: the device detected a broken invariant of the library (never a hang, never wrong bits)


class HacError(RuntimeError):
    """A C-ABI call returned a non-zero hac_status."""

    def __init__(self, code, msg):
        super().__init__(f"haconvdr error {code}: {msg}")
        self.code = code


_int, _vp, _i64, _u32, _str = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32, ctypes.c_char_p
_f32p, _i64p, _u64p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint64)
_intp, _i32p = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int32)

# Every symbol include/haconvdr.h declares, once: name -> (restype, argtypes).  _declare() and EXPORTED_SYMBOLS read this table
# (tests/test_host_logic.py compares it with the header).
_SIGNATURES = {
    "hac_last_error": (_str, []),
    "hac_version": (_str, []),
    "hac_index_create": (_int, [_int, _intp, _int, ctypes.POINTER(_vp)]),
    "hac_index_destroy": (None, [_vp]),
    "hac_index_add": (_int, [_vp, _f32p, _i64]),
    "hac_index_add_device": (_int, [_vp, _vp, _i64, _vp]),
    "hac_index_search": (_int, [_vp, _f32p, _i64, _int, _f32p, _i64p]),
    "hac_index_search_device": (_int, [_vp, _vp, _i64, _int, _vp, _vp, _vp, _vp]),
    "hac_index_search_keys_device": (_int, [_vp, _vp, _i64, _int, _vp, _u32, _vp]),
    "hac_index_reset": (_int, [_vp]),
    "hac_index_reconstruct": (_int, [_vp, _i64, _i64, _f32p]),
    "hac_index_reconstruct_ids": (_int, [_vp, _i64p, _i64, _f32p]),
    "hac_index_reconstruct_device": (_int, [_vp, _vp, _i64, _i64, _vp, _vp]),
    "hac_index_score_ids": (_int, [_vp, _f32p, _i64, _i64p, _i64, _f32p]),
    "hac_index_score_ids_device": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _vp]),
    "hac_index_count_ahead_device": (_int, [_vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp]),
    "hac_index_rank_ids": (_int, [_vp, _f32p, _i64, _i64p, _i64, _i64p]),
    "hac_index_rank_ids_device": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _vp]),
    "hac_index_range_search": (_int, [_vp, _f32p, _i64, _f32p, _i64, _i64p, _f32p, _i64p]),
    "hac_index_range_search_device": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "hac_index_remove_ids": (_int, [_vp, _i64p, _i64, _i64p]),
    "hac_index_search_among": (_int, [_vp, _f32p, _i64, _int, _i64p, _i64, _f32p, _i64p]),
    "hac_index_search_among_device": (_int, [_vp, _vp, _i64, _int, _vp, _i64, _vp, _vp, _vp, _vp]),
    "hac_index_search_among_keys_device": (_int, [_vp, _vp, _i64, _int, _vp, _i64, _vp, _u32, _vp]),
    "hac_index_search_masked": (_int, [_vp, _f32p, _i64, _int, _u64p, _i64, _i64, _i64p, _f32p, _i64p]),
    "hac_index_search_masked_device": (_int, [_vp, _vp, _i64, _int, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp]),
    "hac_index_search_masked_keys_device": (_int, [_vp, _vp, _i64, _int, _vp, _i64, _i64, _vp, _vp, _u32, _vp]),
    "hac_index_search_masked_after": (_int, [_vp, _f32p, _i64, _int, _u64p, _i64, _i64, _i64p, _f32p, _i64p, _f32p, _i64p]),
    "hac_index_search_masked_after_device": (_int, [_vp, _vp, _i64, _int, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hac_index_search_masked_after_keys_device": (_int, [_vp, _vp, _i64, _int, _vp, _i64, _i64, _vp, _vp, _vp, _u32, _vp]),
    "hac_index_search_grouped": (_int, [_vp, _f32p, _i64, _int, _i64p, _i64, _f32p, _i64p, _i64p]),
    "hac_index_search_grouped_device": (_int, [_vp, _vp, _i64, _int, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "hac_index_search_after": (_int, [_vp, _f32p, _i64, _int, _f32p, _i64p, _f32p, _i64p]),
    "hac_index_search_after_device": (_int, [_vp, _vp, _i64, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hac_index_search_after_keys_device": (_int, [_vp, _vp, _i64, _int, _vp, _vp, _u32, _vp]),
    "hac_index_entries_at": (_int, [_vp, _f32p, _i64, _i64p, _i64, _f32p, _i64p]),
    "hac_index_entries_at_device": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
    "hac_index_entries_at_keys_device": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _u32, _vp]),
    "hac_index_ntotal": (_i64, [_vp]),
    "hac_index_set_option": (_int, [_vp, _str, _str]),
    "hac_index_set_profiling": (_int, [_vp, _int]),
    "hac_index_profile_drain": (_int, [_vp, _f32p, _int, _intp]),
    "hac_index_last_plan": (_str, [_vp]),
    "hac_index_last_status": (_int, [_vp]),
    "hac_merge_keys_device": (_int, [_int, _vp, _int, _i64, _int, _vp, _vp]),
    "hac_keys_to_results_device": (_int, [_int, _vp, _i64, _vp, _vp, _vp, _vp]),
    "hac_filter_keys_device": (_int, [_int, _vp, _i64, _int, _vp, _int, _int, _vp, _vp]),
    "hac_index_search_excluding": (_int, [_vp, _f32p, _i64, _int, _i64p, _int, _f32p, _i64p]),
    "hac_index_search_excluding_device": (_int, [_vp, _vp, _i64, _int, _vp, _int, _vp, _vp, _vp, _vp]),
    "hac_encoder_create": (_int, [_vp, _int, ctypes.POINTER(_vp)]),
    "hac_encoder_destroy": (None, [_vp]),
    "hac_encoder_set_weight": (_int, [_vp, _str, _f32p, ctypes.c_size_t]),
    "hac_encoder_finalize": (_int, [_vp]),
    "hac_encoder_forward": (_int, [_vp, _i32p, _i32p, _int, _int, _f32p]),
    "hac_encoder_forward_device": (_int, [_vp, _vp, _vp, _int, _int, _int, _vp, _vp]),
    "hac_encoder_set_option": (_int, [_vp, _str, _str]),
    "hac_encoder_last_plan": (_str, [_vp]),
    "hac_encoder_set_profiling": (_int, [_vp, _int]),
    "hac_encoder_profile_drain": (_int, [_vp, _f32p, _int, _intp]),
    "hac_encoder_profile_drain_class": (_int, [_vp, _int, _f32p, _int, _intp]),
    "hac_encoder_last_clock": (_int, [_vp, _u64p]),
    "hac_encoder_attention_redo": (_int, [_vp, ctypes.POINTER(ctypes.c_longlong)]),
    "hac_encoder_layer_state": (_int, [_vp, _i32p, _i32p, _int, _int, _int, _f32p, _f32p, _f32p]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def _declare(L):
    for name, (restype, argtypes) in _SIGNATURES.items():
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes


class EncoderConfig(ctypes.Structure):
    _fields_ = [("n_layers", ctypes.c_int), ("hidden", ctypes.c_int), ("n_heads", ctypes.c_int), ("ffn", ctypes.c_int),
                ("vocab", ctypes.c_int), ("max_pos", ctypes.c_int), ("type_vocab", ctypes.c_int), ("pad_token_id", ctypes.c_int),
                ("ln_eps", ctypes.c_float)]


def lib():
    """The loaded library; raises if it was never built (run __graft_entry__.build())."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build the HIP library first (python -c 'import __graft_entry__ as g; "
                "g.build()' or make -C haconvdr_amd/csrc).  haconvdr_amd has no CPU fallback.")
        # torch bundles its own libamdhip64.so.7; it must be the one HIP runtime of the process,
        # so it is loaded first and libhaconvdr.so binds to it by soname (two runtimes in one
        # process leave the second without devices).
        import torch  # noqa: F401
        L = ctypes.CDLL(LIB_PATH)
        _declare(L)
        _LIB = L
    return _LIB


def check(rc):
    if rc != 0:
        raise HacError(rc, lib().hac_last_error().decode("utf-8", "replace"))
