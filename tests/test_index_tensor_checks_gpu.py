"""The public *_tensor methods of FlatIPIndex against mistakes in real CUDA tensors, with the library stubbed out.

The tensor forms hand raw device pointers to kernels, so a CPU tensor, a wrong dtype, a wrong shape or a tensor on another
device must raise ValueError BEFORE any entry point of the library is called.  This file must not be able to launch a kernel
with a bad pointer, so _lib.lib is replaced by a stub that records the entry points it is asked for and returns 0; the index
is made without a handle.  (score_ids_tensor / rank_ids_tensor: tests/test_index_rows_gpu.py.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, NQ, NTOTAL, K = 96, 3, 130, 10
W = (NTOTAL + 63) // 64

# the tensor arguments: name -> (dtype name, shape, the dimension whose length the checks fix or None)
ARGS = {
    "q": ("float32", (NQ, D), 1),
    "id_map": ("int64", (NTOTAL,), None),             # (its length is the library's to know)
    "exclude": ("int64", (NQ, 4), 0),
    "cand": ("int64", (NQ, 4), 0),
    "masks": ("int64", (2, W), 1),
    "mask_of": ("int64", (NQ,), 0),
    "group_of": ("int64", (NTOTAL,), 0),
    "scores": ("float32", (NQ,), 0),                  # the cursor pair of after=
    "rows": ("int64", (NQ,), 0),
    "after_keys": ("int64", (NQ,), 0),
    "ranks": ("int64", (NQ, 4), 0),
    "start": ("int64", (NQ,), 0),
    "radius": ("float32", (NQ,), 0),
    "ref_scores": ("float32", (NQ, 4), 0),
    "ref_bounds": ("int64", (NQ, 4), 0),
}

# method -> (call(idx, a, pos_base), its tensor arguments, the entry points one good call makes, takes pos_base)
METHODS = {
    "search_tensor": (lambda idx, a, pb: idx.search_tensor(a["q"], K, id_map=a["id_map"]),
                      ["id_map"], ["hac_index_search_device"], False),    # (its q is checked by assert, not by ValueError)
    "search_excluding_tensor": (lambda idx, a, pb: idx.search_excluding_tensor(a["q"], K, a["exclude"], id_map=a["id_map"]),
                                ["q", "exclude", "id_map"], ["hac_index_search_excluding_device"], False),
    "search_among_tensor": (lambda idx, a, pb: idx.search_among_tensor(a["q"], K, a["cand"], id_map=a["id_map"]),
                            ["q", "cand", "id_map"], ["hac_index_search_among_device"], False),
    "search_among_keys_tensor": (lambda idx, a, pb: idx.search_among_keys_tensor(a["q"], K, a["cand"], pos_base=pb),
                                 ["q", "cand"], ["hac_index_search_among_keys_device"], True),
    "search_masked_tensor": (lambda idx, a, pb: idx.search_masked_tensor(a["q"], K, a["masks"], a["mask_of"], id_map=a["id_map"],
                                                                         after=(a["scores"], a["rows"])),
                             ["q", "masks", "mask_of", "id_map", "scores", "rows"], ["hac_index_search_masked_after_device"], False),
    "search_masked_keys_tensor": (lambda idx, a, pb: idx.search_masked_keys_tensor(a["q"], K, a["masks"], a["mask_of"], pos_base=pb,
                                                                                   after_keys=a["after_keys"]),
                                  ["q", "masks", "mask_of", "after_keys"], ["hac_index_search_masked_after_keys_device"], True),
    "search_grouped_tensor": (lambda idx, a, pb: idx.search_grouped_tensor(a["q"], K, a["group_of"], id_map=a["id_map"], return_groups=True),
                              ["q", "group_of", "id_map"], ["hac_index_search_grouped_device"], False),
    "search_after_tensor": (lambda idx, a, pb: idx.search_after_tensor(a["q"], K, (a["scores"], a["rows"]), id_map=a["id_map"]),
                            ["q", "scores", "rows", "id_map"], ["hac_index_search_after_device"], False),
    "search_after_keys_tensor": (lambda idx, a, pb: idx.search_after_keys_tensor(a["q"], K, a["after_keys"], pos_base=pb),
                                 ["q", "after_keys"], ["hac_index_search_after_keys_device"], True),
    "entries_at_tensor": (lambda idx, a, pb: idx.entries_at_tensor(a["q"], a["ranks"], id_map=a["id_map"]),
                          ["q", "ranks", "id_map"], ["hac_index_entries_at_device"], False),
    "entry_keys_at_tensor": (lambda idx, a, pb: idx.entry_keys_at_tensor(a["q"], a["ranks"], pos_base=pb),
                             ["q", "ranks"], ["hac_index_entries_at_keys_device"], True),
    "search_at_keys_tensor": (lambda idx, a, pb: idx.search_at_keys_tensor(a["q"], K, a["start"], pos_base=pb),   # two calls, composed on the device
                              ["q", "start"], ["hac_index_entries_at_keys_device", "hac_index_search_after_keys_device"], True),
    "search_at_tensor": (lambda idx, a, pb: idx.search_at_tensor(a["q"], K, a["start"], id_map=a["id_map"]),
                         ["q", "start", "id_map"], ["hac_index_entries_at_keys_device", "hac_index_search_after_keys_device"], False),
    "range_search_tensor": (lambda idx, a, pb: idx.range_search_tensor(a["q"], a["radius"], 50, id_map=a["id_map"]),
                            ["q", "radius", "id_map"], ["hac_index_range_search_device"], False),
    "count_ahead_tensor": (lambda idx, a, pb: idx.count_ahead_tensor(a["q"], a["ref_scores"], a["ref_bounds"]),
                           ["q", "ref_scores", "ref_bounds"], ["hac_index_count_ahead_device"], False),
}
MISTAKES = ["cpu tensor", "wrong dtype", "wrong rank", "wrong length", "second device"]


class _StubLib:
    """every hac_* entry point records its name and returns 0 (hac_index_ntotal: 130); nothing reaches the GPU"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("hac_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append(name)
            return NTOTAL if name == "hac_index_ntotal" else 0
        return entry

    def index_calls(self):
        return [c for c in self.calls if c.startswith("hac_index_") and c != "hac_index_ntotal"]


@pytest.fixture
def stub(monkeypatch):
    from haconvdr_amd import _lib
    s = _StubLib()
    monkeypatch.setattr(_lib, "lib", lambda: s)
    return s


@pytest.fixture
def idx():
    from haconvdr_amd.index import FlatIPIndex
    i = object.__new__(FlatIPIndex)
    i.d, i.devices, i._h = D, (0,), None
    return i


@pytest.fixture(scope="module")
def good():
    import torch
    dev = torch.device("cuda", 0)
    return {name: (torch.arange(int(np.prod(shape)), device=dev) % 2).to(getattr(torch, dtype)).reshape(shape) for name, (dtype, shape, _) in ARGS.items()}


def _spoil(t, name, mistake):
    import torch
    dtype, shape, fixed = ARGS[name]
    if mistake == "cpu tensor":
        return t.cpu()
    if mistake == "wrong dtype":                      # (q may be any floating dtype: an integer one is the mistake)
        return t.to(torch.int64 if name == "q" else torch.int32 if dtype == "int64" else torch.float64)
    if mistake == "wrong rank":
        return t[..., None]
    if mistake == "wrong length":
        return torch.cat([t, t.narrow(fixed, 0, 1)], dim=fixed)
    if torch.cuda.device_count() < 2:
        pytest.skip("this machine shows one device")
    return t.to(torch.device("cuda", 1))


@pytest.mark.parametrize("method", list(METHODS))
def test_a_good_call_makes_exactly_its_entry_points(stub, idx, good, method):
    call, _, entries, _ = METHODS[method]
    call(idx, good, 0)
    assert stub.index_calls() == entries


@pytest.mark.parametrize("method, arg, mistake", [(m, arg, mistake) for m, (_, args, _, _) in METHODS.items() for arg in args for mistake in MISTAKES
                                                  if mistake != "wrong length" or ARGS[arg][2] is not None])
def test_a_bad_tensor_raises_before_the_library_is_called(stub, idx, good, method, arg, mistake):
    bad = dict(good)
    bad[arg] = _spoil(good[arg], arg, mistake)
    with pytest.raises(ValueError):
        METHODS[method][0](idx, bad, 0)
    assert stub.index_calls() == []


@pytest.mark.parametrize("pos_base", [-1, 2 ** 32])
@pytest.mark.parametrize("method", [m for m, spec in METHODS.items() if spec[3]])
def test_a_bad_pos_base_raises_before_the_library_is_called(stub, idx, good, method, pos_base):
    with pytest.raises(ValueError):
        METHODS[method][0](idx, good, pos_base)
    assert stub.index_calls() == []
