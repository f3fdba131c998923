"""entries_at / search_at, the parts that need no GPU: the C-ABI surface of the three entry points, the resource lines of
rank_hist_kernel / rank_narrow_kernel, the identities of include/haconvdr.h ("entry at a rank") proved over the oracle on the
inputs of tests/test_index_at_rank_gpu.py (against after_ref, rank_ref and range_ref), proofs that those inputs show what they
are for, the documented pass count, and the argument checks of the Python mirrors (ValueError before the library is called, no
handle needed)."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import after_ref, at_rank_cases as cases, at_rank_ref, range_ref, rank_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("hac_index_entries_at", "hac_index_entries_at_device", "hac_index_entries_at_keys_device")
FMAX = after_ref.FMAX
_CASES = {}


def scores(name, oracle):
    """(x, q, S) of the GPU tests' inputs, computed once and never changed"""
    if name not in _CASES:
        x, q = {"hostile32": lambda: cases.hostile_case(32), "hostile96": lambda: cases.hostile_case(96),
                "hostile768": lambda: cases.hostile_case(768), "zero": cases.tie_zero_case, "dup": cases.tie_dup_case,
                "grid": cases.grid_case, "at": cases.at_case}[name]()
        with np.errstate(all="ignore"):
            S = rank_ref.canon_scores(oracle, x, q)
        S.setflags(write=False)
        _CASES[name] = (x, q, S)
    return _CASES[name]


# ---------------------------------------------------------------------------------------------------------------------
# symbols, registers
def test_new_entry_points_are_declared_listed_and_exported():
    from haconvdr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "haconvdr.h")).read()
    assert "entry at a rank" in hdr
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
    assert [len(getattr(L, sym).argtypes) for sym in NEW_SYMBOLS] == [7, 9, 8]


def test_at_rank_kernels_keep_everything_in_registers():
    path = os.path.join(ROOT, "haconvdr_amd", "csrc", "flat_ip.resources.txt")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(path)])
    blocks = re.split(r"remark: Function Name: ", open(path).read())
    for kernel in ("rank_hist_kernel", "rank_narrow_kernel"):
        mine = [b for b in blocks if re.search(r"\d+%s[A-Z]" % kernel, b.split("\n", 1)[0])]
        assert len(mine) == 1, (kernel, [b.split("\n", 1)[0] for b in mine])
        assert int(re.search(r"VGPRs: (\d+)", mine[0]).group(1)) <= 256, kernel
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", mine[0]).group(1)) == 0, kernel
        assert int(re.search(r"VGPRs Spill: (\d+)", mine[0]).group(1)) == 0, kernel


# ---------------------------------------------------------------------------------------------------------------------
# the identities, on the GPU tests' inputs
IDENTITY_CASES = ("hostile32", "hostile96", "hostile768", "grid", "at")


@pytest.mark.parametrize("name", IDENTITY_CASES)
def test_first_k_ranks_are_search(name, oracle):
    x, q, S = scores(name, oracle)
    for k in (1, 100, 2048):
        want = oracle.flat_ip_search(x, q, k)
        got = at_rank_ref.entries_at_from_scores(S, np.tile(np.arange(k, dtype=np.int64), (len(q), 1)))
        after_ref.assert_same(got, want, f"{name} k={k}")


@pytest.mark.parametrize("name", IDENTITY_CASES)
def test_rank_ids_inverts_entries_at_and_back(name, oracle):
    x, q, S = scores(name, oracle)
    nq, n = S.shape
    ranks = cases.all_ranks(nq, n)
    D, I = at_rank_ref.entries_at_from_scores(S, ranks)
    back = rank_ref.rank_ids_from_scores(S, I)
    np.testing.assert_array_equal(back[I >= 0], ranks[I >= 0])
    assert (back[I < 0] == -1).all()
    # and the other way round: naming every row, entries_at of its rank names it again, with score_ids' bits
    ids = np.tile(np.arange(n, dtype=np.int64), (nq, 1))
    r = rank_ref.rank_ids_from_scores(S, ids)
    D2, I2 = at_rank_ref.entries_at_from_scores(S, r)
    np.testing.assert_array_equal(I2[r >= 0], ids[r >= 0])
    np.testing.assert_array_equal(after_ref.bits(D2[r >= 0]), after_ref.bits(S[r >= 0]))
    assert (I2[r < 0] == -1).all() and (r < 0).any() == bool(np.isnan(S).any())


@pytest.mark.parametrize("name", IDENTITY_CASES)
def test_search_after_behind_an_entry_continues_the_list(name, oracle):
    x, q, S = scores(name, oracle)
    nq, n = S.shape
    L = at_rank_ref.list_len(S)
    for t in (0, 1, 99, int(L.min()) - 2, int(L.min()) - 1, int(L.max()), n + 5):
        for k in (1, 100):
            cD, cI = at_rank_ref.entries_at_from_scores(S, np.full((nq, 1), t, np.int64))
            got = after_ref.after_from_scores(S, cD[:, 0], cI[:, 0], k)
            want = at_rank_ref.search_at_from_scores(S, np.full(nq, t + 1, np.int64), k)
            # behind a padding entry (t at or past the end) the list is exhausted, as search_at past the end is
            after_ref.assert_same(got, want, f"{name} t={t} k={k}")
            # the keys form: an entry's key is the cursor of the page behind it
            keys = at_rank_ref.entry_keys_from_scores(S, np.full((nq, 1), t, np.int64), 1000)[:, 0]
            after_ref.assert_same(after_ref.unpack(after_ref.after_from_keys(S, keys, 1000, k), 1000), want, f"{name} keys t={t} k={k}")


@pytest.mark.parametrize("name", IDENTITY_CASES)
def test_range_count_brackets_the_score_at_a_rank(name, oracle):
    x, q, S = scores(name, oracle)
    nq, n = S.shape
    L = at_rank_ref.list_len(S)
    rng = np.random.default_rng(0xD01)
    seen = 0
    for trial in range(8):
        rows = rng.integers(0, n, nq)
        radius = np.where(np.isnan(S[np.arange(nq), rows]), np.float32(0.25), S[np.arange(nq), rows]).astype(np.float32)
        lims = range_ref.range_from_scores(S, radius)[0]
        c = np.diff(lims).astype(np.int64)
        D = at_rank_ref.entries_at_from_scores(S, np.stack([c - 1, c], 1))[0]
        for i in range(nq):
            if c[i] >= 1:
                assert D[i, 0] > radius[i]
            if c[i] < L[i]:
                assert radius[i] >= D[i, 1]
            seen += int(1 <= c[i] < L[i])
    assert seen > 0


@pytest.mark.parametrize("name", IDENTITY_CASES + ("zero", "dup"))
def test_list_length_is_the_first_padding_rank(name, oracle):
    x, q, S = scores(name, oracle)
    nq, n = S.shape
    L = at_rank_ref.list_len(S)
    D, I = at_rank_ref.entries_at_from_scores(S, np.stack([L - 1, L, L + 1, np.full(nq, -1)], 1))
    assert (I[L > 0, 0] >= 0).all() and (I[:, 1:] == -1).all() and (D[:, 1:] == -FMAX).all()
    keys = at_rank_ref.entry_keys_from_scores(S, np.stack([L - 1, L], 1))
    assert (keys[L > 0, 0] != 0).all() and (keys[:, 1] == 0).all()


def test_keys_of_all_ranks_are_the_sorted_key_list(oracle):
    x, q, S = scores("hostile96", oracle)
    nq, n = S.shape
    for pos_base in (0, 2 ** 24 - 500, 2 ** 32 - 1 - n):
        keys = at_rank_ref.entry_keys_from_scores(S, np.tile(np.arange(n, dtype=np.int64), (nq, 1)), pos_base)
        np.testing.assert_array_equal(keys, after_ref.after_from_keys(S, None, pos_base, n))


# ---------------------------------------------------------------------------------------------------------------------
# the inputs do what they claim
@pytest.mark.parametrize("d", cases.HOSTILE_DS)
def test_hostile_case_holds_nan_inf_and_flt_max_scoring_rows(d, oracle):
    x, q, S = scores(f"hostile{d}", oracle)
    assert (q[0] == 0).all() and (q[3] == -q[2]).all()
    assert np.isnan(S).any(axis=1).all()                                        # NaN-scoring rows for every query
    assert S[2, cases.ROW_PINF] == np.inf and S[2, cases.ROW_NINF] == -np.inf
    assert S[3, cases.ROW_PINF] == -np.inf and S[3, cases.ROW_NINF] == np.inf
    assert after_ref.bits(S[2, cases.ROW_NFMAX]) == after_ref.bits(np.float32(-FMAX))      # exactly -FLT_MAX: a real row
    L = at_rank_ref.list_len(S)
    assert (L < S.shape[1]).all() and (L > 900).all()
    D, I = at_rank_ref.entries_at_from_scores(S[2:3], cases.all_ranks(1, S.shape[1]))
    at = np.flatnonzero(I[0] == cases.ROW_NFMAX)
    assert len(at) == 1 and D[0, at[0]] == -FMAX                                # ... listed with its id, unlike padding
    assert D[0, 2] == np.inf and D[0, 2 + L[2] - 1] == -np.inf and I[0, 2 + L[2]] == -1   # (ranks start at -2) both ends of the list
    # the zero query: every listed score is +0
    assert (S[0][~np.isnan(S[0])] == 0).all() and (after_ref.bits(S[0][~np.isnan(S[0])]) == 0).all()
    # more than 3000 pairs at nq = 3: several launches of 1024 and a partial last tile
    pairs = 3 * cases.all_ranks(3, S.shape[1]).shape[1]
    assert pairs > 3000 and pairs > 2 * 1024 and pairs % 1024 % 16 != 0


def test_tie_runs_span_the_position_digit_edges(oracle):
    x, q, S = scores("zero", oracle)
    assert S.shape == (1, cases.TIE_N) and (after_ref.bits(S) == 0).all()        # every score +0: the entry at rank t is row t
    ranks = np.array([cases.TIE_RANKS], np.int64)
    D, I = at_rank_ref.entries_at_from_scores(S, ranks)
    inside = (ranks >= 0) & (ranks < cases.TIE_N)
    np.testing.assert_array_equal(I[inside], ranks[inside])
    assert (I[~inside] == -1).all() and inside.sum() == len(cases.TIE_RANKS) - 2
    low = lambda r: 0xFFFFFFFF - r                                                # the key's low word
    for a, b, widths in ((255, 256, (8,)), (65535, 65536, (8, 11))):
        assert a in cases.TIE_RANKS and b in cases.TIE_RANKS
        for bits_ in widths:                                                      # a digit ABOVE the lowest changes between the two
            assert low(a) >> bits_ != low(b) >> bits_
    assert low(65535) >> 16 != low(65536) >> 16 and low(65535) >> 22 == low(65536) >> 22
    assert at_rank_ref.passes(0, cases.TIE_N) == 7

    # duplicated rows: the asked rows sit inside runs of equal scores that straddle the edges named
    x, q, S = scores("dup", oracle)
    rows = cases.tie_dup_rows()
    from tests.test_search_plans_gpu import _cuts
    c1, c2 = _cuts(cases.TIE_N)
    for e in (c1, c2, 6400, 1792, 65536):
        assert (x[e - 2:e + 2] == x[e]).all() and e - 2 in rows and e + 1 in rows
        assert (after_ref.bits(S[:, e - 2:e + 2]) == after_ref.bits(S[:, e:e + 1])).all()
    assert c1 % 64 and c2 % 64 and 6400 % 64 == 0 and 1792 % 256 == 0
    for i in range(len(q)):
        assert len(np.unique(S[i])) <= 16
    r = rank_ref.rank_ids_from_scores(S, np.tile(rows, (len(q), 1)))
    assert (r >= 0).all()
    np.testing.assert_array_equal(at_rank_ref.entries_at_from_scores(S, r)[1], np.tile(rows, (len(q), 1)))


def test_grid_case_puts_the_score_digit_edges_into_one_ranking(oracle):
    x, q, S = scores("grid", oracle)
    grid = (np.abs(x) >= 0.125) & (np.abs(x) < 2.0 ** 22)
    assert (x[grid] * 8 == np.round(x[grid] * 8)).all() and grid.sum() >= 150     # grid-valued, but for the specials
    ok = ~np.isnan(S[0])
    np.testing.assert_array_equal(after_ref.bits(S[0][ok]), after_ref.bits((x[:, 0] + np.float32(0))[ok]))    # the scores ARE the values
    o = np.unique(after_ref.pack(S[0][ok], 0) >> np.uint64(32)).astype(np.int64)
    assert (np.diff(o) == 1).sum() >= 16                                        # adjacent floats, many pairs
    b21 = int(after_ref.pack(np.array([2.0 ** 21], np.float32), 0)[0] >> np.uint64(32))
    assert b21 in o and b21 - 1 in o and b21 & 0xFFFFFF == 0                    # 2^21 - 1/8 | 2^21: every lower score digit rolls over
    xb = after_ref.bits(x[:, 0])
    assert (xb == 0x80000000).any() and (xb == 0).any()                         # rows of -0.0 and of +0.0 ...
    assert (after_ref.bits(S[0][(xb == 0x80000000) | (xb == 0)]) == 0).all()    # ... tie at +0.0
    assert not (after_ref.bits(S) == 0x80000000).any()
    for v in (np.inf, -np.inf, FMAX, -FMAX):
        assert (S[0] == np.float32(v)).any() and (S[1] == np.float32(v)).any()
    den = np.abs(S[0][(S[0] != 0) & ~np.isnan(S[0])]) < np.finfo(np.float32).tiny
    assert den.sum() >= 4 * 9                                                    # denormals of both signs, not flushed
    D, I = at_rank_ref.entries_at_from_scores(S, cases.all_ranks(3, cases.GRID_N))
    assert ((D == -FMAX) & (I >= 0)).any(axis=1)[:2].all()                     # -FLT_MAX as a real entry ...
    assert ((D == -FMAX) & (I == -1)).any(axis=1).all()                        # ... and as padding, in one answer
    assert np.isnan(S[2]).sum() >= 3 * 9 and (S[2][~np.isnan(S[2])] == 0).all()


def test_search_at_starts_cover_both_ends(oracle):
    x, q, S = scores("at", oracle)
    L = at_rank_ref.list_len(S)
    start = cases.at_starts(L)
    assert (L > 3000 + 2048).all() and (L < cases.AT_N).all()
    assert start[4] == L[4] - 1 and start[5] == L[5] and start[6] == L[6] + 5
    for k in cases.AT_KS:
        D, I = at_rank_ref.search_at_from_scores(S, start, k)
        assert (I[0] >= 0).all() and I[4, 0] >= 0 and (I[4, 1:] == -1).all() and (I[5:] == -1).all()
        after_ref.assert_same((D[:1], I[:1]), oracle.flat_ip_search(x, q[:1], k), "start 0 is search")


def test_documented_pass_count():
    p = at_rank_ref.passes
    assert [p(0, n) for n in (1, 2, 256, 257, 1000, 65536, 65537, 66000, 2 ** 24, 2 ** 24 + 1, 2 ** 32 - 1)] == [4, 5, 5, 6, 6, 6, 7, 7, 7, 8, 8]
    assert p(2 ** 24 - 500, 1000) == 8 and p(2 ** 32 - 1 - 1000, 1000) == 6 and p(2 ** 24, 256) == 5 and p(255, 2) == 6


# ---------------------------------------------------------------------------------------------------------------------
# argument checks (no handle)
def test_rank_args_pass_good_arguments_through():
    from haconvdr_amd import index
    q, r = index._rank_args(np.zeros((3, 96), np.float64), np.full((3, 5), -7, np.int32), 96)
    assert q.dtype == np.float32 and r.dtype == np.int64 and r.shape == (3, 5) and r.flags.c_contiguous and (r == -7).all()
    assert index._rank_args(np.zeros((3, 96)), np.zeros((3, 0), np.int64), 96)[1].shape == (3, 0)
    assert index._rank_args(np.zeros((0, 96)), np.zeros((0, 4), np.int64), 96)[0].shape == (0, 96)
    assert index._rank_args(np.zeros((1, 96)), np.array([[2 ** 62, -2 ** 62]]), 96)[1].tolist() == [[2 ** 62, -2 ** 62]]   # values, not ids
    np.testing.assert_array_equal(index._as_start(5, 3, "search_at"), [5, 5, 5])
    np.testing.assert_array_equal(index._as_start(np.array([0, 2, 9], np.int32), 3, "search_at"), [0, 2, 9])
    assert index._as_pos_base(2 ** 32 - 1, "x") == 2 ** 32 - 1


@pytest.mark.parametrize("q, ranks", [
    (np.zeros((3, 96)), np.zeros((3, 5), np.float32)),       # float ranks
    (np.zeros((3, 96)), np.zeros((3, 5), np.bool_)),
    (np.zeros((3, 96)), np.zeros(5, np.int64)),              # one list, not one per query
    (np.zeros((3, 96)), np.zeros((3, 5, 1), np.int64)),
    (np.zeros((3, 96)), np.zeros((2, 5), np.int64)),         # ranks.shape[0] != nq
    (np.zeros((3, 95)), np.zeros((3, 5), np.int64)),         # wrong dimension
    (np.zeros(96), np.zeros((1, 5), np.int64)),
    (np.zeros((3, 96)), np.array([[2 ** 63] * 2] * 3, np.uint64)),
])
def test_rank_args_raise_value_error(q, ranks):
    from haconvdr_amd import index
    with pytest.raises(ValueError):
        index._rank_args(q, ranks, 96)


@pytest.mark.parametrize("start", [-1, np.array([0, -3, 1]), 1.0, np.array([0.0, 1.0, 2.0]), True, np.zeros(2, np.int64),
                                   np.zeros((3, 1), np.int64), np.array([2 ** 63] * 3, np.uint64), None])
def test_search_at_start_raises_value_error(start):
    from haconvdr_amd import index
    with pytest.raises(ValueError):
        index._as_start(start, 3, "search_at")


def test_methods_raise_before_the_library_is_called():
    """a FlatIPIndex without a handle: a mistake in the arguments never reaches the C ABI"""
    from haconvdr_amd.index import FlatIPIndex
    idx = object.__new__(FlatIPIndex)
    idx.d, idx.devices, idx._h = 96, (0,), None
    q = np.zeros((3, 96), np.float32)
    with pytest.raises(ValueError):
        idx.entries_at(q, np.zeros((3, 5), np.float64))
    with pytest.raises(ValueError):
        idx.entries_at(q, np.zeros((2, 5), np.int64))
    with pytest.raises(ValueError):
        idx.search_at(q, 10, -1)
    with pytest.raises(ValueError):
        idx.search_at(q, 0, 0)
    with pytest.raises(ValueError):
        idx.search_at(q, 10, np.array([0.5, 1, 2]))


def test_tensor_checks_refuse_host_tensors_and_bad_pos_base():
    """The tensor forms hand raw device pointers to kernels: a CPU tensor or an ndarray must never get there."""
    import torch
    from haconvdr_amd import index
    with pytest.raises(ValueError):
        index._rank_args_tensor(torch.zeros(3, 96), torch.zeros(3, 5, dtype=torch.int64), 96)
    with pytest.raises(ValueError):
        index._rank_args_tensor(np.zeros((3, 96), np.float32), np.zeros((3, 5), np.int64), 96)
    with pytest.raises(ValueError):
        index._start_tensor(torch.zeros(3, dtype=torch.int64), torch.zeros(3, 96), "search_at_tensor")      # a host tensor
    for bad in (-1, 2 ** 32, 1.0, True):
        with pytest.raises(ValueError):
            index._as_pos_base(bad, "entry_keys_at_tensor")
