"""search_among: hac_index_search_among* (the among_* kernels of csrc/among.inc) through FlatIPIndex, i.e. the C ABI.

Every assertion is equality of I and of the bits of D with tests/among_ref.py, the definition of include/haconvdr.h restated
over the CPU oracle's canonical scores.  Indexes are built like _index() of tests/test_search_plans_gpu.py: three adds cut off
the 64-row grid, so the rows straddle segments and the last group is partial.  Every case checks the host form and the tensor
form and leaves the status word clean."""
import re

import numpy as np
import pytest

from haconvdr_amd import synth
from tests import among_ref, nonfinite, rank_ref
from tests.golden import cases
from tests.test_index_rank_gpu import hostile_queries
from tests.test_index_rows_gpu import hostile_corpus
from tests.test_search_plans_gpu import _index

pytestmark = pytest.mark.gpu

HAC_ERR_INVALID, HAC_ERR_UNSUPPORTED = 1, 4
MAX_K, MAX_AMONG = 2048, 4096
_PLAN = re.compile(r"^among_keys_kernel grid=(?P<grid>\d+) among_select_kernel P=(?P<P>\d+) k=(?P<k>\d+) lds=(?P<lds>\d+)$")


def parse_plan(text):
    m = _PLAN.match(text)
    assert m, "not the plan of a search among named rows: %r" % text
    return {k: int(v) for k, v in m.groupdict().items()}


def _cuda(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def tensor_form(idx, q, cand, k, id_map=None):
    """(D, I) of search_among_tensor as ndarrays"""
    import torch
    D, I = idx.search_among_tensor(_cuda(q, np.float32), k, _cuda(cand, np.int64), id_map=id_map)
    torch.cuda.synchronize()
    return D.cpu().numpy(), I.cpu().numpy()


def both_forms(idx, q, cand, k, want, what=""):
    """host form and tensor form against the reference; the status word stays clean"""
    among_ref.assert_same(idx.search_among(q, k, cand), want, f"{what} host form")
    among_ref.assert_same(tensor_form(idx, q, cand, k), want, f"{what} tensor form")
    idx.check_status()


def _distinct(seed, nq, n, m):
    """per query m distinct rows of [0, n), in a random order"""
    return np.stack([np.argsort(synth.uniform_u32(seed + i, n), kind="stable")[:m] for i in range(nq)]).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# 1. list lengths at the edges of P (the LDS sort's power of two) and of the key kernel's 256-candidate workgroup
_SWEEP = {}


def _sweep_case(oracle):
    if not _SWEEP:
        n, d, nq = 5000, 96, 3
        x, q, _ = cases.search_case_inputs("gauss", 0x8A0, n, nq, d=d)
        _SWEEP["case"] = (x, q, rank_ref.canon_scores(oracle, x, q))
    return _SWEEP["case"]


@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257, 4095, 4096])
def test_list_lengths_at_the_sort_and_workgroup_edges(m, oracle):
    x, q, S = _sweep_case(oracle)
    nq, n = S.shape
    cand = _distinct(0x8A1 + m, nq, n, m)
    if m >= 3:
        cand[1, m // 2] = -1                          # padding in the middle of a list
        cand[2, 0] = cand[2, m - 1]                   # a row named at both ends
    idx = _index(96, x)
    ks = sorted({1, max(1, m - 1), m, m + 1} | ({MAX_K} if m >= MAX_K else set()))
    for k in ks:
        if k > MAX_K:                                 # beyond the ceiling: refused before the library is called
            with pytest.raises(ValueError):
                idx.search_among(q, k, cand)
            continue
        want = among_ref.among_from_scores(S, cand, k)
        assert (want[1][0, :min(k, m)] >= 0).all() and (want[1][0, m:] == -1).all()
        both_forms(idx, q, cand, k, want, f"m={m} k={k}")
        plan = parse_plan(idx.last_plan())
        P = 1 << (m - 1).bit_length()
        assert plan == {"grid": nq * ((m + 255) // 256), "P": P, "k": k, "lds": P * 8 + 32}, plan


def test_no_candidates_is_padding_only():
    import torch
    d, nq, k = 96, 5, 7
    x = synth.embeddings(0x8B0, 300, d)
    q = synth.embeddings(0x8B1, nq, d)
    idx = _index(d, x)
    want = (np.full((nq, k), -among_ref.FMAX, np.float32), np.full((nq, k), -1, np.int64))
    both_forms(idx, q, np.zeros((nq, 0), np.int64), k, want, "m=0")
    both_forms(idx, q, np.full((nq, 9), -1, np.int64), k, want, "only padding")
    # nq == 0: HAC_OK, nothing touched
    D, I = idx.search_among(np.zeros((0, d), np.float32), k, np.zeros((0, 4), np.int64))
    assert D.shape == I.shape == (0, k)
    D, I = idx.search_among_tensor(torch.zeros((0, d), device="cuda"), k, torch.zeros((0, 4), dtype=torch.int64, device="cuda"))
    assert tuple(D.shape) == tuple(I.shape) == (0, k)
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 2. repeats and ties
def _tie_corpus(d, n, nq, seed):
    """16 distinct grid-valued rows repeated and interleaved, integer queries: every score is exact and shared by dozens of rows"""
    base = ((synth.uniform_u32(seed, 16 * d) % np.uint32(17)).astype(np.float32).reshape(16, d) - 8.0) / 8.0
    x = base[np.arange(n) % 16]
    q = (synth.uniform_u32(seed + 1, nq * d) % np.uint32(9)).astype(np.float32).reshape(nq, d) - 4.0
    q[0] = 0.0
    return x, q


def test_repeats_and_ties(oracle):
    d, n, nq = 96, 1000, 6
    x, q = _tie_corpus(d, n, nq, 0x8C0)
    S = rank_ref.canon_scores(oracle, x, q)
    assert all(len(np.unique(S[i])) <= 16 for i in range(nq))
    idx = _index(d, x)
    # every candidate the same row
    cand = np.full((nq, 300), 77, np.int64)
    want = among_ref.among_from_scores(S, cand, 5)
    assert (want[1][:, 0] == 77).all() and (want[1][:, 1:] == -1).all()
    both_forms(idx, q, cand, 5, want, "one row 300 times")
    # a repeat straddles position k: the rows in descending order, each named twice in a row; k odd and even
    for k in (10, 11):
        order = among_ref.among_from_scores(S, np.tile(np.arange(200), (nq, 1)), 200)[1]
        cand = np.repeat(order, 2, axis=1)
        want = among_ref.among_from_scores(S, cand, k)
        np.testing.assert_array_equal(want[1], order[:, :k])
        both_forms(idx, q, cand, k, want, f"repeats straddle k={k}")
    # the tie corpus: equal scores ascend by row, and a tie is cut at k
    cand = _distinct(0x8C2, nq, n, 500)
    for k in (37, 499):
        want = among_ref.among_from_scores(S, cand, k)
        wD, wI = want
        same = np.diff(wD, axis=1) == 0
        assert same.sum() > nq * k // 2 and (np.diff(wI, axis=1)[same] > 0).all()
        full = among_ref.among_from_scores(S, cand, 500)
        assert sum(full[0][i, k - 1] == full[0][i, k] for i in range(nq)) >= nq - 1       # the cut falls inside a tie
        both_forms(idx, q, cand, k, want, f"ties k={k}")
    np.testing.assert_array_equal(among_ref.among_from_scores(S[:1], cand[:1], 500)[1][0], np.sort(cand[0]))    # the zero query: row order


# ---------------------------------------------------------------------------------------------------------------------
# 3. ids outside the rows
def test_ids_outside_the_rows(oracle):
    import torch
    from haconvdr_amd import _lib
    from haconvdr_amd.index import _f32p, _i64p
    d, n, nq, m, k = 96, 1000, 4, 70, 20
    x = hostile_corpus(0x8D0, n, d)
    q = hostile_queries(0x8D1, nq, d)
    S = rank_ref.canon_scores(oracle, x, q)
    idx = _index(d, x)
    cand = _distinct(0x8D2, nq, n, m)
    cand[:, 31] = -1                                  # padding in the middle of every list
    want = among_ref.among_from_scores(S, cand, k)
    both_forms(idx, q, cand, k, want, "-1 in the middle")
    # the tensor form ignores every id outside [0, ntotal); the host form refuses the first one that is not -1
    wild = cand.copy()
    wild[0, 3], wild[1, 0], wild[2, 69], wild[3, 40] = n, -2, 2 ** 40, np.iinfo(np.int64).min
    wild[2, 5] = n + 63                               # inside the last group's allocation, behind ntotal
    want_wild = among_ref.among_from_scores(S, wild, k)
    among_ref.assert_same(tensor_form(idx, q, wild, k), want_wild, "ids outside the rows, tensor form")
    D = np.full((nq, k), np.float32(-123.5))
    I = np.full((nq, k), -99, np.int64)
    one = cand.copy()
    one[2, 5] = n
    with pytest.raises(_lib.HacError) as err:
        _lib.check(_lib.lib().hac_index_search_among(idx._h, _f32p(q), nq, k, _i64p(one), m, _f32p(D), _i64p(I)))   # the caller's D and I
    assert err.value.code == HAC_ERR_INVALID
    assert f"id {n} " in str(err.value) and "(query 2, column 5)" in str(err.value), str(err.value)
    assert (D == np.float32(-123.5)).all() and (I == -99).all()
    for bad in (-2, n + 5):
        one[2, 5] = bad
        with pytest.raises(_lib.HacError) as err:
            idx.search_among(q, k, one)
        assert err.value.code == HAC_ERR_INVALID and f"id {bad} " in str(err.value)
    # argument mistakes on real CUDA tensors: ValueError before the library is called
    qt, ct = _cuda(q, np.float32), _cuda(cand, np.int64)
    for args in ((qt, 0, ct), (qt, MAX_K + 1, ct), (qt, k, ct[:-1]), (qt, k, ct[0]), (qt, k, ct.to(torch.int32)), (qt, k, ct.cpu()),
                 (qt, k, torch.zeros((nq, MAX_AMONG + 1), dtype=torch.int64, device="cuda"))):
        with pytest.raises(ValueError):
            idx.search_among_tensor(*args)
    # ... and the library's own check of k and m (the C ABI called directly)
    rc = _lib.lib().hac_index_search_among_device(idx._h, qt.data_ptr(), nq, k, ct.data_ptr(), MAX_AMONG + 1, None, None, None, None)
    msg = _lib.lib().hac_last_error().decode()
    assert rc == HAC_ERR_INVALID and f"k={k}" in msg and f"m={MAX_AMONG + 1}" in msg and str(MAX_AMONG) in msg, msg
    rc = _lib.lib().hac_index_search_among_device(idx._h, qt.data_ptr(), nq, MAX_K + 1, ct.data_ptr(), m, None, None, None, None)
    assert rc == HAC_ERR_INVALID and f"k={MAX_K + 1}" in _lib.lib().hac_last_error().decode()
    among_ref.assert_same(tensor_form(idx, q, cand, k), want, "after the refused calls")
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 4. dimensions, on hostile rows (NaN, Inf, denormals, -0.0) and hostile queries
@pytest.mark.parametrize("d", [32, 96, 768, 1024])
def test_dimensions_on_hostile_rows(d, oracle):
    n, nq, m = 1000, 17, 300
    x = hostile_corpus(0x8E0 + d, n, d)
    q = hostile_queries(0x8E1 + d, nq, d)
    S = rank_ref.canon_scores(oracle, x, q)
    cand = _distinct(0x8E2 + d, nq, n, m)
    cand[:, :40] = np.arange(3, 403, 10)              # forty of the raw-word rows: NaN scores among the candidates
    assert np.isnan(np.take_along_axis(S, cand, 1)).any()
    idx = _index(d, x)
    for k in (1, 100, m):
        want = among_ref.among_from_scores(S, cand, k)
        assert not np.isnan(want[0]).any()
        both_forms(idx, q, cand, k, want, f"d={d} k={k}")


# ---------------------------------------------------------------------------------------------------------------------
# 5. index states
def test_after_remove_and_after_reset(oracle):
    d, n, nq, m, k = 96, 1000, 5, 200, 50
    x = synth.embeddings(0x8F0, n, d)
    q = synth.embeddings(0x8F1, nq, d)
    idx = _index(d, x)
    cand = _distinct(0x8F2, nq, n, m)
    both_forms(idx, q, cand, k, among_ref.among(oracle, x, q, cand, k), "as built")
    gone = np.arange(100, 900, 7)
    assert idx.remove_ids(gone) == len(gone)
    left = np.delete(x, gone, 0)
    cand2 = _distinct(0x8F3, nq, len(left), m)
    both_forms(idx, q, cand2, k, among_ref.among(oracle, left, q, cand2, k), "after remove_ids")
    # reset() and a smaller add(): the stale rows behind the new ntotal are unreachable
    idx.reset()
    small = synth.embeddings(0x8F4, 130, d)
    idx.add(small)
    cand3 = np.tile(np.arange(m), (nq, 1)).astype(np.int64)          # names rows 130 .. 199 too: they were rows once
    want = among_ref.among(oracle, small, q, cand3, k + 100)
    assert (want[1][:, :130] >= 0).all() and (want[1][:, 130:] == -1).all() and want[1].max() < 130
    among_ref.assert_same(tensor_form(idx, q, cand3, k + 100), want, "after reset and a smaller add")
    cand3[cand3 >= 130] = -1
    both_forms(idx, q, cand3, k + 100, want, "after reset and a smaller add")


def test_same_bits_from_the_tiles_and_from_the_row_major_copy(oracle):
    d, n, nq, m, k = 768, 5000, 32, 300, 100
    x = synth.embeddings(0x900, n, d)
    q = synth.embeddings(0x901, nq, d)
    idx = _index(d, x, split="1", rescore_rows="1", fp16_image="eager")
    cand = (synth.uniform_u32(0x902, nq * m) % np.uint32(n)).astype(np.int64).reshape(nq, m)       # with repeats
    want = among_ref.among(oracle, x, q, cand, k)
    both_forms(idx, q, cand, k, want, "before any search: tiles")
    for _ in range(2):
        idx.search(q, 10)
    assert "rescore=rows" in idx.last_plan(), idx.last_plan()
    both_forms(idx, q, cand, k, want, "row-major copy current")
    idx.set_option("rescore_rows", "0")
    idx.search(q, 10)
    assert "rescore=tiles" in idx.last_plan(), idx.last_plan()
    both_forms(idx, q, cand, k, want, "copy freed: tiles")


# ---------------------------------------------------------------------------------------------------------------------
# 6. the identities of include/haconvdr.h
@pytest.mark.parametrize("split", ["0", "1"])
def test_among_the_rows_of_a_search_is_that_search(split, oracle):
    d, n, nq, kp = 768, 3001, 64, 100
    x, q, _ = cases.search_case_inputs("dup", 0x910, n, nq, d=d)      # twin rows: every score is a tie of two
    idx = _index(d, x, split=split)
    D, I = idx.search(q, kp)
    assert idx.last_plan().startswith("split:") == (split == "1"), idx.last_plan()
    oD, oI = oracle.flat_ip_search(x, q, kp)
    among_ref.assert_same((D, I), (oD, oI), "search")
    rng = np.random.default_rng(0x911)
    cand = np.stack([rng.permutation(np.concatenate([I[i], I[i, ::3], np.full(7, -1)])) for i in range(nq)]).astype(np.int64)
    for k in (1, 50, kp):
        both_forms(idx, q, cand, k, (D[:, :k], I[:, :k]), f"split={split} k={k}")
    # D has the bits score_ids gives the rows I names
    import torch
    aD, aI = tensor_form(idx, q, cand, kp + 5)
    assert (aI[:, kp:] == -1).all()
    sD = idx.score_ids_tensor(_cuda(q, np.float32), _cuda(aI, np.int64))
    torch.cuda.synchronize()
    named = aI >= 0
    np.testing.assert_array_equal(among_ref.bits(aD)[named], among_ref.bits(sD.cpu().numpy())[named])
    np.testing.assert_array_equal(among_ref.bits(aD)[named], among_ref.bits(idx.score_ids(q, aI))[named])


# ---------------------------------------------------------------------------------------------------------------------
# 7. non-finite queries next to healthy ones
@pytest.mark.parametrize("kind", nonfinite.KINDS)
def test_nonfinite_queries(kind, oracle):
    d, n, nq, m, k = 96, 3001, 33, 400, 100
    x, q, pos, _ = nonfinite.case(kind, d, n, nq, 0x920)
    with np.errstate(all="ignore"):
        S = rank_ref.canon_scores(oracle, x, q)
    cand = _distinct(0x921, nq, n, m)
    want = among_ref.among_from_scores(S, cand, k)
    if kind in nonfinite.NAN_KINDS:
        assert all((want[1][i] == -1).all() for i in pos)             # a NaN query: padding only
    if kind in nonfinite.INF_KINDS:
        assert all(np.isinf(want[0][i]).any() for i in pos)           # +-Inf are ordinary scores
    healthy = [i for i in range(nq) if i not in pos]
    assert (want[1][healthy] >= 0).all()
    idx = _index(d, x)
    both_forms(idx, q, cand, k, want, kind)


# ---------------------------------------------------------------------------------------------------------------------
# 8. many queries, determinism, the plan, the keys form
def test_many_queries_with_short_lists(oracle):
    d, n, nq, m, k = 96, 1000, 1025, 9, 5
    x = synth.embeddings(0x930, n, d)
    q = synth.embeddings(0x931, nq, d)
    cand = (synth.uniform_u32(0x932, nq * m) % np.uint32(n + 1)).astype(np.int64).reshape(nq, m) - 1     # -1 .. n - 1, with repeats
    idx = _index(d, x)
    both_forms(idx, q, cand, k, among_ref.among(oracle, x, q, cand, k), "nq=1025")
    assert parse_plan(idx.last_plan()) == {"grid": nq, "P": 16, "k": k, "lds": 16 * 8 + 32}


def test_past_one_chunk_of_the_key_workspace_and_of_the_host_staging(oracle):
    """The [queries][P] candidate keys are produced 64 MiB at a time (2048 queries at P = 4096), and the host form stages
    queries and lists ~64 MiB at a time (2040 queries at d = 32, m = 4096): 2049 queries cross both edges."""
    d, n, nq, m, k = 32, 5000, 2049, 4096, 3
    x = synth.embeddings(0x938, n, d)
    q = synth.embeddings(0x939, nq, d)
    cand = (synth.uniform_u32(0x93A, nq * m) % np.uint32(n + 1)).astype(np.int64).reshape(nq, m) - 1
    idx = _index(d, x)
    both_forms(idx, q, cand, k, among_ref.among(oracle, x, q, cand, k), "nq=2049 m=4096")
    assert parse_plan(idx.last_plan()) == {"grid": 2048 * 16, "P": 4096, "k": k, "lds": 4096 * 8 + 32}


def test_two_identical_calls_return_identical_bytes():
    import torch
    d, n, nq, m, k = 96, 3000, 40, 1000, 300
    x, q = _tie_corpus(d, n, nq, 0x940)
    idx = _index(d, x)
    cand = _cuda((synth.uniform_u32(0x942, nq * m) % np.uint32(n)).astype(np.int64).reshape(nq, m), np.int64)
    qt = _cuda(q, np.float32)
    a = idx.search_among_tensor(qt, k, cand)
    b = idx.search_among_tensor(qt, k, cand)
    ka = idx.search_among_keys_tensor(qt, k, cand, pos_base=5)
    kb = idx.search_among_keys_tensor(qt, k, cand, pos_base=5)
    torch.cuda.synchronize()
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(ka, kb)
    h1, h2 = idx.search_among(q, k, cand.cpu().numpy()), idx.search_among(q, k, cand.cpu().numpy())
    assert h1[0].tobytes() == h2[0].tobytes() and h1[1].tobytes() == h2[1].tobytes()
    among_ref.assert_same(h1, (a[0].cpu().numpy(), a[1].cpu().numpy()), "host form vs tensor form")


def test_keys_form_feeds_merge_keys_and_keys_to_results(oracle):
    """Two indexes hold the two halves of a corpus; each selects among the candidates it holds with pos_base = its first row:
    merged, the keys are those of one index over the whole corpus."""
    import torch
    from haconvdr_amd.index import keys_to_results, merge_keys
    d, n, nq, m, k = 96, 1501, 7, 200, 60
    x, q, ids = cases.search_case_inputs("dup", 0x950, n, nq, d=d)    # row r and row r + 750 are twins: ties cross the cut
    cut = 751
    cand = _distinct(0x951, nq, n, m)
    cand[:, :40] = np.concatenate([np.arange(20), np.arange(20) + 750])[None, :]
    cand[:, 50] = -1
    lo, hi = _index(d, x[:cut]), _index(d, x[cut:])
    qt = _cuda(q, np.float32)
    mine = lambda a, b: _cuda(np.where((cand >= a) & (cand < b), cand - a, -1), np.int64)     # noqa: E731
    k_lo = lo.search_among_keys_tensor(qt, k, mine(0, cut), pos_base=0)
    k_hi = hi.search_among_keys_tensor(qt, k, mine(cut, n), pos_base=cut)
    D, I = keys_to_results(merge_keys(torch.stack([k_lo, k_hi])), id_map=_cuda(ids, np.int64))
    torch.cuda.synchronize()
    wD, wI = among_ref.among(oracle, x, q, cand, k)
    assert any(wD[i, j] == wD[i, j + 1] and wI[i, j] < cut <= wI[i, j + 1] for i in range(nq) for j in range(k - 1))
    among_ref.assert_same((D.cpu().numpy(), I.cpu().numpy()), (wD, ids[wI]), "two shards merged")
    # id_map through the tensor form of one index
    whole = _index(d, x)
    among_ref.assert_same(tensor_form(whole, q, cand, k, id_map=_cuda(ids, np.int64)), (wD, ids[wI]), "id_map")
    for i in (lo, hi, whole):
        i.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 9. several shards in one process
@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)])
def test_multi_device_index(devices, oracle):
    from haconvdr_amd import _lib
    d, n, nq, m, k = 96, 1501, 9, 300, 80
    x, q, _ = cases.search_case_inputs("dup", 0x960, n, nq, d=d)      # twins 750 rows apart: they land on different shards
    idx = _index(d, x, devices=devices)
    cand = _distinct(0x961, nq, n, m)
    cand[:, :40] = np.concatenate([np.arange(20), np.arange(20) + 750])[None, :]
    cand[:, 60], cand[:, 61] = -1, cand[:, 0]
    for kk in (1, k, m + 3):
        want = among_ref.among(oracle, x, q, cand, kk)
        among_ref.assert_same(idx.search_among(q, kk, cand), want, f"{len(devices)} shards k={kk}")
    assert any(want[0][i, j] == want[0][i, j + 1] for i in range(nq) for j in range(40))
    among_ref.assert_same(idx.search_among(q, 4, np.zeros((nq, 0), np.int64)), among_ref.among(oracle, x, q, np.zeros((nq, 0), np.int64), 4), "m=0")
    bad = cand.copy()
    bad[1, 2] = n
    with pytest.raises(_lib.HacError) as err:
        idx.search_among(q, k, bad)
    assert err.value.code == HAC_ERR_INVALID and "(query 1, column 2)" in str(err.value)
    qt, ct = _cuda(q, np.float32), _cuda(cand, np.int64)
    for call in (lambda: idx.search_among_tensor(qt, k, ct), lambda: idx.search_among_keys_tensor(qt, k, ct)):
        with pytest.raises(_lib.HacError) as err:
            call()
        assert err.value.code == HAC_ERR_UNSUPPORTED
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 10. captured into a graph
def test_captured_into_a_graph_replays_on_new_candidates(oracle):
    import torch
    d, n, nq, m, k = 96, 1000, 17, 257, 64
    x = hostile_corpus(0x970, n, d)
    qs = [hostile_queries(0x971 + r, nq, d) for r in range(2)]
    cands = [_distinct(0x973 + 100 * r, nq, n, m) for r in range(2)]
    for c in cands:
        c[0, 0], c[1, 1], c[2, 2] = -1, n, c[2, 3]     # padding, an id past the end and a repeat in every replay
    wants = [among_ref.among(oracle, x, qs[r], cands[r], k) for r in range(2)]
    idx = _index(d, x)
    qt, ct = _cuda(qs[0], np.float32), _cuda(cands[0], np.int64)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()                            # a single stream: no parallel branches in the graph
    replayed = []
    with torch.cuda.stream(side):
        eager = idx.search_among_tensor(qt, k, ct)        # the largest shape once: workspaces and the segment table exist
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            D, I = idx.search_among_tensor(qt, k, ct)
        for r in (1, 0, 1):
            qt.copy_(torch.from_numpy(qs[r]))
            ct.copy_(torch.from_numpy(cands[r]))
            D.zero_()
            I.fill_(-7)
            g.replay()
            side.synchronize()
            replayed.append((r, D.cpu().numpy(), I.cpu().numpy()))
    torch.cuda.synchronize()
    among_ref.assert_same((eager[0].cpu().numpy(), eager[1].cpu().numpy()), wants[0], "eager")
    for r, D, I in replayed:
        among_ref.assert_same((D, I), wants[r], f"replay on contents {r}")
    idx.check_status()
