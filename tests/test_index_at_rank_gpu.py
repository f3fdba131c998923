"""Entry at a rank: hac_index_entries_at* (rank_hist_kernel, rank_narrow_kernel of csrc/at_rank.inc) and search_at through
FlatIPIndex and ResidentCorpus, i.e. the C ABI.

Every assertion is equality with tests/at_rank_ref.py, the definition of include/haconvdr.h restated over the CPU oracle's
canonical scores: I as integers, D by bits.  tests/test_index_at_rank.py proves on the CPU that the inputs (tests/at_rank_cases.py)
show what they are for.  Indexes are built like _index() of tests/test_search_plans_gpu.py: three adds cut off the 64-row grid,
so the last group is partial and its tail rows must never be listed."""
import os
import re

import numpy as np
import pytest

from haconvdr_amd import synth
from tests import after_ref, at_rank_cases as cases, at_rank_ref, nonfinite, range_ref, rank_ref
from tests.test_index_rank_gpu import hostile_queries
from tests.test_index_rows_gpu import hostile_corpus
from tests.test_search_plans_gpu import _index

pytestmark = pytest.mark.gpu

FMAX = after_ref.FMAX
HAC_ERR_UNSUPPORTED = 4
_PLAN = re.compile(r"^rank_hist_kernel<BITS=(?P<BITS>\d+)> grid=\((?P<P>\d+),(?P<T>\d+)\) QT=(?P<QT>\d+) passes=(?P<passes>\d+) lds=(?P<lds>\d+)$")
_CASES = {}


def parse_plan(text):
    m = _PLAN.match(text)
    assert m, "not the plan of an entries_at call: %r" % text
    return {k: int(v) for k, v in m.groupdict().items()}


def _cuda(a, dtype):
    import torch
    return torch.from_numpy(np.array(a, dtype, order="C")).cuda()      # (a copy: the shared cases are read-only)


def _host(*tensors):
    import torch
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in tensors)


def scored(name, make, oracle):
    """(x, q, S) of a case, the reference scores computed once and never changed"""
    if name not in _CASES:
        x, q = make()
        with np.errstate(all="ignore"):
            S = rank_ref.canon_scores(oracle, x, q)
        S.setflags(write=False)
        _CASES[name] = (x, q, S)
    return _CASES[name]


def tensor_entries(idx, q, ranks, id_map=None):
    return _host(*idx.entries_at_tensor(_cuda(q, np.float32), _cuda(ranks, np.int64), id_map=id_map))


def tensor_keys(idx, q, ranks, pos_base=0):
    return _host(idx.entry_keys_at_tensor(_cuda(q, np.float32), _cuda(ranks, np.int64), pos_base=pos_base))[0].view(np.uint64)


def both_forms(idx, q, ranks, want, what=""):
    """host and tensor form against the reference; the status word stays clean"""
    got = idx.entries_at(q, ranks)
    assert got[0].shape == got[1].shape == np.shape(ranks)
    after_ref.assert_same(got, want, what + " host form")
    after_ref.assert_same(tensor_entries(idx, q, ranks), want, what + " tensor form")
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 1. every rank of a hostile corpus: -2 .. n + 2 for every query.  nq = 3 is 3015 pairs: two launches of 1024 and one of 967
# (60 tiles and a partial one of 7 pairs); nq = 1 is the all-zero query alone (every score a +0 tie, or NaN)
@pytest.mark.parametrize("nq", cases.HOSTILE_NQS)
@pytest.mark.parametrize("d", cases.HOSTILE_DS)
def test_every_rank_of_a_hostile_corpus(d, nq, oracle):
    x, q17, S17 = scored(f"hostile{d}", lambda: cases.hostile_case(d), oracle)
    n = len(x)
    q, S = cases.hostile_queries_of(q17, nq), S17[:nq]
    ranks = cases.all_ranks(nq, n)
    want = at_rank_ref.entries_at_from_scores(S, ranks)
    L = at_rank_ref.list_len(S)
    for i in range(nq):     # padding exactly from |L(q)| on, and in front of rank 0
        assert (want[1][i, 2:2 + L[i]] >= 0).all() and (want[1][i, 2 + L[i]:] == -1).all() and (want[1][i, :2] == -1).all()
    idx = _index(d, x)
    both_forms(idx, q, ranks, want, f"d={d} nq={nq}")
    plan = parse_plan(idx.last_plan())
    assert plan["BITS"] == 8 and plan["QT"] == 16 and plan["T"] == min(64, (ranks.size + 15) // 16) and plan["passes"] == at_rank_ref.passes(0, n) == 6, plan


# ---------------------------------------------------------------------------------------------------------------------
# 2. ties decided by position digits: n = 66 000 rows (7 passes: three position digits)
def test_ties_decided_by_position_digits_zero_query(oracle):
    x, q, S = scored("zero", cases.tie_zero_case, oracle)
    ranks = np.array([cases.TIE_RANKS], np.int64)
    idx = _index(cases.TIE_D, x)
    both_forms(idx, q, ranks, at_rank_ref.entries_at_from_scores(S, ranks), "zero query")
    assert parse_plan(idx.last_plan())["passes"] == at_rank_ref.passes(0, cases.TIE_N) == 7


def test_ties_decided_by_position_digits_duplicated_rows(oracle):
    x, q, S = scored("dup", cases.tie_dup_case, oracle)
    rows = np.tile(cases.tie_dup_rows(), (len(q), 1))
    r = rank_ref.rank_ids_from_scores(S, rows)                 # the ranks of rows on both sides of a group / segment / byte edge
    ranks = np.concatenate([r, np.array([cases.TIE_RANKS] * len(q), np.int64)], 1)
    want = at_rank_ref.entries_at_from_scores(S, ranks)
    np.testing.assert_array_equal(want[1][:, :rows.shape[1]], rows)
    idx = _index(cases.TIE_D, x)
    both_forms(idx, q, ranks, want, "duplicated rows")


# ---------------------------------------------------------------------------------------------------------------------
# 3. score digit edges: adjacent floats, +0 against -0, +-Inf, exactly -FLT_MAX (a real row), denormals; every rank
def test_score_digit_edges(oracle):
    x, q, S = scored("grid", cases.grid_case, oracle)
    ranks = cases.all_ranks(len(q), cases.GRID_N)
    want = at_rank_ref.entries_at_from_scores(S, ranks)
    assert ((want[0] == -FMAX) & (want[1] >= 0)).any()          # -FLT_MAX with a row id: not padding
    idx = _index(cases.GRID_D, x)
    both_forms(idx, q, ranks, want, "grid")


# ---------------------------------------------------------------------------------------------------------------------
# 4. pos_base: the keys are after_ref.pack's, and the last column is the cursor of the page behind it
def test_pos_base(oracle):
    import torch
    from haconvdr_amd._lib import HacError
    d, nq = 96, 3
    x, q17, S17 = scored("hostile96", lambda: cases.hostile_case(96), oracle)
    n = len(x)
    q, S = q17[:nq], S17[:nq]
    L = at_rank_ref.list_len(S)
    ranks = np.stack([np.array([0, 1, 255, 256, 257, 700, L[i] - 7, -1, n + 1, L[i] - 30], np.int64) for i in range(nq)])
    idx = _index(d, x)
    qt = _cuda(q, np.float32)
    top = 2 ** 32 - 1 - n                                       # the largest pos_base the keys forms admit: pos_base + ntotal <= 2^32 - 1
    for pos_base in (0, 2 ** 24 - 500, top):
        want = at_rank_ref.entry_keys_from_scores(S, ranks, pos_base)
        keys = idx.entry_keys_at_tensor(qt, _cuda(ranks, np.int64), pos_base=pos_base)
        assert parse_plan(idx.last_plan())["passes"] == at_rank_ref.passes(pos_base, n)
        page = idx.search_after_keys_tensor(qt, 40, keys[:, -1].contiguous(), pos_base=pos_base)
        keys, page = _host(keys, page)
        np.testing.assert_array_equal(keys.view(np.uint64), want, err_msg=f"pos_base={pos_base}")
        after_ref.assert_same(after_ref.unpack(page, pos_base), at_rank_ref.search_at_from_scores(S, L - 29, 40), f"page pos_base={pos_base}")
    assert at_rank_ref.passes(2 ** 24 - 500, n) == 8 and at_rank_ref.passes(top, n) == 6
    # 2^32 - n: the last row would sit at position 2^32 - 1.  The keys forms refuse pos_base + ntotal > 2^32 - 1; so does this one
    for call in (lambda: idx.entry_keys_at_tensor(qt, _cuda(ranks, np.int64), pos_base=2 ** 32 - n),
                 lambda: idx.search_after_keys_tensor(qt, 40, None, pos_base=2 ** 32 - n),
                 lambda: idx.search_keys_tensor(qt, 40, pos_base=2 ** 32 - n)):
        with pytest.raises(HacError) as e:
            call()
        assert e.value.code == HAC_ERR_UNSUPPORTED and "32 bits" in str(e.value)
    torch.cuda.synchronize()
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 5. plan independence: one row stream against auto, one pair tile per launch against 64
def test_plans_give_the_same_bytes(oracle):
    d, nq = 96, 3
    x, q17, S17 = scored("hostile96", lambda: cases.hostile_case(96), oracle)
    q = q17[:nq]
    rng = np.random.default_rng(0xD50)
    ranks = rng.integers(-3, len(x) + 3, (nq, 23)).astype(np.int64)     # 69 pairs: five tiles, the last of 5 pairs
    want = at_rank_ref.entries_at_from_scores(S17[:nq], ranks)
    seen = {}
    for p, tiles in (("auto", 0), ("1", 0), ("auto", 1), ("1", 1), ("7", 2)):
        idx = _index(d, x, at_rank_p=p, debug_at_rank_tiles=tiles)
        got = idx.entries_at(q, ranks)
        keys = tensor_keys(idx, q, ranks)
        plan = parse_plan(idx.last_plan())
        after_ref.assert_same(got, want, f"p={p} tiles={tiles}")
        seen[(p, tiles)] = (got[0].tobytes(), got[1].tobytes(), keys.tobytes())
        assert plan["passes"] == at_rank_ref.passes(0, len(x)) and plan["T"] == (tiles or 5) and plan["QT"] == 16, plan
        assert plan["P"] == (int(p) if p != "auto" and int(p) <= 4 else plan["P"]) and (p != "1" or plan["P"] == 1), plan
        assert plan["lds"] == (d // 4) * 16 * 16 + 16 * 256 * 4 + 16 * 8 + 16 * 4, plan
        idx.check_status()
    assert len(set(seen.values())) == 1
    with pytest.raises(Exception):
        idx.set_option("at_rank_p", "0")
    with pytest.raises(Exception):
        idx.set_option("debug_at_rank_tiles", "-1")


# ---------------------------------------------------------------------------------------------------------------------
# 6. the identities on GPU results
@pytest.mark.parametrize("d, split", [(96, "0"), (768, "1")])
def test_identities_on_gpu_results(d, split, oracle):
    import torch
    x, q17, S17 = scored(f"hostile{d}", lambda: cases.hostile_case(d), oracle)
    n, nq = len(x), 17
    q, S = q17, S17
    idx = _index(d, x, split=split)
    qt = _cuda(q, np.float32)
    for k in (1, 100, 2048):                                    # entries_at(q, arange(k)) == search(q, k), padding included
        ranks = np.tile(np.arange(k, dtype=np.int64), (nq, 1))
        after_ref.assert_same(idx.entries_at(q, ranks), idx.search(q, k), f"search k={k}")
    ranks = cases.all_ranks(nq, n)
    Dt, It = idx.entries_at_tensor(qt, _cuda(ranks, np.int64))
    back = _host(idx.rank_ids_tensor(qt, torch.clamp(It, min=-1)))[0]          # rank_ids(q, I_at) == ranks wherever I_at >= 0
    D, I = _host(Dt, It)
    np.testing.assert_array_equal(back[I >= 0], ranks[I >= 0])
    assert (back[I < 0] == -1).all()
    ids = np.tile(np.arange(n, dtype=np.int64), (nq, 1))         # entries_at(q, rank_ids(q, ids)) names ids and score_ids again
    r = idx.rank_ids(q, ids)
    D2, I2 = idx.entries_at(q, r)
    np.testing.assert_array_equal(I2[r >= 0], ids[r >= 0])
    np.testing.assert_array_equal(after_ref.bits(D2[r >= 0]), after_ref.bits(idx.score_ids(q, ids)[r >= 0]))
    assert (I2[r < 0] == -1).all() and (r < 0).any()
    radius = S[np.arange(nq), (np.arange(nq) * 37 + 11) % n].copy()      # range_count brackets the score at a rank
    radius[np.isnan(radius)] = 0.125
    c = idx.range_count(q, radius)
    np.testing.assert_array_equal(c, np.diff(range_ref.range_from_scores(S, radius)[0]))
    Dc = idx.entries_at(q, np.stack([c - 1, c], 1))[0]
    L = at_rank_ref.list_len(S)
    assert (Dc[c >= 1, 0] > radius[c >= 1]).all() and (radius[c < L] >= Dc[c < L, 1]).all() and ((c >= 1) & (c < L)).any()
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 7. search_at: per-query starts 0, 1, 2047, 3000, |L| - 1, |L|, |L| + 5 over 6000 rows
@pytest.mark.parametrize("k", cases.AT_KS)
def test_search_at(k, oracle):
    x, q, S = scored("at", cases.at_case, oracle)
    start = cases.at_starts(at_rank_ref.list_len(S))
    idx = _scoped_index("at", cases.AT_D, x)
    want = at_rank_ref.search_at_from_scores(S, start, k)
    after_ref.assert_same(idx.search_at(q, k, start), want, f"host k={k}")
    qt, st = _cuda(q, np.float32), _cuda(start, np.int64)
    after_ref.assert_same(_host(*idx.search_at_tensor(qt, k, st)), want, f"tensor k={k}")
    keys = _host(idx.search_at_keys_tensor(qt, k, st, pos_base=1000))[0]
    after_ref.assert_same(after_ref.unpack(keys, 1000), want, f"keys k={k}")
    # start = 0 is search, bit for bit; an integer start serves every query
    after_ref.assert_same(idx.search_at(q, k, 0), idx.search(q, k), f"start 0 k={k}")
    after_ref.assert_same(_host(*idx.search_at_tensor(qt, k, 0)), idx.search(q, k), f"start 0 tensor k={k}")
    after_ref.assert_same(idx.search_at(q, k, 3000), at_rank_ref.search_at_from_scores(S, np.full(len(q), 3000), k), f"start 3000 k={k}")
    idx.check_status()


_INDEXES = {}


def _scoped_index(name, d, x):
    """one index for the cases of a parametrised test that only read it"""
    if name not in _INDEXES:
        _INDEXES[name] = _index(d, x)
    return _INDEXES[name]


def test_resident_corpus_window_and_score_at_rank(oracle):
    from haconvdr_amd.passages import read_embedding_block
    from haconvdr_amd.search import ResidentCorpus
    g61 = os.path.join(os.path.dirname(__file__), "golden", "passages61")
    rc = ResidentCorpus(g61, 4)
    blocks = [read_embedding_block(g61, b) for b in range(4)]
    x = np.concatenate([np.asarray(e) for e, _ in blocks])
    ext = np.concatenate([np.asarray(i, np.int64) for _, i in blocks])
    n, nq = len(x), 3
    q = synth.embeddings(0xD72, nq, 768)
    S = rank_ref.canon_scores(oracle, x, q)
    start = np.array([0, 7, 58], np.int64)
    for width in (1, 10, 2100):                                  # 2100: a second page behind the first 2048 slots
        D, I = rc.search_window(q, start, width)
        wD, wI = at_rank_ref.search_at_from_scores(S, start, width)
        assert D.dtype == np.float64 and I.dtype == np.int64
        np.testing.assert_array_equal(I, np.where(wI >= 0, ext[np.maximum(wI, 0)], -1))
        np.testing.assert_array_equal(D, wD.astype(np.float64))
    sD, sI = rc.search(q, 10)
    wD, wI = rc.search_window(q, 0, 10)
    np.testing.assert_array_equal(wI, sI)
    np.testing.assert_array_equal(wD, sD)
    ranks = np.tile(np.array([0, 30, 60, 61, -1], np.int64), (nq, 1))
    got = rc.score_at_rank(q, ranks)
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, at_rank_ref.entries_at_from_scores(S, ranks)[0].astype(np.float64))
    for bad in (lambda: rc.search_window(q, -1, 5), lambda: rc.search_window(q, 0, 0), lambda: rc.score_at_rank(q, ranks.astype(np.float32))):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------------------------------------------------------------
# 8. non-finite queries next to healthy ones in one tile
@pytest.mark.parametrize("kind", nonfinite.KINDS)
def test_non_finite_queries(kind, oracle):
    d, n, nq = 96, 1001, 17
    x, q, pos, base = nonfinite.case(kind, d, n, nq, 0xD80)
    with np.errstate(all="ignore"):
        S = rank_ref.canon_scores(oracle, x, q)
    L = at_rank_ref.list_len(S)
    ranks = np.stack([np.concatenate([np.arange(-1, 60), [100, 500, L[i] - 1, L[i], n - 1, n, n + 2]]) for i in range(nq)]).astype(np.int64)
    want = at_rank_ref.entries_at_from_scores(S, ranks)
    if kind in nonfinite.NAN_KINDS:                             # a NaN query: padding at every rank
        assert (L[pos] == 0).all() and (want[1][pos] == -1).all() and (L[[1, 2]] == n).all()
    idx = _index(d, x)
    both_forms(idx, q, ranks, want, kind)


# ---------------------------------------------------------------------------------------------------------------------
# 9. lifetimes
def test_stale_rows_and_removed_rows_are_never_listed(oracle):
    d, nq = 96, 5
    old = synth.embeddings(0xD90, 1000, d) * np.float32(8.0)     # stale rows that would beat everything
    idx = _index(d, old)
    idx.reset()
    x = hostile_corpus(0xD91, 500, d)
    idx.add(x[:77])
    idx.add(x[77:])
    q = hostile_queries(0xD92, nq, d)
    ranks = cases.all_ranks(nq, 500)
    both_forms(idx, q, ranks, at_rank_ref.entries_at(oracle, x, q, ranks), "reset + smaller add")
    assert parse_plan(idx.last_plan())["passes"] == at_rank_ref.passes(0, 500)
    gone = np.array([0, 63, 64, 65, 130, 255, 256, 499], np.int64)
    assert idx.remove_ids(gone) == len(gone)
    kept = np.delete(x, gone, axis=0)
    ranks = cases.all_ranks(nq, len(kept))
    both_forms(idx, q, ranks, at_rank_ref.entries_at(oracle, kept, q, ranks), "remove_ids")


def test_empty_index_and_empty_calls():
    import torch
    d = 96
    x = synth.embeddings(0xDA0, 300, d)
    q = synth.embeddings(0xDA1, 2, d)
    idx = _index(d, x)
    assert [a.shape for a in idx.entries_at(np.zeros((0, d), np.float32), np.zeros((0, 3), np.int64))] == [(0, 3)] * 2
    assert [a.shape for a in idx.entries_at(q, np.zeros((2, 0), np.int64))] == [(2, 0)] * 2
    assert tuple(idx.entry_keys_at_tensor(_cuda(q, np.float32), torch.zeros((2, 0), dtype=torch.int64, device="cuda")).shape) == (2, 0)
    idx.reset()
    ranks = np.array([[0, -1, 5], [1, 2 ** 40, -2 ** 40]], np.int64)
    D, I = idx.entries_at(q, ranks)
    assert (D == -FMAX).all() and (I == -1).all()
    D, I = tensor_entries(idx, q, ranks)
    assert (D == -FMAX).all() and (I == -1).all()
    assert (tensor_keys(idx, q, ranks, pos_base=77) == 0).all()
    D, I = idx.search_at(q, 5, 0)
    assert (D == -FMAX).all() and (I == -1).all()
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 10. captured: the tensor form in a HIP graph, replayed with the ranks rewritten between the replays
def test_entries_at_tensor_captured_and_replayed(oracle):
    import torch
    d, nq, m = 96, 17, 11
    x, q17, S17 = scored("hostile96", lambda: cases.hostile_case(96), oracle)
    n = len(x)
    q = _cuda(q17, np.float32)
    rng = np.random.default_rng(0xDB0)
    rank_sets = [rng.integers(-2, n + 2, (nq, m)).astype(np.int64) for _ in range(3)]
    ranks = _cuda(rank_sets[0], np.int64)
    idx = _index(d, x)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()                            # a single stream: no parallel branches in the graph
    replayed = []
    with torch.cuda.stream(side):
        eager = idx.entries_at_tensor(q, ranks)           # the largest shape once: workspaces and the segment table exist
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            D, I = idx.entries_at_tensor(q, ranks)
        for rs in rank_sets:
            ranks.copy_(torch.from_numpy(rs))
            D.fill_(7.0)
            I.fill_(-7)
            g.replay()
            side.synchronize()
            replayed.append((D.cpu().numpy(), I.cpu().numpy()))
    torch.cuda.synchronize()
    after_ref.assert_same(_host(*eager), at_rank_ref.entries_at_from_scores(S17, rank_sets[0]), "eager")
    for rs, got in zip(rank_sets, replayed):
        after_ref.assert_same(got, at_rank_ref.entries_at_from_scores(S17, rs), "replay")
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 11. multi-device indexes are refused by all three entry points, and nothing is written.  Two shards on device 0 make a
# multi-device index wherever one device is visible; with two visible, one on each as well.
def test_multi_device_is_unsupported():
    import torch
    from haconvdr_amd._lib import HacError
    d = 96
    x = synth.embeddings(0xDC0, 300, d)
    q = synth.embeddings(0xDC1, 2, d)
    ranks = np.array([[0, 5], [1, 7]], np.int64)
    for devices in [(0, 0)] + ([(0, 1)] if torch.cuda.device_count() >= 2 else []):
        multi = _index(d, x, devices=devices)
        with pytest.raises(HacError) as e:
            multi.entries_at(q, ranks)
        assert e.value.code == HAC_ERR_UNSUPPORTED
        D = torch.full((2, 2), 7.0, device="cuda")
        I = torch.full((2, 2), -7, dtype=torch.int64, device="cuda")
        keys = torch.full((2, 2), -7, dtype=torch.int64, device="cuda")
        from haconvdr_amd import _lib
        from haconvdr_amd.index import _devp, _stream_ptr
        qt, rt = _cuda(q, np.float32), _cuda(ranks, np.int64)
        rc = _lib.lib().hac_index_entries_at_device(multi._h, _devp(qt), 2, _devp(rt), 2, _devp(D), _devp(I), _devp(None), _stream_ptr(None))
        assert rc == HAC_ERR_UNSUPPORTED
        rc = _lib.lib().hac_index_entries_at_keys_device(multi._h, _devp(qt), 2, _devp(rt), 2, _devp(keys), 0, _stream_ptr(None))
        assert rc == HAC_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert (D == 7.0).all() and (I == -7).all() and (keys == -7).all()        # nothing was written
        for call in (lambda: multi.entries_at_tensor(qt, rt), lambda: multi.entry_keys_at_tensor(qt, rt), lambda: multi.search_at(q, 5, 1)):
            with pytest.raises(HacError) as e:
                call()
            assert e.value.code == HAC_ERR_UNSUPPORTED
        multi.check_status()
