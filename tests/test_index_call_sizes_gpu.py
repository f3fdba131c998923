"""Rank, count and range calls past one query chunk and one merge pair: count_ahead_kernel and range_emit_kernel behind the
launch loop of csrc/rows_host.inc (QUERY_CHUNK = 1024 queries a launch, every launch with offsets of its own into the caller's
arrays and the workspace), range_offsets_kernel where a thread owns a run of queries, range_merge_kernel beyond its second
pass, and search_excluding over more queries than a chunk -- through FlatIPIndex, i.e. the C ABI.

The inputs are tests/call_sizes.py's; tests/test_index_call_sizes.py proves on the CPU that they tell every query from the
queries one and two launches before it, so a result that belongs to another query cannot pass.  Every assertion is equality
with tests/range_ref.py / tests/rank_ref.py over the CPU oracle's canonical scores (lims and I equal, D bit for bit), in the
host form and the tensor form, and the status word stays clean.  Corpora are tiny (300 rows) where the query count is the
subject; the merge cases need 8 * sort_lds + 70 rows of d = 32.

Measured on MI355X: this file 4.4 s (33 tests; the whole -m gpu suite with it: 1096 passed in 10 min 00 s, so 0.7 % of that)."""
import numpy as np
import pytest

from tests import call_sizes as cs
from tests import excluding, range_ref, rank_ref
from tests import test_index_range_gpu as rg
from tests import test_index_rank_gpu as rk
from tests.test_index_rows_gpu import tensor_scores
from tests.test_search_excluding_gpu import _excl, _excl_tensor, _same
from tests.test_search_plans_gpu import _index

pytestmark = pytest.mark.gpu

N = cs.SORT_N
SENT_D, SENT_I = np.float32(-123.5), np.int64(-99)


def _seam_index(d, nq, oracle, **kw):
    c = cs.seam(d, nq, oracle)
    return c, _index(d, c["x"], **kw)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the query-chunk seam
@pytest.mark.parametrize("nq", cs.SEAM_NQ)
@pytest.mark.parametrize("d", cs.SEAM_D)
def test_range_calls_across_the_query_chunk(d, nq, oracle):
    c, idx = _seam_index(d, nq, oracle)
    rg.both_forms(idx, c["q"], c["radius"], c["want"])               # range_search, range_count, range_search_tensor
    plan = rg.parse_plan(idx.last_plan())
    # the plan text is the LAST launch's: one launch of 1025 queries would say T == 65
    assert (plan["QT"], plan["T"]) == {1024: (16, 64), 1025: (1, 1), 1041: (16, 2), 2049: (1, 1)}[nq] == cs.last_launch_plan(nq), plan
    assert plan["cap"] == c["want"][0][-1]


@pytest.mark.parametrize("d", cs.SEAM_D)
def test_capacity_is_all_or_nothing_across_the_query_chunk(d, oracle):
    import torch
    nq = 1025
    c, idx = _seam_index(d, nq, oracle)
    q, radius, want = c["q"], c["radius"], c["want"]
    total = int(want[0][-1])
    qd, rd = rg._cuda(q, np.float32), rg._cuda(radius, np.float32)
    for cap in (total, total - 1, 0):
        fits = cap >= total
        D, I = np.full(total + 8, SENT_D, np.float32), np.full(total + 8, SENT_I, np.int64)
        rc, lims = rg.raw_host(idx, q, radius, cap, D if cap else None, I if cap else None)
        assert rc == 0
        np.testing.assert_array_equal(lims, want[0], err_msg="lims is exact whatever cap is")
        if fits:
            range_ref.assert_same((lims, D[:total], I[:total]), want, "host form, cap = total")
            assert (D[total:] == SENT_D).all() and (I[total:] == SENT_I).all()
        else:
            assert (D == SENT_D).all() and (I == SENT_I).all(), "an overflowing host call leaves D and I untouched"
        Dt = torch.full((total + 8,), float(SENT_D), dtype=torch.float32, device="cuda")
        It = torch.full((total + 8,), int(SENT_I), dtype=torch.int64, device="cuda")
        lt = torch.full((nq + 1,), -7, dtype=torch.int64, device="cuda")
        assert rg.raw_device(idx, qd, rd, cap, lt, Dt[:cap] if cap else None, It[:cap] if cap else None) == 0
        torch.cuda.synchronize()
        np.testing.assert_array_equal(lt.cpu().numpy(), want[0])
        Dn, In = Dt.cpu().numpy(), It.cpu().numpy()
        behind = total if fits else cap
        assert (Dn[behind:] == SENT_D).all() and (In[behind:] == SENT_I).all()
        if fits:
            range_ref.assert_same((lims, Dn[:total], In[:total]), want, "tensor form, cap = total")
    idx.check_status()


@pytest.mark.parametrize("nq", cs.SEAM_NQ)
@pytest.mark.parametrize("d", cs.SEAM_D)
def test_rank_count_and_score_calls_across_the_query_chunk(d, nq, oracle):
    c, idx = _seam_index(d, nq, oracle)
    q, S, radius = c["q"], c["S"], c["radius"]
    idx.rank_ids(q[:1], np.zeros((1, 1), np.int64))
    MT = rk.parse_plan(idx.last_plan())["MT"]
    assert MT + 1 == 9                                               # (the m the CPU proofs are made for)
    for m in (1, MT + 1):
        ids, ranks, own = cs.seam_rank(c, m)
        scores = np.where(ids >= 0, own, -cs.FMAX).astype(np.float32)
        cs.assert_scores(idx.score_ids(q, ids), scores, "score_ids")
        rk.both_forms(idx, q, ids, ranks)                            # rank_ids, rank_ids_tensor
        plan = rk.parse_plan(idx.last_plan())
        assert (plan["QT"], plan["T"]) == cs.last_launch_plan(nq) and plan["chunks"] == (m + MT - 1) // MT, plan
        # rank_ids_tensor keeps the ids' scores in the workspace behind its nq * m counters: neither plane shows in the other call
        cs.assert_scores(tensor_scores(idx, q, ids), scores, "score_ids_tensor")
        np.testing.assert_array_equal(rk.tensor_ranks(idx, q, ids), ranks, err_msg="rank_ids_tensor again")
        # count_ahead_tensor on the oracle's scores and bounds
        np.testing.assert_array_equal(rk.tensor_counts(idx, q, own, ids), ranks, err_msg="count_ahead_tensor")
    # a bound of 0 at score = radius counts the range list
    ahead = rk.tensor_counts(idx, q, radius[:, None], np.zeros((nq, 1), np.int64))[:, 0]
    np.testing.assert_array_equal(ahead, rank_ref.count_ahead(S, radius[:, None], np.zeros((nq, 1), np.int64))[:, 0])
    lens = idx.range_count(q, radius)
    np.testing.assert_array_equal(lens, np.diff(c["want"][0]))
    real = ~np.isnan(radius)
    assert (ahead[~real] == -1).all() and (lens[~real] == 0).all()
    np.testing.assert_array_equal(ahead[real], lens[real])
    idx.check_status()


@pytest.mark.parametrize("d", cs.SEAM_D)
def test_two_shards_each_run_the_chunk_loop(d, oracle):
    nq = 1025
    c, idx = _seam_index(d, nq, oracle, devices=(0, 0))
    q, radius, want = c["q"], c["radius"], c["want"]
    range_ref.assert_same(idx.range_search(q, radius), want, "two shards")
    np.testing.assert_array_equal(idx.range_count(q, radius), np.diff(want[0]))
    for m in (1, 9):
        ids, ranks, own = cs.seam_rank(c, m)
        np.testing.assert_array_equal(idx.rank_ids(q, ids), ranks, err_msg="two shards, m = %d" % m)
        cs.assert_scores(idx.score_ids(q, ids), np.where(ids >= 0, own, -cs.FMAX).astype(np.float32), "two shards")
    idx.check_status()


@pytest.mark.parametrize("d", cs.SEAM_D)
def test_search_excluding_across_the_query_chunk(d, oracle):
    nq, k, e = 1025, 10, 3
    c, idx = _seam_index(d, nq, oracle)
    x, q = c["x"], c["q"]
    _, top = oracle.flat_ip_search(x, q, k + e)
    E = top[:, :e].copy()                                            # each query's own top hits (the NaN query's: padding)
    assert (E[1023] == -1).all() and (np.delete(E, 1023, 0) >= 0).all()
    want = excluding.filtered_topk(oracle, x, q, k, E)
    np.testing.assert_array_equal(want[1][np.arange(nq) != 1023], np.delete(top, 1023, 0)[:, e:])      # the whole list shifts by e
    assert not np.array_equal(want[1][1024:1025], want[1][0:1])
    _same(_excl(idx, q, k, E), want, "host form")
    _same(_excl_tensor(idx, q, k, E), want, "tensor form")


# ---------------------------------------------------------------------------------------------------------------------
# 2. runs of range_offsets_kernel: one corpus, one index
_SHARED = {}


def _offsets(oracle):
    if "offsets" not in _SHARED:
        x, q, S = cs.planted(32, N + 70, max(cs.OFFSETS_NQ), 0x7D0, oracle)
        _SHARED["offsets"] = (q, S, _index(32, x))
    return _SHARED["offsets"]


@pytest.mark.parametrize("nq", cs.OFFSETS_NQ)
def test_offsets_where_a_thread_owns_a_run_of_queries(nq, oracle):
    q, S, idx = _offsets(oracle)
    L = cs.offsets_lengths(nq, N)
    radius = cs.radii_for_lengths(S[:nq], L)
    want = range_ref.range_from_scores(S[:nq], radius)
    np.testing.assert_array_equal(np.diff(want[0]), L)
    rg.both_forms(idx, q[:nq], radius, want)
    plan = rg.parse_plan(idx.last_plan())
    assert plan["sort_lds"] == N and plan["cap"] == L.sum() and plan["merge_passes"] == cs.passes_of(int(L.sum()), N), plan


# ---------------------------------------------------------------------------------------------------------------------
# 3. merge depth, uneven pairs, ties across sorted blocks and merge tiles
def _merge(oracle):
    if "merge" not in _SHARED:
        x, q, S = cs.planted(32, 8 * N + 70, 6, 0x7D8, oracle)
        _SHARED["merge"] = (q, S, _index(32, x))
    return _SHARED["merge"]


@pytest.mark.parametrize("name, passes", [("0 to 3 passes side by side", 4), ("4 passes, 8N meets 1", 4), ("more passes than any segment needs", 6)])
def test_merge_depth_and_uneven_pairs(name, passes, oracle):
    q, S, idx = _merge(oracle)
    lengths, extra = cs.merge_sets(N)[name]
    k, n = len(lengths), S.shape[1]
    radius = cs.radii_for_lengths(S[:k], lengths)
    want = range_ref.range_from_scores(S[:k], radius)
    np.testing.assert_array_equal(np.diff(want[0]), lengths)
    rg.both_forms(idx, q[:k], radius, want, extra_cap=extra)
    plan = rg.parse_plan(idx.last_plan())
    assert plan["sort_lds"] == N and plan["cap"] == sum(lengths) + extra, plan
    assert plan["merge_passes"] == passes == cs.passes_of(min(sum(lengths) + extra, k * n), N), plan


def test_tie_runs_across_sorted_blocks_and_merge_tiles(oracle):
    x, q, S, radius = cs.tie_case(32, N, oracle)
    want = range_ref.range_from_scores(S, radius)
    D0 = cs.lists(want, 0)[0]
    assert len(D0) > 4 * N and all(D0[o - 1] == D0[o] for o in (N, 2 * N, 3 * N, 4 * N))
    idx = _index(32, x)
    rg.both_forms(idx, q, radius, want)
    assert rg.parse_plan(idx.last_plan())["merge_passes"] == 3
    total = int(want[0][-1])
    rg.both_forms(idx, q, radius, want, extra_cap=40 * N)           # the 4N segment joins at pass 2 of 5
    assert rg.parse_plan(idx.last_plan())["merge_passes"] == cs.passes_of(min(total + 40 * N, len(q) * len(x)), N) == 5


# ---------------------------------------------------------------------------------------------------------------------
# 4. one workspace, many shapes: the RangeWs layout moves with (nq, cap) over what the call before left there
def test_one_workspace_many_shapes(oracle):
    d = 32
    w = cs.workspace_case(d, N, oracle)
    x, q, n, big_r, big, small_r, small, L, ids, ranks = (w[k] for k in ("x", "q", "n", "big_r", "big", "small_r", "small", "L", "ids", "ranks"))
    idx = _index(d, x)

    def range_step(qs, rs, want):
        fresh = _index(d, x)
        for i in (idx, fresh):
            rg.both_forms(i, qs, rs, want)
        assert idx.last_plan() == fresh.last_plan()

    range_step(q[:2], big_r, big)                                    # 1. the largest call of part 3
    range_step(q, small_r, small)                                    # 2. nq = 1025, small lists
    np.testing.assert_array_equal(idx.range_count(q, small_r), L)    # 3. the count alone
    np.testing.assert_array_equal(_index(d, x).range_count(q, small_r), L)
    range_step(q[:2], big_r, big)                                    # 4. the large call again
    rk.both_forms(idx, q, ids, ranks)                                # 5. ws_rank: the two workspaces do not share
    rk.both_forms(_index(d, x), q, ids, ranks)
    range_step(q[:2], big_r, big)
    idx.check_status()
