"""Exact corpus rank of named rows: hac_index_rank_ids*, hac_index_count_ahead_device (count_ahead_kernel, rank_finish_kernel
of csrc/rank.inc) through FlatIPIndex and ResidentCorpus, i.e. the C ABI.

Every assertion is integer equality with tests/rank_ref.py, the definition of include/haconvdr.h restated over the CPU
oracle's canonical scores.  Indexes are built like _index() of tests/test_search_plans_gpu.py: three adds cut off the 64-row
grid, so the last group is partial and its tail rows must never count."""
import os
import re

import numpy as np
import pytest

from haconvdr_amd import synth
from tests import rank_ref
from tests.test_index_rows_gpu import PAIR_MC, STAGE_BYTES, hostile_corpus, pair_chunk_corpus, pair_chunk_ids
from tests.test_search_plans_gpu import _adversarial, _index

pytestmark = pytest.mark.gpu

FMAX = np.finfo(np.float32).max
HAC_ERR_INVALID, HAC_ERR_UNSUPPORTED = 1, 4
_PLAN = re.compile(r"^count_ahead_kernel<MT=(?P<MT>\d+)> grid=\((?P<P>\d+),(?P<T>\d+)\) QT=(?P<QT>\d+) chunks=(?P<chunks>\d+) lds=(?P<lds>\d+)$")


def parse_plan(text):
    m = _PLAN.match(text)
    assert m, "not the plan of a rank call: %r" % text
    return {k: int(v) for k, v in m.groupdict().items()}


def _cuda(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def tensor_ranks(idx, q, ids):
    import torch
    out = idx.rank_ids_tensor(_cuda(q, np.float32), _cuda(ids, np.int64))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def tensor_counts(idx, q, s, b):
    import torch
    out = idx.count_ahead_tensor(_cuda(q, np.float32), _cuda(s, np.float32), _cuda(b, np.int64))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def both_forms(idx, q, ids, want):
    """host and tensor form against the reference; the status word stays clean"""
    got = idx.rank_ids(q, ids)
    assert got.dtype == np.int64 and got.shape == np.shape(ids)
    np.testing.assert_array_equal(got, want, err_msg="host form")
    np.testing.assert_array_equal(tensor_ranks(idx, q, ids), want, err_msg="tensor form")
    idx.check_status()


def hostile_queries(seed, nq, d):
    """unit-ish queries; query 0 all zero (every score a +-0 tie) where there are two or more, and a negated pair"""
    q = synth.embeddings(seed, nq, d)
    if nq >= 2:
        q[0] = 0.0
    if nq >= 4:
        q[3] = -q[2]
    return q


# ---------------------------------------------------------------------------------------------------------------------
# 1. every row named, on hostile rows: m = n >> MT (125 chunks), negative reference scores against the zero-padded tail of
# the last group, NaN rows that must not count, NaN-scored named rows -> -1.  d = 32: the zero-trip chunk loop.
_HOSTILE = {}


def _hostile_case(d, oracle):
    """(x, q of 33 queries, their canonical scores): computed once per d, shared by the query counts"""
    if d not in _HOSTILE:
        x = hostile_corpus(0x4A9 + d, 1000, d)
        q = hostile_queries(0x4AA + d, 33, d)
        _HOSTILE[d] = (x, q, rank_ref.canon_scores(oracle, x, q))
    return _HOSTILE[d]


@pytest.mark.parametrize("nq", [1, 16, 17, 33])
@pytest.mark.parametrize("d", [32, 96, 768, 1024])
def test_every_row_named_on_hostile_rows(d, nq, oracle):
    x, q33, S33 = _hostile_case(d, oracle)
    n = len(x)
    # nq = 1: the all-zero query on its own; otherwise the first nq (zero query, negated pair included)
    q, S = (q33[:1], S33[:1]) if nq == 1 else (q33[:nq], S33[:nq])
    ids = np.tile(np.arange(n, dtype=np.int64), (nq, 1))
    want = rank_ref.rank_ids_from_scores(S, ids)
    assert (want == -1).any() and (want[0] >= 0).sum() == (~np.isnan(S[0])).sum()
    # the all-zero query: every score a +-0 tie or NaN, rank = the non-NaN rows in front
    np.testing.assert_array_equal(want[0], np.where(np.isnan(S[0]), -1, np.cumsum(~np.isnan(S[0])) - 1))
    for i in range(nq):     # naming all rows gives a permutation of 0 .. (non-NaN rows - 1)
        r = want[i][want[i] >= 0]
        np.testing.assert_array_equal(np.sort(r), np.arange(len(r)))
    idx = _index(d, x)
    both_forms(idx, q, ids, want)
    plan = parse_plan(idx.last_plan())
    assert plan["T"] == (nq + 15) // 16 and plan["QT"] == min(nq, 16) and plan["chunks"] == (n + plan["MT"] - 1) // plan["MT"], plan


# ---------------------------------------------------------------------------------------------------------------------
# 2. m at the chunk edges
def test_m_at_the_chunk_edges(oracle):
    d, n, nq = 96, 1000, 5
    x, q33, S33 = _hostile_case(d, oracle)
    q, S = q33[:nq], S33[:nq]
    idx = _index(d, x)
    idx.rank_ids(q[:1], np.zeros((1, 1), np.int64))
    MT = parse_plan(idx.last_plan())["MT"]
    assert MT >= 2
    pool = (synth.uniform_u32(0x4B0, nq * (2 * MT + 3)) % np.uint32(n)).astype(np.int64).reshape(nq, -1)
    for m in (1, MT - 1, MT, MT + 1, 2 * MT + 3):
        ids = pool[:, :m].copy()
        if m >= 3:
            ids[:, 1] = ids[:, 0]             # a repeated id
            ids[1, 2] = -1                    # padding slots
            ids[2, m - 1] = -1
        want = rank_ref.rank_ids_from_scores(S, ids)
        both_forms(idx, q, ids, want)
        plan = parse_plan(idx.last_plan())
        assert plan["chunks"] == (m + MT - 1) // MT and plan["T"] == 1 and plan["QT"] == nq, (m, plan)


# ---------------------------------------------------------------------------------------------------------------------
# 3. ties
def test_ties_of_interleaved_repeated_rows(oracle):
    """16 distinct grid-valued rows, each repeated ~62 times and interleaved; integer queries: every score is exact and every
    score value is shared by dozens of rows, so the row order inside a tie decides almost every rank"""
    d, n, nq = 96, 1000, 6
    base = ((synth.uniform_u32(0x4C0, 16 * d) % np.uint32(17)).astype(np.float32).reshape(16, d) - 8.0) / 8.0
    x = base[np.arange(n) % 16]
    q = (synth.uniform_u32(0x4C1, nq * d) % np.uint32(9)).astype(np.float32).reshape(nq, d) - 4.0
    S = rank_ref.canon_scores(oracle, x, q)
    assert all(len(np.unique(S[i])) <= 16 for i in range(nq))
    ids = np.tile(np.arange(n, dtype=np.int64), (nq, 1))
    both_forms(_index(d, x), q, ids, rank_ref.rank_ids_from_scores(S, ids))


def test_identical_rows_rank_by_id(oracle):
    d, n = 64, 1000
    x = np.tile(synth.embeddings(0x4C2, 1, d), (n, 1))
    q = synth.embeddings(0x4C3, 3, d)
    ids = np.tile(np.arange(n, dtype=np.int64), (3, 1))
    want = rank_ref.rank_ids(oracle, x, q, ids)
    np.testing.assert_array_equal(want, ids)
    both_forms(_index(d, x), q, ids, want)


def test_infinite_scores_are_ordinary_scores(oracle):
    d, n = 64, 1000
    x = synth.embeddings(0x4C4, n, d)
    x[[5, 400, 999]] = FMAX                    # +Inf against q[0], -Inf against q[1]: ties at both ends
    x[[6, 401]] = -FMAX
    q = np.stack([np.full(d, 2.0, np.float32), np.full(d, -2.0, np.float32), synth.embeddings(0x4C5, 1, d)[0]])
    S = rank_ref.canon_scores(oracle, x, q)
    assert np.isposinf(S[0, 5]) and np.isneginf(S[0, 6]) and np.isneginf(S[1, 5]) and not np.isnan(S[:2]).any()
    ids = np.tile(np.arange(n, dtype=np.int64), (3, 1))
    want = rank_ref.rank_ids_from_scores(S, ids)
    assert want[0, 5] == 0 and want[0, 400] == 1 and want[0, 999] == 2 and want[0, 401] == n - 1 and want[1, 999] == n - 1
    both_forms(_index(d, x), q, ids, want)


# ---------------------------------------------------------------------------------------------------------------------
# 4. beyond the top-k ceiling
def test_ranks_beyond_the_top_k_ceiling(oracle):
    d, n, nq = 64, 5000, 3
    x, q = _adversarial(d, n, nq, 0x4D0)
    ids = np.tile(np.arange(n, dtype=np.int64), (nq, 1))
    want = rank_ref.rank_ids(oracle, x, q, ids)
    np.testing.assert_array_equal(want, n - 1 - ids)        # row i has rank n - 1 - i: up to 4999 > HAC_MAX_K
    both_forms(_index(d, x), q, ids, want)


# ---------------------------------------------------------------------------------------------------------------------
# 5. agreement with search, both routes
@pytest.mark.parametrize("split", ["0", "1"])
def test_rank_of_a_search_result_is_its_column(split, oracle):
    d, n, nq = 192, 5000, 20
    x = synth.embeddings(0x4E0, n, d)
    x[1000:1040] = x[17]                                     # a run of equal rows inside the lists
    q = synth.embeddings(0x4E1, nq, d)
    idx = _index(d, x, split=split)
    for k in (1, 100, 2048):
        D, I = idx.search(q, k)
        if split == "1" and k == 100:
            assert idx.last_plan().startswith("split:"), idx.last_plan()
        assert (I >= 0).all()
        want = np.tile(np.arange(k, dtype=np.int64), (nq, 1))
        both_forms(idx, q, I, want)
    np.testing.assert_array_equal(rank_ref.rank_ids(oracle, x, q, I), want)


def test_padding_slots_of_a_short_list_rank_minus_one():
    d, n, k = 96, 50, 64
    x = synth.embeddings(0x4E2, n, d)
    q = synth.embeddings(0x4E3, 4, d)
    idx = _index(d, x)
    D, I = idx.search(q, k)
    assert (I[:, n:] == -1).all() and (I[:, :n] >= 0).all()
    both_forms(idx, q, I, np.tile(np.where(np.arange(k) < n, np.arange(k), -1).astype(np.int64), (4, 1)))


# ---------------------------------------------------------------------------------------------------------------------
# 6. stale tail: reset() keeps the allocation, the smaller add() leaves rows of the old corpus behind its last row
def test_stale_rows_behind_a_smaller_add_never_count(oracle):
    d, nq = 96, 5
    old = synth.embeddings(0x4F0, 1000, d) * np.float32(8.0)     # stale rows that would beat everything
    idx = _index(d, old)
    idx.reset()
    x = hostile_corpus(0x4F1, 500, d)
    idx.add(x[:77])
    idx.add(x[77:])
    assert idx.ntotal == 500
    q = hostile_queries(0x4F2, nq, d)
    ids = np.tile(np.arange(500, dtype=np.int64), (nq, 1))
    both_forms(idx, q, ids, rank_ref.rank_ids(oracle, x, q, ids))


# ---------------------------------------------------------------------------------------------------------------------
# 7. count_ahead_tensor on its own
def test_count_ahead_tensor(oracle):
    d, n, nq = 96, 1000, 3
    base = ((synth.uniform_u32(0x500, 4 * d) % np.uint32(17)).astype(np.float32).reshape(4, d) - 8.0) / 8.0
    x = base[np.arange(n) % 4]                                # four score values per query, 250 rows each
    x[3] = np.nan
    q = (synth.uniform_u32(0x501, nq * d) % np.uint32(9)).astype(np.float32).reshape(nq, d) - 4.0
    S = rank_ref.canon_scores(oracle, x, q)
    tied = S[:, 1]                                            # a score 250 rows share
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    bounds = np.array([0, 1, n // 2, n, n + 5, -1, 7, 0, n, 0, 0], np.int64)
    scores = np.stack([np.array([t, t, t, t, t, t, nan, inf, inf, -inf, -FMAX], np.float32) for t in tied])
    B = np.tile(bounds, (nq, 1))
    want = rank_ref.count_ahead(S, scores, B)
    assert (want[:, 5] == -1).all() and (want[:, 6] == -1).all() and (want[:, 7] == 0).all()
    assert (want[:, 9] == n - 1).all()                        # everything but the NaN row beats -Inf
    np.testing.assert_array_equal(want[:, 3], want[:, 4])     # a bound above ntotal behaves like ntotal
    idx = _index(d, x)
    np.testing.assert_array_equal(tensor_counts(idx, q, scores, B), want)
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 8. multi-device host path: three shards on one device, every add split across them, ties straddling shards
def test_multi_device_host_path(oracle):
    d, nq = 96, 5
    hostile = hostile_corpus(0x510, 700, d)
    base = ((synth.uniform_u32(0x511, 16 * d) % np.uint32(17)).astype(np.float32).reshape(16, d) - 8.0) / 8.0
    x = np.concatenate([hostile, base[np.arange(500) % 16]])
    n = len(x)
    q = hostile_queries(0x512, nq, d)
    q[4] = np.round(q[4] * 4.0)                               # exact scores on the grid-valued half
    ids = np.tile(np.arange(n, dtype=np.int64), (nq, 1))
    ids[1, 10] = ids[3, 0] = -1
    want = rank_ref.rank_ids(oracle, x, q, ids)
    multi = _index(d, x, devices=(0, 0, 0))
    got = multi.rank_ids(q, ids)
    np.testing.assert_array_equal(got, want)
    multi.check_status()
    np.testing.assert_array_equal(_index(d, x).rank_ids(q, ids), got)


# ---------------------------------------------------------------------------------------------------------------------
# 9. errors and empties
def test_errors_and_empties():
    import torch
    from haconvdr_amd._lib import HacError
    d, n = 96, 300
    x = synth.embeddings(0x520, n, d)
    q = synth.embeddings(0x521, 2, d)
    idx = _index(d, x)
    for bad in (n, -2):
        ids = np.array([[0, 5], [bad, 7]], np.int64)
        with pytest.raises(HacError) as e:
            idx.rank_ids(q, ids)
        assert e.value.code == HAC_ERR_INVALID and str(bad) in str(e.value) and "query 1, column 0" in str(e.value), str(e.value)
        got = tensor_ranks(idx, q, ids)
        assert got[1, 0] == -1 and (got[[0, 0, 1], [0, 1, 1]] >= 0).all()
        idx.check_status()
    assert idx.rank_ids(np.zeros((0, d), np.float32), np.zeros((0, 3), np.int64)).shape == (0, 3)
    assert idx.rank_ids(q, np.zeros((2, 0), np.int64)).shape == (2, 0)
    assert tuple(idx.rank_ids_tensor(_cuda(q, np.float32), torch.zeros((2, 0), dtype=torch.int64, device="cuda")).shape) == (2, 0)
    assert tuple(idx.count_ahead_tensor(torch.zeros((0, d), device="cuda"), torch.zeros((0, 4), device="cuda"),
                                        torch.zeros((0, 4), dtype=torch.int64, device="cuda")).shape) == (0, 4)
    idx.check_status()
    # an empty index: every id is outside, nothing is ahead of anything
    empty = _index(d, x)
    empty.reset()
    np.testing.assert_array_equal(tensor_ranks(empty, q, np.array([[0, -1], [5, 1]], np.int64)), -1)
    np.testing.assert_array_equal(tensor_counts(empty, q, np.zeros((2, 2), np.float32), np.array([[0, 5], [-1, 1]], np.int64)), [[0, 0], [-1, 0]])
    empty.check_status()
    multi = _index(d, x, devices=(0, 0))
    for call in (lambda: multi.rank_ids_tensor(_cuda(q, np.float32), _cuda(np.zeros((2, 1)), np.int64)),
                 lambda: multi.count_ahead_tensor(_cuda(q, np.float32), _cuda(np.zeros((2, 1)), np.float32), _cuda(np.zeros((2, 1)), np.int64))):
        with pytest.raises(HacError) as e:
            call()
        assert e.value.code == HAC_ERR_UNSUPPORTED
    multi.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 10. capture
def test_rank_ids_tensor_captured_and_replayed(oracle):
    import torch
    d, n, nq, m = 96, 1000, 17, 11
    x, q33, S33 = _hostile_case(d, oracle)
    q = _cuda(q33[:nq], np.float32)
    ids_np = (synth.uniform_u32(0x530, nq * m) % np.uint32(n)).astype(np.int64).reshape(nq, m)
    ids = _cuda(ids_np, np.int64)
    idx = _index(d, x)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()                            # a single stream: no parallel branches in the graph
    replayed = []
    with torch.cuda.stream(side):
        eager = idx.rank_ids_tensor(q, ids)               # the largest shape once: workspaces and the segment table exist
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            out = idx.rank_ids_tensor(q, ids)
        for _ in range(2):
            out.fill_(-7)
            g.replay()
            side.synchronize()
            replayed.append(out.cpu().numpy())
    torch.cuda.synchronize()
    want = rank_ref.rank_ids_from_scores(S33[:nq], ids_np)
    np.testing.assert_array_equal(eager.cpu().numpy(), want)
    for r in replayed:
        np.testing.assert_array_equal(r, want)
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 11. ResidentCorpus.rank by external passage id
def test_resident_corpus_rank(oracle):
    from haconvdr_amd.passages import read_embedding_block
    from haconvdr_amd.search import ResidentCorpus
    g61 = os.path.join(os.path.dirname(__file__), "golden", "passages61")
    rc = ResidentCorpus(g61, 4)
    blocks = [read_embedding_block(g61, b) for b in range(4)]
    x = np.concatenate([np.asarray(e) for e, _ in blocks])
    ext = np.concatenate([np.asarray(i, np.int64) for _, i in blocks])
    n, nq, k = len(x), 3, 10
    assert rc.ntotal == n == 61
    q = synth.embeddings(0x540, nq, 768)
    D, I = rc.search(q, k)                                    # I: external ids
    np.testing.assert_array_equal(rc.rank(q, I), np.tile(np.arange(k), (nq, 1)))
    pids = np.tile(ext[::-1], (nq, 1))
    pids[:, 4] = 10 ** 9                                      # an id no block holds
    got = rc.rank(q, pids)
    want = rank_ref.rank_ids(oracle, x, q, rc.rows_of(pids))
    assert got.dtype == np.int64 and (got[:, 4] == -1).all() and (np.delete(got, 4, 1) >= 0).all()
    np.testing.assert_array_equal(got, want)
    with pytest.raises(ValueError):
        rc.rank(q, ext)


# ---------------------------------------------------------------------------------------------------------------------
# 12. the host form across both of its chunk loops (sizes: tests/test_index_rows_gpu.py, 11.): QC = 64 MiB // (2^20 * 20 +
# 4d) = 3 queries and 2^20 columns at a time.  A column chunk of 2^20 ids is 131072 chunks of MT = 8: the launch loop steps
# over its 65535-wide grid limit twice.  Rows 5 and 120 are identical and lie on different shards of the two-shard index.
@pytest.mark.parametrize("devices", [(0,), (0, 0)])
def test_ranks_across_both_chunk_loops(devices, oracle):
    x, q6 = pair_chunk_corpus()
    n, d = x.shape
    nq = 4
    q = q6[:nq]
    assert STAGE_BYTES // (PAIR_MC * 20 + 4 * d) == 3                   # query chunks 3 + 1, column chunks 2^20 + 1
    ids = pair_chunk_ids(0xC53, nq, n)
    assert ids.min() == -1 and ids.max() == n - 1
    table = rank_ref.rank_ids_from_scores(rank_ref.canon_scores(oracle, x, q), np.tile(np.arange(n, dtype=np.int64), (nq, 1)))
    assert (table[:, 120] == table[:, 5] + 1).all()                     # the tie pair: neighbours, the lower row first
    want = np.take_along_axis(table, np.clip(ids, 0, None), 1)
    want[ids < 0] = -1
    idx = _index(d, x, devices=devices)
    got = idx.rank_ids(q, ids)
    assert got.dtype == np.int64
    np.testing.assert_array_equal(got, want)
    assert PAIR_MC // parse_plan(idx.last_plan())["MT"] > 2 * 65535     # (the plan is the last column chunk's: MT alone is read)
    idx.check_status()
