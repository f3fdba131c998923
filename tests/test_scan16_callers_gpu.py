"""The callers of csrc/scan16_core.inc at its zero-trip edge: d = 32 is K4 == PF, where scan16_group_mfma's chunk loop runs
no block and only the last-block sequence computes.  scan16_kernel (test_search_plans_gpu.py) and count_ahead_kernel
(test_index_rank_gpu.py) are pinned there already; this file pins the other five kernels: scan16_masked_kernel,
scan16_grouped_kernel, scan16_after_kernel, range_emit_kernel and rank_hist_kernel.

One corpus of 200 rows in one add (three full groups and one of 8 rows), 3 queries (one tile, QTr = 3 < 16), the prefilter
off.  The truth is oracle.flat_ip_search of the same inputs, scores and rows bit for bit, through the identities the CPU
tests of these routes prove over the oracle: an all-ones mask, a label per row and the start cursor are search; the page
behind entry 9 is the entries 10 .. 19; the rows strictly above entry 10's score are the ten in front of it; the entry at
rank t is entry t of the whole list."""
import numpy as np
import pytest

from haconvdr_amd import synth

D, N, NQ, K = 32, 200, 3, 10
SEED = 0x5C16
_CASE = {}


def case(oracle):
    """(x, q, oD, oI): rows, queries and the oracle's whole list of every query, computed once and never changed"""
    if not _CASE:
        x, q = synth.embeddings(SEED, N, D), synth.embeddings(SEED + 1, NQ, D)
        oD, oI = oracle.flat_ip_search(x, q, N)
        # what the identities below need of the inputs: no NaN score (all 200 rows are listed), and no tie among the first 21
        # entries (entry 10's score as a radius then cuts exactly behind entry 9; a page boundary never splits a tie)
        assert oD.shape == (NQ, N) and (oI >= 0).all() and not np.isnan(oD).any()
        assert (oD[:, :20] > oD[:, 1:21]).all(), "pick another seed: a tie among the first 21 scores"
        for a in (x, q, oD, oI):
            a.setflags(write=False)
        _CASE["c"] = (x, q, oD, oI)
    return _CASE["c"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, oD, oI, what):
    gD, gI = got
    np.testing.assert_array_equal(gI, oI, err_msg=what + ": rows")
    np.testing.assert_array_equal(bits(gD), bits(oD), err_msg=what + ": scores")


@pytest.fixture
def idx(oracle):
    from haconvdr_amd.index import FlatIPIndex
    index = FlatIPIndex(D, devices=(0,))
    index.set_option("split", "0")
    index.add(case(oracle)[0])
    assert index.ntotal == N
    return index


def test_inputs_have_no_tie_among_the_first_entries(oracle):
    case(oracle)


@pytest.mark.gpu
def test_masked_all_ones_is_search(idx, oracle):
    x, q, oD, oI = case(oracle)
    same(idx.search_masked(q, K, np.ones(N, bool)), oD[:, :K], oI[:, :K], "search_masked, all ones")
    assert "scan16_masked_kernel" in idx.last_plan(), idx.last_plan()
    idx.check_status()


@pytest.mark.gpu
def test_grouped_by_row_is_search(idx, oracle):
    x, q, oD, oI = case(oracle)
    same(idx.search_grouped(q, K, np.arange(N, dtype=np.int64)), oD[:, :K], oI[:, :K], "search_grouped, label = row")
    assert "scan16_grouped_kernel" in idx.last_plan(), idx.last_plan()
    idx.check_status()


@pytest.mark.gpu
def test_after_from_the_start_and_behind_entry_9(idx, oracle):
    x, q, oD, oI = case(oracle)
    same(idx.search_after(q, K), oD[:, :K], oI[:, :K], "search_after, start cursor")
    assert "scan16_after_kernel" in idx.last_plan(), idx.last_plan()
    after = (oD[:, K - 1].copy(), oI[:, K - 1].copy())
    same(idx.search_after(q, K, after), oD[:, K:2 * K], oI[:, K:2 * K], "search_after, behind entry 9")
    idx.check_status()


@pytest.mark.gpu
def test_range_above_entry_10_is_the_ten_in_front(idx, oracle):
    x, q, oD, oI = case(oracle)
    lims, gD, gI = idx.range_search(q, oD[:, K].copy())
    np.testing.assert_array_equal(lims, np.arange(NQ + 1) * K)
    same((gD.reshape(NQ, K), gI.reshape(NQ, K)), oD[:, :K], oI[:, :K], "range_search")
    idx.check_status()


@pytest.mark.gpu
def test_entries_at_ranks_0_9_199(idx, oracle):
    x, q, oD, oI = case(oracle)
    ranks = np.array([0, K - 1, N - 1], np.int64)
    same(idx.entries_at(q, np.tile(ranks, (NQ, 1))), oD[:, ranks], oI[:, ranks], "entries_at")
    idx.check_status()
