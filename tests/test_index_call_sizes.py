"""The inputs of tests/test_index_call_sizes_gpu.py do what they are for -- proved on the CPU oracle alone, at the shapes the
GPU file uses -- and its comparison helpers reject references altered in the ways a wrong offset or a wrong merge would alter
a result.  A copied offset bug moves a result to another query: the inputs must tell every query from its neighbours one and
two launches away."""
import numpy as np
import pytest

from tests import call_sizes as cs
from tests import range_ref, rank_ref

N = cs.SORT_N
CHUNK = cs.QUERY_CHUNK


def _same_list(want, i, j):
    (Di, Ii), (Dj, Ij) = cs.lists(want, i), cs.lists(want, j)
    return np.array_equal(Ii, Ij) and np.array_equal(range_ref.bits(Di), range_ref.bits(Dj))


def test_launches_and_the_plan_of_the_last_one():
    assert cs.launches(1024) == [(0, 1024)] and cs.launches(1025) == [(0, 1024), (1024, 1)]
    assert cs.launches(2049) == [(0, 1024), (1024, 1024), (2048, 1)]
    assert [cs.last_launch_plan(nq) for nq in cs.SEAM_NQ] == [(16, 64), (1, 1), (16, 2), (1, 1)]
    assert all((min(16, nq), -(-nq // 16)) != cs.last_launch_plan(nq) for nq in cs.SEAM_NQ[1:])    # one launch of nq would say otherwise


@pytest.mark.parametrize("nq", cs.SEAM_NQ)
@pytest.mark.parametrize("d", cs.SEAM_D)
def test_every_seam_query_differs_from_the_queries_a_launch_before(d, nq, oracle):
    c = cs.seam(d, nq, oracle)
    want, radius, S = c["want"], c["radius"], c["S"]
    assert c["x"].shape == (cs.SEAM_N, d) and c["q"].shape == (nq, d) and cs.SEAM_N % 64
    lens = np.diff(want[0])
    rank_cases = [cs.seam_rank(c, m) for m in (1, 9)]
    for i in range(CHUNK, nq):
        for j in (i - CHUNK, i - 2 * CHUNK):
            if j < 0:
                continue
            assert not _same_list(want, i, j), (i, j)
            assert range_ref.bits(radius[i]) != range_ref.bits(radius[j]), (i, j)
            assert not np.array_equal(c["q"][i], c["q"][j], equal_nan=True)
            for ids, ranks, own in rank_cases:
                assert not np.array_equal(ranks[i], ranks[j]), (i, j, ranks[i])
                assert not np.array_equal(own[i], own[j], equal_nan=True), (i, j)
    # every launch of more than one query holds an empty and a non-empty list; a launch of one query (QT = 1) a non-empty one:
    # an empty list there would be what a launch that never ran leaves behind
    for off, n in cs.launches(nq):
        assert (lens[off:off + n] > 0).any(), off
        assert n == 1 or (lens[off:off + n] == 0).any(), off
    # the lengths follow the query: 5 + i % 41 away from ties and special radii, so they differ across 1024 (= 40 mod 41)
    plain = np.array([i not in cs.SPECIALS for i in range(nq)])
    assert (np.abs(lens[plain] - (5 + np.arange(nq)[plain] % 41)) <= len(cs.TIE_ROWS)).all()


@pytest.mark.parametrize("d", cs.SEAM_D)
def test_the_specials_are_what_they_are_called(d, oracle):
    c = cs.seam(d, 2049, oracle)
    S, q, want, radius, T = c["S"], c["q"], c["want"], c["radius"], c["table"]
    lens = np.diff(want[0])
    ok = ~np.isnan(S)
    assert sorted(cs.SPECIALS) == [1022, 1023, 1024, 1025, 1026, 2047, 2048]
    assert np.isnan(S[:, cs.NAN_ROW]).all() and ok[np.arange(2049) != 1023].sum(1).min() > 150
    assert np.isnan(q[1023]).sum() == 1 and not ok[1023].any() and lens[1023] == 0 and (T[1023] == -1).all()
    assert not q[1024].any() and (S[1024][ok[1024]] == 0).all() and lens[1024] == ok[1024].sum() > 150
    np.testing.assert_array_equal(cs.lists(want, 1024)[1], np.flatnonzero(ok[1024]))          # one tie, in row order
    assert np.array_equal(q[1025], -q[1026]) and np.array_equal(q[2048], -q[2047]) and np.array_equal(q[0], -q[1])
    assert lens[1022] == 0 and np.isposinf(radius[1022]) and lens[1026] == 0 and np.isnan(radius[1026])
    assert lens[1025] == 0 and radius[1025] == S[1025][ok[1025]].max()                          # strictness alone empties it
    assert np.isneginf(radius[2047]) and lens[2047] == (ok[2047] & ~np.isneginf(S[2047])).sum() > 150
    assert 0 < lens[2048] < 50
    a, b, e = cs.TIE_ROWS                                                                       # the tied rows: neighbours in every search, in row order
    assert (range_ref.bits(S[:, a]) == range_ref.bits(S[:, b])).all() and (range_ref.bits(S[:, a]) == range_ref.bits(S[:, e])).all()
    live = ok[:, a] & (np.arange(2049) != 1024)                                                 # (the zero query ties every row)
    assert live.sum() >= 2040 and (T[live, b] == T[live, a] + 1).all() and (T[live, e] == T[live, a] + 2).all()
    # what stands in the columns of the second and third launch: -1, the NaN row, and ties the bound decides
    for m in (1, 9):
        ids, ranks, own = cs.seam_rank(c, m)
        for off, n in cs.launches(2049)[1:2]:
            part = ids[off:off + n]
            assert (part == -1).any() and (part == cs.NAN_ROW).any() and np.isin(part, cs.TIE_ROWS[1:]).any()
        assert (ranks[ids == -1] == -1).all() and (ranks[ids == cs.NAN_ROW] == -1).all()
        assert ids.min() == -1 and ids.max() < cs.SEAM_N and (ids[:CHUNK] >= 0).all()
        np.testing.assert_array_equal(ranks, np.where(ids >= 0, np.take_along_axis(T, np.clip(ids, 0, None), 1), -1))     # counting == sorting
    ids, ranks, own = cs.seam_rank(c, 9)
    assert set(ids[2048].tolist()) >= {-1, cs.NAN_ROW, a, b} and ranks[2048][ids[2048] == b] == ranks[2048][ids[2048] == a] + 1
    assert np.isin(cs.seam_rank(c, 1)[0][[1024, 2048], 0], cs.TIE_ROWS).all()


def test_the_helpers_reject_results_moved_between_queries(oracle):
    for nq in (1025, 2049):
        c = cs.seam(32, nq, oracle)
        want = c["want"]
        range_ref.assert_same(tuple(a.copy() for a in want), want)
        for by in (CHUNK, 2 * CHUNK):
            if by >= nq:
                continue
            moved = cs.moved_by_a_launch(c, by)              # queries 1024.. answered as queries 0..
            for pair in ((moved, want), (want, moved)):
                with pytest.raises(AssertionError):
                    range_ref.assert_same(*pair)
            with pytest.raises(AssertionError):              # ... range_count's comparison too
                np.testing.assert_array_equal(np.diff(moved[0]), np.diff(want[0]))
            for m in (1, 9):
                ids, ranks, own = cs.seam_rank(c, m)
                wrong = ranks.copy()
                wrong[by:] = ranks[:nq - by]
                with pytest.raises(AssertionError):
                    np.testing.assert_array_equal(wrong, ranks)
                wrong = rank_ref.count_ahead(c["S"], np.concatenate([own[:by], own[:nq - by]]), ids)   # ref_score without its offset
                with pytest.raises(AssertionError):
                    np.testing.assert_array_equal(wrong, ranks)
                stale = own.copy()
                stale[by:] = own[:nq - by]
                with pytest.raises(AssertionError):
                    cs.assert_scores(stale, own)
        # one tie swapped: the all-zero query's list is one tie in row order
        lo = int(want[0][1024])
        assert want[1][lo] == want[1][lo + 1] == 0
        swapped = want[2].copy()
        swapped[[lo, lo + 1]] = swapped[[lo + 1, lo]]
        with pytest.raises(AssertionError):
            range_ref.assert_same((want[0], want[1], swapped), want)
        # lims shifted by one query, the lists as they are
        shifted = np.concatenate([want[0][:1], want[0][:-1]])
        shifted[-1] = want[0][-1]
        with pytest.raises(AssertionError):
            range_ref.assert_same((shifted, want[1], want[2]), want)
    cs.assert_scores(np.array([np.nan, 1.0], np.float32), np.array([-np.nan, 1.0], np.float32))      # a NaN's payload is left open
    with pytest.raises(AssertionError):
        cs.assert_scores(np.array([0.0], np.float32), np.array([-0.0], np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# 2. runs of range_offsets_kernel
_OFFSETS = {}


def _offsets_case(oracle):
    if not _OFFSETS:
        _OFFSETS["case"] = cs.planted(32, N + 70, max(cs.OFFSETS_NQ), 0x7D0, oracle)
    return _OFFSETS["case"]


@pytest.mark.parametrize("nq", cs.OFFSETS_NQ)
def test_offsets_lengths_are_the_planned_ones(nq, oracle):
    x, q, S = _offsets_case(oracle)
    assert np.all(np.diff(S, axis=1) > 0)                    # no ties: the radius alone sets the length
    L = cs.offsets_lengths(nq, N)
    want = range_ref.range_from_scores(S[:nq], cs.radii_for_lengths(S[:nq], L))
    np.testing.assert_array_equal(np.diff(want[0]), L)
    n = len(x)
    for i in (0, 9 * -(-nq // 256), nq // 2, nq - 2):
        np.testing.assert_array_equal(cs.lists(want, i)[1], n - 1 - np.arange(L[i]))
    assert 4 * N < L.sum() < 40000
    per = -(-nq // 256)
    runs = cs.runs(nq)
    assert per == {255: 1, 256: 1, 257: 2, 511: 2, 513: 3, 1000: 4}[nq]
    assert runs[0] == (0, per) and max(hi for lo, hi in runs) == nq and all(hi - lo <= per for lo, hi in runs)
    behind = [t for t, (lo, hi) in enumerate(runs) if lo == hi]
    assert len(behind) == 256 - -(-nq // per) and (nq in (255, 256, 511) or len(behind) >= 6)      # runs behind nq, from nq = 257
    whole_empty = [t for t, (lo, hi) in enumerate(runs) if hi - lo == per and not L[lo:hi].any()]
    assert {1, 2, 5} <= set(whole_empty)
    lo, hi = runs[7]
    assert L[lo] == (3 if per > 1 else 5) and L[hi - 1] == 5 and not L[lo + 1:hi - 1].any()
    if per > 1:
        assert L[lo:hi].sum() == 8
    lo, hi = runs[9]
    assert L[lo] == N and L[lo + 1] == N + 1 and (per == 1 or hi - lo >= 2)                       # blk + 1, then blk + 2, inside one run
    assert sorted(L[nq // 2:nq // 2 + 2].tolist()) == [N, N + 1]
    assert (L[-1] == 0) == (nq in cs.OFFSETS_LAST_EMPTY)
    blocks = -(-L // N)
    assert set(blocks.tolist()) == {0, 1, 2} and (np.diff(want[0]) >= N).sum() == 4


# ---------------------------------------------------------------------------------------------------------------------
# 3. merge depth, uneven pairs, ties across blocks and tiles
def test_merge_sets_have_the_planned_lengths_and_passes(oracle):
    n = 8 * N + 70
    x, q, S = cs.planted(32, n, 6, 0x7D8, oracle)
    assert np.all(np.diff(S, axis=1) > 0)
    sets = cs.merge_sets(N)
    for name, (lengths, extra) in sets.items():
        k = len(lengths)
        want = range_ref.range_from_scores(S[:k], cs.radii_for_lengths(S[:k], lengths))
        np.testing.assert_array_equal(np.diff(want[0]), lengths, err_msg=name)
        np.testing.assert_array_equal(cs.lists(want, 0)[1], n - 1 - np.arange(lengths[0]))
    first = sets["0 to 3 passes side by side"][0]
    assert [cs.passes_of(c, N) for c in first] == [3, 0, 1, 0, 3, 0]
    assert cs.passes_of(sum(first), N) == 4                                     # the call plans one more than its deepest segment
    # the 4N + 1 segment: passes of runs N, 2N, 4N -- the third merges a = 4N keys with b = 1 key
    assert first[0] - 4 * N == 1 and first[4] - 4 * N == N
    deep = sets["4 passes, 8N meets 1"][0]
    assert [cs.passes_of(c, N) for c in deep] == [4, 2] and cs.passes_of(sum(deep), N) == 4 and deep[0] - 8 * N == 1
    lengths, extra = sets["more passes than any segment needs"]
    assert cs.passes_of(min(sum(lengths) + extra, 6 * n), N) == 6 > max(cs.passes_of(c, N) for c in lengths)
    assert cs.passes_of(1, N) == 0 and cs.passes_of(N, N) == 0 and cs.passes_of(N + 1, N) == 1 and cs.passes_of(4 * N + 1, N) == 3


def test_tie_runs_cross_sorted_blocks_and_merge_tiles(oracle):
    x, q, S, radius = cs.tie_case(32, N, oracle)
    n = len(x)
    assert n == 5 * N + 70 and len(np.unique(x, axis=0)) == 16
    want = range_ref.range_from_scores(S, radius)
    lens = np.diff(want[0])
    assert lens[0] > 4 * N and 4 * N > lens[1] > N > lens[2] > 0 and lens[3] == 0, lens
    for i in range(3):
        D, I = cs.lists(want, i)
        values, counts = np.unique(S[i], return_counts=True)
        assert len(values) >= 8 and counts.min() >= n // 16 > N // 4           # every score value is shared by about N / 3 rows
        assert (S[i] == radius[i]).sum() >= n // 16 and not (D == radius[i]).any()      # the radius sits on a shared value
        same = np.diff(D) == 0
        assert same.mean() > 0.99 and (np.diff(I)[same] > 0).all()              # rows ascend inside every tie
        assert (np.diff(D)[~same] < 0).all()
    for i, offsets in ((0, (N, 2 * N, 3 * N, 4 * N)), (1, (N,))):               # a tie run spans the block / tile boundaries
        D, I = cs.lists(want, i)
        for o in offsets:
            assert D[o - 1] == D[o] and I[o - 1] < I[o], (i, o)
    # one tie swapped across the boundary at 4N is rejected
    lo = int(want[0][0]) + 4 * N
    swapped = want[2].copy()
    swapped[[lo - 1, lo]] = swapped[[lo, lo - 1]]
    with pytest.raises(AssertionError):
        range_ref.assert_same((want[0], want[1], swapped), want)


# ---------------------------------------------------------------------------------------------------------------------
# 4. one workspace, many shapes
def test_workspace_case_lengths_and_ranks(oracle):
    w = cs.workspace_case(32, N, oracle)
    n, ids = w["n"], w["ids"]
    np.testing.assert_array_equal(np.diff(w["big"][0]), cs.merge_sets(N)["4 passes, 8N meets 1"][0])
    np.testing.assert_array_equal(np.diff(w["small"][0]), w["L"])
    assert w["L"][1024] > 0 and (w["L"] == 0).sum() == 21 and w["L"].sum() < 1024 * 1025      # small lists: the host form's first call fits
    assert ids[1024, 1] == -1 and (np.delete(ids.reshape(-1), 2049) >= 0).all()
    np.testing.assert_array_equal(w["ranks"], np.where(ids >= 0, n - 1 - ids, -1))             # row r has rank n - 1 - r
