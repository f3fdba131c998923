"""remove_ids without a GPU: the compaction kernel's source formula, the argument check of FlatIPIndex.remove_ids and the span
rewrite of a multi-device index, each against np.delete."""
import numpy as np
import pytest

from tests import remove_ref


# ---------------------------------------------------------------------------------------------------------------------
# 1. src(j) = j + t of compact_rows_kernel
def _check_src_map(n, rem):
    rem = np.asarray(rem, np.int64)
    want = np.delete(np.arange(n), rem)
    np.testing.assert_array_equal(remove_ref.src_map(rem, n - len(rem)), want, err_msg=f"n={n} rem={rem.tolist()[:20]}")
    assert (want >= np.arange(len(want))).all()          # what makes the in-place order safe: a row never moves up


@pytest.mark.parametrize("n,rem", [
    (200, []),
    (200, [0]),
    (200, [199]),
    (200, list(range(64, 128))),
    (200, list(range(0, 200, 2))),
    (200, list(range(1, 200))),
    (200, list(range(0, 199))),
    (200, list(range(50, 141))),                         # a run across 64 and 128
    (64, list(range(64))),
], ids=["nothing", "first", "last", "one-group", "every-other", "all-but-first", "all-but-last", "run-across-groups", "everything"])
def test_src_map_equals_np_delete(n, rem):
    _check_src_map(n, rem)


def test_src_map_equals_np_delete_random():
    rng = np.random.RandomState(0x5EED)
    for _ in range(200):
        n = int(rng.randint(1, 1001))
        R = int(rng.randint(0, n + 1)) if rng.rand() < 0.5 else int(rng.randint(0, min(n, 8) + 1))
        _check_src_map(n, np.sort(rng.choice(n, size=R, replace=False)))


def test_reference_helpers():
    x = np.arange(10)
    ids = np.array([7, -1, 2, 7, 2])
    np.testing.assert_array_equal(remove_ref.removed(x, ids), [0, 1, 3, 4, 5, 6, 8, 9])
    np.testing.assert_array_equal(remove_ref.renumber([[0, 1, 3], [9, -1, 8]], ids), [[0, 1, 2], [7, -1, 6]])


# ---------------------------------------------------------------------------------------------------------------------
# 2. the argument check: ValueError before the library is called
def test_remove_args():
    from haconvdr_amd.index import _remove_args
    with pytest.raises(ValueError, match="integers"):
        _remove_args(np.array([1.0, 2.0]), 10)
    with pytest.raises(ValueError, match="dimension"):
        _remove_args(np.array([[1, 2], [3, 4]]), 10)
    with pytest.raises(ValueError, match="int64"):
        _remove_args(np.array([1, 2 ** 63], np.uint64), 10)
    with pytest.raises(ValueError, match="mask"):
        _remove_args(np.zeros(9, bool), 10)
    with pytest.raises(ValueError, match="mask"):
        _remove_args(np.zeros((2, 5), bool), 10)
    mask = np.zeros(10, bool)
    mask[[2, 3, 9]] = True
    got = _remove_args(mask, 10)
    assert got.dtype == np.int64 and got.flags.c_contiguous
    np.testing.assert_array_equal(got, [2, 3, 9])
    got = _remove_args(np.array([5, -1, 5, 0], np.int32), 10)       # duplicates and padding pass through: the library's business
    assert got.dtype == np.int64
    np.testing.assert_array_equal(got, [5, -1, 5, 0])
    assert _remove_args(np.zeros(0, np.int64), 10).shape == (0,)
    assert _remove_args(np.zeros(0, bool), 0).shape == (0,)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the spans of a multi-device index
def _spans_of_adds(S, adds):
    """hac_index_add's split: per shard a list of [local0, count, global0], one per add that gave the shard a row"""
    spans, rows, total = [[] for _ in range(S)], [0] * S, 0
    for n in adds:
        off = 0
        for s in range(S):
            m = n // S + (1 if s < n % S else 0)
            if m:
                spans[s].append([rows[s], m, total + off])
                rows[s] += m
            off += m
        total += n
    return spans, total


def _rewrite_spans(spans, rem):
    """rewrite_spans_after_remove of haconvdr_amd/csrc/rows_host.inc, restated: per span rows -= the removed rows inside it,
    global0 -= the removed rows below the old global0, local0 = the running sum of the shard's spans; empty spans are dropped."""
    rem = np.asarray(rem, np.int64)
    out = []
    for shard in spans:
        kept, local0 = [], 0
        for _, count, global0 in shard:
            below = int(np.searchsorted(rem, global0, side="left"))
            inside = int(np.searchsorted(rem, global0 + count, side="left")) - below
            if count - inside == 0:
                continue
            kept.append([local0, count - inside, global0 - below])
            local0 += count - inside
        out.append(kept)
    return out


def _placement(spans, total):
    """global row -> (shard, local row) of a span table; every global row exactly once"""
    where = np.full((total, 2), -1, np.int64)
    for s, shard in enumerate(spans):
        for local0, count, global0 in shard:
            assert (where[global0:global0 + count] == -1).all()
            where[global0:global0 + count, 0] = s
            where[global0:global0 + count, 1] = local0 + np.arange(count)
    assert (where >= 0).all()
    return where


@pytest.mark.parametrize("S", [2, 3])
def test_span_rewrite_places_every_survivor_where_its_shard_keeps_it(S):
    adds = [103, 1, 58]                                  # the one-row add gives shard 0 alone a span: removing that row empties it
    spans, total = _spans_of_adds(S, adds)
    before = _placement(spans, total)
    rng = np.random.RandomState(7 + S)
    rem = np.unique(np.concatenate([[0, 103, total - 1], rng.choice(total, 40, replace=False)]))
    assert all((before[rem, 0] == s).any() for s in range(S))     # every shard loses a row
    after = _rewrite_spans(spans, rem)
    assert sum(len(a) for a in after) == sum(len(b) for b in spans) - 1     # the emptied span is gone
    got = _placement(after, total - len(rem))
    # what the shards do: each keeps its surviving rows in order, so a survivor's new local row is its old one minus the removed
    # rows of ITS shard in front of it, and its new global row is np.delete's
    keep = np.delete(np.arange(total), rem)
    want = before[keep].copy()
    for s in range(S):
        gone = np.sort(before[rem][before[rem, 0] == s, 1])
        mine = want[:, 0] == s
        want[mine, 1] -= np.searchsorted(gone, want[mine, 1], side="left")
    np.testing.assert_array_equal(got, want)
    # and that is where adding the survivors' shares span by span would have put them: per shard the local rows are dense
    for s in range(S):
        np.testing.assert_array_equal(np.sort(got[got[:, 0] == s, 1]), np.arange((got[:, 0] == s).sum()))
