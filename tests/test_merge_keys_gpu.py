"""merge_keys_kernel and keys_to_results_kernel alone, on synthetic keys: no index.  The merge runs for every multi-block
and multi-shard search (the reference's add / search / reset loop); its buffer holds Cm = next_pow2(k + 256) keys and is
compacted to the k best when more than Cm - 256 are buffered, so at k = 256, 768 and 1792 it is exactly full after a
compaction plus one chunk of 256.  Keys are built with tests/doubles.py (pack_keys), the expected output is doubles.merge /
doubles.to_results: every comparison is of whole 64-bit keys, float words and int64 ids.

One launch merges five queries, each with a pattern of its own (a wrong query stride mixes them up):
  0 improving:  every key of list l + 1 beats all of list l (everything passes the running threshold);
  1 worsening:  everything after the first list is rejected by it;
  2 random:     lists interleave at random;
  3 short:      lists filled with 0 .. k keys, the rest empty, at least one list empty (L >= 2); the whole query empty
                where L is 3 or 40;
  4 ties:       one score for every key: the order is position ascending across the lists.
Within a query all positions are distinct, as the contract has it."""
import numpy as np
import pytest

from tests import doubles

pytestmark = pytest.mark.gpu

FMAX = np.finfo(np.float32).max
KS = (1, 100, 256, 257, 768, 769, 1792, 1793, 2048)
LS = (1, 2, 3, 9, 40)
NQ = 5


def _lists(k, L, seed):
    """(D float32 [L, NQ, k], pos int64 [L, NQ, k]), every list sorted by key descending, empty slots (pos -1) last."""
    rng = np.random.default_rng(seed)
    D = np.zeros((L, NQ, k), np.float32)
    pos = np.full((L, NQ, k), -1, np.int64)
    for qi in range(NQ):
        p = rng.permutation(L * k).reshape(L, k).astype(np.int64) + 1000 * qi       # distinct within the query
        if qi == 0:
            s = np.arange(L, dtype=np.float32)[:, None] * 4.0 + rng.random((L, k), dtype=np.float32)
        elif qi == 1:
            s = -np.arange(L, dtype=np.float32)[:, None] * 4.0 + rng.random((L, k), dtype=np.float32)
        elif qi in (2, 3):
            s = rng.standard_normal((L, k)).astype(np.float32)
        else:
            s = np.full((L, k), 0.625, np.float32)
        fill = np.full(L, k)
        if qi == 3:
            fill = rng.integers(0, k + 1, L)
            if L >= 2:
                fill[rng.integers(0, L)] = 0
            if L in (3, 40):
                fill[:] = 0
        for l in range(L):
            n = int(fill[l])
            keys = doubles.pack_keys(s[l, :n], p[l, :n]).view(np.uint64)
            order = np.argsort(keys, kind="stable")[::-1]
            D[l, qi, :n] = s[l, :n][order]
            pos[l, qi, :n] = p[l, :n][order]
    return D, pos


def _run_merge(D, pos):
    import torch
    from haconvdr_amd.index import merge_keys
    keys = doubles.pack_keys(D, pos)
    u = keys.view(np.uint64)
    assert (u[..., :-1] >= u[..., 1:]).all()                                        # sorted lists, empty slots (0) last
    want = doubles.merge(torch.from_numpy(keys))
    got = merge_keys(torch.from_numpy(keys).cuda())
    torch.cuda.synchronize()
    return got, want


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("k", KS)
def test_merge_at_its_buffer_edges(k, L):
    import torch
    from haconvdr_amd.index import keys_to_results
    D, pos = _lists(k, L, 0x3E6 + 64 * k + L)
    got, want = _run_merge(D, pos)
    g, w = got.cpu().numpy().view(np.uint64), want.numpy().view(np.uint64)
    for qi in range(NQ):
        np.testing.assert_array_equal(g[qi], w[qi], err_msg=f"query {qi} (k={k}, L={L})")
    # what the patterns promise, from the expected keys themselves
    live = (w != 0).sum(1)
    assert live[0] == live[1] == live[2] == live[4] == k
    if L in (3, 40):
        assert live[3] == 0
    wD, wpos = doubles.unpack_keys(want.numpy())
    if L > 1:
        assert wD[0].min() >= 4.0 * (L - 1) and wD[1].min() >= 0.0                  # improving: the last list alone; worsening: the first
    assert (np.diff(wpos[4]) > 0).all() if k > 1 else True                          # ties: position ascending
    # ... and on through keys_to_results, without and with an id_map
    id_map = (np.random.default_rng(k + L).integers(-2 ** 62, 2 ** 62, 1000 * NQ + L * k)).astype(np.int64)
    for m in (None, id_map):
        Dg, Ig = keys_to_results(got, None if m is None else torch.from_numpy(m).cuda())
        torch.cuda.synchronize()
        Dw, Iw = doubles.to_results(want, m)
        np.testing.assert_array_equal(Dg.cpu().numpy().view(np.uint32), np.ascontiguousarray(Dw, np.float32).view(np.uint32))
        np.testing.assert_array_equal(Ig.cpu().numpy(), Iw)
        assert (Iw[w == 0] == -1).all() and (Dw[w == 0] == -FMAX).all()


def test_results_at_the_position_and_score_extremes():
    """Positions 0 and 2^32 - 2, scores +-0.0 (both pack as +0.0), the smallest denormal, +-FLT_MAX, +-Inf, empty slots: through
    keys_to_results directly, and merged first."""
    import torch
    from haconvdr_amd.index import keys_to_results, merge_keys
    tiny = np.float32(1e-45)
    scores = np.array([np.inf, FMAX, 1.0, tiny, 0.0, -0.0, -tiny, -1.0, -FMAX, -np.inf], np.float32)
    assert scores[3].view(np.uint32) == 1 and scores[6].view(np.uint32) == 0x80000001
    top = 2 ** 32 - 2
    rows = []
    for positions in (np.arange(10), top - np.arange(10), np.array([0, top] * 5)):
        rows.append((scores, positions.astype(np.int64)))
    # one score at both extreme positions, and the other way round; then a mostly empty and an empty list
    rows.append((np.array([FMAX, FMAX, 0.0, -0.0, -FMAX, -FMAX, -np.inf, -np.inf, 0, 0], np.float32),
                 np.array([0, top, 0, top, 0, top, 0, top, -1, -1], np.int64)))
    rows.append((np.zeros(10, np.float32), np.array([top] + [-1] * 9, np.int64)))
    rows.append((np.zeros(10, np.float32), np.full(10, -1, np.int64)))
    D = np.stack([r[0] for r in rows])
    pos = np.stack([r[1] for r in rows])
    keys = doubles.pack_keys(D, pos)
    u = keys.view(np.uint64)
    assert (u[pos >= 0] != 0).all() and (u[pos < 0] == 0).all()
    wD, wI = doubles.to_results(torch.from_numpy(keys))
    np.testing.assert_array_equal(wI, pos)
    np.testing.assert_array_equal(wD.view(np.uint32)[pos >= 0], (D + np.float32(0.0)).view(np.uint32)[pos >= 0])
    assert not (wD.view(np.uint32) == 0x80000000).any()                             # -0.0 never comes back
    Dg, Ig = keys_to_results(torch.from_numpy(keys).cuda())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(Dg.cpu().numpy().view(np.uint32), wD.view(np.uint32))
    np.testing.assert_array_equal(Ig.cpu().numpy(), wI)
    # with an id_map (positions that index it), ids at the int64 extremes
    small = np.where(pos >= 0, pos % 16, -1)
    id_map = np.array([np.iinfo(np.int64).max, np.iinfo(np.int64).min, -1, 0] * 4, np.int64)
    keys_s = doubles.pack_keys(D, small)
    wD, wI = doubles.to_results(torch.from_numpy(keys_s), id_map)
    Dg, Ig = keys_to_results(torch.from_numpy(keys_s).cuda(), torch.from_numpy(id_map).cuda())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(Dg.cpu().numpy().view(np.uint32), wD.view(np.uint32))
    np.testing.assert_array_equal(Ig.cpu().numpy(), wI)
    # merged first: each row as one query, its keys dealt to two sorted lists of k = 10 (odd and even ranks), the rest empty
    order = np.argsort(u, axis=1)[:, ::-1]
    srt = np.take_along_axis(u, order, 1)
    lists = np.zeros((2, len(rows), 10), np.uint64)
    lists[0, :, :5], lists[1, :, :5] = srt[:, 0::2], srt[:, 1::2]
    for l in range(2):                                                              # (empty slots last)
        lists[l] = np.sort(lists[l], axis=1)[:, ::-1]
    lists = np.ascontiguousarray(lists).view(np.int64)
    want = doubles.merge(torch.from_numpy(lists))
    got = merge_keys(torch.from_numpy(lists).cuda())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), want.numpy())
    np.testing.assert_array_equal(want.numpy().view(np.uint64), srt)                # nothing lost: the same keys, in order
    Dg, Ig = keys_to_results(got)
    torch.cuda.synchronize()
    wD, wI = doubles.to_results(want)
    np.testing.assert_array_equal(Dg.cpu().numpy().view(np.uint32), wD.view(np.uint32))
    np.testing.assert_array_equal(Ig.cpu().numpy(), wI)
