"""search_grouped without a GPU: the argument checks of the Python layer, the identities of include/haconvdr.h ("search by
group") proved over the CPU oracle's canonical scores, and proofs that the inputs of tests/test_index_grouped_gpu.py show what
they are for."""
import numpy as np
import pytest

from tests import grouped_cases, grouped_ref, masked_cases, masked_ref, range_ref, rank_ref

D, N, NQ = grouped_cases.D, grouped_cases.N, grouped_cases.NQ
MAX_K = grouped_cases.MAX_K
_BASE = {}


def _base(oracle):
    if not _BASE:
        x, q = masked_cases.base_case()
        S = rank_ref.canon_scores(oracle, x, q)
        S.setflags(write=False)
        _BASE["case"] = (x, q, S)
    return _BASE["case"]


def _planted_scores():
    """float32 [6, 400]: ties, NaN, +-Inf planted so that whole groups score NaN, -Inf, or lose their best row to a NaN"""
    from haconvdr_amd import synth
    S = ((synth.uniform_u32(0xB30, 6 * 400) % np.uint32(41)).astype(np.float32).reshape(6, 400) - 20.0) / 4.0
    S[:, 0:400:40] = np.nan            # label r % 40 == 0: ten NaN rows ...
    S[1, 5:400:40] = -np.inf           # a group that scores -Inf throughout
    S[2, 7] = np.inf
    S[3, :] = np.nan                   # a NaN query
    S[4, :] = 0.0                      # everything ties: row order
    S[5, 200:] = -np.inf               # half the rows at -Inf
    return rank_ref.canon(S)


# ---------------------------------------------------------------------------------------------------------------------
# argument checks
def test_argument_checks():
    from haconvdr_amd import _lib
    from haconvdr_amd.index import _grouped_args, _grouped_args_tensor
    q = np.zeros((3, D), np.float32)
    good = np.arange(50, dtype=np.int64)
    qq, k, g = _grouped_args(q, 10, good.astype(np.int32), D, 50)
    assert g.dtype == np.int64 and g.flags.c_contiguous and k == 10 and qq.dtype == np.float32
    _grouped_args(q, 1, good.astype(np.uint64), D, 50)
    _grouped_args(q, _lib.HAC_MAX_K, good, D, 50)
    for bad_q, bad_k, bad_g in ((q, 10, good.astype(np.float32)), (q, 10, good[:-1]), (q, 10, np.arange(51)), (q, 10, good.reshape(5, 10)),
                                (q, 10, good.reshape(50, 1)), (q, 0, good), (q, -1, good), (q, _lib.HAC_MAX_K + 1, good), (q, 2.0, good), (q, True, good),
                                (q[:, :-1], 10, good), (q, 10, np.full(50, 2 ** 63, np.uint64))):
        with pytest.raises(ValueError):
            _grouped_args(bad_q, bad_k, bad_g, D, 50)
    import torch
    with pytest.raises(ValueError):                                        # not a CUDA tensor: refused before the library is called
        _grouped_args_tensor(torch.zeros(3, D), 10, torch.arange(50), None, D, 50)
    assert _lib.HAC_MAX_K == MAX_K


def test_symbols_declared():
    from haconvdr_amd import _lib
    assert {"hac_index_search_grouped", "hac_index_search_grouped_device"} <= set(_lib.EXPORTED_SYMBOLS)
    header = open(__import__("os").path.join(__import__("os").path.dirname(__file__), "..", "include", "haconvdr.h")).read()
    assert "search by group" in header and "hac_index_search_grouped_device(" in header


# ---------------------------------------------------------------------------------------------------------------------
# the five identities
def _score_sets(oracle):
    S = _base(oracle)[2]
    P = _planted_scores()
    labels = grouped_cases.interleaved_labels()
    return [("base r % 7", S, labels["r % 7"]), ("base r // 3", S, labels["r // 3"]), ("base permuted", S, labels["permuted r // 5"]),
            ("planted r % 40", P, np.arange(400, dtype=np.int64) % 40), ("planted r // 9", P, np.arange(400, dtype=np.int64) // 9)]


@pytest.mark.parametrize("k", [1, 10, 100, 2047, 2048])
def test_distinct_labels_are_search(k, oracle):
    x, q, S = _base(oracle)
    want = masked_ref.masked_from_scores(S, np.ones(N, np.bool_), None, k)
    got = grouped_ref.grouped_from_scores(S, np.arange(N, dtype=np.int64), k)
    grouped_ref.assert_same(got[:2], (want[0], want[1], None))
    np.testing.assert_array_equal(got[2], want[1])                         # the label of row r is r; -1 in padding
    if k == 100:
        oD, oI = oracle.flat_ip_search(x, q, k)
        grouped_ref.assert_same(got[:2], (rank_ref.canon(oD), oI, None))
    P = _planted_scores()
    grouped_ref.assert_same(grouped_ref.grouped_from_scores(P, np.arange(400) * 7 + 2 ** 31, k)[:2],
                            masked_ref.masked_from_scores(P, np.ones(400, np.bool_), None, k) + (None,))


def test_one_label_is_the_best_row_and_padding(oracle):
    for S in (_base(oracle)[2], _planted_scores()):
        n = S.shape[1]
        for k in (1, 7):
            top = masked_ref.masked_from_scores(S, np.ones(n, np.bool_), None, 1)
            D, I, G = grouped_ref.grouped_from_scores(S, np.full(n, 5, np.int64), k)
            np.testing.assert_array_equal(I[:, :1], top[1])
            np.testing.assert_array_equal(grouped_ref.bits(D[:, :1]), grouped_ref.bits(top[0]))
            assert (I[:, 1:] == -1).all() and (G[:, 1:] == -1).all() and (D[:, 1:] == -grouped_ref.FMAX).all()
            assert ((G[:, 0] == 5) == (I[:, 0] >= 0)).all()


def _rep_masks(S, g):
    """bool [nq, n]: per query the representative of every label, found label by label (not by a de-dup of a sorted list)"""
    nq, n = S.shape
    M = np.zeros((nq, n), np.bool_)
    for i in range(nq):
        for lab in np.unique(g):
            rows = np.flatnonzero((g == lab) & ~np.isnan(S[i]))
            if len(rows):
                M[i, rows[np.lexsort((rows, -S[i, rows].astype(np.float64)))[0]]] = True
    return M


def test_mask_form_rank_form_and_range_form(oracle):
    for name, S, g in _score_sets(oracle):
        S = S[:6]
        nq, n = S.shape
        n_labels = len(np.unique(g))
        M = _rep_masks(S, g)
        lims, rD, rI = range_ref.range_from_scores(S, -np.inf)
        for k in (1, 10, n_labels - 1, n_labels, n_labels + 1):
            if not 1 <= k <= MAX_K:
                continue
            want = grouped_ref.grouped_from_scores(S, g, k)
            D, I, G = want
            # mask form
            grouped_ref.assert_same(masked_ref.masked_from_scores(S, M, None, k), want, f"{name} k={k} mask form")
            # ranks: strictly increasing, >= the slot; score_ids has the bits of D
            ranks = rank_ref.rank_ids_from_scores(S, I)
            for i in range(nq):
                m = int((I[i] >= 0).sum())
                assert (I[i, m:] == -1).all() and (ranks[i, m:] == -1).all()
                assert (np.diff(ranks[i, :m]) > 0).all() and (ranks[i, :m] >= np.arange(m)).all(), (name, k, i)
                np.testing.assert_array_equal(grouped_ref.bits(S[i, I[i, :m]]), grouped_ref.bits(D[i, :m]))
                np.testing.assert_array_equal(G[i, :m], g[I[i, :m]])
                # range form: the rows above -inf at their label's first occurrence, then the -Inf representatives if there is room
                rows = rI[lims[i]:lims[i + 1]]
                first = rows[np.sort(np.unique(g[rows], return_index=True)[1])][:k]
                seen = set(g[rows].tolist())
                tail = [r for r in np.flatnonzero(M[i] & np.isneginf(S[i])) if g[r] not in seen]
                np.testing.assert_array_equal(np.concatenate([first, np.asarray(tail, np.int64)])[:k], I[i, :m], err_msg=f"{name} k={k} query {i}")
    P = _planted_scores()
    gp = np.arange(400, dtype=np.int64) % 40
    D, I, G = grouped_ref.grouped_from_scores(P, gp, 40)
    assert (I[3] == -1).all()                                              # a NaN query: padding only
    assert 0 not in G[0] and (G[0] >= 0).sum() == 39                       # a group of NaN rows only is absent
    assert np.isneginf(D[1, 38]) and G[1, 38] == 5 and np.isposinf(D[2, 0]) and I[2, 0] == 7       # +-Inf are ordinary scores
    np.testing.assert_array_equal(I[4], np.arange(40))                     # everything ties: the lowest row of each label, in row order


def test_out_of_range_labels_are_in_no_list():
    P = _planted_scores()
    g = np.arange(400, dtype=np.int64) % 40
    best = grouped_ref.grouped_from_scores(P, g, 40)[1]
    wild = g.copy()
    wild[best[0, 0]] = -1                                                  # the best row of query 0's best group
    wild[best[0, 1]] = 2 ** 32
    D, I, G = grouped_ref.grouped_from_scores(P, wild, 40)
    assert best[0, 0] not in I[0] and best[0, 1] not in I[0]
    assert g[best[0, 0]] in G[0] and g[best[0, 1]] in G[0]                 # the groups are still there, by their next rows
    assert (G >= -1).all() and (G < 2 ** 32).all()


# ---------------------------------------------------------------------------------------------------------------------
# the GPU inputs do what they claim
def test_giant_group_defeats_search_then_dedup(oracle):
    x, q, labels = grouped_cases.giant_case()
    S = rank_ref.canon_scores(oracle, x, q)
    giant = labels == 0
    assert giant.sum() == grouped_cases.GIANT_ROWS > MAX_K
    # the giant group's rows lead every query's list, all of them
    assert (S[:, giant].min(axis=1) > S[:, ~giant].max(axis=1)).all()
    # ... and lie in every 64-row group and on both sides of both add cuts
    assert all(giant[g0:g0 + 64].any() and (~giant[g0:g0 + 64]).any() for g0 in range(0, N, 64))
    for k in (10, 100):
        D, I, G = grouped_ref.grouped_from_scores(S, labels, k)
        assert (G[:, 0] == 0).all() and (G[:, 1:] > 0).all() and (I >= 0).all()
        ranks = rank_ref.rank_ids_from_scores(S, I)
        assert (ranks[:, 1] == grouped_cases.GIANT_ROWS).all()             # the second representative: behind all 3000 giant rows
        assert (ranks[:, k - 1] > MAX_K).all()                             # the k-th is beyond any legal k'
        # a search at the largest legal k' followed by a de-dup falls short: one group
        sD, sI = masked_ref.masked_from_scores(S, np.ones(N, np.bool_), None, MAX_K)
        assert all(len(np.unique(labels[sI[i]])) == 1 for i in range(len(q)))
    # ties inside the giant group: the representative is its lowest row among equals
    D, I, G = grouped_ref.grouped_from_scores(S, labels, 2)
    for i in range(len(q)):
        assert I[i, 0] == np.flatnonzero(S[i] == S[i].max())[0] and (S[i] == S[i].max()).sum() > 100


def test_interleaved_labels_and_label_edges(oracle):
    labels = grouped_cases.interleaved_labels()
    from tests.test_search_plans_gpu import _cuts
    c1, c2 = _cuts(N)
    assert len(np.unique(labels["r % 7"])) == 7 and len(np.unique(labels["r // 3"])) == 1667 and len(np.unique(labels["permuted r // 5"])) == 1000
    p = labels["permuted r // 5"]
    spans = np.array([np.ptp(np.flatnonzero(p == lab)) for lab in range(0, 1000, 37)])
    assert (spans > 64).all() and (spans > 1000).mean() > 0.5             # members far apart: other 64-row groups, other segments
    assert labels["r // 3"][c1 - 1] == labels["r // 3"][c1] or labels["r // 3"][c2 - 1] == labels["r // 3"][c2]      # a group across an add cut
    e = grouped_cases.edge_labels()
    assert {0, 2 ** 32 - 1, 2 ** 31, 2 ** 31 + 5, 2 ** 32 - 12} <= set(e.tolist()) and e.min() == 0 and e.max() == 2 ** 32 - 1
    assert len(np.unique(e)) == 11 and len(np.unique(e.astype(np.int32))) == 11      # (distinct either way: what a truncation breaks is the RANGE check and G)
    assert (e.astype(np.int32) < 0).sum() > 1000
    S = _base(oracle)[2]
    D, I, G = grouped_ref.grouped_from_scores(S, e, 12)
    assert (G[:, :11] >= 0).all() and (G[:, 11] == -1).all() and all(set(G[i, :11].tolist()) == set(e.tolist()) for i in range(NQ))


def test_grid_corpus_ties_across_groups(oracle):
    x, q, g = grouped_cases.grid_tie_corpus(96, 1200, 6, 0xB40)
    S = rank_ref.canon_scores(oracle, x, q)
    assert len(np.unique(g)) == 300
    for k in (37, 150):
        D, I, G = grouped_ref.grouped_from_scores(S, g, k)
        same = np.diff(D, axis=1) == 0
        assert same.sum() > 6 * k // 2 and (np.diff(I, axis=1)[same] > 0).all()      # runs of groups tie; inside a run the rows ascend
    full = grouped_ref.grouped_from_scores(S, g, 38)[0]
    assert sum(full[i, 36] == full[i, 37] for i in range(6)) >= 4          # the cut at 37 falls inside a tie


def test_plan_arithmetic():
    assert grouped_cases.plan_tile(96, 10, 37) == (16, 512, 16 * (384 + 4096) + 4 * 4096 + 128)
    assert grouped_cases.plan_tile(96, 100, 37)[0] == 16
    assert grouped_cases.plan_tile(96, 2048, 37)[0] == 2 and grouped_cases.plan_tile(96, 1000, 37)[0] == 5      # 2 x 33152 + 2 x 32768; 5 x 16768 + 4 x 16384
    assert grouped_cases.plan_tile(768, 2048, 16)[0] == 2 and grouped_cases.plan_tile(768, 100, 16)[0] == 16
    assert grouped_cases.plan_tile(96, 10, 5)[0] == 5


# ---------------------------------------------------------------------------------------------------------------------
# ResidentCorpus.search_distinct over a stand-in index
class _StandInIndex:
    """search_tensor and search_grouped_tensor of FlatIPIndex over the oracle's canonical scores, on CPU tensors"""

    def __init__(self, oracle, x):
        self.oracle, self.x, self.labels_seen = oracle, x, []

    @property
    def ntotal(self):
        return len(self.x)

    def _out(self, D, I, id_map):
        import torch
        if id_map is not None:
            I = np.where(I >= 0, id_map.numpy()[np.clip(I, 0, None)], -1)
        return torch.from_numpy(D), torch.from_numpy(I)

    def search_tensor(self, q, k, id_map=None, stream=None):
        D, I = masked_ref.masked(self.oracle, self.x, q.numpy(), np.ones(len(self.x), np.bool_), None, k)
        return self._out(D, I, id_map)

    def search_grouped_tensor(self, q, k, group_of, id_map=None, return_groups=False, stream=None):
        from haconvdr_amd.index import _as_k
        assert group_of.dtype.is_floating_point is False and tuple(group_of.shape) == (len(self.x),) and not return_groups
        self.labels_seen.append(group_of)
        D, I, _ = grouped_ref.grouped(self.oracle, self.x, q.numpy(), group_of.numpy(), _as_k(k, "stand-in"))
        return self._out(D, I, id_map)

    def remove_ids(self, rows):
        self.x = np.delete(self.x, rows, 0)
        return len(rows)


def _seen_pid(pids_row, topN):
    """output_test_res's de-dup of one query's list: the first hit per passage id"""
    out, seen = [], set()
    for p in pids_row[:topN]:
        if p not in seen:
            seen.add(p)
            out.append(p)
    return out


def test_resident_corpus_search_distinct(oracle):
    import torch
    from haconvdr_amd import synth
    from haconvdr_amd.search import ResidentCorpus
    n, d, nq, k = 300, 32, 4, 60
    x = synth.embeddings(0xB50, n, d)
    q = synth.embeddings(0xB51, nq, d)
    x[100:220] = x[:120] * np.float32(0.5)                                 # a hundred passages have a second, weaker row ...
    x[220:260] = q[0][None, :] * np.linspace(3.0, 2.0, 40, dtype=np.float32)[:, None]     # ... and passage 500 has forty rows that lead query 0's list
    pids = np.arange(n, dtype=np.int64) * 3 + 7                           # row -> external passage id, not dense, not a row number
    pids[100:220] = pids[:120]
    pids[220:260] = 500 * 3 + 7
    rc = ResidentCorpus.__new__(ResidentCorpus)
    rc.index, rc._ids, rc._lookup = _StandInIndex(oracle, x), pids, None
    rc.dev, rc.id_map = torch.device("cpu"), torch.from_numpy(pids)
    n_pids = len(np.unique(pids))
    assert n_pids == 161                                                   # 100 ids on two rows each, one on forty, sixty on one
    # default groups: the rows that carry one passage id.  Full lists of distinct pids, where search + seen_pid falls short
    D, I = rc.search_distinct(q, k)
    assert D.dtype == np.float64 and I.dtype == np.int64 and D.shape == I.shape == (nq, k)
    sD, sI = rc.search(q, k)
    short = [len(_seen_pid(sI[i].tolist(), k)) for i in range(nq)]
    assert short[0] <= k - 39 and all(s < k for s in short)                # what the reference's after-the-cut de-dup leaves
    S = rank_ref.canon_scores(oracle, x, q)
    for i in range(nq):
        assert len(set(I[i].tolist())) == k and (I[i] >= 0).all()
        # the order of a long enough search, de-duplicated: each passage by its best row
        full = rc.search(q[i:i + 1], n)
        want = _seen_pid(full[1][0].tolist(), n)[:k]
        assert I[i].tolist() == want
        best = np.array([S[i, pids == p].max() for p in I[i]], np.float32)
        np.testing.assert_array_equal(D[i].astype(np.float32).view(np.uint32), best.view(np.uint32))
    # the labels handed to the index: dense, one per distinct pid, and cached while the rows stay as they are
    lab = rc.index.labels_seen[-1]
    assert lab.dtype == torch.int64 and int(lab.min()) == 0 and int(lab.max()) == n_pids - 1
    assert all((lab.numpy()[pids == p] == lab.numpy()[pids == p][0]).all() for p in (7, 10, 500 * 3 + 7)) and len(np.unique(lab.numpy())) == n_pids
    rc.search_distinct(q, 5)
    assert rc.index.labels_seen[-1] is lab
    # fewer groups than topN: the tail is padding
    D2, I2 = rc.search_distinct(q, n_pids + 3)
    assert (I2[:, :n_pids] >= 0).all() and (I2[:, n_pids:] == -1).all() and (D2[:, n_pids:] == -float(grouped_ref.FMAX)).all()
    # an explicit group_of over the EXTERNAL ids: pages of five passages
    page_of = np.arange(pids.max() + 1, dtype=np.int64) // 15
    Dp, Ip = rc.search_distinct(q, 20, group_of=page_of)
    for i in range(nq):
        wD, wI, _ = grouped_ref.grouped_from_scores(S[i:i + 1], page_of[pids], 20)
        assert Ip[i].tolist() == pids[wI[0]].tolist() and len(set(page_of[Ip[i]].tolist())) == 20
        np.testing.assert_array_equal(Dp[i].astype(np.float32).view(np.uint32), wD[0].view(np.uint32))
    assert rc.index.labels_seen[-1] is not lab and rc.index.labels_seen[-1].numpy().tolist() == page_of[pids].tolist()
    rc.search_distinct(q, 20, group_of=page_of.astype(np.uint32))          # any integer dtype
    # the three ValueErrors
    for bad in (page_of.astype(np.float32), page_of.reshape(1, -1), page_of[:-1], np.full(len(page_of), -1, np.int64), np.full(len(page_of), 2 ** 32, np.int64)):
        with pytest.raises(ValueError):
            rc.search_distinct(q, 5, group_of=bad)
    # remove(): the default labels are renewed for the rows that are left
    assert rc.remove(np.array([500 * 3 + 7, pids[0]])) == 40 + 2
    assert len(rc._ids) == n - 42 == rc.index.ntotal
    D3, I3 = rc.search_distinct(q, k)
    lab3 = rc.index.labels_seen[-1]
    assert lab3 is not lab and tuple(lab3.shape) == (n - 42,) and int(lab3.max()) == n_pids - 3
    assert not np.isin(I3, [500 * 3 + 7, pids[0]]).any() and all(len(set(I3[i].tolist())) == k for i in range(nq))
    x_left = rc.index.x
    S3 = rank_ref.canon_scores(oracle, x_left, q)
    for i in range(nq):
        wD, wI, _ = grouped_ref.grouped_from_scores(S3[i:i + 1], rc._ids, k)
        assert I3[i].tolist() == rc._ids[wI[0]].tolist()
