"""Hostile QUERIES -- NaN, +-Inf, chains that overflow, magnitudes next to FLT_MAX, subnormals -- through every search route
of FlatIPIndex (the C ABI), in the same batch, tile and chunk as healthy Gaussian neighbours (tests/nonfinite.py; what the
inputs do on the CPU oracle is proved by tests/test_nonfinite_queries.py).  The rest of the suite pins the result contract
for hostile ROWS only; a NaN query is what the encoder hands the index for a sequence with a bad mask or token id.

Every search here
  * compares EVERY query, ids and score words (uint32), with oracle.flat_ip_search -- nothing is skipped or sampled;
  * calls check_status(): a non-finite query is legal input and must not reach a candidate loop's pass bound;
  * asserts the plan it was written for;
  * asserts that the lists of the untouched queries equal those of the same batch with the special queries replaced by
    Gaussian ones: a hostile neighbour costs a healthy query nothing.

What the plan assertions prove was run, per route:
  scan16          scan16_kernel (force_scan16), QT = min(16, nq), one and two query tiles, select_keys_kernel behind it; with
                  n = 70 < k both scan16_kernel and scanq_kernel on lists that end in padding
  scanq           scanq_kernel<NT, W> for every pinnable (NT, W) that fits the LDS at C = 128 (k = 100) and at the single slack
                  slot C = k + 1 = 32 (k = 31), three NQ tiles with a one-query last tile; at nq = 1030 the host's 1024-query
                  chunking (the plan text is the last chunk's: scan16 over 6 queries, which one launch of 1030 would not be)
  seeded          sample_scores_kernel / kth_select_kernel (seed=1) in front of scanq_kernel (d = 768) and scan16_kernel (d = 96)
  prefilter       split_queries_kernel, scanh_kernel<1 | 3>, select_keys_kernel, rescore_kernel, and for the queries that fail
                  the certificate the host cascade or compact_failed / gather / scatter (split_decide) and the exact kernels;
                  fallback= counts the special queries and at most nq // 20 more
  device entries  search_tensor + id_map (keys_to_results_kernel), search_keys_tensor at pos_base = 2^32 - 2 - n with
                  merge_keys_kernel over two shards, search_excluding[_tensor] (filter_keys_kernel)
  by id           score_ids_kernel, count_ahead_kernel / rank_finish_kernel with +Inf, -Inf and NaN reference scores
  multi-device    two shards on one device, remap_positions_kernel + merge_keys_kernel
  encoder         a 2-layer encoder's NaN rows (mask with a hole, id == vocab) straight into search_tensor on one stream

Defects found: none in the kernels.  One statement of the case list was wrong and is corrected in tests/nonfinite.py: the
overflow_order chain does not end NaN.  fmaf does not round its product, so once k = 0 has overflowed the accumulator to +Inf
the finite product of k = d-1 leaves it there; the ordered chain gives +Inf where every other order gives a finite number, -Inf
or NaN, which tells the orders apart just as well.

The cases were also run once against a scan16_kernel changed to admit what fails "s < threshold" instead of what passes
"s >= threshold" (NaN scores enter the candidate lists): every NaN-kind scan16 case fails, and so does every scan16-routed
case of test_fewer_scoring_rows_than_k -- the n = 3001 Inf cases alone do not, the admitted NaN keys sort below the -Inf run
and k = 100 never reaches them, which is why that test exists.

Measured on MI355X: this file's 224 tests run in 13.4 s (the slowest 2.2 s, the first one, which loads the library; every
other under 0.8 s); the whole -m gpu suite with them takes 10 min 06 s for 1035 tests (2 of them skipped for want of a second GPU) on the machine that ran both (9 min 05 s
were quoted for the suite before this file).  No shape here is sized by a workload."""
import functools

import numpy as np
import pytest

from tests import excluding, nonfinite, rank_ref
from tests.test_search_plans_gpu import _index, _search_checked, parse_plan

pytestmark = pytest.mark.gpu

FMAX = np.finfo(np.float32).max
ALL_KINDS = nonfinite.KINDS


# ---------------------------------------------------------------------------------------------------------------------
# the comparison every test goes through (tests/test_nonfinite_queries.py proves that it rejects mutated references)
def assert_same_bits(D, I, oD, oI):
    """(D, I) of a search against the reference's: same shape, same ids, same score WORDS (the reference's scores after the
    "+ 0.0f" of a packed key, rank_ref.canon), no NaN anywhere, and padding exactly where the id is -1."""
    D, oD = np.ascontiguousarray(D, np.float32), np.ascontiguousarray(oD, np.float32)
    I, oI = np.asarray(I, np.int64), np.asarray(oI, np.int64)
    assert D.shape == oD.shape == I.shape == oI.shape, (D.shape, I.shape, oD.shape, oI.shape)
    assert not np.isnan(D).any(), "a NaN score was returned"
    assert np.all(D[I < 0] == -FMAX), "an empty slot does not score -FLT_MAX"
    np.testing.assert_array_equal(I, oI)
    got, want = D.view(np.uint32), np.ascontiguousarray(rank_ref.canon(oD)).view(np.uint32)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%d score words differ, first at %s: got %r, want %r" % (
        len(bad), tuple(bad[0]), D[tuple(bad[0])], oD[tuple(bad[0])])


@functools.lru_cache(maxsize=8)
def _rows(kind, d, n):
    x = nonfinite.rows(kind, d, n, (d * 32768 + n) * 8 + 0x4E46)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=16)
def _case(kind, d, n, nq, extra=()):
    """One case per (kind, d, n, nq), shared by the tests that use it and never written to (add() and search() copy)
    -> (x, q, planted positions, the batch before the planting)."""
    seed = ((d * 32768 + n) * 2048 + nq) * 8 + 0x4E47
    q, pos = nonfinite.queries(kind, d, nq, seed, extra)
    qb = nonfinite.base(d, nq, seed)
    for a in (q, qb):
        a.setflags(write=False)
    return _rows(kind, d, n), q, tuple(pos), qb


def _healthy(nq, pos):
    return np.setdiff1d(np.arange(nq), np.asarray(pos, np.int64))


def _assert_special_lists(kind, D, I, pos):
    if kind in nonfinite.NAN_KINDS:           # every score NaN: nothing but padding
        assert np.all(I[list(pos)] == -1) and np.all(D[list(pos)] == -FMAX)


def _run_exact(idx, kind, x, q, pos, qb, k, oracle):
    """The file's four checks for an exact (split = 0) host search -> (plan fields, D, I)."""
    plan, D, I = _search_checked(idx, x, q, k, oracle)                   # status word, plan text, values
    assert_same_bits(D, I, *oracle.flat_ip_search(x, q, k))              # every query, words
    _assert_special_lists(kind, D, I, pos)
    keep = _healthy(len(q), pos)
    if len(keep):
        plan0, D0, I0 = _search_checked(idx, x, qb, k, oracle)           # the same batch without its special queries
        assert plan0 == plan, (plan0, plan)
        assert_same_bits(D[keep], I[keep], D0[keep], I0[keep])
    return plan, D, I


def _tiles(nq, qt):
    return (nq + qt - 1) // qt


# ---------------------------------------------------------------------------------------------------------------------
# scan16_kernel
@pytest.mark.parametrize("k", [1, 100])
@pytest.mark.parametrize("nq", [1, 16, 17])
@pytest.mark.parametrize("kind", ALL_KINDS)
@pytest.mark.parametrize("d", [768, 96])
def test_scan16(d, nq, k, kind, oracle):
    x, q, pos, qb = _case(kind, d, 3001, nq)
    idx = _index(d, x, force_scan16="1")
    plan, _, _ = _run_exact(idx, kind, x, q, pos, qb, k, oracle)
    assert plan["kernel"] == "scan16" and plan["QT"] == min(16, nq) and plan["T"] == _tiles(nq, 16) and plan["seed"] == 0, plan


@pytest.mark.parametrize("force16", ["1", "0"])
@pytest.mark.parametrize("kind", nonfinite.INF_KINDS + nonfinite.NAN_KINDS)
@pytest.mark.parametrize("d", [768, 96])
def test_fewer_scoring_rows_than_k(d, kind, force16, oracle):
    """n = 70 < k = 100: an Inf query's list is its +Inf rows, its -Inf rows, then padding -- every row that scores at all is
    in it, so a NaN-scored row that was let in has nowhere to hide, whichever end of the order its key sorts to."""
    n, nq, k = 70, 17, 100
    x, q, pos, qb = _case(kind, d, n, nq)
    idx = _index(d, x, force_scan16=force16)
    plan, D, I = _run_exact(idx, kind, x, q, pos, qb, k, oracle)
    assert plan["kernel"] == ("scanq" if force16 == "0" and d % 64 == 0 else "scan16") and plan["seed"] == 0, plan
    if kind in nonfinite.INF_KINDS:
        S = oracle.ip_scores(x, q[list(pos)])
        scoring = (~np.isnan(S)).sum(1)
        assert np.all((scoring > 0) & (scoring < n))
        np.testing.assert_array_equal((I[list(pos)] >= 0).sum(1), scoring)
        assert np.all(D[list(pos), 0] == np.inf) and np.all(D[list(pos), scoring - 1] == -np.inf)


# ---------------------------------------------------------------------------------------------------------------------
# scanq_kernel<NT, W>: k = 100 is C = 128 (NT = 4 no longer fits the LDS), k = 31 the single slack slot C = k + 1 = 32
SCANQ_KINDS = ("nan_one", "inf_one", "overflow_order", "denormal")
SCANQ_FORMS = [(nt, w, k) for k in (100, 31) for nt in ("1", "2", "3", "4") for w in ("4", "8") if not (k == 100 and nt == "4")]


@pytest.mark.parametrize("nt,waves,k", SCANQ_FORMS)
@pytest.mark.parametrize("kind", SCANQ_KINDS)
def test_scanq(nt, waves, k, kind, oracle):
    d, n, nq = 768, 3001, 2 * 32 * int(nt) + 1                           # two NQ tiles and one query
    x, q, pos, qb = _case(kind, d, n, nq)
    idx = _index(d, x, scanq_nt=nt, scanq_waves=waves)
    plan, _, _ = _run_exact(idx, kind, x, q, pos, qb, k, oracle)
    assert plan["kernel"] == "scanq" and plan["NT"] == int(nt) and plan["W"] == int(waves) and plan["seed"] == 0, plan
    assert plan["QT"] == 32 * int(nt) and plan["T"] == 3 and plan["C"] == (128 if k == 100 else k + 1), plan


@pytest.mark.parametrize("kind", ["nan_one", "inf_one"])
def test_scanq_pair_straddles_the_1024_query_chunk(kind, oracle):
    """Special queries at 1023 and 1024: the last of the host's first chunk and the first of its second.  The plan text is the
    last chunk's -- 6 queries, scan16_kernel -- which proves the batch was cut: one launch of 1030 queries is scanq_kernel."""
    d, n, nq, k = 768, 3001, 1030, 100
    x, q, pos, qb = _case(kind, d, n, nq, (1023, 1024))
    assert 1023 in pos and 1024 in pos and 1022 not in pos and 1025 not in pos
    idx = _index(d, x)
    plan, _, _ = _run_exact(idx, kind, x, q, pos, qb, k, oracle)
    assert plan["kernel"] == "scan16" and plan["QT"] == nq - 1024 and plan["T"] == 1, plan


# ---------------------------------------------------------------------------------------------------------------------
# threshold seeding: sample_scores_kernel / kth_select_kernel on scores that are all NaN, +-Inf and NaN, next to FLT_MAX
@pytest.mark.parametrize("kind", ["nan_all", "inf_pair", "near_max"])
@pytest.mark.parametrize("d", [768, 96])
def test_seeded_thresholds(d, kind, oracle):
    n, nq, k = 16449, 20, 10
    x, q, pos, qb = _case(kind, d, n, nq)
    idx = _index(d, x)
    plan, _, _ = _run_exact(idx, kind, x, q, pos, qb, k, oracle)
    assert plan["seed"] == 1 and plan["kernel"] == ("scanq" if d % 64 == 0 else "scan16") and plan["T"] >= 1, plan


# ---------------------------------------------------------------------------------------------------------------------
# the prefilter: a special query cannot be certified (its bound is infinite, or every s~ ties at zero) and must fall back;
# its tile-mates must not
def _fallback(idx):
    plan = idx.last_plan()
    assert plan.startswith("split:"), plan
    nfail, nq = (int(v) for v in plan.split("fallback=")[1].split()[0].split("/"))
    return nfail, nq


@pytest.mark.parametrize("decide", ["host", "device"])
@pytest.mark.parametrize("terms", ["1", "3"])
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_prefilter(terms, decide, kind, oracle):
    d, n, nq, k = 768, 4000, 64, 100                                     # three segments (the adds of _index)
    x, q, pos, qb = _case(kind, d, n, nq)
    idx = _index(d, x, split_terms=terms, split_decide=decide)
    D0, I0 = idx.search(q, k)                                            # split = "0"
    idx.check_status()
    parse_plan(idx.last_plan())                                          # (an exact scan)
    oD, oI = oracle.flat_ip_search(x, q, k)
    assert_same_bits(D0, I0, oD, oI)
    idx.set_option("split", "1")
    D1, I1 = idx.search(q, k)
    idx.check_status()
    nfail, nq_ = _fallback(idx)
    print("prefilter %s terms=%s decide=%s: %s" % (kind, terms, decide, idx.last_plan()))
    assert nq_ == nq and len(pos) <= nfail <= len(pos) + nq // 20, idx.last_plan()
    assert_same_bits(D1, I1, oD, oI)
    assert_same_bits(D1, I1, D0, I0)
    _assert_special_lists(kind, D1, I1, pos)
    Db, Ib = idx.search(qb, k)                                           # the batch without its special queries, same route
    idx.check_status()
    nfail_b, _ = _fallback(idx)
    assert nfail_b <= nq // 20, idx.last_plan()
    keep = _healthy(nq, pos)
    assert_same_bits(D1[keep], I1[keep], Db[keep], Ib[keep])


# ---------------------------------------------------------------------------------------------------------------------
# device entry points
def _cuda(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()                # (a copy: the shared cases are read-only)


def _host(*tensors):
    import torch
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in tensors)


def _assert_exact_plan(idx, nq, d):
    idx.check_status()
    plan = parse_plan(idx.last_plan())
    assert plan["kernel"] == ("scanq" if nq > 16 and d % 64 == 0 else "scan16"), plan
    return plan


@pytest.mark.parametrize("kind", ["nan_one", "inf_one", "near_max"])
@pytest.mark.parametrize("d", [768, 96])
def test_search_tensor_with_id_map(d, kind, oracle):
    from tests.golden import cases
    n, nq, k = 3001, 17, 100
    x, q, pos, qb = _case(kind, d, n, nq)
    ids = cases.search_case_inputs("gauss", 5, n, 1, d=32)[2]
    idx = _index(d, x)
    D, I = _host(*idx.search_tensor(_cuda(q), k, id_map=_cuda(ids)))
    _assert_exact_plan(idx, nq, d)
    oD, oI = oracle.flat_ip_search(x, q, k)
    assert_same_bits(D, I, oD, np.where(oI >= 0, ids[np.clip(oI, 0, None)], -1))
    _assert_special_lists(kind, D, I, pos)
    Db, Ib = _host(*idx.search_tensor(_cuda(qb), k, id_map=_cuda(ids)))
    idx.check_status()
    keep = _healthy(nq, pos)
    assert_same_bits(D[keep], I[keep], Db[keep], Ib[keep])


@pytest.mark.parametrize("kind", ["nan_one", "inf_one", "inf_pair"])
def test_search_keys_at_the_top_of_the_position_range_and_merge(kind, oracle):
    """pos_base = 2^32 - 2 - n: the last row's position is 2^32 - 3 and its key's low word 2.  Two shards, merged: both shards'
    lists are EMPTY (all-zero keys) for the NaN queries, and for inf_pair one shard may hold fewer than k rows that score at all."""
    import torch
    from haconvdr_amd.index import keys_to_results, merge_keys
    d, n, nq, k = 768, 3001, 17, 100
    x, q, pos, qb = _case(kind, d, n, nq)
    base, half = 2 ** 32 - 2 - n, 1501
    h1, h2 = _index(d, x[:half]), _index(d, x[half:])
    qd = _cuda(q)
    k1 = h1.search_keys_tensor(qd, k, pos_base=base)
    k2 = h2.search_keys_tensor(qd, k, pos_base=base + half)
    torch.cuda.synchronize()
    for h in (h1, h2):
        _assert_exact_plan(h, nq, d)
    if kind in nonfinite.NAN_KINDS:
        assert not k1[list(pos)].any().item() and not k2[list(pos)].any().item()
    D, I = _host(*keys_to_results(merge_keys(torch.stack([k1, k2]))))
    oD, oI = oracle.flat_ip_search(x, q, k)
    assert_same_bits(D, np.where(I >= 0, I - base, -1), oD, oI)
    _assert_special_lists(kind, D, I, pos)
    kb = merge_keys(torch.stack([h1.search_keys_tensor(_cuda(qb), k, pos_base=base), h2.search_keys_tensor(_cuda(qb), k, pos_base=base + half)]))
    Db, Ib = _host(*keys_to_results(kb))
    for h in (h1, h2):
        h.check_status()
    keep = _healthy(nq, pos)
    assert_same_bits(D[keep], I[keep], Db[keep], Ib[keep])


@pytest.mark.parametrize("kind", ["inf_one", "nan_one"])
@pytest.mark.parametrize("d", [768, 96])
def test_search_excluding_rows_of_the_inf_tie_run(d, kind, oracle):
    """e = 3 rows per query out of the head of its list: for an inf_one query rows 2, 3 and 4 of the +Inf tie run."""
    n, nq, k, e = 3001, 17, 100, 3
    x, q, pos, qb = _case(kind, d, n, nq)
    _, top = oracle.flat_ip_search(x, q, 8)
    excl = np.ascontiguousarray(top[:, 1:1 + e])                         # (-1 for the NaN queries: padding)
    if kind == "inf_one":
        S = oracle.ip_scores(x, q[list(pos)])
        assert np.all(np.take_along_axis(S, excl[list(pos)], 1) == np.inf)
    want = excluding.filtered_topk(oracle, x, q, k, excl)
    want_b = excluding.filtered_topk(oracle, x, qb, k, excl)
    keep = _healthy(nq, pos)
    idx = _index(d, x)
    for form in ("host", "tensor"):
        if form == "host":
            D, I = idx.search_excluding(q, k, excl)
            Db, Ib = idx.search_excluding(qb, k, excl)
        else:
            D, I = _host(*idx.search_excluding_tensor(_cuda(q), k, _cuda(excl)))
            Db, Ib = _host(*idx.search_excluding_tensor(_cuda(qb), k, _cuda(excl)))
        _assert_exact_plan(idx, nq, d)
        assert_same_bits(D, I, *want)
        assert_same_bits(Db, Ib, *want_b)
        _assert_special_lists(kind, D, I, pos)
        assert_same_bits(D[keep], I[keep], Db[keep], Ib[keep])


# ---------------------------------------------------------------------------------------------------------------------
# by id
@pytest.mark.parametrize("kind", ["inf_one", "inf_pair", "nan_one", "near_max", "denormal"])
@pytest.mark.parametrize("d", [768, 96])
def test_score_ids_and_rank_ids_of_a_search_result(d, kind, oracle):
    n, nq, k = 3001, 17, 100
    x, q, pos, qb = _case(kind, d, n, nq)
    idx = _index(d, x)
    plan, D, I = _run_exact(idx, kind, x, q, pos, qb, k, oracle)
    assert plan["kernel"] == ("scanq" if d % 64 == 0 else "scan16"), plan
    # score_ids(q, I) is D, word for word (-1 scores -FLT_MAX); rank_ids(q, I)[i][j] == j, inside the +-Inf tie runs too
    np.testing.assert_array_equal(idx.score_ids(q, I).view(np.uint32), D.view(np.uint32))
    np.testing.assert_array_equal(idx.rank_ids(q, I), np.where(I >= 0, np.arange(k)[None, :], -1))
    # named rows, the NaN-scored ones among them: NaN stays NaN (the payload is not part of the contract), rank -1
    ids = np.tile(np.arange(130, dtype=np.int64), (nq, 1))
    S = rank_ref.canon_scores(oracle, x, q)
    got = idx.score_ids(q, ids)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(S[:, :130]))
    ok = ~np.isnan(got)
    np.testing.assert_array_equal(got.view(np.uint32)[ok], np.ascontiguousarray(S[:, :130]).view(np.uint32)[ok])
    want = rank_ref.rank_ids_from_scores(S, ids)
    if kind in nonfinite.INF_KINDS or kind in nonfinite.NAN_KINDS:
        assert (want[list(pos)] == -1).any()
    np.testing.assert_array_equal(idx.rank_ids(q, ids), want)
    idx.check_status()


@pytest.mark.parametrize("kind", ["inf_one", "nan_all"])
@pytest.mark.parametrize("d", [768, 96])
def test_count_ahead_with_inf_and_nan_reference_scores(d, kind, oracle):
    n, nq = 3001, 17
    x, q, pos, _ = _case(kind, d, n, nq)
    S = rank_ref.canon_scores(oracle, x, q)
    ref = np.tile(np.array([np.inf, np.inf, np.inf, -np.inf, -np.inf, -np.inf, np.nan, 0.0, np.inf], np.float32), (nq, 1))
    bound = np.tile(np.array([0, 1500, n + 7, 0, 1500, n, 1500, 1500, -1], np.int64), (nq, 1))
    want = rank_ref.count_ahead(S, ref, bound)
    if kind == "inf_one":                                                # the tie runs really are counted into
        assert 0 < want[0, 1] < want[0, 2] < want[0, 4] < want[0, 5] < n and want[0, 0] == 0 and want[0, 6] == -1
    idx = _index(d, x)
    got, = _host(idx.count_ahead_tensor(_cuda(q), _cuda(ref), _cuda(bound)))
    idx.check_status()
    assert idx.last_plan().startswith("count_ahead_kernel<MT=8>"), idx.last_plan()
    np.testing.assert_array_equal(got, want)


# ---------------------------------------------------------------------------------------------------------------------
# two shards in one process
@pytest.mark.parametrize("kind", ["nan_all", "inf_one"])
@pytest.mark.parametrize("d", [768, 96])
def test_two_shards_in_process(d, kind, oracle):
    n, nq, k = 3001, 17, 100
    x, q, pos, qb = _case(kind, d, n, nq)
    idx = _index(d, x, devices=(0, 0))
    plan, _, _ = _run_exact(idx, kind, x, q, pos, qb, k, oracle)         # (the plan text is shard 0's)
    assert plan["kernel"] == ("scanq" if d % 64 == 0 else "scan16") and plan["T"] == (1 if d % 64 == 0 else 2), plan


# ---------------------------------------------------------------------------------------------------------------------
# encoder -> index on one stream: the NaN rows the encoder reports a bad sequence with are queries like any other
def test_encoder_nan_rows_into_search_tensor(oracle):
    import torch
    from haconvdr_amd import synth
    from haconvdr_amd.encoder import ANCEEncoder
    vocab, B, L, k, n = 512, 4, 16, 10, 3001
    enc = ANCEEncoder.from_state_dict(synth.ance_state_dict(0xA11CE, 2, vocab=vocab, max_pos=L + 4))
    tok, lens = synth.token_batch(0x4E51, B, L, min_len=6, vocab=vocab)
    mask = (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)
    ids = tok.astype(np.int64)
    bad_ids, bad_mask = ids.copy(), mask.copy()
    bad_mask[1, 2] = 0                                                   # a hole: not a prefix mask
    bad_ids[3, 3] = vocab                                                # an attended id outside [0, vocab)
    x = nonfinite.rows("nan_all", 768, n, 0x4E52)
    idx = _index(768, x)
    E = enc(_cuda(bad_ids), _cuda(bad_mask))
    D, I = idx.search_tensor(E, k)                                       # same stream, no host round trip in between
    H = enc(_cuda(ids), _cuda(mask))                                     # the healthy batch: the same four sequences, repaired
    Dh, Ih = idx.search_tensor(H, k)
    E, D, I, H, Dh, Ih = _host(E, D, I, H, Dh, Ih)
    plan = _assert_exact_plan(idx, B, 768)
    assert plan["kernel"] == "scan16" and plan["QT"] == B, plan
    assert np.isnan(E[[1, 3]]).all() and np.isfinite(E[[0, 2]]).all() and np.isfinite(H).all()
    assert np.all(I[[1, 3]] == -1) and np.all(D[[1, 3]] == -FMAX)
    assert_same_bits(D, I, *oracle.flat_ip_search(x, E, k))
    assert_same_bits(Dh, Ih, *oracle.flat_ip_search(x, H, k))
    # a flagged sequence is a NaN row "for THAT sequence only": its batch-mates' embeddings are the healthy batch's, word for
    # word, and so are their lists
    np.testing.assert_array_equal(E[[0, 2]].view(np.uint32), H[[0, 2]].view(np.uint32))
    assert_same_bits(D[[0, 2]], I[[0, 2]], Dh[[0, 2]], Ih[[0, 2]])
