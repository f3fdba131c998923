"""Range search: hac_index_range_search* (the range_* kernels of csrc/range.inc) through FlatIPIndex and ResidentCorpus, i.e.
the C ABI.

Every assertion is equality of lims, of the bits of D and of I with tests/range_ref.py, the definition of include/haconvdr.h
restated over the CPU oracle's canonical scores.  Indexes are built like _index() of tests/test_search_plans_gpu.py: three
adds cut off the 64-row grid, so the last group is partial and its tail rows must never be returned.  Every case checks the
host form and the tensor form and leaves the status word clean."""
import ctypes
import re

import numpy as np
import pytest

from haconvdr_amd import synth
from tests import range_ref, rank_ref
from tests.golden import cases
from tests.test_index_rank_gpu import hostile_queries
from tests.test_index_rows_gpu import hostile_corpus
from tests.test_search_plans_gpu import _adversarial, _index

pytestmark = pytest.mark.gpu

HAC_ERR_INVALID, HAC_ERR_UNSUPPORTED = 1, 4
INF = np.float32(np.inf)
_PLAN = re.compile(r"^range_emit_kernel grid=\((?P<P>\d+),(?P<T>\d+)\) QT=(?P<QT>\d+) cap=(?P<cap>\d+) sort_lds=(?P<sort_lds>\d+) "
                   r"merge_passes=(?P<merge_passes>\d+) lds=(?P<lds>\d+)$")


def parse_plan(text):
    m = _PLAN.match(text)
    assert m, "not the plan of a range search: %r" % text
    return {k: int(v) for k, v in m.groupdict().items()}


def _cuda(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def tensor_form(idx, q, radius, cap, id_map=None):
    """(lims, D [cap], I [cap]) of range_search_tensor as ndarrays"""
    import torch
    lims, D, I = idx.range_search_tensor(_cuda(q, np.float32), _cuda(radius, np.float32), cap, id_map=id_map)
    torch.cuda.synchronize()
    return lims.cpu().numpy(), D.cpu().numpy(), I.cpu().numpy()


def both_forms(idx, q, radius, want, extra_cap=0):
    """host form and tensor form (at cap = the total + extra_cap) against the reference; the status word stays clean"""
    radius = np.array(np.broadcast_to(np.asarray(radius, np.float32), (len(q),)))
    got = idx.range_search(q, radius)
    assert got[0].dtype == np.int64 and got[1].dtype == np.float32 and got[2].dtype == np.int64
    range_ref.assert_same(got, want, "host form")
    np.testing.assert_array_equal(idx.range_count(q, radius), np.diff(want[0]), err_msg="range_count")
    total = int(want[0][-1])
    lims, D, I = tensor_form(idx, q, radius, total + extra_cap)
    range_ref.assert_same((lims, D[:total], I[:total]), want, "tensor form")
    idx.check_status()


def raw_host(idx, q, radius, cap, D=None, I=None):
    """hac_index_range_search as it stands: the caller's cap and the caller's D / I (None: null) -> (status, lims)"""
    from haconvdr_amd import _lib
    from haconvdr_amd.index import _f32p, _i64p
    q, radius = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(radius, np.float32)
    lims = np.full(len(q) + 1, -7, np.int64)
    null_f, null_i = ctypes.POINTER(ctypes.c_float)(), ctypes.POINTER(ctypes.c_int64)()
    rc = _lib.lib().hac_index_range_search(idx._h, _f32p(q), len(q), _f32p(radius), cap, _i64p(lims), null_f if D is None else _f32p(D),
                                           null_i if I is None else _i64p(I))
    return rc, lims


def raw_device(idx, q, radius, cap, lims, D, I, id_map=None):
    """hac_index_range_search_device on the current stream over the caller's tensors (None: null) -> status"""
    from haconvdr_amd import _lib
    from haconvdr_amd.index import _devp, _stream_ptr
    return _lib.lib().hac_index_range_search_device(idx._h, _devp(q), q.shape[0], _devp(radius), cap, _devp(lims), _devp(D), _devp(I), _devp(id_map),
                                                    _stream_ptr(None))


# ---------------------------------------------------------------------------------------------------------------------
# 1. hostile rows, radii mixed inside one call
_HOSTILE = {}


def _hostile_case(d, oracle):
    """(x, q of 33 queries, their canonical scores): computed once per d, shared by the query counts"""
    if d not in _HOSTILE:
        x = hostile_corpus(0x6A9 + d, 1000, d)
        q = hostile_queries(0x6AA + d, 33, d)
        _HOSTILE[d] = (x, q, rank_ref.canon_scores(oracle, x, q))
    return _HOSTILE[d]


def _score_at(S_row, pos):
    """the score at descending position pos among the row's non-NaN scores"""
    s = S_row[~np.isnan(S_row)]
    return np.sort(s)[::-1][pos]


def _mixed_radii(S):
    """-Inf, +Inf, NaN, 0.0, -0.0 and the score of the row at a chosen position, in turn"""
    r = np.zeros(len(S), np.float32)
    for i in range(len(S)):
        r[i] = (-INF, INF, np.float32(np.nan), np.float32(0.0), np.float32(-0.0), _score_at(S[i], 37 + 11 * i))[i % 6]
    return r


@pytest.mark.parametrize("nq", [1, 16, 17, 33])
@pytest.mark.parametrize("d", [32, 96, 768, 1024])
def test_hostile_rows_mixed_radii(d, nq, oracle):
    x, q33, S33 = _hostile_case(d, oracle)
    q, S = q33[:nq], S33[:nq]                        # nq = 1: the all-zero query on its own, radius -Inf
    radius = _mixed_radii(S)
    want = range_ref.range_from_scores(S, radius)
    lens = np.diff(want[0])
    full = (~np.isnan(S) & ~np.isneginf(S)).sum(1)
    assert lens[0] == full[0] > 0 and np.isnan(S).any()
    if nq >= 16:
        assert lens[1] == 0 and lens[2] == 0 and lens[6] == full[6] and 0 < lens[5] < full[5]
    for i in range(nq):                              # NaN-scored rows are in no list
        assert not np.isnan(S[i][want[2][want[0][i]:want[0][i + 1]]]).any()
    idx = _index(d, x)
    both_forms(idx, q, radius, want)
    plan = parse_plan(idx.last_plan())
    assert plan["T"] == (nq + 15) // 16 and plan["QT"] == min(nq, 16) and plan["cap"] == want[0][-1], plan


# ---------------------------------------------------------------------------------------------------------------------
# 2. strictness on ties
def test_ties_are_excluded_and_row_ordered(oracle):
    """16 distinct grid-valued rows, each repeated ~62 times and interleaved; integer queries: every score is exact and every
    score value is shared by dozens of rows.  A radius equal to such a value returns none of its rows, and every tie above
    it comes out in row order."""
    d, n, nq = 96, 1000, 6
    base = ((synth.uniform_u32(0x6C0, 16 * d) % np.uint32(17)).astype(np.float32).reshape(16, d) - 8.0) / 8.0
    x = base[np.arange(n) % 16]
    q = (synth.uniform_u32(0x6C1, nq * d) % np.uint32(9)).astype(np.float32).reshape(nq, d) - 4.0
    q[0] = 0.0
    S = rank_ref.canon_scores(oracle, x, q)
    assert all(len(np.unique(S[i])) <= 16 for i in range(nq))
    idx = _index(d, x)
    for pos in (100, 500):
        radius = np.array([_score_at(S[i], pos) for i in range(nq)], np.float32)
        radius[0] = 0.0 if pos == 100 else -0.0     # the zero query: every score is +0.0
        want = range_ref.range_from_scores(S, radius)
        lens = np.diff(want[0])
        assert lens[0] == 0
        for i in range(1, nq):
            shared = (S[i] == radius[i]).sum()
            seg = want[2][want[0][i]:want[0][i + 1]]
            assert shared >= 40 and lens[i] <= pos and lens[i] + shared > pos and not (S[i][seg] == radius[i]).any()
            same = np.diff(S[i][seg]) == 0           # inside a tie the rows ascend
            assert same.any() and (np.diff(seg)[same] > 0).all()
        both_forms(idx, q, radius, want)
    want = range_ref.range_from_scores(S[:1], np.float32(-1e-30))
    np.testing.assert_array_equal(want[2], np.arange(n))
    both_forms(idx, q[:1], np.float32(-1e-30), want)


# ---------------------------------------------------------------------------------------------------------------------
# 3. segments at the edges of the LDS sort, and beyond it (the only place segments leave LDS)
def test_segment_lengths_around_the_lds_sort(oracle):
    d, nq = 32, 3
    idx0 = _index(d, np.zeros((3, d), np.float32))
    idx0.range_count(np.zeros((1, d), np.float32), 0.0)
    N = parse_plan(idx0.last_plan())["sort_lds"]
    assert N >= 64 and N & (N - 1) == 0
    n = 3 * N + 70
    x, q = _adversarial(d, n, nq, 0x6D0)             # scores strictly increase with the row: no ties
    S = rank_ref.canon_scores(oracle, x, q)
    idx = _index(d, x)
    for cs, extra in (((0, N, 3 * N + 5), 0), ((1, N + 1, 2 * N), 0), ((N - 1, 2 * N + 1, N), 0), ((3 * N + 5, 1, 2 * N + 1), 9 * N)):
        radius = np.array([S[i, n - 1 - c] for i, c in enumerate(cs)], np.float32)     # the row at descending position c
        want = range_ref.range_from_scores(S, radius)
        np.testing.assert_array_equal(np.diff(want[0]), cs)
        for i, c in enumerate(cs):
            np.testing.assert_array_equal(want[2][want[0][i]:want[0][i + 1]], n - 1 - np.arange(c))
        both_forms(idx, q, radius, want, extra_cap=extra)      # (a larger cap: more merge passes than the segments need)
        plan = parse_plan(idx.last_plan())
        blocks = -(-plan["cap"] // N)
        assert plan["merge_passes"] == (blocks - 1).bit_length() >= 2, plan


# ---------------------------------------------------------------------------------------------------------------------
# 4. capacity: all or nothing
def test_capacity_is_all_or_nothing(oracle):
    import torch
    d, nq = 96, 17
    x, q33, S33 = _hostile_case(d, oracle)
    q, S = q33[:nq], S33[:nq]
    radius = np.array([_score_at(S[i], 20 + 13 * i) for i in range(nq)], np.float32)
    want = range_ref.range_from_scores(S, radius)
    total = int(want[0][-1])
    assert total > 500
    idx = _index(d, x)
    SENT_D, SENT_I = np.float32(-123.5), np.int64(-99)
    qd, rd = _cuda(q, np.float32), _cuda(radius, np.float32)
    for cap in (total, total - 1, 1):
        fits = cap >= total
        D, I = np.full(total + 8, SENT_D, np.float32), np.full(total + 8, SENT_I, np.int64)
        rc, lims = raw_host(idx, q, radius, cap, D, I)
        assert rc == 0
        np.testing.assert_array_equal(lims, want[0], err_msg="lims is exact whatever cap is")
        if fits:
            range_ref.assert_same((lims, D[:total], I[:total]), want, "host form, cap = total")
            assert (D[total:] == SENT_D).all() and (I[total:] == SENT_I).all()
        else:
            assert (D == SENT_D).all() and (I == SENT_I).all(), "an overflowing host call leaves D and I untouched"
        # the tensor form over views of larger buffers: nothing behind cap (fits: behind the total) is written
        Dt = torch.full((total + 8,), float(SENT_D), dtype=torch.float32, device="cuda")
        It = torch.full((total + 8,), int(SENT_I), dtype=torch.int64, device="cuda")
        lt = torch.full((nq + 1,), -7, dtype=torch.int64, device="cuda")
        assert raw_device(idx, qd, rd, cap, lt, Dt[:cap], It[:cap]) == 0
        torch.cuda.synchronize()
        np.testing.assert_array_equal(lt.cpu().numpy(), want[0])
        Dn, In = Dt.cpu().numpy(), It.cpu().numpy()
        behind = total if fits else cap
        assert (Dn[behind:] == SENT_D).all() and (In[behind:] == SENT_I).all()
        if fits:
            range_ref.assert_same((lims, Dn[:total], In[:total]), want, "tensor form, cap = total")
    # the pure count: cap = 0 with null D / I
    rc, lims = raw_host(idx, q, radius, 0)
    assert rc == 0
    np.testing.assert_array_equal(lims, want[0])
    np.testing.assert_array_equal(idx.range_count(q, radius), np.diff(want[0]))
    lt = torch.full((nq + 1,), -7, dtype=torch.int64, device="cuda")
    assert raw_device(idx, qd, rd, 0, lt, None, None) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(lt.cpu().numpy(), want[0])
    idx.check_status()


def test_range_search_answers_when_its_first_guess_overflows(oracle):
    d, n, nq = 32, 9000, 3
    x = synth.embeddings(0x6E0, n, d)
    q = synth.embeddings(0x6E1, nq, d)
    want = range_ref.range_search(oracle, x, q, -INF)
    idx = _index(d, x)
    assert want[0][-1] == nq * n > idx.RANGE_FIRST_CAP * nq
    range_ref.assert_same(idx.range_search(q, -np.inf), want, "second call")
    assert parse_plan(idx.last_plan())["cap"] == nq * n
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 5. agreement with search, count_ahead and rank_ids
def _agreement(idx, x, q, oracle, route):
    """route(k): how the plan of search(q, k) must begin"""
    import torch
    nq = len(q)
    S = rank_ref.canon_scores(oracle, x, q)
    radius = np.array([_score_at(S[i], 149) for i in range(nq)], np.float32)      # each query's 150th score
    want = range_ref.range_from_scores(S, radius)
    np.testing.assert_array_equal(np.diff(want[0]), 149)
    both_forms(idx, q, radius, want)
    assert idx.last_plan().startswith("range_emit_kernel")
    lims, D, I = idx.range_search(q, radius)
    for k in (1, 100, 2048):
        sD, sI = idx.search(q, k)
        assert idx.last_plan().startswith(route(k)), (k, idx.last_plan())
        for i in range(nq):
            keep = sD[i] > radius[i]
            take = min(k, 149)
            assert keep.sum() == take
            np.testing.assert_array_equal(sI[i][keep], I[lims[i]:lims[i] + take])
            np.testing.assert_array_equal(range_ref.bits(sD[i][keep]), range_ref.bits(D[lims[i]:lims[i] + take]))
    counts = idx.count_ahead_tensor(_cuda(q, np.float32), _cuda(radius[:, None], np.float32), _cuda(np.zeros((nq, 1)), np.int64))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(counts.cpu().numpy()[:, 0], np.diff(lims))
    np.testing.assert_array_equal(idx.rank_ids(q, I.reshape(nq, 149)), np.tile(np.arange(149), (nq, 1)))
    idx.check_status()


def test_agrees_with_search_count_ahead_and_rank_ids(oracle):
    x, q, _ = cases.search_case_inputs("gauss", 0x6F0, 3001, 20, d=96)
    _agreement(_index(96, x), x, q, oracle, lambda k: "scan")


def test_agrees_with_the_prefilter_route(oracle):
    x = synth.embeddings(0x6F1, 3000)
    q = synth.embeddings(0x6F2, 96)
    _agreement(_index(768, x, split="1"), x, q, oracle, lambda k: "split:" if k <= 100 else "scan")      # (k = 2048 is beyond the prefilter)


# ---------------------------------------------------------------------------------------------------------------------
# 6. lifetime
def test_reset_smaller_add_later_add_and_empty_index(oracle):
    d = 96
    x, q33, _ = _hostile_case(d, oracle)
    q = q33[:5]
    idx = _index(d, x)
    both_forms(idx, q, -INF, range_ref.range_search(oracle, x, q, -INF))
    idx.reset()                                       # empty: all-zero lims
    empty = (np.zeros(6, np.int64), np.zeros(0, np.float32), np.zeros(0, np.int64))
    both_forms(idx, q, -INF, empty)
    idx.add(x[:130])                                  # stale rows 130.. of the old segments are never returned
    both_forms(idx, q, -INF, range_ref.range_search(oracle, x[:130], q, -INF))
    idx.add(x[500:777])                               # rows added after a range search are found
    y = np.concatenate([x[:130], x[500:777]])
    S = rank_ref.canon_scores(oracle, y, q)
    radius = np.array([_score_at(S[i], 60) for i in range(5)], np.float32)
    want = range_ref.range_from_scores(S, radius)
    assert (want[2] >= 130).any()
    both_forms(idx, q, radius, want)


# ---------------------------------------------------------------------------------------------------------------------
# 7. several devices in one process: the host form
@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)])
def test_multi_device_host_form(devices, oracle):
    from haconvdr_amd._lib import HacError
    d = 96
    x, q33, S33 = _hostile_case(d, oracle)
    q, S = q33[:17], S33[:17]
    idx = _index(d, x, devices=devices)
    for radius in (_mixed_radii(S), np.array([_score_at(S[i], 300 + i) for i in range(17)], np.float32)):
        want = range_ref.range_from_scores(S, radius)
        range_ref.assert_same(idx.range_search(q, radius), want, "hostile rows")
        np.testing.assert_array_equal(idx.range_count(q, radius), np.diff(want[0]))
    # the tie corpus: a tie spans the shards, the rows still ascend inside it
    n = 1000
    base = ((synth.uniform_u32(0x6C0, 16 * d) % np.uint32(17)).astype(np.float32).reshape(16, d) - 8.0) / 8.0
    xt = base[np.arange(n) % 16]
    qt = (synth.uniform_u32(0x6C1, 6 * d) % np.uint32(9)).astype(np.float32).reshape(6, d) - 4.0
    St = rank_ref.canon_scores(oracle, xt, qt)
    radius = np.array([_score_at(St[i], 500) for i in range(6)], np.float32)
    tie = _index(d, xt, devices=devices)
    range_ref.assert_same(tie.range_search(qt, radius), range_ref.range_from_scores(St, radius), "tie corpus")
    rc, lims = raw_host(tie, qt, radius, 5, np.zeros(5, np.float32), np.zeros(5, np.int64))       # overflow: lims still exact
    assert rc == 0
    np.testing.assert_array_equal(lims, range_ref.range_from_scores(St, radius)[0])
    with pytest.raises(HacError) as e:
        idx.range_search_tensor(_cuda(q, np.float32), _cuda(np.zeros(17), np.float32), 10)
    assert e.value.code == HAC_ERR_UNSUPPORTED
    idx.check_status()
    tie.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 8. id_map, ResidentCorpus
def test_id_map_in_the_tensor_form(oracle):
    d = 96
    x, q33, S33 = _hostile_case(d, oracle)
    q, S = q33[:7], S33[:7]
    radius = np.array([_score_at(S[i], 50 + i) for i in range(7)], np.float32)
    want = range_ref.range_from_scores(S, radius)
    ext = np.argsort(synth.uniform_u32(0x710, len(x)), kind="stable").astype(np.int64) * 5 + 10 ** 10
    total = int(want[0][-1])
    lims, D, I = tensor_form(_index(d, x), q, radius, total + 3, id_map=_cuda(ext, np.int64))
    range_ref.assert_same((lims, D[:total], I[:total]), (want[0], want[1], ext[want[2]]), "id_map")


def test_resident_corpus_range_search_and_ahead_of(tmp_path, oracle):
    from haconvdr_amd.passages import write_embedding_block
    from haconvdr_amd.search import ResidentCorpus
    d, n0, n1, nq = 768, 150, 101, 4
    x = synth.embeddings(0x720, n0 + n1, d)
    ext = (np.argsort(synth.uniform_u32(0x721, n0 + n1), kind="stable").astype(np.int64) * 7 + 1000)
    write_embedding_block(str(tmp_path), 0, x[:n0], ext[:n0])
    write_embedding_block(str(tmp_path), 1, x[n0:], ext[n0:])
    rc = ResidentCorpus(str(tmp_path), 2)
    q = synth.embeddings(0x722, nq, d)
    S = rank_ref.canon_scores(oracle, x, q)
    radius = np.array([_score_at(S[i], 30 + i) for i in range(nq)], np.float32)
    want = range_ref.range_from_scores(S, radius)
    lims, D, I = rc.range_search(q, radius)
    np.testing.assert_array_equal(lims, want[0])
    np.testing.assert_array_equal(I, ext[want[2]])
    np.testing.assert_array_equal(D, want[1].astype(np.float64))
    full = oracle.flat_ip_search(x, q, n0 + n1)[1]
    gold = ext[np.array([full[0, 0], full[1, 12], full[2, 250], 0])]
    gold[3] = 1001                                       # between two ids that exist: in no block
    lims, D, I = rc.ahead_of(q, gold)
    np.testing.assert_array_equal(np.diff(lims), [0, 12, 250, 0])
    np.testing.assert_array_equal(I[lims[1]:lims[2]], ext[full[1, :12]])
    np.testing.assert_array_equal(I[lims[2]:lims[3]], ext[full[2, :250]])


# ---------------------------------------------------------------------------------------------------------------------
# 9. capture
def test_range_search_tensor_captured_and_replayed(oracle):
    import torch
    d, nq = 96, 17
    x, q33, S33 = _hostile_case(d, oracle)
    fit_q, fit_S = q33[:nq], S33[:nq]
    over_q, over_S = q33[33 - nq:], S33[33 - nq:]
    fit_r = np.array([_score_at(fit_S[i], 40 + i) for i in range(nq)], np.float32)
    over_r = np.array([_score_at(over_S[i], 200 + i) for i in range(nq)], np.float32)
    fit_want, over_want = range_ref.range_from_scores(fit_S, fit_r), range_ref.range_from_scores(over_S, over_r)
    cap = 1500
    assert fit_want[0][-1] <= cap < over_want[0][-1]
    idx = _index(d, x)
    q, r = _cuda(fit_q, np.float32), _cuda(fit_r, np.float32)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()                            # a single stream: no parallel branches in the graph
    got = []
    with torch.cuda.stream(side):
        idx.range_search_tensor(q, r, cap)                # the largest shape once: workspaces and the segment table exist
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            lims, D, I = idx.range_search_tensor(q, r, cap)
        for qn, rn in ((over_q, over_r), (fit_q, fit_r), (over_q, over_r), (fit_q, fit_r)):
            q.copy_(torch.from_numpy(qn))
            r.copy_(torch.from_numpy(rn))
            lims.fill_(-7)
            g.replay()
            side.synchronize()
            got.append((lims.cpu().numpy(), D.cpu().numpy(), I.cpu().numpy()))
    torch.cuda.synchronize()
    for (l, D, I), want in zip(got, (over_want, fit_want, over_want, fit_want)):
        total = int(want[0][-1])
        np.testing.assert_array_equal(l, want[0])
        if total <= cap:
            range_ref.assert_same((l, D[:total], I[:total]), want, "replayed")
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 10. determinism
def test_identical_calls_return_identical_bytes(oracle):
    d, nq = 96, 33
    x, q33, S33 = _hostile_case(d, oracle)
    want = range_ref.range_from_scores(S33, -INF)
    idx = _index(d, x)
    total = int(want[0][-1])
    first = None
    for _ in range(5):
        host = idx.range_search(q33, -np.inf)
        dev = tensor_form(idx, q33, np.full(nq, -INF), total)
        blob = b"".join(a.tobytes() for a in host + dev)
        first = first or blob
        assert blob == first
    range_ref.assert_same(host, want, "host form")
    range_ref.assert_same(dev, want, "tensor form")


# ---------------------------------------------------------------------------------------------------------------------
# 11. refused arguments
def test_refused_arguments_leave_the_handle_usable(oracle):
    import torch
    from haconvdr_amd._lib import HacError
    d = 96
    x, q33, S33 = _hostile_case(d, oracle)
    q, S = q33[:3], S33[:3]
    radius = np.zeros(3, np.float32)
    idx = _index(d, x)
    D, I = np.zeros(8, np.float32), np.zeros(8, np.int64)
    assert raw_host(idx, q, radius, -1, D, I)[0] == HAC_ERR_INVALID
    assert raw_host(idx, q, radius, 8, None, I)[0] == HAC_ERR_INVALID
    assert raw_host(idx, q, radius, 8, D, None)[0] == HAC_ERR_INVALID
    qd, rd = _cuda(q, np.float32), _cuda(radius, np.float32)
    lt, Dt, It = torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(8, device="cuda"), torch.zeros(8, dtype=torch.int64, device="cuda")
    assert raw_device(idx, qd, rd, -1, lt, Dt, It) == HAC_ERR_INVALID
    assert raw_device(idx, qd, rd, 8, lt, None, It) == HAC_ERR_INVALID
    assert raw_device(idx, qd, rd, 8, None, Dt, It) == HAC_ERR_INVALID
    unaligned = _cuda(np.zeros(3 * d + 1), np.float32)[1:].view(3, d)            # 4 bytes off a 16-byte boundary
    assert unaligned.data_ptr() % 16 == 4
    assert raw_device(idx, unaligned, rd, 8, lt, Dt, It) == HAC_ERR_INVALID
    for bad in (np.zeros(2, np.float32), np.zeros((3, 1), np.float32)):
        with pytest.raises(ValueError):
            idx.range_search(q, bad)
        with pytest.raises(ValueError):
            idx.range_search_tensor(qd, _cuda(bad, np.float32), 8)
    for bad_cap in (-1, 8.0):
        with pytest.raises(ValueError):
            idx.range_search_tensor(qd, rd, bad_cap)
    with pytest.raises(ValueError):
        idx.range_search_tensor(qd, torch.zeros(3), 8)                           # a CPU radius
    # nq == 0: lims[0] = 0 and nothing else
    rc, lims = raw_host(idx, np.zeros((0, d), np.float32), np.zeros(0, np.float32), 0)
    assert rc == 0 and lims.tolist() == [0]
    lims0, D0, I0 = idx.range_search(np.zeros((0, d), np.float32), 0.0)
    assert lims0.tolist() == [0] and len(D0) == 0 and len(I0) == 0
    both_forms(idx, q, radius, range_ref.range_from_scores(S, radius))          # the handle still answers
    with pytest.raises(HacError):
        from haconvdr_amd import _lib
        _lib.check(raw_host(idx, q, radius, -1, D, I)[0])
