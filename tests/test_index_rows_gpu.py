"""Rows by id: hac_index_reconstruct* (faiss reconstruct / reconstruct_n / reconstruct_batch / search_and_reconstruct) and
hac_index_score_ids* (exact scores of named rows), through FlatIPIndex and ResidentCorpus, i.e. the C ABI.

Every assertion is bitwise.  Rows are copies: they are compared as uint32 words, and a tenth of each round-trip corpus is
raw random bit patterns (NaNs with payloads, Infs, denormals) plus one row of -0.0.  Scores are the oracle's fmaf chain
(oracle.ip_scores) followed by the "+ 0.0f" of make_key: compared as uint32 words too, except where a NaN score is the
point (the NaN's payload is the hardware's: there the NaN mask and every other word are compared).

Indexes are built like _index() of tests/test_search_plans_gpu.py: three adds cut off the 64-row grid, so the rows of one
add straddle segments and the last group is partial."""
import numpy as np
import pytest

from haconvdr_amd import synth
from tests.test_search_plans_gpu import _cuts, _index

pytestmark = pytest.mark.gpu

FMAX = np.finfo(np.float32).max
ONES = np.uint32(0xFFFFFFFF)
HAC_ERR_INVALID, HAC_ERR_UNSUPPORTED = 1, 4


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bits(got, want, msg=""):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=msg)


def hostile_corpus(seed, n, d):
    """Unit-ish rows, every tenth row (3, 13, ...) raw random words (row 3 starts with +-Inf, a signalling and a quiet NaN
    with payloads, the smallest and the largest denormal, -0.0, FLT_MAX), row 7 all -0.0."""
    x = synth.embeddings(seed, n, d)
    rows = np.arange(3, n, 10)
    x.view(np.uint32)[rows] = synth.uniform_u32(seed + 1, len(rows) * d).reshape(len(rows), d)
    if n > 7:
        x[7] = -0.0
    w = x.view(np.uint32)
    # (random words hold NaNs and denormals now and then, an Inf practically never: the special values are planted)
    w[3, :8] = [0x7F800000, 0xFF800000, 0x7FA00001, 0xFFC12345, 0x00000001, 0x807FFFFF, 0x80000000, 0x7F7FFFFF]
    if n >= 100:
        assert np.isnan(x).any() and np.isinf(x).any() and ((w & 0x7F800000) == 0).any() and (w[7] == 0x80000000).all()
    return x


def canon(scores):
    """make_key's "+ 0.0f": -0.0 -> +0.0, everything else unchanged."""
    return (np.asarray(scores, np.float32) + np.float32(0.0)).astype(np.float32)


def tensor_rows(idx, ids=None, **kw):
    import torch
    t = None if ids is None else torch.from_numpy(np.ascontiguousarray(ids, np.int64)).cuda()
    out = idx.reconstruct_tensor(t, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def tensor_scores(idx, q, ids):
    import torch
    out = idx.score_ids_tensor(torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda(),
                               torch.from_numpy(np.ascontiguousarray(ids, np.int64)).cuda())
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# 1. round trip
@pytest.mark.parametrize("d", [32, 96, 768, 1024])
def test_rows_come_back_bit_for_bit(d):
    n = 1000
    x = hostile_corpus(0x20D + d, n, d)
    idx = _index(d, x)
    c1, c2 = _cuts(n)
    assert_bits(idx.reconstruct_n(), x, "whole index")
    assert_bits(tensor_rows(idx), x, "whole index, tensor form")
    for i0, m in ((0, 1), (63, 2), (c1 - 1, 3), (n - 1, 1), (n, 0), (1, 130), (64, 64), (c2 - 70, 141)):
        got = idx.reconstruct_n(i0, m)
        assert got.shape == (m, d) and got.dtype == np.float32
        assert_bits(got, x[i0:i0 + m], f"range ({i0}, {m})")
        assert_bits(tensor_rows(idx, i0=i0, n=m), x[i0:i0 + m], f"range ({i0}, {m}), tensor form")
    perm = np.argsort(synth.uniform_u32(5 + d, n), kind="stable").astype(np.int64)
    assert sorted(perm.tolist()) == list(range(n))
    assert_bits(idx.reconstruct_batch(perm), x[perm], "permutation")
    assert_bits(tensor_rows(idx, perm), x[perm], "permutation, tensor form")
    rep = np.array([5, 5, n - 1, 5, 0, n - 1, 63, 64, 64], np.int64)
    assert_bits(idx.reconstruct_batch(rep), x[rep], "repeated ids")
    pad = np.array([-1, 3, -1, n - 1, 7, -1], np.int64)
    for got in (idx.reconstruct_batch(pad), tensor_rows(idx, pad)):
        w = bits(got)
        assert (w[pad < 0] == ONES).all()
        np.testing.assert_array_equal(w[pad >= 0], bits(x[pad[pad >= 0]]))
    boundary = (c1 + 63) // 64 * 64                      # first row of the second segment
    for i in (0, n - 1, boundary, boundary - 1, c1):
        got = idx.reconstruct(i)
        assert got.shape == (d,)
        assert_bits(got, x[i], f"reconstruct({i})")
    assert_bits(idx.reconstruct(np.int64(7)), x[7])
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 2. errors
def test_ids_and_ranges_outside_the_index():
    import torch
    from haconvdr_amd._lib import HacError
    from haconvdr_amd.index import FlatIPIndex
    d, n = 96, 300
    x = synth.embeddings(0xE44, n, d)
    q = synth.embeddings(0xE45, 2, d)
    idx = _index(d, x)
    for i0, m in ((n - 1, 2), (n + 1, 0), (0, n + 1), (-1, 1), (0, -1), (-5, 0)):
        with pytest.raises(HacError) as e:
            idx.reconstruct_n(i0, m)
        assert e.value.code == HAC_ERR_INVALID, (i0, m, str(e.value))
    for bad in (n, -2, n + 12345, -2 ** 40):
        ids = np.array([1, 2, bad, 3, n + 7], np.int64)
        for call in (lambda: idx.reconstruct_batch(ids), lambda: idx.score_ids(q, np.stack([ids, ids])),
                     lambda: idx.reconstruct(bad)):
            with pytest.raises(HacError) as e:
                call()
            assert e.value.code == HAC_ERR_INVALID and str(bad) in str(e.value), (bad, str(e.value))
        with pytest.raises(HacError) as e:
            idx.reconstruct_batch(ids)
        assert "position 2" in str(e.value), str(e.value)
        # the device entry points cannot look: all-ones rows / -FLT_MAX, no error, a clean status word
        w = bits(tensor_rows(idx, ids))
        assert (w[[2, 4]] == ONES).all()
        np.testing.assert_array_equal(w[[0, 1, 3]], bits(x[[1, 2, 3]]))
        D = tensor_scores(idx, q, np.stack([ids, ids]))
        assert (D[:, [2, 4]] == -FMAX).all() and (D[:, [0, 1, 3]] != -FMAX).all()
        idx.check_status()
    for call in (lambda: idx.reconstruct_tensor(i0=n - 1, n=2), lambda: idx.reconstruct_tensor(i0=-1, n=1)):
        with pytest.raises(HacError) as e:                # a RANGE outside the index is an error on every entry point
            call()
        assert e.value.code == HAC_ERR_INVALID
    # shape and dtype mistakes on CUDA tensors: ValueError, before the library is called
    qt, it = torch.from_numpy(q).cuda(), torch.zeros((2, 3), dtype=torch.int64, device="cuda")
    for call in (lambda: idx.reconstruct_tensor(it), lambda: idx.reconstruct_tensor(it[0].int()),
                 lambda: idx.score_ids_tensor(qt, it[0]), lambda: idx.score_ids_tensor(qt[:1], it),
                 lambda: idx.score_ids_tensor(qt[:, :64], it), lambda: idx.score_ids_tensor(qt, it.float()),
                 lambda: idx.search_and_reconstruct_tensor(qt, 0), lambda: idx.reconstruct_n(0.5),
                 lambda: idx.reconstruct_batch([[1]]), lambda: idx.score_ids(q, [1, 2])):
        with pytest.raises(ValueError):
            call()
    # nothing to do is not an error
    assert idx.reconstruct_batch(np.zeros(0, np.int64)).shape == (0, d)
    assert idx.score_ids(q, np.zeros((2, 0), np.int64)).shape == (2, 0)
    assert idx.score_ids(q[:0], np.zeros((0, 4), np.int64)).shape == (0, 4)
    assert tensor_scores(idx, q, np.zeros((2, 0), np.int64)).shape == (2, 0)
    empty = FlatIPIndex(d)
    got = empty.reconstruct_n(0, 0)
    assert got.shape == (0, d) and got.dtype == np.float32
    assert empty.reconstruct_n().shape == (0, d)
    assert (bits(empty.reconstruct_batch(np.array([-1], np.int64))) == ONES).all()
    assert (bits(tensor_rows(empty, np.array([0, -1, 5], np.int64))) == ONES).all()
    with pytest.raises(HacError):
        empty.reconstruct(0)


# ---------------------------------------------------------------------------------------------------------------------
# 3. reset
def test_rows_of_the_old_content_are_unreachable_after_reset():
    from haconvdr_amd._lib import HacError
    d = 96
    x = hostile_corpus(0x4E5, 1000, d)
    y = hostile_corpus(0x4E6, 300, d)
    idx = _index(d, x)
    assert_bits(idx.reconstruct_n(), x)
    idx.reset()
    assert idx.reconstruct_n().shape == (0, d)
    idx.add(y[:130])
    idx.add(y[130:])
    assert_bits(idx.reconstruct_n(), y)
    assert_bits(idx.reconstruct_batch(np.arange(299, -1, -1)), y[::-1])
    for call in (lambda: idx.reconstruct(300), lambda: idx.reconstruct_n(299, 2), lambda: idx.reconstruct_batch([999])):
        with pytest.raises(HacError) as e:
            call()
        assert e.value.code == HAC_ERR_INVALID
    w = bits(tensor_rows(idx, np.array([299, 300, 999], np.int64)))
    np.testing.assert_array_equal(w[0], bits(y[299]))
    assert (w[1:] == ONES).all()
    q = synth.embeddings(0x4E7, 1, d)
    assert tensor_scores(idx, q, np.array([[300, 299]], np.int64))[0, 0] == -FMAX


# ---------------------------------------------------------------------------------------------------------------------
# 4. every storage state: tiles only, row-major copy current, copy stale after an add, copy dropped
def test_same_bits_from_the_tiles_and_from_the_row_major_copy(oracle):
    d, n, nq, k = 768, 5000, 32, 10
    x = synth.embeddings(0x570, n + 700, d)
    q = synth.embeddings(0x571, nq, d)
    idx = _index(d, x[:n], split="1", rescore_rows="1", fp16_image="eager")
    perm = np.argsort(synth.uniform_u32(0x572, n + 700), kind="stable").astype(np.int64)
    cand = (synth.uniform_u32(0x573, nq * 300) % np.uint32(n)).astype(np.int64).reshape(nq, 300)
    want_scores = canon(np.take_along_axis(oracle.ip_scores(x, q), cand, 1))

    def read_everything(rows, state):
        p = perm[perm < rows]
        assert_bits(idx.reconstruct_n(), x[:rows], state)
        assert_bits(tensor_rows(idx), x[:rows], state)
        assert_bits(idx.reconstruct_batch(p), x[p], state)
        assert_bits(tensor_rows(idx, p), x[p], state)
        assert_bits(idx.score_ids(q, cand), want_scores, state)
        assert_bits(tensor_scores(idx, q, cand), want_scores, state)

    read_everything(n, "before any search: tiles")
    for _ in range(2):
        D, I = idx.search(q, k)
    plan = idx.last_plan()
    assert plan.startswith("split:") and "rescore=rows" in plan, plan
    read_everything(n, "row-major copy current")
    idx.add(x[n:])                                        # the tail group of the last segment and a new segment: the copy is stale there
    read_everything(n + 700, "after an add: copy stale where the add landed")
    idx.search(q, k)
    assert "rescore=rows" in idx.last_plan(), idx.last_plan()
    read_everything(n + 700, "copy current again")
    idx.set_option("rescore_rows", "0")
    read_everything(n + 700, "switched off, copy not yet freed")
    idx.search(q, k)
    assert "rescore=tiles" in idx.last_plan(), idx.last_plan()
    read_everything(n + 700, "copy freed: tiles")
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 5. scores vs the oracle
@pytest.mark.parametrize("d, nq, m", [(32, 1, 1), (96, 5, 7), (768, 5, 256), (768, 3, 257), (768, 300, 1000)])
def test_scores_by_id_are_the_oracles_chain(d, nq, m, oracle):
    n = 1000
    x = synth.embeddings(0x5C0 + d, n, d)
    x[11] = 0.0
    x[11, ::2] = -0.0                                    # a zero row: chain ends in +-0.0, returned as +0.0
    q = synth.embeddings(0x5C1 + m, nq, d)
    ids = (synth.uniform_u32(0x5C2 + nq, nq * m) % np.uint32(n)).astype(np.int64).reshape(nq, m)
    if m >= 7:
        ids[:, 2] = ids[:, 5] = 11                       # duplicates in every list, and the zero row
        ids[0, :] = ids[0, 0]
    S = oracle.ip_scores(x, q)
    want = canon(np.take_along_axis(S, ids, 1))
    idx = _index(d, x)
    assert_bits(idx.score_ids(q, ids), want)
    assert_bits(tensor_scores(idx, q, ids), want)
    # padding slots and ids past the end on the tensor form: -FLT_MAX there, the oracle everywhere else
    for bad in (-1, n):
        ids_t, want_t = ids.copy(), want.copy()
        ids_t[:, m // 2] = bad
        want_t[:, m // 2] = -FMAX
        assert_bits(tensor_scores(idx, q, ids_t), want_t)
    if m >= 3:
        ids_t, want_t = ids.copy(), want.copy()
        ids_t[:, 0], ids_t[:, m - 1] = -1, n
        want_t[:, 0] = want_t[:, m - 1] = -FMAX
        assert_bits(tensor_scores(idx, q, ids_t), want_t)
        ids_h = ids_t.copy()
        ids_h[:, m - 1] = ids[:, m - 1]                  # the host form takes -1 ...
        want_h = want_t.copy()
        want_h[:, m - 1] = want[:, m - 1]
        assert_bits(idx.score_ids(q, ids_h), want_h)
    idx.check_status()


def test_a_nan_row_scores_nan_in_exactly_the_slots_that_name_it(oracle):
    d, n, nq, m = 96, 1000, 4, 50
    x = synth.embeddings(0xA7A, n, d)
    x[500, 17] = np.nan
    q = synth.embeddings(0xA7B, nq, d)
    ids = (synth.uniform_u32(0xA7C, nq * m) % np.uint32(n)).astype(np.int64).reshape(nq, m)
    ids[ids == 500] = 499
    ids[0, 3] = ids[2, 0] = ids[2, 49] = 500
    want = canon(np.take_along_axis(oracle.ip_scores(x, q), ids, 1))
    idx = _index(d, x)
    for got in (idx.score_ids(q, ids), tensor_scores(idx, q, ids)):
        np.testing.assert_array_equal(np.isnan(got), ids == 500)
        np.testing.assert_array_equal(bits(got)[ids != 500], bits(want)[ids != 500])


# ---------------------------------------------------------------------------------------------------------------------
# 6. scores reproduce search
@pytest.mark.parametrize("d", [96, 768])
def test_scores_of_a_search_result_are_its_distances_exact_route(d):
    n, nq, k = 3000, 20, 10
    x = synth.embeddings(0x6E0 + d, n, d)
    q = synth.embeddings(0x6E1 + d, nq, d)
    idx = _index(d, x, split="0")
    D, I = idx.search(q, k)
    assert not idx.last_plan().startswith("split:"), idx.last_plan()
    assert_bits(idx.score_ids(q, I), D)
    assert_bits(tensor_scores(idx, q, I), D)


def test_scores_of_a_search_result_are_its_distances_prefilter_route():
    d, n, nq, k = 768, 20000, 64, 100
    x = synth.embeddings(0x6F0, n, d)
    q = synth.embeddings(0x6F1, nq, d)
    idx = _index(d, x, split="1")
    D, I = idx.search(q, k)
    assert idx.last_plan().startswith("split:"), idx.last_plan()
    assert (I >= 0).all()
    assert_bits(idx.score_ids(q, I), D)
    assert_bits(tensor_scores(idx, q, I), D)


def test_scores_of_a_short_corpus_pad_like_search():
    d, n, nq, k = 96, 7, 3, 10
    x = synth.embeddings(0x6F8, n, d)
    q = synth.embeddings(0x6F9, nq, d)
    idx = _index(d, x)
    D, I = idx.search(q, k)
    assert (I[:, n:] == -1).all() and (D[:, n:] == -FMAX).all() and (I[:, :n] >= 0).all()
    assert_bits(idx.score_ids(q, I), D)
    assert_bits(tensor_scores(idx, q, I), D)


# ---------------------------------------------------------------------------------------------------------------------
# 7. search_and_reconstruct
@pytest.mark.parametrize("n, k", [(2000, 10), (7, 10)])
def test_search_and_reconstruct_returns_the_rows_of_its_ids(n, k):
    import torch
    d, nq = 96, 6
    x = hostile_corpus(0x7A0 + n, n, d) if n > 100 else synth.embeddings(0x7A0 + n, n, d)
    x[~(np.abs(x) < 1e3)] = 1.0                           # (finite scores: no NaN, Inf or huge word; denormals and -0.0 stay)
    q = synth.embeddings(0x7A1, nq, d)
    idx = _index(d, x)
    D0, I0 = idx.search(q, k)
    D, I, R = idx.search_and_reconstruct(q, k)
    Dt, It, Rt = idx.search_and_reconstruct_tensor(torch.from_numpy(q).cuda(), k)
    torch.cuda.synchronize()
    for d_, i_, r_ in ((D, I, R), (Dt.cpu().numpy(), It.cpu().numpy(), Rt.cpu().numpy())):
        assert_bits(d_, D0)
        np.testing.assert_array_equal(i_, I0)
        assert r_.shape == (nq, k, d) and r_.dtype == np.float32
        w = bits(r_)
        np.testing.assert_array_equal(w[i_ >= 0], bits(x[i_[i_ >= 0]]))
        assert (w[i_ < 0] == ONES).all()
    assert (I0 < 0).any() == (n < k)
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 8. several devices in one process
@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)])
def test_multi_device_index_reads_rows_by_the_global_numbering(devices, oracle):
    import torch
    from haconvdr_amd._lib import HacError
    d, n, nq, m = 96, 1000, 5, 40
    x = hostile_corpus(0x8D0, n, d)
    q = synth.embeddings(0x8D1, nq, d)
    ids = (synth.uniform_u32(0x8D2, nq * m) % np.uint32(n)).astype(np.int64).reshape(nq, m)
    ids[:, 7] = -1
    perm = np.argsort(synth.uniform_u32(0x8D3, n), kind="stable").astype(np.int64)
    one, many = _index(d, x), _index(d, x, devices=devices)
    assert many.ntotal == n
    assert_bits(many.reconstruct_n(), x)
    assert_bits(many.reconstruct_n(), one.reconstruct_n())
    for i0, cnt in ((0, 1), (331, 5), (n - 3, 3), (n, 0)):
        assert_bits(many.reconstruct_n(i0, cnt), x[i0:i0 + cnt])
    assert_bits(many.reconstruct_batch(perm), one.reconstruct_batch(perm))
    assert_bits(many.reconstruct_batch(perm), x[perm])
    pad = np.array([-1, 999, -1, 0], np.int64)
    assert_bits(many.reconstruct_batch(pad), one.reconstruct_batch(pad))
    got, ref = many.score_ids(q, ids), one.score_ids(q, ids)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    np.testing.assert_array_equal(bits(got)[~np.isnan(ref)], bits(ref)[~np.isnan(ref)])
    assert (got[:, 7] == -FMAX).all()
    xf = np.where(np.isfinite(x), x, np.float32(0.5)).astype(np.float32)     # a finite corpus: every word compared
    one.reset(), many.reset()
    for ix in (one, many):
        ix.add(xf[:333])
        ix.add(xf[333:])
    want = canon(np.take_along_axis(oracle.ip_scores(xf, q), np.clip(ids, 0, None), 1))
    want[ids < 0] = -FMAX
    assert_bits(many.score_ids(q, ids), want)
    assert_bits(one.score_ids(q, ids), want)
    with pytest.raises(HacError) as e:
        many.reconstruct_batch([n])
    assert e.value.code == HAC_ERR_INVALID
    qt, it = torch.from_numpy(q).cuda(), torch.from_numpy(ids).cuda()
    for call in (lambda: many.reconstruct_tensor(it[0]), lambda: many.reconstruct_tensor(i0=0, n=4),
                 lambda: many.score_ids_tensor(qt, it)):
        with pytest.raises(HacError) as e:
            call()
        assert e.value.code == HAC_ERR_UNSUPPORTED, str(e.value)


# ---------------------------------------------------------------------------------------------------------------------
# 9. capture (recipe and precautions of test_device_search_is_graph_capturable_on_the_prefilter_path)
def test_device_forms_are_graph_capturable(oracle):
    """The *_device entry points enqueue and return: no synchronize, no read-back, no allocation -- checked the hard way, by
    capturing reconstruct_tensor + score_ids_tensor into one HIP graph and replaying it with the ids and the queries
    overwritten in place between the replays."""
    import torch
    d, n, nq, m = 768, 3000, 8, 33
    x = synth.embeddings(0x9C0, n, d)
    idx = _index(d, x)
    qs = [synth.embeddings(0x9C1 + r, nq, d) for r in range(2)]
    idss = [(synth.uniform_u32(0x9C4 + r, nq * m) % np.uint32(n + 2)).astype(np.int64).reshape(nq, m) - 1 for r in range(2)]
    for i in idss:
        i[0, 0], i[1, 1] = -1, n                         # a padding slot and an id past the end in every replay
    qt, it = torch.from_numpy(qs[0]).cuda(), torch.from_numpy(idss[0]).cuda()
    side = torch.cuda.Stream()
    eager, replayed = [], []
    with torch.cuda.stream(side):
        for r in range(2):                               # warm-up at the captured shape: the segment table goes up here
            qt.copy_(torch.from_numpy(qs[r]))
            it.copy_(torch.from_numpy(idss[r]))
            R0, D0 = idx.reconstruct_tensor(it.view(-1)), idx.score_ids_tensor(qt, it)
            side.synchronize()
            eager.append((R0.cpu().numpy(), D0.cpu().numpy()))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            R1, D1 = idx.reconstruct_tensor(it.view(-1)), idx.score_ids_tensor(qt, it)
        for r in range(2):
            qt.copy_(torch.from_numpy(qs[r]))
            it.copy_(torch.from_numpy(idss[r]))
            R1.zero_()
            D1.zero_()
            g.replay()
            side.synchronize()
            replayed.append((R1.cpu().numpy(), D1.cpu().numpy()))
    torch.cuda.synchronize()
    S = [oracle.ip_scores(x, q) for q in qs]
    for r in range(2):
        ids = idss[r]
        ok = (ids >= 0) & (ids < n)
        assert_bits(replayed[r][0], eager[r][0], f"replay {r}: rows")
        assert_bits(replayed[r][1], eager[r][1], f"replay {r}: scores")
        w = bits(replayed[r][0]).reshape(nq, m, d)
        np.testing.assert_array_equal(w[ok], bits(x[ids[ok]]))
        assert (w[~ok] == ONES).all()
        want = canon(np.take_along_axis(S[r], np.clip(ids, 0, n - 1), 1))
        want[~ok] = -FMAX
        assert_bits(replayed[r][1], want, f"replay {r}: scores vs the oracle")
    assert not np.array_equal(replayed[0][1], replayed[1][1])
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 10. ResidentCorpus: rows and scores by external passage id
def test_resident_corpus_scores_and_reconstructs_by_passage_id(tmp_path, oracle):
    from haconvdr_amd.passages import write_embedding_block
    from haconvdr_amd.search import ResidentCorpus
    d, n0, n1, nq = 768, 150, 101, 4
    x = synth.embeddings(0xB10, n0 + n1, d)
    ext = (np.argsort(synth.uniform_u32(0xB11, n0 + n1), kind="stable").astype(np.int64) * 7 + 1000)     # non-contiguous, unsorted
    write_embedding_block(str(tmp_path), 0, x[:n0], ext[:n0])
    write_embedding_block(str(tmp_path), 1, x[n0:], ext[n0:])
    rc = ResidentCorpus(str(tmp_path), 2)
    assert rc.ntotal == n0 + n1
    absent = np.array([0, 1001, 999, 10 ** 12, -5], np.int64)                  # 1001 = 1000 + 1: between two ids that exist
    assert not np.isin(absent, ext).any()
    np.testing.assert_array_equal(rc.rows_of(ext), np.arange(n0 + n1))
    np.testing.assert_array_equal(rc.rows_of(absent), -1)
    np.testing.assert_array_equal(rc.rows_of(ext[[5, 200, 5]].reshape(1, 3)), [[5, 200, 5]])
    q = synth.embeddings(0xB12, nq, d)
    rows = (synth.uniform_u32(0xB13, nq * 20) % np.uint32(n0 + n1)).astype(np.int64).reshape(nq, 20)
    pids = ext[rows]
    pids[:, 4] = absent[:nq]
    S = rc.score(q, pids)
    assert S.dtype == np.float64 and S.shape == (nq, 20)
    want = canon(np.take_along_axis(oracle.ip_scores(x, q), rows, 1)).astype(np.float64)
    want[:, 4] = -float(FMAX)
    np.testing.assert_array_equal(S, want)
    # ... which is what search() reports for the same pairs
    Ds, Is = rc.search(q, 10)
    np.testing.assert_array_equal(rc.score(q, Is), Ds)
    R = rc.reconstruct(np.concatenate([ext[::-1], absent]))
    np.testing.assert_array_equal(bits(R[:n0 + n1]), bits(x[::-1]))
    assert (bits(R[n0 + n1:]) == ONES).all()
    with pytest.raises(ValueError):
        rc.rows_of(np.array([1.5]))
    with pytest.raises(ValueError):
        rc.score(q, pids[0])


# ---------------------------------------------------------------------------------------------------------------------
# 11. the host forms across their staging chunks.  The sizes follow from the host code: rows are staged stage_rows() =
# 64 MiB / 4d (down to a multiple of 64) at a time; a pair matrix goes MC = 2^20 columns and QC = 64 MiB // (MC *
# bytes per pair + 4d) queries at a time.  One device, and two shards on one device (the positions scatter of
# reconstruct_batch, the write-back that leaves the other shard's slots alone).
STAGE_BYTES, PAIR_MC = 64 << 20, 1 << 20
_CHUNKED = {}


def stage_chunk_corpus():
    """d = 1024 (the widest row: the fewest rows per chunk), one full staging chunk + one group + one row"""
    if "rows" not in _CHUNKED:
        d = 1024
        chunk = STAGE_BYTES // (4 * d) // 64 * 64
        assert chunk == 16384
        _CHUNKED["rows"] = hostile_corpus(0xC40, chunk + 65, d)
    return _CHUNKED["rows"]


def pair_chunk_corpus():
    """(x [130, 32] finite with rows 5 and 120 identical -- on different shards of a two-shard index --, 6 queries)"""
    if "pairs" not in _CHUNKED:
        d, n = 32, 130
        x = synth.embeddings(0xC50, n, d)
        x[120] = x[5]
        _CHUNKED["pairs"] = (x, synth.embeddings(0xC51, 6, d))
    return _CHUNKED["pairs"]


def pair_chunk_ids(seed, nq, n):
    """int64 [nq, 2^20 + 1] over [-1, n)"""
    m = PAIR_MC + 1
    return (synth.uniform_u32(seed, nq * m) % np.uint32(n + 1)).astype(np.int64).reshape(nq, m) - 1


@pytest.mark.parametrize("devices", [(0,), (0, 0)])
def test_rows_across_a_staging_chunk(devices):
    x = stage_chunk_corpus()
    n, d = x.shape
    idx = _index(d, x, devices=devices)
    assert_bits(idx.reconstruct_n(), x, "whole index: two chunks")
    assert_bits(idx.reconstruct_n(16383, 3), x[16383:16386], "a range across the chunk edge")
    perm = np.argsort(synth.uniform_u32(0xC41, n), kind="stable").astype(np.int64)
    assert sorted(perm.tolist()) == list(range(n))
    pad = np.array([0, 64, 16383, 16384, n - 1])
    perm[pad] = -1
    w = bits(idx.reconstruct_batch(perm))
    assert (w[pad] == ONES).all()
    keep = perm >= 0
    np.testing.assert_array_equal(w[keep], bits(x[perm[keep]]))
    idx.check_status()


@pytest.mark.parametrize("devices", [(0,), (0, 0)])
def test_scores_across_both_chunk_loops(devices, oracle):
    x, q = pair_chunk_corpus()
    n, d = x.shape
    nq = len(q)
    assert STAGE_BYTES // (PAIR_MC * 12 + 4 * d) == 5 and nq == 6       # query chunks 5 + 1, column chunks 2^20 + 1
    ids = pair_chunk_ids(0xC52, nq, n)
    assert ids.min() == -1 and ids.max() == n - 1 and (ids[:, -1] >= 0).any()
    table = canon(oracle.ip_scores(x, q))
    want = np.take_along_axis(table, np.clip(ids, 0, None), 1)
    want[ids < 0] = -FMAX
    idx = _index(d, x, devices=devices)
    assert_bits(idx.score_ids(q, ids), want)
    idx.check_status()
