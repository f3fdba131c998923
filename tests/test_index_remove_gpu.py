"""remove_ids: hac_index_remove_ids (compact_rows_kernel of csrc/remove.inc and its driver) through FlatIPIndex and
ResidentCorpus, i.e. the C ABI.

After a removal the index must be indistinguishable from one built by adding the surviving rows: every check compares ntotal,
the bits of reconstruct_n(), D (bits) and I of a search, rank_ids of that I and a range search with tests/remove_ref.py
(np.delete) plus the CPU oracle over the surviving rows."""
import functools

import numpy as np
import pytest

from haconvdr_amd import synth
from tests import range_ref, remove_ref
from tests.test_index_rows_gpu import assert_bits, hostile_corpus
from tests.test_search_plans_gpu import _index

pytestmark = pytest.mark.gpu

HAC_ERR_INVALID = 1
NQ, K = 8, 10


@functools.lru_cache(maxsize=None)
def _data(d, n=400):
    """(rows, queries) per dimension: made once, never written to"""
    x, q = synth.embeddings(0x4E0 + d, n, d), synth.embeddings(0x4E1 + d, NQ, d)
    x.setflags(write=False)
    q.setflags(write=False)
    return x, q


def _fresh(d, *adds):
    from haconvdr_amd.index import FlatIPIndex
    idx = FlatIPIndex(d)
    idx.set_option("split", "0")
    for a in adds:
        idx.add(a)
    return idx


def check_all(idx, xs, q, oracle, what=""):
    """the index against one that holds exactly the rows xs"""
    assert idx.ntotal == len(xs), what
    got = idx.reconstruct_n()
    assert got.shape == xs.shape, what
    assert_bits(got, xs, what + ": reconstruct_n")
    D, I = idx.search(q, K)
    oD, oI = oracle.flat_ip_search(xs, q, K)
    np.testing.assert_array_equal(I, oI, err_msg=what + ": I")
    assert_bits(D, oD, what + ": D")
    np.testing.assert_array_equal(idx.rank_ids(q, I), np.tile(np.arange(K), (len(q), 1)), err_msg=what + ": rank_ids")
    radius = oD[:, K // 2].copy()
    range_ref.assert_same(idx.range_search(q, radius), range_ref.range_search(oracle, xs, q, radius), what + ": range_search")
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 1. one segment of 200 rows
ONE_SEGMENT = {
    "first": [0],
    "last": [199],
    "one-group": list(range(64, 128)),
    "every-other": list(range(0, 200, 2)),
    "duplicates-and-padding": [17, -1, 130, 17, 63, -1, 64, 130],
    "nothing": [],
    "only-padding": [-1, -1, -1],
}


@pytest.mark.parametrize("case", list(ONE_SEGMENT))
@pytest.mark.parametrize("d", [64, 96])
def test_one_segment(d, case, oracle):
    x, q = _data(d)
    x = x[:200]
    ids = np.array(ONE_SEGMENT[case], np.int64)
    idx = _fresh(d, x)
    n = idx.remove_ids(ids)
    assert n == len(remove_ref.removed_rows(ids)) == 200 - len(remove_ref.removed(x, ids))
    check_all(idx, remove_ref.removed(x, ids), q, oracle, case)


@pytest.mark.parametrize("d", [64, 96])
def test_three_removals_on_one_index_and_a_mask(d, oracle):
    x, q = _data(d)
    xs = x[:200]
    idx = _fresh(d, xs)
    for step, ids in enumerate(([199, 0], list(range(60, 70)) + [-1], [5, 5, 100])):
        assert idx.remove_ids(ids) == len(remove_ref.removed_rows(ids))
        xs = remove_ref.removed(xs, ids)
        check_all(idx, xs, q, oracle, f"removal {step}")
    mask = np.zeros(len(xs), bool)
    mask[[1, 64, len(xs) - 1]] = True
    assert idx.remove_ids(mask) == 3
    check_all(idx, xs[~mask], q, oracle, "mask")


@pytest.mark.parametrize("d", [64, 96])
def test_everything_then_add_again(d, oracle):
    x, q = _data(d)
    idx = _fresh(d, x[:200])
    assert idx.remove_ids(np.arange(200)) == 200
    assert idx.ntotal == 0 and idx.reconstruct_n().shape == (0, d)
    D, I = idx.search(q, K)
    assert (I == -1).all()
    idx.add(x[200:330])
    check_all(idx, x[200:330], q, oracle, "added again")


def test_a_call_that_names_no_row_leaves_the_segment_table_alone():
    """Seen through a capture: a call that finds the segment table changed is refused while its stream is being captured into
    a HIP graph (include/haconvdr.h), so a read-back captured right after remove_ids of nothing shows the table was left alone."""
    import torch
    d = 64
    x, _ = _data(d)
    idx = _fresh(d, x[:200])
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        idx.reconstruct_tensor(i0=0, n=200)                # the table goes up
        side.synchronize()
        assert idx.remove_ids(np.zeros(0, np.int64)) == 0 and idx.remove_ids([-1, -1]) == 0
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            out = idx.reconstruct_tensor(i0=0, n=200)
        out.zero_()
        g.replay()
        side.synchronize()
    torch.cuda.synchronize()
    assert_bits(out.cpu().numpy(), x[:200], "replayed read-back")


# ---------------------------------------------------------------------------------------------------------------------
# 2. segment edges: adds of 64, 100 and 92 rows are segments of 64, 128 and 64 rows (the third add fills the second first)
SEGMENT_EDGES = {
    "partial-last": list(range(10, 20)) + list(range(70, 110)) + list(range(200, 220)),      # 256 - 70 = 186 rows
    "multiple-of-64": list(range(10, 20)) + list(range(70, 104)) + list(range(200, 220)),    # 256 - 64 = 192 rows: two full segments
}


@pytest.mark.parametrize("case", list(SEGMENT_EDGES))
@pytest.mark.parametrize("d", [64, 96])
def test_segment_edges_then_add(d, case, oracle):
    x, q = _data(d)
    idx = _fresh(d, x[:64], x[64:164], x[164:256])
    ids = np.array(SEGMENT_EDGES[case], np.int64)
    assert idx.remove_ids(ids) == len(ids)
    xs = remove_ref.removed(x[:256], ids)
    assert len(xs) == (186 if case == "partial-last" else 192)
    check_all(idx, xs, q, oracle, case)
    idx.add(x[256:326])                                   # continues in the partial last segment / opens a new one
    xs = np.concatenate([xs, x[256:326]])
    check_all(idx, xs, q, oracle, case + ", then an add")
    assert idx.remove_ids([len(xs) - 1, 0]) == 2          # and the index that results is an ordinary one
    check_all(idx, xs[1:-1], q, oracle, case + ", then an add and a removal")


# ---------------------------------------------------------------------------------------------------------------------
# 3. the border between two staging chunks
def test_staging_chunk_border():
    d = 64
    stage_rows = (64 << 20) // (4 * d) // 64 * 64         # include/haconvdr.h: ~64 MiB of rows per chunk, whole groups
    n = stage_rows + 197
    x = np.arange(n * d, dtype=np.uint32).view(np.float32).reshape(n, d)     # every word its own: a misplaced piece shows
    idx = _fresh(d, x)
    ids = [0, stage_rows - 1, stage_rows + 1]
    assert idx.remove_ids(ids) == 3
    assert idx.ntotal == n - 3
    assert_bits(idx.reconstruct_n(), remove_ref.removed(x, ids), "two chunks")


# ---------------------------------------------------------------------------------------------------------------------
# 4. bits only move
@pytest.mark.parametrize("d", [64, 96])
def test_hostile_bits_survive_the_move(d):
    x = hostile_corpus(0x4F0 + d, 300, d)
    idx = _index(d, x)                                    # three segments, cuts off the 64-row grid
    ids = [0, 2, 6, 64, 65, 101, 250]                     # rows 3 (Inf, NaN payloads, denormals) and 7 (-0.0) move, as do 13, 23, ...
    assert idx.remove_ids(ids) == len(ids)
    assert_bits(idx.reconstruct_n(), remove_ref.removed(x, ids), "hostile rows")
    assert_bits(idx.reconstruct_batch([0, 1, 2, 3]), x[[1, 3, 4, 5]], "by id")


# ---------------------------------------------------------------------------------------------------------------------
# 5. the fp16 image and the row-major copy are current again when the call returns
def test_images_are_rebuilt(oracle):
    d, n, nq = 768, 3000, 96
    x, q = synth.embeddings(0x4F8, n, d), synth.embeddings(0x4F9, nq, d)
    idx = _index(d, x, split="1", fp16_image="eager", rescore_rows="1")
    idx.search(q, K)
    plan = idx.last_plan()
    assert plan.startswith("split:") and "rescore=rows" in plan, plan
    ids = np.concatenate([[5, 1000, 1001, 2999], np.arange(1500, 3000, 7), np.arange(2100, 2200)])
    assert idx.remove_ids(ids) == len(remove_ref.removed_rows(ids))
    xs = remove_ref.removed(x, ids)
    D, I = idx.search(q, K)
    plan = idx.last_plan()
    assert plan.startswith("split:") and "rescore=rows" in plan, plan
    idx.check_status()
    oD, oI = oracle.flat_ip_search(xs, q, K)
    np.testing.assert_array_equal(I, oI)
    assert_bits(D, oD, "prefilter route")
    assert_bits(idx.reconstruct_batch(I[:, 0]), xs[I[:, 0]], "rows out of the row-major copy")
    idx.set_option("split", "0")
    D0, I0 = idx.search(q, K)
    assert not idx.last_plan().startswith("split:")
    np.testing.assert_array_equal(I0, I)
    assert_bits(D0, D, "exact route")
    assert idx.ntotal == len(xs)


# ---------------------------------------------------------------------------------------------------------------------
# 6. without the oracle: hiding rows per query and removing them give the same lists
@pytest.mark.parametrize("d", [64, 96])
def test_agrees_with_search_excluding(d):
    x, q = _data(d)
    idx = _index(d, x)
    _, top = idx.search(q, 2)
    R = np.unique(np.concatenate([top.reshape(-1), [0, 399, 128]]))           # every query loses its two best rows
    eD, eI = idx.search_excluding(q, K, np.tile(R, (NQ, 1)))
    assert idx.remove_ids(R) == len(R)
    D, I = idx.search(q, K)
    np.testing.assert_array_equal(I, remove_ref.renumber(eI, R))
    assert_bits(D, eD, "D")
    idx.check_status()


# ---------------------------------------------------------------------------------------------------------------------
# 7. several devices
@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)])
@pytest.mark.parametrize("d", [64, 96])
def test_several_devices(d, devices, oracle):
    from haconvdr_amd.index import FlatIPIndex
    x, q = _data(d)
    S = len(devices)
    idx = FlatIPIndex(d, devices=devices)
    idx.set_option("split", "0")
    idx.add(x[:150])
    idx.add(x[150:153])                                   # S = 2: rows 150, 151 | 152; S = 3: one row each
    ids = np.array([3, 60, 80, 120, 149, 152, 80, -1], np.int64)             # every shard's first span, and all of the last shard's second
    per = 150 // S
    assert {min(int(i) // per, S - 1) for i in ids if 0 <= i < 150} == set(range(S))
    assert idx.remove_ids(ids) == 6
    xs = remove_ref.removed(x[:153], ids)
    check_all(idx, xs, q, oracle, "removed")
    np.testing.assert_array_equal(idx.reconstruct_batch([len(xs) - 1, 0, 77]).view(np.uint32), xs[[len(xs) - 1, 0, 77]].view(np.uint32))
    idx.add(x[153:223])
    xs = np.concatenate([xs, x[153:223]])
    check_all(idx, xs, q, oracle, "removed, then an add")
    assert idx.remove_ids(np.arange(100, 160)) == 60
    check_all(idx, remove_ref.removed(xs, np.arange(100, 160)), q, oracle, "and a second removal")


# ---------------------------------------------------------------------------------------------------------------------
# 8. a bad id is refused on the host and changes nothing
@pytest.mark.parametrize("bad", [200, -2])
def test_an_id_outside_is_refused_and_nothing_changes(bad):
    from haconvdr_amd._lib import HacError
    d = 64
    x, _ = _data(d)
    idx = _fresh(d, x[:200])
    with pytest.raises(HacError) as e:
        idx.remove_ids([3, bad, 5])
    assert e.value.code == HAC_ERR_INVALID and str(bad) in str(e.value) and "position 1" in str(e.value), str(e.value)
    assert idx.ntotal == 200
    assert_bits(idx.reconstruct_n(), x[:200], "untouched")


# ---------------------------------------------------------------------------------------------------------------------
# 9. ResidentCorpus.remove: by external passage id
def test_resident_corpus_remove(tmp_path, oracle):
    from haconvdr_amd.passages import write_embedding_block
    from haconvdr_amd.search import ResidentCorpus
    d, n0, n1, nq, topN = 768, 150, 101, 4, 10
    x = synth.embeddings(0x4FA, n0 + n1, d)
    q = synth.embeddings(0x4FB, nq, d)
    ext = np.arange(n0 + n1, dtype=np.int64) * 7 + 1000
    _, top = oracle.flat_ip_search(x, q, 40)
    r0 = int(top[0, 0])                                                  # query 0's best row ...
    r1 = int(next(r for r in top[0, 1:] if (r < n0) != (r0 < n0)))       # ... and the best one the other block holds
    ext[r1] = ext[r0]                                                    # one external id, a row of each block
    write_embedding_block(str(tmp_path), 0, x[:n0], ext[:n0])
    write_embedding_block(str(tmp_path), 1, x[n0:], ext[n0:])
    rc = ResidentCorpus(str(tmp_path), 2)
    shared, absent = int(ext[r0]), 999                                   # 999: held by no block
    r2 = int(next(r for r in top[1] if r not in (r0, r1)))
    assert rc.remove([shared, absent, int(ext[r2]), -1]) == 3
    rows = [r0, r1, r2]
    xs, ext_s = remove_ref.removed(x, rows), remove_ref.removed(ext, rows)
    assert rc.ntotal == n0 + n1 - 3 and rc.sizes == [n0, n1]
    D, I = rc.search(q, topN)
    rc.index.check_status()
    oD, oI = oracle.flat_ip_search(xs, q, topN)
    np.testing.assert_array_equal(I, ext_s[oI])
    np.testing.assert_array_equal(D, oD.astype(np.float64))
    assert shared not in I and int(ext[r2]) not in I
    np.testing.assert_array_equal(rc.rows_of([shared, int(ext[r2]), absent]), [-1, -1, -1])
    np.testing.assert_array_equal(rc.rows_of(ext_s[[0, 100, len(ext_s) - 1]]), [0, 100, len(ext_s) - 1])
    assert rc.remove([absent]) == 0 and rc.ntotal == n0 + n1 - 3
