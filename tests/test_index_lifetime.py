"""tests/index_lifetime.py on the CPU: the planted winners of every case table of tests/test_index_lifetime_gpu.py really are
winners at every checkpoint (from the oracle alone: no case is vacuous), and Life.check, given a fake index that answers
from the oracle, passes while the fake masks what lies behind its row count and fails -- in a PLANTED query -- for each of
the three ways an index can get a group, piece or segment edge wrong."""
import numpy as np
import pytest

from tests import index_lifetime as il
from tests.index_lifetime import FMAX, Life, LifeMismatch, roundup64


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_planted_rows_win_with_margin_at_every_checkpoint(name, oracle):
    for x, q, where, sizes in il.checkpoints_of(name):
        assert len(q) == il.NQ and len(where) == il.NQ - il.N_PLAIN
        assert sizes[-1] == len(x) <= 12000
        for n in sizes:
            checked = il.check_planted(oracle, x, q, where, n)
            assert checked >= 2, (name, n)                                  # the newest edges are planted at every checkpoint
            assert n - 1 in where, (name, n)                                # ... the index's last row among them
        assert il.check_planted(oracle, x, q, where) == len(where)


def test_case_tables_put_rows_on_the_edges_they_are_named_for():
    _, _, where, pieces = il.case_a()
    cum = np.cumsum(pieces).tolist()
    assert cum == [4113, 4114, 4160, 4161, 4224, 4288, 4353, 4480]
    for lo, hi in zip([0] + cum[:-1], cum):
        assert lo in where and hi - 1 in where
    assert {4159, 4160, 4415, 4416}.issubset(where)                         # segment ends of the handle: 4160 (first add's capacity), 4416
    for n2 in il.B_N2:
        x1, x2, x3, q, w = il.case_b(n2)
        assert len(x1) == il.B_N1 and len(x2) == n2 and len(x3) == 70 and {n2 - 1, n2 - 2}.issubset(w)
        h = x1[n2:n2 + il.B_HOSTILE]
        assert np.isnan(h[0::5]).any(1).all() and np.isposinf(h[1::5]).any(1).all() and np.isneginf(h[2::5]).any(1).all()
        assert (h[3::5] == np.float32(3.3e38)).all()
        norms = np.sqrt((h[4::5].astype(np.float64) ** 2).sum(1))
        assert np.isfinite(h[4::5]).all() and (np.abs(norms - 7e4) < 1).all() and 7e4 > float(np.finfo(np.float16).max)
        assert np.isfinite(x1[:n2]).all() and np.isfinite(x1[n2 + il.B_HOSTILE:]).all() and np.isfinite(x2).all()
        assert roundup64(n2) - n2 <= il.B_HOSTILE                           # the live tail group's padding is hostile throughout
    _, _, where, pieces = il.case_c()
    assert sum(pieces[:64]) == 8192 and sum(pieces) == 8620
    for s in (0, 31, 63, 64):
        assert 128 * s in where and 128 * s + 127 in where
    assert il.shard_shares((300, 1, 700)) == [(0, 150), (150, 150), (300, 1), (301, 350), (651, 350)]
    assert il.shard_shares((513, 64)) == [(0, 257), (257, 256), (513, 32), (545, 32)]


# ---------------------------------------------------------------------------------------------------------------------
class FakeIndex:
    """The calls Life.check makes, answered from the oracle over the rows added since the last reset.  Like the real index it
    keeps a buffer that reset() does not clear (rows of the life before stay behind the count) and MASKS it by the count.
    `mutate` takes the masking away in one of three ways, in what a search scans only (rows read back and scored by id
    stay honest, so a failure is the search comparison's):
      "tail_zeroed": the last ntotal % 64 rows score as zero rows (a partial tail group that was never tiled);
      "stale_tail":  rows [ntotal, roundup64(ntotal)) of the life before are still searched;
      "swap":        rows `swap_at` and `swap_at + 1` (the first group of a new segment) change places."""
    devices = ("cpu",)

    def __init__(self, oracle, d=768, mutate=None, swap_at=None):
        self.oracle, self.d, self.mutate, self.swap_at = oracle, d, mutate, swap_at
        self.buf = np.zeros((0, d), np.float32)              # what the device memory holds, stale rows included
        self.ntotal = 0
        self.opt = {"split": "auto", "split_terms": "1", "split_decide": "auto", "rescore_rows": "auto"}
        self.plan = "none"

    def set_option(self, name, value):
        assert name in self.opt, name
        self.opt[name] = value

    def add(self, x):
        x = np.ascontiguousarray(x, np.float32)
        end = self.ntotal + len(x)
        if end > len(self.buf):
            self.buf = np.concatenate([self.buf, np.zeros((end - len(self.buf), self.d), np.float32)], 0)
        self.buf[self.ntotal:end] = x
        self.ntotal = end

    def reset(self):
        self.ntotal = 0

    def _scanned(self):
        n = self.ntotal
        x = self.buf[:n].copy()
        if self.mutate == "tail_zeroed" and n % 64:
            x[n - n % 64:] = 0.0
        elif self.mutate == "stale_tail":
            x = self.buf[:min(roundup64(n), len(self.buf))].copy()
        elif self.mutate == "swap" and self.swap_at + 1 < n:
            x[[self.swap_at, self.swap_at + 1]] = x[[self.swap_at + 1, self.swap_at]]
        return x

    def _search(self, q, k, device):
        nq = len(q)
        D, I = self.oracle.flat_ip_search(self._scanned(), q, k)
        pre = self.opt["split"] == "1" and self.d % 64 == 0 and self.d >= 192 and k <= 192 and self.ntotal >= 256
        if pre:
            self.plan = (f"split: scanh_kernel<{self.opt['split_terms']}> grid=(1,1) NQ=256 K2=256 chunks=1 lds=0 seed=0 passes=1 "
                         f"rescore={'tiles' if self.opt['rescore_rows'] == '0' else 'rows'} fallback=0/{nq} err/bound=0"
                         + (" decided=device" if device or self.opt["split_decide"] == "device" else ""))
        elif nq > 16 and self.d % 64 == 0:
            self.plan = f"scanq_kernel<NT=2,W=8> grid=(1,1) NQ=64 C=128 lds=0 seed=0"
        else:
            self.plan = f"scan16_kernel<W=4> grid=(1,1) QT={min(nq, 16)} C=512 lds=0 seed=0"
        return D, I

    def search(self, q, k):
        return self._search(np.ascontiguousarray(q, np.float32), k, False)

    def search_tensor(self, q, k):
        import torch
        D, I = self._search(q.numpy(), k, True)
        return torch.from_numpy(D), torch.from_numpy(I)

    def last_plan(self):
        return self.plan

    def check_status(self):
        pass

    def reconstruct_n(self):
        return self.buf[:self.ntotal].copy()

    def score_ids(self, q, ids):
        S = (self.oracle.ip_scores(self.buf[:max(self.ntotal, 1)], q) + np.float32(0.0)).astype(np.float32)
        out = np.take_along_axis(S, np.clip(ids, 0, None), 1)
        out[ids < 0] = -FMAX
        return out


def _life_a(oracle, fake, upto=None):
    """Scenario A's adds on `fake`, a checkpoint by every route after each; returns the Life."""
    x, q, where, pieces = il.case_a()
    life = Life(q, where)
    fake.set_option("split", "1")
    fake.set_option("rescore_rows", "1")
    lo = 0
    for m in pieces[:upto]:
        fake.add(x[lo:lo + m])
        life.add(x[lo:lo + m])
        lo += m
        for route in il.ALL5:
            plan, D, I = life.check(fake, oracle, route, 10, rescore="rows")
            assert fake.opt["split"] == "1" and fake.opt["split_terms"] == "1" and fake.opt["split_decide"] == "auto"
    return life


def _planted_failure(e, life):
    planted = set(range(len(life.where)))
    assert e.what.startswith("search by"), str(e)
    assert planted & set(e.queries), f"only plain queries noticed: {e.queries}"


def test_comparer_passes_on_an_index_that_masks_its_padding(oracle):
    life = _life_a(oracle, FakeIndex(oracle))
    assert len(life.rows) == 4480
    # scenario B's shape: a hostile life behind the count, then short lives, then fewer rows than the prefilter takes
    x1, x2, x3, q, where = il.case_b(1000)
    fake = FakeIndex(oracle)
    life = Life(q, where)
    fake.add(x1), life.add(x1)
    for route in il.ALL5:
        life.check(fake, oracle, route, 10)
    fake.reset(), life.reset()
    fake.add(x2), life.add(x2)
    for route in il.ALL5:
        plan, D, I = life.check(fake, oracle, route, 10)
    assert il.fallback_of(plan) == (0, il.NQ)
    fake.reset(), life.reset()
    fake.add(x3), life.add(x3)
    for route in ("few_rows16", "few_rowsq"):
        plan, D, I = life.check(fake, oracle, route, 100)
        assert (I[:, 70:] == -1).all() and (D[:, 70:] == -FMAX).all() and (I[:, :70] >= 0).all()


@pytest.mark.parametrize("route", il.ALL5)
def test_comparer_fails_in_a_planted_query_when_the_partial_tail_group_is_lost(route, oracle):
    x, q, where, pieces = il.case_a()
    fake, life = FakeIndex(oracle, mutate="tail_zeroed"), Life(q, where)
    fake.add(x[:pieces[0]]), life.add(x[:pieces[0]])                        # 4113 rows: 17 in the tail group
    with pytest.raises(LifeMismatch) as e:
        life.check(fake, oracle, route, 10)
    _planted_failure(e.value, life)
    j = where.index(pieces[0] - 1)
    assert j in e.value.queries                                             # the query planted on the last row


@pytest.mark.parametrize("n2", il.B_N2)
def test_comparer_fails_in_a_planted_query_when_rows_of_the_life_before_are_searched(n2, oracle):
    x1, x2, x3, q, where = il.case_b(n2)
    for route in il.ALL5:
        fake, life = FakeIndex(oracle, mutate="stale_tail"), Life(q, where)
        fake.add(x1), fake.reset(), fake.add(x2), life.add(x2)
        with pytest.raises(LifeMismatch) as e:
            life.check(fake, oracle, route, 10)
        _planted_failure(e.value, life)


def test_comparer_fails_in_a_planted_query_when_a_new_segments_first_rows_change_places(oracle):
    x, q, where, pieces = il.case_a()
    cum = np.cumsum(pieces).tolist()
    for upto, at in ((5, 4160), (8, 4416)):                                 # the one-row segment's row and its successor; the segment the 127-row piece opens
        fake = FakeIndex(oracle, mutate="swap", swap_at=at)
        with pytest.raises(LifeMismatch) as e:
            _life_a(oracle, fake, upto)
        _planted_failure(e.value, Life(q, where))
        assert {j for j, w in enumerate(where) if w in (at, at + 1)} & set(e.value.queries)
    assert cum[3] == 4161 and cum[4] == 4224


def test_comparer_notices_rows_and_scores_too(oracle):
    x, q, where, pieces = il.case_a()
    fake, life = FakeIndex(oracle), Life(q, where)
    fake.add(x[:500]), life.add(x[:500])
    life.check(fake, oracle, "pre1", 10)
    fake.buf.view(np.uint32)[499, 700] ^= 1                                 # one bit of one row, after the search was answered
    honest = fake._scanned
    fake._scanned = lambda: life.rows
    with pytest.raises(LifeMismatch) as e:
        life.check(fake, oracle, "scanq", 10)
    assert e.value.what.startswith("reconstruct_n"), str(e.value)
    fake._scanned = honest
    fake.buf[:500] = life.rows
    fake.score_ids = lambda q_, ids: np.zeros(ids.shape, np.float32)
    with pytest.raises(LifeMismatch) as e:
        life.check(fake, oracle, "scan16", 10)
    assert e.value.what.startswith("score_ids"), str(e.value)
    other = FakeIndex(oracle)                                               # a route that was not taken fails the checkpoint
    other.set_option("split", "1")
    other.add(x[:500])
    with pytest.raises(AssertionError, match="few_rowsq"):
        life.check(other, oracle, "few_rowsq", 10)
