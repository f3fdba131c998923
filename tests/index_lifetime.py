"""Index lifetimes (tests only): a numpy model of the live rows of a FlatIPIndex, one comparer for every search route, rows
planted so that whatever lands on a group, piece or segment edge is some query's winner, and the case tables of
tests/test_index_lifetime_gpu.py.  Nothing here needs a GPU: tests/test_index_lifetime.py checks the tables and the comparer
on the CPU, against a fake index that answers from the oracle.

The index keeps four kinds of state that have to follow the rows: the T64 tiles (a segment's tail group may be partial), the
fp16 image the prefilter streams, the row-major copy the rescoring reads, and the bookkeeping around them (norm2_max, the
segment table, the multi-device spans).  `Life.check` looks at all of them through the public calls only: one search by a
named route, bit for bit against oracle.flat_ip_search over the model's rows, the plan text of that route, the rows read
back as words, and the scores of the returned ids by score_ids."""
import numpy as np

FMAX = np.finfo(np.float32).max
GROUP = 64
N_PLAIN = 8                                   # the last queries of every set are plain Gaussian ones
NQ = 40                                       # queries of a case: NQ - N_PLAIN planted, N_PLAIN plain
COEF = (3.0, 2.5, 2.0)                        # planted rows are COEF * q_j: row where[j], where[j] - 1, where[j] + 1
MARGIN = 2.0                                  # rank 1 >= MARGIN x the best row that was not planted for the query

# route -> (queries, options set on the live handle, entry point, how the plan text must start, what it must contain)
ROUTES = {
    "scan16": (3, {"split": "0"}, "host", "scan16_kernel<", ()),
    "scanq": (NQ, {"split": "0"}, "host", "scanq_kernel<", ()),
    "pre1": (NQ, {"split": "1", "split_terms": "1", "split_decide": "auto"}, "host", "split: scanh_kernel<1>", ()),
    "pre3": (NQ, {"split": "1", "split_terms": "3", "split_decide": "auto"}, "host", "split: scanh_kernel<3>", ()),
    "pre_dev": (NQ, {"split": "1", "split_terms": "1", "split_decide": "device"}, "tensor", "split: scanh_kernel<1>", ("decided=device",)),
    # shapes the planner keeps away from the prefilter or from scanq, whatever the options say
    "scan16_many": (NQ, {"split": "0"}, "host", "scan16_kernel<", ()),          # d % 64 == 32: scan16 at every query count
    "few_rows16": (3, {"split": "1", "split_terms": "1", "split_decide": "auto"}, "host", "scan16_kernel<", ()),   # fewer rows than SPLIT_K2
    "few_rowsq": (NQ, {"split": "1", "split_terms": "1", "split_decide": "auto"}, "host", "scanq_kernel<", ()),
}
ALL5 = ("scan16", "scanq", "pre1", "pre3", "pre_dev")
RESTORE = {"split_terms": "1", "split_decide": "auto"}


def roundup64(n):
    return (n + GROUP - 1) // GROUP * GROUP


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(D, I, oD, oI):
    from tests.test_search_gpu import assert_same as same          # the comparer of the search tests (NaN-safe)
    same(D, I, oD, oI)


def fallback_of(plan):
    """'... fallback=a/b ...' of a prefilter plan -> (a, b)."""
    assert plan.startswith("split:"), plan
    a, b = plan.split("fallback=")[1].split()[0].split("/")
    return int(a), int(b)


class LifeMismatch(AssertionError):
    """What Life.check found: `what` names the comparison, `queries` the indices (into life.q) of the queries that differ
    (empty where the comparison is not per query)."""

    def __init__(self, what, queries, text):
        super().__init__(f"{what}: {text}")
        self.what = what
        self.queries = tuple(int(i) for i in queries)


# ---------------------------------------------------------------------------------------------------------------------
# planted winners
def planted(rng, n, where, nq, d=768):
    """(x float32 [n, d], q float32 [nq, d]): background rows N(0, 1), queries N(0, 1); row where[j] is query j's rank 1 and
    rows where[j] - 1 / where[j] + 1 (where they exist) its ranks 2 and 3, for the first nq - N_PLAIN queries.  A planted row
    is the sum of COEF * q_j over the queries that claim it (edges come in pairs: 64m - 1 and 64m are neighbours), with no
    background: |q_j|^2 ~ d against cross terms q_i . q_j ~ sqrt(d) keeps the order, and check_planted asserts it."""
    where = [int(w) for w in where]
    assert len(where) == nq - N_PLAIN and len(set(where)) == len(where), (len(where), nq)
    assert all(0 <= w < n for w in where), (n, where)
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    touched = sorted({r for w in where for r in (w - 1, w, w + 1) if 0 <= r < n})
    x[touched] = 0.0
    for j, w in enumerate(where):
        for c, r in zip(COEF, (w, w - 1, w + 1)):
            if 0 <= r < n:
                x[r] += np.float32(c) * q[j]
    return x, q


def check_planted(oracle, x, q, where, n_live=None):
    """From the oracle alone: over the rows x[:n_live], every planted query whose row is live has it at rank 1, its live
    neighbours behind it in COEF order, and rank 1 >= MARGIN x the best other row.  Returns the number of queries checked."""
    n = len(x) if n_live is None else int(n_live)
    live = [(j, int(w)) for j, w in enumerate(where) if w < n]
    if not live or n == 0:
        return 0
    D, I = oracle.flat_ip_search(x[:n], q[[j for j, _ in live]], 4)
    for i, (j, w) in enumerate(live):
        want = [r for r in (w, w - 1, w + 1) if 0 <= r < n]
        assert I[i, :len(want)].tolist() == want, (j, w, n, I[i].tolist())
        if I[i, len(want)] >= 0:                          # (no other row at all in a tiny index)
            assert D[i, 0] > 0 and D[i, 0] >= MARGIN * D[i, len(want)], (j, w, n, D[i].tolist())
    return len(live)


def fill_where(rng, edges, n, total=NQ - N_PLAIN):
    """The edge rows first (in the order given, duplicates dropped), then distinct random rows of [0, n) up to `total`."""
    where = list(dict.fromkeys(int(e) for e in edges))
    assert len(where) <= total and all(0 <= w < n for w in where), (len(where), total, n)
    seen = set(where)
    while len(where) < total:
        r = int(rng.integers(0, n))
        if r not in seen:
            seen.add(r)
            where.append(r)
    return where


# ---------------------------------------------------------------------------------------------------------------------
# the model
class Life:
    """The rows an index should hold (add / reset / rows) and the queries they are searched with."""

    def __init__(self, q, where, split="1"):
        self.q = np.ascontiguousarray(q, np.float32)
        self.where = [int(w) for w in where]
        self.rows = np.zeros((0, self.q.shape[1]), np.float32)
        self.split = split                                 # what `split` goes back to after a checkpoint

    def add(self, x):
        self.rows = np.concatenate([self.rows, np.ascontiguousarray(x, np.float32)], 0)

    def reset(self, q=None, where=None):
        self.rows = self.rows[:0]
        if q is not None:
            self.q, self.where = np.ascontiguousarray(q, np.float32), [int(w) for w in where]

    def queries_of(self, route):
        """Indices into self.q.  The 3-query route takes the two planted queries whose rows are the highest live ones (the
        newest edges: the index's last row is always planted) and the last plain query."""
        nq = ROUTES[route][0]
        if nq >= len(self.q):
            return np.arange(len(self.q))
        live = sorted((w, j) for j, w in enumerate(self.where) if w < len(self.rows))
        pick = [j for _, j in live[-(nq - 1):]]
        pick += [j for j in range(len(self.q)) if j not in pick][:nq - 1 - len(pick)]
        return np.array(pick + [len(self.q) - 1])

    def check(self, idx, oracle, route, k, rescore=None):
        """One search by `route`; returns (plan, D, I).  Raises LifeMismatch / AssertionError."""
        nq, options, entry, head, inside = ROUTES[route]
        sel = self.queries_of(route)
        q = self.q[sel]
        for name, value in options.items():
            idx.set_option(name, value)
        try:
            if entry == "tensor":
                D, I = _device_search(idx, q, k)
            else:
                D, I = idx.search(q, k)
            plan = idx.last_plan()
            idx.check_status()
        finally:
            for name, value in dict(RESTORE, split=self.split).items():
                idx.set_option(name, value)
        assert plan.startswith(head) and all(s in plan for s in inside), (route, head, inside, plan)
        if rescore is not None and head.startswith("split:"):
            assert f"rescore={rescore}" in plan.split(" ; then ")[0], (route, rescore, plan)
        assert D.shape == (len(q), k) and I.shape == (len(q), k) and D.dtype == np.float32 and I.dtype == np.int64
        oD, oI = oracle.flat_ip_search(self.rows, q, k)
        bad = [sel[i] for i in range(len(q)) if not (np.array_equal(I[i], oI[i]) and _same_words(D[i], oD[i]))]
        if bad:
            i = list(sel).index(bad[0])
            raise LifeMismatch(f"search by {route}", bad, f"queries {bad} differ from the oracle over {len(self.rows)} rows; query {bad[0]}: "
                               f"ids {I[i][:6].tolist()} scores {D[i][:6].tolist()}, oracle {oI[i][:6].tolist()} {oD[i][:6].tolist()} ({plan})")
        assert_same(D, I, oD, oI)
        rows = idx.reconstruct_n()
        if rows.shape != self.rows.shape or not np.array_equal(bits(rows), bits(self.rows)):
            first = -1 if rows.shape != self.rows.shape else int(np.flatnonzero((bits(rows) != bits(self.rows)).any(1))[0])
            raise LifeMismatch(f"reconstruct_n after {route}", (), f"shape {rows.shape} vs {self.rows.shape}, first differing row {first}")
        S = idx.score_ids(q, I)
        badS = [sel[i] for i in range(len(q)) if not _same_words(S[i], D[i])]
        if badS:
            raise LifeMismatch(f"score_ids after {route}", badS, f"scores of the returned ids differ from the search's for queries {badS}")
        assert (S[I < 0] == -FMAX).all()
        return plan, D, I


def _same_words(a, b):
    """float32 vectors equal word for word, a NaN equal to any NaN (its payload is the hardware's)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def _device_search(idx, q, k):
    import torch
    dev = idx.devices[0]
    dev = torch.device(dev) if isinstance(dev, str) else torch.device("cuda", dev)
    D, I = idx.search_tensor(torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(dev), k)
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    return D.cpu().numpy(), I.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# the case tables of tests/test_index_lifetime_gpu.py: (rows, queries, planted rows, the adds as row counts)
def _cum(pieces):
    return np.cumsum(pieces).tolist()


A_PIECES = (4096 + 17, 1, 46, 1, 63, 64, 65, 127)


def case_a():
    """Adds into every edge: 4113 rows, then pieces that end inside a group, fill the segment to its last row (4160), open
    one-row, one-group and two-group segments and straddle a segment end (the 127-row piece: 63 rows fill the tail, 64 open
    the next segment at row 4416)."""
    rng = np.random.default_rng(0xA11FE)
    cum = _cum(A_PIECES)
    n = cum[-1]
    edges = []
    for lo, hi in zip([0] + cum[:-1], cum):
        edges += [hi - 1, lo]                              # last and first row of the piece (hi - 1: the last row before the next add)
    edges += [4415, 4416, 4351, 63, 64, 4095, 4096, 2047, 2048]
    where = fill_where(rng, edges, n)
    x, q = planted(rng, n, where, NQ)
    return x, q, where, A_PIECES


B_N1, B_HOSTILE = 3000, 200
B_N2 = (257, 1000, 1025)
B_LIFE3 = 70


def hostile_rows(rng, n, d=768):
    """n rows holding, in turn: a NaN, +Inf, -Inf (one element of a Gaussian row each), all 3.3e38, and a row of norm 7e4
    (every element 7e4 / sqrt(d): finite in fp32, its norm beyond fp16)."""
    x = rng.standard_normal((n, d)).astype(np.float32)
    for i in range(n):
        kind, col = i % 5, (7 * i + 3) % d
        if kind == 0:
            x[i, col] = np.nan
        elif kind == 1:
            x[i, col] = np.inf
        elif kind == 2:
            x[i, col] = -np.inf
        elif kind == 3:
            x[i] = np.float32(3.3e38)
        else:
            x[i] = np.float32(7e4 / np.sqrt(d))
    return x


def case_b(n2):
    """(life 1 rows, life 2 rows, life 3 rows, q, where of life 2): life 1 is Gaussian with the hostile rows at [n2, n2 + 200),
    life 2 ends on planted rows n2 - 1 and n2 - 2, life 3 is 70 plain rows."""
    rng = np.random.default_rng(0xB0B + n2)
    x1 = rng.standard_normal((B_N1, 768)).astype(np.float32)
    x1[n2:n2 + B_HOSTILE] = hostile_rows(rng, B_HOSTILE)
    where = fill_where(rng, [n2 - 1, n2 - 2, 255, 256, 63, 64, 0], n2)
    x2, q = planted(rng, n2, where, NQ)
    x3 = rng.standard_normal((B_LIFE3, 768)).astype(np.float32)
    return x1, x2, x3, q, where


C_SEG_ROWS, C_TAIL_PIECES = 128, (100, 100, 100)
C_CHECKPOINTS = (10, 64, 65)                               # live segments of 128 rows at the first three checkpoints


def case_c(d=768):
    """65 adds of 128 rows (the 65th fuses the 64 segments before it), then three adds of 100."""
    rng = np.random.default_rng(0xC5E6 + d)
    pieces = (C_SEG_ROWS,) * 65 + C_TAIL_PIECES
    cum = _cum(pieces)
    n = cum[-1]
    edges = []
    for s in (0, 31, 63, 64, 9):                           # first row of the first group, last row of the last group
        edges += [C_SEG_ROWS * s, C_SEG_ROWS * s + C_SEG_ROWS - 1]
    for lo, hi in zip(cum[64:-1], cum[65:]):               # the post-consolidation adds
        edges += [lo, hi - 1]
    edges += [C_SEG_ROWS * 31 + 63, C_SEG_ROWS * 31 + 64, C_SEG_ROWS * 63 + 63, C_SEG_ROWS * 63 + 64, 8447, 8448]
    where = fill_where(rng, edges, n)
    x, q = planted(rng, n, where, NQ, d)
    return x, q, where, pieces


D_LIVES = ((300, 1, 700), (513, 64))


def shard_shares(pieces, n_shards=2):
    """[(first row, rows)] of every shard's share of every add, as hac_index_add splits them (n // S, the first n % S
    shards one more), in global numbering."""
    out, base = [], 0
    for n in pieces:
        off = 0
        for s in range(n_shards):
            m = n // n_shards + (1 if s < n % n_shards else 0)
            if m:
                out.append((base + off, m))
            off += m
        base += n
    return out


def case_d(life):
    rng = np.random.default_rng(0xD0D0 + life)
    pieces = D_LIVES[life]
    n = sum(pieces)
    edges = []
    for lo, m in shard_shares(pieces):
        edges += [lo, lo + m - 1]
    where = fill_where(rng, edges, n)
    x, q = planted(rng, n, where, NQ)
    return x, q, where, pieces


def checkpoints_of(name):
    """(x, q, where, [live rows at each checkpoint]) of every case table: what tests/test_index_lifetime.py checks margins on."""
    if name == "A":
        x, q, where, pieces = case_a()
        return [(x, q, where, _cum(pieces))]
    if name == "B":
        return [(case_b(n2)[1], case_b(n2)[3], case_b(n2)[4], [n2]) for n2 in B_N2]
    if name == "C":
        out = []
        for d in (768, 96):
            x, q, where, pieces = case_c(d)
            cum = _cum(pieces)
            out.append((x, q, where, [cum[c - 1] for c in C_CHECKPOINTS] + [cum[-1]]))
        return out
    if name == "D":
        return [case_d(life)[:3] + (_cum(D_LIVES[life])[-1:],) for life in range(len(D_LIVES))]
    raise KeyError(name)
