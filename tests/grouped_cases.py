"""Inputs of the search_grouped GPU tests (tests only, numpy only), kept apart from them so that tests/test_index_grouped.py
can prove on the CPU that the inputs show what they are for.  The rows are the shared 5000-row case of masked_cases: three
adds cut off the 64-row grid (tests/test_search_plans_gpu._index), 79 groups of 64 rows, the last of 8."""
import numpy as np

from haconvdr_amd import synth
from tests import masked_cases

D, N, NQ = masked_cases.D, masked_cases.N, masked_cases.NQ
MAX_K = 2048
GIANT_ROWS = 3000


def plan_tile(d, k, nq):
    """(QT, C, lds) by the grouped plan's arithmetic (include/haconvdr.h, "search by group"): C candidate slots per query and
    one scratch array of C per compacting wave (at most 4, at most QT); as many queries as 160 KiB of LDS hold, <= 16"""
    C = 1 << (k + 256 - 1).bit_length()
    per_q = (d // 4) * 16 + C * 8
    fits = [t for t in range(1, 17) if t * per_q + min(4, t) * C * 8 + 128 <= 160 * 1024]
    QT = min(fits[-1], nq)
    return QT, C, QT * per_q + min(4, QT) * C * 8 + 128


def interleaved_labels(n=N):
    """{name: int64 [n]}: members of a group straddle tiles of rows, row streams, segments and the partial last group"""
    r = np.arange(n, dtype=np.int64)
    perm = np.argsort(synth.uniform_u32(0xB10, n), kind="stable")
    return {"r % 7": r % 7, "r // 3": r // 3, "permuted r // 5": (r // 5)[perm]}


def giant_case():
    """-> (x [N, D], q [16, D], labels int64 [N]): GIANT_ROWS rows, three in every five, carry label 0 and are scaled copies of
    one direction v that every query leans on, so they lead every query's list; the other rows are the base case's, in 997
    groups of two or three rows."""
    x, q = masked_cases.base_case()
    x, q = x.copy(), q[:16].copy()
    v = synth.embeddings(0xB20, 1, D)[0]
    v /= np.float32(np.linalg.norm(v))
    r = np.arange(N)
    giant = r % 5 < 3
    scale = (4.0 + (r % 7) / 8.0).astype(np.float32)                       # few distinct scores: long runs of ties inside the group
    x[giant] = scale[giant, None] * v[None, :]
    q += np.float32(3.0 * np.abs(q).max() * np.sqrt(D)) * v[None, :]       # q . v dominates whatever else the query holds
    labels = np.where(giant, 0, 1 + r % 997).astype(np.int64)
    assert giant.sum() == GIANT_ROWS
    return x, q, labels


def edge_labels(n=N):
    """int64 [n]: the labels 0, 2^32 - 1, 2^31 and 2^31 + 5 among small ones -- a truncation to int32 merges 2^32 - 1 ... with
    nothing legal, a sign slip drops the labels from 2^31 on"""
    r = np.arange(n, dtype=np.int64)
    lab = r % 11
    lab[r % 11 == 3] = 2 ** 32 - 1
    lab[r % 11 == 4] = 2 ** 31
    lab[r % 11 == 5] = 2 ** 31 + 5
    lab[r % 11 == 6] = 2 ** 32 - 1 - 11                                   # low words 0xFFFFFFF4: int32 -12
    return lab


def grid_tie_corpus(d, n, nq, seed):
    """(x, q, labels): rows on a coarse grid and integer queries, so that scores are exact and whole runs of GROUPS tie: group G
    holds rows G, G + n/4, G + n/2, G + 3n/4 (n a multiple of 4), and neighbouring groups share their best row's value"""
    base = ((synth.uniform_u32(seed, 8 * d) % np.uint32(5)).astype(np.float32).reshape(8, d) - 2.0) / 2.0
    r = np.arange(n)
    x = base[(r // 3) % 8]
    q = (synth.uniform_u32(seed + 1, nq * d) % np.uint32(5)).astype(np.float32).reshape(nq, d) - 2.0
    return x, q, (r % (n // 4)).astype(np.int64)
