"""Inputs of the search_masked GPU tests (tests only, numpy only), kept apart from them so that tests/test_index_masked.py can
prove on the CPU that the inputs show what they are for: that per-query masks inside one tile really differ in their answers,
that the deselected rows really are the unmasked answer."""
import numpy as np

from haconvdr_amd import synth
from tests.golden import cases

D, N, NQ = 96, 5000, 37          # 79 groups, the last of 8 rows; 37 queries: three tiles of 16, the last partial


def base_case():
    """-> (x float32 [N, D], q float32 [NQ, D]) Gaussian"""
    x, q, _ = cases.search_case_inputs("gauss", 0xA00, N, NQ, d=D)
    return x, q


def random_masks(seed, n_masks, n, one_in):
    """bool [n_masks, n], every row selected with probability 1 / one_in"""
    return (synth.uniform_u32(seed, n_masks * n) % np.uint32(one_in) == 0).reshape(n_masks, n)


def per_query_masks(n=N, nq=NQ):
    """bool [nq, n]: query i's mask has density 1 / (2 + i % 5) and a seed of its own -- neighbours in a tile share few rows"""
    return np.stack([random_masks(0xA10 + i, 1, n, 2 + i % 5)[0] for i in range(nq)])


def grouped_masks(n=N, nq=NQ):
    """(bool [5, n], mask_of int64 [nq]): five masks of different densities, dealt to the queries out of order, so that every
    tile of 16 (and of 4) holds several of them"""
    masks = np.stack([random_masks(0xA20 + m, 1, n, (2, 64, 3, 1000, 7)[m])[0] for m in range(5)])
    mask_of = (np.arange(nq) * 3 + np.arange(nq) // 7) % 5
    return masks, mask_of.astype(np.int64)


def disjoint_masks(n=N, nq=16):
    """bool [nq, n], pairwise disjoint: mask i selects the rows r with r % nq == i -- every group is in the tile's list and each
    lane may take a sixteenth of it"""
    return (np.arange(n)[None, :] % nq) == np.arange(nq)[:, None]


def deselected_half(S):
    """bool [nq, n]: per query the lower-scoring half of its rows (NaN scores count as low)"""
    S = np.where(np.isnan(S), -np.inf, S.astype(np.float64))
    return S < np.median(S, axis=1, keepdims=True)


def monotone_case(ascending):
    """-> (x [N, D], q [5, D]): scores that ascend (or descend) with the row for every query -- ascending, every row of a dense
    mask beats every threshold so far and every compaction keeps only the newest rows"""
    v = cases.search_case_inputs("gauss", 0xA30, 1, 1, d=D)[1][0]
    ramp = 1.0 + np.arange(N, dtype=np.float64) / N
    if not ascending:
        ramp = ramp[::-1]
    x = (v[None, :].astype(np.float64) * ramp[:, None]).astype(np.float32)
    q = (v[None, :] * np.array([1.0, 0.5, 2.0, 3.0, 0.25], np.float32)[:, None]).astype(np.float32)
    return x, q


def union_of_tile(masks, mask_of, QT):
    """bool [nq, n]: per query the OR of the masks of its tile of QT queries: what a scan that tested the tile's mask, not the
    lane's own, would search"""
    nq = len(mask_of)
    out = np.zeros((nq, masks.shape[1]), np.bool_)
    for t0 in range(0, nq, QT):
        out[t0:t0 + QT] = masks[mask_of[t0:t0 + QT]].any(axis=0)
    return out
