"""Expectations of search_excluding (tests only), both from the CPU oracle's flat_ip_search and numpy alone.

filtered_topk  (a) the oracle's top-(k + e) of the whole corpus, filtered: what the implementation does, restated on the host.
deleted_topk   (b) per query, the oracle's top-k over the corpus with the excluded rows DELETED, rows mapped back.  It does not
               assume that the top-k of (rows minus E) lies inside the top-(k + e) of the rows: agreeing with (a) proves it."""
import numpy as np

FMAX = np.finfo(np.float32).max


def _valid(row, n):
    return row[(row >= 0) & (row < n)]


def filtered_topk(oracle, x, q, k, excl):
    excl = np.asarray(excl, np.int64).reshape(len(q), -1)
    oD, oI = oracle.flat_ip_search(x, q, k + excl.shape[1])
    D = np.full((len(q), k), -FMAX, np.float32)
    I = np.full((len(q), k), -1, np.int64)
    for i in range(len(q)):
        keep = (oI[i] >= 0) & ~np.isin(oI[i], _valid(excl[i], len(x)))
        m = min(k, int(keep.sum()))
        D[i, :m], I[i, :m] = oD[i][keep][:m], oI[i][keep][:m]
    return D, I


def deleted_topk(oracle, x, q, k, excl):
    excl = np.asarray(excl, np.int64).reshape(len(q), -1)
    D = np.empty((len(q), k), np.float32)
    I = np.empty((len(q), k), np.int64)
    for i in range(len(q)):
        gone = np.unique(_valid(excl[i], len(x)))
        left = np.delete(np.arange(len(x)), gone)
        d, j = oracle.flat_ip_search(np.delete(x, gone, 0), q[i:i + 1], k)
        D[i], I[i] = d[0], np.where(j[0] >= 0, left[np.clip(j[0], 0, None)] if len(left) else -1, -1)
    return D, I


def exclusion_sets(oracle, x, q, k, e):
    """The issue's five contents for one (k, e): name -> int64 [nq, e] (the last one [nq, 0])."""
    nq, n = len(q), len(x)
    _, top = oracle.flat_ip_search(x, q, k + 2 * e)
    worst = np.argsort(oracle.ip_scores(x, q), axis=1, kind="stable")[:, :e]            # far outside any top-(k + e)
    assert n >= k + 3 * e and not any(np.isin(worst[i], top[i]).any() for i in range(nq))
    holes = np.full((nq, e), -1, np.int64)
    for j in range(e):
        if j % 3 != 2:
            holes[:, j] = top[:, j // 3]                                                 # every named row twice; every third slot -1
    return {
        "own top-e": top[:, :e].copy(),
        "every second of top-2e": top[:, 0:2 * e:2].copy(),
        "outside top-(k+e)": worst.astype(np.int64),
        "duplicates and holes": holes,
        "e = 0": np.zeros((nq, 0), np.int64),
    }
