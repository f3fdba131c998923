"""Test doubles (tests only) for the two rank hooks of haconvdr_amd.sharded.ShardedSearcher, beside tests/doubles.py: numpy /
oracle stand-ins for FlatIPIndex.score_ids_tensor and FlatIPIndex.count_ahead_tensor over one shard's rows, restating their
contracts from include/haconvdr.h."""
import numpy as np
import torch

from tests import rank_ref

FMAX = np.finfo(np.float32).max
CALLS = []          # ("scores" | "counts", shape) of every call


def make_local_scores(oracle, x_shard):
    """(q, local ids [nq, m]) -> float32 [nq, m]: the canonical score, -FLT_MAX for an id outside [0, n_local)."""
    def local_scores(q, ids):
        ids = ids.numpy()
        CALLS.append(("scores", ids.shape))
        n = len(x_shard)
        S = rank_ref.canon_scores(oracle, x_shard, q.numpy())
        inside = (ids >= 0) & (ids < n)
        got = np.take_along_axis(S, np.where(inside, ids, 0), 1) if n else np.zeros(ids.shape, np.float32)
        return torch.from_numpy(np.where(inside, got, np.float32(-FMAX)).astype(np.float32))
    return local_scores


def make_count_ahead(oracle, x_shard):
    """(q, ref_scores [nq, m], ref_bounds [nq, m]) -> int64 [nq, m] over the shard's rows; -1 for a NaN score or a bound < 0."""
    def count_ahead(q, ref_scores, ref_bounds):
        CALLS.append(("counts", tuple(ref_bounds.shape)))
        assert ref_scores.dtype == torch.float32 and ref_bounds.dtype == torch.int64
        S = rank_ref.canon_scores(oracle, x_shard, q.numpy())
        return torch.from_numpy(rank_ref.count_ahead(S, ref_scores.numpy(), ref_bounds.numpy()))
    return count_ahead
