"""Test double (tests only) of ShardedSearcher's local_among_keys hook: tests/among_ref.py over the shard's rows, packed like
index.search_among_keys_tensor packs (tests/doubles.py restates the key format).  CALLS records (k, m, pos_base) of every call."""
import numpy as np
import torch

from tests import among_ref, doubles

CALLS = []


def make_local_among_keys(oracle, x_shard):
    def local_among_keys(q, k, local_cand, base):
        CALLS.append((int(k), int(local_cand.shape[1]), int(base)))
        D, I = among_ref.among(oracle, x_shard, q.numpy(), local_cand.numpy(), k)
        return torch.from_numpy(doubles.pack_keys(D, np.where(I >= 0, I + base, -1)))
    return local_among_keys
