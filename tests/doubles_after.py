"""Test double (tests only) of ShardedSearcher's local_after_keys hook: tests/after_ref.py over the shard's rows, packed like
index.search_after_keys_tensor packs.  CALLS records (k, has cursor, pos_base) of every call."""
import torch

from tests import after_ref, rank_ref

CALLS = []


def make_local_after_keys(oracle, x_shard):
    def local_after_keys(q, k, after_keys, base):
        CALLS.append((int(k), after_keys is not None, int(base)))
        S = rank_ref.canon_scores(oracle, x_shard, q.numpy())
        keys = after_ref.after_from_keys(S, None if after_keys is None else after_keys.numpy(), int(base), int(k))
        return torch.from_numpy(keys.view("int64"))
    return local_after_keys
