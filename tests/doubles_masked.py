"""Test double (tests only) of ShardedSearcher's local_masked_keys hook: tests/masked_ref.py over the shard's rows, packed like
index.search_masked_keys_tensor packs (tests/doubles.py restates the key format).  CALLS records (k, n_masks, words, pos_base)
of every call."""
import numpy as np
import torch

from haconvdr_amd.index import unpack_mask
from tests import doubles, masked_ref

CALLS = []


def make_local_masked_keys(oracle, x_shard):
    def local_masked_keys(q, k, local_masks, mask_of, base):
        CALLS.append((int(k), int(local_masks.shape[0]), int(local_masks.shape[1]), int(base)))
        masks = unpack_mask(local_masks.numpy(), len(x_shard))
        D, I = masked_ref.masked(oracle, x_shard, q.numpy(), masks, None if mask_of is None else mask_of.numpy(), k)
        return torch.from_numpy(doubles.pack_keys(D, np.where(I >= 0, I + base, -1)))
    return local_masked_keys
