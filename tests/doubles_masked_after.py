"""Test double (tests only) of ShardedSearcher's local_masked_after_keys hook: tests/masked_after_ref.py over the shard's rows,
packed like index.search_masked_keys_tensor(after_keys=) packs.  CALLS records (k, n_masks, words, has cursor, pos_base) of
every call."""
import torch

from haconvdr_amd.index import unpack_mask
from tests import masked_after_ref, rank_ref

CALLS = []


def make_local_masked_after_keys(oracle, x_shard):
    def local_masked_after_keys(q, k, local_masks, mask_of, after_keys, base):
        CALLS.append((int(k), int(local_masks.shape[0]), int(local_masks.shape[1]), after_keys is not None, int(base)))
        masks = unpack_mask(local_masks.numpy(), len(x_shard))
        S = rank_ref.canon_scores(oracle, x_shard, q.numpy())
        keys = masked_after_ref.from_keys(S, masks, None if mask_of is None else mask_of.numpy(),
                                          None if after_keys is None else after_keys.numpy(), int(base), int(k))
        return torch.from_numpy(keys.view("int64"))
    return local_masked_after_keys
