"""One rank of the gloo test of ShardedSearcher.search_masked (CPU, test doubles; in the style of tests/_gloo_worker_among.py)."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from haconvdr_amd.index import pack_mask  # noqa: E402
from haconvdr_amd.sharded import ShardedSearcher, shard_range  # noqa: E402
from oracle import oracle  # noqa: E402
from tests import doubles, doubles_masked, masked_ref  # noqa: E402
from tests.golden import cases  # noqa: E402


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    n, nq, k = 1501, 7, 20                                     # 7 queries: the ranks do not divide them
    x, q, ids = cases.search_case_inputs("dup", 9393, n, nq)   # row r and row r + 750 are twins: every tie crosses the shard boundary
    lo, hi = shard_range(n, rank, world)
    cut = shard_range(n, 1, world)[0]
    s = ShardedSearcher(None, shard_base=lo, id_map=ids, n_local=hi - lo, merge=doubles.merge, to_results=doubles.to_results,
                        local_masked_keys=doubles_masked.make_local_masked_keys(oracle, x[lo:hi]))
    # three masks over the WHOLE corpus, the same on every rank; each rank packs its own rows' slice.  Mask 0 keeps both twins of
    # two thirds of the pairs (ties across the cut), mask 1 only rows around the cut, mask 2 a handful of rows (k beyond them)
    r = np.arange(n)
    masks = np.stack([(r % 750) % 3 != 1, (r >= cut - 40) & (r < cut + 25), np.isin(r, [3, cut - 1, cut, n - 1])])
    mask_of = (np.arange(nq) % 3).astype(np.int64)
    local = torch.from_numpy(pack_mask(masks[:, lo:hi]))
    ok = tuple(local.shape) == (3, (hi - lo + 63) // 64)
    wD, wI = masked_ref.masked(oracle, x, q, masks, mask_of, k)            # the reference over the whole corpus
    ok = ok and any(wD[i, j] == wD[i, j + 1] and wI[i, j] < cut <= wI[i, j + 1] for i in range(nq) for j in range(k - 1))
    ok = ok and (wI[2, 4:] == -1).all() and (wI[2, :4] >= 0).all()
    D, I = s.search_masked(torch.from_numpy(q), k, local, torch.from_numpy(mask_of))
    ok = ok and np.array_equal(I, np.where(wI >= 0, ids[np.clip(wI, 0, None)], -1)) and np.array_equal(masked_ref.bits(D), masked_ref.bits(wD))
    ok = ok and doubles_masked.CALLS == [(k, 3, (hi - lo + 63) // 64, lo)]   # one local call, at k, positions based at the shard
    # one mask for every query, mask_of None
    D1, I1 = s.search_masked(torch.from_numpy(q), k, local[:1])
    wD1, wI1 = masked_ref.masked(oracle, x, q, masks[:1], None, k)
    ok = ok and np.array_equal(I1, ids[wI1]) and np.array_equal(masked_ref.bits(D1), masked_ref.bits(wD1))
    keys = s.search_masked_keys(torch.from_numpy(q), k, local, torch.from_numpy(mask_of))
    ok = ok and tuple(keys.shape) == (nq, k) and np.array_equal(doubles.to_results(keys, ids)[1], I)
    for bad_masks, bad_of in ((local[0], None), (local.to(torch.int32), None), (local[:2], None), (local, torch.from_numpy(mask_of[:-1])),
                              (local, torch.from_numpy(mask_of.astype(np.int32)))):
        try:
            s.search_masked(torch.from_numpy(q), k, bad_masks, bad_of)
            ok = False
        except ValueError:
            pass
    flag = torch.tensor([1 if ok else 0])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    dist.destroy_process_group()
    print(f"rank {rank}: {'OK' if ok else 'MISMATCH'} shard=[{lo},{hi})", flush=True)
    sys.exit(0 if int(flag) == 1 else 1)


if __name__ == "__main__":
    main()
