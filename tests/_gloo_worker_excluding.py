"""One rank of the gloo test of ShardedSearcher's exclude= (CPU, test doubles; in the style of tests/_gloo_worker.py)."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from haconvdr_amd.sharded import ShardedSearcher, shard_range  # noqa: E402
from oracle import oracle  # noqa: E402
from tests import doubles, doubles_filter, excluding  # noqa: E402
from tests.golden import cases  # noqa: E402


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    n, nq, k, e = 1501, 7, 20, 6                               # 7 queries: the ranks do not divide them
    x, q, ids = cases.search_case_inputs("dup", 9191, n, nq)   # duplicated rows straddle the shard boundary
    lo, hi = shard_range(n, rank, world)
    s = ShardedSearcher(None, shard_base=lo, id_map=ids, local_keys=doubles.make_local_keys(oracle, x[lo:hi]),
                        merge=doubles.merge, to_results=doubles.to_results, filter=doubles_filter.filter)
    # exclude=None: today's path, the hook is never called
    D0, I0 = s.search(torch.from_numpy(q), k)
    oD, oI = oracle.flat_ip_search(x, q, k)
    ok = np.array_equal(I0, ids[oI]) and np.array_equal(D0, oD) and doubles_filter.CALLS == []
    # global positions, the same on every rank: of each twin pair in the top-2e the first or the second row in turn, i.e. rows
    # of both shards, plus a hole and a duplicate
    top = oracle.flat_ip_search(x, q, 2 * e)[1]
    E = top[:, [0, 3, 4, 7, 8, 11]].copy()
    E[1, 2], E[2, 3] = -1, E[2, 0]
    ok = ok and any((E[i] < shard_range(n, 1, world)[0]).any() and (E[i] >= shard_range(n, 1, world)[0]).any() for i in range(nq))
    D, I = s.search(torch.from_numpy(q), k, exclude=torch.from_numpy(E))
    wD, wI = excluding.filtered_topk(oracle, x, q, k, E)       # the unsharded expectation ...
    bD, bI = excluding.deleted_topk(oracle, x, q, k, E)        # ... which is the top-k of the corpus without those rows
    ok = ok and np.array_equal(wI, bI) and np.array_equal(wD, bD)
    ok = ok and np.array_equal(I, ids[wI]) and np.array_equal(D, wD) and not np.array_equal(I, I0)
    ok = ok and doubles_filter.CALLS == [(k + e, e, k)]        # searched, gathered and merged at k + e, filtered once
    keys = s.search_keys(torch.from_numpy(q), k, exclude=torch.from_numpy(E))
    ok = ok and tuple(keys.shape) == (nq, k) and np.array_equal(doubles.to_results(keys, ids)[1], I)
    try:
        s.search(torch.from_numpy(q), k, exclude=torch.from_numpy(E[:-1]))
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
