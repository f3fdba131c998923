"""One rank of the gloo test of ShardedSearcher.rank (CPU, test doubles; in the style of tests/_gloo_worker_excluding.py)."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from haconvdr_amd.sharded import ShardedSearcher, shard_range  # noqa: E402
from oracle import oracle  # noqa: E402
from tests import doubles_rank, rank_ref  # noqa: E402
from tests.golden import cases  # noqa: E402


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    n, nq = 1501, 7                                            # 7 queries: the ranks do not divide them
    x, q, _ = cases.search_case_inputs("dup", 9292, n, nq)     # duplicated rows: score ties between rows of different shards
    per = shard_range(n, 0, world)[1]
    x[per - 1] = x[per] = x[per + 1] = x[3]                    # one tie group across the first shard boundary for certain
    nan_row = per + 5
    x[nan_row, 0] = np.nan                                     # a row whose score is NaN for every query: never ranked, never counted
    lo, hi = shard_range(n, rank, world)
    s = ShardedSearcher(None, shard_base=lo, n_local=hi - lo, local_scores=doubles_rank.make_local_scores(oracle, x[lo:hi]),
                        count_ahead=doubles_rank.make_count_ahead(oracle, x[lo:hi]))
    ids = np.tile(np.arange(0, n, 13, dtype=np.int64), (nq, 1))          # rows of every shard, the same on every rank
    ids[:, 0:6] = [3, per - 1, per, per + 1, nan_row, n - 1]
    ids[1, 7], ids[2, 8], ids[3, 9] = -1, -5, n + 3                      # padding, and a position no rank holds
    want = rank_ref.rank_ids(oracle, x, q, ids)
    ok = (want[:, 4] == -1).all() and want[1, 7] == want[2, 8] == want[3, 9] == -1 and (want >= 0).sum() == want.size - nq - 3
    ok = ok and (want[:, 1] == want[:, 0] + 1).all() and (want[:, 3] == want[:, 0] + 3).all()      # the tie group, in row order
    got = s.rank(torch.from_numpy(q), torch.from_numpy(ids))
    ok = ok and got.dtype == torch.int64 and np.array_equal(got.numpy(), want)
    ok = ok and doubles_rank.CALLS == [("scores", ids.shape), ("counts", ids.shape)]
    everyone = [torch.empty_like(got) for _ in range(world)]             # every rank holds the same array
    dist.all_gather(everyone, got)
    ok = ok and all(torch.equal(t, got) for t in everyone)
    assert tuple(s.rank(torch.from_numpy(q), torch.zeros((nq, 0), dtype=torch.int64)).shape) == (nq, 0)
    try:
        s.rank(torch.from_numpy(q), torch.from_numpy(ids[:-1]))
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
