"""One rank of the gloo test of ShardedSearcher.search_among (CPU, test doubles; in the style of tests/_gloo_worker_excluding.py)."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from haconvdr_amd.sharded import ShardedSearcher, shard_range  # noqa: E402
from oracle import oracle  # noqa: E402
from tests import among_ref, doubles, doubles_among  # noqa: E402
from tests.golden import cases  # noqa: E402


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    n, nq, k, m = 1501, 7, 20, 64                              # 7 queries: the ranks do not divide them
    x, q, ids = cases.search_case_inputs("dup", 9292, n, nq)   # row r and row r + 750 are twins: every tie crosses the shard boundary
    lo, hi = shard_range(n, rank, world)
    cut = shard_range(n, 1, world)[0]
    s = ShardedSearcher(None, shard_base=lo, id_map=ids, n_local=hi - lo, merge=doubles.merge, to_results=doubles.to_results,
                        local_among_keys=doubles_among.make_local_among_keys(oracle, x[lo:hi]))
    # global positions, the same on every rank: the top-24 of the whole corpus (twin pairs, one row on each shard), 30 rows
    # spread over both shards, repeats, padding in the middle and positions nobody holds
    top = oracle.flat_ip_search(x, q, 24)[1]
    spread = (np.arange(30)[None, :] * 47 + np.arange(nq)[:, None] * 13) % n
    cand = np.concatenate([top, spread, top[:, :6], np.full((nq, 2), -1), np.full((nq, 1), n), np.full((nq, 1), -5)], 1).astype(np.int64)
    assert cand.shape == (nq, m)
    cand = cand[:, np.argsort(np.arange(m) * 29 % m)]          # shuffled: padding and repeats anywhere
    ok = all((cand[i][cand[i] >= 0] < cut).any() and ((cand[i] >= cut) & (cand[i] < n)).any() for i in range(nq))
    wD, wI = among_ref.among(oracle, x, q, cand, k)            # the reference over the whole corpus
    ok = ok and any(wD[i, j] == wD[i, j + 1] and wI[i, j] < cut <= wI[i, j + 1] for i in range(nq) for j in range(k - 1))
    D, I = s.search_among(torch.from_numpy(q), k, torch.from_numpy(cand))
    ok = ok and np.array_equal(I, ids[wI]) and np.array_equal(among_ref.bits(D), among_ref.bits(wD))
    ok = ok and doubles_among.CALLS == [(k, m, lo)]            # one local call, at k, positions based at the shard
    # k beyond the candidates: the tail is padding
    D2, I2 = s.search_among(torch.from_numpy(q), 80, torch.from_numpy(cand))
    wD2, wI2 = among_ref.among(oracle, x, q, cand, 80)
    ok = ok and (wI2[:, -1] == -1).all() and np.array_equal(I2, np.where(wI2 >= 0, ids[np.clip(wI2, 0, None)], -1))
    ok = ok and np.array_equal(among_ref.bits(D2), among_ref.bits(wD2))
    keys = s.search_among_keys(torch.from_numpy(q), k, torch.from_numpy(cand))
    ok = ok and tuple(keys.shape) == (nq, k) and np.array_equal(doubles.to_results(keys, ids)[1], I)
    for bad in (torch.from_numpy(cand[:-1]), torch.from_numpy(cand[0]), torch.from_numpy(cand.astype(np.int32))):
        try:
            s.search_among(torch.from_numpy(q), k, bad)
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
