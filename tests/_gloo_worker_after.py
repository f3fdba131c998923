"""One rank of the gloo tests of ShardedSearcher.search_after.  argv[1]: "double" -- CPU, test doubles (in the style of
tests/_gloo_worker_masked.py) -- or "hip": every rank builds its shard on the HIP index of device 0 (the ranks share the GPU,
the collective runs over gloo, as in tests/_sharded_gpu_rank.py) and searches through the HIP defaults."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from haconvdr_amd.index import cursor_keys  # noqa: E402
from haconvdr_amd.sharded import ShardedSearcher, shard_range  # noqa: E402
from oracle import oracle  # noqa: E402
from tests import after_cases, after_ref, rank_ref  # noqa: E402


def main():
    hip = sys.argv[1] == "hip"
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    if hip:
        torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    x, q = after_cases.tie_case()                              # every score is shared by dozens of rows on every shard
    n, nq, k = len(x), len(q), 37
    ids = (np.arange(n, dtype=np.int64) * 3 + 5)
    lo, hi = shard_range(n, rank, world)
    dev = "cuda" if hip else "cpu"
    if hip:
        from haconvdr_amd.index import FlatIPIndex
        idx = FlatIPIndex(after_cases.TIE_D, devices=(0,))
        idx.set_option("split", "0")
        idx.add(x[lo:lo + 100])                                # two segments per shard
        idx.add(x[lo + 100:hi])
        s = ShardedSearcher(idx, shard_base=lo, id_map=torch.from_numpy(ids).to(dev))
        calls = None
    else:
        from tests import doubles, doubles_after
        s = ShardedSearcher(None, shard_base=lo, id_map=ids, n_local=hi - lo, merge=doubles.merge, to_results=doubles.to_results,
                            local_after_keys=doubles_after.make_local_after_keys(oracle, x[lo:hi]))
        calls = doubles_after.CALLS

    def host(t):
        return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)

    S = rank_ref.canon_scores(oracle, x, q)
    whole = after_ref.unbounded(S)
    qt = torch.from_numpy(q).to(dev)
    ok = True
    # pages chained through the merged keys' last column: the unbounded search over the whole corpus, in external ids
    cursor, got_D, got_I = None, [], []
    for page in range(4):
        keys = s.search_after_keys(qt, k, cursor)
        want = after_ref.after_from_keys(S, None if cursor is None else host(cursor), 0, k)
        ok = ok and tuple(keys.shape) == (nq, k) and np.array_equal(host(keys).view(np.uint64), want)
        D, I = s.search_after(qt, k, cursor)
        got_D.append(host(D))
        got_I.append(host(I))
        cursor = keys[:, -1].contiguous()
    if hip:
        torch.cuda.synchronize()
    got_D, got_I = np.concatenate(got_D, 1), np.concatenate(got_I, 1)
    for i in range(nq):
        sc, rows = whole[i]
        ok = ok and np.array_equal(got_I[i], ids[rows[:4 * k]]) and np.array_equal(after_ref.bits(got_D[i]), after_ref.bits(sc[:4 * k]))
    # every page boundary fell inside a run of equal scores that both sides of a shard cut hold
    ok = ok and all(whole[i][0][p * k - 1] == whole[i][0][p * k] for i in range(nq) for p in (1, 2, 3))
    if calls is not None:
        ok = ok and calls == [(k, page > 0, lo) for page in range(4) for _ in range(2)]     # one local call per search, at k, based at the shard
    # a (score, row) cursor packed by cursor_keys: global rows, the same on every rank; an exhausted one next to it
    j = 3 * k + 11
    sc = np.array([whole[i][0][j] for i in range(nq)], np.float32)
    rw = np.array([whole[i][1][j] for i in range(nq)], np.int64)
    rw[1] = -1
    ck = cursor_keys(sc, rw)
    D, I = s.search_after(qt, k, torch.from_numpy(ck).to(dev))
    wD, wI = after_ref.after_from_scores(S, sc, rw, k)
    ok = ok and (wI[1] == -1).all() and np.array_equal(host(I), np.where(wI >= 0, ids[np.clip(wI, 0, None)], -1))
    ok = ok and np.array_equal(after_ref.bits(host(D)), after_ref.bits(wD))
    for bad in (torch.zeros((nq, 1), dtype=torch.int64, device=dev), torch.zeros(nq - 1, dtype=torch.int64, device=dev),
                torch.zeros(nq, dtype=torch.int32, device=dev)):
        try:
            s.search_after(qt, k, bad)
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
