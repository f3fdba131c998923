"""One rank of the gloo tests of ShardedSearcher.search_masked_after.  argv[1]: "double" -- CPU, test doubles -- or "hip": every
rank builds its shard on the HIP index of device 0 (the ranks share the GPU, the collective runs over gloo) and searches through
the HIP defaults.  In the style of tests/_gloo_worker_after.py."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from haconvdr_amd.index import cursor_keys, pack_mask  # noqa: E402
from haconvdr_amd.sharded import ShardedSearcher, shard_range  # noqa: E402
from oracle import oracle  # noqa: E402
from tests import after_cases, masked_after_ref, rank_ref  # noqa: E402


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
    # three masks over the WHOLE corpus, the same on every rank; each rank packs its own rows' slice: two rows of three, a
    # band around the first cut, and a handful of rows (k beyond them)
    r = np.arange(n)
    cut = shard_range(n, 1, world)[0]
    masks = np.stack([r % 3 != 1, (r >= cut - 90) & (r < cut + 70), np.isin(r, [3, cut - 1, cut, n - 1])])
    mask_of = (np.arange(nq) % 3).astype(np.int64)
    local = torch.from_numpy(pack_mask(masks[:, lo:hi])).to(dev)
    mo = torch.from_numpy(mask_of).to(dev)
    if hip:
        from haconvdr_amd.index import FlatIPIndex
        idx = FlatIPIndex(after_cases.TIE_D, devices=(0,))
        idx.set_option("split", "0")
        idx.add(x[lo:lo + 100])                                # two segments per shard
        idx.add(x[lo + 100:hi])
        s = ShardedSearcher(idx, shard_base=lo, id_map=torch.from_numpy(ids).to(dev))
        calls = None
    else:
        from tests import doubles, doubles_masked_after
        s = ShardedSearcher(None, shard_base=lo, id_map=ids, n_local=hi - lo, merge=doubles.merge, to_results=doubles.to_results,
                            local_masked_after_keys=doubles_masked_after.make_local_masked_after_keys(oracle, x[lo:hi]))
        calls = doubles_masked_after.CALLS

    def host(t):
        return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)

    S = rank_ref.canon_scores(oracle, x, q)
    whole = masked_after_ref.unbounded(S, masks, mask_of)
    qt = torch.from_numpy(q).to(dev)
    ok = tuple(local.shape) == (3, (hi - lo + 63) // 64)
    # pages chained through the merged keys' last column: the unbounded masked list over the whole corpus, in external ids
    cursor, got_D, got_I = None, [], []
    for page in range(4):
        keys = s.search_masked_after_keys(qt, k, local, mo, cursor)
        want = masked_after_ref.from_keys(S, masks, mask_of, None if cursor is None else host(cursor), 0, k)
        ok = ok and tuple(keys.shape) == (nq, k) and np.array_equal(host(keys).view(np.uint64), want)
        D, I = s.search_masked_after(qt, k, local, mo, cursor)
        got_D.append(host(D))
        got_I.append(host(I))
        cursor = keys[:, -1].contiguous()
    if hip:
        torch.cuda.synchronize()
    got_D, got_I = np.concatenate(got_D, 1), np.concatenate(got_I, 1)
    for i in range(nq):
        sc, rows = whole[i]
        m = min(4 * k, len(rows))
        ok = ok and np.array_equal(got_I[i, :m], ids[rows[:m]]) and np.array_equal(masked_after_ref.bits(got_D[i, :m]), masked_after_ref.bits(sc[:m]))
        ok = ok and (got_I[i, m:] == -1).all()
    # the lists of mask 0 and 1 go on past four pages with page boundaries inside runs of equal scores; mask 2's ends on page one
    ok = ok and all(len(whole[i][1]) > 4 * k and all(whole[i][0][p * k - 1] == whole[i][0][p * k] for p in (1, 2, 3)) for i in (0, 3))
    ok = ok and len(whole[1][1]) == 160 and len(whole[2][1]) == 4
    if calls is not None:
        W = (hi - lo + 63) // 64
        ok = ok and calls == [(k, 3, W, page > 0, lo) for page in range(4) for _ in range(2)]   # one local call per search, at k, based at the shard
    # a (score, row) cursor packed by cursor_keys: global rows the masks leave out, the same on every rank; an exhausted one next to it
    full = [masked_after_ref.after_ref._ordered(S[i]) for i in range(nq)]
    rw = np.array([next(int(r) for r in full[i][50:] if not masks[mask_of[i], r]) for i in range(nq)], np.int64)
    sc = S[np.arange(nq), rw].astype(np.float32)
    rw[1] = -1
    ck = cursor_keys(sc, rw)
    D, I = s.search_masked_after(qt, k, local, mo, torch.from_numpy(ck).to(dev))
    wD, wI = masked_after_ref.from_scores(S, masks, mask_of, sc, rw, k)
    ok = ok and (wI[1] == -1).all() and (wI[0] >= 0).all() and np.array_equal(host(I), np.where(wI >= 0, ids[np.clip(wI, 0, None)], -1))
    ok = ok and np.array_equal(masked_after_ref.bits(host(D)), masked_after_ref.bits(wD))
    # one mask for every query, no mask_of, no cursor: search_masked
    D1, I1 = s.search_masked_after(qt, k, local[:1].contiguous())
    wD1, wI1 = masked_after_ref.from_scores(S, masks[:1], None, None, None, k)
    ok = ok and np.array_equal(host(I1), ids[wI1]) and np.array_equal(masked_after_ref.bits(host(D1)), masked_after_ref.bits(wD1))
    for bad_masks, bad_of, bad_cur in ((local[0], None, None), (local.to(torch.int32), mo, None), (local[:2], None, None), (local, mo[:-1], None),
                                       (local, mo, torch.zeros((nq, 1), dtype=torch.int64, device=dev)),
                                       (local, mo, torch.zeros(nq - 1, dtype=torch.int64, device=dev)),
                                       (local, mo, torch.zeros(nq, dtype=torch.int32, device=dev))):
        try:
            s.search_masked_after(qt, k, bad_masks, bad_of, bad_cur)
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
