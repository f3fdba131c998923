"""Corpus sharding across GPUs — one process per GPU, torch.distributed over RCCL/xGMI.

SURVEY.md §8(e): rows are independent, so the corpus is partitioned by contiguous
global-offset range (what faiss ``shard=True`` does inside one process,
src/test_HAConvDR_topiocqa.py:55-66).  Every rank computes an exact local top-k whose
keys already carry GLOBAL positions, then ONE all-gather of the packed keys
([nq, k] uint64 = 8 B per entry; 0.8 MB per rank at nq=1000, k=100) is followed by a
deterministic R-way merge on every rank.  Key order (score desc, global position asc)
equals the reference's sequential ``>=`` block merge (:138) when shards are in block
order.  No other collective touches the data path.
"""
import torch
import torch.distributed as dist


def shard_range(n_total, rank, world_size):
    """Rows [lo, hi) of rank: contiguous ceil(N/R)-sized ranges."""
    per = (n_total + world_size - 1) // world_size
    lo = min(n_total, rank * per)
    return lo, min(n_total, lo + per)


# The two checks below see host tensors too (the hooks' test doubles run on CPU), so they ask for dtype and shape only.
def _check_local_masks(local_masks, mask_of, q):
    if local_masks.dim() != 2 or local_masks.dtype != torch.int64:
        raise ValueError(f"local_masks must be packed int64 [n_masks, W], got {local_masks.dtype} {tuple(local_masks.shape)}")
    if mask_of is not None and (mask_of.dim() != 1 or mask_of.shape[0] != q.shape[0] or mask_of.dtype != torch.int64):
        raise ValueError(f"mask_of must be int64 [nq] with nq = {q.shape[0]}, got {mask_of.dtype} {tuple(mask_of.shape)}")
    if mask_of is None and local_masks.shape[0] not in (1, q.shape[0]):
        raise ValueError(f"{local_masks.shape[0]} masks for {q.shape[0]} queries and no mask_of: needs one mask, one per query, or mask_of")


def _check_after_keys(after_keys, q):
    if after_keys is not None:
        if after_keys.dim() != 1 or after_keys.shape[0] != q.shape[0]:
            raise ValueError(f"after_keys must be [nq] with nq = {q.shape[0]}, got shape {tuple(after_keys.shape)}")
        if after_keys.dtype != torch.int64:
            raise ValueError(f"after_keys must be int64 (the view of the packed keys), got {after_keys.dtype}")


class ShardedSearcher:
    """search(q, k) over a corpus sharded across the ranks of ``group``.

    local_keys(q, k, pos_base) -> int64(uint64 bits) tensor [nq, k]   (default: the HIP index)
    merge(lists [R, nq, k])    -> [nq, k]                              (default: HIP merge kernel)
    to_results(keys, id_map)   -> (D, I)                               (default: HIP kernel)
    filter(keys [nq, k + e], exclude [nq, e], k) -> [nq, k]            (default: HIP filter kernel)
    local_scores(q, local_ids [nq, m]) -> float32 [nq, m]              (default: index.score_ids_tensor)
    count_ahead(q, ref_scores, ref_bounds [nq, m]) -> int64 [nq, m]    (default: index.count_ahead_tensor)
    local_among_keys(q, k, local_cand [nq, m], pos_base) -> [nq, k]    (default: index.search_among_keys_tensor)
    local_masked_keys(q, k, local_masks [n_masks, W], mask_of, pos_base) -> [nq, k]   (default: index.search_masked_keys_tensor)
    local_after_keys(q, k, after_keys [nq] or None, pos_base) -> [nq, k]   (default: index.search_after_keys_tensor)
    local_masked_after_keys(q, k, local_masks, mask_of, after_keys [nq] or None, pos_base) -> [nq, k]
                                                           (default: index.search_masked_keys_tensor(after_keys=))
    The ten hooks exist so that the distributed plumbing can be exercised on CPU with
    gloo and a test double; the product path always uses the HIP defaults.
    n_local: rows this rank holds (default: index.ntotal when rank() / search_among() is called).

    exclude (optional, int64 [nq, e], on the keys' device): per query, GLOBAL positions (shard_base + local row) that must
    not be returned, identical on every rank; < 0 is padding.  Every rank then searches k + e, the all-gather and the merge
    run at k + e, and the merged lists are filtered down to k: the top-k of (corpus minus E) lies inside the top-(k + |E|)
    of the corpus, in the same order.  exclude=None is the path above, unchanged; the filter hook is not called.
    """

    def __init__(self, index, shard_base, group=None, id_map=None, local_keys=None, merge=None, to_results=None, filter=None,
                 local_scores=None, count_ahead=None, n_local=None, local_among_keys=None, local_masked_keys=None,
                 local_after_keys=None, local_masked_after_keys=None):
        from . import index as _index
        self.index = index
        self.shard_base = int(shard_base)
        self.group = group
        self.id_map = id_map
        self._local_keys = local_keys or (lambda q, k, base: index.search_keys_tensor(q, k, pos_base=base))
        self._merge = merge or _index.merge_keys
        self._to_results = to_results or _index.keys_to_results
        self._filter = filter or _index.filter_keys
        self._local_scores = local_scores or (lambda q, ids: index.score_ids_tensor(q, ids))
        self._count_ahead = count_ahead or (lambda q, s, b: index.count_ahead_tensor(q, s, b))
        self._n_local = n_local
        self._local_among_keys = local_among_keys or (lambda q, k, cand, base: index.search_among_keys_tensor(q, k, cand, pos_base=base))
        self._local_masked_keys = local_masked_keys or (lambda q, k, masks, mask_of, base: index.search_masked_keys_tensor(q, k, masks, mask_of, pos_base=base))
        self._local_after_keys = local_after_keys or (lambda q, k, after_keys, base: index.search_after_keys_tensor(q, k, after_keys, pos_base=base))
        self._local_masked_after_keys = local_masked_after_keys or (
            lambda q, k, masks, mask_of, after_keys, base: index.search_masked_keys_tensor(q, k, masks, mask_of, pos_base=base, after_keys=after_keys))

    def _gather_and_merge(self, keys):
        if not dist.is_initialized():
            return keys                                   # a single process holding the whole corpus
        world = dist.get_world_size(self.group)
        nq, k = keys.shape
        gathered = torch.empty((world * nq, k), dtype=keys.dtype, device=keys.device)   # rank-major slabs
        dist.all_gather_into_tensor(gathered, keys.contiguous(), group=self.group)
        return self._merge(gathered.view(world, nq, k))

    def search_keys(self, q, k, exclude=None):
        if exclude is not None:
            if exclude.dim() != 2 or exclude.shape[0] != q.shape[0]:
                raise ValueError(f"exclude must be [nq, e] with nq = {q.shape[0]}, got shape {tuple(exclude.shape)}")
            return self._filter(self.search_keys(q, k + exclude.shape[1]), exclude, k)
        return self._gather_and_merge(self._local_keys(q, k, self.shard_base))

    def search(self, q, k, exclude=None):
        return self._to_results(self.search_keys(q, k, exclude), self.id_map)

    def search_among_keys(self, q, k, cand):
        """The merged keys [nq, k] of search_among."""
        if cand.dim() != 2 or cand.shape[0] != q.shape[0]:
            raise ValueError(f"cand must be [nq, m] with nq = {q.shape[0]}, got shape {tuple(cand.shape)}")
        if cand.dtype != torch.int64:
            raise ValueError(f"cand must be int64, got {cand.dtype}")
        n_local = int(self.index.ntotal if self._n_local is None else self._n_local)
        local = cand - self.shard_base
        mine = (cand >= 0) & (local >= 0) & (local < n_local)
        local = torch.where(mine, local, torch.full_like(local, -1)).contiguous()
        return self._gather_and_merge(self._local_among_keys(q, k, local, self.shard_base))

    def search_among(self, q, k, cand):
        """Exact top-k over each query's candidate rows, over the whole sharded corpus: cand int64 [nq, m] GLOBAL positions
        (shard_base + local row), identical on every rank, a set, < 0 is padding -> (D, I) like search().  Every rank selects among
        the candidates it holds (positions it does not hold become -1, the rest cand - shard_base; a row lives on one rank, so no
        repeat crosses ranks), then the same one all-gather and merge as search_keys, at k."""
        return self._to_results(self.search_among_keys(q, k, cand), self.id_map)

    def search_masked_keys(self, q, k, local_masks, mask_of=None):
        """The merged keys [nq, k] of search_masked."""
        _check_local_masks(local_masks, mask_of, q)
        return self._gather_and_merge(self._local_masked_keys(q, k, local_masks, mask_of, self.shard_base))

    def search_masked(self, q, k, local_masks, mask_of=None):
        """Exact top-k over the rows a bitmap selects, over the whole sharded corpus -> (D, I) like search().  local_masks: packed
        int64 [n_masks, W_local] (index.pack_mask) over THIS RANK'S OWN rows -- bit r is local row r, global position shard_base
        + r --, the same number of masks on every rank; mask_of int64 [nq] (or None: one mask, or one per query) is identical on
        every rank.  Every rank searches its rows under its masks, then the same one all-gather and merge as search_keys, at k."""
        return self._to_results(self.search_masked_keys(q, k, local_masks, mask_of), self.id_map)

    def search_after_keys(self, q, k, after_keys=None):
        """The merged keys [nq, k] of search_after; their last column is the cursor of the next page."""
        _check_after_keys(after_keys, q)
        return self._gather_and_merge(self._local_after_keys(q, k, after_keys, self.shard_base))

    def search_after(self, q, k, after_keys=None):
        """The next page over the whole sharded corpus -> (D, I) like search(): per query the k best rows whose key lies below
        after_keys [nq] (int64 view of the packed keys, GLOBAL positions, identical on every rank: index.cursor_keys, or the last
        column of search_keys / search_after_keys; 0 = an exhausted list, -1 = the start, None = every query from the start).
        Nothing is translated: a key carries a global position, and every rank searches with pos_base = shard_base, so the same
        comparison holds on every rank.  Then the same one all-gather and merge as search_keys, at k."""
        return self._to_results(self.search_after_keys(q, k, after_keys), self.id_map)

    def search_masked_after_keys(self, q, k, local_masks, mask_of=None, after_keys=None):
        """The merged keys [nq, k] of search_masked_after; their last column is the cursor of the next page."""
        _check_local_masks(local_masks, mask_of, q)
        _check_after_keys(after_keys, q)
        return self._gather_and_merge(self._local_masked_after_keys(q, k, local_masks, mask_of, after_keys, self.shard_base))

    def search_masked_after(self, q, k, local_masks, mask_of=None, after_keys=None):
        """The next page of the rows a bitmap selects, over the whole sharded corpus -> (D, I) like search().  local_masks and
        mask_of as in search_masked (THIS RANK'S OWN rows, the same number of masks on every rank); after_keys as in search_after
        (int64 [nq], GLOBAL positions, identical on every rank; 0 = an exhausted list, -1 = the start, None = every query from
        the start).  Nothing is translated: every rank searches its rows under its masks with pos_base = shard_base, so the same
        key comparison holds on every rank.  Then the same one all-gather and merge as search_keys, at k."""
        return self._to_results(self.search_masked_after_keys(q, k, local_masks, mask_of, after_keys), self.id_map)

    def rank(self, q, ids):
        """Exact rank of named rows over the whole sharded corpus: ids int64 [nq, m] GLOBAL positions (shard_base + local row),
        identical on every rank, < 0 is padding -> int64 [nq, m] on every rank, the 0-based position the row takes in an unbounded
        search of q[i]; -1 for padding, a position no rank holds, and a row whose score is NaN.

        The rank that holds a row scores it (every other rank contributes -inf) and one all_reduce(MAX) hands the score to
        everyone; next to it travels a flag word (1 = somebody holds the row, 3 = and its score is NaN: a NaN does not survive a
        MAX reliably, so it goes through as a flag and the score as -inf).  Every rank then counts its own rows ahead of (score,
        clamp(id - shard_base, 0, n_local)) -- a shard's local order is the global order, so score ties still break by global
        position -- and one all_reduce(SUM) adds the counts.  Two collectives of [nq, m] words, no rows moved."""
        if ids.dim() != 2 or ids.shape[0] != q.shape[0]:
            raise ValueError(f"ids must be [nq, m] with nq = {q.shape[0]}, got shape {tuple(ids.shape)}")
        if ids.dtype != torch.int64:
            raise ValueError(f"ids must be int64, got {ids.dtype}")
        n_local = int(self.index.ntotal if self._n_local is None else self._n_local)
        local = ids - self.shard_base
        mine = (ids >= 0) & (local >= 0) & (local < n_local)
        neg_inf = float("-inf")
        if ids.numel() == 0:
            return torch.empty_like(ids)
        s = self._local_scores(q, torch.where(mine, local, torch.full_like(local, -1)))
        nan = mine & torch.isnan(s)
        score = torch.where(mine & ~nan, s, torch.full_like(s, neg_inf))
        flags = mine.to(torch.int32) + 2 * nan.to(torch.int32)
        distributed = dist.is_initialized()
        if distributed:
            dist.all_reduce(score, op=dist.ReduceOp.MAX, group=self.group)
            dist.all_reduce(flags, op=dist.ReduceOp.MAX, group=self.group)      # (at most one rank holds a row: MAX is that rank's word)
        ranked = flags == 1
        score = torch.where(flags == 3, torch.full_like(score, float("nan")), score)
        counts = self._count_ahead(q, score.contiguous(), local.clamp(0, n_local).contiguous())
        counts = torch.where(ranked, counts, torch.zeros_like(counts))
        if distributed:
            dist.all_reduce(counts, op=dist.ReduceOp.SUM, group=self.group)
        return torch.where(ranked, counts, torch.full_like(counts, -1))
