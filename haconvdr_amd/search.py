"""Block-wise retrieval: host-side mirror of ``search_one_by_one_with_faiss``
(src/test_HAConvDR_topiocqa.py:74-162 = src/test_HAConvDR_qrecc.py:74-162).

Same arguments, same file formats, same result contract (float64 scores, int64
passage ids, global top-``topN`` in the first ``topN`` columns, earlier block wins
score ties), but the per-block python merge (:111-149) is replaced by keeping every
block resident in HBM and running ONE exact top-k over all of them, with the
``passage_embedding2id[I]`` remap (:110) fused into the result kernel.

Shape of the result.  The reference's merge loop appends BOTH lists' leftovers (:144-149), so with two or more
blocks it returns ``(nq, 2*topN)``: the global top-``topN`` followed by what is left of {top-``topN`` of blocks
0..B-2, top-``topN`` of block B-1} in merge order; its consumers slice ``[:topN]`` (:238-239).  By default this
module returns the ``(nq, topN)`` that is read; ``reference_shape=True`` returns the reference's literal matrix
(every column equal to the reference's, tested against the goldens' full ``ref_D`` / ``ref_I``) at the price of
a second search (the last block on its own).
"""
import logging
import os

import numpy as np

logger = logging.getLogger(__name__)


def _load_block(passage_embeddings_dir, block_id, mmap, readahead):
    from .passages import read_embedding_block
    emb, ids = read_embedding_block(passage_embeddings_dir, block_id, mmap=mmap)
    if readahead and isinstance(emb, np.memmap):
        # ask the kernel to start reading the payload now (asynchronous read-ahead into the page cache): by the time add()
        # walks these pages -- pageable -> pinned staging -> H2D, double-buffered inside hac_index_add -- they are resident
        try:
            import mmap as _mmap
            emb._mmap.madvise(_mmap.MADV_WILLNEED)
        except Exception:
            pass
    return emb, np.asarray(ids)


def iter_embedding_blocks(passage_embeddings_dir, passage_block_num, mmap=True, prefetch=True):
    """Yield (emb float32 [n,768], ids int64 [n]) for block 0,1,… ; stops at the first
    block that cannot be loaded, like the reference's bare ``except: break`` (:94-95).
    mmap=True maps the pickled ndarray payload in place (haconvdr_amd.passages) instead of copying
    the 7.7 GB block through ``pickle.load`` — the reference's dominant wall time at search.
    prefetch=True opens block b+1 on a background thread and starts its read-ahead while the caller still works on
    block b (its add(): the H2D of 7.7 GB; in the reference's own loop also its search, :98-122): disk and PCIe overlap."""
    if not prefetch or passage_block_num <= 1:
        for block_id in range(passage_block_num):
            try:
                yield _load_block(passage_embeddings_dir, block_id, mmap, False)
            except Exception:
                break
        return
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=1) as pool:
        nxt = pool.submit(_load_block, passage_embeddings_dir, 0, mmap, True)
        for block_id in range(passage_block_num):
            try:
                cur = nxt.result()
            except Exception:
                break
            if block_id + 1 < passage_block_num:
                nxt = pool.submit(_load_block, passage_embeddings_dir, block_id + 1, mmap, True)
            yield cur


def _with_last_flag(it):
    """(item, is_last) for every item of an iterator (one item of look-ahead)."""
    it = iter(it)
    try:
        cur = next(it)
    except StopIteration:
        return
    for nxt in it:
        yield cur, False
        cur = nxt
    yield cur, True


def _search_resident(index, q, dev, id_parts, sizes, last_ids, topN):
    """One exact top-topN over the blocks now resident in `index` (rows in block order), ids remapped on the device,
    the reference's padding of a degenerate corpus reproduced.  Resets the index (:122)."""
    import torch
    id_map = torch.from_numpy(np.concatenate(id_parts)).to(dev)
    if len(index.devices) == 1:
        D, I = index.search_tensor(torch.from_numpy(q).to(dev), topN, id_map=id_map)
        D, I = D.cpu().numpy(), I.cpu().numpy()
    else:
        D, I = index.search(q, topN)
        idm = id_map.cpu().numpy()
        I = np.where(I >= 0, idm[np.clip(I, 0, None)], -1)
    index.reset()                                         # :122
    D = D.astype(np.float64)                              # .tolist() widens to python float (:111)
    total = int(sum(sizes))
    if total < topN:
        # Degenerate corpus (< topN rows in all blocks together): the reference's padded
        # slots carry score -FLT_MAX and, through numpy's negative indexing at :110
        # (I == -1), the LAST id of their block; earlier blocks' pads sort first (:138).
        pads = []
        for n_b, lid in zip(sizes, last_ids):
            pads += [lid] * max(0, topN - n_b)
        I[:, total:] = np.asarray(pads[:topN - total], dtype=np.int64)[None, :]
    return D, I


def search_blocks(index, blocks, query_embeddings, topN, reference_shape=False):
    """Resident multi-block search.  blocks: iterable of (emb, ids) in block order.
    Returns (D float64 [nq, topN], I int64 [nq, topN]); with reference_shape=True and two or more blocks the
    reference's literal (nq, 2*topN) matrices (module docstring)."""
    import torch
    dev = torch.device("cuda", index.devices[0])
    q = np.ascontiguousarray(query_embeddings, dtype=np.float32)
    index.reset()
    id_parts, sizes, last_ids = [], [], []
    head = None                                           # reference_shape: result over blocks 0..B-2
    for (emb, ids), is_last in _with_last_flag(blocks):
        if reference_shape and is_last and id_parts:
            head = _search_resident(index, q, dev, id_parts, sizes, last_ids, topN)
            id_parts, sizes, last_ids = [], [], []
        index.add(emb)                                    # :98 (blocks stay resident; no reset between them)
        ids = np.asarray(ids, dtype=np.int64)
        id_parts.append(ids)
        sizes.append(len(ids))
        last_ids.append(int(ids[-1]) if len(ids) else -1)
    if not id_parts:
        raise ValueError("no passage block could be loaded")  # the reference fails too (None has no len, :152)
    D, I = _search_resident(index, q, dev, id_parts, sizes, last_ids, topN)
    if head is None:
        return D, I
    # :131-149 on (merged[:topN], cur[:topN]): a stable two-way merge, the running list first on equal scores (`>=`,
    # :138), BOTH leftovers appended.  Both lists are sorted descending (pads, -FLT_MAX, last), so the merge is a stable
    # sort of their concatenation by descending score.
    cD, cI = np.concatenate([head[0], D], 1), np.concatenate([head[1], I], 1)
    order = np.argsort(-cD, axis=1, kind="stable")
    return np.take_along_axis(cD, order, 1), np.take_along_axis(cI, order, 1)


def search_one_by_one(args, passage_embeddings_dir, index, query_embeddings, topN, reference_shape=False):
    """Drop-in for search_one_by_one_with_faiss(args, dir, index, Q, topN).  reference_shape=True: the reference's
    literal (nq, 2*topN) result when two or more blocks load (:144-162), see the module docstring."""
    blocks = iter_embedding_blocks(passage_embeddings_dir, args.passage_block_num)
    merged_D, merged_I = search_blocks(index, blocks, query_embeddings, topN, reference_shape=reference_shape)
    logger.info(merged_I.shape)
    return merged_D, merged_I


def rows_carrying(sorted_ids, order, exclude):
    """External ids int64 [nq, e] (-1 = padding) -> int64 [nq, w]: per query EVERY row that carries one of its ids (an id two
    blocks hold names two rows), in the order of the ids, padded with -1 to the widest list (w = 0 when no id is held).
    (sorted_ids, order): the row -> id array sorted ascending and the rows in that order.  An id no row carries adds nothing."""
    pid = np.asarray(exclude)
    if pid.dtype.kind not in "iu":
        raise ValueError(f"exclude: passage ids must be integers, got dtype {pid.dtype}")
    if pid.ndim != 2:
        raise ValueError(f"exclude must be [nq, e], got shape {pid.shape}")
    pid = pid.astype(np.int64)
    lo = np.searchsorted(sorted_ids, pid, side="left")
    cnt = np.where(pid == -1, 0, np.searchsorted(sorted_ids, pid, side="right") - lo)
    per_query = cnt.sum(axis=1)
    out = np.full((pid.shape[0], int(per_query.max()) if pid.shape[0] else 0), -1, np.int64)
    cnt, lo = cnt.reshape(-1), lo.reshape(-1)
    total = int(cnt.sum())
    if total:
        first = np.cumsum(cnt) - cnt                                          # of each (query, id) run, in the flat output
        within = np.arange(total) - np.repeat(first, cnt)
        query = np.repeat(np.repeat(np.arange(pid.shape[0]), pid.shape[1]), cnt)
        col = np.arange(total) - np.repeat(np.cumsum(per_query) - per_query, per_query)
        out[query, col] = order[np.repeat(lo, cnt) + within]
    return out


class ResidentCorpus:
    """All passage blocks of a directory resident in HBM, searched many times (the reference reloads
    every block for every evaluation run, :77-123).  Same result contract as search_one_by_one.
    ``sizes`` describes the blocks as they were loaded: remove() does not change it."""

    def __init__(self, passage_embeddings_dir, passage_block_num, index=None, device=0):
        import torch
        from .index import FlatIPIndex
        self.index = index if index is not None else FlatIPIndex(768, devices=(device,))
        self.index.reset()
        ids, self.sizes = [], []
        for emb, bid in iter_embedding_blocks(passage_embeddings_dir, passage_block_num):
            self.index.add(emb)
            ids.append(np.asarray(bid, dtype=np.int64))
            self.sizes.append(len(bid))
        if not ids:
            raise ValueError("no passage block could be loaded")
        self.dev = torch.device("cuda", self.index.devices[0])
        self._ids = np.concatenate(ids)                       # row -> external passage id
        self.id_map = torch.from_numpy(self._ids).to(self.dev)
        self._lookup = None

    @property
    def ntotal(self):
        return self.index.ntotal

    def _id_lookup(self):
        """(ids sorted ascending, their rows): built once, on the host, by the first call that needs it."""
        if self._lookup is None:
            order = np.argsort(self._ids, kind="stable")
            self._lookup = (self._ids[order], order.astype(np.int64))
        return self._lookup

    def rows_mask(self, passage_ids):
        """bool [ntotal], true at every row that carries one of the EXTERNAL passage ids (integers of any shape, -1 = padding;
        an id two blocks hold sets two rows, an id no block holds sets none): a mask for search(within=).  Nothing is cached: a
        mask describes the rows as they are now, and remove() renumbers them."""
        pid = np.asarray(passage_ids)
        if pid.dtype.kind not in "iu":
            raise ValueError(f"rows_mask: passage ids must be integers, got dtype {pid.dtype}")
        rows = rows_carrying(*self._id_lookup(), pid.reshape(1, -1))[0]
        mask = np.zeros(len(self._ids), np.bool_)
        mask[rows[rows >= 0]] = True
        return mask

    def first_rows_mask(self):
        """bool [ntotal], true at the first row of each external id: searching within it gives lists without repeated passage
        ids, filled to topN (the TREC writer de-duplicates per query afterwards and leaves filler at the tail)."""
        sorted_ids, order = self._id_lookup()   # (stable sort: equal ids keep row order)
        mask = np.zeros(len(self._ids), np.bool_)
        if len(sorted_ids):
            first = np.ones(len(sorted_ids), np.bool_)
            first[1:] = sorted_ids[1:] != sorted_ids[:-1]
            mask[order[first]] = True
        return mask

    def search(self, query_embeddings, topN, exclude=None, within=None, within_of=None):
        """query_embeddings: float32 [nq,768] (numpy or CUDA tensor) -> (D float64 [nq,topN], I int64 [nq,topN]).
        exclude: optional int64 [nq, e] EXTERNAL passage ids (-1 = padding) the query must not get back -- its gold passages
        when mining hard negatives, what a conversation has already shown; every row that carries such an id is left out, an
        id no block holds is ignored, and the list is still filled to topN (the search runs at topN + the widest row list).
        within: optional masks over the ROWS, bool [ntotal] or [n_masks, ntotal] (rows_mask, first_rows_mask, a topic's or a
        block's rows) or packed words (index.pack_mask): only selected rows are returned, however many or few they are
        (index.search_masked; faiss's IDSelectorBitmap); within_of int64 [nq] names each query's mask (None: one mask for all,
        or one per query).  exclude and within together raise ValueError: fold the exclusions into per-query masks
        (within & ~rows_mask(ids))."""
        import torch
        q = query_embeddings if isinstance(query_embeddings, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(query_embeddings, dtype=np.float32))
        if exclude is not None and within is not None:
            raise ValueError("search: exclude and within together are not supported: fold the exclusions into per-query masks")
        if within_of is not None and within is None:
            raise ValueError("search: within_of without within")
        if within is not None:
            from .index import _as_masks
            words, mask_of = _as_masks(within, within_of, q.shape[0], self.ntotal, "search(within=)")
            if mask_of is not None and mask_of.size and (mask_of.min() < 0 or mask_of.max() >= words.shape[0]):
                raise ValueError(f"search(within=): within_of names a mask outside [0, {words.shape[0]})")   # (the tensor form would answer with an empty list)
            D, I = self.index.search_masked_tensor(q.to(self.dev), topN, torch.from_numpy(words).to(self.dev),
                                                   None if mask_of is None else torch.from_numpy(mask_of).to(self.dev), id_map=self.id_map)
        elif exclude is None:
            D, I = self.index.search_tensor(q.to(self.dev), topN, id_map=self.id_map)
        else:
            rows = rows_carrying(*self._id_lookup(), exclude)
            D, I = self.index.search_excluding_tensor(q.to(self.dev), topN, torch.from_numpy(rows).to(self.dev), id_map=self.id_map)
        return D.cpu().numpy().astype(np.float64), I.cpu().numpy()

    def _passage_labels(self):
        """int64 CUDA [ntotal]: the rows' external passage ids relabelled densely (0 .. distinct ids - 1), the default groups of
        search_distinct.  Kept on the device for the rows as they are now: remove() replaces the id array and with it this."""
        import torch
        cached = getattr(self, "_labels", None)
        if cached is None or cached[0] is not self._ids:
            dense = np.unique(self._ids, return_inverse=True)[1].astype(np.int64).reshape(-1)
            self._labels = cached = (self._ids, torch.from_numpy(dense).to(self.dev))
        return cached[1]

    def search_distinct(self, query_embeddings, topN, group_of=None):
        """search, with every group of rows represented once, by its best row: (D float64 [nq,topN], passage ids int64
        [nq,topN]) of the topN best groups, exact however many rows a group has (index.search_grouped_tensor; faiss's grouped
        search).  group_of=None: a group is the rows that carry one external passage id -- a full list of distinct passage
        ids, what output_test_res's seen_pid de-dup leaves of a list that was long enough.  group_of: an integer array over the
        EXTERNAL ids, group_of[passage id] = the group (the page of a passage), values in [0, 2^32); every id a row carries must
        index it.  Fewer than topN groups: the tail is -FLT_MAX / -1."""
        import torch
        q = query_embeddings if isinstance(query_embeddings, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(query_embeddings, dtype=np.float32))
        if group_of is None:
            labels = self._passage_labels()
        else:
            g = np.asarray(group_of)
            if g.dtype.kind not in "iu" or g.ndim != 1:
                raise ValueError(f"search_distinct: group_of must be a 1-D integer array over the passage ids, got {g.dtype} {g.shape}")
            if len(self._ids) and (self._ids.min() < 0 or self._ids.max() >= g.shape[0]):
                raise ValueError(f"search_distinct: group_of has {g.shape[0]} entries but the rows carry passage ids in "
                                 f"[{int(self._ids.min())}, {int(self._ids.max())}]")
            rows = g[self._ids].astype(np.int64)
            if rows.size and (rows.min() < 0 or rows.max() >= 2 ** 32):
                raise ValueError("search_distinct: group_of values must lie in [0, 2^32)")
            labels = torch.from_numpy(np.ascontiguousarray(rows)).to(self.dev)
        D, I = self.index.search_grouped_tensor(q.to(self.dev), topN, labels, id_map=self.id_map)
        return D.cpu().numpy().astype(np.float64), I.cpu().numpy()

    def remove(self, passage_ids):
        """Drop passages from the resident corpus in place (a withdrawn passage, a duplicate): passage_ids, integers of any
        shape, EXTERNAL ids (-1 = padding).  Every row that carries one of them goes (an id two blocks hold names two rows), an
        id no block holds is ignored; returns the number of rows removed.  The rows left keep their order (index.remove_ids),
        so later results are those of a corpus loaded without the removed rows."""
        import torch
        pid = np.asarray(passage_ids)
        if pid.dtype.kind not in "iu":
            raise ValueError(f"remove: passage ids must be integers, got dtype {pid.dtype}")
        rows = rows_carrying(*self._id_lookup(), pid.reshape(1, -1))[0]
        rows = np.unique(rows[rows >= 0])
        removed = self.index.remove_ids(rows)
        self._ids = np.delete(self._ids, rows)
        self.id_map = torch.from_numpy(self._ids).to(self.dev)
        self._lookup = None
        return removed

    # ---- the seam of a re-ranker: rows and exact scores by EXTERNAL passage id --------------------------------------
    def rows_of(self, passage_ids):
        """External passage ids (any shape) -> rows of the index, int64 of the same shape; -1 where no block holds the id.
        The lookup (the block id arrays sorted once, on the host) is built by the first call; an id that several rows
        carry resolves to the first of them."""
        pid = np.asarray(passage_ids)
        if pid.dtype.kind not in "iu":
            raise ValueError(f"rows_of: passage ids must be integers, got dtype {pid.dtype}")
        pid = pid.astype(np.int64)
        sorted_ids, order = self._id_lookup()
        if len(sorted_ids) == 0:
            return np.full(pid.shape, -1, np.int64)
        at = np.minimum(np.searchsorted(sorted_ids, pid, side="left"), len(sorted_ids) - 1)
        return np.where(sorted_ids[at] == pid, order[at], -1).astype(np.int64)

    def _pairs(self, query_embeddings, passage_ids, what):
        """(host queries, rows int64 [nq, m]) of score / rank"""
        import torch
        q = query_embeddings.cpu().numpy() if isinstance(query_embeddings, torch.Tensor) else query_embeddings
        pid = np.asarray(passage_ids)
        if pid.ndim != 2:
            raise ValueError(f"{what}: passage_ids must be [nq, m], got shape {pid.shape}")
        return q, self.rows_of(pid)

    def score(self, query_embeddings, passage_ids):
        """Exact scores of named passages -- dense re-ranking of another system's run (a BM25 top-1000, the gold passages):
        query_embeddings float32 [nq,768], passage_ids int64 [nq,m] -> float64 [nq,m], the score search() gives that pair;
        -FLT_MAX where the passage is in no block."""
        return self.index.score_ids(*self._pairs(query_embeddings, passage_ids, "score")).astype(np.float64)

    def rank(self, query_embeddings, passage_ids):
        """Exact corpus rank of named passages: query_embeddings float32 [nq,768], passage_ids int64 [nq,m] EXTERNAL ids ->
        int64 [nq,m], the 0-based position search() of unbounded depth would give the passage's row; -1 where no block holds
        the id (or the row's score is NaN).  The rank is over ROWS, not over de-duplicated passage ids: an id several rows
        carry resolves to the first of them (rows_of), and the other rows that carry it count as rows in front or behind like
        any other -- the TREC writer's per-query de-duplication (trec.output_test_res) is not applied."""
        return self.index.rank_ids(*self._pairs(query_embeddings, passage_ids, "rank"))

    def rerank(self, query_embeddings, passage_ids, topN):
        """Dense re-ranking of another system's run, as a ranking: query_embeddings float32 [nq,768] (numpy or CUDA tensor),
        passage_ids int64 [nq, m] EXTERNAL ids (-1 = padding) -> (D float64 [nq,topN], I int64 [nq,topN] external ids) like
        search(), over the query's named passages only.  The candidates are every row that carries one of the ids
        (rows_carrying: an id two blocks hold names two rows, and both are ranked); an id no block holds adds nothing; lists
        shorter than topN are padded with -FLT_MAX / -1.  Raises ValueError if the widest row list exceeds HAC_MAX_AMONG."""
        import torch
        from . import _lib
        q = query_embeddings if isinstance(query_embeddings, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(query_embeddings, dtype=np.float32))
        rows = rows_carrying(*self._id_lookup(), passage_ids)
        if rows.shape[0] != q.shape[0]:
            raise ValueError(f"rerank: {q.shape[0]} queries but passage_ids of shape {np.asarray(passage_ids).shape} (one list per query)")
        if rows.shape[1] > _lib.HAC_MAX_AMONG:
            raise ValueError(f"rerank: the widest list names {rows.shape[1]} rows, more than {_lib.HAC_MAX_AMONG}")
        D, I = self.index.search_among_tensor(q.to(self.dev), topN, torch.from_numpy(rows).to(self.dev), id_map=self.id_map)
        return D.cpu().numpy().astype(np.float64), I.cpu().numpy()

    # ---- lists whose length follows the scores ---------------------------------------------------------------------
    def _host_queries(self, query_embeddings):
        import torch
        return query_embeddings.cpu().numpy() if isinstance(query_embeddings, torch.Tensor) else query_embeddings

    def range_search(self, query_embeddings, radius):
        """Every passage scoring STRICTLY above a radius (a scalar, or one float32 per query): query_embeddings float32
        [nq,768] -> (lims int64 [nq+1], D float64 [total], I int64 [total] EXTERNAL passage ids); query i owns
        D[lims[i]:lims[i+1]] and I[lims[i]:lims[i+1]], ordered like search() (score desc, row asc) -- the head of a search of
        unbounded depth.  Over ROWS: an id several rows carry appears once per row."""
        lims, D, I = self.index.range_search(self._host_queries(query_embeddings), radius)
        return lims, D.astype(np.float64), self._ids[I]

    def ahead_of(self, query_embeddings, passage_ids):
        """The rows an unbounded search puts ahead of each query's named passage by SCORE: passage_ids int64 [nq] EXTERNAL ids
        -> (lims, D, I) as range_search, with the radius score() of that passage.  The comparison is strict: rows that TIE the
        passage's score are not included, whichever side of it search() lists them on (so len can be below rank() when
        scores tie), and the passage itself never is.  A passage no block holds, or one whose score is NaN, gives an
        empty list."""
        q = self._host_queries(query_embeddings)
        pid = np.asarray(passage_ids)
        if pid.ndim != 1:
            raise ValueError(f"ahead_of: passage_ids must be [nq], got shape {pid.shape}")
        rows = self.rows_of(pid)[:, None]
        radius = self.index.score_ids(q, rows)[:, 0]
        radius = np.where(rows[:, 0] < 0, np.float32(np.inf), radius).astype(np.float32)
        return self.range_search(q, radius)

    # ---- lists deeper than HAC_MAX_K, and the rows behind a passage (index.search_after*) ---------------------------
    def _within_masks(self, within, within_of, nq, what):
        """(words int64 [n_masks, W], mask_of int64 [nq] or None) of a within= / within_of= pair, checked on the host as
        search(within=) checks them (the tensor forms would answer a mask outside [0, n_masks) with an empty list)."""
        from .index import _as_masks
        words, mask_of = _as_masks(within, within_of, nq, self.ntotal, what)
        if mask_of is not None and mask_of.size and (mask_of.min() < 0 or mask_of.max() >= words.shape[0]):
            raise ValueError(f"{what}: within_of names a mask outside [0, {words.shape[0]})")
        return words, mask_of

    def search_deep(self, query_embeddings, depth, page=1024, within=None, within_of=None):
        """search() to ANY depth: query_embeddings float32 [nq,768] (numpy or CUDA tensor) -> (D float64 [nq,depth], I int64
        [nq,depth] EXTERNAL passage ids), the head of an unbounded search, padded with -FLT_MAX / -1 behind the last row whose
        score is not NaN.  The list is fetched in pages of `page` <= HAC_MAX_K rows: page one through search's own routes
        (index.search_keys_tensor), every later page behind the last key of the page before it
        (index.search_after_keys_tensor), each at the cost of an exact scan whatever its depth; the keys are unpacked once, at
        the end.  Over ROWS, like search().
        within / within_of: masks over the rows as in search(within=) -- the list is then the head of the unbounded search of
        the SELECTED rows ("more results, but only from this topic"): page one through index.search_masked_keys_tensor, every
        later page behind the last key of the page before it under the same masks (after_keys=), each at the cost of the
        masks' own groups."""
        import torch
        from . import _lib
        from .index import keys_to_results
        for name, v in (("depth", depth), ("page", page)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 1:
                raise ValueError(f"search_deep: {name} must be an integer >= 1, got {v!r}")
        depth, page = int(depth), int(page)
        if page > _lib.HAC_MAX_K:
            raise ValueError(f"search_deep: page = {page} exceeds {_lib.HAC_MAX_K}")
        if within_of is not None and within is None:
            raise ValueError("search_deep: within_of without within")
        q = query_embeddings if isinstance(query_embeddings, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(query_embeddings, dtype=np.float32))
        q = q.to(self.dev)
        if within is None:
            first = lambda k: self.index.search_keys_tensor(q, k)
            later = lambda k, cursor: self.index.search_after_keys_tensor(q, k, cursor)
        else:
            words, mask_of = self._within_masks(within, within_of, q.shape[0], "search_deep(within=)")
            masks = torch.from_numpy(words).to(self.dev)
            mask_of = None if mask_of is None else torch.from_numpy(mask_of).to(self.dev)
            first = lambda k: self.index.search_masked_keys_tensor(q, k, masks, mask_of)
            later = lambda k, cursor: self.index.search_masked_keys_tensor(q, k, masks, mask_of, after_keys=cursor)
        pages = [first(min(page, depth))]
        got = pages[0].shape[1]
        while got < depth:
            k = min(page, depth - got)
            pages.append(later(k, pages[-1][:, -1].contiguous()))
            got += k
        D, I = keys_to_results(torch.cat(pages, dim=1), self.id_map)
        return D.cpu().numpy().astype(np.float64), I.cpu().numpy()

    def search_window(self, query_embeddings, start, n):
        """The ranks [start, start + n) of an unbounded search WITHOUT the ranks in front of them -- hard negatives from a rank
        window, page 57 of a listing: query_embeddings float32 [nq,768] (numpy or CUDA tensor), start an integer >= 0 or int64
        [nq], n >= 1 -> (D float64 [nq,n], I int64 [nq,n] EXTERNAL passage ids), padded with -FLT_MAX / -1 behind the last row
        whose score is not NaN.  The first page stands behind the entry at rank start - 1 (index.search_at_keys_tensor: its cost
        does not grow with start); beyond HAC_MAX_K rows the window is paged like search_deep.  Over ROWS, like search()."""
        import torch
        from . import _lib
        from .index import _as_start, keys_to_results
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or int(n) < 1:
            raise ValueError(f"search_window: n must be an integer >= 1, got {n!r}")
        n = int(n)
        q = query_embeddings if isinstance(query_embeddings, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(query_embeddings, dtype=np.float32))
        q = q.to(self.dev)
        start = torch.from_numpy(_as_start(start, q.shape[0], "search_window")).to(self.dev)
        page = _lib.HAC_MAX_K
        pages = [self.index.search_at_keys_tensor(q, min(page, n), start)]
        got = pages[0].shape[1]
        while got < n:
            k = min(page, n - got)
            pages.append(self.index.search_after_keys_tensor(q, k, pages[-1][:, -1].contiguous()))
            got += k
        D, I = keys_to_results(torch.cat(pages, dim=1), self.id_map)
        return D.cpu().numpy().astype(np.float64), I.cpu().numpy()

    def score_at_rank(self, query_embeddings, ranks):
        """The score at a rank -- the radius that makes range_search return exactly that many rows, score quantiles of the
        corpus: query_embeddings float32 [nq,768], ranks int64 [nq, m] -> float64 [nq, m], the score of the entry at each
        0-based rank of an unbounded search; -FLT_MAX where the rank lies outside the list (index.entries_at)."""
        q = np.ascontiguousarray(self._host_queries(query_embeddings), dtype=np.float32)
        return self.index.entries_at(q, ranks)[0].astype(np.float64)

    def behind(self, query_embeddings, passage_ids, n, within=None, within_of=None):
        """The n rows an unbounded search lists right BEHIND each query's named passage -- negatives from just below the gold
        passage; the mirror of ahead_of: passage_ids int64 [nq] EXTERNAL ids -> (D float64 [nq,n], I int64 [nq,n] EXTERNAL
        ids) like search(), n <= HAC_MAX_K.  The cursor is (score() of the passage, its row): rows that tie its score and come
        later are included, the passage itself never is.  A passage no block holds, or one whose score is NaN, gives an
        empty list (-FLT_MAX / -1).
        within / within_of: masks over the rows as in search(within=) -- the n SELECTED rows right behind the passage ("the n
        passages behind the gold one that the user has not seen"); the passage's own row need not be selected
        (index.search_masked(after=))."""
        q = np.ascontiguousarray(self._host_queries(query_embeddings), dtype=np.float32)
        pid = np.asarray(passage_ids)
        if pid.ndim != 1:
            raise ValueError(f"behind: passage_ids must be [nq], got shape {pid.shape}")
        if within_of is not None and within is None:
            raise ValueError("behind: within_of without within")
        rows = self.rows_of(pid)                                  # (-1 where no block holds the id: the exhausted cursor)
        scores = self.index.score_ids(q, rows[:, None])[:, 0]
        if within is None:
            D, I = self.index.search_after(q, n, (scores, rows))
        else:
            words, mask_of = self._within_masks(within, within_of, q.shape[0], "behind(within=)")
            D, I = self.index.search_masked(q, n, words, mask_of, after=(scores, rows))
        return D.astype(np.float64), np.where(I >= 0, self._ids[np.maximum(I, 0)], -1)

    def reconstruct(self, passage_ids):
        """passage_ids int64 [n] -> float32 [n,768], the embeddings as the blocks hold them (all-ones words for an absent id)."""
        return self.index.reconstruct_batch(self.rows_of(passage_ids))
