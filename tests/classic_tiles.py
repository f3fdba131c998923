"""Host mirror of gemm_bf16_nt_kernel<EPI, 2>'s item runs (haconvdr_amd/csrc/encoder.hip, the classic 128 x 128 kernel): test code only.

The kernel is persistent: launch_gemm128 starts n_wg = 2 * n_cu workgroups.  A launch has n = row tiles x nx x S work items;
item t is output tile t / S (row tile (t / S) / nx, column tile (t / S) % nx) and, for RESID with split-K, slice t % S (k-tiles
[slice * KT / S, (slice + 1) * KT / S)); every other launch has S = 1.  Workgroup b sits on XCD x = b & 7 in slot b >> 3; XCD x
owns the run [n * x / 8, n * (x + 1) / 8) of items, and its per_xcd = (n_wg + 7 - x) >> 3 workgroups take the items
run_lo + slot, run_lo + slot + per_xcd, ...: `seq` counts a workgroup's items, my_items is how many it takes.  During the last
k-step of an item the first k-tile of the next one is staged (for RESID: k-tile (next_tile % S) * KT / S of tile next_tile / S),
so everything that can go wrong at an item seam goes wrong between seq and seq + 1 of one workgroup.

The launches, as (nx, what the rows are):

  class       launch                                   nx   rows                 first row-tile count with a second item on 512 workgroups
  QKV         EPI_QKV, N = 2304                        18   the packed rows      29
  GELU        EPI_GELU: FFN-up, N = 3072               24   the packed rows      22
  RESID       EPI_RESID: out-proj and FFN-down, N=768   6   the packed rows      86 at S = 1 (never reached: this family ends at 72 row tiles);
                                                                                 with S slices from 512 / (6 S) row tiles on
  TAIL_GELU   the last layer's FFN-up on the <s> rows  24   one per sequence     22 (2689 sequences)
  TAIL_RESID  the last layer's two RESID GEMMs          6   one per sequence     86, S = 1 always

(tests/test_classic_tiles.py asserts these thresholds and the exact cover of every (tile, slice) by the mirror.)

Inside a 128 x 128 tile wave (wm, wn) of the 2 x 2 grid owns rows wm * 64 .. + 64 and columns wn * 64 .. + 64; its two 32-row MFMA
tiles a = 0, 1 go out as two 16 x 64 sub-tiles each (half = 0, 1), transposed through the wave's LDS patch: the unit in which the
epilogue loads the residual, computes and stores."""
import numpy as np

CLASSES = {"QKV": 18, "GELU": 24, "RESID": 6, "TAIL_GELU": 24, "TAIL_RESID": 6}      # class -> nx (column tiles of 128)
# the first row-tile count at which some workgroup of a 256-CU device (512 workgroups) takes a second item, S = 1
SECOND_ITEM_AT = {"QKV": 29, "GELU": 22, "RESID": 86, "TAIL_GELU": 22, "TAIL_RESID": 86}
TILE = 128
SEQ_ALIGN = 32


def item_runs(n_items, n_wg):
    """The kernel's run arithmetic, line for line, for all workgroups at once: arrays (workgroup, seq, item, my_items of that
    workgroup), one entry per item a workgroup takes, ordered by workgroup and seq."""
    n = int(n_items)
    b = np.arange(n_wg, dtype=np.int64)
    xcd, slot, per_xcd = b & 7, b >> 3, (n_wg + 7 - (b & 7)) >> 3
    run_lo, run_hi = n * xcd // 8, n * (xcd + 1) // 8
    tile0 = run_lo + slot
    my_items = np.where(tile0 >= run_hi, 0, (run_hi - tile0 + per_xcd - 1) // np.maximum(per_xcd, 1))
    seq = np.arange(max(int(my_items.max()), 1), dtype=np.int64)[None, :]
    live = seq < my_items[:, None]
    item = tile0[:, None] + seq * per_xcd[:, None]
    wg = np.broadcast_to(b[:, None], live.shape)
    return wg[live], np.broadcast_to(seq, live.shape)[live], item[live], np.broadcast_to(my_items[:, None], live.shape)[live]


def tile_runs(row_tiles, nx, S, n_wg):
    """item_runs of a launch of row_tiles x nx output tiles in S slices, each item resolved as the kernel does (otile = t / S,
    slice = t % S, row tile otile / nx, column tile otile % nx): arrays (workgroup, seq, row tile, column tile, slice, my_items)."""
    wg, seq, item, my = item_runs(int(row_tiles) * nx * S, n_wg)
    otile, sl = item // S, item % S
    return wg, seq, otile // nx, otile % nx, sl, my


def owners(row_tiles, nx, S, n_wg):
    """{(row tile, column tile, slice): (xcd, slot, seq, my_items)}.  A (tile, slice) met twice is an error."""
    out = {}
    wg, seq, rt, ct, sl, my = tile_runs(row_tiles, nx, S, n_wg)
    for b, q, r, c, s, m in zip(wg.tolist(), seq.tolist(), rt.tolist(), ct.tolist(), sl.tolist(), my.tolist()):
        assert (r, c, s) not in out, ("item covered twice", (r, c, s), out[(r, c, s)], b)
        out[(r, c, s)] = (b & 7, b >> 3, q, m)
    return out


def depths(row_tiles, cls, n_wg, S=1):
    """The sorted my_items values of the workgroups that take any item of a launch of class cls."""
    my = item_runs(int(row_tiles) * CLASSES[cls] * S, n_wg)[3]
    return sorted(set(my.tolist()))


def max_items(row_tiles, S_out=1, S_down=1):
    """The largest item count among the launches of one layer on row_tiles row tiles."""
    return int(row_tiles) * max(CLASSES["QKV"], CLASSES["GELU"], CLASSES["RESID"] * max(S_out, S_down))


def _where(own, cls, packed_row, column, slice_):
    rt, ct = int(packed_row) >> 7, int(column) >> 7
    xcd, slot, seq, my = own[(rt, ct, int(slice_))]
    r, c = int(packed_row) & 127, int(column) & 127
    return {"cls": cls, "row_tile": rt, "col_tile": ct, "slice": int(slice_), "xcd": xcd, "slot": slot, "seq": seq, "my_items": my,
            "wm": r >> 6, "wn": c >> 6, "a": (r >> 5) & 1, "half": (r >> 4) & 1}


class Geometry:
    """The item ownership of every launch of a layer for one batch: row_tiles row tiles of 128 packed rows on n_wg workgroups, the
    out-proj in S_out and the FFN-down in S_down slices.  Classes: QKV, GELU, RESID_OUT, RESID_DOWN."""

    def __init__(self, row_tiles, n_wg, S_out=1, S_down=1):
        self.row_tiles, self.n_wg = int(row_tiles), int(n_wg)
        self.nx = {"QKV": 18, "GELU": 24, "RESID_OUT": 6, "RESID_DOWN": 6}
        self.S = {"QKV": 1, "GELU": 1, "RESID_OUT": int(S_out), "RESID_DOWN": int(S_down)}
        self.own = {c: owners(self.row_tiles, self.nx[c], self.S[c], self.n_wg) for c in self.nx}

    def locate(self, packed_row, column, cls, slice_=0):
        """Who computes element (packed_row, column) of a launch of class cls (column: the output feature, 0 .. N - 1), slice
        slice_ of its k range: a dict of the row tile, column tile, slice, xcd, slot, seq, my_items, the wave (wm, wn), the 32-row
        MFMA tile a and the 16-row half."""
        return _where(self.own[cls], cls, packed_row, column, slice_)

    def row_seqs(self, row_tile, cls):
        """The (seq, my_items) of every item of one row tile, column tiles in order, slices innermost."""
        return tuple(self.own[cls][(int(row_tile), c, s)][2:] for c in range(self.nx[cls]) for s in range(self.S[cls]))

    def row_tile_kinds(self, row_tile, cls):
        """Which parts of a workgroup's run compute row tile `row_tile` in class cls: a subset of {"first", "middle", "last"}
        ("first": seq = 0; "last": seq = my_items - 1 >= 1; "middle": strictly between)."""
        kinds = set()
        for seq, my in self.row_seqs(row_tile, cls):
            kinds.add("first" if seq == 0 else ("last" if seq == my - 1 else "middle"))
        return kinds

    def run_bounds(self, cls):
        """(row tile of the last item of XCD x - 1, row tile of the first item of XCD x) for x = 1 .. 7."""
        nx, S = self.nx[cls], self.S[cls]
        n = self.row_tiles * nx * S
        return [((n * x // 8 - 1) // S // nx, n * x // 8 // S // nx) for x in range(1, 8)]


def locate(packed_row, column, cls, S=1, row_tiles=None, n_wg=512, slice_=0):
    """Geometry.locate without a Geometry: cls one of CLASSES (the tail classes: packed_row is the sequence index), S slices,
    row_tiles row tiles in the launch (default: just enough to hold packed_row)."""
    rt_all = int(packed_row) // TILE + 1 if row_tiles is None else int(row_tiles)
    return _where(owners(rt_all, CLASSES[cls], S, n_wg), cls, packed_row, column, slice_)


def packed_offsets(lens):
    """Packed row offset of every sequence and the total (seq_prep_kernel / seq_offsets_kernel: roundup(len, 32) rows per
    sequence, in batch order).  Token t of sequence b is packed row off[b] + t."""
    l32 = (np.asarray(lens, np.int64) + SEQ_ALIGN - 1) // SEQ_ALIGN * SEQ_ALIGN
    off = np.concatenate([[0], np.cumsum(l32)])
    return off[:-1], int(off[-1])


def row_tiles_of(off, lens, b):
    """The row tiles that hold valid tokens of sequence b."""
    return list(range(int(off[b]) >> 7, ((int(off[b]) + int(lens[b]) - 1) >> 7) + 1))


def chunks_by_items(lens, max_items_, S_out=1, S_down=1):
    """Cut the sequences, in order, into runs [b0, b1) in which no launch of a layer has more than max_items_ items (a single
    sequence that exceeds it alone is an error)."""
    l32 = (np.asarray(lens, np.int64) + SEQ_ALIGN - 1) // SEQ_ALIGN * SEQ_ALIGN

    def items(rows):
        return max_items((rows + TILE - 1) // TILE, S_out, S_down)
    out, b0, rows = [], 0, 0
    for b, r in enumerate(l32.tolist()):
        assert items(r) <= max_items_, ("sequence", b, "alone has", items(r), "items")
        if b > b0 and items(rows + r) > max_items_:
            out.append((b0, b))
            b0, rows = b, 0
        rows += r
    out.append((b0, len(l32)))
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def diff_elements(a, b, valid):
    """The comparer: index arrays of the valid tokens' elements whose BITS differ between two state arrays over [n, L, 768] (or
    [n, L]: the statistics), and the number of elements compared."""
    v = np.asarray(valid, bool)
    ne = bits(a) != bits(b)
    ne &= v[..., None] if ne.ndim == 3 else v
    return (np.nonzero(ne) if ne.any() else tuple(np.zeros(0, np.int64) for _ in range(ne.ndim))), int(v.sum()) * (a.shape[2] if a.ndim == 3 else 1)


def describe(geo, off, b, t, c=None, limit=6):
    """Who computed the differing elements (sequence b, token t, feature c; c = None: a row statistic) of a layer's output, the
    FFN-down launch (RESID_DOWN): the first `limit` through locate (slice 0, the item that adds bias and residual), with the
    (seq, my_items) of the row tile's QKV, GELU and out-proj items (an upstream launch spoils whole rows), and the count of
    differing elements per seq value of the slice-0 item and, with slices, of the deepest item of the element's tile."""
    row = np.asarray(off)[np.asarray(b)] + np.asarray(t)
    col = np.zeros_like(row) if c is None else np.asarray(c)
    S = geo.S["RESID_DOWN"]
    first = []
    for r, cc, bb, tt in list(zip(row.tolist(), col.tolist(), np.asarray(b).tolist(), np.asarray(t).tolist()))[:limit]:
        loc = geo.locate(r, cc, "RESID_DOWN")
        loc.update(sequence=bb, token=tt, packed_row=r, column=None if c is None else cc,
                   slice_seqs=tuple(geo.own["RESID_DOWN"][(r >> 7, cc >> 7, s)][2] for s in range(S)),
                   qkv_seqs=geo.row_seqs(r >> 7, "QKV"), gelu_seqs=geo.row_seqs(r >> 7, "GELU"), out_proj_seqs=geo.row_seqs(r >> 7, "RESID_OUT"))
        first.append(loc)
    tiles = list(zip((row >> 7).tolist(), (col >> 7).tolist()))
    seq0 = np.array([geo.own["RESID_DOWN"][(r, cc, 0)][2] for r, cc in tiles], np.int64)
    deep = np.array([max(geo.own["RESID_DOWN"][(r, cc, s)][2] for s in range(S)) for r, cc in tiles], np.int64)
    count = lambda a: {int(s): int(n) for s, n in zip(*np.unique(a, return_counts=True))}
    return {"differing": int(len(row)), "per_seq": count(seq0), "per_deepest_slice_seq": count(deep), "rows": int(len(np.unique(row))), "first": first}
