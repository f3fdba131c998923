"""Host mirror of gemm8_kernel's tile runs (haconvdr_amd/csrc/gemm8.inc, "XCD-aware tile runs"): test code only.

The kernel is launched with one persistent workgroup per CU.  Workgroup b sits on XCD x = b & 7 in slot b >> 3; XCD x owns
column group x % n_groups (nxg = nx / n_groups column tiles) and the (x / n_groups)-th of NP = 8 / n_groups shares of the
row tiles, [mt_all * p / NP, mt_all * (p + 1) / NP) (floors: the shares differ by one).  Inside that run the local tile
l is (row tile mt_lo + l / nxg, column tile n_base + l % nxg), and the XCD's per_xcd workgroups take l = slot,
slot + per_xcd, ... -- `seq` counts a workgroup's tiles, my_tiles is how many it takes.  Everything that happens at a tile
seam of the kernel (the DMA stream running on into the next tile, the RESID epilogue re-staging the next tile's first
k-tiles, s_tile += per_xcd) happens between seq and seq + 1 of one workgroup.

The launches of one encoder layer (encoder.hip layer_gemm8, and qkv_gemm8 from tail_classic for the last layer), as (nx, n_groups, n_tile0):

  class     launch                         nx  groups  tile0   first mt_all at which a workgroup of 256 takes a 2nd tile
  QKV       EPI8_QKV, N = 2304              9     1      0      25
  QKV_KV    the last layer's K | V only     6     1      3      41
  RESID     EPI8_RESID: out-proj, FFN-down  3     1      0      81
  GELU      EPI8_GELU: FFN-up, N = 3072    12     2      0      21

(tests/test_gemm8_tiles.py asserts these thresholds and the exact cover of every tile by the mirror.)

Inside a 256 x 256 tile wave (wr, wc) of the 2 x 4 grid owns rows {i * 128 + wr * 64 .. + 64 : i = 0, 1} and the 64
contiguous columns wc * 64 .. + 64; a sub-band (i, mt) is 16 of its rows (mt = 0 .. 3) by its 64 columns: the unit in which
the RESID epilogue lands the residual in LDS, computes and stores."""
import numpy as np

CLASSES = {"QKV": (9, 1, 0), "QKV_KV": (6, 1, 3), "RESID": (3, 1, 0), "GELU": (12, 2, 0)}
# the first row-tile count at which some workgroup of a 256-CU device takes a second tile
SECOND_TILE_AT = {"QKV": 25, "QKV_KV": 41, "RESID": 81, "GELU": 21}
TILE = 256
SEQ_ALIGN = 32


def tile_runs(mt_all, nx, n_groups, n_wg, n_tile0=0):
    """gemm8.inc's run arithmetic, line for line, for all workgroups at once: arrays (workgroup, seq, row tile, column tile,
    my_tiles of that workgroup), one entry per tile a workgroup takes, ordered by workgroup and seq."""
    NG, nxg, NP = n_groups, nx // n_groups, 8 // n_groups
    b = np.arange(n_wg, dtype=np.int64)
    xcd, slot, per_xcd = b & 7, b >> 3, (n_wg + 7 - (b & 7)) >> 3
    mt_lo, mt_hi = mt_all * (xcd // NG) // NP, mt_all * (xcd // NG + 1) // NP
    n_base = n_tile0 + (xcd % NG) * nxg
    run_hi = (mt_hi - mt_lo) * nxg
    tile0 = slot
    my_tiles = np.where(tile0 >= run_hi, 0, (run_hi - tile0 + per_xcd - 1) // np.maximum(per_xcd, 1))
    seq = np.arange(max(int(my_tiles.max()), 1), dtype=np.int64)[None, :]
    live = seq < my_tiles[:, None]
    tile = tile0[:, None] + seq * per_xcd[:, None]
    rt, ct = mt_lo[:, None] + tile // nxg, n_base[:, None] + tile % nxg
    wg = np.broadcast_to(b[:, None], live.shape)
    return wg[live], np.broadcast_to(seq, live.shape)[live], rt[live], ct[live], np.broadcast_to(my_tiles[:, None], live.shape)[live]


def tile_map(mt_all, nx, n_groups, n_wg, n_tile0=0):
    """For every workgroup 0 .. n_wg - 1 its ordered list of (row tile, column tile)."""
    runs = [[] for _ in range(n_wg)]
    wg, _, rt, ct, _ = tile_runs(mt_all, nx, n_groups, n_wg, n_tile0)
    for w, r, c in zip(wg.tolist(), rt.tolist(), ct.tolist()):
        runs[w].append((r, c))
    return runs


def owners(mt_all, nx, n_groups, n_wg, n_tile0=0):
    """tile_map inverted: {(row tile, column tile): (xcd, slot, seq, my_tiles)}.  A tile met twice is an error."""
    out = {}
    for b, run in enumerate(tile_map(mt_all, nx, n_groups, n_wg, n_tile0)):
        for seq, t in enumerate(run):
            assert t not in out, ("tile covered twice", t, out[t], b)
            out[t] = (b & 7, b >> 3, seq, len(run))
    return out


def my_tiles_present(mt_all, cls, n_wg):
    """The sorted my_tiles values of the workgroups that take any tile of a launch of class cls."""
    nx, ng, t0 = CLASSES[cls]
    return sorted({len(r) for r in tile_map(mt_all, nx, ng, n_wg, t0) if r})


def share_bounds(mt_all, cls):
    """The row tiles at which an XCD's share of class cls begins (mt_lo of every share but the first)."""
    NP = 8 // CLASSES[cls][1]
    return sorted({mt_all * p // NP for p in range(1, NP)})


class Geometry:
    """The tile ownership of every launch class for one batch: mt_all row tiles on n_wg workgroups."""

    def __init__(self, mt_all, n_wg):
        self.mt_all, self.n_wg = int(mt_all), int(n_wg)
        self.own = {c: owners(self.mt_all, nx, ng, self.n_wg, t0) for c, (nx, ng, t0) in CLASSES.items()}

    def locate(self, packed_row, column, cls):
        """Who computes element (packed_row, column) of a launch of class cls (column: the output feature, 0 .. N - 1): a dict
        of the row tile, column tile, xcd, slot, seq, my_tiles, the wave (wr, wc), the 128-row half i and the sub-band mt."""
        rt, ct = int(packed_row) >> 8, int(column) >> 8
        xcd, slot, seq, my = self.own[cls][(rt, ct)]
        r, c = int(packed_row) & 255, int(column) & 255
        return {"cls": cls, "row_tile": rt, "col_tile": ct, "xcd": xcd, "slot": slot, "seq": seq, "my_tiles": my,
                "wr": (r & 127) >> 6, "wc": c >> 6, "i": r >> 7, "mt": (r & 63) >> 4}

    def row_seqs(self, row_tile, cls):
        """The seq values of the column tiles of one row tile, in column order."""
        nx, _, t0 = CLASSES[cls]
        return tuple(self.own[cls][(int(row_tile), t0 + c)][2] for c in range(nx))

    def row_tile_kinds(self, row_tile, cls):
        """Which parts of a workgroup's run compute row tile `row_tile` in class cls: a subset of {"first", "middle", "last"}
        ("first": seq = 0; "last": seq = my_tiles - 1 >= 1; "middle": strictly between)."""
        nx, _, t0 = CLASSES[cls]
        kinds = set()
        for c in range(nx):
            _, _, seq, my = self.own[cls][(int(row_tile), t0 + c)]
            if seq == 0:
                kinds.add("first")
            elif seq == my - 1:
                kinds.add("last")
            else:
                kinds.add("middle")
        return kinds


def packed_offsets(lens):
    """Packed row offset of every sequence and the total (seq_prep_kernel / seq_offsets_kernel: roundup(len, 32) rows per
    sequence, in batch order).  Token t of sequence b is packed row off[b] + t."""
    l32 = (np.asarray(lens, np.int64) + SEQ_ALIGN - 1) // SEQ_ALIGN * SEQ_ALIGN
    off = np.concatenate([[0], np.cumsum(l32)])
    return off[:-1], int(off[-1])


def row_tiles_of(off, lens, b):
    """The row tiles that hold valid tokens of sequence b."""
    return list(range(int(off[b]) >> 8, ((int(off[b]) + int(lens[b]) - 1) >> 8) + 1))


def chunks_by_tiles(lens, max_tiles):
    """Cut the sequences, in order, into runs [b0, b1) of at most max_tiles row tiles (of 256 packed rows) each."""
    l32 = (np.asarray(lens, np.int64) + SEQ_ALIGN - 1) // SEQ_ALIGN * SEQ_ALIGN
    out, b0, rows = [], 0, 0
    for b, r in enumerate(l32):
        if b > b0 and rows + r > max_tiles * TILE:
            out.append((b0, b))
            b0, rows = b, 0
        rows += int(r)
    out.append((b0, len(l32)))
    return out
