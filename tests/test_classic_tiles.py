"""The host mirror of the classic 128 x 128 kernel's item runs (tests/classic_tiles.py) covers every (tile, slice) exactly once,
and the row-tile counts at which a workgroup first takes a second item, the depths of the batches of
tests/test_encoder_classic_tiles_gpu.py and its seam-free chunking are what the mirror's table says.  The comparer of that
file is checked here too, on the host: a stale 16 x 64 sub-tile is reported as exactly its 1024 elements."""
import numpy as np

from tests import classic_tiles as ct

N_WG = (512, 608, 160)                  # 2 workgroups per CU on 256, 304 and 80 CUs
ROW_TILES = (1, 2, 5, 7, 13, 21, 22, 28, 29, 42, 43, 60, 72, 85, 86, 173)
SLICES = (1, 2, 3, 4, 6, 12, 16)


def test_mirror_covers_every_item_exactly_once():
    for n_wg in N_WG:
        for nx in sorted(set(ct.CLASSES.values())):
            for S in (SLICES if nx == 6 else (1,)):
                for row_tiles in ROW_TILES:
                    wg, seq, rt, c, sl, my = ct.tile_runs(row_tiles, nx, S, n_wg)
                    what = (n_wg, nx, S, row_tiles)
                    assert len(rt) == row_tiles * nx * S, what + (len(rt),)
                    assert rt.min() >= 0 and rt.max() < row_tiles and c.min() >= 0 and c.max() < nx and sl.min() >= 0 and sl.max() < S, what
                    assert (np.bincount((rt * nx + c) * S + sl, minlength=row_tiles * nx * S) == 1).all(), what
                    assert wg.max() < n_wg and (seq < my).all(), what
                    # a workgroup's items ascend, a constant stride apart (the kernel's tile += per_xcd)
                    item = (rt * nx + c) * S + sl
                    same = wg[1:] == wg[:-1]
                    assert (np.diff(item)[same] == ((n_wg + 7 - (wg[1:][same] & 7)) >> 3)).all(), what


def test_every_item_count_from_1_to_6000_on_512_workgroups():
    for n in range(1, 6001):
        wg, seq, item, my = ct.item_runs(n, 512)
        assert len(item) == n and (np.bincount(item, minlength=n) == 1).all(), n
        assert (my.max() == 1) == (n <= 512), n          # up to 512 items nobody takes a second one, beyond them somebody must


def test_owners_inverts_the_runs():
    for cls, S in (("QKV", 1), ("GELU", 1), ("RESID", 4), ("RESID", 16)):
        nx = ct.CLASSES[cls]
        own = ct.owners(60, nx, S, 512)
        assert len(own) == 60 * nx * S
        wg, seq, rt, c, sl, my = ct.tile_runs(60, nx, S, 512)
        for b, q, r, cc, s, m in zip(wg.tolist(), seq.tolist(), rt.tolist(), c.tolist(), sl.tolist(), my.tolist()):
            assert own[(r, cc, s)] == (b & 7, b >> 3, q, m)


def test_second_item_thresholds():
    """512 workgroups: a second item from 29 (QKV), 22 (FFN-up) and 86 (RESID, S = 1) row tiles on, below them none."""
    assert ct.SECOND_ITEM_AT == {"QKV": 29, "GELU": 22, "RESID": 86, "TAIL_GELU": 22, "TAIL_RESID": 86}
    for cls, at in ct.SECOND_ITEM_AT.items():
        for row_tiles in range(1, at):
            assert ct.depths(row_tiles, cls, 512) == [1], (cls, row_tiles)
        assert ct.depths(at, cls, 512) == [1, 2], (cls, at)
    # RESID with slices: the largest seam-free row-tile count
    for S, most in ((2, 42), (3, 28), (4, 21), (6, 14), (12, 7), (16, 5)):
        for row_tiles in range(1, most + 1):
            assert ct.depths(row_tiles, "RESID", 512, S) == [1], (S, row_tiles)
        assert max(ct.depths(most + 1, "RESID", 512, S)) == 2, (S, most)
    # the family ends at 9216 rows = 72 row tiles: RESID at S = 1 never reaches a seam
    assert ct.depths(72, "RESID", 512) == [1]


def test_depths_of_the_gpu_batches():
    """The depths tests/test_encoder_classic_tiles_gpu.py's batches are built for (512 workgroups)."""
    assert ct.depths(60, "QKV", 512) == [2, 3] and ct.depths(60, "GELU", 512) == [2, 3]
    assert ct.depths(60, "RESID", 512, 4) == [2, 3] and ct.depths(60, "RESID", 512, 16) == [11, 12]
    assert ct.depths(60, "RESID", 512, 3) == [2, 3] and ct.depths(60, "RESID", 512, 6) == [4, 5]
    assert ct.depths(72, "GELU", 512) == [3, 4]
    # the tail: one compact row per sequence
    assert ct.depths((2688 + 127) // 128, "TAIL_GELU", 512) == [1] and ct.depths((2689 + 127) // 128, "TAIL_GELU", 512) == [1, 2]
    assert ct.depths((3000 + 127) // 128, "TAIL_GELU", 512) == [1, 2] and ct.depths((1000 + 127) // 128, "TAIL_GELU", 512) == [1]
    assert ct.depths((3000 + 127) // 128, "TAIL_RESID", 512) == [1]


def test_locate_names_wave_tile_and_half():
    geo = ct.Geometry(60, 512, 4, 16)
    # QKV: 1080 items, XCD 0 owns [0, 135) on 64 workgroups: item 64 = (row tile 3, column tile 10) is slot 0's second of three
    loc = geo.locate(3 * 128 + 64 + 32 + 16 + 5, 10 * 128 + 64 + 7, "QKV")
    assert loc == {"cls": "QKV", "row_tile": 3, "col_tile": 10, "slice": 0, "xcd": 0, "slot": 0, "seq": 1, "my_items": 3, "wm": 1, "wn": 1, "a": 1, "half": 1}
    assert geo.locate(0, 0, "GELU")["seq"] == 0 and geo.locate(0, 3071, "GELU")["col_tile"] == 23
    # FFN-down in 16 slices: 5760 items, XCD 0 owns [0, 720): item 64 * 3 + 5 = 197 = tile 12 (row tile 2, column tile 0), slice 5
    loc = geo.locate(2 * 128, 0, "RESID_DOWN", slice_=5)
    assert (loc["xcd"], loc["slot"], loc["seq"], loc["my_items"]) == (0, 5, 3, 12)
    assert loc == ct.locate(2 * 128, 0, "RESID", 16, row_tiles=60, n_wg=512, slice_=5) | {"cls": "RESID_DOWN"}
    assert len(geo.row_seqs(2, "RESID_DOWN")) == 96 and geo.row_tile_kinds(2, "RESID_DOWN") == {"middle"}
    assert geo.row_tile_kinds(0, "QKV") == {"first"} and "last" in geo.row_tile_kinds(59, "QKV")
    # XCD run boundaries: QKV's first lies at item 135 = row tile 7, column tile 9 -- inside a row tile
    assert geo.run_bounds("QKV")[0] == (7, 7) and geo.run_bounds("RESID_DOWN")[0] == (7, 7) and len(geo.run_bounds("GELU")) == 7


def test_packed_offsets_and_chunks():
    lens = [1, 32, 33, 512, 255, 257, 128, 97]
    off, total = ct.packed_offsets(lens)
    assert off.tolist() == [0, 32, 64, 128, 640, 896, 1184, 1312] and total == 1440
    assert ct.row_tiles_of(off, lens, 3) == [1, 2, 3, 4] and ct.row_tiles_of(off, lens, 5) == [7, 8, 9]
    for S_out, S_down, tiles in ((1, 1, 21), (3, 6, 14), (4, 16, 5)):
        assert ct.max_items(tiles, S_out, S_down) <= 512 < ct.max_items(tiles + 1, S_out, S_down)
        ch = ct.chunks_by_items(lens, 512, S_out, S_down)
        assert ch[0][0] == 0 and ch[-1][1] == len(lens) and all(a[1] == b[0] for a, b in zip(ch, ch[1:]))
        for b0, b1 in ch:
            rows = ct.packed_offsets(lens[b0:b1])[1]
            assert (rows + 127) // 128 <= tiles, (S_out, S_down, b0, b1)
            for cls, S in (("QKV", 1), ("GELU", 1), ("RESID", S_out), ("RESID", S_down)):
                assert ct.depths((rows + 127) // 128, cls, 512, S) == [1]
    assert ct.chunks_by_items(lens, 512, 4, 16) == [(0, 4), (4, 6), (6, 8)]       # 640 | 576 | 256 packed rows


def test_comparison_localises_a_stale_sub_tile():
    """A random [rows, 768] layer output of 60 row tiles; one 16 x 64 sub-tile of an item with seq >= 1 overwritten with the
    sub-tile 16 rows above it (what a stale LDS patch would leave).  The comparer must report exactly those 1024 elements and
    locate must name the tile, wave, a and half -- for FFN-down with one slice and with 16."""
    lens = np.full(15, 512, np.int64)
    off, total = ct.packed_offsets(lens)
    assert total == 60 * 128
    rng = np.random.default_rng(0xC1A551C)
    clean = rng.standard_normal((15, 512, 768)).astype(np.float32)
    valid = np.ones((15, 512), bool)
    for S_down in (1, 16):
        geo = ct.Geometry(60, 512, 4, S_down)
        cls = "RESID_DOWN" if S_down > 1 else "GELU"       # (RESID at S = 1 has no second item on 60 row tiles: place it by FFN-up's items)
        target = None
        for p0 in range(16, total, 16):
            if (p0 & 127) < 16:
                continue                                   # the 16 rows above belong to another tile
            for c0 in range(0, 768, 64):
                loc = geo.locate(p0, c0, cls)
                if loc["seq"] >= 1:
                    target = (p0, c0, loc)
                    break
            if target:
                break
        p0, c0, loc = target
        b, t0 = p0 // 512, p0 % 512
        stale = clean.copy()
        stale[b, t0:t0 + 16, c0:c0 + 64] = clean[b, t0 - 16:t0, c0:c0 + 64]
        d, cnt = ct.diff_elements(stale, clean, valid)
        assert cnt == total * 768 and len(d[0]) == 1024
        assert set(d[0].tolist()) == {b} and set(d[1].tolist()) == set(range(t0, t0 + 16)) and set(d[2].tolist()) == set(range(c0, c0 + 64))
        assert len(ct.diff_elements(clean, clean.copy(), valid)[0][0]) == 0
        named = {tuple(sorted(geo.locate(int(off[bb]) + tt, cc, cls).items())) for bb, tt, cc in zip(*(x.tolist() for x in d))}
        assert named == {tuple(sorted(loc.items()))}, named
        assert (loc["wm"], loc["wn"], loc["a"], loc["half"]) == ((p0 & 127) >> 6, (c0 & 127) >> 6, (p0 >> 5) & 1, (p0 >> 4) & 1)
        rep = ct.describe(geo, off, *d, limit=1024)
        assert rep["differing"] == 1024 and rep["rows"] == 16 and len(rep["first"]) == 1024
        down = geo.locate(p0, c0, "RESID_DOWN")
        assert rep["per_seq"] == {down["seq"]: 1024}, rep["per_seq"]
        assert {(f["row_tile"], f["col_tile"], f["wm"], f["wn"], f["a"], f["half"]) for f in rep["first"]} == \
            {(p0 >> 7, c0 >> 7, loc["wm"], loc["wn"], loc["a"], loc["half"])}
        if S_down > 1:
            assert down["seq"] >= 1 and len(rep["first"][0]["slice_seqs"]) == 16 and set(rep["per_deepest_slice_seq"]) == {max(rep["first"][0]["slice_seqs"])}
        # a row statistic that differs is attributed to its row tile's first column tile
        srep = ct.describe(geo, off, np.array([b]), np.array([t0]))
        assert srep["first"][0]["column"] is None and srep["first"][0]["row_tile"] == p0 >> 7
