"""The host mirror of gemm8's tile runs (tests/gemm8_tiles.py) covers every output tile exactly once, and the row-tile counts
at which a workgroup first takes a second tile are what the mirror's table (and tests/test_encoder_gemm8_tiles_gpu.py's choice
of a 20-row-tile seam-free route) says."""
import numpy as np

from tests import gemm8_tiles as g8

LAUNCHES = [(9, 1, 0), (6, 1, 3), (3, 1, 0), (12, 2, 0)]   # QKV, the last layer's K | V, RESID, FFN-up
N_WG = (256, 304, 64)


def test_launch_table_matches_the_classes():
    assert sorted(g8.CLASSES.values()) == sorted(LAUNCHES)


def test_mirror_covers_every_tile_exactly_once():
    for n_wg in N_WG:
        for nx, ng, t0 in LAUNCHES:
            for mt_all in range(1, 2101):
                wg, seq, rt, ct, my = g8.tile_runs(mt_all, nx, ng, n_wg, t0)
                what = (n_wg, nx, ng, t0, mt_all)
                # every tile once: mt_all x nx pairs, rows inside [0, mt_all), columns inside [t0, t0 + nx), none twice
                assert len(rt) == mt_all * nx, what + (len(rt),)
                assert rt.min() >= 0 and rt.max() < mt_all and ct.min() >= t0 and ct.max() < t0 + nx, what
                assert (np.bincount(rt * nx + (ct - t0), minlength=mt_all * nx) == 1).all(), what
                assert wg.max() < n_wg and (seq < my).all(), what


def test_tile_map_lists_the_runs_in_order():
    for nx, ng, t0 in LAUNCHES:
        for mt_all in (1, 20, 21, 90, 173, 346):
            runs = g8.tile_map(mt_all, nx, ng, 256, t0)
            assert len(runs) == 256 and sum(len(r) for r in runs) == mt_all * nx
            assert all(r == sorted(r) for r in runs)           # a run walks its XCD's tiles in row-major order
            assert len({t for r in runs for t in r}) == mt_all * nx


def test_owners_inverts_the_map():
    for cls, (nx, ng, t0) in g8.CLASSES.items():
        own = g8.owners(173, nx, ng, 256, t0)
        runs = g8.tile_map(173, nx, ng, 256, t0)
        assert len(own) == 173 * nx
        for (rt, ct), (xcd, slot, seq, my) in own.items():
            assert runs[slot * 8 + xcd][seq] == (rt, ct) and len(runs[slot * 8 + xcd]) == my


def test_second_tile_thresholds():
    """81 / 25 / 21 (and 41 for the K | V-only QKV) on 256 workgroups: below them every workgroup has one tile."""
    assert g8.SECOND_TILE_AT == {"QKV": 25, "QKV_KV": 41, "RESID": 81, "GELU": 21}
    for cls, at in g8.SECOND_TILE_AT.items():
        for mt_all in range(1, at):
            assert g8.my_tiles_present(mt_all, cls, 256) == [1], (cls, mt_all)
        assert g8.my_tiles_present(at, cls, 256) == [1, 2], (cls, at)
    # so up to 20 row tiles no launch of a layer gives any workgroup a second tile
    assert min(g8.SECOND_TILE_AT.values()) == 21


def test_runs_of_the_gpu_batches():
    """The depths tests/test_encoder_gemm8_tiles_gpu.py's batches are built for (256 workgroups)."""
    want = {90: {"RESID": [1, 2], "QKV": [3, 4], "GELU": [4, 5]},
            173: {"RESID": [1, 2, 3], "QKV": [5, 6, 7], "GELU": [8, 9]},
            346: {"RESID": [4, 5], "QKV": [12, 13], "GELU": [16, 17]}}
    for mt_all, per in want.items():
        for cls, depths in per.items():
            assert g8.my_tiles_present(mt_all, cls, 256) == depths, (mt_all, cls, g8.my_tiles_present(mt_all, cls, 256))


def test_locate_names_wave_and_sub_band():
    geo = g8.Geometry(90, 256)
    # RESID, XCD 0 owns row tiles 0 .. 10 (33 tiles on 32 workgroups): local tile 32 = (row tile 10, column tile 2) is slot 0's second
    loc = geo.locate(10 * 256 + 128 + 64 + 2 * 16 + 5, 2 * 256 + 3 * 64 + 7, "RESID")
    assert loc == {"cls": "RESID", "row_tile": 10, "col_tile": 2, "xcd": 0, "slot": 0, "seq": 1, "my_tiles": 2, "wr": 1, "wc": 3, "i": 1, "mt": 2}
    assert geo.locate(0, 0, "RESID")["seq"] == 0 and geo.locate(0, 768, "QKV_KV")["col_tile"] == 3
    assert geo.row_seqs(10, "RESID") == (0, 0, 1) and geo.row_tile_kinds(10, "RESID") == {"first", "last"}


def test_packed_offsets_and_chunks():
    lens = [1, 32, 33, 512, 255, 257]
    off, total = g8.packed_offsets(lens)
    assert off.tolist() == [0, 32, 64, 128, 640, 896] and total == 1184
    assert g8.row_tiles_of(off, lens, 3) == [0, 1, 2] and g8.row_tiles_of(off, lens, 5) == [3, 4]
    ch = g8.chunks_by_tiles(lens, 2)
    assert ch[0][0] == 0 and ch[-1][1] == len(lens) and all(a[1] == b[0] for a, b in zip(ch, ch[1:]))
    for b0, b1 in ch:
        assert g8.packed_offsets(lens[b0:b1])[1] <= 2 * 256 or b1 - b0 == 1
