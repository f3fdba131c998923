"""The host mirror of the rules that shape a captured forward (tests/graph_shapes.py), pinned at 256 CUs: the query split per
batch size, the family edge at 9472 rows, the eligibility edge at 16384 rows, the form of every shape of
tests/test_encoder_graph_shapes_gpu.py, and the batches that file calls them with."""
import numpy as np

from tests import classic_tiles as ct
from tests import graph_shapes as gs

N_CU = 256


def test_query_split_per_batch_size():
    want = {1: 16, 2: 8, 3: 4, 4: 4, 5: 4, 6: 2, 7: 2, 8: 2, 9: 2, 10: 2, 11: 1, 12: 1, 32: 1, 512: 1}
    assert {B: gs.att_qs(B, N_CU) for B in want} == want
    # one launch for both classes only with a split and a long class; without a long class there is one launch anyway
    assert gs.att_one(8, 512, N_CU) and gs.att_one(10, 257, N_CU) and not gs.att_one(8, 256, N_CU) and not gs.att_one(11, 512, N_CU)
    assert [gs.attention_launches(*s, N_CU) for s in ((8, 512), (8, 256), (12, 512), (256, 64))] == [1, 1, 2, 1]
    # other CU counts move the edges: 304 CUs keep the split up to 12 sequences, 80 CUs lose it at 4
    assert gs.att_qs(12, 304) == 2 and gs.att_qs(13, 304) == 1 and gs.att_qs(3, 80) == 2 and gs.att_qs(4, 80) == 1


def test_family_and_eligibility_edges():
    assert gs.pick_family(18, 512) == "classic128" and gs.pick_family(19, 512) == "gemm8"
    assert gs.Mp(18, 512) == 9216 and gs.Mp(19, 512) == 9728
    # the edge itself: 37 tiles of 256 rows = 9472 rows, whatever the lengths
    assert gs.pick_family(37, 256) == "gemm8" and gs.pick_family(36, 256) == "classic128" and gs.pick_family(289, 32) == "gemm8"
    assert gs.pick_family(288, 32) == "classic128" and gs.Mp(289, 32) == 9472
    assert gs.pick_family(19, 512, gemm="classic") == "classic256" and gs.pick_family(4, 512, gemm="8phase") == "gemm8"
    assert gs.pick_family(19, 512, precision="split") == "split128"
    assert gs.graph_eligible(32, 512) and not gs.graph_eligible(33, 512)
    assert gs.graph_eligible(512, 32) and not gs.graph_eligible(513, 32) and gs.graph_eligible(32, 481) and not gs.graph_eligible(33, 481)
    assert not gs.graph_eligible(8, 512, max_tokens=4095) and gs.graph_eligible(8, 512, max_tokens=4096)
    assert gs.pad_len(1) == 32 and gs.pad_len(257) == 288 and gs.Mc(256) == 256 and gs.Mc(257) == 512 and gs.Mc(19) == 256


def test_ksplit_of_the_small_shapes():
    """The serving shapes the existing capture tests hold (4 x 512: 2/3) and where the slices end."""
    assert gs.ksplit(4, 512, N_CU) == "2/3" and gs.ksplit(1, 64, N_CU) == "3/6"
    assert gs.ksplit(8, 512, N_CU) == "1/2" and gs.ksplit(12, 512, N_CU) == "1/1" and gs.ksplit(19, 512, N_CU) == "1/1"
    assert gs.ksplit(12, 512, N_CU, precision="split") == "1/1" and gs.ksplit(4, 512, N_CU, precision="split") == "2/2"


FORMS = {   # name: (rows, gemm, ksplit, attn_form, att_qs, att_one, Mc)
    "qs2_long": ("4096", "classic128", "1/2", "single", 2, True, 256),
    "qs2_short": ("2048", "classic128", "2/3", "single", 2, False, 256),
    "woven_c128": ("6144", "classic128", "1/1", "woven", 1, False, 256),
    "c128_top": ("9216", "classic128", "1/1", "woven", 1, False, 256),
    "g8_first": ("9728", "gemm8", "1/1", "woven", 1, False, 256),
    "g8_384": ("15360", "gemm8", "1/1", "woven", 1, False, 256),
    "g8_top": ("16384", "gemm8", "1/1", "woven", 1, False, 256),
    "g8_short64": ("16384", "gemm8", "1/1", "single", 1, False, 256),
    "g8_short32": ("16384", "gemm8", "1/1", "single", 1, False, 512),
}


def test_form_of_every_shape_of_the_gpu_file():
    assert set(FORMS) == set(gs.SHAPES)
    for name, (B, L) in gs.SHAPES.items():
        f = gs.form(B, L, N_CU)
        assert (f["rows"], f["gemm"], f["ksplit"], f["attn_form"], f["att_qs"], f["att_one"], f["Mc"]) == FORMS[name], (name, f)
        assert f["eligible"], name
    # the modes of the GPU file's section d
    assert gs.form(19, 512, N_CU, pooling="mean")["attn_form"] == "woven" and gs.form(19, 512, N_CU, n_layers=1)["attn_form"] == "single"
    assert gs.form(19, 512, N_CU, n_layers=1, pooling="mean")["attn_form"] == "woven"
    s = gs.form(12, 512, N_CU, precision="split")
    assert (s["gemm"], s["attn_form"], s["ksplit"]) == ("split128", "split", "1/1")
    # woven_c128 is the first batch size without a query split, and its classic-kernel workgroups take second items
    assert gs.att_qs(11, N_CU) == 1 and gs.att_qs(10, N_CU) == 2
    assert gs.form(12, 512, N_CU)["row_tiles_128"] == 48 >= ct.SECOND_ITEM_AT["QKV"] and ct.depths(48, "QKV", 2 * N_CU) == [1, 2]
    assert gs.form(8, 512, N_CU)["row_tiles_128"] == 32 and gs.form(18, 512, N_CU)["row_tiles_128"] == 72


def test_batches_of_the_calls():
    """Every call of a shape has lengths of its own; shapes with a long class see it empty in the third call and, but for a
    one-token sequence, alone in the fourth; the ragged 512-token shapes hold both classes when they are captured."""
    for name, (B, L) in gs.SHAPES.items():
        cs = gs.calls(name)
        assert len(cs) == 4
        for ids, mask, lens in cs:
            assert ids.shape == mask.shape == (B, L) and ids.dtype == mask.dtype == np.int32
            assert lens.min() >= 1 and lens.max() <= L and (mask.sum(1) == lens).all()
            assert (ids[:, 0][lens > 1] == 0).all() and (ids[np.arange(B), lens - 1] == 2).all() and (ids[mask == 0] == 0).all()
            assert gs.packed_rows(lens) <= gs.padded_rows(B, L)
        assert len({tuple(lens.tolist()) for _, _, lens in cs}) == 4 and len({ids.tobytes() for ids, _, _ in cs}) == 4, name
        if L > 256:
            for i in (0, 1):
                assert (cs[i][2] > 256).any() and (cs[i][2] <= 256).any(), (name, i)
            assert cs[2][2].max() <= 256, name
            assert (cs[3][2] == 1).sum() == 1 and cs[3][2][B // 2] == 1 and (np.delete(cs[3][2], B // 2) > 256).all(), name
    # woven_c128's last call packs enough rows for second items in the classic kernels, from the device's row count
    assert (gs.packed_rows(gs.calls("woven_c128")[3][2]) + 127) // 128 >= ct.SECOND_ITEM_AT["QKV"]
    # gemm8 runs on the packed rows while the family was chosen from the padded ones: the short calls pack far fewer
    assert gs.packed_rows(gs.calls("g8_first")[2][2]) < 9472 <= gs.padded_rows(19, 512)
    for name in gs.SHAPES:
        for _, _, lens in gs.calls(name):
            p = gs.pick_six(lens)
            assert len(set(p)) == 6 and lens[p[0]] == lens.min() and lens[p[1]] == lens.max() and min(p) >= 0 and max(p) < len(lens)
