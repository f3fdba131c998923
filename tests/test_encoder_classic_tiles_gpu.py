"""The classic 128 x 128 kernel at its own geometry: every row of every layer where a persistent workgroup walks SEVERAL items.

gemm_bf16_nt_kernel<EPI, 2> (haconvdr_amd/csrc/encoder.hip) answers every forward of fewer than 9472 padded rows and the <s>-row
tail of the last layer in every bf16 family.  It starts two workgroups per CU; XCD x owns the run [n x / 8, n (x + 1) / 8) of the
launch's n items and its workgroups take every per_xcd-th of them.  In the last k-step of an item the first k-tile of the next
one is staged, for RESID with split-K that of (tile, slice) = (t / S, t % S).  The element-wise layer parity of
tests/test_encoder_layers_gpu.py runs this kernel on 16 row tiles (at most 384 items for 512 workgroups): none of that seam
code.  tests/classic_tiles.py mirrors the run arithmetic (tests/test_classic_tiles.py checks the mirror on the CPU).  Here:

  batches (synth.token_batch, trimmed; padded rows B x roundup(L, 32) = 9216, the family's last size), items per workgroup on
  256 CUs (asserted from the mirror):
    deep18   18 x 512, 60 row tiles of 128 (7584 packed rows, % 128 == 32: a partial last tile), both attention length classes
             QKV 2-3, FFN-up 2-3; with ksplit_pin = 3/6: out-proj 2-3, FFN-down 4-5; with 4/16: out-proj 2-3, FFN-down 11-12
    many72   72 x 128, lengths 1 .. 128, the last sequence 7 tokens short of its block edge: QKV 1-2, FFN-up 2-3

  Tier A (test_every_row_bit_equal_to_the_seam_free_route): the same sequences, in the same order, cut by
    classic_tiles.chunks_by_items into chunks in which no launch has more than 512 items -- no workgroup takes a second one,
    the route the `edges` batch pins against the fp64 reference -- must give the same BITS: rows, mean, rstd and norm of every
    valid token after stages -1, 0 and 1, and the final embedding of every sequence.  The big batch runs twice and must repeat
    its bits: a seam race need not be deterministic.  (a) ksplit = off on both batches: the QKV and FFN-up seams.
    (b) ksplit_pin = 3/6 and 4/16 on deep18 with ksplit = auto: RESID items across slice and tile seams; a pin holds at any row
    count, so big batch and chunks (then at most 14 / 5 row tiles) sum in the same order.  A mismatch is reported through
    classic_tiles.describe: row tile, column tile, xcd, slot, seq of my_items, wave, MFMA tile and half of the first differing
    elements, and the count of differing elements per seq value.  Attribution aid: chunks of <= 10 sequences take the
    attention query split (bit-identical by test_small_batch_attention_split_same_bits); if a mismatch sits in every tile of
    such a short chunk, run the chunks again with attn_qsplit = off before suspecting the GEMM.

  Tier B (test_late_item_rows_vs_fp64_reference): teacher-forced against oracle.ance_oracle, family "classic", on sequences of
    deep18 picked with the mirror so that for each of QKV, FFN-up and the pinned out-proj (S = 4) and FFN-down (S = 16) they
    hold rows of a workgroup's first, a middle and its last item, of the partial last row tile and of both sides of an XCD run
    boundary (asserted), with ksplit = off and with ksplit_pin = 4/16.  Bounds: test_encoder_layers_gpu.BOUNDS, imported,
    unchanged.

  Tail (test_tail_behind_many_sequences): one forward of 3000 sequences of L = 32 (96000 padded rows, one sub-batch): the last
    layer's FFN-up on the 3000 compact <s> rows is 24 row tiles x 24 column tiles = 576 items, a second item for 64 workgroups
    (from 2689 sequences on); chunks of 1000 have none.  Final embeddings bit-equal, the big forward twice, under gemm = 8phase
    (gemm8 in front of the tail) and gemm = classic (the 256 x 256 tile in front of it).

Measured on MI355X (256 CUs, 512 workgroups), this file 7 s (14 tests; the whole -m gpu suite with it: 572 passed in 9 min 05 s, so 1.3 % of that):
  Tier A: no differing bit -- deep18: 5 568 000 elements each of rows and of norm (= sum(len) x 768) and 7250 each of mean and of rstd
    per stage, against 3 chunks (ksplit = off), 5 (pin 3/6) and 17 (pin 4/16); many72: 3 527 424 and 4593 against 3 chunks; both
    weight sets; 18 / 72 final embeddings per case; the second run of every big batch repeats the first.  No defect found in
    the kernel's seam code, with or without slices.
  Tier B (sequences 0, 1, 9 and 17 of deep18, 1914 rows, on row tiles 0-7, 28-32 and 55-59; rel / bias at stages -1 | 0 | 1):
    std002  ksplit off  6.8e-8 / 1.3e-8 | 1.41e-4 / 4.1e-6 | 2.17e-4 / 5.8e-6     pin 4/16  6.8e-8 / 1.3e-8 | 1.41e-4 / 4.1e-6 | 2.43e-4 / 6.3e-6
    std010  ksplit off  6.8e-8 / 1.3e-8 | 9.88e-4 / 2.3e-5 | 1.47e-3 / 4.6e-5     pin 4/16  6.8e-8 / 1.3e-8 | 9.85e-4 / 2.3e-5 | 1.47e-3 / 3.6e-5
    -- the figures of the 16-row-tile batches (test_encoder_layers_gpu.BOUNDS' table: 1.6e-4 | 2.3e-4 and 9.4e-4 | 1.3e-3): rows of
    a workgroup's 12th item carry the error of rows of its first.  (std010, stage 1: 1.47e-3 is 1.13 x that table's worst, 0.54 x
    the bound.)
  Sensitivity, once, with a library built aside in which the seam stages item tile + 1 instead of tile + per_xcd (in bounds;
    only items with seq >= 1 start on a wrong first k-tile): all 14 tests fail -- Tier A with 5.3 M of deep18's 5.57 M
    stage-0 elements differing, Tier B beyond its bounds, the tail's embeddings differing in both families.
  Tail: 2 304 000 elements of 3000 embeddings, behind gemm8 and behind the 256 x 256 tile: no differing bit against 3 chunks of
    1000, the second run repeats the first.
"""
import time

import numpy as np
import pytest

from tests import classic_tiles as ct
from tests.test_encoder_layers_gpu import BOUNDS, DEFAULTS, EDGE_LENS, GEMM, STAGES, assert_within, encoder, figures, reference, weights

pytestmark = pytest.mark.gpu

MAX_ITEMS = 512                        # no launch of a chunk has more items than a 256-CU device has workgroups: no second item
FAMILY_ROWS = 9216                     # padded rows B x roundup(L, 32) up to which gemm = classic runs the 128 x 128 tile
# name -> (B, L, seed): see batch()
BATCHES = {"deep18": (18, 512, 0xDEE938), "many72": (72, 128, 0x3A2773)}
ROW_TILES = {"deep18": 60, "many72": None}       # many72: whatever its lengths give, at least 29
# route -> (options, the plan's ksplit, (S_out, S_down))
ROUTES = {"ksplit_off": ({"ksplit": "off"}, "1/1", (1, 1)),
          "pin_3_6": ({"ksplit": "auto", "ksplit_pin": "3/6"}, "3/6", (3, 6)),
          "pin_4_16": ({"ksplit": "auto", "ksplit_pin": "4/16"}, "4/16", (4, 16))}
RESTORE = {"gemm": DEFAULTS["gemm"], "graph": "auto", "attn": DEFAULTS["attn"], "ksplit": "auto", "ksplit_pin": "0/0"}
TIER_A = [("deep18", "ksplit_off"), ("many72", "ksplit_off"), ("deep18", "pin_3_6"), ("deep18", "pin_4_16")]
# my_items values per launch on 512 workgroups (tests/test_classic_tiles.py asserts the 60-row-tile ones from the mirror alone)
DEPTHS = {("deep18", "ksplit_off"): {"QKV": [2, 3], "GELU": [2, 3], "RESID_OUT": [1], "RESID_DOWN": [1]},
          ("deep18", "pin_3_6"): {"QKV": [2, 3], "GELU": [2, 3], "RESID_OUT": [2, 3], "RESID_DOWN": [4, 5]},
          ("deep18", "pin_4_16"): {"QKV": [2, 3], "GELU": [2, 3], "RESID_OUT": [2, 3], "RESID_DOWN": [11, 12]},
          ("many72", "ksplit_off"): {"QKV": [1, 2], "GELU": [2, 3], "RESID_OUT": [1], "RESID_DOWN": [1]}}
KINDS = ("std002", "std010")
TIER_B_ROUTES = ("ksplit_off", "pin_4_16")
TIER_B_CLASSES = {"ksplit_off": ("QKV", "GELU"), "pin_4_16": ("QKV", "GELU", "RESID_OUT", "RESID_DOWN")}
TIER_B_MAX = 9                         # sequences: half of deep18
KEYS = ("rows", "mean", "rstd", "norm")
TAIL_B, TAIL_L, TAIL_CHUNK, TAIL_SEED = 3000, 32, 1000, 0x7A113000
_BATCH, _REF = {}, {}


def n_workgroups():
    import torch
    return 2 * int(torch.cuda.get_device_properties(0).multi_processor_count)


def batch(name):
    """(ids int32 [B, L], mask int32 [B, L], lens), tokens from synth.token_batch, trimmed.
    deep18: 4 sequences of 1 .. 256 tokens among 13 of 449 .. 512, and the last one trimmed so that the packed rows end exactly
    32 rows into the 60th row tile, 7 tokens short of its block edge.
    many72: lengths 1 .. 128 as drawn; the last sequence 7 tokens short of its block edge."""
    from haconvdr_amd import synth
    if name in _BATCH:
        return _BATCH[name]
    B, L, seed = BATCHES[name]
    ids, _ = synth.token_batch(seed, B, L, fixed_len=L)               # body tokens in every position; trimmed to lens below
    lens = synth.token_batch(seed, B, L, min_len=1)[1].astype(np.int64)
    if name == "deep18":
        u = synth.uniform_u32(seed + 2, B).astype(np.int64)
        short = np.isin(np.arange(B), (2, 7, 11, 14))
        lens = np.where(short, 1 + u % 256, 449 + u % 64)
        target = (ROW_TILES[name] - 1) * ct.TILE + 32
        room = target - int(((lens[:-1] + 31) // 32 * 32).sum())      # rows left for the last sequence: a multiple of 32
        assert 32 <= room <= L and room % 32 == 0, (name, room)
        lens[-1] = room - 7
    else:
        lens[-1] = (lens[-1] + 31) // 32 * 32 - 7
    pos = np.arange(L)[None, :]
    ids = ids.copy()
    ids[pos == (lens[:, None] - 1)] = 2
    ids[:, 0] = np.where(lens > 1, 0, 2)
    ids[pos >= lens[:, None]] = 0
    mask = (pos < lens[:, None]).astype(np.int32)
    off, total = ct.packed_offsets(lens)
    tiles = (total + ct.TILE - 1) // ct.TILE
    assert B * ((L + 31) // 32 * 32) <= FAMILY_ROWS and lens.min() >= 1 and lens.max() <= L and lens[-1] % 32 == 25, (name, lens)
    straddle = sum(1 for b in range(B) if len(ct.row_tiles_of(off, lens, b)) > 1)
    if name == "deep18":
        assert 58 <= tiles <= 62 and tiles == ROW_TILES[name] and total % ct.TILE == 32, (name, total)
        assert (lens > 256).sum() >= 8 and (lens <= 256).sum() >= 4 and straddle * 4 >= B, (name, lens, straddle)   # both attention classes; seams inside sequences
    else:
        assert tiles >= 29 and lens.max() <= 128, (name, total)
    _BATCH[name] = (ids.astype(np.int32), mask, lens)
    return _BATCH[name]


def row_tiles(name):
    return (ct.packed_offsets(batch(name)[2])[1] + ct.TILE - 1) // ct.TILE


def geometry(name, route):
    """The mirror at the device's workgroup count, with the coverage this batch is built for asserted (256 CUs) or reported."""
    tiles, n_wg, (s_out, s_down) = row_tiles(name), n_workgroups(), ROUTES[route][2]
    geo = ct.Geometry(tiles, n_wg, s_out, s_down)
    present = {c: sorted({my for rt in range(tiles) for _, my in geo.row_seqs(rt, c)}) for c in geo.nx}
    print(f"{name} {route}: {tiles} row tiles on {n_wg} workgroups, my_items per launch {present}")
    if n_wg == 512:
        assert present == DEPTHS[(name, route)], (name, route, present)
    elif max(present["QKV"]) < 2:
        pytest.skip(f"{name}: on {n_wg} workgroups no QKV workgroup takes a second item ({present})")
    return geo


class pinned:
    """gemm = classic, graph off (every call the same plain launches), attn = stream and a split-K route; every option restored
    on the way out."""

    def __init__(self, enc, route, gemm="classic"):
        self.enc, self.opts = enc, {"gemm": GEMM.get(gemm, gemm), "graph": "off", "attn": "stream", **ROUTES[route][0]}

    def __enter__(self):
        try:
            for k, v in self.opts.items():
                self.enc.set_option(k, v)
        except Exception:
            self.__exit__()
            raise
        return self.enc

    def __exit__(self, *exc):
        for k, v in RESTORE.items():
            self.enc.set_option(k, v)


def check_plan(enc, route, what, gemm="classic128", stage=0):
    """(The embedding stage, stage = -1, stops in front of the layers: it plans no split-K and reports the last call's.)"""
    plan = dict(kv.split("=") for kv in enc.last_plan().split())
    assert plan["gemm"] == gemm and (stage < 0 or plan["ksplit"] == ROUTES[route][1]) and plan["sub_batches"] == "1" and plan["attn"] == "stream", (what, plan)
    return plan


def chunks_of(name, route):
    lens = batch(name)[2]
    s_out, s_down = ROUTES[route][2]
    chunks = ct.chunks_by_items(lens, min(MAX_ITEMS, n_workgroups()), s_out, s_down)
    for b0, b1 in chunks:           # seam-free, from the mirror: every launch of every chunk has depth 1
        tiles = (ct.packed_offsets(lens[b0:b1])[1] + ct.TILE - 1) // ct.TILE
        assert all(ct.depths(tiles, c, n_workgroups(), S) == [1] for c, S in (("QKV", 1), ("GELU", 1), ("RESID", s_out), ("RESID", s_down))), (b0, b1, tiles)
    return chunks


@pytest.mark.parametrize("name,route", TIER_A, ids=[f"{n}-{r}" for n, r in TIER_A])
@pytest.mark.parametrize("kind", KINDS)
def test_every_row_bit_equal_to_the_seam_free_route(kind, name, route):
    """Tier A: every valid row of stages -1, 0, 1 and every final embedding, big batch == chunks of <= 512 items per launch, bit
    for bit; the big batch twice."""
    t_start = time.time()
    geo = geometry(name, route)
    ids, mask, lens = batch(name)
    off, _ = ct.packed_offsets(lens)
    valid = mask.astype(bool)
    chunks = chunks_of(name, route)
    want = int(lens.sum()) * 768
    bad = {}
    with pinned(encoder(kind), route) as enc:
        for n in STAGES:
            big = enc.layer_state(ids, mask, n, normalized=True)
            plan = check_plan(enc, route, (kind, name, n), stage=n)
            again = enc.layer_state(ids, mask, n, normalized=True)
            unstable = [k for k in KEYS if not np.array_equal(ct.bits(big[k]), ct.bits(again[k]))]
            if unstable:
                d, _ = ct.diff_elements(big["norm"], again["norm"], valid)
                bad[(n, "run-to-run")] = (unstable, ct.describe(geo, off, *d))
            del again
            compared = dict.fromkeys(KEYS, 0)
            found = {k: [[], [], []] for k in KEYS}
            for b0, b1 in chunks:
                ch = enc.layer_state(ids[b0:b1], mask[b0:b1], n, normalized=True)
                check_plan(enc, route, (kind, name, n, b0, b1), stage=n)
                for k in KEYS:
                    d, cnt = ct.diff_elements(big[k][b0:b1], ch[k], valid[b0:b1])
                    compared[k] += cnt
                    if len(d[0]):
                        found[k][0].append(d[0] + b0)
                        found[k][1].append(d[1])
                        found[k][2].append(d[2] if len(d) == 3 else None)
                del ch
            assert compared["rows"] == compared["norm"] == want and compared["mean"] == compared["rstd"] == int(lens.sum()), (compared, want)
            print(f"{kind} {name} {route} stage {n}: {compared['rows']} elements of rows and of norm, {compared['mean']} of mean and of rstd compared "
                  f"against {len(chunks)} chunks; plan {plan['gemm']}" + (f" ksplit={plan['ksplit']}" if n >= 0 else ""))
            for k in KEYS:
                if found[k][0]:
                    b_, t_ = np.concatenate(found[k][0]), np.concatenate(found[k][1])
                    c_ = None if found[k][2][0] is None else np.concatenate(found[k][2])
                    bad[(n, k)] = ct.describe(geo, off, b_, t_, c_)
            del big
        emb = np.asarray(enc(ids, mask))
        check_plan(enc, route, (kind, name, "forward"))
        emb2 = np.asarray(enc(ids, mask))
        parts = []
        for b0, b1 in chunks:
            parts.append(np.asarray(enc(ids[b0:b1], mask[b0:b1])))
            check_plan(enc, route, (kind, name, "forward", b0, b1))
        parts = np.concatenate(parts)
    assert emb.shape == parts.shape == (len(lens), 768) and np.isfinite(emb).all()
    if not np.array_equal(ct.bits(emb), ct.bits(emb2)):
        bad[("forward", "run-to-run")] = np.nonzero((ct.bits(emb) != ct.bits(emb2)).any(1))[0].tolist()[:16]
    if not np.array_equal(ct.bits(emb), ct.bits(parts)):
        rows_ = np.nonzero((ct.bits(emb) != ct.bits(parts)).any(1))[0]
        bad[("forward", "embedding")] = {"sequences": rows_.tolist()[:16], "count": int(len(rows_)),
                                         "qkv_seqs_of_their_first_row_tile": [geo.row_seqs(int(off[b]) >> 7, "QKV") for b in rows_[:4]]}
    print(f"{kind} {name} {route} forward: {emb.size} elements of {len(lens)} embeddings compared; {time.time() - t_start:.1f} s")
    assert not bad, (kind, name, route, bad)


def tier_b_subset(name="deep18"):
    """(sequence indices, coverage): per launch class (the RESID ones with the slices of pin 4/16) the first sequences with rows
    in a row tile that holds a workgroup's first / a middle / its last item, in the partial last row tile, and on both sides of an
    XCD run boundary."""
    geo = ct.Geometry(row_tiles(name), n_workgroups(), *ROUTES["pin_4_16"][2])
    _, _, lens = batch(name)
    off, _ = ct.packed_offsets(lens)
    tiles_of = [ct.row_tiles_of(off, lens, b) for b in range(len(lens))]
    chosen, cover = [], {}

    def pick(cls, what, pred):
        for b in chosen + list(range(len(lens))):
            hit = [rt for rt in tiles_of[b] if pred(rt)]
            if hit:
                if b not in chosen:
                    chosen.append(b)
                cover[(cls, what)] = (b, hit[0])
                return
    for cls in TIER_B_CLASSES["pin_4_16"]:
        for kind_ in ("first", "middle", "last"):
            pick(cls, kind_, lambda rt, k=kind_, c=cls: k in geo.row_tile_kinds(rt, c))
        pick(cls, "partial", lambda rt: rt == geo.row_tiles - 1)
        depth = max(s for rt in range(geo.row_tiles) for s, _ in geo.row_seqs(rt, cls))
        for s in sorted({1, depth // 2, depth}):                   # and rows of a 2nd, a half-way and the deepest item of a run
            pick(cls, f"seq{s}", lambda rt, s=s, c=cls: any(q == s for q, _ in geo.row_seqs(rt, c)))
        below, above = geo.run_bounds(cls)[3]                      # the boundary between XCD 3's run and XCD 4's: the middle of the batch
        pick(cls, "below_bound", lambda rt, m=below: rt == m)
        pick(cls, "above_bound", lambda rt, m=above: rt == m)
    for b in range(len(lens)):                                     # the bias figure falls with the row count: no fewer rows than the `edges` batch BOUNDS were taken on
        if lens[chosen].sum() >= sum(EDGE_LENS):
            break
        if b not in chosen:
            chosen.append(b)
    return sorted(chosen), cover


def tier_b_states(kind, name, route):
    seqs, _ = tier_b_subset(name)
    ids, mask, _ = batch(name)
    out = {}
    with pinned(encoder(kind), route) as enc:
        for n in STAGES:
            st = enc.layer_state(ids, mask, n, normalized=True)
            check_plan(enc, route, (kind, name, route, n), stage=n)
            out[n] = {k: st[k][seqs].copy() for k in KEYS}
            del st
    return out


@pytest.mark.parametrize("route", TIER_B_ROUTES)
@pytest.mark.parametrize("kind", KINDS)
def test_late_item_rows_vs_fp64_reference(kind, route):
    """Tier B: the big batch's own rows in first, middle, last and partial tiles and at an XCD run boundary, each stage against the
    fp64 reference of that stage on the kernels' previous state, within the committed bounds."""
    name = "deep18"
    geo = geometry(name, route)
    seqs, cover = tier_b_subset(name)
    assert len(seqs) <= TIER_B_MAX, (name, seqs)
    ids, mask, lens = batch(name)
    off, _ = ct.packed_offsets(lens)
    rts = sorted({rt for b in seqs for rt in ct.row_tiles_of(off, lens, b)})
    if n_workgroups() == 512:
        for cls in TIER_B_CLASSES[route]:          # the coverage, from the mirror
            kinds_ = set().union(*(geo.row_tile_kinds(rt, cls) for rt in rts))
            below, above = geo.run_bounds(cls)[3]
            assert kinds_ == {"first", "middle", "last"} and geo.row_tiles - 1 in rts and below in rts and above in rts, (name, cls, kinds_, rts, cover)
            deepest = max(s for rt in rts for s, _ in geo.row_seqs(rt, cls))
            print(f"{name} {route} {cls}: {len(seqs)} sequences on row tiles {rts}; deepest seq {deepest}; XCD 3 | 4 boundary in row tiles {below} | {above}")
    states = tier_b_states(kind, name, route)
    valid = mask[seqs].astype(bool)
    sd = weights(kind)
    figs = {}
    for n in STAGES:       # (the reference of a stage depends on the route only through the kernels' own previous state)
        key = (kind, n) if n < 0 else (kind, route, n)
        if key not in _REF:
            _REF[key] = reference(sd, "classic", n, ids[seqs], mask[seqs], states)["norm"].numpy()
        figs[n] = figures(states[n]["norm"], _REF[key], valid)
    print(f"{kind} {name} {route} Tier B ({len(seqs)} sequences, {int(valid.sum())} rows): "
          + " | ".join(f"stage {n}: rel {f['rel']:.2e} bias {f['bias']:.2e}" for n, f in figs.items())
          + f"   bounds embed {BOUNDS[(kind, 'classic', 'embed')]} layer {BOUNDS[(kind, 'classic', 'layer')]}")
    assert_within(kind, "classic", figs, (kind, name, route, "late items"))


def tail_batch():
    from haconvdr_amd import synth
    if "tail" not in _BATCH:
        ids, lens = synth.token_batch(TAIL_SEED, TAIL_B, TAIL_L, min_len=1)
        mask = (np.arange(TAIL_L)[None, :] < lens[:, None]).astype(np.int32)
        assert lens.min() == 1 and lens.max() == TAIL_L
        _BATCH["tail"] = (ids.astype(np.int32), mask, lens.astype(np.int64))
    return _BATCH["tail"]


@pytest.mark.parametrize("gemm,family", [("8phase", "gemm8"), ("classic", "classic256")])
def test_tail_behind_many_sequences(gemm, family):
    """The last layer's <s> rows of 3000 sequences in one sub-batch (the compact FFN-up: 576 items, depth 1-2) against the same
    sequences in chunks of 1000 (168 items), bit for bit; the big forward twice."""
    n_wg = n_workgroups()
    big_d, chunk_d = (ct.depths((b + ct.TILE - 1) // ct.TILE, "TAIL_GELU", n_wg) for b in (TAIL_B, TAIL_CHUNK))
    print(f"tail: FFN-up my_items {big_d} at {TAIL_B} sequences, {chunk_d} at {TAIL_CHUNK}, on {n_wg} workgroups")
    if n_wg == 512:
        assert big_d == [1, 2] and chunk_d == [1], (big_d, chunk_d)
        assert ct.depths((TAIL_B + ct.TILE - 1) // ct.TILE, "TAIL_RESID", n_wg) == [1]
    elif max(big_d) < 2 or chunk_d != [1]:
        pytest.skip(f"on {n_wg} workgroups the tail's FFN-up has depths {big_d} / {chunk_d}")
    ids, mask, lens = tail_batch()
    enc = encoder("std002")
    with pinned(enc, "ksplit_off", gemm=gemm):
        emb = np.asarray(enc(ids, mask))
        check_plan(enc, "ksplit_off", (gemm, "big"), gemm=family)
        emb2 = np.asarray(enc(ids, mask))
        parts = []
        for b0 in range(0, TAIL_B, TAIL_CHUNK):
            parts.append(np.asarray(enc(ids[b0:b0 + TAIL_CHUNK], mask[b0:b0 + TAIL_CHUNK])))
            check_plan(enc, "ksplit_off", (gemm, b0), gemm=family)
        parts = np.concatenate(parts)
    assert emb.shape == parts.shape == (TAIL_B, 768) and np.isfinite(emb).all()
    geo_rt = (TAIL_B + ct.TILE - 1) // ct.TILE
    bad = {}
    for what, other in (("run-to-run", emb2), ("chunks", parts)):
        ne = ct.bits(emb) != ct.bits(other)
        if ne.any():
            rows_ = np.nonzero(ne.any(1))[0]
            # the compact row of sequence b is row b: who computed its FFN-up and RESID items
            bad[what] = {"sequences": rows_.tolist()[:16], "count": int(len(rows_)), "elements": int(ne.sum()),
                         "ffn_up_items_of_the_first": [ct.locate(int(rows_[0]), c * 128, "TAIL_GELU", 1, geo_rt, n_wg) for c in range(24)
                                                       if ct.locate(int(rows_[0]), c * 128, "TAIL_GELU", 1, geo_rt, n_wg)["seq"] >= 1],
                         "ffn_down_item_of_the_first_element": ct.locate(int(rows_[0]), int(np.nonzero(ne[rows_[0]])[0][0]), "TAIL_RESID", 1, geo_rt, n_wg)}
    print(f"tail {gemm}: {emb.size} elements of {TAIL_B} embeddings compared with {TAIL_B // TAIL_CHUNK} chunks of {TAIL_CHUNK}")
    assert not bad, (gemm, bad)
