"""gemm8 at its own geometry: every row of every layer where a persistent workgroup walks SEVERAL output tiles.

gemm8_kernel (haconvdr_amd/csrc/gemm8.inc) runs one workgroup per CU over a run of 256 x 256 tiles; its DMA stream runs on
across the tile seams and the RESID epilogue re-stages the next tile's first k-tiles from inside itself, behind counted
waits.  tests/test_encoder_layers_gpu.py observes every element, but on 8 and 40 row tiles, where no RESID workgroup ever
takes a second tile (tests/gemm8_tiles.py: the first second tile comes at 81 row tiles for RESID, 25 for QKV, 21 for
FFN-up); the tests that do reach the seams look at the <s> row's final embedding at 1 - cos < 1e-4.  Here:

  batches (synth.token_batch, L = 512, ragged, the last sequence trimmed; total rows % 256 == 32: a partial last tile;
  sequences straddle tile seams; both attention length classes), tiles per workgroup on 256 CUs (asserted from the mirror):
    seam90    90 row tiles   RESID 1-2    QKV 3-4     FFN-up 4-5    (K | V-only QKV of the last layer 2-3)
    odd173   173 row tiles   RESID 1-3    QKV 5-7     FFN-up 8-9
    deep346  346 row tiles   RESID 4-5    QKV 12-13   FFN-up 16-17

  Tier A (test_every_row_bit_equal_to_the_seam_free_route): the same sequences, in the same order, cut into chunks of at
    most 20 row tiles -- below every threshold above, the route the `edges` batch pins against the fp64 reference -- must give
    the same BITS: rows, mean, rstd and norm of every valid token after stages -1, 0 and 1, and the final embedding of every
    sequence (the last layer's K | V-only QKV and the <s> tail behind a multi-tile run).  "A row's arithmetic does not depend
    on its tile or its sub-batch" (test_large_batch_subbatching), applied to every row.  The big batch runs twice and must
    repeat its bits: a seam race need not be deterministic.  A mismatch is reported through gemm8_tiles.Geometry.locate:
    class, row tile, column tile, xcd, slot, seq of my_tiles, wave, half and sub-band of the first differing elements, and the
    count of differing elements per seq value.  Attribution aid: chunks of <= 10 sequences take the attention query split
    (bit-identical by test_small_batch_attention_split_same_bits); if a mismatch sits in every tile of such a short chunk,
    run the chunks again with attn_qsplit = off before suspecting gemm8.

  Tier B (test_late_tile_rows_vs_fp64_reference): teacher-forced against oracle.ance_oracle, family "gemm8", on sequences
    picked with the mirror from odd173 and deep346 so that for each of RESID, QKV and GELU they hold rows of a workgroup's
    first, a middle and its last tile (and of its 2nd, a half-way and its deepest one), of the partial last row tile and of
    both sides of an XCD share boundary (asserted).
    Bounds: test_encoder_layers_gpu.BOUNDS, imported, unchanged.

  Self-check (test_comparison_localises_a_stale_sub_band): on the host a 16 x 64 sub-band of a stage-0 state, in a tile with
    seq >= 1, is overwritten with the sub-band 16 rows above it (what a stale LDS region would leave).  Tier A's comparer must
    report exactly those 1024 elements and locate must name the tile, wave and sub-band; Tier B's rel with the corruption is
    printed next to its bound, and the corrupted state is carried through the fp64 reference to the sequence's embedding.

Measured on MI355X (256 CUs), this file 14 s (11 tests; the parent's -m gpu suite takes about 6.7 min):
  Tier A: no differing bit -- 16 419 840 / 32 020 224 / 64 031 232 elements each of rows and of norm (= sum(len) x 768) and 21 380 /
    41 693 / 83 374 each of mean and of rstd per stage for seam90 / odd173 / deep346, against 5 / 9 / 18 chunks, both weight sets;
    88 / 152 / 314 final embeddings; the second run of every big batch repeats the first.  deep346's host copies (0.5 GB per
    array) are fetched and dropped one stage at a time.  No defect found in gemm8's seam code.
  Tier B (11 + 11 sequences, 3386 + 3738 rows; rel / bias at stages -1 | 0 | 1):
    std002  odd173   1.3e-5 / 2.3e-7 | 1.02e-3 / 3.7e-5 | 1.01e-3 / 3.7e-5     deep346  1.8e-5 / 2.9e-7 | 1.02e-3 / 3.8e-5 | 1.01e-3 / 3.9e-5
    std010  odd173   1.3e-5 / 2.3e-7 | 1.48e-3 / 2.6e-5 | 1.58e-3 / 2.6e-5     deep346  1.8e-5 / 2.9e-7 | 1.63e-3 / 2.7e-5 | 1.61e-3 / 2.7e-5
    -- the figures of the edges and varlen batches (test_encoder_layers_gpu.BOUNDS' table): rows of a workgroup's 17th tile carry
    the error of rows of its first.
  Self-check (std002, odd173, stage 0; sequence 17, tokens 16..31, columns 0..63 = row tile 18, column tile 0, XCD 0, slot 22,
    seq 1 of 2, wave (1, 0), half 0, sub-band 3): the comparer reports the 1024 elements and nothing else.  Tier B over the 11
    sequences moves from rel 1.02e-3 / bias 3.7e-5 to 2.3e-2 / 3.7e-4 (bounds 2.1e-3 / 8.5e-5): on a subset of 3386 rows one
    stale sub-band IS beyond the bound (it holds another row's values, an error of ~1.4 x the rows' rms on 1024 of 2.6 M
    elements); by the same arithmetic it is 6.6e-3 over all of odd173's 41 693 rows and below the bound from about 540 k rows on.  Carried
    through the fp64 reference it moves that sequence's final embedding by 1 - cos = 4.2e-6: 24 x below the 1e-4 the CLS-level
    tests allow, and every other sequence's not at all.
"""
import time

import numpy as np
import pytest

from tests import gemm8_tiles as g8
from tests.test_encoder_layers_gpu import BOUNDS, DEFAULTS, GEMM, STAGES, assert_within, encoder, figures, reference, weights

pytestmark = pytest.mark.gpu

L = 512
CHUNK_TILES = 20                       # < min(gemm8_tiles.SECOND_TILE_AT.values()) = 21: no workgroup of any launch takes a second tile
BATCHES = {"seam90": (90, 0x5EA90), "odd173": (173, 0x0DD173), "deep346": (346, 0xDEE346)}      # name -> (row tiles, seed)
# my_tiles values per class on 256 workgroups (tests/test_gemm8_tiles.py asserts the same from the mirror alone)
DEPTHS = {"seam90": {"RESID": [1, 2], "QKV": [3, 4], "GELU": [4, 5], "QKV_KV": [2, 3]},
          "odd173": {"RESID": [1, 2, 3], "QKV": [5, 6, 7], "GELU": [8, 9], "QKV_KV": [3, 4, 5]},
          "deep346": {"RESID": [4, 5], "QKV": [12, 13], "GELU": [16, 17], "QKV_KV": [8, 9]}}
KINDS = ("std002", "std010")
TIER_B_BATCHES = ("odd173", "deep346")
TIER_B_CLASSES = ("RESID", "QKV", "GELU")
TIER_B_MAX = 14                        # sequences per batch: "about 24" over the two batches
KEYS = ("rows", "mean", "rstd", "norm")
_BATCH, _SUB, _REF = {}, {}, {}


def n_workgroups():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def batch(name):
    """(ids int32 [B, L], mask int32 [B, L], lens): ragged sequences whose packed rows end exactly 32 rows into the last tile."""
    from haconvdr_amd import synth
    if name in _BATCH:
        return _BATCH[name]
    tiles, seed = BATCHES[name]
    target = (tiles - 1) * g8.TILE + 32
    ids, lens = synth.token_batch(seed, target // 32, L, min_len=1)
    l32 = (lens.astype(np.int64) + 31) // 32 * 32
    B = int(np.searchsorted(np.cumsum(l32), target)) + 1          # the first sequence count that reaches the target
    ids, lens = ids[:B].copy(), lens[:B].copy()
    room = target - int(l32[:B - 1].sum())                        # rows left for the last sequence: a multiple of 32, >= 32
    assert room >= 32 and room % 32 == 0 and room <= l32[B - 1], (name, room)
    if room != l32[B - 1]:                                        # trim it (ragged: 7 tokens short of its block edge)
        lens[B - 1] = room - 7
        ids[B - 1, lens[B - 1] - 1] = 2
        ids[B - 1, lens[B - 1]:] = 0
    mask = (np.arange(L)[None, :] < lens[:, None]).astype(np.int32)
    off, total = g8.packed_offsets(lens)
    assert total == target and total % 256 == 32 and (total + 255) // 256 == tiles, (name, total)
    straddle = sum(1 for b in range(B) if len(g8.row_tiles_of(off, lens, b)) > 1)
    assert straddle >= tiles // 4 and (lens <= 256).sum() >= 8 and (lens > 256).sum() >= 8, (name, straddle)   # seams inside sequences; both attention classes
    _BATCH[name] = (ids.astype(np.int32), mask, lens.astype(np.int64))
    return _BATCH[name]


def geometry(name):
    """The mirror at the device's workgroup count, with the coverage this batch is built for asserted (256 CUs) or reported."""
    tiles, n_wg = BATCHES[name][0], n_workgroups()
    present = {c: g8.my_tiles_present(tiles, c, n_wg) for c in g8.CLASSES}
    print(f"{name}: {tiles} row tiles on {n_wg} workgroups, my_tiles per class {present}")
    if n_wg == 256:
        assert present == DEPTHS[name], (name, present)
    elif max(present["RESID"]) < 2:
        pytest.skip(f"{name}: on {n_wg} workgroups no RESID workgroup takes a second tile ({present})")
    return g8.Geometry(tiles, n_wg)


class pinned:
    """gemm = 8phase, graph off (every call the same plain launches), restored on the way out."""

    def __init__(self, enc):
        self.enc = enc

    def __enter__(self):
        self.enc.set_option("gemm", GEMM["gemm8"])
        self.enc.set_option("graph", "off")
        return self.enc

    def __exit__(self, *exc):
        self.enc.set_option("gemm", DEFAULTS["gemm"])
        self.enc.set_option("graph", "auto")


def check_plan(enc, what):
    plan = dict(kv.split("=") for kv in enc.last_plan().split())
    assert plan["gemm"] == "gemm8" and plan["sub_batches"] == "1", (what, plan)
    return plan


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def diff_elements(a, b, valid):
    """The comparer of Tier A: index arrays of the valid tokens' elements whose BITS differ between two state arrays over
    [n, L, 768] (or [n, L]: the statistics), and the number of elements compared."""
    v = np.asarray(valid, bool)
    ne = bits(a) != bits(b)
    ne &= v[..., None] if ne.ndim == 3 else v
    return (np.nonzero(ne) if ne.any() else tuple(np.zeros(0, np.int64) for _ in range(ne.ndim))), int(v.sum()) * (a.shape[2] if a.ndim == 3 else 1)


def describe(geo, off, b, t, c=None, limit=6):
    """Who computed the differing elements (sequence b, token t, feature c; c = None: a row statistic) of a layer's output, the
    RESID launch of FFN-down: the first `limit` through locate, with the seq values of the row tile's QKV and GELU column tiles
    (an upstream launch spoils whole rows), and the count of differing elements per RESID seq value."""
    row = np.asarray(off)[np.asarray(b)] + np.asarray(t)
    col = np.zeros_like(row) if c is None else np.asarray(c)
    first = []
    for r, cc, bb, tt in list(zip(row.tolist(), col.tolist(), np.asarray(b).tolist(), np.asarray(t).tolist()))[:limit]:
        loc = geo.locate(r, cc, "RESID")
        loc.update(sequence=bb, token=tt, packed_row=r, column=None if c is None else cc,
                   qkv_seqs=geo.row_seqs(r >> 8, "QKV"), gelu_seqs=geo.row_seqs(r >> 8, "GELU"))
        first.append(loc)
    seqs = np.array([geo.own["RESID"][(r >> 8, cc >> 8)][2] for r, cc in zip(row.tolist(), col.tolist())], np.int64)
    per_seq = {int(s): int(n) for s, n in zip(*np.unique(seqs, return_counts=True))}
    return {"differing": int(len(row)), "per_resid_seq": per_seq, "rows": int(len(np.unique(row))), "first": first}


def stash(kind, name, n, state, seqs):
    sub = _SUB.setdefault((kind, name), {})
    sub[n] = {k: state[k][seqs].copy() for k in KEYS}


def subset_states(kind, name):
    """{stage: state} of the Tier B sequences of a batch, sliced from the big batch's own states (Tier A leaves them behind;
    fetched here when this test runs alone)."""
    seqs, _ = tier_b_subset(name)
    if len(_SUB.get((kind, name), {})) < len(STAGES):
        ids, mask, _ = batch(name)
        with pinned(encoder(kind)) as enc:
            for n in STAGES:
                st = enc.layer_state(ids, mask, n, normalized=True)
                check_plan(enc, (kind, name, n))
                stash(kind, name, n, st, seqs)
                del st
    return _SUB[(kind, name)]


def tier_b_subset(name):
    """(sequence indices, coverage): per class of TIER_B_CLASSES the first sequences with rows in a tile that is a workgroup's
    first / a middle one / its last, in the partial last row tile, and on both sides of an XCD share boundary."""
    geo = g8.Geometry(BATCHES[name][0], n_workgroups())
    _, _, lens = batch(name)
    off, _ = g8.packed_offsets(lens)
    tiles_of = [g8.row_tiles_of(off, lens, b) for b in range(len(lens))]
    chosen, cover = [], {}

    def pick(cls, what, pred):
        for b in chosen + list(range(len(lens))):
            hit = [rt for rt in tiles_of[b] if pred(rt)]
            if hit:
                if b not in chosen:
                    chosen.append(b)
                cover[(cls, what)] = (b, hit[0])
                return
    for cls in TIER_B_CLASSES:
        for kind_ in ("first", "middle", "last"):
            pick(cls, kind_, lambda rt, k=kind_, c=cls: k in geo.row_tile_kinds(rt, c))
        pick(cls, "partial", lambda rt: rt == geo.mt_all - 1)
        depth = max(s for rt in range(geo.mt_all) for s in geo.row_seqs(rt, cls))
        for s in sorted({1, depth // 2, depth - 1, depth}):           # and rows of a 2nd, a half-way, the last-but-one and the deepest tile of a run
            pick(cls, f"seq{s}", lambda rt, s=s, c=cls: s in geo.row_seqs(rt, c))
        bounds = g8.share_bounds(geo.mt_all, cls)
        for tag, bound in (("", bounds[len(bounds) // 2]), ("2", bounds[0])):   # the boundary in the middle of the batch, and the first one
            pick(cls, "below_bound" + tag, lambda rt, m=bound: rt == m - 1)
            pick(cls, "above_bound" + tag, lambda rt, m=bound: rt == m)
    return sorted(chosen), cover


@pytest.mark.parametrize("name", list(BATCHES))
@pytest.mark.parametrize("kind", KINDS)
def test_every_row_bit_equal_to_the_seam_free_route(kind, name):
    """Tier A: every valid row of stages -1, 0, 1 and every final embedding, big batch == chunks of <= 20 row tiles, bit for bit;
    the big batch twice."""
    t_start = time.time()
    geo = geometry(name)
    ids, mask, lens = batch(name)
    off, total = g8.packed_offsets(lens)
    valid = mask.astype(bool)
    chunks = g8.chunks_by_tiles(lens, CHUNK_TILES)
    assert all(g8.packed_offsets(lens[b0:b1])[1] <= CHUNK_TILES * g8.TILE for b0, b1 in chunks), chunks
    seqs_b = tier_b_subset(name)[0] if name in TIER_B_BATCHES else []
    want = int(lens.sum()) * 768
    bad = {}
    with pinned(encoder(kind)) as enc:
        for n in STAGES:
            big = enc.layer_state(ids, mask, n, normalized=True)
            plan = check_plan(enc, (kind, name, n))
            again = enc.layer_state(ids, mask, n, normalized=True)
            unstable = [k for k in KEYS if not np.array_equal(bits(big[k]), bits(again[k]))]
            if unstable:
                d, _ = diff_elements(big["norm"], again["norm"], valid)
                bad[(n, "run-to-run")] = (unstable, describe(geo, off, *d))
            del again
            if seqs_b:
                stash(kind, name, n, big, seqs_b)
            compared = dict.fromkeys(KEYS, 0)
            found = {k: [[], [], []] for k in KEYS}
            for b0, b1 in chunks:
                ch = enc.layer_state(ids[b0:b1], mask[b0:b1], n, normalized=True)
                check_plan(enc, (kind, name, n, b0, b1))
                for k in KEYS:
                    d, cnt = diff_elements(big[k][b0:b1], ch[k], valid[b0:b1])
                    compared[k] += cnt
                    if len(d[0]):
                        found[k][0].append(d[0] + b0)
                        found[k][1].append(d[1])
                        found[k][2].append(d[2] if len(d) == 3 else None)
                del ch
            assert compared["rows"] == compared["norm"] == want and compared["mean"] == compared["rstd"] == int(lens.sum()), (compared, want)
            print(f"{kind} {name} stage {n}: {compared['rows']} elements of rows and of norm, {compared['mean']} of mean and of rstd compared "
                  f"against {len(chunks)} chunks; plan {plan['gemm']} sub_batches={plan['sub_batches']}")
            for k in KEYS:
                if found[k][0]:
                    b_, t_ = np.concatenate(found[k][0]), np.concatenate(found[k][1])
                    c_ = None if found[k][2][0] is None else np.concatenate(found[k][2])
                    bad[(n, k)] = describe(geo, off, b_, t_, c_)
            del big
        emb = np.asarray(enc(ids, mask))
        plan = check_plan(enc, (kind, name, "forward"))
        emb2 = np.asarray(enc(ids, mask))
        parts = []
        for b0, b1 in chunks:
            parts.append(np.asarray(enc(ids[b0:b1], mask[b0:b1])))
            check_plan(enc, (kind, name, "forward", b0, b1))
        parts = np.concatenate(parts)
    assert emb.shape == parts.shape == (len(lens), 768) and np.isfinite(emb).all()
    if not np.array_equal(bits(emb), bits(emb2)):
        bad[("forward", "run-to-run")] = np.nonzero((bits(emb) != bits(emb2)).any(1))[0].tolist()[:16]
    if not np.array_equal(bits(emb), bits(parts)):
        rows_ = np.nonzero((bits(emb) != bits(parts)).any(1))[0]
        bad[("forward", "embedding")] = {"sequences": rows_.tolist()[:16], "count": int(len(rows_)),
                                         "kv_seqs_of_their_first_row_tile": [geo.row_seqs(int(off[b]) >> 8, "QKV_KV") for b in rows_[:16]]}
    print(f"{kind} {name} forward: {emb.size} elements of {len(lens)} embeddings compared; plan {plan['gemm']} sub_batches={plan['sub_batches']}; "
          f"{time.time() - t_start:.1f} s")
    assert not bad, (kind, name, bad)


@pytest.mark.parametrize("name", TIER_B_BATCHES)
@pytest.mark.parametrize("kind", KINDS)
def test_late_tile_rows_vs_fp64_reference(kind, name):
    """Tier B: the big batch's own rows in first, middle, last and partial tiles and at a share boundary, each stage against the
    fp64 reference of that stage on the kernels' previous state, within the committed bounds."""
    geo = geometry(name)
    seqs, cover = tier_b_subset(name)
    assert len(seqs) <= TIER_B_MAX, (name, seqs)
    _, _, lens = batch(name)
    off, _ = g8.packed_offsets(lens)
    for cls in TIER_B_CLASSES:          # the coverage, from the mirror
        rts = sorted({rt for b in seqs for rt in g8.row_tiles_of(off, lens, b)})
        kinds_ = set().union(*(geo.row_tile_kinds(rt, cls) for rt in rts))
        bound = cover[(cls, "above_bound")][1]
        assert kinds_ == {"first", "middle", "last"} and geo.mt_all - 1 in rts and bound in g8.share_bounds(geo.mt_all, cls) \
            and bound in rts and bound - 1 in rts, (name, cls, kinds_, rts, cover)
        deepest = max(max(geo.row_seqs(rt, cls)) for rt in rts)
        print(f"{name} {cls}: {len(seqs)} sequences on row tiles {rts}; deepest seq {deepest}; share boundary {bound}")
    figs = tier_b_figures(kind, name)
    print(f"{kind} {name} Tier B: " + " | ".join(f"stage {n}: rel {f['rel']:.2e} bias {f['bias']:.2e}" for n, f in figs.items())
          + f"   bounds embed {BOUNDS[(kind, 'gemm8', 'embed')]} layer {BOUNDS[(kind, 'gemm8', 'layer')]}")
    assert_within(kind, "gemm8", figs, (kind, name, "late tiles"))


def tier_b_reference(kind, name, n):
    if (kind, name, n) not in _REF:
        seqs, _ = tier_b_subset(name)
        ids, mask, _ = batch(name)
        _REF[(kind, name, n)] = reference(weights(kind), "gemm8", n, ids[seqs], mask[seqs], subset_states(kind, name))["norm"].numpy()
    return _REF[(kind, name, n)]


def tier_b_figures(kind, name):
    seqs, _ = tier_b_subset(name)
    valid = batch(name)[1][seqs].astype(bool)
    states = subset_states(kind, name)
    return {n: figures(states[n]["norm"], tier_b_reference(kind, name, n), valid) for n in STAGES}


def test_comparison_localises_a_stale_sub_band():
    """Self-check, host only: a stale 16 x 64 sub-band in a seq >= 1 tile of a stage-0 state.  (1) the comparer reports exactly its
    1024 elements and locate names tile, wave and sub-band; (2) Tier B's rel with it, next to the bound; (3) what it does to the
    sequence's final embedding through the fp64 reference (1 - cos, next to the 1e-4 of the CLS-level tests)."""
    from oracle import ance_oracle
    kind, name, n = "std002", "odd173", 0
    geo = geometry(name)
    seqs, _ = tier_b_subset(name)
    ids, mask, lens = batch(name)
    off, _ = g8.packed_offsets(lens)
    clean = subset_states(kind, name)[n]
    valid = mask[seqs].astype(bool)
    target = None
    for k, b in enumerate(seqs):        # the first sub-band of a seq >= 1 tile whose 16 rows and the 16 above are valid, no <s> row, all 1024 elements change
        for t0 in range(16, int(lens[b]) - 15, 16):
            p0 = int(off[b]) + t0
            if (p0 & 255) < 16:
                continue                # the 16 rows above would belong to another tile
            for c0 in range(0, 768, 64):
                loc = geo.locate(p0, c0, "RESID")
                src, dst = (slice(t0 - 16, t0), slice(c0, c0 + 64)), (slice(t0, t0 + 16), slice(c0, c0 + 64))
                if loc["seq"] >= 1 and all((bits(clean[key][k][src]) != bits(clean[key][k][dst])).all() for key in ("rows", "norm")):
                    target = (k, b, t0, c0, loc)
                    break
            if target:
                break
        if target:
            break
    assert target, "no sub-band of the subset qualifies"
    k, b, t0, c0, loc = target
    stale = {key: clean[key].copy() for key in KEYS}
    for key in ("rows", "norm"):
        stale[key][k, t0:t0 + 16, c0:c0 + 64] = clean[key][k, t0 - 16:t0, c0:c0 + 64]
    # (1) the comparer and locate
    for key in ("rows", "norm"):
        d, cnt = diff_elements(stale[key], clean[key], valid)
        assert cnt == int(valid.sum()) * 768 and len(d[0]) == 1024, (key, len(d[0]))
        assert set(d[0].tolist()) == {k} and set(d[1].tolist()) == set(range(t0, t0 + 16)) and set(d[2].tolist()) == set(range(c0, c0 + 64)), key
        rep = describe(geo, off, np.asarray(seqs)[d[0]], d[1], d[2], limit=1024)
        assert rep["differing"] == 1024 and rep["per_resid_seq"] == {loc["seq"]: 1024} and rep["rows"] == 16, rep
        named = {(f["row_tile"], f["col_tile"], f["xcd"], f["slot"], f["seq"], f["my_tiles"], f["wr"], f["wc"], f["i"], f["mt"]) for f in rep["first"]}
        assert named == {(loc["row_tile"], loc["col_tile"], loc["xcd"], loc["slot"], loc["seq"], loc["my_tiles"], loc["wr"], loc["wc"], loc["i"], loc["mt"])}, named
    for key in ("mean", "rstd"):
        assert len(diff_elements(stale[key], clean[key], valid)[0][0]) == 0
    print(f"injected: sequence {b} tokens {t0}..{t0 + 15} columns {c0}..{c0 + 63} -> {loc}")
    # (2) Tier B's figure with the stale sub-band (a measurement: it may well stay inside the bound)
    ref = tier_b_reference(kind, name, n)
    f_clean, f_stale = figures(clean["norm"], ref, valid), figures(stale["norm"], ref, valid)
    rb, bb = BOUNDS[(kind, "gemm8", "layer")]
    print(f"Tier B over the {len(seqs)} sequences ({int(valid.sum())} rows): rel {f_clean['rel']:.3e} clean, {f_stale['rel']:.3e} stale (bound {rb:.1e}); "
          f"bias {f_clean['bias']:.3e} clean, {f_stale['bias']:.3e} stale (bound {bb:.1e})")
    assert np.isfinite(f_stale["rel"]) and np.isfinite(f_stale["bias"])
    # (3) the embedding of that sequence, fp64 reference from the clean and from the stale state
    sd = weights(kind)
    one = slice(k, k + 1)
    embs = []
    for st in (clean, stale):
        st1 = ance_oracle.ance_layer(sd, 1, {key: st[key][one] for key in KEYS}, mask[seqs][one], "gemm8")
        embs.append(ance_oracle.ance_tail(sd, 2, st1, mask[seqs][one], "gemm8").numpy()[0])
    cos = float(embs[0] @ embs[1] / (np.linalg.norm(embs[0]) * np.linalg.norm(embs[1])))
    print(f"the stale sub-band moves the embedding of sequence {b} (length {int(lens[b])}) by 1 - cos = {1 - cos:.3e} (the CLS-level tests allow 1e-4)")
    assert np.isfinite(cos)
