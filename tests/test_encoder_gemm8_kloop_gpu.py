"""gemm8's k-loop at the start and the end of its DMA stream: the smallest runs.

gemm8_kernel (haconvdr_amd/csrc/gemm8.inc) keeps a stream of LDS-DMA pieces running ahead of its fragment reads: a prologue
stages the first two k-tiles, every loading part of the k-loop adds one k-tile per wave group, the tile seam tops the stream
up and drains it, and the stream ends (h_left) one or two k-tiles before the last tile's k-loop does.  The QKV and FFN-up
instantiations run one 64-MFMA phase per k-tile and wave group, in which group 0 stages the weights and group 1 the
activations; every counted wait of that loop is derived from its issue order.  tests/test_encoder_gemm8_tiles_gpu.py pins
the bits where a workgroup walks many tiles (90, 173 and 346 row tiles).  What it does not reach is the other end: launches
in which most workgroups have no tile, the stream is as long as ONE tile (its end follows its prologue within the same
k-loop), and a workgroup's very first seam.

  batches (synth.token_batch, L = 512, ragged, the last sequence trimmed; total rows % 256 == 32: a partial last tile), on
  256 CUs (asserted from the mirror tests/gemm8_tiles.py):
    one1      1 row tile    every launch: one XCD (FFN-up: two) holds all the tiles, 244 to 253 workgroups have none; one short sequence
    xcd8      8 row tiles   QKV, RESID: one row tile per XCD; no workgroup takes a second tile
    second22  22 row tiles  FFN-up: the first second tile of a workgroup (gemm8_tiles.SECOND_TILE_AT["GELU"] = 21); QKV: none
  The last layer's K | V-only QKV (n_tile0 = 3) runs in the forward of each of them.

  test_smallest_runs_bit_equal_to_one_sequence_at_a_time: rows, mean, rstd and norm of every valid token after stages -1, 0
    and 1, and every final embedding, must equal BIT FOR BIT the same sequences encoded one at a time ("a row's arithmetic
    does not depend on its tile or its sub-batch"); every batch runs twice and must repeat its bits.  A mismatch is named
    through the comparer and Geometry.locate of the tile tests: class, row tile, column tile, xcd, slot, seq, wave, sub-band.
  test_xcd8_vs_fp64_reference: the 8-tile batch teacher-forced against oracle.ance_oracle, family "gemm8", within
    test_encoder_layers_gpu.BOUNDS, imported unchanged -- so that the bit equality above does not compare the loop only with
    itself.

Measured on MI355X (256 CUs), this file 6 s (8 tests):
  bit equality: no differing bit -- 19 200 / 1 352 448 / 3 965 952 elements each of rows and of norm (1 / 7 / 19 sequences) per
    stage and weight set for one1 / xcd8 / second22, and every final embedding; the second run of every batch repeats the first.
  xcd8 against the fp64 reference (rel / bias at stages -1 | 0 | 1):
    std002  2.03e-5 / 4.83e-7 | 1.01e-3 / 4.16e-5 | 1.01e-3 / 4.26e-5     std010  2.03e-5 / 4.83e-7 | 1.56e-3 / 3.79e-5 | 1.85e-3 / 4.53e-5
    -- the figures of the larger batches (test_encoder_layers_gpu.BOUNDS' table).
"""
import time

import numpy as np
import pytest

from tests import gemm8_tiles as g8
from tests.test_encoder_gemm8_tiles_gpu import KEYS, KINDS, bits, check_plan, describe, diff_elements, n_workgroups, pinned
from tests.test_encoder_layers_gpu import BOUNDS, STAGES, assert_within, encoder, stage_figures, weights

pytestmark = pytest.mark.gpu

L = 512
BATCHES = {"one1": (1, 0x0E1), "xcd8": (8, 0x8CD8), "second22": (22, 0x5EC22)}      # name -> (row tiles, seed)
# my_tiles values per class on 256 workgroups, and how many of the 256 take no tile at all
DEPTHS = {"one1": {"RESID": [1], "QKV": [1], "GELU": [1], "QKV_KV": [1]},
          "xcd8": {"RESID": [1], "QKV": [1], "GELU": [1], "QKV_KV": [1]},
          "second22": {"RESID": [1], "QKV": [1], "GELU": [1, 2], "QKV_KV": [1]}}
IDLE = {"one1": {"RESID": 253, "QKV": 247, "GELU": 244, "QKV_KV": 250},
        "xcd8": {"RESID": 232, "QKV": 184, "GELU": 160, "QKV_KV": 208}}
_BATCH, _STATES = {}, {}


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
    _, total = g8.packed_offsets(lens)
    assert total == target and total % 256 == 32 and (total + 255) // 256 == tiles, (name, total)
    _BATCH[name] = (ids.astype(np.int32), mask, lens.astype(np.int64))
    return _BATCH[name]


def geometry(name):
    """The mirror at the device's workgroup count, with the coverage this batch is built for asserted (256 CUs) or reported."""
    tiles, n_wg = BATCHES[name][0], n_workgroups()
    maps = {c: g8.tile_map(tiles, nx, ng, n_wg, t0) for c, (nx, ng, t0) in g8.CLASSES.items()}
    present = {c: sorted({len(r) for r in m if r}) for c, m in maps.items()}
    idle = {c: sum(1 for r in m if not r) for c, m in maps.items()}
    print(f"{name}: {tiles} row tiles on {n_wg} workgroups, my_tiles per class {present}, workgroups without a tile {idle}")
    if n_wg == 256:
        assert present == DEPTHS[name], (name, present)
        assert tiles >= g8.SECOND_TILE_AT["GELU"] or idle == IDLE[name], (name, idle)
        if name == "second22":
            assert g8.SECOND_TILE_AT["GELU"] <= tiles < g8.SECOND_TILE_AT["QKV"]
    return g8.Geometry(tiles, n_wg)


def big_states(kind, name):
    """{stage: layer_state} of the whole batch, each stage run twice (the second run is compared and dropped), and the plan."""
    if (kind, name) not in _STATES:
        ids, mask, _ = batch(name)
        states, unstable = {}, {}
        with pinned(encoder(kind)) as enc:
            for n in STAGES:
                states[n] = enc.layer_state(ids, mask, n, normalized=True)
                check_plan(enc, (kind, name, n))
                again = enc.layer_state(ids, mask, n, normalized=True)
                unstable[n] = [k for k in KEYS if not np.array_equal(bits(states[n][k]), bits(again[k]))]
        _STATES[(kind, name)] = (states, unstable)
    return _STATES[(kind, name)]


@pytest.mark.parametrize("name", list(BATCHES))
@pytest.mark.parametrize("kind", KINDS)
def test_smallest_runs_bit_equal_to_one_sequence_at_a_time(kind, name):
    """Every valid row of stages -1, 0, 1 and every final embedding: the batch == its sequences one at a time, bit for bit; the
    batch twice."""
    t_start = time.time()
    geo = geometry(name)
    ids, mask, lens = batch(name)
    off, _ = g8.packed_offsets(lens)
    valid = mask.astype(bool)
    states, unstable = big_states(kind, name)
    bad = {}
    with pinned(encoder(kind)) as enc:
        for n in STAGES:
            big = states[n]
            if unstable[n]:
                bad[(n, "run-to-run")] = unstable[n]
            compared = dict.fromkeys(KEYS, 0)
            found = {k: [[], [], []] for k in KEYS}
            for b in range(len(lens)):
                one = enc.layer_state(ids[b:b + 1], mask[b:b + 1], n, normalized=True)
                check_plan(enc, (kind, name, n, b))
                for k in KEYS:
                    d, cnt = diff_elements(big[k][b:b + 1], one[k], valid[b:b + 1])
                    compared[k] += cnt
                    if len(d[0]):
                        found[k][0].append(d[0] + b)
                        found[k][1].append(d[1])
                        found[k][2].append(d[2] if len(d) == 3 else None)
            assert compared["rows"] == compared["norm"] == int(lens.sum()) * 768 and compared["mean"] == compared["rstd"] == int(lens.sum()), compared
            print(f"{kind} {name} stage {n}: {compared['rows']} elements of rows and of norm, {compared['mean']} of mean and of rstd compared "
                  f"against {len(lens)} single sequences")
            for k in KEYS:
                if found[k][0]:
                    b_, t_ = np.concatenate(found[k][0]), np.concatenate(found[k][1])
                    c_ = None if found[k][2][0] is None else np.concatenate(found[k][2])
                    bad[(n, k)] = describe(geo, off, b_, t_, c_)
        emb = np.asarray(enc(ids, mask))
        check_plan(enc, (kind, name, "forward"))
        emb2 = np.asarray(enc(ids, mask))
        parts = []
        for b in range(len(lens)):
            parts.append(np.asarray(enc(ids[b:b + 1], mask[b:b + 1])))
            check_plan(enc, (kind, name, "forward", b))
        parts = np.concatenate(parts)
    assert emb.shape == parts.shape == (len(lens), 768) and np.isfinite(emb).all()
    if not np.array_equal(bits(emb), bits(emb2)):
        bad[("forward", "run-to-run")] = np.nonzero((bits(emb) != bits(emb2)).any(1))[0].tolist()[:16]
    if not np.array_equal(bits(emb), bits(parts)):
        rows_ = np.nonzero((bits(emb) != bits(parts)).any(1))[0]
        bad[("forward", "embedding")] = {"sequences": rows_.tolist()[:16], "count": int(len(rows_)),
                                         "kv_seqs_of_their_first_row_tile": [geo.row_seqs(int(off[b]) >> 8, "QKV_KV") for b in rows_[:16]]}
    print(f"{kind} {name} forward: {emb.size} elements of {len(lens)} embeddings compared; {time.time() - t_start:.1f} s")
    assert not bad, (kind, name, bad)


@pytest.mark.parametrize("kind", KINDS)
def test_xcd8_vs_fp64_reference(kind):
    """The 8-tile batch, each stage against the fp64 reference of that stage on the kernels' previous state, within the committed
    bounds."""
    name = "xcd8"
    geometry(name)
    ids, mask, _ = batch(name)
    states, _ = big_states(kind, name)
    figs = stage_figures(weights(kind), "gemm8", ids, mask, states)
    print(f"{kind} {name}: " + " | ".join(f"stage {n}: rel {f['rel']:.2e} bias {f['bias']:.2e}" for n, f in figs.items())
          + f"   bounds embed {BOUNDS[(kind, 'gemm8', 'embed')]} layer {BOUNDS[(kind, 'gemm8', 'layer')]}")
    assert_within(kind, "gemm8", figs, (kind, name, "smallest runs"))
