"""precision = split, teacher-forced per stage (tests/split_parity.teacher_forced: the kernels' layer_state / forward against the
unrounded fp64 chain on the kernels' own previous state), at the split kernels' OWN geometry -- what the one tight batch of
tests/test_encoder_precision_gpu.py (lengths at the bf16 kernels' edges, 1472 packed rows, default options) does not reach:

  A  attention_split_kernel's 64-key chunks and 128-row query parts (SPLIT_EDGES: both sides of 64, 96, 128, 160, 384, ...;
     1, 2, 3 active waves in a part; the redirected DMA pieces of a half-filled last chunk), L = 100 and 200 (L32 = 128, 224:
     query parts beyond len32 return), and gemm_split_nt_kernel's persistent tile loop (3104 packed rows: 25 x 18 QKV tiles,
     every workgroup takes the `tile += per_xcd` step and the prefetch across a tile seam);
  B  split-K: off, every pinned slice count up to 4 / 16 (ln_split_rows_kernel adds up to 15 partial buffers; the RESID
     epilogue's `partial` branch; the prefetch across a slice seam), the model's own choice on 1 x 64 and 4 x 512;
  C  the compact <s> tail on one, two and three 128-row tiles (B = 64, 65, 129, 257), head_ns 8 -> 64, varlen40 (~10 k rows), the
     serving shapes through eager-first, capture and replay;
  D  peaked logits (the moving softmax reference: ballot branch, delta, rescaling of lsum and o) and outlier channels (large hi,
     where lo carries real weight);
  E  the self-check: every mutation of the reference, key_chunk (a wrong masked-step condition of the 64-key chunk loop) among
     them, lies >= 3 x beyond the bounds on the SPLIT_EDGES batch.

Bounds.  Embedding stage and layers of the std-0.08 / std-0.12 weights: the committed LAYER_BOUNDS of
tests/test_encoder_precision_gpu.py, on any batch (the emulated figure does not depend on the batch: 1.103e-5 / 1.102e-5 at std
0.08, 1.671e-5 / 1.670e-5 at std 0.12 on the two edge batches).  Everything else -- the peaked and outlier layers, every tail on a
batch other than `edges` -- is split_parity.EMUL_FACTOR (2.6) x E_EMUL below: the figure of the split-faithful fp64 reference
(oracle.ance_oracle family="split") against the unrounded chain, computed on the CPU from the reference alone and re-derived
by tests/test_encoder_precision.py::test_recorded_emulation_constants_match_the_split_faithful_reference.  The embedding stage
has no rounded operand (E_emul = 0): its bound is LAYER_BOUNDS' 1.4e-7 = 2^-23 + 2^-24, an fp32 LayerNorm's own rounding,
for every recipe (a relative figure: the outlier gain scales kernel and reference alike).  No bound comes from what this file
measures.

The model's split-K choice (encoder.hip pick_ksplit, with the split family's one workgroup slot per CU) goes by the PADDED rows B x L32 of a call, not the packed rows: on a
256-CU part the 8 x 512 `edges` batch and SPLIT_EDGES run 1/1, L = 100 runs 2/3, 1 x 64 runs 3/6 and 4 x 512 runs 2/2
(model_ksplit below mirrors the rule; every case asserts what ran from last_plan()).

Measured on MI355X, first run of this file (rel: embed / layer 0 / layer 1 / tail; the ksplit that ran; bound in brackets):
  every case: embed 6.7e-8 ... 6.8e-8 (1.4e-7)
  A std008 (layers 2.9e-5): split_edges 1/1 1.428e-5 / 1.030e-5 / 8.60e-6 (1.80e-5); L100 2/3 1.418e-5 / 1.097e-5 / 9.54e-6 (1.91e-5);
           L200 1/1 1.436e-5 / 1.050e-5 / 9.09e-6 (1.85e-5)
    std012 (layers 4.4e-5): split_edges 1/1 2.173e-5 / 1.793e-5 / 1.464e-5 (3.01e-5); L100 2/3 2.032e-5 / 1.798e-5 / 1.388e-5 (2.51e-5);
           L200 1/1 2.148e-5 / 1.769e-5 / 1.405e-5 (2.60e-5)
  B edges, off and the seven pins: std008 layer 0 1.417e-5 ... 1.419e-5, layer 1 1.020e-5 ... 1.035e-5, tail 9.28e-6 ... 9.50e-6 (2.9e-5);
           std012 layer 0 2.196e-5 ... 2.197e-5, layer 1 1.791e-5 ... 1.819e-5, tail 1.367e-5 ... 1.541e-5 (4.5e-5)
    split_edges 4/16: std008 1.426e-5 / 1.037e-5 / 8.83e-6, std012 2.173e-5 / 1.799e-5 / 1.511e-5
    by the model: 1 x 64 ran 3/6: 1.827e-5 / 1.565e-5 / 1.434e-5; 4 x 512 ran 2/2: 2.197e-5 / 1.864e-5 / 1.633e-5
  C tails, 3 layers / 1 layer (bound = 2.6 x E_EMUL): b64 1.426e-5 / 1.969e-5, b65 1.450e-5 / 1.926e-5, b129 1.347e-5 / 1.851e-5,
    b257 1.356e-5 / 1.852e-5, varlen40 1.466e-5 / 2.004e-5, 1 x 64 1.434e-5 / 2.582e-5, 1 x 512 1.254e-5 / 1.170e-5, 2 x 64 1.335e-5 /
    1.571e-5, 4 x 512 1.633e-5 / 2.056e-5 (eager, capture and replay bit-equal): 1.08 ... 1.46 x E_emul
  D peaked 1.080e-4 / 1.004e-4 / 8.50e-5 (2.13e-4 / 1.90e-4 / 1.35e-4); outlier 3.73e-5 / 1.89e-5 / 2.00e-5 (7.78e-5 / 3.61e-5 / 2.92e-5)
  E weakest separations: gelu_tanh 4.3 / 4.4 / 7.5 (std008), 1.9 / 1.9 / 2.9 (std012); logits 53 ... 163; key_chunk 461 ... 26936
The kernels sit 1.1 ... 1.4 x above the emulation on the layers of every std-weight case (1.29 ... 1.33 on the four cells the bounds
come from), at most 1.8 x anywhere (the outlier tail): no case here needed a margin of its own, and no defect of split.inc / the split layer bodies (layer_split, tail_split) showed.
"""
import numpy as np
import pytest

from tests import split_parity as sp
from tests.test_encoder_precision_gpu import LAYER_BOUNDS, NOT_SEPARABLE

pytestmark = pytest.mark.gpu

STD = {"std008": 0.08, "std012": 0.12}
# E_emul, (recipe, layers of the encoder, batch) -> {(stage, n): rel(family "split", family None)}: CPU, reference alone
E_EMUL = {
    # A: tails of the edge batches
    ("std008", 3, "split_edges"): {("tail", 2): 6.925e-6}, ("std012", 3, "split_edges"): {("tail", 2): 1.156e-5},
    ("std008", 3, "L100"): {("tail", 2): 7.361e-6}, ("std012", 3, "L100"): {("tail", 2): 9.638e-6},
    ("std008", 3, "L200"): {("tail", 2): 7.117e-6}, ("std012", 3, "L200"): {("tail", 2): 9.996e-6},
    # C: tail shapes, std 0.12
    ("std012", 3, "b64"): {("tail", 2): 1.062e-5}, ("std012", 1, "b64"): {("tail", 0): 1.567e-5},
    ("std012", 3, "b65"): {("tail", 2): 1.072e-5}, ("std012", 1, "b65"): {("tail", 0): 1.503e-5},
    ("std012", 3, "b129"): {("tail", 2): 1.026e-5}, ("std012", 1, "b129"): {("tail", 0): 1.439e-5},
    ("std012", 3, "b257"): {("tail", 2): 1.018e-5}, ("std012", 1, "b257"): {("tail", 0): 1.448e-5},
    ("std012", 3, "varlen40"): {("tail", 2): 1.143e-5}, ("std012", 1, "varlen40"): {("tail", 0): 1.486e-5},
    ("std012", 3, "serve1x64"): {("tail", 2): 9.748e-6}, ("std012", 1, "serve1x64"): {("tail", 0): 2.128e-5},
    ("std012", 3, "serve1x512"): {("tail", 2): 1.016e-5}, ("std012", 1, "serve1x512"): {("tail", 0): 1.082e-5},
    ("std012", 3, "serve2x64"): {("tail", 2): 9.677e-6}, ("std012", 1, "serve2x64"): {("tail", 0): 1.456e-5},
    ("std012", 3, "serve4x512"): {("tail", 2): 1.121e-5}, ("std012", 1, "serve4x512"): {("tail", 0): 1.714e-5},
    # D: recipes on SPLIT_EDGES
    ("peaked", 3, "split_edges"): {("layer", 0): 8.188e-5, ("layer", 1): 7.315e-5, ("tail", 2): 5.197e-5},
    ("outlier", 3, "split_edges"): {("layer", 0): 2.991e-5, ("layer", 1): 1.388e-5, ("tail", 2): 1.122e-5},
}
# the four cells the committed LAYER_BOUNDS stand 2.6 x above, (recipe, batch) -> (layer 0, layer 1)
LAYER_EMUL = {("std008", "edges"): (1.103e-5, 7.844e-6), ("std008", "split_edges"): (1.102e-5, 7.886e-6),
              ("std012", "edges"): (1.671e-5, 1.343e-5), ("std012", "split_edges"): (1.670e-5, 1.341e-5)}
SEPARATION = 3.0
PINS = ["2/2", "3/3", "4/4", "2/6", "3/8", "4/12", "4/16"]
_ENC, _CACHE = {}, {}


def bound(recipe, depth, batch, stage, n):
    if stage == "embed":
        return LAYER_BOUNDS[0.08]["embed"]
    if recipe in STD and (stage == "layer" or batch == "edges"):
        return LAYER_BOUNDS[STD[recipe]][stage]
    return sp.EMUL_FACTOR * E_EMUL[(recipe, depth, batch)][(stage, n)]


def encoder(recipe, depth):
    from haconvdr_amd.encoder import ANCEEncoder
    if (recipe, depth) not in _ENC:
        _ENC[(recipe, depth)] = ANCEEncoder.from_state_dict(sp.weights(recipe, depth), precision="split")
    return _ENC[(recipe, depth)]


def model_ksplit(B, L, n_cu):
    """encoder.hip's pick_ksplit with the split family's slots (ksplit_slots: n_cu) for one sub-batch of B x L: "a/b" for out-proj (K = 768) and FFN-down (K = 3072)."""
    Mp = (B * ((L + 31) // 32 * 32) + 255) // 256 * 256

    def pick(KT, min_kt):
        S, best, tiles = 1, KT * 0.6, (Mp // 128) * 6
        for cand in (2, 3, 4, 6):
            if KT % cand or KT // cand < min_kt or tiles * cand > n_cu:
                continue
            cost = KT / cand * 0.6 + (cand - 1) * Mp * 1.3e-3
            if cost < best:
                S, best = cand, cost
        return S
    return f"{pick(12, 4)}/{pick(48, 8)}"


def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def run(recipe, depth, batch, ksplit=None, pin=None, mutations=False, layers=True, calls=1):
    """teacher_forced of one case on the recipe's handle, every plan checked for the ksplit it must have run
    (default: the model's).  Returns (figs, sep, plans, outs)."""
    from oracle import ance_oracle
    key = (recipe, depth, batch, ksplit, pin, mutations, layers, calls)
    if key in _CACHE:
        return _CACHE[key]
    enc, sd = encoder(recipe, depth), sp.weights(recipe, depth)
    ids, mask = sp.batch(batch)
    expect = pin or ("1/1" if ksplit == "off" else model_ksplit(ids.shape[0], ids.shape[1], n_cu()))
    try:
        if ksplit:
            enc.set_option("ksplit", ksplit)
        if pin:
            enc.set_option("ksplit_pin", pin)
        lm = ance_oracle.LAYER_MUTATIONS + ance_oracle.CHUNK_MUTATIONS if mutations else ()
        tm = ance_oracle.TAIL_MUTATIONS + ance_oracle.CHUNK_MUTATIONS if mutations else ()
        figs, sep, plans, outs = sp.teacher_forced(enc, sd, ids, mask, depth, lm, tm, layers=layers, calls=calls)
    finally:
        enc.set_option("ksplit", "auto")
        enc.set_option("ksplit_pin", "0/0")
    for p in plans[0 if depth > 1 else 1:]:      # (a 1-layer encoder's layer_state stops at the embedding stage, before split-K is planned)
        assert p["ksplit"] == expect, (recipe, depth, batch, p, expect)
    print(f"{recipe} x{depth} {batch} ksplit={plans[-1]['ksplit']} rows={plans[-1]['rows']}", {k: f"{v:.3e}" for k, v in figs.items()})
    _CACHE[key] = (figs, sep, plans, outs)
    return _CACHE[key]


def assert_within(recipe, depth, batch, figs, what=None):
    bad = {k: (f, bound(recipe, depth, batch, k[0], k[1])) for k, f in figs.items()
           if not (np.isfinite(f) and f <= bound(recipe, depth, batch, k[0], k[1]))}
    assert not bad, (what or (recipe, depth, batch), "stage: (rel, bound)", bad)


# ------------------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("batch", ["split_edges", "L100", "L200"])
@pytest.mark.parametrize("recipe", ["std008", "std012"])
def test_attention_chunk_and_tile_edges(recipe, batch):
    """Every stage of a 3-layer forward.  SPLIT_EDGES: 3104 packed rows, 450 QKV tiles on n_cu workgroups (every XCD's run
    longer than its slots), split-K 1/1 by the model."""
    figs, _, plans, _ = run(recipe, 3, batch)
    if batch == "split_edges":
        assert plans[0]["ksplit"] == "1/1", plans[0]
    assert_within(recipe, 3, batch, figs)


# ------------------------------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("pin", ["off"] + PINS)
@pytest.mark.parametrize("recipe", ["std008", "std012"])
def test_split_k_off_and_pinned_slice_counts(recipe, pin):
    """The `edges` batch (12 row tiles x 6 x S work items) with split-K off and with every pinned count: slice s > 0 goes through
    the RESID epilogue's partial branch into partial buffer s - 1, ln_split_rows_kernel adds 1 ... 15 of them."""
    figs, _, _, _ = run(recipe, 3, "edges", ksplit="off") if pin == "off" else run(recipe, 3, "edges", pin=pin)
    assert_within(recipe, 3, "edges", figs, (recipe, pin))


@pytest.mark.parametrize("recipe", ["std008", "std012"])
def test_split_k_16_slices_across_tile_and_slice_seams(recipe):
    """SPLIT_EDGES pinned to 4/16: FFN-down is 150 x 16 work items, every workgroup's prefetch crosses slice and tile seams."""
    figs, _, _, _ = run(recipe, 3, "split_edges", pin="4/16")
    assert_within(recipe, 3, "split_edges", figs, (recipe, "4/16"))


def test_split_k_by_the_model_on_small_batches():
    """1 x 64 and 4 x 512 with the model's own slice counts: at least one of the four (batch, GEMM) pairs runs S >= 4 (on a
    256-CU part: 3/6 and 2/2)."""
    chosen = []
    for batch in ("serve1x64", "serve4x512"):
        figs, _, plans, _ = run("std012", 3, batch)
        chosen += [int(v) for v in plans[-1]["ksplit"].split("/")]
        assert_within("std012", 3, batch, figs)
    print("split-K by the model, (1 x 64 out-proj, FFN-down, 4 x 512 out-proj, FFN-down):", chosen)
    assert max(chosen) >= 4, chosen


# ------------------------------------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("batch", ["b64", "b65", "b129", "b257", "varlen40"])
@pytest.mark.parametrize("depth", [3, 1])
def test_tail_shapes(depth, batch):
    """The <s>-row tail on 1, 2 and 3 compact 128-row tiles, the head's switch to 64 features per workgroup at B > 64."""
    figs, _, _, _ = run("std012", depth, batch, layers=False)
    assert_within("std012", depth, batch, figs)


@pytest.mark.parametrize("shape", ["1x64", "1x512", "2x64", "4x512"])
@pytest.mark.parametrize("depth", [3, 1])
def test_tail_serving_shapes_eager_capture_replay(depth, shape):
    """Three calls of a serving shape: every one inside the bound, the replays bit-equal to the eager call."""
    enc = encoder("std012", depth)
    enc.set_option("ksplit_pin", "0/0")      # (its default; setting it drops the captured graphs: the first call is eager)
    figs, _, plans, outs = run("std012", depth, "serve" + shape, layers=False, calls=3)
    assert [p["graph"] for p in plans[1:]] == ["eager-first", "replay", "replay"], plans
    assert all(np.array_equal(o, outs[0]) for o in outs[1:])
    assert len(figs) == 3
    assert_within("std012", depth, "serve" + shape, figs)


# ------------------------------------------------------------------------------------------------------------------------- D
@pytest.mark.parametrize("recipe", ["peaked", "outlier"])
def test_peaked_logits_and_outlier_channels(recipe):
    """peaked: Q and K x 8, the softmax reference moves on every (sequence, head) item of layer 0 (asserted on the reference
    alone by tests/test_encoder_precision.py::test_peaked_recipe_moves_the_softmax_reference); outlier: three channels x 60."""
    figs, _, _, _ = run(recipe, 3, "split_edges")
    assert_within(recipe, 3, "split_edges", figs)


# ------------------------------------------------------------------------------------------------------------------------- E
@pytest.mark.parametrize("recipe", ["std008", "std012"])
def test_bounds_reject_every_mutation_on_the_split_edges(recipe):
    """Every LAYER_MUTATIONS / TAIL_MUTATIONS entry and key_chunk, on the kernels' own SPLIT_EDGES state, lies >= 3 x beyond the
    bound, or is listed in test_encoder_precision_gpu.NOT_SEPARABLE with the reason given there (eps / head_eps everywhere;
    gelu_tanh at std 0.12, still > 1.5 x)."""
    _, sep, _, _ = run(recipe, 3, "split_edges", mutations=True)
    ratio = {k: v / bound(recipe, 3, "split_edges", k[0], k[1]) for k, v in sep.items()}
    print("separations", recipe, {k: f"{v:.1f}" for k, v in ratio.items()})
    weak = {k: v for k, v in ratio.items() if v < SEPARATION and (STD[recipe], 3) + k not in NOT_SEPARABLE}
    assert not weak, (recipe, weak)
    for k, v in ratio.items():
        if k[2] == "gelu_tanh":
            assert v > 1.5, (recipe, k, v)
        if k[2] == "key_chunk":
            assert v >= SEPARATION, (recipe, k, v)

