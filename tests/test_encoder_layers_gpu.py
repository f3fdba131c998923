"""Teacher-forced, layer-by-layer parity of the encoder kernels against a bf16-faithful fp64 reference.

The CLS-level tests (test_encoder_gpu.py, tests/parity.py) cannot be tighter than the bf16 path's rounding noise accumulated
over twelve layers, and subtle slips (tanh GELU, a wrong LayerNorm eps, logits off by 1 %) hide below it.  Here every stage
is observed on its own: ANCEEncoder.layer_state (hac_encoder_layer_state: the same launches as a forward, stopped after
layer N) gives the kernels' residual stream after layer N-1, oracle.ance_oracle.ance_layer computes layer N from exactly
that state in fp64 with bf16 roundings where the kernel's GEMM family rounds, and the kernel's own layer N is compared with
it element by element on the valid rows.  Only one layer's rounding flips separate the two.

Figures (over the valid rows of the normalized output [B, L, 768], d = kernel - reference):
  rel   = ||d|| / ||ref||                                     (every element)
  bias  = rms over features of mean_rows(d) / rms(ref)         (the systematic part: noise averages out over the rows)

  along = |<mean_rows(d), u>| / |u| / rms(ref), u = a mutation's own per-feature mean shift (its signature)

Bounds (BOUNDS) are 2x the worst figure measured on MI355X per (weights, family, stage) over all routes and batches; every
mutation of the reference (run on the kernel's own input) must land >= 3x beyond them in one figure, and the kernel must not
lean towards any mutation's signature (LEAN_LIMIT).  The streaming attention kernels round P relative to a reference that
stays at 0 (ance_oracle._window_reference): modelled as such, their floor equals the exact-maximum two-pass kernel's;
modelled with the row maximum it was 4x higher (the rounding points differ, not the kernels' arithmetic).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_LAYERS = 3                      # stages -1 (embedding LayerNorm), 0 and 1 are observable (the last layer is CLS-only)
STAGES = (-1, 0, 1)
GEMM = {"classic": "classic", "gemm8": "8phase"}
# the bounds: (weights, family, "embed" | "layer") -> (rel, bias), each 2x the worst figure measured on MI355X over the routes
# and batches of those weights (embed | layer 0 | layer 1, rel / bias):
#   std002  classic 6.9e-8 / 1.4e-8 | 1.6e-4 / 4.4e-6 | 2.3e-4 / 6.1e-6    gemm8 2.0e-5 / 4.7e-7 | 1.0e-3 / 4.1e-5 | 1.0e-3 / 4.2e-5
#   std010  classic 6.9e-8 / 1.4e-8 | 9.4e-4 / 2.3e-5 | 1.3e-3 / 3.9e-5    gemm8 2.0e-5 / 4.7e-7 | 1.6e-3 / 3.7e-5 | 1.7e-3 / 3.9e-5
#   peaked  classic 6.9e-8 / 1.4e-8 | 2.4e-4 / 6.2e-6 | 3.2e-4 / 8.2e-6    gemm8 2.0e-5 / 4.7e-7 | 1.1e-3 / 4.4e-5 | 1.2e-3 / 4.4e-5
#   outlier classic 6.8e-8 / 8.4e-9 | 3.8e-4 / 1.0e-5 | 5.7e-4 / 2.3e-5    gemm8 6.9e-6 / 1.6e-7 | 1.8e-3 / 4.8e-5 | 3.1e-3 / 1.2e-4
# (the classic embedding rows are fp32: only fp32-vs-fp64 LayerNorm arithmetic separates them from the reference)
BOUNDS = {}
for _k, _cl, _g8 in (("std002", (5e-4, 1.3e-5), (2.1e-3, 8.5e-5)), ("std010", (2.7e-3, 8e-5), (3.5e-3, 8e-5)),
                     ("peaked", (7e-4, 2e-5), (2.5e-3, 9e-5)), ("outlier", (1.2e-3, 4.5e-5), (6.3e-3, 2.4e-4))):
    BOUNDS[(_k, "classic", "embed")] = (1.4e-7, 3e-8)
    BOUNDS[(_k, "gemm8", "embed")] = (4.1e-5, 1e-6)
    BOUNDS[(_k, "classic", "layer")] = _cl
    BOUNDS[(_k, "gemm8", "layer")] = _g8
SEPARATION = 3.0
# lengths at the kernels' block edges (32-row blocks, 256-row length classes, 512 = the longest), one sequence each:
# 1984 packed rows = 7.75 tiles of 256 (a partial last tile), 9 sequences (few enough for the query split)
EDGE_LENS = [1, 31, 32, 33, 255, 256, 257, 511, 512]
ROUTES = {   # option sets (ANCEEncoder.set_option) of the attention and split-K routes; every one ends at its default again
    "default": {},
    "ksplit_off": {"ksplit": "off"},
    "twopass": {"attn": "twopass"},
    "pipe_all": {"attn_pipe": "all", "attn_qsplit": "off"},   # (the woven kernel takes whole items only: no query split)
    "qsplit_off": {"attn_qsplit": "off"},
}
DEFAULTS = {"ksplit": "auto", "attn": "stream", "attn_pipe": "auto", "attn_qsplit": "auto", "gemm": "auto"}
_SD, _ENC = {}, {}


def weights(kind):
    """std002 / std010: synth weights with layer matrices of that std; peaked: std 0.02 with Q and K x 8 (logits x 64: the
    woven attention kernel hands most items to its fix-up pass); outlier: test_outlier_channels_and_row_means_vs_oracle's
    weights (three 60x channels, row means of several sigma)."""
    from haconvdr_amd import synth
    if kind in _SD:
        return _SD[kind]
    std = 0.10 if kind == "std010" else 0.02
    sd = dict(synth.ance_state_dict(0x1A7E, N_LAYERS, layer_matrix_std=std))
    if kind == "peaked":
        for i in range(N_LAYERS):
            for nm in ("query", "key"):
                for part in ("weight", "bias"):
                    key = f"roberta.encoder.layer.{i}.attention.self.{nm}.{part}"
                    sd[key] = (sd[key] * 8.0).astype(np.float32)
    if kind == "outlier":
        dims = [7, 300, 701]
        g = sd["roberta.embeddings.LayerNorm.weight"].copy()
        g[dims] *= 60.0
        sd["roberta.embeddings.LayerNorm.weight"] = g
        for i in range(N_LAYERS):
            for nm in ("attention.output.dense", "output.dense"):
                w = sd[f"roberta.encoder.layer.{i}.{nm}.weight"].copy()
                w[dims, :] *= 60.0
                sd[f"roberta.encoder.layer.{i}.{nm}.weight"] = w
            b = sd[f"roberta.encoder.layer.{i}.output.dense.bias"].copy()
            sd[f"roberta.encoder.layer.{i}.output.dense.bias"] = (b + 3.0).astype(np.float32)
    _SD[kind] = sd
    return sd


def encoder(kind):
    from haconvdr_amd.encoder import ANCEEncoder
    if kind not in _ENC:
        _ENC[kind] = ANCEEncoder.from_state_dict(weights(kind))
    return _ENC[kind]


def batch(name):
    from haconvdr_amd import synth
    from tests.golden.make_golden_encoder import encoder_case_inputs
    if name == "edges":
        return encoder_case_inputs(0x5EED, EDGE_LENS, 512)
    ids, lens = synth.token_batch(0xB16, 40, 512, min_len=1)           # mixed lengths, ~10 k rows: several tiles, a partial one
    mask = (np.arange(512)[None, :] < lens[:, None]).astype(np.int64)
    return ids.astype(np.int64), mask


def figures(out, ref, valid):
    d = (np.asarray(out, np.float64) - np.asarray(ref, np.float64))[valid]
    r = np.asarray(ref, np.float64)[valid]
    scale = np.sqrt((r ** 2).mean())
    return {"rel": float(np.sqrt((d ** 2).mean()) / scale), "bias": float(np.sqrt((d.mean(0) ** 2).mean()) / scale)}


def kernel_states(enc, family, ids, mask, route):
    """{stage: layer_state} of one forward route, and the plan string of the last call."""
    enc.set_option("gemm", GEMM[family])
    for k, v in ROUTES[route].items():
        enc.set_option(k, v)
    try:
        states = {n: enc.layer_state(ids, mask, n, normalized=True) for n in STAGES}
        plan = dict(kv.split("=") for kv in enc.last_plan().split())
        redo = enc.attention_redo() if ROUTES[route].get("attn_pipe") == "all" else None
    finally:
        for k in list(ROUTES[route]) + ["gemm"]:
            enc.set_option(k, DEFAULTS[k])
    return states, plan, redo


def reference(sd, family, n, ids, mask, states, mutate=None, attn="stream"):
    """The fp64 reference of stage n on the kernel's stage n-1 state (the embedding stage: on the token ids)."""
    from oracle import ance_oracle
    if n < 0:
        return ance_oracle.ance_embed(sd, ids, mask, family, mutate=mutate)
    return ance_oracle.ance_layer(sd, n, states[n - 1], mask, family, mutate=mutate, attn=attn)


def stage_figures(sd, family, ids, mask, states, attn="stream"):
    valid = np.asarray(mask, bool)
    return {n: figures(states[n]["norm"], reference(sd, family, n, ids, mask, states, attn=attn)["norm"].numpy(), valid) for n in STAGES}


def assert_within(kind, family, figs, what):
    for n, f in figs.items():
        rb, bb = BOUNDS[(kind, family, "embed" if n < 0 else "layer")]
        assert np.isfinite(f["rel"]) and f["rel"] <= rb and f["bias"] <= bb, (what, family, "stage", n, f, "bounds", (rb, bb))


def _check(kind, family, route, batch_name):
    enc, sd = encoder(kind), weights(kind)
    ids, mask = batch(batch_name)
    states, plan, redo = kernel_states(enc, family, ids, mask, route)
    assert plan["gemm"] == "gemm8" if family == "gemm8" else plan["gemm"].startswith("classic"), plan
    if route == "twopass":
        assert plan["attn"] == "twopass", plan
    if route == "pipe_all":
        assert plan["attn_form"] == "woven", plan
    figs = stage_figures(sd, family, ids, mask, states, attn="twopass" if route == "twopass" else "stream")
    assert_within(kind, family, figs, (kind, route, batch_name))
    return figs, redo


# (split-K exists on the classic 128-row kernels only)
FAMILY_ROUTES = [(f, r) for f in GEMM for r in ROUTES if not (f == "gemm8" and r == "ksplit_off")]


@pytest.mark.parametrize("family,route", FAMILY_ROUTES, ids=[f"{f}-{r}" for f, r in FAMILY_ROUTES])
@pytest.mark.parametrize("kind", ["std002", "std010"])
def test_layers_vs_bf16_faithful_reference(kind, family, route):
    """Every route of both GEMM families, lengths at every block edge, a partial last 256-row tile."""
    _check(kind, family, route, "edges")


@pytest.mark.parametrize("family", list(GEMM))
def test_layers_mixed_varlen_batch(family):
    _check("std010", family, "default", "varlen")


@pytest.mark.parametrize("family", list(GEMM))
def test_layers_peaked_logits_through_the_fixup_pass(family):
    """Q and K x 8: the woven kernel flags most items and the one-block kernel computes them again (asserted: it ran)."""
    _, redo = _check("peaked", family, "pipe_all", "edges")
    assert redo > 0, redo


@pytest.mark.parametrize("family", list(GEMM))
def test_layers_outlier_channels_and_row_means(family):
    _check("outlier", family, "default", "edges")


def along(d, u, valid, scale):
    """|<mean_rows(d), u>| / |u| / scale: the part of d's systematic error that lies along a mutation's signature u (the
    per-feature mean of mutated - unmutated reference).  Rounding noise puts ~ its per-feature rms there (the bias figure);
    a mutation all of its |u|, sqrt(768) times its own bias figure."""
    m = (np.asarray(d, np.float64)[valid]).mean(0)
    return float(abs(m @ u) / np.linalg.norm(u) / scale)


def mutation_ratios(kind, family):
    """{(stage, mutation): (separation, kernel)}: separation = max over the figures rel, bias and along of the mutated reference's
    distance from the reference / bound, on the kernel's own input; kernel = the kernel's own along figure for that mutation's
    signature / the bias bound (must stay <= 1: the kernel shows none of the mutation)."""
    from oracle import ance_oracle
    enc, sd = encoder(kind), weights(kind)
    ids, mask = batch("edges")
    states, _, _ = kernel_states(enc, family, ids, mask, "default")
    valid = np.asarray(mask, bool)
    out = {}
    for n in STAGES:
        rb, bb = BOUNDS[(kind, family, "embed" if n < 0 else "layer")]
        base = reference(sd, family, n, ids, mask, states)["norm"].numpy()
        scale = np.sqrt((base[valid] ** 2).mean())
        for m in (ance_oracle.EMBED_MUTATIONS if n < 0 else ance_oracle.LAYER_MUTATIONS):
            mut = reference(sd, family, n, ids, mask, states, mutate=m)["norm"].numpy()
            f = figures(mut, base, valid)
            u = (mut - base)[valid].mean(0)
            sep = max(f["rel"] / rb, f["bias"] / bb, along(mut - base, u, valid, scale) / bb)
            out[(n, m)] = (sep, along(states[n]["norm"] - base, u, valid, scale) / bb)
    return out


# Measured separations (MI355X, edges batch): every mutation >= 3x in every case except the LayerNorm eps inside the layers
# with std-0.10 weights, whose rows have a variance ~1 that eps 1e-12 vs 1e-5 moves by 5e-6: 0.80 / 0.79 (classic, layers
# 0 / 1) and 0.92 / 0.83 (gemm8).  eps is rejected at the embedding stage (rows of variance ~1e-3: ratio 6.6e4 .. 2.2e6)
# and inside the layers with std-0.02 weights (3.2 .. 11.8).  tanh GELU is separated through its signature (8.1 .. 83).
NOT_SEPARABLE = {("std010", "classic", 0, "eps"), ("std010", "classic", 1, "eps"), ("std010", "gemm8", 0, "eps"), ("std010", "gemm8", 1, "eps")}
# The kernels' own lean towards a mutation's signature, in units of the bias bound: <= 1 except where measured higher, pinned
# there at 2x the measurement.  The fp32 LayerNorm of the classic embedding rows (rsqrtf) leans along the eps signature by
# 3.7e-7 of the rows' rms; the GELU polynomials' systematic error (|error| <= 8.8e-5, gemm8.inc gelu8_2 / encoder.hip
# gelu_erf2) lies partly along tanh GELU's: gemm8 shows 62 % of a tanh substitution with std-0.02 weights (lean 9.2 against
# separation 14.9), 19 % with std 0.10; the classic form 5 %.
LEAN_LIMIT = {
    ("std002", "classic", -1, "eps"): 25.0, ("std002", "classic", -1, "pos"): 3.0, ("std010", "classic", -1, "eps"): 25.0,
    ("std010", "classic", -1, "pos"): 3.0, ("std002", "classic", 0, "eps"): 2.1, ("std002", "classic", 1, "eps"): 3.3,
    ("std002", "classic", 1, "logits"): 2.2, ("std002", "classic", 0, "gelu_tanh"): 8.7, ("std002", "classic", 1, "gelu_tanh"): 7.7,
    ("std010", "classic", 0, "gelu_tanh"): 2.2, ("std002", "gemm8", 0, "logits"): 3.5, ("std002", "gemm8", 1, "logits"): 4.1,
    ("std002", "gemm8", 0, "gelu_tanh"): 18.5, ("std002", "gemm8", 1, "gelu_tanh"): 17.8, ("std010", "gemm8", 0, "gelu_tanh"): 5.0,
    ("std010", "gemm8", 1, "gelu_tanh"): 3.3,
}


@pytest.mark.parametrize("family", list(GEMM))
@pytest.mark.parametrize("kind", ["std002", "std010"])
def test_bounds_reject_every_mutation(kind, family):
    """The self-check of the bounds: each mutation of the reference, on the kernel's input, must be >= 3x beyond them (in rel,
    bias or along its own signature), and the kernel's output must not lean towards any of them beyond LEAN_LIMIT."""
    r = mutation_ratios(kind, family)
    weak = {k: v for k, v in r.items() if v[0] < SEPARATION and (kind, family) + k not in NOT_SEPARABLE}
    leaning = {k: v for k, v in r.items() if v[1] > LEAN_LIMIT.get((kind, family) + k, 1.0)}
    assert not weak and not leaning, (kind, family, weak, leaning, r)
    for k in NOT_SEPARABLE:
        if k[:2] == (kind, family):
            assert r[k[2:]][0] > 0.5, (k, r[k[2:]])     # still measured: a bound twice as loose would hide it entirely
