"""precision = split, stage by stage: what tests/test_encoder_precision_gpu.py, tests/test_encoder_precision_shapes_gpu.py (the
kernels, teacher-forced) and tests/test_encoder_precision.py (the yardstick of their bounds, CPU alone) share.

Figure of a stage: rel = rms(out - ref) / rms(ref) over the valid rows of the normalized state (the tail: over the embeddings).
  * teacher_forced: the kernels' stage on the kernels' own previous state (ANCEEncoder.layer_state in split mode) against the
    UNROUNDED fp64 chain (oracle.ance_oracle, family=None) on that same state;
  * emulation: E_emul(stage) = rel(family="split", family=None), both on the state of the unrounded chain run freely from
    ance_embed -- how far a correct hi + lo implementation with exact accumulation sits from the unrounded chain.  Bounds
    that are not committed LAYER_BOUNDS are EMUL_FACTOR x E_emul: the ratio the committed bounds have to the emulation on the
    four cells measured on MI355X (2.9e-5 / 1.103e-5 = 4.4e-5 / 1.671e-5 = 2.63: the usual 2 x on a worst figure, times the
    1.3 x that fp32 accumulation adds to the fp64 emulation).
"""
import numpy as np

EMUL_FACTOR = 2.6
SEED = 0x1A7E
# lengths at the bf16 kernels' edges (32-row blocks, 256-row classes): len32 in {32, 64, 256, 288, 512}
EDGE_LENS = [1, 31, 32, 33, 255, 256, 257, 512]
# lengths at attention_split_kernel's own edges: both sides of the 64-key chunks and the 128-row query parts (1, 2, 3 active
# waves in the last part; a half-filled last chunk; len32 = 64 ... 512), 3104 packed rows: 25 x 18 QKV tiles
SPLIT_EDGES = [63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 161, 383, 385, 449, 481]
# L that is no multiple of 32 / 128: L32 = 128 (one query part) and L32 = 224 (two; the second with 1, 2 and 3 active waves)
L100_LENS = [1, 31, 33, 63, 64, 65, 95, 96, 97, 99, 100]
L200_LENS = [1, 64, 127, 128, 129, 159, 160, 161, 191, 192, 193, 199, 200]
TAIL_SHAPES = {"short40": (40, 64), "varlen40": (40, 512), "b64": (64, 128), "b65": (65, 128), "b129": (129, 64), "b257": (257, 64)}
_SD = {}


def rel(out, ref, valid=None):
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    if valid is not None:
        out, ref = out[valid], ref[valid]
    return float(np.sqrt(((out - ref) ** 2).mean()) / np.sqrt((ref ** 2).mean()))


def add_outlier_channels(sd, scale, dims=(7, 300, 701)):
    """Three channels x scale in the embedding LayerNorm's gain and in the rows of both output denses of the first three
    layers, FFN output bias + 3 (tools/parity_survey.py's recipe).  Returns a new dict."""
    sd, dims = dict(sd), list(dims)
    g = sd["roberta.embeddings.LayerNorm.weight"].copy()
    g[dims] *= scale
    sd["roberta.embeddings.LayerNorm.weight"] = g
    for i in range(3):
        for nm in ("attention.output.dense", "output.dense"):
            w = sd[f"roberta.encoder.layer.{i}.{nm}.weight"].copy()
            w[dims, :] *= scale
            sd[f"roberta.encoder.layer.{i}.{nm}.weight"] = w
        b = sd[f"roberta.encoder.layer.{i}.output.dense.bias"].copy()
        sd[f"roberta.encoder.layer.{i}.output.dense.bias"] = (b + 3.0).astype(np.float32)
    return sd


def peak_logits(sd, scale):
    """Q and K weight and bias of every layer x scale (logits x scale^2): softmax references that move."""
    sd = dict(sd)
    for k in list(sd):
        if ".attention.self.query." in k or ".attention.self.key." in k:
            sd[k] = (sd[k] * scale).astype(np.float32)
    return sd


PEAKED_SCALE = 8.0     # moves the reference on 100 % of layer 0's (sequence, head) items of SPLIT_EDGES (test_encoder_precision.py)
OUTLIER_SCALE = 60.0


def weights(recipe, n_layers=3):
    """std008 / std012: synth weights of seed SEED at layer-matrix std 0.08 / 0.12 (LAYER_BOUNDS' weights); peaked, outlier:
    the 3-layer std008 weights through peak_logits(PEAKED_SCALE) / add_outlier_channels(OUTLIER_SCALE)."""
    from haconvdr_amd import synth
    key = (recipe, n_layers)
    if key not in _SD:
        if recipe in ("std008", "std012"):
            _SD[key] = synth.ance_state_dict(SEED, n_layers, layer_matrix_std={"std008": 0.08, "std012": 0.12}[recipe])
        else:
            assert n_layers == 3, key
            _SD[key] = {"peaked": lambda s: peak_logits(s, PEAKED_SCALE), "outlier": lambda s: add_outlier_channels(s, OUTLIER_SCALE)}[recipe](weights("std008", 3))
    return _SD[key]


def batch(name):
    """(ids, mask) int64 [B, L].  edges / split_edges / L100 / L200: the length lists above; the TAIL_SHAPES and serveBxL as
    tests/test_encoder_tail_gpu.batch builds them (b129: two compact 128-row tiles of the split GEMM, b257: three)."""
    from haconvdr_amd import synth
    from tests.golden.make_golden_encoder import encoder_case_inputs
    fixed = {"edges": (EDGE_LENS, 512), "split_edges": (SPLIT_EDGES, 512), "L100": (L100_LENS, 100), "L200": (L200_LENS, 200)}
    if name in fixed:
        return encoder_case_inputs(0x5EED, *fixed[name])
    if name.startswith("serve"):
        B, L = (int(v) for v in name[5:].split("x"))
        ids, lens = synth.token_batch(0x5E7 + B * 1000 + L, B, L, min_len=max(1, L // 4))
    else:
        B, L = TAIL_SHAPES[name]
        ids, lens = synth.token_batch(0x7A1 + B + L, B, L, min_len=1)
    return ids.astype(np.int64), (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)


def plan_of(enc):
    return dict(kv.split("=") for kv in enc.last_plan().split())


def assert_split_plan(enc, ksplit=None):
    """The most recent forward ran the split kernels (and the split-K slice counts "a/b" it was meant to)."""
    plan = plan_of(enc)
    assert plan["gemm"] == "split128" and plan.get("precision") == "split" and plan["attn_form"] == "split", plan
    assert ksplit is None or plan["ksplit"] == ksplit, (plan, ksplit)
    return plan


def teacher_forced(enc, sd, ids, mask, n_layers, layer_mutations=(), tail_mutations=(), layers=True, calls=1):
    """Every stage of a split-mode forward of (ids, mask) against the unrounded chain on the kernels' own previous state.
    Returns (figs {(stage, n): rel}, sep {(stage, n, mutation): rel(mutated reference, reference)}, plans, outs): plans[0]
    is the plan of the layer_state calls, the others and outs those of `calls` forwards.  layers=False: the tail alone."""
    from oracle import ance_oracle
    first = -1 if layers else n_layers - 2
    states = {n: enc.layer_state(ids, mask, n, normalized=True) for n in range(first, n_layers - 1)}
    plans = [assert_split_plan(enc)]
    outs = []
    for _ in range(calls):
        outs.append(np.array(enc(ids.astype(np.int32), mask.astype(np.int32))))
        plans.append(assert_split_plan(enc))
    valid = np.asarray(mask, bool)
    figs, sep = {}, {}
    if layers:
        figs[("embed", -1)] = rel(states[-1]["norm"], ance_oracle.ance_embed(sd, ids, mask)["norm"].numpy(), valid)
        for n in range(n_layers - 1):
            base = ance_oracle.ance_layer(sd, n, states[n - 1], mask)["norm"].numpy()
            figs[("layer", n)] = rel(states[n]["norm"], base, valid)
            for m in layer_mutations:
                sep[("layer", n, m)] = rel(ance_oracle.ance_layer(sd, n, states[n - 1], mask, mutate=m)["norm"].numpy(), base, valid)
    base = ance_oracle.ance_tail(sd, n_layers - 1, states[n_layers - 2], mask).numpy()
    figs[("tail", n_layers - 1)] = rel(outs[-1], base)
    for c, o in enumerate(outs[:-1]):
        figs[("tail", n_layers - 1, c)] = rel(o, base)
    for m in tail_mutations:
        sep[("tail", n_layers - 1, m)] = rel(ance_oracle.ance_tail(sd, n_layers - 1, states[n_layers - 2], mask, mutate=m).numpy(), base)
    return figs, sep, plans, outs


def unrounded_chain(sd, ids, mask, n_layers):
    """States of the unrounded fp64 chain run freely from ance_embed: {-1: embed, 0 .. n_layers - 2: layers}."""
    from oracle import ance_oracle
    st = {-1: ance_oracle.ance_embed(sd, ids, mask)}
    for n in range(n_layers - 1):
        st[n] = ance_oracle.ance_layer(sd, n, st[n - 1], mask)
    return st


def emulation(sd, ids, mask, n_layers, layers=True, tail=True, chain=None):
    """E_emul per stage, {("layer", n) / ("tail", n_layers - 1): rel(family "split", family None)} on the unrounded chain's states."""
    from oracle import ance_oracle
    chain = chain or unrounded_chain(sd, ids, mask, n_layers)
    valid = np.asarray(mask, bool)
    e = {}
    if layers:
        for n in range(n_layers - 1):
            e[("layer", n)] = rel(ance_oracle.ance_layer(sd, n, chain[n - 1], mask, family="split")["norm"].numpy(), chain[n]["norm"].numpy(), valid)
    if tail:
        e[("tail", n_layers - 1)] = rel(ance_oracle.ance_tail(sd, n_layers - 1, chain[n_layers - 2], mask, family="split").numpy(),
                                        ance_oracle.ance_tail(sd, n_layers - 1, chain[n_layers - 2], mask).numpy())
    return e
