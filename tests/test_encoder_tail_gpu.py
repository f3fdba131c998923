"""Teacher-forced parity of the last encoder layer and the ANCE head against a bf16-faithful fp64 reference.

tests/test_encoder_layers_gpu.py observes every stage up to layer n-2; the last layer is a code path of its own and ends in
the embeddings the project returns.  Keys and values of every row, the query of the <s> row only (gemm8: cls_q_kernel),
attention for that row (cls_only), then out-projection, LayerNorm, FFN and LayerNorm on the gathered <s> rows (compact
matrices, gemm_bf16_nt_kernel and ln_rows_kernel on both families: the gemm8 family's last layer keeps an fp32 residual), and
the fp32 head (cls_head_proj_kernel, cls_head_norm_kernel).  ANCEEncoder.layer_state(.., n_layers - 2) gives the kernels'
state in front of it, oracle.ance_oracle.ance_tail computes the embeddings from exactly that state, and the kernels' own
forward of the same batch is compared with them.

Figures over the B embeddings (d = kernel - reference): rel and bias as in the layer test (bias only on batches of >= 40
sequences: on fewer the rows' noise does not average out), and cos = the worst row's 1 - cosine (the contract is per row).
"""
import numpy as np
import pytest

from tests.test_encoder_layers_gpu import DEFAULTS, EDGE_LENS, GEMM, ROUTES, along, encoder, figures, weights

pytestmark = pytest.mark.gpu

TAIL_ROUTES = ("default", "twopass", "qsplit_off")
MIN_BIAS_ROWS = 40
# the bounds: (weights, family, depth) -> (rel, bias, cos), each 2x the worst figure measured on MI355X over the routes and
# batches of that key (depth 3: the tail taught from stage 1; depth 1: from the embedding stage), rel / bias / cos:
#   std002  classic  3: 3.9e-4 / 2.9e-5 / 1.9e-7   1: 1.1e-4 / 1.8e-5 / 1.1e-7    gemm8  3: 2.4e-4 / 4.0e-5 / 1.7e-7   1: 1.4e-4 / 1.5e-5 / 6.2e-8
#   std010  classic  3: 2.3e-3 / 2.0e-4 / 7.8e-6   1: 1.1e-3 / 1.8e-4 / 3.7e-6    gemm8  3: 2.0e-3 / 1.5e-4 / 5.9e-6   1: 9.9e-4 / 1.7e-4 / 4.3e-6
#   outlier classic  3: 5.2e-4 / 7.9e-5 / 6.5e-7                                 gemm8  3: 6.9e-4 / 8.1e-5 / 2.7e-6
#   peaked  classic  3: 3.6e-4 / 5.3e-5 / 4.0e-7                                 gemm8  3: 3.6e-4 / 4.6e-5 / 3.5e-7
# (the worst rel of std010 comes from single sequences -- serve1x512, serve2x64 -- where one bf16 rounding flip in the
# sequence's FFN is the whole difference; the bias figure exists only on the batches of >= 40 sequences)
BOUNDS = {
    ("std002", "classic", 3): (7.9e-4, 5.9e-5, 3.9e-7), ("std002", "classic", 1): (2.3e-4, 3.7e-5, 2.2e-7),
    ("std002", "gemm8", 3): (4.8e-4, 8.1e-5, 3.5e-7), ("std002", "gemm8", 1): (2.9e-4, 3.0e-5, 1.3e-7),
    ("std010", "classic", 3): (4.6e-3, 4.1e-4, 1.6e-5), ("std010", "classic", 1): (2.3e-3, 3.6e-4, 7.5e-6),
    ("std010", "gemm8", 3): (4.0e-3, 3.0e-4, 1.2e-5), ("std010", "gemm8", 1): (2.0e-3, 3.4e-4, 8.7e-6),
    ("outlier", "classic", 3): (1.1e-3, 1.6e-4, 1.3e-6), ("outlier", "gemm8", 3): (1.4e-3, 1.7e-4, 5.5e-6),
    ("peaked", "classic", 3): (7.2e-4, 1.1e-4, 8.1e-7), ("peaked", "gemm8", 3): (7.3e-4, 9.3e-5, 7.1e-7),
}
SEPARATION = 3.0
_SD1, _ENC1 = {}, {}


def weights_at(kind, depth):
    """weights(kind) of the layer test (3 layers), or its first layer only (depth 1)."""
    if depth == 3:
        return weights(kind)
    if kind not in _SD1:
        _SD1[kind] = {k: v for k, v in weights(kind).items() if not k.startswith(("roberta.encoder.layer.1.", "roberta.encoder.layer.2."))}
    return _SD1[kind]


def encoder_at(kind, depth):
    from haconvdr_amd.encoder import ANCEEncoder
    if depth == 3:
        return encoder(kind)
    if kind not in _ENC1:
        _ENC1[kind] = ANCEEncoder.from_state_dict(weights_at(kind, depth))
    return _ENC1[kind]


def batch(name):
    """edges: the layer test's 9 block-edge lengths (a partial second CLS_SB group of 8, head_ns 8); short40: 40 sequences
    of <= 64 tokens; varlen40: 40 of <= 512 (~10 k rows); b64 / b65: the head's switch from 8 to 64 features per workgroup;
    b257: a partial second 256-row compact tile; serveBxL: the reference's serving shape (query split, att_one, graphs)."""
    from haconvdr_amd import synth
    from tests.golden.make_golden_encoder import encoder_case_inputs
    if name == "edges":
        return encoder_case_inputs(0x5EED, EDGE_LENS, 512)
    if name.startswith("serve"):
        B, L = (int(v) for v in name[5:].split("x"))
        ids, lens = synth.token_batch(0x5E7 + B * 1000 + L, B, L, min_len=max(1, L // 4))
    else:
        B, L, lo = {"short40": (40, 64, 1), "varlen40": (40, 512, 1), "b64": (64, 128, 1), "b65": (65, 128, 1), "b257": (257, 64, 1)}[name]
        ids, lens = synth.token_batch(0x7A1 + B + L, B, L, min_len=lo)
    return ids.astype(np.int64), (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)


def set_route(enc, family, route):
    enc.set_option("gemm", GEMM[family])
    for k, v in ROUTES[route].items():
        enc.set_option(k, v)


def reset_route(enc, route):
    for k in list(ROUTES[route]) + ["gemm"]:
        enc.set_option(k, DEFAULTS[k])


def kernel_tail(kind, depth, family, route, ids, mask, calls=1):
    """The kernels' state in front of the last layer, `calls` forwards of the batch, and their plans."""
    enc = encoder_at(kind, depth)
    set_route(enc, family, route)
    try:
        state = enc.layer_state(ids, mask, depth - 2)
        outs, plans = [], []
        for _ in range(calls):
            outs.append(np.asarray(enc(ids, mask)))
            plans.append(dict(kv.split("=") for kv in enc.last_plan().split()))
    finally:
        reset_route(enc, route)
    return state, outs, plans


def reference(kind, depth, family, state, mask, mutate=None, attn="stream"):
    from oracle import ance_oracle
    return ance_oracle.ance_tail(weights_at(kind, depth), depth - 1, state, mask, family, mutate=mutate, attn=attn).numpy()


def tail_figures(out, ref):
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    f = figures(out, ref, np.ones(len(out), bool))
    cos = (out * ref).sum(1) / (np.linalg.norm(out, axis=1) * np.linalg.norm(ref, axis=1))
    f["cos"] = float((1.0 - cos).max())
    if len(out) < MIN_BIAS_ROWS:
        f["bias"] = None
    return f


def measure(kind, depth, family, route, batch_name, calls=1):
    """(figures of the last call's embeddings, plans, outputs): nothing asserted (the measurement of the bounds uses it)."""
    ids, mask = batch(batch_name)
    state, outs, plans = kernel_tail(kind, depth, family, route, ids, mask, calls)
    ref = reference(kind, depth, family, state, mask, attn="twopass" if route == "twopass" else "stream")
    return tail_figures(outs[-1], ref), plans, outs


def assert_within(kind, family, depth, f, what):
    rb, bb, cb = BOUNDS[(kind, family, depth)]
    assert np.isfinite(f["rel"]) and f["rel"] <= rb and f["cos"] <= cb and (f["bias"] is None or f["bias"] <= bb), \
        (what, f, "bounds", (rb, bb, cb))


def _check(kind, depth, family, route, batch_name, calls=1):
    f, plans, outs = measure(kind, depth, family, route, batch_name, calls)
    for plan in plans:
        assert plan["gemm"] == "gemm8" if family == "gemm8" else plan["gemm"].startswith("classic"), plan
        assert plan["attn"] == ("twopass" if route == "twopass" else "stream"), plan
        assert (plan["attn_form"] == "twopass") == (route == "twopass"), plan
    assert_within(kind, family, depth, f, (kind, depth, route, batch_name))
    return f, plans, outs


@pytest.mark.parametrize("route", TAIL_ROUTES)
@pytest.mark.parametrize("family", list(GEMM))
@pytest.mark.parametrize("kind", ["std002", "std010"])
def test_tail_vs_bf16_faithful_reference(kind, family, route):
    """Both GEMM families through each attention route: block-edge lengths, and 40 short sequences (the bias figure)."""
    for name in ("edges", "short40"):
        _check(kind, 3, family, route, name)


@pytest.mark.parametrize("family", list(GEMM))
@pytest.mark.parametrize("kind", ["std002", "std010"])
def test_tail_of_a_one_layer_encoder(kind, family):
    """n_layers = 1: the gather reads the normalized embedding rows (no deferred LayerNorm), and gemm8's <s> query takes
    the identity statistics (idstats) into cls_q_kernel."""
    for name in ("edges", "short40"):
        _check(kind, 1, family, "default", name)


@pytest.mark.parametrize("name", ["b64", "b65", "b257", "varlen40"])
@pytest.mark.parametrize("family", list(GEMM))
def test_tail_batch_shapes(family, name):
    """The tail's own edges: head_ns 8 -> 64 at B > 64, a partial second compact tile (257 <s> rows), a long varlen batch."""
    _check("std010", 3, family, "default", name)


@pytest.mark.parametrize("L", [64, 512])
@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("family", list(GEMM))
@pytest.mark.parametrize("kind", ["std002", "std010"])
def test_tail_serving_shape_eager_capture_replay(kind, family, B, L):
    """About four queries per call (the reference's serving loop): query-split attention (att_one at L = 512), the graph
    path -- eager first, then capture and replay -- whose replays must give the eager call's bits."""
    enc = encoder_at(kind, 3)
    enc.set_option("attn_qs_pin", "0")    # (its default, the rule's split; setting it drops the captured graphs: the first call is eager)
    f, plans, outs = _check(kind, 3, family, "default", f"serve{B}x{L}", calls=3)
    assert [p["graph"] for p in plans] == ["eager-first", "replay", "replay"], plans
    assert all(np.array_equal(o, outs[0]) for o in outs[1:])


@pytest.mark.parametrize("family", list(GEMM))
@pytest.mark.parametrize("kind", ["outlier", "peaked"])
def test_tail_outlier_channels_and_peaked_logits(kind, family):
    """outlier: three 60x channels reach the head through the last layer's output dense; peaked: Q and K x 8."""
    for name in ("edges", "short40"):
        _check(kind, 3, family, "default", name)


def mutation_ratios(kind, family):
    """{mutation: (separation, kernel)} on the short40 batch, as test_encoder_layers_gpu.mutation_ratios: separation = max of
    the mutated reference's rel, bias and along figures (from the reference) / their bounds, on the kernel's own input;
    kernel = the kernel's own along figure for that mutation's signature / the bias bound."""
    from oracle import ance_oracle
    ids, mask = batch("short40")
    state, outs, _ = kernel_tail(kind, 3, family, "default", ids, mask)
    rb, bb, _ = BOUNDS[(kind, family, 3)]
    base = reference(kind, 3, family, state, mask)
    scale = np.sqrt((base ** 2).mean())
    valid = np.ones(len(base), bool)
    out = {}
    for m in ance_oracle.TAIL_MUTATIONS:
        mut = reference(kind, 3, family, state, mask, mutate=m)
        f = figures(mut, base, valid)
        u = (mut - base).mean(0)
        sep = max(f["rel"] / rb, f["bias"] / bb, along(mut - base, u, valid, scale) / bb)
        out[m] = (sep, along(outs[0] - base, u, valid, scale) / bb)
    return out


# Measured separations (MI355X, short40 batch): >= 3x everywhere except
#   * head_eps with std-0.10 weights: 0.99 (classic) and 1.36 (gemm8).  The head's rows have a variance of ~0.3, which eps
#     1e-12 vs 1e-5 moves by 1.7e-5 of the rows' rms, against bounds set by one layer's bf16 noise (std002: 7.3 / 5.3);
#   * the layers' eps with std-0.10 weights (BELOW_ROUNDING): on rows of variance ~40 it moves the exact embeddings by
#     ~1e-8 (measured 9.5e-9 through the gemm8 rounding points: ratio 0.00; 1.41 on classic, where it happens to flip one bf16
#     rounding).  Nothing any bound could see: the test asserts that the exact arithmetic shows it below 1 % of the rel
#     bound, and the std-0.02 weights reject it (15.0 classic, 6.9 gemm8).
NOT_SEPARABLE = {("std010", "classic", "head_eps"): 0.99, ("std010", "gemm8", "head_eps"): 1.36}
BELOW_ROUNDING = {("std010", "classic", "eps"), ("std010", "gemm8", "eps")}
# The kernels' own lean towards a mutation's signature, in units of the bias bound: <= 1 except where measured higher, pinned
# there at 2x the measurement (40 rows: a noise projection reaches 1 - 1.5 here and there; logits x 1.01 shows as in the
# layer test -- 1.91 / 2.38 classic, 2.92 gemm8 with std-0.02 weights: a few percent of the mutation).
LEAN_LIMIT = {
    ("std002", "classic", "logits"): 3.9, ("std002", "classic", "key_minus"): 2.6, ("std002", "classic", "bias"): 2.2,
    ("std002", "gemm8", "eps"): 2.8, ("std002", "gemm8", "logits"): 5.9, ("std002", "gemm8", "gelu_tanh"): 2.8,
    ("std002", "gemm8", "pool_mean"): 2.5, ("std010", "classic", "logits"): 4.8, ("std010", "classic", "key_plus"): 2.7,
    ("std010", "classic", "gelu_tanh"): 2.1, ("std010", "classic", "prev_ln"): 3.2, ("std010", "gemm8", "key_plus"): 2.9,
    ("std010", "gemm8", "pool_row1"): 2.7,
}


@pytest.mark.parametrize("family", list(GEMM))
@pytest.mark.parametrize("kind", ["std002", "std010"])
def test_tail_bounds_reject_every_mutation(kind, family):
    """The self-check of the bounds: every TAIL_MUTATIONS entry, on the kernel's input, lands >= 3x beyond them (rel, bias
    or along its own signature), and the kernel's embeddings do not lean towards any of them beyond LEAN_LIMIT."""
    r = mutation_ratios(kind, family)
    exempt = set(NOT_SEPARABLE) | BELOW_ROUNDING
    weak = {m: v for m, v in r.items() if v[0] < SEPARATION and (kind, family, m) not in exempt}
    leaning = {m: v for m, v in r.items() if v[1] > LEAN_LIMIT.get((kind, family, m), 1.0)}
    assert not weak and not leaning, (kind, family, weak, leaning, r)
    for k in NOT_SEPARABLE:
        if k[:2] == (kind, family):
            assert r[k[2]][0] > 0.5, (k, r[k[2]])     # still measured: a bound twice as loose would hide it entirely
    for k in BELOW_ROUNDING:
        if k[:2] == (kind, family):
            assert (kind, "classic" if family == "gemm8" else "gemm8", k[2]) in BELOW_ROUNDING
            assert exact_effect(kind, k[2]) < 0.01 * BOUNDS[(kind, family, 3)][0], k


def exact_effect(kind, mutate):
    """rel of a mutation in exact arithmetic (family None, from the chained exact reference's state): what no bound of
    rounded kernels could be asked to see when it lies far below their noise."""
    from oracle import ance_oracle
    sd = weights(kind)
    ids, mask = batch("short40")
    st = ance_oracle.ance_embed(sd, ids, mask)
    for i in range(2):
        st = ance_oracle.ance_layer(sd, i, st, mask)
    base = ance_oracle.ance_tail(sd, 2, st, mask).numpy()
    mut = ance_oracle.ance_tail(sd, 2, st, mask, mutate=mutate).numpy()
    return float(np.sqrt(((mut - base) ** 2).mean() / (base ** 2).mean()))
