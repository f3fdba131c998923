"""The attention context per query row and head, observed through a probe layer (test infrastructure; no GPU import here).

ANCEEncoder.layer_state shows a layer's output rows, where the context has gone through the out-projection, a residual ten
times its size, the FFN and two LayerNorms.  probe_weights rewrites layer 0 of a 2-layer synthetic checkpoint so that all of
that is transparent -- out-projection = I (a bf16 GEMM with exact ones and zeros is exact), both LayerNorms unit, FFN = 0,
nothing common to all tokens (embedding LayerNorm unit, no token-type row, no value bias) -- and layer 0's rows become
    classic   LN(xn + ctx)                  in fp32
    gemm8     bf16(LN(bf16(xn + ctx)))      (statistics of the unrounded sum)
with xn the embedding rows (layer_state(..., -1)): features 64h .. 64h+63 of row t are head h's context of query row t times
that row's rstd, minus a mean the reference forms too (closed_form: the corresponding lines of ance_oracle.ance_layer).

Recipes (probe_weights): "flat" leaves Q and K as drawn (logits of sigma ~0.4: nearly uniform weights, every key counts 1/n),
"mid" scales them x 3, "peaked" x 8 (the streaming kernels' softmax reference moves, the woven kernel's fix-up pass runs).
Two sentinel tokens make single keys count: S (= 2, </s>: the last valid token of every sequence) and S2 (= 0, <s>: the first)
have word embeddings SENTINEL_EMB x a unit direction of their own, and the value weight maps that direction onto a +-1
pattern x SENTINEL_GAIN: their V rows are ~15 x the others'.  For the gemm8 family every value weight is scaled by
VALUE_SCALE_GEMM8 on top (its residual stream is bf16: the context has to stand above the rounding of xn + ctx).

Figure per (sequence b, query row t, head h), figure():
    e = rms_64(rows - rows_ref) / (rstd_ref(b, t) . max(rms_64(ctx_ref(b, t, h)), 0.25 . rms of head h's ctx_ref over the sequence))
"""
import numpy as np

SEED = 0xA77E
NH, DH, H = 12, 64, 768
S, S2 = 2, 0                    # what tests.golden.make_golden_encoder.encoder_case_inputs puts last and first
SENTINEL_EMB = 50.0
SENTINEL_GAIN = 8.0
VALUE_SCALE_GEMM8 = 8.0
QK_SCALE = {"flat": 1.0, "mid": 3.0, "peaked": 8.0}
# one sequence per length.  short class (L = 256): 1 .. 8 key blocks of 32, 64-key chunks 1 .. 4 (the fourth wraps the
# three-stage ring), partly filled last blocks; long class (L = 512): odd numbers of 32-row blocks (the woven wave's second
# block empty or partial), waves without rows, 128-key chunks 3 and 4 -- given twice in two orders: the kernels sort by class
# and length, so equal lengths sit next to each other and every length has two packed neighbours over the batch, and
# 32 x 12 items on 256 workgroups make several workgroups walk two items
SHORT_LENS = [1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 160, 191, 192, 193, 224, 255, 256]
LONG_LENS = [257, 288, 289, 320, 321, 352, 383, 384, 385, 416, 448, 449, 480, 481, 511, 512]
LONG_ORDER2 = [512, 257, 481, 288, 449, 320, 416, 352, 384, 383, 385, 321, 448, 289, 480, 511]
BATCHES = {"short": (SHORT_LENS, 256), "long": (LONG_LENS + LONG_ORDER2, 512)}
_SD = {}


def _unit(seed, against=()):
    """A unit vector of zero mean, orthogonal to those in `against`."""
    from haconvdr_amd import synth
    v = synth.normal(seed, (H,)).astype(np.float64)
    v -= v.mean()
    for a in against:
        v -= (v @ a) * a
    return v / np.linalg.norm(v)


def probe_weights(recipe, family="classic"):
    """The 2-layer probe checkpoint (name -> float32 array) of recipe "flat" | "mid" | "peaked" for family "classic" | "gemm8"
    (classic serves the split kernels and the unrounded reference too)."""
    from haconvdr_amd import synth
    key = (recipe, "gemm8" if family == "gemm8" else "classic")
    if key in _SD:
        return _SD[key]
    if "base" not in _SD:
        _SD["base"] = synth.ance_state_dict(SEED, 2)
    sd = dict(_SD["base"])
    e, q = "roberta.embeddings.", "roberta.encoder.layer.0."
    one, zero = np.ones(H, np.float32), np.zeros(H, np.float32)
    sd[e + "LayerNorm.weight"], sd[e + "LayerNorm.bias"] = one, zero
    sd[e + "token_type_embeddings.weight"] = np.zeros_like(sd[e + "token_type_embeddings.weight"])
    sd[q + "attention.output.dense.weight"], sd[q + "attention.output.dense.bias"] = np.eye(H, dtype=np.float32), zero
    sd[q + "attention.output.LayerNorm.weight"], sd[q + "attention.output.LayerNorm.bias"] = one, zero
    for nm in ("intermediate.dense", "output.dense"):
        for part in ("weight", "bias"):
            sd[q + f"{nm}.{part}"] = np.zeros_like(sd[q + f"{nm}.{part}"])
    sd[q + "attention.self.value.bias"] = zero
    u = _unit(SEED + 1)
    u2 = _unit(SEED + 2, (u,))
    word = sd[e + "word_embeddings.weight"].copy()
    word[S], word[S2] = SENTINEL_EMB * u, SENTINEL_EMB * u2
    sd[e + "word_embeddings.weight"] = word
    z, z2 = (np.where(synth.uniform_u32(SEED + 3 + k, H) & 1, 1.0, -1.0) for k in (0, 1))
    wv = sd[q + "attention.self.value.weight"].astype(np.float64) + SENTINEL_GAIN / np.sqrt(H) * (np.outer(z, u) + np.outer(z2, u2))
    sd[q + "attention.self.value.weight"] = (wv * (VALUE_SCALE_GEMM8 if family == "gemm8" else 1.0)).astype(np.float32)
    for nm in ("query", "key"):
        for part in ("weight", "bias"):
            sd[q + f"attention.self.{nm}.{part}"] = (sd[q + f"attention.self.{nm}.{part}"] * QK_SCALE[recipe]).astype(np.float32)
    _SD[key] = sd
    return sd


def batch(lens, L):
    """(ids, mask) int64 [len(lens), L]: S2 first, S last valid, random tokens between."""
    from tests.golden.make_golden_encoder import encoder_case_inputs
    return encoder_case_inputs(0x5EED, list(lens), L)


def closed_form(xn, ctx, family, eps=1e-5):
    """Layer 0's output state on probe weights from its input rows xn and attention context ctx (float64 [B, L, 768]): ance_layer's
    lines with out-projection I, unit LayerNorms and a zero FFN.  Returns (rows, rstd of xn + ctx)."""
    import torch
    from oracle.ance_oracle import _stats, bf16
    y = torch.as_tensor(np.asarray(ctx), dtype=torch.float64) + torch.as_tensor(np.asarray(xn), dtype=torch.float64)
    m, r = _stats(y, eps)
    if family == "gemm8":
        return bf16((bf16(y) - m[..., None]) * r[..., None]), r
    return (y - m[..., None]) * r[..., None], r


def denominator(rstd, ctx):
    """rstd_ref . max(rms_64(ctx_ref), 0.25 . rms of the head's ctx_ref over the sequence's rows), [B, L, NH]; 0 in the padding
    (rstd: [B, L], zero there)."""
    B, L = rstd.shape
    c2 = (np.asarray(ctx, np.float64).reshape(B, L, NH, DH) ** 2).mean(-1)
    n = np.maximum((rstd > 0).sum(1), 1)[:, None, None]
    seq = np.sqrt(c2.sum(1, keepdims=True) / n)
    return rstd[..., None] * np.maximum(np.sqrt(c2), 0.25 * seq)


def reference(sd, x_in, mask, family, attn="stream", mutate=None, where=None, qkv=None):
    """(rows_ref [B, L, 768], den [B, L, NH]) as float64 arrays: closed_form of ance_attention on the state x_in of the
    embedding stage, and figure()'s denominator; zeros in the padding."""
    from oracle import ance_oracle
    ctx = ance_oracle.ance_attention(sd, 0, x_in, mask, family, attn, mutate=mutate, where=where, qkv=qkv)
    valid = np.asarray(mask, bool)
    rows, r = closed_form(np.asarray(x_in["rows"], np.float64), ctx, family)
    return rows.numpy() * valid[..., None], denominator(r.numpy() * valid, ctx.numpy())


def figure(rows, ref):
    """e [B, L, NH] of `rows` against ref = (rows_ref, den) of reference(); 0 in the padding."""
    rows_ref, den = ref
    B, L, _ = rows_ref.shape
    d = (np.asarray(rows, np.float64) - rows_ref).reshape(B, L, NH, DH)
    return np.where(den > 0, np.sqrt((d ** 2).mean(-1)) / np.where(den > 0, den, 1.0), 0.0)


def worst(e, lens, k=10):
    """The k largest slices of e as (figure, length, row, head): the position is the diagnosis."""
    flat = np.argsort(e, axis=None)[::-1][:k]
    return [(float(f"{e[b, t, h]:.3e}"), int(lens[b]), int(t), int(h)) for b, t, h in zip(*np.unravel_index(flat, e.shape))]


def assert_within(e, bound, lens, what):
    assert np.isfinite(e).all() and e.max() <= bound, (what, "bound", bound, "worst (figure, length, row, head)", worst(e, lens))


def slices(lens, pick_lens, heads=(0, 5, 11)):
    """{(b, t, h)}: first, middle and last row x heads of the first sequence of each length in pick_lens."""
    out = set()
    for n in pick_lens:
        b = list(lens).index(n)
        out |= {(b, t, h) for t in (0, n // 2, n - 1) for h in heads}
    return out
