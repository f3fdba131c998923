"""ORACLE — TEST INFRASTRUCTURE ONLY.

fp32 CPU restatement (torch ops) of the reference's encoder path:
  ANCE.forward / query_emb / masked_mean_or_first   /root/reference/src/models.py:39-64
  RobertaModel forward (third-party: transformers, pinned 4.2.0 at README.md:11; 5.15.0 is
  what is installed in the authoring container and what the goldens were produced with).
The arithmetic restated is the published RoBERTa-base forward (post-LN BERT block):
  emb = LN(word[id] + pos[cumsum(id != 1)*(id != 1) + 1] + type[0])
  x   = LN(x + Wo . softmax(Q K^T / sqrt(64) + mask) V)        (12 heads x 64)
  x   = LN(x + W2 . gelu_erf(W1 . x))
  out = LN_768(embeddingHead(x[:, 0]))                           (use_mean = False, models.py:30,:56)
Pinned against the reference itself: tests/golden/encoder_*.npz hold outputs of the reference's
``models.ANCE`` (run by tests/golden/make_golden_encoder.py) on seeded synthetic weights/inputs.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F


def _t(sd, name):
    v = sd[name]
    return v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))


def ance_forward(sd, input_ids, attention_mask, n_layers=None, n_heads=12, eps=1e-5, pad_id=1, hidden=False):
    """sd: name -> float32 array (reference checkpoint names).  input_ids/attention_mask: int [B, L].
    Returns float32 ndarray [B, 768] (= the reference's model(input_ids, attention_mask)); hidden=True: instead the list of
    hidden states [B, L, 768] (float32 ndarrays) after the embedding LayerNorm and after every layer (rows beyond a sequence's
    length are whatever the padded forward makes of them)."""
    ids = torch.as_tensor(np.asarray(input_ids), dtype=torch.long)
    mask = torch.as_tensor(np.asarray(attention_mask), dtype=torch.long)
    B, L = ids.shape
    if n_layers is None:
        n_layers = 1 + max(int(k.split(".")[3]) for k in sd if k.startswith("roberta.encoder.layer."))
    p = "roberta.embeddings."
    nonpad = (ids != pad_id).long()
    pos = torch.cumsum(nonpad, 1) * nonpad + pad_id                     # HF create_position_ids_from_input_ids
    x = _t(sd, p + "word_embeddings.weight")[ids] + _t(sd, p + "position_embeddings.weight")[pos] \
        + _t(sd, p + "token_type_embeddings.weight")[0]
    H = x.shape[-1]
    x = F.layer_norm(x, (H,), _t(sd, p + "LayerNorm.weight"), _t(sd, p + "LayerNorm.bias"), eps)
    dh = H // n_heads
    add_mask = (1.0 - mask.float())[:, None, None, :] * torch.finfo(torch.float32).min
    hs = [x]
    for i in range(n_layers):
        q = f"roberta.encoder.layer.{i}."

        def lin(name, t):
            return F.linear(t, _t(sd, q + name + ".weight"), _t(sd, q + name + ".bias"))

        def heads(t):
            return t.view(B, L, n_heads, dh).transpose(1, 2)
        Q, K, V = heads(lin("attention.self.query", x)), heads(lin("attention.self.key", x)), heads(lin("attention.self.value", x))
        s = Q @ K.transpose(-1, -2) / math.sqrt(dh) + add_mask
        ctx = (torch.softmax(s, -1) @ V).transpose(1, 2).reshape(B, L, H)
        x = F.layer_norm(x + lin("attention.output.dense", ctx), (H,), _t(sd, q + "attention.output.LayerNorm.weight"),
                         _t(sd, q + "attention.output.LayerNorm.bias"), eps)
        h = F.gelu(lin("intermediate.dense", x))                         # exact erf GELU (hidden_act = "gelu")
        x = F.layer_norm(x + lin("output.dense", h), (H,), _t(sd, q + "output.LayerNorm.weight"),
                         _t(sd, q + "output.LayerNorm.bias"), eps)
        hs.append(x)
    if hidden:
        return [h.numpy().astype(np.float32) for h in hs]
    cls = x[:, 0]                                                        # masked_mean_or_first, use_mean=False
    e = F.linear(cls, _t(sd, "embeddingHead.weight"), _t(sd, "embeddingHead.bias"))
    out = F.layer_norm(e, (e.shape[-1],), _t(sd, "norm.weight"), _t(sd, "norm.bias"), 1e-5)
    return out.numpy().astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# One stage at a time, fp64, with the HIP kernels' bf16 rounding points (tests/test_encoder_layers_gpu.py: teacher-forced parity)

LAYER_MUTATIONS = ("eps", "logits", "key_plus", "key_minus", "bias", "gelu_tanh")   # what ance_layer(mutate=...) knows
ATTN_MUTATIONS = ("logits", "key_plus", "key_minus", "key_next", "top_key", "head_next", "block_stale")   # ance_attention's, local
CHUNK_MUTATIONS = ("key_chunk",)      # of the split attention kernel's 64-key chunk loop (tests/test_encoder_precision_shapes_gpu.py)
EMBED_MUTATIONS = ("eps", "pos")                                                    # what ance_embed(mutate=...) knows
LOG2E = 1.4426950408889634


def bf16(t):
    """Round to bf16 (nearest even) and back: the kernels' (bf16) conversions of fp32 values."""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def split2(t):
    """The pair rounding of precision = split: v -> bf16(v) + bf16(v - bf16(v)), hi + lo summed in fp64 (host twin of the
    kernels' helper: haconvdr_amd.encoder.split_bf16; the difference is formed in fp32 as there -- it is exact)."""
    t32 = t.to(torch.float32)
    hi = t32.to(torch.bfloat16).to(torch.float32)
    lo = (t32 - hi).to(torch.bfloat16)
    return hi.to(torch.float64) + lo.to(torch.float64)


FAMILIES = (None, "classic", "gemm8", "split")


def _rounding(family):
    """The rounding a family applies where the classic kernels convert to bf16: none (family None), bf16, or the hi + lo pair
    ("split": the arithmetic of "classic" with every bf16(.) replaced by split2(.))."""
    return (lambda t: t) if not family else (split2 if family == "split" else bf16)


def _t64(sd, name):
    return _t(sd, name).to(torch.float64)


def _stats(y, eps):
    mean = y.mean(-1)
    var = ((y - mean[..., None]) ** 2).mean(-1)
    return mean, 1.0 / torch.sqrt(var + eps)


def _state(rows, mean, rstd, gamma, beta):
    return {"rows": rows, "mean": mean, "rstd": rstd, "norm": (rows - mean[..., None]) * rstd[..., None] * gamma + beta}


def ance_embed(sd, input_ids, attention_mask, family=None, eps=1e-5, pad_id=1, mutate=None):
    """Embedding stage, fp64: LN(word[id] + type[0] + pos[HF position id]) of every token (mask: the prefix of valid tokens).
    Returns the state dict of ance_layer ({rows, mean, rstd, norm} as torch float64 over [B, L]); the rows are already
    normalized (mean 0, rstd 1, norm = rows).  family "classic": rows are fp32 (embed_ln_kernel, encoder.hip: ln768_store writes
    x_f32 unrounded) -- modelled as exact; "gemm8": the rows are stored only as bf16 (ln768_store's x_bf; fwd_build passes
    x_f32 = nullptr on that path); "split": as classic (the pair of the rows is formed by the consumer).  mutate: "eps" (LayerNorm eps 1e-12) or "pos" (position ids one too high, the last one clamped to the table)."""
    ids = torch.as_tensor(np.asarray(input_ids), dtype=torch.long)
    mask = torch.as_tensor(np.asarray(attention_mask), dtype=torch.long)
    p = "roberta.embeddings."
    nonpad = (ids != pad_id).long()
    pos = torch.cumsum(nonpad, 1) * nonpad + pad_id
    if mutate == "pos":
        pos = torch.clamp(pos + 1, max=_t(sd, p + "position_embeddings.weight").shape[0] - 1)
    x = (_t64(sd, p + "word_embeddings.weight")[ids] + _t64(sd, p + "token_type_embeddings.weight")[0]) \
        + _t64(sd, p + "position_embeddings.weight")[pos]
    mean, rstd = _stats(x, 1e-12 if mutate == "eps" else eps)
    x = (x - mean[..., None]) * rstd[..., None] * _t64(sd, p + "LayerNorm.weight") + _t64(sd, p + "LayerNorm.bias")
    if family == "gemm8":
        x = bf16(x)
    x = x * mask[..., None]
    one = mask.to(torch.float64)
    return {"rows": x, "mean": torch.zeros_like(one), "rstd": one, "norm": x}


ATT_TAU = 64.0   # encoder.hip ATT_TAU: how far (log2) a score may rise above the streaming kernels' softmax reference


def _window_reference(lg):
    """The streaming attention kernels' softmax reference per query row and 32-key block (attention_stream_kernel, round 6
    rule, shared by attn_pipe.inc and the fix-up pass): m starts at 0 and moves to the block's maximum only when that
    lies more than ATT_TAU above it (or, first block, more than ATT_TAU below).  lg: base-2 logits [..., n, nk].
    Returns m after each block, [..., n, nblocks]."""
    ms, m = [], torch.zeros(lg.shape[:-1], dtype=lg.dtype)
    for kb in range(0, lg.shape[-1], 32):
        d = lg[..., kb:kb + 32].max(-1).values - m
        move = (d > ATT_TAU) | ((d < -ATT_TAU) if kb == 0 else torch.zeros_like(d, dtype=torch.bool))
        m = torch.where(move, m + d, m)
        ms.append(m)
    return torch.stack(ms, -1)


def _layer_input(sd, i, x_in):
    """Layer i's input state as float64 tensors: (rows, mean, rstd, gamma, beta, LN(rows)) with the previous layer's output
    LayerNorm (gamma, beta) -- layer 0: (1, 0), the embedding rows are already normalized.  LN(rows) is what both families
    form in fp32 for the residual adds (and the classic family rounds to bf16 for its QKV A operand)."""
    x, mean, rstd = (torch.as_tensor(np.asarray(x_in[k])).to(torch.float64) for k in ("rows", "mean", "rstd"))
    H = x.shape[-1]
    pq = f"roberta.encoder.layer.{i - 1}.output.LayerNorm."
    g_in = _t64(sd, pq + "weight") if i else torch.ones(H, dtype=torch.float64)
    b_in = _t64(sd, pq + "bias") if i else torch.zeros(H, dtype=torch.float64)
    xn = (x - mean[..., None]) * rstd[..., None] * g_in + b_in
    return x, mean, rstd, g_in, b_in, xn


def _folded(A, m, r, Wf, bias, gamma, beta, scale=1.0):
    """rstd (A.W'^T - mean wsum) + cvec (gemm8 QKV / FFN-up epilogue, cls_q_kernel), W' = bf16(W.diag(gamma).scale)."""
    Wp = bf16(Wf * gamma * scale)
    return r[..., None] * (A @ Wp.T - m[..., None] * Wp.sum(1)) + (bias + Wf @ beta) * scale


def _project(sd, i, nm, x, mean, rstd, xn, g_in, b_in, family, n_heads, mutate=None):
    """Layer i's attention projection nm ("query": scaled by log2(e)/sqrt(dh) before its rounding, "key", "value") of the
    input rows x [..., H] with their (mean, rstd) and LN(x) = xn (_layer_input), bf16 as the family stores it."""
    p = f"roberta.encoder.layer.{i}.attention.self.{nm}."
    Wf = _t64(sd, p + "weight")
    bias = torch.zeros(Wf.shape[0], dtype=torch.float64) if (nm == "value" and mutate == "bias") else _t64(sd, p + "bias")
    c = LOG2E / math.sqrt(x.shape[-1] // n_heads)
    if family == "gemm8":
        return bf16(_folded(x, mean, rstd, Wf, bias, g_in, b_in, c if nm == "query" else 1.0))
    R = _rounding(family)
    A = R(xn)
    return R((A @ R(Wf).T + bias) * c) if nm == "query" else R(A @ R(Wf).T + bias)


def _attend(Qs, K, V, n, n_heads, family, attn, mutate=None, nxt=None):
    """Attention context [nq, H] of the query rows Qs [nq, H] (base 2, _project) of one sequence of n valid rows over its
    keys and values K, V [>= n, H]: the arithmetic of ance_layer's docstring (mutations "logits", "key_plus", "key_minus";
    ance_attention's: "key_next" with nxt = (k, v), one more key row [H] each, "top_key", "head_next", "block_stale")."""
    R = _rounding(family)
    nq, H = Qs.shape
    dh = H // n_heads
    nk = min(K.shape[0], n + 1) if mutate == "key_plus" else (max(1, n - 1) if mutate == "key_minus" else n)
    if mutate == "key_chunk":
        nk = min(K.shape[0], (n + 63) // 64 * 64)
    K, V = K[:nk], V[:nk]
    if mutate == "key_next":
        K, V, nk = torch.cat([K, nxt[0][None]]), torch.cat([V, nxt[1][None]]), nk + 1
    qh = Qs.reshape(nq, n_heads, dh).transpose(0, 1)
    kh = K.reshape(nk, n_heads, dh).transpose(0, 1)
    vh = V.reshape(nk, n_heads, dh).transpose(0, 1)
    if mutate == "head_next":
        vh = vh.roll(-1, 0)
    lg = qh @ kh.transpose(-1, -2)                                         # base-2 logits
    if mutate == "logits":
        lg = lg * 1.01
    if mutate == "top_key" and nk > 1:                                     # (weight exactly 0, and out of every maximum)
        lg = lg.masked_fill(F.one_hot(lg.argmax(-1), nk).bool(), -1e30)
    if family and attn == "stream":
        mb = _window_reference(lg)                                         # [heads, nq, blocks]
        mk = mb.repeat_interleave(32, -1)[..., :nk]                        # the reference in force at each key's block
        P = torch.exp2(lg - mb[..., -1:])
        Pr = R(torch.exp2(lg - mk)) * torch.exp2(mk - mb[..., -1:])
        if mutate == "block_stale":                                        # l and O of the earlier blocks never rescaled
            P = torch.exp2(lg - mk)
            Pr = R(P)
    else:
        P = torch.exp2(lg - lg.max(-1, keepdim=True).values)
        Pr = R(P)
    o = (Pr @ vh) / P.sum(-1, keepdim=True)
    return R(o).transpose(0, 1).reshape(nq, H)


def ance_qkv(sd, i, x_in, family=None, n_heads=12):
    """(Q, K, V) of layer i, float64 [B, L, H] as the family stores them (_project), from the state x_in of ance_layer."""
    x, mean, rstd, g_in, b_in, xn = _layer_input(sd, i, x_in)
    return tuple(_project(sd, i, nm, x, mean, rstd, xn, g_in, b_in, family, n_heads) for nm in ("query", "key", "value"))


def attention_moves(qkv, attention_mask, n_heads=12):
    """bool [B, L, heads]: the (row, head) slices whose streaming softmax reference moves at a key block after the first
    (_window_reference) -- the only ones that "block_stale" changes."""
    Q, K, _ = qkv
    B, L, H = Q.shape
    lens = torch.as_tensor(np.asarray(attention_mask), dtype=torch.long).sum(1).tolist()
    out = torch.zeros(B, L, n_heads, dtype=torch.bool)
    for s, n in enumerate(lens):
        lg = Q[s, :n].reshape(n, n_heads, -1).transpose(0, 1) @ K[s, :n].reshape(n, n_heads, -1).transpose(0, 1).transpose(-1, -2)
        mb = _window_reference(lg)
        out[s, :n] = (mb[..., 1:] != mb[..., :-1]).any(-1).transpose(0, 1)
    return out


def ance_attention(sd, i, x_in, attention_mask, family=None, attn="stream", mutate=None, where=None, n_heads=12, qkv=None):
    """Layer i's attention context alone, float64 [B, L, H] (zeros beyond each sequence's length): ance_layer's Q, K, V and
    attend step on the state x_in, nothing behind them (tests/attn_probe.py observes it through a transparent layer).
    qkv: ance_qkv's result for the same (sd, i, x_in, family), to share it among calls.

    mutate (ATTN_MUTATIONS), applied in the slices where = {(b, t, h)} only (None: in every slice): "logits" / "key_plus" /
    "key_minus" as in ance_layer, and
      "key_next"    the row also attends the first row of the next sequence of the batch ((b + 1) % B) with that row's own K
                    and V: what a kernel over packed rows reads one past a sequence's end;
      "top_key"     the key with the row's largest logit is dropped (lengths > 1);
      "head_next"   V of head (h + 1) % n_heads;
      "block_stale" (family set, attn = "stream") when the softmax reference moves at a key block, the sum and the context
                    of the blocks before it are not rescaled (a no-op in the rows of which attention_moves says False)."""
    assert family in FAMILIES and attn in ("stream", "twopass") and (mutate is None or mutate in ATTN_MUTATIONS), (family, attn, mutate)
    assert mutate != "block_stale" or (family and attn == "stream"), (family, attn)
    lens = torch.as_tensor(np.asarray(attention_mask), dtype=torch.long).sum(1).tolist()
    Q, K, V = qkv if qkv is not None else ance_qkv(sd, i, x_in, family, n_heads)
    B, L, H = Q.shape
    dh = H // n_heads
    ctx = torch.zeros(B, L, H, dtype=torch.float64)
    for s, n in enumerate(lens):
        nxt = (K[(s + 1) % B, 0], V[(s + 1) % B, 0])
        if mutate is None or where is not None:
            ctx[s, :n] = _attend(Q[s, :n], K[s], V[s], n, n_heads, family, attn)
        else:
            ctx[s, :n] = _attend(Q[s, :n], K[s], V[s], n, n_heads, family, attn, mutate, nxt)
        rows = sorted({t for b, t, _ in where if b == s}) if (mutate and where is not None) else []
        if rows:
            mut = _attend(Q[s, rows], K[s], V[s], n, n_heads, family, attn, mutate, nxt)
            for b, t, h in where:
                if b == s:
                    ctx[s, t, h * dh:(h + 1) * dh] = mut[rows.index(t), h * dh:(h + 1) * dh]
    return ctx


def ance_layer(sd, i, x_in, attention_mask, family=None, n_heads=12, eps=1e-5, mutate=None, attn="stream"):
    """Encoder layer i in fp64 from the state the layers before it left: x_in = {rows, mean, rstd} over [B, L, ...] (arrays or
    tensors: the kernels' own hac_encoder_layer_state output -- teacher forcing -- or this function's / ance_embed's), the rows
    being pre-LayerNorm with layer i-1's output LayerNorm still to apply (i = 0: the normalized embedding rows, statistics
    (0, 1)).  Returns {rows, mean, rstd, norm} of layer i (float64 tensors, zeros beyond each sequence's length): pre-LayerNorm
    rows, their exact statistics, and LN(rows) with this layer's output LayerNorm.

    family None: no rounding at all -- layer for layer the arithmetic of ance_forward.  Otherwise bf16 exactly where the
    kernels round (haconvdr_amd/csrc; everything else is fp64: true erf, exact softmax, exact statistics):
      both families
        * weights of every GEMM are bf16 (hac_encoder_finalize: f32_to_bf16_kernel / to_bf16 for wqkv, wo, w1, w2; gemm8
          reads wo, w2 unfolded, and fold_ln_kernel rounds W.diag(gamma).scale for wqkv8, w18);
        * Q is scaled by log2(e)/8 BEFORE its rounding (gemm_bf16_nt_kernel EPI_QKV "sc"; gemm8: the scale is folded into
          wqkv8's q rows and cvec, finalize "qscale"); Q, K, V are bf16 (EPI_QKV / EPI8_QKV pack_bf16);
        * attention (attention_stream_kernel / attention_kernel / attn_pipe.inc): logits s = Q.K in base 2, P = 2^(s - m)
          unrounded in the row sum l, bf16(P) as the PV MFMA operand, context = bf16(O / l).  The reference m is where
          bf16(P) rounds: attn="twopass" (attention_kernel) takes the exact row maximum; attn="stream" (the streaming,
          woven and query-split kernels) the window rule of _window_reference, a block's P rounded relative to the m of
          that block and rescaled exactly (fp32 factor 2^-delta on l and O) when m moves later;
      classic (gemm_bf16_nt_kernel, ln_stats_rows_kernel): the residual stream is fp32 (modelled exact); the A operands of QKV
        and FFN-up are bf16(LN(y)) (ln_stats_rows_kernel x_bf, embed: ln768_store x_bf); FFN-up stores bf16(gelu(.))
        (EPI_GELU); the RESID epilogues add the fp32 residual LN(y) recomputed from (mean, rstd) (fmaf form);
      gemm8 (gemm8.inc): the residual stream is bf16 -- the RESID epilogue stores bf16(acc + bias + residual) and takes
        (mean, rstd) from the fp32 values before that rounding (partial sums -> ln_combine_kernel); the consumer's LayerNorm
        is folded: out = rstd (A.W'^T - mean wsum) + cvec with W' = bf16(W.diag(gamma)), wsum = sum_k W' (of the rounded
        values), cvec = bias + W.beta (fold_ln_kernel); layer 0 folds nothing (gamma = 1, beta = 0: the embedding rows are
        normalized); the residual of the RESID epilogues is (bf16 row - mean) rstd gamma + beta; FFN-up stores bf16(gelu).

      split (split.inc, precision = split): the classic family's arithmetic with every bf16(.) above replaced by the pair rounding
        split2(.) = bf16(v) + bf16(v - bf16(v)), hi + lo summed exactly (the dropped lo.lo terms and the fp32 accumulation are
        not modelled).  Not what the split kernels are compared with -- that is family None -- but the yardstick of their
        bounds (tests/split_parity.py: E_emul).

    mutate (the self-checks of the tests): "eps" (both LayerNorms with eps 1e-12), "logits" (x 1.01), "key_plus" /
    "key_minus" (every sequence attends one key more -- the pad row behind it -- or one fewer), "bias" (the value
    projection's bias dropped), "gelu_tanh" (tanh-approximate GELU); of CHUNK_MUTATIONS, "key_chunk" (every sequence whose
    length is no multiple of 64 attends the keys up to the next multiple of 64, clamped to the rows that exist: a wrong
    masked-step condition in the split attention kernel's 64-key chunk loop)."""
    assert family in FAMILIES and attn in ("stream", "twopass") and (mutate is None or mutate in LAYER_MUTATIONS + CHUNK_MUTATIONS), \
        (family, attn, mutate)
    R = _rounding(family)
    lens = torch.as_tensor(np.asarray(attention_mask), dtype=torch.long).sum(1).tolist()
    x, mean, rstd, g_in, b_in, xn = _layer_input(sd, i, x_in)
    B, L, H = x.shape
    q = f"roberta.encoder.layer.{i}."
    leps = 1e-12 if mutate == "eps" else eps

    def W(name):
        return _t64(sd, q + name + ".weight")

    def b(name):
        return _t64(sd, q + name + ".bias")

    Q, K, V = (_project(sd, i, nm, x, mean, rstd, xn, g_in, b_in, family, n_heads, mutate) for nm in ("query", "key", "value"))
    ctx = torch.zeros(B, L, H, dtype=torch.float64)
    for s in range(B):
        n = lens[s]
        ctx[s, :n] = _attend(Q[s, :n], K[s], V[s], n, n_heads, family, attn, mutate)
    gelu = (lambda t: F.gelu(t, approximate="tanh")) if mutate == "gelu_tanh" else F.gelu
    if family == "gemm8":
        yA = ctx @ bf16(W("attention.output.dense")).T + b("attention.output.dense") + xn
        mA, rA = _stats(yA, leps)
        yA = bf16(yA)
        g1, b1 = _t64(sd, q + "attention.output.LayerNorm.weight"), _t64(sd, q + "attention.output.LayerNorm.bias")
        h = bf16(gelu(_folded(yA, mA, rA, W("intermediate.dense"), b("intermediate.dense"), g1, b1)))
        xa = (yA - mA[..., None]) * rA[..., None] * g1 + b1
        yF = h @ bf16(W("output.dense")).T + b("output.dense") + xa
        mF, rF = _stats(yF, leps)
        yF = bf16(yF)
    else:
        yA = ctx @ R(W("attention.output.dense")).T + b("attention.output.dense") + xn
        mA, rA = _stats(yA, leps)
        xa = (yA - mA[..., None]) * rA[..., None] * _t64(sd, q + "attention.output.LayerNorm.weight") \
            + _t64(sd, q + "attention.output.LayerNorm.bias")
        h = R(gelu(R(xa) @ R(W("intermediate.dense")).T + b("intermediate.dense")))
        yF = h @ R(W("output.dense")).T + b("output.dense") + xa
        mF, rF = _stats(yF, leps)
    valid = (torch.arange(L)[None, :] < torch.as_tensor(lens)[:, None]).to(torch.float64)
    out = _state(yF, mF, rF, _t64(sd, q + "output.LayerNorm.weight"), _t64(sd, q + "output.LayerNorm.bias"))
    return {k: v * (valid[..., None] if v.dim() == 3 else valid) for k, v in out.items()}


# the last layer and the ANCE head (tests/test_encoder_tail_gpu.py): the layer's mutations, then the tail's own
TAIL_MUTATIONS = LAYER_MUTATIONS + ("prev_ln", "pool_mean", "pool_row1", "head_eps", "head_bias", "head_bf16")


def _head(sd, x, mutate=None):
    """ANCE head on the pooled rows x [B, H]: LN_768(embeddingHead(x)), fp32 weights and activations (cls_head_proj_kernel,
    cls_head_norm_kernel: eps 1e-5 whatever the layers' eps).  mutate: "head_eps" (eps 1e-12), "head_bias" (embeddingHead's
    bias dropped), "head_bf16" (its weight and input rounded to bf16)."""
    Wh, bh = _t64(sd, "embeddingHead.weight"), _t64(sd, "embeddingHead.bias")
    if mutate == "head_bias":
        bh = torch.zeros_like(bh)
    if mutate == "head_bf16":
        Wh, x = bf16(Wh), bf16(x)
    e = x @ Wh.T + bh
    m, r = _stats(e, 1e-12 if mutate == "head_eps" else 1e-5)
    return (e - m[:, None]) * r[:, None] * _t64(sd, "norm.weight") + _t64(sd, "norm.bias")


def ance_tail(sd, i, x_in, attention_mask, family=None, n_heads=12, eps=1e-5, mutate=None, attn="stream"):
    """The last encoder layer i and the ANCE head in fp64 from the state the layers before it left (x_in as for ance_layer;
    i = 0: ance_embed's state).  Returns the embeddings, float64 [B, H] (= ance_forward's output when family is None).

    Only what the kernels compute (encoder.hip tail_classic / tail_split): keys and values of every row, the query of row 0 of each sequence,
    its attention (cls_only), then out-projection, LayerNorm, FFN and LayerNorm on the gathered <s> rows, and the head.
      classic (and split, with its pair rounding): Q, K, V as in ance_layer;
      gemm8: K, V folded as in ance_layer; the <s> query in the same folded form, scale folded in, bf16 (cls_q_kernel);
      both, the <s> rows (gather_cls_kernel, then gemm_bf16_nt_kernel and ln_rows_kernel on the compact matrices, on gemm8
      too): x_c = LN_prev(row) in fp32 (gemm8: of the bf16 row); y = bf16(ctx).bf16(Wo)^T + bo + x_c and x2 = LN1(y) in
      fp32; h = bf16(gelu(bf16(x2).bf16(W1)^T + b1)); x_out = LN2(h.bf16(W2)^T + b2 + x2) in fp32; then _head.

    mutate: LAYER_MUTATIONS for this layer, or "prev_ln" (the gather normalizes with this layer's own output LayerNorm
    instead of the previous layer's), "pool_mean" (masked mean of every row's layer output -- ance_layer's -- instead of
    row 0), "pool_row1" (row min(1, len - 1) instead of row 0), and the head's of _head."""
    assert family in FAMILIES and attn in ("stream", "twopass") and (mutate is None or mutate in TAIL_MUTATIONS + CHUNK_MUTATIONS), \
        (family, attn, mutate)
    R = _rounding(family)
    mask = torch.as_tensor(np.asarray(attention_mask), dtype=torch.long)
    lens = mask.sum(1).tolist()
    lmut = mutate if mutate in LAYER_MUTATIONS + CHUNK_MUTATIONS else None
    q = f"roberta.encoder.layer.{i}."
    if mutate == "pool_mean":
        st = ance_layer(sd, i, x_in, attention_mask, family, n_heads, eps, attn=attn)
        return _head(sd, st["norm"].sum(1) / torch.as_tensor(lens, dtype=torch.float64)[:, None])
    x, mean, rstd, g_in, b_in, xn = _layer_input(sd, i, x_in)
    B = x.shape[0]
    sel = (torch.arange(B), torch.as_tensor([min(1, n - 1) if mutate == "pool_row1" else 0 for n in lens]))
    Q = _project(sd, i, "query", x[sel], mean[sel], rstd[sel], xn[sel], g_in, b_in, family, n_heads)
    K, V = (_project(sd, i, nm, x, mean, rstd, xn, g_in, b_in, family, n_heads, lmut) for nm in ("key", "value"))
    ctx = torch.cat([_attend(Q[s:s + 1], K[s], V[s], lens[s], n_heads, family, attn, lmut) for s in range(B)])
    if mutate == "prev_ln":
        x_c = (x[sel] - mean[sel][:, None]) * rstd[sel][:, None] * _t64(sd, q + "output.LayerNorm.weight") \
            + _t64(sd, q + "output.LayerNorm.bias")
    else:
        x_c = xn[sel]
    leps = 1e-12 if mutate == "eps" else eps

    def W(name):
        return R(_t64(sd, q + name + ".weight"))

    def b(name):
        return _t64(sd, q + name + ".bias")

    def ln(y, name):
        m, r = _stats(y, leps)
        return (y - m[:, None]) * r[:, None] * _t64(sd, q + name + ".weight") + _t64(sd, q + name + ".bias")
    gelu = (lambda t: F.gelu(t, approximate="tanh")) if mutate == "gelu_tanh" else F.gelu
    x2 = ln(ctx @ W("attention.output.dense").T + b("attention.output.dense") + x_c, "attention.output.LayerNorm")
    h = R(gelu(R(x2) @ W("intermediate.dense").T + b("intermediate.dense")))
    x_out = ln(h @ W("output.dense").T + b("output.dense") + x2, "output.LayerNorm")
    return _head(sd, x_out, mutate)
