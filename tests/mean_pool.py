"""Host helper of the mean-pooling tests (test infrastructure): masked mean of a hidden state and the ANCE head, fp64.

The reference pools ``sum(t * mask) / sum(mask)`` over the last hidden state and applies ``norm(embeddingHead(.))``
(src/models.py:39-61, use_mean = True).  ``pool_and_head`` restates that on a normalized state [B, L, 768];
``pool_rows_and_head`` on the kernels' own view of the last layer -- un-normalized rows, their (mean, rstd) and the last layer's
output LayerNorm (hac_encoder_layer_state, pool_mean_kernel's input) -- which is what the teacher-forced GPU tests use.
``emulate_pool_mean_kernel`` is the fp32 restatement of pool_mean_kernel's sums, from which tests/test_encoder_mean_pool.py
derives the GPU tests' pool-stage bound.
"""
import numpy as np

H = 768


def lens_of(mask):
    return np.asarray(mask).astype(np.int64).sum(1)


def masked_mean(state, mask):
    """[B, L, 768] normalized hidden state -> fp64 [B, 768]: the mean of each sequence's first len rows."""
    state, lens = np.asarray(state, np.float64), lens_of(mask)
    return np.stack([state[b, :n].sum(0) / n for b, n in enumerate(lens)])


def head(sd, pooled):
    """LN_768(embeddingHead(pooled)) in fp64, eps 1e-5: the arithmetic of oracle.ance_oracle._head, restated."""
    pooled = np.asarray(pooled, np.float64)
    e = pooled @ np.asarray(sd["embeddingHead.weight"], np.float64).T + np.asarray(sd["embeddingHead.bias"], np.float64)
    m = e.mean(-1, keepdims=True)
    r = 1.0 / np.sqrt(((e - m) ** 2).mean(-1, keepdims=True) + 1e-5)
    return (e - m) * r * np.asarray(sd["norm.weight"], np.float64) + np.asarray(sd["norm.bias"], np.float64)


def pool_and_head(sd, state, mask):
    return head(sd, masked_mean(state, mask))


def last_ln(sd, n_layers):
    q = f"roberta.encoder.layer.{n_layers - 1}.output.LayerNorm."
    return np.asarray(sd[q + "weight"], np.float64), np.asarray(sd[q + "bias"], np.float64)


def pool_rows(rows, mean, rstd, gamma, beta, lens, pad_to=1):
    """fp64 [B, 768]: (1 / n) sum_{t < n} ((rows_t - mean_t) rstd_t gamma + beta), n = len rounded up to pad_to.  pad_to = 1 is
    the pooling; pad_to = 32 is the tests' mutation -- a kernel that walks the sequence's padded rows: the dead rows are zeros
    with statistics (0, 0), i.e. beta under the LayerNorm, and the divisor counts them too."""
    rows, mean, rstd = (np.asarray(v, np.float64) for v in (rows, mean, rstd))
    out = []
    for b, n in enumerate(lens):
        n = int(n)
        n_pad = (n + pad_to - 1) // pad_to * pad_to
        live = (((rows[b, :n] - mean[b, :n, None]) * rstd[b, :n, None]) * gamma + beta).sum(0)
        out.append((live + (n_pad - n) * beta) / n_pad)
    return np.stack(out)


def pool_rows_and_head(sd, n_layers, state, mask, pad_to=1):
    """Embeddings from a layer_state dict ({rows, mean, rstd}) of the last layer."""
    g, b = last_ln(sd, n_layers)
    return head(sd, pool_rows(state["rows"], state["mean"], state["rstd"], g, b, lens_of(mask), pad_to))


def emulate_pool_mean_kernel(rows, mean, rstd, gamma, beta, row_groups):
    """pool_mean_kernel's arithmetic in fp32 for EVERY prefix length of one sequence: rows [n, 768] float32 (the stored values:
    bf16-representable on gemm8), mean / rstd [n] float32, gamma / beta [768] float32; row_groups = 16 (bf16 rows) or 8 (fp32).
    Per element fmaf((v - mean) * rstd, gamma, beta); row group rg adds its rows rg, rg + RG, ... in order; the RG partial sums
    are added in the order 0 .. RG - 1; the total is divided by float(len).  Returns float32 [n, 768], row len - 1 = the pooled
    row of the prefix of len rows.  (The fma is formed in fp64 and rounded once to fp32: the product of two fp32 values is exact
    there.)"""
    rows, mean, rstd, gamma, beta = (np.asarray(v, np.float32) for v in (rows, mean, rstd, gamma, beta))
    n, RG = len(rows), row_groups
    a = ((rows - mean[:, None]) * rstd[:, None]).astype(np.float32)
    norm = (a.astype(np.float64) * gamma.astype(np.float64) + beta.astype(np.float64)).astype(np.float32)
    steps = (n + RG - 1) // RG
    padded = np.zeros((steps * RG, H), np.float32)
    padded[:n] = norm
    cums = np.cumsum(padded.reshape(steps, RG, H), axis=0, dtype=np.float32)     # sequential fp32 sums within a row group
    out = np.empty((n, H), np.float32)
    for ln in range(1, n + 1):
        total = np.zeros(H, np.float32)
        for rg in range(RG):
            cnt = (ln - rg + RG - 1) // RG if ln > rg else 0
            total = total + (cums[cnt - 1, rg] if cnt else np.float32(0.0))
        out[ln - 1] = total / np.float32(ln)
    return out


def head_fp32(sd, pooled):
    """The head in fp32 torch (cls_head_proj_kernel / cls_head_norm_kernel keep fp32 weights, activations and statistics)."""
    import torch
    import torch.nn.functional as F
    t = {k: torch.from_numpy(np.ascontiguousarray(sd[k], dtype=np.float32)) for k in ("embeddingHead.weight", "embeddingHead.bias", "norm.weight", "norm.bias")}
    e = F.linear(torch.from_numpy(np.ascontiguousarray(pooled, dtype=np.float32)), t["embeddingHead.weight"], t["embeddingHead.bias"])
    return F.layer_norm(e, (H,), t["norm.weight"], t["norm.bias"], 1e-5).numpy()


def rel_rows(out, ref):
    """Per row ||out - ref|| / ||ref||: the pool-stage figure (its maximum over the rows is what the bound is on)."""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    return np.linalg.norm(out - ref, axis=1) / np.linalg.norm(ref, axis=1)
