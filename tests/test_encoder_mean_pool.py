"""Mean pooling (pooling = "mean", the reference's use_mean = True), host side: the fp64 helper of tests/mean_pool.py pinned
against the reference's own mean-pooled outputs (tests/golden/encoder_mean/*.npz), and the derivation of the pool-stage bound
the GPU tests (tests/test_encoder_mean_pool_gpu.py) hold pool_mean_kernel to.  No GPU needed.
"""
import functools
import os

import numpy as np
import pytest

from tests import mean_pool, parity

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("l2_edges", "l12_mixed")

# The helper against the goldens: fp32 torch (this repository's restatement of the RoBERTa forward, then the pooling and head in
# fp64) against fp32 torch (the reference's model): max over rows of ||helper - golden|| / ||golden||.
#   measured: l2_edges 1.16e-6, l12_mixed 7.1e-7; the bound is twice the figure (BLAS summation orders differ between hosts).
HELPER_VS_GOLDEN = {"l2_edges": 2.4e-6, "l12_mixed": 1.5e-6}

# The pool-stage bound of the GPU tests: on (rows, statistics) taken from the kernels, the kernels' embeddings against the fp64
# helper's pooling of those very rows + head.  What separates the two is fp32 arithmetic only -- pool_mean_kernel's fmaf
# normalization, its fixed-order fp32 sums and division, and the fp32 head -- and emulate_pool_mean_kernel + head_fp32 restate
# exactly that.  Worst rel_rows figure of the restatement over every length 1 .. 512 of the longest sequence of l2_edges
# (layer-1 state of the bf16-faithful fp64 oracle; bf16 rows in 16 row groups, fp32 rows in 8):
#   measured: bf16 rows 3.95e-7 (at len 212), fp32 rows 4.00e-7 (at len 492)
# times 2.6, the margin the split-precision shape tests use over an emulation figure (tests/split_parity.py).
POOL_EMULATION_WORST = 4.0e-7
POOL_STAGE_MARGIN = 2.6
POOL_STAGE_BOUND = POOL_STAGE_MARGIN * POOL_EMULATION_WORST


@functools.lru_cache(maxsize=None)
def golden(name):
    from tests.golden.make_golden_encoder import load_case
    path = os.path.join(GOLDEN, "encoder_mean", f"{name}.npz")
    ids, mask, ref, n_layers, mstd = load_case(path)
    return ids, mask, ref, np.load(path)["ref_first"], n_layers, mstd


@functools.lru_cache(maxsize=None)
def weights(n_layers, mstd):
    from haconvdr_amd import synth
    return synth.ance_state_dict(0xA11CE, n_layers, layer_matrix_std=mstd)


@functools.lru_cache(maxsize=None)
def helper_embeddings(name):
    from oracle import ance_oracle
    ids, mask, _, _, n_layers, mstd = golden(name)
    sd = weights(n_layers, mstd)
    hs = ance_oracle.ance_forward(sd, ids, mask, hidden=True)[-1]
    return mean_pool.pool_and_head(sd, hs, mask)


@pytest.mark.parametrize("name", CASES)
def test_helper_reproduces_the_reference_mean_pooling(name):
    _, _, ref, _, _, _ = golden(name)
    fig = float(mean_pool.rel_rows(helper_embeddings(name), ref).max())
    print(name, "helper vs golden: rel", fig)
    assert fig <= HELPER_VS_GOLDEN[name], (name, fig)
    parity.assert_embeddings_match(helper_embeddings(name), ref, what=name)


@pytest.mark.parametrize("name", CASES)
def test_fixture_tells_the_poolings_and_the_sequences_apart(name):
    """What make_golden_encoder_mean.py checked while generating: <s> pooling fails against mean pooling, rows rotated by one
    fail, and a one-token sequence has the same embedding either way."""
    ids, mask, ref, ref_first, _, _ = golden(name)
    assert not parity.embeddings_match(ref_first, ref)
    parity.assert_negative_control(ref, ref)
    for b in np.flatnonzero(mean_pool.lens_of(mask) == 1):
        assert np.abs(ref[b] - ref_first[b]).max() <= 1e-6, b


@functools.lru_cache(maxsize=None)
def oracle_last_state(family):
    """The bf16-faithful fp64 oracle's state after the last layer of the 2-layer model, l2_edges' longest sequence (512 rows):
    rows as the family stores them (gemm8: bf16 values; classic: fp32), statistics in fp32 (the kernels' format)."""
    from oracle import ance_oracle
    ids, mask, _, _, n_layers, mstd = golden("l2_edges")
    sd = weights(n_layers, mstd)
    b = int(np.argmax(mean_pool.lens_of(mask)))
    ids, mask = ids[b:b + 1], mask[b:b + 1]
    st = ance_oracle.ance_embed(sd, ids, mask, family)
    for i in range(n_layers):
        st = ance_oracle.ance_layer(sd, i, st, mask, family)
    return tuple(np.asarray(st[k][0].numpy(), np.float32) for k in ("rows", "mean", "rstd"))


def prefix_embeddings(family, pad_to=1):
    """(fp32 restatement of the kernel, fp64 helper) embeddings [512, 768] of every prefix length 1 .. 512 of that sequence."""
    ids, mask, _, _, n_layers, mstd = golden("l2_edges")
    sd = weights(n_layers, mstd)
    rows, mean, rstd = oracle_last_state(family)
    g, b = mean_pool.last_ln(sd, n_layers)
    n = len(rows)
    lens = np.arange(1, n + 1)
    tile = lambda v: np.broadcast_to(v, (n,) + v.shape)      # noqa: E731  (every prefix reads the same rows)
    ref = mean_pool.head(sd, mean_pool.pool_rows(tile(rows), tile(mean), tile(rstd), g, b, lens, pad_to))
    emu = mean_pool.head_fp32(sd, mean_pool.emulate_pool_mean_kernel(rows, mean, rstd, g, b, 16 if family == "gemm8" else 8))
    return emu, ref


@functools.lru_cache(maxsize=None)
def emulation_figures(family):
    emu, ref = prefix_embeddings(family)
    return mean_pool.rel_rows(emu, ref)


@pytest.mark.parametrize("family", ["gemm8", "classic"])
def test_pool_stage_bound_covers_the_fp32_restatement(family):
    """The named constant covers the restatement run here: its worst figure is at most a quarter above the constant (its fp32
    head goes through the host's BLAS, whose summation order is not ours to fix, so the figure moves a little between hosts;
    a host that lands BELOW the recorded figure has nothing wrong with it, so only this side is asserted)."""
    worst = float(emulation_figures(family).max())
    print(family, "fp32 restatement vs fp64 helper: worst rel", worst, "at len", 1 + int(emulation_figures(family).argmax()))
    assert 0 < worst <= 1.25 * POOL_EMULATION_WORST, (family, worst)


@pytest.mark.parametrize("family", ["gemm8", "classic"])
def test_pool_stage_bound_rejects_a_mean_over_the_padded_rows(family):
    """A pooling that walks roundup(len, 32) rows (dead rows become beta, the divisor counts them) lies beyond the bound for
    every length that is no multiple of 32."""
    _, ref = prefix_embeddings(family)
    _, mut = prefix_embeddings(family, pad_to=32)
    d = mean_pool.rel_rows(mut, ref)
    lens = np.arange(1, len(d) + 1)
    off = lens % 32 != 0
    assert (d[off] > POOL_STAGE_BOUND).all(), (family, float(d[off].min()), int(lens[off][d[off].argmin()]))
    assert (d[~off] == 0).all()
    print(family, "padded-rows mutation: smallest rel", float(d[off].min()), "= %.0f x bound" % (d[off].min() / POOL_STAGE_BOUND))
