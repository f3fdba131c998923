"""precision = split on the GPU, through ANCEEncoder / the C ABI: the contract where the bf16 path fails it, how much closer
the mode gets, teacher-forced parity per layer against the unrounded fp64 chain, and the mechanics (graph, sub-batches,
batch invariance, bad rows, switching back).  Every test here fails on a library without the option ("precision" is
HAC_ERR_INVALID there).

Reference side alone (CPU): max 1-cos between oracle.ance_forward (fp32 torch) and the fp64 chain (ance_embed / ance_layer /
ance_tail, family=None) on the sweep batch's twelve picked rows -- the fp32 floor of the comparison -- see FP32_FLOOR.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import parity, split_parity  # noqa: E402
from tests.parity import one_minus_cos  # noqa: E402
from tests.split_parity import EDGE_LENS  # noqa: E402,F401

pytestmark = pytest.mark.gpu

PICK = [0, 1, 2, 5, 9, 17, 30, 31, 32, 45, 62, 63]
# layer-matrix std: (fp32 floor measured on the CPU, reference side alone; GPU figures of this file's first run: bf16, split)
FP32_FLOOR = {0.02: 2.8e-13, 0.08: 1.8e-12, 0.12: 1.2e-10, 0.16: 1.4e-8}
# std 0.08 with outlier channels (tools/parity_survey.py sweep's recipe, first three layers), x scale: emulation on THIS batch,
# run once on the CPU (tests/bf16_attribution.py's forward): (shipped rounding, hi + lo everywhere)
OUTLIER_EMULATION = {60.0: (8.5e-2, 5.4e-6), 200.0: (4.3e-2, 3.3e-6), 600.0: (1.5e-2, 1.9e-5)}
_CACHE = {}


def sweep_batch():
    from tests.golden.make_golden_encoder import encoder_case_inputs
    lens = [512 if i % 3 == 0 else 64 + (i * 37) % 449 for i in range(64)]
    ids, mask = encoder_case_inputs(0x5EED, lens, 512)
    return ids.astype(np.int32), mask.astype(np.int32)


def sens_weights(std, outlier=1.0):
    from haconvdr_amd import synth
    key = ("sd", std, outlier)
    if key not in _CACHE:
        sd = dict(synth.ance_state_dict(0x0D17, 12, layer_matrix_std=std))
        if outlier != 1.0:
            sd = split_parity.add_outlier_channels(sd, outlier)
        _CACHE[key] = sd
    return _CACHE[key]


def both_modes(std, outlier=1.0):
    """(bf16 embeddings, split embeddings, oracle) of the sweep batch's picked rows, one handle."""
    from haconvdr_amd.encoder import ANCEEncoder
    from oracle import ance_oracle
    key = ("out", std, outlier)
    if key not in _CACHE:
        sd = sens_weights(std, outlier)
        ids, mask = sweep_batch()
        enc = ANCEEncoder.from_state_dict(sd)
        o_bf = enc(ids, mask)[PICK]
        assert "precision" not in enc.last_plan()
        enc.set_option("precision", "split")
        o_sp = enc(ids, mask)[PICK]
        plan = enc.last_plan()
        assert "gemm=split128" in plan and "attn_form=split" in plan and plan.endswith(" precision=split"), plan
        assert enc.attention_redo() == 0
        ref = ance_oracle.ance_forward(sd, ids[PICK], mask[PICK])
        _CACHE[key] = (o_bf, o_sp, ref)
        del enc
    return _CACHE[key]


@pytest.mark.parametrize("std", [0.12, 0.16])
def test_split_keeps_the_contract_where_bf16_fails_it(std):
    o_bf, o_sp, ref = both_modes(std)
    print("std", std, "bf16", parity.measure(o_bf, ref), "split", parity.measure(o_sp, ref))
    parity.assert_embeddings_match(o_sp, ref, what=("split", std))
    parity.assert_negative_control(o_sp, ref)
    assert not parity.embeddings_match(o_bf, ref), "the bf16 path holds the contract on this recipe: the test no longer shows what the mode buys"


@pytest.mark.parametrize("std", [0.02, 0.08, 0.12, 0.16])
def test_split_is_100x_closer_than_bf16_or_at_the_fp32_floor(std):
    """max 1-cos(split, oracle) <= max(1/100 of max 1-cos(bf16, oracle), 4 x the oracle's own fp32 floor): the operand error
    shrinks 2^8-fold and 1-cos goes with its square; 100 leaves two orders for accumulation order and v_exp_f32.  The floor is
    FP32_FLOOR (ance_forward against the fp64 chain); 4 = the usual 2 x on a measured worst figure, twice, because two fp32
    evaluations with different summation orders are compared."""
    o_bf, o_sp, ref = both_modes(std)
    e_bf, e_sp = float(one_minus_cos(o_bf, ref).max()), float(one_minus_cos(o_sp, ref).max())
    print(f"std {std}: bf16 {e_bf:.3e} split {e_sp:.3e} floor {FP32_FLOOR[std]:.3e}")
    assert np.isfinite(o_sp).all()
    assert e_sp <= max(e_bf / 100.0, 4.0 * FP32_FLOOR[std]), (std, e_sp, e_bf, FP32_FLOOR[std])


@pytest.mark.parametrize("scale", [60.0, 200.0, 600.0])
def test_outlier_cells(scale):
    """std 0.08 with outlier channels x scale: the 1/100 relation in every cell, the 1e-3 contract for split where the
    emulation on this batch (OUTLIER_EMULATION) is below 2.5e-4."""
    o_bf, o_sp, ref = both_modes(0.08, scale)
    e_bf, e_sp = float(one_minus_cos(o_bf, ref).max()), float(one_minus_cos(o_sp, ref).max())
    print(f"outlier x{scale}: bf16 {e_bf:.3e} split {e_sp:.3e} emulation {OUTLIER_EMULATION[scale]}")
    assert np.isfinite(o_sp).all()
    assert e_sp <= max(e_bf / 100.0, 4.0 * FP32_FLOOR[0.08]), (scale, e_sp, e_bf)
    if OUTLIER_EMULATION[scale][1] < 2.5e-4:
        assert e_sp <= parity.CONTRACT, (scale, e_sp)


def test_small_batches_and_two_sub_batches_hold_the_contract():
    """4 x 512 and 1 x 256 (the graph route), and a batch that crosses a lowered max_tokens (two sub-batches), std 0.12."""
    from haconvdr_amd.encoder import ANCEEncoder
    from oracle import ance_oracle
    sd = sens_weights(0.12)
    ids, mask = sweep_batch()
    enc = ANCEEncoder.from_state_dict(sd, precision="split")
    for rows, L in (([0, 1, 2, 5], 512), ([17], 256)):
        i, m = np.ascontiguousarray(ids[rows, :L]), np.ascontiguousarray(mask[rows, :L])
        m[:, 0] = 1
        ref = ance_oracle.ance_forward(sd, i, m)
        for call in range(3):                      # eager-first, capture + replay, replay
            out = enc(i, m)
            assert float(one_minus_cos(out, ref).max()) <= parity.CONTRACT / 4, (rows, call, one_minus_cos(out, ref))
        assert "graph=replay" in enc.last_plan() and "precision=split" in enc.last_plan(), enc.last_plan()
    enc.set_option("max_tokens", "4096")
    sub = list(range(16))
    out = enc(ids[sub], mask[sub])
    plan = dict(kv.split("=") for kv in enc.last_plan().split())
    assert int(plan["sub_batches"]) >= 2 and plan["gemm"] == "split128", plan
    ref = ance_oracle.ance_forward(sd, ids[sub], mask[sub])
    parity.assert_embeddings_match(out, ref, what="two sub-batches")


@pytest.mark.parametrize("B,L", [(1, 64), (1, 512), (4, 64), (4, 512)])
def test_eager_capture_and_replay_are_bit_identical(B, L):
    from haconvdr_amd import synth
    from haconvdr_amd.encoder import ANCEEncoder
    sd = synth.ance_state_dict(0xA11CE, 2)
    ids, lens = synth.token_batch(21 + B + L, B, L, min_len=3)
    ids = ids.astype(np.int32)
    mask = (np.arange(L)[None, :] < lens[:, None]).astype(np.int32)
    enc = ANCEEncoder.from_state_dict(sd, precision="split")
    outs, plans = [], []
    for _ in range(3):
        outs.append(enc(ids, mask).copy())
        plans.append(enc.last_plan())
    assert "graph=eager-first" in plans[0] and "graph=replay" in plans[1] and "graph=replay" in plans[2], plans
    enc.set_option("graph", "off")
    outs.append(enc(ids, mask).copy())
    assert "graph=off" in enc.last_plan()
    assert np.isfinite(outs[0]).all()
    for o in outs[1:]:
        assert np.array_equal(outs[0], o)


def test_a_sequence_has_the_same_bits_alone_in_a_batch_and_in_a_second_sub_batch():
    from haconvdr_amd.encoder import ANCEEncoder
    sd = sens_weights(0.08)
    ids, mask = sweep_batch()
    enc = ANCEEncoder.from_state_dict(sd, precision="split")
    enc.set_option("ksplit", "off")                # one summation order for every batch size
    full = enc(ids, mask)
    for b in (1, 31, 63):
        alone = enc(ids[b:b + 1], mask[b:b + 1])
        assert np.array_equal(alone[0], full[b]), b
    enc.set_option("max_tokens", "8192")
    cut = enc(ids, mask)
    assert int(dict(kv.split("=") for kv in enc.last_plan().split())["sub_batches"]) >= 2
    assert np.array_equal(cut, full)


def test_lengths_at_the_block_edges_and_bad_rows():
    """Lengths 1, 31, 32, 33, 255, 256, 257, 512 against the oracle; a bad mask / token id gives NaN in that row only."""
    import torch
    from haconvdr_amd import synth
    from haconvdr_amd.encoder import ANCEEncoder
    from oracle import ance_oracle
    from tests.golden.make_golden_encoder import encoder_case_inputs
    sd = synth.ance_state_dict(0xA11CE, 3, layer_matrix_std=0.08)
    ids, mask = encoder_case_inputs(9, [1, 31, 32, 33, 255, 256, 257, 512], 512)
    enc = ANCEEncoder.from_state_dict(sd, precision="split")
    out = enc(ids.astype(np.int32), mask.astype(np.int32))
    ref = ance_oracle.ance_forward(sd, ids, mask)
    d = one_minus_cos(out, ref)
    print("edge lengths, max 1-cos", d.max())
    assert np.isfinite(out).all() and d.max() <= parity.CONTRACT / 100, d      # (the 1/100 relation applied to the contract itself)
    bad_ids, bad_mask = ids.copy(), mask.copy()
    bad_mask[2, 40] = 1                                        # not a prefix mask
    bad_ids[5, 3] = 10 ** 6                                    # token id outside the vocabulary
    o = enc(torch.from_numpy(bad_ids).cuda(), torch.from_numpy(bad_mask).cuda()).cpu().numpy()
    assert np.isnan(o[2]).all() and np.isnan(o[5]).all()
    good = [0, 1, 3, 4, 6, 7]
    assert np.array_equal(o[good], out[good])


def test_switching_back_to_bf16_gives_a_fresh_handles_bits():
    import torch
    from haconvdr_amd.encoder import ANCEEncoder
    sd = sens_weights(0.08)
    ids, mask = sweep_batch()
    fresh = ANCEEncoder.from_state_dict(sd)
    used = ANCEEncoder.from_state_dict(sd)
    used.set_option("precision", "split")
    for sel in (slice(0, 64), slice(0, 4)):
        split = used(ids[sel], mask[sel])
        assert "precision=split" in used.last_plan()
        used.set_option("precision", "bf16")
        a, b = used(ids[sel], mask[sel]), fresh(ids[sel], mask[sel])
        assert used.last_plan() == fresh.last_plan() and "precision" not in used.last_plan(), (used.last_plan(), fresh.last_plan())
        assert torch.equal(torch.from_numpy(a), torch.from_numpy(b))
        assert not np.array_equal(split, a)
        used.set_option("precision", "split")
    with pytest.raises(Exception):
        used.set_option("precision", "fp32")


@pytest.mark.parametrize("scale", [3.0, 4.0, 10.0, 20.0])
def test_peaked_attention_through_the_split_kernel(scale):
    """test_peaked_attention_both_kernels_vs_oracle's recipe (Q and K x scale: logits x 9 ... x 400, references that move)
    through attention_split_kernel, that test's bound."""
    from haconvdr_amd import synth
    from haconvdr_amd.encoder import ANCEEncoder
    from oracle import ance_oracle
    from tests.golden.make_golden_encoder import encoder_case_inputs
    sd = dict(synth.ance_state_dict(0xFACE, 2))
    for i in range(2):
        for nm in ("query", "key"):
            for part in ("weight", "bias"):
                key = f"roberta.encoder.layer.{i}.attention.self.{nm}.{part}"
                sd[key] = (sd[key] * scale).astype(np.float32)
    enc = ANCEEncoder.from_state_dict(sd, precision="split")
    ids, mask = encoder_case_inputs(7, [1, 5, 31, 32, 33, 64, 100, 129, 255, 256, 257, 290, 384, 400, 511, 512], 512)
    ref = ance_oracle.ance_forward(sd, ids, mask)
    out = enc(ids.astype(np.int32), mask.astype(np.int32))
    d = one_minus_cos(out, ref)
    print("peaked x", scale, "max 1-cos", d.max())
    assert np.isfinite(out).all() and np.all(d < 2e-4), d
    assert "attn_form=split" in enc.last_plan() and enc.attention_redo() == 0


# ---------------------------------------------------------------------------------------------------------------------------
# per layer, teacher-forced: layer_state in split mode against the UNROUNDED fp64 chain (family=None) on the kernels' own
# previous state.  Figure: rms(out - ref) / rms(ref) over the valid rows of the normalized state (the tail: of the embeddings).
# Bounds = 2 x the worst figure measured on MI355X against that exact chain (first run of this file):
# measured: embed 6.8e-8 (both); std 0.08: layers 1.42e-5 / 1.02e-5, tails 1.43e-5 (1 layer) / 9.4e-6 (3 layers); std 0.12: layers
# 2.20e-5 / 1.79e-5, tails 2.22e-5 / 1.37e-5.  (The bf16 files' bounds are rel 1e-4 ... 2.3e-3.)
LAYER_BOUNDS = {0.08: {"embed": 1.4e-7, "layer": 2.9e-5, "tail": 2.9e-5}, 0.12: {"embed": 1.4e-7, "layer": 4.4e-5, "tail": 4.5e-5}}
# mutations of the reference that do NOT lie 3 x beyond the bound, with the reason
# (measured separation / bound in brackets).  eps: the rows the LayerNorms see have a variance of ~1, which eps 1e-12 against 1e-5
# moves by 5e-6 of itself -- below any fp32 forward's own error; the bf16 files list it for the same reason (layers 0.000 .. 0.004,
# head 0.3 .. 0.6).  gelu_tanh at std 0.12: the tanh form lies 1.9 .. 2.0 x beyond the bound (4.3 .. 4.8 x at std 0.08, where it
# is asserted): a kernel with a tanh GELU would still miss the bound, with less than the 3 x margin; asserted to stay > 1.5.
NOT_SEPARABLE = {(std, nl, st, n, m) for std in (0.08, 0.12) for nl, stages in ((1, [("tail", 0)]), (3, [("layer", 0), ("layer", 1), ("tail", 2)]))
                 for st, n in stages for m in (("eps", "head_eps") if st == "tail" else ("eps",))}
NOT_SEPARABLE |= {(0.12, nl, st, n, "gelu_tanh") for nl, stages in ((1, [("tail", 0)]), (3, [("layer", 0), ("layer", 1), ("tail", 2)])) for st, n in stages}


def _teacher_forced(std, n_layers):
    """(figures, separations of every mutation) of the EDGE_LENS batch: the loop is tests/split_parity.teacher_forced."""
    from haconvdr_amd import synth
    from haconvdr_amd.encoder import ANCEEncoder
    from oracle import ance_oracle
    key = ("tf", std, n_layers)
    if key in _CACHE:
        return _CACHE[key]
    sd = synth.ance_state_dict(split_parity.SEED, n_layers, layer_matrix_std=std)
    ids, mask = split_parity.batch("edges")
    enc = ANCEEncoder.from_state_dict(sd, precision="split")
    figs, sep, _, _ = split_parity.teacher_forced(enc, sd, ids, mask, n_layers, ance_oracle.LAYER_MUTATIONS, ance_oracle.TAIL_MUTATIONS)
    _CACHE[key] = (figs, sep)
    return figs, sep


@pytest.mark.parametrize("n_layers", [1, 3])
@pytest.mark.parametrize("std", [0.08, 0.12])
def test_layers_and_tail_teacher_forced_vs_the_unrounded_chain(std, n_layers):
    figs, _ = _teacher_forced(std, n_layers)
    print("teacher-forced", std, n_layers, {k: f"{v:.3e}" for k, v in figs.items()})
    for (stage, n), f in figs.items():
        assert np.isfinite(f) and f <= LAYER_BOUNDS[std][stage], (std, n_layers, stage, n, f, LAYER_BOUNDS[std][stage])


@pytest.mark.parametrize("n_layers", [1, 3])
@pytest.mark.parametrize("std", [0.08, 0.12])
def test_teacher_forced_bounds_reject_every_mutation(std, n_layers):
    """Every mutation of the reference (a tanh GELU among them), on the kernels' own input, lies at least 3 x beyond the
    bound, or is listed in NOT_SEPARABLE with the reason."""
    _, sep = _teacher_forced(std, n_layers)
    print("separations", std, n_layers, {k: f"{v / LAYER_BOUNDS[std][k[0]]:.1f}" for k, v in sep.items()})
    weak = {k: v / LAYER_BOUNDS[std][k[0]] for k, v in sep.items() if v < 3.0 * LAYER_BOUNDS[std][k[0]] and (std, n_layers) + k not in NOT_SEPARABLE}
    assert not weak, (std, n_layers, weak)
    for k, v in sep.items():
        if k[2] == "gelu_tanh":
            assert v > 1.5 * LAYER_BOUNDS[std][k[0]], (std, n_layers, k, v)
