"""The encoder oracle (fp32 torch restatement) against goldens produced by the REFERENCE's own
models.ANCE (tests/golden/make_golden_encoder.py).  CPU only; the 12-layer cases take ~20 s."""
import glob
import os

import numpy as np
import pytest

GOLD = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "encoder_*.npz")))
_SD = {}


def state_dict(n_layers, layer_matrix_std=0.02):
    from haconvdr_amd import synth
    key = (n_layers, layer_matrix_std)
    if key not in _SD:
        _SD[key] = synth.ance_state_dict(0xA11CE, n_layers, layer_matrix_std=layer_matrix_std)
    return _SD[key]


def cosine(a, b):
    return (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


def test_encoder_goldens_present():
    assert len(GOLD) >= 7


@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p)[8:-4] for p in GOLD])
def test_oracle_matches_reference_ance(path):
    from oracle import ance_oracle
    from tests import parity
    from tests.golden.make_golden_encoder import load_case
    ids, mask, ref, n_layers, mstd = load_case(path)
    assert ref.shape == (len(ids), 768)
    if len(ids) > 32:      # the 320-sequence fixture: twelve rows spread over it (the whole batch is minutes of CPU)
        pick = np.r_[0:len(ids):29][:12]
        ids, mask, ref = ids[pick], mask[pick], ref[pick]
    out = ance_oracle.ance_forward(state_dict(n_layers, mstd), ids.astype(np.int64), mask.astype(np.int64))
    assert out.shape == ref.shape and out.dtype == np.float32
    # fp32 vs fp32 (sdpa vs explicit softmax): 2e-4 absolute on outputs of norm ~27.7 with the reference's init; the
    # content-sensitive weights (layer matrices x 4) amplify reassociation noise by about as much
    np.testing.assert_allclose(out, ref, atol=2e-4 if mstd == 0.02 else 1e-3, rtol=0)
    assert np.all(1.0 - cosine(out, ref) < 1e-6)
    m = parity.assert_embeddings_match(out, ref, what=os.path.basename(path))
    parity.assert_negative_control(out, ref)
    assert m["raw"] < 0.01 * m["spread"]["raw_min"]          # the oracle is a hundred times closer to the reference than two of its rows are
    g = np.load(path)
    if "pad_invariance_maxdiff" in g.files:
        assert float(g["pad_invariance_maxdiff"]) == 0.0


def test_oracle_varlen_equals_padded():
    """Dropping the padded tail entirely (what the HIP varlen path does) changes nothing beyond fp32
    reassociation noise."""
    from oracle import ance_oracle
    g = np.load([p for p in GOLD if "l2_mixed" in p][0])
    sd = state_dict(2)
    ids, mask, lens = g["ids"].astype(np.int64), g["mask"].astype(np.int64), g["lens"]
    full = ance_oracle.ance_forward(sd, ids, mask)
    for b in (0, 3, 5):
        n = int(lens[b])
        cut = ance_oracle.ance_forward(sd, ids[b:b + 1, :n], mask[b:b + 1, :n])
        np.testing.assert_allclose(cut[0], full[b], atol=1e-4, rtol=0)


def test_layer_reference_without_rounding_equals_ance_forward():
    """oracle.ance_embed / ance_layer (family None: fp64, no rounding), chained stage by stage, give ance_forward's hidden
    states on every valid row: the per-layer reference of tests/test_encoder_layers_gpu.py restates the same model."""
    from oracle import ance_oracle
    from tests.golden.make_golden_encoder import encoder_case_inputs
    sd = state_dict(3, 0.08)
    ids, mask = encoder_case_inputs(0x1A7, [1, 7, 32, 33, 64], 64)
    hs = ance_oracle.ance_forward(sd, ids, mask, hidden=True)
    valid = mask.astype(bool)
    st = ance_oracle.ance_embed(sd, ids, mask)
    np.testing.assert_allclose(st["norm"].numpy()[valid], hs[0][valid], atol=2e-6, rtol=0)
    for i in range(3):
        st = ance_oracle.ance_layer(sd, i, st, mask)
        np.testing.assert_allclose(st["norm"].numpy()[valid], hs[i + 1][valid], atol=1e-4, rtol=0)   # fp32 vs fp64, values up to ~5


@pytest.mark.parametrize("family", ["classic", "gemm8"])
def test_layer_reference_rounding_and_mutations_change_the_output(family):
    """The bf16-faithful reference differs from the exact one by the bf16 path's noise (~1e-2 relative per layer); each
    mutation of the self-checks changes the output (the GPU tests require them to clear the bounds by 3x)."""
    from oracle import ance_oracle
    from tests.golden.make_golden_encoder import encoder_case_inputs
    sd = state_dict(2, 0.08)
    ids, mask = encoder_case_inputs(0x1A8, [1, 33, 64], 64)
    valid = mask.astype(bool)

    def rel(a, b):
        a, b = a["norm"].numpy()[valid], b["norm"].numpy()[valid]
        return np.sqrt(((a - b) ** 2).mean() / (b ** 2).mean())
    emb = ance_oracle.ance_embed(sd, ids, mask, family)
    assert (rel(emb, ance_oracle.ance_embed(sd, ids, mask)) > 1e-4) == (family == "gemm8")   # classic keeps the fp32 rows
    for m in ance_oracle.EMBED_MUTATIONS:
        assert rel(ance_oracle.ance_embed(sd, ids, mask, family, mutate=m), emb) > 1e-3, m
    base = ance_oracle.ance_layer(sd, 0, emb, mask, family)
    assert 1e-3 < rel(base, ance_oracle.ance_layer(sd, 0, emb, mask)) < 5e-2
    assert 0 < rel(base, ance_oracle.ance_layer(sd, 0, emb, mask, family, attn="twopass")) < 1e-2
    for m in ance_oracle.LAYER_MUTATIONS:
        assert rel(ance_oracle.ance_layer(sd, 0, emb, mask, family, mutate=m), base) > 1e-5, m
