"""BERT checkpoints (load_model's BERT_Query / BERT_Passage, the reference's ``models.BERT``), host side: the synthetic
weights carry the names and shapes of the reference model's state dict, tests/bert_ref.py's restatement reproduces the
reference's own outputs (tests/golden/encoder_bert/*.npz), and each fixture can tell BERT's position rule from RoBERTa's.
No GPU needed.
"""
import functools

import numpy as np
import pytest

from tests import bert_ref, parity

UNUSED = ("bert.pooler.", "classifier.")      # in a checkpoint, unused by models.BERT.forward


@functools.lru_cache(maxsize=None)
def helper(name, mean):
    g = bert_ref.golden(name)
    sd = bert_ref.weights(g["n_layers"], g["mstd"])
    return (bert_ref.bert_forward_mean if mean else bert_ref.bert_forward)(sd, g["ids"].astype(np.int64), g["mask"].astype(np.int64))


@functools.lru_cache(maxsize=None)
def roberta_rule(name, pad):
    g = bert_ref.golden(name)
    sd = bert_ref.weights(g["n_layers"], g["mstd"])
    return dict(zip(("first", "mean"), bert_ref.roberta_rule_forward(sd, g["ids"].astype(np.int64), g["mask"].astype(np.int64), pad)))


@pytest.mark.parametrize("name", bert_ref.CASES)
def test_synth_weights_carry_the_reference_state_dict_names_and_shapes(name):
    g = bert_ref.golden(name)
    want = {k: s for k, s in zip(g["sd_names"], g["sd_shapes"]) if not k.startswith(UNUSED) and not k.endswith("position_ids")}
    have = {k: tuple(v.shape) for k, v in bert_ref.weights(g["n_layers"], g["mstd"]).items()}
    assert have == want, (sorted(set(have) ^ set(want)), [k for k in have if k in want and have[k] != want[k]])
    dropped = [k for k in g["sd_names"] if k not in want]
    assert any(k.startswith("bert.pooler.") for k in dropped) and any(k.startswith("classifier.") for k in dropped), dropped
    assert have["bert.embeddings.token_type_embeddings.weight"] == (2, 768) and have["bert.embeddings.position_embeddings.weight"] == (512, 768)
    assert all(v.dtype == np.float32 for v in bert_ref.weights(g["n_layers"], g["mstd"]).values())


def test_bert_and_ance_synth_weights_share_no_tensor():
    """bert_state_dict draws every tensor under its own name; ance_state_dict of the same seed keeps its bits (one tensor pinned
    by value: the refactoring behind bert_state_dict must not move the streams)."""
    from haconvdr_amd import synth
    small = dict(vocab=64, max_pos=8)          # (the tables are most of a state dict's generation time)
    b, a = synth.bert_state_dict(0xA11CE, 1, **small), synth.ance_state_dict(0xA11CE, 1, **small)
    assert not np.array_equal(b["bert.encoder.layer.0.output.dense.bias"], a["roberta.encoder.layer.0.output.dense.bias"])
    assert not np.array_equal(b["embeddingHead.weight"], synth.bert_state_dict(0xA11CF, 1, **small)["embeddingHead.weight"])
    assert a["roberta.embeddings.token_type_embeddings.weight"].shape == (1, 768) and b["bert.embeddings.token_type_embeddings.weight"].shape == (2, 768)
    assert a["norm.bias"][:3].tolist() == synth.normal_fast(synth._name_seed(0xA11CE, "norm.bias"), (768,), 0.05)[:3].tolist()


@pytest.mark.parametrize("pooling", ["first", "mean"])
@pytest.mark.parametrize("name", bert_ref.CASES)
def test_helper_reproduces_the_reference_bert(name, pooling):
    """tests/test_encoder_oracle.py's tolerances of ance_forward against the ANCE goldens, applied to the BERT restatement."""
    g = bert_ref.golden(name)
    ref, out = g["ref_" + pooling], np.asarray(helper(name, pooling == "mean"))
    assert out.shape == ref.shape == (len(g["ids"]), 768)
    print(name, pooling, "max abs", float(np.abs(out - ref).max()), "1-cos max", float(parity.one_minus_cos(out, ref).max()))
    np.testing.assert_allclose(out, ref, atol=2e-4 if g["mstd"] == 0.02 else 1e-3, rtol=0)
    assert np.all(parity.one_minus_cos(out, ref) < 1e-6)
    m = parity.assert_embeddings_match(out, ref, what=(name, pooling))
    parity.assert_negative_control(out, ref)
    assert m["raw"] < 0.01 * m["spread"]["raw_min"]


@pytest.mark.parametrize("name", bert_ref.CASES)
def test_fixture_inputs(name):
    g = bert_ref.golden(name)
    ids, mask = g["ids"], g["mask"]
    lens = mask.sum(1)
    assert (ids[:, 0] == bert_ref.CLS).all() and ids.min() >= 0 and ids.max() < bert_ref.VOCAB
    inside = [(set(row[1:n].tolist()) >= {0, 1}) for row, n in zip(ids, lens)]
    assert sum(inside) >= 2, inside
    b = int(np.argmax(lens))
    assert lens[b] == 512 and ids[b, 511] != 0
    regenerated, _ = bert_ref.bert_case_inputs(g["seed"], [int(n) for n in lens], ids.shape[1])
    np.testing.assert_array_equal(regenerated, ids)


@pytest.mark.parametrize("name", bert_ref.CASES)
def test_fixture_tells_sequences_poolings_and_position_rules_apart(name):
    """What make_golden_encoder_bert.py checked while generating, from the stored arrays: rotated rows fail, the [CLS]-pooled
    output fails as the mean-pooled one, and the RoBERTa position rule (pad 0 and pad 1) fails on EVERY sequence."""
    g = bert_ref.golden(name)
    for pooling in ("first", "mean"):
        parity.assert_negative_control(g["ref_" + pooling], g["ref_" + pooling])
    assert not parity.embeddings_match(g["ref_first"], g["ref_mean"])
    for pad in (0, 1):
        for pooling in ("first", "mean"):
            wrong, ref = roberta_rule(name, pad)[pooling], g["ref_" + pooling]
            failing = bert_ref.rows_failing(wrong, ref)
            print(name, "RoBERTa rule pad", pad, pooling, "min per-sequence 1-cos", float(parity.one_minus_cos(wrong, ref).min()), failing)
            assert failing.all(), (name, pad, pooling, failing)
    assert not bert_ref.rows_failing(helper(name, False), g["ref_first"]).any()
