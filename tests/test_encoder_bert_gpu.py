"""BERT checkpoints on the GPU: hac_encoder_set_option(enc, "model", "bert") -- the reference's ``models.BERT``, load_model's
BERT_Query / BERT_Passage arm -- through the C ABI, BERTEncoder and load_model.

What is new is the embedding stage (position ids = t, eps from the config, ``bert.*`` names, L up to max_pos); the layer stack is
the kernel set ANCEEncoder runs.  So every bound here is one the project already holds: tests/parity.py's fixture-scaled rule
against the reference's own outputs (tests/golden/encoder_bert/*.npz), and the committed per-stage BOUNDS of
tests/test_encoder_layers_gpu.py for the teacher-forced stages.  The reference is oracle.ance_oracle under BERT's rule
(tests/bert_ref.py, pinned on the CPU by tests/test_encoder_bert.py).  Every figure is printed before it is asserted.
"""
import functools
import json
import os

import numpy as np
import pytest

from tests import bert_ref, parity
from tests.test_encoder_layers_gpu import BOUNDS, EDGE_LENS, SEPARATION, figures

pytestmark = pytest.mark.gpu

ROUTES = {"auto": {}, "classic": {"gemm": "classic"}, "8phase": {"gemm": "8phase"}, "split": {"precision": "split"}}
PLAN_GEMM = {"auto": "classic128", "classic": "classic128", "8phase": "gemm8", "split": "split128"}   # (the fixtures hold < 2 k rows: auto = classic128)
DEFAULTS = {"gemm": "auto", "precision": "bf16", "pooling": "first", "graph": "auto"}
FAMILY_GEMM = {"classic": "classic", "gemm8": "8phase"}
LAYER_STD = {"std002": 0.02, "std010": 0.10}       # the weight kinds of tests/test_encoder_layers_gpu.py's BOUNDS
POS = "roberta.embeddings.position_embeddings.weight"


@functools.lru_cache(maxsize=None)
def encoder(n_layers, mstd):
    from haconvdr_amd.encoder import BERTEncoder
    return BERTEncoder.from_state_dict(bert_ref.weights(n_layers, mstd))


@functools.lru_cache(maxsize=None)
def rule_encoder(n_layers, mstd):
    """The control: the same tensors behind an ANCEEncoder -- HF's RoBERTa position rule with pad 0, on a lengthened table."""
    from haconvdr_amd.encoder import ANCEEncoder
    rsd = bert_ref.with_long_positions(bert_ref.to_roberta_keys(bert_ref.weights(n_layers, mstd)))
    return ANCEEncoder.from_state_dict(rsd, pad_token_id=0, ln_eps=bert_ref.EPS)


def reset(enc):
    for k, v in DEFAULTS.items():
        enc.set_option(k, v)


def plan(enc):
    return dict(kv.split("=") for kv in enc.last_plan().split())


def forward(enc, ids, mask, pooling="first", **options):
    """One forward under the options (undone afterwards): (embeddings, plan dict)."""
    try:
        for k, v in dict(options, pooling=pooling).items():
            enc.set_option(k, v)
        return np.asarray(enc(np.asarray(ids, np.int32), np.asarray(mask, np.int32))), plan(enc)
    finally:
        reset(enc)


def brief(m):
    return {k: v for k, v in m.items() if k != "spread"}


# ---------------------------------------------------------------------------------------------------------------- 1. goldens
@pytest.mark.parametrize("pooling", ["first", "mean"])
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", bert_ref.CASES)
def test_golden_parity_with_the_reference_bert(name, route, pooling):
    g = bert_ref.golden(name)
    ref = g["ref_" + pooling]
    enc = encoder(g["n_layers"], g["mstd"])
    out, p = forward(enc, g["ids"], g["mask"], pooling, **ROUTES[route])
    print(name, route, pooling, brief(parity.measure(out, ref)), p)
    wrong, pw = forward(rule_encoder(g["n_layers"], g["mstd"]), g["ids"], g["mask"], pooling, **ROUTES[route])
    failing = bert_ref.rows_failing(wrong, ref)
    print(name, route, pooling, "the RoBERTa rule (pad 0) on the same tensors:", brief(parity.measure(wrong, ref)), "failing rows", failing, pw)
    assert p["gemm"] == PLAN_GEMM[route] and p.get("model") == "bert" and p.get("pool") == ("mean" if pooling == "mean" else None), p
    assert pw["gemm"] == PLAN_GEMM[route] and "model" not in pw, pw
    parity.assert_embeddings_match(out, ref, what=(name, route, pooling))
    parity.assert_negative_control(out, ref)
    assert not parity.embeddings_match(wrong, ref), "the RoBERTa position rule passes for BERT's"


# ---------------------------------------------------------------------------------------------------------------- 2. / 3. stages
@functools.lru_cache(maxsize=None)
def edge_batch():
    """Lengths at the kernels' block edges, [CLS] first, ids 0 and 1 inside, a token at t = 511."""
    ids, mask = bert_ref.bert_case_inputs(0xBE5EED, EDGE_LENS, 512)
    assert (ids[:, 0] == bert_ref.CLS).all() and mask[-1, 511] == 1 and ids[-1, 511] != 0
    return ids, mask


@functools.lru_cache(maxsize=None)
def kernel_states(kind, family):
    """({stage: layer_state} of the 3-layer BERT of that weight kind on the edge batch, plan), the family's default route."""
    enc = encoder(3, LAYER_STD[kind])
    ids, mask = edge_batch()
    try:
        enc.set_option("gemm", FAMILY_GEMM[family])
        states = {n: enc.layer_state(ids, mask, n, normalized=True) for n in (-1, 0, 1)}
        p = plan(enc)
    finally:
        reset(enc)
    return states, p


def beyond(fig, bounds):
    return max(fig["rel"] / bounds[0], fig["bias"] / bounds[1])


@pytest.mark.parametrize("family", list(FAMILY_GEMM))
def test_embedding_stage_position_rule_and_eps(family):
    """LN_eps=1e-12(word[id] + type[0] + pos[t]) against the fp64 reference inside the COMMITTED embedding bounds; the same
    reference under the RoBERTa rule (pad 0), and with eps 1e-5, lies >= SEPARATION x beyond them."""
    ids, mask = edge_batch()
    valid = mask.astype(bool)
    sd = bert_ref.weights(3, LAYER_STD["std002"])
    states, p = kernel_states("std002", family)
    got = states[-1]["norm"]
    bounds = BOUNDS[("std002", family, "embed")]
    fig = figures(got, bert_ref.bert_embed(sd, ids, mask, family)["norm"].numpy(), valid)
    controls = {"RoBERTa rule, pad 0": figures(got, bert_ref.bert_embed(sd, ids, mask, family, pad_id=0)["norm"].numpy(), valid),
                "eps 1e-5": figures(got, bert_ref.bert_embed(sd, ids, mask, family, eps=1e-5)["norm"].numpy(), valid)}
    print(family, "embedding stage", fig, "bounds", bounds, p)
    for k, f in controls.items():
        print(family, "control:", k, f, "= %.1f x the bounds" % beyond(f, bounds))
    assert (p["gemm"] == "gemm8" if family == "gemm8" else p["gemm"].startswith("classic")) and p.get("model") == "bert", p
    assert np.isfinite(got).all() and fig["rel"] <= bounds[0] and fig["bias"] <= bounds[1], (family, fig, bounds)
    for k, f in controls.items():
        assert beyond(f, bounds) >= SEPARATION, (family, k, f, bounds)


@pytest.mark.parametrize("family", list(FAMILY_GEMM))
@pytest.mark.parametrize("kind", list(LAYER_STD))
def test_layers_teacher_forced_inside_the_committed_bounds(kind, family):
    """Layers 0 and 1 from the kernels' own previous state (eps 1e-12 in their LayerNorms): the kernels are ANCE's, and so are
    the bounds."""
    ids, mask = edge_batch()
    valid = mask.astype(bool)
    sd = bert_ref.weights(3, LAYER_STD[kind])
    states, p = kernel_states(kind, family)
    figs = {n: figures(states[n]["norm"], bert_ref.bert_layer(sd, n, states[n - 1], mask, family)["norm"].numpy(), valid) for n in (0, 1)}
    bounds = BOUNDS[(kind, family, "layer")]
    print(kind, family, "layers", figs, "bounds", bounds, p)
    assert (p["gemm"] == "gemm8" if family == "gemm8" else p["gemm"].startswith("classic")) and p.get("model") == "bert", p
    for n, f in figs.items():
        assert np.isfinite(f["rel"]) and f["rel"] <= bounds[0] and f["bias"] <= bounds[1], (kind, family, "layer", n, f, bounds)


# ---------------------------------------------------------------------------------------------------------------- 4. same kernels
def test_bert_and_roberta_handles_give_the_same_bits_where_their_rules_agree():
    """An ANCEEncoder (pad 1) whose position table is two rows followed by the BERT table reads, on ids that contain no 1, the
    rows a BERTEncoder reads (t + 2 against t): the two handles must agree bit for bit in every family and pooling."""
    from haconvdr_amd import synth
    from haconvdr_amd.encoder import ANCEEncoder
    sd = bert_ref.weights(2, 0.08)
    rsd = bert_ref.to_roberta_keys(sd)
    rsd[POS] = np.concatenate([synth.normal_fast(0x2B17, (2, 768), 0.02), rsd[POS]])
    bert, ance = encoder(2, 0.08), ANCEEncoder.from_state_dict(rsd, pad_token_id=1, ln_eps=bert_ref.EPS)
    ids, mask = bert_ref.bert_case_inputs(0xB175, EDGE_LENS, 512, interior=False)
    ids[mask.sum(1) >= 5, 2] = 0                  # [PAD] inside a sequence: an ordinary token for both (RoBERTa's pad is 1 here)
    assert not (ids == 1).any() and (ids[:, 0] == bert_ref.CLS).all()
    for route in ("8phase", "classic", "split"):
        for pooling in ("first", "mean"):
            a, pa = forward(ance, ids, mask, pooling, **ROUTES[route])
            b, pb = forward(bert, ids, mask, pooling, **ROUTES[route])
            print(route, pooling, "max |ance - bert|", float(np.abs(a - b).max()), pb)
            assert pa["gemm"] == pb["gemm"] == PLAN_GEMM[route] and "model" not in pa and pb["model"] == "bert", (pa, pb)
            assert np.isfinite(b).all() and np.array_equal(a, b), (route, pooling)


# ---------------------------------------------------------------------------------------------------------------- 5. bounds, option
def test_length_bounds_of_the_two_models():
    import torch
    from haconvdr_amd._lib import HacError
    from haconvdr_amd.encoder import ANCEEncoder
    sd = bert_ref.weights(2, 0.08)
    bert = encoder(2, 0.08)
    ids, mask = bert_ref.bert_case_inputs(0xB0B, [512, 300, 7], 512)
    out = bert(ids, mask)
    assert np.isfinite(out).all() and plan(bert).get("model") == "bert"
    ids513, mask513 = np.pad(ids, ((0, 0), (0, 1))), np.pad(mask, ((0, 0), (0, 1)))
    calls = {"forward": lambda: bert(ids513, mask513), "layer_state": lambda: bert.layer_state(ids513, mask513, -1),
             "forward_device": lambda: bert(torch.from_numpy(ids513).cuda(), torch.from_numpy(mask513).cuda())}
    for what, call in calls.items():
        with pytest.raises(HacError) as e:
            call()
        print(what, "L = 513:", e.value)
        assert e.value.code == 1, (what, str(e.value))                 # HAC_ERR_INVALID
    assert "L must be in [1, min(512, max_pos)]" in str(e.value)
    # RoBERTa on a 512-row table: positions reach L + 1, so L = 510 is the last one -- today's bound, today's words
    ance = ANCEEncoder.from_state_dict(bert_ref.to_roberta_keys(sd))
    ids510, mask510 = bert_ref.bert_case_inputs(0xB0C, [510, 300, 7], 510)
    assert np.isfinite(ance(ids510, mask510)).all() and "model" not in plan(ance)
    with pytest.raises(HacError) as e:
        ance(ids[:, :511], mask[:, :511])
    print("roberta, max_pos 512, L = 511:", e.value)
    assert e.value.code == 1 and "forward: bad arguments (B=3, L=511; L must be in [1, min(512, max_pos-2)])" in str(e.value)
    with pytest.raises(HacError):
        ance.layer_state(ids[:, :511], mask[:, :511], -1)


def test_model_option_and_tensor_names():
    import ctypes
    from haconvdr_amd import _lib, synth
    from haconvdr_amd._lib import HacError
    from haconvdr_amd.encoder import ANCEEncoder, BERTEncoder
    small = dict(vocab=128, max_pos=8)
    h = BERTEncoder(n_layers=1, **small)
    h.set_option("model", "roberta")              # accepted until the first tensor arrives
    h.set_option("model", "bert")
    with pytest.raises(HacError) as e:
        h.set_option("model", "gpt2")
    assert e.value.code == 1 and "roberta | bert" in str(e.value)
    with pytest.raises(HacError) as e:            # a BERT handle fed a RoBERTa state dict: finalize names the first tensor it misses
        h.load_state_dict(synth.ance_state_dict(7, 1, **small))
    print("bert handle, roberta names:", e.value)
    assert e.value.code == 1 and "bert.embeddings.word_embeddings.weight" in str(e.value)
    for v in ("roberta", "bert"):
        with pytest.raises(HacError) as e:
            h.set_option("model", v)
        assert e.value.code == 1 and "before the first hac_encoder_set_weight" in str(e.value)
    a = ANCEEncoder(n_layers=1, **small)
    one = np.zeros(768, np.float32)
    _lib.check(_lib.lib().hac_encoder_set_weight(a._h, b"norm.bias", one.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), one.size))
    with pytest.raises(HacError) as e:
        a.set_option("model", "bert")
    assert e.value.code == 1
    with pytest.raises(HacError) as e:
        a.load_state_dict(synth.bert_state_dict(7, 1, **small))
    assert "roberta.embeddings.word_embeddings.weight" in str(e.value)
    # an 8-row position table serves L = 8 in bert mode (6 in roberta mode)
    bsd = synth.bert_state_dict(7, 1, layer_matrix_std=0.08, **small)
    b = BERTEncoder.from_state_dict(bsd)
    ids, mask = bert_ref.bert_case_inputs(0xB0D, [8, 5, 1], 8, vocab=128)
    out, ref = b(ids, mask), bert_ref.bert_forward(bsd, ids, mask)
    print("max_pos = 8, L = 8:", brief(parity.measure(out, ref)), b.last_plan())
    assert b.last_plan().endswith(" model=bert")
    parity.assert_embeddings_match(out, ref, what="max_pos 8")
    with pytest.raises(HacError):
        b(np.pad(ids, ((0, 0), (0, 1))), np.pad(mask, ((0, 0), (0, 1))))


# ---------------------------------------------------------------------------------------------------------------- 6. graph
@pytest.mark.parametrize("B,L", [(4, 512), (1, 256)])
def test_capture_and_replay_give_the_eager_bits_beside_an_ance_handle(B, L):
    bert, ance = encoder(2, 0.08), rule_encoder(2, 0.08)
    ids, mask = bert_ref.bert_case_inputs(0x6A0 + B, {4: [512, 130, 257, 31], 1: [200]}[B], L)
    want = {"bert": forward(bert, ids, mask, graph="off")[0], "ance": forward(ance, ids, mask, graph="off")[0]}
    assert not np.array_equal(want["bert"], want["ance"])
    for enc in (bert, ance):
        enc.set_option("attn_qs_pin", "0")      # (its default; setting it drops the captured graphs: every shape starts eager)
    seen = []
    for _ in range(3):
        for tag, enc in (("bert", bert), ("ance", ance)):
            out, p = forward(enc, ids, mask)
            seen.append((tag, p["graph"], p.get("model")))
            assert p.get("model") == ("bert" if tag == "bert" else None), seen
            assert np.array_equal(out, want[tag]), seen
    print(B, L, seen)
    for tag in ("bert", "ance"):
        assert [g for t, g, _ in seen if t == tag] == ["eager-first", "replay", "replay"], seen


# ---------------------------------------------------------------------------------------------------------------- 7. loader
LOADER_VOCAB = 2048


@functools.lru_cache(maxsize=None)
def loader_weights():
    from haconvdr_amd import synth
    return synth.bert_state_dict(bert_ref.SEED, 2, layer_matrix_std=0.08, vocab=LOADER_VOCAB)


def checkpoint_dir(path, sd, drop=(), **cfg_over):
    """A HF-style BERT checkpoint directory: pytorch_model.bin with what BertForSequenceClassification adds to the tensors the
    forward reads (pooler, classifier, position_ids), and config.json."""
    import torch
    os.makedirs(path, exist_ok=True)
    full = dict(sd)
    full["bert.pooler.dense.weight"] = np.zeros((768, 768), np.float32)
    full["bert.pooler.dense.bias"] = np.zeros(768, np.float32)
    full["classifier.weight"] = np.zeros((2, 768), np.float32)
    full["classifier.bias"] = np.zeros(2, np.float32)
    full["bert.embeddings.position_ids"] = np.arange(512, dtype=np.int64)[None]
    torch.save({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in full.items()}, os.path.join(path, "pytorch_model.bin"))
    cfg = {"architectures": ["BertForSequenceClassification"], "model_type": "bert", "num_hidden_layers": 2, "hidden_size": 768,
           "num_attention_heads": 12, "intermediate_size": 3072, "vocab_size": LOADER_VOCAB, "max_position_embeddings": 512, "type_vocab_size": 2,
           "layer_norm_eps": 1e-12, "pad_token_id": 0, "hidden_act": "gelu", "position_embedding_type": "absolute"}
    cfg.update(cfg_over)
    for k in drop:
        cfg.pop(k)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(cfg, f)
    return path


def test_load_model_reads_a_bert_checkpoint_directory(tmp_path):
    from haconvdr_amd.encoder import BERTEncoder
    from haconvdr_amd.passages import load_model
    sd = loader_weights()
    ids, mask = bert_ref.bert_case_inputs(0x10AD, [64, 5, 33, 1, 48], 64, vocab=LOADER_VOCAB)
    tok, enc = load_model("BERT_Query", checkpoint_dir(str(tmp_path / "bert"), sd))
    assert tok is None and isinstance(enc, BERTEncoder)
    out, ref = enc(ids, mask), bert_ref.bert_forward(sd, ids, mask)
    print("loaded checkpoint", brief(parity.measure(out, ref)), enc.last_plan())
    assert enc.last_plan().endswith(" model=bert")
    parity.assert_embeddings_match(out, ref, what="load_model")
    parity.assert_negative_control(out, ref)
    # layer_norm_eps comes from the file
    _, enc2 = load_model("BERT_Passage", checkpoint_dir(str(tmp_path / "eps"), sd, layer_norm_eps=1e-2))
    out2 = enc2(ids, mask)
    cos = parity.one_minus_cos(out2, bert_ref.bert_forward(sd, ids, mask, eps=1e-2))
    print("layer_norm_eps 1e-2 from config.json: 1-cos", cos, "max |out2 - out|", float(np.abs(out2 - out).max()))
    assert np.all(cos < 1e-4) and np.abs(out2 - out).max() > 1e-3
    # refused, never mis-encoded
    refused = {
        "model_type roberta": lambda: load_model("BERT_Query", checkpoint_dir(str(tmp_path / "r1"), sd, model_type="roberta")),
        "a RoBERTa directory": lambda: load_model("BERT_Query", checkpoint_dir(str(tmp_path / "r2"), bert_ref.to_roberta_keys(sd), model_type="roberta", type_vocab_size=1)),
        "roberta.* tensors, no model_type": lambda: load_model("BERT_Query", checkpoint_dir(str(tmp_path / "r3"), bert_ref.to_roberta_keys(sd), drop=("model_type",))),
        "vocab_size": lambda: load_model("BERT_Query", checkpoint_dir(str(tmp_path / "r4"), sd, vocab_size=30522)),
        "a BERT directory as ANCE": lambda: load_model("ANCE_Query", str(tmp_path / "bert")),
        "unknown type": lambda: load_model("DPR_Query", str(tmp_path / "bert")),
    }
    for what, call in refused.items():
        with pytest.raises(ValueError):
            call()
        print("refused:", what)


def test_generate_new_ann_with_model_type_bert(tmp_path):
    """generate_new_ann(args) with model_type = "BERT" (gen_doc_embeddings.py:190-212 through load_model's second arm) on a
    23-record collection: the block it writes holds what the loaded encoder returns for the same batches."""
    import torch
    from types import SimpleNamespace
    from haconvdr_amd.passages import generate_new_ann, load_model, read_embedding_block, write_tokenized_passages
    sd = loader_weights()
    ckpt = checkpoint_dir(str(tmp_path / "bert"), sd)
    lens = [(11 * i) % 62 + 3 for i in range(23)]
    lens[5], lens[17] = 64, 1
    ids, mask = bert_ref.bert_case_inputs(0x23, lens, 64, vocab=LOADER_VOCAB)
    os.makedirs(tmp_path / "tokenized")
    write_tokenized_passages(str(tmp_path / "tokenized" / "passages"), ids.astype(np.int32), lens)
    args = SimpleNamespace(model_type="BERT", pretrained_passage_encoder=ckpt, max_seq_length=64, per_gpu_eval_batch_size=4, local_rank=-1, n_gpu=1,
                           tokenized_passage_collection_dir_path=str(tmp_path / "tokenized"), data_output_path=str(tmp_path / "embeds"))
    assert generate_new_ann(args) == 23
    e, i = read_embedding_block(args.data_output_path, 0)
    np.testing.assert_array_equal(i, np.arange(23))
    _, enc = load_model("BERT_Passage", ckpt)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()      # noqa: E731  (encode_passages' call shape)
    direct = np.concatenate([enc(dev(ids[s:s + 4]), dev(mask[s:s + 4])).cpu().numpy() for s in range(0, 23, 4)])
    ref = bert_ref.bert_forward(sd, ids, mask)
    print("generate_new_ann BERT: max |block - direct|", float(np.abs(e - direct).max()), brief(parity.measure(e, ref)), enc.last_plan())
    assert e.dtype == np.float32 and e.shape == (23, 768)
    np.testing.assert_array_equal(e, direct)
    parity.assert_embeddings_match(e, ref, what="generate_new_ann")
    parity.assert_negative_control(e, ref)
