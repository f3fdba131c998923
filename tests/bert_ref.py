"""Host reference of the BERT encoder tests (test infrastructure): the reference's ``BERT`` class (src/models.py:66-110) restated
through the ANCE oracle.

``BertModel`` and ``RobertaModel`` run the same post-LN block; what differs is the embedding stage: BERT's position ids are
``arange(L)`` whatever the token ids, its LayerNorm eps is 1e-12, and its tensors are named ``bert.*``.  HF's RoBERTa rule
``cumsum(id != pad) * (id != pad) + pad`` with pad = -1 (an id no token has) IS ``arange(L)``, so oracle.ance_oracle serves
unchanged: a key rename plus ``pad_id=-1, eps=1e-12``.  tests/test_encoder_bert.py pins that against outputs of the
reference's own class (tests/golden/encoder_bert/*.npz, written by tests/golden/make_golden_encoder_bert.py).
"""
import functools
import os

import numpy as np

from tests import mean_pool, parity

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_bert")
CASES = ("l2_edges", "l12_mixed")
SEED = 0xBE27            # synth.bert_state_dict's seed in every BERT test and fixture
EPS = 1e-12              # BertConfig.layer_norm_eps
VOCAB, MAX_POS = 30522, 512
CLS, SEP = 101, 102      # bert-base-uncased's [CLS] / [SEP]; [PAD] = 0


def to_roberta_keys(sd):
    """The same tensors under the names oracle.ance_oracle reads (``bert.`` -> ``roberta.``; head names are shared)."""
    return {("roberta." + k[5:] if k.startswith("bert.") else k): v for k, v in sd.items()}


def with_long_positions(rsd, extra=2):
    """rsd with ``extra`` more rows behind its position table: the RoBERTa position rule reaches rows L and L + 1 (pad 0 / 1),
    which a 512-row BERT table does not have.  Only the controls that run that rule on purpose read them."""
    from haconvdr_amd import synth
    k = "roberta.embeddings.position_embeddings.weight"
    out = dict(rsd)
    out[k] = np.concatenate([np.asarray(rsd[k], np.float32), synth.normal_fast(0x10E6, (extra, 768), 0.02)])
    return out


def bert_forward(sd, ids, mask, hidden=False, eps=EPS):
    """models.BERT.forward with use_mean = False on ``bert.*`` weights: float32 [B, 768] (hidden=True: ance_forward's list)."""
    from oracle import ance_oracle
    return ance_oracle.ance_forward(to_roberta_keys(sd), ids, mask, eps=eps, pad_id=-1, hidden=hidden)


def bert_forward_mean(sd, ids, mask):
    """use_mean = True: the masked mean of the last hidden state and the head in fp64 (tests/mean_pool.py)."""
    return mean_pool.pool_and_head(sd, bert_forward(sd, ids, mask, hidden=True)[-1], mask)


def roberta_rule_forward(sd, ids, mask, pad_id):
    """The control: the same weights under HF's RoBERTa position rule with ``pad_id`` (0 or 1), on a lengthened table.
    Returns the pair ([CLS]-pooled, mean-pooled) embeddings of one forward (head in fp64, tests/mean_pool.py)."""
    from oracle import ance_oracle
    hs = ance_oracle.ance_forward(with_long_positions(to_roberta_keys(sd)), ids, mask, eps=EPS, pad_id=pad_id, hidden=True)[-1]
    return mean_pool.head(sd, hs[:, 0]), mean_pool.pool_and_head(sd, hs, mask)


def bert_embed(sd, ids, mask, family=None, eps=EPS, pad_id=-1):
    """ance_embed under BERT's rule; ``eps`` / ``pad_id`` other than the defaults are the GPU tests' controls (the RoBERTa
    rule runs on a lengthened position table)."""
    from oracle import ance_oracle
    rsd = to_roberta_keys(sd)
    return ance_oracle.ance_embed(rsd if pad_id < 0 else with_long_positions(rsd), ids, mask, family, eps=eps, pad_id=pad_id)


def bert_layer(sd, i, x_in, mask, family=None, attn="stream"):
    from oracle import ance_oracle
    return ance_oracle.ance_layer(to_roberta_keys(sd), i, x_in, mask, family, eps=EPS, attn=attn)


def bert_case_inputs(seed, lens, L, interior=True, vocab=VOCAB):
    """ids int64 [B, L], mask: every sequence is [CLS] body [SEP] padded with [PAD] = 0, body ids in [3, vocab).  interior:
    id 1 at t = 2 and id 0 at t = len - 2 of every sequence of 5+ tokens -- under BERT's rule they are ordinary tokens; the
    RoBERTa rule skips its pad id in the count, so with pad 0 an id 0 EARLY in a sequence would put every later token back on
    BERT's position (t + 1 - 1): the 0 sits at the end, and all tokens in front of it are one position off (two, with pad 1,
    in front of the id 1).  A sequence of L tokens has its [SEP] at t = L - 1: the last row of a 512-row position table is
    read."""
    from haconvdr_amd import synth
    B = len(lens)
    ids, _ = synth.token_batch(seed, B, L, fixed_len=L, vocab=vocab)
    ids = ids.astype(np.int64)
    mask = np.zeros((B, L), np.int64)
    for b, n in enumerate(lens):
        ids[b, n - 1] = SEP
        ids[b, 0] = CLS
        ids[b, n:] = 0
        mask[b, :n] = 1
        if interior and n >= 5:
            ids[b, 2], ids[b, n - 2] = 1, 0
    return ids, mask


def rows_failing(out, ref):
    """Per row: does ``out[i]`` fail tests/parity.py's bounds of the fixture ``ref`` (any of its three figures)?"""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    m = parity.measure(ref, ref)
    mu = ref.mean(0, keepdims=True)
    raw = parity.one_minus_cos(out, ref)
    cen = parity.one_minus_cos(out - mu, ref - mu)
    rel = np.linalg.norm(out - ref, axis=1) / np.linalg.norm(ref - mu, axis=1)
    return (raw > m["raw_bound"]) | (cen > m["centred_bound"]) | (rel > m["rel_l2_bound"]) | ~np.isfinite(out).all(1)


@functools.lru_cache(maxsize=None)
def weights(n_layers, mstd):
    from haconvdr_amd import synth
    return synth.bert_state_dict(SEED, n_layers, layer_matrix_std=mstd)


@functools.lru_cache(maxsize=None)
def golden(name):
    """dict of a fixture: ids, mask (int32), ref_first, ref_mean, n_layers, mstd, sd_names, sd_shapes."""
    g = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    return {"ids": g["ids"].astype(np.int32), "mask": g["mask"].astype(np.int32), "ref_first": g["ref_first"], "ref_mean": g["ref_mean"],
            "n_layers": int(g["n_layers"]), "mstd": float(g["layer_matrix_std"]), "seed": int(g["seed"]),
            "sd_names": [str(s) for s in g["sd_names"]], "sd_shapes": [tuple(int(v) for v in str(s).split(",") if v) for s in g["sd_shapes"]]}
