#!/usr/bin/env python3
"""Generate tests/golden/encoder_bert/*.npz by RUNNING THE REFERENCE's own ``models.BERT`` (src/models.py:66-110, what
load_model's BERT_Query / BERT_Passage arm builds) on haconvdr_amd.synth.bert_state_dict weights, with ``use_mean`` False and
True.  Fixtures are data only: the seed, token ids, masks, the reference's two outputs (``ref_first``, ``ref_mean``) and the
sorted names and shapes of the reference model's state dict (what a BERT checkpoint holds).  They live in a directory of their
own because tests/test_encoder_oracle.py and tests/test_encoder_gpu.py take every tests/golden/encoder_*.npz as an ANCE
fixture.

Inputs (tests/bert_ref.bert_case_inputs): every sequence starts with [CLS] = 101, never with id 0.  HF's RoBERTa position rule
with pad 0 coincides with BERT's ``arange(L)`` on a sequence whose only id-0 token is the first one, so batches in the style of
make_golden_encoder.encoder_case_inputs (every sequence starts with id 0) cannot tell the two rules apart.  Ids 0 and 1 sit
inside the sequences, and the 512-token sequence reads the last row of the 512-row position table.

While generating, on the CPU, each fixture must show under tests/parity.py (otherwise change its ids or lengths, never the
bounds) that
  * rows rotated by one fail;
  * the reference's use_mean = False output fails as its use_mean = True output;
  * the RoBERTa position rule, pad 0 and pad 1 (oracle.ance_oracle.ance_forward on a lengthened position table), fails on
    EVERY sequence, in both poolings;
and that tests/bert_ref.py's restatement (ance_forward with pad_id = -1, eps = 1e-12) reproduces the reference.

Run:  python tests/golden/make_golden_encoder_bert.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import bert_ref, parity  # noqa: E402
from tests.golden.make_golden_encoder import REF, SENS_STD  # noqa: E402

CASES = [
    # name, n_layers, L, lens, layer_matrix_std: every 32-row block edge, a one-token sequence, 511 and 512 tokens
    ("l2_edges", 2, 512, [1, 5, 31, 32, 33, 64, 257, 511, 512], SENS_STD),
    # the lengths and the std of encoder_mean/l12_mixed (make_golden_encoder_mean.py: why 0.03)
    ("l12_mixed", 12, 512, [8, 31, 64, 129, 256, 384, 512, 40, 500, 333], 0.03),
]


def main(only=None):
    sys.path[:0] = [REF, os.path.join(REF, "src")]
    import torch
    import models  # the reference's src/models.py
    from transformers import BertConfig
    for name, n_layers, L, lens, mstd in CASES:
        if only and name not in only:
            continue
        seed = int.from_bytes(("b" + name).encode()[:4], "little")
        cfg = BertConfig(vocab_size=bert_ref.VOCAB, hidden_size=768, num_hidden_layers=n_layers, num_attention_heads=12,
                         intermediate_size=3072, max_position_embeddings=bert_ref.MAX_POS, type_vocab_size=2, layer_norm_eps=bert_ref.EPS,
                         pad_token_id=0)
        model = models.BERT(cfg).eval()
        sd = bert_ref.weights(n_layers, mstd)
        missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        assert not unexpected and all(m.startswith(("classifier.", "bert.pooler.")) or "position_ids" in m for m in missing), (missing, unexpected)
        ref_sd = sorted((k, tuple(v.shape)) for k, v in model.state_dict().items())
        ids, mask = bert_ref.bert_case_inputs(seed, lens, L)
        assert (ids[:, 0] == bert_ref.CLS).all() and ids.max() < bert_ref.VOCAB and ids.min() >= 0
        assert sum(((row[1:n] == 0).any() and (row[1:n] == 1).any()) for row, n in zip(ids, lens)) >= 2
        assert mask[lens.index(512), 511] == 1 and ids[lens.index(512), 511] != 0
        outs = {}
        for use_mean in (False, True):
            model.use_mean = use_mean
            with torch.no_grad():
                outs[use_mean] = model(torch.from_numpy(ids), torch.from_numpy(mask)).numpy()
        ref_first, ref_mean = outs[False], outs[True]
        # the fixture's controls
        for what, ref in (("first", ref_first), ("mean", ref_mean)):
            assert not parity.embeddings_match(np.roll(ref, 1, axis=0), ref), f"{name}/{what}: rotated rows pass"
        assert not parity.embeddings_match(ref_first, ref_mean), f"{name}: [CLS] pooling passes for mean pooling"
        for pad in (0, 1):
            for mean, wrong, ref in zip((False, True), bert_ref.roberta_rule_forward(sd, ids, mask, pad), (ref_first, ref_mean)):
                failing = bert_ref.rows_failing(wrong, ref)
                print(name, f"RoBERTa rule pad {pad}, {'mean' if mean else 'first'}: min per-sequence 1-cos %.3e, every sequence fails: %s"
                      % (parity.one_minus_cos(wrong, ref).min(), bool(failing.all())))
                assert failing.all(), (name, pad, mean, failing)
        # the restatement the tests use
        for what, out, ref in (("first", bert_ref.bert_forward(sd, ids, mask), ref_first), ("mean", bert_ref.bert_forward_mean(sd, ids, mask), ref_mean)):
            print(name, what, "restatement vs reference: 1-cos max %.2e, max abs %.2e" % (parity.one_minus_cos(out, ref).max(), np.abs(out - ref).max()))
            parity.assert_embeddings_match(out, ref, what=(name, what))
        os.makedirs(bert_ref.GOLDEN, exist_ok=True)
        np.savez_compressed(os.path.join(bert_ref.GOLDEN, f"{name}.npz"), seed=seed, n_layers=n_layers, L=L, lens=np.array(lens),
                            ids=ids.astype(np.int32), mask=mask.astype(np.int8), ref_first=ref_first, ref_mean=ref_mean, layer_matrix_std=mstd,
                            sd_names=np.array([k for k, _ in ref_sd]), sd_shapes=np.array([",".join(str(v) for v in s) for _, s in ref_sd]))
        for what, ref in (("first", ref_first), ("mean", ref_mean)):
            sp = parity.spread(ref)
            print(name, what, ref.shape, "min pairwise 1-cos %.3e (centred %.3e)" % (sp["raw_min"], sp["centred_min"]))


if __name__ == "__main__":
    main(set(sys.argv[1:]))
