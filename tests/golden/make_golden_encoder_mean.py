#!/usr/bin/env python3
"""Generate tests/golden/encoder_mean/*.npz by RUNNING THE REFERENCE's own ``models.ANCE`` with ``model.use_mean = True``
(src/models.py:52-61: masked_mean_or_first -> masked_mean) on the seeded synthetic weights and token batches of
make_golden_encoder.py.  Fixtures are data only: seeds, token ids, masks, the reference's mean-pooled outputs (``ref_out``,
what make_golden_encoder.load_case returns) and, for the controls, its ``use_mean = False`` outputs of the same inputs
(``ref_first``).  They live in a directory of their own because tests/test_encoder_oracle.py and tests/test_encoder_gpu.py take every
tests/golden/encoder_*.npz as a fixture of the default, <s>-pooled forward.

Weights: with N(0, 0.02^2) layer matrices every sequence maps onto nearly one direction, and averaging a sequence's rows makes
that worse, so the 2-layer case uses the content-sensitive weights (layer_matrix_std = 0.08).  Twelve such layers do the
opposite damage: every row of a sequence ends as the same vector.  The reference's use_mean = False output against its
use_mean = True output on the 12-layer case's inputs, 1 - cos / rel L2 of tests/parity.py: 1.7e-13 / 0.0000 at 0.08, 2.0e-8 /
0.0012 at 0.05, 2.7e-5 / 0.058 at 0.04 -- each PASSES as the other pooling, so a 12-layer fixture with such weights could not
tell the poolings apart.  At 0.03 it is 7.9e-3 / 1.33 (fails, as it must): the rows of a sequence stay distinct, and different
sequences are still 2.2e-3 apart.

While generating, on the CPU, each fixture must show that it can tell the two poolings and the sequences apart under
tests/parity.py (otherwise change its lengths or weights, never the bounds):
  * the reference's own use_mean = False output FAILS against its use_mean = True output;
  * the use_mean = True output with its rows rotated by one fails too;
  * the len = 1 sequence (where a fixture has one) has the same embedding either way: the mean of one row is that row.

Run:  python tests/golden/make_golden_encoder_mean.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from haconvdr_amd import synth  # noqa: E402
from tests import parity  # noqa: E402
from tests.golden.make_golden_encoder import REF, SENS_STD, encoder_case_inputs, load_case  # noqa: E402,F401

CASES = [
    # name, n_layers, L, lens, layer_matrix_std: every 32-row block edge, a one-token sequence, and sequences that cross 256-row tile seams
    ("l2_edges", 2, 512, [1, 5, 31, 32, 33, 64, 257, 511, 512], SENS_STD),
    # the lengths of make_golden_encoder's l12_sens_mixed
    ("l12_mixed", 12, 512, [8, 31, 64, 129, 256, 384, 512, 40, 500, 333], 0.03),
]


def case_path(name):
    return os.path.join(HERE, "encoder_mean", f"{name}.npz")


def main(only=None):
    sys.path[:0] = [REF, os.path.join(REF, "src")]
    import torch
    import models  # the reference's src/models.py
    from transformers import RobertaConfig
    for name, n_layers, L, lens, mstd in CASES:
        if only and name not in only:
            continue
        seed = int.from_bytes(("m" + name).encode()[:4], "little")
        cfg = RobertaConfig(vocab_size=50265, hidden_size=768, num_hidden_layers=n_layers, num_attention_heads=12,
                            intermediate_size=3072, max_position_embeddings=514, type_vocab_size=1, layer_norm_eps=1e-5,
                            pad_token_id=1, bos_token_id=0, eos_token_id=2)
        model = models.ANCE(cfg).eval()
        sd = synth.ance_state_dict(0xA11CE, n_layers, layer_matrix_std=mstd)
        missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        assert not unexpected and all(m.startswith("classifier.") or "position_ids" in m for m in missing), (missing, unexpected)
        ids, mask = encoder_case_inputs(seed, lens, L)
        ids[1, 3] = 1            # RoBERTa's pad id INSIDE two sequences (as l2_mixed): the cumsum position rule
        ids[6, 100] = 1
        outs = {}
        for use_mean in (True, False):
            model.use_mean = use_mean
            with torch.no_grad():
                outs[use_mean] = model(torch.from_numpy(ids), torch.from_numpy(mask)).numpy()
        ref_mean, ref_first = outs[True], outs[False]
        assert not parity.embeddings_match(ref_first, ref_mean), f"{name}: <s> pooling passes for mean pooling"
        assert not parity.embeddings_match(np.roll(ref_mean, 1, axis=0), ref_mean), f"{name}: rotated rows pass"
        for b, n in enumerate(lens):
            if n == 1:
                d = float(np.abs(ref_mean[b] - ref_first[b]).max())
                assert d <= 1e-6, (name, b, d)
                print(name, f"len-1 sequence {b}: |mean - first| max {d:.1e}")
        os.makedirs(os.path.dirname(case_path(name)), exist_ok=True)
        np.savez_compressed(case_path(name), seed=seed, n_layers=n_layers, L=L, lens=np.array(lens), ids=ids.astype(np.int32),
                            mask=mask.astype(np.int8), ref_out=ref_mean, ref_first=ref_first, layer_matrix_std=mstd)
        sp, m = parity.spread(ref_mean), parity.measure(ref_first, ref_mean)
        print(name, ref_mean.shape, "min pairwise 1-cos %.3e (centred %.3e)" % (sp["raw_min"], sp["centred_min"]),
              "| first vs mean: 1-cos %.3e (bound %.1e), centred %.3e (bound %.1e), rel L2 %.3f (bound %.2f)"
              % (m["raw"], m["raw_bound"], m["centred"], m["centred_bound"], m["rel_l2"], m["rel_l2_bound"]))


if __name__ == "__main__":
    main(set(sys.argv[1:]))
