"""precision = split (hi + lo bf16 operand pairs, three MFMAs per product: haconvdr_amd/csrc/split.inc), the CPU side:
the premise and scope of the mode by emulation, the pair's defining property, and what the shipped library's code objects
must show for the new kernels."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_attribution  # noqa: E402
from haconvdr_amd import synth  # noqa: E402
from haconvdr_amd.encoder import split_bf16  # noqa: E402
from oracle import ance_oracle  # noqa: E402

CSRC = os.path.join(ROOT, "haconvdr_amd", "csrc")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
SPLIT_KERNELS = ("gemm_split_nt_kernelILi0E", "gemm_split_nt_kernelILi1E", "gemm_split_nt_kernelILi2E", "attention_split_kernel",
                 "ln_split_rows_kernel", "f32_to_bf16_lo_kernel")


def _split_round(t):
    hi = t.to(torch.bfloat16).to(torch.float32)
    return hi + (t - hi).to(torch.bfloat16).to(torch.float32)


def test_split_everywhere_is_1000x_closer_and_splitting_the_gemms_alone_is_not(monkeypatch):
    """The emulation behind the issue's table on a size that runs in well under a minute (4 sequences x 128, 12 layers,
    layer-matrix std 0.12): tests/bf16_attribution.py's forward with its rounding function swapped, against
    oracle.ance_forward (the unrounded fp32 run).
      * every MFMA operand as hi + lo, fp32 residual stream (what precision = split computes): at least 1000 x closer to the
        unrounded run than bf16 everywhere (what the shipped kernels compute);
      * the projection / FFN operands exact -- the limit of splitting the GEMMs alone -- with Q, K, P, V still bf16 keeps more
        than a tenth of the bf16 error: the mode has to cover the attention products too."""
    L, std = 128, 0.12
    ids, lens = synth.token_batch(0x5EED, 4, L, min_len=L // 4)
    mask = (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)
    sd = synth.ance_state_dict(0x0D17, 12, layer_matrix_std=std)
    with torch.no_grad():
        ref = ance_oracle.ance_forward(sd, ids, mask)
        assert bf16_attribution.omc(bf16_attribution.forward(sd, ids, mask, set()), ref) < 1e-9     # the same arithmetic when nothing is rounded
        e_bf16 = bf16_attribution.omc(bf16_attribution.forward(sd, ids, mask, {"qk", "pv", "gemm", "resid"}), ref)
        e_attn = bf16_attribution.omc(bf16_attribution.forward(sd, ids, mask, {"qk", "pv"}), ref)
        monkeypatch.setattr(bf16_attribution, "bf", _split_round)
        e_split = bf16_attribution.omc(bf16_attribution.forward(sd, ids, mask, {"qk", "pv", "gemm"}), ref)
    print(f"max 1-cos vs ance_forward: bf16 everywhere {e_bf16:.2e}, GEMM operands exact {e_attn:.2e}, hi+lo everywhere {e_split:.2e}")
    assert e_bf16 > 1e-5, e_bf16                       # (the recipe is sensitive to the operand format at all)
    assert e_split * 1000 <= e_bf16, (e_split, e_bf16)
    assert e_attn > 0.1 * e_bf16, (e_attn, e_bf16)


def test_hi_plus_lo_reproduces_fp32_to_2_pow_minus_16_and_never_worse_than_bf16():
    """The pair's defining property on the host twin of the device helper (split.inc split_bf16): hi + lo reproduces an fp32
    value to <= 2^-16 relative for normal values (zero and the ends of the bf16 range included), and where lo underflows
    (values near the smallest normals) it degrades to the bf16 error, never beyond it."""
    rng = np.random.default_rng(7)
    big = float(torch.finfo(torch.bfloat16).max)
    x = np.concatenate([rng.standard_normal(200000).astype(np.float32) * np.float32(10.0) ** rng.integers(-20, 20, 200000).astype(np.float32),
                        np.array([0.0, -0.0, big, -big, 1.0, -1.0, 1.0 + 2.0 ** -9, 1.0 + 2.0 ** -8 + 2.0 ** -17, 3.0e38, -3.0e38], np.float32)])
    x = x[np.isfinite(x)]
    hi, lo = split_bf16(x)
    assert np.isfinite(hi).all() and np.isfinite(lo).all()
    err = np.abs((hi.astype(np.float64) + lo.astype(np.float64)) - x.astype(np.float64))
    err_hi = np.abs(hi.astype(np.float64) - x.astype(np.float64))
    assert (err <= err_hi).all()                                           # never worse than bf16 alone
    assert (err <= np.abs(x.astype(np.float64)) * 2.0 ** -16).all()        # normal values: lo is a normal or zero bf16
    assert (hi[x == 0] == 0).all() and (lo[x == 0] == 0).all()
    # lo underflows: the smallest normal fp32 values (lo would lie below bf16's subnormals or is flushed): bf16's own error bounds it
    tiny = (np.float32(2.0 ** -126) * (1.0 + rng.random(1000))).astype(np.float32)
    hi, lo = split_bf16(tiny)
    err = np.abs((hi.astype(np.float64) + lo.astype(np.float64)) - tiny.astype(np.float64))
    assert (err <= np.abs(hi.astype(np.float64) - tiny.astype(np.float64))).all()
    assert (err <= tiny.astype(np.float64) * 2.0 ** -8).all()


def _resource_blocks():
    path = os.path.join(CSRC, "encoder.resources.txt")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", CSRC])
    return re.split(r"remark: Function Name: ", open(path).read())


def test_split_kernels_have_no_spill_no_scratch_and_fit_the_lds():
    """A spill reload is a vmcnt(0) in the LDS-DMA stream of the split GEMM / attention kernels: hipcc's resource report must
    show none, for every new kernel; the dynamic LDS the host asks for fits a CU's 160 KiB."""
    seen = set()
    for b in _resource_blocks():
        head = b.split("\n", 1)[0]
        for k in SPLIT_KERNELS:
            if k in head:
                seen.add(k)
                assert int(re.search(r"VGPRs Spill: (\d+)", b).group(1)) == 0, b[:200]
                assert int(re.search(r"SGPRs Spill: (\d+)", b).group(1)) == 0, b[:200]
                assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b[:200]
                assert int(re.search(r"VGPRs: (\d+)", b).group(1)) <= 256
    assert seen == set(SPLIT_KERNELS), seen
    src = open(os.path.join(CSRC, "split.inc")).read()
    m = re.search(r"constexpr int SPLIT_GEMM_LDS = ([0-9 *+]+);", src)
    assert m and eval(m.group(1)) == 147456 <= 163840                        # two stages of four 16-KiB tiles + four 4-KiB patches
    m = re.search(r"constexpr int ATS_STAGE = ATS_CHUNK \* 128 \* 4;", src)
    assert m and "constexpr int ATS_CHUNK = 64;" in src and 2 * 64 * 128 * 4 <= 81920   # two workgroups per CU


def test_split_kernels_are_in_the_library_with_three_mfmas_per_product(tmp_path):
    """The shipped library is disassembled: every new kernel is there, and the split GEMM holds three times the bf16 MFMAs of
    the classic 128^2 kernel it is modelled on (16 per k-tile there: 4 k-steps x 2 x 2 fragment pairs), the split attention
    kernel three per product of the one-block step -- the mode cannot silently be two terms."""
    if not os.path.exists(OBJDUMP):
        pytest.skip("no llvm-objdump in this image")
    lib = os.path.join(CSRC, "libhaconvdr.so")
    assert os.path.exists(lib), "libhaconvdr.so is not built (python -c 'import __graft_entry__ as g; g.build()')"
    shutil.copy(lib, tmp_path / "libhaconvdr.so")
    subprocess.run([OBJDUMP, "--offloading", "libhaconvdr.so"], cwd=tmp_path, check=True, capture_output=True)
    mfma, scratch = {}, {}
    for c in sorted(f for f in os.listdir(tmp_path) if f.startswith("libhaconvdr.so.") and "gfx950" in f):
        dis = subprocess.run([OBJDUMP, "-d", c], cwd=tmp_path, check=True, capture_output=True, text=True).stdout
        name = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.*)>:", line)
            if m:
                name = m.group(1)
                continue
            if name and "v_mfma_f32_32x32x16_bf16" in line:
                mfma[name] = mfma.get(name, 0) + 1
            if name and "scratch_" in line:
                scratch[name] = scratch.get(name, 0) + 1

    def of(needle):
        hit = [n for n in mfma if needle in n]
        assert len(hit) == 1, (needle, hit)
        return hit[0]
    for epi in (0, 1, 2):
        classic = mfma[of(f"gemm_bf16_nt_kernelILi{epi}ELi2E")]
        split = mfma[of(f"gemm_split_nt_kernelILi{epi}E")]
        assert classic == 16 and split == 3 * classic, (epi, classic, split)
    # the one-block step: 4 k-steps of S^T = K.Q^T and 2 x 2 of O^T = V^T.P^T, in the common and the masked form
    assert mfma[of("attention_split_kernel")] == 3 * 2 * (4 + 4), mfma[of("attention_split_kernel")]
    assert not [n for n in scratch if "split" in n], scratch


# ---------------------------------------------------------------------------------------------------------------------------
# the yardstick of the teacher-forced bounds (tests/split_parity.py): oracle.ance_oracle family="split" against family=None


def test_split_family_is_the_classic_arithmetic_with_the_pair_rounding(monkeypatch):
    """family="split" = family="classic" with every bf16(.) replaced by v -> bf16(v) + bf16(v - bf16(v)) (the host twin
    split_bf16, hi + lo summed in fp64), embed, layer and tail; and it is far closer to the unrounded chain than classic."""
    from tests import split_parity as sp
    from tests.golden.make_golden_encoder import encoder_case_inputs
    sd = sp.weights("std012", 3)
    ids, mask = encoder_case_inputs(3, [1, 33, 64, 70], 96)
    x = torch.randn(1000, dtype=torch.float64) * 10.0 ** torch.randint(-6, 6, (1000,))
    hi, lo = split_bf16(x.numpy().astype(np.float32))
    assert np.array_equal(ance_oracle.split2(x).numpy(), hi.astype(np.float64) + lo.astype(np.float64))
    st = ance_oracle.ance_embed(sd, ids, mask)
    got = [ance_oracle.ance_embed(sd, ids, mask, family="split")["norm"], ance_oracle.ance_layer(sd, 0, st, mask, family="split")["norm"],
           ance_oracle.ance_tail(sd, 0, st, mask, family="split")]
    classic = ance_oracle.ance_layer(sd, 0, st, mask, family="classic")["norm"]
    exact = ance_oracle.ance_layer(sd, 0, st, mask)["norm"]
    monkeypatch.setattr(ance_oracle, "bf16", ance_oracle.split2)
    want = [ance_oracle.ance_embed(sd, ids, mask, family="classic")["norm"], ance_oracle.ance_layer(sd, 0, st, mask, family="classic")["norm"],
            ance_oracle.ance_tail(sd, 0, st, mask, family="classic")]
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    valid = np.asarray(mask, bool)
    assert sp.rel(got[1].numpy(), exact.numpy(), valid) * 100 < sp.rel(classic.numpy(), exact.numpy(), valid)


def test_recorded_emulation_constants_match_the_split_faithful_reference():
    """E_emul(stage) = rel(family "split", family None) on the unrounded chain run freely from ance_embed, recomputed for every
    (recipe, batch, stage) whose bound tests/test_encoder_precision_shapes_gpu.py derives from it: the recorded constants are
    within 5 %; the layer figure does not depend on the batch (the two std-0.08 edge batches agree within 2 %), which is what
    lets the committed LAYER_BOUNDS carry over to new batches; those bounds stand EMUL_FACTOR (within 5 %) above the emulation;
    and the key_chunk mutation lies >= 3 x beyond every bound of the SPLIT_EDGES batch it is asserted on."""
    from tests import split_parity as sp
    from tests import test_encoder_precision_shapes_gpu as shapes
    cases = {k: set(v) for k, v in shapes.E_EMUL.items()}
    for recipe, batch in shapes.LAYER_EMUL:
        cases.setdefault((recipe, 3, batch), set()).update({("layer", 0), ("layer", 1)})
    got = {}
    with torch.no_grad():
        for (recipe, depth, batch), stages in cases.items():
            sd = sp.weights(recipe, depth)
            ids, mask = sp.batch(batch)
            chain = sp.unrounded_chain(sd, ids, mask, depth)
            got[(recipe, depth, batch)] = e = sp.emulation(sd, ids, mask, depth, layers=any(s[0] == "layer" for s in stages),
                                                            tail=any(s[0] == "tail" for s in stages), chain=chain)
            if batch == "split_edges" and recipe in shapes.STD:
                valid = np.asarray(mask, bool)
                for n in range(depth - 1):
                    mut = ance_oracle.ance_layer(sd, n, chain[n - 1], mask, mutate="key_chunk")["norm"].numpy()
                    assert sp.rel(mut, chain[n]["norm"].numpy(), valid) >= 3.0 * shapes.bound(recipe, depth, batch, "layer", n), (recipe, n)
                base = ance_oracle.ance_tail(sd, depth - 1, chain[depth - 2], mask).numpy()
                mut = ance_oracle.ance_tail(sd, depth - 1, chain[depth - 2], mask, mutate="key_chunk").numpy()
                assert sp.rel(mut, base) >= 3.0 * shapes.bound(recipe, depth, batch, "tail", depth - 1), recipe
    for key, rec in shapes.E_EMUL.items():
        for stage, v in rec.items():
            print(key, stage, f"recorded {v:.3e} recomputed {got[key][stage]:.4e}")
            assert abs(v / got[key][stage] - 1.0) <= 0.05, (key, stage, v, got[key][stage])
    for (recipe, batch), rec in shapes.LAYER_EMUL.items():
        e = got[(recipe, 3, batch)]
        print(recipe, batch, f"layers {e[('layer', 0)]:.4e} {e[('layer', 1)]:.4e}")
        for n in (0, 1):
            assert abs(rec[n] / e[("layer", n)] - 1.0) <= 0.05, (recipe, batch, n, rec[n], e[("layer", n)])
        worst = max(e[("layer", 0)], e[("layer", 1)])
        assert abs(shapes.LAYER_BOUNDS[shapes.STD[recipe]]["layer"] / worst / sp.EMUL_FACTOR - 1.0) <= 0.05, (recipe, batch, worst)
    for n in (0, 1):
        a, b = got[("std008", 3, "edges")][("layer", n)], got[("std008", 3, "split_edges")][("layer", n)]
        assert abs(a / b - 1.0) <= 0.02, (n, a, b)


def test_peaked_recipe_moves_the_softmax_reference():
    """The peaked recipe (Q and K x PEAKED_SCALE) does what it is for, on the reference alone: the window rule
    (_window_reference on the unrounded chain's base-2 logits) moves its reference -- the split attention kernel's ballot
    branch, delta, the rescaling of lsum and o -- on at least 10 % of the (sequence, head) items of layer 0 of SPLIT_EDGES;
    the plain std-0.08 weights never move it."""
    from tests import split_parity as sp
    ids, mask = sp.batch("split_edges")
    lens = mask.sum(1).tolist()
    frac = {}
    for recipe in ("std008", "peaked"):
        sd = sp.weights(recipe, 3)
        x, mean, rstd, g_in, b_in, xn = ance_oracle._layer_input(sd, 0, ance_oracle.ance_embed(sd, ids, mask))
        Q, K = (ance_oracle._project(sd, 0, nm, x, mean, rstd, xn, g_in, b_in, None, 12) for nm in ("query", "key"))
        moved = later = total = 0
        for s, n in enumerate(lens):
            qh, kh = (t[s, :n].reshape(n, 12, 64).transpose(0, 1) for t in (Q, K))
            m = ance_oracle._window_reference(qh @ kh.transpose(-1, -2))          # [heads, n, blocks]
            moved += int((m != 0).flatten(1).any(1).sum())
            later += int((m[..., 1:] != m[..., :-1]).flatten(1).any(1).sum())      # moved after the first block: l and O are rescaled
            total += 12
        frac[recipe] = (moved / total, later / total)
    print("share of (sequence, head) items whose reference moves (at all, after the first block):", frac)
    assert frac["std008"][0] == 0.0, frac
    assert frac["peaked"][0] >= 0.10 and frac["peaked"][1] >= 0.10, (sp.PEAKED_SCALE, frac)
