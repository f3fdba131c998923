"""Mean pooling on the GPU: hac_encoder_set_option(enc, "pooling", "mean") -- the reference's model.use_mean = True
(src/models.py:52-61) -- through every forward structure (gemm8, classic, precision = split), through the C ABI.

Two yardsticks:
  * the pool-stage bound (tests/test_encoder_mean_pool.py: POOL_STAGE_BOUND, derived there on the CPU) for everything that is
    teacher-forced -- hac_encoder_layer_state(n_layers - 1) gives the very rows and statistics pool_mean_kernel read, the fp64
    helper pools them and applies the head, and only fp32 arithmetic separates that from the forward's output;
  * the fixture-scaled bounds of tests/parity.py for everything compared with the reference's own outputs
    (tests/golden/encoder_mean/*.npz) or with this repository's fp32 restatement of the forward + the fp64 helper.
Every figure is printed before it is asserted.
"""
import numpy as np
import pytest

from tests import mean_pool, parity
from tests.test_encoder_mean_pool import POOL_STAGE_BOUND, golden, weights

pytestmark = pytest.mark.gpu

ROUTES = {                      # option sets; every one is undone by reset()
    "8phase": {"gemm": "8phase"},
    "classic": {"gemm": "classic"},
    "split": {"precision": "split"},
}
DEFAULTS = {"gemm": "auto", "precision": "bf16", "pooling": "first", "graph": "auto", "max_tokens": "524288"}
PLAN_GEMM = {"8phase": "gemm8", "classic": "classic128", "split": "split128"}
_ENC = {}


def encoder(n_layers, mstd):
    from haconvdr_amd.encoder import ANCEEncoder
    if (n_layers, mstd) not in _ENC:
        _ENC[(n_layers, mstd)] = ANCEEncoder.from_state_dict(weights(n_layers, mstd))
    return _ENC[(n_layers, mstd)]


def reset(enc):
    for k, v in DEFAULTS.items():
        enc.set_option(k, v)


def plan(enc):
    return dict(kv.split("=") for kv in enc.last_plan().split())


def forward(enc, ids, mask, pooling="mean", **options):
    """One forward under the options (undone afterwards): (embeddings, plan dict)."""
    try:
        for k, v in dict(options, pooling=pooling).items():
            enc.set_option(k, v)
        return np.asarray(enc(ids, mask)), plan(enc)
    finally:
        reset(enc)


def batch(seed, B, L, min_len):
    from haconvdr_amd import synth
    ids, lens = synth.token_batch(seed, B, L, min_len=min_len)
    return ids.astype(np.int32), (np.arange(L)[None, :] < lens[:, None]).astype(np.int32)


def batch_of(lens, L=512, seed=0x3EA9):
    from tests.golden.make_golden_encoder import encoder_case_inputs
    ids, mask = encoder_case_inputs(seed, lens, L)
    return ids.astype(np.int32), mask.astype(np.int32)


_REF = {}


def reference(key, n_layers, mstd, ids, mask):
    """This repository's fp32 restatement of the forward (oracle.ance_forward's last hidden state) + the fp64 helper; cached."""
    from oracle import ance_oracle
    if key not in _REF:
        sd = weights(n_layers, mstd)
        _REF[key] = mean_pool.pool_and_head(sd, ance_oracle.ance_forward(sd, ids, mask, hidden=True)[-1], mask)
    return _REF[key]


def teacher_forced(enc, sd, n_layers, ids, mask, **options):
    """(forward's embeddings, helper's embeddings from the forward's own last-layer state, plan) in mean mode."""
    try:
        for k, v in dict(options, pooling="mean").items():
            enc.set_option(k, v)
        st = enc.layer_state(ids, mask, n_layers - 1)
        out = np.asarray(enc(ids, mask))
        p = plan(enc)
    finally:
        reset(enc)
    return out, mean_pool.pool_rows_and_head(sd, n_layers, st, mask), p


# ---------------------------------------------------------------------------------------------------------------- 1. pool stage
@pytest.mark.parametrize("route", list(ROUTES))
def test_pool_stage_teacher_forced(route):
    """pool_mean_kernel + head alone, on the 9-sequence edge batch (lens 1 .. 512; on gemm8 bf16 rows over >= 7 row tiles, the
    257- and 511-row sequences crossing tile seams)."""
    ids, mask, _, _, n_layers, mstd = golden("l2_edges")
    enc, sd = encoder(n_layers, mstd), weights(n_layers, mstd)
    out, ref, p = teacher_forced(enc, sd, n_layers, ids, mask, **ROUTES[route])
    fig = mean_pool.rel_rows(out, ref)
    print(route, "pool stage rel per sequence", fig, "bound", POOL_STAGE_BOUND, p)
    assert p["gemm"] == PLAN_GEMM[route] and p["pool"] == "mean", p
    assert np.isfinite(out).all() and fig.max() <= POOL_STAGE_BOUND, (route, fig)


# ---------------------------------------------------------------------------------------------------------------- 2. goldens
@pytest.mark.parametrize("name,route", [("l2_edges", "classic"), ("l2_edges", "8phase"), ("l12_mixed", "classic"), ("l12_mixed", "8phase"),
                                        ("l12_mixed", "split")])
def test_golden_parity_with_the_reference_use_mean(name, route):
    ids, mask, ref, _, n_layers, mstd = golden(name)
    enc = encoder(n_layers, mstd)
    out, p = forward(enc, ids, mask, **ROUTES[route])
    print(name, route, {k: v for k, v in parity.measure(out, ref).items() if k != "spread"}, p)
    assert p["gemm"] == PLAN_GEMM[route] and p["pool"] == "mean", p
    parity.assert_embeddings_match(out, ref, what=(name, route))
    parity.assert_negative_control(out, ref)
    first, p1 = forward(enc, ids, mask, pooling="first", **ROUTES[route])
    assert "pool" not in p1, p1
    assert not parity.embeddings_match(first, ref), "the <s>-pooled embeddings pass for the mean-pooled reference"


# ---------------------------------------------------------------------------------------------------------------- 3. len = 1
@pytest.mark.parametrize("route", ["classic", "8phase"])
def test_one_token_sequence_is_its_own_mean(route):
    ids, mask, ref, _, n_layers, mstd = golden("l2_edges")
    enc, sd = encoder(n_layers, mstd), weights(n_layers, mstd)
    b = int(np.flatnonzero(mean_pool.lens_of(mask) == 1)[0])
    try:
        for k, v in dict(ROUTES[route], pooling="mean").items():
            enc.set_option(k, v)
        st = enc.layer_state(ids, mask, n_layers - 1, normalized=True)
        out = np.asarray(enc(ids, mask))
    finally:
        reset(enc)
    row0 = mean_pool.head(sd, st["norm"][b, :1])                # the head applied to the sequence's row 0
    fig = float(mean_pool.rel_rows(out[b:b + 1], row0)[0])
    first, _ = forward(enc, ids, mask, pooling="first", **ROUTES[route])
    m = parity.measure(out, ref)
    cos = float(parity.one_minus_cos(first[b], out[b]))
    rel = float(np.linalg.norm(first[b].astype(np.float64) - out[b]) / np.linalg.norm(ref[b] - ref.mean(0)))
    print(route, "len-1: mean vs head(row 0) rel", fig, "bound", POOL_STAGE_BOUND, "| first vs mean 1-cos", cos, "bound", m["raw_bound"],
          "rel L2", rel, "bound", m["rel_l2_bound"])
    assert fig <= POOL_STAGE_BOUND
    assert cos <= m["raw_bound"] and rel <= m["rel_l2_bound"]


# ---------------------------------------------------------------------------------------------------------------- 4. serving
@pytest.mark.parametrize("precision", ["bf16", "split"])
@pytest.mark.parametrize("B,L", [(4, 512), (1, 256)])
def test_serving_shapes_capture_replay_and_mode_switches(B, L, precision):
    enc = encoder(2, 0.08)
    ids, mask = batch(0x5E7 + B * 1000 + L, B, L, max(1, L // 4))
    opts = {"precision": precision}
    before, _ = forward(enc, ids, mask, pooling="first", graph="off", **opts)
    eager, p = forward(enc, ids, mask, graph="off", **opts)
    assert p["graph"] == "off" and p["pool"] == "mean", p
    after, _ = forward(enc, ids, mask, pooling="first", graph="off", **opts)
    assert np.array_equal(before, after), "a mean-mode call changed the default mode's bits"
    enc.set_option("attn_qs_pin", "0")          # (its default; setting it drops the captured graphs: every shape starts eager)
    seen = []
    for pooling in ("mean", "mean", "mean", "first", "first", "mean", "first", "mean"):
        out, p = forward(enc, ids, mask, pooling=pooling, **opts)
        seen.append((pooling, p["graph"], p.get("pool")))
        assert p.get("pool") == ("mean" if pooling == "mean" else None), (seen, p)      # the plan of THIS mode's forward ...
        assert np.array_equal(out, eager if pooling == "mean" else before), seen         # ... and its bits, never the other mode's graph
    assert [g for _, g, _ in seen] == ["eager-first", "replay", "replay", "eager-first", "replay", "replay", "replay", "replay"], seen
    assert not np.array_equal(eager, before)


# ---------------------------------------------------------------------------------------------------------------- 5. sub-batches
def test_sub_batches_of_a_max_tokens_split():
    lens = [512, 511, 500, 480, 450, 400, 384, 333, 300, 257, 64, 1]        # 4352 padded rows: two passes of <= 4096
    ids, mask = batch_of(lens)
    enc = encoder(2, 0.08)
    ref = reference("sub12", 2, 0.08, ids, mask)
    out, p = forward(enc, ids, mask, max_tokens="4096")
    again, _ = forward(enc, ids, mask, max_tokens="4096")
    print("sub-batches", {k: v for k, v in parity.measure(out, ref).items() if k != "spread"}, p)
    assert int(p["sub_batches"]) >= 2 and p["pool"] == "mean", p
    parity.assert_embeddings_match(out, ref, what="sub-batches")
    parity.assert_negative_control(out, ref)
    assert np.array_equal(out, again)


# ---------------------------------------------------------------------------------------------------------------- 6. few / many
def test_single_sequences():
    """B = 1: one sequence spread over the pool kernel's six column workgroups.  Each alone against its own last-layer state
    (pool-stage bound), and the three single-sequence embeddings together against the reference of the three as a batch."""
    lens = [512, 33, 100]
    ids, mask = batch_of(lens, seed=0x3EAA)
    enc, sd = encoder(2, 0.08), weights(2, 0.08)
    ref = reference("single3", 2, 0.08, ids, mask)
    outs = []
    for b in range(len(lens)):
        out, tf, p = teacher_forced(enc, sd, 2, ids[b:b + 1], mask[b:b + 1])
        fig = float(mean_pool.rel_rows(out, tf)[0])
        print("B = 1, len", lens[b], "pool stage rel", fig, "bound", POOL_STAGE_BOUND, p)
        assert p["pool"] == "mean" and fig <= POOL_STAGE_BOUND, (lens[b], fig, p)
        outs.append(out[0])
    print("singles vs batch reference", {k: v for k, v in parity.measure(np.stack(outs), ref).items() if k != "spread"})
    parity.assert_embeddings_match(np.stack(outs), ref, what="single sequences")


def test_forty_ragged_sequences_through_the_large_batch_family():
    """40 x <= 512, ragged (drawn with min_len = 1): 11456 rows -- auto-routed to gemm8, both attention classes, a partial last 256-row tile."""
    ids, mask = batch(0x3EA0, 40, 512, 1)
    enc = encoder(2, 0.08)
    ref = reference("ragged40", 2, 0.08, ids, mask)
    out, p = forward(enc, ids, mask)
    print("ragged40", {k: v for k, v in parity.measure(out, ref).items() if k != "spread"}, p)
    rows = (mean_pool.lens_of(mask) + 31) // 32 * 32
    assert rows.sum() == 11456 and rows.sum() % 256 and (rows > 256).any() and (rows <= 256).any()
    assert p["gemm"] == "gemm8" and p["pool"] == "mean", p
    parity.assert_embeddings_match(out, ref, what="ragged40")
    parity.assert_negative_control(out, ref)


# ---------------------------------------------------------------------------------------------------------------- 7. flags
def test_flagged_sequence_is_nan_in_its_row_only():
    import torch
    from haconvdr_amd._lib import HacError
    enc = encoder(2, 0.08)
    ids, mask = batch(0x3EAB, 4, 64, 8)
    bad = mask.copy()
    bad[2, 3] = 0                                   # a hole: not a prefix mask
    try:
        enc.set_option("pooling", "mean")
        dev = lambda a: torch.from_numpy(a.astype(np.int64)).cuda()      # noqa: E731
        good = enc(dev(ids), dev(mask)).cpu().numpy()
        out = enc(dev(ids), dev(bad)).cpu().numpy()
        with pytest.raises(HacError) as e:
            enc(ids, bad)
    finally:
        reset(enc)
    assert "sequence 2" in str(e.value), str(e.value)
    assert np.isfinite(good).all() and np.isnan(out[2]).all()
    np.testing.assert_array_equal(out[[0, 1, 3]], good[[0, 1, 3]])


# ---------------------------------------------------------------------------------------------------------------- 8. interface
def test_interface():
    from haconvdr_amd._lib import HacError
    from haconvdr_amd.encoder import ANCEEncoder
    enc = encoder(2, 0.08)
    ids, mask = batch(0x3EAB, 4, 64, 8)
    with pytest.raises(HacError) as e:
        enc.set_option("pooling", "max")
    assert e.value.code == 1                        # HAC_ERR_INVALID
    assert enc.use_mean is False
    with pytest.raises(HacError) as e:
        enc.layer_state(ids, mask, 1)
    assert "the last layer continues the <s> rows only" in str(e.value)
    enc(ids, mask)
    assert "pool=" not in enc.last_plan(), enc.last_plan()
    try:
        enc.use_mean = True
        assert enc.use_mean is True
        st = enc.layer_state(ids, mask, 1)
        assert st["rows"].shape == (4, 64, 768) and np.isfinite(st["rows"]).all() and (st["rstd"][mask == 1] > 0).all()
        with pytest.raises(HacError):
            enc.layer_state(ids, mask, 2)
        enc(ids, mask)
        assert enc.last_plan().endswith(" pool=mean"), enc.last_plan()
        enc.use_mean = False
        assert enc.use_mean is False
        enc(ids, mask)
        assert "pool=" not in enc.last_plan(), enc.last_plan()
    finally:
        reset(enc)
    assert ANCEEncoder(n_layers=1, pooling="mean").use_mean is True
