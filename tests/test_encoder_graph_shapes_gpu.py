"""Captured forwards at their own shapes: HIP-graph capture and replay beyond four sequences.

A forward of at most 16384 padded rows is captured on its second call and replayed afterwards (forward_graph, encoder.hip).  The
other capture / replay tests stop at 4 x 512: classic 128^2 GEMMs with split-K, query-split attention in one launch, no woven
kernel, no fix-up pass.  The eligible range is eight times wider, and inside a captured graph it reaches code those tests only run
under plain launches.  The shapes here (tests/graph_shapes.py, SHAPES; forms pinned on the CPU by tests/test_graph_shapes.py):

  qs2_long     8 x 512   att_qs 2, both length classes in one launch, classic128, split-K 1/2
  qs2_short    8 x 256   att_qs 2, no long class
  woven_c128  12 x 512   first batch size without a query split: attention_pipe_kernel<8>, the captured memset of its counters and
                         the fix-up launches; classic-kernel workgroups take second items
  c128_top    18 x 512   last classic128 shape (9216 rows)
  g8_first    19 x 512   first gemm8 shape (9728 rows): the persistent 256^2 kernels, ln_combine_kernel, the folded LayerNorm,
                         cls_q_kernel and the classic tail on Mc = 256 compact rows, on total_rows read from the device
  g8_384      40 x 384   gemm8, woven at L32 = 384
  g8_top      32 x 512   largest eligible shape (16384 rows); 33 x 512 reports graph=off
  g8_short64 256 x  64   gemm8, short class only
  g8_short32 512 x  32   gemm8, Mc = 512, seq_offsets_kernel with two sequences per thread

The referee of every comparison is a second handle on the same state dict with graph = off and attn_pipe = off: plain launches and
the one-block attention kernel.  Every comparison is bit for bit.
  a. four calls per shape, each on ids and lengths of its own (eager-first, replay, replay, replay; with a long class the third
     call has no sequence beyond 256 tokens, the fourth none below 257 but one of a single token): a graph that read stale
     inputs or host-frozen lengths cannot pass;
  b. six sequences of the last call of three shapes against the fp32 oracle, tests/parity.py's fixture-scaled bounds and its
     negative control;
  c. the fix-up pass inside a replay (Q and K x 8: flagged items on every replay, the same count each time; x 3: none);
  d. pooling = mean, BERTEncoder and precision = split at a large shape; first and mean alternating on one handle;
  e. a capture whose eager-first forward ran with every woven-eligible layer in pipe_skip_mask and whose capturing call is the 64th
     run_forward, the one that clears the mask: ws_redo must have been sized outside the capture (fwd_build);
  f. a larger forward between replays of a gemm8 shape regrows gemm8's workspaces: re-captured, same bits.

Measured (MI355X, 256 CUs; every test prints its figures before it asserts): 22 tests, 7.5 s for the file, 2.7 s of it the first
test's state dict and handles, about 1 s per new state dict, every other test 0.01 - 0.3 s (a forward here is 0.3 - 1.3 ms).
  a. plans eager-first, replay, replay, replay at all nine shapes, the form of the mirror; 24576 ... 1572864 embedding elements per
     shape, 2.8 M in all, no differing bit.  Packed rows of the calls, e.g. 19 x 512: 4736, 6048, 2688 (no long sequence), 7936 of 9728.
  b. 1-cos / centred 1-cos / relative L2 against the oracle, with tests/parity.py's bounds for these fixtures (rows >= 0.10 apart):
     12 x 512   1.2e-4 (1e-3)   8.8e-4 (9.7e-2)   0.042 (0.25)
     19 x 512   1.0e-4 (1e-3)   9.9e-4 (9.6e-2)   0.045 (0.25)
     256 x 64   2.2e-4 (1e-3)   1.1e-3 (9.1e-2)   0.046 (0.25)       rows rotated by one fail
  c. redo counts (wave-level flags) after the eager-first call, the capturing call and two replays: x 8 at 12 x 512 1152 four times,
     at 19 x 512 1824 four times; x 3: 0.
  e. forward 1 at 12 x 512 woven with 1152 flags, forward 2 single, single after 62 forwards; 24 x 512: eager-first / single,
     replay / woven, replay / woven, 2304 flags, the referee's bits.
No defect found beyond the ws_redo reservation (LABNOTES.md).
"""
import functools
import time

import numpy as np
import pytest

from tests import bert_ref, parity
from tests import graph_shapes as gs
from tests.classic_tiles import bits
from tests.test_encoder_gpu import _plan, _scaled_qk_encoder, state_dict

pytestmark = pytest.mark.gpu

KINDS4 = ["eager-first", "replay", "replay", "replay"]


def n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def referee(cls, sd, **kw):
    """graph = off and attn_pipe = off: plain launches, the one-block attention kernel."""
    ref = cls.from_state_dict(sd, **kw)
    ref.set_option("graph", "off")
    ref.set_option("attn_pipe", "off")
    return ref


@functools.lru_cache(maxsize=None)
def calm_pair():
    """(handle under test, referee, state dict): 2 layers, layer matrices N(0, 0.08^2) -- attention depends on content."""
    from haconvdr_amd.encoder import ANCEEncoder
    sd = state_dict(2, 0.08)
    return ANCEEncoder.from_state_dict(sd), referee(ANCEEncoder, sd), sd


@functools.lru_cache(maxsize=None)
def scaled_weights(scale):
    """(state dict with Q and K x scale, its referee).  The handle under test is made new for every test: a handle that has
    seen flagged items under plain launches skips the woven kernel from then on (pipe_skip_mask)."""
    from haconvdr_amd.encoder import ANCEEncoder
    _, sd = _scaled_qk_encoder(scale)
    return sd, referee(ANCEEncoder, sd)


def run(enc, ids, mask, device=False):
    """One forward: (embeddings, plan dict).  device: int64 CUDA tensors on the caller's stream (the serving call shape);
    otherwise the host entry point (int32, the encoder's own stream)."""
    if device:
        import torch
        out = enc(torch.from_numpy(np.asarray(ids, np.int64)).cuda(), torch.from_numpy(np.asarray(mask, np.int64)).cuda()).cpu().numpy()
    else:
        out = np.asarray(enc(np.asarray(ids, np.int32), np.asarray(mask, np.int32)))
    return out, _plan(enc)


def same_bits(out, ref, lens, what):
    """Bit equality of two [B, 768] outputs; a difference is reported by sequence, length and length class."""
    assert np.isfinite(out).all() and np.isfinite(ref).all(), (what, "not finite")
    ne = (bits(out) != bits(ref)).any(1)
    if ne.any():
        b = np.nonzero(ne)[0]
        lens = np.asarray(lens)
        raise AssertionError((what, "sequences that differ from the referee", b.tolist(), "their lengths", lens[b].tolist(),
                              "long class", int((lens[b] > 256).sum()), "short class", int((lens[b] <= 256).sum()),
                              "elements", int((bits(out) != bits(ref)).sum())))
    return out.size


def check_form(p, expect, what):
    """The plan's fields against the mirror: asserted on 256 CUs (where tests/test_graph_shapes.py pins the mirror), printed otherwise."""
    got = {k: p[k] for k in gs.PLAN_FIELDS}
    want = {k: expect[k] for k in gs.PLAN_FIELDS}
    if got != want or what[-1] == 0:           # (once per test, and whenever they differ)
        print(what, "form", got, "mirror", want, "att_qs", expect["att_qs"], "att_one", expect["att_one"], "Mc", expect["Mc"], "CUs", n_cu())
    if n_cu() == 256:
        assert got == want, (what, got, want)


def but(p, *drop):
    return {k: v for k, v in p.items() if k not in drop}


_REPLAYS = {}


def replays(name):
    """The four calls of a shape on the shared graph handle and on the referee, run once: a list of dicts (out, ref, plan,
    ref_plan, ids, mask, lens, seconds).  A failure is kept and raised again: nothing is run twice."""
    if name not in _REPLAYS:
        try:
            enc, ref_enc, _ = calm_pair()
            res = []
            for ids, mask, lens in gs.calls(name):
                t0 = time.time()
                out, p = run(enc, ids, mask, device=True)
                dt = time.time() - t0
                ref, rp = run(ref_enc, ids, mask, device=True)
                res.append({"out": out, "ref": ref, "plan": p, "ref_plan": rp, "ids": ids, "mask": mask, "lens": lens, "seconds": dt})
            _REPLAYS[name] = res
        except BaseException as e:          # noqa: B902  (kept for the tests that share this run)
            _REPLAYS[name] = e
    if isinstance(_REPLAYS[name], BaseException):
        raise _REPLAYS[name]
    return _REPLAYS[name]


# ------------------------------------------------------------------------------------------------------ a. replays on fresh data
@pytest.mark.parametrize("name", list(gs.SHAPES))
def test_replays_on_fresh_data_equal_plain_launches(name):
    B, L = gs.SHAPES[name]
    t0 = time.time()
    res = replays(name)
    expect = gs.form(B, L, n_cu())
    compared = 0
    for i, r in enumerate(res):
        print(name, "call", i, r["plan"], "packed rows", gs.packed_rows(r["lens"]), "of", gs.padded_rows(B, L),
              "long / short sequences", int((r["lens"] > 256).sum()), int((r["lens"] <= 256).sum()), "%.4f s" % r["seconds"])
    assert [r["plan"]["graph"] for r in res] == KINDS4, [r["plan"] for r in res]
    for i, r in enumerate(res):
        compared += same_bits(r["out"], r["ref"], r["lens"], (name, "call", i, r["plan"]))
        assert r["ref_plan"]["graph"] == "off" and r["ref_plan"]["attn_form"] == "single", r["ref_plan"]
        assert but(r["plan"], "graph", "attn_form") == but(r["ref_plan"], "graph", "attn_form"), (name, i, r["plan"], r["ref_plan"])
        check_form(r["plan"], expect, (name, "call", i))
    assert len({r["out"].tobytes() for r in res}) == len(res)          # (four different batches gave four different answers)
    if name == "g8_top":       # one sequence more: not eligible, plain launches
        from haconvdr_amd import synth
        enc, ref_enc, _ = calm_pair()
        ids, lens = synth.token_batch(0x6B33, 33, 512, min_len=1)
        mask = (np.arange(512)[None, :] < lens[:, None]).astype(np.int32)
        out, p = run(enc, ids, mask, device=True)
        ref, _ = run(ref_enc, ids, mask, device=True)
        print(name, "33 x 512:", p)
        assert p["graph"] == "off" and p["rows"] == str(gs.Mp(33, 512)) and not gs.graph_eligible(33, 512), p
        compared += same_bits(out, ref, lens, (name, "33 x 512", p))
    print(name, "elements compared", compared, "seconds", "%.2f" % (time.time() - t0))


# ------------------------------------------------------------------------------------------------------ b. against the oracle
@pytest.mark.parametrize("name", ["woven_c128", "g8_first", "g8_short64"])
def test_last_replay_against_the_fp32_oracle(name):
    from oracle import ance_oracle
    t0 = time.time()
    r = replays(name)[-1]
    assert r["plan"]["graph"] == "replay", r["plan"]
    pick = gs.pick_six(r["lens"])
    ref = ance_oracle.ance_forward(calm_pair()[2], r["ids"][pick], r["mask"][pick])
    m = parity.measure(r["out"][pick], ref)
    print(name, "sequences", pick, "lengths", r["lens"][pick].tolist(), {k: v for k, v in m.items() if k != "spread"}, m["spread"],
          "seconds", "%.2f" % (time.time() - t0))
    assert m["spread"]["raw_min"] >= parity.DEGENERATE_BELOW, m["spread"]
    parity.assert_embeddings_match(r["out"][pick], ref, what=name)
    parity.assert_negative_control(r["out"][pick], ref)


# ------------------------------------------------------------------------------------------------------ c. the fix-up pass in a replay
@pytest.mark.parametrize("name", ["woven_c128", "g8_first"])
@pytest.mark.parametrize("scale", [8.0, 3.0])
def test_fixup_pass_inside_a_replay(scale, name):
    """Q and K x 8: the woven kernel flags items, the captured fix-up launches take and clear the flags on every replay (the same
    count after the capturing call and after each further replay, the referee's bits); x 3: no item is flagged."""
    from haconvdr_amd import synth
    B, L = gs.SHAPES[name]
    t0 = time.time()
    from haconvdr_amd.encoder import ANCEEncoder
    sd, ref_enc = scaled_weights(scale)
    enc = ANCEEncoder.from_state_dict(sd)
    ids, lens = synth.token_batch(0x7C0 + B, B, L, fixed_len=L)
    mask = np.ones_like(ids)
    want, _ = run(ref_enc, ids, mask)
    expect = gs.form(B, L, n_cu())
    kinds, redo, compared = [], [], 0
    for call in range(4):
        out, p = run(enc, ids, mask)
        kinds.append(p["graph"])
        redo.append(enc.attention_redo())
        compared += same_bits(out, want, lens, (name, scale, "call", call, p))
        check_form(p, expect, (name, scale, "call", call))
    print(name, "scale", scale, kinds, "redo counts", redo, "elements compared", compared, "seconds", "%.2f" % (time.time() - t0))
    assert kinds == KINDS4, kinds
    if scale >= 8.0 and expect["attn_form"] == "woven":
        assert redo[0] > 0 and redo[1:] == redo[:1] * 3, redo      # the pass ran inside the graph, and left no flag behind
    else:
        assert redo == [0, 0, 0, 0], redo


# ------------------------------------------------------------------------------------------------------ d. other modes
def mode_calls(enc, ref_enc, batches, what, **form_kw):
    """Every batch through both handles (same mode, ref_enc with graph = off): bits, plan kinds eager-first then replay, the
    plans equal apart from graph=, the form the mirror expects.  Returns the plans."""
    t0 = time.time()
    plans, compared = [], 0
    for i, (ids, mask, lens) in enumerate(batches):
        out, p = run(enc, ids, mask)
        ref, rp = run(ref_enc, ids, mask)
        plans.append(p)
        compared += same_bits(out, ref, lens, (what, "call", i, p))
        assert rp["graph"] == "off" and but(p, "graph") == but(rp, "graph"), (what, i, p, rp)
        check_form(p, gs.form(ids.shape[0], ids.shape[1], n_cu(), **form_kw), (what, "call", i))
    print(what, [p["graph"] for p in plans], "elements compared", compared, "seconds", "%.2f" % (time.time() - t0))
    assert [p["graph"] for p in plans] == KINDS4[:len(plans)], plans
    return plans


def test_mean_pooling_at_the_first_gemm8_shape():
    """pooling = mean: the last layer runs on every row (gemm8, woven), then pool_mean_kernel -- no compact tail."""
    from haconvdr_amd.encoder import ANCEEncoder
    sd = state_dict(2, 0.08)
    enc, ref_enc = ANCEEncoder.from_state_dict(sd, pooling="mean"), ANCEEncoder.from_state_dict(sd, pooling="mean")
    ref_enc.set_option("graph", "off")
    plans = mode_calls(enc, ref_enc, gs.calls("g8_first", n=3, seed=0x6D00), "mean g8_first", pooling="mean")
    assert all(p.get("pool") == "mean" for p in plans), plans


def test_bert_handle_at_the_first_woven_shape():
    from haconvdr_amd.encoder import BERTEncoder
    sd = bert_ref.weights(2, 0.08)
    enc, ref_enc = BERTEncoder.from_state_dict(sd), BERTEncoder.from_state_dict(sd)
    ref_enc.set_option("graph", "off")
    B, L = gs.SHAPES["woven_c128"]
    batches = []
    for i, (_, _, lens) in enumerate(gs.calls("woven_c128", n=3, seed=0x6E00)):
        ids, mask = bert_ref.bert_case_inputs(0x6E00 + i, lens.tolist(), L)
        batches.append((ids, mask, lens))
    plans = mode_calls(enc, ref_enc, batches, "bert woven_c128")
    assert all(p.get("model") == "bert" for p in plans), plans


def test_split_precision_at_the_first_woven_shape():
    from haconvdr_amd.encoder import ANCEEncoder
    sd = state_dict(2, 0.08)
    enc, ref_enc = ANCEEncoder.from_state_dict(sd, precision="split"), ANCEEncoder.from_state_dict(sd, precision="split")
    ref_enc.set_option("graph", "off")
    plans = mode_calls(enc, ref_enc, gs.calls("woven_c128", n=3, seed=0x6F00), "split woven_c128", precision="split")
    assert all(p["attn_form"] == "split" and p["gemm"] == "split128" and p.get("precision") == "split" for p in plans), plans


def test_first_and_mean_alternating_on_one_handle_keep_their_own_graphs():
    from haconvdr_amd.encoder import ANCEEncoder
    t0 = time.time()
    sd = state_dict(2, 0.08)
    enc = ANCEEncoder.from_state_dict(sd)
    refs = {"first": calm_pair()[1], "mean": referee(ANCEEncoder, sd, pooling="mean")}
    seen, compared = [], 0
    batches = gs.calls("g8_first", n=3, seed=0x7000)
    try:
        for ids, mask, lens in batches:
            for mode in ("first", "mean"):
                enc.set_option("pooling", mode)
                out, p = run(enc, ids, mask)
                ref, rp = run(refs[mode], ids, mask)
                seen.append((mode, p["graph"], p.get("pool")))
                compared += same_bits(out, ref, lens, (mode, p))
                assert p.get("pool") == rp.get("pool") == ("mean" if mode == "mean" else None), (p, rp)
                check_form(p, gs.form(*gs.SHAPES["g8_first"], n_cu(), pooling=mode), ("alternating", mode))
    finally:
        enc.set_option("pooling", "first")
    print("alternating", seen, "elements compared", compared, "seconds", "%.2f" % (time.time() - t0))
    for mode in ("first", "mean"):
        assert [g for m, g, _ in seen if m == mode] == KINDS4[:3], seen     # each mode shows its own eager-first once


# ------------------------------------------------------------------------------------------------------ e. mask cleared by the capturing call
def test_capture_whose_call_clears_the_skip_mask_finds_ws_redo_sized():
    """Near one-hot attention (Q and K x 20).  A handle learns at 12 x 512, with graph = off, to skip the woven kernel; 60 more
    forwards later its 63rd run_forward is the eager-first call of 24 x 512 (still skipping: attn_form=single, nothing woven runs)
    and its 64th the capturing call -- the retry that clears the mask, so the captured forward is woven and needs ws_redo for 24
    sequences.  fwd_build sized it during the eager-first call; sized inside attention() it would be grown inside the capture."""
    import torch
    from haconvdr_amd import synth
    from haconvdr_amd.encoder import ANCEEncoder
    t0 = time.time()
    enc, sd = _scaled_qk_encoder(20.0)
    ref_enc = referee(ANCEEncoder, sd)
    cu = n_cu()
    reach = gs.woven(12, 512, cu) and gs.woven(24, 512, cu) and gs.graph_eligible(24, 512)
    ids12, _ = synth.token_batch(0x7E12, 12, 512, fixed_len=512)
    ids24, lens24 = synth.token_batch(0x7E24, 24, 512, fixed_len=512)
    enc.set_option("graph", "off")
    run(enc, ids12, np.ones_like(ids12))
    learn = (_plan(enc)["attn_form"], enc.attention_redo())
    torch.cuda.synchronize()                       # (the counts have arrived; a forward never waits for them)
    _, p = run(enc, ids12, np.ones_like(ids12))
    forwards, learnt = 2, p["attn_form"]
    while forwards < gs.REDO_RETRY - 2:            # one run_forward per call; two short of the retry
        _, p = run(enc, ids12, np.ones_like(ids12))
        forwards += 1
    filler = p["attn_form"]
    enc.set_option("graph", "auto")
    want, _ = run(ref_enc, ids24, np.ones_like(ids24))
    plans, compared = [], 0
    for call in range(3):
        out, p = run(enc, ids24, np.ones_like(ids24))
        plans.append(p)
        compared += same_bits(out, want, lens24, ("24 x 512 call", call, p))
    print("learning forward", learn, "second forward", learnt, "after", forwards, "forwards", filler, "| 24 x 512:",
          [(p["graph"], p["attn_form"]) for p in plans], "redo", enc.attention_redo(), "elements compared", compared, "CUs", cu,
          "seconds", "%.2f" % (time.time() - t0))
    assert [p["graph"] for p in plans] == KINDS4[:3], plans
    if reach:      # the test reached what it is for
        assert learn[0] == "woven" and learn[1] > 2 * 12 * 12 and learnt == "single" and filler == "single", (learn, learnt, filler)
        assert [p["attn_form"] for p in plans] == ["single", "woven", "woven"], plans


# ------------------------------------------------------------------------------------------------------ f. regrown workspaces
def test_a_larger_forward_between_replays_of_a_gemm8_shape():
    """48 x 512 (not eligible) regrows every workspace, gemm8's included: the captured launches hold the old pointers, so the next
    call of the shape captures again (reported as replay), with the referee's bits."""
    from haconvdr_amd import synth
    from haconvdr_amd.encoder import ANCEEncoder
    t0 = time.time()
    _, ref_enc, sd = calm_pair()
    enc = ANCEEncoder.from_state_dict(sd)
    expect = gs.form(*gs.SHAPES["g8_first"], n_cu())
    kinds, compared = [], 0
    for i, (ids, mask, lens) in enumerate(gs.calls("g8_first", seed=0x7100)):
        out, p = run(enc, ids, mask, device=True)
        ref, rp = run(ref_enc, ids, mask, device=True)
        kinds.append(p["graph"])
        compared += same_bits(out, ref, lens, ("g8_first call", i, p))
        assert but(p, "graph", "attn_form") == but(rp, "graph", "attn_form"), (p, rp)
        check_form(p, expect, ("regrow", "call", i))
        if i == 1:
            big, big_lens = synth.token_batch(0x7148, 48, 512, min_len=1)
            big_mask = (np.arange(512)[None, :] < big_lens[:, None]).astype(np.int32)
            out, p = run(enc, big, big_mask, device=True)
            ref, _ = run(ref_enc, big, big_mask, device=True)
            assert p["graph"] == "off" and p["rows"] == str(gs.Mp(48, 512)), p
            compared += same_bits(out, ref, big_lens, ("48 x 512", p))
    print("regrow", kinds, "elements compared", compared, "seconds", "%.2f" % (time.time() - t0))
    assert kinds == KINDS4, kinds
