"""The attention kernels per query row and head against an fp64 softmax, through the probe layer of tests/attn_probe.py.

layer_state(ids, mask, 0) of a probe checkpoint is the attention context itself, head by head (features 64h .. 64h+63 of row t,
times the row's rstd), so one key too few or too many, a neighbour's row, a stale rescale or another head's V shows in the
slice where it happens instead of being averaged over ~2000 rows x 768 features behind an out-projection and a residual.
The reference (oracle.ance_oracle.ance_attention, then attn_probe.closed_form) is teacher-forced from the kernels' own
embedding state, which no attention route changes, and computed once per (probe, family, attention model, batch).

Routes of the bf16 families (every one asserts its plan): single (attention_stream_kernel<16|8>), woven
(attention_pipe_kernel<8|4> and the fix-up pass: attention_redo() == 0 on flat, > 0 on peaked), auto (the long batch
goes woven, the short one single), the query split pinned to 2, 4, 8 and 16 parts (one launch for the long class; a part is
a run of 512 / parts query rows, 256 / min(parts, 8) in the short class: the 512- and 256-row sequences have rows on both
sides of every boundary, the other lengths end inside a part or leave whole parts empty), twopass (attention_kernel,
against the reference with the exact row maximum), and precision = split (attention_split_kernel, against the unrounded
reference as tests/split_parity.py does).  All streaming routes must return the same bits.  The plan string has no field for
the query split: of a pinned split only attn_form=single can be asserted (encoder.hip attention(): a pin takes the woven form
away and, when L > 256, makes one launch), which the single route gives too -- were attn_qs_pin ignored, these routes would
still pass, being the same bits.  Both batches run in both families (gemm = 8phase pins gemm8 whatever the row count; the short batch's 2339
packed rows are nine whole 256-row tiles and a partial one).

Bounds, each 2 x the worst measured on MI355X over the routes and batches of the cell, against the fp64 reference:
BOUNDS[(probe, family, model)] on the maximum of the figure over (b, t, h) -- a defect in single slices -- and
BODY[(probe, family, model)] on its 90th and 99th percentile -- a defect in every slice, far below the few outliers that set
the maximum.  test_bounds_reject_local_mutations checks that they still reject each local mutation of the reference in
fixed slices.
"""
import numpy as np
import pytest

from tests import attn_probe as ap

pytestmark = pytest.mark.gpu

GEMM = {"classic": "classic", "gemm8": "8phase"}
PROBES = ("flat", "mid", "peaked")
DEFAULTS = {"gemm": "auto", "attn": "stream", "attn_pipe": "auto", "attn_qsplit": "auto", "attn_qs_pin": "0"}
STREAM_ROUTES = {   # option sets (ANCEEncoder.set_option); every one ends at its default again
    "single": {"attn_pipe": "off", "attn_qsplit": "off"},
    "woven": {"attn_pipe": "all", "attn_qsplit": "off"},
    "auto": {},
    "qs2": {"attn_qs_pin": "2"}, "qs4": {"attn_qs_pin": "4"}, "qs8": {"attn_qs_pin": "8"}, "qs16": {"attn_qs_pin": "16"},
}
TWOPASS = {"attn": "twopass"}
# Measured on MI355X: the worst figure (max over every valid (sequence, row, head)) per cell, short / long batch.  The streaming
# routes are one number (same bits, asserted).  BOUNDS = 2 x the larger of the two.
#            stream   classic             gemm8               twopass  classic             gemm8               split
#   flat     5.0e-3 / 7.6e-3     6.0e-3 / 1.6e-2              4.9e-3 / 5.3e-3     6.7e-3 / 1.3e-2     1.8e-5 / 2.2e-5
#   mid      7.5e-3 / 1.02e-2    7.8e-3 / 9.5e-3              5.8e-3 / 9.3e-3     8.2e-3 / 8.6e-3     1.3e-4 / 1.5e-4
#   peaked   2.6e-2 / 2.8e-2     2.3e-2 / 3.5e-2              2.7e-2 / 2.8e-2     2.4e-2 / 3.2e-2     6.2e-4 / 5.7e-4
# The body of the distribution, (50th, 90th, 99th percentile) of the figure over the valid slices, long batch (the short one is
# at or below it except where noted; BODY = 2 x the larger 90th and 99th):
#            stream   classic                     gemm8                     twopass  classic                     gemm8
#   flat     2.8e-6  3.1e-5  9.4e-4      0  0       2.2e-3                  3.1e-6  3.7e-5  1.06e-3     0  1.2e-6  2.5e-3
#   mid      4.0e-7  2.4e-5  1.03e-3     0  4.1e-5  1.7e-3                  4.9e-7  2.7e-5  1.11e-3     0  6.7e-5  1.7e-3
#   peaked   1.2e-7  1.6e-5  8.2e-4      0  6.2e-6  1.7e-3                  1.2e-7  1.2e-5  6.8e-4      0  9.5e-7  1.2e-3
#   split    flat 7.8e-6  1.03e-5  1.28e-5    mid 1.6e-5  2.9e-5  4.7e-5 (short: 99th 4.7e-5, long 4.5e-5)    peaked 8.7e-6  7.7e-5  2.0e-4
# (gemm8's rows are bf16: a figure of 0 is the reference's bits.  flat gemm8 stream: 0 at the 90th percentile of both batches.)
# What the floor is made of: the few slices far above the 99th percentile sit at the same (length, row, head) in the streaming
# and the two-pass kernel of a family (they read the same Q, K, V).  Sixteen were looked at, the four worst of four cells.  Nine are
# single bf16 flips of one Q element in front of attention -- the kernels' QKV GEMM accumulates in fp32, the reference in fp64,
# and a value next to a bf16 rounding boundary lands on the other side: moving that one Q element of the reference by one bf16
# ulp brings the kernel's slice to <= 1.5e-4, seven of them to <= 2e-7 (peaked classic long (257, 220, 9) 2.8e-2 -> 1.4e-7,
# (416, 344, 7) 2.7e-2 -> 1.1e-7, (511, 303, 1) 1.7e-2 -> 1.7e-7; peaked gemm8 long (480, 113, 5) 3.5e-2 -> 0, (383, 144, 6)
# 2.1e-2 -> 0; flat gemm8 long (480, 416, 9) 1.6e-2 -> 0, (511, 480, 3) 1.1e-2 -> 0).  The other seven come down only part of
# the way with one Q element (peaked classic short (97, 70, 8) 2.6e-2 -> 9.7e-3; long (385, 192, 5) 2.0e-2 -> 2.2e-3): more than
# one flip, or one in K or V.  This was measured once and is not asserted; what is asserted is that slices above the
# 99th-percentile bound are fewer than one in a hundred (BODY).  An ulp of one Q element moves a peaked row's logits by ~0.01
# bit per key, hence the higher maxima there.
BOUNDS = {
    ("flat", "classic", "stream"): 1.5e-2, ("flat", "gemm8", "stream"): 3.2e-2, ("flat", "classic", "twopass"): 1.1e-2, ("flat", "gemm8", "twopass"): 2.7e-2,
    ("mid", "classic", "stream"): 2.0e-2, ("mid", "gemm8", "stream"): 1.9e-2, ("mid", "classic", "twopass"): 1.9e-2, ("mid", "gemm8", "twopass"): 1.7e-2,
    ("peaked", "classic", "stream"): 5.5e-2, ("peaked", "gemm8", "stream"): 7.0e-2, ("peaked", "classic", "twopass"): 5.6e-2, ("peaked", "gemm8", "twopass"): 6.4e-2,
    ("flat", "split", "twopass"): 4.3e-5, ("mid", "split", "twopass"): 3.1e-4, ("peaked", "split", "twopass"): 1.2e-3,
}
BODY = {   # (90th, 99th percentile)
    ("flat", "classic", "stream"): (6.3e-5, 1.9e-3), ("flat", "gemm8", "stream"): (0.0, 4.5e-3),
    ("flat", "classic", "twopass"): (7.5e-5, 2.1e-3), ("flat", "gemm8", "twopass"): (2.4e-6, 5.0e-3),
    ("mid", "classic", "stream"): (4.8e-5, 2.1e-3), ("mid", "gemm8", "stream"): (8.2e-5, 3.5e-3),
    ("mid", "classic", "twopass"): (5.4e-5, 2.2e-3), ("mid", "gemm8", "twopass"): (1.3e-4, 3.5e-3),
    ("peaked", "classic", "stream"): (3.2e-5, 1.6e-3), ("peaked", "gemm8", "stream"): (1.2e-5, 3.4e-3),
    ("peaked", "classic", "twopass"): (2.3e-5, 1.4e-3), ("peaked", "gemm8", "twopass"): (1.9e-6, 2.3e-3),
    ("flat", "split", "twopass"): (2.1e-5, 2.6e-5), ("mid", "split", "twopass"): (5.7e-5, 9.4e-5), ("peaked", "split", "twopass"): (1.5e-4, 4.0e-4),
}
SEPARATION = 3.0
_ENC, _STATE, _REF, _QKV = {}, {}, {}, {}


def encoder(probe, family):
    """One handle per (probe, weights variant, precision): family "split" is the classic weights in precision = split."""
    from haconvdr_amd.encoder import ANCEEncoder
    key = (probe, family)
    if key not in _ENC:
        kw = {"precision": "split"} if family == "split" else {}
        _ENC[key] = ANCEEncoder.from_state_dict(ap.probe_weights(probe, family), **kw)
    return _ENC[key]


def plan_of(enc):
    return dict(kv.split("=") for kv in enc.last_plan().split())


def kernel_rows(probe, family, batch_name, options):
    """(layer 0's rows, plan, attention_redo) of one route; the embedding state of the cell is read once (_STATE)."""
    enc = encoder(probe, family)
    ids, mask = ap.batch(*ap.BATCHES[batch_name])
    opts = dict(options, **({} if family == "split" else {"gemm": GEMM[family]}))
    for k, v in opts.items():
        enc.set_option(k, v)
    try:
        if (probe, family, batch_name) not in _STATE:
            _STATE[(probe, family, batch_name)] = enc.layer_state(ids, mask, -1)
        rows = enc.layer_state(ids, mask, 0, normalized=False)["rows"]
        plan = plan_of(enc)
        redo = enc.attention_redo()
    finally:
        for k in opts:
            enc.set_option(k, DEFAULTS[k])
    if family == "split":
        assert plan["gemm"] == "split128" and plan["attn_form"] == "split", plan
    else:
        assert plan["gemm"] == "gemm8" if family == "gemm8" else plan["gemm"].startswith("classic"), plan
    return rows, plan, redo


def qkv(probe, family, batch_name):
    """ance_qkv of the cell on the kernels' embedding state (one cell kept: 3 x [B, L, 768] float64)."""
    from oracle import ance_oracle
    key = (probe, family, batch_name)
    if key not in _QKV:
        _QKV.clear()
        fam = None if family == "split" else family
        _QKV[key] = ance_oracle.ance_qkv(ap.probe_weights(probe, family), 0, _STATE[key], fam)
    return _QKV[key]


def reference(probe, family, model, batch_name):
    """(rows_ref, den) of the cell, computed once; the kernels' embedding state must have been read (kernel_rows)."""
    key = (probe, family, model, batch_name)
    if key not in _REF:
        _, mask = ap.batch(*ap.BATCHES[batch_name])
        fam = None if family == "split" else family
        _REF[key] = ap.reference(ap.probe_weights(probe, family), _STATE[key[:2] + key[3:]], mask, fam, model,
                                 qkv=qkv(probe, family, batch_name))
    return _REF[key]


def route_figure(probe, family, model, batch_name, options):
    """(e [B, L, 12], rows, plan, redo) of one route against the cell's reference."""
    rows, plan, redo = kernel_rows(probe, family, batch_name, options)
    return ap.figure(rows, reference(probe, family, model, batch_name)), rows, plan, redo


def body(e, batch_name):
    """(median, 90th, 99th percentile) of the figure over the valid (sequence, row, head) slices."""
    _, mask = ap.batch(*ap.BATCHES[batch_name])
    return np.quantile(e[np.asarray(mask, bool)], (0.5, 0.9, 0.99))


def check(e, probe, family, model, batch_name, route):
    lens = ap.BATCHES[batch_name][0]
    q = body(e, batch_name)
    print(f"MEASURED {probe} {family} {model} {batch_name} {route} p50 {q[0]:.3e} p90 {q[1]:.3e} p99 {q[2]:.3e} max {e.max():.3e} worst {ap.worst(e, lens, 3)}")
    ap.assert_within(e, BOUNDS[(probe, family, model)], lens, (probe, family, model, batch_name, route))
    b90, b99 = BODY[(probe, family, model)]
    assert q[1] <= b90 and q[2] <= b99, ((probe, family, model, batch_name, route), "90th, 99th percentile", q[1:].tolist(), "bounds", (b90, b99))


CELLS = [(p, f, b) for p in PROBES for f in GEMM for b in ap.BATCHES]


@pytest.mark.parametrize("probe,family,batch_name", CELLS, ids=["-".join(c) for c in CELLS])
def test_streaming_routes_per_row_and_head(probe, family, batch_name):
    """single, woven, auto and the pinned query splits: each within the bound in every (row, head), all the same bits."""
    long = batch_name == "long"
    first = None
    for route, options in STREAM_ROUTES.items():
        e, rows, plan, redo = route_figure(probe, family, "stream", batch_name, options)
        assert plan["attn"] == "stream", (route, plan)
        if route == "woven":
            assert plan["attn_form"] == "woven", plan
            assert probe == "mid" or ((redo > 0) if probe == "peaked" else (redo == 0)), (probe, redo)
        elif route == "auto":
            assert plan["attn_form"] == ("woven" if long else "single"), plan
        else:   # (a pinned query split: whole items never reach the woven kernel; one launch when L > 256, encoder.hip attention())
            assert plan["attn_form"] == "single", (route, plan)
        if first is None:
            first = rows
            check(e, probe, family, "stream", batch_name, route)
        else:
            diff = np.argwhere((rows != first).any(-1))
            assert diff.size == 0, (probe, family, batch_name, route, "rows differ from route single at (sequence, row)", diff[:10].tolist())


@pytest.mark.parametrize("probe,family,batch_name", CELLS, ids=["-".join(c) for c in CELLS])
def test_twopass_per_row_and_head(probe, family, batch_name):
    e, _, plan, _ = route_figure(probe, family, "twopass", batch_name, TWOPASS)
    assert plan["attn"] == "twopass" and plan["attn_form"] == "twopass", plan
    check(e, probe, family, "twopass", batch_name, "twopass")


SPLIT_CELLS = [(p, b) for p in PROBES for b in ap.BATCHES]


@pytest.mark.parametrize("probe,batch_name", SPLIT_CELLS, ids=["-".join(c) for c in SPLIT_CELLS])
def test_split_precision_per_row_and_head(probe, batch_name):
    """attention_split_kernel against the unrounded reference (family None)."""
    e, _, _, _ = route_figure(probe, "split", "twopass", batch_name, {})
    check(e, probe, "split", "twopass", batch_name, "split")


# the local mutations (oracle.ance_oracle.ATTN_MUTATIONS) per probe, and where they are applied: first, middle and last row x
# heads 0, 5, 11 of one sequence per length ("block_stale": of the rows of those heads whose softmax reference moves)
MUTATIONS = {"flat": ("key_minus", "key_next", "head_next"), "mid": ("logits",), "peaked": ("top_key", "block_stale")}
MUTATION_LENS = {"short": [33, 65, 129, 256], "long": [257, 385, 512]}
HEADS = (0, 5, 11)
# Measured separations, min over the mutated slices of figure(mutated reference) / BOUNDS, short / long batch:
#   flat    classic  key_minus 12 / 17   key_next 21 / 16   head_next 82 / 74        gemm8  5.8 / 8.1   8.7 / 7.5   38 / 35
#   peaked  classic  top_key 17 / 16     block_stale 17 / 15                         gemm8  14 / 12     13 / 12
#   mid     classic  logits 0.25 / 0.30                                              gemm8  0.30 / 0.32
# and against BODY's 90th percentile every one is >= 69 (logits on mid: 106 / 124 classic, 69 / 75 gemm8; flat gemm8, whose
# bound is 0: every mutated slice differs).  logits x 1.01 on mid (logits of sigma ~4 bits) moves every slice by 5e-3 .. 2.7e-2:
# under the maximum that the few flip outliers set, but above what 99 slices in 100 show.  NOT_SEPARABLE lists it with the
# smallest ratio, over the mutated slices, to BODY's 99th percentile per batch; asserted: that ratio is what is recorded (to
# 10 %) and > 1.
NOT_SEPARABLE = {("mid", "classic", "logits"): {"short": 2.42, "long": 2.84}, ("mid", "gemm8", "logits"): {"short": 1.62, "long": 1.75}}
assert not any(k[:2] == ("flat", "classic") for k in NOT_SEPARABLE) and all(v > 1.0 for r in NOT_SEPARABLE.values() for v in r.values())


def mutation_slices(probe, family, batch_name, mutation):
    from oracle import ance_oracle
    lens = ap.BATCHES[batch_name][0]
    if mutation != "block_stale":
        return ap.slices(lens, MUTATION_LENS[batch_name], HEADS)
    _, mask = ap.batch(*ap.BATCHES[batch_name])
    moves = ance_oracle.attention_moves(qkv(probe, family, batch_name), mask).numpy()
    out = set()
    for n in MUTATION_LENS[batch_name]:
        b = lens.index(n)
        for h in HEADS:
            t = np.flatnonzero(moves[b, :n, h])
            out |= {(b, int(t[i]), h) for i in ((0, len(t) // 2, len(t) - 1) if len(t) else ())}
    return out


@pytest.mark.parametrize("probe,family,batch_name", CELLS, ids=["-".join(c) for c in CELLS])
def test_bounds_reject_local_mutations(probe, family, batch_name):
    """The self-check of the bounds: each mutation, applied to the reference in a fixed set of slices, lands in every one of them
    >= 3 x beyond BOUNDS (a single wrong slice fails the maximum) and >= 3 x beyond BODY's 90th percentile (the same defect in
    every slice puts nine slices in ten, hence that percentile, there), where the kernel itself stays inside BOUNDS.  The
    exceptions to the first are NOT_SEPARABLE, whose recorded ratio to BODY's 99th percentile must hold and stay > 1."""
    _, mask = ap.batch(*ap.BATCHES[batch_name])
    lens = ap.BATCHES[batch_name][0]
    e, _, _, _ = route_figure(probe, family, "stream", batch_name, {})
    base = reference(probe, family, "stream", batch_name)
    bound = BOUNDS[(probe, family, "stream")]
    b90, b99 = BODY[(probe, family, "stream")]
    for m in MUTATIONS[probe]:
        where = sorted(mutation_slices(probe, family, batch_name, m))
        assert where, (probe, family, batch_name, m, "no slice to mutate")
        idx = tuple(np.array(where).T)
        mut, _ = ap.reference(ap.probe_weights(probe, family), _STATE[(probe, family, batch_name)], mask, family, "stream", mutate=m,
                              where=set(where), qkv=qkv(probe, family, batch_name))
        f = ap.figure(mut, base)[idx]
        sep = f / bound
        print(f"SEPARATION {probe} {family} {batch_name} {m} slices {len(where)} figure min {f.min():.3e} median {np.median(f):.3e} max {f.max():.3e}"
              f" kernel max {e[idx].max():.3e}")
        assert e[idx].max() <= bound, (m, "kernel beyond the bound in the mutated slices", ap.worst(e, lens))
        weakest = [(float(f"{v:.3e}"), lens[b], t, h) for v, (b, t, h) in sorted(zip(f.tolist(), where))[:5]]
        assert f.min() > 0 and f.min() >= SEPARATION * b90, (probe, family, batch_name, m, "90th percentile bound", b90, "weakest (figure, length, row, head)", weakest)
        if (probe, family, m) in NOT_SEPARABLE:
            recorded, ratio = NOT_SEPARABLE[(probe, family, m)][batch_name], f.min() / b99
            assert ratio > 1.0 and abs(ratio / recorded - 1.0) <= 0.1, (probe, family, batch_name, m, "ratio", ratio, "recorded", recorded, weakest)
        else:
            assert sep.min() >= SEPARATION, (probe, family, batch_name, m, "bound", bound, "weakest (figure, length, row, head)", weakest)
