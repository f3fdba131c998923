"""Index lifetimes on the GPU: adds into every group, piece and segment edge with the fp16 image and the row-major copy
alive, a hostile first life behind the count of short later ones, the segment table full and fused, and two shards in one
process -- every checkpoint by every search route, bit for bit against oracle/flat_ip_oracle.c (tests/index_lifetime.py:
Life.check; the case tables and their planted winners are checked on the CPU by tests/test_index_lifetime.py).

Every checkpoint asserts the plan text of its route, the rows read back as words and the scores of the returned ids.
Options are switched on the live handle; there are no tolerances and no timings."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import index_lifetime as il
from tests.index_lifetime import ALL5, FMAX, Life

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 10


def _handle(d=768, devices=(0,), **options):
    from haconvdr_amd.index import FlatIPIndex
    idx = FlatIPIndex(d, devices=devices)
    for name, value in options.items():
        idx.set_option(name, value)
    return idx


def _add(idx, life, x):
    idx.add(x)
    life.add(x)
    assert idx.ntotal == len(life.rows)


# ---------------------------------------------------------------------------------------------------------------------
# A. adds into every edge with image and copy alive: 8 checkpoints x 5 routes per variant
@pytest.mark.parametrize("variant", ["copy", "tiles", "eager"])
def test_adds_into_every_edge_with_image_and_copy_alive(variant, oracle):
    x, q, where, pieces = il.case_a()
    rescore = "tiles" if variant == "tiles" else "rows"
    options = {"split": "1", "rescore_rows": "0" if variant == "tiles" else "1"}
    if variant == "eager":
        options["fp16_image"] = "eager"                    # before the first add: add() writes the image of every new segment
    idx, life = _handle(**options), Life(q, where)
    lo = 0
    for n_add, m in enumerate(pieces):
        _add(idx, life, x[lo:lo + m])
        lo += m
        if variant == "eager" and n_add == 0:
            # the handle's FIRST search is a prefilter search, over the image add() wrote; same bits as a lazy handle's
            plan, D, I = life.check(idx, oracle, "pre1", K, rescore)
            lazy = _handle(split="1", rescore_rows="1")
            lazy.add(life.rows)
            plan0, D0, I0 = life.check(lazy, oracle, "pre1", K, rescore)
            np.testing.assert_array_equal(I, I0)
            np.testing.assert_array_equal(il.bits(D), il.bits(D0))
            del lazy
        for route in ALL5:
            life.check(idx, oracle, route, K, rescore)
    assert idx.ntotal == 4480


# ---------------------------------------------------------------------------------------------------------------------
# B. a hostile first life behind the count (in a child process: see the test)
def scenario_b(n2):
    from oracle import oracle
    oracle.lib()
    x1, x2, x3, q, where = il.case_b(n2)
    options = {"split": "1", "rescore_rows": "1"}
    idx, life = _handle(**options), Life(q, where)
    _add(idx, life, x1)                                    # life 1: NaN, +-Inf, 3.3e38 and norm-7e4 rows at [n2, n2 + 200)
    for route in ALL5:
        plan, D, I = life.check(idx, oracle, route, K, "rows")
        assert not np.isnan(D).any() and (I >= 0).all()    # NaN rows are never returned
    idx.reset(), life.reset()
    assert idx.ntotal == 0 and idx.reconstruct_n().shape == (0, 768)
    _add(idx, life, x2)                                    # life 2: the hostile rows sit behind the count, in tiles, image and copy
    plans = {}
    for route in ALL5:
        plans[route], D, I = life.check(idx, oracle, route, K, "rows")
    # norm2_max of life 1 (Inf / NaN) must be gone: it scales the prefilter's error bound, so a stale one changes no result
    # bit, only sends every query to the exact kernels.  What a fresh handle certifies, the recycled one certifies.
    fresh = _handle(**options)
    fresh.add(x2)
    plan_fresh, _, _ = life.check(fresh, oracle, "pre1", K, "rows")
    plan_again, _, _ = life.check(idx, oracle, "pre1", K, "rows")
    f_fresh, f_recycled, f_first = il.fallback_of(plan_fresh), il.fallback_of(plan_again), il.fallback_of(plans["pre1"])
    print(f"B n2={n2} fallback fresh={f_fresh[0]}/{f_fresh[1]} recycled={f_recycled[0]}/{f_recycled[1]} first={f_first[0]}/{f_first[1]}")
    assert f_fresh == (0, il.NQ), plan_fresh
    assert f_recycled == (0, il.NQ) and f_first == (0, il.NQ), (plan_again, plans["pre1"])
    idx.reset(), life.reset()
    _add(idx, life, x3)                                    # life 3: 70 rows < SPLIT_K2: split = "1" takes the exact kernels
    for route in ("few_rows16", "few_rowsq"):
        plan, D, I = life.check(idx, oracle, route, 100)
        assert not plan.startswith("split:")
        assert (I[:, 70:] == -1).all() and (D[:, 70:] == -FMAX).all() and (I[:, :70] >= 0).all()
    print("B_DONE", n2)


@pytest.mark.parametrize("n2", il.B_N2)
def test_hostile_first_life_stays_behind_the_count(n2):
    """Life 1 leaves NaN, +-Inf, 3.3e38 and fp16-overflowing rows at [n2, n2 + 200); after reset() life 2 has n2 rows, so the
    stale rows fill the padding of its tail group and the groups behind it.  The inputs are legal; the one defect the
    history records in this state was a kernel that never ended, hence a child process with a time limit, as
    test_device_decided_fallback_ignores_stale_rows_behind_the_count has."""
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_index_lifetime_gpu import scenario_b; scenario_b({n2})"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert f"B_DONE {n2}" in r.stdout and f"fresh=0/{il.NQ} recycled=0/{il.NQ}" in r.stdout, r.stdout


# ---------------------------------------------------------------------------------------------------------------------
# C. the segment table, full and fused
def test_segment_table_full_then_fused_with_image_and_copy_alive(oracle):
    x, q, where, pieces = il.case_c()
    idx, life = _handle(split="1", rescore_rows="1"), Life(q, where)
    lo = 0
    for n_add, m in enumerate(pieces):
        _add(idx, life, x[lo:lo + m])
        lo += m
        # 10 segments (images and copies alive on all of them from here on), exactly MAX_SEG = 64, the add that fuses them
        # (consolidate drops image and copy: the next prefilter search rebuilds both), and the three 100-row adds behind it
        if n_add + 1 in il.C_CHECKPOINTS or n_add + 1 == len(pieces):
            for route in ALL5:
                plan, D, I = life.check(idx, oracle, route, K, "rows")
    assert idx.ntotal == 8620


def test_segment_table_full_exact_kernels_at_d96(oracle):
    x, q, where, pieces = il.case_c(96)
    idx, life = _handle(d=96, split="0"), Life(q, where, split="0")
    for s in range(64):
        _add(idx, life, x[128 * s:128 * (s + 1)])
    for route in ("scan16", "scan16_many"):                # K4 % 16 != 0: scan16_kernel at every query count
        life.check(idx, oracle, route, K)
    life.check(idx, oracle, "scan16_many", 100)


# ---------------------------------------------------------------------------------------------------------------------
# D. two shards in one process
def test_two_shards_rebuild_their_spans_after_reset(oracle):
    idx = _handle(devices=(0, 0), split="1")
    life = None
    for n_life, pieces in enumerate(il.D_LIVES):
        x, q, where, _ = il.case_d(n_life)
        if life is None:
            life = Life(q, where)
        else:
            idx.reset()
            life.reset(q, where)
            assert idx.ntotal == 0
        lo = 0
        for m in pieces:
            _add(idx, life, x[lo:lo + m])
            lo += m
        for route in ("scan16", "scanq", "pre1"):          # (search_tensor has no multi-device form)
            life.check(idx, oracle, route, K)
