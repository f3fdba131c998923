#!/usr/bin/env python3
"""What range_search costs: range_search_tensor against rank_ids_tensor at m = 1 (count_ahead_kernel streaming the same rows once
per tile of 16 queries: the yardstick) over 1M x 768 rows of bench.py's synthetic corpus, event-timed, warm, the variants
alternating inside every repetition; prints one JSON object.
  python tools/range_timing.py
Per query count (1, 16, 64): rank_ids at m = 1 of the row at position 100; range_search with the radius = that row's score
(100 results per query) at cap = 0 (range_emit_kernel and the offsets only) and at cap = 128 per query (scatter, sort and
results as well); at cap = 0 also with no hit at all (radius +Inf) and with 10 hits per query, beside rank_ids of the row at
position 10.  The documented slow case: one query, radius = -Inf, every row returned (segments on the merge path)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from haconvdr_amd.index import FlatIPIndex  # noqa: E402

D, CH = 768, 125_000


def gen_rows(seed, n, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn((n, D), generator=g, device=dev, dtype=torch.float32)
    return (x - x.mean(1, keepdim=True)) / x.std(1, unbiased=False, keepdim=True)


def main():
    dev = torch.device("cuda", 0)
    idx = FlatIPIndex(D, devices=(0,))
    idx.set_option("split", "0")
    idx.add_tensor(torch.cat([gen_rows(0xC0FFEE + c, CH, dev) for c in range(8)]))
    torch.cuda.synchronize()
    n = idx.ntotal
    q64 = gen_rows(0x9E, 64, dev)
    D64, I64 = idx.search_tensor(q64, 101)
    torch.cuda.synchronize()
    cases, checks = {}, {}
    for nq in (1, 16, 64):
        q = q64[:nq].contiguous()
        gold = I64[:nq, 100:101].contiguous()
        radius = D64[:nq, 100].contiguous()
        cases[f"rank{nq}_m1"] = lambda q=q, gold=gold: idx.rank_ids_tensor(q, gold)
        cases[f"range{nq}_cap0"] = lambda q=q, radius=radius: idx.range_search_tensor(q, radius, 0)
        # where the emit scan's time goes: no hit at all (the any-lane test alone), 10 hits per query
        nohit = torch.full((nq,), float("inf"), device=dev)
        r10 = D64[:nq, 10].contiguous()
        cases[f"range{nq}_cap0_nohit"] = lambda q=q, nohit=nohit: idx.range_search_tensor(q, nohit, 0)
        cases[f"range{nq}_cap0_10hits"] = lambda q=q, r10=r10: idx.range_search_tensor(q, r10, 0)
        cases[f"rank{nq}_m1_rank10"] = lambda q=q, g10=I64[:nq, 10:11].contiguous(): idx.rank_ids_tensor(q, g10)
        cases[f"range{nq}_cap128"] = lambda q=q, radius=radius, nq=nq: idx.range_search_tensor(q, radius, 128 * nq)
        lims, _, I = idx.range_search_tensor(q, radius, 128 * nq)
        torch.cuda.synchronize()
        total = int(lims[-1])
        checks[f"range{nq}_equals_search_head"] = bool(total == 100 * nq and torch.equal(I[:total].reshape(nq, 100), I64[:nq, :100]))
    q1 = q64[:1].contiguous()
    minus_inf = torch.full((1,), float("-inf"), device=dev)
    cases["range1_every_row"] = lambda: idx.range_search_tensor(q1, minus_inf, n)
    lims, Dall, _ = idx.range_search_tensor(q1, minus_inf, n)
    torch.cuda.synchronize()
    checks["range1_every_row_sorted"] = bool(int(lims[-1]) == n and bool((Dall[1:] <= Dall[:-1]).all()))
    reps = {k: (5 if k == "range1_every_row" else 15) for k in cases}
    times = {k: [] for k in cases}
    plans = {}
    for k, f in cases.items():          # warm-up of every shape
        f()
        plans[k] = idx.last_plan()
    torch.cuda.synchronize()
    for r in range(15):                 # alternating
        for k, f in cases.items():
            if r >= reps[k]:
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    idx.check_status()
    med = {k: float(np.median(v)) for k, v in times.items()}
    res = {"rows": n, "d": D, "checks": checks,
           "ms_median": {k: round(v, 4) for k, v in med.items()},
           "ms_min": {k: round(float(np.min(v)), 4) for k, v in times.items()},
           "ms_max": {k: round(float(np.max(v)), 4) for k, v in times.items()},
           "emit_over_count": {str(nq): round(med[f"range{nq}_cap0"] / med[f"rank{nq}_m1"], 4) for nq in (1, 16, 64)},
           "ms_behind_the_scan": {str(nq): round(med[f"range{nq}_cap128"] - med[f"range{nq}_cap0"], 4) for nq in (1, 16, 64)},
           "plans": plans}
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
