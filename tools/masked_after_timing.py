#!/usr/bin/env python3
"""What a page of search_masked behind a cursor costs: search_masked_keys_tensor(after_keys=) against search_masked_keys_tensor
of the same mask and k (scan16_masked_kernel over the same group lists: the yardstick) over 1M x 768 rows of bench.py's
synthetic corpus, event-timed, warm, the variants alternating inside every repetition; prints one JSON object.
  python tools/masked_after_timing.py
Per query count (1, 16) and mask density (1: every row, 1/64: a random row in 64), k = 100: search_masked; one page at the start
cursor (all-ones keys), one behind the entry at rank 1000 and one behind the entry at rank 100 000 of the query's unmasked
ranking (entry_keys_at_tensor: the cursor row need not be selected).  Medians of 15; the yardstick's median is taken five times
over, and the spread of those five is what a difference has to exceed to mean anything."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from haconvdr_amd.index import FlatIPIndex, pack_mask  # noqa: E402

D, CH, K = 768, 125_000, 100
DEPTHS = (1000, 100_000)


def gen_rows(seed, n, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn((n, D), generator=g, device=dev, dtype=torch.float32)
    return (x - x.mean(1, keepdim=True)) / x.std(1, unbiased=False, keepdim=True)


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    dev = torch.device("cuda", 0)
    idx = FlatIPIndex(D, devices=(0,))
    idx.set_option("split", "0")
    idx.add_tensor(torch.cat([gen_rows(0xC0FFEE + c, CH, dev) for c in range(8)]))
    torch.cuda.synchronize()
    n = idx.ntotal
    q16 = gen_rows(0x9E, 16, dev)
    g = torch.Generator(device=dev).manual_seed(0x3A5C)
    masks = {"1": pack_mask(torch.ones(n, dtype=torch.bool, device=dev)).reshape(1, -1),
             "1/64": pack_mask(torch.rand(n, generator=g, device=dev) < 1.0 / 64).reshape(1, -1)}
    cases, checks, yard = {}, {}, []
    for nq in (1, 16):
        q = q16[:nq].contiguous()
        start = torch.full((nq,), -1, dtype=torch.int64, device=dev)
        cursors = {d: idx.entry_keys_at_tensor(q, torch.full((nq, 1), d, dtype=torch.int64, device=dev))[:, 0].contiguous() for d in DEPTHS}
        for name, m in masks.items():
            tag = f"nq{nq}_density{name}"
            cases[f"{tag}_masked"] = lambda q=q, m=m: idx.search_masked_keys_tensor(q, K, m)
            yard.append(f"{tag}_masked")
            cases[f"{tag}_page_start"] = lambda q=q, m=m, c=start: idx.search_masked_keys_tensor(q, K, m, after_keys=c)
            for d in DEPTHS:
                cases[f"{tag}_page_depth{d}"] = lambda q=q, m=m, c=cursors[d]: idx.search_masked_keys_tensor(q, K, m, after_keys=c)
            a, b = cases[f"{tag}_masked"](), cases[f"{tag}_page_start"]()
            deep = cases[f"{tag}_page_depth{DEPTHS[0]}"]()
            torch.cuda.synchronize()
            checks[f"{tag}_start_equals_masked"] = bool(torch.equal(a, b))
            # keys are uint64 viewed as int64: flipping the top bit turns the unsigned order into the signed one
            top = torch.iinfo(torch.int64).min
            below = ((deep ^ top) < (cursors[DEPTHS[0]] ^ top)[:, None]) | (deep == 0)
            checks[f"{tag}_page_lies_behind_its_cursor"] = bool(below.all())
    plans = {}
    for k, f in cases.items():          # warm-up of every shape
        f()
        plans[k] = idx.last_plan()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(15):                 # alternating
        for k, f in cases.items():
            times[k].append(timed(f))
    # the run-to-run spread of the yardstick: its median of 15, five times over
    spread = {}
    for k in yard:
        meds = [float(np.median([timed(cases[k]) for _ in range(15)])) for _ in range(5)]
        spread[k] = {"medians": [round(v, 4) for v in meds], "spread_ms": round(max(meds) - min(meds), 4)}
    idx.check_status()
    med = {k: float(np.median(v)) for k, v in times.items()}
    res = {"rows": n, "d": D, "k": K, "checks": checks,
           "ms_median": {k: round(v, 4) for k, v in med.items()},
           "ms_min": {k: round(float(np.min(v)), 4) for k, v in times.items()},
           "ms_max": {k: round(float(np.max(v)), 4) for k, v in times.items()},
           "yardstick_spread": spread,
           "page_start_minus_masked_ms": {k[:-len("_masked")]: round(med[k[:-len("_masked")] + "_page_start"] - med[k], 4) for k in yard},
           "plans": plans}
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
