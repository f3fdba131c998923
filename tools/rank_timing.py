#!/usr/bin/env python3
"""What rank_ids costs: rank_ids_tensor against the exact scan (search_tensor, split = "0", 16 queries, k = 100) over 1M x 768 rows
of bench.py's synthetic corpus, event-timed, warm, the variants alternating inside every repetition; prints one JSON object.
  python tools/rank_timing.py
Variants: 16 queries at m = 1 and at m = MT + 1 (two chunks), 1000 queries at m = 1; each with ids that rank high (a search's
own results: the group skip of count_ahead_kernel's epilogue is the common case) and with random rows (mid-corpus ranks: most
groups take the counting path)."""
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
    q1000 = gen_rows(0x9E, 1000, dev)
    q16 = q1000[:16].contiguous()
    D16, I16 = idx.search_tensor(q16, 100)
    plan_search = idx.last_plan()
    torch.cuda.synchronize()
    ok = bool(torch.equal(idx.rank_ids_tensor(q16, I16), torch.arange(100, device=dev).repeat(16, 1)))
    plan_rank = idx.last_plan()
    MT = int(plan_rank.split("MT=")[1].split(">")[0])
    _, I1000 = idx.search_tensor(q1000, 100)
    g = torch.Generator(device=dev).manual_seed(5)
    rnd = torch.randint(0, n, (1000, MT + 1), generator=g, device=dev)
    cases = {
        "search16_k100_scan16": lambda: idx.search_tensor(q16, 100),
        "rank16_m1_gold_rank10": lambda: idx.rank_ids_tensor(q16, I16[:, 10:11].contiguous()),
        "rank16_m1_random_row": lambda: idx.rank_ids_tensor(q16, rnd[:16, :1].contiguous()),
        "rank16_mMT+1_gold_ranks_0_99": lambda: idx.rank_ids_tensor(q16, I16[:, ::11][:, :MT + 1].contiguous()),
        "rank16_mMT+1_random_rows": lambda: idx.rank_ids_tensor(q16, rnd[:16].contiguous()),
        "rank1000_m1_gold_rank10": lambda: idx.rank_ids_tensor(q1000, I1000[:, 10:11].contiguous()),
        "rank1000_m1_random_row": lambda: idx.rank_ids_tensor(q1000, rnd[:, :1].contiguous()),
    }
    reps = {k: (5 if "1000" in k else 15) for k in cases}
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
    res = {"rows": n, "d": D, "MT": MT, "rank_of_search_result_is_column": ok, "plan_search16": plan_search,
           "ms_median": {k: round(float(np.median(v)), 4) for k, v in times.items()},
           "ms_min": {k: round(float(np.min(v)), 4) for k, v in times.items()},
           "ms_max": {k: round(float(np.max(v)), 4) for k, v in times.items()}, "plans": plans}
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
