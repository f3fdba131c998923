#!/usr/bin/env python3
"""What search_excluding costs: 1000 queries over N rows, event-timed, warm, the variants alternating inside every repetition.
  python tools/excluding_timing.py [rows] [reps]
Lines: search_tensor at k = 100 and at k' = 108 (the yardstick: the search the call runs inside), search_excluding_tensor(k = 100,
e = 8, the query's own top-8 excluded so that every list shifts), the filter launch and the keys_to_results launch alone on the
same 1000 x 108 keys (20 launches per timing), and the prefilter's edge: k' = 192 against k' = 193, plain and as 100 + 92 / 93."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import bench
    from haconvdr_amd.index import FlatIPIndex, filter_keys, keys_to_results
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    dev = torch.device("cuda", 0)
    idx = FlatIPIndex(768)
    bench.fill_index(idx, 0, rows, dev, max(1, rows // 8))
    q = bench.gen_rows(0xBEEF, 1000, dev)
    _, top = idx.search_tensor(q, 2 * 93)
    E = {e: top[:, :e].contiguous() for e in (8, 92, 93)}
    keys108 = idx.search_keys_tensor(q, 108)
    burst = 20

    def many(fn):
        def run():
            for _ in range(burst):
                fn()
        return run

    variants = [
        ("search_tensor k=100", lambda: idx.search_tensor(q, 100), 1),
        ("search_tensor k=108", lambda: idx.search_tensor(q, 108), 1),
        ("search_excluding_tensor k=100 e=8", lambda: idx.search_excluding_tensor(q, 100, E[8]), 1),
        ("filter_keys 1000x108 -> 100, e=8 (per launch)", many(lambda: filter_keys(keys108, E[8], 100)), burst),
        ("keys_to_results 1000x108 (per launch)", many(lambda: keys_to_results(keys108)), burst),
        ("search_tensor k=192", lambda: idx.search_tensor(q, 192), 1),
        ("search_tensor k=193", lambda: idx.search_tensor(q, 193), 1),
        ("search_excluding_tensor k=100 e=92", lambda: idx.search_excluding_tensor(q, 100, E[92]), 1),
        ("search_excluding_tensor k=100 e=93", lambda: idx.search_excluding_tensor(q, 100, E[93]), 1),
    ]
    plans = {}
    for _ in range(3):                                       # warm every shape (workspaces, the fp16 image, the row-major copy)
        for name, fn, _n in variants:
            fn()
            plans[name] = idx.last_plan()
    torch.cuda.synchronize()
    idx.check_status()
    ms = {name: [] for name, _, _ in variants}
    for _ in range(reps):
        for name, fn, n in variants:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / n)
    idx.check_status()
    print(f"rows {rows}, 1000 queries, {reps} repetitions (ms: median / min / max)")
    for name, _, _ in variants:
        v = np.asarray(ms[name])
        plan = "" if "per launch" in name else " | " + plans[name][:110]
        print(f"  {name:48s} {np.median(v):8.4f} {v.min():8.4f} {v.max():8.4f}{plan}", flush=True)


if __name__ == "__main__":
    main()
