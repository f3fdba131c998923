#!/usr/bin/env python3
"""Development: what search_after_tensor costs on one index beside search_masked_tensor under an all-ones mask (the same pass
structure plus a group list and mask words, no seeding) and search_tensor with "split" = "0" (the exact kernels, seeded
thresholds), timed with device events on the stream the calls run on.  16 queries, the benchmark's synthetic corpus.  Cursors:
the start, the last entry of page 1 (depth k) and the last entry of a search at HAC_MAX_K (depth 2048).
Every shape is warmed up, every figure is the best of ROUNDS windows of at least 0.2 s of back-to-back calls, and the variants
alternate inside each round.
  python tools/after_rate.py [rows] [k] [result.json]        (defaults: 1000000 100, the JSON line on stdout only)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 3
MIN_SECONDS = 0.2


def timed(fn, torch):
    """Seconds per call of fn(): warm-up, a calibration call, then one event-bracketed window of >= MIN_SECONDS."""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    reps = max(2, int(MIN_SECONDS / max(e0.elapsed_time(e1) * 1e-3, 1e-6)) + 1)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def main():
    import torch
    import bench
    from haconvdr_amd.index import FlatIPIndex, pack_mask
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    d = 768
    dev = torch.device("cuda", 0)
    idx = FlatIPIndex(d)
    idx.set_option("split", "0")
    bench.fill_index(idx, 0, rows, dev, max(bench.CH, rows // 8))
    torch.cuda.synchronize()
    q = bench.gen_rows(0xBEEF, 16, dev)
    ones = pack_mask(torch.ones(rows, dtype=torch.bool, device=dev)).reshape(1, -1)
    D1, I1 = idx.search_tensor(q, k)
    Dk, Ik = idx.search_tensor(q, 2048)
    page1 = (D1[:, -1].contiguous(), I1[:, -1].contiguous())
    deep = (Dk[:, -1].contiguous(), Ik[:, -1].contiguous())
    variants = {
        "search_split0": lambda: idx.search_tensor(q, k),
        "masked_ones": lambda: idx.search_masked_tensor(q, k, ones),
        "after_start": lambda: idx.search_after_tensor(q, k),
        "after_page1": lambda: idx.search_after_tensor(q, k, page1),
        "after_depth2048": lambda: idx.search_after_tensor(q, k, deep),
    }
    result = {"rows": rows, "d": d, "k": k, "nq": 16, "rounds": ROUNDS, "min_seconds": MIN_SECONDS, "figures": {}, "plans": {}}
    best = {}
    for _ in range(ROUNDS):
        for name, fn in variants.items():
            best[name] = min(best.get(name, 1e9), timed(fn, torch))
    for name, fn in variants.items():
        fn()
        torch.cuda.synchronize()
        result["plans"][name] = idx.last_plan()
        result["figures"][name] = {"ms": best[name] * 1e3, "over_masked_ones": best[name] / best["masked_ones"]}
        print(f"{name:18s} {best[name] * 1e3:9.4f} ms  {best[name] / best['masked_ones']:6.3f} x masked all-ones", flush=True)
    # the same answers: a start cursor is the search, and page 2 continues the list of a deeper search
    a, b = idx.search_tensor(q, k), idx.search_after_tensor(q, k)
    c = idx.search_after_tensor(q, k, page1)
    torch.cuda.synchronize()
    same = torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(c[1], Ik[:, k:2 * k])
    result["start_is_search_and_page2_continues"] = bool(same)
    idx.check_status()
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))
    assert same


if __name__ == "__main__":
    main()
