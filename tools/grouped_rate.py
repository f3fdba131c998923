#!/usr/bin/env python3
"""Development: what search_grouped_tensor costs on one index beside search_masked_tensor under an all-ones mask (the closest
older kernel: the same passes over the rows, no seeding), timed with device events on the stream the calls run on.  16 queries,
the benchmark's synthetic corpus, "split" = "0".  Labels: r // 4 (groups of four neighbouring rows), distinct labels, and one
giant group of three rows in five (whose rows are ordinary rows here, so it does not lead the lists).
Every shape is warmed up, every figure is the best of ROUNDS windows of at least 0.2 s of back-to-back calls, and the variants
alternate inside each round.
  python tools/grouped_rate.py [rows] [k] [result.json]        (defaults: 1000000 100, the JSON line on stdout only)"""
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
    r = torch.arange(rows, dtype=torch.int64, device=dev)
    ones = pack_mask(torch.ones(rows, dtype=torch.bool, device=dev)).reshape(1, -1)
    labels = {"r//4": r // 4, "distinct": r.clone(), "giant_3_in_5": torch.where(r % 5 < 3, torch.zeros_like(r), 1 + r)}
    variants = {"masked_ones": lambda: idx.search_masked_tensor(q, k, ones)}
    for name, lab in labels.items():
        variants["grouped_" + name] = (lambda lab=lab: idx.search_grouped_tensor(q, k, lab))
    best, plans = {}, {}
    for _ in range(ROUNDS):
        for name, fn in variants.items():
            t = timed(fn, torch)
            best[name] = min(best.get(name, t), t)
            plans[name] = idx.last_plan()
    idx.check_status()
    # the grouped answer under distinct labels is the masked answer under all ones
    a, b = idx.search_grouped_tensor(q, k, labels["distinct"]), idx.search_masked_tensor(q, k, ones)
    torch.cuda.synchronize()
    same = bool(torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)))
    out = {"rows": rows, "k": k, "nq": 16, "ms": {n: round(t * 1e3, 4) for n, t in best.items()},
           "ratio_to_masked": {n: round(t / best["masked_ones"], 3) for n, t in best.items()}, "distinct_equals_masked": same, "plans": plans}
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
