#!/usr/bin/env python3
"""Development: what search_masked_tensor costs on one index, timed with device events on the stream the calls run on.
  (a) a dense mask against the plain search: 1 and 16 queries under an all-ones mask, against search_tensor of the same handle
      forced to scan16_kernel ("force_scan16" = "1", "split" = "0").  Expected: the same row stream plus the list indirection,
      minus the threshold seeding.  Reported: both times, their ratio, and the TB/s of corpus bytes scan16 reaches in this run.
  (b) selective masks at 16 queries: contiguous masks of 1/10, 1/100 and 1/1000 of the rows and a random mask of density 1/1000
      (which touches ~6 % of the 64-row groups).  Reported: the time against (selected groups x 64 x d x 4) bytes, and the call's
      fixed cost -- an all-zeros mask: mask_groups_kernel over every word, a scan that exits at once, the selection.
Every shape is warmed up, every figure is the best of ROUNDS windows of at least 0.2 s of back-to-back calls, and the variants
alternate inside each round.
  python tools/masked_rate.py [rows] [k] [result.json]        (defaults: 1000000 100, the JSON line on stdout only)"""
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
    idx.set_option("force_scan16", "1")
    bench.fill_index(idx, 0, rows, dev, max(bench.CH, rows // 8))
    torch.cuda.synchronize()
    q = bench.gen_rows(0xBEEF, 16, dev)
    group_bytes = 64 * d * 4
    G = (rows + 63) // 64

    def contiguous(frac):
        m = torch.zeros(rows, dtype=torch.bool, device=dev)
        lo = rows // 3
        m[lo:lo + max(1, int(rows * frac))] = True
        return m
    g = torch.Generator(device=dev).manual_seed(0x3A5)
    masks = {
        "ones": torch.ones(rows, dtype=torch.bool, device=dev),
        "zeros": torch.zeros(rows, dtype=torch.bool, device=dev),
        "contiguous_1/10": contiguous(0.1),
        "contiguous_1/100": contiguous(0.01),
        "contiguous_1/1000": contiguous(0.001),
        "random_1/1000": torch.rand(rows, generator=g, device=dev) < 1e-3,
    }
    words = {name: pack_mask(m).reshape(1, -1) for name, m in masks.items()}
    groups = {name: int((w != 0).sum()) for name, w in words.items()}

    variants = {}
    for nq in (1, 16):
        variants[f"a_scan16_nq{nq}"] = (lambda nq=nq: idx.search_tensor(q[:nq], k), G)
        variants[f"a_masked_ones_nq{nq}"] = (lambda nq=nq: idx.search_masked_tensor(q[:nq], k, words["ones"]), G)
    for name in ("zeros", "contiguous_1/10", "contiguous_1/100", "contiguous_1/1000", "random_1/1000"):
        variants[f"b_{name}_nq16"] = (lambda name=name: idx.search_masked_tensor(q, k, words[name]), groups[name])

    result = {"rows": rows, "d": d, "k": k, "groups": G, "rounds": ROUNDS, "min_seconds": MIN_SECONDS, "figures": {}, "plans": {}}
    best = {}
    for _ in range(ROUNDS):
        for name, (fn, _) in variants.items():
            best[name] = min(best.get(name, 1e9), timed(fn, torch))
    for name, (fn, ngroups) in variants.items():
        fn()
        torch.cuda.synchronize()
        result["plans"][name] = idx.last_plan()
        nbytes = ngroups * group_bytes
        fig = {"ms": best[name] * 1e3, "selected_groups": ngroups, "group_bytes": nbytes, "TBps": nbytes / best[name] / 1e12}
        result["figures"][name] = fig
        print(f"{name:26s} {fig['ms']:9.4f} ms  {ngroups:8d} groups  {fig['TBps']:6.3f} TB/s of selected-group bytes", flush=True)
    for nq in (1, 16):
        r = best[f"a_masked_ones_nq{nq}"] / best[f"a_scan16_nq{nq}"]
        result["figures"][f"a_masked_over_scan16_nq{nq}"] = r
        print(f"nq={nq}: all-ones mask at {r:.3f} x the time of search forced to scan16", flush=True)
    # the same answers: an all-ones mask is the search
    a, b = idx.search_tensor(q, k), idx.search_masked_tensor(q, k, words["ones"])
    torch.cuda.synchronize()
    same = torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    result["all_ones_is_search"] = bool(same)
    idx.check_status()
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))
    assert same


if __name__ == "__main__":
    main()
