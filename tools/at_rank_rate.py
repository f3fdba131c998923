#!/usr/bin/env python3
"""Development: what a histogram pass of entries_at costs beside a count_ahead pass, and search_at beside a paged listing, timed
with device events on one index.  16 queries, the benchmark's synthetic corpus.
  - every rank_hist_kernel pass of one entries_at_tensor of 16 pairs (one tile), digit by digit, through the index's own event
    pairs (set_profiling): the first digit (every group reaches the epilogue, nearly every row one bin) apart from the later ones;
  - count_ahead_tensor of 16 queries, m = 1 -- one count_ahead_kernel pass with its memset and finish kernel;
  - a whole entries_at_tensor of 16 pairs (16 queries x 1 rank) and of 256 pairs (16 queries x 16 ranks);
  - search_at_tensor(start, k) beside the pages search_deep fetches to depth start + k (page 1024: search_keys_tensor, then
    search_after_keys_tensor behind each page's last key), and the depth at which the two cost the same.
Every shape is warmed up, every figure is the best of ROUNDS windows of at least 0.2 s of back-to-back calls, and the variants
alternate inside each round.
  python tools/at_rank_rate.py [rows] [start] [k] [result.json]     (defaults: 1000000 10000 100, the JSON line on stdout only)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 3
MIN_SECONDS = 0.2
PAGE = 1024


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
    from haconvdr_amd.index import FlatIPIndex
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    start = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000
    k = int(sys.argv[3]) if len(sys.argv) > 3 else 100
    d = 768
    dev = torch.device("cuda", 0)
    idx = FlatIPIndex(d)
    idx.set_option("split", "0")
    bench.fill_index(idx, 0, rows, dev, max(bench.CH, rows // 8))
    torch.cuda.synchronize()
    q = bench.gen_rows(0xBEEF, 16, dev)
    r1 = torch.full((16, 1), start, dtype=torch.int64, device=dev)
    r16 = (torch.arange(16, dtype=torch.int64, device=dev) * 617 + start).repeat(16, 1).contiguous()
    D1, I1 = idx.entries_at_tensor(q, r1)
    depth = start + k

    def paged():
        pages = [idx.search_keys_tensor(q, min(PAGE, depth))]
        got = pages[0].shape[1]
        while got < depth:
            kk = min(PAGE, depth - got)
            pages.append(idx.search_after_keys_tensor(q, kk, pages[-1][:, -1].contiguous()))
            got += kk
        return torch.cat(pages, dim=1)

    variants = {
        "count_ahead_16x1": lambda: idx.count_ahead_tensor(q, D1, I1),
        "entries_at_16_pairs": lambda: idx.entries_at_tensor(q, r1),
        "entries_at_256_pairs": lambda: idx.entries_at_tensor(q, r16),
        "search_at": lambda: idx.search_at_keys_tensor(q, k, start),
        "one_after_page_1024": lambda: idx.search_after_keys_tensor(q, PAGE, None),
        "paged_to_depth": paged,
    }
    result = {"rows": rows, "d": d, "nq": 16, "start": start, "k": k, "page": PAGE, "rounds": ROUNDS, "min_seconds": MIN_SECONDS,
              "figures_ms": {}, "plans": {}}
    best = {}
    for _ in range(ROUNDS):
        for name, fn in variants.items():
            best[name] = min(best.get(name, 1e9), timed(fn, torch))
    for name, fn in variants.items():
        fn()
        torch.cuda.synchronize()
        result["plans"][name] = idx.last_plan()
        result["figures_ms"][name] = best[name] * 1e3
        print(f"{name:22s} {best[name] * 1e3:9.4f} ms", flush=True)
    # the passes of one tile of 16 pairs, digit by digit: the index's own event pairs around every rank_hist_kernel launch
    idx.set_profiling(True)
    idx.profile_drain()
    per_pass = None
    for _ in range(10):
        idx.entries_at_tensor(q, r1)
        torch.cuda.synchronize()
        ms = idx.profile_drain()
        per_pass = ms if per_pass is None else [min(a, b) for a, b in zip(per_pass, ms)]
    idx.set_profiling(False)
    result["rank_hist_pass_ms"] = per_pass
    result["first_digit_over_count_ahead"] = per_pass[0] / (best["count_ahead_16x1"] * 1e3)
    print("rank_hist_kernel passes (ms, top digit first):", " ".join(f"{v:.4f}" for v in per_pass), flush=True)
    # a listing to depth D costs ~ search + (D / PAGE - 1) after-pages; search_at costs the same at any depth
    page_ms = best["one_after_page_1024"] * 1e3
    result["crossover_depth"] = PAGE * best["search_at"] * 1e3 / page_ms
    print(f"crossover depth ~ {result['crossover_depth']:.0f} rows (search_at {best['search_at'] * 1e3:.3f} ms, one page of {PAGE}: {page_ms:.3f} ms)")
    try:
        result["sclk_MHz_after"] = torch.cuda.clock_rate()
    except Exception:
        result["sclk_MHz_after"] = None
    # the same answers: the window is the tail of the paged listing
    a = idx.search_at_keys_tensor(q, k, start)
    b = paged()[:, start:start + k]
    torch.cuda.synchronize()
    same = torch.equal(a, b)
    result["window_is_the_tail_of_the_listing"] = bool(same)
    idx.check_status()
    if len(sys.argv) > 4:
        with open(sys.argv[4], "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))
    assert same


if __name__ == "__main__":
    main()
