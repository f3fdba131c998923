#!/usr/bin/env python3
"""Development: rates of the rows-by-id entry points (reconstruct_tensor / score_ids_tensor) on one index, as TB/s of
algorithmic bytes, timed with device events on the stream the calls run on.
  (a) reconstruct_tensor of the whole range (2 n d 4 bytes: every row read once, written once) against a device-to-device
      copy of the same n d 4 bytes (also 2 n d 4 moved), taken in the same run: the yardstick;
  (b) reconstruct_tensor of NQ x 100 random ids (2 n d 4), from the tiles and from the row-major copy;
  (c) score_ids_tensor at NQ x 100 and NQ x 1000 random ids (nq m d 4 read), from both sources.
Every shape is warmed up, every figure is the best of ROUNDS windows of at least 0.2 s of back-to-back calls, and the
variants alternate inside each round (the copy beside the range read; the two sources cannot alternate call by call --
switching the source rebuilds or frees the copy -- so each source gets its own block of rounds and the range read and the
copy are repeated in both as a drift check).
  python tools/rows_rate.py [rows] [nq] [result.json]        (defaults: 1000000 1000, the JSON line on stdout only)"""
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
    from haconvdr_amd.index import FlatIPIndex
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    nq = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    d = 768
    dev = torch.device("cuda", 0)
    idx = FlatIPIndex(d)
    idx.set_option("split", "1")
    bench.fill_index(idx, 0, rows, dev, max(bench.CH, rows // 8))
    torch.cuda.synchronize()
    q = bench.gen_rows(0xBEEF, nq, dev)
    g = torch.Generator(device=dev).manual_seed(0x1D5)
    ids = {m: torch.randint(0, rows, (nq, m), generator=g, device=dev, dtype=torch.int64) for m in (100, 1000)}
    src = torch.empty((rows, d), dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    row_bytes = d * 4

    variants = {
        "a_range": (lambda: idx.reconstruct_tensor(), 2 * rows * row_bytes),
        "a_copy_d2d": (lambda: dst.copy_(src), 2 * rows * row_bytes),
        "b_ids_%dx100" % nq: (lambda: idx.reconstruct_tensor(ids[100].view(-1)), 2 * nq * 100 * row_bytes),
        "c_score_%dx100" % nq: (lambda: idx.score_ids_tensor(q, ids[100]), nq * 100 * row_bytes),
        "c_score_%dx1000" % nq: (lambda: idx.score_ids_tensor(q, ids[1000]), nq * 1000 * row_bytes),
    }
    result = {"rows": rows, "d": d, "nq": nq, "rounds": ROUNDS, "min_seconds": MIN_SECONDS, "figures": {}}
    check = {}
    for source in ("tiles", "rows"):
        idx.set_option("rescore_rows", "1" if source == "rows" else "0")
        idx.search_tensor(q[:64], 100)                    # a prefilter search builds (or frees) the row-major copy
        torch.cuda.synchronize()
        plan = idx.last_plan()
        assert ("rescore=" + source) in plan, plan
        best = {}
        for _ in range(ROUNDS):
            for name, (fn, _) in variants.items():
                best[name] = min(best.get(name, 1e9), timed(fn, torch))
        for name, (fn, nbytes) in variants.items():
            fig = {"ms": best[name] * 1e3, "algorithmic_bytes": nbytes, "TBps": nbytes / best[name] / 1e12}
            result["figures"][source + ":" + name] = fig
            print(f"{source:5s} {name:18s} {fig['ms']:9.3f} ms  {fig['TBps']:6.3f} TB/s of algorithmic bytes", flush=True)
        r = best["a_copy_d2d"] / best["a_range"]
        result["figures"][source + ":a_range_over_copy"] = r
        print(f"{source:5s} whole range at {r:.2f} of the device-to-device copy's rate", flush=True)
        check[source] = (idx.reconstruct_tensor(ids[100].view(-1)), idx.score_ids_tensor(q, ids[1000]))
    torch.cuda.synchronize()
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(check["tiles"], check["rows"]))
    result["same_bits_from_both_sources"] = bool(same)
    print("same bits from both sources:", same, flush=True)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))
    assert same


if __name__ == "__main__":
    main()
