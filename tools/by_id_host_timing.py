#!/usr/bin/env python3
"""Development: wall time of the staged HOST forms of the by-id calls on one 1M x 768 index of bench.py's synthetic corpus:
reconstruct_n() of the whole index, score_ids of 1000 x 1000 random pairs, rank_ids of 16 x 1.  Every call warm, several
repetitions alternating between the three; prints one JSON object with median, min and max per call.  To compare two
libraries run it once per library (HAC_LIBRARY_PATH picks one), alternating the runs.
  [HAC_LIBRARY_PATH=other/libhaconvdr.so] python tools/by_id_host_timing.py [rows]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import bench
    from haconvdr_amd import synth
    from haconvdr_amd.index import FlatIPIndex
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    dev = torch.device("cuda", 0)
    idx = FlatIPIndex(768)
    bench.fill_index(idx, 0, rows, dev, max(bench.CH, rows // 8))
    torch.cuda.synchronize()
    q = synth.embeddings(0x71E, 1000)
    ids = (synth.uniform_u32(0x71F, 1000 * 1000) % np.uint32(rows)).astype(np.int64).reshape(1000, 1000)
    cases = {
        "reconstruct_n_all": (lambda: idx.reconstruct_n(), 5),
        "score_ids_1000x1000": (lambda: idx.score_ids(q, ids), 9),
        "rank_ids_16x1": (lambda: idx.rank_ids(q[:16], ids[:16, :1]), 15),
    }
    times = {k: [] for k in cases}
    for fn, _ in cases.values():
        fn()
    for r in range(15):
        for k, (fn, reps) in cases.items():
            if r < reps:
                t0 = time.perf_counter()
                fn()
                times[k].append((time.perf_counter() - t0) * 1e3)
    idx.check_status()
    print(json.dumps({"rows": rows, "library": os.environ.get("HAC_LIBRARY_PATH", "in-tree"),
                      "ms_median": {k: round(float(np.median(v)), 3) for k, v in times.items()},
                      "ms_min": {k: round(float(np.min(v)), 3) for k, v in times.items()},
                      "ms_max": {k: round(float(np.max(v)), 3) for k, v in times.items()}}))


if __name__ == "__main__":
    main()
