#!/usr/bin/env python3
"""What remove_ids costs: FlatIPIndex.remove_ids over 1M x 768 rows of bench.py's synthetic corpus against two yardsticks taken
in the same run, event-timed, warm, the variants alternating inside every repetition; prints one JSON object.
  python tools/remove_timing.py
Removals: row 0 (every row moves), 1 % random rows (nearly every row moves), the last 1 % (nothing in front moves); each on an
index without images (split = "0") and on one that holds a complete fp16 image and row-major copy (split = "1", fp16_image =
"eager", rescore_rows = "1", searched once), which the call has to bring up to date.  The call moves 4 (n - f) d 4 bytes, f the
first removed row: every moved row is gathered into the staging buffer and copied to its place.
Yardsticks: a device-to-device copy_ of (n - f) d 4 bytes (the staged scheme cannot beat twice that copy's time), and what a user
had to do before: reset() plus add() of the surviving rows from the host.
Every timed call starts from the same index: it is reset and refilled from a device copy of the rows in between, untimed."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from haconvdr_amd.index import FlatIPIndex  # noqa: E402

D, CH, REPS = 768, 125_000, 7


def gen_rows(seed, n, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn((n, D), generator=g, device=dev, dtype=torch.float32)
    return (x - x.mean(1, keepdim=True)) / x.std(1, unbiased=False, keepdim=True)


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()                                   # (the host calls end in a synchronise of the index's stream)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    dev = torch.device("cuda", 0)
    x = torch.cat([gen_rows(0xC0FFEE + c, CH, dev) for c in range(8)])
    n = x.shape[0]
    q = gen_rows(0x9E, 96, dev)
    rng = np.random.RandomState(0x4E)
    removals = {"row0": np.array([0], np.int64),
                "random_1pct": np.sort(rng.choice(n, n // 100, replace=False)).astype(np.int64),
                "last_1pct": np.arange(n - n // 100, n, dtype=np.int64)}
    plain, imaged = FlatIPIndex(D, devices=(0,)), FlatIPIndex(D, devices=(0,))
    plain.set_option("split", "0")
    for name, value in (("split", "1"), ("fp16_image", "eager"), ("rescore_rows", "1")):
        imaged.set_option(name, value)

    def refill(idx, images):
        idx.reset()
        idx.add_tensor(x)
        if images:
            idx.search_tensor(q, 10)
            assert "rescore=rows" in idx.last_plan(), idx.last_plan()
        torch.cuda.synchronize()

    # the calls do what they say, once, before anything is timed
    checks = {}
    for key, ids in removals.items():
        keep = np.ones(n, bool)
        keep[ids] = False
        want = x[torch.from_numpy(keep).to(dev)]
        for idx, images in ((plain, False), (imaged, True)):
            refill(idx, images)
            removed = idx.remove_ids(ids)
            got = idx.reconstruct_tensor()
            torch.cuda.synchronize()
            ok = removed == len(ids) and idx.ntotal == n - len(ids) and torch.equal(got.view(torch.int32), want.view(torch.int32))
            if images:
                D0, I0 = idx.search_tensor(q, 10)
                plan = idx.last_plan()
                idx.set_option("split", "0")
                D1, I1 = idx.search_tensor(q, 10)
                idx.set_option("split", "1")
                torch.cuda.synchronize()
                ok = ok and plan.startswith("split:") and "rescore=rows" in plan and torch.equal(I0, I1) and torch.equal(D0, D1)
            checks[f"{key}{'_images' if images else ''}"] = bool(ok)
            del got
        del want
    moved = {key: (n - int(ids[0])) * D * 4 for key, ids in removals.items()}
    scratch = torch.empty_like(x)
    survivors_host = x[1:].cpu().numpy()                    # the rows left by "row0", for the old way
    times = {}

    def note(key, ms):
        times.setdefault(key, []).append(ms)

    for rep in range(REPS + 1):                             # rep 0: warm-up
        for key, ids in removals.items():
            for idx, images in ((plain, False), (imaged, True)):
                refill(idx, images)
                ms = timed(lambda: idx.remove_ids(ids))
                if rep:
                    note(f"remove_{key}{'_images' if images else ''}", ms)
            f = int(ids[0])
            ms = timed(lambda: scratch[f:].copy_(x[f:]))
            if rep:
                note(f"copy_{key}", ms)
        if rep <= 3:                                        # 3 GB over the link each time: three repetitions
            refill(plain, False)

            def old_way():
                plain.reset()
                plain.add(survivors_host)
            ms = timed(old_way)
            if rep:
                note("reset_and_add_survivors_from_host", ms)
    plain.check_status()
    imaged.check_status()
    med = {k: float(np.median(v)) for k, v in times.items()}
    res = {"rows": n, "d": D, "checks": checks,
           "ms_median": {k: round(v, 4) for k, v in med.items()},
           "ms_min": {k: round(float(np.min(v)), 4) for k, v in times.items()},
           "ms_max": {k: round(float(np.max(v)), 4) for k, v in times.items()},
           "bytes_moved_rows": moved,
           "remove_over_copy": {k: round(med[f"remove_{k}"] / med[f"copy_{k}"], 3) for k in removals},
           "remove_images_over_copy": {k: round(med[f"remove_{k}_images"] / med[f"copy_{k}"], 3) for k in removals},
           "copy_TBps": {k: round(2 * moved[k] / med[f"copy_{k}"] * 1e-9, 3) for k in removals},
           "remove_traffic_TBps": {k: round(4 * moved[k] / med[f"remove_{k}"] * 1e-9, 3) for k in removals}}
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
