#!/usr/bin/env python3
"""What search_among costs: 1000 queries x 1000 candidates, k = 100, over N rows, event-timed, warm, the variants alternating
inside every repetition.
  python tools/among_timing.py [rows] [reps]
Lines: search_among_tensor, and the only route to the same answer without it: score_ids_tensor, a device torch.sort (descending,
stable) and a slice -- which is NOT exact on repeats (a row named twice is listed twice) and leaves padding and NaN scores to
the caller.  The candidates are distinct rows, so that both routes return the same lists and the comparison is checked; each
route is timed with the row-major rescoring copy absent (split = "0": the rows come out of the tiles) and current (after three
prefilter searches).  The shader clock held during the run is read the way bench.py reads it (hac_encoder_last_clock, a
2-layer encoder's FFN-up launch of 320 x 512 tokens) before and after the timed loop."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def held_clock_mhz(enc, ids, mask):
    enc.set_profiling(True, classes="all")
    enc(ids, mask)
    enc.profile_drain_class("ffn_up")
    mhz, _ = enc.last_clock_mhz()
    enc.set_profiling(False)
    return mhz


def main():
    import torch
    import bench
    from haconvdr_amd import synth
    from haconvdr_amd.encoder import ANCEEncoder
    from haconvdr_amd.index import FlatIPIndex
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    nq, m, k = 1000, 1000, 100
    dev = torch.device("cuda", 0)
    idx = FlatIPIndex(768)
    idx.set_option("split", "0")
    bench.fill_index(idx, 0, rows, dev, max(1, rows // 8))
    q = bench.gen_rows(0xBEEF, nq, dev)
    g = torch.Generator(device=dev).manual_seed(0xCA9D)
    cand = torch.stack([torch.randperm(rows, generator=g, device=dev)[:m] for _ in range(nq)]).contiguous()      # distinct rows per query

    def among():
        return idx.search_among_tensor(q, k, cand)

    def score_sort():
        S = idx.score_ids_tensor(q, cand)
        D, order = torch.sort(S, dim=1, descending=True, stable=True)
        return D[:, :k], torch.gather(cand, 1, order[:, :k])

    enc = ANCEEncoder.from_state_dict(synth.ance_state_dict(0xA11CE, 2, rich=False))
    ids, _ = synth.token_batch(3, 320, 512, fixed_len=512)
    mask = np.ones_like(ids)
    enc(ids, mask)
    variants = [("search_among_tensor", among), ("score_ids_tensor + torch.sort + slice", score_sort)]
    print(f"rows {rows}, {nq} queries x {m} candidates, k = {k}, {reps} repetitions (ms: median / min / max)", flush=True)
    for state in ("tiles", "row-major copy"):
        if state == "row-major copy":
            idx.set_option("split", "1")
            idx.set_option("rescore_rows", "1")
            for _ in range(3):
                idx.search_tensor(q, k)
            assert "rescore=rows" in idx.last_plan(), idx.last_plan()
        for _ in range(3):                                   # warm every shape
            for _name, fn in variants:
                fn()
        torch.cuda.synchronize()
        (aD, aI), (sD, sI) = among(), score_sort()
        torch.cuda.synchronize()
        # the same lists wherever neighbours do not tie (torch.sort breaks ties by list position, the index by row)
        same = bool(torch.equal(aD.view(torch.int32), sD.contiguous().view(torch.int32)))
        ties = int((aD[:, 1:] == aD[:, :-1]).sum())
        among()
        plan = idx.last_plan()
        clk0 = held_clock_mhz(enc, ids, mask)
        ms = {name: [] for name, _ in variants}
        for _ in range(reps):
            for name, fn in variants:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms[name].append(a.elapsed_time(b))
        clk1 = held_clock_mhz(enc, ids, mask)
        idx.check_status()
        print(f"[{state}] D bits equal on both routes: {same} (tied neighbours: {ties}); held clock {clk0:.0f} MHz before, {clk1:.0f} MHz after", flush=True)
        for name, _ in variants:
            v = np.asarray(ms[name])
            print(f"  {name:42s} {np.median(v):8.4f} {v.min():8.4f} {v.max():8.4f}" + (f" | {plan}" if name == "search_among_tensor" else ""), flush=True)


if __name__ == "__main__":
    main()
