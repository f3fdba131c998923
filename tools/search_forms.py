#!/usr/bin/env python3
"""Development: one search per form of the index's host driver (exact kernels, prefilter with its tile / chunk / pass forms,
the host- and the device-decided fallback, a captured search, shards, the debug options), each on the smallest corpus that
reaches the form.  Per case one line: name, last_plan(), sha256 of the D and I bytes.  Two libraries that drive the same
kernels the same way print the same lines (HAC_LIBRARY_PATH picks the library); under `rocprofv3 --kernel-trace` the run
gives the launch sequence to compare.
  [HAC_LIBRARY_PATH=other/libhaconvdr.so] python tools/search_forms.py"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def report(name, idx, *arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    print(f"{name} | {idx.last_plan() if idx is not None else '-'} | {h.hexdigest()}", flush=True)


def main():
    import torch
    from haconvdr_amd import _lib, synth
    from haconvdr_amd.index import FlatIPIndex

    def index(x, **options):
        idx = FlatIPIndex(x.shape[1])
        for name, value in options.items():
            idx.set_option(name, value)
        idx.add(x)
        return idx

    def host(name, idx, q, k):
        report(name, idx, *idx.search(q, k))

    def device(name, idx, q, k):
        D, I = idx.search_tensor(torch.from_numpy(q).cuda(), k)
        torch.cuda.synchronize()                    # (the status slot's counts are in the text after this)
        report(name, idx, D.cpu().numpy(), I.cpu().numpy())

    # ---- exact kernels: scan16 without / with seeding (255 / 257+ groups), scanq, two query chunks
    x96, q96 = synth.embeddings(11, 16449, 96), synth.embeddings(12, 5, 96)
    host("scan16 unseeded", index(x96[:1000]), q96, 10)
    host("scan16 255 groups", index(x96[:16320]), q96, 10)
    host("scan16 seeded", index(x96), q96, 10)
    host("scanq", index(synth.embeddings(13, 16449, 64)), synth.embeddings(14, 40, 64), 10)
    host("exact 2 chunks", index(x96[:1000]), synth.embeddings(15, 1030, 96), 10)

    # ---- prefilter at its smallest width: quarter / half / full tile, two tiles, two chunks, three products
    x192, q192 = synth.embeddings(21, 4096, 192), synth.embeddings(22, 1030, 192)
    idx = index(x192, split="1")
    for nq in (20, 100, 300, 1030):
        host(f"split nq={nq}", idx, q192[:nq], 10)
    idx.set_option("split_terms", "3")
    host("split terms=3", idx, q192[:100], 10)
    idx.set_option("split_terms", "1")
    for nq in (100, 1030):                          # the same through the device entry point: device-decided, nothing fails
        device(f"split device nq={nq}", idx, q192[:nq], 10)
    idx.set_option("split_decide", "device")        # ... and the host entry point over the device-decided arm
    host("split host decide=device", idx, q192[:100], 10)

    # ---- host-decided fallback: a few failing queries -> exact kernels; 64 or more -> the three-product level
    x768, q768 = synth.embeddings(4242, 6000), synth.embeddings(4243, 80)
    q768[3] = 0.0                                   # a zero query: all scores tie
    idx = index(x768, split="1")
    host("fallback host few", idx, q768, 100)
    device("fallback device few", idx, q768, 100)
    base = synth.embeddings(5, 1)[0]
    dense = (base[None, :] + 0.03 * np.random.default_rng(99).standard_normal((8000, 768))).astype(np.float32)
    qd = (synth.embeddings(6, 96) + 0.5 * base[None, :]).astype(np.float32)
    idx = index(dense, split="1")
    host("fallback host cascade", idx, qd, 100)
    assert "; then scanh_kernel<3>" in idx.last_plan(), idx.last_plan()

    # ---- device-decided fallback over more queries than a chunk of the exact kernels
    qm = synth.embeddings(516, 2100)
    qm[::3] = 0.0
    qm[1::3] *= 1e-30
    device("fallback device 3 chunks", index(synth.embeddings(515, 5000), split="1"), qm, 20)

    # ---- a captured and replayed device search on the prefilter path
    xc, qc = synth.embeddings(0xCA97, 30000), torch.from_numpy(synth.embeddings(0xCA98, 130)).cuda()
    idx = index(xc, split="1")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        idx.search_tensor(qc, 100)                  # warm-up: workspaces, fp16 image, segment table
        side.synchronize()
        assert "decided=device" in idx.last_plan(), idx.last_plan()     # (and its status slot collected: the capture polls no event)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            D, I = idx.search_tensor(qc, 100)
        D.zero_()
        I.zero_()
        graph.replay()
        side.synchronize()
    torch.cuda.synchronize()
    report("captured", idx, D.cpu().numpy(), I.cpu().numpy())
    assert "status not collected" in idx.last_plan(), idx.last_plan()

    # ---- three pinned passes (a corpus of 8 rounds of 128 row streams x 4 groups: cuts after rounds 2 and 5)
    g = torch.Generator(device="cuda").manual_seed(20264)
    xp = torch.randn((262144, 192), generator=g, device="cuda") * torch.linspace(1.0, 1.5, 262144, device="cuda")[:, None]
    idx = FlatIPIndex(192)
    for name, value in (("split", "1"), ("scan_passes", "3"), ("scan_pass_cuts", "300,600")):
        idx.set_option(name, value)
    idx.add_tensor(xp)
    device("split 3 passes", idx, q192[:300], 50)
    assert "passes=3" in idx.last_plan(), idx.last_plan()

    # ---- two in-process shards on one device: search (threads, remap, merge), rows and scores by id
    xs, qs = synth.embeddings(31337, 3000), synth.embeddings(31338, 6)
    xs[1500:] = xs[:1500]
    idx = FlatIPIndex(768, devices=(0, 0))
    idx.add(xs[:1000])
    idx.add(xs[1000:1001])
    idx.add(xs[1001:])
    D, I = idx.search(qs, 100)
    report("shards search", idx, D, I)
    report("shards reconstruct", None, idx.reconstruct_batch(I[0]))
    report("shards score_ids", None, idx.score_ids(qs, I))

    # ---- debug options: an allocation that finds the device full takes the row copies back (rescore_rows = 1: the next search
    # builds them again); a pass bound that is reached
    idx = index(x768, split="1", rescore_rows="1")
    host("rescore rows", idx, q768[:70], 100)
    idx.set_option("debug_oom", "1")
    idx.add(x768[:100])
    host("debug_oom", idx, q768[:70], 100)
    n, nq = 6000, 40
    xb, qb = np.zeros((n, 768), np.float32), np.zeros((nq, 768), np.float32)
    xb[:, 0] = (np.arange(n, dtype=np.float32) + 1.0) / 64.0      # every row beats all rows before it
    qb[:, 0] = 1.0 + np.arange(nq, dtype=np.float32) / 8.0
    idx = index(xb, debug_max_pass="2")
    try:
        idx.search(qb, 10)
        raise AssertionError("the lowered pass bound was not reached")
    except _lib.HacError as e:
        # (how many workgroups overran depends on how fast the chip-wide thresholds spread: not part of the comparison)
        print(f"debug_max_pass | {idx.last_plan()} | code {e.code}: ...{str(e).split('scan workgroup(s)')[-1]}", flush=True)


if __name__ == "__main__":
    main()
