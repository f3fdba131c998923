#!/usr/bin/env python3
"""Development: one search per form of the index's host driver (exact kernels, prefilter with its tile / chunk / pass forms,
the host- and the device-decided fallback, a captured search, shards, the by-id calls and their refusals, the debug options),
each on the smallest corpus that reaches the form.  Per case one line: name, last_plan(), sha256 of the D and I bytes.  Two libraries that drive the same
kernels the same way print the same lines (HAC_LIBRARY_PATH picks the library); under `rocprofv3 --kernel-trace` the run
gives the launch sequence to compare.
  [HAC_LIBRARY_PATH=other/libhaconvdr.so] python tools/search_forms.py"""
import ctypes
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

    # ---- the by-id calls and search_excluding, host and tensor form, on one shard and on the two above; then every refusal
    # of theirs with its code and full message
    def refused(name, call):
        try:
            call()
            raise AssertionError(f"{name}: not refused")
        except _lib.HacError as e:
            print(f"refused {name} | code {e.code}: {e}", flush=True)
        except ValueError as e:
            print(f"refused {name} | ValueError: {e}", flush=True)

    def cuda(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def cpu(t):
        torch.cuda.synchronize()
        return t.cpu().numpy()

    one = FlatIPIndex(768)
    one.add(xs[:1000])
    one.add(xs[1000:1001])
    one.add(xs[1001:])
    n = len(xs)
    ids = (synth.uniform_u32(31339, 6 * 50) % np.uint32(n + 1)).astype(np.int64).reshape(6, 50) - 1
    ids[0, :2] = (7, 1507)                           # a pair of identical rows
    excl = I[:, :7].copy()
    excl[:, 3] = -1
    for name, ix in (("one", one), ("shards", idx)):
        report(f"{name} reconstruct_n", None, ix.reconstruct_n(), ix.reconstruct_n(999, 5))
        report(f"{name} reconstruct_batch", None, ix.reconstruct_batch(ids[1]))
        report(f"{name} score_ids", None, ix.score_ids(qs, ids))
        report(f"{name} rank_ids", ix, ix.rank_ids(qs, ids))
        report(f"{name} search_excluding", ix, *ix.search_excluding(qs, 100, excl))
    qt, it = cuda(qs), cuda(ids)
    report("one reconstruct_tensor", None, cpu(one.reconstruct_tensor(it[1])), cpu(one.reconstruct_tensor(i0=999, n=5)))
    St = one.score_ids_tensor(qt, it)
    report("one score_ids_tensor", None, cpu(St))
    report("one rank_ids_tensor", one, cpu(one.rank_ids_tensor(qt, it)))
    report("one count_ahead_tensor", one, cpu(one.count_ahead_tensor(qt, St, it)))
    report("one search_excluding_tensor", one, *[cpu(t) for t in one.search_excluding_tensor(qt, 100, cuda(excl))])
    bad = ids.copy()
    bad[2, 5] = n
    for name, ix in (("one", one), ("shards", idx)):
        refused(f"{name} reconstruct_batch id", lambda: ix.reconstruct_batch(bad[2]))
        refused(f"{name} reconstruct_n range", lambda: ix.reconstruct_n(n - 1, 2))
        refused(f"{name} score_ids id", lambda: ix.score_ids(qs, bad))
        refused(f"{name} rank_ids id", lambda: ix.rank_ids(qs, bad))
        refused(f"{name} search_excluding id", lambda: ix.search_excluding(qs, 10, bad[:, :9]))
        refused(f"{name} search_excluding k + e", lambda: ix.search_excluding(qs, 2040, excl.repeat(2, axis=1)))
    refused("shards reconstruct_tensor", lambda: idx.reconstruct_tensor(it[1]))
    refused("shards reconstruct_tensor range", lambda: idx.reconstruct_tensor(i0=0, n=4))
    refused("shards score_ids_tensor", lambda: idx.score_ids_tensor(qt, it))
    refused("shards rank_ids_tensor", lambda: idx.rank_ids_tensor(qt, it))
    refused("shards count_ahead_tensor", lambda: idx.count_ahead_tensor(qt, St, it))
    refused("shards search_excluding_tensor", lambda: idx.search_excluding_tensor(qt, 10, cuda(excl)))
    refused("one reconstruct_tensor range", lambda: one.reconstruct_tensor(i0=n - 1, n=2))
    # (what the Python layer refuses first, and pointers it always aligns: the C entry points themselves)
    L, vp = _lib.lib(), ctypes.c_void_p
    out = torch.empty((6, 50, 2), dtype=torch.int64, device="cuda")
    st = vp(torch.cuda.current_stream().cuda_stream)
    Dh, Ih = np.empty((6, 2040), np.float32), np.empty((6, 2040), np.int64)
    f32p, i64p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int64)
    for name, call in (
            ("C search_excluding k + e", lambda: L.hac_index_search_excluding(one._h, qs.ctypes.data_as(f32p), 6, 2040, excl.ctypes.data_as(i64p), 9,
                                                                               Dh.ctypes.data_as(f32p), Ih.ctypes.data_as(i64p))),
            ("C search_excluding_device k + e", lambda: L.hac_index_search_excluding_device(one._h, vp(qt.data_ptr()), 6, 2040, vp(it.data_ptr()), 9,
                                                                                             vp(out.data_ptr()), vp(out.data_ptr()), vp(), st)),
            ("C reconstruct_device out + 4", lambda: L.hac_index_reconstruct_device(one._h, vp(it.data_ptr()), 0, 1, vp(out.data_ptr() + 4), st)),
            ("C reconstruct_device range out + 4", lambda: L.hac_index_reconstruct_device(one._h, vp(), 0, 1, vp(out.data_ptr() + 4), st)),
            ("C score_ids_device q + 4", lambda: L.hac_index_score_ids_device(one._h, vp(qt.data_ptr() + 4), 1, vp(it.data_ptr()), 50, vp(out.data_ptr()), st)),
            ("C rank_ids_device q + 4", lambda: L.hac_index_rank_ids_device(one._h, vp(qt.data_ptr() + 4), 1, vp(it.data_ptr()), 50, vp(out.data_ptr()), st)),
            ("C count_ahead_device q + 4", lambda: L.hac_index_count_ahead_device(one._h, vp(qt.data_ptr() + 4), 1, vp(St.data_ptr()), vp(it.data_ptr()), 50,
                                                                                   vp(out.data_ptr()), st)),
            ("C score_ids_device null", lambda: L.hac_index_score_ids_device(one._h, vp(), 1, vp(it.data_ptr()), 50, vp(out.data_ptr()), st)),
            ("C rank_ids null", lambda: L.hac_index_rank_ids(one._h, None, 1, ids.ctypes.data_as(i64p), 50, Ih.ctypes.data_as(i64p)))):
        refused(name, lambda: _lib.check(call()))
    torch.cuda.synchronize()
    one.check_status()
    idx.check_status()

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
