#!/usr/bin/env python3
"""Headline benchmark = BASELINE.json's metric: queries/sec of ANCE query encode + exact top-100
inner-product search over an N-passage 768-d corpus resident in HBM.

  python bench.py --gpus N --steps K --warmup W

A step = one pass of the hot path over one batch of synthetic input: encode 1000 tokenized queries
(L = 512, fully padded = what the reference computes, 12-layer RoBERTa-base ANCE, random-init weights) and
search their embeddings, top-100, over the resident corpus.

  N = 1   BASELINE configs[2]: 25M x 768 corpus in 8 passage blocks (76.8 GB resident), one MI355X.
  N > 1   BASELINE configs[3] shard size: every rank holds a 6.75M-row shard (N x 6.75M rows in all; N = 8
          is the 54M-row QReCC-scale corpus).  The 1000 queries are encoded data-parallel (1000/N per rank),
          one all-gather brings the embeddings to every rank, every rank searches its shard, ONE all-gather of
          the packed per-shard top-100 keys and an on-device merge finish the step on every rank ("weak":
          the corpus grows with N, a GPU's shard does not).
          Launch: either `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...` (RANK /
          WORLD_SIZE in the environment) or plain `python bench.py --gpus N`, which starts the N ranks itself
          BEFORE anything touches a GPU (children are separate processes, nothing is re-exec'ed).

Rank 0 prints ONE JSON line; DESIGN.md §5 has the roofline arithmetic.

A plain run does only what the headline needs: set up, warm up, time the K steps, print the line.  Everything else (the CPU
baseline, the extras of --extras, the N > 1 self-checks of the collective layer) runs with --full.
  --dump-outputs DIR   after the timed steps, rank 0 writes what the last timed step returned (query embeddings, top-k scores,
                       top-k ids) as DIR/<name>.npy in float32 / float64; the inputs are seeded, the same from run to run.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

D_EMB = 768
PEAK_HBM_GBS = 8000.0       # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
PEAK_F32_MFMA_TF = 157.3    # fp32-input MFMA dense peak
PEAK_F16_MFMA_TF = 2500.0   # fp16 / bf16 MFMA dense peak
CFG3_ROWS, CFG3_BLOCKS = 25_000_000, 8
CFG4_SHARD_ROWS = 6_750_000
NORTH_STAR_ROWS = 10_000_000
CH = 125_000                # rows per generator seed: the same corpus whatever the sharding


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=0, help="total corpus rows (default: 25M at N=1, N x 6.75M at N>1)")
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--query-len", type=int, default=512, help="padded query length (TopiOCQA: 512, QReCC: 256)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: the CPU baseline, the extras (--extras, default 'default') and, at N > 1, the "
                         "self-verification of the collective layer; without it the run is the headline step alone")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extras", action="store_true", help="only the headline step (profiling runs); = --extras none")
    ap.add_argument("--extras", choices=("none", "verify", "default", "full"), default=None,
                    help="what --full adds (default: 'default'; any other value than 'none' needs --full).  default: the step's parts, "
                         "kernel classes, north-star corpus, configs[1] / [3] / [4] shapes (finishes in ~2 min); full: + sustained 30-s "
                         "loops, the encoder batch sweep and peaked attention; verify: only the north-star corpus step with its N > 1 "
                         "self-verification; none: the headline step alone")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="rank 0 writes the last timed step's outputs to DIR/<name>.npy (float32 / float64)")
    ap.add_argument("--north-star-rows", type=int, default=NORTH_STAR_ROWS, help="tests only: a smaller north-star corpus for rehearsals")
    ap.add_argument("--search-only", action="store_true", help="BASELINE configs[1] style: pre-encoded embeddings, no encoder in the step")
    ap.add_argument("--dump-results", default=None, metavar="NPZ",
                    help="rank 0 writes the last timed step's query embeddings and merged (D, I) to this .npz (tests)")
    ap.add_argument("--spawn-selftest", type=int, default=None, metavar="RC",
                    help="tests only: every rank prints its RANK/WORLD_SIZE and exits (rank 1 with code RC); nothing touches a GPU")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.no_extras:
        args.extras = "none"
    if args.extras is None:
        args.extras = "default" if args.full else "none"
    elif args.extras != "none" and not args.full:
        ap.error(f"--extras {args.extras} needs --full")
    return args


# ------------------------------------------------------------------------------ N > 1 without a launcher
def spawn_ranks(n, argv):
    """`python bench.py --gpus N`: start the N ranks as child processes (one per GPU), wait, and fail if any fails.
    The parent never launches GPU work and never exec's: whatever torch.cuda.device_count() does to count the devices
    (amdsmi where present, else hipGetDeviceCount, which does initialise the runtime), the ranks are fresh child
    processes started with Popen."""
    if "--spawn-selftest" not in argv:
        import torch
        have = torch.cuda.device_count()
        if have < n and not (have >= 1 and os.environ.get("HAC_BENCH_REHEARSAL") == "1"):
            raise SystemExit(f"bench.py --gpus {n}: only {have} GPU(s) visible")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    import tempfile
    procs, errs = [], []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # every rank's stderr goes to a file of its own: forwarded when the rank ends, and quoted in the error line if it failed
        errs.append(tempfile.TemporaryFile(mode="w+", prefix=f"bench_rank{r}_", suffix=".err"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env, stderr=errs[-1]))
    rc, first_bad = 0, None
    alive = list(range(n))
    while alive:
        time.sleep(0.2)
        for r in list(alive):
            code = procs[r].poll()
            if code is None:
                continue
            alive.remove(r)
            if code != 0 and rc == 0:
                rc, first_bad = code, r
                for other in alive:          # a dead rank leaves the others waiting in a collective
                    procs[other].terminate()
    tails = {}
    for r in range(n):
        errs[r].seek(0)
        text = errs[r].read()
        errs[r].close()
        if text:
            sys.stderr.write(text if text.endswith("\n") else text + "\n")
        tails[r] = text[-2000:]
    if rc != 0:
        # the run's record says which rank failed and why (a per-rank failure must be readable from the line, not only an exit code)
        print(json.dumps({"error": f"rank {first_bad} of {n} exited with code {rc}; the other ranks were terminated", "n_gpus": n, "failed_rank": first_bad,
                          "exit_code": rc, "stderr_tail": tails.get(first_bad, "")}), flush=True)
    sys.exit(rc)


# ------------------------------------------------------------------------------ synthetic data
def gen_rows(seed, n, device):
    """Row-standardised Gaussian rows (||x|| = sqrt(768)), the shape of the ANCE head's output."""
    import torch
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn((n, D_EMB), generator=g, device=device, dtype=torch.float32)
    return (x - x.mean(1, keepdim=True)) / x.std(1, unbiased=False, keepdim=True)


def fill_index(index, lo, hi, dev, block_rows, keep_first=0):
    """Rows [lo, hi) of the global synthetic corpus, added block by block (one add() per passage block, as
    search_one_by_one_with_faiss does); returns the first keep_first rows on the host for the CPU baseline."""
    import torch
    kept = []
    for b0 in range(lo, hi, block_rows):
        b1 = min(hi, b0 + block_rows)
        blk = torch.empty((b1 - b0, D_EMB), dtype=torch.float32, device=dev)
        c = b0 // CH * CH
        while c < b1:
            a, e = max(b0, c), min(b1, c + CH)
            blk[a - b0:e - b0] = gen_rows(0xC0FFEE + c // CH, CH, dev)[a - c:e - c]
            c += CH
        index.add_tensor(blk)
        if keep_first > 0 and b0 < keep_first:
            kept.append(blk[:max(0, min(b1, keep_first) - b0)].cpu().numpy())
        torch.cuda.synchronize()
        del blk
    return kept


def timed(fn, reps, sync, barrier=None):
    fn()
    sync()
    if barrier:
        barrier()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    if barrier:
        barrier()
    return (time.perf_counter() - t0) / reps


def main():
    argv = sys.argv[1:]
    args = parse_args(argv)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        spawn_ranks(args.gpus, argv)          # never returns
    if args.spawn_selftest is not None:
        r = int(os.environ.get("RANK", "0"))
        print(f"selftest rank {r} of {os.environ.get('WORLD_SIZE')} local {os.environ.get('LOCAL_RANK')} port {os.environ.get('MASTER_PORT')}", flush=True)
        if r == 1 and args.spawn_selftest:
            sys.exit(args.spawn_selftest)
        time.sleep(1.0 if args.spawn_selftest else 0.0)   # a failing rank must bring the waiting ones down
        sys.exit(0)

    import numpy as np
    import torch
    import torch.distributed as dist

    t_begin = time.perf_counter()
    timeline = {}

    def mark(name):        # wall clock of this rank since its start (the driver allows the whole run 600 s)
        timeline[name] = round(time.perf_counter() - t_begin, 1)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py --gpus {args.gpus} launched with WORLD_SIZE={world}")
    # HAC_BENCH_REHEARSAL=1 (development only, the JSON line says so): the N ranks share the GPUs that are present and talk
    # over gloo -- RCCL refuses two ranks on one device -- so that the N > 1 control flow can be exercised on a 1-GPU box.
    rehearsal = world > 1 and os.environ.get("HAC_BENCH_REHEARSAL") == "1"
    if rehearsal:
        local_rank %= torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearsal:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            # a wedged rank must end the run with a non-zero code instead of hanging the node: the watchdog of the NCCL (= RCCL)
            # backend aborts the process when a collective has been pending this long; spawn_ranks() then terminates the others
            import datetime
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev,
                                    timeout=datetime.timedelta(seconds=int(os.environ.get("HAC_BENCH_NCCL_TIMEOUT_S", "240"))))

    from haconvdr_amd import synth
    from haconvdr_amd.encoder import ANCEEncoder
    from haconvdr_amd.index import FlatIPIndex
    from haconvdr_amd.sharded import ShardedSearcher, shard_range

    def sync():
        torch.cuda.synchronize()

    def barrier():
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    def max_over_ranks(v):
        if world == 1:
            return v
        t = torch.tensor([v], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    # ---- the workload ------------------------------------------------------------------------------------
    nq, k, Lq = args.nq, args.k, args.query_len
    if args.rows:
        rows, block_rows, wl_name = args.rows, max(CH, -(-args.rows // (CFG3_BLOCKS * world))), "custom"
    elif world == 1:
        rows, block_rows, wl_name = CFG3_ROWS, CFG3_ROWS // CFG3_BLOCKS, "BASELINE configs[2]"
    else:
        rows, block_rows, wl_name = CFG4_SHARD_ROWS * world, CFG4_SHARD_ROWS, "BASELINE configs[3] shard size"
    lo, hi = shard_range(rows, rank, world)
    n_local = hi - lo
    want_cpu = rank == 0 and world == 1 and args.full and not args.no_cpu_baseline
    index = FlatIPIndex(D_EMB, devices=(local_rank,))
    kept = fill_index(index, lo, hi, dev, block_rows, keep_first=1_000_000 if want_cpu else 0)
    searcher = ShardedSearcher(index, shard_base=lo)
    mark("corpus_resident")

    nq_loc = (nq + world - 1) // world                                   # queries are encoded data-parallel
    enc = None
    if not args.search_only:
        enc = ANCEEncoder.from_state_dict(synth.ance_state_dict(0xA11CE, 12, rich=False), device=local_rank)
        tok, _ = synth.token_batch(0x70C + rank, nq_loc, Lq, fixed_len=Lq)   # fully padded = the reference's behaviour
        ids_t = torch.from_numpy(tok.astype(np.int64)).to(dev)
        mask_t = torch.ones_like(ids_t)
    q_pre = gen_rows(0xBEEF, nq, dev)                                    # pre-encoded queries (search-only figures)
    allq = torch.empty((world * nq_loc, D_EMB), dtype=torch.float32, device=dev) if world > 1 else None

    last = {}

    def step(mask=None, srch=searcher):
        if enc is None:
            emb = q_pre
        else:
            emb = enc(ids_t, mask_t if mask is None else mask)
            last["local_emb"] = emb
            if world > 1:
                dist.all_gather_into_tensor(allq, emb)
                emb = allq[:nq]
        last["emb"] = emb
        return srch.search(emb, k)

    # ---- the timed region: W warm-up steps, then exactly K steps between barrier + synchronize ----------
    if world > 1:
        # communicator set-up (RCCL builds its rings / buffers with the first collective of each shape) and the
        # communicator-dependent allocations of the step happen HERE, whatever --warmup says
        if enc is not None:
            dist.all_gather_into_tensor(allq, torch.zeros((nq_loc, D_EMB), dtype=torch.float32, device=dev))
        warm_keys = torch.zeros((nq, k), dtype=torch.int64, device=dev)
        gath_keys = torch.empty((world * nq, k), dtype=torch.int64, device=dev)
        dist.all_gather_into_tensor(gath_keys, warm_keys)
        sync()
        collective = None
        if args.full:
            # Self-verification of the collective layer (nobody can rehearse the 8-GPU RCCL run): did the backend see N ranks, does an
            # all-gather deliver every rank's slab in rank order, and what do the step's two collectives cost by themselves
            ones = torch.ones(1, device=dev, dtype=torch.int64)
            dist.all_reduce(ones)
            warm_keys.fill_(rank + 1)
            dist.all_gather_into_tensor(gath_keys, warm_keys)
            slabs = gath_keys.view(world, -1)[:, 0].cpu().tolist()
            emb_probe = torch.zeros((nq_loc, D_EMB), dtype=torch.float32, device=dev)
            t_ag_emb = max_over_ranks(timed(lambda: dist.all_gather_into_tensor(allq, emb_probe), 10, sync, barrier)) if enc is not None else None
            t_ag_keys = max_over_ranks(timed(lambda: dist.all_gather_into_tensor(gath_keys, warm_keys), 10, sync, barrier))
            collective = {"backend": dist.get_backend(), "world": world, "ranks_seen": int(ones.item()),
                          "allgather_slabs_in_rank_order": slabs == list(range(1, world + 1)),
                          "allgather_emb_ms": None if t_ag_emb is None else round(t_ag_emb * 1e3, 4), "allgather_emb_bytes_per_rank": nq_loc * D_EMB * 4,
                          "allgather_keys_ms": round(t_ag_keys * 1e3, 4), "allgather_keys_bytes_per_rank": nq * k * 8,
                          "devices": f"rank {rank} on cuda:{local_rank} of {torch.cuda.device_count()} visible"}
            del emb_probe
        del gath_keys
    for _ in range(args.warmup):
        step()
    index.set_profiling(True)
    if enc is not None:
        enc.set_profiling(True, classes="all")      # an event pair around every encoder launch of the timed steps (~2 x 80 per step)
    sync()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        D, I = step()
    sync()
    barrier()
    dt = max_over_ranks(time.perf_counter() - t0)
    mark("timed_steps_done")
    # the shader clock the part sustained inside the last FFN-up launch of the timed steps (boxes of one pool differ by several
    # percent on the same binary: this is the figure to normalise fractions of a peak by); None without an encoder
    clk_read = enc.last_clock_mhz() if enc is not None else None
    shader_mhz, clk_seconds = clk_read if clk_read else (None, 0.0)    # (None: no large-batch FFN-up launch ran with class profiling on)
    scan_ms = index.profile_drain()
    plan = index.last_plan()
    enc_plan = enc.last_plan() if enc is not None else None
    timed_emb = last["local_emb"].clone() if enc is not None else None      # this rank's embeddings of the last timed step
    if args.dump_results and rank == 0:
        np.savez(args.dump_results, emb=last["emb"].cpu().numpy(), D=D.cpu().numpy(), I=I.cpu().numpy(), rows=rows, k=k, block_rows=block_rows)
    if args.dump_outputs and rank == 0:
        # what a caller of the step receives from its last timed run: the merged top-k (scores fp32, ids as float64: exact for any
        # row count) and, when the step encodes, the query embeddings that were searched
        dump = {"topk_scores": D.cpu().numpy().astype(np.float32), "topk_ids": I.cpu().numpy().astype(np.float64)}
        if enc is not None:
            dump["query_embeddings"] = last["emb"].cpu().numpy().astype(np.float32)
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, arr in dump.items():
            np.save(os.path.join(args.dump_outputs, name + ".npy"), arr)
    index.set_profiling(False)
    stack_ms, ffn_up_ms, class_ms = [], [], {}
    if enc is not None:
        stack_ms = enc.profile_drain()
        class_ms = {name: enc.profile_drain_class(name) for name in enc.KERNEL_CLASSES}
        ffn_up_ms = class_ms["ffn_up"]
        enc.set_profiling(False)
    index.check_status()        # a scan that gave up at its pass bound would be HAC_ERR_INTERNAL here (never seen; hang-proofing)
    ms_per_step = dt / args.steps * 1e3
    value = nq * args.steps / dt

    # ---- rooflines (algorithmic figures of SURVEY.md §8d; kernel times = hipEvent brackets inside the timed region)
    prof = load_profile_traffic()

    def pmc(name):
        return None if prof["stale"] else prof["data"].get(name)

    scan_avg_ms = float(np.sum(scan_ms)) / args.steps if scan_ms else float("nan")
    s_bytes = n_local * D_EMB * 4 + nq * D_EMB * 4 + nq * k * 12
    s_flops = 2.0 * nq * n_local * D_EMB
    s_tf = s_flops / (scan_avg_ms * 1e-3) / 1e12
    s_gbs = s_bytes / (scan_avg_ms * 1e-3) / 1e9
    if plan.startswith("split:"):
        terms = int(plan.split("scanh_kernel<")[1].split(">")[0])
        search_roof = {"kernel": f"scanh_kernel<{terms}>", "plan": plan, "bound": "mfma", "achieved": round(s_tf, 2), "peak": PEAK_F16_MFMA_TF,
                       "unit": "TFLOP/s", "frac": round(s_tf / PEAK_F16_MFMA_TF, 4), "kernel_ms": round(scan_avg_ms, 4),
                       "executed_TFLOPs": round(terms * s_tf, 2), "vs_fp32_mfma_peak": round(s_tf / PEAK_F32_MFMA_TF, 3),
                       "hbm_GBps_same_kernel": round(s_gbs, 1),
                       "note": "fp16-MFMA prefilter under a proven error bound + exact fp32 rescoring (results are the fp32 results); "
                               "achieved = algorithmic 2*nq*n*768 flop / the hipEvent bracket around all scanh launches of a search (seeding pass, threshold "
                               "selections and up to three passes over consecutive row ranges); traffic = HBM bytes of the main passes per search"}
    elif (s_flops / s_bytes) > (PEAK_F32_MFMA_TF * 1e12) / (PEAK_HBM_GBS * 1e9):
        search_roof = {"kernel": plan.split(" ")[0], "plan": plan, "bound": "mfma", "achieved": round(s_tf, 2), "peak": PEAK_F32_MFMA_TF,
                       "unit": "TFLOP/s", "frac": round(s_tf / PEAK_F32_MFMA_TF, 4), "kernel_ms": round(scan_avg_ms, 4)}
    else:
        search_roof = {"kernel": plan.split(" ")[0], "plan": plan, "bound": "hbm", "achieved": round(s_gbs, 1), "peak": PEAK_HBM_GBS,
                       "unit": "GB/s", "frac": round(s_gbs / PEAK_HBM_GBS, 4), "kernel_ms": round(scan_avg_ms, 4)}
    search_roof["traffic"] = pmc("search_hbm_bytes_per_launch") if (world == 1 and rows == CFG3_ROWS) else None
    traffic_note = {"traffic_source": prof["note"]}
    if prof["stale"]:
        traffic_note["traffic_stale"] = prof["stale"]

    def mfma_util(needle):
        """Matrix-pipe busy share etc. of a kernel from the committed rocprofv3 SQ pass (profiles/r02_sq.*), same workload."""
        u = pmc("mfma_util") or {}
        for kname, v in u.items():
            if needle in kname and "short" not in kname:
                return dict(v, source=f"profiles/{prof['tag']}_sq.json (rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES ... GRBM_GUI_ACTIVE pass of this bench)")
        return None
    if world == 1 and rows == CFG3_ROWS:
        search_roof["mfma_util"] = mfma_util("scanh_kernel<1, false, 16>")

    T_tok = nq_loc * Lq                                                   # padded tokens a rank encodes per step
    enc_flops = nq_loc * 12.0 * (14155776.0 * Lq + 4.0 * Lq * Lq * 768.0) + nq_loc * 2.0 * 768 * 768
    if enc is not None and ffn_up_ms:
        # dominant kernel of the step: the FFN-up GEMM (768 -> 3072, bias + erf-GELU fused), 11 layers x sub-batches per
        # forward (the last layer runs its FFN on the <s> rows only).  Algorithmic flops per launch = 2 * M * 768 * 3072.
        n_launch = len(ffn_up_ms)
        fl_launch = 11 * args.steps * 2.0 * T_tok * 768 * 3072 / n_launch
        avg_ms = float(np.mean(ffn_up_ms))
        tf = fl_launch / (avg_ms * 1e-3) / 1e12
        stack_avg = float(np.sum(stack_ms)) / args.steps
        roofline = {"kernel": "gemm8_kernel<EPI8_GELU> (FFN-up 768->3072: folded LayerNorm + bias + erf-GELU fused)", "bound": "mfma",
                    "achieved": round(tf, 1), "peak": PEAK_F16_MFMA_TF, "unit": "TFLOP/s", "frac": round(tf / PEAK_F16_MFMA_TF, 4),
                    "traffic": pmc("ffn_up_hbm_bytes_per_launch") if world == 1 else None,
                    "mfma_util": mfma_util("gemm8_kernel<3,") if world == 1 else None,
                    "kernel_ms": round(avg_ms, 4), "launches_per_step": n_launch // args.steps, "flops_per_launch": fl_launch,
                    "share_of_step": round(avg_ms * (n_launch / args.steps) / ms_per_step, 3),
                    "encoder_stack": {"ms_per_step": round(stack_avg, 3), "achieved_TFLOPs": round(enc_flops / (stack_avg * 1e-3) / 1e12, 1),
                                      "mfma_bf16_frac": round(enc_flops / (stack_avg * 1e-3) / 2.5e15, 4),
                                      "flops": "12 x (14,155,776 T + 4 T^2 768) + 2 x 768^2 per padded query, SURVEY 8d"},
                    "encoder_plan": enc_plan, "search": search_roof}
        # the same fractions against the peak at the clock the part actually held (2.5 PF dense bf16 / fp16 is quoted at 2.4 GHz)
        if shader_mhz:
            clk_scale = shader_mhz / 2400.0
            roofline["sustained_shader_clock_MHz"] = round(shader_mhz, 1)
            roofline["frac_of_clock_held_peak"] = round(tf / (PEAK_F16_MFMA_TF * clk_scale), 4)
            roofline["encoder_stack"]["mfma_bf16_frac_of_clock_held_peak"] = round(enc_flops / (stack_avg * 1e-3) / (2.5e15 * clk_scale), 4)
            if search_roof.get("bound") == "mfma" and search_roof.get("peak") == PEAK_F16_MFMA_TF:
                search_roof["frac_of_clock_held_peak"] = round(search_roof["frac"] / clk_scale, 4)
            roofline["clock_note"] = ("sustained_shader_clock_MHz = d(s_memtime) / d(s_memrealtime) x 100 MHz between the first and the last instruction of "
                                      f"workgroup 0 of the LAST FFN-up launch of the timed steps ({clk_seconds * 1e3:.3f} ms; hac_encoder_last_clock); "
                                      "*_of_clock_held_peak = the same achieved rate over peak x clock / 2400 MHz")
        else:
            roofline["sustained_shader_clock_MHz"] = None
        # every kernel class of the step, from the event pairs of the TIMED steps: per-step time, share of the step, fraction of
        # the 2.5 PF bf16 / fp16 peak -- so that "dominant" can be checked from this line alone
        fl_step = {"qkv": 2.0 * T_tok * 768 * 2304 * 12, "out_proj": 2.0 * T_tok * 768 * 768 * 11, "ffn_up": 2.0 * T_tok * 768 * 3072 * 11,
                   "ffn_down": 2.0 * T_tok * 3072 * 768 * 11, "attention": 4.0 * Lq * 768 * T_tok * 12}
        kname = {"qkv": "gemm8_kernel<EPI8_QKV>", "out_proj": "gemm8_kernel<EPI8_RESID> K=768", "ffn_up": "gemm8_kernel<EPI8_GELU>",
                 "ffn_down": "gemm8_kernel<EPI8_RESID> K=3072", "attention": "attention_pipe_kernel<8> + attention_stream_kernel<16|8> (woven form for whole long items, the one-block form for the rest)",
                 "layernorm": "ln_combine_kernel"}
        kernels = []
        for name, msl in class_ms.items():
            if not msl:
                continue
            per_step = float(np.sum(msl)) / args.steps
            ent = {"class": name, "kernel": kname.get(name, name), "ms_per_step": round(per_step, 3), "launches_per_step": len(msl) // args.steps,
                   "share_of_step": round(per_step / ms_per_step, 3)}
            if name in fl_step:
                ent["frac_of_2.5PF"] = round(fl_step[name] / (per_step * 1e-3) / 2.5e15, 4)
            kernels.append(ent)
        if "kernel_ms" in search_roof:
            # scan launches inside the bracket: seeding pass + the main scan's passes (plan text), or the one exact-kernel scan
            scan_launches = (int(plan.split("seed=")[1].split()[0]) + int(plan.split("passes=")[1].split()[0])) if "passes=" in plan else 1
            kernels.append({"class": "search_scan", "kernel": search_roof["kernel"], "ms_per_step": search_roof["kernel_ms"], "launches_per_step": scan_launches,
                            "share_of_step": round(search_roof["kernel_ms"] / ms_per_step, 3),
                            ("frac_of_2.5PF" if search_roof["bound"] == "mfma" and search_roof["peak"] == PEAK_F16_MFMA_TF else "frac"): search_roof["frac"]})
        resid = sum(e["ms_per_step"] for e in kernels if e["class"] in ("out_proj", "ffn_down"))
        kernels.sort(key=lambda e: -e["ms_per_step"])
        roofline["kernels"] = kernels
        # The top-level roofline object describes the LARGEST kernel of the step (the line used to present FFN-up as "the
        # dominant kernel" while its own note said the prefilter scan was larger); the largest encoder GEMM class stays beside it.
        if kernels[0]["class"] == "search_scan":
            enc_dom = {key: roofline.pop(key) for key in ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "mfma_util", "kernel_ms",
                                                          "launches_per_step", "flops_per_launch", "share_of_step", "frac_of_clock_held_peak") if key in roofline}
            roofline.pop("search")
            top = dict(search_roof)
            top["share_of_step"] = kernels[0]["share_of_step"]
            top["launches_per_step"] = kernels[0]["launches_per_step"]
            top.update(roofline)
            roofline = top
            roofline["encoder_dominant"] = enc_dom
            roofline["dominant_note"] = (f"largest per step: {kernels[0]['kernel']} ({kernels[0]['ms_per_step']} ms) = this object's kernel / achieved / peak / frac; "
                                         f"encoder_dominant = FFN-up, the largest encoder class ({enc_dom['kernel_ms']} ms x {enc_dom['launches_per_step']}); "
                                         f"gemm8_kernel<EPI8_RESID> as ONE instantiation (out-proj + FFN-down) {round(resid, 3)} ms")
        else:
            roofline["dominant_note"] = (f"largest per step: {kernels[0]['kernel']} ({kernels[0]['ms_per_step']} ms); gemm8_kernel<EPI8_RESID> as ONE "
                                         f"instantiation (out-proj + FFN-down) {round(resid, 3)} ms")
    else:
        roofline = search_roof
    roofline.update(traffic_note)

    out = {
        "metric": "queries/sec (encode+top-100) over N-passage 768-d corpus; HBM GB/s vs peak" if enc is not None
                  else "queries/sec (top-100 exact IP search, pre-encoded embeddings) over N-passage 768-d corpus",
        "value": round(value, 1), "unit": "queries/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "bf16 MFMA operands with fp32 accumulate / LayerNorm / softmax in the encoder (cosine vs the fp32 reference within 1e-3, "
                 "measured ~1e-5); search scores and order = the fp32 fmaf chain, bit-exact" if enc is not None else "f32",
        "data": "synthetic",
        "config": {"workload": f"{wl_name}: " + ("" if enc is None else f"ANCE query encode ({nq} queries/step, L={Lq} fully padded, 12 layers, random-init) + ")
                               + f"exact top-{k} over a {rows}x768 fp32 corpus resident in HBM"
                               + (f" in {-(-rows // block_rows)} passage blocks, one GPU" if world == 1 else
                                  f", {world} shards of {n_local} rows, queries encoded data-parallel, all-gather of embeddings and of packed top-k keys"),
                   "corpus_rows": rows, "rows_per_gpu": n_local, "queries_per_step": nq, "query_len": Lq, "k": k,
                   "parallelism": f"corpus sharded {world}-way (weak: {n_local} rows per GPU), encode data-parallel" if world > 1 else "single GPU",
                   "per_gpu_rows": n_local,
                   "series_note": ("N = 1 runs BASELINE configs[2] (25M rows on ONE GPU), N > 1 runs configs[3]'s shard size (6.75M rows per GPU, the "
                                   "corpus grows with N, the 1000 queries per step do not): value(N) / value(1) compares DIFFERENT workloads.  "
                                   "The same-workload anchor of the N > 1 series is extras.cfg4_shard_step of the N = 1 line (full step over ONE "
                                   "6.75M-row shard); extras.north_star_10M is like-for-like at every N (strong scaling).")},
        "roofline": roofline,
        "cpu_baseline": None,
    }
    if world > 1:
        out["like_for_like_n1"] = "extras.cfg4_shard_step.queries_per_sec of the N = 1 line (one 6.75M-row shard, all 1000 queries encoded on that GPU)"
        if collective is not None:
            out["collective"] = collective
            if collective["ranks_seen"] != world or not collective["allgather_slabs_in_rank_order"]:
                out["collective"]["error"] = "the process group did not deliver every rank's contribution in rank order"
    if rehearsal:
        out["rehearsal"] = f"NOT a measurement: {world} ranks share {torch.cuda.device_count()} GPU(s) over gloo (HAC_BENCH_REHEARSAL=1)"
    extras = {}

    # ---- CPU baseline (rank 0, N = 1): the oracle on the host cores, bounded sample of the same workload ----
    if want_cpu:
        out["cpu_baseline"] = cpu_baseline(np, torch, synth, enc, D, I, q_pre, kept, rows, nq, k, Lq, tok if enc is not None else None,
                                           timed_emb.cpu().numpy() if timed_emb is not None else None, enc_plan)
    kept = None

    ns_rows = args.north_star_rows
    if args.extras != "none":
        # ---- the step's parts, and the same step with the queries' real lengths ------------------------
        if enc is not None and args.extras != "verify":
            t_enc = max_over_ranks(timed(lambda: enc(ids_t, mask_t), 3, sync, barrier))
            emb_now = enc(ids_t, mask_t)
            if world > 1:
                dist.all_gather_into_tensor(allq, emb_now)
                emb_now = allq[:nq].clone()
            t_srch = max_over_ranks(timed(lambda: searcher.search(emb_now, k), 3, sync, barrier))
            extras["step_parts"] = {"encode_ms": round(t_enc * 1e3, 3), "search_ms": round(t_srch * 1e3, 3),
                                    "encode_queries_per_sec_per_gpu": round(nq_loc / t_enc, 1),
                                    "search_queries_per_sec": round(nq / t_srch, 1)}
            # queries with their real lengths (uniform in [64, L], prefix mask): the reference computes
            # the padding too, this encoder only the real tokens (varlen packing)
            qlens = 64 + (synth.uniform_u32(0x91E45 + rank, nq_loc) % np.uint32(max(1, Lq - 64 + 1))).astype(np.int64)
            qvar = (torch.arange(Lq, device=dev)[None, :] < torch.from_numpy(qlens).to(dev)[:, None]).to(torch.int64)
            t_var = max_over_ranks(timed(lambda: step(qvar), 3, sync, barrier))
            extras["real_query_lengths"] = {"queries_per_sec": round(nq / t_var, 1), "ms_per_step": round(t_var * 1e3, 3),
                                            "mean_len": round(float(qlens.mean()), 1), "lens": f"uniform in [64, {Lq}], prefix mask"}
            # every kernel class of the encoder (hipEvent pairs around each launch; untimed pass)
            # (median of three forwards: one sample is not a measurement -- a committed r05 line carried a 57 ms FFN-up hiccup)
            enc.set_profiling(True, classes="all")
            stacks, samples = [], {name: [] for name in enc.KERNEL_CLASSES}
            launches = {}
            for _ in range(3):
                enc(ids_t, mask_t)
                sync()
                stacks.append(float(np.sum(enc.profile_drain())))
                for name in enc.KERNEL_CLASSES:
                    ms = enc.profile_drain_class(name)
                    if ms:
                        samples[name].append(float(np.sum(ms)))
                        launches[name] = len(ms)
            enc.set_profiling(False)
            stack = float(np.median(stacks))
            per_class = {}
            fl_class = {"qkv": 2.0 * T_tok * 768 * 2304 * 12, "out_proj": 2.0 * T_tok * 768 * 768 * 11, "ffn_up": 2.0 * T_tok * 768 * 3072 * 11,
                        "ffn_down": 2.0 * T_tok * 3072 * 768 * 11, "attention": 4.0 * Lq * 768 * T_tok * 12}
            for name in enc.KERNEL_CLASSES:
                if not samples[name]:
                    continue
                tot = float(np.median(samples[name]))
                per_class[name] = {"ms_per_forward": round(tot, 3), "launches": launches[name], "min_max_ms": [round(min(samples[name]), 3), round(max(samples[name]), 3)]}
                if name in fl_class:
                    per_class[name]["achieved_TFLOPs"] = round(fl_class[name] / (tot * 1e-3) / 1e12, 1)
                    per_class[name]["mfma_bf16_frac"] = round(fl_class[name] / (tot * 1e-3) / 2.5e15, 4)
            extras["encoder_kernels"] = {"layer_stack_ms": round(stack, 3), "per_class": per_class, "attention_form": enc.last_plan().split("attn_form=")[-1].split()[0],
                                         "note": "median of three forwards of this rank's queries with an event pair around every launch"}
        # ---- the north-star corpus: 10M x 768 over the N GPUs, same step ----------------------------------
        if rows != ns_rows:
            lo2, hi2 = shard_range(ns_rows, rank, world)
            idx2 = FlatIPIndex(D_EMB, devices=(local_rank,))
            fill_index(idx2, lo2, hi2, dev, -(-ns_rows // (CFG3_BLOCKS * world)))
            srch2 = ShardedSearcher(idx2, shard_base=lo2)
            for _ in range(2):                   # (lazy images of a fresh index: fp16 with the first prefilter search, row-major copy with the third)
                srch2.search(q_pre, k)
            t_ns = max_over_ranks(timed(lambda: step(None, srch2), 3, sync, barrier))
            extras["north_star_10M"] = {"queries_per_sec": round(nq / t_ns, 1), "ms_per_step": round(t_ns * 1e3, 3),
                                        "what": f"same step over a {ns_rows}x768 corpus on {world} GPU(s) ({hi2 - lo2} rows per GPU); "
                                                "BASELINE.json north_star target: >= 3000 queries/s on 8 GPUs"}
            if world > 1:
                # Self-verification of the sharded result: the 10M rows regenerate from seeds and fit ONE GPU, so rank 0 searches
                # them whole with the exact fp32 kernels (split = "0": no prefilter, no collective, no merge) for eight fixed
                # queries of the step and compares with the merged (D, I) the N-rank step returned for those queries
                Dn, In = step(None, srch2)
                qv = last["emb"][:8].clone()
                sync()
                barrier()
                del idx2, srch2
                verify = None
                if rank == 0:
                    idx_all = FlatIPIndex(D_EMB, devices=(local_rank,))
                    fill_index(idx_all, 0, ns_rows, dev, -(-ns_rows // CFG3_BLOCKS))
                    idx_all.set_option("split", "0")
                    Dv, Iv = idx_all.search_tensor(qv, k)
                    sync()
                    verify = {"queries": 8, "rows": ns_rows, "referee": "one GPU, exact fp32 kernels (" + idx_all.last_plan().split(" ")[0] + ")",
                              "ids_equal": bool(torch.equal(Iv, In[:8])), "scores_equal": bool(torch.equal(Dv, Dn[:8]))}
                    del idx_all
                barrier()
                extras["north_star_10M"]["verify"] = verify
                # the like-for-like anchor of this series, measured on these very GPUs: the FULL step -- all nq queries encoded on
                # this GPU, searched over this GPU's shard, no collective -- i.e. what the N = 1 line calls cfg4_shard_step
                if enc is not None:
                    tok_all, _ = synth.token_batch(0x70C, nq, Lq, fixed_len=Lq)
                    ids_all = torch.from_numpy(tok_all.astype(np.int64)).to(dev)
                    mask_all = torch.ones_like(ids_all)
                    from haconvdr_amd.index import keys_to_results

                    def local_step():
                        return keys_to_results(index.search_keys_tensor(enc(ids_all, mask_all), k, pos_base=lo))
                    t_loc = timed(local_step, 3, sync)
                    rate = torch.tensor([nq / t_loc], device=dev, dtype=torch.float64)
                    rmin, rmax = rate.clone(), rate.clone()
                    dist.all_reduce(rmin, op=dist.ReduceOp.MIN)
                    dist.all_reduce(rmax, op=dist.ReduceOp.MAX)
                    extras["cfg4_shard_step"] = {"queries_per_sec": round(nq / t_loc, 1), "ms_per_step": round(t_loc * 1e3, 3), "rows_per_gpu": n_local,
                                                 "queries_per_step": nq, "min_over_ranks": round(float(rmin.item()), 1), "max_over_ranks": round(float(rmax.item()), 1),
                                                 "what": "the N = 1 anchor of this series measured on THIS run's GPUs: every rank encodes all the step's queries and "
                                                         "searches its own shard (rows_per_gpu; 6.75M at the default size), no collective (rank 0's figure; min / max over the ranks beside it)"}
                    del ids_all, mask_all
            else:
                del idx2, srch2
        if world == 1 and enc is not None and rows == CFG3_ROWS and args.extras != "verify":
            # BASELINE configs[3] on ONE of its eight ranks, part by part (the 8-GPU run is the driver's): encode 1000 / 8
            # queries, search all 1000 over a 6.75M-row shard.  The two all-gathers between them (3 MB of embeddings, 0.8 MB
            # of packed keys per rank) are not in these figures.
            idx4 = FlatIPIndex(D_EMB, devices=(local_rank,))
            fill_index(idx4, 0, CFG4_SHARD_ROWS, dev, -(-CFG4_SHARD_ROWS // CFG3_BLOCKS))
            n8 = nq // 8
            t_e8 = timed(lambda: enc(ids_t[:n8], mask_t[:n8]), 5, sync)
            emb8 = enc(ids_t, mask_t)
            for _ in range(3):
                ShardedSearcher(idx4, shard_base=0).search(emb8, k)
            t_s8 = timed(lambda: ShardedSearcher(idx4, shard_base=0).search(emb8, k), 5, sync)
            extras["cfg4_one_rank_parts"] = {"encode_ms": round(t_e8 * 1e3, 3), "encode_queries": n8, "search_ms": round(t_s8 * 1e3, 3),
                                             "shard_rows": CFG4_SHARD_ROWS, "sum_ms": round((t_e8 + t_s8) * 1e3, 3),
                                             "what": "one rank's work of the N = 8 step (54M-row corpus): NOT a measurement of the 8-GPU step, "
                                                     "which adds two small all-gathers and is the driver's to run"}
            # the same-workload anchor of the N > 1 series: the FULL step (encode all 1000 queries, search, keys -> results)
            # over ONE 6.75M-row shard on this GPU = what `bench.py --gpus N` times per rank, with N = 1
            srch4 = ShardedSearcher(idx4, shard_base=0)
            t_c4 = timed(lambda: step(None, srch4), 5, sync)
            extras["cfg4_shard_step"] = {"queries_per_sec": round(nq / t_c4, 1), "ms_per_step": round(t_c4 * 1e3, 3), "rows_per_gpu": CFG4_SHARD_ROWS,
                                         "queries_per_step": nq, "what": "like-for-like N = 1 anchor of the N > 1 series (BASELINE configs[3] shard size): "
                                                                         "encode 1000 queries (L = 512) + top-100 over one 6.75M-row shard"}
            del idx4, srch4
        if world == 1 and args.extras != "verify":
            extras.update(single_gpu_extras(np, torch, synth, FlatIPIndex, enc, index, q_pre, dev, n_local, nq, k, sync))
            if enc is not None and nq >= 1000 and Lq == 512:
                # the reference's literal call shapes (B = 4 x 512 and the first rows of the sweep) stay in the default line; the
                # whole sweep, the 30-s sustained loops and the peaked-attention series are `--extras full` (they took the default
                # run from 113 s to 222 s of the driver's 600-s limit in round 4)
                extras["encoder_batch_sweep"] = encoder_batch_sweep(np, torch, synth, enc, dev, sync, full=args.extras == "full")
                if args.extras == "full":
                    extras["sustained"] = sustained(np, torch, synth, enc, step, nq, dev, sync)
                    extras["attention_peaked"] = attention_peaked(np, torch, synth, enc, ids_t, mask_t, nq, Lq, sync)
            extras["three_call_protocol"] = three_call_protocol(np, torch, FlatIPIndex, q_pre, dev, k)
        elif enc is not None and args.extras != "verify":
            # BASELINE configs[4] shape on N GPUs: passage encoding is embarrassingly parallel (every rank encodes the blocks it
            # owns, no collective): each rank times 1000 synthetic passages of L = 384, the job rate is the sum over ranks
            Bp, Lp = 1000, 384
            ptok, _ = synth.token_batch(0xD0C + rank, Bp, Lp, fixed_len=Lp)
            plens = np.clip(np.rint(180.0 + 80.0 * synth.normal(0x1E45 + rank, (Bp,))), 8, Lp).astype(np.int64)
            pid_t = torch.from_numpy(ptok.astype(np.int64)).to(dev)
            masks = {"padded": torch.ones_like(pid_t),
                     "varlen": (torch.arange(Lp, device=dev)[None, :] < torch.from_numpy(plens).to(dev)[:, None]).to(torch.int64)}
            psg = {"batch_per_gpu": Bp, "gpus": world}
            for name, m in masks.items():
                rate = torch.tensor([Bp / timed(lambda: enc(pid_t, m), 3, sync, barrier)], device=dev, dtype=torch.float64)
                lo_rate = rate.clone()
                dist.all_reduce(rate, op=dist.ReduceOp.SUM)
                dist.all_reduce(lo_rate, op=dist.ReduceOp.MIN)
                psg[f"docs_per_sec_{name}"] = round(float(rate.item()), 1)
                psg[f"docs_per_sec_per_gpu_{name}_min"] = round(float(lo_rate.item()), 1)
            psg["mfma_bf16_frac_padded"] = round(12.0 * (14155776.0 * Lp + 4.0 * Lp * Lp * 768.0) * psg["docs_per_sec_padded"] / world / 2.5e15, 4)
            psg["block_ownership"] = passage_block_ownership_check(np, torch, dist, synth, enc, rank, world, barrier)
            extras["passages_L384"] = psg

    failed = None
    if rank == 0:
        out.update(extras)
        mark("extras_done")
        out["wall_clock_s"] = dict(timeline, note="rank 0, since the process started (python + torch import included from 'corpus_resident' on); the driver's limit for the run is 600 s")
        print(json.dumps(out), flush=True)
        v = (extras.get("north_star_10M") or {}).get("verify")
        if v is not None and not (v["ids_equal"] and v["scores_equal"]):
            failed = "the sharded step's merged (D, I) differ from the single-GPU exact search (north_star_10M.verify)"
        if world > 1 and "error" in out.get("collective", {}):
            failed = out["collective"]["error"]
        own = (extras.get("passages_L384") or {}).get("block_ownership")
        if own is not None and not own["every_block_once_by_its_owner"]:
            failed = "passage blocks were not written exactly once, each by its owner (passages_L384.block_ownership)"
    if world > 1:
        dist.destroy_process_group()
    if failed:
        raise SystemExit("bench.py: " + failed)       # after the JSON line: the record shows what was measured AND that it is wrong


def passage_block_ownership_check(np, torch, dist, synth, enc, rank, world, barrier):
    """configs[4] on N ranks has no collective: rank r encodes and writes the blocks b = r (mod N) (haconvdr_amd/passages.py:
    encode_passages, the mirror of gen_doc_embeddings.py:65-158, whose DataParallel loop writes every block from one process).  The
    self-check of that split, since nobody can rehearse the 8-GPU run: a small synthetic collection (2 N + 1 blocks of 64 passages, the
    last one short) goes through the real loop on every rank, each rank into a directory of its own; then every block must exist
    exactly once, in its owner's directory, with the ids of its range."""
    import shutil
    import tempfile
    from haconvdr_amd import passages as P

    class Collection:            # what encode_passages needs of TokenizedPassages: len() and batch(lo, hi) -> (ids int32 [m, L], lens int64 [m])
        def __init__(self, n, L):
            self.tok, _ = synth.token_batch(0xB10C, n, L, fixed_len=L)
            self.lens = 8 + (synth.uniform_u32(0xB10D, n) % np.uint32(L - 8 + 1)).astype(np.int64)

        def __len__(self):
            return len(self.lens)

        def batch(self, lo, hi):
            ids = self.tok[lo:hi].copy()
            ids[np.arange(ids.shape[1])[None, :] >= self.lens[lo:hi, None]] = 0
            return ids.astype(np.int32), self.lens[lo:hi]
    n_blocks, per_block = 2 * world + 1, 64
    n = (n_blocks - 1) * per_block + 17
    coll = Collection(n, 64)
    root = [os.path.join(tempfile.gettempdir(), f"hac_bench_blocks_{os.environ.get('MASTER_PORT', '0')}_{os.getppid()}")]   # (one node: the ranks see the same path)
    if rank == 0:
        shutil.rmtree(root[0], ignore_errors=True)
        os.makedirs(root[0])
    barrier()
    mine = os.path.join(root[0], f"rank{rank}")
    wrote = P.encode_passages(enc, coll, mine, per_gpu_eval_batch_size=32, n_gpu=1, rank=rank, world_size=world, expect_per_block_passage_num=per_block)
    barrier()
    res = None
    if rank == 0:
        problems, total = [], 0
        for b in range(n_blocks):
            holders = [r for r in range(world) if os.path.exists(os.path.join(root[0], f"rank{r}", f"passage_emb_block_{b}.pb"))]
            if holders != [b % world]:
                problems.append(f"block {b}: written by ranks {holders}, owner {b % world}")
                continue
            emb, ids = P.read_embedding_block(os.path.join(root[0], f"rank{b % world}"), b)
            lo, hi = b * per_block, min(n, (b + 1) * per_block)
            total += len(ids)
            if not (np.array_equal(np.asarray(ids), np.arange(lo, hi)) and emb.shape == (hi - lo, D_EMB) and np.isfinite(emb).all()):
                problems.append(f"block {b}: ids / shape / values")
        res = {"blocks": n_blocks, "passages": n, "passages_in_blocks": total, "rank0_wrote": int(wrote), "every_block_once_by_its_owner": not problems and total == n}
        if problems:
            res["problems"] = problems[:8]
        shutil.rmtree(root[0], ignore_errors=True)
    barrier()
    return res


# ------------------------------------------------------------------------------ committed PMC passes (roofline.traffic)
KERNEL_SOURCES = ("flat_ip.hip", "scan_split.inc", "encoder.hip", "gemm8.inc", "attn_pipe.inc")


def kernel_sources_sha256():
    """One digest over the four kernel sources of the running tree (what tools/refresh_profiles.py stamps a campaign with)."""
    import hashlib
    h = hashlib.sha256()
    for name in KERNEL_SOURCES:
        with open(os.path.join(ROOT, "haconvdr_amd", "csrc", name), "rb") as f:
            h.update(name.encode() + b"\0" + f.read())
    return h.hexdigest()


def load_profile_traffic():
    """The newest committed profiles/rNN_pmc_traffic.json (HBM bytes per launch and matrix-pipe busy share from separate
    rocprofv3 --pmc passes of this bench, tools/profile_round.sh).  Those numbers belong to the kernels they were measured
    on: the campaign is stamped with the digest of the kernel sources, and when the running tree's differs the line
    carries traffic = null and says why instead of quoting another kernel's counters."""
    import glob
    paths = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_pmc_traffic.json")), reverse=True)
    if not paths:
        return {"data": {}, "tag": None, "stale": "no committed PMC pass", "note": "none"}
    tag = os.path.basename(paths[0])[:3]
    try:
        data = json.load(open(paths[0]))
    except Exception as ex:
        return {"data": {}, "tag": tag, "stale": f"{paths[0]}: {ex!r}", "note": "none"}
    have, now = data.get("kernel_sources_sha256"), kernel_sources_sha256()
    note = (f"profiles/{tag}_pmc_traffic.json: separate rocprofv3 --pmc passes of this bench (FETCH_SIZE x 1024 x 2, WRITE_SIZE x 1024), "
            f"git {data.get('git_head', '?')}, kernel sources {str(have)[:12]}")
    stale = None
    if have != now:
        stale = (f"the committed PMC passes ({tag}) were taken on kernel sources {str(have)[:12]}, this tree is {now[:12]}: "
                 "traffic / mfma_util withheld until tools/profile_round.sh is re-run")
    return {"data": data, "tag": tag, "stale": stale, "note": note}


# ------------------------------------------------------------------------------ CPU baseline
CPU_RESULT = {}   # the oracle's answer over the first 1M rows, checked against the GPU's in single_gpu_extras


def host_cores():
    """(logical CPUs this process may run on, CPUs' worth of time its cgroup grants).  The GPU boxes of this pool show 256
    logical CPUs but cap a 1-GPU job at a share of them: 256 busy threads on a 16-CPU quota run slower than 16."""
    affinity = len(os.sched_getaffinity(0))
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:                       # cgroup v2: "<quota> <period>" or "max <period>"
            a, b = f.read().split()[:2]
            if a != "max":
                quota = float(a) / float(b)
    except Exception:
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())  # cgroup v1
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / per
        except Exception:
            pass
    return affinity, quota


def search_blocked_baseline(np, xh, qh, k, threads, oI, oD=None):
    """faiss-like CPU search: S = q @ x_blk^T (sgemm) over 1024-row blocks, running top-k by argpartition.  Labelled
    "faiss-like, not bit-exact"; the ids are compared with the exact oracle's only as a recall figure."""
    from threadpoolctl import threadpool_limits
    nq_s, n = qh.shape[0], xh.shape[0]
    BLK = 1024

    def run():
        best_s = np.full((nq_s, k), -np.inf, np.float32)
        best_i = np.full((nq_s, k), -1, np.int64)
        for b0 in range(0, n, BLK):
            sblk = qh @ xh[b0:b0 + BLK].T
            cs = np.concatenate([best_s, sblk], 1)
            ci = np.concatenate([best_i, np.broadcast_to(np.arange(b0, b0 + sblk.shape[1], dtype=np.int64), sblk.shape)], 1)
            sel = np.argpartition(-cs, k - 1, axis=1)[:, :k]
            best_s, best_i = np.take_along_axis(cs, sel, 1), np.take_along_axis(ci, sel, 1)
        o = np.argsort(-best_s, axis=1, kind="stable")
        return np.take_along_axis(best_s, o, 1), np.take_along_axis(best_i, o, 1)
    with threadpool_limits(limits=int(threads)):
        run()
        ts = []
        for _ in range(3):
            tp = time.perf_counter()
            _, bI = run()
            ts.append(time.perf_counter() - tp)
    t = float(np.median(ts))
    recall = float(np.mean([len(set(bI[i]) & set(oI[i])) / float(k) for i in range(nq_s)]))
    vs = None
    if oD is not None:
        # what the canonical (fma-chain) order costs against a BLAS-order IndexFlatIP, measured: ids that moved, and that every move
        # sits inside a tie band (oracle/blas_order.py; tests/test_search_gpu.py asserts it on GPU results)
        from oracle import blas_order
        try:
            vs = blas_order.tie_band_report(xh, qh, k, oD, oI)
        except Exception as ex:
            vs = {"error": repr(ex)}
    return {"vs_blas_order": vs, "label": "faiss-like (blocked sgemm + top-k update), numpy/OpenBLAS, NOT bit-exact", "queries_per_sec_over_slice": round(nq_s / t, 2),
            "GFLOPs": round(2.0 * nq_s * n * D_EMB / t / 1e9, 1), "block_rows": BLK, "threads": int(threads), "runs_s": [round(v, 3) for v in ts],
            "recall_vs_exact_ids": round(recall, 5)}


def cpu_baseline(np, torch, synth, enc, D, I, q_pre, kept, rows, nq, k, Lq, tok, timed_emb=None, enc_plan=None):
    """The oracle on this box's host cores: C/OpenMP restatement of IndexFlatIP over a 1M-row slice of the corpus
    (x rows/1M to the full corpus: the scan is linear in rows) + the fp32 torch-CPU restatement of ANCE, each the
    median of 5 runs after one warm-up.  faiss itself is tried first (the reference's CPU path, :52,:68-69).
    Thread counts are set through the libraries' own calls (an OMP_NUM_THREADS exported after libgomp has started does
    nothing) and reported as used."""
    from oracle import ance_oracle, oracle
    affinity, quota = host_cores()
    cores = affinity if quota is None else max(1, min(affinity, int(quota + 0.5)))
    xh = np.concatenate(kept)[:1_000_000]
    n_slice = xh.shape[0]
    # the team size that is fastest on this box: the granted CPUs, or every logical CPU (one probe each)
    probe = {}
    for nt in sorted({cores, affinity}):
        oracle.set_num_threads(nt)
        oracle.flat_ip_search(xh[:100_000], q_pre[:64].cpu().numpy(), k)
        tp = time.perf_counter()
        oracle.flat_ip_search(xh[:100_000], q_pre[:64].cpu().numpy(), k)
        probe[nt] = time.perf_counter() - tp
    oracle.set_num_threads(min(probe, key=probe.get))
    omp_threads = oracle.num_threads()
    try:
        import faiss  # noqa: F401
        faiss_note = "importable: version " + getattr(faiss, "__version__", "?")
    except Exception as ex:
        faiss, faiss_note = None, f"import faiss failed on this box ({type(ex).__name__}): the C/OpenMP port stands in for faiss-cpu"
    # search: queries/s over the slice; per-query time over the full corpus = rows / n_slice times that
    nq_s = min(nq, 200)
    qh = q_pre[:nq_s].cpu().numpy()
    oracle.flat_ip_search(xh, qh[:16], k)
    ts = []
    for _ in range(5):
        tp = time.perf_counter()
        oD, oI = oracle.flat_ip_search(xh, qh, k)
        ts.append(time.perf_counter() - tp)
    t_search_q = float(np.median(ts)) / nq_s * (rows / n_slice)
    search = {"queries_per_sec_over_slice": round(nq_s / float(np.median(ts)), 2), "slice_rows": n_slice, "queries": nq_s,
              "runs_s": [round(t, 3) for t in ts], "threads": omp_threads,
              "decomposition": "(8-query block, row chunk) tasks over all threads; chunk lists merged in the canonical order"}
    CPU_RESULT["slice"] = (oD, oI)
    if faiss is not None:
        fi = faiss.IndexFlatIP(D_EMB)
        fi.add(xh)
        fi.search(qh[:16], k)
        tf = []
        for _ in range(5):
            tp = time.perf_counter()
            fi.search(qh, k)
            tf.append(time.perf_counter() - tp)
        search["faiss_cpu_queries_per_sec_over_slice"] = round(nq_s / float(np.median(tf)), 2)
    search["GFLOPs"] = round(2.0 * nq_s * n_slice * D_EMB / float(np.median(ts)) / 1e9, 1)
    # beside the exact port: the SHAPE of faiss-cpu's IndexFlatIP.search (blocked sgemm over 1024-row database blocks, then a
    # top-k update), with numpy / OpenBLAS -- not bit-exact (BLAS summation order), a speed reference only
    try:
        search["blocked_sgemm"] = search_blocked_baseline(np, xh, qh, k, cores, oI, oD)
    except Exception as ex:
        search["blocked_sgemm"] = {"error": repr(ex)}
    res = {"unit": "queries/s", "kind": "port", "cores": cores, "logical_cpus": affinity, "cgroup_cpu_quota": quota, "faiss": faiss_note, "search": search}
    if enc is None:
        res["value"] = round(1.0 / t_search_q, 3)
        res["sample"] = (f"search only: {nq_s} queries over a {n_slice}-row slice, oracle/flat_ip_oracle.c (OpenMP, {omp_threads} threads, AVX2 fmaf "
                         f"chain), median of 5, scaled x{rows / n_slice:g} to the {rows}-row corpus")
        return res
    # encode: fp32 torch CPU ops; thread count = the faster of all cores and 64 (one probe each)
    sd_cpu = synth.ance_state_dict(0xA11CE, 12, rich=False)
    n_s = 8
    ids_s, mask_s = tok[:n_s].astype(np.int64), np.ones((n_s, Lq), np.int64)
    best = None
    for nt in sorted({cores, affinity, min(affinity, 64)}):
        torch.set_num_threads(nt)
        ance_oracle.ance_forward(sd_cpu, ids_s[:1], mask_s[:1])
        tp = time.perf_counter()
        ance_oracle.ance_forward(sd_cpu, ids_s, mask_s)
        t = time.perf_counter() - tp
        if best is None or t < best[1]:
            best = (nt, t)
    torch.set_num_threads(best[0])
    te = []
    for _ in range(5):
        tp = time.perf_counter()
        ref = ance_oracle.ance_forward(sd_cpu, ids_s, mask_s)
        te.append(time.perf_counter() - tp)
    t_enc_q = float(np.median(te)) / n_s
    import torch as _t
    got = enc(_t.from_numpy(ids_s).cuda(), _t.from_numpy(mask_s).cuda()).cpu().numpy()
    small_plan = enc.last_plan()
    cosd = 1.0 - (got * ref).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(ref, axis=1))
    res["encode"] = {"queries_per_sec": round(1.0 / t_enc_q, 3), "queries": n_s, "seq_len": Lq, "threads": torch.get_num_threads(),
                     "runs_s": [round(t, 3) for t in te], "max_1_minus_cos_gpu_vs_cpu": float(cosd.max()),
                     "max_1_minus_cos_gpu_vs_cpu_kernels": f"these {n_s} queries encoded on their own ({small_plan}): the small-batch kernel family, "
                                                           "NOT the kernels the metric times; the timed batch is checked below"}
    if timed_emb is not None:
        # the path the metric is made of, checked where it is timed: rows of the timed 1000 x 512 batch itself (both
        # sub-batches, tile borders) against the fp32 oracle on those very sequences
        pick = sorted({i for i in (0, 255, 256, 511, 512, len(timed_emb) - 1) if 0 <= i < len(timed_emb)})
        ref_t = ance_oracle.ance_forward(sd_cpu, tok[pick].astype(np.int64), np.ones((len(pick), Lq), np.int64))
        got_t = timed_emb[pick]
        cosd_t = 1.0 - (got_t * ref_t).sum(1) / (np.linalg.norm(got_t, axis=1) * np.linalg.norm(ref_t, axis=1))
        res["encode"]["max_1_minus_cos_timed_batch_vs_cpu"] = float(cosd_t.max())
        # the same check scaled to what these rows can show (tests/parity.py): N(0, 0.02^2) weights put all embeddings close to
        # one direction, so the raw figure is read against the distance between two DIFFERENT sequences of the pick
        from tests import parity
        pm = parity.measure(got_t, ref_t)
        res["encode"]["timed_batch_check"] = {"rows": pick, "one_minus_cos": [float(v) for v in cosd_t], "kernels": enc_plan,
                                              "inter_sequence_min_1_minus_cos": pm["spread"]["raw_min"],
                                              "error_over_inter_sequence_distance": pm["raw"] / pm["spread"]["raw_min"],
                                              "centred_1_minus_cos": pm["centred"], "centred_bound": pm["centred_bound"],
                                              "relative_l2": pm["rel_l2"], "relative_l2_bound": pm["rel_l2_bound"],
                                              "passes_fixture_scaled_bounds": bool(parity.embeddings_match(got_t, ref_t)),
                                              "neighbours_embedding_would_pass": bool(parity.embeddings_match(np.roll(got_t, 1, axis=0), ref_t)),
                                              "what": "embeddings produced INSIDE the timed region (last timed step) vs oracle/ance_oracle.py on the same sequences; "
                                                      "bar 1e-3 (BASELINE.json north_star) and a tenth of the smallest distance between two of these sequences' "
                                                      "reference embeddings; centred = batch mean of the reference rows removed from both sides"}
    res["value"] = round(1.0 / (t_enc_q + t_search_q), 3)
    res["cores"] = max(omp_threads, torch.get_num_threads())          # the threads actually used (the larger of the two legs)
    res["threads"] = {"search_openmp": omp_threads, "encode_torch": torch.get_num_threads()}
    res["sample"] = (f"encode: {n_s} of the {nq} queries (L={Lq}) through oracle/ance_oracle.py (fp32 torch CPU ops, {torch.get_num_threads()} threads); search: "
                     f"{nq_s} queries over a {n_slice}-row slice through oracle/flat_ip_oracle.c (OpenMP, {omp_threads} threads), scaled "
                     f"x{rows / n_slice:g} to {rows} rows; each the median of 5 runs after a warm-up; value = 1 / (encode s/query + search s/query)")
    return res


# ------------------------------------------------------------------------------ extras: the reference's literal call shapes, sustained rates
def enc_flops(B, L):
    """SURVEY 8d, padded: 12 x (14,155,776 T + 4 T^2 768) + 2 x 768^2 per sequence."""
    return B * (12.0 * (14155776.0 * L + 4.0 * L * L * 768.0) + 2.0 * 768 * 768)


def encoder_batch_sweep(np, torch, synth, enc, dev, sync, full=True):
    """The encoder at the batch shapes the reference itself calls it with: 4 x n_gpu queries per call
    (src/test_HAConvDR_topiocqa.py:173,406), 250 x n_gpu passages (Config/gen_doc_embeddings.toml:14,17), fully padded
    (L = 512 TopiOCQA queries, 256 QReCC queries, 384 passages).  ms = wall clock per forward over back-to-back calls (device
    tensors in and out, no host sync between calls).  Small batches replay a HIP graph (graph=replay); `graph_off_ms` is the
    same shape with plain launches."""
    rows = []
    # default line: the reference's literal query call (B = 4) at its two lengths, one sequence, and the passage batch; full: the grid
    shapes = [(L, B) for L in (256, 384, 512) for B in (1, 4, 16, 64, 250, 500)] if full else [(256, 1), (256, 4), (512, 4), (512, 16), (384, 250)]
    for L, B in shapes:
        if True:
            tok, _ = synth.token_batch(0x5EE + B + L, B, L, fixed_len=L)
            ids = torch.from_numpy(tok.astype(np.int64)).to(dev)
            mask = torch.ones_like(ids)
            reps = 200 if B <= 16 else (30 if B <= 64 else 6)
            enc(ids, mask)                                   # (first call of a shape: plain launches; second: capture)
            t = timed(lambda: enc(ids, mask), reps, sync)
            ent = {"B": B, "L": L, "ms": round(t * 1e3, 4), "seq_per_sec": round(B / t, 1), "mfma_bf16_frac": round(enc_flops(B, L) / t / 2.5e15, 4),
                   "plan": enc.last_plan()}
            if "graph=replay" in ent["plan"]:
                enc.set_option("graph", "off")
                ent["graph_off_ms"] = round(timed(lambda: enc(ids, mask), reps, sync) * 1e3, 4)
                enc.set_option("graph", "auto")
            rows.append(ent)
    return {"what": "ANCE forward at the reference's own batch shapes, fully padded; wall clock per call, back-to-back calls on one stream",
            "rows": rows}


def sustained(np, torch, synth, enc, step, nq, dev, sync, seconds=30.0):
    """The headline step and the configs[4]-shape passage encode looped for >= 30 s each: what the chip holds once it is warm
    (the timed region of the headline is a few seconds)."""
    def loop(fn, units, sync_every):
        marks = []
        sync()
        t0 = time.perf_counter()
        n = 0
        while True:
            for _ in range(sync_every):
                fn()
            sync()
            n += sync_every
            now = time.perf_counter() - t0
            marks.append((now, n))
            if now >= seconds:
                break
        total_t, total_n = marks[-1]
        first = next(m for m in marks if m[0] >= 5.0)
        last_from = next(m for m in marks if m[0] >= total_t - 5.0)
        r_first = first[1] / first[0]
        r_last = (total_n - last_from[1]) / max(1e-9, total_t - last_from[0]) if total_n > last_from[1] else total_n / total_t
        return {"seconds": round(total_t, 2), "iterations": total_n, "units_per_sec": round(units * total_n / total_t, 1),
                "first_5s_units_per_sec": round(units * r_first, 1), "last_5s_units_per_sec": round(units * r_last, 1),
                "last_over_first": round(r_last / r_first, 4)}
    out = {"what": f"looped for >= {seconds:g} s, synchronized every few iterations; units = queries (step) / passages (encode)"}
    out["cfg3_step"] = loop(lambda: step(), nq, 4)
    Bp, Lp = 1000, 384
    ptok, _ = synth.token_batch(0xD0C, Bp, Lp, fixed_len=Lp)
    plens = np.clip(np.rint(180.0 + 80.0 * synth.normal(0x1E45, (Bp,))), 8, Lp).astype(np.int64)
    pid_t = torch.from_numpy(ptok.astype(np.int64)).to(dev)
    var_mask = (torch.arange(Lp, device=dev)[None, :] < torch.from_numpy(plens).to(dev)[:, None]).to(torch.int64)
    full_mask = torch.ones_like(pid_t)
    out["cfg5_passages_padded"] = loop(lambda: enc(pid_t, full_mask), Bp, 4)
    out["cfg5_passages_varlen"] = loop(lambda: enc(pid_t, var_mask), Bp, 8)
    return out


def attention_peaked(np, torch, synth, enc, ids_t, mask_t, nq, Lq, sync):
    """The headline's random-init weights N(0, 0.02^2) give near-uniform attention (logit sigma ~0.3), the cheapest case for the
    streaming softmax.  The same 1000 x 512 forward with the query and key projections scaled x4 / x10 (logit sigma ~5 / ~30:
    rows dominated by a few keys, running maxima that keep moving -- tests/test_encoder_gpu.py::test_peaked_attention_*): the
    dependence of the headline on its data, on the record."""
    base = synth.ance_state_dict(0xA11CE, 12, rich=False)
    qk = [k for k in base if ".attention.self.query." in k or ".attention.self.key." in k]
    res = {"what": "encode of the timed batch with query / key projections scaled (logit sigma ~0.3 / ~5 / ~30)", "rows": []}
    fl_attn = 4.0 * Lq * 768 * (nq * Lq) * 12
    try:
        for scale in (1.0, 4.0, 10.0):
            if scale != 1.0:
                enc.load_state_dict({k: (base[k] * scale).astype(np.float32) for k in qk})
            t = timed(lambda: enc(ids_t, mask_t), 3, sync)
            enc.set_profiling(False, classes=("attention",))
            enc(ids_t, mask_t)
            sync()
            att = float(np.sum(enc.profile_drain_class("attention")))
            enc.set_profiling(False)
            res["rows"].append({"qk_scale": scale, "encode_ms": round(t * 1e3, 3), "queries_per_sec": round(nq / t, 1), "attention_ms_per_forward": round(att, 3),
                                "attention_frac_of_2.5PF": round(fl_attn / (att * 1e-3) / 2.5e15, 4)})
    finally:
        enc.load_state_dict({k: base[k] for k in qk})
    return res


def three_call_protocol(np, torch, FlatIPIndex, q_pre, dev, k, block_rows=2_500_000, blocks=3):
    """The reference's literal loop (src/test_HAConvDR_topiocqa.py:77-123): per 2.5M-row passage block index.add(host rows) ->
    index.search(all queries, host in / out) -> index.reset(), through the synchronous host entry points (hac_index_add /
    _search / _reset).  add() is the PCIe-bound part (7.68 GB per block: pageable -> pinned staging -> H2D, double-buffered)."""
    x = torch.cat([gen_rows(0xB10C + c, CH, dev) for c in range(block_rows // CH)]).cpu().numpy()
    qh = q_pre.cpu().numpy()
    idx = FlatIPIndex(D_EMB, devices=(dev.index,))
    parts = []
    for b in range(blocks):
        t0 = time.perf_counter()
        idx.add(x)
        t1 = time.perf_counter()
        D, I = idx.search(qh, k)
        t2 = time.perf_counter()
        idx.reset()
        t3 = time.perf_counter()
        parts.append({"add_ms": round((t1 - t0) * 1e3, 2), "search_ms": round((t2 - t1) * 1e3, 2), "reset_ms": round((t3 - t2) * 1e3, 2),
                      "block_ms": round((t3 - t0) * 1e3, 2)})
    best = min(parts[1:], key=lambda p: p["block_ms"])
    gb = block_rows * D_EMB * 4 / 1e9
    return {"what": "add(host rows) -> search(1000 host queries, top-100) -> reset per 2.5M-row block, host entry points, wall clock",
            "block_rows": block_rows, "block_GB": round(gb, 3), "blocks": parts, "steady_block_ms": best["block_ms"],
            "add_GBps": round(gb / (best["add_ms"] * 1e-3), 1), "plan": idx.last_plan(),
            "note": "search_ms includes the first-search work after every reset: the segment-table upload and, on the prefilter path, "
                    "the fp16 image of the block (one pass over its 7.68 GB)"}


# ------------------------------------------------------------------------------ extras, one GPU
def single_gpu_extras(np, torch, synth, FlatIPIndex, enc, index, q_pre, dev, n_local, nq, k, sync):
    """Kernel-level evidence beside the headline: BASELINE configs[1] (1M rows, search only), the exact fp32 kernels
    alone, the HBM-bound regime of the scan, passage-encoding rates (configs[4] shape)."""
    ex = {}
    # configs[1]: 1M x 768, 1000 pre-encoded queries, search only
    idx1 = FlatIPIndex(D_EMB, devices=(dev.index,))
    xs = torch.cat([gen_rows(0xC0FFEE + c, CH, dev) for c in range(8)])
    idx1.add_tensor(xs)
    sync()
    del xs
    n1 = 1_000_000
    for _ in range(3):                       # (the fp16 image comes with the first prefilter search, the rescoring's row-major copy with the third)
        idx1.search_tensor(q_pre, k)
    sync()
    idx1.set_profiling(True)
    t = timed(lambda: idx1.search_tensor(q_pre, k), 20, sync)
    ms = float(np.sum(idx1.profile_drain())) / 21
    idx1.set_profiling(False)
    fl = 2.0 * nq * n1 * D_EMB
    plan = idx1.last_plan()
    ex["cfg2_search_only"] = {"workload": "BASELINE configs[1]: 1000000x768 corpus, 1000 pre-encoded queries, top-100, IP search only",
                              "queries_per_sec": round(nq / t, 1), "ms_per_step": round(t * 1e3, 4), "plan": plan, "scan_kernel_ms": round(ms, 4),
                              "achieved_TFLOPs": round(fl / (ms * 1e-3) / 1e12, 1),
                              "frac_of_fp16_mfma_peak": round(fl / (ms * 1e-3) / 1e12 / PEAK_F16_MFMA_TF, 4)}
    Ds, Is = idx1.search_tensor(q_pre, k)
    if "slice" in CPU_RESULT:   # the CPU baseline searched these very rows (first 1M of the corpus): same bits?
        oD, oI = CPU_RESULT["slice"]
        ex["cfg2_search_only"]["ids_and_scores_equal_to_cpu_oracle"] = bool(
            np.array_equal(oI, Is[:len(oI)].cpu().numpy()) and np.array_equal(oD, Ds[:len(oD)].cpu().numpy()))
    idx1.set_option("split", "0")
    idx1.set_profiling(True)
    t = timed(lambda: idx1.search_tensor(q_pre, k), 3, sync)
    ms = float(np.sum(idx1.profile_drain())) / 4
    idx1.set_profiling(False)
    De, Ie = idx1.search_tensor(q_pre, k)
    ex["cfg2_exact_fp32_kernels"] = {"plan": idx1.last_plan(), "kernel_ms": round(ms, 4), "queries_per_sec": round(nq / t, 1),
                                     "achieved_TFLOPs": round(fl / (ms * 1e-3) / 1e12, 2),
                                     "frac_of_fp32_mfma_peak": round(fl / (ms * 1e-3) / 1e12 / PEAK_F32_MFMA_TF, 4),
                                     "ids_and_scores_equal_to_prefilter_path": bool(torch.equal(Ie, Is) and torch.equal(De, Ds))}
    idx1.set_option("split", "auto")
    # HBM-bound regime: <= 16 queries per corpus pass (north_star: IP-search kernel >= 60 % of the HBM roofline).  The exact fp32 kernels
    # (split = 0) are the roofline statement: algorithmic bytes = the fp32 corpus once.  What "auto" runs for such calls on an index that
    # keeps being searched is the prefilter over the fp16 image (half the bytes, same bits): its time and the rate of the image stream beside it.
    sweep = []
    for which, ix, n in (("1M", idx1, n1), ("resident corpus", index, n_local)):
        for nqs in (1, 8, 16, 32):
            qs = q_pre[:nqs].contiguous()
            ent = {"corpus": which, "rows": n, "nq": nqs}
            for mode in ("0", "auto"):
                ix.set_option("split", mode)
                ix.set_profiling(True)
                ts = timed(lambda: ix.search_tensor(qs, k), 10 if n <= n1 else 3, sync)
                mss = float(np.mean(ix.profile_drain()))
                ix.set_profiling(False)
                if mode == "0":
                    bs = n * D_EMB * 4 + nqs * D_EMB * 4 + nqs * k * 12
                    ent.update({"kernel": ix.last_plan().split(" ")[0], "kernel_ms": round(mss, 4), "search_ms": round(ts * 1e3, 4),
                                "achieved_GBps": round(bs / (mss * 1e-3) / 1e9, 1), "frac_of_8TBps": round(bs / (mss * 1e-3) / 1e9 / PEAK_HBM_GBS, 4)})
                else:
                    De, Ie = ix.search_tensor(qs, k)
                    plan_a = ix.last_plan()
                    ix.set_option("split", "0")
                    Dx, Ix = ix.search_tensor(qs, k)
                    ix.set_option("split", "auto")
                    ent["auto"] = {"kernel": " ".join(plan_a.split(" ")[:2]), "scan_ms": round(mss, 4), "search_ms": round(ts * 1e3, 4),
                                   "fp16_image_GBps": round(n * D_EMB * 2 / (mss * 1e-3) / 1e9, 1) if plan_a.startswith("split:") else None,
                                   "same_bits_as_exact": bool(torch.equal(De, Dx) and torch.equal(Ie, Ix))}
            sweep.append(ent)
    ex["hbm_regime"] = {"what": "the scan with few queries per corpus pass is HBM-bound: algorithmic bytes (corpus once + queries + results) / kernel time, "
                                "exact fp32 kernels (split = 0); auto = what an index that keeps being searched runs for the same call",
                        "sweep": sweep}
    del idx1
    if enc is None:
        return ex
    # passages (BASELINE configs[4] shape: L=384): fully padded = what the reference computes, varlen = only the real
    # tokens (lens ~ clipped N(180, 80) in [8, 384]), and the whole gen_doc_embeddings loop
    Bp, Lp = 1000, 384
    ptok, _ = synth.token_batch(0xD0C, Bp, Lp, fixed_len=Lp)
    plens = np.clip(np.rint(180.0 + 80.0 * synth.normal(0x1E45, (Bp,))), 8, Lp).astype(np.int64)
    pid_t = torch.from_numpy(ptok.astype(np.int64)).to(dev)
    full_mask = torch.ones_like(pid_t)
    var_mask = (torch.arange(Lp, device=dev)[None, :] < torch.from_numpy(plens).to(dev)[:, None]).to(torch.int64)
    pres = {name: Bp / timed(lambda: enc(pid_t, m), 3, sync) for name, m in (("padded", full_mask), ("varlen", var_mask))}
    fl_pad = Bp * 12.0 * (14155776.0 * Lp + 4.0 * Lp * Lp * 768.0)
    psg = {"docs_per_sec_per_gpu_padded": round(pres["padded"], 1), "docs_per_sec_per_gpu_varlen": round(pres["varlen"], 1),
           "mfma_bf16_frac_padded": round(fl_pad * pres["padded"] / Bp / 2.5e15, 4), "mean_len_varlen": round(float(plens.mean()), 1), "batch": Bp}
    try:
        import shutil
        import tempfile
        from haconvdr_amd import passages as psg_mod
        n_p = 20000
        tmpd = tempfile.mkdtemp(prefix="hac_bench_")
        ptok_all, _ = synth.token_batch(0xD0C5, n_p, Lp, fixed_len=Lp)
        plens_all = np.clip(np.rint(180.0 + 80.0 * synth.normal(0x1E46, (n_p,))), 8, Lp).astype(np.int64)
        psg_mod.write_tokenized_passages(os.path.join(tmpd, "passages"), ptok_all.astype(np.int32), plens_all)
        coll = psg_mod.TokenizedPassages(os.path.join(tmpd, "passages"))
        psg_mod.encode_passages(enc, coll, os.path.join(tmpd, "warm"), per_gpu_eval_batch_size=1000)
        sync()
        t1 = time.perf_counter()
        psg_mod.encode_passages(enc, coll, os.path.join(tmpd, "out"), per_gpu_eval_batch_size=1000)
        sync()
        psg["pipeline_docs_per_sec_per_gpu"] = round(n_p / (time.perf_counter() - t1), 1)
        psg["pipeline"] = f"encode_passages over {n_p} tokenized records (reader, H2D, encode, block files), mean len {plens_all.mean():.0f}"
        shutil.rmtree(tmpd, ignore_errors=True)
    except Exception as e:   # an extra, never the headline
        psg["pipeline_error"] = repr(e)
    ex["passages_L384"] = psg
    return ex


if __name__ == "__main__":
    main()
