"""Rank of named rows, the parts that need no GPU: the C-ABI surface of the three new entry points, the counting kernel's
resource line, the argument checks of the Python mirrors (ValueError before the library is called, no handle needed),
trec.metrics_from_ranks against a hand-worked table and against print_trec_res on a run file of the same ranking, and
ShardedSearcher.rank over gloo with numpy doubles."""
import os
import re
import socket
import subprocess
import sys
import types

import numpy as np
import pytest

from tests import rank_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("hac_index_count_ahead_device", "hac_index_rank_ids", "hac_index_rank_ids_device")


def test_new_entry_points_are_declared_listed_and_exported():
    from haconvdr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "haconvdr.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(hac_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()                      # dlopen only; nothing is computed
    for sym in NEW_SYMBOLS:
        assert sym in declared, sym
        assert sym in _lib.EXPORTED_SYMBOLS, sym
        f = getattr(L, sym)
        assert f.argtypes is not None and f.restype is not None, sym


def test_count_kernels_use_no_scratch():
    path = os.path.join(ROOT, "haconvdr_amd", "csrc", "flat_ip.resources.txt")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(path)])
    blocks = re.split(r"remark: Function Name: ", open(path).read())
    for kernel in ("count_ahead_kernel", "rank_finish_kernel"):
        mine = [b for b in blocks if kernel in b.split("\n", 1)[0]]
        assert len(mine) == 1, kernel
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", mine[0]).group(1)) == 0, kernel
        assert int(re.search(r"VGPRs Spill: (\d+)", mine[0]).group(1)) == 0, kernel


# ---------------------------------------------------------------------------------------------------------------------
# argument checks (no handle)
def test_rank_args_pass_good_arguments_through():
    from haconvdr_amd import index
    q, ids = index._pair_args(np.zeros((3, 96), np.float64), np.zeros((3, 5), np.int32), 96, "rank_ids")
    assert q.dtype == np.float32 and ids.dtype == np.int64 and ids.shape == (3, 5) and ids.flags.c_contiguous
    assert index._pair_args(np.zeros((3, 96)), np.zeros((3, 0), np.int64), 96, "rank_ids")[1].shape == (3, 0)
    assert index._pair_args(np.zeros((0, 96)), np.zeros((0, 4), np.int64), 96, "rank_ids")[0].shape == (0, 96)


@pytest.mark.parametrize("q, ids", [
    (np.zeros((3, 96)), np.zeros((3, 5), np.float32)),       # float ids
    (np.zeros((3, 96)), np.zeros(5, np.int64)),              # one list, not one per query
    (np.zeros((3, 96)), np.zeros((3, 5, 1), np.int64)),
    (np.zeros((3, 96)), np.zeros((2, 5), np.int64)),         # ids.shape[0] != nq
    (np.zeros((3, 95)), np.zeros((3, 5), np.int64)),         # wrong dimension
    (np.zeros(96), np.zeros((1, 5), np.int64)),
    (np.zeros((3, 96)), np.array([[2 ** 63] * 2] * 3, np.uint64)),
])
def test_rank_args_raise_value_error(q, ids):
    from haconvdr_amd import index
    with pytest.raises(ValueError):
        index._pair_args(q, ids, 96, "rank_ids")


def test_tensor_checks_refuse_host_tensors():
    """The tensor forms hand raw device pointers to kernels: a CPU tensor or an ndarray must never get there."""
    import torch
    from haconvdr_amd import index
    with pytest.raises(ValueError):
        index._pair_args_tensor(torch.zeros(3, 96), torch.zeros(3, 5, dtype=torch.int64), 96, "rank_ids_tensor")
    with pytest.raises(ValueError):
        index._pair_args_tensor(np.zeros((3, 96), np.float32), np.zeros((3, 5), np.int64), 96, "rank_ids_tensor")
    with pytest.raises(ValueError):
        index._count_args_tensor(torch.zeros(3, 96), torch.zeros(3, 5), torch.zeros(3, 5, dtype=torch.int64), 96)


def test_sharded_rank_checks_the_ids_before_any_hook_runs():
    import torch
    from haconvdr_amd.sharded import ShardedSearcher

    def never(*a):
        raise AssertionError("a hook ran")
    s = ShardedSearcher(None, 0, n_local=10, local_scores=never, count_ahead=never)
    for bad in (torch.zeros(5, dtype=torch.int64), torch.zeros((2, 5), dtype=torch.int64), torch.zeros((3, 5), dtype=torch.int32)):
        with pytest.raises(ValueError):
            s.rank(torch.zeros(3, 96), bad)


# ---------------------------------------------------------------------------------------------------------------------
# metrics_from_ranks
def test_metrics_from_ranks_hand_worked():
    from haconvdr_amd.trec import metrics_from_ranks
    ranks = np.array([[0, -1, -1],        # RR 1      R@10 1/1   R@100 1/1
                      [4, 12, -1],        # RR 1/5    R@10 1/2   R@100 2/2
                      [150, 99, 10],      # RR 1/11   R@10 0/3   R@100 2/3
                      [-1, -1, -1]],      # nothing relevant: 0, 0, 0
                     np.int64)
    m = metrics_from_ranks(ranks)
    assert set(m) == {"MRR", "Recall@10", "Recall@100"}
    assert m["MRR"] == round((1 + 1 / 5 + 1 / 11 + 0) / 4 * 100, 5)
    assert m["Recall@10"] == round((1 + 1 / 2 + 0 + 0) / 4 * 100, 5)
    assert m["Recall@100"] == round((1 + 1 + 2 / 3 + 0) / 4 * 100, 5)
    # cutoff: ranks >= N are unranked but still relevant
    c = metrics_from_ranks(ranks, cutoff=10)
    assert c["MRR"] == round((1 + 1 / 5 + 0 + 0) / 4 * 100, 5)
    assert c["Recall@10"] == m["Recall@10"] and c["Recall@100"] == round((1 + 1 / 2 + 0 + 0) / 4 * 100, 5)
    # an unranked-only row beyond every list: rank 150 alone
    assert metrics_from_ranks(np.array([[150]]), ks=(10, 100, 1000)) == {"MRR": round(100 / 151, 5), "Recall@10": 0.0, "Recall@100": 0.0,
                                                                        "Recall@1000": 100.0}
    assert metrics_from_ranks(np.zeros((0, 2), np.int64)) == {"MRR": 0.0, "Recall@10": 0.0, "Recall@100": 0.0}
    assert metrics_from_ranks(np.zeros((2, 0), np.int64)) == {"MRR": 0.0, "Recall@10": 0.0, "Recall@100": 0.0}
    for bad in (np.zeros((2, 2), np.float32), np.zeros(3, np.int64)):
        with pytest.raises(ValueError):
            metrics_from_ranks(bad)


def test_metrics_from_ranks_equal_print_trec_res(tmp_path, oracle):
    """The reference's route -- top_k list, run file, metric block -- and exact ranks with cutoff = top_k give the same figures."""
    from haconvdr_amd import synth
    from haconvdr_amd.trec import metrics_from_ranks, output_test_res, print_trec_res
    n, d, nq, top_k = 400, 32, 12, 100
    x = synth.embeddings(0x7E0, n, d)
    q = synth.embeddings(0x7E1, nq, d)
    offset2pid = (np.arange(n, dtype=np.int64) * 3 + 5)[np.argsort(synth.uniform_u32(0x7E2, n), kind="stable")]      # unique passage ids
    D, I = oracle.flat_ip_search(x, q, top_k)
    full = oracle.flat_ip_search(x, q, n)[1]
    # gold rows per query: near the top, inside the list, beyond it; query 5 only beyond it, query 6 three inside the top 10
    gold = np.full((nq, 3), -1, np.int64)
    for i in range(nq):
        gold[i] = full[i, [i % 12, 10 + 7 * i, 100 + 20 * i]]
    gold[5] = full[5, [150, 399, 100]]
    gold[6] = full[6, [0, 9, 3]]
    gold[7, 1:] = -1                                          # one gold passage only
    args = types.SimpleNamespace(top_k=top_k, qrel_output_path=str(tmp_path), output_trec_file="run.trec")
    qids = [f"q{i}" for i in range(nq)]
    run = output_test_res(qids, D, I, offset2pid, args)
    qrel = tmp_path / "gold.qrel"
    with open(qrel, "w") as f:
        for i in range(nq):
            for r in gold[i][gold[i] >= 0]:
                f.write(f"q{i} Q0 {offset2pid[r]} 1\n")
    want = print_trec_res(run, str(qrel))
    ranks = rank_ref.rank_ids(oracle, x, q, gold)
    assert ranks[5].min() >= top_k and (ranks[6] < 10).all() and (ranks[0] >= 0).all() and (ranks[7, 1:] == -1).all()
    got = metrics_from_ranks(ranks, cutoff=top_k)
    for name in ("MRR", "Recall@10", "Recall@100"):
        assert got[name] == want[name], (name, got, want)
    assert 0 < want["Recall@10"] < want["Recall@100"] < 100
    assert metrics_from_ranks(ranks)["MRR"] > got["MRR"]      # without the cutoff, query 5's gold passages count too


# ---------------------------------------------------------------------------------------------------------------------
# ShardedSearcher.rank over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_rank_doubles_restate_the_contract(oracle):
    import torch
    from tests import doubles_rank
    x = np.array([[1, 0], [2, 0], [2, 0], [np.nan, 0], [0.5, 0]], np.float32)
    x = np.concatenate([x, np.zeros((5, 30), np.float32)], 1)
    q = np.zeros((1, 32), np.float32)
    q[0, 0] = 1.0
    s = doubles_rank.make_local_scores(oracle, x)(torch.from_numpy(q), torch.tensor([[1, 3, -1, 5]]))
    assert s[0, 0] == 2.0 and torch.isnan(s[0, 1]) and s[0, 2] == -doubles_rank.FMAX and s[0, 3] == -doubles_rank.FMAX
    c = doubles_rank.make_count_ahead(oracle, x)(torch.from_numpy(q), torch.tensor([[2.0, 2.0, 2.0, 0.0, float("nan"), 2.0]]),
                                                 torch.tensor([[0, 2, 9, 0, 0, -1]]))
    assert c.tolist() == [[0, 1, 2, 4, -1, -1]]
    doubles_rank.CALLS.clear()


@pytest.mark.parametrize("world", [2, 8])
def test_sharded_rank_gloo(world, oracle):
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="2")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_gloo_worker_rank.py")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o
        assert "OK" in o
