"""Host mirror of the rules that decide what a captured forward looks like (haconvdr_amd/csrc/encoder.hip): test code only.

A forward of at most GRAPH_MAX_ROWS padded rows (B * pad_len(L)) is captured into a HIP graph on its second call and replayed
afterwards (forward_graph).  What the captured launches are follows from (B, L) and the device's CU count alone -- a replay runs no
host-side planning -- by these rules, restated here as pure functions (each names the code it restates):

  graph_eligible   graph_eligible():  B * pad_len(L) <= GRAPH_MAX_ROWS and <= max_tokens
  pick_family      pick_family():     Mp = roundup(B * pad_len(L), MT = 256); gemm8 from (Mp / 256) * (H / 256) >= FAMILY_BIG_TILES = 111
                                      on, i.e. from 9472 rows; precision = split is always split128
  ksplit           pick_ksplit() / ksplit_slots() / plan_ksplit(): the split-K of out-proj and FFN-down, "a/b" as the plan prints it
  att_qs, att_one  attention():       the query split doubles while B * NH * att_qs * 2 <= n_cu (at most 16); with a split and
                                      L32 > 256 both length classes run in ONE launch
  woven            attention():       a layer that is not the <s>-only last one takes attention_pipe_kernel<8> in "auto" iff
                                      att_qs == 1 and L32 > 256 (and pipe_skip_mask leaves it alone); the fix-up launches follow
  Mc               fwd_build():       the compact tail's rows, roundup(B, MT)

tests/test_graph_shapes.py pins them at 256 CUs; tests/test_encoder_graph_shapes_gpu.py takes the expected form of every shape
from here and the batches of its calls from `calls`."""
import numpy as np

H, NH, FF = 768, 12, 3072
SEQ_ALIGN, MT = 32, 256
GRAPH_MAX_ROWS = 16384
MAX_TOKENS = 524288              # hac_encoder::max_tokens' default
FAMILY_BIG_TILES = 111
REDO_RETRY = 64                  # redo_poll(): pipe_skip_mask is cleared on every 64th run_forward of a handle

# name -> (B, L): each the smallest or the edge shape that reaches its form (tests/test_encoder_graph_shapes_gpu.py)
SHAPES = {
    "qs2_long": (8, 512),        # att_qs 2, one att_one launch, classic128
    "qs2_short": (8, 256),       # att_qs 2, two launches
    "woven_c128": (12, 512),     # first B with att_qs 1: woven + fix-up launches, classic128, second items
    "c128_top": (18, 512),       # last classic128 shape (9216 rows)
    "g8_first": (19, 512),       # first gemm8 shape (9728 rows), woven
    "g8_384": (40, 384),         # gemm8, woven at L32 = 384
    "g8_top": (32, 512),         # largest eligible shape (16384 rows)
    "g8_short64": (256, 64),     # gemm8, short class only, Mc = 256
    "g8_short32": (512, 32),     # gemm8, Mc = 512, seq_offsets_kernel with two sequences per thread
}


def pad_len(L):
    return (int(L) + SEQ_ALIGN - 1) // SEQ_ALIGN * SEQ_ALIGN


def _roundup(n, m):
    return (int(n) + m - 1) // m * m


def padded_rows(B, L):
    """The rows a forward is planned for: every sequence at full length."""
    return int(B) * pad_len(L)


def graph_eligible(B, L, max_tokens=MAX_TOKENS):
    return padded_rows(B, L) <= GRAPH_MAX_ROWS and padded_rows(B, L) <= max_tokens


def Mp(B, L):
    """Fwd::Mp of a forward without a row hint (a graph forward never has one) = the plan's rows= field."""
    return _roundup(padded_rows(B, L), MT)


def Mc(B):
    return _roundup(B, MT)


def pick_family(B, L, precision="bf16", gemm="auto"):
    if precision == "split":
        return "split128"
    big = (Mp(B, L) // 256) * (H // 256) >= FAMILY_BIG_TILES
    if gemm == "8phase" or (gemm == "auto" and big):
        return "gemm8"
    return "classic256" if big else "classic128"


def _pick_ksplit(K, Mp_plan, wg_slots):
    if wg_slots == 0:
        return 1
    KT = K // 64
    min_kt = 8 if KT >= 48 else 4
    tiles = (Mp_plan // 128) * (H // 128)
    S, best = 1, KT * 0.6
    for cand in (2, 3, 4, 6):
        if KT % cand or KT // cand < min_kt or tiles * cand > wg_slots:
            continue
        cost = KT / cand * 0.6 + (cand - 1) * Mp_plan * 1.3e-3
        if cost < best:
            best, S = cost, cand
    return S


def ksplit(B, L, n_cu, precision="bf16", gemm="auto"):
    """The plan's ksplit= field: slices of out-proj (K = 768) / FFN-down (K = 3072)."""
    family = pick_family(B, L, precision, gemm)
    slots = {"split128": n_cu, "classic128": 2 * n_cu}.get(family, 0)
    return "%d/%d" % (_pick_ksplit(H, Mp(B, L), slots), _pick_ksplit(FF, Mp(B, L), slots))


def att_qs(B, n_cu):
    qs = 1
    while qs < 16 and int(B) * NH * qs * 2 <= n_cu:
        qs *= 2
    return qs


def att_one(B, L, n_cu):
    return att_qs(B, n_cu) > 1 and pad_len(L) > 256


def attention_launches(B, L, n_cu):
    """Launches of one non-woven layer's attention: the long class's (L32 > 256) and, unless att_one folds it in, the short class's."""
    return (1 if pad_len(L) > 256 else 0) + (0 if att_one(B, L, n_cu) else 1)


def woven(B, L, n_cu, n_layers=2, pooling="first", precision="bf16"):
    """Does some layer of an attn_pipe = auto forward take the woven kernel (no layer in pipe_skip_mask)?  The last layer of
    pooling = first never does: it computes the <s> rows only."""
    candidates = n_layers if pooling == "mean" else n_layers - 1
    return precision != "split" and candidates > 0 and att_qs(B, n_cu) == 1 and pad_len(L) > 256


def form(B, L, n_cu, n_layers=2, pooling="first", precision="bf16"):
    """What the plan of a (replayed) forward of B x L must say, and what it does not say but follows from the same rules."""
    split = precision == "split"
    return {"rows": str(Mp(B, L)), "gemm": pick_family(B, L, precision), "ksplit": ksplit(B, L, n_cu, precision),
            "attn_form": "split" if split else ("woven" if woven(B, L, n_cu, n_layers, pooling) else "single"),
            "att_qs": att_qs(B, n_cu), "att_one": att_one(B, L, n_cu), "attention_launches": attention_launches(B, L, n_cu),
            "Mc": Mc(B), "row_tiles_128": _roundup(padded_rows(B, L), 128) // 128, "eligible": graph_eligible(B, L)}


PLAN_FIELDS = ("rows", "gemm", "ksplit", "attn_form")     # the fields of `form` that hac_encoder_last_plan prints


# ---- the batches of the GPU file's calls
def _batch(seed, B, L, lo, hi):
    """synth.token_batch with lengths in [lo, hi], in L columns: (ids int32 [B, L], lens)."""
    from haconvdr_amd import synth
    ids, lens = synth.token_batch(seed, B, hi, min_len=lo)
    return np.pad(ids, ((0, 0), (0, L - hi))), lens


def calls(name, n=4, seed=0x6A00):
    """The n batches a shape is called with, each with ids and lengths of its own: [(ids int32 [B, L], mask int32 [B, L], lens)].
    Shapes with a long class (L > 256): the third call has every length <= 256 -- the long-class launches of the captured graph
    find no item -- and the fourth every length > 256 except one sequence of length 1 in the middle of the batch."""
    B, L = SHAPES[name]
    out = []
    for i in range(n):
        s = seed + 1009 * sorted(SHAPES).index(name) + 17 * i
        if L > 256 and i == 2:
            ids, lens = _batch(s, B, L, 1, 256)
        elif L > 256 and i == 3:
            ids, lens = _batch(s, B, L, 257, L)
            ids, lens = ids.copy(), lens.copy()
            ids[B // 2, 1:] = 0
            ids[B // 2, 0] = 2                    # (synth.token_batch's one-token sequence: the end token alone)
            lens[B // 2] = 1
        else:
            ids, lens = _batch(s, B, L, 1, L)
        mask = (np.arange(L)[None, :] < lens[:, None]).astype(np.int32)
        out.append((np.ascontiguousarray(ids, dtype=np.int32), mask, lens.astype(np.int64)))
    return out


def pick_six(lens):
    """Six different sequences of a batch: the first, the last, the shortest, the longest and two in the middle."""
    lens = np.asarray(lens)
    B = len(lens)
    pick = []
    for b in (int(np.argmin(lens)), int(np.argmax(lens)), 0, B - 1, B // 3, 2 * B // 3):    # (one already taken: its neighbour)
        while b in pick:
            b = (b + 1) % B
        pick.append(b)
    return pick


def packed_rows(lens):
    """The rows a batch really packs (seq_offsets_kernel: roundup(len, 32) per sequence): what total_rows holds on the device."""
    return int(((np.asarray(lens, np.int64) + SEQ_ALIGN - 1) // SEQ_ALIGN * SEQ_ALIGN).sum())
