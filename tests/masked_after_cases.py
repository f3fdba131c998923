"""Inputs of the search_masked(after=) GPU tests (tests only, numpy only), kept apart from them so that
tests/test_index_masked_after.py can prove on the CPU that the inputs show what they are for: that the threshold cases tell a
kernel that selects first and filters afterwards from one that tests eligibility before the append, that the tile cases tell the
lane's own mask and bound from its tile's or its neighbour's."""
import numpy as np

from tests import after_cases, after_ref, masked_cases

D, N, NQ = masked_cases.D, masked_cases.N, masked_cases.NQ   # 96 x 5000 (79 groups, the last of 8 rows), 37 queries
K_EDGES = (1, 100, 1023, 2048)                               # 1, a middling k, 2^m - 1, HAC_MAX_K
SCAN_WAVES = 4
FMAX = np.finfo(np.float32).max


def high_water(k):
    """the compaction high-water mark of the scan16 family: C - 64 * SCAN_WAVES with C = next_pow2(k + 64 * SCAN_WAVES) -- the
    most keys of a query a workgroup holds on to after a compaction"""
    C = 1 << (k + 64 * SCAN_WAVES - 1).bit_length()
    return C - 64 * SCAN_WAVES


def cursors_at(S, depths):
    """(scores float32 [nq], rows int64 [nq]): per query the entry at depths[i] of its own UNMASKED unbounded list -- a cursor a
    search returned; whether a mask selects its row is the mask's business"""
    whole = after_ref.unbounded(S)
    sc = np.array([whole[i][0][depths[i]] for i in range(len(S))], np.float32)
    rw = np.array([whole[i][1][depths[i]] for i in range(len(S))], np.int64)
    return sc, rw


def own_depth_cursors(S):
    """cursors_at after_cases.per_query_depths: every query of a tile of 16 (and of 4) at a depth of its own, 0 .. 2047"""
    return cursors_at(S, after_cases.per_query_depths(len(S)))


# ---- thresholds: masked_p = 1, one workgroup walks every group through its compactions
THRESHOLD_KS = (10, 100)
THRESHOLD_DEPTH = 3000


def threshold_case(ascending):
    """(x [N, D], q [5, D], mask bool [N]): masked_cases.monotone_case under a dense mask that deselects every third row"""
    x, q = masked_cases.monotone_case(ascending)
    return x, q, np.arange(N) % 3 != 0


def threshold_cursors(S):
    """the cursors of the threshold cases: behind roughly the first 3000 rows of each query's unmasked list, 7 further per query"""
    return cursors_at(S, THRESHOLD_DEPTH + 7 * np.arange(len(S)))


def select_then_filter(S, mask, sc, rw, k, first):
    """What a kernel that is almost right returns: it keeps the best high_water(k) keys of a WIDER set than the eligible one --
    first = "all" rows, the "selected" rows whatever the cursor says, or the rows "behind" the cursor whatever the mask says --
    and applies the other tests afterwards.  -> I int64 [nq, k]"""
    nq, n = S.shape
    hw = high_water(k)
    I = np.full((nq, k), -1, np.int64)
    for i in range(nq):
        order = after_ref._ordered(S[i])
        behind = after_ref.eligible(S[i], sc[i], rw[i])
        wide = {"all": np.ones(n, np.bool_), "selected": mask, "behind": behind}[first]
        kept = order[wide[order]][:hw]
        kept = kept[mask[kept] & behind[kept]][:k]
        I[i, :len(kept)] = kept
    return I


# ---- cursor edges mixed inside one tile, over after_cases.hostile_case
def edge_case(S6):
    """-> (pick int64 [16], masks bool [16, n], scores float32 [16], rows int64 [16]) over hostile_case's six queries: query
    j of the tile is hostile query pick[j]; no mask of the tile selects a row of the groups 10 .. 19 (rows 640 .. 1279).
    Every cursor is one the device forms and the host form both accept."""
    n = S6.shape[1]
    pick = (np.arange(16) % 6).astype(np.int64)
    masks = masked_cases.random_masks(0xD10, 16, n, 2)
    masks[:, 20:22] = masks[:, 40] = masks[:, 4001] = True    # the planted +-Inf rows stay selected
    masks[:, 3:203:10] = True                                 # twenty raw-word rows: NaN scores among the selected
    masks[:, 640:1280] = False
    masks[6] = masks[0]                                       # (the two spellings of one cursor, under one mask)
    S = S6[pick]
    sc, rw = cursors_at(S, np.full(16, 300))                  # (12 .. 15 keep these: entry 300 of their own lists)
    sc[0], rw[0] = -0.0, 7                                    # the zero query: every scored row ties at +0.0
    sc[6], rw[6] = 0.0, 7                                     # ... the same query, the same cursor spelled +0.0
    sc[1], rw[1] = np.nan, 5                                  # a NaN score: an empty list
    sc[2], rw[2] = np.inf, 20                                 # row 20 scores +Inf for query 2: row 21 is next
    sc[3], rw[3] = -np.inf, 20                                # ... and -Inf for query 3: only the -Inf rows behind row 20
    rw[4] = -1                                                # an exhausted list, whatever the score
    rw[5] = n + 5                                             # a row the index does not hold: no row tying the score is eligible
    sc[7], rw[7] = S[7, 700], 700                             # a row in a group no mask of the tile selects
    sc[8], rw[8] = np.inf, 2 ** 32                            # query 2 again: no +Inf row is behind 2^32
    sc[9], rw[9] = np.nan, after_ref.START                    # the start: the score is not read
    sc[10], rw[10] = FMAX, 0
    sc[11], rw[11] = -FMAX, 3
    return pick, masks, sc.astype(np.float32), rw.astype(np.int64)


# ---- empty tiles
def empty_tile_masks():
    """(masks bool [3, N], mask_of int64 [NQ]): the queries 16 .. 31 -- the second tile of 16, the tiles 4 .. 7 of 4 -- use mask 2,
    which selects nothing; the others a dense and a selective mask"""
    masks = np.stack([masked_cases.random_masks(0xD20, 1, N, 2)[0], masked_cases.random_masks(0xD21, 1, N, 64)[0], np.zeros(N, np.bool_)])
    mask_of = (np.arange(NQ) % 2).astype(np.int64)
    mask_of[16:32] = 2
    return masks, mask_of


def rows_ahead_masks(S, depth, ahead):
    """bool [nq, n]: per query the first `ahead` rows of its unmasked list -- all of them ahead of a cursor at `depth` > ahead"""
    assert ahead < depth
    masks = np.zeros(S.shape, np.bool_)
    for i, (_, rows) in enumerate(after_ref.unbounded(S)):
        masks[i, rows[:ahead]] = True
    return masks


# ---- more than QUERY_CHUNK queries
CHUNK_N, CHUNK_NQ, CHUNK_K, QUERY_CHUNK = 600, 1030, 20, 1024


def chunk_case():
    """(x [600, 96], q [1030, 96], masks bool [3, 600], mask_of [1030], depths [1030]): two launches of whole tiles; query i and
    query i + 1024 stand at different depths under different masks"""
    from tests.golden import cases
    x, q, _ = cases.search_case_inputs("gauss", 0xD30, CHUNK_N, CHUNK_NQ, d=D)
    masks = np.stack([masked_cases.random_masks(0xD31 + m, 1, CHUNK_N, (2, 3, 5)[m])[0] for m in range(3)])
    i = np.arange(CHUNK_NQ)
    return x, q, masks, ((i + i // 7) % 3).astype(np.int64), ((i * 37 + 5) % 500).astype(np.int64)
