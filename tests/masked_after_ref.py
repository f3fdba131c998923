"""The reference of every search_masked(after=) assertion (tests only): include/haconvdr.h's masked_after(q, M, s_ref, b, k)
restated as after_ref over the canonical scores with every deselected (query, row) set to NaN -- a NaN-scoring row is in no
list, which is exactly the definition.  I is compared as integers, D by bits."""
import numpy as np

from tests import after_ref, masked_ref, rank_ref

FMAX = after_ref.FMAX
START = after_ref.START
bits = after_ref.bits
assert_same = after_ref.assert_same


def deselect(S, masks, mask_of):
    """S float32 [nq, n], masks bool [n] or [n_masks, n], mask_of int64 [nq] or None -> S with NaN wherever the query's own mask
    leaves the row out; a mask_of entry outside [0, n_masks) leaves every row out (the device forms' rule)"""
    S = np.asarray(S, np.float32)
    nq, n = S.shape
    masks = np.asarray(masks, np.bool_).reshape(-1, n)
    mo = masked_ref.resolve_mask_of(len(masks), nq, mask_of)
    out = np.full_like(S, np.nan)
    for i in range(nq):
        if 0 <= mo[i] < len(masks):
            out[i, masks[mo[i]]] = S[i, masks[mo[i]]]
    return out


def from_scores(S, masks, mask_of, after_scores, after_rows, k):
    """(D float32 [nq, k], I int64 [nq, k]) behind the (score, row) cursors, or (None, None) = every query from the start"""
    return after_ref.after_from_scores(deselect(S, masks, mask_of), after_scores, after_rows, k)


def from_keys(S, masks, mask_of, after_keys, pos_base, k):
    """the uint64 KEYS [nq, k] (0 = padding) below after_keys [nq] (None = the start), positions pos_base + row"""
    return after_ref.after_from_keys(deselect(S, masks, mask_of), after_keys, pos_base, k)


def unbounded(S, masks, mask_of):
    """per query the whole masked list: (scores float32 [m_i], rows int64 [m_i])"""
    return after_ref.unbounded(deselect(S, masks, mask_of))


def masked_after(oracle, x, q, masks, mask_of, after_scores, after_rows, k):
    with np.errstate(all="ignore"):
        return from_scores(rank_ref.canon_scores(oracle, x, q), masks, mask_of, after_scores, after_rows, k)
