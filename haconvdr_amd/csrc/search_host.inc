// The searches that return top-k keys (hac_index_search*, hac_index_search_excluding*, hac_index_search_among*,
// hac_index_search_masked*, hac_index_search_grouped*, hac_index_search_after*, hac_index_search_masked_after*): everything between the C ABI and
// DeviceIndex::search_keys / search_keys_masked / search_keys_masked_after / search_keys_grouped / search_keys_after and the kernels of among.inc.  Included by flat_ip.hip behind rows_host.inc (whose
// pin_slab, check_host_ids, RowLocator and key_*_host it uses).  Every host form is built from the same plain pieces, each of
// which exists once: a shard's frame around its staging (shard_keys), the chunked query upload (for_query_chunks), the remap to
// positions of the whole index (remap_keys), the gather and merge on shard 0 (reserve_merge_ws, gather_shard_keys,
// shard_keys_to_host); what differs between the searches is a callable or the key width, never a flag.
namespace {

// ---- the shared pieces

// A shard's span table on its device, for remap_positions_kernel (several devices only); waits for the shard's stream when it
// has to upload.
int upload_spans(hac_index *idx, int si) {
    DeviceIndex *s = idx->shards[si];
    const std::vector<SpanDesc> &sp = idx->spans[si];
    if (sp.empty() || !idx->spans_dirty[si]) return HAC_OK;
    HAC_TRY(idx->ws_spans[si].reserve(sp.size() * sizeof(SpanDesc)));
    HAC_HIP(hipStreamSynchronize(s->stream));
    HAC_HIP(hipMemcpy(idx->ws_spans[si].p, sp.data(), sp.size() * sizeof(SpanDesc), hipMemcpyHostToDevice));
    idx->spans_dirty[si] = 0;
    return HAC_OK;
}
// n keys in a buffer of shard si: shard-local rows -> insertion-order positions of the whole index, enqueued on the shard's
// stream (its device current).  One device, or a shard without a span: local rows are positions, nothing is launched.
int remap_keys(hac_index *idx, int si, u64 *keys, int64_t n) {
    const std::vector<SpanDesc> &sp = idx->spans[si];
    if (idx->shards.size() == 1 || sp.empty()) return HAC_OK;
    HAC_TRY(upload_spans(idx, si));
    const SpanDesc *table = (const SpanDesc *)idx->ws_spans[si].p;
    remap_positions_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, idx->shards[si]->stream>>>(keys, (long)n, table, (int)sp.size());
    HAC_HIP(hipGetLastError());
    return HAC_OK;
}

// One shard's keys of a whole host call, [nq][kq] in its ws_keys, positions of the whole index: stage(x) enqueues on x.stream
// whatever leaves them there as local rows (its device is current, ws_keys reserved).  A shard without rows answers with
// padding only and stages nothing.  Runs on for_each_shard's threads; returns with the shard's stream idle.
template <class Stage>
int shard_keys(hac_index *idx, int si, int64_t nq, int kq, Stage stage) {
    DeviceIndex &x = *idx->shards[si];
    DeviceGuard g(x.device);
    if (!g.ok) return fail(HAC_ERR_HIP, "cannot select HIP device %d", x.device);
    const size_t nk = (size_t)nq * kq;
    HAC_TRY(x.ws_keys.reserve(nk * 8));
    if (x.ntotal == 0) {   // a shard without rows: padding only
        HAC_HIP(hipMemsetAsync(x.ws_keys.p, 0, nk * 8, x.stream));
    } else {
        HAC_TRY(stage(x));
        HAC_TRY(remap_keys(idx, si, (u64 *)x.ws_keys.p, (int64_t)nk));
    }
    HAC_HIP(hipStreamSynchronize(x.stream));
    return HAC_OK;
}

// q [nq][d] through the shard's pinned slab into ws_q, at most QC queries at a time, one chunk in flight: body(q0, nqc, rest)
// enqueues the chunk's work on x.stream; rest is the slab behind the queries, `extra` bytes per query of the largest chunk,
// the body's to stage more through.
template <class Body>
int for_query_chunks(DeviceIndex &x, const float *q, int64_t nq, int64_t QC, size_t extra, Body body) {
    const size_t q_bytes = (size_t)x.d * 4;
    QC = std::min(QC, nq);
    HAC_TRY(x.ws_q.reserve(QC * q_bytes));
    char *slab = nullptr;
    HAC_TRY(pin_slab(x, QC * (q_bytes + extra), slab));
    for (int64_t q0 = 0; q0 < nq; q0 += QC) {
        const int64_t nqc = std::min(QC, nq - q0);
        std::memcpy(slab, q + (size_t)q0 * x.d, nqc * q_bytes);
        HAC_HIP(hipMemcpyAsync(x.ws_q.p, slab, nqc * q_bytes, hipMemcpyHostToDevice, x.stream));
        HAC_TRY(body(q0, nqc, slab + QC * q_bytes));
        HAC_HIP(hipStreamSynchronize(x.stream));   // (the slab is the next chunk's)
    }
    return HAC_OK;
}

// The merge workspaces of a host call with `total` keys per shard, on shard 0: every shard's slab side by side, and the output.
int reserve_merge_ws(hac_index *idx, size_t total) {
    DeviceGuard g0(idx->shards[0]->device);
    HAC_TRY(idx->ws_lists.reserve(idx->shards.size() * total * 8));
    return idx->ws_out.reserve(total * 8);
}
// Every shard's `total` keys (in its ws_keys, its stream idle) into ws_lists, on shard 0's stream (its device current) -- never
// the null stream: the index streams are non-blocking, a legacy-stream D2D copy would not be ordered with them.
int gather_shard_keys(hac_index *idx, size_t total) {
    for (size_t si = 0; si < idx->shards.size(); ++si)
        HAC_HIP(hipMemcpyAsync((char *)idx->ws_lists.p + si * total * 8, idx->shards[si]->ws_keys.p, total * 8, hipMemcpyDeviceToDevice, idx->shards[0]->stream));
    return HAC_OK;
}

// `total` keys on s0's device -> (D, I) on the host, through s0's pinned slab a chunk at a time (s0's device is current); the
// host unpacks them (key_score_host, key_row_host)
int keys_to_host(DeviceIndex *s0, const uint64_t *final_keys, size_t total, float *D, int64_t *I) {
    const size_t chunk = (size_t)8 << 20;
    char *slab = nullptr;
    HAC_TRY(pin_slab(*s0, std::min(chunk, total) * 8, slab));
    for (size_t done = 0; done < total; done += chunk) {
        const size_t n = std::min(chunk, total - done);
        HAC_HIP(hipMemcpyAsync(slab, final_keys + done, n * 8, hipMemcpyDeviceToHost, s0->stream));
        HAC_HIP(hipStreamSynchronize(s0->stream));
        const u64 *kk = reinterpret_cast<const u64 *>(slab);
        for (size_t i = 0; i < n; ++i) {
            D[done + i] = kk[i] ? key_score_host(kk[i]) : -FLT_MAX;
            I[done + i] = kk[i] ? key_row_host(kk[i]) : -1;
        }
    }
    return HAC_OK;
}
// The end of a host search whose shards have left their [nq][k] keys (shard_keys) in their ws_keys: several devices are merged
// at k on the first one (reserve_merge_ws: by the caller, before the shards start), as search merges them; then keys_to_host.
int shard_keys_to_host(hac_index *idx, int64_t nq, int k, float *D, int64_t *I) {
    const int S = (int)idx->shards.size();
    const size_t total = (size_t)nq * k;
    DeviceIndex *s0 = idx->shards[0];
    DeviceGuard g0(s0->device);
    const uint64_t *final_keys = (const uint64_t *)s0->ws_keys.p;
    if (S > 1) {
        HAC_TRY(gather_shard_keys(idx, total));
        HAC_TRY(hac_merge_keys_device(s0->device, (const uint64_t *)idx->ws_lists.p, S, nq, k, (uint64_t *)idx->ws_out.p, s0->stream));
        final_keys = (const uint64_t *)idx->ws_out.p;
    }
    return keys_to_host(s0, final_keys, total, D, I);
}

// the answer of a host search that has nothing to search: padding only
void fill_padding(size_t total, float *D, int64_t *I, int64_t *G = nullptr) {
    std::fill(D, D + total, -FLT_MAX);
    std::fill(I, I + total, (int64_t)-1);
    if (G) std::fill(G, G + total, (int64_t)-1);
}

// The end of a *_device search on one shard: keys(ws_keys) enqueues the [nq][k] keys into the shard's ws_keys on the caller's
// stream, keys_to_results_kernel follows them there.
template <class Keys>
int keys_then_results(DeviceIndex &s, int64_t nq, int k, const int64_t *id_map_dev, float *D_dev, int64_t *I_dev, void *hip_stream, Keys keys) {
    HAC_TRY(s.ws_keys.reserve((size_t)nq * k * 8));
    HAC_TRY(keys((u64 *)s.ws_keys.p));
    return hac_keys_to_results_device(s.device, (const uint64_t *)s.ws_keys.p, nq * k, id_map_dev, D_dev, I_dev, hip_stream);
}

// ---- search and search_excluding.  The host driver of hac_index_search (e == 0: kq == k, no filter) and
// hac_index_search_excluding (the shards search, are remapped and merged at kq = k + e; the merged lists are filtered down to k
// on shard 0).  Arguments checked by the callers.  The benchmarked path: the queries go up in one piece (the exclusion lists
// behind shard 0's), D and I are unpacked on the device and come back in one copy, and a single device waits once, at the end
// -- so the shards run a frame of their own, not shard_keys (which waits, and answers for an empty shard without a search).
int search_host(hac_index *idx, const float *q, int64_t nq, int k, const int64_t *excl, int e, float *D, int64_t *I) {
    const int kq = k + e;
    const int S = (int)idx->shards.size();
    const size_t qbytes = (size_t)nq * idx->d * 4, ebytes = (size_t)nq * e * 8;
    // each shard searches its rows; positions are global (shard base + local row)
    DeviceIndex *s0 = idx->shards[0];
    HAC_TRY(reserve_merge_ws(idx, (size_t)nq * kq));   // (one device too: the filter writes ws_out)
    if (e) {
        DeviceGuard g0(s0->device);
        HAC_TRY(idx->ws_excl.reserve(ebytes));
    }
    // every shard searches its own rows on its own stream (for_each_shard)
    auto search_shard = [&](int si) -> int {
        DeviceIndex *s = idx->shards[si];
        DeviceGuard g(s->device);
        if (!g.ok) return fail(HAC_ERR_HIP, "cannot select HIP device %d", s->device);
        HAC_TRY(s->ws_q.reserve(qbytes));
        HAC_TRY(s->ws_keys.reserve((size_t)nq * kq * 8));
        const size_t xbytes = si == 0 ? ebytes : 0;   // the exclusion lists travel behind shard 0's queries
        HAC_TRY(s->pin_reserve(std::max(qbytes + xbytes, (size_t)nq * k * 12)));
        HAC_HIP(hipStreamSynchronize(s->stream));
        std::memcpy(s->h_pin.p, q, qbytes);
        HAC_HIP(hipMemcpyAsync(s->ws_q.p, s->h_pin.p, qbytes, hipMemcpyHostToDevice, s->stream));
        if (xbytes) {
            std::memcpy((char *)s->h_pin.p + qbytes, excl, xbytes);
            HAC_HIP(hipMemcpyAsync(idx->ws_excl.p, (char *)s->h_pin.p + qbytes, xbytes, hipMemcpyHostToDevice, s->stream));
        }
        HAC_TRY(s->search_keys((const float *)s->ws_q.p, nq, kq, (u64 *)s->ws_keys.p, 0u, s->stream));
        HAC_HIP(hipMemcpyAsync(s->h_err, s->ws_err.p, 8, hipMemcpyDeviceToHost, s->stream));   // checked after the final wait
        HAC_TRY(remap_keys(idx, si, (u64 *)s->ws_keys.p, nq * kq));
        if (S > 1) HAC_HIP(hipStreamSynchronize(s->stream));
        return HAC_OK;
    };
    HAC_TRY(for_each_shard(idx, search_shard));
    DeviceGuard g0(s0->device);
    const uint64_t *final_keys = (const uint64_t *)s0->ws_keys.p;
    if (S > 1) {
        HAC_TRY(gather_shard_keys(idx, (size_t)nq * kq));
        HAC_TRY(hac_merge_keys_device(s0->device, (const uint64_t *)idx->ws_lists.p, S, nq, kq, (uint64_t *)idx->ws_out.p, s0->stream));
        final_keys = (const uint64_t *)idx->ws_out.p;
    }
    if (e) {   // the kq best of all rows -> the k best of (rows minus the query's excluded rows); the merge's input slabs are free by now
        uint64_t *filtered = (uint64_t *)(S > 1 ? idx->ws_lists.p : idx->ws_out.p);
        HAC_TRY(hac_filter_keys_device(s0->device, final_keys, nq, kq, (const int64_t *)idx->ws_excl.p, e, k, filtered, s0->stream));
        final_keys = filtered;
    }
    HAC_TRY(s0->ws_D.reserve((size_t)nq * k * 4));
    HAC_TRY(s0->ws_I.reserve((size_t)nq * k * 8));
    HAC_TRY(hac_keys_to_results_device(s0->device, final_keys, nq * k, nullptr, (float *)s0->ws_D.p, (int64_t *)s0->ws_I.p, s0->stream));
    char *hp = (char *)s0->h_pin.p;
    HAC_HIP(hipMemcpyAsync(hp, s0->ws_I.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost, s0->stream));
    HAC_HIP(hipMemcpyAsync(hp + (size_t)nq * k * 8, s0->ws_D.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s0->stream));
    HAC_HIP(hipStreamSynchronize(s0->stream));
    std::memcpy(I, hp, (size_t)nq * k * 8);
    std::memcpy(D, hp + (size_t)nq * k * 8, (size_t)nq * k * 4);
    // a scan workgroup that ran into its pass bound: the results are delivered (the affected lists EMPTY), the call says so
    // (every shard's words are read and cleared before returning: a word left set would be blamed on a later search)
    return first_shard_error(idx, [](DeviceIndex *s) { return s->check_err(s->stream); });
}

// ---- search among named rows (among.inc)
int check_among_size(const char *what, int k, int64_t m) {
    if (k < 1 || k > HAC_MAX_K || m < 0 || m > HAC_MAX_AMONG)
        return fail(HAC_ERR_INVALID, "%s: k=%d, m=%lld: needs 1 <= k <= %d and 0 <= m <= %d (one LDS sort block of candidates per query)", what, k,
                    (long long)m, HAC_MAX_K, HAC_MAX_AMONG);
    return HAC_OK;
}
// keys_out[i] = the k keys of among(q[i], cand[i], k), positions pos_base + row, enqueued on `st` (nq > 0, k and m checked).  The
// [queries][P] candidate keys of at most 64 MiB of queries at a time live in ws_among, which grows by the rule of the search
// workspaces; the launches depend on (nq, m, k) only.
int among_keys_device(DeviceIndex &x, const char *what, const float *q_dev, int64_t nq, int k, const int64_t *cand_dev, int64_t m, u64 *keys_out,
                      u32 pos_base, hipStream_t st) {
    if (m == 0) {   // lists of padding only
        HAC_HIP(hipMemsetAsync(keys_out, 0, (size_t)nq * k * 8, st));
        return HAC_OK;
    }
    HAC_TRY(check_dev_ptr(q_dev, what));
    if ((uint64_t)pos_base + (uint64_t)x.ntotal > 0xFFFFFFFFull) return fail(HAC_ERR_UNSUPPORTED, "row positions exceed 32 bits");
    const u32 P = next_pow2((u32)m), bpq = (u32)((m + 255) / 256);
    const int64_t QC = std::min<int64_t>(nq, std::max<int64_t>(1, ((int64_t)64 << 20) / ((int64_t)P * 8)));   // (<= 2^23 queries: the grids fit)
    HAC_TRY(x.ws_among.reserve((size_t)QC * P * 8));
    HAC_TRY(x.upload_segs(st));
    const size_t lds = among_lds(P);
    for (int64_t off = 0; off < nq; off += QC) {
        const int64_t n = std::min(QC, nq - off);
        among_keys_kernel<<<dim3((unsigned)(n * bpq)), dim3(256), 0, st>>>(x.d_segs, x.d_rimg, x.nseg_live, q_dev + (size_t)off * x.d,
                                                                          (const long long *)cand_dev + (size_t)off * m, (long)m, bpq, P, (long)x.ntotal, x.K4,
                                                                          pos_base, (u64 *)x.ws_among.p);
        HAC_HIP(hipGetLastError());
        among_select_kernel<<<dim3((unsigned)n), dim3(AMONG_THREADS), lds, st>>>((const u64 *)x.ws_among.p, P, k, keys_out + (size_t)off * k);
        HAC_HIP(hipGetLastError());
    }
    snprintf(x.last_plan, sizeof x.last_plan, "among_keys_kernel grid=%lld among_select_kernel P=%u k=%d lds=%zu", (long long)(std::min(QC, nq) * bpq), P, k, lds);
    x.plan_text_slot = -1;
    return HAC_OK;
}
// The host form on one shard (shard_keys): cand holds the shard's local rows (-1: padding, or a row of another shard), m > 0.
// Queries and lists are staged in chunks of ~64 MiB.  A shard without rows holds no candidate -- its lists are all -1 and
// among_keys_device would answer with all-zero keys --, so shard_keys' shortcut gives the same keys.
int among_shard(hac_index *idx, int si, const float *q, int64_t nq, int k, const int64_t *cand, int64_t m) {
    return shard_keys(idx, si, nq, k, [&](DeviceIndex &x) -> int {
        const size_t q_bytes = (size_t)x.d * 4, c_bytes = (size_t)m * 8;
        const int64_t QC = std::max<int64_t>(1, std::min<int64_t>(nq, (int64_t)(((size_t)64 << 20) / (q_bytes + c_bytes))));
        HAC_TRY(x.ws_ids.reserve(QC * c_bytes));
        return for_query_chunks(x, q, nq, QC, c_bytes, [&](int64_t q0, int64_t nqc, char *lists) -> int {
            std::memcpy(lists, cand + (size_t)q0 * m, nqc * c_bytes);
            HAC_HIP(hipMemcpyAsync(x.ws_ids.p, lists, nqc * c_bytes, hipMemcpyHostToDevice, x.stream));
            return among_keys_device(x, "search_among", (const float *)x.ws_q.p, nqc, k, (const int64_t *)x.ws_ids.p, m, (u64 *)x.ws_keys.p + (size_t)q0 * k, 0u,
                                     x.stream);
        });
    });
}

// ---- search inside a bitmap (masked.inc; DeviceIndex::search_keys_masked)
int check_masked_args(const char *what, const hac_index *idx, int64_t nq, int k, int64_t n_masks, int64_t words, bool has_mask_of, bool pointers_ok) {
    if (k < 1 || k > HAC_MAX_K) return fail(HAC_ERR_INVALID, "%s: k=%d out of range [1, %d]", what, k, HAC_MAX_K);
    if (nq < 0 || !pointers_ok) return fail(HAC_ERR_INVALID, "%s: bad arguments", what);
    if (nq == 0) return HAC_OK;
    const int64_t W = (idx->ntotal + 63) / 64;
    if (words != W)
        return fail(HAC_ERR_INVALID, "%s: words=%lld, but %lld rows need %lld words per mask (a mask packed before an add or a remove?)", what, (long long)words,
                    (long long)idx->ntotal, (long long)W);
    if (n_masks < 1) return fail(HAC_ERR_INVALID, "%s: n_masks=%lld: needs at least one mask", what, (long long)n_masks);
    if (!has_mask_of && n_masks != 1 && n_masks != nq)
        return fail(HAC_ERR_INVALID, "%s: mask_of is null with %lld masks for %lld queries: needs n_masks == 1 (one mask for all) or n_masks == nq (mask i for query i)",
                    what, (long long)n_masks, (long long)nq);
    return HAC_OK;
}

// bits [s0, s0 + n) of src -> bits [d0, d0 + n) of dst, up to 64 at a time (dst's other bits stay)
void copy_bits(const u64 *src, int64_t s0, u64 *dst, int64_t d0, int64_t n) {
    while (n > 0) {
        const int so = (int)(s0 & 63), dof = (int)(d0 & 63);
        const int take = (int)std::min<int64_t>(n, 64 - std::max(so, dof));   // within one word on both sides
        const u64 field = take == 64 ? ~0ull : ((1ull << take) - 1ull);
        const u64 v = (src[s0 >> 6] >> so) & field;
        u64 &dw = dst[d0 >> 6];
        dw = (dw & ~(field << dof)) | (v << dof);
        s0 += take;
        d0 += take;
        n -= take;
    }
}

// The chunk of a masked host call that starts at the first of the queries whose masks are mask_of[0 .. left): as many queries
// as fit `budget` together with the distinct masks they name and their mask_of entries (q_bytes + 8 per query, m_bytes per
// mask), at least one query.  A chunk uploads only the masks it names, renumbered from 0 in the order they first occur.
struct MaskChunk {
    std::vector<int64_t> slot_of;    // local mask number -> the caller's mask
    std::vector<int64_t> local_of;   // per query of the chunk, its local mask number
    int64_t queries() const { return (int64_t)local_of.size(); }
};
MaskChunk pack_mask_chunk(const int64_t *mask_of, int64_t left, size_t q_bytes, size_t m_bytes, size_t budget) {
    MaskChunk c;
    std::unordered_map<int64_t, int64_t> seen;   // the caller's mask -> local number
    for (int64_t nqc = 0; nqc < left; ++nqc) {
        const int64_t mo = mask_of[nqc];
        const bool is_new = seen.find(mo) == seen.end();
        const size_t need = (size_t)(nqc + 1) * (q_bytes + 8) + (c.slot_of.size() + (is_new ? 1 : 0)) * m_bytes;
        if (nqc > 0 && need > budget) break;
        if (is_new) {
            seen.emplace(mo, (int64_t)c.slot_of.size());
            c.slot_of.push_back(mo);
        }
        c.local_of.push_back(seen[mo]);
    }
    return c;
}

// The host form on one shard (shard_keys): every query under ITS shard's slice of its mask.  mask_of: checked, one entry per
// query.  The chunks are pack_mask_chunk's, 64 MiB each: how many queries one holds depends on the masks they name, so this
// loop is not for_query_chunks.  With several devices the slice is cut out of the caller's mask span by span (SpanDesc: local0,
// count, global0).
// bounds: null (search_masked), or the shard's own bound of every query (search_masked_after: shard_bounds_host), which
// travels behind the chunk's mask_of in the slab, 8 more bytes per query, into ws_after.
int masked_shard(hac_index *idx, int si, const float *q, int64_t nq, int k, const u64 *masks, int64_t words, const int64_t *mask_of, const u64 *bounds = nullptr) {
    return shard_keys(idx, si, nq, k, [&](DeviceIndex &x) -> int {
        const bool sliced = idx->shards.size() > 1;
        const int64_t Wl = (x.ntotal + 63) / 64;   // words of a local mask
        const size_t q_bytes = (size_t)x.d * 4, m_bytes = (size_t)Wl * 8, b_bytes = bounds ? 8 : 0;
        for (int64_t q0 = 0; q0 < nq;) {
            const MaskChunk c = pack_mask_chunk(mask_of + q0, nq - q0, q_bytes + b_bytes, m_bytes, (size_t)64 << 20);
            const int64_t nqc = c.queries();
            const size_t nm = c.slot_of.size();
            HAC_TRY(x.ws_q.reserve(nqc * q_bytes));
            HAC_TRY(x.ws_masks.reserve(nm * m_bytes + (size_t)nqc * 8));
            if (bounds) HAC_TRY(x.ws_after.reserve((size_t)nqc * 8));
            char *slab = nullptr;   // queries, masks, mask_of (, bounds)
            HAC_TRY(pin_slab(x, nqc * q_bytes + nm * m_bytes + (size_t)nqc * (8 + b_bytes), slab));
            std::memcpy(slab, q + (size_t)q0 * x.d, nqc * q_bytes);
            u64 *hm = reinterpret_cast<u64 *>(slab + nqc * q_bytes);
            for (size_t s = 0; s < nm; ++s) {
                const u64 *src = masks + (size_t)c.slot_of[s] * words;
                u64 *dst = hm + s * Wl;
                if (!sliced) {
                    std::memcpy(dst, src, m_bytes);
                } else {
                    std::memset(dst, 0, m_bytes);
                    for (const SpanDesc &sp : idx->spans[si]) copy_bits(src, (int64_t)sp.global0, dst, (int64_t)sp.local0, (int64_t)sp.count);
                }
            }
            std::memcpy(hm + nm * Wl, c.local_of.data(), (size_t)nqc * 8);
            HAC_HIP(hipMemcpyAsync(x.ws_q.p, slab, nqc * q_bytes, hipMemcpyHostToDevice, x.stream));
            HAC_HIP(hipMemcpyAsync(x.ws_masks.p, hm, nm * m_bytes + (size_t)nqc * 8, hipMemcpyHostToDevice, x.stream));
            const u64 *md = (const u64 *)x.ws_masks.p;
            if (bounds) {
                u64 *hb = hm + nm * Wl + nqc;
                std::memcpy(hb, bounds + q0, (size_t)nqc * 8);
                HAC_HIP(hipMemcpyAsync(x.ws_after.p, hb, (size_t)nqc * 8, hipMemcpyHostToDevice, x.stream));
                HAC_TRY(x.search_keys_masked_after((const float *)x.ws_q.p, nqc, k, md, (int64_t)nm, Wl, (const int64_t *)(md + nm * Wl), (const u64 *)x.ws_after.p,
                                                   (u64 *)x.ws_keys.p + (size_t)q0 * k, 0u, x.stream));
            } else
                HAC_TRY(x.search_keys_masked((const float *)x.ws_q.p, nqc, k, md, (int64_t)nm, Wl, (const int64_t *)(md + nm * Wl), (u64 *)x.ws_keys.p + (size_t)q0 * k, 0u,
                                             x.stream));
            HAC_HIP(hipStreamSynchronize(x.stream));   // (the slab is the next chunk's)
            q0 += nqc;
        }
        return HAC_OK;
    });
}

// ---- search by group (grouped.inc; DeviceIndex::search_keys_grouped)
int check_grouped_args(const char *what, const hac_index *idx, int64_t nq, int k, int64_t n_labels, bool pointers_ok) {
    if (k < 1 || k > HAC_MAX_K) return fail(HAC_ERR_INVALID, "%s: k=%d out of range [1, %d]", what, k, HAC_MAX_K);
    if (nq < 0 || !pointers_ok) return fail(HAC_ERR_INVALID, "%s: bad arguments", what);
    if (nq == 0) return HAC_OK;
    if (n_labels != idx->ntotal)
        return fail(HAC_ERR_INVALID, "%s: n_labels=%lld, but the index holds %lld rows: one label per row (labels made before an add or a remove?)", what,
                    (long long)n_labels, (long long)idx->ntotal);
    return HAC_OK;
}

// The host form on one shard (shard_keys): its rows under ITS slice of the labels (checked: all in [0, 2^32)), cut out of the
// caller's array span by span with several devices.  The labels are uploaded once per call, the queries in chunks of ~64 MiB.
int grouped_shard(hac_index *idx, int si, const float *q, int64_t nq, int k, const int64_t *group_of) {
    return shard_keys(idx, si, nq, k, [&](DeviceIndex &x) -> int {
        HAC_TRY(x.ws_labels.reserve((size_t)x.ntotal * 8));
        std::vector<int64_t> local;   // (lives until the stream is idle)
        const int64_t *src = group_of;
        if (idx->shards.size() > 1) {
            local.assign((size_t)x.ntotal, 0);
            int64_t covered = 0;
            for (const SpanDesc &sp : idx->spans[si]) {   // the spans tile the shard's rows and lie inside the index's: anything else is a broken table, never a guessed label
                if ((int64_t)sp.local0 != covered || (int64_t)sp.local0 + sp.count > x.ntotal || (int64_t)sp.global0 + sp.count > idx->ntotal)
                    return fail(HAC_ERR_INTERNAL, "search_grouped: span (local %u, count %u, global %u) of shard %d does not fit its %lld rows", sp.local0, sp.count, sp.global0, si,
                                (long long)x.ntotal);
                std::memcpy(local.data() + sp.local0, group_of + sp.global0, (size_t)sp.count * 8);
                covered += sp.count;
            }
            if (covered != x.ntotal) return fail(HAC_ERR_INTERNAL, "search_grouped: the spans of shard %d cover %lld of its %lld rows", si, (long long)covered, (long long)x.ntotal);
            src = local.data();
        }
        HAC_HIP(hipMemcpyAsync(x.ws_labels.p, src, (size_t)x.ntotal * 8, hipMemcpyHostToDevice, x.stream));
        HAC_HIP(hipStreamSynchronize(x.stream));
        const int64_t QC = std::max<int64_t>(1, (int64_t)(((size_t)64 << 20) / ((size_t)x.d * 4)));
        return for_query_chunks(x, q, nq, QC, 0, [&](int64_t q0, int64_t nqc, char *) -> int {
            return x.search_keys_grouped((const float *)x.ws_q.p, nqc, k, (const int64_t *)x.ws_labels.p, (u64 *)x.ws_keys.p + (size_t)q0 * k, x.stream);
        });
    });
}

// ---- search behind a cursor (after.inc; DeviceIndex::search_keys_after)
int check_after_args(const char *what, int64_t nq, int k, bool pointers_ok) {
    if (k < 1 || k > HAC_MAX_K) return fail(HAC_ERR_INVALID, "%s: k=%d out of range [1, %d]", what, k, HAC_MAX_K);
    if (nq < 0 || !pointers_ok) return fail(HAC_ERR_INVALID, "%s: bad arguments", what);
    return HAC_OK;
}

// The bound of a cursor (s, r) whose score is not NaN, r >= -1 a row in the numbering of the rows searched: the key of
// (s, r), computed in 64 bits -- r == -1 (a shard with no row at or before the cursor's) gives (ord + 1) << 32, below which
// every row tying s lies; r at or above 2^32 - 1 packs as 2^32 - 1.  after_bounds_kernel's rule, on the host.
u64 cursor_bound_host(float s, int64_t r) {
    s = s + 0.0f;
    u32 b;
    std::memcpy(&b, &s, 4);
    const u32 ord = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((u64)ord << 32) + (u64)(0xFFFFFFFFll - std::min<int64_t>(r, 0xFFFFFFFFll));
}

// Every shard's bound of every query of a host call with cursors (after_score, after_row: both null, or both [nq], the rows
// checked >= -2), bounds[shard][query]; `what` names the call in a message.  The cursor is in the numbering of the whole index:
// a shard's bound names its last row at or before the cursor's row, b_local = (its rows at global positions <= b) - 1 -- a
// shard's local order is the global order, so its rows tying s_ref behind b are exactly its rows behind b_local; -1 makes every
// tying row of the shard eligible (cursor_bound_host).  No cursors: all-ones, the start, everywhere.
int shard_bounds_host(const char *what, hac_index *idx, int64_t nq, const float *after_score, const int64_t *after_row, std::vector<std::vector<u64>> &bounds) {
    const int S = (int)idx->shards.size();
    bounds.assign(S, std::vector<u64>((size_t)nq, ~0ull));
    if (!after_row) return HAC_OK;
    const RowLocator loc(idx);   // (one device: no spans, never asked)
    std::vector<int32_t> at;
    if (S > 1) {   // the span of every cursor row the index holds
        std::vector<int64_t> inside((size_t)nq);
        for (int64_t i = 0; i < nq; ++i) inside[(size_t)i] = after_row[i] < idx->ntotal ? std::max<int64_t>(after_row[i], -1) : -1;
        at = loc.locate(inside.data(), (size_t)nq);
    }
    for (int64_t i = 0; i < nq; ++i) {
        const int64_t b = after_row[i];
        const float s = after_score[i];
        if (b == HAC_AFTER_START) continue;
        for (int si = 0; si < S; ++si) {
            int64_t r = b;
            if (S > 1 && b >= idx->ntotal) r = idx->shards[si]->ntotal - 1;   // every row of the shard lies before b
            else if (S > 1 && b >= 0) {
                const int32_t a = at[(size_t)i];
                if (a < 0) return fail(HAC_ERR_INTERNAL, "%s: no span holds row %lld of %lld", what, (long long)b, (long long)idx->ntotal);
                r = loc.rows_below(a, b, si) - (loc.shard(a) == si ? 0 : 1);
            }
            bounds[si][(size_t)i] = (b < 0 || s != s) ? 0ull : cursor_bound_host(s, r);
        }
    }
    return HAC_OK;
}
// the cursor pointers and rows of a host call: both given or both null, every row >= -2
int check_host_cursors(const char *what, int64_t nq, const float *after_score, const int64_t *after_row) {
    if ((after_score == nullptr) != (after_row == nullptr))
        return fail(HAC_ERR_INVALID, "%s: after_score and after_row go together: both given, or both null (every query from the start)", what);
    if (after_row)
        for (int64_t i = 0; i < nq; ++i)
            if (after_row[i] < HAC_AFTER_START)
                return fail(HAC_ERR_INVALID, "%s: after_row[%lld] = %lld of query %lld is below %d (a row, -1 = an exhausted list, %d = the start)", what, (long long)i,
                            (long long)after_row[i], (long long)i, HAC_AFTER_START, HAC_AFTER_START);
    return HAC_OK;
}

// The host form on one shard (shard_keys): every query under ITS shard's bound.  The queries go in chunks of ~64 MiB, each
// chunk's bounds behind its queries in the slab.
int after_shard(hac_index *idx, int si, const float *q, int64_t nq, int k, const u64 *bounds) {
    return shard_keys(idx, si, nq, k, [&](DeviceIndex &x) -> int {
        const int64_t QC = std::max<int64_t>(1, (int64_t)(((size_t)64 << 20) / ((size_t)x.d * 4 + 8)));
        HAC_TRY(x.ws_after.reserve((size_t)std::min(QC, nq) * 8));
        return for_query_chunks(x, q, nq, QC, 8, [&](int64_t q0, int64_t nqc, char *slab) -> int {
            std::memcpy(slab, bounds + q0, (size_t)nqc * 8);
            HAC_HIP(hipMemcpyAsync(x.ws_after.p, slab, (size_t)nqc * 8, hipMemcpyHostToDevice, x.stream));
            return x.search_keys_after((const float *)x.ws_q.p, nqc, k, (const u64 *)x.ws_after.p, (u64 *)x.ws_keys.p + (size_t)q0 * k, 0u, x.stream);
        });
    });
}
}  // namespace

extern "C" {

int hac_index_search_device(hac_index *idx, const float *q_dev, int64_t nq, int k, float *D_dev, int64_t *I_dev,
                            const int64_t *id_map_dev, void *hip_stream) {
    return on_single_shard(idx, "search_device", [&](DeviceIndex &s) -> int {
        HAC_TRY(check_k(k));
        if (nq < 0 || (nq > 0 && (!q_dev || !D_dev || !I_dev))) return fail(HAC_ERR_INVALID, "search: bad arguments");
        if (nq == 0) return HAC_OK;
        return keys_then_results(s, nq, k, id_map_dev, D_dev, I_dev, hip_stream,
                                 [&](u64 *keys) { return s.search_keys(q_dev, nq, k, keys, 0u, (hipStream_t)hip_stream, true); });
    });
}

// The top-k of (rows minus E), |E| <= e, lies inside the top-(k + e) of the rows, in the same order: search k + e keys, filter.
int hac_index_search_excluding_device(hac_index *idx, const float *q_dev, int64_t nq, int k, const int64_t *excl_dev, int e, float *D_dev,
                                      int64_t *I_dev, const int64_t *id_map_dev, void *hip_stream) {
    return on_single_shard(idx, "search_excluding_device", [&](DeviceIndex &s) -> int {
        HAC_TRY(check_k_e(k, e));
        if (e == 0) return hac_index_search_device(idx, q_dev, nq, k, D_dev, I_dev, id_map_dev, hip_stream);
        if (nq < 0 || (nq > 0 && (!q_dev || !excl_dev || !D_dev || !I_dev))) return fail(HAC_ERR_INVALID, "search_excluding: bad arguments");
        if (nq == 0) return HAC_OK;
        const int kq = k + e;
        HAC_TRY(s.ws_keys.reserve((size_t)nq * kq * 8));
        HAC_TRY(idx->ws_out.reserve((size_t)nq * k * 8));
        HAC_TRY(s.search_keys(q_dev, nq, kq, (u64 *)s.ws_keys.p, 0u, (hipStream_t)hip_stream, true));
        // (row ids are the positions the keys carry, pos_base = 0; an id outside [0, ntotal) is padding or names no key)
        HAC_TRY(hac_filter_keys_device(s.device, (const uint64_t *)s.ws_keys.p, nq, kq, excl_dev, e, k, (uint64_t *)idx->ws_out.p, hip_stream));
        return hac_keys_to_results_device(s.device, (const uint64_t *)idx->ws_out.p, nq * k, id_map_dev, D_dev, I_dev, hip_stream);
    });
}

int hac_index_search(hac_index *idx, const float *q, int64_t nq, int k, float *D, int64_t *I) {
    if (!idx) return fail(HAC_ERR_INVALID, "null index");
    HAC_TRY(check_k(k));
    if (nq < 0 || (nq > 0 && (!q || !D || !I))) return fail(HAC_ERR_INVALID, "search: bad arguments");
    if (nq == 0) return HAC_OK;
    return search_host(idx, q, nq, k, nullptr, 0, D, I);
}

int hac_index_search_excluding(hac_index *idx, const float *q, int64_t nq, int k, const int64_t *excl, int e, float *D, int64_t *I) {
    if (!idx) return fail(HAC_ERR_INVALID, "null index");
    HAC_TRY(check_k_e(k, e));
    if (nq < 0 || (nq > 0 && (!q || !D || !I || (e > 0 && !excl)))) return fail(HAC_ERR_INVALID, "search_excluding: bad arguments");
    if (nq == 0) return HAC_OK;
    HAC_TRY(check_host_ids("search_excluding", excl, nq, e, idx->ntotal, IdPlace::QUERY_COLUMN, "padding"));   // (-1 is padding; any other id outside the index is the caller's mistake)
    return search_host(idx, q, nq, k, excl, e, D, I);
}

int hac_index_search_among_keys_device(hac_index *idx, const float *q_dev, int64_t nq, int k, const int64_t *cand_dev, int64_t m, uint64_t *keys_dev,
                                       uint32_t pos_base, void *hip_stream) {
    return on_single_shard(idx, "search_among_keys_device", [&](DeviceIndex &s) -> int {
        HAC_TRY(check_among_size("search_among_keys_device", k, m));
        if (nq < 0 || (nq > 0 && (!q_dev || !keys_dev || (m > 0 && !cand_dev)))) return fail(HAC_ERR_INVALID, "search_among_keys_device: bad arguments");
        if (nq == 0) return HAC_OK;
        return among_keys_device(s, "search_among_keys_device", q_dev, nq, k, cand_dev, m, (u64 *)keys_dev, pos_base, (hipStream_t)hip_stream);
    });
}

int hac_index_search_among_device(hac_index *idx, const float *q_dev, int64_t nq, int k, const int64_t *cand_dev, int64_t m, float *D_dev, int64_t *I_dev,
                                  const int64_t *id_map_dev, void *hip_stream) {
    return on_single_shard(idx, "search_among_device", [&](DeviceIndex &s) -> int {
        HAC_TRY(check_among_size("search_among_device", k, m));
        if (nq < 0 || (nq > 0 && (!q_dev || !D_dev || !I_dev || (m > 0 && !cand_dev)))) return fail(HAC_ERR_INVALID, "search_among_device: bad arguments");
        if (nq == 0) return HAC_OK;
        return keys_then_results(s, nq, k, id_map_dev, D_dev, I_dev, hip_stream, [&](u64 *keys) {
            return among_keys_device(s, "search_among_device", q_dev, nq, k, cand_dev, m, keys, 0u, (hipStream_t)hip_stream);
        });
    });
}

int hac_index_search_among(hac_index *idx, const float *q, int64_t nq, int k, const int64_t *cand, int64_t m, float *D, int64_t *I) {
    if (!idx) return fail(HAC_ERR_INVALID, "null index");
    HAC_TRY(check_among_size("search_among", k, m));
    if (nq < 0 || (nq > 0 && (!q || !D || !I || (m > 0 && !cand)))) return fail(HAC_ERR_INVALID, "search_among: bad arguments");
    if (nq == 0) return HAC_OK;
    if (m == 0) {   // lists of padding only
        fill_padding((size_t)nq * k, D, I);
        return HAC_OK;
    }
    HAC_TRY(check_host_ids("search_among", cand, nq, m, idx->ntotal, IdPlace::QUERY_COLUMN, "padding"));
    // Every shard selects among the candidates it holds (one host thread each; a row lives in one shard, so no repeat crosses
    // shards), in the numbering of the whole index; the slabs are merged at k on the first device, as search merges them.
    const int S = (int)idx->shards.size();
    if (S == 1) {
        HAC_TRY(among_shard(idx, 0, q, nq, k, cand, m));
    } else {
        const RowLocator loc(idx);
        const std::vector<int32_t> at = loc.locate(cand, (size_t)(nq * m));
        std::vector<std::vector<int64_t>> local(S, std::vector<int64_t>(at.size(), -1));
        for (size_t i = 0; i < at.size(); ++i)
            if (at[i] >= 0) local[loc.shard(at[i])][i] = loc.local(at[i], cand[i]);
        HAC_TRY(reserve_merge_ws(idx, (size_t)nq * k));
        HAC_TRY(for_each_shard(idx, [&](int si) { return among_shard(idx, si, q, nq, k, local[si].data(), m); }));
    }
    return shard_keys_to_host(idx, nq, k, D, I);
}

int hac_index_search_masked_keys_device(hac_index *idx, const float *q_dev, int64_t nq, int k, const uint64_t *masks_dev, int64_t n_masks, int64_t words,
                                        const int64_t *mask_of_dev, uint64_t *keys_dev, uint32_t pos_base, void *hip_stream) {
    return on_single_shard(idx, "search_masked_keys_device", [&](DeviceIndex &s) -> int {
        HAC_TRY(check_masked_args("search_masked_keys_device", idx, nq, k, n_masks, words, mask_of_dev != nullptr, nq <= 0 || (q_dev && keys_dev && (masks_dev || words == 0))));
        if (nq == 0) return HAC_OK;
        return s.search_keys_masked(q_dev, nq, k, (const u64 *)masks_dev, n_masks, words, mask_of_dev, (u64 *)keys_dev, pos_base, (hipStream_t)hip_stream);
    });
}

int hac_index_search_masked_device(hac_index *idx, const float *q_dev, int64_t nq, int k, const uint64_t *masks_dev, int64_t n_masks, int64_t words,
                                   const int64_t *mask_of_dev, float *D_dev, int64_t *I_dev, const int64_t *id_map_dev, void *hip_stream) {
    return on_single_shard(idx, "search_masked_device", [&](DeviceIndex &s) -> int {
        HAC_TRY(check_masked_args("search_masked_device", idx, nq, k, n_masks, words, mask_of_dev != nullptr, nq <= 0 || (q_dev && D_dev && I_dev && (masks_dev || words == 0))));
        if (nq == 0) return HAC_OK;
        return keys_then_results(s, nq, k, id_map_dev, D_dev, I_dev, hip_stream, [&](u64 *keys) {
            return s.search_keys_masked(q_dev, nq, k, (const u64 *)masks_dev, n_masks, words, mask_of_dev, keys, 0u, (hipStream_t)hip_stream);
        });
    });
}

int hac_index_search_masked(hac_index *idx, const float *q, int64_t nq, int k, const uint64_t *masks, int64_t n_masks, int64_t words, const int64_t *mask_of,
                            float *D, int64_t *I) {
    if (!idx) return fail(HAC_ERR_INVALID, "null index");
    HAC_TRY(check_masked_args("search_masked", idx, nq, k, n_masks, words, mask_of != nullptr, nq <= 0 || (q && D && I && (masks || words == 0))));
    if (nq == 0) return HAC_OK;
    if (idx->ntotal == 0) {
        fill_padding((size_t)nq * k, D, I);
        return HAC_OK;
    }
    std::vector<int64_t> mo((size_t)nq);
    for (int64_t i = 0; i < nq; ++i) {
        mo[(size_t)i] = mask_of ? mask_of[i] : (n_masks == 1 ? 0 : i);
        if (mo[(size_t)i] < 0 || mo[(size_t)i] >= n_masks)
            return fail(HAC_ERR_INVALID, "search_masked: mask_of[%lld] = %lld of query %lld is outside [0, %lld)", (long long)i, (long long)mo[(size_t)i], (long long)i,
                        (long long)n_masks);
    }
    // Every shard searches its own rows under its own slice of every mask (one host thread each), in the numbering of the whole
    // index; the slabs are merged at k on the first device, as search merges them.
    if (idx->shards.size() > 1) HAC_TRY(reserve_merge_ws(idx, (size_t)nq * k));
    HAC_TRY(for_each_shard(idx, [&](int si) { return masked_shard(idx, si, q, nq, k, (const u64 *)masks, words, mo.data()); }));
    return shard_keys_to_host(idx, nq, k, D, I);
}

int hac_index_search_grouped_device(hac_index *idx, const float *q_dev, int64_t nq, int k, const int64_t *group_of_dev, int64_t n_labels, float *D_dev,
                                    int64_t *I_dev, int64_t *G_dev, const int64_t *id_map_dev, void *hip_stream) {
    return on_single_shard(idx, "search_grouped_device", [&](DeviceIndex &s) -> int {
        HAC_TRY(check_grouped_args("search_grouped_device", idx, nq, k, n_labels, nq <= 0 || (q_dev && D_dev && I_dev && (group_of_dev || n_labels == 0))));
        if (nq == 0) return HAC_OK;
        hipStream_t st = (hipStream_t)hip_stream;
        HAC_TRY(s.ws_keys.reserve((size_t)nq * k * 8));
        HAC_TRY(s.search_keys_grouped(q_dev, nq, k, group_of_dev, (u64 *)s.ws_keys.p, st));
        GroupArgs gr{};
        gr.group_of = (const long long *)group_of_dev;
        gr.n_labels = (long)n_labels;
        const long n = (long)nq * k;
        grouped_results_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>((const u64 *)s.ws_keys.p, n, (const long long *)id_map_dev, gr, D_dev,
                                                                                      (long long *)I_dev, (long long *)G_dev);
        HAC_HIP(hipGetLastError());
        return HAC_OK;
    });
}

int hac_index_search_grouped(hac_index *idx, const float *q, int64_t nq, int k, const int64_t *group_of, int64_t n_labels, float *D, int64_t *I, int64_t *G) {
    if (!idx) return fail(HAC_ERR_INVALID, "null index");
    HAC_TRY(check_grouped_args("search_grouped", idx, nq, k, n_labels, nq <= 0 || (q && D && I && (group_of || n_labels == 0))));
    if (nq == 0) return HAC_OK;
    for (int64_t r = 0; r < n_labels; ++r)
        if (group_of[r] < 0 || group_of[r] > 0xFFFFFFFFll)
            return fail(HAC_ERR_INVALID, "search_grouped: group_of[%lld] = %lld is outside [0, 2^32)", (long long)r, (long long)group_of[r]);
    const size_t total = (size_t)nq * k;
    if (idx->ntotal == 0) {
        fill_padding(total, D, I, G);
        return HAC_OK;
    }
    // Every shard searches its own rows under its own slice of the labels (one host thread each) and leaves at most k distinct
    // groups per query, in the numbering of the whole index; the first device then reduces the shards' lists to the best key of
    // every label under the whole label array (grouped_select_kernel: a group may have rows on several shards).
    const int S = (int)idx->shards.size();
    DeviceIndex *s0 = idx->shards[0];
    if (S > 1) {
        HAC_TRY(reserve_merge_ws(idx, total));
        DeviceGuard g0(s0->device);
        HAC_TRY(idx->ws_glabels.reserve((size_t)n_labels * 8));
    }
    HAC_TRY(for_each_shard(idx, [&](int si) { return grouped_shard(idx, si, q, nq, k, group_of); }));
    DeviceGuard g0(s0->device);
    const uint64_t *final_keys = (const uint64_t *)s0->ws_keys.p;
    if (S > 1) {
        HAC_TRY(gather_shard_keys(idx, total));
        HAC_HIP(hipMemcpyAsync(idx->ws_glabels.p, group_of, (size_t)n_labels * 8, hipMemcpyHostToDevice, s0->stream));
        GroupArgs gr{};
        gr.group_of = (const long long *)idx->ws_glabels.p;
        gr.n_labels = (long)n_labels;
        const int Cm = DeviceIndex::grouped_select_cm(k);
        grouped_select_kernel<<<dim3((unsigned)nq), dim3(256), (size_t)Cm * 16, s0->stream>>>((const u64 *)idx->ws_lists.p, S, total, (size_t)k, nullptr, 0u, k, Cm, gr,
                                                                                            (u64 *)idx->ws_out.p);
        HAC_HIP(hipGetLastError());
        final_keys = (const uint64_t *)idx->ws_out.p;
    }
    HAC_TRY(keys_to_host(s0, final_keys, total, D, I));
    if (G)
        for (size_t i = 0; i < total; ++i) G[i] = I[i] >= 0 ? group_of[I[i]] : (int64_t)-1;
    return HAC_OK;
}

int hac_index_search_after_keys_device(hac_index *idx, const float *q_dev, int64_t nq, int k, const uint64_t *after_keys_dev, uint64_t *keys_dev, uint32_t pos_base,
                                       void *hip_stream) {
    return on_single_shard(idx, "search_after_keys_device", [&](DeviceIndex &s) -> int {
        HAC_TRY(check_after_args("search_after_keys_device", nq, k, nq <= 0 || (q_dev && keys_dev)));
        if (nq == 0) return HAC_OK;
        return s.search_keys_after(q_dev, nq, k, (const u64 *)after_keys_dev, (u64 *)keys_dev, pos_base, (hipStream_t)hip_stream);
    });
}

int hac_index_search_after_device(hac_index *idx, const float *q_dev, int64_t nq, int k, const float *after_score_dev, const int64_t *after_row_dev, float *D_dev,
                                  int64_t *I_dev, const int64_t *id_map_dev, void *hip_stream) {
    return on_single_shard(idx, "search_after_device", [&](DeviceIndex &s) -> int {
        HAC_TRY(check_after_args("search_after_device", nq, k, nq <= 0 || (q_dev && D_dev && I_dev)));
        if ((after_score_dev == nullptr) != (after_row_dev == nullptr))
            return fail(HAC_ERR_INVALID, "search_after_device: after_score and after_row go together: both given, or both null (every query from the start)");
        if (nq == 0) return HAC_OK;
        hipStream_t st = (hipStream_t)hip_stream;
        const u64 *bounds = nullptr;
        if (after_row_dev) {
            HAC_TRY(s.ws_after.reserve((size_t)nq * 8));
            after_bounds_kernel<<<dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st>>>(after_score_dev, (const long long *)after_row_dev, (long)nq, (u64 *)s.ws_after.p);
            HAC_HIP(hipGetLastError());
            bounds = (const u64 *)s.ws_after.p;
        }
        return keys_then_results(s, nq, k, id_map_dev, D_dev, I_dev, hip_stream,
                                 [&](u64 *keys) { return s.search_keys_after(q_dev, nq, k, bounds, keys, 0u, st); });
    });
}

int hac_index_search_after(hac_index *idx, const float *q, int64_t nq, int k, const float *after_score, const int64_t *after_row, float *D, int64_t *I) {
    if (!idx) return fail(HAC_ERR_INVALID, "null index");
    HAC_TRY(check_after_args("search_after", nq, k, nq <= 0 || (q && D && I)));
    HAC_TRY(check_host_cursors("search_after", nq, after_score, after_row));
    if (nq == 0) return HAC_OK;
    if (idx->ntotal == 0) {
        fill_padding((size_t)nq * k, D, I);
        return HAC_OK;
    }
    // Every shard searches its own rows behind its own bound (one host thread each: shard_bounds_host).  The slabs are remapped
    // and merged at k on the first device, as search merges them.
    const int S = (int)idx->shards.size();
    std::vector<std::vector<u64>> bounds;
    HAC_TRY(shard_bounds_host("search_after", idx, nq, after_score, after_row, bounds));
    if (S > 1) HAC_TRY(reserve_merge_ws(idx, (size_t)nq * k));
    HAC_TRY(for_each_shard(idx, [&](int si) { return after_shard(idx, si, q, nq, k, bounds[si].data()); }));
    return shard_keys_to_host(idx, nq, k, D, I);
}

int hac_index_search_masked_after_keys_device(hac_index *idx, const float *q_dev, int64_t nq, int k, const uint64_t *masks_dev, int64_t n_masks, int64_t words,
                                              const int64_t *mask_of_dev, const uint64_t *after_keys_dev, uint64_t *keys_dev, uint32_t pos_base, void *hip_stream) {
    return on_single_shard(idx, "search_masked_after_keys_device", [&](DeviceIndex &s) -> int {
        const bool ptrs = nq <= 0 || (q_dev && keys_dev && (masks_dev || words == 0));
        HAC_TRY(check_after_args("search_masked_after_keys_device", nq, k, ptrs));
        HAC_TRY(check_masked_args("search_masked_after_keys_device", idx, nq, k, n_masks, words, mask_of_dev != nullptr, ptrs));
        if (nq == 0) return HAC_OK;
        return s.search_keys_masked_after(q_dev, nq, k, (const u64 *)masks_dev, n_masks, words, mask_of_dev, (const u64 *)after_keys_dev, (u64 *)keys_dev, pos_base,
                                          (hipStream_t)hip_stream);
    });
}

int hac_index_search_masked_after_device(hac_index *idx, const float *q_dev, int64_t nq, int k, const uint64_t *masks_dev, int64_t n_masks, int64_t words,
                                         const int64_t *mask_of_dev, const float *after_score_dev, const int64_t *after_row_dev, float *D_dev, int64_t *I_dev,
                                         const int64_t *id_map_dev, void *hip_stream) {
    return on_single_shard(idx, "search_masked_after_device", [&](DeviceIndex &s) -> int {
        const bool ptrs = nq <= 0 || (q_dev && D_dev && I_dev && (masks_dev || words == 0));
        HAC_TRY(check_after_args("search_masked_after_device", nq, k, ptrs));
        HAC_TRY(check_masked_args("search_masked_after_device", idx, nq, k, n_masks, words, mask_of_dev != nullptr, ptrs));
        if ((after_score_dev == nullptr) != (after_row_dev == nullptr))
            return fail(HAC_ERR_INVALID, "search_masked_after_device: after_score and after_row go together: both given, or both null (every query from the start)");
        if (nq == 0) return HAC_OK;
        hipStream_t st = (hipStream_t)hip_stream;
        const u64 *bounds = nullptr;
        if (after_row_dev) {
            HAC_TRY(s.ws_after.reserve((size_t)nq * 8));
            after_bounds_kernel<<<dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st>>>(after_score_dev, (const long long *)after_row_dev, (long)nq, (u64 *)s.ws_after.p);
            HAC_HIP(hipGetLastError());
            bounds = (const u64 *)s.ws_after.p;
        }
        return keys_then_results(s, nq, k, id_map_dev, D_dev, I_dev, hip_stream, [&](u64 *keys) {
            return s.search_keys_masked_after(q_dev, nq, k, (const u64 *)masks_dev, n_masks, words, mask_of_dev, bounds, keys, 0u, st);
        });
    });
}

int hac_index_search_masked_after(hac_index *idx, const float *q, int64_t nq, int k, const uint64_t *masks, int64_t n_masks, int64_t words, const int64_t *mask_of,
                                  const float *after_score, const int64_t *after_row, float *D, int64_t *I) {
    if (!idx) return fail(HAC_ERR_INVALID, "null index");
    const bool ptrs = nq <= 0 || (q && D && I && (masks || words == 0));
    HAC_TRY(check_after_args("search_masked_after", nq, k, ptrs));
    HAC_TRY(check_masked_args("search_masked_after", idx, nq, k, n_masks, words, mask_of != nullptr, ptrs));
    HAC_TRY(check_host_cursors("search_masked_after", nq, after_score, after_row));
    if (nq == 0) return HAC_OK;
    std::vector<int64_t> mo((size_t)nq);
    for (int64_t i = 0; i < nq; ++i) {
        mo[(size_t)i] = mask_of ? mask_of[i] : (n_masks == 1 ? 0 : i);
        if (mo[(size_t)i] < 0 || mo[(size_t)i] >= n_masks)
            return fail(HAC_ERR_INVALID, "search_masked_after: mask_of[%lld] = %lld of query %lld is outside [0, %lld)", (long long)i, (long long)mo[(size_t)i],
                        (long long)i, (long long)n_masks);
    }
    if (idx->ntotal == 0) {
        fill_padding((size_t)nq * k, D, I);
        return HAC_OK;
    }
    // Every shard searches its own rows under its own slice of every mask, behind its own bound (one host thread each), in the
    // numbering of the whole index; the slabs are merged at k on the first device, as search merges them.
    std::vector<std::vector<u64>> bounds;
    HAC_TRY(shard_bounds_host("search_masked_after", idx, nq, after_score, after_row, bounds));
    if (idx->shards.size() > 1) HAC_TRY(reserve_merge_ws(idx, (size_t)nq * k));
    HAC_TRY(for_each_shard(idx, [&](int si) { return masked_shard(idx, si, q, nq, k, (const u64 *)masks, words, mo.data(), bounds[si].data()); }));
    return shard_keys_to_host(idx, nq, k, D, I);
}

}  // extern "C"
