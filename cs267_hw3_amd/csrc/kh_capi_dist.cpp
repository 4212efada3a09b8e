// kh_capi_dist.cpp — the sharded multi-GPU path of the C ABI: routing records to their owners,
// the batched find across shards, the text paths, and the migrating walk (kh_mwalk_*).
#include "kh_table.hpp"

using namespace khx;

int khx::ensure_route(kh_table* t, uint64_t n, int nranks) {
    const uint64_t m = kh::route_blocks(n) * (uint64_t)nranks + 1;
    int rc;
    if ((rc = t->route_hist.ensure(m * 8))) return rc;
    if ((rc = t->route_off.ensure(m * 8))) return rc;
    if ((rc = t->route_scratch.ensure((kh::scan_scratch_words(m) + 2) * 8))) return rc;
    return KH_OK;
}

// Splitter segments for the migrating walk (on with the table's splitters, KH_SPLIT_BITS=0 off).
bool khx::mseg_enabled(const kh_table* t) { return t->kp.split_bits > 0; }

// Splitter density of the migrating walk: the table's (1 per 256 k-mers at C3 sizes). Measured
// at one rank (C3 / C5 ms per step): segments off 15.4 / 2159, table density 17.8 / 36.5, 4x
// sparser 17.3 / 66.6 — the segment phase is mostly a fixed cost (link, jump, retag rounds),
// while sparser splitters leave longer segments (more rounds) on long chains.
kh::KParams khx::mseg_params(const kh_table* t) {
    kh::KParams p = t->kp;
    if (p.split_bits < 1) p.split_bits = 1;
    return p;
}

namespace {

// The argument checks every record route starts with (kh_route_dev, kh_route_starts*_dev).
int route_args(kh_table* t, const void* dev_recs, uint64_t n, int nranks, const void* words_out,
               const void* counts_out) {
    if (!t) return fail(KH_ERR_ARG, "null table");
    t->ctr_early = false;  // counters may change: assemble reads them on the stream
    if (nranks < 1 || nranks > kh::MAX_RANKS) return fail(KH_ERR_ARG, "nranks %d outside [1,%d]", nranks, kh::MAX_RANKS);
    if (!counts_out || (n && (!dev_recs || !words_out))) return fail(KH_ERR_ARG, "null buffer");
    return KH_OK;
}

// Buffers of a route that also marks start k-mers: the route's own, `own_bytes` of owner scratch and
// the mark buffers. The start list is bounded from host-side counts (collected_n): no device read
// (and no host sync) per call.
int route_starts_open(kh_table* t, uint64_t n, int nranks, uint64_t own_bytes, uint64_t** start_mask) {
    if (int rc = set_device(t)) return rc;
    if (int rc = ensure_route(t, n, nranks)) return rc;
    if (int rc = t->route_own.ensure(own_bytes)) return rc;
    return mark_buffers(t, n, t->collected_n, 8, start_mask, nullptr);
}

// After the route kernel marked the start k-mers: compact them (no splitter mask on this path).
int route_starts_close(kh_table* t, const void* dev_recs, uint64_t n, uint64_t* start_mask) {
    if (n)
        if (int rc = collect_marks(t, (const uint8_t*)dev_recs, n, start_mask, nullptr, t->stream)) return rc;
    t->collected_n += n;
    t->assembled = t->loc_valid = false;
    return KH_OK;
}

}  // namespace

extern "C" {

int kh_pack_text_dev(kh_table* t, const void* dev_text, uint64_t len, void* dev_recs, uint64_t* n_out) {
    if (!t || !n_out) return fail(KH_ERR_ARG, "null argument");
    const uint64_t n = len / ((uint64_t)t->kp.K + 4);  // read_kmers.hpp:64 fixed line length
    *n_out = n;
    if (!dev_recs || n == 0) return KH_OK;
    if (!dev_text) return fail(KH_ERR_ARG, "null text");
    if (!aligned16(dev_recs)) return fail(KH_ERR_ARG, "device records must be 16-byte aligned");
    if (int rc = set_device(t)) return rc;
    KH_HIP(kh::launch_pack_text(t->kp, (const char*)dev_text, n, (uint8_t*)dev_recs,
                                t->stats.as<unsigned long long>(), t->stream));
    return KH_OK;
}

int kh_route_dev(kh_table* t, const void* dev_recs, uint64_t n, int nranks, void* words_out,
                 void* counts_out) {
    if (int rc = route_args(t, dev_recs, n, nranks, words_out, counts_out)) return rc;
    if (!aligned16(dev_recs)) return fail(KH_ERR_ARG, "device records must be 16-byte aligned");
    if (int rc = set_device(t)) return rc;
    if (int rc = ensure_route(t, n, nranks)) return rc;
    if (int rc = t->route_own.ensure((n + 16) * 4)) return rc;
    KH_HIP(kh::launch_route(t->kp, (const uint8_t*)dev_recs, n, (uint32_t)nranks,
                            t->route_hist.as<uint64_t>(), t->route_off.as<uint64_t>(),
                            t->route_scratch.as<uint64_t>(), t->route_own.as<uint32_t>(), (uint64_t*)words_out,
                            (uint64_t*)counts_out, t->stream));
    return KH_OK;
}

// ---- batched find across shards (kh_find.hip): route keys by owner, answer, reorder -------------
int kh_find_route_dev(kh_table* t, const void* dev_keys, uint64_t n, int nranks, void* dev_keys_out,
                      void* dev_index_out, void* dev_counts_out) {
    if (!t) return fail(KH_ERR_ARG, "null table");
    if (nranks < 1 || nranks > kh::MAX_RANKS) return fail(KH_ERR_ARG, "nranks %d outside [1,%d]", nranks, kh::MAX_RANKS);
    if (n >> 32) return fail(KH_ERR_ARG, "%llu keys in one batch (positions are 32-bit)", (unsigned long long)n);
    if (t->staging) return fail(KH_ERR_STATE, "a staged insert is open (kh_insert_words_finish first)");
    if (n == 0) return KH_OK;
    if (!dev_keys || !dev_keys_out || !dev_index_out || !dev_counts_out) return fail(KH_ERR_ARG, "null buffer");
    if ((uintptr_t)dev_index_out & 3u) return fail(KH_ERR_ARG, "positions must be 4-byte aligned");
    if ((uintptr_t)dev_counts_out & 7u) return fail(KH_ERR_ARG, "counts must be 8-byte aligned");
    if (int rc = set_device(t)) return rc;
    if (int rc = ensure_route(t, n, nranks)) return rc;
    if (int rc = t->find_own.ensure((n + 16) * 4)) return rc;
    KH_HIP(kh::launch_find_route(t->kp, (const uint8_t*)dev_keys, n, (uint32_t)nranks, t->route_hist.as<uint64_t>(),
                                 t->route_off.as<uint64_t>(), t->route_scratch.as<uint64_t>(),
                                 t->find_own.as<uint32_t>(), (uint8_t*)dev_keys_out, (uint32_t*)dev_index_out,
                                 (uint64_t*)dev_counts_out, t->stream));
    return KH_OK;
}

int kh_find_answer_dev(kh_table* t, const void* dev_keys, uint64_t m, void* dev_ext_out) {
    if (!t) return fail(KH_ERR_ARG, "null table");
    if (t->staging) return fail(KH_ERR_STATE, "a staged insert is open (kh_insert_words_finish first)");
    if (m == 0) return KH_OK;
    if (!dev_keys || !dev_ext_out) return fail(KH_ERR_ARG, "null buffer");
    if (int rc = set_device(t)) return rc;
    if (int rc = clean_slots(t)) return rc;
    KH_HIP(kh::launch_find_answer(t->kp, (const uint8_t*)dev_keys, m, view(t), (uint8_t*)dev_ext_out, t->stream));
    return KH_OK;
}

int kh_find_gather_dev(kh_table* t, const void* dev_keys, uint64_t n, const void* dev_index,
                       const void* dev_ext_grouped, void* dev_recs_out, void* dev_found_out) {
    if (!t) return fail(KH_ERR_ARG, "null table");
    if (n >> 32) return fail(KH_ERR_ARG, "%llu keys in one batch (positions are 32-bit)", (unsigned long long)n);
    if (t->staging) return fail(KH_ERR_STATE, "a staged insert is open (kh_insert_words_finish first)");
    if (n == 0) return KH_OK;
    if (!dev_keys || !dev_index || !dev_ext_grouped || !dev_recs_out || !dev_found_out)
        return fail(KH_ERR_ARG, "null buffer");
    if ((uintptr_t)dev_index & 3u) return fail(KH_ERR_ARG, "positions must be 4-byte aligned");
    if (int rc = set_device(t)) return rc;
    if (int rc = t->find_ext.ensure((n + 16) * 2)) return rc;
    KH_HIP(kh::launch_find_gather(t->kp, (const uint8_t*)dev_keys, n, (const uint32_t*)dev_index,
                                  (const uint8_t*)dev_ext_grouped, t->find_ext.as<uint16_t>(), (uint8_t*)dev_recs_out,
                                  (uint8_t*)dev_found_out, t->stream));
    return KH_OK;
}

// ---- find over text (kh_text.hip) ---------------------------------------------------------------
static_assert(KH_TEXT_TILE == kh::TEXT_TILE, "text tile of the header comment");

int kh_find_text_dev(kh_table* t, const void* dev_text, uint64_t len, void* dev_ext_out, void* dev_counts_out) {
    if (!t) return fail(KH_ERR_ARG, "null table");
    if (t->staging) return fail(KH_ERR_STATE, "a staged insert is open (kh_insert_words_finish first)");
    if (!dev_ext_out && !dev_counts_out) return fail(KH_ERR_ARG, "no output buffer");
    if (len == 0) return KH_OK;
    if (!dev_text) return fail(KH_ERR_ARG, "null text");
    if ((uintptr_t)dev_counts_out & 7u) return fail(KH_ERR_ARG, "counts must be 8-byte aligned");
    if (int rc = set_device(t)) return rc;
    if (int rc = clean_slots(t)) return rc;
    KH_HIP(kh::launch_find_text(t->kp, (const uint8_t*)dev_text, len, view(t), (uint8_t*)dev_ext_out,
                                (unsigned long long*)dev_counts_out, t->stream));
    return KH_OK;
}

int kh_find_text(kh_table* t, const char* host_text, uint64_t len, uint8_t* host_ext_out, uint64_t* counts2) {
    if (!t) return fail(KH_ERR_ARG, "null table");
    if (t->staging) return fail(KH_ERR_STATE, "a staged insert is open (kh_insert_words_finish first)");
    if (!host_ext_out && !counts2) return fail(KH_ERR_ARG, "no output buffer");
    if (len == 0) return KH_OK;
    if (!host_text) return fail(KH_ERR_ARG, "null text");
    if (int rc = set_device(t)) return rc;
    int rc;
    if ((rc = t->stage.ensure(len))) return rc;
    if (host_ext_out && (rc = t->stage2.ensure(2 * len))) return rc;
    if ((rc = t->stage3.ensure(16))) return rc;
    KH_HIP(hipMemcpyAsync(t->stage.p, host_text, len, hipMemcpyHostToDevice, t->stream));
    if ((rc = kh_find_text_dev(t, t->stage.p, len, host_ext_out ? t->stage2.p : nullptr, t->stage3.p))) return rc;
    if (host_ext_out) KH_HIP(hipMemcpyAsync(host_ext_out, t->stage2.p, 2 * len, hipMemcpyDeviceToHost, t->stream));
    uint64_t c[2] = {0, 0};
    KH_HIP(hipMemcpyAsync(c, t->stage3.p, 16, hipMemcpyDeviceToHost, t->stream));
    KH_SYNC(t);
    if (counts2) {
        counts2[0] = c[0];
        counts2[1] = c[1];
    }
    return KH_OK;
}

int kh_text_keys_dev(kh_table* t, const void* dev_text, uint64_t len, void* dev_keys_out, void* dev_pos_out,
                     void* dev_count_out) {
    if (!t) return fail(KH_ERR_ARG, "null table");
    if (len >> 32) return fail(KH_ERR_ARG, "%llu bytes of text in one call (positions are 32-bit)", (unsigned long long)len);
    if (!dev_count_out || (len && !dev_text)) return fail(KH_ERR_ARG, "null buffer");
    if (!dev_keys_out != !dev_pos_out) return fail(KH_ERR_ARG, "keys and positions go together (both null: count only)");
    if ((uintptr_t)dev_pos_out & 3u) return fail(KH_ERR_ARG, "positions must be 4-byte aligned");
    if ((uintptr_t)dev_count_out & 7u) return fail(KH_ERR_ARG, "the count must be 8-byte aligned");
    if (int rc = set_device(t)) return rc;
    const uint64_t nt = kh::text_tiles(len);
    int rc;
    if ((rc = t->text_cnt.ensure((nt + 1) * 8)) || (rc = t->text_off.ensure((nt + 1) * 8)) ||
        (rc = t->text_scratch.ensure(kh::scan_scratch_words(nt) * 8 + 64)))
        return rc;
    KH_HIP(kh::launch_text_keys(t->kp, (const uint8_t*)dev_text, len, t->text_cnt.as<uint64_t>(),
                                t->text_off.as<uint64_t>(), t->text_scratch.as<uint64_t>(), (uint8_t*)dev_keys_out,
                                (uint32_t*)dev_pos_out, (unsigned long long*)dev_count_out, t->stream));
    return KH_OK;
}

int kh_route_starts_dev(kh_table* t, const void* dev_recs, uint64_t n, int nranks, void* words_out,
                        void* counts_out) {
    if (int rc = route_args(t, dev_recs, n, nranks, words_out, counts_out)) return rc;
    if (!aligned16(dev_recs)) return fail(KH_ERR_ARG, "device records must be 16-byte aligned");
    uint64_t* start_mask;
    if (int rc = route_starts_open(t, n, nranks, (n + 16) * 4, &start_mask)) return rc;
    KH_HIP(kh::launch_route(t->kp, (const uint8_t*)dev_recs, n, (uint32_t)nranks,
                            t->route_hist.as<uint64_t>(), t->route_off.as<uint64_t>(),
                            t->route_scratch.as<uint64_t>(), t->route_own.as<uint32_t>(), (uint64_t*)words_out,
                            (uint64_t*)counts_out, t->stream, n ? start_mask : nullptr,
                            mseg_enabled(t) ? t->route_spl.as<unsigned long long>() : nullptr));
    return route_starts_close(t, dev_recs, n, start_mask);
}

int kh_route_starts_win_dev(kh_table* t, const void* dev_recs, uint64_t n, int nranks, void* words_out,
                            uint64_t win, void* counts_out) {
    if (int rc = route_args(t, dev_recs, n, nranks, words_out, counts_out)) return rc;
    if (!aligned16(dev_recs) || !aligned16(words_out)) return fail(KH_ERR_ARG, "device buffers must be 16-byte aligned");
    if (win < n || win >= (1ull << 32))
        return fail(KH_ERR_ARG, "window of %llu words for %llu records (need n <= win < 2^32)", (unsigned long long)win,
                    (unsigned long long)n);
    if (t->kp.R > 15) return fail(KH_ERR_ARG, "the one-pass route takes records of <= 15 bytes (k <= 52)");
    uint64_t* start_mask;
    if (int rc = route_starts_open(t, n, nranks, kh::MAX_RANKS * 4 + 64, &start_mask)) return rc;
    KH_HIP(kh::launch_route_win(t->kp, (const uint8_t*)dev_recs, n, (uint32_t)nranks, (uint64_t*)words_out, win,
                                t->route_own.as<uint32_t>(), (uint64_t*)counts_out, n ? start_mask : nullptr,
                                t->ctr.as<unsigned long long>(), t->stats.as<unsigned long long>(), t->stream,
                                mseg_enabled(t) ? t->route_spl.as<unsigned long long>() : nullptr));
    return route_starts_close(t, dev_recs, n, start_mask);
}

int kh_route_splitters_dev(kh_table* t, void* dev_out, int nranks) {
    if (!t || !dev_out) return fail(KH_ERR_ARG, "null argument");
    if (nranks < 1 || nranks > kh::MAX_RANKS) return fail(KH_ERR_ARG, "nranks %d outside [1,%d]", nranks, kh::MAX_RANKS);
    if (int rc = set_device(t)) return rc;
    KH_HIP(hipMemcpyAsync(dev_out, t->route_spl.p, (size_t)nranks * 8, hipMemcpyDeviceToDevice, t->stream));
    return KH_OK;
}

}  // extern "C"

// ---- migrating-walker rounds --------------------------------------------------------------------

kh::MSegState khx::mseg_state(kh_table* t) {
    kh::MSegState st;
    st.len = t->ms_len.as<uint32_t>();
    st.link_hi = t->ms_hi.as<uint64_t>();
    st.link_lo = t->ms_lo.as<uint64_t>();
    st.has_link = t->ms_has.as<uint8_t>();
    st.done = t->ms_done.as<uint8_t>();
    st.jump = t->ms_jump.as<uint64_t>();
    st.acc = t->ms_acc.as<uint64_t>();
    return st;
}

// device words of mw_misc: [0] link-scan finish count, [2] text-store count, [3] first round's
// walkers, [4] carry count of buffer 0, [5] of buffer 1
static unsigned long long* mw_word(kh_table* t, int i) { return t->mw_misc.as<unsigned long long>() + i; }

// The origin's line writer (K >= 16): its word-major first chunks (chunk c = contig c, filled by
// the record scan, k_mw_lens / k_mseg_scan), or null at K < 16.
uint64_t* khx::origin_chunks(kh_table* t, uint64_t nc) {
    if (t->kp.K < 16 || nc == 0 || t->chunk_data.ensure(nc * kh::CHUNK_WORDS * 8)) return nullptr;
    return t->chunk_data.as<uint64_t>();
}

// The origin's text, first part (after the contig offsets): at K >= 16 the line writer stores
// every line whole — heads, each contig's first CHUNK_BASES bases of its start segment (from the
// first chunks origin_chunks gave the record scan), newlines — and the word writers that follow
// cover the rest (start-segment words >= CHUNK_WORDS, splitter segments); at K < 16 the heads
// writer runs and the word writers cover every word. Returns the word writers' first word number
// (kh::WMIN_ERR: no memory). slen[c] + slen_add = k-mers of contig c's start segment.
uint32_t khx::origin_lines(kh_table* t, uint64_t nc, const uint32_t* clen, int slen_add, const uint32_t* slen,
                           bool chunks) {
    unsigned long long* ctr = t->ctr.as<unsigned long long>();
    if (chunks && t->kp.K >= 16 && nc) {
        if (t->line_first.ensure(kh::line_first_words(t->text.bytes) * 4)) return kh::WMIN_ERR;
        kh::WalkBuffers wb{};
        wb.starts = t->starts.as<uint64_t>();
        wb.n_starts = nc;
        wb.contig_len = const_cast<uint32_t*>(slen);
        wb.chunk_data = t->chunk_data.as<uint64_t>();
        wb.chunk_cap = nc;
        if (kh::launch_text_lines(t->kp, wb, clen, slen_add, t->contig_off.as<uint64_t>(), t->text.as<char>(), ctr,
                                  t->stream, t->text.bytes, t->line_first.as<uint32_t>(), t->text.bytes))
            return kh::CHUNK_WORDS;
    }
    if (kh::launch_write_heads(t->kp, t->starts.as<uint64_t>(), nc, clen, t->contig_off.as<uint64_t>(),
                               t->text.as<char>(), t->stream, t->text.bytes) != hipSuccess)
        return kh::WMIN_ERR;
    return 0;
}

// the contig text bytes: at most K + 1 per contig + 32 per word record (no device read)
int khx::text_for(kh_table* t, uint64_t nc, uint64_t word_recs) {
    return t->text.ensure(nc * (uint64_t)(t->kp.K + 1) + 32 * word_recs + 64);
}

namespace {

// kh_mwalk_end_dev / kh_mwalk_end_seg_dev, first part: size the origin's contig arrays and its text
// for word_recs word records, and close the walk bracket.
int mwalk_end_open(kh_table* t, uint64_t word_recs) {
    const uint64_t nc = t->ms_ns;
    int rc;
    if ((rc = t->contig_len.ensure((nc + 1) * 4)) || (rc = t->contig_off.ensure((nc + 1) * 8)) ||
        (rc = t->scratch.ensure(kh::scan_scratch_words(nc) * 8 + 64)) || (rc = text_for(t, nc, word_recs)))
        return rc;
    KH_HIP(hipEventRecord(t->ev_walk1, t->stream));
    return KH_OK;
}

// ... second part, once the contig lengths are known: offsets, then heads / lines. *wmin gets the
// word writers' first word number (origin_lines).
int mwalk_end_lines(kh_table* t, int slen_add, const uint32_t* slen, bool chunks, uint32_t* wmin) {
    const uint64_t nc = t->ms_ns;
    unsigned long long* ctr = t->ctr.as<unsigned long long>();
    KH_HIP(kh::launch_contig_offsets(t->kp.K, t->contig_len.as<uint32_t>(), nc, t->contig_off.as<uint64_t>(),
                                     t->scratch.as<uint64_t>(), ctr + kh::CT_OUT_BYTES, t->stream));
    if (nc == 0) KH_HIP(hipMemsetAsync(ctr + kh::CT_OUT_BYTES, 0, 8, t->stream));
    // the text is sized from a host bound (no device read): every writer stops at its end, so a
    // corrupt length or an overflowed store fails at kh_sync instead of writing past it
    *wmin = origin_lines(t, nc, t->contig_len.as<uint32_t>(), slen_add, slen, chunks);
    return *wmin == kh::WMIN_ERR ? KH_ERR_NOMEM : KH_OK;
}

// ... last part, after the word writers are queued.
int mwalk_end_close(kh_table* t) {
    KH_HIP(hipEventRecord(t->ev_mat1, t->stream));
    t->walk_timed = true;
    t->last_contigs = t->ms_ns;
    t->assembled = true;
    t->loc_valid = false;  // a new text: positions in the last one mean nothing
    t->mw_live = false;
    return KH_OK;
}

}  // namespace

extern "C" {

int kh_mwalk_begin(kh_table* t, int nranks, int rank, uint64_t total_kmers, uint64_t n_starts, uint64_t n_splitters,
                   uint64_t total_walkers, uint64_t* n_walkers) {
    if (!t) return fail(KH_ERR_ARG, "null table");
    t->ctr_early = false;  // counters may change: assemble reads them on the stream
    if (nranks < 1 || nranks > kh::MAX_RANKS || rank < 0 || rank >= nranks)
        return fail(KH_ERR_ARG, "bad rank %d of %d", rank, nranks);
    if (int rc = set_device(t)) return rc;
    if (int rc = join_succ(t)) return rc;
    if (int rc = clean_slots(t)) return rc;
    int rc;
    // the counts come from the caller (kh_counters_dev / kh_route_splitters_dev, read together
    // with its own exchange): no device read here
    const uint64_t ns = n_starts;
    if (ns >= (1ull << 31)) return fail(KH_ERR_ARG, "%llu start k-mers on one rank (max 2^31)", (unsigned long long)ns);
    uint64_t nsp = 0;
    // splitter segments: every splitter this shard owns seeds a walker too (kh_mseg.hip), on or
    // off the same way on every rank (walkers stop before splitters owned anywhere)
    t->ms_on = mseg_enabled(t) && t->words_split && !t->mw_seg_off;
    if (t->ms_on) {
        nsp = n_splitters;
        if ((rc = ensure_list(t, t->splits, t->splits_cap, nsp))) return rc;
        if (ns + nsp >= (1ull << 31))
            return fail(KH_ERR_ARG, "%llu walk segments on one rank (max 2^31)", (unsigned long long)(ns + nsp));
    }
    const uint64_t nseg = ns + nsp;
    // walkers of every rank: a rank may host (and hold back) at most all of them in a round
    t->mw_wg = total_walkers > nseg ? total_walkers : nseg;
    // text store: a walker appends each k-mer of this shard once, 32 bases per full word record,
    // and leaves at most a partial word, its finish record and a 2-record link where it ends
    // (held-back walkers flush nothing extra): shard / 32 + 4 per walker of every rank, doubled
    uint64_t store_cap = 2 * (t->n_inserted / 32 + 4 * t->mw_wg) + 4096;
    if (store_cap < t->mw_store_min) store_cap = t->mw_store_min;  // a redo sized by the last attempt
    t->mw_seg_off = false;
    t->mw_store_min = 0;
    t->mw_soft = t->mw_soft_next;
    t->mw_soft_next = 0;
    if ((rc = t->mw_misc.ensure(64)) || (rc = t->mw_store.ensure(store_cap * 16)))
        return rc;
    t->ms_ns = ns;
    t->ms_nsp = nsp;
    if (t->ms_on) {
        uint64_t cap2 = 64;
        while (cap2 < 2 * nsp + 64) cap2 <<= 1;
        t->ms_cap2 = cap2;
        if ((rc = t->ms_len.ensure((nseg + 1) * 4)) || (rc = t->ms_hi.ensure((nseg + 1) * 8)) ||
            (rc = t->ms_lo.ensure((nseg + 1) * 8)) || (rc = t->ms_has.ensure(nseg + 1)) ||
            (rc = t->ms_done.ensure(nseg + 1)) || (rc = t->ms_jump.ensure((nseg + 1) * 8)) ||
            (rc = t->ms_acc.ensure((nseg + 1) * 8)) || (rc = t->ms_stab.ensure(cap2 * 16)) ||
            (rc = t->ms_stab_id.ensure(cap2 * 4)) || (rc = t->ms_misc.ensure(64)))
            return rc;
    }
    unsigned long long* ctr = t->ctr.as<unsigned long long>();
    unsigned long long* stats = t->stats.as<unsigned long long>();
    // the caller's counts must be the device's (a mismatch fails the walk at the next sync)
    KH_HIP(kh::launch_fin_check(ctr + kh::CT_N_STARTS, ns, nullptr, 0, stats, t->stream));
    if (t->ms_on) KH_HIP(kh::launch_fin_check(ctr + kh::CT_N_SPLIT, nsp, nullptr, 0, stats, t->stream));
    t->mw_P = (uint32_t)nranks;
    t->mw_rank = (uint32_t)rank;
    t->rw_n = nseg;
    t->rw_total = total_kmers > ns ? total_kmers : ns;
    t->mw_store_n = 0;
    t->mw_store_bound = store_cap;
    t->mw_store_known = false;
    t->mw_cur = 0;
    KH_HIP(hipMemsetAsync(mw_word(t, 2), 0, 8 * 6, t->stream));  // store count, walkers, carries, long walks
    KH_HIP(hipEventRecord(t->ev_walk0, t->stream));
    t->wk_timed = false;
    // chain records: the first round's walkers read the start and splitter lists themselves and
    // look up their own k-mer first (a record covering its run is read next, as on one GPU), and
    // the records' successor runs are resolved beside the first round (k_rec_succ)
    kh::KParams ikp = t->kp;
    if (t->headrec.p && t->hcap && kh::rec_succ_fits(ikp, t->hcap)) {
        hipStream_t rs = t->stream;
        if (kh::rec_succ_side(ikp) && t->side) {
            KH_HIP(hipEventRecord(t->ev_side, t->stream));
            KH_HIP(hipStreamWaitEvent(t->side, t->ev_side, 0));
            rs = t->side;
            t->succ_pending = true;
        }
        KH_HIP(kh::launch_rec_succ(ikp, view(t), t->headrec.as<uint64_t>(), t->hcap, rs,
                                   t->succ_pending ? 1024u : 0u));
    }
    if (t->succ_pending) KH_HIP(hipEventRecord(t->ev_conv, t->side));
    if (t->ms_on) {
        // (on the side stream beside the first round, behind the record resolve, the splitter
        // table's 780K CAS slowed the round as much as they saved: C3 walk init + rounds 1.51 vs
        // 1.53 ms)
        KH_HIP(kh::launch_mseg_init(ns, nseg, (uint32_t)rank, mseg_state(t), t->stream));
        KH_HIP(kh::launch_mseg_stab(t->kp, t->splits.as<uint64_t>(), nsp, t->ms_stab.as<uint64_t>(),
                                    t->ms_stab_id.as<uint32_t>(), t->ms_cap2, t->stream));
    }
    t->mw_live = true;
    t->mw_stepped = false;
    t->assembled = t->loc_valid = false;
    if (n_walkers) *n_walkers = nseg;
    return KH_OK;
}

int kh_mwalk_round_dev(kh_table* t, const void* in_slots, uint64_t in_cap, void* out_slots, uint64_t out_cap,
                       void* dev_live) {
    if (!t || !t->mw_live) return fail(KH_ERR_STATE, "kh_mwalk_begin first");
    if (!out_slots || !dev_live || out_cap == 0) return fail(KH_ERR_ARG, "null output slots / live word");
    if (t->mw_stepped && !in_slots) return fail(KH_ERR_ARG, "null input slots");
    if (int rc = set_device(t)) return rc;
    const uint32_t P = t->mw_P;
    int rc;
    // this round's walkers: the start and splitter lists (first round), or the P slots received
    const uint64_t* src = nullptr;
    uint64_t nb = t->rw_n;  // bound (every walker is live in the first round)
    unsigned long long* n_dev = mw_word(t, 3);
    if (t->mw_stepped) {
        nb = (uint64_t)P * in_cap;
        if (nb > t->mw_wg) nb = t->mw_wg;  // walkers never multiply
        if ((rc = t->mw_list.ensure((nb + 1) * kh::MSG_WORDS * 8))) return rc;
        KH_HIP(kh::launch_slot_gather((const uint64_t*)in_slots, P, in_cap, t->mw_list.as<uint64_t>(), n_dev, nb,
                                      t->stream, t->stats.as<unsigned long long>()));
        src = t->mw_list.as<uint64_t>();
    } else {
        KH_HIP(kh::launch_add_count(n_dev, t->rw_n, nullptr, 0, t->stream));
    }
    const uint64_t cb = t->mw_wg;  // held-back messages: at most every walker
    if ((rc = t->mw_tmp.ensure((nb + 1) * kh::MSG_WORDS * 8)) || (rc = t->mw_dst.ensure(nb + 1)) ||
        (rc = t->mw_stage.ensure((nb + 1) * kh::MW_REC_SLOTS * 16)) || (rc = t->mw_nrec.ensure(nb + 1)) ||
        (rc = t->mw_off.ensure((nb + 1) * 8)) || (rc = t->scratch.ensure(kh::scan_scratch_words(nb) * 8 + 64)) ||
        (rc = t->mw_cnt.ensure((2 * P + 2) * 8)) ||
        (rc = t->mw_carry[0].ensure((cb + 1) * kh::MSG_WORDS * 8)) ||
        (rc = t->mw_carry[1].ensure((cb + 1) * kh::MSG_WORDS * 8)) || (rc = t->mw_carry_dst[0].ensure(cb + 1)) ||
        (rc = t->mw_carry_dst[1].ensure(cb + 1)) || (rc = ensure_route(t, nb + cb, (int)P)))
        return rc;
    kh::MWalkRound mw;
    mw.P = P;
    mw.rank = t->mw_rank;
    mw.split_bits = t->ms_on ? (uint32_t)mseg_params(t).split_bits : 0u;
    mw.headrec = t->headrec.as<uint64_t>();
    mw.hcap = t->headrec.p ? t->hcap : 0u;
    mw.max_steps = t->rw_total;
    mw.soft_steps = t->mw_soft;
    mw.long_ctr = mw_word(t, 6);
    mw.in = src;
    mw.starts = t->starts.as<uint64_t>();
    mw.splits = t->splits.as<uint64_t>();
    mw.ns = t->ms_ns;
    mw.n_in = nb;
    mw.n_dev = n_dev;
    mw.hot_on = t->ctr.as<unsigned long long>() + kh::CT_HOT;  // the kernel skips the bitmap when 0
    mw.tmp = t->mw_tmp.as<uint64_t>();
    mw.dst = t->mw_dst.as<uint8_t>();
    mw.stage = t->mw_stage.as<uint64_t>();
    mw.nrec = t->mw_nrec.as<uint8_t>();
    KH_HIP(kh::launch_mw_run(t->kp, view(t), mw, t->stats.as<unsigned long long>(), t->stream));
    // text records of this round -> the rank-local store at offsets continuing its device-side
    // count (sized at begin; a walk that would pass it fails instead of overrunning it)
    unsigned long long* store_n = mw_word(t, 2);
    KH_HIP(kh::launch_mw_text_offsets(mw, t->mw_off.as<uint64_t>(), t->scratch.as<uint64_t>(), store_n, t->stream));
    KH_HIP(kh::launch_mw_compact(mw, t->mw_off.as<uint64_t>(), t->mw_store.as<uint64_t>(), t->mw_store_bound,
                                 t->stats.as<unsigned long long>(), t->stream));
    // outgoing walkers (+ the ones held back last round) -> P slots of out_cap; overflow held back
    const int cur = t->mw_cur, nxt = 1 - cur;
    kh::SlotRound r;
    r.P = P;
    r.nb = nb;
    r.n_dev = n_dev;
    r.dst = mw.dst;
    r.tmp = mw.tmp;
    r.cb = t->mw_stepped ? cb : 0;
    r.carry_n = mw_word(t, 4 + cur);
    r.carry_dst = t->mw_carry_dst[cur].as<uint8_t>();
    r.carry = t->mw_carry[cur].as<uint64_t>();
    r.cap = out_cap;
    r.out = (uint64_t*)out_slots;
    r.carry_out = t->mw_carry[nxt].as<uint64_t>();
    r.carry_dst_out = t->mw_carry_dst[nxt].as<uint8_t>();
    r.carry_n_out = mw_word(t, 4 + nxt);
    r.live = (unsigned long long*)dev_live;
    r.cnt = t->mw_cnt.as<uint64_t>();
    KH_HIP(kh::launch_slot_round(r, t->route_hist.as<uint64_t>(), t->route_off.as<uint64_t>(),
                                 t->route_scratch.as<uint64_t>(), t->stream));
    t->mw_cur = nxt;
    t->mw_stepped = true;
    return KH_OK;
}

int kh_mwalk_flags_dev(kh_table* t, void* dev_out) {
    if (!t || !t->mw_live) return fail(KH_ERR_STATE, "kh_mwalk_begin first");
    if (!dev_out) return fail(KH_ERR_ARG, "null output");
    if (int rc = set_device(t)) return rc;
    KH_HIP(kh::launch_mw_flags(t->stats.as<unsigned long long>() + kh::ST_CHUNK_OVF, mw_word(t, 2), (uint64_t*)dev_out,
                               t->stream, t->mw_soft ? mw_word(t, 6) : nullptr));
    return KH_OK;
}

int kh_mwalk_short(kh_table* t, uint64_t total_kmers, uint64_t total_starts, int* armed) {
    if (!t || !armed) return fail(KH_ERR_ARG, "null argument");
    *armed = 0;
    // splitter segments cut the rounds of long contigs; where the mean contig (every rank's k-mers
    // over every rank's starts) is shorter than the splitter spacing (C3: 104 < 256) the walk goes
    // without them first, and a walker past 4 spacings ends it (the hosts then walk segmented)
    if (!mseg_enabled(t) || !t->words_split || t->mw_seg_off || !total_starts) return KH_OK;
    const int sb = mseg_params(t).split_bits;
    if (sb <= 0 || total_kmers / total_starts > (1ull << sb)) return KH_OK;
    t->mw_seg_off = true;
    t->mw_soft_next = 4ull << sb;
    *armed = 1;
    return KH_OK;
}

int kh_mwalk_abandon(kh_table* t) {
    if (!t || !t->mw_live) return fail(KH_ERR_STATE, "kh_mwalk_begin first");
    if (int rc = set_device(t)) return rc;
    if (int rc = join_succ(t)) return rc;
    KH_HIP(hipMemsetAsync(t->stats.as<unsigned long long>() + kh::ST_CHUNK_OVF, 0, 8, t->stream));
    t->mw_live = false;
    t->assembled = t->loc_valid = false;
    return KH_OK;
}

int kh_mwalk_redo(kh_table* t, uint64_t store_records) {
    if (!t || !t->mw_live) return fail(KH_ERR_STATE, "kh_mwalk_begin first");
    if (int rc = set_device(t)) return rc;
    if (int rc = join_succ(t)) return rc;
    // the overlap / overflow this walk reported is answered by the redo, not an error
    KH_HIP(hipMemsetAsync(t->stats.as<unsigned long long>() + kh::ST_CHUNK_OVF, 0, 8, t->stream));
    t->mw_seg_off = true;
    t->mw_store_min = store_records;
    t->mw_live = false;
    t->assembled = t->loc_valid = false;
    return KH_OK;
}

int kh_mwalk_text_bound(kh_table* t, uint64_t* n_records) {
    if (!t || !t->mw_live) return fail(KH_ERR_STATE, "kh_mwalk_begin first");
    if (!n_records) return fail(KH_ERR_ARG, "null output");
    *n_records = t->mw_store_bound;
    return KH_OK;
}

int kh_mwalk_text_dev(kh_table* t, void* out, void* counts) {
    if (!t || !t->mw_live) return fail(KH_ERR_STATE, "kh_mwalk_begin first");
    if (int rc = join_succ(t)) return rc;
    if (!counts || (t->mw_store_bound && !out)) return fail(KH_ERR_ARG, "null buffer");
    if (int rc = set_device(t)) return rc;
    if (int rc = ensure_route(t, t->mw_store_bound, (int)t->mw_P)) return rc;
    // the store's records (device count) grouped by origin; out holds kh_mwalk_text_bound records
    KH_HIP(kh::launch_mw_group_text(t->mw_store.as<uint64_t>(), t->mw_store_bound, t->mw_P,
                                    t->route_hist.as<uint64_t>(), t->route_off.as<uint64_t>(),
                                    t->route_scratch.as<uint64_t>(), (uint64_t*)out, (uint64_t*)counts, t->stream,
                                    mw_word(t, 2)));
    return KH_OK;
}

int kh_mwalk_end_dev(kh_table* t, const void* recs, uint64_t n) {
    if (!t || !t->mw_live) return fail(KH_ERR_STATE, "kh_mwalk_begin first");
    if (t->ms_on && t->ms_nsp)
        return fail(KH_ERR_STATE, "segmented walk: use kh_mwalk_link_dev .. kh_mwalk_end_seg_dev");
    if (n && !recs) return fail(KH_ERR_ARG, "null records");
    if (int rc = set_device(t)) return rc;
    if (int rc = mwalk_end_open(t, n)) return rc;
    const uint64_t nc = t->ms_ns;
    unsigned long long* ctr = t->ctr.as<unsigned long long>();
    KH_HIP(hipMemsetD32Async((hipDeviceptr_t)t->contig_len.p, 1, nc + 1, t->stream));
    KH_HIP(hipMemsetAsync(ctr + kh::CT_MW_FIN, 0, 8, t->stream));
    uint64_t* chunks = origin_chunks(t, nc);
    KH_HIP(kh::launch_mw_lens((const uint64_t*)recs, n, nc, t->contig_len.as<uint32_t>(), ctr + kh::CT_MW_FIN,
                              t->stream, chunks));
    // every walker came home (else kh_sync reports KH_ERR_NOT_FOUND)
    KH_HIP(kh::launch_fin_check(ctr + kh::CT_MW_FIN, nc, nullptr, 0, t->stats.as<unsigned long long>(), t->stream));
    uint32_t wmin;
    if (int rc = mwalk_end_lines(t, 0, t->contig_len.as<uint32_t>(), chunks, &wmin)) return rc;
    KH_HIP(kh::launch_mw_words(t->kp.K, (const uint64_t*)recs, n, nc, t->contig_len.as<uint32_t>(),
                               t->contig_off.as<uint64_t>(), t->text.as<char>(), t->text.bytes, t->stream, wmin));
    return mwalk_end_close(t);
}

int kh_mwalk_segments(kh_table* t, uint64_t* n_splitter_segments) {
    if (!t || !t->mw_live) return fail(KH_ERR_STATE, "kh_mwalk_begin first");
    if (!n_splitter_segments) return fail(KH_ERR_ARG, "null output");
    *n_splitter_segments = t->ms_on ? t->ms_nsp : 0;
    return KH_OK;
}

int kh_mwalk_link_dev(kh_table* t, const void* recs, uint64_t n, void* out, void* counts) {
    if (!t || !t->mw_live || !t->ms_on) return fail(KH_ERR_STATE, "no segmented migrating walk");
    if (!counts || (n && !recs)) return fail(KH_ERR_ARG, "null buffer");
    if (int rc = set_device(t)) return rc;
    const uint64_t nseg = t->ms_ns + t->ms_nsp;
    if (nseg && !out) return fail(KH_ERR_ARG, "null output");
    if (int rc = ensure_route(t, nseg, (int)t->mw_P)) return rc;
    unsigned long long* fin = t->ms_misc.as<unsigned long long>();
    // [0] finished segments, [1] the splitter count (kh_mwalk_pred_dev), [2] start-segment words
    // past the line writer's first chunks
    KH_HIP(hipMemsetAsync(fin, 0, 24, t->stream));
    const kh::MSegState st = mseg_state(t);
    t->ms_chunks = origin_chunks(t, t->ms_ns) != nullptr;
    KH_HIP(kh::launch_mseg_scan((const uint64_t*)recs, n, nseg, st, fin, t->stream,
                                t->ms_chunks ? t->chunk_data.as<uint64_t>() : nullptr, t->ms_ns, fin + 2));
    // every segment's walker came home (else kh_sync reports KH_ERR_NOT_FOUND)
    KH_HIP(kh::launch_fin_check(fin, nseg, nullptr, 0, t->stats.as<unsigned long long>(), t->stream));
    KH_HIP(kh::launch_mseg_link(t->kp, st, t->ms_ns, nseg, t->mw_P, t->mw_rank, t->route_hist.as<uint64_t>(),
                                t->route_off.as<uint64_t>(), t->route_scratch.as<uint64_t>(), (uint64_t*)out,
                                (uint64_t*)counts, t->stream));
    return KH_OK;
}

int kh_mwalk_pred_dev(kh_table* t, const void* links, uint64_t m, void* preds_out, uint64_t stride) {
    if (!t || !t->mw_live || !t->ms_on) return fail(KH_ERR_STATE, "no segmented migrating walk");
    if ((m && !links) || (stride && !preds_out)) return fail(KH_ERR_ARG, "null buffer");
    if (stride < t->ms_nsp)
        return fail(KH_ERR_ARG, "stride %llu below this rank's %llu splitter segments", (unsigned long long)stride,
                    (unsigned long long)t->ms_nsp);
    if (int rc = set_device(t)) return rc;
    const kh::MSegState st = mseg_state(t);
    KH_HIP(kh::launch_mseg_pred((const uint64_t*)links, m, t->ms_stab.as<uint64_t>(), t->ms_stab_id.as<uint32_t>(),
                                t->ms_cap2, t->ms_ns, st, t->stats.as<unsigned long long>(), t->stream));
    // nsp on the device: this rank's exact count (the host's, checked at begin)
    unsigned long long* nsp = t->ms_misc.as<unsigned long long>() + 1;
    KH_HIP(kh::launch_add_count(nsp, t->ms_nsp, nullptr, 0, t->stream));
    KH_HIP(kh::launch_mseg_preds_out(st, t->ms_ns, nsp, t->ms_nsp, stride, (uint64_t*)preds_out, t->stream));
    return KH_OK;
}

int kh_mwalk_resolve_dev(kh_table* t, const void* all_preds, uint64_t stride) {
    if (!t || !t->mw_live || !t->ms_on) return fail(KH_ERR_STATE, "no segmented migrating walk");
    const uint64_t N = (uint64_t)t->mw_P * stride;
    if (N && !all_preds) return fail(KH_ERR_ARG, "null predecessor tables");
    if (int rc = set_device(t)) return rc;
    int rc;
    const uint32_t np = kh::mseg_resolve_passes(N);
    if ((rc = t->ms_res[0].ensure((N + 1) * 8)) || (rc = t->ms_res[1].ensure((N + 1) * 8)) ||
        (rc = t->ms_res[2].ensure(N + 1)) || (rc = t->ms_res[3].ensure((N + 1) * 8)) ||
        (rc = t->ms_res[4].ensure((N + 1) * 8)) || (rc = t->ms_res[5].ensure(N + 1)) ||
        (rc = t->ms_pend.ensure((uint64_t)np * 8 + 8)))
        return rc;
    unsigned long long* nsp = t->ms_misc.as<unsigned long long>() + 1;
    KH_HIP(kh::launch_mseg_resolve((const uint64_t*)all_preds, N, stride, t->mw_rank, t->ms_ns, nsp, t->ms_nsp,
                                   mseg_state(t), t->ms_res[0].as<uint64_t>(), t->ms_res[1].as<uint64_t>(),
                                   t->ms_res[2].as<uint8_t>(), t->ms_res[3].as<uint64_t>(),
                                   t->ms_res[4].as<uint64_t>(), t->ms_res[5].as<uint8_t>(),
                                   t->ms_pend.as<unsigned long long>(), t->stream));
    return KH_OK;
}

int kh_mwalk_retag_dev(kh_table* t, const void* recs, uint64_t n, void* out, void* counts) {
    if (!t || !t->mw_live || !t->ms_on) return fail(KH_ERR_STATE, "no segmented migrating walk");
    if (!counts || (n && !recs) || (n + t->ms_nsp && !out)) return fail(KH_ERR_ARG, "null buffer");
    if (int rc = set_device(t)) return rc;
    if (int rc = ensure_route(t, n + t->ms_nsp, (int)t->mw_P)) return rc;
    const kh::MSegState st = mseg_state(t);
    KH_HIP(kh::launch_mseg_check(t->ms_ns, t->ms_ns + t->ms_nsp, st, nullptr, t->stats.as<unsigned long long>(),
                                 t->stream));
    KH_HIP(kh::launch_mseg_retag((const uint64_t*)recs, n, t->ms_ns, t->ms_nsp, st, t->mw_P,
                                 t->route_hist.as<uint64_t>(), t->route_off.as<uint64_t>(),
                                 t->route_scratch.as<uint64_t>(), (uint64_t*)out, (uint64_t*)counts, t->stream));
    return KH_OK;
}

int kh_mwalk_end_seg_dev(kh_table* t, const void* recs, uint64_t n, const void* seg_recs, uint64_t m) {
    if (!t || !t->mw_live || !t->ms_on) return fail(KH_ERR_STATE, "no segmented migrating walk");
    if ((n && !recs) || (m && !seg_recs)) return fail(KH_ERR_ARG, "null records");
    if (int rc = set_device(t)) return rc;
    if (int rc = mwalk_end_open(t, n + m)) return rc;
    const uint64_t nc = t->ms_ns;
    const kh::MSegState st = mseg_state(t);
    KH_HIP(kh::launch_mseg_lens((const uint64_t*)seg_recs, m, nc, st, t->contig_len.as<uint32_t>(), t->stream));
    uint32_t wmin;
    if (int rc = mwalk_end_lines(t, 1, st.len, t->ms_chunks, &wmin)) return rc;
    KH_HIP(kh::launch_mseg_words(t->kp.K, (const uint64_t*)recs, n, (const uint64_t*)seg_recs, m, nc, st,
                                 t->contig_off.as<uint64_t>(), t->text.as<char>(), t->text.bytes, t->stream, wmin,
                                 wmin ? t->ms_misc.as<unsigned long long>() + 2 : nullptr));
    return mwalk_end_close(t);
}

}  // extern "C"
