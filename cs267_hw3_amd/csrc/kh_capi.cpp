// kh_capi.cpp — C ABI implementation (include/kmer_hash_amd.h), core part: errors, device buffers,
// table lifetime, HIP streams/events, lookups on one table, stats and the device memory helpers.
// The insert pipeline is in kh_capi_insert.cpp, the single-GPU walk in kh_capi_walk.cpp, the sharded
// path (routes, batched find, text, migrating walk) in kh_capi_dist.cpp, the position index in
// kh_capi_locate.cpp; kh_table.hpp is what they share.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <new>
#include <string>

#include "kh_table.hpp"

using namespace khx;

namespace {

thread_local std::string g_err;

// device bytes held by every table's buffers in this process, and their high-water mark
// (kh_device_bytes: checks tools/mem_model.py against what the sharded path really allocates)
std::atomic<uint64_t> g_dev_bytes{0}, g_dev_peak{0};

void dev_account(int64_t delta) {
    const uint64_t now = g_dev_bytes.fetch_add((uint64_t)delta) + (uint64_t)delta;
    uint64_t pk = g_dev_peak.load();
    while (now > pk && !g_dev_peak.compare_exchange_weak(pk, now)) {
    }
}

}  // namespace

int khx::fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int DevBuf::ensure(uint64_t want) {
    if (want <= bytes && p) return KH_OK;
    release();
    if (want == 0) want = 16;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
        p = nullptr;
        return fail(KH_ERR_NOMEM, "hipMalloc(%llu) failed: %s", (unsigned long long)want,
                    hipGetErrorString(e));
    }
    bytes = want;
    dev_account((int64_t)want);
    return KH_OK;
}

void DevBuf::release() {
    if (p) {
        (void)hipFree(p);
        dev_account(-(int64_t)bytes);
    }
    p = nullptr;
    bytes = 0;
}

void kh_set_error_internal(const char* msg) { g_err = msg ? msg : ""; }

bool kh::debug_flag(const char* name) {
    const char* e = getenv("KH_DEBUG");
    if (!e || !*e) return false;
    const size_t n = strlen(name);
    for (const char* p = e; (p = strstr(p, name)) != nullptr; p += n)
        if ((p == e || p[-1] == ',') && (p[n] == 0 || p[n] == ',')) return true;
    return false;
}

int khx::set_device(const kh_table* t) {
    KH_HIP(hipSetDevice(t->device));
    return KH_OK;
}

int khx::ensure_list(kh_table* t, DevBuf& buf, uint64_t& cap, uint64_t need) {
    if (need <= cap) return KH_OK;
    const uint64_t W = (uint64_t)t->kp.W;
    uint64_t newcap = need < 1024 ? 1024 : need;
    if (newcap < 2 * cap) newcap = 2 * cap;  // geometric: many small batches stay O(n) copies
    DevBuf nb;
    int rc = nb.ensure(newcap * W * 8);
    if (rc) return rc;
    if (buf.p && cap)
        KH_HIP(hipMemcpyAsync(nb.p, buf.p, cap * W * 8, hipMemcpyDeviceToDevice, t->stream));
    KH_SYNC(t);
    buf.release();
    buf = nb;
    nb.p = nullptr;
    cap = newcap;
    return KH_OK;
}

int khx::ensure_starts(kh_table* t, uint64_t need) { return ensure_list(t, t->starts, t->starts_cap, need); }

int khx::read_ctr(kh_table* t, int idx, uint64_t* v) {
    unsigned long long x = 0;
    KH_HIP(hipMemcpyAsync(&x, t->ctr.as<unsigned long long>() + idx, sizeof x,
                          hipMemcpyDeviceToHost, t->stream));
    KH_SYNC(t);
    *v = x;
    return KH_OK;
}

// First device-side error of a copy of the stats, as a status code.
int khx::stats_status(const unsigned long long* st) {
    if (st[kh::ST_FULL]) return fail(KH_ERR_FULL, "table full: %llu probes wrapped", st[kh::ST_FULL]);
    if (st[kh::ST_DUP]) return fail(KH_ERR_DUPLICATE, "%llu duplicate k-mers inserted", st[kh::ST_DUP]);
    if (st[kh::ST_BAD_EXT])
        return fail(KH_ERR_BAD_BASE, "%llu extension bytes outside {A,C,G,T,F}", st[kh::ST_BAD_EXT]);
    if (st[kh::ST_MISSING])
        return fail(KH_ERR_NOT_FOUND, "Error: k-mer not found in hash map (%llu walks)",
                    st[kh::ST_MISSING]);
    if (st[kh::ST_CYCLE]) return fail(KH_ERR_CYCLE, "%llu walks exceeded the table size", st[kh::ST_CYCLE]);
    if (st[kh::ST_SPIN]) return fail(KH_ERR_HIP, "%llu inserts timed out on a slot", st[kh::ST_SPIN]);
    if (st[kh::ST_CHUNK_OVF])
        return fail(KH_ERR_NOMEM, "walker output overflow or overlapping walks (malformed input; kh_assemble redoes "
                                  "such a walk unsegmented)");
    if (st[kh::ST_BAD_BASE])
        return fail(KH_ERR_BAD_BASE, "%llu k-mer lines with a base outside {A,C,G,T}", st[kh::ST_BAD_BASE]);
    return KH_OK;
}

// First device-side error, as a status code.
int khx::check_stats(kh_table* t) {
    unsigned long long st[kh::ST_NUM];
    KH_HIP(hipMemcpyAsync(st, t->stats.p, sizeof st, hipMemcpyDeviceToHost, t->stream));
    KH_SYNC(t);
    return stats_status(st);
}

// Empty the slot array (all-ones) unless that already happened since the last clear.
int khx::clean_slots(kh_table* t) {
    if (!t->slots_stale) return KH_OK;
    KH_HIP(hipMemsetAsync(t->slots.p, 0xff, t->cap * (uint64_t)t->kp.W * 8, t->stream));
    t->slots_stale = false;
    return KH_OK;
}

// The migrating walk resolves record successors on the side stream beside its rounds: the
// table's stream waits for it before anything rewrites the records (end of the walk, clear).
int khx::join_succ(kh_table* t) {
    if (!t->succ_pending) return KH_OK;
    KH_HIP(hipStreamWaitEvent(t->stream, t->ev_conv, 0));
    t->succ_pending = false;
    return KH_OK;
}

namespace {

// Balanced region bounds (kh_build.hip k_bounds) above load 0.6, where equal slices overflow
// (at load 0.5 they measured slower: C3 8.84 -> 17.5 ms).
bool balanced_bounds(const kh_table* t) { return t->load > 0.6; }

// Capacity and splitter density for n_kmers (kh_create, kh_reserve).
void size_table(kh_table* t, uint64_t n_kmers) {
    t->n_kmers = n_kmers;
    // splitter density: ~1 per 2^bits k-mers; enough extra walkers for long-chain inputs (C2, C5)
    // at a few % more walkers on short-contig inputs. KH_SPLIT_BITS overrides (0 = off).
    // Collected at insert: 1 per 2^bits k-mers, bits = clamp(log2(n / 2^20) + 1, 4, 12); the walk
    // then uses a subset sized from the start count (kh_assemble_dev).
    int bits = 1;
    while (bits < 12 && (n_kmers >> (20 + bits)) != 0) ++bits;
    bits = bits < 4 ? 4 : bits;
    t->split_forced = false;
    if (const char* e = getenv("KH_SPLIT_BITS")) {  // tests: dense, sparse or no splitters
        bits = atoi(e);
        t->split_forced = true;
    }
    t->kp.split_bits = bits < 0 ? 0 : (bits > 30 ? 30 : bits);
    const double c = (double)(n_kmers ? n_kmers : 1) / t->load;
    t->cap = (uint64_t)c;
    if ((double)t->cap < c) t->cap++;
    if (t->cap < 2) t->cap = 2;
    kh::set_region_bits(t->kp, t->cap);
}

}  // namespace

static_assert(KH_MSG_WORDS == kh::MSG_WORDS, "message layout");

extern "C" {

int kh_abi_version(void) { return KH_ABI_VERSION; }

int kh_device_bytes(uint64_t* now, uint64_t* peak, int reset_peak) {
    if (now) *now = g_dev_bytes.load();
    if (peak) *peak = g_dev_peak.load();
    if (reset_peak) g_dev_peak.store(g_dev_bytes.load());
    return KH_OK;
}
int kh_packed_size(int k) { return (k >= 1 && k <= KH_K_MAX) ? (k + 3) / 4 : KH_ERR_ARG; }
int kh_record_size(int k) { return (k >= 1 && k <= KH_K_MAX) ? (k + 3) / 4 + 2 : KH_ERR_ARG; }
const char* kh_last_error(void) { return g_err.c_str(); }

int kh_device_count(int* n) {
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) {
        *n = 0;
        return fail(KH_ERR_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *n = c;
    return KH_OK;
}

int kh_create(kh_table** out, int k, uint64_t n_kmers, double load_factor, int device) {
    if (!out) return fail(KH_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (k < 1 || k > KH_K_MAX) return fail(KH_ERR_ARG, "k=%d outside [1,%d]", k, KH_K_MAX);
    if (!(load_factor > 0.0 && load_factor < 1.0))
        return fail(KH_ERR_ARG, "load factor %g outside (0,1)", load_factor);
    kh_table* t = new (std::nothrow) kh_table();
    if (!t) return fail(KH_ERR_NOMEM, "host allocation failed");
    t->device = device;
    t->kp = kh::make_params(k);
    t->load = load_factor;
    if (const char* e = getenv("KH_OWNER")) t->kp.owner_mode = strcmp(e, "hash") == 0 ? 1 : 0;
    size_table(t, n_kmers);
    int rc = KH_OK;
    auto bail = [&](int r) {
        kh_destroy(t);
        return r;
    };
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return bail(fail(KH_ERR_HIP, "hipSetDevice(%d): %s", device, hipGetErrorString(e)));
    if (hipStreamCreateWithFlags(&t->own_stream, hipStreamNonBlocking) != hipSuccess)
        return bail(fail(KH_ERR_HIP, "hipStreamCreate failed"));
    t->stream = t->own_stream;
    if (hipStreamCreateWithFlags(&t->side, hipStreamNonBlocking) != hipSuccess)
        return bail(fail(KH_ERR_HIP, "hipStreamCreate failed"));
    hipEvent_t* evs[] = {&t->ev_ins0, &t->ev_ins1, &t->ev_ins2, &t->ev_walk0, &t->ev_walk1, &t->ev_mat1,
                         &t->ev_b0, &t->ev_b1, &t->ev_wk1};
    for (auto* ev : evs)
        if (hipEventCreate(ev) != hipSuccess) return bail(fail(KH_ERR_HIP, "hipEventCreate failed"));
    for (auto* ev : {&t->ev_conv, &t->ev_side, &t->ev_hot, &t->ev_ctr})
        if (hipEventCreateWithFlags(ev, hipEventDisableTiming) != hipSuccess)
            return bail(fail(KH_ERR_HIP, "hipEventCreate failed"));
    if (hipHostMalloc((void**)&t->hctr, kh::CT_NUM * 8, hipHostMallocDefault) != hipSuccess)
        return bail(fail(KH_ERR_NOMEM, "pinned host counters"));
    if ((rc = t->slots.ensure(t->cap * (uint64_t)t->kp.W * 8))) return bail(rc);
    if ((rc = t->hot.ensure(2 * kh::HOT_WORDS * 4))) return bail(rc);
    if (hipMemset(t->hot.p, 0, 2 * kh::HOT_WORDS * 4) != hipSuccess) return bail(fail(KH_ERR_HIP, "hipMemset failed"));
    t->kp.hot = t->hot.as<uint32_t>();
    // region slot ranges: equal until a balanced table's first build (lookups read them only when
    // balanced; the build always does)
    if ((rc = t->rbounds.ensure((kh::HOT_WORDS * 32 + 1) * 8))) return bail(rc);
    if (balanced_bounds(t)) t->kp.rb = t->rbounds.as<uint64_t>();
    kh::launch_bounds(t->kp, t->cap, nullptr, 0, t->rbounds.as<uint64_t>(), t->stream);
    if ((rc = t->ctr.ensure(kh::CT_NUM * 8))) return bail(rc);
    if ((rc = t->route_spl.ensure(kh::MAX_RANKS * 8))) return bail(rc);
    if ((rc = t->stats.ensure(kh::ST_NUM * 8))) return bail(rc);
    if ((rc = kh_clear(t))) return bail(rc);
    if (hipStreamSynchronize(t->stream) != hipSuccess) return bail(fail(KH_ERR_HIP, "sync failed"));
    *out = t;
    return KH_OK;
}

int kh_destroy(kh_table* t) {
    if (!t) return KH_OK;
    (void)hipSetDevice(t->device);
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    DevBuf* bufs[] = {&t->slots, &t->starts, &t->ctr, &t->stats, &t->mask, &t->mask_off,
                      &t->scratch, &t->stage, &t->stage2, &t->stage3, &t->contig_len,
                      &t->contig_off, &t->chunk_data, &t->chunk_owner, &t->chunk_seq, &t->text, &t->line_first,
                      &t->route_hist, &t->route_off, &t->route_scratch, &t->route_own, &t->splits, &t->splits_w, &t->seg_next,
                      &t->seg_key, &t->seg_contig, &t->seg_off, &t->clen, &t->stab, &t->stab_id,
                      &t->seg_jump, &t->seg_jsum, &t->seg_anchor, &t->seg_pend,
                      &t->mw_tmp, &t->mw_dst, &t->mw_stage, &t->mw_nrec, &t->mw_off,
                      &t->mw_misc, &t->mw_store, &t->ms_len, &t->ms_hi, &t->ms_lo, &t->ms_has, &t->ms_done,
                      &t->ms_jump, &t->ms_acc, &t->ms_stab, &t->ms_stab_id, &t->ms_qsrc, &t->ms_misc,
                      &t->mw_cnt, &t->mw_list, &t->mw_carry[0], &t->mw_carry[1], &t->mw_carry_dst[0],
                      &t->mw_carry_dst[1], &t->ms_res[0], &t->ms_res[1], &t->ms_res[2], &t->ms_res[3], &t->ms_res[4],
                      &t->ms_res[5], &t->ms_pend, &t->route_spl, &t->find_own, &t->find_ext,
                      &t->text_cnt, &t->text_off, &t->text_scratch, &t->pb_buf1, &t->pb_buf2, &t->pb_cnt, &t->pb_ovf, &t->headrec, &t->hot, &t->rbounds, &t->loc};
    if (t->side) (void)hipStreamSynchronize(t->side);  // k_rec_succ may still read the table
    for (auto* b : bufs) b->release();
    hipEvent_t evs[] = {t->ev_ins0, t->ev_ins1, t->ev_ins2, t->ev_walk0, t->ev_walk1, t->ev_mat1, t->ev_b0,
                        t->ev_b1, t->ev_wk1, t->ev_conv,
                        t->ev_side, t->ev_hot, t->ev_ctr};
    for (auto ev : evs)
        if (ev) (void)hipEventDestroy(ev);
    if (t->hctr) (void)hipHostFree(t->hctr);
    if (t->side) (void)hipStreamDestroy(t->side);
    if (t->own_stream) (void)hipStreamDestroy(t->own_stream);
    delete t;
    // teardown errors are not the caller's: leave the thread's HIP last-error clear, or the
    // caller's next launch check (torch's, say) reports it as its own
    (void)hipGetLastError();
    return KH_OK;
}

int kh_reserve(kh_table* t, uint64_t n_kmers) {
    if (!t) return fail(KH_ERR_ARG, "null table");
    t->ctr_early = false;  // counters may change: assemble reads them on the stream
    if (n_kmers <= t->n_kmers) return KH_OK;
    if (t->n_inserted || t->staging)
        return fail(KH_ERR_STATE, "kh_reserve on a table holding %llu k-mers (clear it first)",
                    (unsigned long long)t->n_inserted);
    if (int rc = set_device(t)) return rc;
    KH_SYNC(t);
    const uint64_t old_n = t->n_kmers;
    const int old_bits = t->kp.split_bits;
    size_table(t, n_kmers);
    // the splitter density stays the one the table was created with: every shard of a sharded
    // table must use the same (a walker stops before splitters that their owner seeds walkers at)
    t->kp.split_bits = old_bits;
    // the new slot array first: when it cannot be had, the table keeps its old one and old size
    DevBuf ns;
    if (int rc = ns.ensure(t->cap * (uint64_t)t->kp.W * 8)) {
        size_table(t, old_n);
        t->kp.split_bits = old_bits;
        return rc;
    }
    t->slots.release();
    t->slots = ns;
    ns.p = nullptr;
    t->slots_stale = true;
    t->loc_valid = false;  // one position per slot of the old array
    kh::launch_bounds(t->kp, t->cap, nullptr, 0, t->rbounds.as<uint64_t>(), t->stream);
    KH_HIP(hipGetLastError());
    return KH_OK;
}

int kh_clear(kh_table* t) {
    if (!t) return fail(KH_ERR_ARG, "null table");
    t->ctr_early = false;  // counters may change: assemble reads them on the stream
    if (int rc = set_device(t)) return rc;
    if (int rc = join_succ(t)) return rc;
    t->slots_stale = true;
    kh::FillSet f;
    f.add(t->ctr.p, kh::CT_NUM * 8, 0);
    f.add(t->stats.p, kh::ST_NUM * 8, 0);
    f.add(t->hot.p, 2 * kh::HOT_WORDS * 4, 0);  // placement by minimizer again
    f.add(t->route_spl.p, kh::MAX_RANKS * 8, 0);
    KH_HIP(kh::launch_fill(f, t->stream));
    t->n_inserted = 0;
    t->assembled = t->loc_valid = false;
    t->split_ok = true;
    t->starts_explicit = false;
    t->staging = false;
    t->stage_n = 0;
    t->collected_n = 0;
    t->words_split = true;
    return KH_OK;
}

int kh_set_stream(kh_table* t, void* s) {
    if (!t) return fail(KH_ERR_ARG, "null table");
    t->stream = s ? (hipStream_t)s : t->own_stream;
    return KH_OK;
}

int kh_sync(kh_table* t) {
    if (!t) return fail(KH_ERR_ARG, "null table");
    if (int rc = set_device(t)) return rc;
    return check_stats(t);  // one wait: the stats read is ordered after the queued work
}

uint64_t kh_capacity(const kh_table* t) { return t ? t->cap : 0; }

int kh_host_syncs(const kh_table* t, uint64_t* n) {
    if (!t || !n) return fail(KH_ERR_ARG, "null argument");
    *n = t->host_syncs;
    return KH_OK;
}

int kh_find_dev(kh_table* t, const void* dev_keys, uint64_t n, void* dev_out, void* dev_found) {
    if (!t) return fail(KH_ERR_ARG, "null table");
    if (n == 0) return KH_OK;
    if (!dev_keys || !dev_out || !dev_found) return fail(KH_ERR_ARG, "null buffer");
    if (int rc = set_device(t)) return rc;
    if (int rc = clean_slots(t)) return rc;
    KH_HIP(kh::launch_find(t->kp, (const uint8_t*)dev_keys, n, view(t), (uint8_t*)dev_out,
                           (uint8_t*)dev_found, t->stream));
    return KH_OK;
}

int kh_find(kh_table* t, const uint8_t* keys, uint64_t n, uint8_t* out, uint8_t* found) {
    if (!t) return fail(KH_ERR_ARG, "null table");
    if (n == 0) return KH_OK;
    if (!keys || !out || !found) return fail(KH_ERR_ARG, "null buffer");
    if (int rc = set_device(t)) return rc;
    const uint64_t kb = n * (uint64_t)t->kp.P, rb = n * (uint64_t)t->kp.R;
    int rc;
    if ((rc = t->stage.ensure(kb))) return rc;
    if ((rc = t->stage2.ensure(rb))) return rc;
    if ((rc = t->stage3.ensure(n))) return rc;
    KH_HIP(hipMemcpyAsync(t->stage.p, keys, kb, hipMemcpyHostToDevice, t->stream));
    if ((rc = kh_find_dev(t, t->stage.p, n, t->stage2.p, t->stage3.p))) return rc;
    KH_HIP(hipMemcpyAsync(out, t->stage2.p, rb, hipMemcpyDeviceToHost, t->stream));
    KH_HIP(hipMemcpyAsync(found, t->stage3.p, n, hipMemcpyDeviceToHost, t->stream));
    KH_SYNC(t);
    return KH_OK;
}

int kh_get_stats(kh_table* t, kh_stats* s) {
    if (!t || !s) return fail(KH_ERR_ARG, "null argument");
    if (int rc = set_device(t)) return rc;
    KH_SYNC(t);
    unsigned long long st[kh::ST_NUM], ct[kh::CT_NUM];
    KH_HIP(hipMemcpy(st, t->stats.p, sizeof st, hipMemcpyDeviceToHost));
    KH_HIP(hipMemcpy(ct, t->ctr.p, sizeof ct, hipMemcpyDeviceToHost));
    std::memset(s, 0, sizeof *s);
    s->capacity = t->cap;
    s->n_inserted = t->n_inserted;
    s->n_starts = ct[kh::CT_N_STARTS];
    if (t->assembled) {
        s->n_contigs = t->last_contigs;
        s->out_bytes = ct[kh::CT_OUT_BYTES];
        // bytes = sum(K + len) -> lookups = sum(len - 1) = bytes - contigs * (K + 1)
        s->n_lookups = s->out_bytes - s->n_contigs * ((uint64_t)t->kp.K + 1);
        const uint64_t nch = t->last_contigs + ct[kh::CT_CHUNK_NEXT];
        s->n_chunks = nch < t->chunk_cap ? nch : t->chunk_cap;
    }
    s->n_dup = st[kh::ST_DUP];
    s->n_full = st[kh::ST_FULL];
    s->n_bad_ext = st[kh::ST_BAD_EXT];
    s->n_missing = st[kh::ST_MISSING];
    s->n_cycle = st[kh::ST_CYCLE];
    s->n_spin = st[kh::ST_SPIN];
    s->n_chunk_ovf = st[kh::ST_CHUNK_OVF];
    s->n_bad_base = st[kh::ST_BAD_BASE];
    float ms = 0.f;
    if (t->ins_timed) {
        if (hipEventElapsedTime(&ms, t->ev_ins0, t->ev_ins2) == hipSuccess) s->ms_insert = ms;
        if (hipEventElapsedTime(&ms, t->ev_ins0, t->ev_ins1) == hipSuccess) s->ms_insert_kernel = ms;
    }
    if (t->walk_timed) {
        if (hipEventElapsedTime(&ms, t->ev_walk0, t->ev_walk1) == hipSuccess) s->ms_walk = ms;
        if (hipEventElapsedTime(&ms, t->ev_walk1, t->ev_mat1) == hipSuccess) s->ms_materialize = ms;
        if (t->wk_timed && hipEventElapsedTime(&ms, t->ev_walk0, t->ev_wk1) == hipSuccess) s->ms_walk_kernel = ms;
    }
    if (t->build_timed && hipEventElapsedTime(&ms, t->ev_b0, t->ev_b1) == hipSuccess) s->ms_build = ms;
    s->n_hot_regions = ct[kh::CT_HOT];
    s->n_spread_regions = ct[kh::CT_HOT2];
    s->n_overflow = t->last_insert_part ? ct[kh::CT_OVF2] : 0;
    (void)hipGetLastError();  // a failed elapsed-time query is not the caller's error
    return KH_OK;
}

// ---- device memory helpers -------------------------------------------------------------------
int kh_dev_malloc(void** p, uint64_t bytes, int device) {
    if (!p) return fail(KH_ERR_ARG, "null out pointer");
    KH_HIP(hipSetDevice(device));
    hipError_t e = hipMalloc(p, bytes ? bytes : 16);
    if (e != hipSuccess) return fail(KH_ERR_NOMEM, "hipMalloc(%llu): %s", (unsigned long long)bytes,
                                     hipGetErrorString(e));
    return KH_OK;
}
int kh_dev_free(void* p) {
    if (p) KH_HIP(hipFree(p));
    return KH_OK;
}
int kh_memcpy_htod(void* dst, const void* src, uint64_t bytes) {
    if (bytes) KH_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return KH_OK;
}
int kh_memcpy_dtoh(void* dst, const void* src, uint64_t bytes) {
    if (bytes) KH_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return KH_OK;
}

int kh_key_owner(const kh_table* t, const uint8_t* packed_key, int nranks) {
    if (!t || !packed_key) return fail(KH_ERR_ARG, "null argument");
    if (nranks < 1 || nranks > kh::MAX_RANKS) return fail(KH_ERR_ARG, "nranks %d outside [1,%d]", nranks, kh::MAX_RANKS);
    return (int)kh::owner_key(kh::key_from_packed(packed_key, t->kp), t->kp, (uint32_t)nranks);
}

int kh_word_count(int k) { return (k >= 1 && k <= KH_K_MAX) ? kh::make_params(k).W : KH_ERR_ARG; }

}  // extern "C"
