// kh_capi_insert.cpp — the insert pipeline of the C ABI. Every insert entry point (kh_insert and its
// chunked upload, kh_insert_dev, kh_insert_words_dev, the staged kh_insert_words_stage_dev ..
// kh_insert_words_finish) runs the same steps, each written once here: check_room, insert_open,
// mark_buffers, the build, collect_marks, insert_close. What the entry points do differently is
// said in a comment at the step.
#include <cstdlib>
#include <vector>

#include "kh_table.hpp"

using namespace khx;

// Insert strategy: KH_INSERT=cas (global CAS per key), part (partitioned LDS build), auto
// (default: partitioned when the batch is large and the region slices fit LDS).
bool khx::use_part_build(const kh_table* t, uint64_t n) {
    const char* m = getenv("KH_INSERT");
    const bool usable = kh::part_usable(t->kp, t->cap, n);
    if (m && !strcmp(m, "cas")) return false;
    if (m && !strcmp(m, "part"))
        return kh::region_slots_fit(t->kp, t->cap) && n > 0;
    return usable;
}

int khx::ensure_part(kh_table* t, uint64_t n, kh::PartBuffers& b) {
    const uint64_t W = (uint64_t)t->kp.W;
    int rc;
    if ((rc = t->pb_buf1.ensure(kh::part_buf1_words(t->kp, n) * 8)) || (rc = t->pb_buf2.ensure(kh::part_buf2_words(t->kp, n) * 8)) ||
        (rc = t->pb_cnt.ensure(kh::part_count_words() * 8)) ||
        (rc = t->pb_ovf.ensure(kh::part_overflow_cap(n) * W * 8)))
        return rc;
    b.buf1 = t->pb_buf1.as<uint64_t>();
    b.buf2 = t->pb_buf2.as<uint64_t>();
    b.wcnt = t->pb_cnt.as<uint32_t>();
    b.rcnt = b.wcnt + kh::PART_W1_COUNTERS;
    b.hot_list = b.rcnt + kh::HOT_WORDS * 32;
    b.overflow = t->pb_ovf.as<uint64_t>();
    b.hot = t->hot.as<uint32_t>();
    b.rbt = t->rbounds.as<uint64_t>();
    // chain head records: sized by the table (regions x records per region), kept across builds
    const uint32_t hcap = kh::part_head_cap(t->kp, t->cap);
    if (hcap) {
        // + the per-region record counts the build writes after the records (k_rec_succ reads them)
        const uint64_t recb = (uint64_t)hcap * (1ull << t->kp.rbits) * 16, cntb = (1ull << t->kp.rbits) * 4;
        const void* before = t->headrec.p;
        if ((rc = t->headrec.ensure(recb + cntb))) return rc;
        if (t->headrec.p != before) KH_HIP(hipMemsetAsync((char*)t->headrec.p + recb, 0, cntb, t->stream));
    }
    t->hcap = hcap;
    b.headrec = hcap ? t->headrec.as<uint64_t>() : nullptr;
    b.hcap = hcap;
    return KH_OK;
}

// CAS-path insert into an empty table: remap the minimizer regions the batch would overfill
// (kh_build.hip launch_hot_prepass); later batches place keys with the same bitmap.
int khx::cas_hot_prepass(kh_table* t, const void* recs, const void* words, uint64_t n, uint64_t total) {
    if (t->n_inserted != 0) return KH_OK;
    if (int rc = t->pb_cnt.ensure(kh::part_count_words() * 8)) return rc;
    uint32_t* rcnt = t->pb_cnt.as<uint32_t>() + kh::PART_W1_COUNTERS;
    KH_HIP(hipMemsetAsync(t->hot.p, 0, 2 * kh::HOT_WORDS * 4, t->stream));
    KH_HIP(kh::launch_hot_prepass(t->kp, (const uint8_t*)recs, (const uint64_t*)words, n, t->cap, rcnt,
                                  t->hot.as<uint32_t>(), rcnt + kh::HOT_WORDS * 32, t->ctr.as<unsigned long long>(),
                                  t->stream, total));
    return KH_OK;
}

// Sizes the buffers that mark and collect the start (and splitter) k-mers of a batch of n records
// after `base` earlier ones, and hands back the start mask. The record inserts pass split_mask: it
// gets the splitter mask (null with splitters off), the splitter list is sized too and the scratch
// covers a scan over n. The routes and kh_collect_starts_dev pass null and scan mask words only.
int khx::mark_buffers(kh_table* t, uint64_t n, uint64_t base, uint64_t slack, uint64_t** start_mask,
                      uint64_t** split_mask) {
    const uint64_t nw = (n + 63) / 64;
    const bool split = split_mask && t->kp.split_bits > 0;
    int rc;
    if ((rc = t->mask.ensure(nw * 8 * (split ? 2 : 1) + slack))) return rc;
    if ((rc = t->mask_off.ensure(nw * 8 + slack))) return rc;
    if ((rc = t->scratch.ensure(kh::scan_scratch_words(split_mask && n > nw ? n : nw) * 8 + 64))) return rc;
    if ((rc = ensure_starts(t, base + n))) return rc;
    if (split && (rc = ensure_list(t, t->splits, t->splits_cap, base + n))) return rc;
    *start_mask = t->mask.as<uint64_t>();
    if (split_mask) *split_mask = split ? *start_mask + nw : nullptr;
    return KH_OK;
}

// Compacts the marked start k-mers of m records into the start list and, with a splitter mask, the
// marked splitters into the splitter list.
int khx::collect_marks(kh_table* t, const uint8_t* recs, uint64_t m, uint64_t* start_mask, uint64_t* split_mask,
                       hipStream_t stream) {
    unsigned long long* ctr = t->ctr.as<unsigned long long>();
    KH_HIP(kh::launch_collect_starts(t->kp, recs, m, start_mask, t->mask_off.as<uint64_t>(),
                                     t->scratch.as<uint64_t>(), t->starts.as<uint64_t>(), ctr, stream));
    if (split_mask)
        KH_HIP(kh::launch_collect_starts(t->kp, recs, m, split_mask, t->mask_off.as<uint64_t>(),
                                         t->scratch.as<uint64_t>(), t->splits.as<uint64_t>(), ctr, stream,
                                         kh::CT_N_SPLIT));
    return KH_OK;
}

// The counters on the host: from the pinned copy made beside the last kh_insert_dev when it is
// current (wait for that copy, not the build), else read on the stream. One host wait either way.
// kh_assemble_dev consumes the early copy, kh_counters leaves it armed.
int khx::read_counters(kh_table* t, unsigned long long* cv, bool consume) {
    const size_t bytes = kh::CT_NUM * sizeof *cv;
    if (t->ctr_early) {
        ++t->host_syncs;
        KH_HIP(hipEventSynchronize(t->ev_ctr));
        memcpy(cv, t->hctr, bytes);
        if (consume) t->ctr_early = false;
    } else {
        KH_HIP(hipMemcpyAsync(cv, t->ctr.p, bytes, hipMemcpyDeviceToHost, t->stream));
        KH_SYNC(t);
    }
    return KH_OK;
}

namespace {

// whose: "table" (records) or "shard" (routed words); verb: "inserting" or "staging".
int check_room(const kh_table* t, uint64_t n, const char* verb, const char* whose) {
    if (t->n_inserted + n > t->n_kmers)
        return fail(KH_ERR_FULL, "%s %llu k-mers into a %s created for %llu (%llu in)", verb,
                    (unsigned long long)n, whose, (unsigned long long)t->n_kmers,
                    (unsigned long long)t->n_inserted);
    return KH_OK;
}

struct InsertPlan {
    bool part = false, fresh = false;
    kh::PartBuffers pb{};
};

// Opens a build of `total` k-mers: partitioned or CAS, the partitioned build's buffers, the slots
// emptied unless the build rewrites them all, and the start of the insert bracket.
// slots_stale stays the caller's: the one-call inserts clear it right after this, the staged insert
// only at kh_insert_words_finish (a kh_find_dev between stage and finish still clears the slots).
int insert_open(kh_table* t, uint64_t total, InsertPlan& p) {
    p.part = use_part_build(t, total);
    if (p.part)
        if (int rc = ensure_part(t, total, p.pb)) return rc;
    // a partitioned build into a fresh table rewrites every slot: no clear needed
    p.fresh = p.part && t->n_inserted == 0;  // empty (stale or clean): the build writes every slot
    if (!p.fresh)
        if (int rc = clean_slots(t)) return rc;
    KH_HIP(hipEventRecord(t->ev_ins0, t->stream));
    return KH_OK;
}

// kh_insert_dev's partitioned path only: the table's stream joins the side stream's start / splitter
// compaction, and the counters go to pinned memory beside the build (read_counters).
int side_counters(kh_table* t) {
    KH_HIP(hipEventRecord(t->ev_side, t->side));
    KH_HIP(hipStreamWaitEvent(t->stream, t->ev_side, 0));
    // start / splitter counts (final after the compaction above) and the remapped-region count
    // (final after the hot mark, ev_hot) to pinned memory beside the build
    KH_HIP(hipStreamWaitEvent(t->side, t->ev_hot, 0));
    KH_HIP(hipMemcpyAsync(t->hctr, t->ctr.p, kh::CT_NUM * 8, hipMemcpyDeviceToHost, t->side));
    KH_HIP(hipEventRecord(t->ev_ctr, t->side));
    t->ctr_early = true;
    return KH_OK;
}

// Closes the insert bracket after the build of n k-mers is queued. side: the marks were compacted
// on the side stream (kh_insert_dev's partitioned path; every other path runs on the table's stream
// and leaves ctr_early false).
int insert_close(kh_table* t, uint64_t n, bool part, bool side = false) {
    t->build_timed = t->last_insert_part = part;
    KH_HIP(hipEventRecord(t->ev_ins1, t->stream));
    t->ctr_early = false;  // kh_insert_dev's only reset; the other entry points did it on entry
    if (side)
        if (int rc = side_counters(t)) return rc;
    KH_HIP(hipEventRecord(t->ev_ins2, t->stream));
    t->ins_timed = true;
    t->n_inserted += n;
    t->assembled = t->loc_valid = false;
    return KH_OK;
}

// kh_insert of a large batch into an empty table (the reference's boundary: records in host
// memory, kmer_hash.cpp:129): the records go up in chunks on the side stream while the table's
// stream converts and partitions each chunk that has landed (passes 1-2 into the region windows);
// one build after the last chunk. The upload is the bound (~55 GB/s over PCIe for 3 GB at C3);
// all device work but the last chunk's passes, the build and the walk hides behind it.
int insert_chunked_upload(kh_table* t, const uint8_t* host_recs, uint64_t n) {
    const uint64_t R = (uint64_t)t->kp.R, W = (uint64_t)t->kp.W;
    // chunks of a multiple of 8192 records (the convert pass's tiles; start-mask words stay whole)
    uint64_t nch = 16;
    uint64_t chunk = ((n + nch - 1) / nch + 8191) & ~8191ull;
    nch = (n + chunk - 1) / chunk;
    int rc;
    if ((rc = t->stage.ensure(n * R + 16))) return rc;
    if ((rc = t->stage2.ensure(chunk * W * 8 + 16))) return rc;
    uint64_t *start_mask, *split_mask;
    if ((rc = mark_buffers(t, n, 0, 0, &start_mask, &split_mask))) return rc;
    kh::PartBuffers pb{};
    if ((rc = ensure_part(t, n, pb))) return rc;
    struct Events {  // one per chunk: its upload landed
        std::vector<hipEvent_t> e;
        ~Events() {
            for (auto x : e)
                if (x) (void)hipEventDestroy(x);
        }
    } ev;
    ev.e.assign(nch, nullptr);
    for (auto& e : ev.e) KH_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    uint8_t* d = t->stage.as<uint8_t>();
    unsigned long long* ctr = t->ctr.as<unsigned long long>();
    unsigned long long* stats = t->stats.as<unsigned long long>();
    auto upload = [&](uint64_t c) -> hipError_t {
        const uint64_t b = c * chunk, m = (b + chunk < n ? chunk : n - b);
        hipError_t e = hipMemcpyAsync(d + b * R, host_recs + b * R, m * R, hipMemcpyHostToDevice, t->side);
        return e != hipSuccess ? e : hipEventRecord(ev.e[c], t->side);
    };
    // the side stream starts after everything already queued on the table's stream; chunk c + 1's
    // upload is queued after chunk c's passes, so a pageable (host-synchronous) copy overlaps too
    KH_HIP(hipEventRecord(t->ev_side, t->stream));
    KH_HIP(hipStreamWaitEvent(t->side, t->ev_side, 0));
    KH_HIP(upload(0));
    // always partitioned into an empty table, so none of insert_open's decisions (and, as before,
    // no join_succ): only the bracket's start, after the first upload is queued
    KH_HIP(hipEventRecord(t->ev_ins0, t->stream));
    t->slots_stale = false;  // the build of an empty table writes every slot
    for (uint64_t c = 0; c < nch; ++c) {
        const uint64_t b = c * chunk, m = (b + chunk < n ? chunk : n - b);
        KH_HIP(hipStreamWaitEvent(t->stream, ev.e[c], 0));
        KH_HIP(kh::launch_part_stage_recs(t->kp, d + b * R, m, n, c == 0, pb, t->stage2.as<uint64_t>(),
                                          start_mask + b / 64, split_mask ? split_mask + b / 64 : nullptr, ctr, stats,
                                          t->stream, c == 0, t->cap));
        if ((rc = collect_marks(t, d + b * R, m, start_mask + b / 64, split_mask ? split_mask + b / 64 : nullptr,
                                t->stream)))
            return rc;
        if (c + 1 < nch) KH_HIP(upload(c + 1));
    }
    KH_HIP(hipEventRecord(t->ev_b0, t->stream));
    KH_HIP(kh::launch_part_finish(t->kp, n, view(t), true, pb, ctr, stats, t->stream));
    KH_HIP(hipEventRecord(t->ev_b1, t->stream));
    if ((rc = insert_close(t, n, true))) return rc;
    return check_stats(t);  // one wait: the stats read is ordered after the queued work
}

// Routed words: collect the splitter k-mers this shard owns (they head migrating-walk segments).
// *coll: the partitioned insert that follows collects them itself (k_win1, built with mseg_params
// instead of the table's): only size the list.
int collect_word_splits(kh_table* t, const void* words, uint64_t m, bool part, bool* coll) {
    *coll = part && mseg_enabled(t) && t->words_split;
    if (!mseg_enabled(t) || !t->words_split) return KH_OK;
    const kh::KParams mp = mseg_params(t);
    const uint64_t need = (t->n_kmers >> (mp.split_bits > 3 ? mp.split_bits - 3 : 0)) + 4096;
    if (int rc = ensure_list(t, t->splits, t->splits_cap, need)) return rc;
    if (*coll) return KH_OK;
    KH_HIP(kh::launch_split_collect(mp, (const uint64_t*)words, m, t->splits.as<uint64_t>(), t->splits_cap,
                                    t->ctr.as<unsigned long long>(), t->stream));
    return KH_OK;
}

}  // namespace

extern "C" {

int kh_insert_dev(kh_table* t, const void* dev_recs, uint64_t n) {
    if (!t) return fail(KH_ERR_ARG, "null table");
    if (n == 0) return KH_OK;  // (ctr_early stays as it was: see insert_close)
    if (!dev_recs) return fail(KH_ERR_ARG, "null records");
    if (!aligned16(dev_recs)) return fail(KH_ERR_ARG, "device records must be 16-byte aligned");
    if (int rc = check_room(t, n, "inserting", "table")) return rc;
    if (int rc = set_device(t)) return rc;
    if (int rc = join_succ(t)) return rc;
    int rc;
    uint64_t *start_mask, *split_mask;  // split_ok is left alone: these records' splitters are marked
    if ((rc = mark_buffers(t, n, t->n_inserted, 0, &start_mask, &split_mask))) return rc;
    InsertPlan p;
    if ((rc = insert_open(t, n, p))) return rc;
    t->slots_stale = false;
    // partitioned build: the start / splitter bits exist once the record pass has run, so their
    // compaction runs on the side stream, overlapped with the partition passes and the build
    const bool overlap = p.part;
    if (p.part) {
        KH_HIP(kh::launch_part_insert(t->kp, (const uint8_t*)dev_recs, nullptr, n, view(t),
                                      p.fresh, p.pb, start_mask, split_mask,
                                      t->ctr.as<unsigned long long>(),
                                      t->stats.as<unsigned long long>(), t->stream,
                                      overlap ? t->ev_conv : nullptr, nullptr, 0, t->ev_b0,
                                      overlap ? t->ev_hot : nullptr));
        KH_HIP(hipEventRecord(t->ev_b1, t->stream));
    } else {
        if ((rc = cas_hot_prepass(t, dev_recs, nullptr, n))) return rc;
        KH_HIP(kh::launch_insert(t->kp, (const uint8_t*)dev_recs, n, view(t), start_mask,
                                 split_mask, t->stats.as<unsigned long long>(), t->stream));
    }
    if (overlap) KH_HIP(hipStreamWaitEvent(t->side, t->ev_conv, 0));
    if ((rc = collect_marks(t, (const uint8_t*)dev_recs, n, start_mask, split_mask, overlap ? t->side : t->stream)))
        return rc;
    return insert_close(t, n, p.part, overlap);
}

int kh_insert(kh_table* t, const uint8_t* host_recs, uint64_t n) {
    if (!t) return fail(KH_ERR_ARG, "null table");
    t->ctr_early = false;  // counters may change: assemble reads them on the stream
    if (n == 0) return KH_OK;
    if (!host_recs) return fail(KH_ERR_ARG, "null records");
    if (int rc = set_device(t)) return rc;
    if (int rc = check_room(t, n, "inserting", "table")) return rc;
    if (t->n_inserted == 0 && n >= (1ull << 24) && use_part_build(t, n))
        return insert_chunked_upload(t, host_recs, n);
    const uint64_t bytes = n * (uint64_t)t->kp.R;
    if (int rc = t->stage.ensure(bytes)) return rc;
    KH_HIP(hipMemcpyAsync(t->stage.p, host_recs, bytes, hipMemcpyHostToDevice, t->stream));
    if (int rc = kh_insert_dev(t, t->stage.p, n)) return rc;
    return check_stats(t);  // one wait: the stats read is ordered after the queued work
}

int kh_insert_words_dev(kh_table* t, const void* words, uint64_t m) {
    if (!t) return fail(KH_ERR_ARG, "null table");
    t->ctr_early = false;  // counters may change: assemble reads them on the stream
    if (m == 0) return KH_OK;
    if (!words) return fail(KH_ERR_ARG, "null words");
    if (int rc = check_room(t, m, "inserting", "shard")) return rc;
    if (int rc = set_device(t)) return rc;
    if (int rc = join_succ(t)) return rc;
    t->split_ok = false;  // routed words carry no splitter marks: walks on this table use none
    bool coll;
    if (int rc = collect_word_splits(t, words, m, use_part_build(t, m), &coll)) return rc;
    InsertPlan p;
    if (int rc = insert_open(t, m, p)) return rc;
    t->slots_stale = false;
    if (p.part) {
        KH_HIP(kh::launch_part_insert(coll ? mseg_params(t) : t->kp, nullptr, (const uint64_t*)words, m, view(t),
                                      p.fresh, p.pb, nullptr, nullptr, t->ctr.as<unsigned long long>(),
                                      t->stats.as<unsigned long long>(), t->stream, nullptr,
                                      coll ? t->splits.as<uint64_t>() : nullptr, coll ? t->splits_cap : 0, t->ev_b0));
        KH_HIP(hipEventRecord(t->ev_b1, t->stream));
    } else {
        if (int rc = cas_hot_prepass(t, nullptr, words, m)) return rc;
        KH_HIP(kh::launch_insert_words(t->kp, (const uint64_t*)words, m, view(t),
                                       t->stats.as<unsigned long long>(), t->stream));
    }
    return insert_close(t, m, p.part);
}

int kh_insert_words_stage_dev(kh_table* t, const void* words, uint64_t m, uint64_t total_hint) {
    if (!t) return fail(KH_ERR_ARG, "null table");
    t->ctr_early = false;  // counters may change: assemble reads them on the stream
    if (m && !words) return fail(KH_ERR_ARG, "null words");
    if (int rc = set_device(t)) return rc;
    if (int rc = join_succ(t)) return rc;
    InsertPlan p;
    if (!t->staging) {
        if (total_hint < m) total_hint = m;
        if (int rc = check_room(t, total_hint, "staging", "shard")) return rc;
        t->split_ok = false;  // routed words carry no splitter marks
        t->stage_total = total_hint;
        t->stage_n = 0;
        if (int rc = insert_open(t, total_hint, p)) return rc;
        t->stage_part = p.part;
        t->stage_fresh = p.fresh;
        t->staging = true;
        t->loc_valid = false;
        t->last_insert_part = t->stage_part;  // already here: kh_get_stats between stage and finish
        if (t->stage_part)
            KH_HIP(kh::launch_part_stage(t->kp, nullptr, 0, total_hint, true, p.pb, t->ctr.as<unsigned long long>(),
                                         t->stats.as<unsigned long long>(), t->stream));
    } else if (t->stage_part) {
        if (int rc = ensure_part(t, t->stage_total, p.pb)) return rc;
    }
    if (t->stage_n + m > t->stage_total)
        return fail(KH_ERR_FULL, "staged %llu + %llu words exceed the build's %llu",
                    (unsigned long long)t->stage_n, (unsigned long long)m, (unsigned long long)t->stage_total);
    if (m == 0) return KH_OK;
    bool coll;
    if (int rc = collect_word_splits(t, words, m, t->stage_part, &coll)) return rc;
    if (t->stage_part) {
        KH_HIP(kh::launch_part_stage(coll ? mseg_params(t) : t->kp, (const uint64_t*)words, m, t->stage_total, false, p.pb,
                                     t->ctr.as<unsigned long long>(), t->stats.as<unsigned long long>(),
                                     t->stream, coll ? t->splits.as<uint64_t>() : nullptr,
                                     coll ? t->splits_cap : 0, t->stage_fresh && t->stage_n == 0, t->cap));
    } else {
        if (t->stage_n == 0)  // the first staged batch stands for the whole build (stage_total)
            if (int rc = cas_hot_prepass(t, nullptr, words, m, t->stage_total)) return rc;
        KH_HIP(kh::launch_insert_words(t->kp, (const uint64_t*)words, m, view(t),
                                       t->stats.as<unsigned long long>(), t->stream));
    }
    t->stage_n += m;
    return KH_OK;
}

int kh_insert_words_finish(kh_table* t) {
    if (!t) return fail(KH_ERR_ARG, "null table");
    t->ctr_early = false;  // counters may change: assemble reads them on the stream
    if (!t->staging) return fail(KH_ERR_STATE, "no staged insert open");
    if (int rc = set_device(t)) return rc;
    if (t->stage_part) {
        kh::PartBuffers b{};
        if (int rc = ensure_part(t, t->stage_total, b)) return rc;
        KH_HIP(hipEventRecord(t->ev_b0, t->stream));
        KH_HIP(kh::launch_part_finish(t->kp, t->stage_total, view(t), t->stage_fresh, b, t->ctr.as<unsigned long long>(),
                                      t->stats.as<unsigned long long>(), t->stream));
        KH_HIP(hipEventRecord(t->ev_b1, t->stream));
        t->slots_stale = false;
    }
    if (int rc = insert_close(t, t->stage_n, t->stage_part)) return rc;
    t->staging = false;
    t->stage_n = 0;
    return KH_OK;
}

int kh_collect_starts_dev(kh_table* t, const void* dev_recs, uint64_t n) {
    if (!t) return fail(KH_ERR_ARG, "null table");
    t->ctr_early = false;  // counters may change: assemble reads them on the stream
    if (n == 0) return KH_OK;
    if (!dev_recs) return fail(KH_ERR_ARG, "null records");
    if (int rc = set_device(t)) return rc;
    int rc;
    uint64_t have = 0, *start_mask;
    if ((rc = read_ctr(t, kh::CT_N_STARTS, &have))) return rc;
    if ((rc = mark_buffers(t, n, have, 0, &start_mask, nullptr))) return rc;
    KH_HIP(kh::launch_start_mask(t->kp, (const uint8_t*)dev_recs, n, start_mask, t->stream));
    if ((rc = collect_marks(t, (const uint8_t*)dev_recs, n, start_mask, nullptr, t->stream))) return rc;
    t->assembled = t->loc_valid = false;
    return KH_OK;
}

int kh_counters_dev(kh_table* t, void* dev_out) {
    if (!t || !dev_out) return fail(KH_ERR_ARG, "null argument");
    if (int rc = set_device(t)) return rc;
    uint64_t* o = (uint64_t*)dev_out;
    const unsigned long long* c = t->ctr.as<unsigned long long>();
    KH_HIP(hipMemcpyAsync(o, c + kh::CT_N_STARTS, 8, hipMemcpyDeviceToDevice, t->stream));
    KH_HIP(hipMemcpyAsync(o + 1, c + kh::CT_N_SPLIT, 8, hipMemcpyDeviceToDevice, t->stream));
    return KH_OK;
}

int kh_counters(kh_table* t, uint64_t* out) {
    if (!t || !out) return fail(KH_ERR_ARG, "null argument");
    if (int rc = set_device(t)) return rc;
    unsigned long long cv[kh::CT_NUM];
    if (int rc = read_counters(t, cv, false)) return rc;
    out[0] = cv[kh::CT_N_STARTS];
    out[1] = cv[kh::CT_N_SPLIT];
    return KH_OK;
}

}  // extern "C"
