// kh_table.hpp — what the C ABI's translation units (kh_capi*.cpp) share: error reporting, the
// grow-only device buffer, struct kh_table and the small helpers over it. Not part of the ABI:
// everything in namespace khx has hidden visibility.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "../../include/kmer_hash_amd.h"
#include "kh_codec.hpp"
#include "kh_internal.hpp"
#include "kh_kernels.hpp"

namespace khx __attribute__((visibility("hidden"))) {

// Sets the thread's kh_last_error() text and returns `code`.
int fail(int code, const char* fmt, ...);

#define KH_HIP(call)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(KH_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),     \
                        __FILE__, __LINE__);                                                  \
    } while (0)

// A blocking host wait on the table's stream (a device -> host round trip); counted per table so
// that hosts can report the syncs of a sharded step (kh_host_syncs).
#define KH_SYNC(t)                                          \
    do {                                                    \
        ++(t)->host_syncs;                                  \
        KH_HIP(hipStreamSynchronize((t)->stream));          \
    } while (0)

// Grow-only device buffer (kh_capi.cpp; its bytes are counted for kh_device_bytes).
struct DevBuf {
    void* p = nullptr;
    uint64_t bytes = 0;
    int ensure(uint64_t want);
    void release();
    template <class T>
    T* as() const {
        return reinterpret_cast<T*>(p);
    }
};

}  // namespace khx

struct kh_table {
    using DevBuf = khx::DevBuf;
    // ---- table ------------------------------------------------------------------------------
    int device = 0;
    kh::KParams kp{};
    uint64_t cap = 0;       // slots
    uint64_t n_kmers = 0;   // k-mers the table was created (or last reserved) for
    double load = 0.5;      // load factor
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    DevBuf slots, ctr, stats;
    DevBuf hot;                               // remapped-region bitmap (KParams::hot), 2 levels of HOT_WORDS
    DevBuf rbounds;                           // balanced region bounds (KParams::rb), 2^17 + 1 words
    bool slots_stale = true;   // cleared lazily: a partitioned build of an empty table writes every slot
    uint64_t n_inserted = 0;                 // host-side count (what was submitted)
    uint64_t host_syncs = 0;                 // blocking stream waits of this table (KH_SYNC)

    // ---- insert / staging -------------------------------------------------------------------
    DevBuf starts;
    DevBuf splits, splits_w;                 // splitter k-mers (walk segments) / walk subset
    DevBuf mask, mask_off, scratch;          // per insert batch
    DevBuf stage;                            // host-API staging of records / keys
    DevBuf stage2, stage3;
    DevBuf pb_buf1, pb_buf2, pb_cnt, pb_ovf;  // partitioned build
    DevBuf headrec;                           // chain head records (region build -> walker)
    uint32_t hcap = 0;                        // head records per region (0 = no chains)
    bool last_insert_part = false;
    bool staging = false, stage_part = false, stage_fresh = false;  // kh_insert_words_stage_dev build
    uint64_t stage_total = 0, stage_n = 0;
    uint64_t starts_cap = 0;                 // start entries the starts buffer holds
    uint64_t splits_cap = 0, splits_w_cap = 0;
    bool split_ok = true;                    // every inserted k-mer was checked for splitters
    bool split_forced = false; // KH_SPLIT_BITS set: the walk uses every collected splitter

    // ---- single-GPU walk --------------------------------------------------------------------
    DevBuf seg_next, seg_key, seg_contig, seg_off, clen, stab, stab_id;  // splitter segments
    DevBuf seg_jump, seg_jsum, seg_anchor, seg_pend;
    DevBuf contig_len, contig_off, chunk_data, chunk_owner, chunk_seq, text, line_first;
    bool walk_bounded = false; // the last walk's text was sized before it ran (kh_assemble_dev)
    bool starts_explicit = false;            // kh_set_starts: walks may overlap (text not bounded)
    bool text_sync = false;                  // the next assemble sizes the text from the scanned total
    uint64_t chunk_cap = 0;
    uint64_t last_contigs = 0;               // n_starts seen by the last assemble
    bool assembled = false;

    // ---- position index (kh_capi_locate.cpp) ------------------------------------------------
    DevBuf loc;                // one uint64 per slot, allocated by the first kh_locate_reset / _build
    bool loc_valid = false;    // false again wherever `assembled` changes, the table is cleared or grown

    // ---- route / find / text scratch (sharded path) -----------------------------------------
    DevBuf route_hist, route_off, route_scratch, route_own;
    DevBuf find_own, find_ext;                // batched find: owners of routed keys / answers in key order
    DevBuf text_cnt, text_off, text_scratch;  // kh_text_keys_dev: windows per tile, their offsets, the scan's sums
    DevBuf route_spl;                        // splitter k-mers routed to each owner (MAX_RANKS words)
    uint64_t collected_n = 0;  // records passed to kh_route_starts_dev since the last clear
    bool words_split = true;   // every routed word since the last clear went through splitter collection

    // ---- migrating walk ---------------------------------------------------------------------
    DevBuf mw_tmp, mw_dst, mw_stage, mw_nrec, mw_off, mw_misc, mw_store;
    DevBuf mw_cnt, mw_list, mw_carry[2], mw_carry_dst[2];  // fixed-slot rounds
    int mw_cur = 0;                          // carry buffer written by the last round
    uint64_t mw_wg = 0;        // walkers of every rank (bound of a round's input / held-back messages)
    uint64_t mw_store_n = 0;   // text records in mw_store (valid when mw_store_known)
    uint64_t mw_store_bound = 0;  // upper bound of the store's records (its device count: mw_misc[2])
    bool mw_seg_off = false;      // kh_mwalk_redo: the next walk runs without splitter segments
    uint64_t mw_soft_next = 0;    // kh_mwalk_short: the next walk's soft step limit (0: none)
    uint64_t mw_soft = 0;         // this walk's
    uint64_t mw_store_min = 0;    // ... with a text store of at least this many records
    bool mw_store_known = true;
    uint32_t mw_P = 0, mw_rank = 0;
    bool mw_live = false, mw_stepped = false;
    bool mw_hot = true;        // the shard has remapped regions (the walk reads the bitmap)
    bool succ_pending = false; // k_rec_succ of the migrating walk still queued on the side stream
    uint64_t rw_n = 0, rw_total = 0;  // migrating walk: local walkers, bound on contig length

    // ---- splitter segments of the migrating walk (kh_mseg.hip) ------------------------------
    DevBuf ms_len, ms_hi, ms_lo, ms_has, ms_done, ms_jump, ms_acc, ms_stab, ms_stab_id, ms_qsrc, ms_misc;
    DevBuf ms_res[6], ms_pend;               // pointer jumping over the gathered predecessor tables
    bool ms_chunks = false;  // the record scan filled the origin's first chunks (line writer)
    bool ms_on = false;        // the current migrating walk uses splitter segments
    uint64_t ms_ns = 0, ms_nsp = 0, ms_cap2 = 0, ms_nq = 0;

    // ---- timing events, side stream ---------------------------------------------------------
    hipEvent_t ev_ins0 = nullptr, ev_ins1 = nullptr, ev_ins2 = nullptr;
    hipEvent_t ev_walk0 = nullptr, ev_walk1 = nullptr, ev_mat1 = nullptr;
    hipEvent_t ev_b0 = nullptr, ev_b1 = nullptr, ev_wk1 = nullptr;  // build / walk-kernel brackets
    bool build_timed = false;
    // side stream: start / splitter compaction overlapped with the partition passes
    hipStream_t side = nullptr;
    hipEvent_t ev_conv = nullptr, ev_side = nullptr;
    bool ins_timed = false, walk_timed = false, wk_timed = false;  // wk: ev_wk1 recorded by this walk
    // counters copied to pinned host memory on the side stream once the last device insert's start
    // compaction and hot-region mark are final (ev_hot / ev_ctr), so assemble reads them without
    // waiting for the build: ctr_early says the copy belongs to the current table state
    unsigned long long* hctr = nullptr;
    hipEvent_t ev_hot = nullptr, ev_ctr = nullptr;
    bool ctr_early = false;
};

namespace khx __attribute__((visibility("hidden"))) {

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
inline kh::TableView view(const kh_table* t) { return kh::TableView{t->slots.as<uint64_t>(), t->cap}; }

// kh_capi.cpp
int set_device(const kh_table* t);
int ensure_list(kh_table* t, DevBuf& buf, uint64_t& cap, uint64_t need);
int ensure_starts(kh_table* t, uint64_t need);
int read_ctr(kh_table* t, int idx, uint64_t* v);
int stats_status(const unsigned long long* st);  // first device-side error of a copy of the stats
int check_stats(kh_table* t);                    // the same, read from the device (one wait)
int clean_slots(kh_table* t);
int join_succ(kh_table* t);
// kh_capi_insert.cpp
bool use_part_build(const kh_table* t, uint64_t n);
int ensure_part(kh_table* t, uint64_t n, kh::PartBuffers& b);
int cas_hot_prepass(kh_table* t, const void* recs, const void* words, uint64_t n, uint64_t total = 0);
int mark_buffers(kh_table* t, uint64_t n, uint64_t base, uint64_t slack, uint64_t** start_mask,
                 uint64_t** split_mask);
int collect_marks(kh_table* t, const uint8_t* recs, uint64_t m, uint64_t* start_mask, uint64_t* split_mask,
                  hipStream_t stream);
int read_counters(kh_table* t, unsigned long long* cv, bool consume);
// kh_capi_dist.cpp
int ensure_route(kh_table* t, uint64_t n, int nranks);
bool mseg_enabled(const kh_table* t);
kh::KParams mseg_params(const kh_table* t);
kh::MSegState mseg_state(kh_table* t);
int text_for(kh_table* t, uint64_t nc, uint64_t word_recs);
uint64_t* origin_chunks(kh_table* t, uint64_t nc);
uint32_t origin_lines(kh_table* t, uint64_t nc, const uint32_t* clen, int slen_add, const uint32_t* slen,
                      bool chunks);

}  // namespace khx
