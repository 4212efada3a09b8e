// kh_capi_strand.cpp — seeds on both strands of the C ABI (kh_seed_strand_*; kernels in kh_strand.hip):
// per read the longest exact run on either strand of the contigs, from the two position arrays
// kh_locate_text_dev and kh_locate_text_rc_dev answer. The calls mirror kh_seed_runs_dev,
// kh_seed_text_dev and kh_seed_text (kh_capi_seed.cpp) rule for rule; nothing is kept in the table.
#include "kh_table.hpp"

using namespace khx;

static_assert(KH_SEED_STRAND_WORDS == kh::SEED_STRAND_WORDS, "the header's words per strand seed");

namespace {

inline bool aligned8(const void* p) { return ((uintptr_t)p & 7u) == 0; }

// What kh_seed_strand_runs_dev and kh_seed_strand_text_dev check of the reads and the answer.
int reads_ok(const void* dev_read_off, uint64_t n_reads, const void* dev_seeds_out) {
    if (!dev_read_off || !dev_seeds_out) return fail(KH_ERR_ARG, "null buffer");
    if (!aligned8(dev_read_off) || !aligned8(dev_seeds_out))
        return fail(KH_ERR_ARG, "read offsets and seeds must be 8-byte aligned");
    if (n_reads >> 32) return fail(KH_ERR_ARG, "more than 2^32 - 1 reads in one call");
    return KH_OK;
}

// The state rules of kh_locate_text_dev.
int strand_open(kh_table* t) {
    if (!t) return fail(KH_ERR_ARG, "null table");
    if (t->staging) return fail(KH_ERR_STATE, "a staged insert is open (kh_insert_words_finish first)");
    if (!t->loc_valid)
        return fail(KH_ERR_STATE, "no position index (kh_locate_build / kh_locate_reset since the last change of the "
                                  "table, its starts or its contigs)");
    return KH_OK;
}

}  // namespace

extern "C" {

int kh_seed_strand_runs_dev(kh_table* t, const void* dev_pos_fwd, const void* dev_pos_rc, uint64_t len,
                            const void* dev_read_off, uint64_t n_reads, void* dev_seeds_out) {
    if (!t) return fail(KH_ERR_ARG, "null table");
    if (n_reads == 0) return KH_OK;
    if (int rc = reads_ok(dev_read_off, n_reads, dev_seeds_out)) return rc;
    if (len && (!dev_pos_fwd || !dev_pos_rc)) return fail(KH_ERR_ARG, "null positions");
    if (!aligned8(dev_pos_fwd) || !aligned8(dev_pos_rc)) return fail(KH_ERR_ARG, "positions must be 8-byte aligned");
    if (int rc = set_device(t)) return rc;
    KH_HIP(kh::launch_seed_runs_strand((const uint64_t*)dev_pos_fwd, (const uint64_t*)dev_pos_rc, len,
                                       (const uint64_t*)dev_read_off, n_reads, t->kp.K, (uint64_t*)dev_seeds_out,
                                       t->stream));
    return KH_OK;
}

int kh_seed_strand_text_dev(kh_table* t, const void* dev_text, uint64_t len, const void* dev_read_off,
                            uint64_t n_reads, void* dev_pos_scratch, void* dev_seeds_out) {
    if (int rc = strand_open(t)) return rc;
    if (n_reads == 0) return KH_OK;
    if (int rc = reads_ok(dev_read_off, n_reads, dev_seeds_out)) return rc;
    if (len && (!dev_text || !dev_pos_scratch)) return fail(KH_ERR_ARG, "null text or position scratch");
    if (!aligned8(dev_pos_scratch)) return fail(KH_ERR_ARG, "the position scratch must be 8-byte aligned");
    uint64_t* const fwd = (uint64_t*)dev_pos_scratch;
    uint64_t* const rev = len ? fwd + len : fwd;  // v in scratch[0, len), w in scratch[len, 2 * len)
    if (len) {
        if (int rc = kh_locate_text_dev(t, dev_text, len, fwd, nullptr)) return rc;
        if (int rc = kh_locate_text_rc_dev(t, dev_text, len, rev, nullptr)) return rc;
    }
    return kh_seed_strand_runs_dev(t, fwd, rev, len, dev_read_off, n_reads, dev_seeds_out);
}

int kh_seed_strand_text(kh_table* t, const char* host_text, uint64_t len, const uint64_t* host_read_off,
                        uint64_t n_reads, uint64_t* host_seeds_out) {
    if (int rc = strand_open(t)) return rc;
    if (n_reads == 0) return KH_OK;
    if (!host_read_off || !host_seeds_out) return fail(KH_ERR_ARG, "null buffer");
    if (len && !host_text) return fail(KH_ERR_ARG, "null text");
    if (n_reads >> 32) return fail(KH_ERR_ARG, "more than 2^32 - 1 reads in one call");
    if (int rc = set_device(t)) return rc;
    const uint64_t ob = (n_reads + 1) * 8, sb = n_reads * 8 * KH_SEED_STRAND_WORDS;
    int rc;
    if ((rc = t->stage.ensure(len)) || (rc = t->stage2.ensure(16 * len)) || (rc = t->stage3.ensure(ob + sb))) return rc;
    uint8_t* const d_off = t->stage3.as<uint8_t>();
    if (len) KH_HIP(hipMemcpyAsync(t->stage.p, host_text, len, hipMemcpyHostToDevice, t->stream));
    KH_HIP(hipMemcpyAsync(d_off, host_read_off, ob, hipMemcpyHostToDevice, t->stream));
    if ((rc = kh_seed_strand_text_dev(t, t->stage.p, len, d_off, n_reads, t->stage2.p, d_off + ob))) return rc;
    KH_HIP(hipMemcpyAsync(host_seeds_out, d_off + ob, sb, hipMemcpyDeviceToHost, t->stream));
    KH_SYNC(t);
    return KH_OK;
}

}  // extern "C"
