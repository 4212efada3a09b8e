// kh_capi_locate.cpp — the position index of the C ABI (kh_locate_*; kernels in kh_locate.hip): one
// uint64 per table slot beside the table, allocated by the first reset / build and kept until
// kh_locate_drop / kh_destroy. It is valid from a reset until anything changes the table's k-mers,
// its start list or its contig text (loc_valid, kh_table.hpp).
#include "kh_table.hpp"

using namespace khx;

static_assert(KH_LOC_NONE == kh::LOC_NONE, "the header's no-position value");

namespace {

inline bool aligned8(const void* p) { return ((uintptr_t)p & 7u) == 0; }

// What every call checks first: the table, no staged insert left open and, for the calls that read
// or add to the index, a valid index.
int locate_open(kh_table* t, bool need_index) {
    if (!t) return fail(KH_ERR_ARG, "null table");
    if (t->staging) return fail(KH_ERR_STATE, "a staged insert is open (kh_insert_words_finish first)");
    if (need_index && !t->loc_valid)
        return fail(KH_ERR_STATE, "no position index (kh_locate_build / kh_locate_reset since the last change of the "
                                  "table, its starts or its contigs)");
    return KH_OK;
}

uint64_t* loc_of(kh_table* t) { return t->loc.as<uint64_t>(); }

}  // namespace

extern "C" {

int kh_locate_reset(kh_table* t) {
    if (int rc = locate_open(t, false)) return rc;
    if (int rc = set_device(t)) return rc;
    if (int rc = t->loc.ensure(t->cap * 8)) return rc;
    KH_HIP(hipMemsetAsync(t->loc.p, 0xff, t->cap * 8, t->stream));
    t->loc_valid = true;
    return KH_OK;
}

int kh_locate_drop(kh_table* t) {
    if (!t) return fail(KH_ERR_ARG, "null table");
    if (int rc = set_device(t)) return rc;
    if (t->loc.p) KH_SYNC(t);  // queued queries may still read it
    t->loc.release();
    t->loc_valid = false;
    return KH_OK;
}

int kh_locate_build(kh_table* t) {
    if (int rc = locate_open(t, false)) return rc;
    if (!t->assembled) return fail(KH_ERR_STATE, "no assemble since the last insert/clear");
    const char* text = nullptr;
    uint64_t bytes = 0;
    if (int rc = kh_contigs_text_dev(t, &text, &bytes)) return rc;  // waits for the walk: the text's size
    if (int rc = kh_locate_reset(t)) return rc;
    if (int rc = clean_slots(t)) return rc;
    KH_HIP(kh::launch_loc_build(t->kp, (const uint8_t*)text, bytes, view(t), loc_of(t), 0, t->stream));
    return KH_OK;
}

int kh_locate_set_dev(kh_table* t, const void* dev_keys, uint64_t m, const void* dev_values, void* dev_missing_out) {
    if (int rc = locate_open(t, true)) return rc;
    if (m == 0) return KH_OK;
    if (!dev_keys || !dev_values) return fail(KH_ERR_ARG, "null buffer");
    if (!aligned8(dev_values) || !aligned8(dev_missing_out))
        return fail(KH_ERR_ARG, "values and the missing count must be 8-byte aligned");
    if (int rc = set_device(t)) return rc;
    if (int rc = clean_slots(t)) return rc;
    KH_HIP(kh::launch_loc_set(t->kp, (const uint8_t*)dev_keys, m, (const uint64_t*)dev_values, view(t), loc_of(t),
                              (unsigned long long*)dev_missing_out, t->stream));
    return KH_OK;
}

int kh_locate_dev(kh_table* t, const void* dev_keys, uint64_t m, void* dev_pos_out) {
    if (int rc = locate_open(t, true)) return rc;
    if (m == 0) return KH_OK;
    if (!dev_keys || !dev_pos_out) return fail(KH_ERR_ARG, "null buffer");
    if (!aligned8(dev_pos_out)) return fail(KH_ERR_ARG, "positions must be 8-byte aligned");
    if (int rc = set_device(t)) return rc;
    if (int rc = clean_slots(t)) return rc;
    KH_HIP(kh::launch_loc_get(t->kp, (const uint8_t*)dev_keys, m, view(t), loc_of(t), (uint64_t*)dev_pos_out,
                              t->stream));
    return KH_OK;
}

int kh_locate(kh_table* t, const uint8_t* host_keys, uint64_t m, uint64_t* host_pos_out) {
    if (int rc = locate_open(t, true)) return rc;
    if (m == 0) return KH_OK;
    if (!host_keys || !host_pos_out) return fail(KH_ERR_ARG, "null buffer");
    if (int rc = set_device(t)) return rc;
    const uint64_t kb = m * (uint64_t)t->kp.P;
    int rc;
    if ((rc = t->stage.ensure(kb)) || (rc = t->stage2.ensure(m * 8))) return rc;
    KH_HIP(hipMemcpyAsync(t->stage.p, host_keys, kb, hipMemcpyHostToDevice, t->stream));
    if ((rc = kh_locate_dev(t, t->stage.p, m, t->stage2.p))) return rc;
    KH_HIP(hipMemcpyAsync(host_pos_out, t->stage2.p, m * 8, hipMemcpyDeviceToHost, t->stream));
    KH_SYNC(t);
    return KH_OK;
}

int kh_locate_text_dev(kh_table* t, const void* dev_text, uint64_t len, void* dev_pos_out, void* dev_counts_out) {
    if (int rc = locate_open(t, true)) return rc;
    if (!dev_pos_out && !dev_counts_out) return fail(KH_ERR_ARG, "no output buffer");
    if (len == 0) return KH_OK;
    if (!dev_text) return fail(KH_ERR_ARG, "null text");
    if (!aligned8(dev_pos_out) || !aligned8(dev_counts_out))
        return fail(KH_ERR_ARG, "positions and counts must be 8-byte aligned");
    if (int rc = set_device(t)) return rc;
    if (int rc = clean_slots(t)) return rc;
    KH_HIP(kh::launch_loc_text(t->kp, (const uint8_t*)dev_text, len, view(t), loc_of(t), (uint64_t*)dev_pos_out,
                               (unsigned long long*)dev_counts_out, t->stream));
    return KH_OK;
}

int kh_locate_text(kh_table* t, const char* host_text, uint64_t len, uint64_t* host_pos_out, uint64_t* counts2) {
    if (int rc = locate_open(t, true)) return rc;
    if (!host_pos_out && !counts2) return fail(KH_ERR_ARG, "no output buffer");
    if (len == 0) return KH_OK;
    if (!host_text) return fail(KH_ERR_ARG, "null text");
    if (int rc = set_device(t)) return rc;
    int rc;
    if ((rc = t->stage.ensure(len))) return rc;
    if (host_pos_out && (rc = t->stage2.ensure(8 * len))) return rc;
    if ((rc = t->stage3.ensure(16))) return rc;
    KH_HIP(hipMemcpyAsync(t->stage.p, host_text, len, hipMemcpyHostToDevice, t->stream));
    if ((rc = kh_locate_text_dev(t, t->stage.p, len, host_pos_out ? t->stage2.p : nullptr, t->stage3.p))) return rc;
    if (host_pos_out) KH_HIP(hipMemcpyAsync(host_pos_out, t->stage2.p, 8 * len, hipMemcpyDeviceToHost, t->stream));
    uint64_t c[2] = {0, 0};
    KH_HIP(hipMemcpyAsync(c, t->stage3.p, 16, hipMemcpyDeviceToHost, t->stream));
    KH_SYNC(t);
    if (counts2) {
        counts2[0] = c[0];
        counts2[1] = c[1];
    }
    return KH_OK;
}

// The reverse-complement forms (kernel in kh_strand.hip): kh_locate_text*'s rules, word for word.
int kh_locate_text_rc_dev(kh_table* t, const void* dev_text, uint64_t len, void* dev_pos_out, void* dev_counts_out) {
    if (int rc = locate_open(t, true)) return rc;
    if (!dev_pos_out && !dev_counts_out) return fail(KH_ERR_ARG, "no output buffer");
    if (len == 0) return KH_OK;
    if (!dev_text) return fail(KH_ERR_ARG, "null text");
    if (!aligned8(dev_pos_out) || !aligned8(dev_counts_out))
        return fail(KH_ERR_ARG, "positions and counts must be 8-byte aligned");
    if (int rc = set_device(t)) return rc;
    if (int rc = clean_slots(t)) return rc;
    KH_HIP(kh::launch_loc_text_rc(t->kp, (const uint8_t*)dev_text, len, view(t), loc_of(t), (uint64_t*)dev_pos_out,
                                  (unsigned long long*)dev_counts_out, t->stream));
    return KH_OK;
}

int kh_locate_text_rc(kh_table* t, const char* host_text, uint64_t len, uint64_t* host_pos_out, uint64_t* counts2) {
    if (int rc = locate_open(t, true)) return rc;
    if (!host_pos_out && !counts2) return fail(KH_ERR_ARG, "no output buffer");
    if (len == 0) return KH_OK;
    if (!host_text) return fail(KH_ERR_ARG, "null text");
    if (int rc = set_device(t)) return rc;
    int rc;
    if ((rc = t->stage.ensure(len))) return rc;
    if (host_pos_out && (rc = t->stage2.ensure(8 * len))) return rc;
    if ((rc = t->stage3.ensure(16))) return rc;
    KH_HIP(hipMemcpyAsync(t->stage.p, host_text, len, hipMemcpyHostToDevice, t->stream));
    if ((rc = kh_locate_text_rc_dev(t, t->stage.p, len, host_pos_out ? t->stage2.p : nullptr, t->stage3.p))) return rc;
    if (host_pos_out) KH_HIP(hipMemcpyAsync(host_pos_out, t->stage2.p, 8 * len, hipMemcpyDeviceToHost, t->stream));
    uint64_t c[2] = {0, 0};
    KH_HIP(hipMemcpyAsync(c, t->stage3.p, 16, hipMemcpyDeviceToHost, t->stream));
    KH_SYNC(t);
    if (counts2) {
        counts2[0] = c[0];
        counts2[1] = c[1];
    }
    return KH_OK;
}

int kh_locate_lines_dev(kh_table* t, const void* dev_pos, uint64_t m, void* dev_line_out, void* dev_col_out) {
    if (int rc = locate_open(t, false)) return rc;
    if (!t->assembled) return fail(KH_ERR_STATE, "no assemble since the last insert/clear");
    if (m == 0) return KH_OK;
    if (!dev_pos || !dev_line_out || !dev_col_out) return fail(KH_ERR_ARG, "null buffer");
    if (!aligned8(dev_pos) || !aligned8(dev_line_out) || !aligned8(dev_col_out))
        return fail(KH_ERR_ARG, "positions, lines and columns must be 8-byte aligned");
    if (int rc = set_device(t)) return rc;
    KH_HIP(kh::launch_loc_lines((const uint64_t*)dev_pos, m, t->contig_off.as<uint64_t>(), t->last_contigs,
                                t->ctr.as<unsigned long long>() + kh::CT_OUT_BYTES, (uint64_t*)dev_line_out,
                                (uint64_t*)dev_col_out, t->stream));
    return KH_OK;
}

}  // extern "C"
