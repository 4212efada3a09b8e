// kh_capi_walk.cpp — the single-GPU walk of the C ABI: explicit starts, kh_assemble(_dev) and the
// contig text / offsets it leaves.
#include "kh_table.hpp"

using namespace khx;

extern "C" {

int kh_set_starts(kh_table* t, const uint8_t* recs, uint64_t n) {
    if (!t) return fail(KH_ERR_ARG, "null table");
    t->ctr_early = false;  // counters may change: assemble reads them on the stream
    if (n && !recs) return fail(KH_ERR_ARG, "null records");
    if (int rc = set_device(t)) return rc;
    int rc;
    if ((rc = ensure_starts(t, n))) return rc;
    const uint64_t bytes = n * (uint64_t)t->kp.R;
    if ((rc = t->stage.ensure(bytes))) return rc;
    if (n) KH_HIP(hipMemcpyAsync(t->stage.p, recs, bytes, hipMemcpyHostToDevice, t->stream));
    KH_HIP(kh::launch_load_starts(t->kp, t->stage.as<uint8_t>(), n, t->starts.as<uint64_t>(),
                                  t->ctr.as<unsigned long long>(), t->stream));
    KH_SYNC(t);
    t->assembled = t->loc_valid = false;
    t->split_ok = false;  // caller's starts may share segments (e.g. two starts on one contig)
    t->starts_explicit = true;
    return KH_OK;
}

int kh_assemble_dev(kh_table* t) {
    if (!t) return fail(KH_ERR_ARG, "null table");
    t->loc_valid = false;  // a new text: positions in the last one mean nothing
    if (int rc = set_device(t)) return rc;
    if (int rc = join_succ(t)) return rc;
    if (int rc = clean_slots(t)) return rc;
    int rc;
    // The start count decides buffer sizes and the grid (the reference also knows
    // start_nodes.size() on the host before walking, kmer_hash.cpp:41).
    unsigned long long cv[kh::CT_NUM];
    if ((rc = read_counters(t, cv, true))) return rc;
    const uint64_t ns = cv[kh::CT_N_STARTS];
    uint64_t nsp = 0;
    const unsigned long long* nsp_dev = nullptr;
    kh::KParams kp = t->kp;
    if (!cv[kh::CT_HOT]) kp.hot = nullptr;  // no remapped region: the walker skips the bitmap load
    // splitter segments only where walks are known disjoint (table-collected starts): a segment
    // is written once, so walks that overlap (explicit starts, malformed input) walk unsegmented
    const bool disjoint = !t->starts_explicit && !t->text_sync;
    if (kp.split_bits && t->split_ok && disjoint)
        nsp = cv[kh::CT_N_SPLIT];
    else
        kp.split_bits = 0;
    // Walk density: enough segments for ~1M walkers in all (few, long contigs: C2, C5) but at
    // least 1 splitter per 256 k-mers, so that no single chain dominates the critical path (the
    // longest segment bounds the walk: C5 with 10^6-k-mer chains took 64 ms at 1 per 4096, with
    // geometric segment lengths up to ~10x their mean; C3 pays +0.2 ms for the extra segments).
    const uint64_t* splits = t->splits.as<uint64_t>();
    if (kp.split_bits && !t->split_forced) {
        // (round 5, C2: a 2^18-walker target 1.25 -> 1.39 ms/step, 2^19 and 2^21 unchanged)
        const uint64_t want = ns < (1ull << 20) ? (1ull << 20) - ns : 0;
        const uint64_t floor_cnt = t->n_inserted >> 8;
        const uint64_t d = want > floor_cnt ? want : floor_cnt;
        int bw = kp.split_bits;
        while (bw < 12 && d && (t->n_inserted >> (bw + 1)) >= d) ++bw;
        if (bw > kp.split_bits && nsp) {
            if ((rc = ensure_list(t, t->splits_w, t->splits_w_cap, nsp))) return rc;
            if ((rc = t->scratch.ensure(kh::scan_scratch_words(nsp) * 8 + 64)) ||
                (rc = t->mask_off.ensure((nsp + 1) * 8)))
                return rc;
            KH_HIP(kh::launch_filter_splits(kp, splits, nsp, bw, t->mask_off.as<uint64_t>(),
                                            t->scratch.as<uint64_t>(), t->splits_w.as<uint64_t>(),
                                            t->ctr.as<unsigned long long>() + kh::CT_N_SPLIT_W, t->stream));
            // nsp stays the bound for sizes; kernels read the exact count (no host round trip)
            nsp_dev = t->ctr.as<unsigned long long>() + kh::CT_N_SPLIT_W;
            splits = t->splits_w.as<uint64_t>();
        }
        kp.split_bits = bw;
    }
    const uint64_t nseg = ns + nsp;
    const uint64_t n = t->n_inserted > ns ? t->n_inserted : ns;
    const uint64_t chunk_cap = n / kh::CHUNK_BASES + nseg + 64;
    if ((rc = t->contig_len.ensure((nseg + 1) * 4))) return rc;
    if ((rc = t->contig_off.ensure((ns + 1) * 8))) return rc;
    if ((rc = t->chunk_data.ensure(chunk_cap * kh::CHUNK_WORDS * 8))) return rc;
    if ((rc = t->chunk_owner.ensure(chunk_cap * 4))) return rc;
    if ((rc = t->chunk_seq.ensure(chunk_cap * 4))) return rc;
    if ((rc = t->scratch.ensure(kh::scan_scratch_words(ns) * 8 + 64))) return rc;
    t->chunk_cap = chunk_cap;
    kh::WalkBuffers wb{};
    wb.starts = t->starts.as<uint64_t>();
    wb.n_starts = ns;
    wb.contig_len = t->contig_len.as<uint32_t>();
    wb.chunk_data = t->chunk_data.as<uint64_t>();
    wb.chunk_owner = t->chunk_owner.as<uint32_t>();
    wb.chunk_seq = t->chunk_seq.as<uint32_t>();
    wb.chunk_cap = chunk_cap;
    wb.max_steps = n;
    // (32 queue batches per atomic for short contigs measured slower at C5 in round 6: walk kernel
    // 2.745 -> 2.87 ms; round 5's 3.27 -> 2.99 predates the single place() site)
    wb.batches = 0;
    wb.headrec = t->headrec.as<uint64_t>();
    wb.hcap = t->headrec.p ? t->hcap : 0u;
    kh::SegBuffers sb{};
    if (kp.split_bits) {
        // walkers may stop before a splitter k-mer even when none was collected (then the link
        // step reports it missing), so the segment arrays exist whenever splitting is on
        const uint64_t cap2 = 2 * nsp + 64;
        if ((rc = t->seg_next.ensure((nseg + 4) * 4)) || (rc = t->seg_key.ensure((nseg + 1) * 16)) ||
            (rc = t->seg_contig.ensure((nseg + 1) * 4)) || (rc = t->seg_off.ensure((nseg + 1) * 4)) ||
            (rc = t->clen.ensure((ns + 1) * 4)) || (rc = t->stab.ensure(cap2 * 16)) ||
            (rc = t->stab_id.ensure(cap2 * 4)) || (rc = t->seg_jump.ensure((nseg + 1) * 4)) ||
            (rc = t->seg_jsum.ensure((nseg + 1) * 4)) || (rc = t->seg_anchor.ensure(nseg + 1)) ||
            (rc = t->seg_pend.ensure((ns + 6) * 4)))
            return rc;
        wb.splits = splits;
        wb.n_splits = nsp;
        wb.n_splits_dev = nsp_dev;
        wb.seg_next = t->seg_next.as<uint32_t>();
        wb.seg_key = t->seg_key.as<uint64_t>();
        sb.stab = t->stab.as<uint64_t>();
        sb.stab_id = t->stab_id.as<uint32_t>();
        sb.cap2 = cap2;
        sb.seg_contig = t->seg_contig.as<uint32_t>();
        sb.seg_off = t->seg_off.as<uint32_t>();
        sb.clen = t->clen.as<uint32_t>();
        sb.jump = t->seg_jump.as<uint32_t>();
        sb.jsum = t->seg_jsum.as<uint32_t>();
        sb.anchor = t->seg_anchor.as<uint8_t>();
        sb.pend = t->seg_pend.as<uint32_t>();
        sb.long_flag = sb.pend + ns + 1;
        // deferred splitter segments (k_walk_q): a contig's walker stops at a splitter only past
        // the walk density's spacing, so contigs shorter than it (C3: all) need no splitter segment
        // and the splitter walkers are skipped; KH_DEBUG=seg_eager stops at every splitter
        // (not where the mean contig is longer than the splitter spacing, C2: most walkers stop
        // anyway and phase 1 would only run after the start walkers instead of beside them)
        wb.seg_long = sb.pend + ns + 2;  // [0] a contig's walker stopped at a splitter, [1] splitter walkers deferred
        const bool short_mean = ns && n / ns <= (1ull << kp.split_bits);
        wb.split_min = (kh::debug_flag("seg_eager") || !short_mean) ? 0u : (1u << kp.split_bits);
    }
    unsigned long long* ctr = t->ctr.as<unsigned long long>();
    unsigned long long* stats = t->stats.as<unsigned long long>();
    // Walks from the table's own start k-mers are disjoint: the text is at most K + 1 bytes per
    // contig plus one per k-mer, and the chunk pool holds them, so the text is sized before the
    // walk and nothing is read back between walk and text (one host round trip less per assemble;
    // a total past the bound, only possible on malformed input, is not written and kh_assemble
    // redoes the walk the slow way). Otherwise (explicit starts: walks that overlap, e.g. two
    // starts on one contig, make the text longer than the k-mer count) the text is sized from the
    // scanned total, and if overlapping walks exhaust the chunk pool the walk is redone once with
    // the pool the first attempt asked for.
    const bool bounded = !t->starts_explicit && !t->text_sync;
    t->text_sync = false;
    t->walk_bounded = bounded;
    if (bounded) {
        if ((rc = t->text.ensure(ns * (uint64_t)(t->kp.K + 1) + n + 64))) return rc;
        wb.text_cap = t->text.bytes;
    }
    auto materialize = [&](char* out, int phase, uint32_t* line_first, uint64_t out_bytes) {
        uint64_t *off = t->contig_off.as<uint64_t>(), *scr = t->scratch.as<uint64_t>();
        return kp.split_bits
                   ? kh::launch_materialize_seg(kp, wb, sb, off, scr, out, ctr, t->stream, phase, line_first, out_bytes)
                   : kh::launch_materialize(kp, wb, off, scr, out, ctr, t->stream, phase, line_first, out_bytes);
    };
    for (int attempt = 0;; ++attempt) {
        {
            kh::FillSet f;
            f.add(ctr + kh::CT_WALK_NEXT, 8 * 3, 0);  // WALK, CHUNK, OUT
            if (kp.split_bits) f.add(wb.seg_next, nseg * 4, 0xff);
            if (wb.split_min) {
                f.add(wb.seg_long, 16, 0);
                f.add(wb.contig_len + ns, nsp * 4, 0);  // phase 1: not walked yet
            }
            KH_HIP(kh::launch_fill(f, t->stream));
        }
        KH_HIP(hipEventRecord(t->ev_walk0, t->stream));
        // Successor runs of the head records (k_rec_succ). A record read before its successor is
        // resolved still says 0 (the walker probes, as without), so the resolve runs on the side
        // stream beside the walk (request-bound beside a latency-bound walker); the table stream
        // waits for it after the walk (the next build rewrites the records).
        bool succ_side = false;
        if (attempt == 0 && wb.hcap && kh::rec_succ_fits(kp, wb.hcap)) {
            // beside the walk where a torn read is harmless (rec_succ_side: k > 40 at 16-B slots),
            // else before it on the table stream; beside the walk 1024 blocks (C3 walk + resolve
            // 1.28 ms; the full 8192-block grid 1.32-1.34, 256 blocks 1.85: the resolve then lags
            // the walkers; no resolve 1.46)
            const bool conc = kh::rec_succ_side(kp);
            const unsigned blocks = conc ? 1024u : 0u;
            hipStream_t rs = t->stream;
            if (conc && t->side) {
                KH_HIP(hipEventRecord(t->ev_side, t->stream));
                KH_HIP(hipStreamWaitEvent(t->side, t->ev_side, 0));
                rs = t->side;
                succ_side = true;
            }
            KH_HIP(kh::launch_rec_succ(kp, view(t), t->headrec.as<uint64_t>(), wb.hcap, rs, blocks));
        }
        // the splitter table reads only the splitter list: behind the resolve, beside the walk
        // (walk bracket C3 1.35 -> 1.33, C2 0.61 -> 0.59, C5 3.46 -> 3.43 ms;
        // profiles/r05/ab/ab_seg_table_beside_walk.txt)
        if (kp.split_bits) KH_HIP(kh::launch_seg_table(kp, wb, sb, succ_side ? t->side : t->stream));
        if (succ_side) KH_HIP(hipEventRecord(t->ev_conv, t->side));
        // three walker blocks per CU for 16-B slots at load <= 0.6, else two (kh_kernels.hip)
        // (round 5, after the single place() site: 4 / 5 blocks per CU C3 walk 1.40 / 1.43 ms vs 1.16)
        const int wgrid = (kp.W == 2 && t->load <= 0.6) ? -3 : -2;
        KH_HIP(kh::launch_walk(kp, view(t), wb, ctr, stats, wgrid, t->stream));
        if (wb.split_min && wb.n_splits) {  // the splitter walkers, if some contig was long
            kh::WalkBuffers wb1 = wb;
            wb1.phase = 1;
            KH_HIP(hipMemsetAsync(ctr + kh::CT_WALK_NEXT, 0, 8, t->stream));
            KH_HIP(kh::launch_walk(kp, view(t), wb1, ctr, stats, wgrid, t->stream));
        }
        if (succ_side) KH_HIP(hipStreamWaitEvent(t->stream, t->ev_conv, 0));
        // the splitter table, if the walk found it needed and it was not built beside the walk
        if (kp.split_bits && wb.split_min) KH_HIP(kh::launch_seg_table(kp, wb, sb, t->stream, true));
        KH_HIP(hipEventRecord(t->ev_wk1, t->stream));
        t->wk_timed = true;
        if (kp.split_bits) KH_HIP(kh::launch_segments(kp, wb, sb, stats, t->stream));
        KH_HIP(hipEventRecord(t->ev_walk1, t->stream));
        KH_HIP(materialize(nullptr, kh::MAT_SCAN, nullptr, 0));
        if (bounded) break;
        unsigned long long hv[2], ovf = 0;
        KH_HIP(hipMemcpyAsync(hv, ctr + kh::CT_CHUNK_NEXT, sizeof hv, hipMemcpyDeviceToHost, t->stream));
        KH_HIP(hipMemcpyAsync(&ovf, stats + kh::ST_CHUNK_OVF, 8, hipMemcpyDeviceToHost, t->stream));
        KH_SYNC(t);
        if (ns == 0) hv[1] = 0;
        if (ovf && attempt == 0) {
            const uint64_t need = nseg + hv[0] + 64;
            if ((rc = t->chunk_data.ensure(need * kh::CHUNK_WORDS * 8)) || (rc = t->chunk_owner.ensure(need * 4)) ||
                (rc = t->chunk_seq.ensure(need * 4)))
                return rc;
            t->chunk_cap = wb.chunk_cap = need;
            wb.chunk_data = t->chunk_data.as<uint64_t>();
            wb.chunk_owner = t->chunk_owner.as<uint32_t>();
            wb.chunk_seq = t->chunk_seq.as<uint32_t>();
            KH_HIP(hipMemsetAsync(stats + kh::ST_CHUNK_OVF, 0, 8, t->stream));
            continue;  // (seg_next is reset at the top of the attempt)
        }
        if ((rc = t->text.ensure(hv[1] + 64))) return rc;
        break;
    }
    if ((rc = t->line_first.ensure(kh::line_first_words(t->text.bytes) * 4))) return rc;
    KH_HIP(materialize(t->text.as<char>(), kh::MAT_WRITE, t->line_first.as<uint32_t>(), t->text.bytes));
    KH_HIP(hipEventRecord(t->ev_mat1, t->stream));
    t->walk_timed = true;
    t->last_contigs = ns;
    t->assembled = true;
    return KH_OK;
}

int kh_assemble(kh_table* t, uint64_t* n_contigs, uint64_t* out_bytes) {
    if (int rc = kh_assemble_dev(t)) return rc;
    // the stats and the text's byte count in one wait (ordered after the queued work)
    unsigned long long st[kh::ST_NUM], ob = 0;
    KH_HIP(hipMemcpyAsync(st, t->stats.p, sizeof st, hipMemcpyDeviceToHost, t->stream));
    KH_HIP(hipMemcpyAsync(&ob, t->ctr.as<unsigned long long>() + kh::CT_OUT_BYTES, 8, hipMemcpyDeviceToHost,
                          t->stream));
    KH_SYNC(t);
    // a walk sized before it ran (kh_assemble_dev's bound) that passed its text bound or ran out of
    // walker chunks (both only on malformed input, e.g. walks that overlap) is redone the slow way:
    // the text sized from the scanned total, the chunk pool from what the first attempt asked for
    if (t->walk_bounded && t->last_contigs && (st[kh::ST_CHUNK_OVF] || ob > t->text.bytes)) {
        KH_HIP(hipMemsetAsync(t->stats.as<unsigned long long>() + kh::ST_CHUNK_OVF, 0, 8, t->stream));
        t->text_sync = true;
        if (int rc = kh_assemble_dev(t)) return rc;
        if (int rc = check_stats(t)) return rc;
        uint64_t o2 = 0;
        if (int rc = read_ctr(t, kh::CT_OUT_BYTES, &o2)) return rc;
        ob = o2;
    } else if (int rc = stats_status(st)) {
        return rc;
    }
    if (n_contigs) *n_contigs = t->last_contigs;
    if (out_bytes) *out_bytes = ob;
    return KH_OK;
}

int kh_contigs_text_dev(kh_table* t, const char** dev_text, uint64_t* bytes) {
    if (!t || !dev_text || !bytes) return fail(KH_ERR_ARG, "null argument");
    if (!t->assembled) return fail(KH_ERR_STATE, "no assemble since the last insert/clear");
    uint64_t ob = 0;
    if (int rc = read_ctr(t, kh::CT_OUT_BYTES, &ob)) return rc;
    if (t->last_contigs && ob > t->text.bytes)
        return fail(KH_ERR_STATE, "contig text of %llu bytes passed its %llu-byte bound (malformed input?): "
                                  "kh_assemble redoes the walk sized", (unsigned long long)ob,
                    (unsigned long long)t->text.bytes);
    *dev_text = t->text.as<const char>();
    *bytes = t->last_contigs ? ob : 0;
    return KH_OK;
}

int kh_contigs_text(kh_table* t, char* out, uint64_t cap) {
    const char* d = nullptr;
    uint64_t b = 0;
    if (int rc = kh_contigs_text_dev(t, &d, &b)) return rc;
    if (cap < b) return fail(KH_ERR_ARG, "buffer of %llu bytes < %llu", (unsigned long long)cap,
                             (unsigned long long)b);
    if (b) KH_HIP(hipMemcpy(out, d, b, hipMemcpyDeviceToHost));
    return KH_OK;
}

int kh_contigs_offsets(kh_table* t, uint64_t* out, uint64_t n) {
    if (!t || (!out && n)) return fail(KH_ERR_ARG, "null argument");
    if (!t->assembled) return fail(KH_ERR_STATE, "no assemble since the last insert/clear");
    if (n > t->last_contigs) return fail(KH_ERR_ARG, "asked for %llu offsets of %llu contigs",
                                         (unsigned long long)n, (unsigned long long)t->last_contigs);
    if (n) {
        KH_SYNC(t);
        KH_HIP(hipMemcpy(out, t->contig_off.p, n * 8, hipMemcpyDeviceToHost));
    }
    return KH_OK;
}

}  // extern "C"
