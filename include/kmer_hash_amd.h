/* kmer_hash_amd.h — C ABI of the MI355X-native k-mer hash table + contig walker.
 *
 * Drop-in boundary for the hot path of fractalclockwork/CS267_HW3 (hash_map.hpp / kmer_hash.cpp).
 * Plain C: pointers and sizes only, no C++ or torch types, no exceptions across the boundary.
 * Every entry point returns KH_OK (0) or a negative KH_ERR_*; kh_last_error() gives a message
 * (thread-local). A handle is not thread-safe; use one per host thread / process.
 *
 * Record formats (byte-identical to the reference types, align 1):
 *   key    = pkmer_t   : PACKED = (k+3)/4 bytes, 2 bits/base MSB-first, A=0 C=1 G=2 T=3,
 *                        'A'-padded tail                          (pkmer_t.hpp:6, packing.hpp:77-92)
 *   record = kmer_pair : PACKED key bytes + fb_ext[2] = {backward, forward} chars in {A,C,G,T,F}
 *                        sizeof = PACKED + 2 = 7 (k=19) / 15 (k=51)          (kmer_t.hpp:6-8,43-45)
 *   contig text        : one contig per line, extract_contig() bytes + '\n', in start-node order
 *                        = the bytes of test_<rank>.dat                (read_kmers.hpp:81-92,
 *                                                                       kmer_hash.cpp:60-68)
 * Reference entry points replaced (see INTEGRATION.md for the bindings):
 *   kh_create      <- DistributedHashMap(size, rank, world)  hash_map.hpp:50-52; HashMap(size)
 *   kh_insert*     <- DistributedHashMap::insert_all        hash_map.hpp:55-80; HashMap::insert
 *                     + start-node collection               kmer_hash.cpp:21-33
 *   kh_find*       <- DistributedHashMap::find              hash_map.hpp:83-107; HashMap::find
 *   kh_assemble*   <- assemble_contigs                      kmer_hash.cpp:38-55
 *   kh_contigs_*   <- extract_contig + output_results       read_kmers.hpp:81-92, kmer_hash.cpp:60-68
 *   kh_pack_text   <- read_kmers line parsing               read_kmers.hpp:54-79
 */
#ifndef KMER_HASH_AMD_H
#define KMER_HASH_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KH_ABI_VERSION 3
#define KH_K_MAX 60

enum {
    KH_OK = 0,
    KH_ERR_ARG = -1,        /* bad argument / unsupported k / misaligned device pointer */
    KH_ERR_HIP = -2,        /* HIP runtime error (message has the hipError string) */
    KH_ERR_NOMEM = -3,      /* device or host allocation failed */
    KH_ERR_FULL = -4,       /* more k-mers than the table was created for / probe wrapped */
    KH_ERR_NOT_FOUND = -5,  /* walk: next k-mer missing (kmer_hash.cpp:47-49 throws) */
    KH_ERR_DUPLICATE = -6,  /* insert: key already present (input contract: unique k-mers) */
    KH_ERR_CYCLE = -7,      /* walk: chain longer than the table (no 'F' end) */
    KH_ERR_BAD_BASE = -8,   /* extension byte outside {A,C,G,T,F} */
    KH_ERR_STATE = -9       /* call order (e.g. contigs requested before assemble) */
};

typedef struct kh_table kh_table;

typedef struct kh_stats {
    uint64_t capacity;       /* table slots */
    uint64_t n_inserted;     /* records inserted since create/clear */
    uint64_t n_starts;       /* start k-mers collected (bwd == 'F') or set explicitly */
    uint64_t n_contigs;      /* contigs produced by the last assemble (= n_starts) */
    uint64_t n_lookups;      /* successful walk lookups of the last assemble = sum(len - 1) */
    uint64_t out_bytes;      /* contig text bytes of the last assemble, '\n' included */
    uint64_t n_chunks;       /* 256-base chunks used by the walker */
    uint64_t n_dup, n_full, n_bad_ext, n_missing, n_cycle, n_spin, n_chunk_ovf;
    double ms_insert;        /* device ms, last insert call (table insert + start compaction) */
    double ms_insert_kernel; /* device ms, k_insert alone, last insert call */
    double ms_walk;          /* device ms, k_walk, last assemble */
    double ms_materialize;   /* device ms, offsets scan + contig text, last assemble */
    uint64_t n_bad_base;     /* kh_pack_text_dev lines with a k-mer base outside {A,C,G,T} */
    double ms_build;         /* device ms, region build + overflow inserts of the last partitioned insert */
    double ms_walk_kernel;   /* device ms, k_walk_q alone, last assemble */
    uint64_t n_hot_regions;  /* placement regions remapped (shared minimizers overfilled them): keys by (minimizer, neighbour window) */
    uint64_t n_overflow;     /* keys of the last partitioned build inserted by global CAS (full windows,
                                probe runs that left their region slice) */
    uint64_t n_spread_regions; /* remap targets the remap itself overfilled (a family sharing its
                                  neighbour window too): their remapped keys placed by key hash */
} kh_stats;

/* ---- sizes / info --------------------------------------------------------------------------*/
int kh_abi_version(void);
/* Device bytes the library's buffers hold now in this process (every table) and their high-water
 * mark since the last reset (reset_peak != 0 restarts it at `now` after reading). */
int kh_device_bytes(uint64_t* now, uint64_t* peak, int reset_peak);
int kh_packed_size(int k);   /* sizeof(pkmer_t)   */
int kh_record_size(int k);   /* sizeof(kmer_pair) */
const char* kh_last_error(void);
int kh_device_count(int* n);

/* ---- table lifetime --------------------------------------------------------------------------
 * Capacity = ceil(n_kmers / load_factor) slots (kmer_hash.cpp:108-109 uses load 0.5 -> 2n).
 * Device memory: capacity * (8 B if k <= 29 else 16 B) for the table, plus walker buffers.
 * All work is enqueued on the table's stream (its own, or one set with kh_set_stream). */
int kh_create(kh_table** out, int k, uint64_t n_kmers, double load_factor, int device);
int kh_destroy(kh_table* t);
int kh_clear(kh_table* t);                       /* empty table + start list (async) */
/* Grow an empty table (after create or clear) to hold n_kmers at the creation load factor; a
 * no-op when it already does. The sharded path sizes each shard from the routed counts. */
int kh_reserve(kh_table* t, uint64_t n_kmers);
int kh_set_stream(kh_table* t, void* hip_stream); /* NULL = back to the table's own stream */
int kh_sync(kh_table* t);                        /* wait for the stream; report device errors */
uint64_t kh_capacity(const kh_table* t);
/* blocking host waits on the table's stream so far (device -> host reads of counts, syncs):
 * hosts count the round trips of a sharded step with it (tests/test_gpu_dist.py) */
int kh_host_syncs(const kh_table* t, uint64_t* n);
int kh_get_stats(kh_table* t, kh_stats* out);    /* syncs */

/* ---- insert: records in kmer_pair layout. Start k-mers (bwd == 'F') of every batch are appended
 * to the table's start list in record order (kmer_hash.cpp:27-31). --------------------------*/
int kh_insert(kh_table* t, const uint8_t* host_recs, uint64_t n);   /* synchronous */
int kh_insert_dev(kh_table* t, const void* dev_recs, uint64_t n);   /* async, 16-B aligned */

/* ---- find: keys in pkmer_t layout; out gets kmer_pair records, found[i] = 0/1 ----------------*/
int kh_find(kh_table* t, const uint8_t* host_keys, uint64_t n, uint8_t* host_recs_out,
            uint8_t* host_found);
int kh_find_dev(kh_table* t, const void* dev_keys, uint64_t n, void* dev_recs_out,
                void* dev_found);

/* ---- find over text: every k-mer of a batch of sequences ---------------------------------------
 * Batches DistributedHashMap::find / HashMap::find (hash_map.hpp:83-107) over read_kmers.hpp-style
 * text: the caller hands over the bytes of reads, contigs (test_<rank>.dat) or FASTA lines instead
 * of cutting, 2-bit-packing and uploading PACKED bytes per k-mer.
 *   input   len bytes of text, any alignment.
 *   window  position i has a window iff bytes i .. i+K-1 all lie in the text and are each one of
 *           A C G T (upper case). Any other byte ('\n', '\r', space, N, F, lower case, 0, 0xFF, ...)
 *           ends the windows that would cover it, so line structure needs no parsing; a header
 *           line yields whatever windows its letters form.
 *   answer  2 bytes per position: the k-mer is in the table: the {backward, forward} extension
 *           chars of its record, as kh_find_answer_dev gives them; window present, k-mer absent:
 *           {0, 0}; no window at i: {KH_TEXT_NONE, KH_TEXT_NONE}.
 *   counts  2 uint64 {windows, found}.
 *   len == 0: KH_OK, nothing written. len < K: every position NONE, counts {0, 0}.
 *   An empty or cleared table answers absent for every window; a staged insert left open:
 *   KH_ERR_STATE. Legal before and after assemble; changes neither the table, the start list nor
 *   a walk. The kernel works on tiles of KH_TEXT_TILE positions (+ a K-1 byte halo) per block. */
#define KH_TEXT_NONE 0xFF
#define KH_TEXT_TILE 2048
/* async on the table's stream; dev_ext_out: 2*len bytes or NULL (counts only); dev_counts_out:
 * 2 uint64 (8-byte aligned) or NULL; both NULL, a null text with len > 0: KH_ERR_ARG. Text and
 * answers may have any alignment. */
int kh_find_text_dev(kh_table* t, const void* dev_text, uint64_t len, void* dev_ext_out, void* dev_counts_out);
/* synchronous host form (staged upload / download like kh_find); either output may be NULL */
int kh_find_text(kh_table* t, const char* host_text, uint64_t len, uint8_t* host_ext_out, uint64_t* counts2);
/* the windows of the text as pkmer_t keys, in ascending position: keys_out holds up to
 * max(len-K+1, 0) keys of PACKED bytes (any alignment), pos_out the uint32 position of each,
 * count_out 1 uint64 on the device (always written). keys_out and pos_out both NULL: the count
 * only. len >= 2^32: KH_ERR_ARG. Async; needs no table contents (works on an empty table). */
int kh_text_keys_dev(kh_table* t, const void* dev_text, uint64_t len, void* dev_keys_out, void* dev_pos_out,
                     void* dev_count_out);

/* ---- assemble --------------------------------------------------------------------------------
 * Walks every start k-mer (collected by the inserts, or replaced by kh_set_starts) until its
 * forward extension is 'F', producing the contig text in start-node order on the device. */
int kh_set_starts(kh_table* t, const uint8_t* host_start_recs, uint64_t n);
int kh_assemble_dev(kh_table* t);                 /* async */
int kh_assemble(kh_table* t, uint64_t* n_contigs, uint64_t* out_bytes);  /* sync + checks */
int kh_contigs_text(kh_table* t, char* host_out, uint64_t cap);          /* D2H of the text */
int kh_contigs_text_dev(kh_table* t, const char** dev_text, uint64_t* bytes);
int kh_contigs_offsets(kh_table* t, uint64_t* host_offsets, uint64_t n); /* line starts */

/* ---- locate: where in the assembled contigs a k-mer sits ----------------------------------------
 * A position index beside the table: one uint64 per slot (capacity * 8 bytes of device memory,
 * counted by kh_device_bytes), allocated by the first kh_locate_reset / kh_locate_build and kept
 * until kh_locate_drop / kh_destroy. KH_LOC_NONE (all ones) = no position. What later stages
 * (seeding reads against the contigs, scaffolding, coverage per contig) would otherwise rebuild on
 * the host from the downloaded contig text.
 *   build   kh_locate_build: reset, then every k-mer of the table's own contig text (the bytes of
 *           test_<rank>.dat, as kh_contigs_text_dev gives them) gets its byte offset in that text.
 *           kh_locate_set_dev: caller-supplied uint64 values for pkmer_t keys (the sharded path
 *           gives rank << 48 | offset). Every write is a minimum: a k-mer given several positions
 *           (two lines of overlapping walks after kh_set_starts, a key set twice) keeps the
 *           smallest, the same on every run.
 *   query   by keys (kh_locate*) or for every position of a text (kh_locate_text*, windows as for
 *           kh_find_text): the k-mer's value; KH_LOC_NONE when there is no window, the table does
 *           not hold the k-mer, or it has no value (a k-mer on no contig). counts: 2 uint64
 *           {windows, located}. kh_locate_lines_dev turns positions in the table's contig text
 *           into {line index, column} over the last assemble's line starts (kh_contigs_offsets);
 *           KH_LOC_NONE, or a position past the text, gives KH_LOC_NONE for both.
 *   alignment   keys and text: any. Value, position, line, column and count buffers: 8 bytes,
 *           else KH_ERR_ARG.
 *   empty   m == 0 / len == 0: KH_OK, nothing written. len < K: every position KH_LOC_NONE,
 *           counts {0, 0}.
 *   null    a null table, a null required buffer, or both outputs of kh_locate_text* NULL:
 *           KH_ERR_ARG; either single output may be NULL, as for kh_find_text*; dev_missing_out
 *           may be NULL.
 *   state   a staged insert left open: KH_ERR_STATE. set / locate / locate_text without a valid
 *           index: KH_ERR_STATE. build / locate_lines without an assemble: KH_ERR_STATE.
 *   invalidation   every insert entry point, kh_clear, a kh_reserve that grows, kh_set_starts,
 *           the start collection of the routes and a new kh_assemble* / kh_mwalk_* walk make the
 *           index invalid (its memory is kept); kh_locate_build after a walk that kh_assemble
 *           redid internally indexes the final text.
 *   None of these changes the slots, the start list, a walk, the contig text or what kh_find*
 *   answers. All but kh_locate, kh_locate_text (synchronous, staged like kh_find) and
 *   kh_locate_drop are asynchronous on the table's stream; kh_locate_build may first wait for the
 *   walk, as kh_contigs_text_dev does. */
#define KH_LOC_NONE 0xFFFFFFFFFFFFFFFFull
int kh_locate_reset(kh_table* t);      /* allocate if needed, fill with NONE, index becomes valid */
int kh_locate_drop(kh_table* t);       /* free the index's device memory; index invalid */
int kh_locate_build(kh_table* t);      /* reset + positions = byte offsets into test_<rank>.dat */
/* dev_missing_out: 1 uint64 (keys the table does not hold: skipped) or NULL */
int kh_locate_set_dev(kh_table* t, const void* dev_keys, uint64_t m, const void* dev_values,
                      void* dev_missing_out);
int kh_locate_dev(kh_table* t, const void* dev_keys, uint64_t m, void* dev_pos_out);
int kh_locate(kh_table* t, const uint8_t* host_keys, uint64_t m, uint64_t* host_pos_out);
int kh_locate_text_dev(kh_table* t, const void* dev_text, uint64_t len, void* dev_pos_out, void* dev_counts_out);
int kh_locate_text(kh_table* t, const char* host_text, uint64_t len, uint64_t* host_pos_out, uint64_t* counts2);
/* The same for the reverse complement of every window (see "seed, both strands" below): position i
 * answers the value kh_locate_dev gives the key of rc(window i). Rules, counts and alignment as above. */
int kh_locate_text_rc_dev(kh_table* t, const void* dev_text, uint64_t len, void* dev_pos_out, void* dev_counts_out);
int kh_locate_text_rc(kh_table* t, const char* host_text, uint64_t len, uint64_t* host_pos_out, uint64_t* counts2);
int kh_locate_lines_dev(kh_table* t, const void* dev_pos, uint64_t m, void* dev_line_out, void* dev_col_out);

/* ---- seed: where a read lies on the contigs ------------------------------------------------------
 * The consumer of the position index: for each read of a batch, the longest stretch that matches a
 * contig exactly, found on the device from the positions kh_locate_text_dev answers, and the coverage
 * per contig line those seeds give. These calls look at the strand the contigs are written in; the
 * kh_seed_strand_* calls below look at both.
 *   text    len bytes, any alignment, as for kh_locate_text*.
 *   reads   read_off: n_reads + 1 uint64 on the device, 8-byte aligned, non-decreasing. Read r is the
 *           bytes [read_off[r], min(read_off[r+1], len)), empty when that range is empty; bytes
 *           outside every read are ignored. The offsets are clamped: nothing past len or past
 *           read_off[n_reads] is read, whatever they hold.
 *   counted window of read r: a position i with a window in the kh_find_text sense (bytes i .. i+K-1
 *           in the text, each one of A C G T) and i + K <= the end of read r. A window that reaches
 *           into the next read is not counted, separator byte or not.
 *   value   v[i]: what kh_locate_text_dev answers at i; KH_LOC_NONE = not located.
 *   continuation   i continues i-1 iff both are counted windows of the same read, both are located
 *           and v[i] == v[i-1] + 1 in 64 bits. KH_LOC_NONE never continues and is never continued
 *           (0xFFFFFFFFFFFFFFFE + 1 is KH_LOC_NONE).
 *   run     a maximal chain of continuations; a single located window is a run of 1. The seed of a
 *           read is its longest run, the one with the smallest i on a tie.
 *   answer  KH_SEED_WORDS uint64 per read: {start of the run relative to the read's first byte, v at
 *           the run's first window, run length in windows, located counted windows of the read}; a
 *           read without a located window (empty, shorter than K, all absent) answers
 *           {KH_LOC_NONE, KH_LOC_NONE, 0, 0}. Matched bases = run + K - 1. A run over positions that
 *           kh_locate_build gave lies on one contig line: the values v+1 .. v+K after a line's last
 *           window cover its '\n', and no k-mer holds them.
 *   kh_seed_runs_dev   the run search alone over any position array of len uint64 (the sharded path
 *           feeds it rank << 48 | offset values). It needs no index and reads nothing of the table:
 *           the handle supplies K and the stream. Asynchronous.
 *   kh_seed_text_dev   kh_locate_text_dev into dev_pos_scratch (len uint64, 8-byte aligned, the
 *           caller's; it holds the positions afterwards), then the run search, on the table's
 *           stream; the library allocates nothing. State rules of kh_locate_text_dev: no valid index
 *           or a staged insert left open give KH_ERR_STATE.
 *   kh_seed_text       the synchronous host form, staged like kh_locate_text.
 *   kh_seed_coverage_dev   per contig line of the last assemble: every seed with run > 0 whose value
 *           lies in the table's contig text adds 1 to reads_per_line[line] and run + K - 1 to
 *           bases_per_line[line] (64-bit atomics; line as kh_locate_lines_dev finds it). It adds to
 *           what the arrays hold, because reads come in batches: the caller zeroes them. Both are
 *           n_contigs uint64; either may be NULL, not both. A value of KH_LOC_NONE or past the text
 *           is skipped. Without an assemble, or with a staged insert open: KH_ERR_STATE.
 *           Asynchronous.
 *   empty   n_reads == 0: KH_OK, nothing written. len == 0 with reads: every read answers the empty
 *           answer (text, positions and scratch may then be NULL).
 *   errors  a null table or a null required buffer, a read-offset, position, seed or per-line buffer
 *           that is not 8-byte aligned, n_reads >= 2^32: KH_ERR_ARG.
 *   None of these changes the slots, the start list, a walk, the contig text, the index or what
 *   kh_find* / kh_locate* answer. */
#define KH_SEED_WORDS 4
int kh_seed_runs_dev(kh_table* t, const void* dev_pos, uint64_t len, const void* dev_read_off,
                     uint64_t n_reads, void* dev_seeds_out);
int kh_seed_text_dev(kh_table* t, const void* dev_text, uint64_t len, const void* dev_read_off,
                     uint64_t n_reads, void* dev_pos_scratch, void* dev_seeds_out);
int kh_seed_text(kh_table* t, const char* host_text, uint64_t len, const uint64_t* host_read_off,
                 uint64_t n_reads, uint64_t* host_seeds_out);
int kh_seed_coverage_dev(kh_table* t, const void* dev_seeds, uint64_t n_reads,
                         void* dev_reads_per_line, void* dev_bases_per_line);

/* ---- seed, both strands: reads from the strand the contigs were not written in ---------------------
 * A sequencer reads either strand; the table and its contigs hold one. These calls place a read by its
 * own bases (forward) or by their reverse complement (reverse), whichever gives the longer exact run.
 *   rc(window)   the K bases of the window in reverse order, each complemented (A<->T, C<->G; in
 *           2-bit codes, code ^ 3).
 *   w[i]    KH_LOC_NONE unless position i has a window in the kh_find_text sense (K bytes inside the
 *           text, each one of A C G T); where it has one, what the index answers for rc(window i): the
 *           value kh_locate_dev would give that key. kh_locate_text_rc* answer w for a whole text, with
 *           counts {windows, located}, under kh_locate_text*'s rules.
 *   v[i]    what kh_locate_text_dev answers at i.
 *   counted windows and reads: exactly as for kh_seed_* (i + K <= the read's end, offsets clamped).
 *   forward continuation and run: as for kh_seed_* (v[i] == v[i-1] + 1).
 *   reverse continuation   i continues i-1 iff both are counted windows of the same read,
 *           w[i] != KH_LOC_NONE, w[i-1] != KH_LOC_NONE and w[i-1] == w[i] + 1 in 64 bits: if rc(window
 *           i) stands at contig position p, rc(window i+1) stands at p - 1. A window with w == 0 is
 *           never continued (0 - 1 is KH_LOC_NONE). A reverse run is a maximal chain of them.
 *   strand seed of a read: the longest forward run (the first on a tie) and the longest reverse run
 *           (the first on a tie); the longer of the two, the forward one when they are equal.
 *   answer  KH_SEED_STRAND_WORDS uint64 per read: {start, value, run, strand, located_fwd, located_rc}.
 *           start = the run's first window relative to the read's first byte; strand = 0 forward, 1
 *           reverse; value = v at the run's first window (forward), w at the run's LAST window
 *           (reverse): the smallest value of the run, w[start] - (run - 1). On either strand the
 *           matched stretch of contig text is the bytes [value, value + run + K - 1). located_fwd /
 *           located_rc = the read's counted windows with v / w != KH_LOC_NONE. A read with no located
 *           window on either strand answers {KH_LOC_NONE, KH_LOC_NONE, 0, 0, 0, 0}. A reverse run over
 *           positions that kh_locate_build gave lies on one contig line, as a forward one does: the K
 *           values after a line's last window hold no k-mer.
 *   kh_seed_strand_runs_dev   the run search alone over two position arrays of len uint64 each (the
 *           sharded path feeds it rank << 48 | offset values; a run's values are located words of one
 *           rank, so the subtraction never borrows from the rank bits). It needs no index and reads
 *           nothing of the table. Asynchronous.
 *   kh_seed_strand_text_dev   kh_locate_text_dev into dev_pos_scratch[0, len) and
 *           kh_locate_text_rc_dev into dev_pos_scratch[len, 2 * len) (2 * len uint64, 8-byte aligned,
 *           the caller's; they hold v and w afterwards), then the run search, on the table's stream;
 *           the library allocates nothing. State rules of kh_locate_text_dev.
 *   kh_seed_strand_text       the synchronous host form, staged like kh_seed_text (16 * len bytes of
 *           position staging).
 *   empty, errors, state: those of kh_seed_runs_dev, kh_seed_text_dev and kh_seed_text: n_reads == 0
 *           writes nothing; len == 0 with reads answers the empty answer (text, positions and scratch
 *           may then be NULL); a null table or required buffer, a misaligned buffer or n_reads >= 2^32:
 *           KH_ERR_ARG; no valid index or a staged insert left open: KH_ERR_STATE for the calls that
 *           read the index.
 *   coverage   kh_seed_coverage_dev takes 4-word seeds: repack {start, value, run, located_fwd +
 *           located_rc}; value is the lowest contig position of the run on either strand.
 *   None of these changes the slots, the start list, a walk, the contig text, the index or what any
 *   other call answers. */
#define KH_SEED_STRAND_WORDS 6
int kh_seed_strand_runs_dev(kh_table* t, const void* dev_pos_fwd, const void* dev_pos_rc, uint64_t len,
                            const void* dev_read_off, uint64_t n_reads, void* dev_seeds_out);
int kh_seed_strand_text_dev(kh_table* t, const void* dev_text, uint64_t len, const void* dev_read_off,
                            uint64_t n_reads, void* dev_pos_scratch /* 2*len uint64 */, void* dev_seeds_out);
int kh_seed_strand_text(kh_table* t, const char* host_text, uint64_t len, const uint64_t* host_read_off,
                        uint64_t n_reads, uint64_t* host_seeds_out);

/* ---- sharded multi-GPU path --------------------------------------------------------------------
 * One table per rank (GPU). The key space is split by an owner hash; the caller moves the buffers
 * between ranks (RCCL all-to-all over xGMI: include/cs267_hw3_amd/dist_hash_map.hpp, cs267_hw3_amd/dist.py). Replaces the per-owner batched
 * insert RPCs (hash_map.hpp:38-46,64-77) and the per-step remote find RPCs (hash_map.hpp:94-100).
 * Routed records and query keys are kh_word_count(k) 64-bit words each. counts_out receives
 * nranks + 1 uint64 on the device: per-destination counts, then their total. All async. */
int kh_word_count(int k);
/* Rank (0..nranks-1) owning a pkmer_t key under the table's sharding (the route and the walk use
 * the same function); < 0 on a bad argument. Replaces hash_map.hpp:28-30 get_target_rank. */
int kh_key_owner(const kh_table* t, const uint8_t* packed_key, int nranks);
int kh_collect_starts_dev(kh_table* t, const void* dev_recs, uint64_t n); /* local start k-mers */
/* read_kmers.hpp:62-76 on the GPU: len bytes of fixed-width "KMER BF\n" lines (k+4 bytes each)
 * in device memory -> *n_out = len / (k+4) kmer_pair records at dev_recs (16-byte aligned; NULL:
 * count only), on the table's stream. A line whose k-mer has a base outside {A,C,G,T} makes the
 * next kh_sync fail with KH_ERR_BAD_BASE (the host kh_pack_text fails at once). */
int kh_pack_text_dev(kh_table* t, const void* dev_text, uint64_t len, void* dev_recs, uint64_t* n_out);
int kh_route_dev(kh_table* t, const void* dev_recs, uint64_t n, int nranks, void* dev_words_out,
                 void* dev_counts_out);
/* kh_collect_starts_dev + kh_route_dev in one streaming pass over the records (the start bits
 * come from the route's owner pass); successive calls append starts in call order. */
int kh_route_starts_dev(kh_table* t, const void* dev_recs, uint64_t n, int nranks, void* dev_words_out,
                        void* dev_counts_out);
/* kh_route_starts_dev in ONE pass over the records (no owner pre-pass): owner q's words land in
 * the window dev_words_out + q * win words-per-k-mer (win >= n, < 2^32: a window holds every record,
 * whatever the skew), dev_counts_out[q] = their count, [nranks] = n. The all-to-all sends each
 * window's first counts[q] words. Records of <= 15 bytes (k <= 52; KH_ERR_ARG otherwise: use
 * kh_route_starts_dev). Replaces the same hash_map.hpp:28-30,64-77 routing. */
int kh_route_starts_win_dev(kh_table* t, const void* dev_recs, uint64_t n, int nranks, void* dev_words_out,
                            uint64_t win, void* dev_counts_out);
/* dev_words: internal words as kh_route_dev / kh_route_starts_dev emit them (they carry the
 * k-mer's placement bits: minimizer window, order bits). */
int kh_insert_words_dev(kh_table* t, const void* dev_words, uint64_t m);
/* Staged insert of routed words (one call per received all-to-all chunk, hash_map.hpp:55-80's
 * insert_all split so that partitioning overlaps the exchange): stage partitions m words toward
 * one build of at most total_hint words (the first stage after a clear/finish starts it; keep
 * total_hint the same for every stage of one build); finish builds the table from them. Small
 * builds insert each stage directly. dev_words may be reused once the next stage/finish call
 * has been issued on the table's stream. */
int kh_insert_words_stage_dev(kh_table* t, const void* dev_words, uint64_t m, uint64_t total_hint);
int kh_insert_words_finish(kh_table* t);
/* Splitter k-mers routed to each owner since the last clear (async copy of nranks uint64 into
 * device memory): a shard's splitter count is the sum of its column over the senders, learnt with
 * the route counts instead of by a device read. */
int kh_route_splitters_dev(kh_table* t, void* dev_out, int nranks);
/* Async copy of {start k-mers collected, splitter k-mers collected} (2 uint64) into device memory,
 * for hosts that read them together with their own counts (one host round trip). */
int kh_counters_dev(kh_table* t, void* dev_out);
/* The same two counts read on the host (blocking). After kh_insert_dev they come from the copy
 * made beside the region build, so the read waits for the start / splitter compaction, not for the
 * build (the one-rank sharded step reads them without idling the device). */
int kh_counters(kh_table* t, uint64_t* out2);
/* Batched find across shards: DistributedHashMap::find (hash_map.hpp:83-107) for a whole batch of
 * keys from any rank, instead of one blocking RPC per key (hash_map.hpp:94-100). The asker groups
 * its keys by owner, the caller exchanges them, every owner answers the keys it received with 2
 * bytes each, the caller sends the answers back (the same exchange with the splits swapped) and the
 * asker puts them in its own key order:
 *   route(keys) -> exchange of counts, then of keys_out (PACKED B per key)
 *   answer(received keys) -> exchange back (2 B per key, not a record: the asker has the key)
 *   gather(keys, index, answers as they came back) -> records + found flags
 * All three are async on the table's stream and change neither the table, the start list nor a
 * walk. n = 0 / m = 0: KH_OK, nothing is done or written. n >= 2^32, nranks outside [1, 64] or a
 * null buffer: KH_ERR_ARG. A staged insert left open (kh_insert_words_stage_dev without finish):
 * KH_ERR_STATE. Key, record, answer and flag buffers may have any alignment.
 *
 * kh_find_route_dev: n pkmer_t keys (contiguous) -> dev_keys_out: the same n keys, owner 0's first,
 * then owner 1's, ... (order inside a group unspecified); dev_index_out: uint32[n], the position in
 * dev_keys of grouped key j; dev_counts_out: uint64[nranks + 1], the keys per owner, then n. The
 * owner of a key is kh_key_owner(t, key, nranks). */
int kh_find_route_dev(kh_table* t, const void* dev_keys, uint64_t n, int nranks, void* dev_keys_out,
                      void* dev_index_out, void* dev_counts_out);
/* m keys -> dev_ext_out: 2 bytes per key, the {backward, forward} extension chars of the key's
 * record in this table, {0, 0} when the table does not hold the key (an empty or cleared table
 * answers {0, 0} for every key). */
int kh_find_answer_dev(kh_table* t, const void* dev_keys, uint64_t m, void* dev_ext_out);
/* dev_keys / dev_index: as given to / written by kh_find_route_dev; dev_ext_grouped: the answer of
 * grouped key j at bytes 2j, 2j + 1 -> dev_recs_out: n kmer_pair records, dev_found_out: n bytes 0/1,
 * in the order of dev_keys, byte for byte what kh_find_dev writes on one table holding every k-mer
 * (an absent key: a zeroed record and 0). */
int kh_find_gather_dev(kh_table* t, const void* dev_keys, uint64_t n, const void* dev_index,
                       const void* dev_ext_grouped, void* dev_recs_out, void* dev_found_out);
/* Migrating-walker rounds. The table is sharded by a hash of each k-mer's minimizer, so
 * consecutive k-mers of a contig mostly share an owner; a walker walks the local shard until its
 * next k-mer is owned elsewhere and is then sent there. Nothing below reads the device on the host:
 *   begin(n_starts, n_splitters, total_walkers)
 *   loop { round(in slots -> out slots, live) -> all-to-all of the fixed-size slot buffers }
 *          (every few rounds the host reads the global sum of live[0]; rounds past the end find
 *           empty slots and do nothing)
 *   -> text_dev (text records grouped by origin rank, counts[P+1]) -> exchange -> end_dev(records)
 * A round's exchange buffer is nranks slots of KH_SLOT_WORDS(cap) int64 words: [count, 0, up to
 * cap messages of KH_MSG_WORDS]; slot q goes to rank q and the received buffer (slot q = what rank q
 * sent) is the next round's input. Messages past cap are held back on the sender and go out in a
 * later round. live: 2 uint64 on the device = [messages in flight after the round (sent + held
 * back), largest per-destination count]. The first round takes in_slots = NULL (the walkers of
 * begin). n_starts / n_splitters: this rank's counts (kh_counters_dev, or the column sums of
 * kh_route_splitters_dev); total_walkers: the sum of n_starts + n_splitters over all ranks.
 * Routing by minimizer must also be used for the inserts: this sharding and the routes agree. */
#define KH_MSG_WORDS 5
#define KH_TEXT_REC_WORDS 2
#define KH_SLOT_WORDS(cap) (2 + (cap) * KH_MSG_WORDS)
int kh_mwalk_begin(kh_table* t, int nranks, int rank, uint64_t total_kmers, uint64_t n_starts, uint64_t n_splitters,
                   uint64_t total_walkers, uint64_t* n_walkers);
int kh_mwalk_round_dev(kh_table* t, const void* dev_in_slots, uint64_t in_cap, void* dev_out_slots, uint64_t out_cap,
                       void* dev_live);
int kh_mwalk_text_bound(kh_table* t, uint64_t* n_records); /* text_dev writes at most this many */
int kh_mwalk_text_dev(kh_table* t, void* dev_out, void* dev_counts_out);
int kh_mwalk_end_dev(kh_table* t, const void* dev_recs, uint64_t n);
/* Splitter segments of the migrating walk (kh_mseg.hip; on when the shard collects splitters,
 * KH_SPLIT_BITS=0 turns them off). kh_mwalk_begin then also seeds a walker at every splitter
 * k-mer this shard owns (n_walkers includes them) and walkers stop before splitters. When
 * kh_mwalk_segments reports > 0 on any rank, after the text records have come home the end of the
 * walk is, instead of kh_mwalk_end_dev:
 *   kh_mwalk_link_dev(recs)  -> KH_LINK_WORDS-word links grouped by owner -> exchange
 *   kh_mwalk_pred_dev(links, preds, stride) -> this rank's table of {predecessor id, length} for
 *        its splitter segments (stride >= every rank's kh_mwalk_segments entries; the tail is "none")
 *   all-gather of the tables (rank q's at q * stride) -> kh_mwalk_resolve_dev(all, stride): every
 *        segment's contig and offset by pointer jumping on the device (no exchange per step)
 *   kh_mwalk_retag_dev(recs) -> KH_SEG_REC_WORDS-word records grouped by contig origin -> exchange
 *   kh_mwalk_end_seg_dev(recs, received segment records)   (this rank's test_<rank>.dat in HBM)
 * Buffers: links <= n_walkers records, preds 2 * stride words, retag output <= n + segments. */
#define KH_LINK_WORDS 4
#define KH_PRED_WORDS 2
#define KH_SEG_REC_WORDS 3
int kh_mwalk_segments(kh_table* t, uint64_t* n_splitter_segments);
/* Malformed input whose start walks overlap (a k-mer reached by two walks): a segmented walk
 * cannot give one splitter segment two contigs, and an unsegmented one may outgrow its text store.
 * kh_mwalk_flags_dev writes 2 uint64 to device memory (async): [overlap / overflow reports of this
 * walk, text records the store needed]; hosts exchange the first with a count exchange they make
 * anyway, and when any rank reports one, every rank calls kh_mwalk_redo (ends this walk, clears the
 * report) and walks again from kh_mwalk_begin: without splitter segments (each start walked to its
 * end, as kmer_hash.cpp:41-53 does) and with a store of at least store_records records. */
int kh_mwalk_flags_dev(kh_table* t, void* dev_out2);
int kh_mwalk_redo(kh_table* t, uint64_t store_records);
/* Short walk first (round 6): splitter segments only pay for long contigs. Called before
 * kh_mwalk_begin with every rank's k-mer and start counts: where the mean contig is shorter than
 * the splitter spacing, *armed = 1 and the next walk runs without splitter segments; a walker that
 * passes 4 spacings ends and adds 2^40 to the first word kh_mwalk_flags_dev reports. When any rank
 * reports it, every rank calls kh_mwalk_abandon and walks again from kh_mwalk_begin, segmented
 * (hosts keep walking segmented on the same input). */
int kh_mwalk_short(kh_table* t, uint64_t total_kmers, uint64_t total_starts, int* armed);
int kh_mwalk_abandon(kh_table* t);
int kh_mwalk_link_dev(kh_table* t, const void* dev_recs, uint64_t n, void* dev_links_out, void* dev_counts_out);
int kh_mwalk_pred_dev(kh_table* t, const void* dev_links, uint64_t m, void* dev_preds_out, uint64_t stride);
int kh_mwalk_resolve_dev(kh_table* t, const void* dev_all_preds, uint64_t stride);
int kh_mwalk_retag_dev(kh_table* t, const void* dev_recs, uint64_t n, void* dev_seg_recs_out, void* dev_counts_out);
int kh_mwalk_end_seg_dev(kh_table* t, const void* dev_recs, uint64_t n, const void* dev_seg_recs, uint64_t m);

/* ---- device memory helpers (for hosts without an allocator of their own) --------------------*/
int kh_dev_malloc(void** p, uint64_t bytes, int device);
int kh_dev_free(void* p);
int kh_memcpy_htod(void* dst, const void* src, uint64_t bytes);
int kh_memcpy_dtoh(void* dst, const void* src, uint64_t bytes);

/* ---- host codec helpers --------------------------------------------------------------------*/
/* read_kmers.hpp:62-76: fixed-width "KMER BF\n" lines (k+4 bytes) -> kmer_pair records. */
int kh_pack_text(int k, const char* text, uint64_t len, uint8_t* recs_out, uint64_t* n_out);
/* packing.hpp:77-107 */
int kh_pack_kmer(int k, const char* kmer, uint8_t* packed_out);
int kh_unpack_kmer(int k, const uint8_t* packed, char* kmer_out);
/* pkmer_t.hpp:31-37 djb2 (API parity; the table places keys with its own mixer) */
uint64_t kh_djb2(int k, const uint8_t* packed);
/* kmer_t.hpp:51-53 next_kmer of a record, as packed bytes */
int kh_next_kmer(int k, const uint8_t* rec, uint8_t* packed_out);

/* ---- synthetic dataset generator ------------------------------------------
 * n k-mers cut from independent uniform-random contigs of len_min..len_max k-mers (plus
 * single_permille / 1000 single-k-mer contigs), every k-mer unique (contigs containing a repeated
 * k-mer are re-drawn), records shuffled by a seeded bijection. Deterministic in all arguments
 * except `threads`. */
typedef struct kh_gen kh_gen;
int kh_gen_create(kh_gen** out, int k, uint64_t n, uint32_t len_min, uint32_t len_max,
                  uint32_t single_permille, uint64_t seed, int shuffle, int threads);
/* C5-style skewed set (BASELINE configs[4]): the first n_long contigs have long_len
 * k-mers, the rest U[len_min, len_max]; front_starts != 0 puts every start k-mer ahead of every
 * other record (so the block split hands all walkers to the first ranks). */
int kh_gen_create_skewed(kh_gen** out, int k, uint64_t n, uint32_t len_min, uint32_t len_max,
                         uint32_t single_permille, uint64_t seed, int shuffle, int threads, uint32_t n_long,
                         uint32_t long_len, int front_starts);
/* Hot-minimizer / hot-bucket variant (BASELINE configs[4] "skewed/hot-bucket"): additionally,
 * hot_permille / 1000 of the contigs (picked by a seeded hash) carry one of n_motifs (1..64) shared
 * M-mers (M = the table's minimizer length: 16 at k >= 31, 12 at k = 19) every K - M + 1 bases, so
 * every k-mer of a hot contig contains one and the motifs (chosen for the smallest minimizer order)
 * are their minimizers: all k-mers of motif h share one minimizer window, hence one placement
 * region and one shard owner before the table's hot-region remap. Uniqueness and the ground
 * truth hold as for kh_gen_create. hot_permille = 0 is kh_gen_create_skewed. */
int kh_gen_create_hot(kh_gen** out, int k, uint64_t n, uint32_t len_min, uint32_t len_max,
                      uint32_t single_permille, uint64_t seed, int shuffle, int threads, uint32_t n_long,
                      uint32_t long_len, int front_starts, uint32_t hot_permille, uint32_t n_motifs);
/* flags: KH_GEN_HOT_FLANK plants a fixed per-motif M-mer right before every motif occurrence (one
 * flank + motif pattern per K bases, k >= 2M + 8): the k-mers holding the whole pattern (20 of 51
 * phases at k=51) share the minimizer and its neighbour window, the worst case of the table's hot
 * remap (a long exact repeat shared by a family). */
#define KH_GEN_HOT_FLANK 1u
int kh_gen_create_hot_ex(kh_gen** out, int k, uint64_t n, uint32_t len_min, uint32_t len_max,
                         uint32_t single_permille, uint64_t seed, int shuffle, int threads, uint32_t n_long,
                         uint32_t long_len, int front_starts, uint32_t hot_permille, uint32_t n_motifs,
                         uint32_t flags);
int kh_gen_destroy(kh_gen* g);
uint64_t kh_gen_num_contigs(const kh_gen* g);
/* records at output positions [pos_begin, pos_end) in kmer_pair layout (block split of
 * read_kmers.hpp:55-58 = positions [r*ceil(n/P), ...)) */
int kh_gen_records(const kh_gen* g, uint64_t pos_begin, uint64_t pos_end, uint8_t* out);
/* the same records produced by the GPU into device memory (R bytes each, contiguous) on a HIP
 * stream (NULL = default stream): a 200M-record C3 set in milliseconds instead of seconds of host
 * work and a PCIe upload. Async; the generator must outlive the work. */
int kh_gen_records_dev(kh_gen* g, uint64_t pos_begin, uint64_t pos_end, void* dev_out, void* hip_stream);
/* ground-truth contig text of the contigs whose start k-mer lies in [pos_begin, pos_end), in
 * start-node order (= expected test_<rank>.dat bytes); bytes_out gets the size. out may be NULL
 * to query the size. */
int kh_gen_truth(const kh_gen* g, uint64_t pos_begin, uint64_t pos_end, char* out, uint64_t cap,
                 uint64_t* bytes_out);

#ifdef __cplusplus
}
#endif
#endif /* KMER_HASH_AMD_H */
