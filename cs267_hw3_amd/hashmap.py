"""Host-side mirror of the reference's k-mer table API over the C ABI.

Reference surface (fractalclockwork/CS267_HW3) -> here:
  kmer_pair / pkmer_t byte layout (kmer_t.hpp:6-8, pkmer_t.hpp:6)  -> numpy uint8 rows [n, R] / [n, P]
  read_kmers(fname, nprocs, rank)        (read_kmers.hpp:54-79)    -> read_kmers()
  DistributedHashMap(size, rank, world)  (hash_map.hpp:50-52)      -> KmerHashTable(k, n_kmers)
  insert_all(kmers)                      (hash_map.hpp:55-80)      -> KmerHashTable.insert_all()
  find(key, result) -> bool              (hash_map.hpp:83-107)     -> KmerHashTable.find()
  initialize_kmers + assemble_contigs    (kmer_hash.cpp:21-55)     -> insert_all() + assemble()
  extract_contig / test_<rank>.dat       (read_kmers.hpp:81-92)    -> contigs_text()
Errors mirror the reference: a walk that misses a k-mer raises (kmer_hash.cpp:47-49).
"""
import ctypes
import os

import numpy as np

from . import _lib
from ._lib import KhStats, KmerHashError, check


def packed_size(k):
    return (k + 3) // 4


def record_size(k):
    return packed_size(k) + 2


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def pack_text(k, text):
    """Fixed-width "KMER BF\\n" lines -> kmer_pair records, uint8 [n, R] (read_kmers.hpp:62-76)."""
    L = _lib.lib()
    buf = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else text
    n = ctypes.c_uint64(0)
    check(L.kh_pack_text(k, _ptr(buf), buf.size, None, ctypes.byref(n)))
    recs = np.empty((n.value, record_size(k)), dtype=np.uint8)
    check(L.kh_pack_text(k, _ptr(buf), buf.size, _ptr(recs), ctypes.byref(n)))
    return recs


def kmer_size(fname):
    """read_kmers.hpp:14-25: length of the first whitespace-delimited token."""
    with open(fname, "rb") as f:
        return len(f.readline().split()[0])


def read_kmer_lines(fname, k, nprocs=1, rank=0):
    """read_kmers.hpp:54-68 block split: the raw text of lines [r*ceil(n/P), ...) of rank r."""
    line = k + 4
    size = os.path.getsize(fname)
    n = size // line
    split = (n + nprocs - 1) // nprocs
    start = min(split * rank, n)
    cnt = min(split, n - start)
    with open(fname, "rb") as f:
        f.seek(start * line)
        return f.read(cnt * line)


def read_kmers(fname, k, nprocs=1, rank=0):
    """read_kmers.hpp:54-79: rank r's block of the file as kmer_pair records (host codec)."""
    return pack_text(k, read_kmer_lines(fname, k, nprocs, rank))


def pack_kmer(k, kmer):
    out = np.zeros(packed_size(k), dtype=np.uint8)
    check(_lib.lib().kh_pack_kmer(k, kmer.encode() if isinstance(kmer, str) else kmer, _ptr(out)))
    return out


def unpack_kmer(k, packed):
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    out = np.zeros(k, dtype=np.uint8)
    check(_lib.lib().kh_unpack_kmer(k, _ptr(packed), _ptr(out)))
    return out.tobytes().decode()


def djb2(k, packed):
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    return int(_lib.lib().kh_djb2(k, _ptr(packed)))


def next_kmer(k, rec):
    rec = np.ascontiguousarray(rec, dtype=np.uint8)
    out = np.zeros(packed_size(k), dtype=np.uint8)
    check(_lib.lib().kh_next_kmer(k, _ptr(rec), _ptr(out)))
    return out


def read_offsets(text):
    """The reads of a text, one per line -> uint64 [n + 1] offsets (read r = bytes off[r] .. off[r+1]-1):
    every '\\n'-terminated line is a read, its '\\n' included (a '\\r' before it too); a non-empty tail
    without '\\n' is a last read. Empty text gives [0]."""
    buf = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else \
        np.ascontiguousarray(text, dtype=np.uint8).ravel()
    ends = np.flatnonzero(buf == 10).astype(np.uint64) + np.uint64(1)
    off = np.concatenate([np.zeros(1, np.uint64), ends])
    if len(buf) and (not len(ends) or int(ends[-1]) != len(buf)):
        off = np.concatenate([off, np.array([len(buf)], np.uint64)])
    return off


_COMPLEMENT = np.arange(256, dtype=np.uint8)
_COMPLEMENT[list(b"ACGT")] = list(b"TGCA")


def reverse_complement(text):
    """The other strand of a text (bytes or a numpy uint8 array) -> bytes: the byte order reversed and
    A<->T, C<->G swapped; every other byte (lower case, N, '\\n', ...) is kept as it is, so lines stay
    lines, in reverse order."""
    buf = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else \
        np.ascontiguousarray(text, dtype=np.uint8).ravel()
    return _COMPLEMENT[buf[::-1]].tobytes()


def device_count():
    n = ctypes.c_int(0)
    rc = _lib.lib().kh_device_count(ctypes.byref(n))
    return n.value if rc == 0 else 0


class KmerHashTable:
    """GPU-resident open-addressing k-mer table + contig walker (one per GPU / rank)."""

    def __init__(self, k, n_kmers, load_factor=0.5, device=0):
        self.k = k
        self.P = packed_size(k)
        self.R = record_size(k)
        self._device = device
        self._L = _lib.lib()
        h = ctypes.c_void_p()
        check(self._L.kh_create(ctypes.byref(h), k, int(n_kmers), float(load_factor), device))
        self._h = h

    # -- lifetime ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._L.kh_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def capacity(self):
        return int(self._L.kh_capacity(self._h))

    def clear(self):
        check(self._L.kh_clear(self._h))

    def sync(self):
        check(self._L.kh_sync(self._h))

    def set_stream(self, stream_ptr):
        check(self._L.kh_set_stream(self._h, ctypes.c_void_p(stream_ptr) if stream_ptr else None))

    def stats(self):
        s = KhStats()
        check(self._L.kh_get_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    # -- insert / find ------------------------------------------------------------------------
    def _recs(self, recs):
        recs = np.ascontiguousarray(recs, dtype=np.uint8)
        if recs.size % self.R:
            raise ValueError(f"record buffer of {recs.size} bytes is not a multiple of {self.R}")
        return recs, recs.size // self.R

    def insert_all(self, recs):
        """Synchronous bulk insert of host records; raises on duplicate/full/bad base."""
        recs, n = self._recs(recs)
        check(self._L.kh_insert(self._h, _ptr(recs), n))

    insert = insert_all

    def pack_text_dev(self, text_ptr, nbytes, recs_ptr=None):
        """read_kmers.hpp:62-76 on the GPU (device text -> device records at recs_ptr, 16-B
        aligned); returns the record count. Bad bases surface at the next sync()."""
        n = ctypes.c_uint64(0)
        check(self._L.kh_pack_text_dev(self._h, ctypes.c_void_p(text_ptr), nbytes,
                                       ctypes.c_void_p(recs_ptr) if recs_ptr else None, ctypes.byref(n)))
        return n.value

    def insert_dev(self, dev_ptr, n):
        """Asynchronous insert of n records already in device memory (16-B aligned)."""
        check(self._L.kh_insert_dev(self._h, ctypes.c_void_p(dev_ptr), int(n)))

    def find(self, keys):
        """Batched find of pkmer_t keys -> (records [n, R], found bool[n])."""
        keys = np.ascontiguousarray(keys, dtype=np.uint8)
        n = keys.size // self.P
        out = np.zeros((n, self.R), dtype=np.uint8)
        found = np.zeros(n, dtype=np.uint8)
        if n:
            check(self._L.kh_find(self._h, _ptr(keys), n, _ptr(out), _ptr(found)))
        return out, found.astype(bool)

    def find_text(self, text):
        """Every k-mer of a text (bytes or a numpy uint8 array: reads, contig lines, FASTA) looked up:
        -> (ext uint8 [len, 2], windows, found). ext[i] = the {backward, forward} chars of the k-mer
        at bytes i .. i+k-1, {0, 0} when the table does not hold it, {0xFF, 0xFF} (KH_TEXT_NONE) when
        those bytes are not all in the text and one of A C G T."""
        buf = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else \
            np.ascontiguousarray(text, dtype=np.uint8).ravel()
        ext = np.empty((buf.size, 2), dtype=np.uint8)
        counts = np.zeros(2, dtype=np.uint64)
        check(self._L.kh_find_text(self._h, _ptr(buf) if buf.size else None, buf.size, _ptr(ext), _ptr(counts)))
        return ext, int(counts[0]), int(counts[1])

    def find_text_dev(self, text_ptr, nbytes, ext_ptr, counts_ptr):
        """Asynchronous device form (kh_find_text_dev): nbytes of text at text_ptr -> 2 * nbytes answer
        bytes at ext_ptr (0 / None: counts only) and 2 uint64 {windows, found} at counts_ptr (0 / None:
        answers only). nbytes = 0 writes nothing."""
        check(self._L.kh_find_text_dev(self._h, ctypes.c_void_p(text_ptr) if text_ptr else None, int(nbytes),
                                       ctypes.c_void_p(ext_ptr) if ext_ptr else None,
                                       ctypes.c_void_p(counts_ptr) if counts_ptr else None))

    # -- locate: the position index (kh_locate_*) ----------------------------------------------
    def locate_build(self):
        """Index every k-mer of the table's own contig text (after assemble): its position is its byte
        offset in contigs_text(), the smallest one when it stands on several lines."""
        check(self._L.kh_locate_build(self._h))

    def locate_reset(self):
        """An empty index (every k-mer without a position), ready for locate_set_dev."""
        check(self._L.kh_locate_reset(self._h))

    def locate_drop(self):
        """Free the index's device memory (capacity * 8 bytes)."""
        check(self._L.kh_locate_drop(self._h))

    def locate(self, keys):
        """pkmer_t keys -> uint64 [n]: each key's position, LOC_NONE when the table does not hold it or
        it stands on no contig."""
        keys = np.ascontiguousarray(keys, dtype=np.uint8)
        n = keys.size // self.P
        pos = np.empty(n, dtype=np.uint64)
        check(self._L.kh_locate(self._h, _ptr(keys) if n else None, n, _ptr(pos)))
        return pos

    def locate_text(self, text, rc=False):
        """Every k-mer of a text (bytes or a numpy uint8 array) -> (pos uint64 [len], windows, located):
        pos[i] = the position of the k-mer at bytes i .. i+k-1, LOC_NONE where there is no window, the
        k-mer is absent or it has no position. rc=True: the position of the window's reverse
        complement instead (kh_locate_text_rc): the k bases in reverse order, each complemented."""
        buf = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else \
            np.ascontiguousarray(text, dtype=np.uint8).ravel()
        pos = np.empty(buf.size, dtype=np.uint64)
        counts = np.zeros(2, dtype=np.uint64)
        call = self._L.kh_locate_text_rc if rc else self._L.kh_locate_text
        check(call(self._h, _ptr(buf) if buf.size else None, buf.size, _ptr(pos), _ptr(counts)))
        return pos, int(counts[0]), int(counts[1])

    def locate_lines(self, pos):
        """Positions in the table's contig text (uint64) -> (line uint64 [n], col uint64 [n]) over the
        last assemble's line starts; LOC_NONE gives LOC_NONE for both."""
        pos = np.ascontiguousarray(pos, dtype=np.uint64).ravel()
        n = pos.size
        line, col = np.empty(n, dtype=np.uint64), np.empty(n, dtype=np.uint64)
        L = self._L
        d = ctypes.c_void_p()
        check(L.kh_dev_malloc(ctypes.byref(d), 24 * max(n, 1), self._device))
        try:
            p = lambda j: ctypes.c_void_p(d.value + 8 * n * j)  # noqa: E731
            check(L.kh_sync(self._h))
            check(L.kh_memcpy_htod(p(0), _ptr(pos), 8 * n))
            check(L.kh_locate_lines_dev(self._h, p(0), n, p(1), p(2)))
            check(L.kh_sync(self._h))
            check(L.kh_memcpy_dtoh(_ptr(line), p(1), 8 * n))
            check(L.kh_memcpy_dtoh(_ptr(col), p(2), 8 * n))
        finally:
            L.kh_dev_free(d)
        return line, col

    def locate_dev(self, keys_ptr, n, pos_ptr):
        """Asynchronous device form (kh_locate_dev): n keys at keys_ptr -> n uint64 at pos_ptr (8-byte
        aligned). n = 0 writes nothing."""
        check(self._L.kh_locate_dev(self._h, ctypes.c_void_p(keys_ptr) if keys_ptr else None, int(n),
                                    ctypes.c_void_p(pos_ptr) if pos_ptr else None))

    def locate_text_dev(self, text_ptr, nbytes, pos_ptr, counts_ptr):
        """Asynchronous device form (kh_locate_text_dev): nbytes of text at text_ptr -> nbytes uint64 at
        pos_ptr (0 / None: counts only) and 2 uint64 {windows, located} at counts_ptr (0 / None:
        positions only), both 8-byte aligned. nbytes = 0 writes nothing."""
        check(self._L.kh_locate_text_dev(self._h, ctypes.c_void_p(text_ptr) if text_ptr else None, int(nbytes),
                                         ctypes.c_void_p(pos_ptr) if pos_ptr else None,
                                         ctypes.c_void_p(counts_ptr) if counts_ptr else None))

    def locate_text_rc_dev(self, text_ptr, nbytes, pos_ptr, counts_ptr):
        """Asynchronous device form (kh_locate_text_rc_dev): locate_text_dev for the reverse complement
        of every window."""
        check(self._L.kh_locate_text_rc_dev(self._h, ctypes.c_void_p(text_ptr) if text_ptr else None, int(nbytes),
                                            ctypes.c_void_p(pos_ptr) if pos_ptr else None,
                                            ctypes.c_void_p(counts_ptr) if counts_ptr else None))

    def locate_set_dev(self, keys_ptr, n, values_ptr, missing_ptr=None):
        """Asynchronous (kh_locate_set_dev): n keys at keys_ptr each take the uint64 at values_ptr unless
        they hold a smaller one; missing_ptr (0 / None: not counted): 1 uint64, the keys the table lacks."""
        check(self._L.kh_locate_set_dev(self._h, ctypes.c_void_p(keys_ptr) if keys_ptr else None, int(n),
                                        ctypes.c_void_p(values_ptr) if values_ptr else None,
                                        ctypes.c_void_p(missing_ptr) if missing_ptr else None))

    # -- seed: the longest exact run of each read on the contigs (kh_seed_*) ---------------------
    def seed_reads(self, text, read_off=None, strands="+"):
        """A batch of reads (text: bytes or a numpy uint8 array; read_off: uint64 [n + 1] offsets into
        it, None = read_offsets(text), one read per line) -> uint64 [n, 4]: per read {start of its
        longest run of windows that locate_text places one after the other, relative to the read's
        first byte; the position of the run's first window; the run's length in windows; the read's
        located windows}, {LOC_NONE, LOC_NONE, 0, 0} where no window is located. Matched bases =
        run + k - 1. After locate_build.

        strands="both" (kh_seed_strand_text) -> uint64 [n, 6]: {start, value, run, strand, located
        forward, located reverse}: the longer of the read's longest forward run and its longest run as
        a reverse complement (positions going down by one), the forward one when they are equal;
        strand 0 = forward, 1 = reverse; value = the lowest contig position of the run on either
        strand, so the matched contig bytes are [value, value + run + k - 1);
        {LOC_NONE, LOC_NONE, 0, 0, 0, 0} where no window is located on either strand."""
        if strands not in ("+", "both"):
            raise ValueError('strands is "+" (the contigs\' strand) or "both"')
        buf = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else \
            np.ascontiguousarray(text, dtype=np.uint8).ravel()
        off = read_offsets(buf) if read_off is None else np.ascontiguousarray(read_off, dtype=np.uint64).ravel()
        if off.size == 0:
            raise ValueError("read_off holds n + 1 offsets: at least one")
        n = off.size - 1
        both = strands == "both"
        seeds = np.empty((n, _lib.SEED_STRAND_WORDS if both else _lib.SEED_WORDS), dtype=np.uint64)
        call = self._L.kh_seed_strand_text if both else self._L.kh_seed_text
        check(call(self._h, _ptr(buf) if buf.size else None, buf.size, _ptr(off), n, _ptr(seeds) if n else None))
        return seeds

    def seed_strand_text_dev(self, text_ptr, nbytes, read_off_ptr, n_reads, pos_ptr, seeds_ptr):
        """Asynchronous device form (kh_seed_strand_text_dev): as seed_text_dev with 6 * n_reads uint64
        at seeds_ptr and 2 * nbytes uint64 of scratch at pos_ptr: the forward positions, then the
        reverse-complement ones, afterwards."""
        check(self._L.kh_seed_strand_text_dev(self._h, ctypes.c_void_p(text_ptr) if text_ptr else None, int(nbytes),
                                              ctypes.c_void_p(read_off_ptr) if read_off_ptr else None, int(n_reads),
                                              ctypes.c_void_p(pos_ptr) if pos_ptr else None,
                                              ctypes.c_void_p(seeds_ptr) if seeds_ptr else None))

    def seed_strand_runs_dev(self, fwd_ptr, rc_ptr, n, read_off_ptr, n_reads, seeds_ptr):
        """Asynchronous (kh_seed_strand_runs_dev): the run search alone over two arrays of n uint64
        (forward positions at fwd_ptr, reverse-complement ones at rc_ptr; no index needed)."""
        check(self._L.kh_seed_strand_runs_dev(self._h, ctypes.c_void_p(fwd_ptr) if fwd_ptr else None,
                                              ctypes.c_void_p(rc_ptr) if rc_ptr else None, int(n),
                                              ctypes.c_void_p(read_off_ptr) if read_off_ptr else None, int(n_reads),
                                              ctypes.c_void_p(seeds_ptr) if seeds_ptr else None))

    def seed_text_dev(self, text_ptr, nbytes, read_off_ptr, n_reads, pos_ptr, seeds_ptr):
        """Asynchronous device form (kh_seed_text_dev): nbytes of text at text_ptr and n_reads + 1 uint64
        offsets at read_off_ptr -> 4 * n_reads uint64 at seeds_ptr; pos_ptr: nbytes uint64 of scratch,
        the positions afterwards (all 8-byte aligned but the text). n_reads = 0 writes nothing."""
        check(self._L.kh_seed_text_dev(self._h, ctypes.c_void_p(text_ptr) if text_ptr else None, int(nbytes),
                                       ctypes.c_void_p(read_off_ptr) if read_off_ptr else None, int(n_reads),
                                       ctypes.c_void_p(pos_ptr) if pos_ptr else None,
                                       ctypes.c_void_p(seeds_ptr) if seeds_ptr else None))

    def seed_runs_dev(self, pos_ptr, n, read_off_ptr, n_reads, seeds_ptr):
        """Asynchronous (kh_seed_runs_dev): the run search alone over n uint64 positions at pos_ptr (any
        values, LOC_NONE = not located; no index needed)."""
        check(self._L.kh_seed_runs_dev(self._h, ctypes.c_void_p(pos_ptr) if pos_ptr else None, int(n),
                                       ctypes.c_void_p(read_off_ptr) if read_off_ptr else None, int(n_reads),
                                       ctypes.c_void_p(seeds_ptr) if seeds_ptr else None))

    def seed_coverage_dev(self, seeds_ptr, n_reads, reads_ptr, bases_ptr):
        """Asynchronous (kh_seed_coverage_dev): n_reads seeds at seeds_ptr add to the n_contigs uint64 at
        reads_ptr (reads per contig line) and bases_ptr (their matched bases); either may be 0 / None."""
        check(self._L.kh_seed_coverage_dev(self._h, ctypes.c_void_p(seeds_ptr) if seeds_ptr else None, int(n_reads),
                                           ctypes.c_void_p(reads_ptr) if reads_ptr else None,
                                           ctypes.c_void_p(bases_ptr) if bases_ptr else None))

    def seed_coverage(self, seeds):
        """Seeds uint64 [n, 4] (seed_reads) -> (reads uint64 [n_contigs], bases uint64 [n_contigs]) per
        line of contigs_text(), counted from zero: the reads whose seed lies on the line and the bases
        those seeds match. Seeds uint64 [n, 6] (seed_reads(strands="both")) are repacked to {start,
        value, run, located forward + located reverse} first: their value is the lowest position of
        the run on either strand."""
        seeds = np.asarray(seeds, dtype=np.uint64)
        if seeds.ndim == 2 and seeds.shape[1] == _lib.SEED_STRAND_WORDS:
            seeds = np.concatenate([seeds[:, :3], (seeds[:, 4] + seeds[:, 5])[:, None]], axis=1)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64).reshape(-1, _lib.SEED_WORDS)
        n = len(seeds)
        L = self._L
        d = ctypes.c_void_p()
        check(L.kh_seed_coverage_dev(self._h, None, 0, None, None))  # the state errors, whatever n is
        nc = self.stats()["n_contigs"]
        out = np.zeros((2, nc), dtype=np.uint64)
        if n == 0 or nc == 0:
            return out[0], out[1]
        sb = 8 * _lib.SEED_WORDS * n
        check(L.kh_dev_malloc(ctypes.byref(d), sb + 16 * nc, self._device))
        try:
            p = lambda o: ctypes.c_void_p(d.value + o)  # noqa: E731
            check(L.kh_sync(self._h))
            check(L.kh_memcpy_htod(p(0), _ptr(seeds), sb))
            check(L.kh_memcpy_htod(p(sb), _ptr(out), 16 * nc))
            check(L.kh_seed_coverage_dev(self._h, p(0), n, p(sb), p(sb + 8 * nc)))
            check(L.kh_sync(self._h))
            check(L.kh_memcpy_dtoh(_ptr(out), p(sb), 16 * nc))
        finally:
            L.kh_dev_free(d)
        return out[0], out[1]

    # -- assemble -------------------------------------------------------------------------
    def set_starts(self, recs):
        recs, n = self._recs(recs)
        check(self._L.kh_set_starts(self._h, _ptr(recs) if n else None, n))

    def assemble(self):
        nc, nb = ctypes.c_uint64(0), ctypes.c_uint64(0)
        check(self._L.kh_assemble(self._h, ctypes.byref(nc), ctypes.byref(nb)))
        return nc.value, nb.value

    def assemble_dev(self):
        check(self._L.kh_assemble_dev(self._h))

    def contigs_text(self):
        d, b = ctypes.c_void_p(), ctypes.c_uint64(0)
        check(self._L.kh_contigs_text_dev(self._h, ctypes.byref(d), ctypes.byref(b)))
        out = np.empty(b.value, dtype=np.uint8)
        if b.value:
            check(self._L.kh_contigs_text(self._h, _ptr(out), b.value))
        return out.tobytes()

    def contigs(self):
        return self.contigs_text().decode().splitlines()


class SyntheticKmers:
    """Seeded synthetic dataset (kh_gen_*): records at any position range + ground truth."""

    def __init__(self, k, n, len_min=8, len_max=200, single_permille=0, seed=1, shuffle=True,
                 threads=0, n_long=0, long_len=0, front_starts=False, hot_permille=0, n_motifs=0,
                 hot_flank=False):
        """n_long / long_len / front_starts: the C5 walker skew; hot_permille / n_motifs: the C5
        hot-bucket half (contigs sharing a few minimizer motifs, kh_gen_create_hot); hot_flank: a
        fixed flank before every motif too (the shared stretch is 2M bases: the remap's worst case)."""
        self.k, self.n = k, int(n)
        self.R = record_size(k)
        self._L = _lib.lib()
        h = ctypes.c_void_p()
        check(self._L.kh_gen_create_hot_ex(ctypes.byref(h), k, self.n, len_min, len_max,
                                           single_permille, seed, 1 if shuffle else 0, threads,
                                           n_long, long_len, 1 if front_starts else 0, hot_permille, n_motifs,
                                           1 if hot_flank else 0))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.kh_gen_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def num_contigs(self):
        return int(self._L.kh_gen_num_contigs(self._h))

    def block(self, nprocs=1, rank=0):
        """read_kmers.hpp:55-58 block split of the record array."""
        split = (self.n + nprocs - 1) // nprocs
        b = min(split * rank, self.n)
        return b, min(b + split, self.n)

    def records(self, begin=0, end=None, out=None):
        end = self.n if end is None else end
        if out is None:
            out = np.empty((end - begin, self.R), dtype=np.uint8)
        check(self._L.kh_gen_records(self._h, begin, end, _ptr(out)))
        return out

    def records_dev(self, begin=0, end=None, device=None, stream=None):
        """Records [begin, end) generated on the GPU into a uint8 torch tensor [m, R] (16-B
        aligned); stream: a torch stream (default: the current one)."""
        import torch
        end = self.n if end is None else end
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        with torch.cuda.device(dev):
            out = torch.empty(max(end - begin, 1) * self.R + 16, dtype=torch.uint8, device=dev)
            s = stream if stream is not None else torch.cuda.current_stream(dev)
            check(self._L.kh_gen_records_dev(self._h, begin, end, ctypes.c_void_p(out.data_ptr()),
                                             ctypes.c_void_p(s.cuda_stream)))
        return out[:(end - begin) * self.R].view(end - begin, self.R)

    def truth(self, begin=0, end=None):
        end = self.n if end is None else end
        nb = ctypes.c_uint64(0)
        check(self._L.kh_gen_truth(self._h, begin, end, None, 0, ctypes.byref(nb)))
        out = np.empty(nb.value, dtype=np.uint8)
        check(self._L.kh_gen_truth(self._h, begin, end, _ptr(out), nb.value, ctypes.byref(nb)))
        return out.tobytes()


__all__ = ["KmerHashTable", "SyntheticKmers", "KmerHashError", "pack_text", "read_kmers", "read_kmer_lines",
           "kmer_size", "pack_kmer", "unpack_kmer", "djb2", "next_kmer", "device_count",
           "packed_size", "record_size", "read_offsets"]
