"""Shared generators of edge-case inputs and reference helpers (test infrastructure; no GPU, no
product imports)."""
import numpy as np


class RecordDict:
    """key bytes -> record of a record array [n, R] (sorted keys + binary search)."""

    def __init__(self, k, recs):
        self.KP = (k + 3) // 4
        self.R = self.KP + 2
        keys = self._s(recs[:, :self.KP])
        order = np.argsort(keys, kind="stable")
        self.keys, self.recs = keys[order], np.ascontiguousarray(recs[order])
        assert len(np.unique(self.keys)) == len(self.keys)

    def _s(self, a):  # rows as fixed-width byte strings (compared like memcmp)
        return np.ascontiguousarray(a, dtype=np.uint8).view(f"S{self.KP}").ravel()

    def lookup(self, q):
        """-> (records [m, R] (zeroed where absent), found uint8 [m])"""
        q = np.ascontiguousarray(q, dtype=np.uint8).reshape(-1, self.KP)
        out = np.zeros((len(q), self.R), np.uint8)
        if not len(q):
            return out, np.zeros(0, np.uint8)
        v = self._s(q)
        i = np.minimum(np.searchsorted(self.keys, v), len(self.keys) - 1)
        hit = self.keys[i] == v
        out[hit] = self.recs[i[hit]]
        return out, hit.astype(np.uint8)


def merging_walks_text(k, L, seed, every=1):
    """Malformed input whose start walks overlap: one chain C_0..C_{L-1} plus, at every `every`-th
    position j, three extra start k-mers x + C_{j-1}[1:] (bwd 'F') whose next_kmer is C_j. Every
    start walks the shared tail again (kmer_hash.cpp:41-53 does not care), so the text is ~3L^2/2
    bases, far past the table-start bound n + (K+1)·starts that kh_assemble_dev sizes first.
    Returns the fixed-width text (read_kmers.hpp:54-79 lines)."""
    rng = np.random.default_rng(seed)
    B = "ACGT"
    seq = "".join(B[x] for x in rng.integers(0, 4, L + k - 1))
    lines = []
    for i in range(L):
        lines.append((seq[i:i + k], "F" if i == 0 else seq[i - 1], "F" if i == L - 1 else seq[i + k]))
    seen = {x[0] for x in lines}
    for j in range(1, L, every):
        for x in B:
            z = x + seq[j:j + k - 1]
            if x == seq[j - 1] or z in seen:
                continue
            seen.add(z)
            lines.append((z, "F", seq[j + k - 1]))
    order = rng.permutation(len(lines))
    return "".join(f"{lines[i][0]} {lines[i][1]}{lines[i][2]}\n" for i in order).encode()


def contigs_lines(k, contigs, rng, order="shuffled"):
    """The line writer of contigs_text and chain_case: the fixed-width text (read_kmers.hpp:54-79
    lines) of the given contig strings (no k-mer twice among them), bwd 'F' on each first k-mer, fwd
    'F' on each last, the lines shuffled with `rng`; order="first" / "last" then puts the start
    record of the longest contig before / after every other line. Returns (text, contigs in the order
    of their start records, which is the expected test_0.dat)."""
    assert order in ("shuffled", "first", "last")
    lines = []  # (k-mer, bwd, fwd, contig or -1 when the line is not a start record)
    for c, seq in enumerate(contigs):
        L = len(seq) - k + 1
        for i in range(L):
            lines.append((seq[i:i + k], "F" if i == 0 else seq[i - 1], "F" if i == L - 1 else seq[i + k],
                          c if i == 0 else -1))
    perm = [int(i) for i in rng.permutation(len(lines))]
    if order != "shuffled":
        longest = max(range(len(contigs)), key=lambda c: len(contigs[c]))
        at = next(i for i in perm if lines[i][3] == longest)
        perm.remove(at)
        perm.insert(0 if order == "first" else len(perm), at)
    text = "".join(f"{lines[i][0]} {lines[i][1]}{lines[i][2]}\n" for i in perm).encode()
    return text, [contigs[lines[i][3]] for i in perm if lines[i][3] >= 0]


def contigs_text(k, lens, seed, order="shuffled"):
    """Well-formed input of independent random contigs, contig i of lens[i] k-mers (lens[i] + k - 1
    bases): bwd 'F' on each first k-mer, fwd 'F' on each last. A contig that would repeat a k-mer
    (its own or an earlier contig's: likely at small k) is drawn again. The lines are shuffled;
    order="first" / "last" then puts the start record of the longest contig before / after every
    other line. Returns (text, contigs): the fixed-width text (read_kmers.hpp:54-79 lines) and the
    contig strings in the order of their start records, which is the expected test_0.dat."""
    rng = np.random.default_rng(seed)
    B = "ACGT"
    seen = set()
    contigs = []
    for L in lens:
        assert L >= 1
        while True:
            seq = "".join(B[x] for x in rng.integers(0, 4, L + k - 1))
            kmers = [seq[i:i + k] for i in range(L)]
            if len(set(kmers)) == L and seen.isdisjoint(kmers):
                break
        seen.update(kmers)
        contigs.append(seq)
    return contigs_lines(k, contigs, rng, order)


def contigs_truth(contigs):
    """test_0.dat of contigs_text's second result: one contig per line."""
    return "".join(c + "\n" for c in contigs).encode()


_BASE4 = str.maketrans("ACGT", "0123")


def split_hash(kmer):
    """kh_codec.hpp split_hash of a k-mer string (V = 2-bit bases, first base most significant)."""
    v = int(kmer.translate(_BASE4), 4)
    lo = v & ((1 << 62) - 1)
    return (((lo & 0xFFFFFFFF) ^ (lo >> 32)) * 0x9E3779B1) & 0xFFFFFFFF


def walk_splitter_indices(k, contig, bits):
    """Chain indices i >= 1 of the contig's k-mers that are walk splitters at `bits` (kh_codec.hpp
    split_test; a contig's first k-mer is a start and never collected as a splitter)."""
    if not bits:  # split_test: 0 = off
        return []
    return [i for i in range(1, len(contig) - k + 1) if split_hash(contig[i:i + k]) < (1 << (32 - bits))]


def count_walk_splitters(k, contigs, bits):
    """The splitter walkers of the single-GPU walk at `bits`: non-start k-mers passing split_test."""
    return sum(len(walk_splitter_indices(k, c, bits)) for c in contigs)


def lens_for_text_bytes(K, T, seed, long_tail=False):
    """Contig lengths (in k-mers) whose test_0.dat is exactly T bytes (a contig of L k-mers is a
    line of L + K bytes): contigs of 1-3 k-mers, then one that takes the bytes left; with long_tail
    that last contig has at least 300 k-mers (more than one 256-base chunk). None if T is not
    reachable."""
    tail_min = 300 if long_tail else 1
    if T < K + tail_min:
        return None
    rng = np.random.default_rng(seed)
    lens, left = [], T
    while True:
        L = int(rng.integers(1, 4))
        if left - (L + K) < K + tail_min:
            break
        lens.append(L)
        left -= L + K
    lens.append(left - K)
    assert sum(L + K for L in lens) == T and lens[-1] >= tail_min
    return lens


# ---- deferred splitter segments inside one or two work-queue reservations (k_walk_q) ------------
# Shape A: 30 contigs of U[2,8] k-mers plus one of 120; shape B: 90 plus one of 120. The walk's
# splitter density at these sizes is 1 in 2^4 k-mers (kh_capi.cpp size_table / kh_assemble_dev), a
# reservation of the walker queue is 64 walkers (launch_walk: batches = 1 for so few).
DEFERRED_BITS = 4
DEFERRED_SEEDS = (0, 1, 2)


def deferred_facts(k, contigs):
    """What decides the walk's path for these contigs, from the Python mirror alone."""
    ns = len(contigs)
    n = sum(len(c) - k + 1 for c in contigs)
    nsp = count_walk_splitters(k, contigs, DEFERRED_BITS)
    long = max(contigs, key=len)
    stops = [i for i in walk_splitter_indices(k, long, DEFERRED_BITS) if i >= (1 << DEFERRED_BITS)]
    return {"ns": ns, "n": n, "nsp": nsp, "n_all": ns + nsp, "stops": stops}


def deferred_ok(shape, f):
    """The preconditions under which the start walkers defer every splitter walker and the long
    contig then stops at a splitter: mean contig <= 2^4 k-mers (deferred mode), a splitter walker
    exists, the long contig's walker meets a splitter after >= 2^4 bases, and the reservation that
    crosses n_starts also reaches the end of the queue (A: the first, B: the second)."""
    ok = f["n"] // f["ns"] <= (1 << DEFERRED_BITS) and f["nsp"] >= 1 and len(f["stops"]) >= 1
    if shape == "A":
        return ok and f["n_all"] <= 64
    return ok and 64 < f["ns"] < 128 and f["n_all"] <= 128


def deferred_case(k, shape, order="shuffled"):
    """(text, contigs, facts) of shape A or B at the first seed of DEFERRED_SEEDS that satisfies
    deferred_ok; fails if none does. The contigs do not depend on `order`."""
    assert shape in ("A", "B")
    tried = []
    for s in DEFERRED_SEEDS:
        seed = (100 if shape == "A" else 200) + k + s
        rng = np.random.default_rng(seed)
        lens = [int(x) for x in rng.integers(2, 9, 30 if shape == "A" else 90)] + [120]
        text, contigs = contigs_text(k, lens, seed, order)
        f = deferred_facts(k, contigs)
        if deferred_ok(shape, f):
            return text, contigs, dict(f, seed=seed)
        tried.append(dict(f, seed=seed))
    raise AssertionError(f"no seed gives shape {shape}'s preconditions at k={k}: {tried}")


# ---- chains of an exact number of splitter segments (k_seg_chain / k_seg_jump / k_seg_fill, and the
# sharded k_res_pass) ------------------------------------------------------------------------------
CHAIN_SEEDS = (0, 1, 2, 3, 4, 5, 6, 7)


def chain_contig(k, bits, S, seed, tail, first=1, seen=()):
    """A random contig cut so that exactly S of its k-mers at chain index >= `first` are walk
    splitters at `bits` (every prefix of a contig is a contig, and its splitters are a prefix of the
    list). first = 1 counts every splitter (a contig's first k-mer is a start, never a splitter):
    the chain's splitter segments when every walker stops at every splitter; first = 2^bits counts
    those a deferring start walker stops at (k_walk_q: steps >= split_min). tail = "on": the
    contig's last k-mer is the S-th such splitter (a last segment of one k-mer); "after": exactly
    two k-mers follow it, neither a splitter. No k-mer twice, none from `seen`."""
    assert tail in ("on", "after") and S >= 1 and bits >= 1 and first >= 1
    rng = np.random.default_rng(seed)
    B = "ACGT"
    L0 = (S + 4) * (2 << bits) + first + 8  # about twice the k-mers S splitters take
    for _ in range(64):
        seq = "".join(B[x] for x in rng.integers(0, 4, L0 + k - 1))
        sp = [i for i in walk_splitter_indices(k, seq, bits) if i >= first]
        if len(sp) <= S:
            continue
        L = sp[S - 1] + (1 if tail == "on" else 3)
        if sp[S] < L:  # (tail "after": a further splitter among the two k-mers of the tail)
            continue
        kmers = [seq[i:i + k] for i in range(L)]
        if len(set(kmers)) == L and set(seen).isdisjoint(kmers):
            return seq[:L + k - 1]
    raise AssertionError(f"no contig of {S} splitters at k={k}, bits={bits}, seed={seed}")


def chain_facts(k, bits, longs, fillers):
    """What decides the segment passes' path for the contigs `longs` plus `fillers` contigs of one
    k-mer (no non-start k-mer: starts, no splitters), from the Python mirror alone:
    ns, n, nsp     starts, k-mers, walk splitters at `bits`;
    S, S_deferred  per long contig, the splitter segments of its chain when every walker stops at
                   every splitter, and when its start walker defers (splitters at index >= 2^bits);
    deferred       n // ns <= 2^bits: kh_assemble_dev lets the start walkers defer (split_min = 2^bits);
    serial         the segments k_seg_chain follows itself: 128 where nsp >= 16 ns, else 32;
    adjacent, adjacent_jumped   two splitters of one chain at neighbouring indices (a segment of one
                   k-mer inside the chain), anywhere / from the serial-th splitter segment on (the
                   part the jump and fill passes rank), in the mode `deferred` says;
    max_seg        the longest segment of a chain in k-mers, in that mode."""
    ns = len(longs) + fillers
    n = sum(len(c) - k + 1 for c in longs) + fillers
    sps = [walk_splitter_indices(k, c, bits) for c in longs]
    nsp = sum(len(sp) for sp in sps)
    deferred = n // ns <= (1 << bits)
    serial = 128 if nsp >= 16 * ns else 32
    S_def = [[i for i in sp if i >= (1 << bits)] for sp in sps]
    chains = S_def if deferred else sps
    adj = [[j for j in range(len(ch) - 1) if ch[j + 1] == ch[j] + 1] for ch in chains]
    segs = [[b - a for a, b in zip([0] + ch, ch + [len(c) - k + 1])] for c, ch in zip(longs, chains)]
    return {"ns": ns, "n": n, "nsp": nsp, "S": [len(sp) for sp in sps], "S_deferred": [len(sp) for sp in S_def],
            "deferred": deferred, "serial": serial, "adjacent": any(adj),
            "adjacent_jumped": any(j >= serial - 1 for a in adj for j in a),
            "max_seg": max(max(s) for s in segs), "long_lens": [len(c) - k + 1 for c in longs]}


def chain_case(k, bits, S_list, fillers, order="shuffled", tail="after", deferred=False, need=None):
    """(text, contigs, facts): one chain_contig per entry of S_list (its count of splitter segments:
    with `deferred` the count a deferring start walker leaves, facts["S_deferred"], else facts["S"])
    plus `fillers` contigs of one k-mer, written by contigs_lines, at the first seed of CHAIN_SEEDS
    whose chain_facts show those counts and satisfy need(facts); fails with the tried facts if none
    does. The contigs do not depend on `order`."""
    B = "ACGT"
    tried = []
    for s in CHAIN_SEEDS:
        seed = 9000 + 1000 * s + 37 * k + 11 * bits + sum(S_list) + 7 * len(S_list) + fillers
        rng = np.random.default_rng(seed)
        seen, longs = set(), []
        for j, S in enumerate(S_list):
            c = chain_contig(k, bits, S, 64 * seed + j, tail, (1 << bits) if deferred else 1, seen)
            seen.update(c[i:i + k] for i in range(len(c) - k + 1))
            longs.append(c)
        singles = []
        while len(singles) < fillers:
            x = "".join(B[b] for b in rng.integers(0, 4, k))
            if x not in seen:
                seen.add(x)
                singles.append(x)
        f = dict(chain_facts(k, bits, longs, fillers), seed=seed)
        if f["S_deferred" if deferred else "S"] == list(S_list) and (need is None or need(f)):
            text, contigs = contigs_lines(k, longs + singles, rng, order)
            return text, contigs, f
        tried.append(f)
    raise AssertionError(f"no seed gives the chain case k={k}, bits={bits}, S={S_list}, fillers={fillers}: {tried}")


# The single-GPU chain boundaries (test_gpu_segments.py): three regimes at KH_SPLIT_BITS=2 (one
# splitter per 4 k-mers, forced: no filter pass).
#   many          the long contigs alone: nsp >= 16 ns (serial 128), every walker stops at every splitter;
#   few-eager     fillers so that nsp < 16 ns (serial 32) but n // ns > 4 (split_min 0);
#   few-deferred  2 sum(S) fillers so that n // ns <= 4: the start walkers defer (split_min 4) and the
#                 targets count the splitters at index >= 4.
SEG_BITS = 2
SEG_JUMP = 64
SEG_REGIMES = {"many": 128, "few-eager": 32, "few-deferred": 32}  # regime -> SegBuffers::serial


def seg_targets(serial):
    """Splitter segments of one chain: one below / at / above the serial prefix (at: exactly one
    pending segment, its jump pointer SEG_NONE), the prefix plus one and two full jumps of 64 links,
    and plus three jumps and one."""
    return [serial + d for d in (-1, 0, 1, 63, 64, 65, 127, 128, 129, 3 * SEG_JUMP + 1)]


def seg_multi(serial):
    """Four chains in one input: several pend entries live, anchors of different contigs interleaved."""
    return [serial - 1, serial + 1, serial + 64, serial + 129]


def segment_case(k, regime, S_list, tail="after", order="shuffled", bits=SEG_BITS, need=None):
    """chain_case of a regime of SEG_REGIMES with the regime's facts demanded: serial, eager or
    deferred, and the counts of S_list in that mode."""
    serial = SEG_REGIMES[regime]
    total = sum(S_list)
    fillers = {"many": 0, "few-eager": total // 16 + 1, "few-deferred": 2 * total}[regime]
    deferred = regime == "few-deferred"

    def ok(f):
        return f["serial"] == serial and f["deferred"] == deferred and (need is None or need(f))

    return chain_case(k, bits, S_list, fillers, order, tail, deferred, ok)


SEG_SINGLE_PARAMS = [(k, regime, S, tail) for k in (19, 51) for regime, serial in SEG_REGIMES.items()
                     for S in seg_targets(serial) for tail in ("on", "after")]
SEG_MULTI_PARAMS = [(k, regime, order) for k in (19, 51) for regime in SEG_REGIMES
                    for order in ("first", "last", "shuffled")]
# segments longer than one 256-base chunk inside a jumped chain: KH_SPLIT_BITS=6, k = 51
SEG_CHUNK_BITS = 6
SEG_CHUNK_PARAMS = [("few-eager", 33), ("many", 129)]


def segment_chunk_case(regime, S):
    return segment_case(51, regime, [S], "after", "shuffled", SEG_CHUNK_BITS, lambda f: f["max_seg"] > 256)


# The sharded chain boundaries (test_gpu_dist.py): the sharded walker stops at every splitter (the
# count of facts["S"]), and a pointer's span grows 8-fold per k_res_pass (RES_HOPS + 1): chains that
# finish in passes 1, 2, 3 and 4. 2 sum(S) fillers arm the short walk (k-mers / starts <= 4, the
# splitter spacing, kh_mwalk_short) and every long contig passes its 16-base limit (abandoned).
RES_TARGETS = (7, 8, 9, 63, 64, 65, 511, 512, 513)
RES_MULTI = (8, 64, 512)
RES_PARAMS = [(51, 1), (51, 2), (51, 3), (19, 2)]  # (k, ranks)


def sharded_chain_case(k, S_list):
    def ok(f):
        return f["n"] // f["ns"] <= (1 << SEG_BITS) and min(f["long_lens"]) >= 20

    return chain_case(k, SEG_BITS, list(S_list), 2 * sum(S_list), "shuffled", "after", False, ok)


# ---- walker counts around the wave (64) and the queue reservation (64 x batches) ----------------
WALKER_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513)


def short_lens(ns, seed, extra=0):
    """ns contigs of U[1,4] k-mers, plus one of `extra` k-mers if given (deferred mode with a
    contig that really stops at a splitter)."""
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.integers(1, 5, ns)] + ([extra] if extra else [])


# ---- inputs of an exact record count for the sharded route kernels (test_gpu_route.py) ----------
# One below / at / one above a wave (64), a block of the two-pass route (256), its tile
# (ROUTE_TILE = 2048) and the tile of the one-pass route (REC_TILE = 3584), and two full tiles plus
# one record.
ROUTE_SIZES = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 3583, 3584, 3585, 7169)
ROUTE_SEEDS = tuple(range(12))


def route_lens(n, seed):
    """Contig lengths (in k-mers) summing to exactly n: contigs of 1-4 k-mers and, one contig in
    eight after the first two while they fit, one of 40-300: about one record in twenty is a
    start, so the shuffled input has 64-record mask words with several starts and words with
    none."""
    rng = np.random.default_rng(seed)
    lens, left = [], n
    while left:
        long = len(lens) >= 2 and rng.random() < 0.125
        L = int(rng.integers(40, 301)) if long else int(rng.integers(1, 5))
        L = min(L, left)
        lens.append(L)
        left -= L
    assert sum(lens) == n
    return lens


def start_mask_words(k, text):
    """The 64-record start-mask words of a fixed-width text: bit i of word w = record 64 w + i has
    backward extension 'F' (kmer_hash.cpp:27-31)."""
    n = len(text) // (k + 4)
    words = [0] * ((n + 63) // 64)
    for i in range(n):
        if text[i * (k + 4) + k + 1] == ord("F"):
            words[i >> 6] |= 1 << (i & 63)
    return words


def route_ok(n, words):
    """Starts in the first and in the last mask word, a last word that is not full unless n is a
    multiple of 64 (by construction), and from one two-pass tile on a mask word without starts."""
    return bool(words[0]) and bool(words[-1]) and (n < 2047 or not all(words))


def route_text(k, n):
    """(text, contigs, seed) of exactly n k-mers: contigs_text of route_lens with one start record
    moved to the first line and another to the last (they change places with the lines there), at
    the first seed of ROUTE_SEEDS that satisfies route_ok; fails if none does. The contigs are in
    the order of their start records, as contigs_text gives them."""
    w = k + 4
    for s in ROUTE_SEEDS:
        seed = 7000 + 13 * k + n + s
        text, contigs = contigs_text(k, route_lens(n, seed), seed)
        lines = [text[i * w:(i + 1) * w] for i in range(n)]
        at = [i for i in range(n) if lines[i][k + 1] == ord("F")]
        lines[0], lines[at[0]] = lines[at[0]], lines[0]
        if len(at) > 1:
            j = at[-1] if at[-1] != 0 else at[0]  # (the line that was first now stands at at[0])
            lines[n - 1], lines[j] = lines[j], lines[n - 1]
        text = b"".join(lines)
        by_start = {c[:k]: c for c in contigs}
        contigs = [by_start[ln[:k].decode()] for ln in lines if ln[k + 1] == ord("F")]
        if route_ok(n, start_mask_words(k, text)):
            return text, contigs, seed
    raise AssertionError(f"no seed gives the route input's preconditions at k={k}, n={n}")


def chunk_bounds(n, calls, empty=None):
    """Record bounds of `calls` successive route calls over n records: chunk starts at multiples of
    16 records, as DistributedKmerHashMap.insert_all makes them (every chunk stays 16-B aligned);
    `empty` = the index of a call that gets no record (not the last call: an empty chunk too starts
    at a multiple of 16 records; the others split the records)."""
    nch = calls - (empty is not None)
    assert empty is None or 0 <= empty < nch
    b = [min(n, (n * c // nch) & ~15) for c in range(nch)] + [n]
    if empty is not None:
        b.insert(empty, b[empty])
    assert len(b) == calls + 1 and all(x % 16 == 0 for x in b[:-1]) and b == sorted(b)
    return b


def owned_subset_text(k, contigs, owner_of, keep_other, seed):
    """A closed input whose k-mers nearly all share one owner: of `contigs`, those whose k-mers all
    have the most frequent owner (owner_of(k-mer string) -> rank) plus every keep_other-th of the
    rest, their lines shuffled. Returns (text, contigs in start-record order, hot owner)."""
    own = [[owner_of(c[i:i + k]) for i in range(len(c) - k + 1)] for c in contigs]
    flat = [q for o in own for q in o]
    hot = max(set(flat), key=flat.count)
    keep = [c for c, o in zip(contigs, own) if all(q == hot for q in o)]
    keep += [c for c, o in zip(contigs, own) if any(q != hot for q in o)][::keep_other]
    lines = []
    for ci, c in enumerate(keep):
        L = len(c) - k + 1
        for i in range(L):
            lines.append((c[i:i + k], "F" if i == 0 else c[i - 1], "F" if i == L - 1 else c[i + k],
                          ci if i == 0 else -1))
    perm = np.random.default_rng(seed).permutation(len(lines))
    text = "".join(f"{lines[i][0]} {lines[i][1]}{lines[i][2]}\n" for i in perm).encode()
    return text, [keep[lines[i][3]] for i in perm if lines[i][3] >= 0], hot
