"""Shared generators of edge-case inputs (test infrastructure; no GPU, no product imports)."""
import numpy as np


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


def contigs_text(k, lens, seed, order="shuffled"):
    """Well-formed input of independent random contigs, contig i of lens[i] k-mers (lens[i] + k - 1
    bases): bwd 'F' on each first k-mer, fwd 'F' on each last. A contig that would repeat a k-mer
    (its own or an earlier contig's: likely at small k) is drawn again. The lines are shuffled;
    order="first" / "last" then puts the start record of the longest contig before / after every
    other line. Returns (text, contigs): the fixed-width text (read_kmers.hpp:54-79 lines) and the
    contig strings in the order of their start records, which is the expected test_0.dat."""
    assert order in ("shuffled", "first", "last")
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


def contigs_truth(contigs):
    """test_0.dat of contigs_text's second result: one contig per line."""
    return "".join(c + "\n" for c in contigs).encode()


def split_hash(kmer):
    """kh_codec.hpp split_hash of a k-mer string (V = 2-bit bases, first base most significant)."""
    v = 0
    for ch in kmer:
        v = (v << 2) | "ACGT".index(ch)
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


# ---- walker counts around the wave (64) and the queue reservation (64 x batches) ----------------
WALKER_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513)


def short_lens(ns, seed, extra=0):
    """ns contigs of U[1,4] k-mers, plus one of `extra` k-mers if given (deferred mode with a
    contig that really stops at a splitter)."""
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.integers(1, 5, ns)] + ([extra] if extra else [])
