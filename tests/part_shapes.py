"""The partitioned insert's dispatch, mirrored in Python, and the cases of test_gpu_part_shapes.py
(test infrastructure; no GPU, no product import).

Two numbers decide which kernels a partitioned insert (KH_INSERT=part) runs. The region count
2^rbits comes from the table's capacity (kh_capi.cpp size_table, kh_codec.hpp set_region_bits):
pass 2 (k_win2) sorts by b2 = rbits - 9 bits. The region window RC comes from the size of the batch
being built (kh_build.hip part_region_cap: the batch of a one-call insert, the announced total of a
staged one): launch_build_windows picks the prefetching build with 4, 6 or 12 words per thread, or
the plain build, by it. The k-mer length picks the slot words, the compiled instance (KT) and the
records or the convert pass. shape() restates all of it; the searches find table and batch sizes
that put a case where it has to be; test_part_shapes_cpu.py pins the mirror to figures computed
from the C++ formulas and proves every GPU case's preconditions."""
import math
from collections import namedtuple

REGION_BITS_MIN, REGION_BITS_MAX = 9, 17  # kh_codec.hpp
REGION_SLOTS = 3072                       # kh_codec.hpp: target slots per region
B1 = 9                                    # kh_build.hip: pass-1 radix bits
S1 = 8                                    # pass-1 windows per bucket
NW1 = (1 << B1) * S1
CLUMP = 30.0
BUILD_THREADS = 512
KMAX_W1 = 29                              # kh_codec.hpp: one slot word up to here
REC_TILE = 3584                           # records per tile of k_win1_rec

Shape = namedtuple("Shape", "k n_kmers load n_batch cap rbits b2 RC CAP1 variant balanced W KT P R pad "
                            "rec_pass sorted_fresh split_bits")


def capacity(n_kmers, load):
    """size_table: ceil(n_kmers / load) in doubles, at least 2."""
    c = float(n_kmers if n_kmers else 1) / load
    cap = int(c)
    if float(cap) < c:
        cap += 1
    return max(cap, 2)


def region_bits(cap):
    """set_region_bits: the fewest bits in 9..17 that leave at most 3072 slots per region."""
    b = REGION_BITS_MIN
    while b < REGION_BITS_MAX and (cap >> b) > REGION_SLOTS:
        b += 1
    return b


def region_cap(n_batch, rbits):
    """part_region_cap: words per region window of pass 2."""
    mu = float(n_batch) / (1 << rbits)
    return int(mu + 7.0 * math.sqrt(CLUMP * mu) + 16.0)


def win1_cap(n_batch):
    """part_win1_cap: words per pass-1 window."""
    mu = float(n_batch) / NW1
    return int(mu + 10.0 * math.sqrt(mu * (1.0 + CLUMP / S1)) + 64.0)


def build_variant(RC):
    """launch_build_windows without KH_DEBUG=plain_build."""
    if RC <= 4 * BUILD_THREADS:
        return "pf4"
    if RC <= 6 * BUILD_THREADS:
        return "pf6"
    if RC <= 12 * BUILD_THREADS:
        return "pf12"
    return "plain"


def default_split_bits(n_kmers):
    """size_table's splitter density without KH_SPLIT_BITS: clamp(log2(n / 2^20) + 1, 4, 12)."""
    bits = 1
    while bits < 12 and (n_kmers >> (20 + bits)) != 0:
        bits += 1
    return max(bits, 4)


def shape(k, n_kmers, load, n_batch):
    """The dispatch of one build of n_batch k-mers into a table created for n_kmers at `load`."""
    cap = capacity(n_kmers, load)
    rbits = region_bits(cap)
    RC = region_cap(n_batch, rbits)
    P = (k + 3) // 4
    W = 1 if k <= KMAX_W1 else 2
    return Shape(k=k, n_kmers=n_kmers, load=load, n_batch=n_batch, cap=cap, rbits=rbits, b2=rbits - B1, RC=RC,
                 CAP1=win1_cap(n_batch), variant=build_variant(RC), balanced=load > 0.6, W=W,
                 KT=k if k in (19, 51) else 0,                       # kt_of: the compiled instances
                 P=P, R=P + 2, pad=4 * P - k,
                 rec_pass=(P == 13 and W == 2) or (P == 5 and W == 1),  # rec_pass_ok; else the convert pass
                 sorted_fresh=W == 2,                                 # fresh build: sorted 16-B slice, else LDS CAS
                 split_bits=default_split_bits(n_kmers))


def min_cap(rbits):
    """The smallest capacity with this region count: set_region_bits adds a bit while the floor of
    cap / 2^b is above 3072, that is from cap = 3073 * 2^b on."""
    return 2 if rbits == REGION_BITS_MIN else (REGION_SLOTS + 1) << (rbits - 1)


ROOM = 32768  # every table of the sweep has room for the largest record set and a second batch


def n_kmers_for(rbits, load):
    """The smallest n_kmers >= ROOM whose table has 2^rbits regions at `load`."""
    n = max(ROOM, int(min_cap(rbits) * load) - 2)
    while capacity(n, load) < min_cap(rbits):
        n += 1
    assert region_bits(capacity(n, load)) == rbits, (rbits, load, n)
    return n


def smallest_n(k, load, rbits, RC_target, extra=0):
    """The smallest batch n whose window is RC_target words in a table created for n + extra k-mers
    (extra: an earlier batch) that has 2^rbits regions; fails if no such batch exists. RC does not
    fall as n grows and rises by at most one per k-mer, so the first n that reaches the target has
    exactly it."""
    lo, hi = 1, 1 << 34
    while lo < hi:
        mid = (lo + hi) // 2
        if region_cap(mid, rbits) >= RC_target:
            hi = mid
        else:
            lo = mid + 1
    s = shape(k, lo + extra, load, lo)
    assert s.RC == RC_target and s.rbits == rbits, (s, RC_target, rbits)
    assert region_cap(lo - 1, rbits) == RC_target - 1
    return lo


# ---- the cases of test_gpu_part_shapes.py -----------------------------------------------------------
# a. region-count sweep: record counts one above a wave and one above one, two and three tiles of
# k_win1_rec (a subset of test_gpu_win1.SIZES), tables of n_kmers_for(rbits, 0.5)
SWEEP_SIZES = (65, REC_TILE + 1, 2 * REC_TILE + 1, 3 * REC_TILE + 1)
SWEEP = [(19, r) for r in range(9, 18)] + [(51, r) for r in (10, 11, 13, 17)] + [(31, r) for r in (10, 14)]
SWEEP_WAYS = [(19, 12), (51, 13), (31, 10)]           # the other entry ways, one rbits per k
SWEEP_SECOND = [(19, 11), (19, 14), (51, 11), (31, 14)]  # a second batch (non-fresh build) and locate
SECOND_SIZES = (REC_TILE + 1, 2 * REC_TILE + 1)       # first batch, second batch
# b. window spill in pass 1 and pass 2 with b2 > 0
SPILL_K, SPILL_FIRST, SPILL_HOT = 51, 65, 20_000
SPILL_RBITS = (11, 15)
# d. the generic records pass (KT = 0, P = 5 or 13) with pad 2 and 3
PAD_KS = (17, 18, 49, 50)
PAD_RBITS = (9, 11)

# c. build variants at their edges: name -> (load, rbits, RC of the big batch, variant).
# The batch is smallest_n(k, load, rbits, RC, extra); fresh: extra = 0; non-fresh: a first batch of
# BUILD_FIRST records, then the big one (RC comes from the batch being built).
BUILD_FIRST = 65
BUILD_KS = (19, 31, 51)
BUILD_CASES = {
    "rc2048": (0.5, 9, 2048, "pf4"),     # pf4 | pf6
    "rc2049": (0.5, 9, 2049, "pf6"),
    "rc3072": (0.51, 9, 3072, "pf6"),    # pf6 | pf12: load just above 0.5 keeps 512 regions
    "rc3073": (0.51, 9, 3073, "pf12"),
    "bal4487": (0.85, 9, 4487, "pf12"),  # balanced bounds, about 1.3M k-mers
    "r10": (0.5, 10, 2190, "pf6"),       # pass 2 sorts one bit: about 1.0M k-mers
}


def build_case(name, k, fresh):
    """-> (n_kmers, batch, Shape of the big batch's build)."""
    load, rbits, RC, _ = BUILD_CASES[name]
    extra = 0 if fresh else BUILD_FIRST
    n = smallest_n(k, load, rbits, RC, extra)
    return n + extra, n, shape(k, n + extra, load, n)
