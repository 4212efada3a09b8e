"""GPU: the sharded ingest kernels called directly (kh_route_starts_win_dev, kh_route_starts_dev,
kh_collect_starts_dev + kh_route_dev, kh_route_splitters_dev, kh_counters_dev / kh_counters), and the
sharded walk and find at the values of k where the key / slot layout changes.

Everything goes through the public C ABI (GpuShard, _lib); no test reads the internal word layout.
Routed words are decoded by find: owner q's group is inserted into an empty table with
kh_insert_words_dev and every input key is looked up there, so a record is proved to be in exactly
one group, the expected one, with its key and both extension bytes intact.

References (never the code under test):
  records      the input record array itself (cases.RecordDict: key bytes -> record)
  text, starts oracle_bind.assemble of the input (== cases.contigs_truth of the builder, checked on
               the CPU in test_cases.py): the byte-exact text fixes the start list's content and
               its record order, across chunked calls too
  splitters    cases.split_hash at KH_SPLIT_BITS=4, at the k where test_cases.py pins that mirror
               (19, 31, 51)
  owner        NONE. Placement never changes the output, so the owner function is free to be
               anything and has no external reference. What is checked is AGREEMENT: the host
               kh_key_owner, the three record routes and kh_find_route_dev group every key the
               same way, and every grouping is a partition of the input. This is not an
               independent check of the owner function.

Template instances reached (k_win1_rec<W, 512, 3584, PK, KT, true>; k_route_own<KT>;
k_route_scatter<W, KT>; R = record bytes: <= 16 is parsed from two 16-B register loads, 17 goes
through the LDS stage):

  variant         k                   instance
  win             12 14 21 29         k_win1_rec<1, .., 0, 0, true>   (generic parse)
  win             17 20               k_win1_rec<1, .., 5, 0, true>
  win             19                  k_win1_rec<1, .., 5, 19, true>
  win             30 32 41            k_win1_rec<2, .., 0, 0, true>   (generic parse)
  win             49 52               k_win1_rec<2, .., 13, 0, true>
  win             51                  k_win1_rec<2, .., 13, 51, true>
  starts, plain   13 22 29            k_route_own<0>,  k_route_scatter<1, 0>   (R = 6, 8, 10)
  starts, plain   19                  k_route_own<19>, k_route_scatter<1, 19>
  starts, plain   31 40 53            k_route_own<0>,  k_route_scatter<2, 0>   (R = 10, 12, 16)
  starts, plain   51                  k_route_own<51>, k_route_scatter<2, 51>
  starts, plain   60                  k_route_own<0>,  k_route_scatter<2, 0>   (R = 17: LDS stage)

("plain" is kh_collect_starts_dev followed by kh_route_dev.)"""
import ctypes
import functools

import numpy as np
import pytest

import cs267_hw3_amd as kh
from cs267_hw3_amd import _lib
import oracle_bind as ob
import cases
from test_gpu_find_dist import absent_keys, assert_answers, find_np, insert_block, run_ranks
from test_gpu_small import K_BOUNDARIES, boundary_case

pytestmark = pytest.mark.gpu

VARIANTS = ("win", "starts", "plain")
WIN_KS = (12, 14, 17, 19, 20, 21, 29, 30, 32, 41, 49, 51, 52)
TWO_PASS_KS = (13, 19, 22, 29, 31, 40, 51, 53, 60)
# two k per slot width get every size of cases.ROUTE_SIZES: the specialised and a generic instance
EDGE_KS = {"win": (19, 21, 51, 32), "starts": (19, 22, 51, 60), "plain": (19, 22, 51, 60)}
PS_EDGE = (1, 2, 3, 8, 64)
PS = (3, 8)
MIRROR_KS = (19, 31, 51)  # where test_cases.py pins cases.split_hash
SPLIT_BITS = 4


def ks_of(variant):
    return WIN_KS if variant == "win" else TWO_PASS_KS


def sizes_of(variant, k):
    if k <= 13:  # random k-mers collide above ~2,000 (boundary_case keeps to that too)
        return (1999, 2000)
    return cases.ROUTE_SIZES if k in EDGE_KS[variant] else (3585, 7169)


class Case:
    """An input and everything the references say about it (shared, never written to)."""

    def __init__(self, k, text, contigs=None, tag=""):
        self.k, self.tag = k, tag
        self.KP, self.R = (k + 3) // 4, (k + 3) // 4 + 2
        self.recs = kh.pack_text(k, text)
        self.n = len(self.recs)
        rc, self.want, self.nc, nl, _, _ = ob.assemble(k, self.recs)
        assert rc == 0 and nl == self.n - self.nc
        if contigs is not None:
            assert self.want == cases.contigs_truth(contigs)
        self.is_start = self.recs[:, self.KP] == ord("F")
        assert int(self.is_start.sum()) == self.nc
        self.d = cases.RecordDict(k, self.recs)
        r, f = self.d.lookup(self.recs[:, :self.KP])
        assert f.all() and np.array_equal(r, self.recs)
        self.split = None
        if k in MIRROR_KS:  # non-start records that pass the mirror's split test at 4 bits
            w = k + 4
            lim = 1 << (32 - SPLIT_BITS)
            self.split = np.array([text[i * w + k + 1] != ord("F") and
                                   cases.split_hash(text[i * w:i * w + k].decode()) < lim for i in range(self.n)])
        self.recs.setflags(write=False)
        self._own = {}

    def owners(self, sh, P):
        """The host kh_key_owner of every record's key on shard sh's parameters."""
        mode = sh.owner_mode
        if (P, mode) not in self._own:
            keys = np.ascontiguousarray(self.recs[:, :self.KP])
            base, KP, L = keys.ctypes.data, self.KP, sh.L
            own = np.fromiter((L.kh_key_owner(sh.h, ctypes.cast(base + i * KP, _lib.c_u8p), P)
                               for i in range(self.n)), dtype=np.int64, count=self.n)
            assert ((own >= 0) & (own < P)).all()
            self._own[(P, mode)] = own
        return self._own[(P, mode)]


@functools.lru_cache(maxsize=None)
def route_case(k, n):
    text, contigs, _ = cases.route_text(k, n)
    c = Case(k, text, contigs, f"route{n}")
    assert c.n == n
    return c


def text_of_records(k, recs):
    """The fixed-width text of a record array (host codec)."""
    KP = (k + 3) // 4
    return b"".join(kh.unpack_kmer(k, r[:KP]).encode() + b" " + bytes(r[KP:KP + 2]) + b"\n" for r in recs)


def make_shard(k, n):
    import os
    from cs267_hw3_amd.dist import GpuShard
    sh = GpuShard(k, max(n, 1))
    sh.owner_mode = os.environ.get("KH_OWNER", "")
    return sh


def sorted_words(a, W):
    a = a.reshape(-1, W)
    return a[np.lexsort(tuple(a[:, j] for j in range(W - 1, -1, -1)))]


def run_route(variant, c, P, bounds=None, win=None, splitters=True, build_part=False):
    """Steps 1-5 of the route parity on a fresh shard: route c's records to P owners in the calls
    `bounds` describes, check the counts against the host owner, decode every group by find, build
    the whole table from the groups and compare its text, start count and splitter counts with
    the references. Returns the groups (numpy words per owner) and the text."""
    import torch
    k, n, KP, R = c.k, c.n, c.KP, c.R
    A, B = make_shard(k, n), make_shard(k, n)
    W = A.W
    bounds = bounds or [0, n]
    with torch.cuda.stream(A.stream):
        B.table.set_stream(A.stream.cuda_stream)
        own = c.owners(A, P)
        dev = torch.from_numpy(c.recs.copy()).to(A.dev)
        parts = [[] for _ in range(P)]
        total = np.zeros(P + 1, np.int64)
        for c0, c1 in zip(bounds, bounds[1:]):
            m, chunk = c1 - c0, dev[c0:c1]
            if variant == "win":
                w = max(m, 1) if win is None else win
                words = torch.empty(P * w * W, dtype=torch.int64, device=A.dev)
                counts = A.route_win(chunk, P, words, w)
            else:
                if variant == "plain":
                    A.collect_starts(chunk)
                words, counts = A.route(chunk, P, starts=variant == "starts")
            cn = counts.cpu().numpy()[:P + 1]
            # 2. counts: per owner what the host owner says of this chunk's keys, then the total
            assert cn[P] == m, (c0, c1)
            assert np.array_equal(cn[:P], np.bincount(own[c0:c1], minlength=P)), (c0, c1)
            offs = [q * w for q in range(P)] if variant == "win" else np.concatenate([[0], np.cumsum(cn[:P])])
            for q in range(P):  # (words past counts[q] of a window are never read)
                parts[q].append(words[int(offs[q]) * W:(int(offs[q]) + int(cn[q])) * W])
            total += cn
        assert total[P] == n and np.array_equal(total[:P], np.bincount(own, minlength=P))
        groups = [torch.cat(p) for p in parts]  # (a copy: 16-B aligned whatever the window offset)
        # 4b / 5. start and splitter counts of the routes, before anything else touches the shard
        assert int(A.counters().cpu()[0]) == c.nc
        assert A.counters_host()[0] == c.nc
        spl = A.route_splitters(P).cpu().numpy()[:P]
        if not splitters or variant == "plain":  # KH_SPLIT_BITS=0; kh_route_dev counts none
            assert not spl.any()
        elif c.split is not None:
            assert np.array_equal(spl, np.bincount(own[c.split], minlength=P))
        # 3. decode by find: owner q's group alone in an empty table
        keys = dev[:, :KP].contiguous()
        found = torch.empty((P, n), dtype=torch.uint8, device=A.dev)
        out = torch.empty((P, n, R), dtype=torch.uint8, device=A.dev)
        p = A._p
        for q in range(P):
            if q:
                B.clear()
            B.insert_words(groups[q], int(total[q]))
            _lib.check(B.L.kh_find_dev(B.h, p(keys), n, p(out[q]), p(found[q])))
            s = B.stats()
            assert s["n_inserted"] == total[q] and s["n_dup"] == s["n_full"] == s["n_bad_ext"] == 0, (q, s)
            if build_part and total[q]:
                assert s["ms_build"] > 0, "the partitioned build did not run"
        mine = own[None, :] == np.arange(P)[:, None]
        assert np.array_equal(found.cpu().numpy(), mine.astype(np.uint8))
        assert np.array_equal(out.cpu().numpy(), c.recs[None] * mine[:, :, None].astype(np.uint8))
        # 4. every group into A itself: the table holds every k-mer, the starts come from the route
        for q in range(P):
            A.insert_words(groups[q], int(total[q]))
        nc, nb = A.table.assemble()
        text = A.table.contigs_text()
        assert nc == c.nc and nb == len(c.want)
        assert text == c.want
        s = A.stats()
        assert s["n_inserted"] == n and s["n_dup"] == s["n_missing"] == 0
        host_groups = [g.cpu().numpy() for g in groups]
        # ... and kh_clear takes the route's counts back to zero
        A.clear()
        assert not A.route_splitters(P).cpu().numpy()[:P].any()
        assert A.counters_host() == [0, 0]
    B.table.close()
    A.table.close()
    return host_groups, text


@pytest.fixture
def route_env(monkeypatch):
    monkeypatch.setenv("KH_INSERT", "cas")  # the decode tables: isolate the route from the region build
    monkeypatch.setenv("KH_SPLIT_BITS", str(SPLIT_BITS))
    monkeypatch.delenv("KH_OWNER", raising=False)
    monkeypatch.delenv("KH_DEBUG", raising=False)
    return monkeypatch


# ---- A. route parity ----------------------------------------------------------------------------
@pytest.mark.parametrize("variant,k,n", [(v, k, n) for v in VARIANTS for k in ks_of(v) for n in sizes_of(v, k)])
def test_route_parity(route_env, variant, k, n):
    """One call over n records: tile, block and wave edges at two k per slot width (P = 1, 2, 3, 8,
    64), one tile plus one record and two tiles plus one at every other k (P = 3, 8)."""
    c = route_case(k, n)
    for P in (PS_EDGE if k in EDGE_KS[variant] and k > 13 else PS):
        run_route(variant, c, P)


@pytest.mark.parametrize("calls,empty", [(2, None), (2, 0), (5, None), (5, 2)])
@pytest.mark.parametrize("variant,k", [(v, k) for v in VARIANTS for k in EDGE_KS[v]])
def test_route_chunked_calls(route_env, variant, k, calls, empty):
    """Successive calls append: counts per call, splitter counts accumulated, starts in call order
    (the text is byte-exact); chunk starts at multiples of 16 records, one call without records;
    the one-pass route with a window per call of that call's size."""
    c = route_case(k, 7169)
    run_route(variant, c, 3, bounds=cases.chunk_bounds(c.n, calls, empty))
    if calls == 5:
        c = route_case(k, 257)  # most calls get 48 records, none a whole wave
        run_route(variant, c, 8, bounds=cases.chunk_bounds(c.n, calls, empty))


@pytest.mark.parametrize("k", [19, 51])
def test_route_win_larger_than_n(route_env, k):
    c = route_case(k, 3585)
    run_route("win", c, 8, win=c.n + 1000)
    run_route("win", c, 3, bounds=cases.chunk_bounds(c.n, 2), win=c.n + 1000)


@pytest.mark.parametrize("variant", VARIANTS)
def test_route_hash_owner(route_env, variant):
    route_env.setenv("KH_OWNER", "hash")
    c = route_case(51, 3585)
    run_route(variant, c, 8)
    import torch  # and the hash owner is another function than the minimizer owner
    sh = make_shard(51, 16)
    hashed = c.owners(sh, 8)
    sh.table.close()
    route_env.delenv("KH_OWNER")
    sh = make_shard(51, 16)
    assert (c.owners(sh, 8) != hashed).any()
    sh.table.close()
    torch.cuda.synchronize()


@pytest.mark.parametrize("variant", ["win", "starts"])
def test_route_no_splitters(route_env, variant):
    """KH_SPLIT_BITS=0: the routes count no splitter."""
    route_env.setenv("KH_SPLIT_BITS", "0")
    run_route(variant, route_case(51, 3585), 3, splitters=False)
    run_route(variant, route_case(19, 3585), 3, bounds=cases.chunk_bounds(3585, 2), splitters=False)


@pytest.mark.parametrize("variant,k", [("win", 19), ("win", 51), ("starts", 29), ("starts", 31)])
def test_route_words_into_partitioned_build(route_env, variant, k):
    """KH_INSERT=part: the j* and order bits the routed words carry are consumed by the region
    build (decode tables and the whole table alike)."""
    route_env.setenv("KH_INSERT", "part")
    run_route(variant, route_case(k, 7169), 3, build_part=True)


@functools.lru_cache(maxsize=None)
def skew_case(k):
    """Records that nearly all share one owner at P = 8. k = 51: every contig carries one shared
    minimizer motif (the generator's hot mode). k = 19: the motif (12 bases) is the minimizer of
    only a third of a hot contig's k-mers, so the input is made by selection instead: of 60,000
    contigs of 1-4 k-mers, those wholly owned by the most frequent owner and one in 150 of the
    others."""
    if k == 51:
        g = kh.SyntheticKmers(51, 60_000, 8, 200, 0, hot_permille=1000, n_motifs=1)
        recs = g.records()
        c = Case(51, text_of_records(51, recs), tag="skew")
        assert c.want == g.truth()
        return c
    g = kh.SyntheticKmers(k, 150_000, 1, 4, 0, seed=k)
    contigs = g.truth().decode().splitlines()
    with kh.KmerHashTable(k, 16) as t:  # kh_key_owner reads the table's parameters only
        L = _lib.lib()

        def owner_of(kmer):
            return L.kh_key_owner(t._h, kh.pack_kmer(k, kmer).ctypes.data_as(_lib.c_u8p), 8)
        text, kept, _ = cases.owned_subset_text(k, contigs, owner_of, 150, seed=k)
    return Case(k, text, kept, tag="skew")


@pytest.mark.parametrize("variant", ["win", "starts"])
@pytest.mark.parametrize("k", [19, 51])
def test_route_skewed_owner(route_env, k, variant):
    """Nearly every record goes to one owner: the one-pass route places them all in that owner's
    window (win = n), the two-pass route packs one long group."""
    c = skew_case(k)
    sh = make_shard(k, 16)
    share = np.bincount(c.owners(sh, 8), minlength=8).max() / c.n  # host only, before any launch
    sh.table.close()
    assert share >= 0.9, share
    run_route(variant, c, 8)


@pytest.mark.parametrize("calls", [1, 2])
@pytest.mark.parametrize("k", TWO_PASS_KS)
def test_collect_then_route_equals_route_starts(route_env, k, calls):
    """6. kh_collect_starts_dev + kh_route_dev == kh_route_starts_dev: the same groups (sorted word
    arrays per owner: the order inside a group is not part of the contract) and the same text."""
    c = route_case(k, 2000 if k <= 13 else 3585)
    bounds = cases.chunk_bounds(c.n, calls)
    ga, ta = run_route("plain", c, 3, bounds=bounds)
    gb, tb = run_route("starts", c, 3, bounds=bounds)
    assert ta == tb == c.want
    W = _lib.lib().kh_word_count(k)
    for q in range(3):
        assert len(ga[q]) == len(gb[q]) > 0
        assert np.array_equal(sorted_words(ga[q], W), sorted_words(gb[q], W)), q


@pytest.mark.parametrize("k", [19, 29, 51, 60])
def test_find_route_agrees_with_record_routes(route_env, k):
    """kh_find_route_dev groups the keys of the records as the record routes group the records
    (both are held to the host owner; here side by side on one shard)."""
    import torch
    c = route_case(k, 3585)
    sh = make_shard(k, c.n)
    with torch.cuda.stream(sh.stream):
        for P in (3, 64):
            own = c.owners(sh, P)
            keys = torch.from_numpy(np.ascontiguousarray(c.recs[:, :c.KP])).to(sh.dev)
            out, index, counts = sh.find_route(keys, P)
            _, rcounts = sh.route(torch.from_numpy(c.recs.copy()).to(sh.dev), P, starts=True)
            sh.sync()
            index, counts = index.cpu().numpy()[:c.n], counts.cpu().numpy()[:P + 1]
            assert np.array_equal(counts, rcounts.cpu().numpy()[:P + 1])
            assert np.array_equal(np.sort(index), np.arange(c.n))
            assert np.array_equal(own[index], np.repeat(np.arange(P), counts[:P]))
            sh.clear()
    sh.table.close()


def test_route_argument_errors(route_env):
    """KH_ERR_ARG before any launch, nothing written; n = 0 is KH_OK with all P + 1 counts zero."""
    import torch
    c = route_case(51, 257)
    n, P = c.n, 3
    sh = make_shard(51, n)
    big = make_shard(53, 16)
    L, h, p = sh.L, sh.h, sh._p
    ARG = _lib.KH_ERR_ARG
    with torch.cuda.stream(sh.stream):
        big.table.set_stream(sh.stream.cuda_stream)
        dev = torch.from_numpy(c.recs.copy()).to(sh.dev)
        SENT = 0x5A5A5A5A5A5A5A5A
        words = torch.full((P * n * 2 + 2,), SENT, dtype=torch.int64, device=sh.dev)
        counts = torch.full((P + 2,), SENT, dtype=torch.int64, device=sh.dev)
        odd = torch.zeros(n * c.R + 16, dtype=torch.uint8, device=sh.dev)
        odd[1:1 + n * c.R].copy_(dev.view(-1))
        routes = {
            "win": lambda r=dev, nn=n, PP=P, w=words, win=n, cn=counts, t=h: L.kh_route_starts_win_dev(
                t, p(r) if r is not None else None, nn, PP, p(w) if w is not None else None, win,
                p(cn) if cn is not None else None),
            "starts": lambda r=dev, nn=n, PP=P, w=words, win=None, cn=counts, t=h: L.kh_route_starts_dev(
                t, p(r) if r is not None else None, nn, PP, p(w) if w is not None else None,
                p(cn) if cn is not None else None),
            "plain": lambda r=dev, nn=n, PP=P, w=words, win=None, cn=counts, t=h: L.kh_route_dev(
                t, p(r) if r is not None else None, nn, PP, p(w) if w is not None else None,
                p(cn) if cn is not None else None),
        }
        for name, f in routes.items():
            for bad in (0, 65, -1):
                assert f(PP=bad) == ARG, (name, bad)
            assert f(cn=None) == ARG, name
            assert f(r=None) == ARG and f(w=None) == ARG, name
            assert f(r=odd[1:]) == ARG, name       # records at a 16-byte-misaligned address
            assert f(t=None) == ARG, name
        win = routes["win"]
        assert win(w=words[1:]) == ARG             # window words at a 16-byte-misaligned address
        assert win(win=n - 1) == ARG and win(win=1 << 32) == ARG
        wide = torch.zeros(64 * 16, dtype=torch.uint8, device=sh.dev)  # k = 53: records of 16 bytes
        assert L.kh_route_starts_win_dev(big.h, p(wide), 64, P, p(words), 64, p(counts)) == ARG
        sh.sync()
        assert (words.cpu().numpy() == SENT).all() and (counts.cpu().numpy() == SENT).all()
        assert sh.counters_host() == [0, 0]
        # n = 0: KH_OK whatever the record / word pointers, all P + 1 counts zero, the rest untouched
        for name, f in routes.items():
            counts.fill_(SENT)
            assert f(r=None, nn=0, w=None, win=1) == _lib.KH_OK, name
            sh.sync()
            got = counts.cpu().numpy()
            assert not got[:P + 1].any() and got[P + 1] == SENT, (name, got)
        assert L.kh_collect_starts_dev(h, None, 0) == _lib.KH_OK
        assert L.kh_collect_starts_dev(h, None, 5) == ARG and L.kh_collect_starts_dev(None, p(dev), 5) == ARG
        two = torch.zeros(2, dtype=torch.int64, device=sh.dev)
        assert L.kh_counters_dev(h, None) == ARG and L.kh_counters_dev(None, p(two)) == ARG
        assert L.kh_counters(h, None) == ARG and L.kh_counters(None, (ctypes.c_uint64 * 2)()) == ARG
        assert L.kh_route_splitters_dev(h, None, P) == ARG and L.kh_route_splitters_dev(None, p(two), 2) == ARG
        for bad in (0, 65):
            assert L.kh_route_splitters_dev(h, p(words), bad) == ARG
        # the largest rank count is legal
        assert routes["win"](PP=64, w=torch.empty(64 * n * 2, dtype=torch.int64, device=sh.dev),
                             cn=torch.empty(65, dtype=torch.int64, device=sh.dev)) == _lib.KH_OK
        sh.sync()
    big.table.close()
    sh.table.close()


@pytest.mark.parametrize("hash_owner", [False, True])
def test_key_owner_host(route_env, hash_owner):
    """kh_key_owner (host code; it needs a table, hence a device, for the parameters): in [0, P),
    0 at P = 1, KH_ERR_ARG outside 1..64 and on null arguments."""
    if hash_owner:
        route_env.setenv("KH_OWNER", "hash")
    L = _lib.lib()
    for k in (13, 19, 31, 51, 60):
        c = route_case(k, 1999 if k <= 13 else 2049)
        sh = make_shard(k, 16)
        for P in PS_EDGE:
            own = c.owners(sh, P)
            assert own.min() >= 0 and own.max() < P
            if P == 1:
                assert not own.any()
            if P == 64:
                assert len(np.unique(own)) > 8  # (not a constant, not a few ranks only)
        key = np.ascontiguousarray(c.recs[0, :c.KP])
        for bad in (0, -1, 65):
            assert L.kh_key_owner(sh.h, key.ctypes.data_as(_lib.c_u8p), bad) == _lib.KH_ERR_ARG
        assert L.kh_key_owner(None, key.ctypes.data_as(_lib.c_u8p), 2) == _lib.KH_ERR_ARG
        assert L.kh_key_owner(sh.h, None, 2) == _lib.KH_ERR_ARG
        sh.table.close()


def test_key_owner_hash_differs_from_minimizer(route_env):
    c = route_case(51, 2049)
    keys = c.recs[:1000]
    assert len(keys) == 1000
    sh = make_shard(51, 16)
    mini = c.owners(sh, 8)[:1000]
    sh.table.close()
    route_env.setenv("KH_OWNER", "hash")
    sh = make_shard(51, 16)
    assert (c.owners(sh, 8)[:1000] != mini).any()
    sh.table.close()


# ---- B. the sharded walk at the key-layout boundaries -------------------------------------------
def rank_texts(k, recs, want, P):
    """The oracle's text of each rank's block: its contigs are in start-record order, so contig i
    belongs to the rank whose block (read_kmers.hpp:55-58) holds the i-th start record."""
    KP = (k + 3) // 4
    starts = np.nonzero(recs[:, KP] == ord("F"))[0]
    lines = want.splitlines(keepends=True)
    assert len(lines) == len(starts)
    n = len(recs)
    split = (n + P - 1) // P
    out = []
    for r in range(P):
        b = min(r * split, n)
        e = min(b + split, n)
        out.append(b"".join(ln for s, ln in zip(starts, lines) if b <= s < e))
    return out


def check_sharded(k, P, **kw):
    from cs267_hw3_amd.dist import run_threaded
    recs, want, nc, _, _ = boundary_case(k)
    info = {}
    texts = run_threaded(k, recs, P, info=info, **kw)
    for r, (got, exp) in enumerate(zip(texts, rank_texts(k, recs, want, P))):
        assert got == exp, f"rank {r}"
    assert sorted(b"".join(texts).splitlines()) == sorted(want.splitlines())
    return info


@pytest.fixture
def walk_env(monkeypatch):
    for v in ("KH_INSERT", "KH_SPLIT_BITS", "KH_OWNER", "KH_DEBUG"):
        monkeypatch.delenv(v, raising=False)
    return monkeypatch


@pytest.mark.parametrize("P", [1, 2, 3])
@pytest.mark.parametrize("k", K_BOUNDARIES)
def test_sharded_walk_k_boundaries(walk_env, k, P):
    """boundary_case(k)'s records over P logical ranks (P = 1 with the route and the exchanges
    forced): each rank's text is the oracle's text of its block."""
    from cs267_hw3_amd.dist import DistributedKmerHashMap
    if P == 1:
        walk_env.setattr(DistributedKmerHashMap, "ROUTE_ONE_RANK", True)
        walk_env.setattr(DistributedKmerHashMap, "SELF_EXCHANGE", True)
    check_sharded(k, P)


@pytest.mark.parametrize("k", K_BOUNDARIES)
def test_sharded_walk_k_boundaries_segmented(walk_env, k):
    """KH_SPLIT_BITS=3: a splitter every 8 k-mers, so the segmented end of the walk (link / pred /
    resolve / retag / end_seg) runs at every k."""
    walk_env.setenv("KH_SPLIT_BITS", "3")
    info = check_sharded(k, 3)
    assert sum(c["nsp"] for c in info["counts"].values()) > 0


@pytest.mark.parametrize("k", [19, 29, 30, 51, 52])
def test_sharded_walk_two_pass_route(walk_env, k):
    """ROUTE_WINDOW_BYTES = 0: the whole sharded step through the two-pass route at k <= 52, in
    one call and in chunks."""
    from cs267_hw3_amd.dist import DistributedKmerHashMap
    walk_env.setattr(DistributedKmerHashMap, "ROUTE_WINDOW_BYTES", 0)
    check_sharded(k, 3)
    check_sharded(k, 2, insert_chunks=3)


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("k", [12, 14, 20, 22, 41, 52, 53])
def test_sharded_find_k_boundaries(walk_env, k, P):
    """dm.find after the walk at the k test_find_golden does not reach: every inserted key and the
    one-base-changed absent keys, asked by rank 0 and (another shuffle) by the last rank."""
    recs, want, nc, _, _ = boundary_case(k)
    KP = (k + 3) // 4
    d = cases.RecordDict(k, recs)
    present = np.ascontiguousarray(recs[:, :KP])
    q = np.concatenate([present, absent_keys(k, d, present)])
    qs = [np.ascontiguousarray(q[np.random.default_rng(k + r).permutation(len(q))]) if r in (0, P - 1) else q[:0]
          for r in range(P)]
    assert len(q) > len(present)

    def body(r, dm, shard, comm):
        insert_block(dm, shard, comm, recs, P, r)
        dm.assemble(len(recs))
        return dm.contigs_text(), find_np(dm, shard, qs[r])

    out = run_ranks(k, P, len(recs), body)
    for r, exp in enumerate(rank_texts(k, recs, want, P)):
        assert out[r][0] == exp, f"rank {r}"
        assert_answers(d, qs[r], out[r][1], f"rank {r}")
