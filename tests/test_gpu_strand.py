"""GPU: reads on both strands (kh_locate_text_rc*, kh_seed_strand_*, KmerHashTable.locate_text(rc=True) /
seed_reads(strands="both") / seed_coverage over 6-word seeds, GpuShard.seed_strand_*,
DistributedKmerHashMap.locate_text(rc=True) / seed_reads(strands="both")).

Expected answers come from the text alone (strand_cases: a Python loop straight from the definitions
over locate_cases' positions), never from the code under test; every word is compared exactly.
test_strand_cpu.py checks the model on hand-written arrays and that no case used here is vacuous."""
import ctypes

import numpy as np
import pytest

import cs267_hw3_amd as kh
from cs267_hw3_amd import _lib
import locate_cases as lc
import seed_cases as sc
import strand_cases as st
import text_cases as tc
from test_gpu_find_dist import insert_block, run_ranks

pytestmark = pytest.mark.gpu

NONE = st.LOC_NONE
GUARD = 0x5A5A5A5A5A5A5A5A
G = 4  # guard words on each side of an output
W6 = st.STRAND_WORDS
_dicts = {}


def dict_of(k, text, tag):
    if (k, tag) not in _dicts:
        _dicts[(k, tag)] = lc.position_dict(k, text)
    return _dicts[(k, tag)]


def indexed(k, case=None):
    """A table of contig_case(k), assembled and indexed."""
    case = case or tc.contig_case(k)
    t = kh.KmerHashTable(k, len(case["recs"]))
    t.insert_all(case["recs"])
    t.assemble()
    t.locate_build()
    return t


def same(got, want, what=""):
    assert got.dtype == np.uint64 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1)) if len(want) else []
    assert not len(bad), (what, len(bad), bad[:6], got[bad[:6]].tolist(), want[bad[:6]].tolist())


def same1(got, want, what=""):
    assert got.dtype == np.uint64 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert not len(bad), (what, len(bad), bad[:6], got[bad[:6]].tolist(), want[bad[:6]].tolist())


def u64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def dev_text(text, to=0):
    import torch
    n = len(text)
    tbuf = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    if n:
        tbuf[to:to + n] = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    assert tbuf.data_ptr() % 16 == 0
    return tbuf


def locate_rc_dev(t, text, to=0, po=0):
    """kh_locate_text_rc_dev with the text `to` bytes and the positions `po` words from a 16-byte
    boundary -> (positions, counts); the guard words round the positions must be untouched."""
    import torch
    n = len(text)
    tbuf = dev_text(text, to)
    pbuf = torch.full((n + 2 * G + 2,), GUARD, dtype=torch.int64, device="cuda")
    counts = torch.full((2,), 77, dtype=torch.int64, device="cuda")
    assert pbuf.data_ptr() % 16 == 0
    lo = G + po
    torch.cuda.synchronize()
    t.locate_text_rc_dev(tbuf.data_ptr() + to, n, pbuf.data_ptr() + 8 * lo, counts.data_ptr())
    t.sync()
    p = pbuf.cpu().numpy().view(np.uint64)
    assert (p[:lo] == GUARD).all() and (p[lo + n:] == GUARD).all(), (to, po)
    return p[lo:lo + n].copy(), counts.cpu().numpy().view(np.uint64).tolist()


def strand_dev(t, text, off, to=0, so=0, runs_only=None):
    """kh_seed_strand_text_dev (or kh_seed_strand_runs_dev over the arrays `runs_only` = (v, w)) with the
    text `to` bytes and the seeds `so` words from a 16-byte boundary (the scratch the other way round)
    -> (seeds, v, w); the guard words round the seeds and round the position arrays must be untouched."""
    import torch
    n, m = len(text), len(off) - 1
    tbuf = dev_text(text, to)
    doff = u64(off)
    sbuf = torch.full((W6 * m + 2 * G + 2,), GUARD, dtype=torch.int64, device="cuda")
    pbuf = torch.full((2 * n + 2 * G + 2,), GUARD, dtype=torch.int64, device="cuda")
    qbuf = torch.full((n + 2 * G + 2,), GUARD, dtype=torch.int64, device="cuda")  # runs_only: w apart from v
    assert sbuf.data_ptr() % 16 == 0 and pbuf.data_ptr() % 16 == 0 and qbuf.data_ptr() % 16 == 0
    lo, plo = G + so, G + (so ^ 1)
    if runs_only is not None:
        pbuf[plo:plo + n] = u64(runs_only[0])
        qbuf[lo:lo + n] = u64(runs_only[1])
    torch.cuda.synchronize()
    if runs_only is None:
        t.seed_strand_text_dev(tbuf.data_ptr() + to, n, doff.data_ptr(), m, pbuf.data_ptr() + 8 * plo,
                               sbuf.data_ptr() + 8 * lo)
    else:
        t.seed_strand_runs_dev(pbuf.data_ptr() + 8 * plo, qbuf.data_ptr() + 8 * lo, n, doff.data_ptr(), m,
                               sbuf.data_ptr() + 8 * lo)
    t.sync()
    s, p, q = (x.cpu().numpy().view(np.uint64) for x in (sbuf, pbuf, qbuf))
    assert (s[:lo] == GUARD).all() and (s[lo + W6 * m:] == GUARD).all(), (to, so)
    seeds = s[lo:lo + W6 * m].reshape(m, W6).copy()
    if runs_only is None:
        assert (p[:plo] == GUARD).all() and (p[plo + 2 * n:] == GUARD).all() and (q == GUARD).all(), (to, so)
        return seeds, p[plo:plo + n].copy(), p[plo + n:plo + 2 * n].copy()
    assert (p[:plo] == GUARD).all() and (p[plo + n:] == GUARD).all(), (to, so)
    assert (q[:lo] == GUARD).all() and (q[lo + n:] == GUARD).all(), (to, so)
    return seeds, p[plo:plo + n].copy(), q[lo:lo + n].copy()


def state_error(f, *args, **kw):
    with pytest.raises(kh.KmerHashError) as e:
        f(*args, **kw)
    assert e.value.code == _lib.KH_ERR_STATE, e.value


def arg_error(f, *args):
    with pytest.raises(kh.KmerHashError) as e:
        f(*args)
    assert e.value.code == _lib.KH_ERR_ARG, e.value


# ---- 1: locate_text(rc=True) against the model ---------------------------------------------------
@pytest.mark.parametrize("k", tc.K_COVER)
def test_locate_rc_against_the_model(k):
    case = tc.contig_case(k)
    truth = case["truth"]
    d = dict_of(k, truth, "truth")
    texts = [truth, st.revcomp(truth), tc.mutated_text(st.revcomp(truth)), tc.mutated_text(truth),
             tc.dirty_text(k, case["contigs"]), st.revcomp(tc.dirty_text(k, case["contigs"]))]
    texts += tc.length_texts(k, max(case["contigs"], key=len))
    texts += [st.revcomp(x) for x in tc.length_texts(k, max(case["contigs"], key=len))]
    located = 0
    with indexed(k) as t:
        assert t.contigs_text() == truth
        for j, text in enumerate(texts):
            want, windows, loc = st.expected_locate_text_rc(k, d, text)
            got = t.locate_text(text, rc=True)
            same1(got[0], want, j)
            assert got[1:] == (windows, loc), (j, got[1:], windows, loc)
            if len(text):
                dev, counts = locate_rc_dev(t, text, to=j % 16, po=j & 1)
                same1(dev, want, (j, "dev"))
                assert counts == [windows, loc], j
            # the same answer by the other road: forward over the reverse complement, mirrored
            fwd = t.locate_text(st.revcomp(text))
            same1(got[0], st.mirrored(k, fwd[0]), (j, "mirror"))
            assert got[1:] == fwd[1:], j
            located += loc
        # the reverse complement of the table's own text answers every window, going down
        own = t.locate_text(st.revcomp(truth), rc=True)
    assert located > len(case["recs"]) and own[2] == len(case["recs"]) == own[1]


# ---- 2: tile edges -------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [19, 51])
def test_tile_edges(k):
    """The 20 000-base line, reverse-complemented: position i answers line_len - k - i."""
    case = tc.tile_case(k)
    line = case["contig"].encode()
    query = st.revcomp(line)
    n = len(line)
    assert tc.crosses_every_tile_edge(k, query) and n > 3 * tc.TEXT_TILE
    want = np.full(n, NONE, np.uint64)
    want[:n - k + 1] = (n - k - np.arange(n - k + 1)).astype(np.uint64)
    with indexed(k, case) as t:
        assert t.contigs_text() == line + b"\n"
        for to in tc.POINTER_OFFSETS:
            for po in (0, 1):
                got, counts = locate_rc_dev(t, query, to=to, po=po)
                same1(got, want, (to, po))
                assert counts == [n - k + 1, n - k + 1]
        # preceded by newline bytes: the line's offset in the query moves, its answers do not
        for pre in (1, 3):
            got, counts = locate_rc_dev(t, b"\n" * pre + query, to=pre, po=pre & 1)
            same1(got[pre:], want, pre)
            assert (got[:pre] == NONE).all() and counts == [n - k + 1, n - k + 1]
        # the whole line as one reverse read
        got = t.seed_reads(query + b"\n", strands="both")
    model = st.expected_for(k, dict_of(k, line + b"\n", "tile"), query + b"\n", [0, n + 1])
    same(got, model)
    assert model[0, :4].tolist() == [0, 0, n - k + 1, 1] and int(model[0, 5]) == n - k + 1 and int(model[0, 4]) <= 2


# ---- 3: reads that are the reverse complement of contig substrings -------------------------------
@pytest.mark.parametrize("k", [19, 31, 32, 51, 60])
def test_reverse_reads(k):
    d = dict_of(k, tc.contig_case(k)["truth"], "truth")
    cases = st.rc_length_reads(k)
    fwd = sc.length_reads(k)
    with indexed(k) as t:
        # at the parent these reads had no seed: the forward call still says so
        old_text, old_off = sc.join_reads([x for x, _, _ in cases])
        old = t.seed_reads(old_text, old_off)
        for read, at, w in cases:
            want = st.expected_for(k, d, read, [0, len(read)])
            assert want[0, :4].tolist() == ([0, at, w, 1] if w else list(st.EMPTY[:4])) and int(want[0, 5]) == w
            same(t.seed_reads(read, [0, len(read)], strands="both"), want, w)
            same(strand_dev(t, read, [0, len(read)])[0], want, w)
        for sep in (b"\n", b""):
            text, off = sc.join_reads([x for x, _, _ in cases], sep=sep)
            want = st.expected_for(k, d, text, off)
            same(t.seed_reads(text, off, strands="both"), want, ("batch", sep))
            assert [int(x) for x in want[:, 2]] == list(sc.WINDOW_COUNTS) and want[1:, 3].all()
        # forward and reverse reads alternate
        mixed = [x for pair in zip([r for r, _ in fwd], [r for r, _, _ in cases]) for x in pair]
        text, off = sc.join_reads(mixed)
        got = t.seed_reads(text, off, strands="both")
        plain = t.seed_reads(text, off)
    same(old, sc.expected_for(k, d, old_text, old_off), "strands='+'")
    assert (old[:, 2] <= 2).all()
    same(got, st.expected_for(k, d, text, off), "mixed")
    assert got[2::2, 3].tolist() == [0] * (len(fwd) - 1) and got[3::2, 3].tolist() == [1] * (len(fwd) - 1)
    same(got[0::2, :3], plain[0::2, :3], "forward reads: kh_seed_text's words 0-2")
    assert np.array_equal(got[:, 4], plain[:, 3])  # located_fwd is kh_seed_text's located, for every read
    assert got[2::2, 2].tolist() == got[3::2, 2].tolist() == list(sc.WINDOW_COUNTS[1:])


# ---- 4: chunk carry on the reverse strand --------------------------------------------------------
@pytest.mark.parametrize("k", [19, 51])
def test_reverse_chunk_carry(k):
    """Descending runs that end at window 62, 63, 64 of the read, and runs that begin there."""
    d = dict_of(k, tc.contig_case(k)["truth"], "truth")
    cases = st.rc_carry_reads(k)
    with indexed(k) as t:
        alone = [t.seed_reads(read, [0, len(read)], strands="both") for read, _ in cases]
        text, off = sc.join_reads([read for read, _ in cases])
        batch = t.seed_reads(text, off, strands="both")
        dev = strand_dev(t, text, off, to=3, so=1)[0]
    want = st.expected_for(k, d, text, off)
    same(batch, want, "batch")
    same(dev, want, "dev")
    for j, (read, (a, b)) in enumerate(cases):
        same(alone[j], want[j:j + 1], j)
        assert int(want[j, 2]) == max(a, b) and int(want[j, 3]) == 1 and int(want[j, 5]) == a + b, (j, want[j])
        assert int(want[j, 0]) == (0 if a >= b else len(read) - k + 1 - b), (j, want[j])


# ---- 5: the choice between the strands -----------------------------------------------------------
@pytest.mark.parametrize("k", [19, 51])
def test_choice_between_strands(k):
    d = dict_of(k, tc.contig_case(k)["truth"], "truth")
    cases = st.choice_reads(k)
    with indexed(k) as t:
        alone = [t.seed_reads(read, [0, len(read)], strands="both") for read, _, _ in cases]
        text, off = sc.join_reads([read for read, _, _ in cases])
        batch = t.seed_reads(text, off, strands="both")
    want = st.expected_for(k, d, text, off)
    same(batch, want, "batch")
    for j, (read, (a, b), order) in enumerate(cases):
        same(alone[j], want[j:j + 1], j)
        assert int(want[j, 2]) == max(a, b) and int(want[j, 3]) == (1 if b > a else 0), (j, order, want[j])
        assert (int(want[j, 4]), int(want[j, 5])) == (a, b), (j, order, want[j])  # the joint windows: the model's


# ---- 6: a table that holds both strands ----------------------------------------------------------
@pytest.mark.parametrize("k", [19, 51])
def test_table_with_both_strands(k):
    case = st.both_strands_case(k)
    lines = [c.encode() for c in case["contigs"]]
    assert st.shares_no_kmer(k, lines)
    truth = case["truth"]
    d = lc.position_dict(k, truth)
    reads = [x[j:len(x) - j % 3] for j, x in enumerate(lines)] + [x[5:5 + k + 63] for x in lines]
    text, off = sc.join_reads(reads)
    with indexed(k, case) as t:
        assert t.contigs_text() == truth
        got = t.seed_reads(text, off, strands="both")
    same(got, st.expected_for(k, d, text, off))
    windows = np.array([len(x) - k + 1 for x in reads], np.uint64)
    assert not got[:, 3].any() and np.array_equal(got[:, 4], got[:, 5]) and np.array_equal(got[:, 2], windows)
    assert np.array_equal(got[:, 4], windows) and not got[:, 0].any()


# ---- 7: the run search alone ---------------------------------------------------------------------
def test_runs_on_made_up_arrays():
    """kh_seed_strand_runs_dev over arrays no index gave, on a table that never built one."""
    k = 19
    v, w = st.made_up_arrays()
    n = len(v)
    rng = np.random.default_rng(79)
    cuts = np.sort(rng.integers(0, n + 1, 40)).astype(np.uint64)
    offs = [np.array([0, n], np.uint64), np.concatenate([[0], cuts, [n]]).astype(np.uint64),
            np.arange(0, n + 64, 64, dtype=np.uint64), np.array([n - 200, n], np.uint64),
            np.array([0, 120, 10 ** 9, 2 ** 63], np.uint64)]  # offsets past len clamp (the last one too)
    L = _lib.lib()
    with kh.KmerHashTable(k, 64) as t:  # nothing inserted, assembled or indexed
        for j, off in enumerate(offs):
            for so in (0, 1):
                got, v1, w1 = strand_dev(t, b"\x00" * n, off, so=so, runs_only=(v, w))
                same(got, st.expected_strand_seeds(k, v, w, off), (j, so))
                assert np.array_equal(v1, v) and np.array_equal(w1, w)  # inputs are read only
        # w alone, v alone: one strand each
        none = np.full(n, NONE, np.uint64)
        same(strand_dev(t, b"\x00" * n, offs[1], runs_only=(none, w))[0], st.expected_strand_seeds(k, none, w, offs[1]))
        only_v = strand_dev(t, b"\x00" * n, offs[1], runs_only=(v, none))[0]
        same(only_v, st.expected_strand_seeds(k, v, none, offs[1]))
        same(only_v[:, [0, 1, 2, 4]], sc.expected_seeds(k, v, offs[1]), "kh_seed_runs_dev's answer")
        # n_reads = 0: nothing written; len = 0: every read is empty, pointers may be NULL
        guard = np.full(4, 7, np.uint64)
        p = ctypes.c_void_p(guard.ctypes.data)
        assert L.kh_seed_strand_runs_dev(t._h, None, None, 5, None, 0, None) == _lib.KH_OK
        assert L.kh_seed_strand_runs_dev(t._h, p, p, 4, p, 0, p) == _lib.KH_OK
        assert guard.tolist() == [7] * 4
        same(strand_dev(t, b"", [0, 3, 9], runs_only=(v[:0], w[:0]))[0], np.array([st.EMPTY] * 2, np.uint64))
        state_error(t.seed_reads, b"ACGT", [0, 4], strands="both")  # ... which the text form needs
        state_error(t.locate_text, b"ACGT", rc=True)
    want = st.expected_strand_seeds(k, v, w, offs[0])
    assert want[0, 2:4].tolist() == [300, 1] and st.expected_strand_seeds(k, v, w, offs[3]).tolist() == [list(st.EMPTY)]


# ---- 8: alignment and guards ---------------------------------------------------------------------
def test_alignment_and_guards():
    import torch
    k = 51
    case = tc.contig_case(k)
    d = dict_of(k, case["truth"], "truth")
    whole = case["truth"]
    text = tc.mutated_text(whole[:len(whole) // 2]) + tc.mutated_text(st.revcomp(whole[len(whole) // 2:]))
    off = kh.read_offsets(text)
    vf = lc.expected_locate_text(k, d, text)[0]
    wr = st.expected_locate_text_rc(k, d, text)[0]
    want = st.expected_strand_seeds(k, vf, wr, off)
    assert len({int(x) for x in want[:, 2]}) > 10 and {0, 1} == set(want[:, 3].tolist())
    with indexed(k) as t:
        for to in tc.POINTER_OFFSETS:
            for so in (0, 1):
                got, v, w = strand_dev(t, text, off, to=to, so=so)
                same(got, want, (to, so))
                same1(v, vf, (to, so, "scratch: forward half"))
                same1(w, wr, (to, so, "scratch: reverse half"))
        same1(t.locate_text(text)[0], vf)
        same1(t.locate_text(text, rc=True)[0], wr)
        buf = torch.zeros(2 * len(text) + 64, dtype=torch.int64, device="cuda")
        q, n, m = buf.data_ptr(), len(text), len(off) - 1
        for args in ((q, n, q + 4, m, q, q), (q, n, q, m, q + 4, q), (q, n, q, m, q, q + 4)):
            arg_error(t.seed_strand_text_dev, *args)
        for args in ((q + 4, q, n, q, m, q), (q, q + 4, n, q, m, q), (q, q, n, q + 4, m, q), (q, q, n, q, m, q + 2)):
            arg_error(t.seed_strand_runs_dev, *args)
        for args in ((q, n, q + 4, q), (q, n, q, q + 4)):
            arg_error(t.locate_text_rc_dev, *args)


# ---- 9: states and side effects ------------------------------------------------------------------
def test_argument_errors_and_empty_inputs():
    import torch
    k = 51
    with indexed(k) as t:
        L = _lib.lib()
        d8 = torch.zeros(64, dtype=torch.int64, device="cuda")
        q = d8.data_ptr()
        # null required buffers and n_reads >= 2^32
        for args in ((q, 8, 0, 1, q, q), (q, 8, q, 1, q, 0), (0, 8, q, 1, q, q), (q, 8, q, 1, 0, q),
                     (q, 8, q, 2 ** 32, q, q)):
            arg_error(t.seed_strand_text_dev, *args)
        for args in ((q, q, 8, 0, 1, q), (q, q, 8, q, 1, 0), (0, q, 8, q, 1, q), (q, 0, 8, q, 1, q),
                     (q, q, 8, q, 2 ** 32, q)):
            arg_error(t.seed_strand_runs_dev, *args)
        for args in ((q, 8, 0, 0), (0, 8, q, q)):
            arg_error(t.locate_text_rc_dev, *args)
        host = (ctypes.c_uint64 * 16)()
        hp = ctypes.cast(host, ctypes.c_void_p)
        assert L.kh_seed_strand_text(t._h, hp, 8, None, 1, hp) == _lib.KH_ERR_ARG
        assert L.kh_seed_strand_text(t._h, hp, 8, hp, 1, None) == _lib.KH_ERR_ARG
        assert L.kh_seed_strand_text(t._h, None, 8, hp, 1, hp) == _lib.KH_ERR_ARG
        assert L.kh_seed_strand_text(t._h, hp, 8, hp, 2 ** 32, hp) == _lib.KH_ERR_ARG
        assert L.kh_locate_text_rc(t._h, hp, 8, None, None) == _lib.KH_ERR_ARG
        assert L.kh_locate_text_rc(t._h, None, 8, hp, hp) == _lib.KH_ERR_ARG
        # n_reads = 0 and len = 0
        guard = np.full(4, 7, np.uint64)
        p = ctypes.c_void_p(guard.ctypes.data)
        assert L.kh_seed_strand_text(t._h, None, 0, p, 0, p) == _lib.KH_OK
        assert L.kh_seed_strand_text_dev(t._h, None, 5, None, 0, None, None) == _lib.KH_OK
        assert L.kh_locate_text_rc(t._h, None, 0, p, p) == _lib.KH_OK
        assert L.kh_locate_text_rc_dev(t._h, None, 0, p, p) == _lib.KH_OK
        assert guard.tolist() == [7] * 4
        assert t.seed_reads(b"", [0], strands="both").shape == (0, 6)
        assert t.seed_reads(b"", strands="both").shape == (0, 6)
        same(t.seed_reads(b"", [0, 0, 5], strands="both"), np.array([st.EMPTY] * 2, np.uint64))
        same(strand_dev(t, b"", [0, 3, 9])[0], np.array([st.EMPTY] * 2, np.uint64))
        got = t.locate_text(b"", rc=True)
        assert got[0].shape == (0,) and got[1:] == (0, 0)
        short = t.locate_text(b"ACGT", rc=True)
        assert short[0].tolist() == [NONE] * 4 and short[1:] == (0, 0)
        with pytest.raises(ValueError):
            t.seed_reads(b"ACGT\n", strands="x")


def test_states():
    import torch
    from cs267_hw3_amd.dist import GpuShard
    k = 51
    case = tc.contig_case(k)
    recs, text = case["recs"], st.revcomp(case["truth"])
    more = tc.contig_case(k, seed=977)["recs"]
    start = lc.record_of(k, recs, max(case["contigs"], key=len)[:k])[None, :]

    def both(t):
        return t.seed_reads(text, strands="both")

    def fails(t):
        state_error(both, t)
        state_error(t.locate_text, text, rc=True)

    with kh.KmerHashTable(k, len(recs) + len(more)) as t:
        fails(t)                                  # nothing built
        t.insert_all(recs)
        fails(t)
        t.assemble()
        fails(t)                                  # before locate_build
        t.locate_build()
        first = both(t)
        w0 = t.locate_text(text, rc=True)
        # (the text begins with the last line's '\n': its first read is empty)
        assert first[1:, 3].all() and not first[0, 2] and w0[2] == len(recs)
        t.insert_all(more)                        # after an insert
        fails(t)
        t.assemble()
        t.locate_build()
        same(both(t), first)
        t.set_starts(start)                       # after kh_set_starts
        fails(t)
        t.assemble()                              # a new walk
        fails(t)
        t.locate_build()
        t.assemble()
        fails(t)
        t.locate_build()
        both(t)
        t.clear()                                 # after kh_clear
        fails(t)
        t.locate_reset()
        assert not both(t)[:, 2].any()            # a valid, empty index
        _lib.check(_lib.lib().kh_reserve(t._h, 1))  # a reserve that does not grow keeps it
        both(t)
        _lib.check(_lib.lib().kh_reserve(t._h, 4 * (len(recs) + len(more))))  # one that grows does not
        fails(t)
    sh = GpuShard(k, len(recs))                   # a stage left open
    with torch.cuda.stream(sh.stream):
        dev = torch.from_numpy(recs).to(sh.dev)
        dtext = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to(sh.dev)
        doff = torch.from_numpy(kh.read_offsets(text).view(np.int64)).to(sh.dev)
        words, _ = sh.route(dev, 1)
        sh.stage_words(words, len(recs), len(recs))
        state_error(sh.seed_strand_text, dtext, doff)
        state_error(sh.locate_text, dtext, rc=True)
        sh.finish_words()
        state_error(sh.seed_strand_text, dtext, doff)
        none = torch.full((dtext.numel(),), -1, dtype=torch.int64, device=sh.dev)
        assert tuple(sh.seed_strand_runs(none, none, doff).shape) == (doff.numel() - 1, 6)
        sh.sync()
    sh.table.close()


COUNTERS = ("capacity", "n_inserted", "n_starts", "n_contigs", "n_lookups", "out_bytes", "n_chunks", "n_dup",
            "n_full", "n_bad_ext", "n_missing", "n_cycle", "n_chunk_ovf", "n_bad_base", "n_hot_regions", "n_overflow")


@pytest.mark.parametrize("k", [19, 51])
def test_no_side_effects(k):
    case = tc.contig_case(k)
    KP = (k + 3) // 4
    query = tc.dirty_text(k, case["contigs"]) + b"\n" + tc.mutated_text(st.revcomp(case["truth"]))

    def snapshot(t):
        return (t.contigs_text(), t.find(case["recs"][:, :KP]), t.find_text(query), t.locate_text(query),
                t.seed_reads(query), t.stats())

    with indexed(k) as t:
        a = snapshot(t)
        t.seed_reads(query, strands="both")
        t.locate_text(query, rc=True)
        strand_dev(t, query, kh.read_offsets(query), to=1)
        locate_rc_dev(t, query, to=5, po=1)
        t.seed_coverage(t.seed_reads(query, strands="both"))
        b = snapshot(t)
    assert a[0] == b[0] == case["truth"]
    assert np.array_equal(a[1][0], b[1][0]) and np.array_equal(a[1][1], b[1][1]) and a[1][1].all()
    assert np.array_equal(a[2][0], b[2][0]) and a[2][1:] == b[2][1:]
    assert np.array_equal(a[3][0], b[3][0]) and a[3][1:] == b[3][1:]
    assert np.array_equal(a[4], b[4]) and a[4].shape[1] == 4
    assert [a[5][c] for c in COUNTERS] == [b[5][c] for c in COUNTERS]


# ---- 10: coverage --------------------------------------------------------------------------------
def test_coverage_of_strand_seeds():
    k = 51
    case = tc.contig_case(k)
    truth = case["truth"]
    d = dict_of(k, truth, "truth")
    lines = truth.split(b"\n")[:-1]
    reads = [st.revcomp(x) if j % 2 else x for j, x in enumerate(lines)]
    reads += [st.revcomp(x[3:]) for x in lines if len(x) >= k + 3] + [tc.mutated_text(st.revcomp(truth), first=70)]
    text, off = sc.join_reads(reads)
    with indexed(k) as t:
        nc = t.stats()["n_contigs"]
        seeds = t.seed_reads(text, off, strands="both")
        reads_pl, bases_pl = t.seed_coverage(seeds)
        r4, b4 = t.seed_coverage(st.repacked(seeds))
        assert t.seed_coverage(np.zeros((0, 6), np.uint64))[0].tolist() == [0] * nc
    want = st.expected_for(k, d, text, off)
    same(seeds, want)
    assert {0, 1} == set(want[:, 3].tolist())
    wr, wb = sc.expected_coverage(k, truth, st.repacked(want))
    assert reads_pl.dtype == bases_pl.dtype == np.uint64 and len(reads_pl) == nc == len(lines)
    assert np.array_equal(reads_pl, wr) and np.array_equal(bases_pl, wb)
    assert np.array_equal(r4, wr) and np.array_equal(b4, wb)
    assert (wr >= 1).all() and (wr >= 2).any() and int(wr.sum()) == int((want[:, 2] > 0).sum())
    # a whole line read from the other strand covers the line it came from
    for j, x in enumerate(lines):
        assert int(want[j, 2]) == len(x) - k + 1 and int(want[j, 3]) == j % 2


# ---- 11: sharded ---------------------------------------------------------------------------------
@pytest.mark.parametrize("P,self_exchange", [(1, False), (1, True), (2, False), (3, False)])
def test_sharded_both_strands(P, self_exchange):
    """After assemble and locate_build every rank asks for the lines of every rank's contig text, half
    of them reverse-complemented and some mutated; the answers are the single-table model's over
    rank << 48 | position values. The last rank of three asks with an empty text; rank 0 passes device
    tensors. One rank without a self-exchange must take the fused calls."""
    import torch
    k = 51
    case = tc.contig_case(k)
    recs = case["recs"]
    shared = {}

    def body(r, dm, shard, comm):
        if self_exchange:
            dm.SELF_EXCHANGE = True
        calls = []
        for name in ("seed_strand_text", "seed_strand_runs"):
            def spy(*a, _f=getattr(shard, name), _n=name, **kw):
                calls.append(_n)
                return _f(*a, **kw)
            setattr(shard, name, spy)
        rc_calls = []
        real_lt = shard.locate_text

        def lt(text, rc=False):
            rc_calls.append(bool(rc))
            return real_lt(text, rc=rc)

        shard.locate_text = lt
        insert_block(dm, shard, comm, recs, P, r)
        dm.assemble(len(recs))
        dm.locate_build()
        shard.sync()
        shared[r] = dm.contigs_text()
        comm.barrier()
        texts = [shared[q] for q in range(P)]
        lines = b"".join(texts).split(b"\n")[:-1]
        query = b"".join((st.revcomp(x) if j % 2 else x) + b"\n" for j, x in enumerate(lines))
        query += tc.mutated_text(st.revcomp(b"".join(texts)))
        quiet = P == 3 and r == 2
        ask = query if not quiet else b""
        loc = dm.locate_text(ask, rc=True)
        host = dm.seed_reads(ask, strands="both")
        assert all(isinstance(x, np.ndarray) and x.dtype == np.uint64 for x in host + loc)
        assert len(host) == 7 and len(loc) == 2
        off = kh.read_offsets(query)[::2].copy()  # two lines a read: a forward and a reverse one
        off[-1] = len(query)
        dq = torch.from_numpy(np.frombuffer(query, np.uint8).copy()).to(shard.dev)
        doff = torch.from_numpy(off.view(np.int64)).to(shard.dev)
        dev = dm.seed_reads(dq, doff if r == 0 else off, strands="both")
        dloc = dm.locate_text(dq, rc=True)
        assert all(torch.is_tensor(x) and x.dtype == torch.int64 for x in dev + dloc)
        plus = dm.seed_reads(ask)  # today's path: five entries, as before
        assert len(plus) == 5
        shard.sync()
        return {"texts": texts, "query": query, "quiet": quiet, "off": off, "host": host, "loc": loc,
                "dev": tuple(x.cpu().numpy().view(np.uint64) for x in dev),
                "dloc": tuple(x.cpu().numpy().view(np.uint64) for x in dloc),
                "calls": calls, "rc_calls": rc_calls, "plus": plus}

    outs = run_ranks(k, P, len(recs), body)
    texts, query = outs[0]["texts"], outs[0]["query"]
    where = [lc.position_dict(k, x) for x in texts]
    assert sum(len(w) for w in where) == len(recs)  # every k-mer stands on one rank, once
    raw = {}
    for q, w in enumerate(where):
        for key, x in w.items():
            raw[key] = (q << 48) | x
    v = lc.expected_locate_text(k, raw, query)[0]
    w = st.expected_locate_text_rc(k, raw, query)[0]

    def split1(x):
        none = x == NONE
        return np.where(none, x, x >> np.uint64(48)), np.where(none, x, x & np.uint64(2 ** 48 - 1))

    def split(seeds):
        rank, pos = split1(seeds[:, 1])
        return (seeds[:, 0], rank, pos) + tuple(seeds[:, j] for j in range(2, 6))

    by_line = split(st.expected_strand_seeds(k, v, w, kh.read_offsets(query)))
    by_two = split(st.expected_strand_seeds(k, v, w, outs[0]["off"]))
    plus = sc.expected_seeds(k, v, kh.read_offsets(query))
    assert {0, 1} == set(by_line[4].tolist()) and set(by_line[1].tolist()) - {NONE} == set(range(P))
    assert (by_line[3] > 0).sum() > len(by_line[3]) // 2
    empty = [np.zeros(0, np.uint64)] * 7
    for r, o in enumerate(outs):
        for got, want in zip(o["host"], by_line if not o["quiet"] else empty):
            assert np.array_equal(got, want), r
        for got, want in zip(o["loc"], split1(w) if not o["quiet"] else empty):
            assert np.array_equal(got, want), r
        for got, want in zip(o["dev"], by_two):
            assert np.array_equal(got, want), r
        for got, want in zip(o["dloc"], split1(w)):
            assert np.array_equal(got, want), r
        if not o["quiet"]:
            assert np.array_equal(o["plus"][0], plus[:, 0]) and np.array_equal(o["plus"][3], plus[:, 2])
        fused = P == 1 and not self_exchange
        assert set(o["calls"]) == ({"seed_strand_text"} if fused else {"seed_strand_runs"}), (r, o["calls"])
        assert (True in o["rc_calls"]) == fused, (r, o["rc_calls"])  # the routed path never asks a shard for rc
