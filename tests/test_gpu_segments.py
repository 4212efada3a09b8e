"""GPU: the single-GPU splitter-segment passes at the chain lengths where they change path, checked
from the walk alone. k_seg_chain follows SegBuffers::serial segments of a contig's chain itself (32,
or 128 where splitters are many per start), hands the rest to jump pointers of SEG_JUMP = 64 links
(k_seg_jump, k_seg_chain_jump) and k_seg_fill fills in the 63 segments after each anchor. The
builders of cases.py make contigs of an exact splitter-segment count at KH_SPLIT_BITS=2 (one splitter
per 4 k-mers, forced: no filter pass; inputs under 3K k-mers), in three regimes whose facts are
asserted from the Python mirror of split_hash before the GPU is touched (and proven against the
oracle on the CPU in test_cases.py):
  many          long contigs alone: serial = 128, every walker stops at every splitter;
  few-eager     a few one-k-mer contigs beside them: serial = 32, still eager;
  few-deferred  twice as many one-k-mer contigs as splitters: serial = 32, the start walkers defer
                (split_min = 4) and phase 1 of k_walk_q walks the splitter segments.
Every case is first checked with walk_checks.first_attempt (assemble_dev + sync + stats + text: a
raised ST_CHUNK_OVF cannot be repaired by kh_assemble's unsegmented second walk there), then with two
kh_assemble of the same table, then again under KH_DEBUG=seg_eager with the same text demanded."""
import functools

import pytest

import cs267_hw3_amd as kh
import oracle_bind as ob
import cases
from walk_checks import assemble_syncs, first_attempt

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def chain_input(k, regime, S_list, tail, order, bits=cases.SEG_BITS):
    """(records, oracle text, contig count, facts) of a segment case; the builder's truth is the
    oracle's text."""
    if bits == cases.SEG_CHUNK_BITS:
        text, contigs, f = cases.segment_chunk_case(regime, S_list[0])
    else:
        text, contigs, f = cases.segment_case(k, regime, list(S_list), tail, order, bits)
    recs = kh.pack_text(k, text)
    rc, want, nc, nl, _, _ = ob.assemble(k, recs)
    assert rc == 0 and nl == len(recs) - nc and len(recs) == f["n"] and nc == f["ns"]
    assert want == cases.contigs_truth(contigs)
    return recs, want, nc, f


def assert_regime(f, regime, S_list):
    """The facts the case relies on, from the mirror alone."""
    assert f["serial"] == cases.SEG_REGIMES[regime]
    assert (f["nsp"] >= 16 * f["ns"]) == (regime == "many")
    assert f["deferred"] == (regime == "few-deferred")
    assert f["S_deferred" if f["deferred"] else "S"] == list(S_list)


def check_walks(k, recs, want, nc):
    """The walk alone, then two kh_assemble of the same table (the second reads resolved records)."""
    n = len(recs)
    with kh.KmerHashTable(k, n, device=0) as t:
        t.insert_all(recs)
        first_attempt(t, n, want, nc)
        for _ in range(2):
            got_nc, nb = t.assemble()
            s = t.stats()
            assert got_nc == nc == s["n_contigs"] == s["n_starts"]
            assert nb == len(want) and t.contigs_text() == want
            assert s["n_lookups"] == n - nc
            assert s["n_missing"] == s["n_cycle"] == s["n_chunk_ovf"] == s["n_bad_ext"] == s["n_dup"] == 0


def check_case(monkeypatch, k, bits, recs, want, nc):
    monkeypatch.setenv("KH_SPLIT_BITS", str(bits))
    monkeypatch.delenv("KH_DEBUG", raising=False)
    check_walks(k, recs, want, nc)
    monkeypatch.setenv("KH_DEBUG", "seg_eager")
    check_walks(k, recs, want, nc)


@pytest.mark.parametrize("k,regime,S,tail", cases.SEG_SINGLE_PARAMS)
def test_chain_boundaries(monkeypatch, k, regime, S, tail):
    """One long contig of exactly S splitter segments: serial - 1 / serial / serial + 1 (at `serial`
    exactly one segment is left pending and its jump pointer is SEG_NONE), serial + 64 j -1 / 0 / +1
    for one and two full jumps, and three jumps plus one; the contig ends on its last splitter (a
    last segment of one k-mer) or two k-mers after it."""
    recs, want, nc, f = chain_input(k, regime, (S,), tail, "shuffled")
    assert_regime(f, regime, [S])
    assert S in cases.seg_targets(f["serial"]) and f["n"] < 3000
    check_case(monkeypatch, k, cases.SEG_BITS, recs, want, nc)


@pytest.mark.parametrize("k,regime,order", cases.SEG_MULTI_PARAMS)
def test_chain_boundaries_four_contigs(monkeypatch, k, regime, order):
    """Four long contigs at once (serial - 1, serial + 1, serial + 64, serial + 129 segments), the
    longest contig's start record first, last or anywhere: three pend entries are live, anchors of
    different contigs interleave in k_seg_fill, and the long flag one contig sets leaves the contig
    that stayed serial alone."""
    S_list = tuple(cases.seg_multi(cases.SEG_REGIMES[regime]))
    recs, want, nc, f = chain_input(k, regime, S_list, "after", order)
    assert_regime(f, regime, S_list)
    check_case(monkeypatch, k, cases.SEG_BITS, recs, want, nc)


def test_adjacent_splitters_in_jumped_part():
    """Every regime has a case, at each k, whose chain holds two neighbouring splitters past the
    serial prefix: a segment of one k-mer that only the jump and fill passes rank."""
    for k in (19, 51):
        for regime, serial in cases.SEG_REGIMES.items():
            f = chain_input(k, regime, (cases.seg_targets(serial)[-1],), "after", "shuffled")[3]
            assert f["adjacent_jumped"], (k, regime, f)


@pytest.mark.parametrize("regime,S", cases.SEG_CHUNK_PARAMS)
def test_chain_segments_past_one_chunk(monkeypatch, regime, S):
    """KH_SPLIT_BITS=6, k = 51: a chain one segment past the serial prefix whose segments average 64
    k-mers and one of which has more than 256 (a splitter segment with chunks of its own beyond the
    first: k_write_chunks_seg places them by seg_off + chunk number)."""
    recs, want, nc, f = chain_input(51, regime, (S,), "after", "shuffled", cases.SEG_CHUNK_BITS)
    assert_regime(f, regime, [S])
    assert S == f["serial"] + 1 and f["max_seg"] > 256 and f["n"] < 10_000
    check_case(monkeypatch, 51, cases.SEG_CHUNK_BITS, recs, want, nc)


# ---- the second attempt costs blocking host waits -----------------------------------------------------
def syncs_of_assemble(monkeypatch, bits, k, recs, want, nc):
    """Blocking host waits (kh_host_syncs) of the kh_assemble that follows a first walk of the same
    table, with KH_SPLIT_BITS = bits (None: the table's own density)."""
    if bits is None:
        monkeypatch.delenv("KH_SPLIT_BITS", raising=False)
    else:
        monkeypatch.setenv("KH_SPLIT_BITS", str(bits))
    n = len(recs)
    with kh.KmerHashTable(k, n, device=0) as t:
        t.insert_all(recs)
        first_attempt(t, n, want, nc)
        waits, got_nc, nb = assemble_syncs(t)
        assert got_nc == nc and nb == len(want) and t.contigs_text() == want
    return waits


SYNC_CASES = [("deferred", k, shape, None, None) for k in (19, 31, 51) for shape in ("A", "B")] + \
             [("chain", k, regime, S, None) for k, regime, S, tail in cases.SEG_SINGLE_PARAMS if tail == "after"] + \
             [("multi", k, regime, None, order) for k, regime, order in cases.SEG_MULTI_PARAMS if order == "shuffled"] + \
             [("chunk", 51, regime, S, None) for regime, S in cases.SEG_CHUNK_PARAMS]


@pytest.mark.parametrize("kind,k,shape,S,order", SYNC_CASES)
def test_assemble_waits_no_more_than_unsegmented(monkeypatch, kind, k, shape, S, order):
    """kh_assemble's second attempt adds blocking host waits (a stats read, a sized walk, a counter
    read). On well-formed input the segmented kh_assemble must wait no more often than the same call
    on the same input with splitter segments off (KH_SPLIT_BITS=0), which has no second attempt to
    take: two configurations in one run, no count written down. Over the one-reservation shapes of
    test_gpu_small.py (the table's own density) and the chain cases above."""
    monkeypatch.delenv("KH_DEBUG", raising=False)
    bits = cases.SEG_BITS
    if kind == "deferred":
        text, contigs, f = cases.deferred_case(k, shape)
        recs = kh.pack_text(k, text)
        rc, want, nc, _, _, _ = ob.assemble(k, recs)
        assert rc == 0 and want == cases.contigs_truth(contigs)
        bits = None
    elif kind == "chain":
        recs, want, nc, _ = chain_input(k, shape, (S,), "after", "shuffled")
    elif kind == "multi":
        recs, want, nc, _ = chain_input(k, shape, tuple(cases.seg_multi(cases.SEG_REGIMES[shape])), "after", order)
    else:
        recs, want, nc, _ = chain_input(k, shape, (S,), "after", "shuffled", cases.SEG_CHUNK_BITS)
        bits = cases.SEG_CHUNK_BITS
    seg = syncs_of_assemble(monkeypatch, bits, k, recs, want, nc)
    off = syncs_of_assemble(monkeypatch, 0, k, recs, want, nc)
    print(f"kh_assemble waits: segmented {seg}, unsegmented {off}")
    assert seg <= off
