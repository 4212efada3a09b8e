"""Checks of the single-GPU walk that a second attempt cannot satisfy (test infrastructure; no
product import at module level).

kh_assemble walks again without splitter segments whenever the first walk raised ST_CHUNK_OVF (a
segment claimed twice, a linked segment nobody walked, a splitter not found in the splitter table),
and resets the counter: after it the text, the contig count and n_lookups are right whatever the
segment passes did. kh_assemble_dev is the walk alone (what the benchmark's timed step runs), and
kh_sync after it reports a raised ST_CHUNK_OVF as KH_ERR_NOMEM (check_stats / stats_status)."""
import ctypes


def first_attempt(t, n, want, nc):
    """Well-formed input only: table t holds n k-mers whose oracle text is `want` (nc contigs).
    assemble_dev, sync, stats: no error, no overflow / overlap report, and the oracle's text byte for
    byte from that one walk."""
    t.assemble_dev()
    err = None
    try:
        t.sync()
    except Exception as e:  # KmerHashError: reported below, after the counters that say why
        err = e
    s = t.stats()
    assert s["n_chunk_ovf"] == s["n_cycle"] == s["n_missing"] == 0, (s, err)
    assert err is None, err
    assert s["n_contigs"] == nc
    assert s["out_bytes"] == len(want)
    assert s["n_lookups"] == n - nc
    assert t.contigs_text() == want
    return s


def host_syncs(t):
    """The table's blocking host waits so far (kh_host_syncs)."""
    from cs267_hw3_amd import _lib
    v = ctypes.c_uint64(0)
    _lib.check(_lib.lib().kh_host_syncs(t._h, ctypes.byref(v)))
    return v.value


def assemble_syncs(t):
    """One kh_assemble of table t -> (its blocking host waits, n_contigs, text bytes)."""
    s0 = host_syncs(t)
    nc, nb = t.assemble()
    return host_syncs(t) - s0, nc, nb
