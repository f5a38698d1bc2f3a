"""Lifetime of the engine's GPU resources (csrc/bsw_engine.h): a slot's streams, events, device
and pinned buffers are freed by their owners' destructors when a context is destroyed or a failed
call's recovery trims the slot pool.  Contexts are created, driven through every slot lease --
the coalesced small call, the one-chunk host pipeline, mate rescue, global alignment -- and
destroyed in a loop; every second round its first call loses one buffer growth to
BSW_OPT_TEST_FAIL_ALLOC, so that round also frees its cached slots and reruns.  Every output of
every round must equal the oracle's, and `recovery` must be 1 for exactly the injected calls."""

import numpy as np
import pytest

import bsw
import oracle
from ksw_ext_ref import bwa_fill_scmat

pytestmark = pytest.mark.gpu

N_SMALL, N_CHUNK, N_SPLIT = 3000, 20_000, 60_000


@pytest.fixture(scope="module")
def work():
    pairs, ref, qer = bsw.synth_batch(N_SPLIT)
    want = pairs.copy()
    oracle.get_scores(oracle.make_params(), want, ref, qer, 100, nthreads=16)
    gref = bsw.synth_reference(2_000_000, seed=23)
    mpairs, mqer = bsw.synth_mates(gref, 300)
    mwant = oracle.ksw_align2_batch(mpairs, gref, mqer, bwa_fill_scmat(), nthreads=16)
    gpairs, gqer = bsw.synth_globals(gref, 300)
    gwant = oracle.ksw_global2_batch(gpairs, gref, gqer, bwa_fill_scmat(), stride=64, nthreads=16)
    return dict(pairs=pairs, ref=ref, qer=qer, want=want, gref=gref, mpairs=mpairs, mqer=mqer, mwant=mwant,
                gpairs=gpairs, gqer=gqer, gwant=gwant)


def _scores(e, w, n, tag):
    got = w["pairs"][:n].copy()
    e.get_scores(got, w["ref"], w["qer"], 100)
    for f in bsw.OUT_FIELDS:
        bad = int((w["want"][f][:n] != got[f]).sum())
        assert bad == 0, f"{tag}: field {f} differs in {bad} of {n} pairs"
    return e.last_stats()


def _mates(e, w, tag):
    got = bsw.ksw_align2(e, w["mpairs"], w["gref"], w["mqer"])
    for f in bsw.KSWR_DTYPE.names:
        bad = int((w["mwant"][f] != got[f]).sum())
        assert bad == 0, f"{tag}: mate field {f} differs in {bad} jobs"


def _globals(e, w, tag):
    ws, wc, wn = w["gwant"]
    gs, gc, gn = bsw.ksw_global2(e, w["gpairs"].copy(), w["gref"], w["gqer"], stride=64)
    assert np.array_equal(ws, gs) and np.array_equal(wn, gn), f"{tag}: global scores / op counts differ"
    for i in np.flatnonzero(wn > 0):
        assert np.array_equal(wc[i, :wn[i]], gc[i, :wn[i]]), f"{tag}: global job {i}: CIGAR differs"


def test_create_run_destroy_rounds(work):
    for rnd in range(8):
        inject = rnd % 2 == 1
        tag = f"round {rnd}"
        e = bsw.Engine()
        e.set_option("test_fail_alloc", 1 if inject else 0)
        try:
            st = _scores(e, work, N_SMALL, tag + " coalesced")
        finally:
            e.set_option("test_fail_alloc", 0)
        assert st.recovery == (1 if inject else 0), f"{tag}: first call recovery {st.recovery}"
        st = _scores(e, work, N_CHUNK, tag + " one chunk")
        assert st.recovery == 0, f"{tag}: second call recovery {st.recovery}"
        _mates(e, work, tag)
        _globals(e, work, tag)
        e.close()


def test_two_logical_devices_then_destroy(work):
    """a context over two logical devices (both on the box's GPU), destroyed after one call"""
    e = bsw.Engine(devices=[0, 0])
    st = _scores(e, work, N_SPLIT, "two devices")
    assert st.recovery == 0
    e.close()
