"""Automatic frequency control (include/navtex_amd_afc.h) on the GPU (-m gpu).  The k trace of every tracking chain equals
the restatement (tests/afc_ref.py) applied to the chain's own per-launch signal records, launch for launch, and its bits
equal tune_ref's with that trace; a handle whose tracking is off, and the untracked sibling of a tracking chain, give a
plain handle's bits; launches queued without a fetch track as fetched ones do; a drifting carrier delivers its message
only with tracking; steps, gates, limits, absent streams, resets, re-centring and groups."""
import numpy as np
import pytest

import afc_ref as ar
import signal_ref as sr
import tune_ref as tr

pytestmark = pytest.mark.gpu

REC = ("samples", "b_samples", "sum_dphi_b", "sum_dphi_y", "sum_mf_hi", "sum_mf_lo")


def _frame(nv, raw):
    return nv.FRAME_RAW if raw else nv.FRAME_IN


def _rate(nv, raw):
    return nv.RATE_RAW if raw else nv.RATE_IN


def _run(nv, iqs, raw=False, launches=None, afc=None, fetch_each=True, reports=True, soft=False, masks=None):
    """Resident launches over streams `iqs` (whole frames each), launches = frames per launch; afc: {(stream, chain): fields}.
    Returns (trace per chain, bits per chain, records per chain per launch -- when fetched after every launch with reports on)."""
    n, frame = len(iqs), _frame(nv, raw)
    frames = iqs[0].shape[0] // frame
    launches = launches or [1] * frames
    pitch = frames * frame
    buf = nv.DeviceBuffer(n * pitch * 4)
    for s in range(n):
        buf.upload(iqs[s], s * pitch * 4)
    masks = masks or [3] * n
    chains = [(s, c) for s in range(n) for c in range(2) if (masks[s] >> c) & 1]
    recs = {sc: [] for sc in chains}
    with nv.Pipeline(n_streams=n, raw_rate=raw, chain_masks=masks, max_frames=max(launches), char_layer=False) as p:
        if reports:
            p.enable_signal_report(True)
        if soft:
            p.enable_soft(nv.SOFT_DECODE)
        for (s, c), fields in (afc or {}).items():
            p.afc_enable(s, c, **fields)
        f0 = 0
        for nf in launches:
            p.process_resident(buf, pitch, f0, nf)
            f0 += nf
            if fetch_each:
                p.fetch()
                if reports:
                    for sc in chains:
                        r = p.signal_report(*sc, reset=True)
                        recs[sc].append({k: r[k] for k in REC})
        p.fetch()
        traces = {sc: p.afc_trace(*sc) for sc in chains}
        bits = {sc: p.bits(*sc) for sc in chains}
        status = {sc: p.afc_status(*sc) for sc in chains}
    buf.free()
    return traces, bits, recs, status


def _want_bits(nv, iq, raw, ch, trace, launches):
    ks = [k for k, nf in zip(trace, launches) for _ in range(nf)]
    return tr.decode(tr.chain(tr.front(iq, raw), ch, ks))


# ---- 1. off is off
@pytest.mark.parametrize("raw", [False, True], ids=["252k", "raw"])
def test_off_is_off(nv, raw):
    iq = ar.segment(nv, _rate(nv, raw), 3, ar.FILLER, 25)
    _, plain, _, _ = _run(nv, [iq], raw, [2, 1], reports=False)
    frame, pitch = _frame(nv, raw), 3 * _frame(nv, raw)
    buf = nv.DeviceBuffer(pitch * 4)
    buf.upload(iq)
    with nv.Pipeline(n_streams=1, raw_rate=raw, chain_mask=3, max_frames=2, char_layer=False) as p:      # enabled, then disabled
        for c in (0, 1):
            p.afc_enable(0, c)
        for c in (0, 1):
            p.afc_disable(0, c, keep=False)
        p.process_resident(buf, pitch, 0, 2); p.process_resident(buf, pitch, 2, 1); p.fetch()
        assert {(0, c): p.bits(0, c) for c in (0, 1)} == plain
        assert p.afc_status(0, 0)["enabled"] == 0 and p.afc_trace(0, 0) == []
    buf.free()
    assert frame > 0 and len(plain[(0, 0)]) > 20          # (three frames: the bit timing is primed after two)
    # tracking on chain 0 only: the sibling's bits are the plain handle's (its k comes from the tracking arrays)
    traces, bits, _, _ = _run(nv, [iq], raw, [2, 1], afc={(0, 0): {}}, reports=False)
    assert bits[(0, 1)] == plain[(0, 1)] and len(traces[(0, 0)]) == 2 and traces[(0, 1)] == []


# ---- 2. + 3. the law exactly, and the ordering
DRIFTS = ((10, 40.0), (-5, -30.0))       # per stream: (offset of the carriers at the start, drift over the input) in Hz
FRAMES = 9


@pytest.fixture(scope="module")
def drifting(nv):
    """Two streams x two chains whose carriers drift over nine frames; one-frame launches fetched one by one with reports."""
    iqs = [ar.chirp(ar.segment(nv, nv.RATE_IN, FRAMES, ar.FILLER, d0, seed=31 + s), nv.RATE_IN, hz, FRAMES * nv.FRAME_IN) for s, (d0, hz) in enumerate(DRIFTS)]
    afc = {(s, c): {} for s in range(2) for c in range(2)}
    return iqs, afc, _run(nv, iqs, False, [1] * FRAMES, afc)


def test_the_law_exactly(nv, drifting):
    iqs, afc, (traces, bits, recs, status) = drifting
    moved = 0
    for (s, c), got in traces.items():
        want, flags = ar.trace(ar.DEFAULTS, tr.NOMINAL[c], recs[(s, c)])
        assert got == want, (s, c, got, want)
        assert bits[(s, c)] == _want_bits(nv, iqs[s], False, c, got, [1] * FRAMES), (s, c)
        st = status[(s, c)]
        assert (st["enabled"], st["centre_k"], st["k_last"], st["launches"]) == (1, tr.NOMINAL[c], got[-1], FRAMES)
        assert st["updates"] == sum(f & ar.UPDATE != 0 for f in flags) and st["held"] == FRAMES - st["updates"]
        assert st["clamped"] == sum(f & ar.CLAMP != 0 for f in flags) and st["offset_hz"] == got[-1] * 3.125
        moved += got[-1] != got[0]
    assert moved == 4                                     # every chain followed its carrier somewhere: the comparison is not of constants


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
def test_queued_launches_track_as_fetched_ones(nv, drifting, soft):
    """All launches queued back to back without a fetch (the update kernel of launch L and the cascade of L + 2 are ordered
    by the event alone), with and without soft decisions (the event then sits behind the FSM either way)."""
    iqs, afc, (traces, bits, _, _) = drifting
    t2, b2, _, _ = _run(nv, iqs, False, [1] * FRAMES, afc, fetch_each=False, reports=False, soft=soft)
    assert t2 == traces and b2 == bits


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
def test_three_frame_launches_on_both_array_parities(nv, drifting, soft):
    """Three launches (an odd number: both k arrays are written and read) of three frames: the trace from the launches' own
    records, the bits with a k per launch, and the same queued without a fetch."""
    iqs, afc, _ = drifting
    L = [3, 3, 3]
    traces, bits, recs, _ = _run(nv, iqs, False, L, afc)
    for (s, c), got in traces.items():
        assert got == ar.trace(ar.DEFAULTS, tr.NOMINAL[c], recs[(s, c)])[0], (s, c)
        assert bits[(s, c)] == _want_bits(nv, iqs[s], False, c, got, L), (s, c)
    assert any(t[2] != t[0] for t in traces.values())
    t2, b2, _, _ = _run(nv, iqs, False, L, afc, fetch_each=False, reports=False, soft=soft)
    assert t2 == traces and b2 == bits


# ---- 4. what it is for
@pytest.mark.parametrize("raw", [False, True], ids=["252k", "raw"])
def test_a_drifting_carrier_delivers_its_message_only_with_tracking(nv, raw):
    iq, ramp, frames = ar.drift_then_hold(nv, _rate(nv, raw))
    for track in (True, False):
        with nv.Pipeline(n_streams=1, raw_rate=raw, chain_mask=3, max_frames=1, push_mode=True) as p:
            if track:
                p.afc_enable(0, 0); p.afc_enable(0, 1)
            p.push(0, iq); p.flush()
            got = {f: [m[3] for m in p.messages if m[1] == f] for f in (518, 490)}
            assert got == ({518: [ar.MESSAGE], 490: [ar.MESSAGE]} if track else {518: [], 490: []}), (track, got)
            if track:
                for c in (0, 1):
                    t = np.array(p.afc_trace(0, c))
                    assert t.shape[0] == frames
                    assert np.all(np.abs((t[ramp + 10:] - tr.NOMINAL[c]) * 3.125 - ar.DRIFT_HZ) <= sr.OFFSET_TOL), (c, t)


# ---- 5. a step
def test_a_step_at_a_launch_boundary(nv):
    iq = ar.stepped(nv, nv.RATE_IN, 5, 15, 25)
    traces, bits, recs, _ = _run(nv, [iq], False, None, {(0, 0): {}, (0, 1): {}})
    for (s, c), got in traces.items():
        assert got == ar.trace(ar.DEFAULTS, tr.NOMINAL[c], recs[(s, c)])[0], (c, got)
        assert abs((got[-1] - tr.NOMINAL[c]) * 3.125 - 25) <= sr.OFFSET_TOL, (c, got)
        assert bits[(s, c)] == _want_bits(nv, iq, False, c, got, [1] * 20)


# ---- 6. gates and limits
def test_gates_and_limits(nv):
    frames = 8
    noise = nv.synth_host(nv.make_stream([], seed=11, noise_amp=1500), nv.RATE_IN, frames * nv.FRAME_IN)
    traces, _, recs, status = _run(nv, [noise], False, None, {(0, 0): {}, (0, 1): {}})
    for (s, c), got in traces.items():
        assert got == [tr.NOMINAL[c]] * frames and status[(s, c)]["held"] == frames == status[(s, c)]["launches"] and status[(s, c)]["updates"] == 0
        assert all(sr.derive(dict(r, sum_power=1.0, sum_dphi2_b=0.0, sum_dphi2_y=0.0))["contrast"] < sr.CONTRAST_SPLIT for r in recs[(s, c)])
    # a carrier 40 Hz off against a range of 4 k (12.5 Hz): k stops at the range's edge
    iq = ar.segment(nv, nv.RATE_IN, 10, ar.FILLER, 40)
    par = dict(ar.DEFAULTS, range_k=4)
    traces, _, recs, status = _run(nv, [iq], False, None, {(0, 0): dict(range_k=4)}, masks=[1])
    got = traces[(0, 0)]
    assert got == ar.trace(par, tr.NOMINAL[0], recs[(0, 0)])[0] and got[-1] == tr.NOMINAL[0] + 4 and max(got) == tr.NOMINAL[0] + 4
    assert status[(0, 0)]["clamped"] > 0
    # max_step 1: no launch moves k by more than one
    par = dict(ar.DEFAULTS, max_step=1)
    traces, _, recs, status = _run(nv, [iq], False, None, {(0, 0): dict(max_step=1)}, masks=[1])
    got = traces[(0, 0)]
    assert got == ar.trace(par, tr.NOMINAL[0], recs[(0, 0)])[0]
    assert max(abs(b - a) for a, b in zip(got, got[1:])) == 1 and got[-1] > got[0] + 3 and status[(0, 0)]["clamped"] > 0


# ---- 7. independent streams
def test_a_stalled_stream_holds_its_k_and_the_other_is_unaffected(nv):
    """Push mode, frame by frame.  Stream 1 goes silent for four launches (the list kernels), comes back, and both end on a
    ragged length (nvx_finish).  Per launch of the handle every participant's record is read; a stream's trace is the
    restatement with the launches it missed as holds, taken at the launches it took part in."""
    F, tail = nv.FRAME_IN, 30000
    # which streams push a frame in step i: stream 1 misses steps 4 .. 7
    steps = [(0, 1)] * 4 + [(0,)] * 4 + [(0, 1)] * 4
    n = len(steps)
    total = [sum(s in who for who in steps) for s in range(2)]
    iqs = [ar.segment(nv, nv.RATE_IN, total[s] + 1, ar.FILLER, d, seed=41 + s)[:total[s] * F + tail] for s, d in enumerate((25, -20))]
    recs = {(s, c): [] for s in range(2) for c in range(2)}
    pos = [0, 0]
    with nv.Pipeline(n_streams=2, chain_mask=3, max_frames=1, push_mode=True, char_layer=False, stall_timeout_ms=-1) as p:
        p.enable_signal_report(True)
        for sc in recs:
            p.afc_enable(*sc)
        for who in steps:
            p.set_active(1, 1 in who)
            for s in who:
                p.push(s, iqs[s][pos[s]:pos[s] + F]); pos[s] += F
            p.fetch()
            assert p.stream_stats(0)[1] == pos[0] // F and p.stream_stats(1)[1] == pos[1] // F      # one launch per step, of exactly `who`
            for (s, c) in recs:
                r = p.signal_report(s, c, reset=True)
                recs[(s, c)].append({k: r[k] for k in REC} if s in who else None)
                assert (r["samples"] > 0) == (s in who)
        p.set_active(1, True)
        for s in range(2):
            p.push(s, iqs[s][pos[s]:])
        p.finish()                                        # launch n: the ragged ends of both streams
        traces = {sc: p.afc_trace(*sc) for sc in recs}
        bits = {sc: p.bits(*sc) for sc in recs}
        assert p.stream_stats(0)[2] >= 4                  # launches that covered only some of the streams
    for (s, c), got in traces.items():
        K, _ = ar.trace(ar.DEFAULTS, tr.NOMINAL[c], recs[(s, c)], n + 1)
        assert got == [K[L] for L in range(n) if recs[(s, c)][L] is not None] + [K[n]], (s, c, got, K)
        if s == 1:                                        # absent in launches 4 .. 7: K[6] .. K[9] hold K[5]
            assert K[5] == K[6] == K[7] == K[8] == K[9] and got[4] == K[8]
    assert traces[(0, 0)][-1] != tr.NOMINAL[0] and traces[(1, 1)][-1] != tr.NOMINAL[1]
    # stream 0 alone through a handle of its own, same launches: the stalled neighbour changes nothing
    with nv.Pipeline(n_streams=1, chain_mask=3, max_frames=1, push_mode=True, char_layer=False) as p:
        p.afc_enable(0, 0); p.afc_enable(0, 1)
        for i in range(total[0]):
            p.push(0, iqs[0][i * F:(i + 1) * F])
        p.push(0, iqs[0][total[0] * F:])
        p.finish()
        for c in (0, 1):
            assert p.afc_trace(0, c) == traces[(0, c)] and p.bits(0, c) == bits[(0, c)], c


# ---- 8. configuration
def test_resets_recentring_keep_and_groups(nv):
    iq = ar.segment(nv, nv.RATE_IN, 8, ar.FILLER, 25)
    F = nv.FRAME_IN
    buf = nv.DeviceBuffer(8 * F * 4)
    buf.upload(iq)
    kc = tr.NOMINAL[0]

    def launches(p, n, f0=0):
        for f in range(n):
            p.process_resident(buf, 8 * F, f0 + f, 1)
        p.fetch()
        return p.afc_trace(0, 0)
    with nv.Pipeline(n_streams=1, chain_mask=3, char_layer=False) as p:
        p.afc_enable(0, 0, gain_shift=0)
        first = launches(p, 8)
        assert first[:2] == [kc, kc] and first[-1] > kc + 3
        # nvx_stream_reset: the tracked k returns to the centre, tracking stays on, the same input tracks the same way
        p.stream_reset(0)
        st = p.afc_status(0, 0)
        assert (st["enabled"], st["k_last"], st["centre_k"], st["launches"]) == (1, kc, kc, 0) and p.carrier(0, 0) == (14000.0, True)
        assert launches(p, 8) == first
        p.reset()
        assert p.afc_status(0, 0)["enabled"] == 1 and launches(p, 8) == first
        # nvx_set_carrier on a tracking chain: the centre moves, tracking restarts there
        assert p.set_carrier(0, 0, 14012.5) == 14012.5
        st = p.afc_status(0, 0)
        assert (st["enabled"], st["centre_k"], st["k_last"], st["launches"]) == (1, kc + 4, kc + 4, 0) and p.carrier(0, 0) == (14012.5, False)
        p.reset()
        p.enable_signal_report(True)
        recs, again = [], []
        for f in range(8):                                # fetched one by one, for the launches' records
            p.process_resident(buf, 8 * F, f, 1); p.fetch()
            r = p.signal_report(0, 0, reset=True)
            recs.append({k: r[k] for k in REC})
            again += p.afc_trace(0, 0)
        K, _ = ar.trace(dict(ar.DEFAULTS, gain_shift=0), kc + 4, recs, 9)
        assert again == K[:8] and again[:2] == [kc + 4, kc + 4] and abs(again[-1] - first[-1]) <= 2
        # disable(keep = 1): the carrier stays where tracking had it -- the k the next launch would have run with
        p.afc_disable(0, 0, keep=True)
        kept = K[8]
        assert p.afc_status(0, 0)["enabled"] == 0 and p.carrier(0, 0) == (kept * 3.125, False) and kept > kc + 3
        p.enable_signal_report(False)
        # ... and a chain that tracked and was switched off with keep = 0 is back at its centre
        p.afc_enable(0, 1); launches(p, 3); p.afc_disable(0, 1, keep=False)
        assert p.carrier(0, 1) == (-14000.0, True) and p.carrier(0, 0) == (kept * 3.125, False)
    buf.free()
    with nv.Group([0, 0], n_streams=4, raw_rate=False, chain_mask=3, char_layer=False) as g:
        g.afc_enable(3, 1, range_k=7)
        m = g.member_of(3)
        assert g.afc_status(3, 1)["enabled"] == 1 and g.member_view(m).afc_status(3 - g.members[m][1], 1)["enabled"] == 1
        assert g.afc_status(0, 1)["enabled"] == 0 and g.afc_status(2, 1)["enabled"] == 0 and g.afc_trace(3, 1) == []
        g.afc_disable(3, 1, keep=True)
        assert g.afc_status(3, 1)["enabled"] == 0 and g.carrier(3, 1) == (-14000.0, True)
        for call in (lambda: g.afc_enable(4, 0), lambda: g.afc_disable(4, 0), lambda: g.afc_status(-1, 0), lambda: g.afc_trace(4, 0),
                     lambda: g.afc_enable(0, 2), lambda: g.afc_enable(0, 0, max_step=0)):
            with pytest.raises(nv.NvxError) as e:
                call()
            assert e.value.code == nv._native.ERR_ARG
