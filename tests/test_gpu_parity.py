"""GPU parity tests: the HIP path (through the C ABI) against the oracle on the
same seeded inputs.  Bar: 900 S/s FIR output bit-exact (fp64 bit patterns),
'B'/'Y' bits and decoded messages identical; delta-phi within 1 ulp of the
oracle's glibc atan2 (tolerance explained in DESIGN.md, "atan2")."""
import hashlib
from pathlib import Path

import numpy as np
import pytest

import signals

pytestmark = pytest.mark.gpu


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _two_carrier_stream(nv, rate):
    spb = rate // 100
    b518 = nv.sitor_encode("ZCZC EA01\nTEST MESSAGE 123 OK\nNNNN\n", 40)
    b490 = nv.sitor_encode("ZCZC GB42\nGALE WARNING 7/8 NW-LY.\nNNNN\n", 45)
    st = nv.make_stream([dict(freq_hz=14000, bits=b518, bit_offset=777 % spb, phase0=12345678),
                         dict(freq_hz=-14000, bits=b490, bit_offset=(1999 * (spb // 2520)) % spb, phase0=987654321,
                              amplitude=6000)], seed=7, noise_amp=1500)
    return st


@pytest.mark.parametrize("raw", [False, True], ids=["252k", "raw2016k"])
def test_single_stream_both_chains_y3_and_bits(nv, oracle, raw):
    """configs[1]/[2]: one IQ stream, 518 and 490 chains, several launches with carried state."""
    rate = nv.RATE_RAW if raw else nv.RATE_IN
    frame = nv.FRAME_RAW if raw else nv.FRAME_IN
    n_frames = 6 if raw else 60                       # 1.9 s / 19.2 s of signal
    iq = nv.synth_host(_two_carrier_stream(nv, rate), rate, n_frames * frame)

    ref = oracle.Pipe(chain_mask=3, tap_y3=n_frames * nv.FRAME_Y3)
    (ref.push_raw if raw else ref.push)(iq)

    with nv.Pipeline(n_streams=1, raw_rate=raw, max_frames=4, push_mode=True) as p:
        p.enable_debug(True)
        got_y3 = {0: [], 1: []}
        pos = 0
        # odd-sized pushes: launches happen whenever whole frames are staged
        rng = np.random.default_rng(3)
        while pos < iq.shape[0]:
            m = int(min(iq.shape[0] - pos, rng.integers(1, 3 * frame)))
            before = p.bit_count(0, 0)
            p.push(0, iq[pos:pos + m]); pos += m
        p.flush()
        for c in (0, 1):
            assert p.bits(0, c) == ref.bits(c), f"chain {c}: bit streams differ"
        assert len(p.bits(0, 0)) > (n_frames * 32 - 80)
        if not raw:
            msgs = sorted((f, b, m) for (_s, f, b, m) in p.messages)
            assert msgs == sorted(ref.messages)
            assert (518, "EA01", "ZCZC EA01\nTEST MESSAGE 123 OK\nNNNN\n") in msgs


@pytest.mark.parametrize("raw", [False, True], ids=["252k", "raw2016k"])
def test_y3_bitexact_one_launch(nv, oracle, raw):
    rate = nv.RATE_RAW if raw else nv.RATE_IN
    frame = nv.FRAME_RAW if raw else nv.FRAME_IN
    n_frames = 3
    iq = nv.synth_host(_two_carrier_stream(nv, rate), rate, n_frames * frame)
    ref = oracle.Pipe(chain_mask=3, tap_y3=n_frames * nv.FRAME_Y3, charlayer=False)
    (ref.push_raw if raw else ref.push)(iq)
    with nv.Pipeline(n_streams=1, raw_rate=raw, max_frames=n_frames, push_mode=True, char_layer=False) as p:
        p.enable_debug(True)
        p.push(0, iq)
        p.flush()
        for c in (0, 1):
            y3 = p.debug_y3(0, c)
            assert y3.shape[0] == n_frames * nv.FRAME_Y3
            assert np.array_equal(_u64(y3), _u64(ref.y3(c))), f"chain {c}: FIR cascade output not bit-exact"
            # discriminator: device atan2 is correctly rounded, glibc's is within 1 ulp of it
            bits_ref, dphi_ref = oracle.decode(ref.y3(c))
            dphi = p.debug_dphi(0, c)
            ulp = np.abs(_u64(dphi).astype(np.int64) - _u64(dphi_ref).astype(np.int64))
            assert ulp.max() <= 1, "delta-phi differs from glibc atan2 by more than 1 ulp"
            assert (ulp != 0).mean() < 5e-3
            # ... and bit-identical to the host build of the same nvx_atan2
            y = ref.y3(c)
            prev = np.vstack([[0.0, 0.0], y[:-1]])
            re = y[:, 0] * prev[:, 0] + y[:, 1] * prev[:, 1]
            im = y[:, 1] * prev[:, 0] - y[:, 0] * prev[:, 1]
            host = np.array([nv.lib.nvx_atan2_host(float(a), float(b)) for a, b in zip(im, re)])
            assert np.array_equal(_u64(dphi), _u64(host))
            assert p.bits(0, c) == bits_ref


def test_many_streams_single_chain(nv, oracle):
    """configs[3] shape at test size: independent one-chain streams, raw rate, mixed 518/490 chains."""
    n_streams, n_frames = 24, 3
    masks = [1 if s % 3 else 2 for s in range(n_streams)]
    streams, iqs = [], []
    for s in range(n_streams):
        st, _bits = signals.stream_params(nv, s, nv.RATE_RAW, freq_hz=14000 if masks[s] == 1 else -14000)
        streams.append(st)
        iqs.append(nv.synth_host(st, nv.RATE_RAW, n_frames * nv.FRAME_RAW))
    pitch = n_frames * nv.FRAME_RAW
    buf = nv.DeviceBuffer(n_streams * pitch * 4)
    nv.synth_device(streams, nv.RATE_RAW, pitch, buf, pitch)
    dev = buf.download(n_streams * pitch * 4, dtype=np.int16).reshape(n_streams, pitch, 2)
    for s in range(n_streams):
        assert np.array_equal(dev[s], iqs[s]), f"device generator differs from host generator on stream {s}"
    with nv.Pipeline(n_streams=n_streams, raw_rate=True, chain_masks=masks, max_frames=2, char_layer=False) as p:
        p.process_resident(buf, pitch, 0, 2)
        p.process_resident(buf, pitch, 2, 1)          # second launch continues from carried state
        p.fetch()
        for s in range(n_streams):
            c = 0 if masks[s] == 1 else 1
            ref = oracle.Pipe(chain_mask=masks[s], charlayer=False)
            ref.push_raw(iqs[s])
            assert p.bits(s, c) == ref.bits(c), f"stream {s}"
            assert p.bits(s, 1 - c) == ""
    buf.free()


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_randomized_configurations(nv, oracle, seed):
    """Random stream counts, chain masks (1, 2, 3 mixed -> both kernel instantiations), input rate,
    carrier offsets/levels and launch partitions; every chain of every stream against the oracle."""
    rng = np.random.default_rng(seed)
    raw = bool(rng.integers(0, 2))
    rate = nv.RATE_RAW if raw else nv.RATE_IN
    frame = nv.FRAME_RAW if raw else nv.FRAME_IN
    n_streams = int(rng.integers(1, 40 if raw else 70))
    n_frames = int(rng.integers(3, 6 if raw else 12))
    masks = [int(rng.choice([1, 2, 3])) for _ in range(n_streams)]
    if seed % 2:
        masks = [m if m != 3 else 1 for m in masks]            # exercise the single-chain kernel too
    spb = rate // 100
    iqs = []
    for s in range(n_streams):
        carriers = []
        for c, f in ((0, 14000), (1, -14000)):
            if (masks[s] >> c) & 1 or rng.random() < 0.3:       # sometimes a carrier nobody decodes
                carriers.append(dict(freq_hz=f + int(rng.integers(-10, 11)), bits=nv.sitor_encode(signals.stream_text(100 * seed + s), 8),
                                     bit_offset=int(rng.integers(0, spb)), phase0=int(rng.integers(0, 2**32)),
                                     amplitude=int(rng.integers(1500, 9000))))
        st = nv.make_stream(carriers, seed=1000 * seed + s, noise_amp=int(rng.integers(0, 4000)))
        iqs.append(nv.synth_host(st, rate, n_frames * frame))
    pitch = n_frames * frame + 4 * int(rng.integers(0, 64))
    buf = nv.DeviceBuffer(n_streams * pitch * 4)
    for s in range(n_streams):
        buf.upload(iqs[s], offset=s * pitch * 4)
    max_frames = int(rng.integers(1, n_frames + 1))
    with nv.Pipeline(n_streams=n_streams, raw_rate=raw, chain_masks=masks, max_frames=max_frames, char_layer=False) as p:
        f0 = 0
        while f0 < n_frames:
            k = int(min(n_frames - f0, rng.integers(1, max_frames + 1)))
            p.process_resident(buf, pitch, f0, k); f0 += k
        p.fetch()
        for s in range(n_streams):
            ref = oracle.Pipe(chain_mask=masks[s], charlayer=False)
            (ref.push_raw if raw else ref.push)(iqs[s])
            for c in range(2):
                want = ref.bits(c) if (masks[s] >> c) & 1 else ""
                assert p.bits(s, c) == want, f"seed {seed} stream {s} chain {c} mask {masks[s]} raw {raw}"
    buf.free()


def test_long_run_state_carry(nv, oracle):
    """100 s of signal through ~105 launches of 1-3 frames: FIR histories, the 567-deep
    correlation window, the sample counter g0 and the character layer never drift."""
    text = "ZCZC LR01\n" + "".join(f"LONG RUN LINE {i:02d} 0123456789\n" for i in range(12)) + "NNNN\n"
    bits_tx = nv.sitor_encode(text, 40)
    st = nv.make_stream([dict(freq_hz=14000, bits=bits_tx, bit_offset=1111, phase0=99)], seed=321, noise_amp=2500)
    n = 313 * nv.FRAME_IN                               # 100.2 s
    iq = nv.synth_host(st, nv.RATE_IN, n)
    ref = oracle.Pipe(chain_mask=1)
    ref.push(iq)
    with nv.Pipeline(n_streams=1, raw_rate=False, chain_mask=nv.CHAIN_518, max_frames=3, push_mode=True) as p:
        rng = np.random.default_rng(0)
        pos = 0
        while pos < n:
            m = int(min(n - pos, rng.integers(10000, 250000)))
            p.push(0, iq[pos:pos + m]); pos += m
        p.flush()
        assert p.bits(0, 0) == ref.bits(0) and len(ref.bits(0)) > 9900
        assert [(f, b, m) for (_s, f, b, m) in p.messages] == ref.messages and len(ref.messages) >= 1


def test_full_size_properties_config3(nv, oracle):
    """BASELINE configs[3] at full size (4096 streams x 2.016 MS/s, 12 frames = 127 GB in HBM), checked
    through size-independent properties: run-to-run determinism, identical streams decode identically,
    a different launch partition changes nothing, and a sample of streams matches the oracle bit for bit
    (test_full_size_total_parity_config3 compares ALL of them)."""
    S, F = 4096, 12
    pitch = F * nv.FRAME_RAW
    try:
        buf = nv.DeviceBuffer(S * pitch * 4)
    except nv.NvxError:
        pytest.skip("not enough device memory for the full-size batch")
    streams = [signals.stream_params(nv, s, nv.RATE_RAW)[0] for s in range(S)]
    twins = [(5, 4000), (77, 2049), (1023, 1024)]
    for a, b in twins:
        streams[b] = streams[a]
    nv.synth_device(streams, nv.RATE_RAW, pitch, buf, pitch)
    with nv.Pipeline(n_streams=S, raw_rate=True, chain_mask=nv.CHAIN_518, max_frames=F, char_layer=False) as p:
        runs = []
        for plan in ([12], [12], [5, 7]):
            p.reset()
            f0 = 0
            for k in plan:
                p.process_resident(buf, pitch, f0, k); f0 += k
            p.fetch()
            runs.append([p.bits(s, 0) for s in range(S)])
        assert runs[0] == runs[1], "two identical runs differ"
        assert runs[0] == runs[2], "launch partition changed the result"
        for a, b in twins:
            assert runs[0][a] == runs[0][b]
        assert min(len(b) for b in runs[0]) > 300
        for s in (0, 1, 4095, 2048, 3333):
            iq = buf.download(pitch * 4, offset=s * pitch * 4, dtype=np.int16).reshape(-1, 2)
            ref = oracle.Pipe(chain_mask=1, charlayer=False)
            ref.push_raw(iq)
            assert runs[0][s] == ref.bits(0), f"stream {s}"
    buf.free()


@pytest.mark.parametrize("raw", [False, True], ids=["252k", "raw2016k"])
def test_queue_handoff_stress(nv, oracle, raw):
    """Few streams x many frames in ONE launch: every (stream, frame) unit gets its own workgroup,
    so each stream is a 48-deep chain of agent-scope release/acquire hand-offs with all consumers
    spinning at once.  The complete 900 S/s output of every chain must be bit-exact."""
    rate = nv.RATE_RAW if raw else nv.RATE_IN
    frame = nv.FRAME_RAW if raw else nv.FRAME_IN
    n_streams, n_frames = (3, 24) if raw else (5, 48)
    masks = [3, 1, 2, 3, 1][:n_streams]
    iqs = []
    for s in range(n_streams):
        carriers = [dict(freq_hz=f, bits=nv.sitor_encode(signals.stream_text(900 + s), 10), bit_offset=(131 * (s + 1)) % (rate // 100),
                         phase0=s * 1234567, amplitude=5000) for f in (14000, -14000)]
        iqs.append(nv.synth_host(nv.make_stream(carriers, seed=50 + s, noise_amp=2000), rate, n_frames * frame))
    pitch = n_frames * frame
    buf = nv.DeviceBuffer(n_streams * pitch * 4)
    for s in range(n_streams):
        buf.upload(iqs[s], offset=s * pitch * 4)
    with nv.Pipeline(n_streams=n_streams, raw_rate=raw, chain_masks=masks, max_frames=n_frames, char_layer=False) as p:
        for rep in range(3):                               # repeat: L1-warm consumers on the later rounds
            p.reset()
            p.process_resident(buf, pitch, 0, n_frames)
            p.fetch()
            for s in range(n_streams):
                ref = oracle.Pipe(chain_mask=masks[s], charlayer=False, tap_y3=n_frames * nv.FRAME_Y3)
                (ref.push_raw if raw else ref.push)(iqs[s])
                for c in range(2):
                    if (masks[s] >> c) & 1:
                        assert np.array_equal(_u64(p.debug_y3(s, c)), _u64(ref.y3(c))), f"rep {rep} stream {s} chain {c}"
                        assert p.bits(s, c) == ref.bits(c)
    buf.free()


@pytest.mark.parametrize("baud", [99.6, 100.35, 101.2])
def test_baud_rate_drift_exercises_the_timing_slew(nv, oracle, baud):
    """A transmitter whose clock is off makes the bit timing walk: the slew limiter steps every few
    dozen bits and some bit periods hold two decisions or none.  Built with numpy (the library's generator
    has a fixed 100 baud), both chains carry FSK with the same drift; bits bit-exact against the oracle and
    the walk really happens (the bit count differs from the nominal 100 per second)."""
    frames = 24
    n = frames * nv.FRAME_IN
    rng = np.random.default_rng(int(baud * 100))
    t = np.arange(n)
    iq = rng.normal(size=(n, 2)) * 300.0
    for f0 in (14000.0, -14000.0):
        bits = rng.integers(0, 2, int(n * baud / nv.RATE_IN) + 2)
        shift = np.where(bits[(t * (baud / nv.RATE_IN)).astype(np.int64)] == 1, 85.0, -85.0)
        ph = 2 * np.pi * np.cumsum((f0 + shift) / nv.RATE_IN)
        iq += np.stack([np.cos(ph), np.sin(ph)], 1) * 6000.0
    iq = np.clip(np.round(iq), -32768, 32767).astype(np.int16)
    ref = oracle.Pipe(chain_mask=3, charlayer=False)
    ref.push(iq)
    with nv.Pipeline(n_streams=1, raw_rate=False, max_frames=5, push_mode=True, char_layer=False) as p:
        p.push(0, iq)
        p.flush()
        for c in (0, 1):
            want = ref.bits(c)
            assert p.bits(0, c) == want, f"chain {c}"
            nominal = frames * 32 - 66
            assert abs(len(want) - nominal * baud / 100.0) < 6 and len(want) != nominal


def _units_digest(nv, forms):
    h = hashlib.sha256()
    for raw in (False, True):
        for masks in ([1, 2, 1], [3, 1, 3]):
            rate = nv.RATE_RAW if raw else nv.RATE_IN
            frame = nv.FRAME_RAW if raw else nv.FRAME_IN
            streams = [signals.stream_params(nv, 500 + s, rate)[0] for s in range(3)]
            pitch = 10 * frame
            buf = nv.DeviceBuffer(3 * pitch * 4)
            nv.synth_device(streams, rate, pitch, buf, pitch)
            with nv.Pipeline(n_streams=3, raw_rate=raw, chain_masks=masks, max_frames=7, char_layer=False, forms=forms) as p:
                p.process_resident(buf, pitch, 0, 7); p.fetch()
                signals.assert_cascade_form(p, forms)
                for s in range(3):
                    for c in range(2):
                        if (masks[s] >> c) & 1: h.update(p.debug_y3(s, c).tobytes())
                p.process_resident(buf, pitch, 7, 3); p.fetch()
                signals.assert_cascade_form(p, forms)
                for s in range(3):
                    for c in range(2):
                        h.update(p.bits(s, c).encode())
                        if (masks[s] >> c) & 1: h.update(p.debug_y3(s, c).tobytes())
            buf.free()
    return h.hexdigest()


def test_dependent_and_independent_units_agree_bit_for_bit(nv):
    """The cascade has two ways to carry filter state across the frames of a launch: hand it from unit
    to unit (many streams) or let every unit rebuild it from the nine passes in front of it (few
    streams; chosen automatically).  Forced either way (signals.CASCADE_FORMS), the 900 S/s output and the bits
    of a 7-frame launch + a 3-frame launch are identical, for both input rates and both kernels."""
    digests = [_units_digest(nv, forms) for forms in signals.CASCADE_FORMS]
    assert digests[0] == digests[1] == digests[2] and len(digests[0]) == 64


RAILS_F, RAILS_F2 = 4, 2


def _rails_cases(nv, oracle):
    """(masks, samples, the oracle's pipes) of the one-chain and of the two-chain kernel"""
    F, F2 = RAILS_F, RAILS_F2
    n = (F + F2) * nv.FRAME_RAW
    rng = np.random.default_rng(77)
    cases = []
    for masks in ([1, 1, 2], [3, 2, 3]):
        S = len(masks)
        raw = rng.integers(-32768, 32768, size=(S, n, 2), dtype=np.int16)
        for s in range(S):
            at = 1000 + 977 * s
            raw[s, at:at + 70000] = 32767                              # both components at the positive rail
            raw[s, at + 100000:at + 170000] = -32768                   # ... the negative one
            raw[s, at + 200000:at + 230000, 0] = 32767; raw[s, at + 200000:at + 230000, 1] = -32768
            alt = np.where(np.arange(40000) & 1, 32767, -32768).astype(np.int16)
            raw[s, at + 300000:at + 340000, 0] = alt; raw[s, at + 300000:at + 340000, 1] = -1 - alt      # alternating rails, opposite signs
            # the rails across a frame (= unit) boundary and across the launch boundary
            raw[s, nv.FRAME_RAW - 5000:nv.FRAME_RAW + 5000] = -32768
            raw[s, F * nv.FRAME_RAW - 3000:F * nv.FRAME_RAW + 3000] = 32767
        refs = []
        for s in range(S):
            r = oracle.Pipe(chain_mask=masks[s], charlayer=False, tap_y3=(F + F2) * nv.FRAME_Y3)
            r.push_raw(raw[s])
            refs.append(r)
        cases.append((masks, raw, refs))
    return cases


def _rails_run(nv, cases, forms):
    F, F2 = RAILS_F, RAILS_F2
    n = (F + F2) * nv.FRAME_RAW
    checked = 0
    for masks, raw, refs in cases:
        S = len(masks)
        buf = nv.DeviceBuffer(S * n * 4)
        buf.upload(raw)
        with nv.Pipeline(n_streams=S, raw_rate=True, chain_masks=masks, max_frames=F, char_layer=False, forms=forms) as p:
            for f0, k in ((0, F), (F, F2)):
                p.process_resident(buf, n, f0, k); p.fetch()
                signals.assert_cascade_form(p, forms)
                for s in range(S):
                    for c in range(2):
                        if (masks[s] >> c) & 1:
                            want = np.ascontiguousarray(refs[s].y3(c)[f0 * nv.FRAME_Y3:(f0 + k) * nv.FRAME_Y3])
                            got = p.debug_y3(s, c)
                            assert got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64)), (masks, s, c, f0)
                            assert np.abs(want).max() > 10.0
                            checked += 1
            for s in range(S):
                for c in range(2):
                    assert p.bits(s, c) == (refs[s].bits(c) if (masks[s] >> c) & 1 else ""), (masks, s, c)
        buf.free()
    return checked


def test_full_scale_rails_through_the_raw_rate_stage0(nv, oracle):
    """The headline kernel's own stage 0 (SDWA half-word adds over the packed int16 pairs, nvx_cascade.hip) at the int16
    rails: uniform random samples over the whole range with stretches of +32767 and of -32768 on both components, mixed
    stretches and alternating rails (the sums of eight reach +-262 144 and round to the rails), through the one-chain and
    the two-chain raw-rate kernels, in the hand-over form (waiting and pre-rolling) and with independent units: the
    complete 900 S/s output as bit patterns and the bits == the oracle's raw-rate pipe (stage replaced:
    receiver/capt_sched.c:412-413, the vendor's /8 decimation; first consumer receiver/fir1cpp.C:80-136)."""
    cases = _rails_cases(nv, oracle)
    for forms in signals.CASCADE_FORMS + (signals.AUTOMATIC,):
        assert _rails_run(nv, cases, forms) == 16, forms


def _run_full_size_total(nv, oracle, S, F, ncpu, forms=None):
    """All S streams of a configs[3]-shaped batch against the oracle, bit for bit, in the cascade form `forms` forces (None:
    the launcher's own choice); returns (checked, bad, seconds, ties)."""
    import fullsize
    pitch = F * nv.FRAME_RAW
    buf = nv.DeviceBuffer(S * pitch * 4)
    streams = [signals.stream_params(nv, s, nv.RATE_RAW)[0] for s in range(S)]
    nv.synth_device(streams, nv.RATE_RAW, pitch, buf, pitch)
    with nv.Pipeline(n_streams=S, raw_rate=True, chain_mask=nv.CHAIN_518, max_frames=F, char_layer=False, forms=forms) as p:
        p.process_resident(buf, pitch, 0, F)
        p.fetch()
        if forms is not None:
            signals.assert_cascade_form(p, forms)
        checked, bad, secs = fullsize.verify_streams(oracle, buf, pitch, pitch, True, lambda s: p.bits(s, 0), range(S), ncpu)
        ties = p.tie_stats()
    buf.free()
    return checked, bad, secs, ties


def test_full_size_total_parity_config3(nv, oracle, tmp_path):
    """BASELINE configs[3] at full size: EVERY one of the 4096 streams' bits equals the oracle's (the batch is copied back
    in 64 chunks of 2 GB and decoded by the oracle with OpenMP) -- in the unit form the launcher picks at this size
    (hand-over between the frames of a stream) and, in a second process, with independent units forced.  No bit-timing
    decision of the whole batch is anywhere near a tie (nvx_demod_tie_stats)."""
    import os, subprocess, sys, json
    S, F = 4096, 12
    ncpu = min(16, len(os.sched_getaffinity(0)))
    try:
        checked, bad, secs, ties = _run_full_size_total(nv, oracle, S, F, ncpu)
    except nv.NvxError:
        pytest.skip("not enough device memory for the full-size batch")
    print(f"total parity: {checked} streams in {secs:.1f} s; ties {ties}")
    assert checked == S and bad == [], f"{len(bad)} of {checked} streams differ from the oracle: {bad[:20]}"
    near, evals, margin = ties
    assert near == 0 and evals > S * 250 and margin > 2.0 ** -40
    script = tmp_path / "indep.py"
    script.write_text('''
import sys, os, json
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import navtex_amd as nv, oracle_binding as ob, signals
import test_gpu_parity as T
checked, bad, secs, ties = T._run_full_size_total(nv, ob, 4096, 12, int(sys.argv[2]), signals.INDEPENDENT)
print(json.dumps({"checked": checked, "bad": bad[:20], "n_bad": len(bad), "secs": secs, "ties": ties}))
''')
    root = str(Path(__file__).resolve().parent.parent)
    out = subprocess.run([sys.executable, str(script), root, str(ncpu)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    assert rec["checked"] == S and rec["n_bad"] == 0, rec
    assert rec["ties"][0] == 0


def test_noise_only_has_no_near_tie(nv, oracle):
    """The golden noise-only case (the worst case for near-ties: no signal dominates the class sums): bits equal the
    compiled reference's, and the smallest relative margin of a timing decision is reported and far above 2^-40."""
    import json, cases
    gold = json.loads((Path(__file__).parent / "golden" / "golden.json").read_text())["iq"]["noise_only"]
    iq = cases.make_iq(nv, gold["spec"])
    with nv.Pipeline(n_streams=1, raw_rate=False, max_frames=4, push_mode=True, char_layer=False) as p:
        p.push(0, iq); p.finish()                        # the whole input, ended at its true length
        b518, b490 = p.bits(0, 0), p.bits(0, 1)
        near, evals, margin = p.tie_stats()
    assert b518 == gold["bits518"] and b490 == gold["bits490"] and len(b518) > 400
    print(f"noise only: {evals} timing evaluations, smallest relative margin {margin:.3e}")
    assert near == 0 and evals > 800 and margin > 1e-9


def test_three_carriers_resident_raw_rate_config2(nv, oracle):
    """BASELINE configs[2] through the roofline kernel form: three carriers in two 2.016 MS/s streams resident in HBM --
    stream 0 carries 518 (+14 kHz) and 490 (-14 kHz) with different texts, stream 1 the "4209.5 kHz" carrier at +14 kHz of
    its own centre, decoded by a 518-type chain under the label 4209 (the reference knows only 518 / 490:
    receiver/nav_sched.C:10-11).  Bits against the oracle, messages with their labels."""
    F = 62                                                        # 19.8 s
    n = F * nv.FRAME_RAW
    spb = nv.RATE_RAW // 100
    texts = {518: "ZCZC EA01\nTEST MESSAGE 123 OK\nNNNN\n", 490: "ZCZC GB42\nGALE WARNING 7/8 NW-LY.\nNNNN\n", 4209: "ZCZC QA07\nHF NAVTEX 4209.5\nNNNN\n"}
    s0 = nv.make_stream([dict(freq_hz=14000, bits=nv.sitor_encode(texts[518], 40), bit_offset=6217 % spb, phase0=11, amplitude=7000),
                         dict(freq_hz=-14000, bits=nv.sitor_encode(texts[490], 44), bit_offset=15991 % spb, phase0=22, amplitude=6000)], seed=3, noise_amp=1500)
    s1 = nv.make_stream([dict(freq_hz=14000, bits=nv.sitor_encode(texts[4209], 42), bit_offset=9001 % spb, phase0=33, amplitude=8000)], seed=4, noise_amp=1500)
    buf = nv.DeviceBuffer(2 * n * 4)
    nv.synth_device([s0, s1], nv.RATE_RAW, n, buf, n)
    with nv.Pipeline(n_streams=2, raw_rate=True, chain_masks=[3, 1], labels=[[518, 490], [4209, 0]], max_frames=16) as p:
        f0 = 0
        while f0 < F:
            k = min(16, F - f0)
            p.process_resident(buf, n, f0, k); f0 += k
        p.fetch()
        for s, st, mask in ((0, s0, 3), (1, s1, 1)):
            ref = oracle.Pipe(chain_mask=mask, charlayer=False)
            ref.push_raw(buf.download(n * 4, offset=s * n * 4, dtype=np.int16).reshape(-1, 2))
            for c in range(2):
                assert p.bits(s, c) == (ref.bits(c) if (mask >> c) & 1 else ""), f"stream {s} chain {c}"
        got = sorted((s, f, b, m) for (s, f, b, m) in p.messages)
        assert got == sorted([(0, 518, "EA01", texts[518]), (0, 490, "GB42", texts[490]), (1, 4209, "QA07", texts[4209])])
    buf.free()


def test_launches_on_different_streams_stay_ordered(nv, oracle):
    """nvx_process_resident takes a caller stream per call; the carried state (work queue, FIR histories, demodulator
    state) makes the launches of a handle sequential whatever streams they are given: calls alternate between two
    caller streams and the handle's own, and the result is that of one stream."""
    S, F = 40, 18
    masks = [3 if s % 4 == 0 else 1 for s in range(S)]
    pitch = F * nv.FRAME_IN
    streams = [signals.stream_params(nv, 300 + s, nv.RATE_IN)[0] for s in range(S)]
    buf = nv.DeviceBuffer(S * pitch * 4)
    nv.synth_device(streams, nv.RATE_IN, pitch, buf, pitch)
    sa, sb = nv.lib.nvx_stream_create(0), nv.lib.nvx_stream_create(0)
    assert sa and sb and sa != sb
    with nv.Pipeline(n_streams=S, raw_rate=False, chain_masks=masks, max_frames=2, char_layer=False) as p:
        for rep in range(3):
            p.reset()
            f0, k = 0, 0
            while f0 < F:
                n = 1 + (k % 2)
                n = min(n, F - f0)
                hs = (sa, None, sb)[k % 3]
                p.process_resident(buf, pitch, f0, n, hip_stream=hs); f0 += n; k += 1
            p.fetch()
            for s in range(0, S, 3):
                ref = oracle.Pipe(chain_mask=masks[s], charlayer=False)
                ref.push(nv.synth_host(streams[s], nv.RATE_IN, pitch))
                assert p.bits(s, 0) == ref.bits(0), f"round {rep} stream {s}"
    nv.lib.nvx_stream_destroy(0, sa); nv.lib.nvx_stream_destroy(0, sb)
    buf.free()


def _front_run(nv, forms):
    h = hashlib.sha256()
    masks = [1, 3, 2]
    streams = [signals.stream_params(nv, 900 + s, nv.RATE_IN, n_phasing=14)[0] for s in range(3)]
    F = 39
    buf = nv.DeviceBuffer(3 * F * nv.FRAME_IN * 4)
    nv.synth_device(streams, nv.RATE_IN, F * nv.FRAME_IN, buf, F * nv.FRAME_IN)
    with nv.Pipeline(n_streams=3, raw_rate=False, chain_masks=masks, max_frames=25, forms=forms) as p:
        p.enable_debug(True)
        f0 = 0
        for k in (4, 25, 9, 1):
            p.process_resident(buf, F * nv.FRAME_IN, f0, k); f0 += k
            p.fetch()
            signals.assert_front_form(p, forms, tiles_fit=k > 1)
            for s in range(3):
                for c in range(2):
                    if (masks[s] >> c) & 1: h.update(p.debug_dphi(s, c)[: k * nv.FRAME_Y3].tobytes())
        for s in range(3):
            for c in range(2): h.update(p.bits(s, c).encode())
        h.update(repr(sorted(p.messages)).encode()); h.update(repr(p.tie_stats()).encode())
        nbits = sum(len(p.bits(s, c)) for s in range(3) for c in range(2))
        n_messages = len(p.messages)
    buf.free()
    return h.hexdigest(), nbits, n_messages


def test_demodulator_front_forms_agree_bit_for_bit(nv):
    """The demodulator's front has two forms (r3): one workgroup per chain walking the tiles of a launch (many chains), or
    one workgroup per tile from the third tile on, each rebuilding its 577-sample look-back (few chains, long launches;
    chosen automatically).  Forced either way: delta-phi, bits and messages of launches of 4 + 25 + 9 + 1
    frames (one to six tiles, carried state in between) are identical, and so are the tie statistics."""
    outs = [_front_run(nv, forms) for forms in (signals.WALK, signals.TILES)]
    assert outs[0] == outs[1] and outs[0][1] > 4000, outs
