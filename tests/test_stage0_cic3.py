"""The third-order stage 0 (nvx_config.stage0_order = 3): three cascaded 8-sample boxcars decimated by 8.
Build-owned definition (the reference starts at 252 kS/s: receiver/capt_sched.c:31-34), so the chain of evidence is
    numpy restatement of the definition  ==  oracle (nvxo_stage0_cic3)            CPU tests below
    oracle stage 0 -> oracle pipeline (pinned to the compiled reference)  ==  HIP path    GPU tests below, bit for bit
plus what makes it worth having: its alias rejection at the NAVTEX offsets."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import signals

W3 = np.convolve(np.convolve(np.ones(8, dtype=np.int64), np.ones(8, dtype=np.int64)), np.ones(8, dtype=np.int64))


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------ CPU: the definition
def test_weights_are_three_boxcars():
    assert W3.tolist() == [1, 3, 6, 10, 15, 21, 28, 36, 42, 46, 48, 48, 46, 42, 36, 28, 21, 15, 10, 6, 3, 1] and W3.sum() == 512


@pytest.mark.parametrize("seed", [1, 2])
def test_oracle_matches_the_written_definition(oracle, seed):
    """out[m] = floor((sum_j w[j] x[8m+7-j] + 256) / 512), x[n<0] = 0, on full-scale noise (extremes included)."""
    rng = np.random.default_rng(seed)
    raw = rng.integers(-32768, 32768, size=(8 * 700, 2), dtype=np.int16)
    raw[100:140] = 32767; raw[300:340] = -32768                                # rails: the result must stay in int16
    x = np.vstack([np.zeros((14, 2), np.int64), raw.astype(np.int64)])
    want = np.empty((700, 2), np.int64)
    for m in range(700):
        seg = x[14 + 8 * m + 7 - 21: 14 + 8 * m + 8][::-1]                     # newest first
        want[m] = (seg * W3[:, None]).sum(0) + 256
    want = np.floor_divide(want, 512)
    got = oracle.stage0_cic3(raw)
    assert np.array_equal(got.astype(np.int64), want)
    assert got.max() == 32767 and got.min() == -32768


def test_oracle_history_makes_chunking_invisible(oracle):
    rng = np.random.default_rng(5)
    raw = rng.integers(-20000, 20000, size=(8 * 900, 2), dtype=np.int16)
    whole = oracle.stage0_cic3(raw)
    h = np.zeros((14, 2), np.int16)
    cuts = [0, 8, 16, 24, 800, 808, 4000, 7200]
    parts = [oracle.stage0_cic3(raw[a:b], h) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(np.vstack(parts), whole)
    assert np.array_equal(h, raw[-14:])


def test_alias_rejection_at_the_navtex_offsets(oracle):
    """What folds onto a carrier at +-14 kHz comes from m * 252 kHz +- 14 kHz.  Integrate-and-dump: 25 dB at the worst
    image; third-order form: three times that, also +-500 Hz around the carriers (the bar the round-1 review set: >= 60 dB
    at +-14 kHz +- 500 Hz).  Pass band (the carrier itself) unchanged to 0.1 dB."""
    fs, n = 2016000, 8 * 30000
    t = np.arange(n)

    def level(fn, f):
        z = np.round(20000 * np.exp(2j * np.pi * f * t / fs))
        y = fn(np.stack([z.real, z.imag], 1).astype(np.int16)).astype(float)
        return 20 * np.log10(max(np.sqrt((y[200:] ** 2).sum(1).mean()), 1e-9) / 20000)

    assert abs(level(oracle.stage0_cic3, 14000)) < 0.15 and abs(level(oracle.stage0_cic3, -14085)) < 0.15
    worst_box = max(level(oracle.stage0, f) for f in (252000 + 14000, 252000 - 14000, -252000 + 14085, 504000 - 14000))
    worst_cic = max(level(oracle.stage0_cic3, f) for f in (252000 + 14000, 252000 - 14000, -252000 + 14085, 504000 - 14000,
                                                            756000 + 14000, 1008000 - 14000,
                                                            252000 + 14500, 252000 - 14500, 252000 + 13500, -252000 - 14500))   # +-500 Hz around the carriers
    assert -26.5 < worst_box < -24.0
    assert worst_cic < -72.0


def test_pipe_with_third_order_stage0_is_stage0_then_pipe(oracle, nv):
    st = signals.stream_params(nv, 77, nv.RATE_RAW)[0]
    raw = nv.synth_host(st, nv.RATE_RAW, 4 * nv.FRAME_RAW)
    a = oracle.Pipe(chain_mask=1, charlayer=False); a.set_stage0(3)
    for lo, hi in ((0, 8 * 1000), (8 * 1000, 8 * 1001), (8 * 1001, raw.shape[0])):
        a.push_raw(raw[lo:hi])
    b = oracle.Pipe(chain_mask=1, charlayer=False)
    b.push(oracle.stage0_cic3(raw))
    assert a.bits(0) == b.bits(0) and len(a.bits(0)) > 40
    secs, bits = oracle.bench(raw[None], 1, 4 * nv.FRAME_IN, 3, 1, 1, want_bits=True)
    assert bits[0] == a.bits(0)


def test_config_errors_need_no_gpu(nv):
    """stage0_order is checked before any device call: 2 is no order, 3 needs raw-rate input."""
    from navtex_amd import _native as N
    for kw, frag in ((dict(raw_rate=1, stage0_order=2), "stage0_order"), (dict(raw_rate=0, stage0_order=3), "raw_rate"),
                     (dict(raw_rate=1, wideband=1, stage0_order=3), "raw_rate")):
        cfg = N.Config()
        nv.lib.nvx_config_default(C.byref(cfg))
        for k, v in kw.items(): setattr(cfg, k, v)
        h = C.c_void_p()
        assert nv.lib.nvx_create(C.byref(cfg), C.byref(h)) == N.ERR_ARG and not h.value
        assert frag in nv.lib.nvx_last_error().decode()


# ------------------------------------------------------------------------------------------------ GPU: the HIP path
def _two_carriers(nv):
    spb = nv.RATE_RAW // 100
    b518 = nv.sitor_encode("ZCZC EA01\nTEST MESSAGE 123 OK\nNNNN\n", 40)
    b490 = nv.sitor_encode("ZCZC GB42\nGALE WARNING 7/8 NW-LY.\nNNNN\n", 45)
    return nv.make_stream([dict(freq_hz=14000, bits=b518, bit_offset=777 % spb, phase0=12345678),
                           dict(freq_hz=-14000, bits=b490, bit_offset=1999 % spb, phase0=987654321, amplitude=6000)], seed=7, noise_amp=1500)


@pytest.mark.gpu
def test_y3_bitexact_and_bits_with_carried_state(nv, oracle):
    """One stream, both chains, odd-sized pushes (several launches): the 900 S/s output carries the fp64 bit patterns of
    oracle stage 0 -> oracle cascade, so the 22-tap sums, their two carried blocks and the rounding are the oracle's."""
    n_frames = 5
    iq = nv.synth_host(_two_carriers(nv), nv.RATE_RAW, n_frames * nv.FRAME_RAW)
    iq[1000:1100] = 32767; iq[5000:5050] = -32768                              # full scale through the dot products
    ref = oracle.Pipe(chain_mask=3, tap_y3=n_frames * nv.FRAME_Y3, charlayer=False)
    ref.set_stage0(3)
    ref.push_raw(iq)
    box = oracle.Pipe(chain_mask=3, charlayer=False)
    box.push_raw(iq)
    with nv.Pipeline(n_streams=1, raw_rate=True, max_frames=2, push_mode=True, char_layer=False, stage0_order=3) as p:
        p.enable_debug(True)
        rng = np.random.default_rng(11)
        pos, y3 = 0, {0: [], 1: []}
        while pos < iq.shape[0]:
            m = int(min(iq.shape[0] - pos, rng.integers(1, 2 * nv.FRAME_RAW)))
            p.push(0, iq[pos:pos + m]); pos += m
        p.flush()
        for c in (0, 1):
            assert p.bits(0, c) == ref.bits(c)
    # one launch: the whole y3 record
    with nv.Pipeline(n_streams=1, raw_rate=True, max_frames=n_frames, push_mode=True, char_layer=False, stage0_order=3) as p:
        p.enable_debug(True)
        p.push(0, iq); p.flush()
        for c in (0, 1):
            assert np.array_equal(_u64(p.debug_y3(0, c)), _u64(ref.y3(c))), f"chain {c}: not bit-exact"
    assert ref.bits(0) != "" and len(ref.bits(0)) == len(box.bits(0))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_randomized_configurations(nv, oracle, seed):
    """Random stream counts, chain masks (both kernels), carrier levels up to the rails, launch partitions with carried
    state; every chain of every stream against the oracle."""
    rng = np.random.default_rng(900 + seed)
    n_streams = int(rng.integers(1, 30))
    n_frames = int(rng.integers(3, 7))
    masks = [int(rng.choice([1, 2, 3])) for _ in range(n_streams)]
    if seed % 2: masks = [m if m != 3 else 2 for m in masks]
    spb = nv.RATE_RAW // 100
    iqs = []
    for s in range(n_streams):
        carriers = [dict(freq_hz=f + int(rng.integers(-10, 11)), bits=nv.sitor_encode(signals.stream_text(7 * seed + s), 8),
                         bit_offset=int(rng.integers(0, spb)), phase0=int(rng.integers(0, 2**32)), amplitude=int(rng.integers(1500, 14000)))
                    for c, f in ((0, 14000), (1, -14000)) if (masks[s] >> c) & 1 or rng.random() < 0.3]
        iqs.append(nv.synth_host(nv.make_stream(carriers, seed=5000 * seed + s, noise_amp=int(rng.integers(0, 6000))), nv.RATE_RAW, n_frames * nv.FRAME_RAW))
    pitch = n_frames * nv.FRAME_RAW + 4 * int(rng.integers(0, 64))
    buf = nv.DeviceBuffer(n_streams * pitch * 4)
    for s in range(n_streams): buf.upload(iqs[s], offset=s * pitch * 4)
    max_frames = int(rng.integers(1, n_frames + 1))
    with nv.Pipeline(n_streams=n_streams, raw_rate=True, chain_masks=masks, max_frames=max_frames, char_layer=False, stage0_order=3) as p:
        f0 = 0
        while f0 < n_frames:
            k = int(min(n_frames - f0, rng.integers(1, max_frames + 1)))
            p.process_resident(buf, pitch, f0, k); f0 += k
        p.fetch()
        for s in range(n_streams):
            ref = oracle.Pipe(chain_mask=masks[s], charlayer=False); ref.set_stage0(3)
            ref.push_raw(iqs[s])
            for c in range(2):
                assert p.bits(s, c) == (ref.bits(c) if (masks[s] >> c) & 1 else ""), f"seed {seed} stream {s} chain {c}"
    buf.free()


@pytest.mark.gpu
def test_hand_over_form_more_streams_than_resident_waves(nv, oracle):
    """3000 streams x 3 frames in launches of 2 + 1: more streams than the chip holds waves, so the frames of a stream go
    from unit to unit through the state block (the two carried blocks of stage 0 with them), and from launch to launch.
    A sample of streams against the oracle; twins identical."""
    S, F = 3000, 3
    streams = [signals.stream_params(nv, 20000 + s, nv.RATE_RAW)[0] for s in range(S)]
    streams[1777] = streams[5]
    pitch = F * nv.FRAME_RAW
    buf = nv.DeviceBuffer(S * pitch * 4)
    nv.synth_device(streams, nv.RATE_RAW, pitch, buf, pitch)
    with nv.Pipeline(n_streams=S, raw_rate=True, chain_mask=nv.CHAIN_518, max_frames=2, char_layer=False, stage0_order=3) as p:
        p.process_resident(buf, pitch, 0, 2)
        p.process_resident(buf, pitch, 2, 1)
        p.fetch()
        polls, units, launches = p.wait_stats()
        assert launches == 2
        assert p.bits(1777, 0) == p.bits(5, 0)
        for s in (0, 1, 5, 999, 1500, 2047, 2048, 2815, 2816, 2999):
            iq = buf.download(pitch * 4, offset=s * pitch * 4, dtype=np.int16).reshape(-1, 2)
            ref = oracle.Pipe(chain_mask=1, charlayer=False); ref.set_stage0(3)
            ref.push_raw(iq)
            assert p.bits(s, 0) == ref.bits(0), f"stream {s}"
    buf.free()


def _unit_forms_digest(nv, forms):
    h = hashlib.sha256()
    for masks in ([1, 2, 1], [3, 1, 3]):
        streams = [signals.stream_params(nv, 800 + s, nv.RATE_RAW)[0] for s in range(3)]
        pitch = 8 * nv.FRAME_RAW
        buf = nv.DeviceBuffer(3 * pitch * 4)
        nv.synth_device(streams, nv.RATE_RAW, pitch, buf, pitch)
        with nv.Pipeline(n_streams=3, raw_rate=True, chain_masks=masks, max_frames=5, char_layer=False, stage0_order=3, forms=forms) as p:
            p.enable_debug(True)
            p.process_resident(buf, pitch, 0, 5); p.fetch()
            signals.assert_cascade_form(p, forms)
            for s in range(3):
                for c in range(2):
                    if (masks[s] >> c) & 1: h.update(p.debug_y3(s, c).tobytes())
            p.process_resident(buf, pitch, 5, 3); p.fetch()
            signals.assert_cascade_form(p, forms)
            for s in range(3):
                for c in range(2): h.update(p.bits(s, c).encode())
        buf.free()
    return h.hexdigest()


@pytest.mark.gpu
def test_both_unit_forms_agree(nv):
    """Hand-over and independent units (nine-pass pre-roll in front of silence for stage 0's history), each forced:
    identical 900 S/s output and bits."""
    digests = [_unit_forms_digest(nv, forms) for forms in signals.CASCADE_FORMS]
    assert digests[0] == digests[1] == digests[2] and len(digests[0]) == 64


# The input of the rails test below, and the checks it runs in each unit form.
# CIC^3 geometry: a 1-KiB load is 256 raw samples (lane l holds 4l .. 4l+3: the pair 62 / 63 holds the
# last block, whose C and t cross to the next load by the wave rotation and to the next unit through the state block), a
# pass 2048, a frame 645 120 (a unit), a third 215 040 (a unit in a launch's last frame or in independent launches), the
# pre-roll 9 passes = 18 432 in front of a unit that rebuilds its histories.
LOAD, PRE = 256, 9 * 2048
RAILS3_F, RAILS3_F2 = 4, 2
HI, LO = 32767, -32768
ALT = np.where(np.arange(1 << 16) & 1, HI, LO).astype(np.int16)


def _rail(kind, m):
    """m samples of rail kind 0..4: both +full scale, both -full scale, I up / Q down, I down / Q up, alternating (I, Q opposite)."""
    if kind == 4:
        return np.stack([ALT[:m], -1 - ALT[:m]], 1)
    return np.tile(np.array([(HI, HI), (LO, LO), (HI, LO), (LO, HI)][kind], np.int16), (m, 1))


def _rails3_input(nv, rng, n, s):
    FR, THIRD = nv.FRAME_RAW, nv.FRAME_RAW // 3
    raw = rng.integers(LO, HI + 1, size=(n, 2), dtype=np.int16)            # full-range uniform noise
    at = 1000 + 977 * s
    for k in range(5):                                                      # long stretches of every kind of rail
        raw[at + 70000 * k:at + 70000 * k + 50000] = _rail(k, 50000)
    # samples 240 .. 271 of 600 consecutive loads: the last block pair of a load (lanes 60 .. 63) and the first of the next,
    # a different kind of rail from load to load, noise in between
    base = (at + 360000) // LOAD * LOAD
    for j in range(600):
        raw[base + LOAD * j + 240:base + LOAD * j + 272] = _rail(j % 5, 32)
    # a step from one rail to another exactly at every unit boundary (frames, thirds; the launch boundary is one of them)
    # and at the first sample of the pre-roll window in front of each
    for k in range(1, n // THIRD):
        for i, b in enumerate((k * THIRD, k * THIRD - PRE)):
            raw[b - 600:b] = _rail((k + i) % 5, 600); raw[b:b + 600] = _rail((k + i + 2) % 5, 600)
    # the carriers of both chains (+-14 kHz) as full-scale square waves: nothing but rails in the input, and 900 S/s output
    # near the largest the cascade can produce, across a frame boundary and a third-of-frame boundary
    t = np.arange(80000)
    for b, f in ((2 * FR, 14000), (3 * FR + THIRD, -14000)):
        ph = 2 * np.pi * f * (t + b) / nv.RATE_RAW
        raw[b - 40000:b + 40000] = np.stack([np.where(np.cos(ph) >= 0, HI, LO), np.where(np.sin(ph) >= 0, HI, LO)], 1)
    return raw


def _rails3_oracle_pipe(ob, mask, raw, n3):
    r = ob.Pipe(chain_mask=mask, charlayer=False, tap_y3=n3)
    r.set_stage0(3)
    r.push_raw(raw)
    for c in range(2):          # the full-scale carrier of each enabled chain reaches the 900 S/s output: |y3| ~ 35 600
        assert not (mask >> c) & 1 or np.abs(r.y3(c)).max() > 30000.0, (mask, c)
    return r


def _same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64)), (what, got.shape, want.shape)
    assert np.abs(want).max() > 300.0, what                                 # not near-silence: the noise alone gives ~700 per frame


def _rails3_cases(nv, ob):
    """The inputs with the oracle's pipes over them, computed once for every unit form: (masks, samples, pipes) of the
    resident runs, (masks, samples, pipes, pushes as (stream, samples)) of the push-mode runs."""
    FR, FY = nv.FRAME_RAW, nv.FRAME_Y3
    rng = np.random.default_rng(303)
    resident, pushed = [], []
    n = (RAILS3_F + RAILS3_F2) * FR
    for masks in ([1, 1, 2], [3, 2, 3]):                                    # the one-chain and the two-chain kernel
        raw = np.stack([_rails3_input(nv, rng, n, s) for s in range(len(masks))])
        y0 = ob.stage0_cic3(raw[0])
        assert y0.max() == HI and y0.min() == LO, (y0.min(), y0.max())      # stage 0 reaches the rails
        resident.append((masks, raw, [_rails3_oracle_pipe(ob, m, raw[s], (RAILS3_F + RAILS3_F2) * FY) for s, m in enumerate(masks)]))
    n = 4 * FR
    for masks in ([1, 2], [3, 1]):
        S = len(masks)
        raw = np.stack([_rails3_input(nv, rng, n, s) for s in range(S)])
        refs = [_rails3_oracle_pipe(ob, masks[s], raw[s], 4 * FY) for s in range(S)]
        pos, plan = [0] * S, []
        while min(pos) < n:                                                 # ragged pushes, the streams in random order
            s = int(rng.integers(0, S)) if max(pos) < n else pos.index(min(pos))
            if pos[s] >= n:
                continue
            m = int(min(n - pos[s], rng.choice([1, 7, 255, 257, 2047, 2049, 18433, int(rng.integers(1, FR))])))   # < a frame: one launch at most
            plan.append((s, m)); pos[s] += m
        pushed.append((masks, raw, refs, plan))
    return resident, pushed


def _rails3_run(nv, cases, forms):
    FR, FY = nv.FRAME_RAW, nv.FRAME_Y3
    F, F2 = RAILS3_F, RAILS3_F2
    resident, pushed = cases
    checked_resident = 0
    n = (F + F2) * FR
    for masks, raw, refs in resident:
        S = len(masks)
        buf = nv.DeviceBuffer(S * n * 4)
        buf.upload(raw)
        with nv.Pipeline(n_streams=S, raw_rate=True, chain_masks=masks, max_frames=F, char_layer=False, stage0_order=3, forms=forms) as p:
            for f0, k in ((0, F), (F, F2)):
                p.process_resident(buf, n, f0, k); p.fetch()
                signals.assert_cascade_form(p, forms)
                for s in range(S):
                    for c in range(2):
                        if (masks[s] >> c) & 1:
                            _same(p.debug_y3(s, c), np.ascontiguousarray(refs[s].y3(c)[f0 * FY:(f0 + k) * FY]), (masks, s, c, f0))
                            checked_resident += 1
            for s in range(S):
                for c in range(2):
                    assert p.bits(s, c) == (refs[s].bits(c) if (masks[s] >> c) & 1 else ""), (masks, s, c)
        buf.free()

    # push mode, ragged pushes, streams launched as soon as each has a frame (eager_launch): the streams come apart in time, so
    # the launches name their streams -- the list kernels -- and every launch is held against the oracle right after its push
    checked_push = 0
    for masks, raw, refs, plan in pushed:
        S = len(masks)
        with nv.Pipeline(n_streams=S, raw_rate=True, chain_masks=masks, max_frames=2, push_mode=True, eager_launch=True,
                         char_layer=False, stage0_order=3, forms=forms) as p:
            pos = [0] * S
            seen = [[0, 0] for _ in range(S)]                               # frames checked per (stream, chain)
            for s, m in plan:
                before = [p.stream_stats(t)[1] for t in range(S)]
                p.push(s, raw[s, pos[s]:pos[s] + m]); pos[s] += m
                for t in range(S):
                    after = p.stream_stats(t)[1]
                    if after == before[t]:
                        continue
                    signals.assert_cascade_form(p, forms)
                    for c in range(2):
                        if (masks[t] >> c) & 1:
                            _same(p.debug_y3(t, c), np.ascontiguousarray(refs[t].y3(c)[before[t] * FY:after * FY]), (masks, t, c, before[t]))
                            seen[t][c] += after - before[t]
            p.flush()
            assert [p.stream_stats(t)[1] for t in range(S)] == [4] * S
            assert p.stream_stats(0)[2] > 0, "no launch named its streams: the list kernels were not run"
            for t in range(S):
                for c in range(2):
                    assert seen[t][c] == (4 if (masks[t] >> c) & 1 else 0), (masks, t, c, seen[t][c])
                    checked_push += seen[t][c]
                    assert p.bits(t, c) == (refs[t].bits(c) if (masks[t] >> c) & 1 else ""), (masks, t, c)
    return checked_resident, checked_push


@pytest.mark.gpu
def test_full_scale_rails_through_every_third_order_kernel_and_unit_form(nv, oracle):
    """The third-order stage 0 at the int16 rails, every one of its four kernels, in every unit form, against the oracle:
    full-range noise with long stretches of each kind of rail; rails over samples 240 .. 271 of 600 consecutive loads
    (the lane pair 62 / 63 whose C and t the wave rotation and the state block carry on); a step from one rail to another
    exactly at every frame, third-of-frame and launch boundary and at the first sample of every pre-roll window.  Resident
    input through the one- and two-chain kernels (two launches), and host input in ragged pushes through the list kernels:
    every launch's 900 S/s output as fp64 bit patterns and the bits == oracle stage 0 -> oracle cascade.  Waiting and
    pre-rolling hand-over, independent units, and the launcher's own choice."""
    cases = _rails3_cases(nv, oracle)
    for forms in signals.CASCADE_FORMS + (signals.AUTOMATIC,):
        # resident: (3 + 5 enabled chains) x 2 launches; push: (2 + 3 enabled chains) x 4 frames
        assert _rails3_run(nv, cases, forms) == (16, 20), forms
