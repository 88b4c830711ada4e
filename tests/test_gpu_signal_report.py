"""Per-chain signal reports (include/navtex_amd_signal.h) on the GPU (-m gpu).

Every report is held against the numpy restatement (tests/signal_ref.py) on the device's OWN y3 and delta-phi, collected
launch by launch with the debug taps (timing_ref.DeviceTaps): the counts equal, every sum within 1e-12 of the sum of its
terms' magnitudes, the derived fields the header's formulas of the returned sums.  Covered: 252 kS/s resident, raw rate
in both stage-0 forms, push mode with ragged ends (tails below and around g = 8), a wideband handle, both front forms
(each bit-identical across two runs), bits and messages unchanged by reports, the read / reset / enable semantics, the
physical checks of tests/test_signal_report.py on decoded streams, the headline scale and a group."""
import numpy as np
import pytest

import signal_ref as sr
import signals
import timing_ref as tr

pytestmark = pytest.mark.gpu


def check_reports(oracle, p, taps, reset=False):
    """Every chain `taps` collected: the handle's report against the restatement over the chain's samples since reset."""
    fR, fI = oracle.bitfilter_table()
    total = 0
    for sc in taps.chains:
        d = taps.chain(sc)
        want = sr.report(d["y3"], d["dphi"], fR, fI)
        got = p.signal_report(*sc, reset=reset)
        sr.check_sums(got, want, where=f"stream {sc[0]} chain {sc[1]}")
        sr.check_derived(got)
        total += got["samples"]
    return total


def _resident(nv, raw, order, masks, n_frames, launches, seed):
    rate = nv.RATE_RAW if raw else nv.RATE_IN
    frame = nv.FRAME_RAW if raw else nv.FRAME_IN
    pitch = n_frames * frame
    buf = nv.DeviceBuffer(len(masks) * pitch * 4)
    rng = np.random.default_rng(seed)
    for s in range(len(masks)):
        st, _ = signals.stream_params(nv, seed + s, rate, freq_hz=int(rng.choice([14000, -14000])) + int(rng.integers(-20, 21)),
                                      noise_amp=int(rng.integers(0, 6000)))
        buf.upload(nv.synth_host(st, rate, pitch), offset=s * pitch * 4)
    return buf, pitch


@pytest.mark.parametrize("raw,order", [(False, 1), (True, 1), (True, 3)], ids=["252k", "raw_cic1", "raw_cic3"])
def test_resident_reports_equal_the_restatement(nv, oracle, raw, order):
    masks = [3, 1, 2, 3]
    buf, pitch = _resident(nv, raw, order, masks, 12, None, 500 + 2 * raw + order)
    with nv.Pipeline(n_streams=len(masks), raw_rate=raw, chain_masks=masks, max_frames=6, char_layer=False, stage0_order=order) as p:
        p.enable_debug(True)
        p.enable_signal_report(True)
        taps = tr.DeviceTaps(p, [(s, c) for s in range(len(masks)) for c in range(2) if (masks[s] >> c) & 1], push_mode=False)
        f0 = 0
        for k in (1, 5, 2, 4):
            taps.launch(lambda: p.process_resident(buf, pitch, f0, k)); f0 += k
        total = check_reports(oracle, p, taps)
        for s, m in enumerate(masks):                     # a chain outside its stream's mask reports nothing
            for c in range(2):
                if not (m >> c) & 1:
                    r = p.signal_report(s, c)
                    assert r["samples"] == 0 and np.isnan(r["power_db"]) and np.isnan(r["offset_hz"])
    buf.free()
    assert total == 6 * (12 * nv.FRAME_Y3 - sr.G_DAB)


@pytest.mark.parametrize("n3s", [(7, 8, 9), (290, 300, 575), (2592, 2593, 2600)], ids=["below_8", "one_frame", "nine_frames"])
def test_push_mode_ragged_ends_equal_the_restatement(nv, oracle, n3s):
    """Push-mode streams ended by nvx_finish at 900 S/s counts below, at and just above g = 8, and ragged ones later on
    (the streams of a case have the same whole frames: one launch of those, then one that ends every stream at its n3)."""
    frames = max(n // 288 for n in n3s)
    with nv.Pipeline(n_streams=len(n3s), raw_rate=False, chain_mask=3, max_frames=max(frames, 1), push_mode=True, char_layer=False) as p:
        p.enable_debug(True)
        p.enable_signal_report(True)
        taps = tr.DeviceTaps(p, [(s, c) for s in range(len(n3s)) for c in range(2)], push_mode=True)
        iqs = [nv.synth_host(signals.stream_params(nv, 80 + n3, nv.RATE_IN)[0], nv.RATE_IN, n3 * 280 + 139) for n3 in n3s]
        for s, iq in enumerate(iqs[:-1]):
            p.push(s, iq)
        taps.launch(lambda: p.push(len(iqs) - 1, iqs[-1]), launches=int(frames > 0))
        taps.launch(p.finish, launches=int(any(n % 288 for n in n3s)))
        check_reports(oracle, p, taps)
        for s, n3 in enumerate(n3s):
            assert p.signal_report(s, 0)["samples"] == max(0, n3 - sr.G_DAB)


def test_wideband_reports_equal_the_restatement(nv, oracle):
    F = 5
    n = F * nv.FRAME_RAW
    car = [dict(freq_hz=(k * 252000 if k < 4 else (k - 8) * 252000) + off, bits=nv.sitor_encode(f"ZCZC SR{k}{c}\nREPORT\nNNNN\n", 6),
                bit_offset=613 * (2 * k + c + 1), phase0=7654321 * (2 * k + c + 1) % 2**32, amplitude=1500)
           for k in range(8) for c, off in ((0, 14000 + 3 * k), (1, -14000 - 2 * k))]
    raw = nv.synth_host(nv.make_stream(car, seed=78, noise_amp=500), nv.RATE_RAW, n)
    buf = nv.DeviceBuffer(n * 4)
    buf.upload(raw)
    with nv.Pipeline(n_streams=1, wideband=True, chain_mask=3, max_frames=3, char_layer=False) as p:
        p.enable_debug(True)
        p.enable_signal_report(True)
        taps = tr.DeviceTaps(p, [(s, c) for s in range(8) for c in range(2)], push_mode=False)
        for f0, k in ((0, 3), (3, 2)):
            taps.launch(lambda: p.process_resident(buf, n, f0, k))
        total = check_reports(oracle, p, taps)
    buf.free()
    assert total == 16 * (F * nv.FRAME_Y3 - sr.G_DAB)


def _front_form_reports(nv, oracle, buf, F, forms):
    """(samples reported, {chain: report with its floats as hex}) of launches of 1, 4, 25 and 9 frames in the front form `forms` forces"""
    masks = [1, 3, 2]
    with nv.Pipeline(n_streams=3, raw_rate=False, chain_masks=masks, max_frames=25, forms=forms) as p:
        p.enable_debug(True)
        p.enable_signal_report(True)
        chains = [(s, c) for s in range(3) for c in range(2) if (masks[s] >> c) & 1]
        taps = tr.DeviceTaps(p, chains, push_mode=False)
        f0 = 0
        for k in (1, 4, 25, 9):
            taps.launch(lambda: p.process_resident(buf, F * nv.FRAME_IN, f0, k)); f0 += k
            signals.assert_front_form(p, forms, tiles_fit=k > 1)
        total = check_reports(oracle, p, taps)
        reps = {f"{s}/{c}": {k: float(v).hex() if isinstance(v, float) else v for k, v in p.signal_report(s, c).items()} for s, c in chains}
    return total, reps


def test_both_front_forms_equal_the_restatement_and_repeat_bit_for_bit(nv, oracle):
    """The walk and head + tiles, each forced, twice: launches of 1, 4, 25 and 9 frames
    (with tiles forced three of them take the tile form).  Each run equals the restatement; the two runs of a form agree in
    every bit of every field."""
    streams = [signals.stream_params(nv, 950 + s, nv.RATE_IN, n_phasing=14)[0] for s in range(3)]
    F = 39
    buf = nv.DeviceBuffer(3 * F * nv.FRAME_IN * 4)
    nv.synth_device(streams, nv.RATE_IN, F * nv.FRAME_IN, buf, F * nv.FRAME_IN)
    seen = {}
    for forms in (signals.WALK, signals.TILES):
        runs = []
        for _ in range(2):
            total, reps = _front_form_reports(nv, oracle, buf, F, forms)
            assert total == 4 * (39 * 288 - 8)
            runs.append(reps)
        assert runs[0] == runs[1], f"forms {forms}: two runs differ"
        seen[forms] = runs[0]
    buf.free()
    for k in seen[signals.WALK]:                            # the forms count the same samples (their sums may differ in the last bits)
        assert seen[signals.WALK][k]["samples"] == seen[signals.TILES][k]["samples"] and seen[signals.WALK][k]["b_samples"] == seen[signals.TILES][k]["b_samples"]


def test_reports_change_no_bit_and_no_message(nv, oracle):
    """The same raw-rate input (a short message on each chain) through a handle with reports on and one with them off, and
    through the oracle: the same bits on both chains and the same messages."""
    n_frames = 26
    car = [dict(freq_hz=f, bits=nv.sitor_encode(f"ZCZC SR{c:02d}\nREPORT {c}\nNNNN\n", 12), bit_offset=1001 + 500 * c, phase0=77 + c,
                amplitude=6000) for c, f in ((0, 14000), (1, -14000))]
    iq = nv.synth_host(nv.make_stream(car, seed=31, noise_amp=1200), nv.RATE_RAW, n_frames * nv.FRAME_RAW)
    out = []
    for on in (False, True):
        with nv.Pipeline(n_streams=1, raw_rate=True, chain_mask=3, max_frames=8, push_mode=True) as p:
            if on:
                p.enable_signal_report(True)
            p.push(0, iq)
            p.flush()
            out.append((p.bits(0, 0), p.bits(0, 1), sorted((f, b, t) for _, f, b, t in p.messages)))
            if on:
                assert p.signal_report(0, 0)["samples"] == n_frames * nv.FRAME_Y3 - sr.G_DAB
    ref = oracle.Pipe(chain_mask=3)
    ref.push_raw(iq)
    assert out[0] == out[1]
    assert out[0][0] == ref.bits(0) and out[0][1] == ref.bits(1) and len(out[0][0]) > 700
    assert out[0][2] == sorted(ref.messages) and len(out[0][2]) == 2


def _same(a: dict, b: dict) -> bool:
    return all(a[k] == b[k] or (isinstance(a[k], float) and np.isnan(a[k]) and np.isnan(b[k])) for k in a)


def test_read_reset_stream_reset_disable_and_enable_mid_stream(nv, oracle):
    buf, pitch = _resident(nv, False, 1, [3, 3], 6, None, 640)
    fR, fI = oracle.bitfilter_table()
    with nv.Pipeline(n_streams=2, raw_rate=False, chain_mask=3, max_frames=2, char_layer=False) as p:
        with pytest.raises(nv.NvxError) as e:
            p.signal_report(0, 0)                              # off by default
        assert e.value.code == nv._native.ERR_STATE
        p.enable_debug(True)
        taps = tr.DeviceTaps(p, [(0, 0), (0, 1), (1, 0), (1, 1)], push_mode=False)
        taps.launch(lambda: p.process_resident(buf, pitch, 0, 2))          # launched while off: never counted
        p.enable_signal_report(True)
        taps.launch(lambda: p.process_resident(buf, pitch, 2, 2))
        n1 = 2 * nv.FRAME_Y3
        for sc in taps.chains:                                 # the later launch alone, its windows reaching into the first
            d = taps.chain(sc)
            got = p.signal_report(*sc)
            sr.check_sums(got, sr.report(d["y3"], d["dphi"], fR, fI, start=n1), where=str(sc))
            sr.check_derived(got)
            assert got["samples"] == n1
            assert _same(p.signal_report(*sc, reset=True), got)
            z = p.signal_report(*sc)
            assert z["samples"] == 0 and z["b_samples"] == 0 and z["sum_power"] == 0.0 and np.isnan(z["power_db"])
        taps.launch(lambda: p.process_resident(buf, pitch, 4, 2))
        before = {sc: p.signal_report(*sc) for sc in taps.chains}
        for sc in taps.chains:                                 # read with reset: the launch after it only
            d = taps.chain(sc)
            sr.check_sums(before[sc], sr.report(d["y3"], d["dphi"], fR, fI, start=2 * n1), where=str(sc))
        p.stream_reset(1)                                      # that stream only
        assert p.signal_report(1, 0)["samples"] == 0 and p.signal_report(1, 1)["samples"] == 0
        assert _same(p.signal_report(0, 0), before[(0, 0)]) and _same(p.signal_report(0, 1), before[(0, 1)])
        p.enable_signal_report(False)
        with pytest.raises(nv.NvxError) as e:
            p.signal_report(0, 0)
        assert e.value.code == nv._native.ERR_STATE
        p.enable_signal_report(True)
        assert p.signal_report(0, 0)["samples"] == 0            # off dropped what was summed
        p.process_resident(buf, pitch, 0, 2)
        p.fetch()
        assert p.signal_report(0, 0)["samples"] > 0
        p.reset()
        assert p.signal_report(0, 0)["samples"] == 0 and p.signal_report(1, 1)["samples"] == 0
        for bad in ((2, 0), (-1, 0), (0, 2)):
            with pytest.raises(nv.NvxError) as e:
                p.signal_report(*bad)
            assert e.value.code == nv._native.ERR_ARG
    buf.free()


def test_a_stalled_stream_does_not_advance(nv, oracle):
    """Independent streams of a push-mode handle: stream 1 stops delivering, stream 0 goes on; only stream 0's report grows."""
    st = [signals.stream_params(nv, 700 + s, nv.RATE_IN)[0] for s in range(2)]
    iq = [nv.synth_host(s, nv.RATE_IN, 4 * nv.FRAME_IN) for s in st]
    with nv.Pipeline(n_streams=2, raw_rate=False, chain_mask=3, max_frames=2, push_mode=True, char_layer=False) as p:
        p.enable_signal_report(True)
        p.push(0, iq[0][:2 * nv.FRAME_IN]); p.push(1, iq[1][:2 * nv.FRAME_IN]); p.flush(); p.fetch()
        first = [p.signal_report(s, 0)["samples"] for s in range(2)]
        assert first == [2 * nv.FRAME_Y3 - sr.G_DAB] * 2
        p.set_active(1, False)
        p.push(0, iq[0][2 * nv.FRAME_IN:]); p.flush(); p.fetch()
        assert p.signal_report(0, 0)["samples"] == 4 * nv.FRAME_Y3 - sr.G_DAB
        assert p.signal_report(1, 0)["samples"] == first[1] and p.signal_report(1, 1)["samples"] == first[1]


@pytest.mark.parametrize("rate", [252000, 2016000])
def test_estimator_on_decoded_streams(nv, rate):
    """tests/test_signal_report.py's physical checks with the same tolerances, on the device's reports."""
    cache = {}

    def reports(chain, **kw):
        key = tuple(sorted(kw.items()))
        if key not in cache:
            iq, frames = sr.synth(nv, rate, **kw)
            with nv.Pipeline(n_streams=1, raw_rate=rate == nv.RATE_RAW, chain_mask=3, max_frames=16, push_mode=True, char_layer=False) as p:
                p.enable_signal_report(True)
                p.push(0, iq)
                p.flush()
                p.fetch()
                cache[key] = [p.signal_report(0, c) for c in (0, 1)]
                assert cache[key][0]["samples"] == frames * nv.FRAME_Y3 - sr.G_DAB
        return cache[key][chain]
    sr.check_physics(reports)


def test_headline_scale(nv, oracle):
    """4096 streams at the raw rate x 12 frames, reports on: every chain counts its samples; the bits are those of the same
    run with reports off; 64 chains spread over the handle equal the restatement."""
    S, F = 4096, 12
    pitch = F * nv.FRAME_RAW
    buf = nv.DeviceBuffer(S * pitch * 4)
    nv.synth_device([signals.stream_params(nv, s, nv.RATE_RAW)[0] for s in range(S)], nv.RATE_RAW, pitch, buf, pitch)
    spread = [(int(s), 0) for s in np.linspace(0, S - 1, 64).astype(int)]
    bits = []
    for on in (False, True):
        with nv.Pipeline(n_streams=S, raw_rate=True, chain_mask=nv.CHAIN_518, max_frames=F, char_layer=False) as p:
            if on:
                p.enable_debug(True)
                p.enable_signal_report(True)
                taps = tr.DeviceTaps(p, spread, push_mode=False)
                taps.launch(lambda: p.process_resident(buf, pitch, 0, F))
                for s in range(S):
                    assert p.signal_report(s, 0)["samples"] == F * nv.FRAME_Y3 - sr.G_DAB, s
                check_reports(oracle, p, taps)
            else:
                p.process_resident(buf, pitch, 0, F)
                p.fetch()
            bits.append([p.bits(s, 0) for s in range(0, S, 17)])
    buf.free()
    assert bits[0] == bits[1]


def test_group_report_is_the_member_handles(nv):
    S, F = 6, 3
    masks = [3] * S
    with nv.Group([0, 0], n_streams=S, chain_masks=masks, max_frames=F, char_layer=False, push_mode=True) as g:
        g.enable_signal_report(True)
        for s in range(S):
            g.push(s, nv.synth_host(signals.stream_params(nv, 810 + s, nv.RATE_IN)[0], nv.RATE_IN, F * nv.FRAME_IN))
        g.flush()
        g.fetch()
        for s in range(S):
            m = g.member_of(s)
            local = s - g.members[m][1]
            for c in (0, 1):
                a = g.signal_report(s, c)
                b = g.member_view(m).signal_report(local, c)
                assert _same(a, b)
                assert a["samples"] == F * nv.FRAME_Y3 - sr.G_DAB
