"""Per-chain carrier tuning (include/navtex_amd_tune.h) on the GPU (-m gpu): y3 and bits of every tuned chain
bit-identical to the restatement (tests/tune_ref.py) in every kernel form, nominal chains bit-identical to an untuned
handle's, messages on carriers the reference mixer cannot decode, retuning at a frame boundary, scale, groups, errors
and signal reports against the tuned carrier."""
import hashlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import signal_ref as sr
import signals
import tune_ref as tr

pytestmark = pytest.mark.gpu


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _iq(nv, rate, frames, sid, freq_hz=14000, text=None):
    st, _ = signals.stream_params(nv, sid, rate, freq_hz=freq_hz, text=text)
    frame = nv.FRAME_RAW if rate == nv.RATE_RAW else nv.FRAME_IN
    return nv.synth_host(st, rate, frames * frame)


# (stream masks, {(stream, chain): offset Hz}): two-chain streams with a different k per chain, negative k, k = 0, k
# coprime to N (4481 * 3.125 Hz), one stream with a nominal chain beside a tuned one, a one-chain stream
CASE2 = ([3, 3, 1], {(0, 0): 3000.0, (0, 1): -9000.0, (1, 1): 4481 * 3.125, (2, 0): 0.0})
CASE1 = ([1, 2, 1], {(0, 0): -9000.0, (1, 1): 4481 * 3.125, (2, 0): 19000.0})


def _run(nv, raw, s0, masks, tune, frames=3, launches=(3,), forms=None):
    """Launch a handle over streams 500.. with `tune` applied, in the cascade form `forms` forces (None: the launcher's own);
    returns (y3 per launch per slot, bits per slot, iqs)."""
    rate = nv.RATE_RAW if raw else nv.RATE_IN
    frame = nv.FRAME_RAW if raw else nv.FRAME_IN
    n = len(masks)
    iqs = [_iq(nv, rate, frames, 500 + s, freq_hz=[14000, -14000, 3000][s % 3]) for s in range(n)]
    pitch = frames * frame
    buf = nv.DeviceBuffer(n * pitch * 4)
    for s in range(n):
        buf.upload(iqs[s], s * pitch * 4)
    y3s, bits = {}, {}
    with nv.Pipeline(n_streams=n, raw_rate=raw, chain_masks=masks, max_frames=max(launches), char_layer=False, stage0_order=s0, forms=forms) as p:
        for (s, c), hz in tune.items():
            assert p.set_carrier(s, c, hz) == tr.k_of(hz) * 3.125
        f0 = 0
        for nf in launches:
            p.process_resident(buf, pitch, f0, nf)
            p.fetch()
            if forms is not None:
                signals.assert_cascade_form(p, forms)
            for s in range(n):
                for c in range(2):
                    if (masks[s] >> c) & 1:
                        y3s.setdefault((s, c), []).append(p.debug_y3(s, c).copy())
            f0 += nf
        for s in range(n):
            for c in range(2):
                if (masks[s] >> c) & 1:
                    bits[(s, c)] = p.bits(s, c)
    buf.free()
    return {k: np.concatenate(v) for k, v in y3s.items()}, bits, iqs


def _k(tune, s, c):
    return tr.k_of(tune[(s, c)]) if (s, c) in tune else tr.NOMINAL[c]


@pytest.mark.parametrize("raw,s0", [(True, 1), (True, 3), (False, 1)], ids=["raw", "raw-cic3", "252k"])
@pytest.mark.parametrize("case", [CASE2, CASE1], ids=["two-chain", "one-chain"])
def test_tuned_chains_are_bit_identical_to_the_restatement(nv, raw, s0, case):
    masks, tune = case
    y3s, bits, iqs = _run(nv, raw, s0, masks, tune)
    for (s, c), y3 in y3s.items():
        want = tr.chain(tr.front(iqs[s], raw, s0), c, _k(tune, s, c))
        assert np.array_equal(_u64(y3), _u64(want[:y3.shape[0]])), (s, c)
        assert bits[(s, c)] == tr.decode(want), (s, c)
    # the nominal chain beside a tuned one (and every chain of the untuned handle): an untuned handle's bits
    if masks[1] == 3:
        y3u, bitsu, _ = _run(nv, raw, s0, masks, {})
        assert np.array_equal(_u64(y3s[(1, 0)]), _u64(y3u[(1, 0)])) and bits[(1, 0)] == bitsu[(1, 0)]


def test_unit_forms_agree_with_the_restatement(nv):
    """The hand-over forms (waiting, pre-rolling) and independent units, each forced: y3 and bits of 7 + 3
    frames with tuned chains, as digests, equal among themselves and to the restatement's."""
    digests = []
    for forms in signals.CASCADE_FORMS:
        h = hashlib.sha256()
        for raw in (False, True):
            y3s, bits, _ = _run(nv, raw, 1, [3, 1, 3], {(0, 0): 3000.0, (0, 1): -9000.0, (2, 1): 4481 * 3.125, (1, 0): 150.0}, frames=10, launches=(7, 3), forms=forms)
            for k in sorted(y3s): h.update(y3s[k].tobytes()); h.update(bits[k].encode())
        digests.append(h.hexdigest())
    assert digests[0] == digests[1] == digests[2] and len(digests[0]) == 64
    # and one of them against the restatement (the 252 kS/s run)
    tune = {(0, 0): 3000.0, (0, 1): -9000.0, (2, 1): 4481 * 3.125, (1, 0): 150.0}
    y3s, bits, iqs = _run(nv, False, 1, [3, 1, 3], tune, frames=10, launches=(7, 3))
    for (s, c), y3 in y3s.items():
        want = tr.chain(tr.front(iqs[s], False), c, _k(tune, s, c))
        assert np.array_equal(_u64(y3), _u64(want[:y3.shape[0]])) and bits[(s, c)] == tr.decode(want), (s, c)


def test_push_mode_eager_lagging_stream_and_ragged_finish(nv):
    """Push mode with eager launches and a stream that lags (the list kernels), ended by nvx_finish on a ragged length."""
    rate, frames = nv.RATE_IN, 4
    iqs = [_iq(nv, rate, frames, 600 + s, freq_hz=3000) for s in range(2)]
    n_end = 3 * nv.FRAME_IN + 12345
    tune = {(0, 0): 3000.0, (1, 1): -3000.0 + 4481 * 3.125 - 14000.0}
    with nv.Pipeline(n_streams=2, raw_rate=False, chain_mask=3, max_frames=2, push_mode=True, eager_launch=True, char_layer=False) as p:
        for (s, c), hz in tune.items():
            p.set_carrier(s, c, hz)
        F = nv.FRAME_IN                                    # stream 1 lags stream 0 by a frame and a half, then both end
        p.push(0, iqs[0][:2 * F]); p.push(1, iqs[1][:F // 2])
        p.push(0, iqs[0][2 * F:n_end]); p.push(1, iqs[1][F // 2:n_end])
        p.finish()
        got = {(s, c): p.bits(s, c) for s in range(2) for c in range(2)}
    for (s, c), b in got.items():
        want = tr.decode(tr.chain(tr.front(iqs[s][:n_end], False), c, _k(tune, s, c)))
        assert b == want and len(b) > 20, (s, c, len(b), len(want))


CARRIERS = ((150.0, "ZCZC AA01\nCARRIER PLUS 150 HZ\nNNNN\n"), (1000.0, "ZCZC AB02\nCARRIER PLUS 1 KHZ\nNNNN\n"),
            (-5000.0, "ZCZC AC03\nCARRIER MINUS 5 KHZ\nNNNN\n"), (19000.0, "ZCZC AD04\nCARRIER PLUS 19 KHZ\nNNNN\n"))


def test_messages_on_carriers_the_reference_mixer_misses(nv):
    frames = 40
    iqs = [_iq(nv, nv.RATE_IN, frames, 700 + i, freq_hz=int(hz), text=txt) for i, (hz, txt) in enumerate(CARRIERS)]
    for tuned in (False, True):
        with nv.Pipeline(n_streams=len(CARRIERS), chain_mask=nv.CHAIN_518, max_frames=4, push_mode=True) as p:
            if tuned:
                for s, (hz, _) in enumerate(CARRIERS):
                    assert p.set_carrier(s, 0, hz) == hz and p.carrier(s, 0) == (hz, False)
            for s in range(len(CARRIERS)):
                p.push(s, iqs[s])
            p.flush()
            got = {s: [m[3] for m in p.messages if m[0] == s] for s in range(len(CARRIERS))}
        for s, (_, txt) in enumerate(CARRIERS):
            assert got[s] == ([txt] if tuned else []), (tuned, s, got[s])


def test_retune_at_a_frame_boundary_and_back(nv):
    rate, frames = nv.RATE_RAW, 4
    iq = _iq(nv, rate, frames, 800, freq_hz=3000)
    pitch = frames * nv.FRAME_RAW
    buf = nv.DeviceBuffer(pitch * 4)
    buf.upload(iq)
    ks = [tr.NOMINAL[0], 960, 960, tr.NOMINAL[0]]
    with nv.Pipeline(n_streams=1, raw_rate=True, chain_mask=nv.CHAIN_518, max_frames=2, char_layer=False) as p:
        p.process_resident(buf, pitch, 0, 1); p.fetch()
        assert p.set_carrier(0, 0, 3000.0) == 3000.0
        p.process_resident(buf, pitch, 1, 2); p.fetch()
        p.set_carrier(0, 0, 14000.0)
        assert p.carrier(0, 0) == (14000.0, True)
        p.process_resident(buf, pitch, 3, 1); p.fetch()
        bits = p.bits(0, 0)
    buf.free()
    assert bits == tr.decode(tr.chain(tr.front(iq, True), 0, ks))


def test_scale_1024_raw_streams_random_carriers(nv):
    n, frames = 1024, 3
    rng = np.random.default_rng(5)
    ks = rng.integers(-8000, 8001, size=(n, 2))
    streams = [signals.stream_params(nv, 900 + s, nv.RATE_RAW)[0] for s in range(n)]
    pitch = frames * nv.FRAME_RAW
    buf = nv.DeviceBuffer(n * pitch * 4)
    nv.synth_device(streams, nv.RATE_RAW, pitch, buf, pitch)
    with nv.Pipeline(n_streams=n, raw_rate=True, chain_mask=3, max_frames=frames, char_layer=False) as p:
        for s in range(n):
            for c in range(2):
                p.set_carrier(s, c, ks[s, c] * 3.125)
        p.process_resident(buf, pitch, 0, frames); p.fetch()
        got = {(s, c): p.bits(s, c) for s in range(n) for c in range(2)}
    buf.free()

    def want(s):
        y1 = tr.front(nv.synth_host(streams[s], nv.RATE_RAW, pitch), True)
        return [tr.decode(tr.chain(y1, c, int(ks[s, c]))) for c in range(2)]
    with ThreadPoolExecutor(16) as ex:
        for s, w in enumerate(ex.map(want, range(n))):
            assert got[(s, 0)] == w[0] and got[(s, 1)] == w[1], s


def test_group_routes_to_the_member_and_errors(nv):
    with nv.Group([0, 0], n_streams=4, raw_rate=True, chain_mask=3, char_layer=False) as g:
        assert g.set_carrier(3, 1, -1000.0) == -1000.0 and g.carrier(3, 1) == (-1000.0, False)
        m = g.member_of(3)
        assert g.member_view(m).carrier(3 - g.members[m][1], 1) == (-1000.0, False)
        assert g.carrier(0, 1) == (-14000.0, True) and g.carrier(2, 1) == (-14000.0, True)
        with pytest.raises(nv.NvxError) as e:
            g.set_carrier(4, 0, 0.0)
        assert e.value.code == nv._native.ERR_ARG
    with nv.Pipeline(n_streams=2, chain_masks=[1, 3], char_layer=False) as p:
        assert p.set_carrier(0, 0, 1.6) == 3.125 and p.set_carrier(0, 0, 1.5) == 0.0     # rint, ties to even
        assert p.set_carrier(1, 1, 25000.0) == 25000.0
        for args in ((0, 1, 0.0), (2, 0, 0.0), (-1, 0, 0.0), (0, 2, 0.0), (0, 0, 25000.1), (0, 0, float("nan")), (0, 0, float("inf"))):
            with pytest.raises(nv.NvxError) as e:
                p.set_carrier(*args)
            assert e.value.code == nv._native.ERR_ARG, args
        p.reset(); p.stream_reset(1)
        assert p.carrier(0, 0) == (0.0, False) and p.carrier(1, 1) == (25000.0, False)   # configuration: survives resets
    with nv.Pipeline(n_streams=1, wideband=True, raw_rate=True, char_layer=False) as p:
        with pytest.raises(nv.NvxError) as e:
            p.set_carrier(0, 0, 0.0)
        assert e.value.code == nv._native.ERR_STATE


@pytest.mark.parametrize("tuned_hz", [3000.0, -9000.0])
def test_signal_report_measures_against_the_tuned_carrier(nv, tuned_hz):
    offs = []
    for d in sr.OFFSETS:
        frames = sr.SECONDS * nv.RATE_IN // nv.FRAME_IN
        car = [dict(freq_hz=int(tuned_hz) + d, bits=nv.sitor_encode(signals.stream_text(7), 40), bit_offset=301, phase0=5, amplitude=8000)]
        iq = nv.synth_host(nv.make_stream(car, seed=11, noise_amp=1500), nv.RATE_IN, frames * nv.FRAME_IN)
        with nv.Pipeline(n_streams=1, chain_mask=nv.CHAIN_518, max_frames=8, push_mode=True, char_layer=False) as p:
            p.set_carrier(0, 0, tuned_hz)
            p.enable_signal_report(True)
            p.push(0, iq); p.flush()
            offs.append(p.signal_report(0, 0)["offset_hz"])
    for d, o in zip(sr.OFFSETS, offs):
        assert abs(o - d) <= sr.OFFSET_TOL, (d, o)
    assert all(b > a for a, b in zip(offs, offs[1:])), offs
