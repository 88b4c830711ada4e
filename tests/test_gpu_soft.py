"""Soft-decision decoding (include/navtex_amd_soft.h) on the GPU (-m gpu).

The values: nvx_poll_soft, bit for bit (viewed as uint32), equals the restatement (tests/soft_ref.py) on the device's OWN
900 S/s samples (nvx_debug_y3, collected launch by launch), at the samples where the oracle's bit FSM -- run on those
samples with the device's atan2 -- decides a bit; as many values as bits, signs = bits; bits and hard messages unchanged
by the mode.  Covered: resident and list launches, a ragged end, raw rate in both stage-0 forms, a tuned chain, a
wideband handle, both forms of the front, chains spread over several FSM workgroups, the mode's semantics, and the
acceptance case end to end (tests/test_soft.py) through one handle."""
import ctypes as C

import numpy as np
import pytest

import signals
import soft_ref

pytestmark = pytest.mark.gpu


class Collector:
    """The device's y3 of every chain, launch by launch (the debug tap holds the last launch only)."""

    def __init__(self, p, n_streams, push_mode):
        self.p, self.push_mode = p, push_mode
        self.y3 = {(s, c): [] for s in range(n_streams) for c in range(2)}

    def step(self, op, streams, launches=1):
        """op() makes exactly `launches` launches (0 or 1), in which `streams` (decoded streams) take part."""
        before = self.p.integrity_stats()[2]
        op()
        self.p.flush() if self.push_mode else self.p.fetch()
        got = self.p.integrity_stats()[2] - before
        assert got == launches, f"{got} launches where {launches} were meant"
        if got:
            for s in streams:
                for c in range(2):
                    self.y3[(s, c)].append(self.p.debug_y3(s, c))

    def chain(self, sc):
        return np.concatenate(self.y3[sc]) if self.y3[sc] else np.zeros((0, 2))


def check_values(nv, oracle, p, col, chains, soft=None):
    """Every chain: values == restatement on the device's y3 (as uint32), count == bit count, signs == bits == the oracle's
    on those samples.  soft: values polled already (else polled here).  Returns {chain: (bits, values)}."""
    fR, fI = oracle.bitfilter_table()
    fn = C.cast(nv.lib.nvx_atan2_host, C.c_void_p)
    out = {}
    for sc in chains:
        y3 = col.chain(sc)
        taps = oracle.decode_taps(y3, fn)
        want = soft_ref.values(y3, fR, fI, taps["bit_at"])
        got = p.soft_values(*sc) if soft is None else soft[sc]
        bits = p.bits(*sc)
        assert bits == taps["bits"], sc
        assert got.dtype == np.float32 and got.shape == want.shape, (sc, got.shape, want.shape)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (sc, np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:8])
        assert p.soft_count(*sc) == p.bit_count(*sc) == len(bits), sc
        assert "".join("B" if v > 0 else "Y" for v in got) == bits, sc
        out[sc] = (bits, got)
    return out


def _three_streams(nv, rate):
    """one strong, one at amplitude 300 under noise_amp 6000, one noise only"""
    bits = nv.sitor_encode(signals.stream_text(7), 40)
    return [signals.stream_params(nv, 4100, rate)[0],
            nv.make_stream([dict(freq_hz=14000, bits=bits, bit_offset=301, phase0=5, amplitude=300)], seed=11, noise_amp=6000),
            nv.make_stream([], seed=4102, noise_amp=6000)]


def _values_run(nv, oracle, mode):
    """Three resident launches of two frames, then the same streams again in push mode: a list launch without the lagging
    stream 1, one of stream 1 alone, one of all three, and nvx_finish with tails of 3, 100 and 287 samples at 900 S/s."""
    rate, frame = nv.RATE_IN, nv.FRAME_IN
    sts = _three_streams(nv, rate)
    chains = [(s, c) for s in range(3) for c in range(2)]
    result = {}
    F = 6
    buf = nv.DeviceBuffer(3 * F * frame * 4)
    nv.synth_device(sts, rate, F * frame, buf, F * frame)
    with nv.Pipeline(n_streams=3, chain_mask=3, max_frames=2) as p:
        if mode:
            p.enable_soft(mode)
        col = Collector(p, 3, False)
        for f0 in (0, 2, 4):
            col.step(lambda: p.process_resident(buf, F * frame, f0, 2), range(3))
        result["resident"] = check_values(nv, oracle, p, col, chains) if mode else {sc: (p.bits(*sc), None) for sc in chains}
        result["resident_messages"] = list(p.messages)
    buf.free()
    tails = (3, 100, 287)
    iqs = [nv.synth_host(st, rate, 4 * frame + t * 280 + 139) for st, t in zip(sts, tails)]
    with nv.Pipeline(n_streams=3, chain_mask=3, max_frames=2, push_mode=True) as p:
        if mode:
            p.enable_soft(mode)
        col = Collector(p, 3, True)
        p.push(0, iqs[0][:2 * frame]); p.push(2, iqs[2][:2 * frame])
        col.step(lambda: None, (0, 2))                              # the flush: streams 0 and 2, stream 1 lags
        assert p.stream_stats(0)[2] == 1                            # ... a launch with a list
        p.push(1, iqs[1][:2 * frame])
        col.step(lambda: None, (1,))
        p.push(0, iqs[0][2 * frame:]); p.push(1, iqs[1][2 * frame:])
        col.step(lambda: p.push(2, iqs[2][2 * frame:]), range(3))
        col.step(p.finish, range(3))
        for s, t in enumerate(tails):
            assert col.chain((s, 0)).shape[0] == 4 * nv.FRAME_Y3 + t
        result["push"] = check_values(nv, oracle, p, col, chains) if mode else {sc: (p.bits(*sc), None) for sc in chains}
        result["push_messages"] = list(p.messages)
    return result


def test_values_equal_the_restatement_and_change_no_bit(nv, oracle):
    on, off = _values_run(nv, oracle, nv.SOFT_DECODE | nv.SOFT_KEEP), _values_run(nv, oracle, 0)
    for part in ("resident", "push"):
        for sc in on[part]:
            assert on[part][sc][0] == off[part][sc][0], (part, sc)
            assert len(on[part][sc][0]) > 50
        assert on[part + "_messages"] == off[part + "_messages"]


def _config_case(nv, oracle, name):
    rate, frame, kw, n_streams, chains, tune = nv.RATE_IN, nv.FRAME_IN, {}, 2, None, None
    if name in ("raw_cic1", "raw_cic3"):
        rate, frame, kw = nv.RATE_RAW, nv.FRAME_RAW, dict(raw_rate=True, stage0_order=1 if name == "raw_cic1" else 3)
    if name == "wideband":
        rate, frame, kw, n_streams = nv.RATE_RAW, nv.FRAME_RAW, dict(wideband=True), 1
        car = [dict(freq_hz=(k * 252000 if k < 4 else (k - 8) * 252000) + off, bits=nv.sitor_encode(f"ZCZC SF{k}{c}\nSOFT\nNNNN\n", 6),
                    bit_offset=613 * (2 * k + c + 1), phase0=7654321 * (2 * k + c + 1) % 2**32, amplitude=1500)
               for k in range(8) for c, off in ((0, 14000), (1, -14000))]
        sts = [nv.make_stream(car, seed=79, noise_amp=500)]
        chains = [(s, c) for s in range(8) for c in range(2)]
    else:
        sts = [signals.stream_params(nv, 4200 + s, rate, freq_hz=15000 if name == "tuned" else 14000, noise_amp=3000) for s in range(2)]
        sts = [s[0] for s in sts]
        chains = [(s, c) for s in range(2) for c in range(2)]
    F = 4                                                              # (the timing filter decides its first bit at sample 582: the third frame)
    buf = nv.DeviceBuffer(n_streams * F * frame * 4)
    nv.synth_device(sts, rate, F * frame, buf, F * frame)
    with nv.Pipeline(n_streams=n_streams, chain_mask=3, max_frames=2, char_layer=False, **kw) as p:
        if name == "tuned":
            assert p.set_carrier(0, 0, 15000.0) == 15000.0 and p.set_carrier(1, 0, 15000.0) == 15000.0
        p.enable_soft(nv.SOFT_DECODE | nv.SOFT_KEEP)
        col = Collector(p, len(chains) // 2, False)
        for f0 in (0, 2, 3):                                           # launches of 2, 1 and 1 frames: the later ones' first windows reach back
            col.step(lambda: p.process_resident(buf, F * frame, f0, 2 if f0 == 0 else 1), range(len(chains) // 2))
        got = check_values(nv, oracle, p, col, chains)
    buf.free()
    assert sum(len(b) for b, _ in got.values()) > 20 * len(chains)


@pytest.mark.parametrize("name", ["raw_cic1", "raw_cic3", "tuned", "wideband"])
def test_other_configurations(nv, oracle, name):
    _config_case(nv, oracle, name)


def test_both_forms_of_the_front_give_the_same_values(nv, oracle):
    """One stream x 12 frames, twice, with the walk and with head + tiles forced: each
    equals the restatement, and the two agree in every bit."""
    F = 12
    st = signals.stream_params(nv, 4300, nv.RATE_IN, noise_amp=4000)[0]
    buf = nv.DeviceBuffer(2 * F * nv.FRAME_IN * 4)
    nv.synth_device([st], nv.RATE_IN, 2 * F * nv.FRAME_IN, buf, 2 * F * nv.FRAME_IN)
    seen = []
    for forms in (signals.WALK, signals.TILES):
        with nv.Pipeline(n_streams=1, chain_mask=3, max_frames=F, char_layer=False, forms=forms) as p:
            p.enable_soft(3)
            col = Collector(p, 1, False)
            for f0 in (0, F):                     # 12 frames = 8 tiles: head + 6 tile workgroups when the tile form is taken
                col.step(lambda: p.process_resident(buf, 2 * F * nv.FRAME_IN, f0, F), [0])
                assert p.last_forms()[2] == (6 if forms == signals.TILES else 0)
            got = check_values(nv, oracle, p, col, [(0, 0), (0, 1)])
        assert sum(len(b) for b, _ in got.values()) > 2 * 20 * 32      # (two chains, 24 frames of 32 bits less the timing filter's priming)
        seen.append(" ".join(v.tobytes().hex() for _, v in got.values()))
    buf.free()
    assert seen[0] == seen[1]


def test_many_chains_over_several_fsm_workgroups(nv, oracle):
    """100 streams x 2 chains x 4 frames, a seed each: 200 lanes of nvx_demod_fsm in four workgroups."""
    S, F = 100, 4
    rate, frame = nv.RATE_IN, nv.FRAME_IN
    sts = [signals.stream_params(nv, 4400 + s, rate, freq_hz=14000 if s % 2 else -14000, noise_amp=1500 + 60 * s)[0] for s in range(S)]
    buf = nv.DeviceBuffer(S * F * frame * 4)
    nv.synth_device(sts, rate, F * frame, buf, F * frame)
    with nv.Pipeline(n_streams=S, chain_mask=3, max_frames=2, char_layer=False) as p:
        p.enable_soft(nv.SOFT_DECODE | nv.SOFT_KEEP)
        col = Collector(p, S, False)
        for f0 in (0, 2):
            col.step(lambda: p.process_resident(buf, F * frame, f0, 2), range(S))
        got = check_values(nv, oracle, p, col, [(s, c) for s in range(S) for c in range(2)])
    buf.free()
    assert len({len(b) for b, _ in got.values()}) > 3                   # the chains are not in step


def test_mode_semantics(nv, oracle):
    rate, frame, F = nv.RATE_IN, nv.FRAME_IN, 12
    sts = [signals.stream_params(nv, 4500 + s, rate)[0] for s in range(2)]
    buf = nv.DeviceBuffer(2 * F * frame * 4)
    nv.synth_device(sts, rate, F * frame, buf, F * frame)
    chains = [(s, c) for s in range(2) for c in range(2)]

    def launch(p, f0, n=2):
        p.process_resident(buf, F * frame, f0, n)
        p.fetch()

    with nv.Pipeline(n_streams=2, chain_mask=3, max_frames=2, char_layer=False) as p:
        launch(p, 0); launch(p, 2)                                      # mode 0: nothing counted, nothing kept (the first bits come in the third frame)
        n0 = [p.bit_count(*sc) for sc in chains]
        assert all(n > 0 for n in n0) and all(p.soft_count(*sc) == 0 and p.soft_values(*sc).size == 0 for sc in chains)
        p.enable_soft(nv.SOFT_DECODE)                                   # 0 -> 1: counted, not kept
        launch(p, 4)
        n1 = [p.bit_count(*sc) for sc in chains]
        assert [p.soft_count(*sc) for sc in chains] == [b - a for a, b in zip(n0, n1)]
        assert all(p.soft_values(*sc).size == 0 for sc in chains)
        p.enable_soft(nv.SOFT_DECODE | nv.SOFT_KEEP)                    # 1 -> 3: kept from here on; the count goes on
        launch(p, 6)
        n2 = [p.bit_count(*sc) for sc in chains]
        assert [p.soft_count(*sc) for sc in chains] == [b - a for a, b in zip(n0, n2)]
        kept = [p.soft_values(*sc) for sc in chains]
        assert [v.size for v in kept] == [b - a for a, b in zip(n1, n2)]
        for sc, v, a in zip(chains, kept, n1):                          # ... and they are the values of that launch's bits
            assert "".join("B" if x > 0 else "Y" for x in v) == p.bits(*sc)[a:]
        assert all(p.soft_values(*sc).size == 0 for sc in chains)       # consumed
        # nvx_stream_reset: stream 1's values and count go, stream 0's stay
        launch(p, 8)
        p.stream_reset(1)
        assert p.soft_count(1, 0) == 0 and p.soft_count(1, 1) == 0 and p.soft_values(1, 0).size == 0
        assert p.soft_count(0, 0) == p.bit_count(0, 0) - n0[0] and p.soft_values(0, 0).size == p.bit_count(0, 0) - n2[0]
        p.enable_soft(0)                                                # 3 -> 0
        assert all(p.soft_count(*sc) == 0 and p.soft_values(*sc).size == 0 for sc in chains)
        # enabling waits for the work in flight: a launch made before it is no soft launch, the next one is
        p.reset()
        launch(p, 0)
        p.process_resident(buf, F * frame, 2, 2)
        p.enable_soft(nv.SOFT_DECODE | nv.SOFT_KEEP)
        p.fetch()
        first = p.bit_count(0, 0)
        assert first > 0 and p.soft_count(0, 0) == 0
        launch(p, 4)
        assert p.soft_count(0, 0) == p.bit_count(0, 0) - first == p.soft_values(0, 0).size > 0
        p.reset()                                                       # the setting survives nvx_reset
        launch(p, 0); launch(p, 2)
        assert p.soft_count(0, 0) == p.bit_count(0, 0) == p.soft_values(0, 0).size > 0
        for bad in ((2, 0), (-1, 0), (0, 2)):
            assert p.soft_count(*bad) == 0 and p.soft_values(*bad).size == 0
    buf.free()


def test_stream_reset_restarts_one_soft_layer_and_history_rule(nv, oracle):
    """(a) Two streams carry the same transmission; stream 1 is reset in the middle of it, so its soft layer (like its hard
    one) loses the message while stream 0's delivers it.  (b) A reader that never polled, behind a bit_history of 64:
    it resumes at the oldest value held, as nvx_poll_bits does."""
    rate, frame = nv.RATE_IN, nv.FRAME_IN
    text = "ZCZC SR01\nRESET\nNNNN\n"
    bits = nv.sitor_encode(text, 12)
    F = (len(bits) + 150) * (rate // 100) // frame + 1
    st = nv.make_stream([dict(freq_hz=14000, bits=bits, bit_offset=301, phase0=5, amplitude=8000)], seed=3, noise_amp=1500)
    buf = nv.DeviceBuffer(2 * F * frame * 4)
    nv.synth_device([st, st], rate, F * frame, buf, F * frame)
    half = F // 2
    with nv.Pipeline(n_streams=2, chain_mask=1, max_frames=F) as p, nv.Pipeline(n_streams=2, chain_mask=1, max_frames=F, bit_history=64) as q:
        for h in (p, q):
            h.enable_soft(nv.SOFT_DECODE | nv.SOFT_KEEP)
        p.process_resident(buf, F * frame, 0, half); p.fetch()
        p.stream_reset(1)
        p.process_resident(buf, F * frame, half, F - half); p.fetch()
        assert p.soft_messages == [(0, 518, "SR01", text)] and [m for m in p.messages if m[0] == 0] == [(0, 518, "SR01", text)]
        assert not [m for m in p.messages if m[0] == 1]
        assert p.soft_count(0, 0) == p.bit_count(0, 0) and p.soft_count(1, 0) == p.bit_count(1, 0) < p.bit_count(0, 0)
        q.process_resident(buf, F * frame, 0, half); q.process_resident(buf, F * frame, half, F - half); q.fetch()
        q_bits, q_vals, all_vals = q.bits(0, 0), q.soft_values(0, 0), p.soft_values(0, 0)
        assert 64 <= q_vals.size <= 128 and q_vals.size == len(q_bits) and q.soft_count(0, 0) == all_vals.size
        assert np.array_equal(q_vals.view(np.uint32), all_vals[-q_vals.size:].view(np.uint32))
    buf.free()


def test_acceptance_end_to_end(nv, oracle):
    """The twelve acceptance runs (tests/soft_ref.py: amplitude 300, noise_amp 6000, seeds 11 .. 22) as twelve streams of one
    handle, twelve frames a launch.  on_message delivers what the reference's rule delivers on the oracle's bits; the soft
    callback what the restated layer delivers on the device's values; S >= H + 6.  Counted on the device: H = 1, S = 12."""
    rate, frame = nv.RATE_IN, nv.FRAME_IN
    runs = [soft_ref.accept_stream(nv, seed, 300, 6000) for seed in soft_ref.ACCEPT_SEEDS]
    F, want = runs[0][1], runs[0][2]
    S_n = len(runs)
    buf = nv.DeviceBuffer(S_n * F * frame * 4)
    nv.synth_device([r[0] for r in runs], rate, F * frame, buf, F * frame)
    with nv.Pipeline(n_streams=S_n, chain_mask=1, max_frames=12) as p:
        p.enable_soft(nv.SOFT_DECODE | nv.SOFT_KEEP)
        for f0 in range(0, F, 12):
            p.process_resident(buf, F * frame, f0, min(12, F - f0))
        p.fetch()
        hard, soft = sorted(p.messages), sorted(p.soft_messages)
        values = [p.soft_values(s, 0) for s in range(S_n)]
        bits = [p.bits(s, 0) for s in range(S_n)]
    buf.free()
    want_hard, want_soft = [], []
    for s, (st, _, _) in enumerate(runs):
        ref = oracle.Pipe(chain_mask=1)
        ref.push(nv.synth_host(st, rate, F * frame))
        assert bits[s] == ref.bits(0)
        want_hard += [(s, f, b, t) for f, b, t in ref.messages]
        layer = soft_ref.SoftLayer(518)
        layer.feed(values[s])
        want_soft += [(s, f, b, t) for f, b, t in layer.messages]
    assert hard == sorted(want_hard)
    assert soft == sorted(want_soft)
    H = sum([m[1:] for m in hard if m[0] == s] == [(518,) + want] for s in range(S_n))
    S = sum([m[1:] for m in soft if m[0] == s] == [(518,) + want] for s in range(S_n))
    print(f"acceptance on the device: H = {H}, S = {S} of {S_n}")
    assert S >= H + 6, (H, S)
