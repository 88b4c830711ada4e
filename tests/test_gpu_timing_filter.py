"""The demodulator's bit-timing filter on the GPU against the oracle, bit for bit (-m gpu).

With nvx_enable_debug on, the front kernels store |corr| and the class sum S of every sample (nvx_debug_timing, beside
nvx_debug_dphi) and hand the FSM one word per bit period (nine window decisions, arg-max << 12).  For every chain of
every run, over all its launches, the oracle is fed that chain's own 900 S/s samples with the device's atan2
(oracle_binding.decode_taps with nvx_atan2_host) and must give

  * delta-phi, |corr| (g >= 8) and S (g >= 574) with the same fp64 bit patterns;
  * the same arg-max in every word (15 where there is no evaluation);
  * decision bits equal to a numpy restatement of front_decision / decoder.C:96-132 at every sample (tests/timing_ref.py);

and nvx_demod_tie_stats must report what the oracle's class sums give.  tests/test_timing_filter.py pins the oracle's
taps to the compiled reference and to a restatement of decoder.C on CPU."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import signals
import timing_ref as tr

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def check_chains(nv, oracle, taps, p=None, cover=None):
    """Every chain `taps` collected against the oracle; returns (chains, samples) compared.  p: also the handle's tie
    statistics (taps must hold every chain it decoded).  cover: a set that receives the residues g mod 5103 at which S
    was compared."""
    fn = C.cast(nv.lib.nvx_atan2_host, C.c_void_p)
    fR, fI = oracle.bitfilter_table()
    sums, n_chains, n_samples = [], 0, 0
    for sc in taps.chains:
        d = taps.chain(sc)
        n = d["y3"].shape[0]
        o = oracle.decode_taps(d["y3"], fn)
        what = f"stream {sc[0]} chain {sc[1]}"
        assert d["dphi"].shape[0] == n and d["corr"].shape[0] == n and d["csum"].shape[0] == n, what
        assert np.array_equal(tr.u64(d["dphi"]), tr.u64(o["dphi"])), f"{what}: delta-phi"
        assert np.array_equal(tr.u64(d["corr"][8:]), tr.u64(o["corr"][8:])), f"{what}: |corr|"
        assert np.array_equal(tr.u64(d["csum"][574:]), tr.u64(o["csum"][574:])), f"{what}: class sums"
        w = d["words"].astype(np.int64)
        assert w.shape[0] == (n + 8) // 9, what
        m = np.arange(w.shape[0])
        g = 9 * m + 6
        want_arg = np.where(g < n, o["argmax"][np.minimum(g, n - 1)] if n else 15, 15)
        want_arg = np.where(want_arg < 0, 15, want_arg)
        assert np.array_equal(w >> 12, want_arg), f"{what}: arg-max"
        dec = np.zeros(9 * w.shape[0], dtype=np.int64)
        dec[:n] = tr.decisions(d["y3"], fR, fI) if n else dec[:0]
        assert np.array_equal(w & 0x1ff, (dec.reshape(-1, 9) << np.arange(9)).sum(axis=1)), f"{what}: window decisions"
        assert not np.any(w & 0xe00), what
        if cover is not None and n > 574:
            cover.update(np.unique(np.arange(574, n) % tr.MOD).tolist())
        sums.append(o["csum"])
        n_chains += 1; n_samples += n
    if p is not None:
        near, evals, margin = p.tie_stats()
        want = tr.tie_stats(sums)
        assert (near, evals) == want[:2], f"tie counter {(near, evals)} != {want[:2]}"
        assert (margin == -1.0) if want[2] is None else (np.float32(margin) == want[2]), (margin, want[2])
    return n_chains, n_samples


def test_both_front_forms_equal_the_oracle_at_every_stage(nv, oracle):
    """The walk and head + tiles, each forced: launches of 1, 4, 25 and 9 frames of three
    streams (four chains) carry the state from launch to launch; with tiles forced the launches of 4, 25 and 9 frames have
    3, 17 and 6 tiles and take the tile form (launcher rule: tiles >= 3; the handle reports what ran), each tile storing
    only its own samples.  Every stage equals the oracle, and S is compared at every residue g mod 5103 (the ring algebra's
    whole period)."""
    masks = [1, 3, 2]
    streams = [signals.stream_params(nv, 900 + s, nv.RATE_IN, n_phasing=14)[0] for s in range(3)]
    F = 39
    buf = nv.DeviceBuffer(3 * F * nv.FRAME_IN * 4)
    nv.synth_device(streams, nv.RATE_IN, F * nv.FRAME_IN, buf, F * nv.FRAME_IN)
    for forms in (signals.WALK, signals.TILES):
        cover = set()
        ran_tiles = 0
        with nv.Pipeline(n_streams=3, raw_rate=False, chain_masks=masks, max_frames=25, forms=forms) as p:
            p.enable_debug(True)
            taps = tr.DeviceTaps(p, [(s, c) for s in range(3) for c in range(2) if (masks[s] >> c) & 1], push_mode=False)
            f0 = 0
            for k in (1, 4, 25, 9):
                taps.launch(lambda: p.process_resident(buf, F * nv.FRAME_IN, f0, k)); f0 += k
                signals.assert_front_form(p, forms, tiles_fit=k > 1)
                ran_tiles += p.last_forms()[2] > 0
            chains, samples = check_chains(nv, oracle, taps, p, cover)
        assert ran_tiles == (3 if forms == signals.TILES else 0)
        print(f"forms {forms}: {chains} chains, {samples} samples, {taps.n_launches} launches ({ran_tiles} in the tile form), "
              f"{len(cover)} residues mod 5103")
        assert chains == 4 and samples == 4 * 39 * 288 and taps.n_launches == 4 and len(cover) == tr.MOD
    buf.free()


# (900 S/s samples of the stream, as whole frames F + the rest r): priming thresholds 8 / 574 / 582 and the ninth sample
TAIL_GROUPS = {0: (7, 8, 9), 1: (573, 574, 575), 2: (581, 582, 583), 8: (2591,), 9: (2592, 2593)}


@pytest.mark.parametrize("frames", sorted(TAIL_GROUPS))
def test_priming_and_ragged_ends_equal_the_oracle(nv, oracle, frames):
    """Push-mode streams ended by nvx_finish where their 900 S/s count n3 lands on either side of each priming threshold and
    of a bit period: one launch of the whole frames, then ONE launch that ends every stream at its own n3 (the list path,
    a count per participant).  Every chain equals the oracle up to its last sample; the tie counter too."""
    n3s = TAIL_GROUPS[frames]
    with nv.Pipeline(n_streams=len(n3s), raw_rate=False, chain_mask=3, max_frames=max(frames, 1), push_mode=True, char_layer=False) as p:
        p.enable_debug(True)
        taps = tr.DeviceTaps(p, [(s, c) for s in range(len(n3s)) for c in range(2)], push_mode=True)
        iqs = []
        for s, n3 in enumerate(n3s):
            st, _ = signals.stream_params(nv, 60 + n3, nv.RATE_IN)
            iqs.append(nv.synth_host(st, nv.RATE_IN, n3 * 280 + 139))
        for s, iq in enumerate(iqs[:-1]):                # (a flush here would launch the streams pushed so far on their own)
            p.push(s, iq)
        # the last push completes the whole frames of every stream: one launch of them all (lock-step)
        taps.launch(lambda: p.push(len(iqs) - 1, iqs[-1]), launches=int(frames > 0))
        tails = sum(1 for n3 in n3s if n3 % 288)
        taps.launch(p.finish, launches=int(tails > 0))
        chains, samples = check_chains(nv, oracle, taps, p)
        for s, n3 in enumerate(n3s):
            assert taps.chain((s, 0))["y3"].shape[0] == n3
    print(f"n3 {n3s}: {chains} chains, {samples} samples in {taps.n_launches} launches")
    assert chains == 2 * len(n3s) and samples == 2 * sum(n3s)


@pytest.mark.parametrize("power,frames_before", [(31, 487), (32, 410)], ids=["2^31", "2^32"])
def test_clock_far_from_zero_equals_the_oracle(nv, oracle, power, frames_before):
    """The stream's clock is put 3.4 / 3.9 frames below 2^31 / 2^32 (nvx_debug_advance_clock: whole periods of everything
    derived from it) and the next launches cross it.  g is 64 bits and t_cb 32 bits in the kernels; the oracle's
    arithmetic does not depend on g at all: every stage must still be its, bit for bit, in both front forms (launches
    of 25 frames take the tile form, the last one of 2 the walk)."""
    st, _ = signals.stream_params(nv, 4242, nv.RATE_IN)
    chunk = 25
    before = [chunk] * (frames_before // chunk) + ([frames_before % chunk] if frames_before % chunk else [])
    after = [chunk, chunk, 2]
    iq = nv.synth_host(st, nv.RATE_IN, chunk * nv.FRAME_IN)          # pushed again and again: the state runs on
    with nv.Pipeline(n_streams=1, raw_rate=False, chain_mask=3, max_frames=chunk, push_mode=True, char_layer=False) as p:
        p.enable_debug(True)
        taps = tr.DeviceTaps(p, [(0, 0), (0, 1)], push_mode=True)
        f0 = 0
        for k in before:
            taps.launch(lambda: p.push(0, iq[:k * nv.FRAME_IN])); f0 += k
        g = p.stream_stats(0)[1] * nv.FRAME_Y3
        periods = (2 ** power - g) // p.CLOCK_PERIOD
        p.debug_advance_clock(0, periods)
        g_new = g + periods * p.CLOCK_PERIOD
        assert p.stream_stats(0)[1] * nv.FRAME_Y3 == g_new and 0 < 2 ** power - g_new < 4 * nv.FRAME_Y3
        for k in after:
            taps.launch(lambda: p.push(0, iq[:k * nv.FRAME_IN])); f0 += k
        assert p.stream_stats(0)[1] * nv.FRAME_Y3 > 2 ** power + nv.FRAME_Y3
        chains, samples = check_chains(nv, oracle, taps, p)
        assert p.integrity_stats()[:2] == (0, 0)
    print(f"clock across 2^{power}: {chains} chains, {samples} samples")
    assert chains == 2 and samples == 2 * f0 * nv.FRAME_Y3


def test_golden_iq_cases_equal_the_oracle(nv, oracle):
    """The golden iq cases (tests/golden/golden.json), each pushed in launches of 25 frames and ended at its true length.
    Silence: every class sum is exactly 0 and every arg-max 0 (strict '>' from -1), and the tie counter counts nothing."""
    import json
    import cases
    gold = json.loads((ROOT / "tests" / "golden" / "golden.json").read_text())["iq"]
    total = 0
    for name in sorted(gold):
        iq = cases.make_iq(nv, gold[name]["spec"])
        with nv.Pipeline(n_streams=1, raw_rate=False, chain_mask=3, max_frames=25, push_mode=True, char_layer=False) as p:
            p.enable_debug(True)
            taps = tr.DeviceTaps(p, [(0, 0), (0, 1)], push_mode=True)
            step = 25 * nv.FRAME_IN
            for a in range(0, iq.shape[0], step):
                part = iq[a:a + step]
                taps.launch(lambda: p.push(0, part), launches=int(part.shape[0] >= nv.FRAME_IN))
            taps.launch(p.finish, launches=int((iq.shape[0] % nv.FRAME_IN) >= 280))
            chains, samples = check_chains(nv, oracle, taps, p)
            assert chains == 2 and samples == 2 * (iq.shape[0] // 280)
            if name == "silence":
                for c in (0, 1):
                    d = taps.chain((0, c))
                    w = d["words"] >> 12                   # word m evaluates at g = 9 m + 6: from m = 64 on (g >= 582)
                    assert not np.any(d["csum"]) and np.all(w[:64] == 15) and np.all(w[64:] == 0) and w.shape[0] > 200
                assert p.tie_stats() == (0, 0, -1.0)
            total += samples
    print(f"golden iq cases: {total} samples")


@pytest.mark.parametrize("raw,order", [(False, 1), (True, 1), (True, 3)], ids=["252k", "raw_cic1", "raw_cic3"])
def test_random_resident_batches_equal_the_oracle(nv, oracle, raw, order):
    """Random multi-stream resident batches with mixed chain masks and launch lengths, at 252 kS/s and at the raw rate in
    both stage-0 forms."""
    rng = np.random.default_rng(71 + 2 * raw + order)
    rate = nv.RATE_RAW if raw else nv.RATE_IN
    frame = nv.FRAME_RAW if raw else nv.FRAME_IN
    n_streams, n_frames = int(rng.integers(3, 7)), 12
    masks = [int(rng.choice([1, 2, 3])) for _ in range(n_streams)]
    pitch = n_frames * frame
    buf = nv.DeviceBuffer(n_streams * pitch * 4)
    for s in range(n_streams):
        st, _ = signals.stream_params(nv, 300 + s, rate, freq_hz=int(rng.choice([14000, -14000])) + int(rng.integers(-10, 11)),
                                      noise_amp=int(rng.integers(0, 6000)))
        buf.upload(nv.synth_host(st, rate, pitch), offset=s * pitch * 4)
    with nv.Pipeline(n_streams=n_streams, raw_rate=raw, chain_masks=masks, max_frames=6, char_layer=False, stage0_order=order) as p:
        p.enable_debug(True)
        taps = tr.DeviceTaps(p, [(s, c) for s in range(n_streams) for c in range(2) if (masks[s] >> c) & 1], push_mode=False)
        f0 = 0
        while f0 < n_frames:
            k = int(min(n_frames - f0, rng.integers(1, 7)))
            taps.launch(lambda: p.process_resident(buf, pitch, f0, k)); f0 += k
        chains, samples = check_chains(nv, oracle, taps, p)
    buf.free()
    n_chains = sum(bin(m).count("1") for m in masks)
    print(f"{n_streams} streams, {chains} chains, {samples} samples in {taps.n_launches} launches")
    assert chains == n_chains and samples == n_chains * n_frames * nv.FRAME_Y3


def test_wideband_handle_equals_the_oracle(nv, oracle):
    """One wideband input: eight sub-bands x two chains, the demodulator's per-entry stream mapping (per_part = 8)."""
    F = 7
    n = F * nv.FRAME_RAW
    car = [dict(freq_hz=(k * 252000 if k < 4 else (k - 8) * 252000) + off, bits=nv.sitor_encode(f"ZCZC TF{k}{c}\nTIMING\nNNNN\n", 6),
                bit_offset=911 * (2 * k + c + 1), phase0=7654321 * (2 * k + c + 1) % 2**32, amplitude=1500)
           for k in range(8) for c, off in ((0, 14000), (1, -14000))]
    raw = nv.synth_host(nv.make_stream(car, seed=77, noise_amp=500), nv.RATE_RAW, n)
    buf = nv.DeviceBuffer(n * 4)
    buf.upload(raw)
    with nv.Pipeline(n_streams=1, wideband=True, chain_mask=3, max_frames=4, char_layer=False) as p:
        p.enable_debug(True)
        taps = tr.DeviceTaps(p, [(s, c) for s in range(8) for c in range(2)], push_mode=False)
        for f0, k in ((0, 4), (4, 3)):
            taps.launch(lambda: p.process_resident(buf, n, f0, k))
        chains, samples = check_chains(nv, oracle, taps, p)
    buf.free()
    print(f"wideband: {chains} chains, {samples} samples")
    assert chains == 16 and samples == 16 * F * nv.FRAME_Y3
