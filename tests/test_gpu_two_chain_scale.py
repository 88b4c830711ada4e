"""The two-chain cascade kernels and tuned chains at hand-over scale (-m gpu): more streams than the chip holds waves, so
the frames of a stream go from work unit to work unit through the sealed state block, with BOTH chains' histories in it.

1. nvx_fir_cascade<true, 2>: 4096 streams x 12 frames at the raw rate (127 GB), both carriers in every stream: all 8192
   chains == the oracle, y3 bit patterns on a 64-stream spread, launch partition 5 + 7 and signal reports change no bit.
2. nvx_fir_cascade<false, 2>: 4096 streams x 12 frames at 252 kS/s, masks 1 / 2 / 3 mixed, launches of 5 + 7.
3. nvx_fir_cascade_cic3_2: 3000 streams x 3 frames, launches of 2 + 1, in the launcher's own form, waiting and pre-rolling.
4. Tuned chains (include/navtex_amd_tune.h) in those three forms, 3000 streams x 3 frames, every chain's y3 and bits as a
   digest == the restatement (tests/tune_ref.py); and each chain at the OTHER chain's nominal k.

Every comparison is ==; every check counts what it compared and the count is asserted (fullsize.verify_chains)."""
import hashlib
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

import fullsize
import signals
import tune_ref as tr

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

# the unit forms (Pipeline(forms=...)): the launcher's own choice / hand-over where a unit whose predecessor is still
# running waits for it / hand-over where such a unit pre-rolls instead (its first FIR1 output index goes back behind the
# frame start)
FORMS = (None, signals.HANDOVER_WAITING, signals.HANDOVER_PREROLLING)


def two_carrier_stream(nv, sid, rate):
    """signals.stream_params with two carriers: +14 kHz carries stream_text(sid), -14 kHz stream_text(sid + 50000), each
    with a bit offset (odd: off the middle between two 900 S/s instants) and a phase of its own.  Both bit offsets lie
    within one bit period and every text starts "ZCZC ", so the carriers get phasing of different lengths (1 and 8
    pairs of 14 bits): with stream_params' 40 pairs a 12-frame batch (384 bit periods) would hold nothing but phasing on
    both carriers and the oracle decodes both chains alike; with equal short phasing the 30-odd bits
    a 3-frame batch yields (periods 64 .. 96) would be the same characters.  So one carrier is in its text while the
    other is still phasing, and verify_chains' distinct_failures stays empty (tests/test_two_chain_scale_inputs.py)."""
    spb = rate // 100
    h = signals.mix32(signals.GLOBAL_SEED ^ signals.mix32(sid + 1))
    car = []
    for c, (freq, tid, n_phasing) in enumerate(((14000, sid, 1), (-14000, sid + 50000, 8))):
        hc = signals.mix32(h ^ (0x2C4A1E00 + c))
        off = (signals.mix32(hc ^ 0xA5A5A5A5) % spb) | 1
        car.append(dict(freq_hz=freq, bits=nv.sitor_encode(signals.stream_text(tid), n_phasing), bit_offset=off % spb,
                        phase0=signals.mix32(hc ^ 0x3C3C3C3C), amplitude=6000))
    return nv.make_stream(car, seed=h, noise_amp=1500)


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _ncpu():
    return min(16, len(os.sched_getaffinity(0)))


def _popcount(masks):
    return int(sum(bin(int(m)).count("1") for m in masks))


def _launches(nv, p, buf, pitch, plan, taps=(), forms=None):
    """Launch `plan` (frames per launch) from frame 0; with taps [(stream, chain)] every launch is fetched and their y3
    collected: returns {(s, c): y3 of all launches}.  forms: what the handle was made with -- every launch took it."""
    got = {key: [] for key in taps}
    f0 = 0
    for k in plan:
        p.process_resident(buf, pitch, f0, k); f0 += k
        if forms is not None:
            signals.assert_cascade_form(p, forms)
        if taps:
            p.fetch()
            for key in taps:
                got[key].append(p.debug_y3(*key)[: k * nv.FRAME_Y3].copy())
    p.fetch()
    return {key: np.concatenate(v) for key, v in got.items()}


def _all_bits(p, S):
    return {(s, c): p.bits(s, c) for s in range(S) for c in range(2)}


def _y3_against_pipes(nv, ob, buf, pitch, F, raw, order, masks, y3):
    """y3 {(s, c): [F * FRAME_Y3, 2]} as bit patterns against ob.Pipe fed the downloaded samples; returns (chains compared,
    [(s, c)] that differ)."""
    bad, n = [], 0
    for s in sorted({s for s, _ in y3}):
        iq = buf.download(pitch * 4, offset=s * pitch * 4, dtype=np.int16).reshape(-1, 2)
        ref = ob.Pipe(chain_mask=int(masks[s]), charlayer=False, tap_y3=F * nv.FRAME_Y3)
        if raw:
            ref.set_stage0(order); ref.push_raw(iq)
        else:
            ref.push(iq)
        for c in range(2):
            if (s, c) in y3:
                want = ref.y3(c)
                n += 1
                if want.shape[0] != F * nv.FRAME_Y3 or y3[(s, c)].shape != want.shape or not np.array_equal(_u64(y3[(s, c)]), _u64(want)):
                    bad.append((s, c))
    return n, bad


def _spread_taps(S, masks):
    return [(s, c) for s in fullsize.spread(S, 64) for c in range(2) if (int(masks[s]) >> c) & 1]


def _verdict(p, ob, buf, pitch, masks, raw, bits, ncpu):
    checked, bad, indistinct, secs = fullsize.verify_chains(ob, buf, pitch, pitch, raw, masks, lambda s, c: bits[(s, c)], ncpu)
    return dict(checked=checked, n_bad=len(bad), bad=bad[:20], indistinct=indistinct[:20], secs=round(secs, 1), ties=list(p.tie_stats()),
                seals=list(p.integrity_stats()[:2]), launches=p.wait_stats()[2])


# ------------------------------------------------------------------------------------------------ the runs (parent or child)
def run_raw_total(nv, ob, S=4096, F=12, ncpu=16, extras=True, buf=None, forms=None):
    """Test 1: S two-carrier streams x F frames at the raw rate, chain_mask 3, one launch.  extras: the y3 spread, the 5 + 7
    partition and the run with signal reports on.  buf: the input buffer of S * F * FRAME_RAW * 4 bytes, allocated by the
    caller (who alone decides what a failed allocation means) or, in a child process, here; it is freed here either way."""
    pitch = F * nv.FRAME_RAW
    if buf is None:
        buf = nv.DeviceBuffer(S * pitch * 4)
    try:
        nv.synth_device([two_carrier_stream(nv, s, nv.RATE_RAW) for s in range(S)], nv.RATE_RAW, pitch, buf, pitch)
        masks = [3] * S
        with nv.Pipeline(n_streams=S, raw_rate=True, chain_mask=3, max_frames=F, char_layer=False, forms=forms) as p:
            y3 = _launches(nv, p, buf, pitch, [F], _spread_taps(S, masks) if extras else (), forms)
            bits = _all_bits(p, S)
            rec = _verdict(p, ob, buf, pitch, masks, True, bits, ncpu)
            if extras:
                rec["y3_checked"], rec["y3_bad"] = _y3_against_pipes(nv, ob, buf, pitch, F, True, 1, masks, y3)
                p.reset()
                _launches(nv, p, buf, pitch, [5, 7])
                again = _all_bits(p, S)
                rec["partition_compared"] = len(again)
                rec["partition_differs"] = [k for k in bits if again[k] != bits[k]][:20]
                p.reset()
                p.enable_signal_report(True)
                _launches(nv, p, buf, pitch, [F])
                again = _all_bits(p, S)
                rec["report_differs"] = [k for k in bits if again[k] != bits[k]][:20]
                samples = [p.signal_report(s, c)["samples"] for s in range(S) for c in range(2)]
                rec["report_chains"] = len(samples)
                rec["report_samples_wrong"] = int(sum(n != F * nv.FRAME_Y3 - 8 for n in samples))
                rec["seals_all_runs"] = list(p.integrity_stats()[:2])
    finally:
        buf.free()
    return rec


def mixed_masks(S):
    return [int(m) for m in np.random.default_rng(41).choice([1, 2, 3], size=S, p=[.25, .25, .5])]


def run_252k_mixed(nv, ob, S=4096, F=12, ncpu=16, extras=True, forms=None):
    """Test 2: S two-carrier streams x F frames at 252 kS/s, masks 1 / 2 / 3 mixed, launches of 5 + 7."""
    pitch = F * nv.FRAME_IN
    masks = mixed_masks(S)
    buf = nv.DeviceBuffer(S * pitch * 4)
    try:
        nv.synth_device([two_carrier_stream(nv, s, nv.RATE_IN) for s in range(S)], nv.RATE_IN, pitch, buf, pitch)
        with nv.Pipeline(n_streams=S, raw_rate=False, chain_masks=masks, max_frames=7, char_layer=False, forms=forms) as p:
            y3 = _launches(nv, p, buf, pitch, [5, 7], _spread_taps(S, masks) if extras else (), forms)
            bits = _all_bits(p, S)
            rec = _verdict(p, ob, buf, pitch, masks, False, bits, ncpu)
            if extras:
                rec["y3_checked"], rec["y3_bad"] = _y3_against_pipes(nv, ob, buf, pitch, F, False, 1, masks, y3)
    finally:
        buf.free()
    return rec


def run_cic3_hand_over(nv, ob, S=3000, ncpu=16, forms=None):
    """Test 3: S two-carrier streams x 3 frames at the raw rate through the third-order stage 0, launches of 2 + 1."""
    F = 3
    pitch = F * nv.FRAME_RAW
    masks = [3] * S
    buf = nv.DeviceBuffer(S * pitch * 4)
    try:
        nv.synth_device([two_carrier_stream(nv, s, nv.RATE_RAW) for s in range(S)], nv.RATE_RAW, pitch, buf, pitch)
        with nv.Pipeline(n_streams=S, raw_rate=True, chain_mask=3, max_frames=2, char_layer=False, stage0_order=3, forms=forms) as p:
            _launches(nv, p, buf, pitch, [2, 1], forms=forms)
            rec = _verdict(p, ob, buf, pitch, masks, 3, _all_bits(p, S), ncpu)
    finally:
        buf.free()
    return rec


# ---- test 4: tuned chains
KINDS = {"raw": (True, 1), "raw-cic3": (True, 3), "252k": (False, 1)}
TUNED_S, TUNED_F, TUNED_PLAN = 3000, 3, (2, 1)
# forced on the first streams: the ends of the range, 0, +-1, a k coprime to N, each chain at the OTHER chain's nominal k
# (begin_table_mix must send it to T, not to a reference table), both chains of a stream at one k
FORCED_K = {(0, 0): 8000, (0, 1): -8000, (1, 0): 0, (1, 1): 1, (2, 0): -1, (2, 1): 4481, (3, 0): -4480, (3, 1): 4480, (4, 0): 1234, (4, 1): 1234}


def tuned_ks(S=TUNED_S):
    """[S, 2] k per chain and the mask of the chains LEFT at their nominal k (no nvx_set_carrier call for them)."""
    ks = np.random.default_rng(7).integers(-8000, 8001, size=(S, 2))
    left = (np.arange(2 * S).reshape(S, 2) % 5) == 0               # every fifth chain
    for (s, c), k in FORCED_K.items():
        ks[s, c] = k; left[s, c] = False
    ks[left[:, 0], 0] = tr.NOMINAL[0]
    ks[left[:, 1], 1] = tr.NOMINAL[1]
    return ks, left


def _tuned_streams(nv, rate, S):
    return [signals.stream_params(nv, 500 + s, rate, freq_hz=[14000, -14000, 3000][s % 3])[0] for s in range(S)]


def _digest(y3, bits):
    return hashlib.sha256(np.ascontiguousarray(y3, dtype=np.float64).tobytes() + bits.encode()).hexdigest()


def run_tuned(nv, ob, kind, out_path, untuned=False, S=TUNED_S, forms=None):
    """One child of test 4: the tuned handle over S streams x 3 frames in launches of 2 + 1; one digest per chain over its y3 of
    both launches and its bits, written to out_path as JSON.  untuned: the same batch through an untuned handle too, and the
    digests of the chains left at their nominal k from it."""
    raw, order = KINDS[kind]
    rate, frame = (nv.RATE_RAW, nv.FRAME_RAW) if raw else (nv.RATE_IN, nv.FRAME_IN)
    pitch = TUNED_F * frame
    ks, left = tuned_ks(S)
    chains = [(s, c) for s in range(S) for c in range(2)]
    buf = nv.DeviceBuffer(S * pitch * 4)
    rec = dict(kind=kind)
    try:
        nv.synth_device(_tuned_streams(nv, rate, S), rate, pitch, buf, pitch)
        for tuned in ((True, False) if untuned else (True,)):
            with nv.Pipeline(n_streams=S, raw_rate=raw, chain_mask=3, max_frames=max(TUNED_PLAN), char_layer=False, stage0_order=order, forms=forms) as p:
                if tuned:
                    rec["carrier_bad"] = [(s, c) for s, c in chains if not left[s, c] and p.set_carrier(s, c, int(ks[s, c]) * 3.125) != int(ks[s, c]) * 3.125][:20]
                    rec["carriers_set"] = int((~left).sum())
                y3 = _launches(nv, p, buf, pitch, TUNED_PLAN, chains, forms)
                dig = {f"{s},{c}": _digest(y3[(s, c)], p.bits(s, c)) for s, c in chains if tuned or left[s, c]}
                rec["digests" if tuned else "untuned_digests"] = dig
                rec["seals" if tuned else "untuned_seals"] = list(p.integrity_stats()[:2])
                rec["launches"] = p.wait_stats()[2]
    finally:
        buf.free()
    Path(out_path).write_text(json.dumps(rec))
    return dict(kind=kind, digests=len(rec["digests"]), seals=rec["seals"])


def restate_tuned(nv, kind, S=TUNED_S):
    """{"s,c": digest} of every chain from the restatement (tests/tune_ref.py), 16 threads (the oracle's C calls release the GIL)."""
    raw, order = KINDS[kind]
    rate, frame = (nv.RATE_RAW, nv.FRAME_RAW) if raw else (nv.RATE_IN, nv.FRAME_IN)
    ks, _left = tuned_ks(S)
    streams = _tuned_streams(nv, rate, S)

    def want(s):
        y1 = tr.front(nv.synth_host(streams[s], rate, TUNED_F * frame), raw, order)
        out = []
        for c in range(2):
            y3 = tr.chain(y1, c, int(ks[s, c]))
            assert y3.shape[0] == TUNED_F * nv.FRAME_Y3
            out.append(_digest(y3, tr.decode(y3)))
        return out
    with ThreadPoolExecutor(16) as ex:
        return {f"{s},{c}": d for s, pair in enumerate(ex.map(want, range(S))) for c, d in enumerate(pair)}


# ------------------------------------------------------------------------------------------------ children
CHILD = '''
import sys, json
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import navtex_amd as nv, oracle_binding as ob
import test_gpu_two_chain_scale as T
print(json.dumps(getattr(T, sys.argv[2])(nv, ob, **json.loads(sys.argv[3]))))
'''


def _child(tmp_path, func, kwargs, forms, timeout):
    """func(nv, oracle, forms=forms, **kwargs) of this module in a fresh process (a second batch of this size needs an address
    space of its own); the child asserts that its launches took `forms`; its last stdout line is its JSON answer."""
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    t0 = time.perf_counter()
    out = subprocess.run([sys.executable, str(script), str(ROOT), func, json.dumps(dict(kwargs, forms=forms))], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, (forms, out.stderr[-3000:])
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    print(f"{func} {kwargs} {forms}: {rec} ({time.perf_counter() - t0:.0f} s)")
    return rec


# ------------------------------------------------------------------------------------------------ tests
def test_full_size_two_chain_total_parity_raw_rate(nv, oracle, tmp_path):
    """4096 streams x 12 frames at 2.016 MS/s, both carriers in every stream, chain_mask 3: ALL 8192 chains == the oracle in
    the form the launcher picks and, in a second process, with independent units; y3 of 128 chains as bit patterns; the
    launch partition and the signal reports change nothing."""
    S, F = 4096, 12
    try:                                                         # the input allocation alone may skip: every other error fails
        buf = nv.DeviceBuffer(S * F * nv.FRAME_RAW * 4)
    except nv.NvxError:
        pytest.skip("not enough device memory for the full-size batch")
    rec = run_raw_total(nv, oracle, S, F, _ncpu(), buf=buf)
    print(f"two-chain total parity: {rec}")
    assert rec["indistinct"] == [] and rec["n_bad"] == 0 and rec["checked"] == 2 * S, rec
    near, evals, margin = rec["ties"]
    assert near == 0 and evals > 2 * S * 250 and margin > 2.0 ** -40
    assert rec["seals"] == [0, 0] and rec["seals_all_runs"] == [0, 0]
    assert rec["y3_bad"] == [] and rec["y3_checked"] == 2 * len(fullsize.spread(S, 64)) == 128
    assert rec["partition_differs"] == [] and rec["partition_compared"] == 2 * S       # the library against itself: beside the oracle, never instead
    assert rec["report_differs"] == [] and rec["report_samples_wrong"] == 0 and rec["report_chains"] == 2 * S
    child = _child(tmp_path, "run_raw_total", dict(S=S, F=F, ncpu=_ncpu(), extras=False), signals.INDEPENDENT, 900)
    assert child["indistinct"] == [] and child["n_bad"] == 0 and child["checked"] == 2 * S, child
    assert child["ties"][0] == 0 and child["ties"][1] > 2 * S * 250 and child["ties"][2] > 2.0 ** -40 and child["seals"] == [0, 0]


def test_two_chain_at_scale_252k_mixed_masks(nv, oracle, tmp_path):
    """4096 streams x 12 frames at 252 kS/s, both carriers in every stream, masks 1 / 2 / 3 mixed (the two-chain kernel runs
    streams that decode one chain only), launches of 5 + 7: every chain inside its mask == the oracle, every chain outside
    is empty; y3 on a 64-stream spread; again with independent units."""
    S, F = 4096, 12
    masks = mixed_masks(S)
    chains = _popcount(masks)
    assert S < chains < 2 * S and {1, 2, 3} == set(masks)
    rec = run_252k_mixed(nv, oracle, S, F, _ncpu())
    print(f"252 kS/s mixed masks: {chains} chains: {rec}")
    assert rec["indistinct"] == [] and rec["n_bad"] == 0 and rec["checked"] == chains, rec
    near, evals, margin = rec["ties"]
    assert near == 0 and evals > chains * 250 and margin > 2.0 ** -40
    assert rec["seals"] == [0, 0] and rec["launches"] == 2
    assert rec["y3_bad"] == [] and rec["y3_checked"] == _popcount([masks[s] for s in fullsize.spread(S, 64)])
    child = _child(tmp_path, "run_252k_mixed", dict(S=S, F=F, ncpu=_ncpu(), extras=False), signals.INDEPENDENT, 900)
    assert child["indistinct"] == [] and child["n_bad"] == 0 and child["checked"] == chains, child
    assert child["ties"][0] == 0 and child["ties"][1] > chains * 250 and child["ties"][2] > 2.0 ** -40 and child["seals"] == [0, 0]


def test_third_order_two_chain_hand_over_across_launches(nv, tmp_path):
    """3000 streams x 3 frames through nvx_fir_cascade_cic3_2 in launches of 2 + 1, in the launcher's own form, with waiting
    units and with pre-rolling units: all 6000 chains == the oracle (third-order stage 0) in each."""
    S = 3000
    for forms in FORMS:
        rec = _child(tmp_path, "run_cic3_hand_over", dict(S=S, ncpu=_ncpu()), forms, 600)
        assert rec["indistinct"] == [] and rec["n_bad"] == 0 and rec["checked"] == 2 * S, (forms, rec)
        assert rec["launches"] == 2 and rec["seals"] == [0, 0], (forms, rec)
        # 3 frames are 864 samples at 900 S/s; a chain's bit-timing window is primed after 574 of them and is evaluated once
        # per bit period of 9 from there: 32 evaluations per chain, of which 25 are asked for; the margin as at full size
        near, evals, margin = rec["ties"]
        assert near == 0 and evals > 2 * S * 25 and margin > 2.0 ** -40, (forms, rec["ties"])


@pytest.mark.parametrize("kind", list(KINDS))
def test_tuned_chains_in_the_many_streams_form(nv, kind, tmp_path):
    """3000 streams x 3 frames, both chains of every stream on a k of their own (a fifth left nominal), launches of 2 + 1, in
    the launcher's own form, waiting and pre-rolling: every chain's y3 of both launches and bits == the restatement; the
    chains left at their nominal k == an untuned handle's, whatever their sibling chain does."""
    S = TUNED_S
    ks, left = tuned_ks(S)
    assert ks[3, 0] == tr.NOMINAL[1] and ks[3, 1] == tr.NOMINAL[0] and ks[4, 0] == ks[4, 1] and abs(ks).max() == 8000
    n_left = int(left.sum())
    assert n_left == 2 * S // 5 - 2                                 # every fifth of 6000, less the two that are forced
    t0 = time.perf_counter()
    want = restate_tuned(nv, kind, S)
    print(f"restatement of {len(want)} chains: {time.perf_counter() - t0:.0f} s")
    # no two chains alike (a swapped pair would show) but the two of stream 4, which run at one k on one input
    assert len(want) == 2 * S and len(set(want.values())) == 2 * S - 1 and want["4,0"] == want["4,1"]
    for i, forms in enumerate(FORMS):
        out = tmp_path / f"digests{i}.json"
        _child(tmp_path, "run_tuned", dict(kind=kind, out_path=str(out), untuned=(i == 0), S=S), forms, 600)
        rec = json.loads(out.read_text())
        got = rec["digests"]
        bad = [key for key in want if got.get(key) != want[key]]
        assert bad == [] and len(got) == len(want) == 2 * S, (forms, len(bad), bad[:20])
        assert rec["carrier_bad"] == [] and rec["carriers_set"] == 2 * S - n_left, forms
        assert rec["seals"] == [0, 0] and rec["launches"] == 2, (forms, rec["seals"])
        if i == 0:
            un = rec["untuned_digests"]
            nominal = [f"{s},{c}" for s in range(S) for c in range(2) if left[s, c]]
            assert sorted(un) == sorted(nominal) and len(un) == n_left
            assert [key for key in nominal if un[key] != got[key]] == [] and rec["untuned_seals"] == [0, 0]


@pytest.mark.parametrize("mask", [1, 2, 3])
@pytest.mark.parametrize("kind", list(KINDS))
def test_each_chain_at_the_other_chains_nominal_k(nv, oracle, kind, mask):
    """Chain 0 at -14 kHz (k = -4480, chain 1's nominal) and chain 1 at +14 kHz: not the reference mixer (carrier() says
    so), y3 and bits == the restatement's tuned mixer -- and y3 is NOT what the opposite chain's reference mixer gives."""
    raw, order = KINDS[kind]
    rate, frame = (nv.RATE_RAW, nv.FRAME_RAW) if raw else (nv.RATE_IN, nv.FRAME_IN)
    S, F, plan = 3, 3, (2, 1)
    pitch = F * frame
    iqs = [nv.synth_host(st, rate, pitch) for st in _tuned_streams(nv, rate, S)]
    buf = nv.DeviceBuffer(S * pitch * 4)
    for s in range(S):
        buf.upload(iqs[s], s * pitch * 4)
    chains = [(s, c) for s in range(S) for c in range(2) if (mask >> c) & 1]
    with nv.Pipeline(n_streams=S, raw_rate=raw, chain_masks=[mask] * S, max_frames=2, char_layer=False, stage0_order=order) as p:
        for s, c in chains:
            hz = -14000.0 if c == 0 else 14000.0
            assert p.set_carrier(s, c, hz) == hz and p.carrier(s, c) == (hz, False)
        y3 = _launches(nv, p, buf, pitch, plan, chains)
        bits = {key: p.bits(*key) for key in chains}
        assert p.integrity_stats()[:2] == (0, 0)
    buf.free()
    for s, c in chains:
        y1 = tr.front(iqs[s], raw, order)
        want = tr.chain(y1, c, tr.NOMINAL[1 - c])
        assert y3[(s, c)].shape == want.shape == (F * nv.FRAME_Y3, 2)
        assert np.array_equal(_u64(y3[(s, c)]), _u64(want)) and bits[(s, c)] == tr.decode(want), (s, c)
        # Found on the CPU for these inputs (all three kinds, streams 500 .. 502): T at multiples of 2240 and the reference
        # mixer's nine entries differ in the last bits of 15 of their 18 numbers, and the two y3 differ in 1508 .. 1728 of
        # their 1728 words (relative difference <= 2e-14; the bits are the same) -- so a chain sent to the opposite
        # chain's reference table would show here and nowhere in the bits
        other = oracle.fir3(oracle.fir2(oracle.mix(y1, 1 - c)))
        assert other.shape == want.shape and not np.array_equal(_u64(want), _u64(other))
        assert not np.array_equal(_u64(y3[(s, c)]), _u64(other)), (s, c)
