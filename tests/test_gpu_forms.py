"""The per-handle kernel-form hook (nvx_debug_set_forms / nvx_debug_last_forms, -m gpu): a forced form is the form that
runs, the handle reports what its last launch took, every form gives the same bits, and the form may change between the
launches of one handle.  The other GPU tests force forms the same way (Pipeline(forms=...), signals.CASCADE_FORMS) and
assert last_forms() after their launches; here the hook itself is pinned on the smallest launches that have a choice."""
import functools

import numpy as np
import pytest

import signals

pytestmark = pytest.mark.gpu

MASKS = [1, 3, 2]
CHAINS = [(s, c) for s in range(3) for c in range(2) if (MASKS[s] >> c) & 1]


def _plan(raw):
    """(frames of the first launch, of the second): 7 + 3 at 252 kS/s, two frames less at the raw rate"""
    return (5, 2) if raw else (7, 3)


@functools.lru_cache(maxsize=None)
def _input(nv, raw):
    rate, frame = (nv.RATE_RAW, nv.FRAME_RAW) if raw else (nv.RATE_IN, nv.FRAME_IN)
    return [nv.synth_host(signals.stream_params(nv, 520 + s, rate)[0], rate, sum(_plan(raw)) * frame) for s in range(3)]


@functools.lru_cache(maxsize=None)
def _cascade_run(nv, raw, forms, then=None):
    """Two launches of three streams with `forms` forced (then: the forms set between the launches of the ONE handle).
    Returns (y3 of both launches per chain as bytes, bits per chain, last_forms() after each launch)."""
    frame = nv.FRAME_RAW if raw else nv.FRAME_IN
    first, second = _plan(raw)
    pitch = (first + second) * frame
    buf = nv.DeviceBuffer(3 * pitch * 4)
    for s, iq in enumerate(_input(nv, raw)):
        buf.upload(iq, s * pitch * 4)
    y3, took = {sc: b"" for sc in CHAINS}, []
    with nv.Pipeline(n_streams=3, raw_rate=raw, chain_masks=MASKS, max_frames=first, char_layer=False, stage0_order=3 if raw else 1, forms=forms) as p:
        for f0, k in ((0, first), (first, second)):
            if f0 and then is not None:
                p.set_forms(*then)
            p.process_resident(buf, pitch, f0, k); p.fetch()
            took.append(p.last_forms())
            for sc in CHAINS:
                y3[sc] += p.debug_y3(*sc).tobytes()
        bits = {sc: p.bits(*sc) for sc in CHAINS}
    buf.free()
    return y3, bits, took


@pytest.mark.parametrize("raw", [False, True], ids=["252k", "raw-cic3"])
def test_forced_forms_run_and_agree(nv, oracle, raw):
    """Waiting hand-over, pre-rolling hand-over, independent units and the launcher's own choice: each launch reports the form
    that was asked for (three streams are fewer than the resident waves: the automatic choice is independent units), y3
    and bits are the same in all four and stream 0's are the oracle's."""
    runs = {forms: _cascade_run(nv, raw, forms) for forms in signals.CASCADE_FORMS + (signals.AUTOMATIC,)}
    for forms, (_y3, _bits, took) in runs.items():
        for got in took:
            assert all(want < 0 or have == want for have, want in zip(got[:2], forms[:2])), (forms, took)
    assert [t[0] for t in runs[signals.AUTOMATIC][2]] == [1, 1]
    assert [t[:2] for t in runs[signals.HANDOVER_WAITING][2]] == [(0, 0)] * 2 and [t[:2] for t in runs[signals.HANDOVER_PREROLLING][2]] == [(0, 1)] * 2
    y3, bits, _ = runs[signals.AUTOMATIC]
    for forms in signals.CASCADE_FORMS:
        assert runs[forms][0] == y3 and runs[forms][1] == bits, forms
    n3 = sum(_plan(raw)) * nv.FRAME_Y3
    ref = oracle.Pipe(chain_mask=MASKS[0], charlayer=False, tap_y3=n3)
    if raw:
        ref.set_stage0(3); ref.push_raw(_input(nv, raw)[0])
    else:
        ref.push(_input(nv, raw)[0])
    assert y3[(0, 0)] == np.ascontiguousarray(ref.y3(0)).tobytes() and len(y3[(0, 0)]) == n3 * 16
    assert bits[(0, 0)] == ref.bits(0) and len(bits[(0, 0)]) > 32 * (sum(_plan(raw)) - 3)


def test_form_changes_between_launches_of_one_handle(nv):
    """ONE handle, no reset: seven frames as independent units, then nvx_debug_set_forms, then three frames handed over by
    waiting units.  The report follows, the output is that of the runs above (the launcher's own rule mixes forms from
    launch to launch in the same way), and the request survives nvx_reset."""
    y3, bits, took = _cascade_run(nv, False, signals.INDEPENDENT, then=signals.HANDOVER_WAITING)
    assert took[0][0] == 1 and took[1][:2] == (0, 0), took
    want = _cascade_run(nv, False, signals.AUTOMATIC)
    assert y3 == want[0] and bits == want[1]
    with nv.Pipeline(n_streams=1, max_frames=2, char_layer=False, forms=signals.AUTOMATIC) as p:
        with pytest.raises(nv.NvxError) as e:                      # nothing launched yet
            p.last_forms()
        assert e.value.code == nv._native.ERR_STATE
        for bad in ((2, -1, -1), (-1, -2, -1), (-1, -1, 7)):
            with pytest.raises(nv.NvxError) as e:
                p.set_forms(*bad)
            assert e.value.code == nv._native.ERR_ARG
        buf = nv.DeviceBuffer(2 * nv.FRAME_IN * 4)
        buf.upload(_input(nv, False)[0][:2 * nv.FRAME_IN])
        p.set_forms(0, 0, -1)
        p.reset()
        p.process_resident(buf, 2 * nv.FRAME_IN, 0, 2); p.fetch()
        assert p.last_forms()[:2] == (0, 0)
        buf.free()


def test_front_form_request_and_report(nv):
    """One stream, both chains.  A launch of four frames has three tiles: one tile workgroup per chain with the tile form
    forced, none with the walk forced, one by the launcher's own rule (8 chain-frames <= 2560); a launch of one frame has
    one tile and walks whatever is asked.  Delta-phi, bits and the tie statistics are the same in all three."""
    F = 5
    iq = nv.synth_host(signals.stream_params(nv, 530, nv.RATE_IN)[0], nv.RATE_IN, F * nv.FRAME_IN)
    buf = nv.DeviceBuffer(F * nv.FRAME_IN * 4)
    buf.upload(iq)
    seen = {}
    for forms, wgs in ((signals.TILES, 1), (signals.WALK, 0), (signals.AUTOMATIC, 1)):
        with nv.Pipeline(n_streams=1, chain_mask=3, max_frames=4, char_layer=False, forms=forms) as p:
            p.enable_debug(True)
            p.process_resident(buf, F * nv.FRAME_IN, 0, 4); p.fetch()
            assert p.last_forms()[2] == wgs, (forms, p.last_forms())
            dphi = [p.debug_dphi(0, c).tobytes() for c in range(2)]
            p.process_resident(buf, F * nv.FRAME_IN, 4, 1); p.fetch()
            assert p.last_forms()[2] == 0, (forms, p.last_forms())
            dphi += [p.debug_dphi(0, c).tobytes() for c in range(2)]
            seen[forms] = (dphi, p.bits(0, 0), p.bits(0, 1), p.tie_stats())
    buf.free()
    assert seen[signals.TILES] == seen[signals.WALK] == seen[signals.AUTOMATIC]
    dphi, b0, _b1, ties = seen[signals.WALK]
    assert len(dphi[0]) == 4 * nv.FRAME_Y3 * 8 and len(dphi[2]) == nv.FRAME_Y3 * 8 and len(b0) > 32 and ties[1] > 0


def test_wideband_form_request_and_report(nv):
    """One wideband stream x 2 frames through the fused kernel as hand-over and as independent units: the handle reports the
    form, no dynamic pre-roll (-1: the kernel has none), and the 900 S/s output of all sixteen chains is the same."""
    n = 2 * nv.FRAME_RAW
    car = [dict(freq_hz=(k * 252000 if k < 4 else (k - 8) * 252000) + off, bits=nv.sitor_encode(f"ZCZC FM{k}{c}\nFORMS\nNNNN\n", 6),
                bit_offset=613 * (2 * k + c + 1), phase0=1234567 * (2 * k + c + 1) % 2**32, amplitude=1500)
           for k in range(8) for c, off in ((0, 14000), (1, -14000))]
    buf = nv.DeviceBuffer(n * 4)
    buf.upload(nv.synth_host(nv.make_stream(car, seed=81, noise_amp=500), nv.RATE_RAW, n))
    y3 = []
    for independent in (0, 1):
        with nv.Pipeline(n_streams=1, wideband=True, chain_mask=3, max_frames=2, char_layer=False, forms=(independent, -1, -1)) as p:
            p.process_resident(buf, n, 0, 2); p.fetch()
            assert p.last_forms()[:2] == (independent, -1)
            y3.append([p.debug_y3(s, c).tobytes() for s in range(8) for c in range(2)])
    buf.free()
    assert y3[0] == y3[1] and all(len(v) == 2 * nv.FRAME_Y3 * 16 for v in y3[0]) and len(set(y3[0])) == 16
