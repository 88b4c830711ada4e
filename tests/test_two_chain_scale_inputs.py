"""The checker and the inputs of tests/test_gpu_two_chain_scale.py, on the CPU: fullsize.verify_chains over a numpy-backed
stand-in for DeviceBuffer, with the "GPU" answered by oracle_binding.Pipe -- it passes what is right, reports exactly the
(stream, chain) that was corrupted, a chain answered with its sibling's bits and a chain that should be silent; and the
two carriers of two_carrier_stream decode to different, non-empty bit strings (what the GPU tests rely on)."""
import numpy as np
import pytest

import fullsize
from test_gpu_two_chain_scale import two_carrier_stream


class HostBuffer:
    """DeviceBuffer's download() over host memory."""

    def __init__(self, a: np.ndarray):
        self.bytes = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        self.downloads = 0

    def download(self, nbytes, offset=0, dtype=np.uint8):
        assert 0 <= offset and offset + nbytes <= self.bytes.size
        self.downloads += 1
        return self.bytes[offset:offset + nbytes].copy().view(dtype)


def _pipe_bits(ob, iq, mask, raw):
    """{chain: bits} of one stream from ob.Pipe, decoding the chains of `mask`."""
    ref = ob.Pipe(chain_mask=mask, charlayer=False)
    if raw:
        ref.set_stage0(3 if raw == 3 else 1); ref.push_raw(iq)
    else:
        ref.push(iq)
    return {c: (ref.bits(c) if (mask >> c) & 1 else "") for c in range(2)}


@pytest.fixture(scope="module")
def batch(nv, oracle):
    """40 two-carrier streams x 12 frames at 252 kS/s with a pitch wider than the frames, mixed masks, and what a correct
    handle would answer."""
    S, F = 40, 12
    n = F * nv.FRAME_IN
    pitch = n + 256
    masks = [int(m) for m in np.random.default_rng(41).choice([1, 2, 3], size=S, p=[.25, .25, .5])]
    assert {1, 2, 3} == set(masks)
    host = np.zeros((S, pitch, 2), dtype=np.int16)
    for s in range(S):
        host[s, :n] = nv.synth_host(two_carrier_stream(nv, s, nv.RATE_IN), nv.RATE_IN, n)
    right = {}
    for s in range(S):
        for c, b in _pipe_bits(oracle, host[s, :n], masks[s], False).items():
            right[(s, c)] = b
    return dict(S=S, n=n, pitch=pitch, masks=masks, buf=HostBuffer(host), right=right, chains=sum(bin(m).count("1") for m in masks))


def _verify(oracle, batch, answer, chunk=16):
    return fullsize.verify_chains(oracle, batch["buf"], batch["pitch"], batch["n"], False, batch["masks"], answer, 2, chunk=chunk)


def test_a_correct_answer_passes_with_the_exact_count(oracle, batch):
    for chunk in (16, 64, 7):
        checked, bad, indistinct, secs = _verify(oracle, batch, lambda s, c: batch["right"][(s, c)], chunk)
        assert (checked, bad, indistinct) == (batch["chains"], [], []) and secs > 0
    assert batch["S"] < batch["chains"] < 2 * batch["S"]


def test_one_flipped_bit_is_reported_as_its_stream_and_chain(oracle, batch):
    s = next(s for s in range(batch["S"]) if batch["masks"][s] == 3 and s > 20)
    for c in (0, 1):
        wrong = dict(batch["right"])
        b = wrong[(s, c)]
        at = len(b) // 2
        wrong[(s, c)] = b[:at] + ("Y" if b[at] == "B" else "B") + b[at + 1:]
        checked, bad, indistinct, _ = _verify(oracle, batch, lambda s, c: wrong[(s, c)])
        assert (checked, bad, indistinct) == (batch["chains"], [(s, c)], [])
    wrong = dict(batch["right"])                              # a bit short is a difference too
    wrong[(0, 0 if batch["masks"][0] & 1 else 1)] = wrong[(0, 0 if batch["masks"][0] & 1 else 1)][:-1]
    assert _verify(oracle, batch, lambda s, c: wrong[(s, c)])[1] == [(0, 0 if batch["masks"][0] & 1 else 1)]


def test_chain_0s_bits_answered_for_chain_1_fail_every_two_chain_stream(oracle, batch):
    def swapped(s, c):
        return batch["right"][(s, 0)] if c == 1 and batch["masks"][s] == 3 else batch["right"][(s, c)]
    checked, bad, indistinct, _ = _verify(oracle, batch, swapped)
    both = [s for s in range(batch["S"]) if batch["masks"][s] == 3]
    assert len(both) > 10 and bad == [(s, 1) for s in both] and checked == batch["chains"] and indistinct == []


def test_bits_on_a_chain_outside_its_mask_are_reported(oracle, batch):
    s1 = next(s for s in range(batch["S"]) if batch["masks"][s] == 1)
    s2 = next(s for s in range(batch["S"]) if batch["masks"][s] == 2)
    wrong = dict(batch["right"])
    wrong[(s1, 1)] = "B"
    wrong[(s2, 0)] = batch["right"][(s2, 1)]
    checked, bad, indistinct, _ = _verify(oracle, batch, lambda s, c: wrong[(s, c)])
    assert sorted(bad) == sorted([(s1, 1), (s2, 0)]) and checked == batch["chains"] and indistinct == []


def test_an_input_that_cannot_tell_the_chains_apart_is_reported(nv, oracle):
    """Silence decodes to the same bits on both chains: distinct_failures names the stream."""
    n = 12 * nv.FRAME_IN
    host = np.zeros((2, n, 2), dtype=np.int16)
    host[1] = nv.synth_host(two_carrier_stream(nv, 1, nv.RATE_IN), nv.RATE_IN, n)
    right = {(s, c): b for s in range(2) for c, b in _pipe_bits(oracle, host[s], 3, False).items()}
    checked, bad, indistinct, _ = fullsize.verify_chains(oracle, HostBuffer(host), n, n, False, [3, 3], lambda s, c: right[(s, c)], 2)
    assert (checked, bad, indistinct) == (4, [], [0])
    with pytest.raises(ValueError):
        fullsize.verify_chains(oracle, HostBuffer(host), n, n, False, [3, 0], lambda s, c: "", 2)


@pytest.mark.parametrize("raw", [True, 3], ids=["raw", "raw-cic3"])
def test_raw_rate_and_both_stage0_forms(nv, oracle, raw):
    S, F = 4, 3
    n = F * nv.FRAME_RAW
    masks = [3, 1, 2, 3]
    host = np.stack([nv.synth_host(two_carrier_stream(nv, 100 + s, nv.RATE_RAW), nv.RATE_RAW, n) for s in range(S)])
    right = {(s, c): b for s in range(S) for c, b in _pipe_bits(oracle, host[s], masks[s], raw).items()}
    buf = HostBuffer(host)
    checked, bad, indistinct, _ = fullsize.verify_chains(oracle, buf, n, n, raw, masks, lambda s, c: right[(s, c)], 2)
    assert (checked, bad, indistinct) == (6, [], []) and buf.downloads == 1           # pitch == n_samples: one copy per chunk
    wrong = dict(right); wrong[(3, 1)] = right[(3, 1)][:-1] + ("Y" if right[(3, 1)][-1] == "B" else "B")
    assert fullsize.verify_chains(oracle, buf, n, n, raw, masks, lambda s, c: wrong[(s, c)], 2)[1] == [(3, 1)]


def test_the_two_carriers_decode_to_different_bits(nv, oracle):
    """64 ids spread over 0 .. 4095 at 252 kS/s: both oracle bit strings non-empty and different, over 12 frames and over
    the first 3 (the short batches of the GPU tests), and no two chains of the 64 streams alike."""
    n = 12 * nv.FRAME_IN
    seen = set()
    for sid in fullsize.spread(4096, 64):
        st = two_carrier_stream(nv, sid, nv.RATE_IN)
        assert st.n_carriers == 2 and st.carrier[0].bit_offset % 2 == 1 and st.carrier[1].bit_offset % 2 == 1
        assert st.carrier[0].phase0 != st.carrier[1].phase0
        iq = nv.synth_host(st, nv.RATE_IN, n)
        b = _pipe_bits(oracle, iq, 3, False)
        assert len(b[0]) > 300 and len(b[1]) > 300 and b[0] != b[1], sid
        seen.add(b[0]); seen.add(b[1])
        b = _pipe_bits(oracle, iq[:3 * nv.FRAME_IN], 3, False)
        assert len(b[0]) > 20 and len(b[1]) > 20 and b[0] != b[1], sid
    assert len(seen) == 128


def test_three_frames_at_the_raw_rate_tell_the_chains_apart(nv, oracle):
    """... and through both stage-0 forms at the raw rate, on 8 ids spread over 0 .. 2999."""
    for sid in fullsize.spread(3000, 8):
        iq = nv.synth_host(two_carrier_stream(nv, sid, nv.RATE_RAW), nv.RATE_RAW, 3 * nv.FRAME_RAW)
        for raw in (True, 3):
            b = _pipe_bits(oracle, iq, 3, raw)
            assert len(b[0]) > 20 and len(b[1]) > 20 and b[0] != b[1], (sid, raw)
