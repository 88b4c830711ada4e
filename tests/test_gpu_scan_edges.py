"""The band scan's edges on the GPU (-m gpu): the forms, offsets, orders and streams tests/test_gpu_scan.py does not reach.
Every comparison is == on the rows' uint64 words against the restatement (tests/scan_ref.py); the form a case is meant
to take is asserted on what the host handed the launcher (nvx_scan_debug_last_launch), not on a copy of the host's rule.

  a  the form boundaries: 511 / 512 streams, 16 384 / 16 388 frame rows (form 2's 256 MB scratch at its limit)
  b  65 536 streams (form 2 forced, form 1 taken): streams behind byte 2^32, word 2^31 and word 2^32 of the operand
  c  first_frame behind byte 2^32 of one row, all three input kinds, both forms
  d  two streams at a pitch of 2^32 + 322 560 samples
  e  the order of the sums: 33 frames whose slots differ in power by up to nine decades
  f  a frame's row depends on that frame's samples alone
  g  calls on a caller's HIP streams, back to back, timed and untimed
  h  four host threads in the library at once

Long rows (b, c, d, f) are restated from a cut (scan_ref.power_row_of_cut); tests/test_scan.py holds that against the
restatement over the whole stream.  A stream's offset past 2^32 is carried by d (a pitch that alone passes 2^32 words) and
by b (65 536 short rows).  Where d's 34 GB allocation is refused it skips with the refusal's text, and b alone carries that
proof.  On the MI355X both ran (the allocation was granted; tests/README.md has the wall times)."""
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import scan_ref as sr
import signals
from test_gpu_scan import KINDS, KIND_IDS, _frame, _iq, _u64, _upload, sc            # noqa: F401  (sc: the fixture)

pytestmark = pytest.mark.gpu
FORMS = pytest.mark.parametrize("form", [1, 2], ids=["per-stream", "per-frame+fold"])
KINDS_P = pytest.mark.parametrize("raw,s0", KINDS, ids=KIND_IDS)
ROW_BYTES = sr.N * 8


class _At:
    """A device address where a DeviceBuffer is expected."""
    def __init__(self, ptr, device=0):
        self.ptr, self.device = ptr, device


def _rate(nv, raw):
    return nv.RATE_RAW if raw else nv.RATE_IN


def _scan(sc, ask, took, buf, pitch, f0, nf, ns, raw, s0=1):
    """scan_resident with form `ask` set; the launcher must have been handed form `took` with that form's grid and scratch."""
    sc.set_form(ask)
    before = sc.debug_last_launch()["launches"]
    rows = sc.scan_resident(buf, pitch, f0, nf, ns, raw, s0)
    last = sc.debug_last_launch()
    assert last["launches"] == before + 1 and last["form"] == took, (ask, took, last)
    if took == 1:
        assert last["grid"] == (ns, 1) and last["scratch_bytes"] == 0, last
    else:
        assert last["grid"] == (nf, ns) and last["scratch_bytes"] == ns * nf * ROW_BYTES, last
    return rows


def _same(got, want, what=""):
    assert np.array_equal(_u64(got), _u64(want)), (what, int(np.count_nonzero(_u64(got) != _u64(want))))


_memo = {}


def _memo_get(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def _tones(nv, rate, freqs, first_id, shift_hz=85):
    """A one-carrier stream per frequency: its own seed, phase and bit offset; shift_hz 0 is a pure tone."""
    bits = _memo_get("bits", lambda: nv.sitor_encode(signals.stream_text(1), 40))
    spb = rate // 100
    out = []
    for k, f in enumerate(freqs):
        h = signals.mix32(signals.GLOBAL_SEED ^ signals.mix32(first_id + k + 1))
        out.append(nv.make_stream([dict(freq_hz=int(f), shift_hz=shift_hz, bits=bits, bit_offset=(h % spb) | 1, phase0=signals.mix32(h ^ 0x3C3C3C3C))],
                                  seed=h, noise_amp=1500))
    return out


# ------------------------------------------------------------------------------------------------- a. the form boundaries
def test_form_boundaries_at_512_streams_and_16384_frame_rows(nv, sc):
    """4097 streams x 4 frames at 252 kS/s (5.3 GB), a seed and a carrier per stream.  Automatic: 511 streams take form 2,
    512 take form 1.  Form 2 forced: 4096 x 4 = 16 384 frame rows take it, with exactly 256 MB of scratch; 4097 x 4 fall back
    to form 1.  The three 4-frame results agree in every row of the first 4096 streams, and 16 streams of each call equal
    the restatement."""
    ns, frames = 4097, 4
    n = frames * nv.FRAME_IN
    freqs = np.random.default_rng(41).integers(-24000, 24001, size=ns)
    streams = _tones(nv, nv.RATE_IN, freqs, 5000)
    buf = nv.DeviceBuffer(ns * n * 4)
    nv.synth_device(streams, nv.RATE_IN, n, buf, n)
    one_511 = _scan(sc, 0, 2, buf, n, 0, 1, 511, False)
    assert sc.debug_last_launch()["grid"] == (1, 511)
    one_512 = _scan(sc, 0, 1, buf, n, 0, 1, 512, False)
    f2 = _scan(sc, 2, 2, buf, n, 0, frames, 4096, False)
    assert sc.debug_last_launch()["scratch_bytes"] == 268435456 and sc.debug_last_launch()["grid"] == (4, 4096)
    fb = _scan(sc, 2, 1, buf, n, 0, frames, 4097, False)
    assert sc.debug_last_launch()["scratch_bytes"] == 0 and sc.debug_last_launch()["grid"] == (4097, 1)
    f1 = _scan(sc, 1, 1, buf, n, 0, frames, 4096, False)
    buf.free()
    assert np.array_equal(_u64(f2), _u64(f1)) and np.array_equal(_u64(fb[:4096]), _u64(f1))
    assert np.array_equal(_u64(one_511), _u64(one_512[:511]))
    spread4 = [0, 1, 255, 510, 511, 512, 1023, 1024, 2047, 2048, 3071, 3583, 4094, 4095, 4096, 2999]
    spread1 = [0, 1, 2, 63, 64, 127, 128, 255, 256, 300, 383, 447, 500, 509, 510, 511]

    def want(s):
        y1 = sr.front(nv.synth_host(streams[s], nv.RATE_IN, n), False)
        return sr.power_row(y1, 0, frames), sr.power_row(y1, 0, 1)
    with ThreadPoolExecutor(16) as ex:
        wants = dict(zip(sorted(set(spread4 + spread1)), ex.map(want, sorted(set(spread4 + spread1)))))
    for s in spread4:
        _same(fb[s], wants[s][0], ("4 frames", s))
    for s in spread1:
        _same(one_512[s], wants[s][1], ("1 frame", s))
    assert not np.array_equal(_u64(fb[0]), _u64(fb[4096]))


# ----------------------------------------------------------------------------------------------------- b. 65 536 streams
B_NAMED = [0, 13315, 13316, 26630, 26631, 32767, 32768, 53260, 53261, 53262, 65534, 65535]


def test_65536_streams_fall_back_to_form_1_and_pass_2_to_32_words(nv, sc):
    """65 536 streams x 1 frame at 252 kS/s, pitch exactly one frame (21 GB), a pure tone in noise per stream, its frequency
    drawn from +-24 kHz.  Form 2 is forced and must not be taken (its grid would need y = 65 536): the launcher is handed
    form 1 with 65 536 workgroups.  Stream 13 316 is the first wholly behind byte 2^32 of the operand, 26 631 behind word
    2^31, 53 262 behind word 2^32 (13 315, 26 630 and 53 261 straddle them).  Every row's strongest bin lies within 2 bins
    of its tone's (the generator's frequency is exact, the Hann window's main lobe is +-2 bins), 64 streams equal the
    restatement word for word, and the 16 KiB behind the rows -- where a row 65 536 would land -- keep their sentinel."""
    ns, n = 65536, nv.FRAME_IN
    assert 13315 * n * 4 < 2 ** 32 < 13316 * n * 4 and 26630 * n < 2 ** 31 < 26631 * n and 53261 * n < 2 ** 32 < 53262 * n
    freqs = np.random.default_rng(65536).integers(-24000, 24001, size=ns)
    bins = np.rint(freqs / sr.BIN_HZ).astype(np.int64) + sr.N // 2
    streams = _tones(nv, nv.RATE_IN, freqs, 100000, shift_hz=0)
    spread = sorted(set(B_NAMED) | set(int(s) for s in np.linspace(0, ns - 1, 64 - len(B_NAMED) + 2)))
    assert len(spread) == 64 and set(B_NAMED) <= set(spread)
    with ThreadPoolExecutor(16) as ex:
        want = dict(zip(spread, ex.map(lambda s: sr.power_row_of_cut(nv.synth_host(streams[s], nv.RATE_IN, n), False, 1, 1), spread)))
    for s in spread:                                                           # the input's own condition, on the CPU
        assert abs(int(np.argmax(want[s])) - int(bins[s])) <= 2, (s, int(freqs[s]))
    buf = nv.DeviceBuffer(ns * n * 4)
    for s0 in range(0, ns, 32768):                                             # the generator's grid has the y limit too
        nv.synth_device(streams[s0:s0 + 32768], nv.RATE_IN, n, _At(buf.ptr + s0 * n * 4), n)
    power = nv.DeviceBuffer(ns * ROW_BYTES + 16384)
    sentinel = np.full(2048, 0x5A5A12345A5A1234, dtype=np.uint64)
    power.upload(sentinel, ns * ROW_BYTES)
    sc.set_form(2)
    before = sc.debug_last_launch()["launches"]
    sc.scan_resident_into(buf, n, 0, 1, ns, False, 1, power)
    last = sc.debug_last_launch()
    assert last["launches"] == before + 1 and last["form"] == 1 and last["grid"] == (65536, 1) and last["scratch_bytes"] == 0, last
    words = power.download(ns * ROW_BYTES + 16384, dtype=np.uint64)
    buf.free(); power.free()
    assert np.array_equal(words[ns * sr.N:], sentinel), "words behind the last row were written"
    rows = words[:ns * sr.N].view(np.float64).reshape(ns, sr.N)
    off = np.abs(np.argmax(rows, axis=1) - bins)
    assert off.max() <= 2, (int(np.argmax(off)), int(off.max()), int(np.count_nonzero(off > 2)))
    for s in spread:
        _same(rows[s], want[s], s)


# ------------------------------------------------------------------------------- c. first_frame behind byte 2^32 of a row
def _case_c(nv, raw, s0):
    frame = _frame(nv, raw)
    total, f0 = (1668, 1664) if raw else (13320, 13315)
    assert f0 * frame * 4 < 2 ** 32 < (f0 + 1) * frame * 4 and f0 + 3 < total
    st, _ = signals.stream_params(nv, 333, _rate(nv, raw), freq_hz=-11003)
    part = nv.synth_host(st, _rate(nv, raw), 5 * frame, (f0 - 1) * frame)    # frames f0 - 1 .. f0 + 3
    return total, f0, part, sr.power_row_of_cut(part[frame:], raw, s0, 3)


@FORMS
@KINDS_P
def test_first_frame_behind_byte_2_to_32_of_its_row(nv, sc, raw, s0, form):
    """One stream in a buffer of 13 320 frames at 252 kS/s (1668 at raw rate; 4.3 GB either way), of which only the five
    frames around byte 2^32 are uploaded; the three frames from the one that straddles the boundary are scanned."""
    total, f0, part, want = _memo_get(("c", raw, s0), lambda: _case_c(nv, raw, s0))
    frame = _frame(nv, raw)
    buf = nv.DeviceBuffer(total * frame * 4)
    buf.upload(part, (f0 - 1) * frame * 4)
    got = _scan(sc, form, form, buf, total * frame, f0, 3, 1, raw, s0)
    buf.free()
    assert want.any()
    _same(got[0], want, (raw, s0, form))


# ------------------------------------------------------------------------------------- d. a pitch beyond 2^32 samples
def test_two_streams_at_a_pitch_beyond_2_to_32_samples(nv, sc):
    """Two streams of four frames at 252 kS/s, 2^32 + 322 560 samples apart: 34 GB allocated, 2.6 MB of it written."""
    frames = 4
    n = frames * nv.FRAME_IN
    pitch = 2 ** 32 + n
    try:
        buf = nv.DeviceBuffer(2 * pitch * 4)
    except nv.NvxError as e:
        pytest.skip(f"no 34 GB device buffer: {e}")
    iqs = [_iq(nv, False, frames, 410 + s, f) for s, f in enumerate((9001, -3002))]
    for s, iq in enumerate(iqs):
        buf.upload(iq, s * pitch * 4)
    y1 = [sr.front(iq, False) for iq in iqs]
    for form in (1, 2):
        for f0, nf in ((0, 4), (1, 3)):
            got = _scan(sc, form, form, buf, pitch, f0, nf, 2, False)
            want = [sr.power_row(y, f0, nf) for y in y1]
            _same(got[1], want[1], (form, f0, "stream 1"))
            _same(got[0], want[0], (form, f0, "stream 0"))
            assert not np.array_equal(_u64(got[0]), _u64(got[1]))
    buf.free()


# ------------------------------------------------------------------------------------------- e. the order of the sums
E_FRAMES, E_SPANS = 33, ((0, 33), (1, 32), (5, 9))


def _stepped(nv, raw, seed):
    """33 frames of full-scale noise whose amplitude changes from slot to slot: a seeded permutation of 297 values that
    cover 1 ... 32 767 evenly on a logarithmic scale (a slot's power: nine decades)."""
    rng = np.random.default_rng(seed)
    slot = _frame(nv, raw) // sr.SLOTS
    amp = rng.permutation(np.rint(np.geomspace(1, 32767, E_FRAMES * sr.SLOTS)).astype(np.int32))
    assert amp.min() == 1 and amp.max() == 32767
    u = rng.integers(-32767, 32768, size=(E_FRAMES * sr.SLOTS, slot, 2), dtype=np.int32)          # |u * amp| < 2^30
    return ((u * amp[:, None, None]) // 32767).astype(np.int16).reshape(-1, 2)


def _other_orders(p):
    """The row of slot powers p [frames, 9, 2048] in three orders that are not the header's."""
    rows = []
    for f in range(p.shape[0]):
        row = np.zeros(sr.N)
        for j in range(sr.SLOTS):
            row = row + p[f, j]
        rows.append(row)
    down = np.zeros(sr.N)
    for row in rows[::-1]:
        down = down + row
    pair = list(rows)
    while len(pair) > 1:
        pair = [pair[i] + pair[i + 1] if i + 1 < len(pair) else pair[i] for i in range(0, len(pair), 2)]
    across = np.zeros(sr.N)
    for j in range(sr.SLOTS):
        col = np.zeros(sr.N)
        for f in range(p.shape[0]):
            col = col + p[f, j]
        across = across + col
    return {"frames descending": np.roll(down, sr.N // 2), "pairwise over frames": np.roll(pair[0], sr.N // 2),
            "slot j over all frames first": np.roll(across, sr.N // 2)}


def _case_e(nv, raw, s0):
    iqs = [_stepped(nv, raw, 700 + 10 * s0 + raw + 100 * s) for s in range(2)]
    y1 = [sr.front(iq, raw, s0) for iq in iqs]
    want = {(f0, nf): [sr.power_row(y, f0, nf) for y in y1] for f0, nf in E_SPANS}
    for (f0, nf), rows in want.items():                                        # the input's own condition, on the CPU
        for s, y in enumerate(y1):
            for name, other in _other_orders(sr.slot_powers(y, f0, nf)).items():
                assert not np.array_equal(_u64(other), _u64(rows[s])), f"{name} gives the same words for frames {f0}+{nf} of stream {s}: take another seed"
    return iqs, want


@FORMS
@KINDS_P
def test_the_sums_run_in_the_stated_order(nv, sc, raw, s0, form):
    """a frame's row is its nine slots summed in order from 0.0, the scan's row the frame rows summed in order.
    Two streams of 33 frames whose slots differ in power by up to nine decades, in a seeded permutation: on the
    restatement's own slot powers, frames descending, pairwise over frames and slot j over all frames first each change
    at least one word of every row compared here (asserted before the GPU is used)."""
    iqs, want = _memo_get(("e", raw, s0), lambda: _case_e(nv, raw, s0))
    pitch = E_FRAMES * _frame(nv, raw)
    buf = _upload(nv, iqs, pitch)
    for f0, nf in E_SPANS:
        got = _scan(sc, form, form, buf, pitch, f0, nf, 2, raw, s0)
        for s in range(2):
            _same(got[s], want[(f0, nf)][s], (f0, nf, s))
    buf.free()


# ------------------------------------------------------------------------------- f. a frame's row: that frame's samples
def _case_f(nv, raw, s0):
    iq = _iq(nv, raw, 2, 505, -17017, amplitude=12000)
    return iq, sr.power_row_of_cut(iq, raw, s0, 2)


@FORMS
@KINDS_P
def test_a_frames_row_depends_on_its_frame_alone(nv, sc, raw, s0, form):
    """The same two frames between silence; between full-scale alternating rails (the frames in front and behind, the
    pitch gap and both neighbouring streams' rows); at the very start of an allocation; and at the very end of one sized
    exactly.  The same words every time: the restatement of those two frames alone."""
    iq, want = _memo_get(("f", raw, s0), lambda: _case_f(nv, raw, s0))
    frame = _frame(nv, raw)
    pitch = 4 * frame + 4096
    rails = np.empty((3 * pitch, 2), dtype=np.int16)
    rails[:, 0] = np.where((np.arange(3 * pitch) // 5) % 2, 32767, -32768)
    rails[:, 1] = -1 - rails[:, 0]
    assert want.any()
    for name, fill in (("silence", np.zeros((3 * pitch, 2), dtype=np.int16)), ("rails", rails)):
        host = fill.copy()
        host[pitch + frame:pitch + 3 * frame] = iq
        buf = nv.DeviceBuffer(3 * pitch * 4)
        buf.upload(host)
        got = _scan(sc, form, form, buf, pitch, 1, 2, 3, raw, s0)
        buf.free()
        _same(got[1], want, name)
        for s in (0, 2):                                                       # the fill's own rows, both sides
            cut = host[s * pitch + frame:s * pitch + 3 * frame]
            _same(got[s], _memo_get(("f", raw, s0, name, s), lambda: sr.power_row_of_cut(cut, raw, s0, 2)), (name, s))
            assert got[s].any() == (name == "rails")
    start = nv.DeviceBuffer(2 * frame * 4)
    start.upload(iq)
    _same(_scan(sc, form, form, start, 2 * frame, 0, 2, 1, raw, s0)[0], want, "start of an allocation")
    start.free()
    end = nv.DeviceBuffer(3 * frame * 4)
    end.upload(np.concatenate([rails[:frame], iq]))
    _same(_scan(sc, form, form, end, 3 * frame, 1, 2, 1, raw, s0)[0], want, "end of an allocation")
    end.free()


# ------------------------------------------------------------------------------------------------ g. a caller's streams
def _case_g(nv):
    frames = 4
    iqs = [_iq(nv, False, frames, 810 + s, f) for s, f in enumerate((-21000, 4004, 12345))]
    y1 = [sr.front(iq, False) for iq in iqs]
    return iqs, y1


G_CALLS = ((0, 4), (1, 2), (2, 2), (0, 1), (3, 1), (1, 3), (0, 3), (2, 1))


def test_eight_calls_on_two_streams_without_a_host_wait(nv, sc):
    """Eight calls alternate between two non-null HIP streams and between forms 2 and 1, each into its own rows, with no
    host synchronisation in between; then the same again with timing events recorded on the callers' streams.  After one
    nvx_device_sync all sixteen results equal the restatement, the timing has counted 8 and the launcher 16."""
    iqs, y1 = _memo_get("g", lambda: _case_g(nv))
    pitch = 4 * nv.FRAME_IN
    buf = _upload(nv, iqs, pitch)
    hs = [nv.lib.nvx_stream_create(0), nv.lib.nvx_stream_create(0)]
    assert hs[0] and hs[1] and hs[0] != hs[1]
    outs = [nv.DeviceBuffer(3 * ROW_BYTES) for _ in range(16)]
    sc.time_stats(reset=True)
    start = sc.debug_last_launch()["launches"]
    try:
        for rep in range(2):
            sc.timing(rep == 1)
            for k, (f0, nf) in enumerate(G_CALLS):
                form = 2 - k % 2
                sc.set_form(form)
                sc.scan_resident_into(buf, pitch, f0, nf, 3, False, 1, outs[8 * rep + k], hs[k % 2])
                last = sc.debug_last_launch()
                assert last["form"] == form and last["launches"] == start + 8 * rep + k + 1, last
                assert last["grid"] == ((nf, 3) if form == 2 else (3, 1)) and last["scratch_bytes"] == (3 * nf * ROW_BYTES if form == 2 else 0), last
        assert nv.lib.nvx_device_sync(0) == 0
        ms, n = sc.time_stats()
        assert n == 8 and ms > 0.0 and sc.debug_last_launch()["launches"] == start + 16
        for rep in range(2):
            for k, (f0, nf) in enumerate(G_CALLS):
                got = outs[8 * rep + k].download(3 * ROW_BYTES, dtype=np.float64).reshape(3, sr.N)
                for s in range(3):
                    _same(got[s], sr.power_row(y1[s], f0, nf), (rep, k, s))
    finally:
        sc.timing(False)
        sc.time_stats(reset=True)
        nv.lib.nvx_device_sync(0)
        for h in hs:
            nv.lib.nvx_stream_destroy(0, h)
        for b in outs + [buf]:
            b.free()


def test_five_form_2_calls_on_one_stream_into_one_row_buffer(nv, sc):
    """Five form-2 calls on one non-null stream write the same rows from different frames, nothing waited for in between;
    the rows read at the end are the last call's.  Each call's scratch is allocated and released in stream order
    (hipMallocAsync / hipFreeAsync), so a later call may be handed the memory an earlier one still computes in -- correct
    only because the stream orders them.  This test cannot prove that order: kernels that happen to be over in time pass
    without it.  It is the only sequence in the suite whose result depends on it."""
    iqs, y1 = _memo_get("g", lambda: _case_g(nv))
    pitch = 4 * nv.FRAME_IN
    buf = _upload(nv, iqs, pitch)
    hs = nv.lib.nvx_stream_create(0)
    assert hs
    out = nv.DeviceBuffer(3 * ROW_BYTES)
    calls = ((0, 4), (1, 3), (3, 1), (0, 2), (2, 2))
    sc.set_form(2)
    try:
        for f0, nf in calls:
            sc.scan_resident_into(buf, pitch, f0, nf, 3, False, 1, out, hs)
            last = sc.debug_last_launch()
            assert last["form"] == 2 and last["grid"] == (nf, 3) and last["scratch_bytes"] == 3 * nf * ROW_BYTES, last
        assert nv.lib.nvx_device_sync(0) == 0
        got = out.download(3 * ROW_BYTES, dtype=np.float64).reshape(3, sr.N)
        for s in range(3):
            _same(got[s], sr.power_row(y1[s], *calls[-1]), s)
            assert not np.array_equal(_u64(got[s]), _u64(sr.power_row(y1[s], *calls[-2])))
    finally:
        nv.lib.nvx_device_sync(0)
        nv.lib.nvx_stream_destroy(0, hs)
        out.free(); buf.free()


# --------------------------------------------------------------------------------------------------- h. four host threads
def test_four_host_threads_in_the_library_at_once(nv, sc):
    """Four threads, each with its own input of 512 one-frame streams (eight different frames, repeated) and its own rows,
    make eight calls each with the form left automatic: 512 streams (form 1) and 3 to 9 streams (form 2) in turn.  Thread 0
    provokes an NVX_ERR_ARG between its calls.  Every row equals the same calls made from one thread (where each call's form
    is asserted) and the restatement; the failing thread reads its own error text, the others still read the text of the
    error each of them provoked before the first call; the launcher has counted exactly 32."""
    n = nv.FRAME_IN
    T, big = 4, 512
    frames = [[_iq(nv, False, 1, 900 + 8 * t + k, 1000 * (8 * t + k) - 15000) for k in range(8)] for t in range(T)]
    with ThreadPoolExecutor(16) as ex:
        want = list(ex.map(lambda iq: sr.power_row_of_cut(iq, False, 1, 1), [iq for fs in frames for iq in fs]))
    want = [np.stack(want[8 * t:8 * t + 8]) for t in range(T)]
    bufs = []
    for t in range(T):
        b = nv.DeviceBuffer(big * n * 4)
        b.upload(np.concatenate(frames[t] * (big // 8)))
        bufs.append(b)
    shapes = [big if k % 2 == 0 else 3 + k - 1 for k in range(8)]              # 512, 3, 512, 5, 512, 7, 512, 9
    outs = [[[nv.DeviceBuffer(ns * ROW_BYTES) for ns in shapes] for t in range(T)] for rep in range(2)]
    sc.set_form(0)
    ARG = nv._native.ERR_ARG
    try:
        for t in range(T):                                                     # one thread: the forms, call by call
            for k, ns in enumerate(shapes):
                sc.scan_resident_into(bufs[t], n, 0, 1, ns, False, 1, outs[0][t][k])
                assert sc.debug_last_launch()["form"] == (1 if ns == big else 2)
        assert nv.lib.nvx_device_sync(0) == 0
        start = sc.debug_last_launch()["launches"]
        gate = threading.Barrier(T)

        def work(t):
            assert sc.lib.nvx_scan_set_form(3 + t) == ARG                      # this thread's own error text
            mine = sc.lib.nvx_scan_last_error()
            assert f"form {3 + t} ".encode() in mine, mine
            gate.wait(20)
            seen = None
            for k, ns in enumerate(shapes):
                sc.scan_resident_into(bufs[t], n, 0, 1, ns, False, 1, outs[1][t][k])
                if t == 0 and k == 3:
                    assert sc.lib.nvx_scan_resident(0, bufs[t].ptr, n, 0, 0, 1, 0, 1, outs[1][t][k].ptr, None) == ARG
                    seen = sc.lib.nvx_scan_last_error()
            return mine, seen, sc.lib.nvx_scan_last_error()
        with ThreadPoolExecutor(T) as ex:
            texts = list(ex.map(work, range(T)))
        assert nv.lib.nvx_device_sync(0) == 0
        assert sc.debug_last_launch()["launches"] == start + 32
        assert b"nvx_scan_resident: bad argument" in texts[0][1] and texts[0][2] == texts[0][1]
        for t in range(1, T):
            assert texts[t][1] is None and texts[t][2] == texts[t][0] and texts[t][0] != texts[0][0], texts[t]
        assert len({texts[t][0] for t in range(T)}) == T
        for t in range(T):
            for k, ns in enumerate(shapes):
                one = outs[0][t][k].download(ns * ROW_BYTES, dtype=np.uint64).reshape(ns, sr.N)
                many = outs[1][t][k].download(ns * ROW_BYTES, dtype=np.uint64).reshape(ns, sr.N)
                assert np.array_equal(one, many), (t, k)
                assert np.array_equal(many, _u64(want[t])[np.arange(ns) % 8]), (t, k)
    finally:
        nv.lib.nvx_device_sync(0)
        for b in bufs + [o for rep in outs for per in rep for o in per]:
            b.free()
