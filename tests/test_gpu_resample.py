"""The resampler (include/navtex_amd_resample.h) on the GPU (-m gpu): output words equal to the restatement
(tests/resample_ref.py, run with the plan's own taps) for every format, rate and kernel form, on signal, full-scale random
input, the rails, silence and float32 specials; chunked calls against one shot; push against resident; pitches and
out_first; reset; the error paths (no launch); 1024 streams of a frame each; and the product paths resample -> decode and
resample -> scan."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

import resample_ref as rr
import signals

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GPU_RATES = (2048000, 2400000, 768000, 250000, 96000)
FORMATS = (rr.CS16, rr.CU8, rr.CS8, rr.CF32)
FORMAT_IDS = ("cs16", "cu8", "cs8", "cf32")
BIG_L_RATE = 252252                       # L = 1000: the tap table does not fit the LDS and is read from global memory


@pytest.fixture(scope="module")
def rs(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_resample.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.resample
    return navtex_amd.resample


class _At:
    """A device address as Resampler.resident takes it."""
    def __init__(self, ptr):
        self.ptr = ptr


def _bits(nv, sid=3):
    return nv.sitor_encode(signals.stream_text(sid), 8)


def _inputs(nv, fi, fmt, n, seed):
    """Four streams in format fmt: a signal, full-scale random, the rails, silence."""
    rng = np.random.default_rng(seed)
    sig = rr.to_format(rr.cpfsk(_bits(nv), fi, n, seed=seed), fmt, gain=3.0 if fmt in (rr.CU8, rr.CS8) else 1.0)
    dt = rr.DTYPES[fmt]
    if fmt == rr.CF32:
        rnd = rng.uniform(-1.3, 1.3, size=(n, 2)).astype(np.float32)
        special = np.array([np.nan, np.inf, -np.inf, 1e-42, -1e-42, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768,
                            32766.5 / 32768, 32767.5 / 32768, -32768.5 / 32768, 1.0, -1.0, 3e38, -3e38, 0.0, -0.0, 123.5 / 32768], dtype=np.float32)
        at = rng.integers(0, n, size=(400, 2))
        rnd[at[:, 0], at[:, 1] % 2] = special[rng.integers(0, len(special), size=400)]
        rnd[:len(special), 0] = special
        lo, hi = np.float32(-1.0), np.float32(32767.0 / 32768.0)
    else:
        info = np.iinfo(dt)
        rnd = rng.integers(info.min, info.max + 1, size=(n, 2)).astype(dt)
        lo, hi = info.min, info.max
    rails = np.empty((n, 2), dtype=dt)
    rails[:, 0] = np.where((np.arange(n) // 5) % 2, hi, lo)
    rails[:, 1] = lo
    rails[n // 2:, 1] = hi
    silence = np.zeros((n, 2), dtype=dt) if fmt != rr.CU8 else np.full((n, 2), 128, dtype=dt)
    return [sig, rnd, rails, silence]


def _run_resident(nv, r, rows, chunks, pitch_extra=0, out_first=0, sentinel=0x5a5a1234):
    """The rows ([n, 2] each, all of one length) through nvx_resample_resident in calls of `chunks` samples; every call's
    input is uploaded to the start of the input rows (rows are 16-byte aligned) as whole rows: behind a call's n_in samples
    the row is full scale up to the pitch (with pitch_extra = 0 that is the rounding to 8 alone), so a read behind n_in
    changes the output.  Returns int16 [streams, n_out, 2]."""
    ns, n = len(rows), len(rows[0])
    assert sum(chunks) == n and ns == r.n_streams
    bps = rows[0].dtype.itemsize * 2
    start, _ = r.position(0)
    total = rr.outputs_after(start + n, r.L, r.M) - rr.outputs_after(start, r.L, r.M)
    pitch_out = out_first + total + pitch_extra
    pitch_in = (max(max(chunks), 1) + 7) // 8 * 8 + 8 * pitch_extra
    d_in = nv.DeviceBuffer(ns * pitch_in * bps)
    d_out = nv.DeviceBuffer(ns * pitch_out * 4)
    d_out.upload(np.full(ns * pitch_out, sentinel, dtype=np.uint32))
    dt = rows[0].dtype
    block = np.empty((ns, pitch_in, 2), dtype=dt)
    pos = made = 0
    for c in chunks:
        block[:, c:] = 1.0 if dt == np.float32 else np.iinfo(dt).max
        for s in range(ns):
            block[s, :c] = rows[s][pos:pos + c]
        d_in.upload(block)
        got = r.resident(d_in, pitch_in, c, d_out, pitch_out, out_first + made)
        assert got == rr.outputs_after(start + pos + c, r.L, r.M) - rr.outputs_after(start + pos, r.L, r.M)
        pos, made = pos + c, made + got
    assert made == total and r.position(ns - 1) == (start + n, rr.outputs_after(start + n, r.L, r.M))
    words = d_out.download(ns * pitch_out * 4, dtype=np.uint32).reshape(ns, pitch_out)
    d_in.free(); d_out.free()
    assert np.all(words[:, :out_first] == sentinel) and np.all(words[:, out_first + total:] == sentinel), "words outside the span were written"
    return np.ascontiguousarray(words[:, out_first:out_first + total]).view(np.int16).reshape(ns, total, 2)


def _want(rows, fmt, taps, L, M):
    return [rr.resample_all(row, fmt, taps, L, M) for row in rows]


@pytest.mark.parametrize("form", [1, 2], ids=["per-stream", "spread"])
@pytest.mark.parametrize("fi", GPU_RATES + (BIG_L_RATE,))
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_output_equals_the_restatement(nv, rs, fmt, fi, form):
    """Signal, full-scale random (float32: with NaN, infinities, denormals and exact .5 ties), the rails and silence in one
    call; a pitch larger than the data and out_first > 0."""
    L, M, T, S, taps = rs.design(fi)
    n = 40013
    rows = _inputs(nv, fi, fmt, n, seed=fi % 1000 + fmt)
    want = _want(rows, fmt, taps, L, M)
    with rs.Resampler(fi, fmt, n_streams=len(rows)) as r:
        assert (r.L, r.M, r.T) == (L, M, T)
        r.set_form(form)
        got = _run_resident(nv, r, rows, [n], pitch_extra=3, out_first=7)
    for s in range(len(rows)):
        assert np.array_equal(got[s], want[s]), (s, int(np.argmax(np.any(got[s] != want[s], axis=1))))
    # silence: unsigned 8-bit has no zero (the 127.5 offset), its mid-scale 128 is the constant +128
    fill = rr.outputs_after(T - 1, L, M)
    assert np.all(want[3][fill:] == (128 if fmt == rr.CU8 else 0)) and want[1].any()


@pytest.mark.parametrize("fi,fmt", [(2048000, rr.CS16), (2048000, rr.CU8), (250000, rr.CS16), (96000, rr.CF32), (2400000, rr.CS8),
                                    (BIG_L_RATE, rr.CS16)])
def test_one_shot_equals_random_chunkings(nv, rs, fi, fmt):
    """Calls of 0, 1, T-2 and T-1 samples, calls that yield no output, and random cuts: the same words as one call."""
    L, M, T, S, taps = rs.design(fi)
    n = 30011
    rows = _inputs(nv, fi, fmt, n, seed=77)[:2]
    want = _want(rows, fmt, taps, L, M)
    rng = np.random.default_rng(fi + fmt)
    for trial in range(3):
        chunks = [0, 1, T - 2, T - 1, 1, 1, 0, 2, T - 1, T - 2, T, 1]
        rest = n - sum(chunks)
        while rest:
            c = int(min(rest, rng.choice([1, 3, T - 1, T + 1, int(rng.integers(1, 9000))])))
            chunks.append(c); rest -= c
        if trial:
            rng.shuffle(chunks)
        assert rr.exact_counts(fi, chunks) == [rs.out_count(fi, sum(chunks[:k]), c) for k, c in enumerate(chunks)]
        with rs.Resampler(fi, fmt, n_streams=2) as r:
            r.set_form(1 + trial % 2)
            got = _run_resident(nv, r, rows, chunks)
        for s in range(2):
            assert np.array_equal(got[s], want[s]), (trial, s, int(np.argmax(np.any(got[s] != want[s], axis=1))))


@pytest.mark.parametrize("fi,fmt", [(2048000, rr.CU8), (250000, rr.CS16), (768000, rr.CF32)])
def test_push_equals_resident_and_streams_pushed_apart_meet_again(nv, rs, fi, fmt):
    L, M, T, S, taps = rs.design(fi)
    n = 20000
    rows = _inputs(nv, fi, fmt, 2 * n, seed=5)[:3]
    want = _want(rows, fmt, taps, L, M)
    first = rr.outputs_after(n, L, M)
    with rs.Resampler(fi, fmt, n_streams=3) as r:
        # every stream pushed with a chunking of its own (so they read different history rows), up to the same position
        for s, cuts in enumerate(([n], [1, T - 1, n - T], [7, 0, 5000, 1, n - 5008])):
            pos, parts = 0, []
            for c in cuts:
                parts.append(r.push(s, rows[s][pos:pos + c])); pos += c
            out = np.concatenate(parts)
            assert out.dtype == np.int16 and np.array_equal(out, want[s][:first]), s
            assert r.position(s) == (n, first)
        got = _run_resident(nv, r, [row[n:] for row in rows], [n])
        for s in range(3):
            assert np.array_equal(got[s], want[s][first:]), s
        # a buffer too small: refused, nothing consumed
        small = np.empty((3, 2), dtype=np.int16)
        k = C.c_size_t(99)
        a = np.ascontiguousarray(rows[0][:4000])
        assert rs.lib.nvx_resample_push(r._h, 0, a.ctypes.data_as(C.c_void_p), 4000, small.ctypes.data_as(C.c_void_p), 3, C.byref(k)) == nv._native.ERR_ARG
        assert r.position(0) == (2 * n, rr.outputs_after(2 * n, L, M))


def test_reset_of_one_stream_leaves_the_others_alone_and_positions_must_agree(nv, rs):
    fi, fmt = 2048000, rr.CS16
    L, M, T, S, taps = rs.design(fi)
    n = 16384
    rows = _inputs(nv, fi, fmt, 2 * n, seed=9)[:2]
    want = _want(rows, fmt, taps, L, M)
    first = rr.outputs_after(n, L, M)
    with rs.Resampler(fi, fmt, n_streams=2) as r:
        got = _run_resident(nv, r, [row[:n] for row in rows], [n])
        assert all(np.array_equal(got[s], want[s][:first]) for s in range(2))
        r.reset(1)
        assert r.position(0) == (n, first) and r.position(1) == (0, 0)
        d = nv.DeviceBuffer(2 * n * 4); o = nv.DeviceBuffer(2 * n * 4)
        k = C.c_size_t()
        rc = rs.lib.nvx_resample_resident(r._h, d.ptr, n, n, o.ptr, n, 0, C.byref(k), None)
        assert rc == nv._native.ERR_STATE and b"same position" in rs.lib.nvx_resample_last_error()
        d.free(); o.free()
        # stream 1 starts anew: the first n samples of another signal give what a fresh stream gives
        again = r.push(1, rows[0][:n])
        assert np.array_equal(again, want[0][:first])
        got = _run_resident(nv, r, [rows[0][n:], rows[0][n:]], [n])
        assert np.array_equal(got[0], want[0][first:]) and np.array_equal(got[1], want[0][first:])
        r.reset()
        assert r.position(0) == (0, 0) and r.position(1) == (0, 0)
        got = _run_resident(nv, r, [row[:n] for row in rows], [n])
        assert all(np.array_equal(got[s], want[s][:first]) for s in range(2))


def test_span_errors_launch_nothing(nv, rs):
    ARG = nv._native.ERR_ARG
    fi, n = 2048000, 8192
    with rs.Resampler(fi, rr.CU8, n_streams=2) as r:
        outs = rs.out_count(fi, 0, n)
        d_in = nv.DeviceBuffer(2 * n * 2); d_out = nv.DeviceBuffer(2 * outs * 4)
        one_in = nv.DeviceBuffer(n * 2); one_out = nv.DeviceBuffer(outs * 4)
        r.timing(True)
        r.time_stats(reset=True)
        k = C.c_size_t()
        call = lambda *a: rs.lib.nvx_resample_resident(r._h, *a, C.byref(k), None)            # noqa: E731
        bad = {"more samples than the pitch": (d_in.ptr, n - 8, n, d_out.ptr, outs, 0),
               "outputs beyond the pitch": (d_in.ptr, n, n, d_out.ptr, outs - 1, 0),
               "out_first pushes them beyond it": (d_in.ptr, n, n, d_out.ptr, outs, 1),
               "input rows for one stream": (one_in.ptr, n, n, d_out.ptr, outs, 0),
               "output rows for one stream": (d_in.ptr, n, n, one_out.ptr, outs, 0),
               "misaligned input": (d_in.ptr + 4, n, n - 8, d_out.ptr, outs, 0),
               "misaligned output": (d_in.ptr, n, n, d_out.ptr + 2, outs, 0),
               "rows not 16-byte aligned": (d_in.ptr, n - 3, n - 8, d_out.ptr, outs, 0),
               "null input": (None, n, n, d_out.ptr, outs, 0),
               "null output": (d_in.ptr, n, n, None, outs, 0),
               "too many samples": (d_in.ptr, 2 ** 31, 2 ** 30 + 1, d_out.ptr, 2 ** 31, 0),
               "a pitch that wraps": (d_in.ptr, 2 ** 63, n, d_out.ptr, outs, 0),
               "out_first that wraps": (d_in.ptr, n, n, d_out.ptr, outs, 2 ** 64 - 8)}
        for name, args in bad.items():
            assert call(*args) == ARG, name
            assert rs.lib.nvx_resample_last_error() != b""
        assert r.time_stats() == (0.0, 0) and r.position(0) == (0, 0) and r.position(1) == (0, 0)
        # more outputs than an int holds: 2^30 samples at 96 kS/s are 2.8e9 outputs
        with rs.Resampler(96000, rr.CS16) as up:
            up.timing(True)
            assert rs.out_count(96000, 0, 2 ** 30) == 2 ** 30 * 21 // 8 > 2 ** 31 - 1
            k.value = 99
            assert rs.lib.nvx_resample_resident(up._h, d_in.ptr, 2 ** 30, 2 ** 30, d_out.ptr, 2 ** 32, 0, C.byref(k), None) == ARG, "too many outputs"
            assert rs.lib.nvx_resample_last_error() != b"" and k.value == 99
            assert up.time_stats() == (0.0, 0) and up.debug_last_launch()["launches"] == 0 and up.position(0) == (0, 0)
        assert call(d_in.ptr, n, 0, d_out.ptr, outs, 0) == 0 and k.value == 0 and r.time_stats()[1] == 0       # nothing to do: no launch
        assert call(d_in.ptr, n, n, d_out.ptr, outs, 0) == 0 and k.value == outs
        ms, launches = r.time_stats()
        assert launches == 1 and ms > 0.0
        r.timing(False)
        assert call(d_in.ptr, n, n, d_out.ptr, outs, 0) == 0 and r.time_stats(reset=True)[1] == 1 and r.time_stats() == (0.0, 0)
        for b in (d_in, d_out, one_in, one_out):
            b.free()
    with pytest.raises(nv.NvxError) as e:
        rs.Resampler(fi, rr.CS16, device=99)
    assert e.value.code == ARG
    with pytest.raises(nv.NvxError) as e:
        rs.Resampler(3200001)
    assert e.value.code == ARG


def test_scale_1024_streams_of_one_frame_each(nv, rs):
    """1024 streams x 655360 samples (one frame of 80640 outputs) at 2.048 MS/s, full-scale random with a seed each: every
    stream equals the restatement."""
    fi, ns = 2048000, 1024
    L, M, T, S, taps = rs.design(fi)
    n = fi * 8 // 25
    assert rs.out_count(fi, 0, n) == nv.FRAME_IN

    def row(s):
        return np.random.default_rng(4000 + s).integers(-32768, 32768, size=(n, 2)).astype(np.int16)
    d_in = nv.DeviceBuffer(ns * n * 4); d_out = nv.DeviceBuffer(ns * nv.FRAME_IN * 4)
    for s in range(ns):
        d_in.upload(row(s), s * n * 4)
    with rs.Resampler(fi, rr.CS16, n_streams=ns) as r:
        assert r.resident(d_in, n, n, d_out, nv.FRAME_IN) == nv.FRAME_IN
        got = d_out.download(ns * nv.FRAME_IN * 4, dtype=np.int16).reshape(ns, nv.FRAME_IN, 2)
    d_in.free(); d_out.free()

    def check(s):
        return np.array_equal(got[s], rr.resample_all(row(s), rr.CS16, taps, L, M))
    with ThreadPoolExecutor(16) as ex:
        ok = list(ex.map(check, range(ns)))
    assert all(ok), [s for s in range(ns) if not ok[s]][:10]


@pytest.mark.parametrize("fi,fmt", [(2048000, rr.CS16), (250000, rr.CS16), (2400000, rr.CU8)])
def test_resample_then_decode_on_the_device(nv, rs, oracle, fi, fmt):
    """resampler -> a raw_rate = 0 handle by nvx_process_resident on the handle's own stream: the message arrives, and the
    bits equal the oracle's fed the restatement's output."""
    L, M, T, S, taps = rs.design(fi)
    text = signals.stream_text(31)
    bits = nv.sitor_encode(text, 40)
    per_frame = fi * 8 // 25
    frames = (len(bits) + 300) * (fi // 100) // per_frame + 1
    n = frames * per_frame
    src = rr.to_format(rr.cpfsk(bits, fi, n, freq_hz=14000, amplitude=8000, noise_amp=1500, seed=31), fmt, gain=3.0 if fmt == rr.CU8 else 1.0)
    want = rr.resample_all(src, fmt, taps, L, M)
    assert len(want) == frames * nv.FRAME_IN
    ref = oracle.Pipe(chain_mask=1)
    ref.push(want)
    assert [m[2] for m in ref.messages] == [text]
    bps = src.dtype.itemsize * 2
    d_in = nv.DeviceBuffer(n * bps); d_out = nv.DeviceBuffer(len(want) * 4)
    d_in.upload(src)
    with rs.Resampler(fi, fmt) as r, nv.Pipeline(n_streams=1, chain_mask=nv.CHAIN_518, max_frames=8) as p:
        hs = p.hip_stream
        f0 = 0
        while f0 < frames:                              # eight frames at a time: resample, then decode, both on the handle's stream
            k = min(8, frames - f0)
            assert r.resident(_At(d_in.ptr + f0 * per_frame * bps), n, k * per_frame, d_out, len(want), f0 * nv.FRAME_IN, hip_stream=hs) == k * nv.FRAME_IN
            p.process_resident(d_out, len(want), f0, k, hip_stream=hs)
            f0 += k
        p.fetch()
        got_bits, got_msgs = p.bits(0, 0), [m[3] for m in p.messages]
        words = d_out.download(len(want) * 4, dtype=np.int16).reshape(-1, 2)
    d_in.free(); d_out.free()
    assert np.array_equal(words, want)
    assert got_bits == ref.bits(0) and got_msgs == [text]


def test_resample_then_scan_finds_the_carrier(nv, rs):
    """resampler -> nvx_scan_resident -> nvx_scan_find: a carrier put at +1000 Hz of a 2.048 MS/s unsigned 8-bit stream is
    found within the scan's 5 Hz."""
    import navtex_amd.scan as sc
    fi, frames = 2048000, 3
    n = frames * fi * 8 // 25
    src = rr.to_format(rr.cpfsk(_bits(nv, 12), fi, n, freq_hz=1000, amplitude=8000, noise_amp=1500, seed=12), rr.CU8, gain=3.0)
    d_in = nv.DeviceBuffer(n * 2); d_out = nv.DeviceBuffer(frames * nv.FRAME_IN * 4)
    d_in.upload(src)
    with rs.Resampler(fi, rr.CU8) as r:
        assert r.resident(d_in, n, n, d_out, frames * nv.FRAME_IN) == frames * nv.FRAME_IN
        row = sc.scan_resident(d_out, frames * nv.FRAME_IN, 0, frames, 1, False)[0]
    d_in.free(); d_out.free()
    hits = sc.find(row)
    assert len(hits) == 1 and abs(hits[0]["offset_hz"] - 1000.0) <= 5.0 and abs(hits[0]["shift_hz"] - 170.0) <= 15.0, hits
