"""The impulse noise blanker (include/navtex_amd_blank.h) on the GPU (-m gpu): output words equal to the restatement
(tests/blank_ref.py) for every format on signal with bursts, the rails, full-scale random input (float32 specials) and
silence; calls cut anywhere against one shot, a reset stream rejoining the others; the multi-chunk form against one chunk
per stream; 1024 streams; positions beyond 2^32; the parameters' ends and the bypass; push against resident; the error
paths (no launch); and the product paths blank -> decode and blank -> resample -> decode of the acceptance case."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

import blank_cases as bc
import blank_ref as br
import resample_ref as rr
import signals

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FORMATS = (br.CS16, br.CU8, br.CS8, br.CF32)
FORMAT_IDS = ("cs16", "cu8", "cs8", "cf32")
SENTINEL = 0x5a5a1234


@pytest.fixture(scope="module")
def bl(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_blank.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.blank
    return navtex_amd.blank


class _At:
    """A device address as Blanker.resident takes it."""
    def __init__(self, ptr):
        self.ptr = ptr


def _noise_with_bursts(n, seed, at=(), noise=1500, rate=6000):
    """int16 [n, 2]: uniform noise of +-noise, bursts of 1 .. 300 samples of +-30000 about every `rate` samples, and one
    (first, length) for every entry of `at`."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-noise, noise + 1, size=(n, 2)).astype(np.float64)
    spots = [(int(s), int(rng.integers(1, 301))) for s in rng.integers(0, max(1, n - 300), n // rate)] + list(at)
    for s, L in spots:
        x[s:s + L] += rng.uniform(-30000, 30000, size=(min(L, n - s), 2))
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def _inputs(nv, fmt, n, kind, seed):
    """Two streams of one kind in format fmt."""
    rng = np.random.default_rng(seed)
    dt = rr.DTYPES[fmt]
    gain = 3.0 if fmt in (br.CU8, br.CS8) else 1.0
    if fmt == br.CF32:
        lo, hi = np.float32(-1.0), np.float32(32767.0 / 32768.0)
    else:
        lo, hi = np.iinfo(dt).min, np.iinfo(dt).max
    if kind == "signal":
        bits = nv.sitor_encode(signals.stream_text(3), 8)
        rows = []
        for s in range(2):
            x = rr.cpfsk(bits, 252000, n, amplitude=300 if s else 8000, seed=seed + s).astype(np.float64)
            x += _noise_with_bursts(n, seed + 10 + s, noise=0, rate=4000)
            rows.append(rr.to_format(np.clip(x, -32768, 32767).astype(np.int16), fmt, gain=gain))
        return rows
    if kind == "rails":
        # quiet noise with stretches at the rails in the four combinations, and a row that never leaves them
        quiet = rr.to_format(_noise_with_bursts(n, seed, noise=600, rate=10 ** 9), fmt, gain=gain)
        combos = [(lo, lo), (lo, hi), (hi, lo), (hi, hi)]
        for k, s in enumerate(rng.integers(4096, n - 3000, 24)):
            quiet[s:s + int(rng.integers(1, 2500))] = combos[k % 4]
        rails = np.empty((n, 2), dtype=dt)
        rails[:, 0] = np.where((np.arange(n) // 5) % 2, hi, lo)
        rails[:, 1] = lo
        rails[n // 2:, 1] = hi
        return [quiet, rails]
    if kind == "random":
        rows = []
        for s in range(2):
            if fmt == br.CF32:
                rnd = rng.uniform(-1.3, 1.3, size=(n, 2)).astype(np.float32)
                special = np.array([np.nan, np.inf, -np.inf, 1e-42, -1e-42, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768,
                                    32766.5 / 32768, 32767.5 / 32768, -32768.5 / 32768, 1.0, -1.0, 3e38, -3e38, 0.0, -0.0, 123.5 / 32768], dtype=np.float32)
                at = rng.integers(0, n, size=(400, 2))
                rnd[at[:, 0], at[:, 1] % 2] = special[rng.integers(0, len(special), size=400)]
                rnd[:len(special), 0] = special
            else:
                rnd = rng.integers(int(lo), int(hi) + 1, size=(n, 2)).astype(dt)
            if s:                                          # full scale in short stretches over a quiet floor: detections everywhere
                keep = (np.arange(n) // 97) % 9 == 0
                rnd = np.where(keep[:, None], rnd, rr.to_format(_noise_with_bursts(n, seed, noise=400, rate=10 ** 9), fmt, gain=gain))
            rows.append(np.ascontiguousarray(rnd))
        return rows
    silence = np.zeros((n, 2), dtype=dt) if fmt != br.CU8 else np.full((n, 2), 128, dtype=dt)
    return [silence, silence.copy()]


def _run_resident(nv, b, rows, cuts, pitch_extra=0, out_first=0):
    """The rows ([n, 2] each, all of one length) through nvx_blank_resident in calls of `cuts` samples; every call's input is
    uploaded to the start of the input rows as whole rows: behind a call's n_in samples the row is full scale up to the pitch,
    so a read behind n_in changes the output.  Sentinels around every output row.  Returns int16 [streams, n, 2]."""
    ns, n = len(rows), len(rows[0])
    assert sum(cuts) == n and ns == b.n_streams
    dt = rows[0].dtype
    bps = dt.itemsize * 2
    pitch_out = out_first + n + pitch_extra
    pitch_in = (max(max(cuts), 1) + 7) // 8 * 8 + 8 * pitch_extra
    d_in = nv.DeviceBuffer(ns * pitch_in * bps)
    d_out = nv.DeviceBuffer(ns * pitch_out * 4)
    d_out.upload(np.full(ns * pitch_out, SENTINEL, dtype=np.uint32))
    block = np.empty((ns, pitch_in, 2), dtype=dt)
    start = b.position(0)
    pos = 0
    for c in cuts:
        block[:, c:] = 1.0 if dt == np.float32 else np.iinfo(dt).max
        for s in range(ns):
            block[s, :c] = rows[s][pos:pos + c]
        d_in.upload(block)
        b.resident(d_in, pitch_in, c, d_out, pitch_out, out_first + pos)
        pos += c
    assert b.position(ns - 1) == start + n
    words = d_out.download(ns * pitch_out * 4, dtype=np.uint32).reshape(ns, pitch_out)
    d_in.free(); d_out.free()
    assert np.all(words[:, :out_first] == SENTINEL) and np.all(words[:, out_first + n:] == SENTINEL), "words outside the span were written"
    return np.ascontiguousarray(words[:, out_first:out_first + n]).view(np.int16).reshape(ns, n, 2)


def _first_difference(got, want):
    return int(np.argmax(np.any(got != want, axis=1)))


# ------------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("kind", ["signal", "rails", "random", "silence"])
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_output_and_counters_equal_the_restatement(nv, bl, fmt, kind):
    """2 streams x 40 013 samples (39 blocks and a ragged one) in one call; a pitch larger than the data, out_first = 7 (the
    unaligned stores) and 8 (the aligned ones), sentinels around every row."""
    n = 40013
    rows = _inputs(nv, fmt, n, kind, seed=100 + fmt)
    refs = [br.blank(row, fmt) for row in rows]
    for out_first in (7, 8):
        with bl.Blanker(fmt, n_streams=2) as b:
            got = _run_resident(nv, b, rows, [n], pitch_extra=3 + out_first % 2, out_first=out_first)
            for s in range(2):
                want, ref = refs[s]
                assert np.array_equal(got[s], want), (out_first, s, _first_difference(got[s], want))
                assert b.stats(s) == (n, ref.detections, ref.blanked), (out_first, s)
    if kind == "silence":
        assert all(ref.detections == 0 and ref.blanked == 0 for _, ref in refs)
    else:                                                  # a row that is loud throughout sets its own level: nothing to detect there
        ref = refs[0 if kind == "rails" else 1][1]
        assert ref.detections > 0 and ref.blanked > ref.detections


# ------------------------------------------------------------------------------------------------------------------ (b)
CUTS = [4097, 1, 0, 1023, 1024, 1025, 31, 5119, 10, 12, 1, 0, 33, 2047, 4096, 4095, 8193]


@pytest.mark.parametrize("fmt", [br.CS16, br.CU8, br.CF32], ids=["cs16", "cu8", "cf32"])
def test_one_shot_equals_calls_cut_anywhere_and_a_reset_stream_rejoins(nv, bl, fmt):
    """A burst straddles the boundary behind the first four calls; a single detection sits on the last sample of the call
    of 5119, and its hold runs through the calls of 10 and 12 samples into the next.  Then stream 1 is reset, pushed alone up
    to the others' position, and all three go on together."""
    n1 = sum(CUTS) + 1500
    cuts = CUTS + [1500]
    gain = 3.0 if fmt == br.CU8 else 1.0
    edge = sum(CUTS[:5])
    spike = sum(CUTS[:8]) - 1
    rows = []
    for s in range(3):
        x = _noise_with_bursts(2 * n1, 40 + s, at=[(edge - 60, 200)], noise=700)
        x[spike - 400:spike + 400] = np.clip(x[spike - 400:spike + 400], -700, 700)
        x[spike] = (30000, -30000)
        rows.append(rr.to_format(x, fmt, gain=gain))
    refs = [br.blank(row, fmt) for row in rows]
    for s in range(3):
        ref = br.Blanker(fmt)
        ref.push(rows[s][:spike + 1])
        assert ref.d[-1] and not ref.d[-300:-1].any(), "the detection on the call's last sample"
        assert refs[s][1].gone[spike:spike + 33].all() and not refs[s][1].gone[spike + 33]
    with bl.Blanker(fmt, n_streams=3) as b:
        got = _run_resident(nv, b, [row[:n1] for row in rows], cuts)
        for s in range(3):
            assert np.array_equal(got[s], refs[s][0][:n1]), (s, _first_difference(got[s], refs[s][0][:n1]))
        b.reset(1)
        assert b.position(1) == 0 and b.position(0) == n1
        d = nv.DeviceBuffer(3 * 64 * 8); o = nv.DeviceBuffer(3 * 64 * 4)
        assert bl.lib.nvx_blank_resident(b._h, d.ptr, 64, 64, o.ptr, 64, 0, None) == nv._native.ERR_STATE
        assert b"same position" in bl.lib.nvx_blank_last_error()
        d.free(); o.free()
        # stream 1 starts anew on other data, alone and in calls of its own, up to where the others stand
        fresh = br.Blanker(fmt)
        other = rows[0][n1 - 7:2 * n1 - 7]
        pos = 0
        for c in (5000, 1, 1023, n1 - 6024):
            assert np.array_equal(b.push(1, other[pos:pos + c]), fresh.push(other[pos:pos + c])), pos
            pos += c
        assert b.position(1) == n1
        tail = [rows[0][n1:], rows[2][n1:2 * n1], rows[2][n1:]]
        got = _run_resident(nv, b, tail, [n1])
        assert np.array_equal(got[0], refs[0][0][n1:]) and np.array_equal(got[2], refs[2][0][n1:])
        assert np.array_equal(got[1], fresh.push(tail[1]))
        assert b.stats(0) == (2 * n1, refs[0][1].detections, refs[0][1].blanked)


# ------------------------------------------------------------------------------------------------------------------ (c)
def test_the_multi_chunk_form_equals_one_chunk_per_stream(nv, bl):
    """3 streams x 300 000 samples behind a first call of 777 (blocks and tiles apart): three workgroups per stream, the later
    ones behind a pre-roll of eight blocks.  Bursts in each block of both pre-rolls, one ending within `hold` of each chunk's
    first sample, and one filling a whole block in front of it.  The same input in calls of one chunk: the same words."""
    n, first, tile = 300000, 777, 4096
    starts = [32 * tile, 64 * tile]                          # of the later chunks, in samples of the second call
    rows = []
    for s in range(3):
        at = []
        for c in starts:
            at += [(first + c - 8192 + 1024 * k + 300 + 100 * s, 60) for k in range(8)]        # a burst in each pre-roll block
            at += [(first + c - 40 - s, 30)]                                                   # within hold of the chunk's first sample
            at += [(first + c - 3 * 1024 - 777 % 1024, 1024)]                                  # a whole block of the stream
        rows.append(_noise_with_bursts(first + n, 60 + s, at=at))
    refs = [br.blank(row) for row in rows]
    with bl.Blanker(br.CS16, n_streams=3) as b:
        got = _run_resident(nv, b, rows, [first, n])
        shape = b.debug_last_launch()
        assert shape == {"launches": 2, "chunks": 3, "blocks_per_chunk": 128, "preroll_blocks": 8, "form": 2}, shape
        for s in range(3):
            assert np.array_equal(got[s], refs[s][0]), (s, _first_difference(got[s], refs[s][0]))
            assert b.stats(s) == (first + n, refs[s][1].detections, refs[s][1].blanked)
    with bl.Blanker(br.CS16, n_streams=3) as b:
        one = _run_resident(nv, b, rows, [first, 100000, 100000, 100000])
        shape = b.debug_last_launch()
        assert shape["chunks"] == 1 and shape["form"] == 1 and shape["preroll_blocks"] == 0 and shape["launches"] == 4, shape
        assert np.array_equal(one, got)
    # the hold reaches across both chunk boundaries in the restatement, so the kernel's pre-roll is what carried it
    for s in range(3):
        for c in starts:
            assert refs[s][1].gone[first + c - 12:first + c + 8].all()


# ------------------------------------------------------------------------------------------------------------------ (d)
def test_scale_1024_streams_a_seed_each(nv, bl):
    ns, n = 1024, 8192

    def row(s):
        return _noise_with_bursts(n, 7000 + s, rate=1500)
    d_in = nv.DeviceBuffer(ns * n * 4); d_out = nv.DeviceBuffer(ns * n * 4)
    for s in range(ns):
        d_in.upload(row(s), s * n * 4)
    with bl.Blanker(br.CS16, n_streams=ns) as b:
        b.resident(d_in, n, n, d_out, n)
        got = d_out.download(ns * n * 4, dtype=np.int16).reshape(ns, n, 2)
        assert b.debug_last_launch()["form"] == 1
        stats = [b.stats(s) for s in (0, 511, 1023)]
    d_in.free(); d_out.free()

    def check(s):
        want, ref = br.blank(row(s))
        return np.array_equal(got[s], want), (n, ref.detections, ref.blanked)
    with ThreadPoolExecutor(16) as ex:
        res = list(ex.map(check, range(ns)))
    assert all(ok for ok, _ in res), [s for s in range(ns) if not res[s][0]][:10]
    assert stats == [res[s][1] for s in (0, 511, 1023)] and sum(r[1][1] for r in res) > 0


# ------------------------------------------------------------------------------------------------------------------ (e)
@pytest.mark.parametrize("position", [2 ** 32 - 1000, 2 ** 40 + 5])
def test_positions_beyond_32_bits(nv, bl, position):
    n = 20011
    rows = [_noise_with_bursts(n, 80 + s, rate=2500) for s in range(2)]
    with bl.Blanker(br.CS16, n_streams=2) as b:
        b.debug_set_position(position)
        assert b.position(1) == position
        got = _run_resident(nv, b, rows, [9000, n - 9000])
        for s in range(2):
            want, ref = br.blank(rows[s], position=position)
            assert np.array_equal(got[s], want), (s, _first_difference(got[s], want))
            assert ref.detections > 0 and b.stats(s) == (n, ref.detections, ref.blanked)
            # nothing in front of the position: as a stream that starts there, not one that has run that long
            assert not ref.gone[:4 * 1024 - position % 1024].any()


# ------------------------------------------------------------------------------------------------------------------ (f)
@pytest.mark.parametrize("params", [dict(hold=0), dict(hold=1024), dict(thr_q8=256), dict(thr_q8=4096), dict(floor=0), dict(floor=65535)],
                         ids=["hold0", "hold1024", "thr256", "thr4096", "floor0", "floor65535"])
def test_the_ends_of_the_parameters(nv, bl, params):
    n = 30011
    rows = [_noise_with_bursts(n, 90 + s, rate=2000) for s in range(2)]
    rows[1][20000:20040] = -32768                            # m = 65536
    with bl.Blanker(br.CS16, n_streams=2, **params) as b:
        got = _run_resident(nv, b, rows, [n // 2, n - n // 2], out_first=4)
        for s in range(2):
            want, ref = br.blank(rows[s], **params)
            assert np.array_equal(got[s], want), (s, _first_difference(got[s], want))
            assert b.stats(s) == (n, ref.detections, ref.blanked)
            if params.get("hold") == 0:
                assert ref.detections == ref.blanked > 0
            if params.get("floor") == 65535:
                assert ref.detections == (40 if s else 0)


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_bypass_is_the_conversion_and_the_resampler_agrees_with_it(nv, bl, fmt):
    """thr_q8 = 0: out is the conversion and nothing is counted.  The resampler's own conversion is the same one: its
    L = M = 1 plan in format fmt on the raw buffer gives the words its CS16 plan gives on the blanker's output."""
    import navtex_amd.resample as rs
    n = 24000
    rows = _inputs(nv, fmt, n, "random", seed=300 + fmt)
    with bl.Blanker(fmt, n_streams=2, thr_q8=0) as b:
        got = _run_resident(nv, b, rows, [n])
        for s in range(2):
            assert np.array_equal(got[s], rr.convert(rows[s], fmt).astype(np.int16)), s
            assert b.stats(s) == (n, 0, 0)
    bps = rows[0].dtype.itemsize * 2
    d_raw = nv.DeviceBuffer(n * bps); d_conv = nv.DeviceBuffer(n * 4); d_a = nv.DeviceBuffer(n * 4); d_b = nv.DeviceBuffer(n * 4)
    d_raw.upload(rows[0]); d_conv.upload(got[0])
    with rs.Resampler(252000, fmt) as ra, rs.Resampler(252000, rs.CS16) as rb:
        assert (ra.L, ra.M) == (1, 1)
        assert ra.resident(d_raw, n, n, d_a, n) == n and rb.resident(d_conv, n, n, d_b, n) == n
        a, c = d_a.download(n * 4, dtype=np.uint32), d_b.download(n * 4, dtype=np.uint32)
    for d in (d_raw, d_conv, d_a, d_b):
        d.free()
    assert np.array_equal(a, c) and a.any()


# ------------------------------------------------------------------------------------------------------------------ (g)
@pytest.mark.parametrize("fmt", [br.CS16, br.CS8], ids=["cs16", "cs8"])
def test_push_equals_resident(nv, bl, fmt):
    n = 21000
    rows = [rr.to_format(_noise_with_bursts(2 * n, 120 + s, rate=3000), fmt, gain=3.0 if fmt == br.CS8 else 1.0) for s in range(3)]
    refs = [br.blank(row, fmt) for row in rows]
    with bl.Blanker(fmt, n_streams=3) as b:
        for s, cuts in enumerate(([n], [1, 1023, n - 1024], [7, 0, 5000, 1, n - 5008])):
            pos, parts = 0, []
            for c in cuts:
                parts.append(b.push(s, rows[s][pos:pos + c])); pos += c
            out = np.concatenate(parts)
            assert out.dtype == np.int16 and np.array_equal(out, refs[s][0][:n]), s
            assert b.position(s) == n
        got = _run_resident(nv, b, [row[n:] for row in rows], [n])
        for s in range(3):
            assert np.array_equal(got[s], refs[s][0][n:]), s
            assert b.stats(s) == (2 * n, refs[s][1].detections, refs[s][1].blanked)
            assert b.stats(s, reset=True)[0] == 2 * n and b.stats(s) == (0, 0, 0)


def test_span_and_position_errors_launch_nothing(nv, bl):
    ARG = nv._native.ERR_ARG
    n = 8192
    with bl.Blanker(br.CU8, n_streams=2) as b:
        d_in = nv.DeviceBuffer(2 * n * 2); d_out = nv.DeviceBuffer(2 * n * 4)
        one_in = nv.DeviceBuffer(n * 2); one_out = nv.DeviceBuffer(n * 4)
        b.timing(True)
        call = lambda *a: bl.lib.nvx_blank_resident(b._h, *a, None)            # noqa: E731
        bad = {"more samples than the pitch": (d_in.ptr, n - 8, n, d_out.ptr, n, 0),
               "words beyond the pitch": (d_in.ptr, n, n, d_out.ptr, n - 1, 0),
               "out_first pushes them beyond it": (d_in.ptr, n, n, d_out.ptr, n, 1),
               "input rows for one stream": (one_in.ptr, n, n, d_out.ptr, n, 0),
               "output rows for one stream": (d_in.ptr, n, n, one_out.ptr, n, 0),
               "misaligned input": (d_in.ptr + 4, n, n - 8, d_out.ptr, n, 0),
               "misaligned output": (d_in.ptr, n, n, d_out.ptr + 2, n, 0),
               "rows not 16-byte aligned": (d_in.ptr, n - 3, n - 8, d_out.ptr, n, 0),
               "null input": (None, n, n, d_out.ptr, n, 0),
               "null output": (d_in.ptr, n, n, None, n, 0),
               "too many samples": (d_in.ptr, 2 ** 31, 2 ** 30 + 1, d_out.ptr, 2 ** 31, 0),
               "a pitch that wraps": (d_in.ptr, 2 ** 63, n, d_out.ptr, n, 0),
               "an output pitch that wraps": (d_in.ptr, n, n, d_out.ptr, 2 ** 62, 0),
               "out_first that wraps": (d_in.ptr, n, n, d_out.ptr, n, 2 ** 64 - 8)}
        for name, args in bad.items():
            assert call(*args) == ARG, name
            assert bl.lib.nvx_blank_last_error() != b""
        b.debug_set_position(2 ** 62 - 100)
        assert call(d_in.ptr, n, n, d_out.ptr, n, 0) == ARG and b"2^62" in bl.lib.nvx_blank_last_error()
        small = np.zeros((200, 2), dtype=np.uint8)
        assert bl.lib.nvx_blank_push(b._h, 0, small.ctypes.data_as(C.c_void_p), 200, small.ctypes.data_as(C.c_void_p)) == ARG
        assert bl.lib.nvx_blank_debug_set_position(b._h, 0, 2 ** 62) == ARG and bl.lib.nvx_blank_debug_set_position(b._h, 2, 0) == ARG
        assert bl.lib.nvx_blank_reset(b._h, 2) == ARG and bl.lib.nvx_blank_stats(b._h, -1, None, None, None, 0) == ARG
        assert b.time_stats() == (0.0, 0) and b.debug_last_launch()["launches"] == 0 and b.position(0) == 2 ** 62 - 100
        b.reset()
        assert call(d_in.ptr, n, 0, d_out.ptr, n, 0) == 0 and b.debug_last_launch()["launches"] == 0       # nothing to do: no launch
        assert call(d_in.ptr, n, n, d_out.ptr, n, 0) == 0
        ms, launches = b.time_stats()
        assert launches == 1 and ms > 0.0 and b.debug_last_launch()["launches"] == 1 and b.stats(1)[0] == n
        for d in (d_in, d_out, one_in, one_out):
            d.free()
    for kw in (dict(device=99), dict(thr_q8=255), dict(thr_q8=4097), dict(hold=1025), dict(floor=65536), dict(format=4), dict(n_streams=0)):
        with pytest.raises(nv.NvxError) as e:
            bl.Blanker(**kw)
        assert e.value.code == ARG, kw


# ------------------------------------------------------------------------------------------------------------------ (h)
def _decode_rows(nv, bl, rows, blanker):
    """Twelve rows at 252 kS/s as twelve streams: (blanked by `blanker` on the handle's stream, or as they are) ->
    nvx_process_resident.  Returns (the words handed to the handle, bits per stream, messages per stream)."""
    ns, n = len(rows), len(rows[0])
    frames = n // nv.FRAME_IN
    d_in = nv.DeviceBuffer(ns * n * 4); d_out = nv.DeviceBuffer(ns * n * 4)
    for s in range(ns):
        d_in.upload(rows[s], s * n * 4)
    with nv.Pipeline(n_streams=ns, chain_mask=nv.CHAIN_518, max_frames=8) as p:
        hs = p.hip_stream
        f0 = 0
        while f0 < frames:
            k = min(8, frames - f0)
            if blanker:
                at = f0 * nv.FRAME_IN
                blanker.resident(_At(d_in.ptr + at * 4), n, k * nv.FRAME_IN, d_out, n, at, hip_stream=hs)
            p.process_resident(d_out if blanker else d_in, n, f0, k, hip_stream=hs)
            f0 += k
        p.fetch()
        bits = [p.bits(s, 0) for s in range(ns)]
        msgs = [[m[3] for m in p.messages if m[0] == s] for s in range(ns)]
        words = d_out.download(ns * n * 4, dtype=np.int16).reshape(ns, n, 2) if blanker else None
    d_in.free(); d_out.free()
    return words, bits, msgs


def test_the_acceptance_case_on_the_device(nv, bl, oracle):
    """The twelve rows of tests/blank_cases.py as twelve streams: blank -> a 252 kS/s handle, on the handle's stream, eight
    frames a call.  The words and the bits are the restatement's and the oracle's, and the counts the CPU's: measured
    H = 0 and B = 12 of 12."""
    text = bc.text()
    bits = nv.sitor_encode(text, 40)
    ys = [bc.rows(nv.FRAME_IN, bits, seed)[1] for seed in bc.SEEDS]
    want = [br.blank(y) for y in ys]
    with bl.Blanker(br.CS16, n_streams=len(ys)) as b:
        words, got_bits, got_msgs = _decode_rows(nv, bl, ys, b)
        for s, (out, ref) in enumerate(want):
            assert np.array_equal(words[s], out), (s, _first_difference(words[s], out))
            assert b.stats(s) == (len(out), ref.detections, ref.blanked)
    cpu = [bc.delivered(oracle, out, nv.FRAME_IN) for out, _ in want]
    for s in range(len(ys)):
        assert got_bits[s] == cpu[s][1] and got_msgs[s] == cpu[s][0], s
    B = sum(m == [text] for m in got_msgs)
    _, raw_bits, raw_msgs = _decode_rows(nv, bl, ys, None)
    cpu_raw = [bc.delivered(oracle, y, nv.FRAME_IN) for y in ys]
    assert [m for m in raw_msgs] == [c[0] for c in cpu_raw] and raw_bits == [c[1] for c in cpu_raw]
    H = sum(m == [text] for m in raw_msgs)
    print("H", H, "B", B, "of", len(ys))
    assert B >= H + 6 and B >= 10


def test_blank_then_resample_then_decode_at_768k(nv, bl, oracle):
    """nvx_blank_resident -> nvx_resample_resident (CS16) -> a 252 kS/s handle, all on the handle's stream: the message
    arrives, and the words are the restatements'."""
    import navtex_amd.resample as rs
    fi = bc.CHAIN_RATE
    text = bc.text()
    bits = nv.sitor_encode(text, 40)
    y = bc.chain_rows(bits)[1]
    n = len(y)
    L, M, T, S, taps = rs.design(fi)
    blanked = br.blank(y, hold=bc.CHAIN_HOLD)[0]
    want = rr.resample_all(blanked, rr.CS16, taps, L, M)
    per_frame = fi * 8 // 25
    frames = n // per_frame
    assert len(want) == frames * nv.FRAME_IN
    d_in = nv.DeviceBuffer(n * 4); d_mid = nv.DeviceBuffer(n * 4); d_out = nv.DeviceBuffer(len(want) * 4)
    d_in.upload(y)
    with bl.Blanker(br.CS16, hold=bc.CHAIN_HOLD) as b, rs.Resampler(fi, rs.CS16) as r, nv.Pipeline(n_streams=1, chain_mask=nv.CHAIN_518, max_frames=8) as p:
        hs = p.hip_stream
        f0 = 0
        while f0 < frames:
            k = min(8, frames - f0)
            b.resident(_At(d_in.ptr + f0 * per_frame * 4), n, k * per_frame, d_mid, n, f0 * per_frame, hip_stream=hs)
            assert r.resident(_At(d_mid.ptr + f0 * per_frame * 4), n, k * per_frame, d_out, len(want), f0 * nv.FRAME_IN, hip_stream=hs) == k * nv.FRAME_IN
            p.process_resident(d_out, len(want), f0, k, hip_stream=hs)
            f0 += k
        p.fetch()
        got_bits, got_msgs = p.bits(0, 0), [m[3] for m in p.messages]
        mid = d_mid.download(n * 4, dtype=np.int16).reshape(-1, 2)
        words = d_out.download(len(want) * 4, dtype=np.int16).reshape(-1, 2)
    for d in (d_in, d_mid, d_out):
        d.free()
    assert np.array_equal(mid, blanked) and np.array_equal(words, want)
    msgs, ref_bits = bc.delivered(oracle, want, nv.FRAME_IN)
    assert got_bits == ref_bits and got_msgs == msgs == [text]
