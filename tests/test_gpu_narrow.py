"""The narrowband interpolator (include/navtex_amd_narrow.h) on the GPU (-m gpu): output words equal to the restatement
(tests/narrow_ref.py) in every format and kind at rates with M = 1, M = 2, an alternating window parity, the largest tables and
the shortest filters, calls cut anywhere against one shot, push against resident, streams pushed apart and a reset stream
rejoining, the rails and full-scale random input (float32 specials), the REAL kind against the IQ kind fed (x, 0), positions
beyond 2^32, the two launch shapes at scale, the refusals, and audio to message on the device: through the converter, the REAL
kind, two stations of a 48 kS/s row, and the scan.  Every comparison is ==, with sentinels around every output row."""
from pathlib import Path

import numpy as np
import pytest

import narrow_cases as nc
import narrow_ref as nr
from narrow_cases import _first_difference, _run_resident, _same

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FORMATS = (nr.S16, nr.U8, nr.S8, nr.F32)
FORMAT_IDS = ("s16", "u8", "s8", "f32")
KINDS = (nr.IQ, nr.REAL)
KIND_IDS = ("iq", "real")
# (rate_num, rate_den): M = 1; M = 2; L = 160, M = 7 (the window's parity alternates); L = 320 (two threads share a window);
# L = 504, M = 25; T = 12
RATES = ((12000, 1), (8000, 1), (11025, 1), (11025, 2), (12500, 1), (96000, 1))
WINDOWS = {(12000, 1): 256, (8000, 1): 256, (11025, 1): 256, (11025, 2): 128, (12500, 1): 256, (96000, 1): 256, (64000, 1): 256, (88200, 1): 256,
           (6250, 1): 128, (2000, 1): 64}


@pytest.fixture(scope="module")
def nb(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_narrow.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.narrow
    return navtex_amd.narrow


@pytest.fixture(scope="module")
def designs(nb):
    cache = {}
    def get(num, den=1):
        if (num, den) not in cache:
            cache[(num, den)] = nb.design(num, den)
        return cache[(num, den)]
    return get


# ------------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("rate", RATES, ids=lambda r: f"{r[0]}_{r[1]}")
def test_three_streams_of_three_tiles_and_a_ragged_fourth(nv, nb, designs, rate, fmt, kind):
    """3 streams x (3 tiles + 37 samples), a seed each, spread over two workgroups.  A pitch larger than the data; out_first at
    each residue mod 4 (residue 0: the aligned 16-byte stores)."""
    L, M, T, h = designs(*rate)
    n = 3 * WINDOWS[rate] + 37
    rows = [nc.signal(fmt, kind, n, 100 * fmt + 10 * kind + s + rate[0]) for s in range(3)]
    want = [nr.interpolate_all(row, h, L, M, fmt, kind)[0] for row in rows]
    with nb.Interpolator(*rate, format=fmt, kind=kind, n_streams=3) as c:
        assert (c.L, c.M, c.T) == (L, M, T)
        for out_first in (8, 5, 6, 7):
            c.reset()
            got = _run_resident(nv, c, rows, [n], pitch_extra=1 + out_first % 4, out_first=out_first)
            shape = c.debug_last_launch()
            assert (shape["chunks"], shape["tiles_per_chunk"], shape["form"], shape["windows"]) == (2, 2, 2, WINDOWS[rate]), shape
            _same(got, want, out_first)


@pytest.mark.parametrize("rate,fmt,kind", [((64000, 1), nr.U8, nr.IQ), ((88200, 1), nr.F32, nr.REAL), ((6250, 1), nr.S16, nr.IQ), ((2000, 1), nr.S8, nr.IQ)],
                         ids=["64000_T28", "88200_T14", "6250_table_80K", "2000_four_threads_a_window"])
def test_the_other_filter_lengths_the_largest_table_and_the_longest_window(nv, nb, designs, rate, fmt, kind):
    """T = 28 and 14; L = 1008, whose table of 80 640 bytes is the largest a supported rate has (beyond 64 KB of LDS); L / M = 126,
    where four threads share a window."""
    L, M, T, h = designs(*rate)
    assert T == {64000: 28, 88200: 14}.get(rate[0], 30)
    n = 3 * WINDOWS[rate] + 37
    rows = [nc.signal(fmt, kind, n, 900 + s) for s in range(2)]
    want = [nr.interpolate_all(row, h, L, M, fmt, kind)[0] for row in rows]
    with nb.Interpolator(*rate, format=fmt, kind=kind, n_streams=2) as c:
        got = _run_resident(nv, c, rows, [n - 100, 100], pitch_extra=2, out_first=3)
        shape = c.debug_last_launch()
        assert shape["windows"] == WINDOWS[rate] and shape["parts"] == 256 // WINDOWS[rate]
        assert shape["lds_bytes"] == L * (((T + 7) // 8) | 1) * 16 + (288 + 8200) * 4
        _same(got, want, rate)


# ------------------------------------------------------------------------------------------------------------------ (b)
def test_one_shot_equals_short_calls_push_equals_resident_and_a_reset_stream_rejoins(nv, nb, designs):
    """Calls of 0, 1, T - 2, T - 1, T and several thousand samples against one shot; then the streams pushed one by one and apart,
    meeting again for a resident call; then stream 1 reset, refused while it stands elsewhere, pushed back up and rejoining."""
    rate = (11025, 1)
    L, M, T, h = designs(*rate)
    cuts = [0, 1, T - 2, T - 1, T, 3000, 0, 1, 2500]
    n1, n2, n3 = sum(cuts), 700, 400
    rows = [nc.signal(nr.S16, nr.IQ, n1 + n2 + n3, 400 + s) for s in range(3)]
    want = [nr.interpolate_all(row, h, L, M)[0] for row in rows]
    o1, o2 = nr.outputs_after(n1, L, M), nr.outputs_after(n1 + n2, L, M)
    with nb.Interpolator(*rate, n_streams=3) as c:
        got = _run_resident(nv, c, [row[:n1] for row in rows], cuts)
        _same(got, [w[:o1] for w in want], "cuts")
        # pushed apart: each stream in calls of its own
        for s, pcuts in enumerate(([n2], [1, 0, T - 1, n2 - T], [333, 1, n2 - 334])):
            pos, parts = n1, []
            for cut in pcuts:
                parts.append(c.push(s, rows[s][pos:pos + cut])); pos += cut
                assert c.position(s) == (pos, nr.outputs_after(pos, L, M))
            out = np.concatenate(parts)
            assert out.dtype == np.int16 and np.array_equal(out, want[s][o1:o2]), (s, _first_difference(out, want[s][o1:o2]))
        # a reset stream stands elsewhere: the resident call is refused and launches nothing
        c.reset(1)
        assert c.position(1) == (0, 0) and c.position(0) == (n1 + n2, o2)
        d = nv.DeviceBuffer(3 * 64 * 4); o = nv.DeviceBuffer(3 * 2048 * 4)
        launches = c.debug_last_launch()["launches"]
        assert nb.lib.nvx_nb_resident(c._h, d.ptr, 64, 64, o.ptr, 2048, 0, None, None) == nv._native.ERR_STATE
        assert b"same position" in nb.lib.nvx_nb_last_error() and c.debug_last_launch()["launches"] == launches
        d.free(); o.free()
        fresh = nr.Interpolator(h, L, M)
        other = nc.signal(nr.S16, nr.IQ, n1 + n2 + n3, 450)
        pos = 0
        for cut in (10, 1, 2000, n1 + n2 - 2011):
            assert np.array_equal(c.push(1, other[pos:pos + cut]), fresh.push(other[pos:pos + cut])), pos
            pos += cut
        got = _run_resident(nv, c, [rows[0][n1 + n2:], other[n1 + n2:], rows[2][n1 + n2:]], [n3])
        _same(got, [want[0][o2:], fresh.push(other[n1 + n2:]), want[2][o2:]], "rejoined")


def test_a_stream_pushed_three_times_meets_two_that_were_not(nv, nb, designs):
    """3 streams of unsigned bytes (REAL: a byte a sample).  Stream 1 alone is pushed 5, 700 and 3 samples -- the staging grows,
    then serves a smaller push, and after three launches the stream reads the other of its two state rows -- while streams 0
    and 2 are set to where it stands with silence in front.  One resident call of a single tile over all three: stream 1's
    state row is brought over to the others' side first, and every word equals the restatement."""
    rate, fmt, kind = (12000, 1), nr.U8, nr.REAL
    L, M, T, h = designs(*rate)
    pushes, n = (5, 700, 3), 200
    at = sum(pushes)
    assert n <= WINDOWS[rate]
    rows = [nc.signal(fmt, kind, at + n, 700 + s) for s in range(3)]
    refs = [nr.Interpolator(h, L, M, fmt, kind, position=0 if s == 1 else at) for s in range(3)]
    with nb.Interpolator(*rate, format=fmt, kind=kind, n_streams=3) as c:
        pos = 0
        for cut in pushes:
            assert np.array_equal(c.push(1, rows[1][pos:pos + cut]), refs[1].push(rows[1][pos:pos + cut])), pos
            pos += cut
        launches = c.debug_last_launch()["launches"]
        assert launches == 3
        c.debug_set_position(at, stream=0); c.debug_set_position(at, stream=2)
        assert all(c.position(s) == (at, nr.outputs_after(at, L, M)) for s in range(3))
        got = _run_resident(nv, c, [row[at:] for row in rows], [n], pitch_extra=1, out_first=1)
        shape = c.debug_last_launch()
        assert (shape["launches"], shape["chunks"], shape["tiles_per_chunk"]) == (launches + 1, 1, 1), shape
        _same(got, [refs[s].push(rows[s][at:]) for s in range(3)], "met")


# ------------------------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_the_rails_and_full_scale_random_input(nv, nb, designs, fmt, kind):
    """Windows matched in sign to the phase with the largest sum |h|, every second one and Q negated: the value before the clamp
    is beyond int16 on both sides (16-bit and float32 input; 8-bit full scale is 0.4 % short of it and still beyond).  And
    full-scale random input with the float32 specials."""
    rate = (12000, 1)
    L, M, T, h = designs(*rate)
    rails = nc.rails(h, fmt, kind, 24)
    n = len(rails)
    rows = [rails, nc.full_scale(fmt, kind, n, 500 + fmt), nc.full_scale(fmt, kind, n, 600 + fmt)]
    refs = [nr.interpolate_all(row, h, L, M, fmt, kind) for row in rows]
    assert refs[0][1].acc_max >> 14 > 70000 and refs[0][1].acc_min >> 14 < -70000
    assert refs[0][0][:, 0].max() == 32767 and refs[0][0][:, 0].min() == -32768
    if kind == nr.IQ:
        assert refs[0][0][:, 1].max() == 32767 and refs[0][0][:, 1].min() == -32768
    with nb.Interpolator(*rate, format=fmt, kind=kind, n_streams=3) as c:
        got = _run_resident(nv, c, rows, [301, n - 301], out_first=3)
        _same(got, [r[0] for r in refs], "rails")


def test_the_rails_where_the_phases_alternate(nv, nb, designs):
    rate = (8000, 1)
    L, M, T, h = designs(*rate)
    rows = [nc.rails(h, nr.S16, nr.IQ, 24, gap=g) for g in (1, 2)]
    n = min(len(r) for r in rows)
    rows = [r[:n] for r in rows]
    refs = [nr.interpolate_all(row, h, L, M) for row in rows]
    assert max(r[1].acc_max for r in refs) >> 14 > 70000 and min(r[1].acc_min for r in refs) >> 14 < -70000
    with nb.Interpolator(*rate, n_streams=2) as c:
        _same(_run_resident(nv, c, rows, [n]), [r[0] for r in refs], "rails at M = 2")


# ------------------------------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_the_real_kind_has_no_q_and_equals_the_iq_kind_fed_zero_q(nv, nb, designs, fmt):
    rate = (11025, 1)
    L, M, T, h = designs(*rate)
    n = 900
    x = nc.full_scale(fmt, nr.REAL, n, 77 + fmt)
    zero = np.full(n, 128 if fmt == nr.U8 else 0, dtype=x.dtype)
    with nb.Interpolator(*rate, format=fmt, kind=nr.REAL) as c:
        real = _run_resident(nv, c, [x], [n])[0]
    assert not real[:, 1].any() and real[:, 0].any()
    assert np.array_equal(real, nr.interpolate_all(x, h, L, M, fmt, nr.REAL)[0])
    if fmt != nr.U8:                                        # no unsigned byte converts to 0: (2 u - 255) * 128 is odd times 128
        with nb.Interpolator(*rate, format=fmt, kind=nr.IQ) as c:
            iq = _run_resident(nv, c, [np.stack([x, zero], axis=1)], [n])[0]
        assert np.array_equal(iq, real)


# ------------------------------------------------------------------------------------------------------------------ (e)
@pytest.mark.parametrize("position", [2 ** 32 - 1000, 2 ** 40 + 6])
def test_positions_beyond_32_bits(nv, nb, designs, position):
    """600 samples in two calls from the position: silence in front of it, and the phase of its first output is the position's."""
    rate = (11025, 1)
    L, M, T, h = designs(*rate)
    rows = [nc.signal(nr.S16, nr.IQ, 600, 80 + s) for s in range(2)]
    refs = [nr.Interpolator(h, L, M, position=position) for _ in rows]
    with nb.Interpolator(*rate, n_streams=2) as c:
        c.debug_set_position(position)
        assert c.position(1) == (position, nr.outputs_after(position, L, M))
        got = _run_resident(nv, c, rows, [222, 378])
        _same(got, [refs[s].push(rows[s]) for s in range(2)], position)
    assert (nr.outputs_after(position, L, M) * M - position * L) % M != 0


# ------------------------------------------------------------------------------------------------------------------ (f)
def _scale(nv, nb, designs, rate, ns, cuts, shape):
    L, M, T, h = designs(*rate)
    kinds = 16
    n = sum(cuts)
    rows = [nc.signal(nr.S16, nr.IQ, n, 7000 + k) for k in range(kinds)]
    want = np.stack([nr.interpolate_all(row, h, L, M)[0] for row in rows])
    n_out = want.shape[1]
    pitch = (max(cuts) + 15) // 16 * 16
    d_in = nv.DeviceBuffer(ns * pitch * 4); d_out = nv.DeviceBuffer(ns * n_out * 4)
    with nb.Interpolator(*rate, n_streams=ns) as c:
        pos = made = 0
        for cut in cuts:
            block = np.full((kinds, pitch, 2), 32767, dtype=np.int16)
            block[:, :cut] = np.stack([row[pos:pos + cut] for row in rows])
            tiled = np.tile(block, ((ns + kinds - 1) // kinds, 1, 1))[:ns]
            d_in.upload(tiled)
            made += c.resident(d_in, pitch, cut, d_out, n_out, made)
            pos += cut
            got_shape = c.debug_last_launch()
            assert (got_shape["chunks"], got_shape["form"]) == shape, got_shape
        assert made == n_out
        got = d_out.download(ns * n_out * 4, dtype=np.int16).reshape(ns, n_out, 2)
    d_in.free(); d_out.free()
    bad = [k for k in range(kinds) if not np.array_equal(got[k::kinds], np.broadcast_to(want[k], got[k::kinds].shape))]
    assert not bad, bad


def test_scale_1024_streams_a_workgroup_each(nv, nb, designs):
    """1024 streams x 200 samples at 12 kS/s: one workgroup per stream; and the same rows as 64 streams spread over workgroups."""
    _scale(nv, nb, designs, (12000, 1), 1024, [200], (1, 1))
    _scale(nv, nb, designs, (12000, 1), 64, [1100], (3, 2))


def test_scale_65535_streams_in_two_short_calls(nv, nb, designs):
    """65 535 streams x two calls of 37 and 40 samples at 8 kS/s."""
    _scale(nv, nb, designs, (8000, 1), 65535, [37, 40], (1, 1))


# ------------------------------------------------------------------------------------------------------------------ (g)
def test_span_count_and_position_errors_launch_nothing(nv, nb):
    ARG = nv._native.ERR_ARG
    n, outs = 1024, 1024 * 21
    with nb.Interpolator(12000, n_streams=2) as c:
        d_in = nv.DeviceBuffer(2 * n * 4); d_out = nv.DeviceBuffer(2 * outs * 4)
        one_in = nv.DeviceBuffer(n * 4); one_out = nv.DeviceBuffer(outs * 4)
        c.timing(True)
        call = lambda *a: nb.lib.nvx_nb_resident(c._h, *a, None, None)          # noqa: E731
        bad = {"more samples than the pitch": (d_in.ptr, n - 16, n, d_out.ptr, outs, 0),
               "words beyond the pitch": (d_in.ptr, n, n, d_out.ptr, outs - 1, 0),
               "out_first pushes them beyond it": (d_in.ptr, n, n, d_out.ptr, outs, 1),
               "input rows for one stream": (one_in.ptr, n, n, d_out.ptr, outs, 0),
               "output rows for one stream": (d_in.ptr, n, n, one_out.ptr, outs, 0),
               "misaligned input": (d_in.ptr + 4, n, n - 16, d_out.ptr, outs, 0),
               "misaligned output": (d_in.ptr, n, n, d_out.ptr + 2, outs, 0),
               "rows not 16-byte aligned": (d_in.ptr, n - 3, n - 16, d_out.ptr, outs, 0),
               "null input": (None, n, n, d_out.ptr, outs, 0),
               "null output": (d_in.ptr, n, n, None, outs, 0),
               "too many samples": (d_in.ptr, 2 ** 32, 2 ** 30 + 1, d_out.ptr, 2 ** 36, 0),
               "an output count at 2^31": (d_in.ptr, 2 ** 30, (2 ** 31 + 20) // 21, d_out.ptr, 2 ** 32, 0),
               "a pitch that wraps": (d_in.ptr, 2 ** 64 - 16, n, d_out.ptr, outs, 0),
               "an output pitch that wraps": (d_in.ptr, n, n, d_out.ptr, 2 ** 62, 0),
               "out_first that wraps": (d_in.ptr, n, n, d_out.ptr, outs, 2 ** 64 - 8)}
        for name, args in bad.items():
            assert call(*args) == ARG, name
            assert nb.lib.nvx_nb_last_error() != b""
        assert call(*bad["an output count at 2^31"]) == ARG and b"2^31" in nb.lib.nvx_nb_last_error()
        # one output fewer is a count the call accepts (and then refuses for its span)
        assert call(d_in.ptr, 2 ** 30, (2 ** 31 - 1) // 21, d_out.ptr, 2 ** 32, 0) == ARG and b"2^31" not in nb.lib.nvx_nb_last_error()
        c.debug_set_position(2 ** 62 - 100)
        assert call(d_in.ptr, n, n, d_out.ptr, outs, 0) == ARG and b"2^62" in nb.lib.nvx_nb_last_error()
        assert nb.lib.nvx_nb_debug_set_position(c._h, 0, 2 ** 62) == ARG and nb.lib.nvx_nb_debug_set_position(c._h, 2, 0) == ARG
        assert nb.lib.nvx_nb_reset(c._h, 2) == ARG and nb.lib.nvx_nb_position(c._h, 2, None, None) == ARG
        assert c.time_stats() == (0.0, 0) and c.debug_last_launch()["launches"] == 0
        assert c.position(0) == (2 ** 62 - 100, (2 ** 62 - 100) * 21 % 2 ** 64)
        c.reset()
        # a push too long for its output buffer consumes nothing
        x = np.zeros((9, 2), dtype=np.int16)
        out = np.zeros((9 * 21, 2), dtype=np.int16)
        n_out = nb.C.c_size_t(77)
        assert nb.lib.nvx_nb_push(c._h, 0, nv._native.as_ptr(x), 9, nv._native.as_ptr(out), 9 * 21 - 1, nb.C.byref(n_out)) == ARG and c.position(0) == (0, 0)
        assert nb.lib.nvx_nb_push(c._h, 2, nv._native.as_ptr(x), 9, nv._native.as_ptr(out), 9 * 21, nb.C.byref(n_out)) == ARG
        assert n_out.value == 77 and c.debug_last_launch()["launches"] == 0
        assert len(c.push(0, x[:0])) == 0 and c.debug_last_launch()["launches"] == 0
        size = nb.C.c_size_t(5)
        assert nb.lib.nvx_nb_resident(c._h, d_in.ptr, n, 0, d_out.ptr, outs, 0, nb.C.byref(size), None) == 0 and size.value == 0
        assert c.debug_last_launch()["launches"] == 0       # nothing to do: no launch
        d_in.upload(np.zeros(2 * n * 2, dtype=np.int16))
        assert call(d_in.ptr, n, n, d_out.ptr, outs, 0) == 0
        ms, calls = c.time_stats()
        assert calls == 1 and ms > 0.0 and c.debug_last_launch()["launches"] == 1 and c.position(1) == (n, outs)
        for d in (d_in, d_out, one_in, one_out):
            d.free()
    for kw in (dict(rate_num=12000, device=99), dict(rate_num=1999), dict(rate_num=96001), dict(rate_num=2001), dict(rate_num=12000, rate_den=3),
               dict(rate_num=12000, kind=2), dict(rate_num=12000, format=4), dict(rate_num=12000, n_streams=0)):
        with pytest.raises(nv.NvxError) as e:
            nb.Interpolator(**kw)
        assert e.value.code == ARG, kw


# ------------------------------------------------------------------------------------------------------------------ (h)
def _decode_on_the_device(nv, d_out, pitch, n_out, n_streams, chain_mask, tune):
    """d_out ([n_streams][pitch] words at 252 kS/s) through a raw_rate = 0 handle on its own stream, eight frames at a time:
    ({(stream, chain): bits}, the handle's messages)."""
    frames = n_out // nv.FRAME_IN
    chains = [c for c in (0, 1) if chain_mask & (nv.CHAIN_518, nv.CHAIN_490)[c]]
    with nv.Pipeline(n_streams=n_streams, chain_mask=chain_mask, max_frames=8) as p:
        for (s, c), hz in tune.items():
            p.set_carrier(s, c, hz)
        for f0 in range(0, frames, 8):
            p.process_resident(d_out, pitch, f0, min(8, frames - f0), hip_stream=p.hip_stream)
        p.fetch()
        return {(s, c): p.bits(s, c) for s in range(n_streams) for c in chains}, list(p.messages)


@pytest.mark.parametrize("seed", [17, 22], ids=["audio_8k_through_the_converter", "audio_44k1_real_kind"])
def test_audio_to_message_on_the_device(nv, nb, seed):
    """The CPU cases of seeds 17 and 22 on the device: (nvx_real ->) nvx_nb -> a tuned one-chain handle on its own
    stream.  The interpolator's words are the restatement's, the message is the text, the bits are the tuned chain's
    restatement's on those words."""
    import navtex_amd.real as rl
    import signals
    import tune_ref as tr
    case = nc.E2E[seed]
    num, den, kind = nc.plan_of(seed)
    L, M, T, h = nb.design(num, den)
    src = nc.source(nv, seed)
    x = nc.interpolator_input(seed, src)
    want, _ = nr.interpolate_all(x, h, L, M, nr.S16, kind)
    n_in, n_out = len(x), len(want)
    d_src = nv.DeviceBuffer(len(src) * 2); d_out = nv.DeviceBuffer(n_out * 4)
    d_src.upload(src)
    with nb.Interpolator(num, den, kind=kind) as c:
        if case["path"] == "converter":
            d_iq = nv.DeviceBuffer(n_in * 4)
            with rl.Converter(rl.S16) as conv:
                conv.resident(d_src, 2 * n_in, 2 * n_in, d_iq, n_in)
                assert c.resident(d_iq, n_in, n_in, d_out, n_out) == n_out
                words = d_out.download(n_out * 4, dtype=np.int16).reshape(-1, 2)
            d_iq.free()
        else:
            assert c.resident(d_src, n_in, n_in, d_out, n_out) == n_out
            words = d_out.download(n_out * 4, dtype=np.int16).reshape(-1, 2)
    assert np.array_equal(words, want), _first_difference(words, want)
    bits, msgs = _decode_on_the_device(nv, d_out, n_out, n_out, 1, nv.CHAIN_518, {(0, 0): case["tuned"]})
    d_src.free(); d_out.free()
    cut = want[:n_out // nv.FRAME_IN * nv.FRAME_IN]
    assert bits[(0, 0)] == tr.decode(tr.chain(tr.front(cut, False), 0, tr.k_of(case["tuned"])))
    assert [m[3] for m in msgs] == [signals.stream_text(seed)]
    if kind == nr.REAL:
        assert not words[:, 1].any()


def test_two_stations_of_a_48k_iq_row_through_an_untuned_two_chain_handle(nv, nb, oracle):
    """A 48 kS/s IQ row holding a station at +14 kHz and another at -14 kHz with different texts: both messages arrive, and both
    chains' bits are the oracle's on the restatement's output."""
    import iqc_cases as ic
    import resample_ref as rr
    import signals
    texts = (signals.stream_text(21), signals.stream_text(23))
    bits = [nv.sitor_encode(t, nc.PHASING) for t in texts]
    n = (max(len(b) for b in bits) + 300) * 480
    a = rr.cpfsk(bits[0], 48000, n, freq_hz=14000, amplitude=nc.AMPLITUDE, noise_amp=nc.NOISE, seed=21).astype(np.int32)
    a += rr.cpfsk(bits[1], 48000, n, freq_hz=-14000, amplitude=nc.AMPLITUDE, noise_amp=0, seed=23, bit_offset=777)
    src = np.clip(a, -32768, 32767).astype(np.int16)
    L, M, T, h = nb.design(48000)
    want, _ = nr.interpolate_all(src, h, L, M)
    n_out = len(want)
    d_in = nv.DeviceBuffer(n * 4); d_out = nv.DeviceBuffer(n_out * 4)
    d_in.upload(src)
    with nb.Interpolator(48000) as c:
        assert c.resident(d_in, n, n, d_out, n_out) == n_out
        words = d_out.download(n_out * 4, dtype=np.int16).reshape(-1, 2)
    assert np.array_equal(words, want), _first_difference(words, want)
    got_bits, msgs = _decode_on_the_device(nv, d_out, n_out, n_out, 1, nv.CHAIN_518 | nv.CHAIN_490, {})
    d_in.free(); d_out.free()
    cpu_msgs, cpu_bits = ic.delivered(oracle, want, nv.FRAME_IN)
    assert (got_bits[(0, 0)], got_bits[(0, 1)]) == cpu_bits
    assert {f: [m[3] for m in msgs if m[1] == f] for f in (518, 490)} == cpu_msgs == {518: [texts[0]], 490: [texts[1]]}


def test_interpolate_then_scan_finds_the_carrier(nv, nb):
    """nvx_nb -> nvx_scan_resident -> nvx_scan_find on the 12 kS/s case: the carrier within 5 Hz of -1000.  It is the first hit (the
    highest score) and the strongest.  A 12 kS/s source fills +-4.8 kHz of the scan's +-31.5 kHz; the rest holds only what the
    interpolator's stop band lets through, and there the scan lists the carrier's images at multiples of 12 kHz as faint
    carriers: the design's bar puts every hit beyond fi - fp = 7.2 kHz from the centre at least 76 dB below it (91 dB and more
    from the restatement's output)."""
    import navtex_amd.scan as sc
    src = nc.source(nv, 20)
    frames = 3
    n = frames * 12000 * 8 // 25
    d_in = nv.DeviceBuffer(n * 4); d_out = nv.DeviceBuffer(frames * nv.FRAME_IN * 4)
    d_in.upload(src[:n])
    with nb.Interpolator(12000) as c:
        assert c.resident(d_in, n, n, d_out, frames * nv.FRAME_IN) == frames * nv.FRAME_IN
        row = sc.scan_resident(d_out, frames * nv.FRAME_IN, 0, frames, 1, False)[0]
    d_in.free(); d_out.free()
    hits = sc.find(row)
    assert hits and abs(hits[0]["offset_hz"] + 1000.0) <= 5.0 and abs(hits[0]["shift_hz"] - 170.0) <= 15.0, hits
    assert all(h["score_db"] < hits[0]["score_db"] and h["band_power_db"] < hits[0]["band_power_db"] for h in hits[1:]), hits
    assert all(h["band_power_db"] <= hits[0]["band_power_db"] - 76.0 for h in hits[1:] if abs(h["offset_hz"]) >= 7200.0), hits
