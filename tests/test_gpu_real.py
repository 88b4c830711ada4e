"""The real-input converter (include/navtex_amd_real.h) on the GPU (-m gpu): output words equal to the restatement
(tests/real_ref.py) in every format, calls cut anywhere against one shot with a history shorter than, equal to and longer
than a call, a reset stream rejoining the others, the rails and full-scale random input (float32 specials), inverted, the two
launch shapes, positions beyond 2^32, push against resident with odd calls, the refusals, and the acceptance case's seed 11
through a two-chain handle.  Every comparison is ==, with sentinels around every output row."""
from pathlib import Path

import numpy as np
import pytest

import real_cases as rc
import real_ref as rf
from real_cases import _first_difference, _run_resident

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FORMATS = (rf.S16, rf.U8, rf.S8, rf.F32)
FORMAT_IDS = ("s16", "u8", "s8", "f32")
T = 4096                                  # outputs of a tile


@pytest.fixture(scope="module")
def rl(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_real.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.real
    assert navtex_amd.real.TILE == T
    return navtex_amd.real


# ------------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_two_streams_of_three_tiles_and_six_in_every_format(nv, rl, fmt):
    """2 streams x (3 T + 6) outputs.  A pitch larger than the data; out_first = 7 (the unaligned stores) and 8."""
    n = 2 * (3 * T + 6)
    rows = [rc.signal(fmt, n, 200 + 10 * fmt + s) for s in range(2)]
    want = [rf.convert_all(row, fmt)[0] for row in rows]
    for out_first in (7, 8):
        with rl.Converter(fmt, n_streams=2) as c:
            got = _run_resident(nv, c, rows, [n], pitch_extra=3 + out_first % 2, out_first=out_first)
            for s in range(2):
                assert np.array_equal(got[s], want[s]), (out_first, s, _first_difference(got[s], want[s]))


# ------------------------------------------------------------------------------------------------------------------ (b)
def test_one_shot_equals_calls_shorter_and_longer_than_the_history_and_a_reset_stream_rejoins(nv, rl):
    """Calls of 2, 54, 56, 58, 0 and 2 T + 2 samples and the rest: 1, 27, 28 and 29 pairs against a history of 28."""
    cuts = [2, 54, 56, 58, 0, 2 * T + 2]
    n1 = 2 * (3 * T + 77)
    cuts = cuts + [n1 - sum(cuts)]
    tail = 2 * (T + 33)
    rows = [rc.signal(rf.S16, n1 + tail, 400 + s) for s in range(3)]
    want = [rf.convert_all(row)[0] for row in rows]
    with rl.Converter(rf.S16, n_streams=3) as c:
        got = _run_resident(nv, c, [row[:n1] for row in rows], cuts)
        for s in range(3):
            assert np.array_equal(got[s], want[s][:n1 // 2]), (s, _first_difference(got[s], want[s][:n1 // 2]))
        c.reset(1)
        assert c.position(1) == (0, 0) and c.position(0) == (n1, n1 // 2)
        d = nv.DeviceBuffer(3 * 64 * 2); o = nv.DeviceBuffer(3 * 64 * 4)
        launches = c.debug_last_launch()["launches"]
        assert rl.lib.nvx_real_resident(c._h, d.ptr, 64, 64, o.ptr, 64, 0, None) == nv._native.ERR_STATE
        assert b"same position" in rl.lib.nvx_real_last_error() and c.debug_last_launch()["launches"] == launches
        d.free(); o.free()
        # stream 1 starts anew on other data, alone and in calls of its own, up to where the others stand
        fresh = rf.Converter(rf.S16)
        other = rc.signal(rf.S16, n1 + tail, 450)
        pos = 0
        for cut in (10, 2, T + 6, n1 - T - 18):
            assert np.array_equal(c.push(1, other[pos:pos + cut]), fresh.push(other[pos:pos + cut])), pos
            pos += cut
        assert c.position(1) == (n1, n1 // 2)
        got = _run_resident(nv, c, [rows[0][n1:], other[n1:], rows[2][n1:]], [tail])
        assert np.array_equal(got[0], want[0][n1 // 2:]) and np.array_equal(got[2], want[2][n1 // 2:])
        assert np.array_equal(got[1], fresh.push(other[n1:]))


# ------------------------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("invert", [0, 1], ids=["upright", "inverted"])
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_the_rails_and_full_scale_random_input(nv, rl, fmt, invert):
    """Every sample at the lowest value, the odd samples stepping between the rails (acc = +-18610 * 65535 in S16: the largest
    sum there is, clamped both ways), and full-scale random input with the float32 specials."""
    n = 2 * (T + 2000)
    dt = rf.DTYPES[fmt]
    lo, hi = (np.float32(-1.0), np.float32(32767.0 / 32768.0)) if fmt == rf.F32 else (np.iinfo(dt).min, np.iinfo(dt).max)
    step = np.where(rc.rails_step(n) > 0, hi, lo).astype(dt)
    rows = [np.full(n, lo, dtype=dt), step, rc.full_scale(fmt, n, 500 + fmt)]
    refs = [rf.convert_all(row, fmt, invert) for row in rows]
    if fmt in (rf.S16, rf.F32):
        assert (refs[1][1].acc_min, refs[1][1].acc_max) == (-rf.ACC_MAX, rf.ACC_MAX)
        assert refs[1][0][:, 1].min() == -32768 and refs[1][0][:, 1].max() == 32767 and refs[0][0][:, 0].max() == 32767
    if fmt == rf.S16:
        assert np.array_equal(rows[0], rc.rails_low(n)) and np.array_equal(rows[1], rc.rails_step(n))
    with rl.Converter(fmt, n_streams=3, invert=invert) as c:
        got = _run_resident(nv, c, rows, [2 * 1011, n - 2 * 1011], out_first=3)
        for s in range(3):
            assert np.array_equal(got[s], refs[s][0]), (s, _first_difference(got[s], refs[s][0]))


# ------------------------------------------------------------------------------------------------------------------ (d)
def test_a_stream_spread_over_chunks(nv, rl):
    """1 stream x (12 T + 5) outputs behind a first call of 38 samples: four workgroups of four tiles each, the last with one
    whole tile and five outputs; every later chunk takes its halo from the input."""
    first, n = 38, 2 * (12 * T + 5)
    row = rc.signal(rf.S16, first + n, 70)
    want, _ = rf.convert_all(row)
    with rl.Converter(rf.S16) as c:
        got = _run_resident(nv, c, [row], [first, n])
        assert c.debug_last_launch() == {"launches": 2, "chunks": 4, "tiles_per_chunk": 4, "form": 2}
        assert np.array_equal(got[0], want), _first_difference(got[0], want)


def test_scale_1024_streams_at_one_chunk_each(nv, rl):
    """1024 streams x (T + 10) outputs of unsigned 8-bit samples, sixteen different rows among them."""
    ns, n, kinds = 1024, 2 * (T + 10), 16
    pitch = (n + 15) // 16 * 16
    rows = [rc.signal(rf.U8, n, 7000 + k) for k in range(kinds)]
    want = [rf.convert_all(row, rf.U8)[0] for row in rows]
    block = np.zeros((kinds, pitch), dtype=np.uint8)
    block[:, :n] = np.stack(rows)
    d_in = nv.DeviceBuffer(ns * pitch); d_out = nv.DeviceBuffer(ns * (n // 2) * 4)
    for s in range(0, ns, kinds):
        d_in.upload(block, s * pitch)
    with rl.Converter(rf.U8, n_streams=ns) as c:
        c.resident(d_in, pitch, n, d_out, n // 2)
        got = d_out.download(ns * (n // 2) * 4, dtype=np.int16).reshape(ns, n // 2, 2)
        assert c.debug_last_launch() == {"launches": 1, "chunks": 1, "tiles_per_chunk": 2, "form": 1}
    d_in.free(); d_out.free()
    bad = [s for s in range(ns) if not np.array_equal(got[s], want[s % kinds])]
    assert not bad, bad[:10]


# ------------------------------------------------------------------------------------------------------------------ (e)
@pytest.mark.parametrize("position", [2 ** 32 - 1000, 2 ** 40 + 6])
def test_positions_beyond_32_bits(nv, rl, position):
    """60 samples in two calls from the position: silence in front of it, and only its parity enters the sign (2^32 - 1000 has
    an even output index, 2^40 + 6 an odd one)."""
    rows = [rc.signal(rf.S16, 60, 80 + s) for s in range(2)]
    refs = [rf.Converter(rf.S16, 0, position) for _ in rows]
    assert (position // 2) % 2 == (0 if position == 2 ** 32 - 1000 else 1)
    with rl.Converter(rf.S16, n_streams=2) as c:
        c.debug_set_position(position)
        assert c.position(1) == (position, position // 2)
        got = _run_resident(nv, c, rows, [22, 38])
        for s in range(2):
            want = refs[s].push(rows[s])
            assert np.array_equal(got[s], want), (s, _first_difference(got[s], want))
        assert rl.lib.nvx_real_debug_set_position(c._h, 0, position + 1) == nv._native.ERR_ARG


# ------------------------------------------------------------------------------------------------------------------ (f)
@pytest.mark.parametrize("fmt", [rf.S16, rf.S8, rf.F32], ids=["s16", "s8", "f32"])
def test_push_equals_resident(nv, rl, fmt):
    n = 2 * (T + 500)
    rows = [rc.signal(fmt, 2 * n, 120 + s) for s in range(3)]
    want = [rf.convert_all(row, fmt)[0] for row in rows]
    with rl.Converter(fmt, n_streams=3) as c:
        for s, cuts in enumerate(([n], [1, 2 * T - 1, n - 2 * T], [7, 0, 1, 2 * T + 501, 3, n - 2 * T - 512])):
            pos, parts = 0, []
            for cut in cuts:
                parts.append(c.push(s, rows[s][pos:pos + cut])); pos += cut
                assert c.position(s) == (pos, pos // 2)
            out = np.concatenate(parts)
            assert out.dtype == np.int16 and np.array_equal(out, want[s][:n // 2]), (s, _first_difference(out, want[s][:n // 2]))
        got = _run_resident(nv, c, [row[n:] for row in rows], [n])
        for s in range(3):
            assert np.array_equal(got[s], want[s][n // 2:]), s


def test_span_odd_and_position_errors_launch_nothing(nv, rl):
    ARG, STATE = nv._native.ERR_ARG, nv._native.ERR_STATE
    n = 8192
    with rl.Converter(rf.U8, n_streams=2) as c:
        d_in = nv.DeviceBuffer(2 * n); d_out = nv.DeviceBuffer(2 * (n // 2) * 4)
        one_in = nv.DeviceBuffer(n); one_out = nv.DeviceBuffer((n // 2) * 4)
        c.timing(True)
        call = lambda *a: rl.lib.nvx_real_resident(c._h, *a, None)            # noqa: E731
        bad = {"an odd number of samples": (d_in.ptr, n, n - 1, d_out.ptr, n // 2, 0),
               "more samples than the pitch": (d_in.ptr, n - 16, n, d_out.ptr, n // 2, 0),
               "words beyond the pitch": (d_in.ptr, n, n, d_out.ptr, n // 2 - 1, 0),
               "out_first pushes them beyond it": (d_in.ptr, n, n, d_out.ptr, n // 2, 1),
               "input rows for one stream": (one_in.ptr, n, n, d_out.ptr, n // 2, 0),
               "output rows for one stream": (d_in.ptr, n, n, one_out.ptr, n // 2, 0),
               "misaligned input": (d_in.ptr + 4, n, n - 16, d_out.ptr, n // 2, 0),
               "misaligned output": (d_in.ptr, n, n, d_out.ptr + 2, n // 2, 0),
               "rows not 16-byte aligned": (d_in.ptr, n - 3, n - 16, d_out.ptr, n // 2, 0),
               "null input": (None, n, n, d_out.ptr, n // 2, 0),
               "null output": (d_in.ptr, n, n, None, n // 2, 0),
               "too many samples": (d_in.ptr, 2 ** 32, 2 ** 31 + 2, d_out.ptr, 2 ** 31, 0),
               "a pitch that wraps": (d_in.ptr, 2 ** 64 - 16, n, d_out.ptr, n // 2, 0),
               "an output pitch that wraps": (d_in.ptr, n, n, d_out.ptr, 2 ** 62, 0),
               "out_first that wraps": (d_in.ptr, n, n, d_out.ptr, n // 2, 2 ** 64 - 8)}
        for name, args in bad.items():
            assert call(*args) == ARG, name
            assert rl.lib.nvx_real_last_error() != b""
        c.debug_set_position(2 ** 62 - 100)
        assert call(d_in.ptr, n, n, d_out.ptr, n // 2, 0) == ARG and b"2^62" in rl.lib.nvx_real_last_error()
        assert rl.lib.nvx_real_debug_set_position(c._h, 0, 2 ** 62) == ARG and rl.lib.nvx_real_debug_set_position(c._h, 2, 0) == ARG
        assert rl.lib.nvx_real_reset(c._h, 2) == ARG and rl.lib.nvx_real_position(c._h, 2, None, None) == ARG
        assert c.time_stats() == (0.0, 0) and c.debug_last_launch()["launches"] == 0 and c.position(0) == (2 ** 62 - 100, 2 ** 61 - 50)
        c.reset()
        # a push too long for its output buffer consumes nothing; one odd sample is held, and a held sample bars a resident call
        x = np.full(9, 128, dtype=np.uint8)
        out = np.zeros((8, 2), dtype=np.int16)
        n_out = rl.C.c_size_t(77)
        assert rl.lib.nvx_real_push(c._h, 0, nv._native.as_ptr(x), 9, nv._native.as_ptr(out), 3, rl.C.byref(n_out)) == ARG and c.position(0) == (0, 0)
        assert c.debug_last_launch()["launches"] == 0
        assert len(c.push(0, x[:1])) == 0 and c.position(0) == (1, 0) and c.debug_last_launch()["launches"] == 0
        assert call(d_in.ptr, n, n, d_out.ptr, n // 2, 0) == STATE and b"odd sample" in rl.lib.nvx_real_last_error()
        c.reset(0)
        assert call(d_in.ptr, n, 0, d_out.ptr, n // 2, 0) == 0 and c.debug_last_launch()["launches"] == 0       # nothing to do: no launch
        d_in.upload(np.full(2 * n, 128, dtype=np.uint8))
        assert call(d_in.ptr, n, n, d_out.ptr, n // 2, 0) == 0
        ms, calls = c.time_stats()
        assert calls == 1 and ms > 0.0 and c.debug_last_launch()["launches"] == 1 and c.position(1) == (n, n // 2)
        for d in (d_in, d_out, one_in, one_out):
            d.free()
    for kw in (dict(device=99), dict(invert=2), dict(format=4), dict(n_streams=0)):
        with pytest.raises(nv.NvxError) as e:
            rl.Converter(**kw)
        assert e.value.code == ARG, kw


# ------------------------------------------------------------------------------------------------------------------ (g)
def test_seed_11_of_the_acceptance_case_on_the_device(nv, rl, oracle):
    """The real row of seed 11 through the converter on the device: the words are the CPU's.  Then the converted and the naive
    row as two streams of a two-chain raw_rate = 0 handle: both messages arrive from the converted row, the 490 message does
    not arrive from the naive one, and the bits of all four chains are the oracle's on the same words."""
    t518, t490 = rc.texts()
    x = rc.real_row(nv, 11)
    n = len(x) // 2
    want, _ = rf.convert_all(x)
    naive = rc.naive(x)
    d_real = nv.DeviceBuffer(len(x) * 2)
    d_in = nv.DeviceBuffer(2 * n * 4)                       # the handle's input: row 0 converted, row 1 naive
    d_real.upload(x)
    d_in.upload(naive, n * 4)
    with rl.Converter(rf.S16) as c:
        c.resident(d_real, len(x), len(x), d_in, n)
        got = d_in.download(2 * n * 4, dtype=np.int16).reshape(2, n, 2)
        assert np.array_equal(got[0], want), _first_difference(got[0], want)
        assert np.array_equal(got[1], naive) and c.debug_last_launch()["form"] == 2
    d_real.free()
    frames = n // nv.FRAME_IN
    with nv.Pipeline(n_streams=2, chain_mask=nv.CHAIN_518 | nv.CHAIN_490, max_frames=8) as p:
        for f0 in range(0, frames, 8):
            p.process_resident(d_in, n, f0, min(8, frames - f0), hip_stream=p.hip_stream)
        p.fetch()
        bits = [(p.bits(s, 0), p.bits(s, 1)) for s in range(2)]
        msgs = [{f: [m[3] for m in p.messages if m[0] == s and m[1] == f] for f in (518, 490)} for s in range(2)]
    d_in.free()
    cpu = [rc.delivered(oracle, row, nv.FRAME_IN) for row in (want, naive)]
    for s in range(2):
        assert bits[s] == cpu[s][1] and msgs[s] == cpu[s][0], s
    assert msgs[0][518] == [t518] and msgs[0][490] == [t490]
    assert msgs[1][490] != [t490]
