"""The channel tap (include/navtex_amd_tap.h) on the GPU (-m gpu): output samples equal to the restatement (tests/tap_ref.py)
in both kinds at every form the kernel takes -- L = 1 with taps wave-uniform (M odd and M even), L > 1 with taps per lane, tiles
of 256 and 128 outputs --, shifts, pitches and every output alignment, calls cut anywhere against one shot, push against
resident, inputs pushed apart and a reset input rejoining, a retune between calls, the rails and full-scale random input,
positions beyond 2^32, two shapes at scale, the refusals, and a station from a 252 kS/s row to a message on the device:
tap -> interpolator -> tuned handle, the audio kind, and the scan.  Every comparison is ==, with sentinels around every output
row and full-scale samples behind every call's input."""
from pathlib import Path

import numpy as np
import pytest

import tap_cases as tc
import tap_ref as tr
from tap_cases import _flat, _run_resident, _same, _set_shifts, tp_bytes

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SHIFTS = ((0.0, 14000.0), (-14000.0, 5000.5), (60000.0, -100.0))       # per input and tap, Hz: one k = 0
# (tile_out, form) the plan takes: form 1 = taps wave-uniform (L = 1 and waves * M a multiple of 4), 2 = per lane (L > 1, and
# 2016 S/s: L = 1, M = 125, two waves)
SHAPES = {(12000, tr.IQ): (256, 1), (48000, tr.IQ): (256, 2), (11025, tr.IQ): (256, 2), (96000, tr.IQ): (256, 2), (6250, tr.IQ): (256, 2),
          (2000, tr.IQ): (128, 1), (2016, tr.IQ): (128, 2), (8000, tr.REAL): (256, 2), (11025, tr.REAL): (256, 2), (48000, tr.REAL): (256, 2), (12000, tr.REAL): (256, 1)}


@pytest.fixture(scope="module")
def tp(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_tap.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.tap
    return navtex_amd.tap


@pytest.fixture(scope="module")
def designs(tp):
    cache = {}
    def get(fo, kind=tr.IQ):
        if (fo, kind) not in cache:
            cache[(fo, kind)] = tp.design(fo, kind)
        return cache[(fo, kind)]
    return get


# ------------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("fo,kind", [(12000, tr.IQ), (48000, tr.IQ), (11025, tr.IQ), (96000, tr.IQ), (6250, tr.IQ), (2000, tr.IQ), (2016, tr.IQ), (8000, tr.REAL),
                                     (11025, tr.REAL), (48000, tr.REAL), (12000, tr.REAL)],
                         ids=lambda v: str(v))
def test_three_inputs_of_two_taps_at_every_output_alignment(nv, tp, designs, fo, kind):
    """3 inputs x 2 taps with different shifts (one k = 0), 20 000 input samples: at 12 kS/s three tiles and a ragged fourth.
    A larger pitch on tap 1 of the audio kind.  A pitch larger than the data; out_first at each residue mod 4 (IQ) and mod 8
    (REAL)."""
    L, M, T, h = designs(fo, kind)
    assert (L, M, T) == tc.PLAN_OF.get((fo, kind), (1, 125, 3574))            # 2016 S/s: L = 1 with M odd and a tile of two waves
    n = 20000
    rows = [tc.signal(n, 100 * kind + s + fo) for s in range(3)]
    with tp.Tap(fo, kind, n_inputs=3, n_taps=2) as c:
        assert (c.L, c.M, c.T) == (L, M, T)
        ks, kps = _set_shifts(c, SHIFTS, kind, (None, 1500.0))
        assert ks[0][0] == 0 and all(k != 0 for k in _flat(ks)[1:])
        want = _flat([tr.tap_all(rows[i], h, L, M, kind, ks[i], kps)[0] for i in range(3)])
        for out_first in ((8, 5, 6, 7) if kind == tr.IQ else (8, 9, 10, 11, 12, 13, 14, 15)):
            c.reset()
            got = _run_resident(nv, c, rows, [n], pitch_extra=1 + out_first % 4, out_first=out_first)
            shape = c.debug_last_launch()
            assert (shape["tile_out"], shape["form"]) == SHAPES[(fo, kind)] and shape["tiles"] == -(-len(want[0]) // shape["tile_out"]), shape
            assert shape["waves"] == shape["tile_out"] // 64 and shape["lds_bytes"] <= 80 * 1024
            _same(got, want, (fo, kind, out_first))


# ------------------------------------------------------------------------------------------------------------------ (b)
def test_one_shot_equals_short_calls_push_equals_resident_a_reset_input_rejoins_and_a_retune_between_calls(nv, tp, designs):
    """Calls of 0, 1, T - 2, T - 1, T and several thousand samples against one shot; then the inputs pushed one by one and apart,
    meeting again for a resident call; then input 1 reset, refused while it stands elsewhere, pushed back up and rejoining;
    then a retune between two calls: the carried samples are mixed with the new shift, as the restatement has it."""
    fo, kind = 11025, tr.IQ
    L, M, T, h = designs(fo, kind)
    cuts = [0, 1, T - 2, T - 1, T, 3000, 0, 1, 2500]
    n1, n2, n3, n4 = sum(cuts), 2100, 900, 1500
    rows = [tc.signal(n1 + n2 + n3 + n4, 400 + s) for s in range(3)]
    with tp.Tap(fo, kind, n_inputs=3, n_taps=2) as c:
        ks, _ = _set_shifts(c, SHIFTS, kind)
        refs = [tr.Tap(h, L, M, kind, ks[i]) for i in range(3)]
        one = [tr.tap_all(rows[i][:n1], h, L, M, kind, ks[i])[0] for i in range(3)]
        got = _run_resident(nv, c, [row[:n1] for row in rows], cuts)
        _same(got, _flat(one), "cuts")
        _same(got, _flat([refs[i].push(rows[i][:n1]) for i in range(3)]), "the restatement in one call")
        # pushed apart: each input in calls of its own
        for s, pcuts in enumerate(([n2], [1, 0, T - 1, n2 - T], [333, 1, n2 - 334])):
            pos, parts = n1, []
            for cut in pcuts:
                parts.append(c.push(s, rows[s][pos:pos + cut])); pos += cut
                assert c.position(s) == (pos, tr.outputs_after(pos, L, M))
            out = np.concatenate(parts, axis=1)
            assert out.dtype == np.int16
            _same(list(out), refs[s].push(rows[s][n1:n1 + n2]), ("pushed", s))
        # a reset input stands elsewhere: the resident call is refused and launches nothing
        c.reset(1)
        assert c.position(1) == (0, 0) and c.position(0) == (n1 + n2, tr.outputs_after(n1 + n2, L, M))
        assert c.get_shift(1, 1)[0] == ks[1][1]                                 # a reset leaves the shifts alone
        d = nv.DeviceBuffer(3 * 64 * 4); o = nv.DeviceBuffer(6 * 2048 * 4)
        launches = c.debug_last_launch()["launches"]
        assert tp.lib.nvx_tap_resident(c._h, d.ptr, 64, 64, o.ptr, 2048, 0, None, None) == nv._native.ERR_STATE
        assert b"same position" in tp.lib.nvx_tap_last_error() and c.debug_last_launch()["launches"] == launches
        d.free(); o.free()
        refs[1].reset()
        other = tc.signal(n1 + n2 + n3 + n4, 450)
        pos = 0
        for cut in (10, 1, 2000, n1 + n2 - 2011):
            _same(list(c.push(1, other[pos:pos + cut])), refs[1].push(other[pos:pos + cut]), ("back up", pos))
            pos += cut
        tail = [rows[0], other, rows[2]]
        got = _run_resident(nv, c, [r[n1 + n2:n1 + n2 + n3] for r in tail], [n3])
        _same(got, _flat([refs[i].push(tail[i][n1 + n2:n1 + n2 + n3]) for i in range(3)]), "rejoined")
        # a retune between calls
        c.set_shift(0, -31000.0, input=0); c.set_shift(1, 777.0)
        refs[0].ks[0] = tr.grid(fo, kind, -31000.0)
        for r in refs:
            r.ks[1] = tr.grid(fo, kind, 777.0)
        got = _run_resident(nv, c, [r[n1 + n2 + n3:] for r in tail], [n4 - 600, 600])
        _same(got, _flat([refs[i].push(tail[i][n1 + n2 + n3:]) for i in range(3)]), "retuned")


# ------------------------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("fo,kind", [(12000, tr.IQ), (8000, tr.REAL)], ids=["iq_12000", "real_8000"])
def test_the_rails_and_full_scale_random_input(nv, tp, designs, fo, kind):
    """Windows matched in sign to the phase with the largest sum |h|, every second one and Q negated, through a tap with k = 0:
    the value before the clamp is beyond int16 on both sides, and the sum needs more than 32 bits.  And full-scale random
    input through shifted taps."""
    L, M, T, h = designs(fo, kind)
    rails = tc.rails(h, L, M, 6)
    n = len(rails)
    rows = [rails, tc.full_scale(n, 500 + kind), tc.full_scale(n, 600 + kind)]
    with tp.Tap(fo, kind, n_inputs=3, n_taps=2) as c:
        ks, kps = _set_shifts(c, SHIFTS, kind, (None, 2000.0))
        refs = [tr.tap_all(rows[i], h, L, M, kind, ks[i], kps) for i in range(3)]
        assert refs[0][1].acc_max >> 21 > 50000 and refs[0][1].acc_min >> 21 < -50000 and refs[0][1].acc_max > 1 << 36
        if kind == tr.IQ:
            r0 = refs[0][0][0]
            assert {int(r0[:, 0].max()), int(r0[:, 0].min()), int(r0[:, 1].max()), int(r0[:, 1].min())} == {32767, -32768}
        got = _run_resident(nv, c, rows, [T + 301, n - T - 301], out_first=3)
        _same(got, _flat([r[0] for r in refs]), "rails")


# ------------------------------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("fo,kind", [(11025, tr.IQ), (8000, tr.REAL)], ids=["iq_11025", "real_8000"])
@pytest.mark.parametrize("position", [2 ** 32 - 1000, 2 ** 40 + 6])
def test_positions_beyond_32_bits(nv, tp, designs, position, fo, kind):
    """6000 samples in two calls from the position: silence in front of it, the phase of its first output is the position's, and
    the mixer's and the pitch's indices are the true ones (odd steps: every bit of the index counts)."""
    L, M, T, h = designs(fo, kind)
    rows = [tc.signal(6000, 80 + s) for s in range(2)]
    with tp.Tap(fo, kind, n_inputs=2, n_taps=2) as c:
        ks, kps = _set_shifts(c, ((61.5, -20000.0), (922.9, 0.0)), kind, (1002.0, 1500.0))
        assert ks[0][0] % 2 == 1 and ks[1][0] % 2 == 1 and (kps is None or kps[0] % 2 == 1)
        refs = [tr.Tap(h, L, M, kind, ks[i], kps, position=position) for i in range(2)]
        c.debug_set_position(position)
        assert c.position(1) == (position, tr.outputs_after(position, L, M))
        got = _run_resident(nv, c, rows, [2222, 3778])
        _same(got, _flat([refs[s].push(rows[s]) for s in range(2)]), position)


# ------------------------------------------------------------------------------------------------------------------ (e)
def _scale(nv, tp, designs, fo, ni, nt, cuts):
    L, M, T, h = designs(fo, tr.IQ)
    kinds = 8
    n = sum(cuts)
    rows = [tc.signal(n, 7000 + k) for k in range(kinds)]
    hz = [0.0, 14000.0, -9000.0][:nt]
    ks = [tr.grid(fo, tr.IQ, f) for f in hz]
    want = np.stack([np.stack(tr.tap_all(row, h, L, M, tr.IQ, ks)[0]) for row in rows])       # [kinds, nt, n_out, 2]
    n_out = want.shape[2]
    pitch = max(cuts) + 4
    d_in = nv.DeviceBuffer(ni * pitch * 4); d_out = nv.DeviceBuffer(ni * nt * n_out * 4)
    with tp.Tap(fo, tr.IQ, n_inputs=ni, n_taps=nt) as c:
        for t, f in enumerate(hz):
            c.set_shift(t, f)
        pos = made = 0
        for cut in cuts:
            block = np.full((kinds, pitch, 2), 32767, dtype=np.int16)
            block[:, :cut] = np.stack([row[pos:pos + cut] for row in rows])
            d_in.upload(np.tile(block, ((ni + kinds - 1) // kinds, 1, 1))[:ni])
            made += c.resident(d_in, pitch, cut, d_out, n_out, made)
            pos += cut
        assert made == n_out
        got = d_out.download(ni * nt * n_out * 4, dtype=np.int16).reshape(ni, nt, n_out, 2)
    d_in.free(); d_out.free()
    bad = [k for k in range(kinds) if not np.array_equal(got[k::kinds], np.broadcast_to(want[k], got[k::kinds].shape))]
    assert not bad, bad


def test_scale_1024_inputs_of_two_taps(nv, tp, designs):
    """1024 inputs x 2 taps x 4000 samples at 12 kS/s."""
    _scale(nv, tp, designs, 12000, 1024, 2, [4000])


def test_scale_65535_rows_in_two_short_calls(nv, tp, designs):
    """21 845 inputs x 3 taps = 65 535 rows x two calls of 37 and 40 samples at 8 kS/s."""
    _scale(nv, tp, designs, 8000, 21845, 3, [37, 40])


# ------------------------------------------------------------------------------------------------------------------ (f)
def test_span_count_position_shift_and_pitch_errors_launch_nothing(nv, tp):
    ARG = nv._native.ERR_ARG
    n, outs = 2100, 100
    with tp.Tap(12000, tr.IQ, n_inputs=2, n_taps=2) as c, tp.Tap(8000, tr.REAL, n_inputs=1, n_taps=2) as a:
        d_in = nv.DeviceBuffer(2 * n * 4); d_out = nv.DeviceBuffer(4 * outs * 4)
        one_in = nv.DeviceBuffer(n * 4); one_out = nv.DeviceBuffer(outs * 4)
        c.timing(True)
        call = lambda *args: tp.lib.nvx_tap_resident(c._h, *args, None, None)          # noqa: E731
        bad = {"more samples than the pitch": (d_in.ptr, n - 1, n, d_out.ptr, outs, 0),
               "outputs beyond the pitch": (d_in.ptr, n, n, d_out.ptr, outs - 1, 0),
               "out_first pushes them beyond it": (d_in.ptr, n, n, d_out.ptr, outs, 1),
               "input rows for one input": (one_in.ptr, n, n, d_out.ptr, outs, 0),
               "output rows for one row": (d_in.ptr, n, n, one_out.ptr, outs, 0),
               "misaligned input": (d_in.ptr + 2, n, n - 1, d_out.ptr, outs, 0),
               "misaligned output": (d_in.ptr, n, n, d_out.ptr + 2, outs, 0),
               "null input": (None, n, n, d_out.ptr, outs, 0),
               "null output": (d_in.ptr, n, n, None, outs, 0),
               "too many samples": (d_in.ptr, 2 ** 32, 2 ** 30 + 1, d_out.ptr, 2 ** 36, 0),
               "a pitch that wraps": (d_in.ptr, 2 ** 64 - 16, n, d_out.ptr, outs, 0),
               "an output pitch that wraps": (d_in.ptr, n, n, d_out.ptr, 2 ** 62, 0),
               "out_first that wraps": (d_in.ptr, n, n, d_out.ptr, outs, 2 ** 64 - 8)}
        for name, args in bad.items():
            assert call(*args) == ARG, name
            assert tp.lib.nvx_tap_last_error() != b""
        c.debug_set_position(2 ** 62 - 100)
        assert call(d_in.ptr, n, n, d_out.ptr, outs, 0) == ARG and b"2^62" in tp.lib.nvx_tap_last_error()
        assert tp.lib.nvx_tap_debug_set_position(c._h, 0, 2 ** 62) == ARG and tp.lib.nvx_tap_debug_set_position(c._h, 2, 0) == ARG
        assert tp.lib.nvx_tap_reset(c._h, 2) == ARG and tp.lib.nvx_tap_position(c._h, 2, None, None) == ARG
        c.reset()
        # shifts: the pass band must stay inside the input's band; rows that do not exist
        limit = 126000 - 4800                               # grid step 1969 is the last inside it, at 121 139.6 Hz
        for hz in (limit + 40.0, -limit - 40.0, float(limit), float("nan"), float("inf"), 1e9):
            assert tp.lib.nvx_tap_set_shift(c._h, 0, 0, hz, None) == ARG, hz
        assert c.set_shift(0, limit - 40.0, input=0) == 1969 * 252000 / 4096 == tr.grid(12000, tr.IQ, limit - 40.0) * 252000 / 4096
        assert tr.grid(12000, tr.IQ, limit + 40.0) is None and tr.grid(12000, tr.IQ, limit) is None and c.set_shift(0, 0.0, input=0) == 0.0
        for args in ((2, 0), (-2, 0), (0, 2), (0, -1)):
            assert tp.lib.nvx_tap_set_shift(c._h, *args, 100.0, None) == ARG, args
        for args in ((2, 0), (-1, 0), (0, 2), (0, -1)):
            assert tp.lib.nvx_tap_get_shift(c._h, *args, None, None) == ARG, args
        # pitches: audio only, 800 Hz .. fo / 2 - 800 Hz
        assert tp.lib.nvx_tap_set_pitch(c._h, 0, 0, 1000.0, None) == ARG and b"only audio" in tp.lib.nvx_tap_last_error()
        assert tp.lib.nvx_tap_get_pitch(c._h, 0, 0, None, None) == ARG
        for hz in (799.0, 3201.5, 0.0, -1000.0, float("nan")):
            assert tp.lib.nvx_tap_set_pitch(a._h, -1, 0, hz, None) == ARG, hz
            assert tr.pitch_grid(8000, hz) is None if hz == hz else True
        assert a.set_pitch(0, 800.8) == tr.pitch_grid(8000, 800.8) * 8000 / 4096 and a.set_pitch(1, 3200.0) == 1638 * 8000 / 4096
        assert a.get_pitch(0)[0] == 410 and a.get_pitch(1) == (tr.pitch_grid(8000, 3200), 1638 * 8000 / 4096)
        assert tp.lib.nvx_tap_set_pitch(a._h, 1, 0, 1000.0, None) == ARG and tp.lib.nvx_tap_set_pitch(a._h, 0, 2, 1000.0, None) == ARG
        assert c.time_stats() == (0.0, 0) and c.debug_last_launch()["launches"] == 0 and a.debug_last_launch()["launches"] == 0
        # a push too long for its output buffer consumes nothing
        x = np.zeros((2100, 2), dtype=np.int16)
        out = np.zeros((2, 100, 2), dtype=np.int16)
        n_out = tp.C.c_size_t(77)
        assert tp.lib.nvx_tap_push(c._h, 0, nv._native.as_ptr(x), 2100, nv._native.as_ptr(out), 99, tp.C.byref(n_out)) == ARG and c.position(0) == (0, 0)
        assert tp.lib.nvx_tap_push(c._h, 2, nv._native.as_ptr(x), 2100, nv._native.as_ptr(out), 100, tp.C.byref(n_out)) == ARG
        assert n_out.value == 77 and c.debug_last_launch()["launches"] == 0
        assert c.push(0, x[:0]).shape == (2, 0, 2) and c.debug_last_launch()["launches"] == 0
        size = tp.C.c_size_t(5)
        assert tp.lib.nvx_tap_resident(c._h, d_in.ptr, n, 0, d_out.ptr, outs, 0, tp.C.byref(size), None) == 0 and size.value == 0
        assert c.debug_last_launch()["launches"] == 0       # nothing to do: no launch
        d_in.upload(np.zeros(2 * n * 2, dtype=np.int16))
        assert call(d_in.ptr, n, n, d_out.ptr, outs, 0) == 0
        ms, calls = c.time_stats()
        assert calls == 1 and ms > 0.0 and c.debug_last_launch()["launches"] == 1 and c.position(1) == (n, outs)
        for d in (d_in, d_out, one_in, one_out):
            d.free()
    for kw in (dict(output_rate_hz=12000, device=99), dict(output_rate_hz=1999), dict(output_rate_hz=96001), dict(output_rate_hz=2001),
               dict(output_rate_hz=7999, kind=tr.REAL), dict(output_rate_hz=48001, kind=tr.REAL), dict(output_rate_hz=12000, kind=2),
               dict(output_rate_hz=12000, n_inputs=0), dict(output_rate_hz=12000, n_taps=0), dict(output_rate_hz=12000, n_inputs=256, n_taps=256)):
        with pytest.raises(nv.NvxError) as e:
            tp.Tap(**kw)
        assert e.value.code == ARG, kw


# ------------------------------------------------------------------------------------------------------------------ (g)
def _decode_on_the_device(nv, d_rows, pitch, n_out, n_streams, tune):
    """d_rows ([n_streams][pitch] words at 252 kS/s) through a raw_rate = 0 one-chain handle on its own stream, eight frames at
    a time: ({stream: bits}, the handle's messages)."""
    frames = n_out // nv.FRAME_IN
    with nv.Pipeline(n_streams=n_streams, chain_mask=nv.CHAIN_518, max_frames=8) as p:
        for s, hz in tune.items():
            p.set_carrier(s, 0, hz)
        for f0 in range(0, frames, 8):
            p.process_resident(d_rows, pitch, f0, min(8, frames - f0), hip_stream=p.hip_stream)
        p.fetch()
        return {s: p.bits(s, 0) for s in range(n_streams)}, list(p.messages)


@pytest.mark.parametrize("case", ["i", "iii"], ids=["two_stations_12k_iq", "audio_8k"])
def test_a_station_of_a_252k_row_to_a_message_on_the_device(nv, tp, case):
    """Cases (i) and (iii) of tests/test_tap.py on the device: nvx_tap -> nvx_nb (IQ or REAL kind) -> a tuned one-chain handle
    on its own stream.  The tap's samples are the restatement's, the message is the text, the bits are the tuned chain's
    restatement's on the interpolator's restatement of those samples.  The stations send a message of one short line: the row
    is a fifth of the CPU case's."""
    import narrow_ref as nr
    import navtex_amd.narrow as nb
    import tune_ref as tu
    cs = tc.E2E[case]
    fo, kind = cs["rate"], cs["kind"]
    L, M, T, h = tp.design(fo, kind)
    x = tc.row(nv, case, short=True)
    n_in = len(x)
    stations = list(cs["stations"].items())
    nt = len(stations)
    nkind = nr.IQ if kind == tr.IQ else nr.REAL
    L2, M2, T2, h2 = nb.design(fo, 1)
    d_in = nv.DeviceBuffer(n_in * 4)
    d_in.upload(x)
    with tp.Tap(fo, kind, n_inputs=1, n_taps=nt) as c, nb.Interpolator(fo, 1, kind=nkind, n_streams=nt) as up:
        ks = [tr.grid(fo, kind, hz) for _, hz in stations]
        for t, (_, hz) in enumerate(stations):
            assert c.set_shift(t, hz) == ks[t] * 252000 / 4096
        kps = [c.get_pitch(t)[0] for t in range(nt)] if kind == tr.REAL else None
        want = tr.tap_all(x, h, L, M, kind, ks, kps)[0]
        n_mid = len(want[0])
        n_out = nr.outputs_after(n_mid, L2, M2)
        d_mid = nv.DeviceBuffer(nt * n_mid * tp_bytes(kind)); d_out = nv.DeviceBuffer(nt * n_out * 4)
        assert c.resident(d_in, n_in, n_in, d_mid, n_mid) == n_mid
        assert up.resident(d_mid, n_mid, n_mid, d_out, n_out) == n_out
        mid = d_mid.download(nt * n_mid * tp_bytes(kind), dtype=np.int16).reshape((nt, n_mid, 2) if kind == tr.IQ else (nt, n_mid))
        _same(list(mid), want, "the tap's samples")
        tune = {t: tc.tuned_hz(case, hz, ks[t], kps[t] if kps else None) for t, (_, hz) in enumerate(stations)}
        bits, msgs = _decode_on_the_device(nv, d_out, n_out, n_out, nt, tune)
    d_in.free(); d_mid.free(); d_out.free()
    for t, (seed, _) in enumerate(stations):
        back = nr.interpolate_all(want[t], h2, L2, M2, nr.S16, nkind)[0]
        cut = back[:n_out // nv.FRAME_IN * nv.FRAME_IN]
        assert bits[t] == tu.decode(tu.chain(tu.front(cut, False), 0, tu.k_of(tune[t]))), t
        assert [m[3] for m in msgs if m[0] == t] == [tc.text(seed, short=True)], (t, msgs)


def test_tap_then_interpolate_then_scan_finds_the_station_at_the_residue(nv, tp):
    """nvx_tap -> nvx_nb -> nvx_scan_resident -> nvx_scan_find on the row of case (i): the strongest hit lies within 5 Hz of the
    shift's residue."""
    import navtex_amd.narrow as nb
    import navtex_amd.scan as sc
    x = tc.row(nv, "i", short=True)
    frames = 3
    n_mid = frames * 12000 * 8 // 25
    n_in = n_mid * 21
    hz = 14000.0
    d_in = nv.DeviceBuffer(n_in * 4); d_mid = nv.DeviceBuffer(n_mid * 4); d_out = nv.DeviceBuffer(frames * nv.FRAME_IN * 4)
    d_in.upload(x[:n_in])
    with tp.Tap(12000) as c, nb.Interpolator(12000) as up:
        residue = hz - c.set_shift(0, hz)
        assert c.resident(d_in, n_in, n_in, d_mid, n_mid) == n_mid
        assert up.resident(d_mid, n_mid, n_mid, d_out, frames * nv.FRAME_IN) == frames * nv.FRAME_IN
        row = sc.scan_resident(d_out, frames * nv.FRAME_IN, 0, frames, 1, False)[0]
    d_in.free(); d_mid.free(); d_out.free()
    hits = sc.find(row)
    strongest = max(hits, key=lambda h: h["band_power_db"])
    assert hits and abs(strongest["offset_hz"] - residue) <= 5.0 and abs(residue) <= 30.8, (residue, hits)
