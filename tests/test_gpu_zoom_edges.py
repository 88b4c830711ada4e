"""The zoom bank's edges on the GPU (-m gpu): an input spread over chunks (each chunk fills its stages' lines from the input in
front of it) behind a first call of D samples, 1024 inputs at one chunk each, positions beyond 2^32 and 2^40, retunes between
calls (the history is re-mixed; a reset leaves the shift), and every refusal with the launch counter unchanged.  Every
comparison against the restatement (tests/zoom_ref.py) is ==, with sentinels around every output row."""
import ctypes as C

import numpy as np
import pytest

import zoom_cases as zc
import zoom_ref as zr
from test_gpu_zoom import set_shifts, shifts, zl  # noqa: F401
from zoom_cases import _run_resident, _same

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("k", (1, 4))
def test_a_row_spread_over_chunks_behind_a_first_call_of_d_samples(nv, zl, k):
    """One input x (12 T + 5) outputs behind a call of D samples: thirteen tiles are two chunks of eight and five (a chunk has
    at least eight times its warm-up), and the second fills its lines from the first's samples."""
    D, T = 1 << k, zl.tile(k)
    n = D * (12 * T + 5)
    row = zc.signal(zr.CS16, D + n, 700 + k)
    kzs = [[-321, 0, 2047]]
    want = zr.zoom_all(row, k, kzs[0])[0]
    with zl.Zoom(k, zr.CS16, n_zooms=3) as z:
        set_shifts(z, kzs)
        first = _run_resident(nv, z, [row[:D]], [D])
        last = z.debug_last_launch()
        assert (last["launches"], last["chunks"], last["tiles_per_chunk"], last["warm_tiles"], last["form"]) == (1, 1, 1, 1, 1)
        got = _run_resident(nv, z, [row[D:]], [n], out_first=3)
        last = z.debug_last_launch()
        assert (last["launches"], last["chunks"], last["tiles_per_chunk"], last["warm_tiles"], last["form"]) == (2, 2, 8, 1, 2)
        assert last["lds_bytes"] == 20480 + 3 * 2 * (128 * k + 4 * (1024 - (1024 >> k)))
        _same(np.concatenate([first, got], axis=1), [want], ("chunks", k))


def test_a_thousand_inputs_of_two_zooms_at_one_chunk_each(nv, zl):
    """1024 inputs x 2 zooms x (T + 10) outputs of CU8 at k = 3: a workgroup per input."""
    k, ni = 3, 1024
    D, T = 1 << k, zl.tile(k)
    n = D * (T + 10)
    base = zc.signal(zr.CU8, n + ni, 800)
    rows = [base[i:i + n] for i in range(ni)]               # every input its own window of one row
    kzs = [[(37 * i) % 4096 - 2048, (i % 7) * 100] for i in range(ni)]
    with zl.Zoom(k, zr.CU8, n_inputs=ni, n_zooms=2) as z:
        set_shifts(z, kzs)
        got = _run_resident(nv, z, rows, [n], out_first=1)
        last = z.debug_last_launch()
        assert (last["chunks"], last["form"]) == (1, 1)
    for i in (0, 1, 511, 1023):
        want = zr.zoom_all(rows[i], k, kzs[i], zr.CU8)[0]
        assert np.array_equal(got[2 * i:2 * i + 2], want), i
    # the rows between: each differs from its neighbour's (a workgroup that took another input's row or shifts would not)
    assert all(not np.array_equal(got[2 * i], got[2 * i + 2]) for i in range(ni - 1))


def test_eight_zooms_at_k_6_take_the_largest_lds_and_a_thread_for_each_of_192_planes(nv, zl):
    """The largest plan: 97 280 bytes of LDS a workgroup, beyond the 64 KB a launch gets unasked; 2 inputs x (5 T + 3) outputs."""
    k, nz = 6, 8
    D, T = 1 << k, zl.tile(k)
    n = D * (5 * T + 3)
    rows = [zc.signal(zr.CS8, n, 850 + s) for s in range(2)]
    kzs = shifts(2, nz)
    with zl.Zoom(k, zr.CS8, n_inputs=2, n_zooms=nz) as z:
        set_shifts(z, kzs)
        got = _run_resident(nv, z, rows, [n], out_first=4)
        assert z.debug_last_launch()["lds_bytes"] == 97280
    _same(got, [zr.zoom_all(row, k, kzs[i], zr.CS8)[0] for i, row in enumerate(rows)], "eight zooms")


# ------------------------------------------------------------------------------------------------------------------ (e)
@pytest.mark.parametrize("k,position", ((3, (1 << 32) - 1000 * 8), (6, (1 << 40) + 6 * 64)))
def test_positions_beyond_two_to_the_32_and_40(nv, zl, k, position):
    """debug_set_position, then two calls: silence counts in front, and the phase comes from the position mod 4096."""
    D, T = 1 << k, zl.tile(k)
    n = D * (2 * T + 3)
    row = zc.signal(zr.CS16, n, 900 + k)
    kzs = [[1001, -3]]
    ref = zr.Zoom(k, kzs[0], position=position)
    want = ref.push(row)
    assert not np.array_equal(want, zr.zoom_all(row, k, kzs[0])[0])      # the position tells
    with zl.Zoom(k, zr.CS16, n_zooms=2) as z:
        set_shifts(z, kzs)
        z.debug_set_position(position)
        assert z.position(0) == (position, position // D)
        got = _run_resident(nv, z, [row], [D * T + D, n - D * T - D])
        _same(got, [want], ("position", k))
        assert z.position(0) == (position + n, (position + n) // D)
        with pytest.raises(zl.ZoomError):
            z.debug_set_position(position + 1)


# ------------------------------------------------------------------------------------------------------------------ (f)
@pytest.mark.parametrize("k", (2, 6))
def test_a_retune_applies_from_the_next_call_on_history_included_and_a_reset_leaves_the_shift(nv, zl, k):
    D, T = 1 << k, zl.tile(k)
    cuts = [D * (T + 2), D * (T + 1), D * 5]
    rows = [zc.signal(zr.CS16, sum(cuts), 1000 + s) for s in range(2)]
    kzs = [[100, -200], [300, 0]]
    refs = [zr.Zoom(k, kzs[i]) for i in range(2)]
    with zl.Zoom(k, zr.CS16, n_inputs=2, n_zooms=2) as z:
        set_shifts(z, kzs)
        pos = 0
        for call, cut in enumerate(cuts):
            if call == 1:                                    # one zoom of one input
                z.set_step(1, 555, input=1); refs[1].set_shift(1, 555)
            if call == 2:                                    # a zoom of every input
                z.set_step(0, -2048); refs[0].set_shift(0, -2048); refs[1].set_shift(0, -2048)
            want = [r.push(row[pos:pos + cut]) for r, row in zip(refs, rows)]
            got = _run_resident(nv, z, [row[pos:pos + cut] for row in rows], [cut])
            _same(got, want, ("retune", k, call))
            pos += cut
        assert [z.get_step(s, input=i) for i in range(2) for s in range(2)] == [-2048, -200, -2048, 555]
        # as if the zoom had always had it: the call behind a retune equals that part of a one-shot run with the new shifts
        always = zr.zoom_all(rows[0], k, (-2048, -200))[0]
        assert np.array_equal(got[:2], always[:, -cuts[2] // D:])
        z.reset()
        assert z.get_step(1, input=1) == 555 and z.position(1) == (0, 0)
        got = _run_resident(nv, z, [row[:cuts[0]] for row in rows], [cuts[0]])
        _same(got, [zr.zoom_all(rows[0][:cuts[0]], k, (-2048, -200))[0], zr.zoom_all(rows[1][:cuts[0]], k, (-2048, 555))[0]], ("reset", k))


# ------------------------------------------------------------------------------------------------------------------ (g)
def test_every_refusal_returns_its_code_and_launches_nothing(nv, zl):
    ARG, STATE = nv._native.ERR_ARG, nv._native.ERR_STATE
    k, D = 3, 8
    for kw in (dict(log2_decim=0), dict(log2_decim=7), dict(log2_decim=3, n_zooms=0), dict(log2_decim=3, n_zooms=9),
               dict(log2_decim=3, n_inputs=0), dict(log2_decim=3, n_inputs=8192, n_zooms=8), dict(log2_decim=3, format=4), dict(log2_decim=3, format=-1)):
        with pytest.raises(nv.NvxError) as e:
            zl.Zoom(**kw)
        assert e.value.code == ARG, kw
    n = 64 * D
    with zl.Zoom(k, zr.CS16, n_inputs=2, n_zooms=2) as z:
        d_in = nv.DeviceBuffer(2 * n * 4); d_out = nv.DeviceBuffer(4 * (n // D) * 4)
        d_in.upload(np.zeros(2 * n * 2, dtype=np.int16))
        res = lambda *a: zl.lib.nvx_zoom_resident(z._h, *a)  # noqa: E731
        assert res(d_in.ptr, n, n, d_out.ptr, n // D, 0, None, None) == 0
        launches = z.debug_last_launch()["launches"]
        assert launches == 1
        # spans that leave their allocation: the input's second row, the output's last row, a first word too far
        assert res(d_in.ptr, n + 16, n, d_out.ptr, n // D, 0, None, None) == ARG and b"input" in zl.lib.nvx_zoom_last_error()
        assert res(d_in.ptr, n, n, d_out.ptr, n // D + 4, 0, None, None) == ARG and b"output" in zl.lib.nvx_zoom_last_error()
        assert res(d_in.ptr, n, n - D, d_out.ptr, n // D, 2, None, None) == ARG
        assert res(d_in.ptr, n, n, d_out.ptr, 1 << 62, 0, None, None) == ARG and b"overflows" in zl.lib.nvx_zoom_last_error()
        # no multiple of D; no pointer; an input row that is not 16-byte aligned
        assert res(d_in.ptr, n, n - 1, d_out.ptr, n // D, 0, None, None) == ARG and b"multiple" in zl.lib.nvx_zoom_last_error()
        assert res(None, n, n, d_out.ptr, n // D, 0, None, None) == ARG and res(d_in.ptr + 4, n, n - D, d_out.ptr, n // D, 0, None, None) == ARG
        assert res(d_in.ptr, n - 1, n - D, d_out.ptr, n // D, 0, None, None) == ARG
        # shifts outside the range, zooms and inputs that are not there
        for args in ((0, 0, 2048), (0, 0, -2049), (0, 2, 0), (2, 0, 0), (-2, 0, 0), (0, -1, 0)):
            assert zl.lib.nvx_zoom_set_shift(z._h, *args) == ARG, args
        assert zl.lib.nvx_zoom_get_shift(z._h, -1, 0, None) == ARG
        # inputs at different positions
        z.reset(1)
        assert res(d_in.ptr, n, n, d_out.ptr, n // D, 0, None, None) == STATE
        assert z.debug_last_launch()["launches"] == launches
        # n_in = 0 is valid and launches nothing
        z.reset()
        nout = C.c_size_t(7)
        assert res(d_in.ptr, n, 0, d_out.ptr, n // D, 0, C.byref(nout), None) == 0 and nout.value == 0
        assert z.debug_last_launch()["launches"] == launches
        d_in.free(); d_out.free()
    for hz, rate in ((2e5, 3e5), (float("nan"), 1e6), (float("inf"), 1e6), (1.0, 0.0), (1.0, float("nan"))):
        with pytest.raises(zl.ZoomError) as e:
            zl.grid(rate, hz)
        assert e.value.code == ARG
