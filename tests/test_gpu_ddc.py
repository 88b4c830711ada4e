"""The down-converter bank (include/navtex_amd_ddc.h) on the GPU (-m gpu): output words equal to the restatement
(tests/ddc_ref.py, run with the plan's own taps) for every format, at four rates, on signal, full-scale random input, the
rails, silence and float32 specials; chunked calls against one shot; k = 0 slices against the resampler library's own words;
every launch shape; positions beyond 2^32; a retune; 64 sibling slices; push against resident and the error paths (no
launch); and one wide input -> three slices -> scan / tune / decode on the device."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import ddc_cases as cases
import ddc_ref as dr
import resample_ref as rr
import signals
import tune_ref as tr

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FORMATS = (rr.CS16, rr.CU8, rr.CS8, rr.CF32)
FORMAT_IDS = ("cs16", "cu8", "cs8", "cf32")
SENTINEL = 0x5a5a1234
# rate -> the shifts of the three slices of case (a): none, a positive one, a negative one (at 96 kS/s: both ends of +-23 kHz)
SHIFTS = {2400000: (0, 1045, -683), 2048000: (0, 777, -1800), 250000: (0, 1638, -1637), 96000: (981, 0, -981)}


@pytest.fixture(scope="module")
def dd(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_ddc.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.ddc
    return navtex_amd.ddc


@pytest.fixture(scope="module")
def rs(dd):
    import navtex_amd.resample
    return navtex_amd.resample


def _random(fmt, n, rng):
    """Full-scale random samples; float32 with NaN, infinities, denormals and exact .5 ties among them."""
    if fmt != rr.CF32:
        info = np.iinfo(rr.DTYPES[fmt])
        return rng.integers(info.min, info.max + 1, size=(n, 2)).astype(rr.DTYPES[fmt])
    rnd = rng.uniform(-1.3, 1.3, size=(n, 2)).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 1e-42, -1e-42, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768,
                        32766.5 / 32768, 32767.5 / 32768, -32768.5 / 32768, 1.0, -1.0, 3e38, -3e38, 0.0, -0.0, 123.5 / 32768], dtype=np.float32)
    at = rng.integers(0, n, size=(400, 2))
    rnd[at[:, 0], at[:, 1] % 2] = special[rng.integers(0, len(special), size=400)]
    rnd[:len(special), 0] = special
    return rnd


def _two_inputs(nv, fi, fmt, n, seed):
    """Input 0: a signal, then the four rail combinations of (I, Q), a quarter of the rest each.  Input 1: full-scale random,
    then silence."""
    rng = np.random.default_rng(seed)
    dt = rr.DTYPES[fmt]
    half = n // 2
    bits = nv.sitor_encode(signals.stream_text(3), 8)
    sig = rr.to_format(rr.cpfsk(bits, fi, half, freq_hz=min(14000.0, fi / 8), seed=seed), fmt, gain=3.0 if fmt in (rr.CU8, rr.CS8) else 1.0)
    lo, hi = (np.float32(-1.0), np.float32(32767.0 / 32768.0)) if fmt == rr.CF32 else (np.iinfo(dt).min, np.iinfo(dt).max)
    rails = np.empty((n - half, 2), dtype=dt)
    quarter = (n - half + 3) // 4
    for c, (i, q) in enumerate(((hi, hi), (lo, lo), (hi, lo), (lo, hi))):
        rails[c * quarter:(c + 1) * quarter] = (i, q)
    silence = np.zeros((n - half, 2), dtype=dt) if fmt != rr.CU8 else np.full((n - half, 2), 128, dtype=dt)
    return [np.concatenate([sig.astype(dt), rails]), np.concatenate([_random(fmt, half, rng), silence])]


def _set_ks(d, ks, fi):
    for s, k in enumerate(ks):
        assert d.set_shift(s, k * fi / dr.N) == k * fi / dr.N
        assert all(d.get_shift(s, i) == (k, k * fi / dr.N) for i in range(d.n_inputs))


def _run(nv, d, rows, chunks, pitch_extra=0, out_first=0):
    """The inputs ([n, 2] each, all of one length) through nvx_ddc_resident in calls of `chunks` samples; every call's input
    is uploaded to the start of the input rows as whole rows: behind a call's n_in samples the row is full scale up to the
    pitch, so a read behind n_in changes the output.  The output rows lie between sentinels, which must survive.  Returns
    int16 [inputs, slices, n_out, 2]."""
    ni, ns, n = len(rows), d.n_slices, len(rows[0])
    assert sum(chunks) == n and ni == d.n_inputs
    bps = rows[0].dtype.itemsize * 2
    start, _ = d.position(0)
    total = rr.outputs_after(start + n, d.L, d.M) - rr.outputs_after(start, d.L, d.M)
    pitch_out = out_first + total + pitch_extra
    pitch_in = (max(max(chunks), 1) + 7) // 8 * 8 + 8 * pitch_extra
    d_in = nv.DeviceBuffer(ni * pitch_in * bps)
    d_out = nv.DeviceBuffer(ni * ns * pitch_out * 4)
    d_out.upload(np.full(ni * ns * pitch_out, SENTINEL, dtype=np.uint32))
    dt = rows[0].dtype
    block = np.empty((ni, pitch_in, 2), dtype=dt)
    pos = made = 0
    for c in chunks:
        block[:, c:] = 1.0 if dt == np.float32 else np.iinfo(dt).max
        for i in range(ni):
            block[i, :c] = rows[i][pos:pos + c]
        d_in.upload(block)
        got = d.resident(d_in, pitch_in, c, d_out, pitch_out, out_first + made)
        assert got == rr.outputs_after(start + pos + c, d.L, d.M) - rr.outputs_after(start + pos, d.L, d.M)
        pos, made = pos + c, made + got
    assert made == total and d.position(ni - 1) == (start + n, rr.outputs_after(start + n, d.L, d.M))
    words = d_out.download(ni * ns * pitch_out * 4, dtype=np.uint32).reshape(ni * ns, pitch_out)
    d_in.free(); d_out.free()
    assert np.all(words[:, :out_first] == SENTINEL) and np.all(words[:, out_first + total:] == SENTINEL), "words outside the span were written"
    return np.ascontiguousarray(words[:, out_first:out_first + total]).view(np.int16).reshape(ni, ns, total, 2)


def _same(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, int(np.argmax(np.any(got != want, axis=-1))))


def _check(got, rows, fmt, taps, L, M, ks, consumed=0):
    for i, row in enumerate(rows):
        x = rr.convert(row, fmt)
        for s, k in enumerate(ks):
            _same(got[i, s], dr.ddc(x, taps, L, M, k, consumed)[0], (i, s, k))


# ------------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("fi", sorted(SHIFTS, reverse=True))
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_output_equals_the_restatement(nv, dd, rs, fmt, fi):
    """2 inputs x 3 slices x 40 013 samples in one call: signal, rails, full-scale random and silence; a pitch larger than
    the data, out_first > 0, sentinels around every output row."""
    L, M, T, S, taps = rs.design(fi)
    n = 40013
    rows = _two_inputs(nv, fi, fmt, n, seed=fi % 1000 + fmt)
    ks = SHIFTS[fi]
    assert max(abs(k) for k in ks) <= dr.k_range(fi) and (fi != 96000 or ks[0] == dr.k_range(fi))
    with dd.Ddc(fi, fmt, n_inputs=2, n_slices=3) as d:
        assert (d.L, d.M, d.T) == (L, M, T) and d.get_shift(1, 1) == (0, 0.0)
        _set_ks(d, ks, fi)
        got = _run(nv, d, rows, [n], pitch_extra=3, out_first=7)
    _check(got, rows, fmt, taps, L, M, ks)
    assert got[1, 1].any()


# ------------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("fi,fmt", [(2400000, rr.CU8), (2048000, rr.CS16), (250000, rr.CF32), (96000, rr.CS8)])
def test_one_shot_equals_chunked_calls_and_inputs_reset_apart_meet_again(nv, dd, rs, fi, fmt):
    """Calls of 4097, 1, 0, T-2, T-1, 8 and 4095 samples leave the position off every multiple of 8 and of N and put
    history into the edge path; then input 1 is reset, pushed up to input 0's position alone, and both go on together."""
    L, M, T, S, taps = rs.design(fi)
    n = 30011
    rows = _two_inputs(nv, fi, fmt, n, seed=77)
    ks = SHIFTS[fi]
    chunks = [4097, 1, 0, T - 2, T - 1, 8, 4095]
    first = sum(chunks)
    with dd.Ddc(fi, fmt, n_inputs=2, n_slices=3) as d:
        _set_ks(d, ks, fi)
        got = _run(nv, d, [r[:first] for r in rows], chunks)
        made = rr.outputs_after(first, L, M)
        want = [[dr.ddc(rr.convert(r, fmt), taps, L, M, k)[0] for k in ks] for r in rows]
        for i in range(2):
            for s in range(3):
                _same(got[i, s], want[i][s][:made], (i, s))
        d.reset(1)
        assert d.position(0) == (first, made) and d.position(1) == (0, 0) and d.get_shift(2, 1)[0] == ks[2]      # the shift survives
        buf = nv.DeviceBuffer(1 << 20)
        k = C.c_size_t()
        assert dd.lib.nvx_ddc_resident(d._h, buf.ptr, 1024, 1024, buf.ptr + (1 << 19), 1024, 0, C.byref(k), None) == nv._native.ERR_STATE
        assert b"same position" in dd.lib.nvx_ddc_last_error()
        buf.free()
        # input 1 alone, in cuts of its own, up to the same position
        parts, pos = [], 0
        for c in (7, T - 1, first - T - 6):
            parts.append(d.push(1, rows[1][pos:pos + c])); pos += c
        again = np.concatenate(parts, axis=1)
        for s in range(3):
            _same(again[s], want[1][s][:made], ("pushed", s))
        assert d.position(1) == (first, made)
        got = _run(nv, d, [r[first:] for r in rows], [n - first])
        for i in range(2):
            for s in range(3):
                _same(got[i, s], want[i][s][made:], ("rest", i, s))


# ------------------------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("fi,fmt", [(2400000, rr.CU8), (2048000, rr.CS16), (250000, rr.CF32)])
def test_k0_slices_equal_the_resampler_librarys_words(nv, dd, rs, fi, fmt):
    n = 40000
    rows = _two_inputs(nv, fi, fmt, n, seed=11)
    bps = rows[0].dtype.itemsize * 2
    outs = rs.out_count(fi, 0, n)
    d_in = nv.DeviceBuffer(2 * n * bps); d_a = nv.DeviceBuffer(2 * outs * 4); d_b = nv.DeviceBuffer(4 * outs * 4)
    d_in.upload(np.stack(rows))
    with rs.Resampler(fi, fmt, n_streams=2) as r, dd.Ddc(fi, fmt, n_inputs=2, n_slices=2) as d:
        d.set_shift(1, 20 * fi / dr.N)
        assert r.resident(d_in, n, n, d_a, outs) == outs and d.resident(d_in, n, n, d_b, outs) == outs
        a = d_a.download(2 * outs * 4, dtype=np.uint32).reshape(2, outs)
        b = d_b.download(4 * outs * 4, dtype=np.uint32).reshape(2, 2, outs)
    for buf in (d_in, d_a, d_b):
        buf.free()
    assert np.array_equal(b[:, 0], a) and not np.array_equal(b[:, 1], a)


# ------------------------------------------------------------------------------------------------------------------- (d)
def test_few_rows_spread_their_tiles_over_workgroups(nv, dd, rs):
    """1 input x 3 slices at 2.048 MS/s: K = 4, tiles of 1024 outputs, a workgroup per tile; the LDS of two workgroups per CU."""
    fi, fmt = 2048000, rr.CS16
    L, M, T, S, taps = rs.design(fi)
    n = 30 * 1024 * M // L + 123
    rng = np.random.default_rng(5)
    rows = [_random(fmt, n, rng)]
    ks = (0, 1998, -3)
    with dd.Ddc(fi, fmt, n_inputs=1, n_slices=3) as d:
        _set_ks(d, ks, fi)
        got = _run(nv, d, rows, [n])
        shape = d.debug_last_launch()
    tiles = -(-rr.outputs_after(n, L, M) // (256 * 4))
    assert tiles == 31 and shape["K"] == 4 and shape["tiles"] == tiles and shape["chunks"] == tiles and shape["tiles_per_chunk"] == 1
    assert shape["taps_in_lds"] and shape["lds_bytes"] == 77536 and (shape["slices"], shape["inputs"]) == (3, 1) and shape["launches"] == 1
    _check(got, rows, fmt, taps, L, M, ks)


def test_the_few_inputs_form_with_several_tiles_per_workgroup_and_a_shorter_last_chunk(nv, dd, rs):
    """704 rows at 3.2 MS/s (K = 2, tiles of 512 outputs) leave three workgroups per row: five tiles go as 2 + 2 + 1."""
    fi, fmt = 3200000, rr.CU8
    L, M, T, S, taps = rs.design(fi)
    n = (4 * 512 + 50) * M // L                            # five tiles, the last one short
    rng = np.random.default_rng(6)
    rows = [_random(fmt, n, rng) for _ in range(44)]
    kmax = dr.k_range(fi)
    ks = tuple(int(k) for k in np.linspace(-kmax, kmax, 16).astype(int))
    ks = ks[:5] + (0,) + ks[6:]
    with dd.Ddc(fi, fmt, n_inputs=44, n_slices=16) as d:
        _set_ks(d, ks, fi)
        got = _run(nv, d, rows, [n])
        shape = d.debug_last_launch()
    assert shape["K"] == 2 and shape["tiles"] == 5 and shape["tiles_per_chunk"] == 2 and shape["chunks"] == 3
    assert (shape["slices"], shape["inputs"]) == (16, 44)
    _check(got, rows, fmt, taps, L, M, ks)


def test_the_many_inputs_form_walks_several_tiles_per_workgroup(nv, dd, rs):
    """1024 rows at 250 kS/s (K = 16): one workgroup per row walks its three tiles."""
    fi, fmt = 250000, rr.CS16
    L, M, T, S, taps = rs.design(fi)
    n = (2 * 4096 + 1000) * M // L + 5
    rng = np.random.default_rng(7)
    rows = [_random(fmt, n, rng) for _ in range(64)]
    kmax = dr.k_range(fi)
    ks = tuple(int(k) for k in np.linspace(-kmax, kmax, 16).astype(int))
    with dd.Ddc(fi, fmt, n_inputs=64, n_slices=16) as d:
        _set_ks(d, ks, fi)
        got = _run(nv, d, rows, [n], pitch_extra=1, out_first=3)
        shape = d.debug_last_launch()
    assert shape["K"] == 16 and shape["tiles"] == 3 and shape["tiles_per_chunk"] == 3 and shape["chunks"] == 1
    assert (shape["slices"], shape["inputs"]) == (16, 64)
    _check(got, rows, fmt, taps, L, M, ks)


@pytest.mark.parametrize("fi,fmt,want_k,in_lds", [(252250, rr.CS16, None, False), (3200000, rr.CF32, 2, True), (3200000, rr.CU8, 2, True)])
def test_taps_in_global_memory_and_two_outputs_per_thread(nv, dd, rs, fi, fmt, want_k, in_lds):
    """252 250 S/s has L = 1008: the tap table does not fit the LDS and is read from global memory.  At 3.2 MS/s a tile's
    input span allows K = 2 only."""
    L, M, T, S, taps = rs.design(fi)
    n = 30011
    rows = _two_inputs(nv, fi, fmt, n, seed=13)
    kmax = dr.k_range(fi)
    ks = (kmax, 0, -kmax // 3)
    with dd.Ddc(fi, fmt, n_inputs=2, n_slices=3) as d:
        _set_ks(d, ks, fi)
        got = _run(nv, d, rows, [n - 4000, 4000], pitch_extra=2, out_first=1)
        shape = d.debug_last_launch()
    assert shape["taps_in_lds"] == in_lds and (want_k is None or shape["K"] == want_k) and shape["launches"] == 2
    assert (L == 1008) == (not in_lds) and shape["lds_bytes"] == (8704 + 2112) * 4 + ((4 * L * _row_dw(T) + 3) // 4 * 4 * 4 if in_lds else 0)
    _check(got, rows, fmt, taps, L, M, ks)


def _row_dw(T):
    tp = (T + 6) // 4 * 4
    return tp // 2 + (2 if tp // 4 % 2 == 0 else 0)


# ------------------------------------------------------------------------------------------------------------------- (e)
@pytest.mark.parametrize("position", [2 ** 32 - 1000, 2 ** 40 + 5])
@pytest.mark.parametrize("fi,fmt", [(2400000, rr.CU8), (250000, rr.CS16)])
def test_positions_beyond_32_bits(nv, dd, rs, fi, fmt, position):
    L, M, T, S, taps = rs.design(fi)
    n = 20011
    rows = _two_inputs(nv, fi, fmt, n, seed=21)
    ks = SHIFTS[fi]
    with dd.Ddc(fi, fmt, n_inputs=2, n_slices=3) as d:
        _set_ks(d, ks, fi)
        d.debug_set_position(position)
        assert d.position(1) == (position, rr.outputs_after(position, L, M))
        got = _run(nv, d, rows, [n - 5000, 5000])
    _check(got, rows, fmt, taps, L, M, ks, consumed=position)


# ------------------------------------------------------------------------------------------------------------------- (f)
def test_a_retune_applies_the_new_shift_to_the_carried_unmixed_history(nv, dd, rs):
    fi, fmt = 2400000, rr.CS16
    L, M, T, S, taps = rs.design(fi)
    n1, n2 = 10003, 9000
    rng = np.random.default_rng(31)
    rows = [_random(fmt, n1 + n2, rng)]
    before, after = (100, 0, -700), (-55, 300, 0)
    with dd.Ddc(fi, fmt, n_inputs=1, n_slices=3) as d:
        _set_ks(d, before, fi)
        a = _run(nv, d, [rows[0][:n1]], [n1])
        _set_ks(d, after, fi)
        b = _run(nv, d, [rows[0][n1:]], [n2])
    x = rr.convert(rows[0], fmt)
    for s in range(3):
        wa, hist = dr.ddc(x[:n1], taps, L, M, before[s])
        wb, _ = dr.ddc(x[n1:], taps, L, M, after[s], n1, hist)
        _same(a[0, s], wa, ("before", s)); _same(b[0, s], wb, ("after", s))
        assert not np.array_equal(wb, dr.ddc(x, taps, L, M, before[s])[0][len(wa):])


# ------------------------------------------------------------------------------------------------------------------- (g)
@pytest.mark.parametrize("fi,fmt", [(2400000, rr.CU8), (2048000, rr.CS16)])
def test_sixty_four_sibling_slices_of_one_input(nv, dd, rs, fi, fmt):
    L, M, T, S, taps = rs.design(fi)
    n = 40013
    rows = [_two_inputs(nv, fi, fmt, n, seed=41)[1]]
    kmax = dr.k_range(fi)
    ks = tuple(i * kmax // 32 for i in range(-32, 32))
    assert ks[0] == -kmax and ks[32] == 0 and len(set(ks)) == 64
    with dd.Ddc(fi, fmt, n_inputs=1, n_slices=64) as d:
        _set_ks(d, ks, fi)
        got = _run(nv, d, rows, [n], out_first=5)
    _check(got, rows, fmt, taps, L, M, ks)


# ------------------------------------------------------------------------------------------------------------------- (h)
def test_push_equals_resident_and_refusals_launch_nothing(nv, dd, rs):
    ARG = nv._native.ERR_ARG
    fi, fmt, n = 2400000, rr.CU8, 8192
    L, M, T, S, taps = rs.design(fi)
    rows = _two_inputs(nv, fi, fmt, n, seed=51)
    ks = (0, 900, -1200)
    with dd.Ddc(fi, fmt, n_inputs=2, n_slices=3) as d:
        _set_ks(d, ks, fi)
        pushed = [d.push(i, rows[i]) for i in range(2)]
        d.reset()
        got = _run(nv, d, rows, [n])
        for i in range(2):
            assert pushed[i].dtype == np.int16
            _same(pushed[i], got[i], ("push", i))
        _check(got, rows, fmt, taps, L, M, ks)
        launches = d.debug_last_launch()["launches"]
        assert launches == 3
        d.reset()
        d.timing(True); d.time_stats(reset=True)
        # shifts outside the range, slices and inputs that do not exist
        applied = C.c_double(-1.0)
        for args in ((0, 0, 1175500.0), (0, 0, -1175500.0), (-1, 1, float("nan")), (0, 3, 0.0), (2, 0, 0.0), (-2, 0, 0.0), (0, -1, 0.0)):
            assert dd.lib.nvx_ddc_set_shift(d._h, *args, C.byref(applied)) == ARG and dd.lib.nvx_ddc_last_error() != b"", args
        assert applied.value == -1.0 and [d.get_shift(s)[0] for s in range(3)] == list(ks)
        outs = rr.outputs_after(n, L, M)
        d_in = nv.DeviceBuffer(2 * n * 2); d_out = nv.DeviceBuffer(6 * outs * 4)
        one_in = nv.DeviceBuffer(n * 2); five_out = nv.DeviceBuffer(5 * outs * 4)
        k = C.c_size_t(99)
        call = lambda *a: dd.lib.nvx_ddc_resident(d._h, *a, C.byref(k), None)            # noqa: E731
        bad = {"more samples than the pitch": (d_in.ptr, n - 8, n, d_out.ptr, outs, 0),
               "outputs beyond the pitch": (d_in.ptr, n, n, d_out.ptr, outs - 1, 0),
               "out_first pushes them beyond it": (d_in.ptr, n, n, d_out.ptr, outs, 1),
               "input rows for one input": (one_in.ptr, n, n, d_out.ptr, outs, 0),
               "output rows for five of six": (d_in.ptr, n, n, five_out.ptr, outs, 0),
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
            assert dd.lib.nvx_ddc_last_error() != b""
        assert k.value == 99 and d.time_stats() == (0.0, 0) and d.position(0) == (0, 0) and d.position(1) == (0, 0)
        # inputs at different positions
        d.push(1, rows[1][:100])
        after_push = d.debug_last_launch()["launches"]
        assert after_push == launches + 1 and call(d_in.ptr, n, n, d_out.ptr, outs, 0) == nv._native.ERR_STATE
        # a push whose rows are too small: nothing consumed
        small = np.empty((3, 3, 2), dtype=np.int16)
        a = np.ascontiguousarray(rows[0][:4000])
        assert dd.lib.nvx_ddc_push(d._h, 0, a.ctypes.data_as(C.c_void_p), 4000, small.ctypes.data_as(C.c_void_p), 3, C.byref(k)) == ARG
        assert d.position(0) == (0, 0) and d.debug_last_launch()["launches"] == after_push and d.time_stats()[1] == 1
        d.reset()
        assert call(d_in.ptr, n, 0, d_out.ptr, outs, 0) == 0 and k.value == 0 and d.debug_last_launch()["launches"] == after_push      # nothing to do
        assert call(d_in.ptr, n, n, d_out.ptr, outs, 0) == 0 and k.value == outs
        ms, timed = d.time_stats()
        assert timed == 2 and ms > 0.0 and d.debug_last_launch()["launches"] == after_push + 1
        for b in (d_in, d_out, one_in, five_out):
            b.free()
    for bad_cfg in (dict(device=99), dict(n_inputs=256, n_slices=256)):
        with pytest.raises(nv.NvxError) as e:
            dd.Ddc(fi, fmt, **bad_cfg)
        assert e.value.code == ARG
    with pytest.raises(nv.NvxError) as e:
        dd.Ddc(3200001)
    assert e.value.code == ARG


# ------------------------------------------------------------------------------------------------------------------- (i)
def test_one_wide_input_three_stations_on_the_device(nv, dd, oracle):
    """The end-to-end case of tests/ddc_cases.py on the device: the bank's rows equal the restatement's; the rows go through
    nvx_process_resident of a three-stream raw_rate = 0 handle; slice 0 is tuned to +14 kHz plus the reported residue, slice
    1 stays nominal, slice 2 goes through nvx_scan_resident -> nvx_scan_find -> nvx_set_carrier.  Three messages, and bits
    equal to the restated chains' on the restatement's rows."""
    import navtex_amd.scan as sc
    fi = cases.RATE
    (src, frames), (want, ks, residues) = cases.source(), cases.slices()
    texts = [t for _, _, t in cases.STATIONS]
    n, outs = len(src), frames * nv.FRAME_IN
    d_in = nv.DeviceBuffer(n * 2); d_out = nv.DeviceBuffer(3 * outs * 4)
    d_in.upload(src)
    with dd.Ddc(fi, dd.CU8, n_inputs=1, n_slices=3) as d, nv.Pipeline(n_streams=3, chain_mask=nv.CHAIN_518, max_frames=8) as p:
        hs = p.hip_stream
        for s, (_, hz, _) in enumerate(cases.STATIONS):
            assert hz - d.set_shift(s, hz) == residues[s] and d.get_shift(s)[0] == ks[s]
        assert d.resident(d_in, n, n, d_out, outs, hip_stream=hs) == outs
        nv.lib.nvx_device_sync(0)
        words = d_out.download(3 * outs * 4, dtype=np.int16).reshape(3, outs, 2)
        assert np.array_equal(words, want)
        # slice 2: where is the carrier?
        row = sc.scan_resident(_At(d_out.ptr + 2 * outs * 4), outs, 0, 3, 1, False)[0]
        hits = sc.find(row)
        assert hits and abs(hits[0]["offset_hz"] - (-14000 + residues[2])) <= 5.0, (hits[:2], residues[2])
        applied = [p.set_carrier(0, 0, 14000 + residues[0]), 14000.0, p.set_carrier(2, 0, hits[0]["offset_hz"])]
        f0 = 0
        while f0 < frames:
            k = min(8, frames - f0)
            p.process_resident(d_out, outs, f0, k, hip_stream=hs)
            f0 += k
        p.fetch()
        got_bits = [p.bits(s, 0) for s in range(3)]
        got_msgs = sorted((m[0], m[3]) for m in p.messages)
    d_in.free(); d_out.free()
    assert got_msgs == [(s, texts[s]) for s in range(3)], got_msgs
    for s in range(3):
        y1 = tr.front(want[s], False)
        assert got_bits[s] == tr.decode(tr.chain(y1, 0, tr.k_of(applied[s]))), s
    ref = oracle.Pipe(chain_mask=1)
    ref.push(want[1])
    assert got_bits[1] == ref.bits(0)


class _At:
    """A device address where a DeviceBuffer is expected."""
    def __init__(self, ptr, device=0):
        self.ptr, self.device = ptr, device
