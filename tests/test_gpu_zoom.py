"""The zoom bank (include/navtex_amd_zoom.h) on the GPU (-m gpu): output words equal to the restatement (tests/zoom_ref.py)
in every format at k = 1 and k = 6 with one zoom and three, calls cut anywhere against one shot with a history shorter than,
equal to and longer than a call, a reset input rejoining the others, push against resident with the samples a push holds
back, the rails of the mixer and of a stage and full-scale random input (float32 specials), and the acceptance case's seed 11
through a raw_rate = 0 handle with the label 4209.  Every comparison is ==, with sentinels around every output row."""
from pathlib import Path

import numpy as np
import pytest

import zoom_cases as zc
import zoom_ref as zr
from zoom_cases import _first_difference, _run_resident, _same

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FORMATS = (zr.CS16, zr.CU8, zr.CS8, zr.CF32)
FORMAT_IDS = ("cs16", "cu8", "cs8", "cf32")


@pytest.fixture(scope="module")
def zl(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_zoom.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.zoom
    assert navtex_amd.zoom.BLOCK == 1024 and [navtex_amd.zoom.tile(k) for k in (1, 6)] == [512, 16]
    return navtex_amd.zoom


def shifts(ni: int, nz: int):
    """All different, input 0's first zoom at kz = 0 and its second negative where there is one."""
    order = (0, -500, 37, 2047, -2048, 512, 1, -1)
    return [[(order[(i * nz + z) % 8] + (i * nz + z) // 8 * 3 + 2048) % 4096 - 2048 for z in range(nz)] for i in range(ni)]


def set_shifts(z, kzs):
    for i, row in enumerate(kzs):
        for s, kz in enumerate(row):
            z.set_step(s, kz, input=i)
            assert z.get_step(s, input=i) == kz


# ------------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("nz", (1, 3))
@pytest.mark.parametrize("k", (1, 6))
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_two_inputs_of_three_tiles_and_five_in_every_format(nv, zl, fmt, k, nz):
    """2 inputs x (3 T + 5) outputs.  A pitch larger than the data; out_first = 7 (the unaligned stores) and 8."""
    D, T = 1 << k, zl.tile(k)
    n = D * (3 * T + 5)
    rows = [zc.signal(fmt, n, 200 + 10 * fmt + s) for s in range(2)]
    kzs = shifts(2, nz)
    want = [zr.zoom_all(row, k, kzs[i], fmt)[0] for i, row in enumerate(rows)]
    for out_first in (7, 8):
        with zl.Zoom(k, fmt, n_inputs=2, n_zooms=nz) as z:
            set_shifts(z, kzs)
            got = _run_resident(nv, z, rows, [n], pitch_extra=3 + out_first % 2, out_first=out_first)
            _same(got, want, (fmt, k, nz, out_first))


# ------------------------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("k", (1, 6))
def test_one_shot_equals_calls_shorter_and_longer_than_the_history_and_a_reset_input_rejoins(nv, zl, k):
    """Calls of D, H - D, H, H + D, 0 and 2 T D + D samples and the rest (H is rounded down to a multiple of D: a call is
    one)."""
    D, T, H = 1 << k, zl.tile(k), zr.history(k) // (1 << k) * (1 << k)
    cuts = [D, H - D, H, H + D, 0, 2 * T * D + D]
    cuts = [c for c in cuts if c >= 0]
    n1 = sum(cuts) + D * (T + 7)
    cuts = cuts + [n1 - sum(cuts)]
    tail = D * (T + 3)
    rows = [zc.signal(zr.CS16, n1 + tail, 400 + s) for s in range(3)]
    kzs = shifts(3, 2)
    want = [zr.zoom_all(row, k, kzs[i])[0] for i, row in enumerate(rows)]
    with zl.Zoom(k, zr.CS16, n_inputs=3, n_zooms=2) as z:
        set_shifts(z, kzs)
        got = _run_resident(nv, z, [row[:n1] for row in rows], cuts)
        _same(got, [w[:, :n1 // D] for w in want], ("cuts", k))
        z.reset(1)
        assert z.position(1) == (0, 0) and z.position(0) == (n1, n1 // D) and z.get_step(1, input=1) == kzs[1][1]
        d = nv.DeviceBuffer(3 * 64 * 4); o = nv.DeviceBuffer(6 * 64 * 4)
        launches = z.debug_last_launch()["launches"]
        assert zl.lib.nvx_zoom_resident(z._h, d.ptr, 64, 64, o.ptr, 64, 0, None, None) == nv._native.ERR_STATE
        assert b"same position" in zl.lib.nvx_zoom_last_error() and z.debug_last_launch()["launches"] == launches
        d.free(); o.free()
        # input 1 starts anew on other data, alone and in pushes of its own, up to where the others stand
        fresh = zr.Zoom(k, kzs[1])
        other = zc.signal(zr.CS16, n1 + tail, 450)
        pos = 0
        for cut in (5 * D, D, T * D + 3 * D, n1 - T * D - 9 * D):
            assert np.array_equal(z.push(1, other[pos:pos + cut]), fresh.push(other[pos:pos + cut])), pos
            pos += cut
        assert z.position(1) == (n1, n1 // D)
        got = _run_resident(nv, z, [rows[0][n1:], other[n1:], rows[2][n1:]], [tail])
        _same(got, [want[0][:, n1 // D:], fresh.push(other[n1:]), want[2][:, n1 // D:]], ("rejoined", k))


@pytest.mark.parametrize("k", (1, 6))
@pytest.mark.parametrize("fmt", (zr.CS16, zr.CU8, zr.CF32), ids=("cs16", "cu8", "cf32"))
def test_pushes_of_any_length_equal_the_resident_calls_words_and_position_counts_the_held_samples(nv, zl, fmt, k):
    """Pushes of 1, D - 1, D + 1 and 3 D + 2 samples, nothing, a tile and a half and the rest; a resident call is refused while
    samples are held."""
    D, T = 1 << k, zl.tile(k)
    n = D * (2 * T + 9)
    row = zc.signal(fmt, n, 500 + fmt)
    kzs = [[-777, 0, 1234]]
    with zl.Zoom(k, fmt, n_zooms=3) as z:
        set_shifts(z, kzs)
        resident = _run_resident(nv, z, [row], [n])
    with zl.Zoom(k, fmt, n_zooms=3) as z:
        set_shifts(z, kzs)
        parts, pos = [], 0
        for cut in (1, D - 1, D + 1, 3 * D + 2, 0, T * D + T * D // 2 + 1, n):
            cut = min(cut, n - pos)
            parts.append(z.push(0, row[pos:pos + cut]))
            pos += cut
            assert z.position(0) == (pos, pos // D) and parts[-1].shape[1] == pos // D - (pos - cut) // D
            if pos % D:
                d = nv.DeviceBuffer(64 * 8); o = nv.DeviceBuffer(3 * 64 * 4)
                assert zl.lib.nvx_zoom_resident(z._h, d.ptr, 64, 64, o.ptr, 64, 0, None, None) == nv._native.ERR_STATE
                assert b"holds" in zl.lib.nvx_zoom_last_error()
                d.free(); o.free()
        got = np.concatenate(parts, axis=1)
    assert pos == n and np.array_equal(got, resident)
    assert np.array_equal(got, zr.zoom_all(row, k, kzs[0], fmt)[0])


# ------------------------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("k", (1, 3))
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_the_rails_of_the_mixer_and_of_a_stage_and_full_scale_rows(nv, zl, fmt, k):
    """Every component at its lowest value under kz = 512 (the mixer's sum reaches +-46340 and clamps); bursts with the taps'
    signs at kz = 0 (stage 1's sum reaches the largest and the smallest value the format allows, and its output clamps);
    full-scale random rows, float32 with the CF32 rule's specials."""
    D, T = 1 << k, zl.tile(k)
    n = D * (2 * T + 5)
    rows = [zc.rails_low(fmt, n), zc.rails_taps(fmt, n), zc.full_scale(fmt, n, 600 + fmt)]
    kzs = [[512, 0], [0, 512], [-1000, 0]]
    refs = [zr.zoom_all(row, k, kzs[i], fmt) for i, row in enumerate(rows)]
    # the rails are reached: the mixer's clamp, and the stage's both ways
    x = zr.rr.convert(rows[0][:8], fmt)
    mixed = zr.dr.mix(x, 512, 0)
    assert 32767 in mixed or -32768 in mixed
    lo, hi = zr.zoom_all(rows[1], k, (0,), fmt)[1].acc
    full = zr.rr.convert(np.array([[zc.highest(fmt), zc.lowest(fmt)]], dtype=zr.DTYPES[fmt]), fmt)[0]
    h = zr.lowpass()
    assert hi == int(h[h > 0].sum() * full[0] + h[h < 0].sum() * full[1]) and lo == int(h[h > 0].sum() * full[1] + h[h < 0].sum() * full[0])
    assert (hi + (1 << 14)) >> 15 > 32767 and (lo + (1 << 14)) >> 15 < -32768
    with zl.Zoom(k, fmt, n_inputs=3, n_zooms=2) as z:
        set_shifts(z, kzs)
        got = _run_resident(nv, z, rows, [n])
        _same(got, [r[0] for r in refs], ("rails", fmt, k))


# ------------------------------------------------------------------------------------------------------------------ (h)
def test_seed_11_of_the_acceptance_case_on_the_device(nv, zl, oracle):
    """The wide row of seed 11 through both zooms on the device: the words are the CPU's.  Then zoom A's row, zoom B's and the
    naive row as three streams of a raw_rate = 0 handle with the labels [[518, 490], [4209, 0], [518, 490]]: all three messages
    arrive from the zoomed rows, the 490 message does not arrive from the naive one, and every chain's bits are the oracle's on
    the same words."""
    t518, t490, _, t4209 = zc.texts()
    (ka, _), (kb, _) = zc.centres()
    x = zc.wide_row(nv, 11)
    n = len(x) >> zc.K
    want, _ = zr.zoom_all(x, zc.K, (ka, kb))
    naive = zr.naive(x, zc.K, ka)
    d_wide = nv.DeviceBuffer(len(x) * 4)
    d_in = nv.DeviceBuffer(3 * n * 4)                       # the handle's input: rows 0 and 1 zoomed, row 2 naive
    d_wide.upload(x)
    d_in.upload(naive, 2 * n * 4)
    with zl.Zoom(zc.K, zr.CS16, n_zooms=2) as z:
        assert z.set_shift(0, zc.HZ_A, zc.RATE) == zc.centres()[0][1] and z.set_shift(1, zc.HZ_B, zc.RATE) == zc.centres()[1][1]
        assert z.resident(d_wide, len(x), len(x), d_in, n) == n
        got = d_in.download(3 * n * 4, dtype=np.int16).reshape(3, n, 2)
        for r in range(2):
            assert np.array_equal(got[r], want[r]), (r, _first_difference(got[r], want[r]))
        assert np.array_equal(got[2], naive) and z.debug_last_launch()["form"] == 2
    d_wide.free()
    frames = n // nv.FRAME_IN
    with nv.Pipeline(n_streams=3, chain_masks=[3, 1, 3], labels=[[518, 490], [4209, 0], [518, 490]], max_frames=8) as p:
        for f0 in range(0, frames, 8):
            p.process_resident(d_in, n, f0, min(8, frames - f0), hip_stream=p.hip_stream)
        p.fetch()
        bits = [(p.bits(s, 0), p.bits(s, 1)) for s in range(3)]
        msgs = [{f: [m[3] for m in p.messages if m[0] == s and m[1] == f] for f in (518, 490, 4209)} for s in range(3)]
    d_in.free()
    cpu = [zc.delivered(oracle, row, nv.FRAME_IN) for row in (want[0], want[1], naive)]
    assert bits[0] == cpu[0][1] and bits[2] == cpu[2][1] and bits[1] == (cpu[1][1][0], "")
    assert msgs[0][518] == cpu[0][0][518] == [t518] and msgs[0][490] == cpu[0][0][490] == [t490]
    assert msgs[1][4209] == cpu[1][0][518] == [t4209]
    assert msgs[2][490] == cpu[2][0][490] != [t490]
