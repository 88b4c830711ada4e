"""The row aligner (include/navtex_amd_align.h) on the GPU (-m gpu).  Measure: the tables and power sums equal to the
restatement (tests/align_ref.py) at N = 1024 and 4096 with 64 and 128 lags, lag_first negative, positive and straddling zero,
both rows at -32768 and at +32767 over several 32-bit folds, all four formats, two pairs with pitches of their own, and the
refused calls.  Apply: all four formats, fractions 0, 1 and 31 of both signs, delay 0 and +-max_delay, one shot against cuts of
0, 1, T - 1, T samples and a chunk boundary, a delay changed between calls, a reset pair rejoining, positions beyond 2^32, both
launch forms, alternating full-scale input that drives the clamp, push against resident.  End to end: one seed of the
acceptance case through measure -> find -> set -> align -> nvx_anc_resident -> a two-chain handle.  Every comparison is ==,
with sentinels around every output row, and both input rows are full scale behind the samples of a call."""
from pathlib import Path

import numpy as np
import pytest

import align_cases as alc
import align_ref as ar
import anc_cases as ac
import anc_ref

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FORMATS = (ar.CS16, ar.CU8, ar.CS8, ar.CF32)
FORMAT_IDS = ("cs16", "cu8", "cs8", "cf32")
SENTINEL = 0x5a5a1234
T = ar.T


@pytest.fixture(scope="module")
def al(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_align.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.align
    return navtex_amd.align


def _upload(nv, pairs, n_call, pitch_extra=0):
    """The first n_call samples of every pair's rows as whole rows, full scale behind them up to the pitch; the sense rows have
    a pitch of their own.  Returns (d_main, pitch_main, d_sense, pitch_sense)."""
    ns = len(pairs)
    dt = pairs[0][0].dtype
    bps = dt.itemsize * 2
    pitch_main = (max(n_call, 1) + 7) // 8 * 8 + 8 * pitch_extra + 8
    pitch_sense = pitch_main + 8 * (pitch_extra + 1)
    full = 1.0 if dt == np.float32 else np.iinfo(dt).max
    block_a = np.full((ns, pitch_main, 2), full, dtype=dt); block_b = np.full((ns, pitch_sense, 2), full, dtype=dt)
    for s in range(ns):
        block_a[s, :n_call] = pairs[s][0][:n_call]
        block_b[s, :n_call] = pairs[s][1][:n_call]
    d_main = nv.DeviceBuffer(ns * pitch_main * bps); d_sense = nv.DeviceBuffer(ns * pitch_sense * bps)
    d_main.upload(block_a); d_sense.upload(block_b)
    return d_main, pitch_main, d_sense, pitch_sense


def _run_resident(nv, c, pairs, cuts, pitch_extra=0, out_first=0, before_call=None):
    """The pairs through nvx_align_resident in calls of `cuts` samples; sentinels around every row of both outputs, which have
    pitches of their own.  before_call(i) runs in front of call i.  Returns two int16 [pairs, n, 2]."""
    ns, n = len(pairs), len(pairs[0][0])
    assert sum(cuts) == n and ns == c.n_pairs
    pitch_om = out_first + n + pitch_extra
    pitch_os = pitch_om + 4 * (pitch_extra + 1)
    d_om = nv.DeviceBuffer(ns * pitch_om * 4); d_os = nv.DeviceBuffer(ns * pitch_os * 4)
    d_om.upload(np.full(ns * pitch_om, SENTINEL, dtype=np.uint32)); d_os.upload(np.full(ns * pitch_os, SENTINEL, dtype=np.uint32))
    start = c.position(0)
    pos = 0
    for i, cut in enumerate(cuts):
        if before_call:
            before_call(i)
        d_main, pitch_main, d_sense, pitch_sense = _upload(nv, [(a[pos:pos + cut], b[pos:pos + cut]) for a, b in pairs], cut, pitch_extra)
        c.resident(d_main, pitch_main, d_sense, pitch_sense, cut, d_om, pitch_om, d_os, pitch_os, out_first + pos)
        d_main.free(); d_sense.free()
        pos += cut
    assert c.position(ns - 1) == start + n
    outs = []
    for d, pitch in ((d_om, pitch_om), (d_os, pitch_os)):
        words = d.download(ns * pitch * 4, dtype=np.uint32).reshape(ns, pitch)
        d.free()
        assert np.all(words[:, :out_first] == SENTINEL) and np.all(words[:, out_first + n:] == SENTINEL), "words outside the span were written"
        outs.append(np.ascontiguousarray(words[:, out_first:out_first + n]).view(np.int16).reshape(ns, n, 2))
    return outs


def _first_difference(got, want):
    return int(np.argmax(np.any(got != want, axis=1)))


def _same(got, want, what):
    assert np.array_equal(got, want), (what, _first_difference(got, want))


# ---------------------------------------------------------------------------------------------------------------- measure
def _measure_and_compare(nv, al, pairs, fmt, n_in, lag_first, n_lags, max_delay=4096, pitch_extra=1):
    d_main, pitch_main, d_sense, pitch_sense = _upload(nv, pairs, n_in, pitch_extra)
    with al.Aligner(fmt if fmt != ar.CF32 else ar.CS16, n_pairs=len(pairs), max_delay=max_delay) as c:      # the call's format is its own
        r, p = c.measure_resident(d_main, pitch_main, d_sense, pitch_sense, n_in, lag_first, n_lags, format=fmt)
    d_main.free(); d_sense.free()
    for s, (a, b) in enumerate(pairs):
        want_r, saa, sbb, n = ar.measure(a[:n_in], b[:n_in], fmt, lag_first, n_lags)
        assert n == al.window(n_in, lag_first, n_lags)
        bad = np.argwhere(r[s] != want_r)
        assert len(bad) == 0, (s, bad[:4], r[s][tuple(bad[0])], want_r[tuple(bad[0])])
        assert (int(p[s, 0]), int(p[s, 1])) == (saa, sbb), s
    return r, p


@pytest.mark.parametrize("window,lag_first,n_lags", [(1024, -96, 64), (1024, 5, 128), (4096, -30, 64), (4096, -127, 128), (4096 + 512, 40, 64)])
def test_measure_equals_the_restatement_over_windows_and_lags(nv, al, window, lag_first, n_lags):
    """N = 1024 and 4096 (and 4608: a tile of which two waves have nothing), lag_first negative, positive and straddling zero;
    n_in leaves up to 255 samples outside the window."""
    lag_last = lag_first + n_lags - 1
    n_in = window + max(0, lag_last) - min(0, lag_first) + 201
    pairs = [alc.random_rows(ar.CS16, n_in, 900 + s + window + n_lags) for s in range(2)]
    assert ar.window(n_in, lag_first, n_lags)[1] == window
    _measure_and_compare(nv, al, pairs, ar.CS16, n_in, lag_first, n_lags)


@pytest.mark.parametrize("value", [-32768, 32767])
def test_measure_with_both_rows_at_a_rail_over_several_folds(nv, al, value):
    """Every product at its largest: a term is 2^23 at -32768, so 128 terms fill 2^30 of a 32-bit partial and 256 would
    reach 2^31.  N = 4096 is thirty-two folds; several chunks add into one table."""
    n_in = 4096 + 63
    pairs = [(alc.rails(n_in, value), alc.rails(n_in, value))]
    r, p = _measure_and_compare(nv, al, pairs, ar.CS16, n_in, 0, 64)
    m = value >> 4
    assert np.all(r[0, :, 0] == 2 * m * m * 4096) and not r[0, :, 1].any() and int(p[0, 0]) == 2 * m * m * 4096


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_measure_in_every_format_with_two_pairs_and_pitches_of_their_own(nv, al, fmt):
    n_in = 2048 + 127 + 9
    pairs = [alc.random_rows(fmt, n_in, 40 + 10 * fmt + s) for s in range(2)]
    _measure_and_compare(nv, al, pairs, fmt, n_in, -64, 128, pitch_extra=2)


def test_measure_finds_the_delay_of_common_noise_on_the_device(nv, al):
    a, b = alc.noise_pair(16384 + 300, 33.25, 77)
    r, p = _measure_and_compare(nv, al, [(a, b)], ar.CS16, len(a), -64, 256)
    n = al.window(len(a), -64, 256)
    e = al.find(r[0], -64, n, int(p[0, 0]), int(p[0, 1]))
    assert e == ar.find(r[0], -64, n, int(p[0, 0]), int(p[0, 1])) and e["reason"] == 0 and abs(e["delay_q5"] - 33.25 * 32) <= 1, e


def test_measure_refuses_before_anything_is_launched(nv, al):
    d = nv.DeviceBuffer(8192 * 4); e = nv.DeviceBuffer(8192 * 4)
    with al.Aligner(ar.CS16, max_delay=200) as c:
        for kw in (dict(n_lags=0), dict(n_lags=65), dict(n_lags=16384), dict(lag_first=-201), dict(lag_first=150, n_lags=64), dict(n_in=1024 + 63 - 1),
                   dict(fmt=4), dict(fmt=-1), dict(n_in=8193)):
            args = dict(n_in=4096, lag_first=0, n_lags=64, fmt=ar.CS16)
            args.update(kw)
            with pytest.raises(nv.NvxError) as err:
                c.measure_resident(d, 8192, e, 8192, args["n_in"], args["lag_first"], args["n_lags"], format=args["fmt"])
            assert err.value.code == nv._native.ERR_ARG, kw
        c.measure_resident(d, 8192, e, 8192, 1024 + 63, 0, 64)
    d.free(); e.free()


# ------------------------------------------------------------------------------------------------------------------ apply
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_apply_in_every_format_with_two_pairs(nv, al, fmt):
    """Full-scale random rows, a fraction in both directions, out_first = 7 (the word-by-word stores) and 8."""
    n = 9000
    pairs = [alc.random_rows(fmt, n, 300 + 10 * fmt + s) for s in range(2)]
    delays = (32 * 5 + 13, -(32 * 3 + 7))
    want = [ar.align(a, b, d, fmt, 64) for (a, b), d in zip(pairs, delays)]
    for out_first in (7, 8):
        with al.Aligner(fmt, n_pairs=2, max_delay=64) as c:
            for s, d in enumerate(delays):
                c.set_delay(d, s)
            assert [c.get_delay(s) for s in range(2)] == list(delays)
            om, os_ = _run_resident(nv, c, pairs, [n], pitch_extra=3 + out_first % 2, out_first=out_first)
            for s in range(2):
                _same(om[s], want[s][0], (out_first, s, "main")); _same(os_[s], want[s][1], (out_first, s, "sense"))


@pytest.mark.parametrize("delay", [0, 1, 31, 32, 33, -1, -31, -32, -33, 32 * 50, -32 * 50, 32 * 50 - 1, -(32 * 50 - 31)])
def test_one_shot_equals_cuts_for_every_kind_of_delay(nv, al, delay):
    """Fractions 0, 1 and 31 of both signs, delay 0 and +-max_delay (50): one shot of the restatement against the device cut at
    0, 1, T - 1, T samples and at a chunk boundary (16 384: the second call starts a pair spread over two workgroups)."""
    n = 16384 + 33 + 6 * 4096 + 5
    a, b = alc.random_rows(ar.CS16, n, 5000 + delay)
    want = ar.align(a, b, delay, ar.CS16, 50)
    cuts = [0, 1, T - 1, T, 16384]
    cuts.append(n - sum(cuts))
    with al.Aligner(ar.CS16, max_delay=50) as c:
        c.set_delay(delay)
        om, os_ = _run_resident(nv, c, [(a, b)], cuts)
        assert c.debug_last_launch()["form"] == 2 and c.debug_last_launch()["chunks"] == 2
    _same(om[0], want[0], "main"); _same(os_[0], want[1], "sense")
    dm, ds, f = ar.split_delay(delay)
    if f == 0:                                          # a whole delay is the conversion word for word, moved
        assert np.array_equal(os_[0][ar.G + ds:], b[:n - ar.G - ds]) and not os_[0][:ar.G + ds].any()
    assert np.array_equal(om[0][ar.G + dm:], a[:n - ar.G - dm]) and not om[0][:ar.G + dm].any()


def test_the_default_max_delay_at_both_ends_and_one_workgroup_per_pair(nv, al):
    n = 9000
    a, b = alc.random_rows(ar.CS16, n, 5)
    with al.Aligner(ar.CS16) as c:
        for delay in (32 * 4096, -32 * 4096, -(32 * 4096 - 1)):
            c.reset(); c.set_delay(delay)
            om, os_ = _run_resident(nv, c, [(a, b)], [4000, 5000])
            want = ar.align(a, b, delay)
            _same(om[0], want[0], (delay, "main")); _same(os_[0], want[1], (delay, "sense"))
            assert c.debug_last_launch()["form"] == 1 and c.debug_last_launch()["chunks"] == 1
        with pytest.raises(nv.NvxError):
            c.set_delay(32 * 4096 + 1)


def test_a_delay_changed_between_calls_a_reset_pair_rejoining_and_positions_beyond_2_to_the_32(nv, al):
    n1, n2 = 5000, 6001
    pairs = [alc.random_rows(ar.CS16, n1 + n2, 60 + s) for s in range(3)]
    refs = [ar.Aligner(ar.CS16, 300, 32 * 200 + 5) for _ in range(3)]
    with al.Aligner(ar.CS16, n_pairs=3, max_delay=300) as c:
        c.debug_set_position((1 << 32) + 12345)
        c.set_delay(32 * 200 + 5)
        om, os_ = _run_resident(nv, c, [(a[:n1], b[:n1]) for a, b in pairs], [n1])
        for s in range(3):
            w = refs[s].push(pairs[s][0][:n1], pairs[s][1][:n1])
            _same(om[s], w[0], (s, "main")); _same(os_[s], w[1], (s, "sense"))
        assert c.position(2) == (1 << 32) + 12345 + n1
        # pair 1 starts anew, alone, up to where the others stand; the others get another delay, which reaches into the carried samples
        d = nv.DeviceBuffer(3 * 64 * 4); e = nv.DeviceBuffer(3 * 64 * 4); o = nv.DeviceBuffer(3 * 64 * 4); o2 = nv.DeviceBuffer(3 * 64 * 4)
        assert al.lib.nvx_align_resident(c._h, d.ptr, 64, e.ptr, 64, 64, o.ptr, 64, o.ptr, 64, 0, None) == nv._native.ERR_ARG      # the outputs overlap
        assert al.lib.nvx_align_resident(c._h, d.ptr, 64, e.ptr, 64, 64, d.ptr, 64, o2.ptr, 64, 0, None) == nv._native.ERR_ARG
        assert al.lib.nvx_align_resident(c._h, d.ptr, 64, e.ptr, 64, 65, o.ptr, 64, o2.ptr, 64, 0, None) == nv._native.ERR_ARG     # leaves the allocation
        c.reset(1)
        assert c.position(1) == 0
        assert al.lib.nvx_align_resident(c._h, d.ptr, 64, e.ptr, 64, 64, o.ptr, 64, o2.ptr, 64, 0, None) == nv._native.ERR_STATE
        assert b"same position" in al.lib.nvx_align_last_error()
        d.free(); e.free(); o.free(); o2.free()
        c.debug_set_position((1 << 32) + 12345, pair=1)
        fresh = ar.Aligner(ar.CS16, 300, -(32 * 7 + 31))
        c.set_delay(-(32 * 7 + 31), pair=1)
        other = alc.random_rows(ar.CS16, n1 + n2, 99)
        pos = 0
        for cut in (1, 0, 4000, n1 - 4001):
            got = c.push(1, other[0][pos:pos + cut], other[1][pos:pos + cut])
            w = fresh.push(other[0][pos:pos + cut], other[1][pos:pos + cut])
            assert np.array_equal(got[0], w[0]) and np.array_equal(got[1], w[1]), pos
            pos += cut
        c.set_delay(-(32 * 300), pair=0); refs[0].set_delay(-(32 * 300))
        c.set_delay(17, pair=2); refs[2].set_delay(17)
        rows = [(pairs[0][0][n1:], pairs[0][1][n1:]), (other[0][n1:], other[1][n1:]), (pairs[2][0][n1:], pairs[2][1][n1:])]
        om, os_ = _run_resident(nv, c, rows, [n2])
        for s, ref in enumerate((refs[0], fresh, refs[2])):
            w = ref.push(*rows[s])
            _same(om[s], w[0], (s, "main, second call")); _same(os_[s], w[1], (s, "sense, second call"))


def test_alternating_full_scale_input_drives_the_clamp(nv, al):
    n = 5000
    a, b = alc.alternating(n)
    with al.Aligner(ar.CS16, max_delay=8) as c:
        c.set_delay(-16)
        om, os_ = _run_resident(nv, c, [(a, b)], [n])
    want = ar.align(a, b, -16, ar.CS16, 8)
    assert (want[1] == 32767).sum() > 100 and (want[1] == -32768).sum() > 100
    acc = sum(np.abs(ar.taps()[16])) * 32768
    assert acc > 32767 << 14 and acc + 8192 < 1 << 31
    _same(om[0], want[0], "main"); _same(os_[0], want[1], "sense")


def test_push_equals_resident(nv, al):
    n = 7000
    a, b = alc.random_rows(ar.CU8, n, 8)
    with al.Aligner(ar.CU8, n_pairs=2, max_delay=100) as c:
        c.set_delay(32 * 40 + 9)
        om, os_ = _run_resident(nv, c, [(a, b), (b, a)], [3000, 4000])
        c.reset()
        got = [c.push(0, a[:3000], b[:3000]), c.push(0, a[3000:], b[3000:])]
        assert np.array_equal(np.concatenate([g[0] for g in got]), om[0]) and np.array_equal(np.concatenate([g[1] for g in got]), os_[0])
        assert c.position(0) == n and c.position(1) == 0
        assert c.push(0, a[:0], b[:0])[0].shape == (0, 2)


# ------------------------------------------------------------------------------------------------------------ end to end
def test_seed_11_of_the_acceptance_case_on_the_device(nv, al, oracle):
    """GPU measure -> find -> set -> align -> nvx_anc_resident -> a two-chain handle: the 490 message arrives from the aligned
    and cancelled row, and not from the row the canceller makes of the same pair without the aligner."""
    import navtex_amd.anc as an
    t490 = ac.text()
    a, b = alc.pair(nv, 11)
    n = len(a)
    d_a = nv.DeviceBuffer(n * 4); d_b = nv.DeviceBuffer(n * 4); d_ya = nv.DeviceBuffer(n * 4); d_yb = nv.DeviceBuffer(n * 4)
    d_rows = nv.DeviceBuffer(2 * n * 4)
    d_a.upload(a); d_b.upload(b)
    with al.Aligner(ar.CS16) as c:
        r, p = c.measure_resident(d_a, n, d_b, n, alc.MEASURE_N, alc.LAG_FIRST, alc.N_LAGS)
        want_r, saa, sbb, nw = ar.measure(a[:alc.MEASURE_N], b[:alc.MEASURE_N], ar.CS16, alc.LAG_FIRST, alc.N_LAGS)
        assert np.array_equal(r[0], want_r) and (int(p[0, 0]), int(p[0, 1])) == (saa, sbb)
        e = c.find(r[0], alc.LAG_FIRST, nw, saa, sbb)
        assert e["reason"] == 0 and abs(e["delay_q5"] - alc.DELAY * 32) <= 1, e
        c.set_delay(e["delay_q5"])
        c.resident(d_a, n, d_b, n, n, d_ya, n, d_yb, n)
        ya, yb = d_ya.download(n * 4, dtype=np.int16).reshape(n, 2), d_yb.download(n * 4, dtype=np.int16).reshape(n, 2)
    want = ar.align(a, b, e["delay_q5"])
    _same(ya, want[0], "main"); _same(yb, want[1], "sense")
    with an.Canceller(ar.CS16) as k:
        k.resident(d_a, n, d_b, n, n, d_rows, n, out_first=0)            # row 0: the canceller alone
        k.reset()
        k.resident(d_ya, n, d_yb, n, n, d_rows, n, out_first=n)          # row 1: behind the aligner
        got = d_rows.download(2 * n * 4, dtype=np.int16).reshape(2, n, 2)
    _same(got[0], anc_ref.cancel(a, b)[0], "plain"); _same(got[1], anc_ref.cancel(ya, yb)[0], "aligned")
    frames = n // nv.FRAME_IN
    with nv.Pipeline(n_streams=2, chain_mask=nv.CHAIN_518 | nv.CHAIN_490, max_frames=8) as pl:
        for f0 in range(0, frames, 8):
            pl.process_resident(d_rows, n, f0, min(8, frames - f0), hip_stream=pl.hip_stream)
        pl.fetch()
        msgs = [[m[3] for m in pl.messages if m[0] == s and m[1] == 490] for s in range(2)]
    for d in (d_a, d_b, d_ya, d_yb, d_rows):
        d.free()
    assert msgs[1] == [t490] and msgs[0] != [t490]
