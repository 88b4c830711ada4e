"""The antenna noise canceller (include/navtex_amd_anc.h) on the GPU (-m gpu): output words equal to the restatement
(tests/anc_ref.py) for every format in one call from position 0, W = 4 cut into calls at and next to the block ends against
one shot, a reset pair rejoining the others, the rails and full-scale random input (float32 specials) with the counters and
the window's sums, the rejection reasons 1, 2 and 3, the two launch shapes, positions beyond 2^32, set / HOLD / TRACK between
calls, push against resident, the calls that are refused before anything is launched, and the acceptance case's seed 11
through a two-chain handle.  Every comparison is ==, with sentinels around every output row, and both input rows are full
scale behind the samples of a call."""
from pathlib import Path

import numpy as np
import pytest

import anc_cases as ac
import anc_ref as ar

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FORMATS = (ar.CS16, ar.CU8, ar.CS8, ar.CF32)
FORMAT_IDS = ("cs16", "cu8", "cs8", "cf32")
SENTINEL = 0x5a5a1234
B = ar.BLOCK


@pytest.fixture(scope="module")
def an(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_anc.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.anc
    return navtex_amd.anc


def _run_resident(nv, c, pairs, cuts, pitch_extra=0, out_first=0):
    """The pairs ((main, sense), [n, 2] each, all of one length) through nvx_anc_resident in calls of `cuts` samples; every
    call's input is uploaded to the start of the input rows as whole rows: behind a call's n_in samples both rows are full
    scale up to the pitch, so a read behind n_in changes the output and the sums.  The sense rows have a pitch of their own.
    Sentinels around every output row.  Returns int16 [pairs, n, 2]."""
    ns, n = len(pairs), len(pairs[0][0])
    assert sum(cuts) == n and ns == c.n_pairs
    dt = pairs[0][0].dtype
    bps = dt.itemsize * 2
    pitch_out = out_first + n + pitch_extra
    pitch_main = (max(max(cuts), 1) + 7) // 8 * 8 + 8 * pitch_extra
    pitch_sense = pitch_main + 8 * (pitch_extra + 1)
    d_main = nv.DeviceBuffer(ns * pitch_main * bps); d_sense = nv.DeviceBuffer(ns * pitch_sense * bps)
    d_out = nv.DeviceBuffer(ns * pitch_out * 4)
    d_out.upload(np.full(ns * pitch_out, SENTINEL, dtype=np.uint32))
    block_a = np.empty((ns, pitch_main, 2), dtype=dt); block_b = np.empty((ns, pitch_sense, 2), dtype=dt)
    full = 1.0 if dt == np.float32 else np.iinfo(dt).max
    start = c.position(0)
    pos = 0
    for cut in cuts:
        block_a[:, cut:] = full; block_b[:, cut:] = full
        for s in range(ns):
            block_a[s, :cut] = pairs[s][0][pos:pos + cut]
            block_b[s, :cut] = pairs[s][1][pos:pos + cut]
        d_main.upload(block_a); d_sense.upload(block_b)
        c.resident(d_main, pitch_main, d_sense, pitch_sense, cut, d_out, pitch_out, out_first + pos)
        pos += cut
    assert c.position(ns - 1) == start + n
    words = d_out.download(ns * pitch_out * 4, dtype=np.uint32).reshape(ns, pitch_out)
    d_main.free(); d_sense.free(); d_out.free()
    assert np.all(words[:, :out_first] == SENTINEL) and np.all(words[:, out_first + n:] == SENTINEL), "words outside the span were written"
    return np.ascontiguousarray(words[:, out_first:out_first + n]).view(np.int16).reshape(ns, n, 2)


def _first_difference(got, want):
    return int(np.argmax(np.any(got != want, axis=1)))


def _status(ref):
    """What nvx_anc_get returns, from the restatement."""
    return {"weight": tuple(int(v) for v in ref.c), "mode": ref.mode, "last_reason": ref.reason, "coherence_q14": ref.coherence, "sums": ref.sums(),
            "samples": ref.samples, "blocks_solved": ref.solved, "blocks_rejected": ref.rejected}


# ------------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_two_pairs_of_six_and_a_half_blocks_in_every_format(nv, an, fmt):
    """W = 4: blocks 4, 5 and 6 are solved.  Pitches larger than the data; out_first = 7 (the unaligned stores) and 8."""
    n = 6 * B + B // 2
    pairs = [ac.formatted_pair(n, 200 + 10 * fmt + s, fmt) for s in range(2)]
    refs = [ar.cancel(a, b, fmt, 2) for a, b in pairs]
    assert all(ref.solved == 3 and len({h[1] for h in ref.history}) == 3 for _, ref in refs)
    for out_first in (7, 8):
        with an.Canceller(fmt, n_pairs=2, window_log2=2) as c:
            got = _run_resident(nv, c, pairs, [n], pitch_extra=3 + out_first % 2, out_first=out_first)
            for s in range(2):
                assert np.array_equal(got[s], refs[s][0]), (out_first, s, _first_difference(got[s], refs[s][0]))
                assert c.get(s) == _status(refs[s][1]), (out_first, s)


# ------------------------------------------------------------------------------------------------------------------ (b)
def test_one_shot_equals_calls_cut_at_the_block_ends_and_a_reset_pair_rejoins(nv, an):
    cuts = [B + 1, 1, 0, B - 1, B]
    n1 = 8 * B
    cuts = cuts + [n1 - sum(cuts)]
    tail = B + 777
    pairs = [ac.drifting_pair(n1 + tail, 400 + s) for s in range(3)]
    refs = [ar.cancel(a, b, ar.CS16, 2) for a, b in pairs]
    with an.Canceller(ar.CS16, n_pairs=3, window_log2=2) as c:
        got = _run_resident(nv, c, [(a[:n1], b[:n1]) for a, b in pairs], cuts)
        for s in range(3):
            assert np.array_equal(got[s], refs[s][0][:n1]), (s, _first_difference(got[s], refs[s][0][:n1]))
        c.reset(1)
        assert c.position(1) == 0 and c.position(0) == n1 and c.get(1)["weight"] == (0, 0) and c.get(1)["coherence_q14"] == 0
        d = nv.DeviceBuffer(3 * 64 * 4); e = nv.DeviceBuffer(3 * 64 * 4); o = nv.DeviceBuffer(3 * 64 * 4)
        assert an.lib.nvx_anc_resident(c._h, d.ptr, 64, e.ptr, 64, 64, o.ptr, 64, 0, None) == nv._native.ERR_STATE
        assert b"same position" in an.lib.nvx_anc_last_error()
        d.free(); e.free(); o.free()
        # pair 1 starts anew on other data, alone and in calls of its own, up to where the others stand
        fresh = ar.Canceller(ar.CS16, 2)
        other = ac.drifting_pair(n1 + tail, 450)
        pos = 0
        for cut in (B + 5, 1, B - 6, n1 - 2 * B):
            assert np.array_equal(c.push(1, other[0][pos:pos + cut], other[1][pos:pos + cut]), fresh.push(other[0][pos:pos + cut], other[1][pos:pos + cut])), pos
            pos += cut
        assert c.position(1) == n1
        got = _run_resident(nv, c, [(pairs[0][0][n1:], pairs[0][1][n1:]), (other[0][n1:], other[1][n1:]), (pairs[2][0][n1:], pairs[2][1][n1:])], [tail])
        assert np.array_equal(got[0], refs[0][0][n1:]) and np.array_equal(got[2], refs[2][0][n1:])
        assert np.array_equal(got[1], fresh.push(other[0][n1:], other[1][n1:]))
        assert c.get(0) == _status(refs[0][1]) and c.get(2) == _status(refs[2][1])
        st = c.get(1)
        assert st["weight"] == fresh.c and st["sums"] == fresh.sums() and st["samples"] == 2 * n1 + tail and st["coherence_q14"] == fresh.coherence


# ------------------------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_the_rails_and_full_scale_random_input_with_counters_and_sums(nv, an, fmt):
    """Every product at its largest: I^2 + Q^2 = 2^31 in both rows and I1 I2 + Q1 Q2 = 2^31 in every sample of the first
    pair.  The counters and the window's four sums are the restatement's integers."""
    n = 5 * B + 21000
    pairs = ac.extremes(fmt, n, 500 + fmt)
    refs = [ar.cancel(a, b, fmt, 2) for a, b in pairs]
    if fmt == ar.CS16:
        assert refs[0][1].sums() == (4 * B * 2 ** 31,) * 3 + (0,) and refs[0][1].c == (8192, 0)
    assert all(ref.solved + ref.rejected == 2 for _, ref in refs)
    with an.Canceller(fmt, n_pairs=3, window_log2=2) as c:
        got = _run_resident(nv, c, pairs, [2 * B + 11, n - 2 * B - 11], out_first=3)
        for s in range(3):
            assert np.array_equal(got[s], refs[s][0]), (s, _first_difference(got[s], refs[s][0]))
            assert c.get(s) == _status(refs[s][1]), s


def test_the_rejection_reasons(nv, an):
    """The CPU suite's rows on the device: a silent sense row (1), a faint one (2), one at a quarter of the main row (3), and one
    at half of it, which solves to (16384, 0) and leaves nothing."""
    n = 5 * B + 100
    pairs = [ac.silent_sense(n), ac.faint_sense(n), ac.quarter_sense(n), ac.half_sense(n)]
    refs = [ar.cancel(a, b, ar.CS16, 2) for a, b in pairs]
    assert [ref.reason for _, ref in refs] == [1, 2, 3, 0] and [ref.rejected for _, ref in refs] == [2, 2, 2, 0]
    assert refs[2][1].coherence == 16384 and refs[3][1].c == (16384, 0) and not refs[3][0][4 * B:].any()
    with an.Canceller(ar.CS16, n_pairs=4, window_log2=2) as c:
        got = _run_resident(nv, c, pairs, [n])
        for s in range(4):
            assert np.array_equal(got[s], refs[s][0]), (s, _first_difference(got[s], refs[s][0]))
            assert c.get(s) == _status(refs[s][1]), s


# ------------------------------------------------------------------------------------------------------------------ (d)
def test_a_pair_spread_over_chunks(nv, an):
    """1 pair x 40 blocks behind a first call of 777 samples: twenty workgroups of two blocks each, block ends inside tiles."""
    first, n = 777, 40 * B
    a, b = ac.drifting_pair(first + n, 70)
    want, ref = ar.cancel(a, b, ar.CS16, 2)
    with an.Canceller(ar.CS16, window_log2=2) as c:
        got = _run_resident(nv, c, [(a, b)], [first, n])
        assert c.debug_last_launch() == {"launches": 4, "chunks": 20, "tiles_per_chunk": 32, "records": 41, "form": 2}
        assert np.array_equal(got[0], want), _first_difference(got[0], want)
        assert c.get(0) == _status(ref) and ref.solved == 37


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_block_ends_everywhere_in_a_tile(nv, an, fmt):
    """The IQ corrector's block-end sweep (iqc_cases.sweep_cuts: 35 blocks in 44 calls; the kernels share its tiles, so its
    model of them holds here): a block ends 1, 3, 4, 255 ... 4092, 4095 samples into a call's first, second or third tile -- in
    every wave, on and beside every edge of a lane's group, a step, a half tile and a wave's region --, seven calls end 1, 5 or
    90 samples behind the end in the same tile and six end on it.  Two pairs: one whose every window solves to another weight,
    so that a sample given the wrong block's weight shows, and full-scale random rows, in which a sample added to the wrong
    block changes the sums and the solves behind them."""
    import iqc_cases as ic
    cuts = ic.sweep_cuts()
    n = sum(cuts)
    splits, ragged, exact = ic.sweep_coverage(cuts)
    assert set(splits) >= set(ic.SWEEP_N_A) and len(ragged) >= 5 and exact >= 5 and n == 35 * B + 777
    pairs = [ac.formatted_pair(n, 900 + fmt, fmt), ac.extremes(fmt, n, 910 + fmt)[2]]
    refs = [ar.cancel(a, b, fmt, 2) for a, b in pairs]
    weights = [h[1] for h in refs[0][1].history]
    assert refs[0][1].solved == 32 and all(x != y for x, y in zip(weights, weights[1:]))
    with an.Canceller(fmt, n_pairs=2, window_log2=2) as c:
        got = _run_resident(nv, c, pairs, cuts)
        for s in range(2):
            assert np.array_equal(got[s], refs[s][0]), (s, _first_difference(got[s], refs[s][0]))
            assert c.get(s) == _status(refs[s][1]), s


# ------------------------------------------------------------------------------------------------------------------ (e)
def test_scale_256_pairs(nv, an):
    """256 pairs x 5.2 blocks of unsigned 8-bit samples, sixteen different pairs among them, every pair checked.  Two calls: two
    blocks, which a workgroup per pair takes (form 1: 32 tiles are one chunk), and the rest, which the launch arithmetic
    spreads over two workgroups per pair (below 1024 pairs it aims at 2048 workgroups, in chunks of at least 32 tiles)."""
    ns, n, kinds = 256, int(5.2 * B) // 8 * 8, 16
    pairs = [ac.formatted_pair(n, 7000 + k, ar.CU8) for k in range(kinds)]
    refs = [ar.cancel(a, b, ar.CU8, 2) for a, b in pairs]
    d_main = nv.DeviceBuffer(ns * n * 2); d_sense = nv.DeviceBuffer(ns * n * 2); d_out = nv.DeviceBuffer(ns * n * 4)
    block_a, block_b = np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])
    for s in range(0, ns, kinds):
        d_main.upload(block_a, s * n * 2); d_sense.upload(block_b, s * n * 2)

    class At:
        def __init__(self, ptr):
            self.ptr = ptr

    with an.Canceller(ar.CU8, n_pairs=ns, window_log2=2) as c:
        c.resident(d_main, n, d_sense, n, 2 * B, d_out, n)
        shape = c.debug_last_launch()
        assert shape == {"launches": 2, "chunks": 1, "tiles_per_chunk": 32, "records": 2, "form": 1}
        rest = n - 2 * B
        c.resident(At(d_main.ptr + 2 * B * 2), n, At(d_sense.ptr + 2 * B * 2), n, rest, d_out, n, 2 * B)
        shape = c.debug_last_launch()
        assert shape == {"launches": 4, "chunks": 2, "tiles_per_chunk": 32, "records": 4, "form": 2} and (rest + 4095) // 4096 == 52
        got = d_out.download(ns * n * 4, dtype=np.int16).reshape(ns, n, 2)
        status = {s: c.get(s) for s in (0, 127, 255)}
    d_main.free(); d_sense.free(); d_out.free()
    bad = [s for s in range(ns) if not np.array_equal(got[s], refs[s % kinds][0])]
    assert not bad, bad[:10]
    assert all(st == _status(refs[s % kinds][1]) for s, st in status.items()) and refs[0][1].solved == 2


# ------------------------------------------------------------------------------------------------------------------ (f)
@pytest.mark.parametrize("position", [2 ** 32 - 1000, 2 ** 40 + 5])
def test_positions_beyond_32_bits(nv, an, position):
    """Three blocks in two calls from the position, then a block and a half more: the block the position lies in counts as
    complete when it ends, with the samples it got."""
    n, more = 3 * B, B + B // 2
    pairs = [ac.drifting_pair(n + more, 80 + s) for s in range(2)]
    refs = [ar.Canceller(ar.CS16, 2, position) for _ in pairs]
    with an.Canceller(ar.CS16, n_pairs=2, window_log2=2) as c:
        c.debug_set_position(position)
        assert c.position(1) == position
        got = _run_resident(nv, c, [(a[:n], b[:n]) for a, b in pairs], [B + 9000, n - B - 9000])
        for s in range(2):
            want = refs[s].push(pairs[s][0][:n], pairs[s][1][:n])
            assert np.array_equal(got[s], want), (s, _first_difference(got[s], want))
            assert c.get(s) == _status(refs[s])
        got = _run_resident(nv, c, [(a[n:], b[n:]) for a, b in pairs], [more])
        for s in range(2):
            want = refs[s].push(pairs[s][0][n:], pairs[s][1][n:])
            assert np.array_equal(got[s], want), (s, _first_difference(got[s], want))
            assert c.get(s) == _status(refs[s]) and refs[s].solved >= 1


# ------------------------------------------------------------------------------------------------------------------ (g)
def test_set_hold_and_back_to_track_between_calls(nv, an):
    n = 11 * B
    a, b = ac.drifting_pair(n, 90)
    ref = ar.Canceller(ar.CS16, 2)
    with an.Canceller(ar.CS16, window_log2=2) as c:
        def step(k):
            got = _run_resident(nv, c, [(a[step.pos:step.pos + k], b[step.pos:step.pos + k])], [k])
            want = ref.push(a[step.pos:step.pos + k], b[step.pos:step.pos + k])
            assert np.array_equal(got[0], want), (step.pos, _first_difference(got[0], want))
            assert c.get(0) == _status(ref), step.pos
            step.pos += k
        step.pos = 0
        c.set(-5170, -8839); ref.set(-5170, -8839)                         # in front of the first sample: held until block 4
        step(2 * B + 100)
        assert ref.c == (-5170, -8839)
        step(3 * B)                                                        # blocks 4 and 5 start: solved
        assert ref.solved == 2
        c.set_mode(an.HOLD); ref.set_mode(ar.HOLD)
        held = ref.c
        step(2 * B)
        assert ref.c == held and ref.solved == 2
        c.set(32767, -32767); ref.set(32767, -32767)                       # a calibrated set-up: set and hold, at the limits
        step(B + 17)
        assert ref.c == (32767, -32767)
        c.set_mode(an.TRACK); ref.set_mode(ar.TRACK)
        step(n - step.pos)
        assert ref.solved == 4 and c.get(0)["mode"] == an.TRACK
        for bad in ((32768, 0), (0, 32768), (-32768, 0), (0, -32768), (100000, 100000)):
            assert an.lib.nvx_anc_set(c._h, 0, *bad) == nv._native.ERR_ARG
        assert an.lib.nvx_anc_set_mode(c._h, 0, 2) == nv._native.ERR_ARG and an.lib.nvx_anc_set_mode(c._h, 0, -1) == nv._native.ERR_ARG
        assert an.lib.nvx_anc_set_mode(c._h, 1, 0) == nv._native.ERR_ARG and an.lib.nvx_anc_set(c._h, 1, 0, 0) == nv._native.ERR_ARG
        assert c.get(0) == _status(ref)


# ------------------------------------------------------------------------------------------------------------------ (h)
@pytest.mark.parametrize("fmt", [ar.CS16, ar.CS8], ids=["cs16", "cs8"])
def test_push_equals_resident(nv, an, fmt):
    n = 5 * B + 3000
    pairs = [ac.formatted_pair(2 * n, 120 + s, fmt) for s in range(3)]
    refs = [ar.cancel(a, b, fmt, 2) for a, b in pairs]
    with an.Canceller(fmt, n_pairs=3, window_log2=2) as c:
        for s, cuts in enumerate(([n], [1, B - 1, n - B], [7, 0, B + 5000, 1, n - B - 5008])):
            pos, parts = 0, []
            for cut in cuts:
                parts.append(c.push(s, pairs[s][0][pos:pos + cut], pairs[s][1][pos:pos + cut])); pos += cut
            out = np.concatenate(parts)
            assert out.dtype == np.int16 and np.array_equal(out, refs[s][0][:n]), s
            assert c.position(s) == n
        got = _run_resident(nv, c, [(a[n:], b[n:]) for a, b in pairs], [n])
        for s in range(3):
            assert np.array_equal(got[s], refs[s][0][n:]), s
            assert c.get(s) == _status(refs[s][1])


# ------------------------------------------------------------------------------------------------------------------ (i)
def test_span_alignment_overlap_and_position_errors_launch_nothing(nv, an):
    ARG = nv._native.ERR_ARG
    n = 8192
    with an.Canceller(ar.CU8, n_pairs=2) as c:
        d_a = nv.DeviceBuffer(2 * n * 2); d_b = nv.DeviceBuffer(2 * n * 2); d_out = nv.DeviceBuffer(2 * n * 4)
        one_in = nv.DeviceBuffer(n * 2); one_out = nv.DeviceBuffer(n * 4)
        both = nv.DeviceBuffer(4 * n * 4)                                     # inputs and output in one allocation
        c.timing(True)
        call = lambda *a: an.lib.nvx_anc_resident(c._h, *a, None)            # noqa: E731
        A, Bp, O = d_a.ptr, d_b.ptr, d_out.ptr
        bad = {"more samples than the main pitch": (A, n - 8, Bp, n, n, O, n, 0),
               "more samples than the sense pitch": (A, n, Bp, n - 8, n, O, n, 0),
               "words beyond the pitch": (A, n, Bp, n, n, O, n - 1, 0),
               "out_first pushes them beyond it": (A, n, Bp, n, n, O, n, 1),
               "main rows for one pair": (one_in.ptr, n, Bp, n, n, O, n, 0),
               "sense rows for one pair": (A, n, one_in.ptr, n, n, O, n, 0),
               "output rows for one pair": (A, n, Bp, n, n, one_out.ptr, n, 0),
               "misaligned main": (A + 4, n, Bp, n, n - 8, O, n, 0),
               "misaligned sense": (A, n, Bp + 8, n, n - 8, O, n, 0),
               "misaligned output": (A, n, Bp, n, n, O + 2, n, 0),
               "main rows not 16-byte aligned": (A, n - 3, Bp, n, n - 8, O, n, 0),
               "sense rows not 16-byte aligned": (A, n, Bp, n - 3, n - 8, O, n, 0),
               "null main": (None, n, Bp, n, n, O, n, 0),
               "null sense": (A, n, None, n, n, O, n, 0),
               "null output": (A, n, Bp, n, n, None, n, 0),
               "too many samples": (A, 2 ** 31, Bp, 2 ** 31, 2 ** 30 + 1, O, 2 ** 31, 0),
               "a main pitch that wraps": (A, 2 ** 63, Bp, n, n, O, n, 0),
               "a sense pitch that wraps": (A, n, Bp, 2 ** 63, n, O, n, 0),
               "an output pitch that wraps": (A, n, Bp, n, n, O, 2 ** 62, 0),
               "out_first that wraps": (A, n, Bp, n, n, O, n, 2 ** 64 - 8),
               "the output on the main rows": (both.ptr, n, Bp, n, n, both.ptr, n, 0),
               "the output on the sense rows": (A, n, both.ptr, n, n, both.ptr, n, 0),
               "the output's first row on the main rows' last": (both.ptr, n, Bp, n, n, both.ptr, n, n - 8),
               "the main rows inside the output's span": (both.ptr + 2 * n * 4, n, Bp, n, n, both.ptr, 2 * n, 0)}
        for name, args in bad.items():
            assert call(*args) == ARG, name
            assert an.lib.nvx_anc_last_error() != b""
        assert b"overlaps" in an.lib.nvx_anc_last_error()
        c.debug_set_position(2 ** 62 - 100)
        assert call(A, n, Bp, n, n, O, n, 0) == ARG and b"2^62" in an.lib.nvx_anc_last_error()
        assert an.lib.nvx_anc_debug_set_position(c._h, 0, 2 ** 62) == ARG and an.lib.nvx_anc_debug_set_position(c._h, 2, 0) == ARG
        assert an.lib.nvx_anc_reset(c._h, 2) == ARG and an.lib.nvx_anc_get(c._h, -1, None) == ARG and an.lib.nvx_anc_get(c._h, 0, None) == ARG
        assert c.time_stats() == (0.0, 0) and c.debug_last_launch()["launches"] == 0 and c.position(0) == 2 ** 62 - 100
        c.reset()
        assert call(A, n, Bp, n, 0, O, n, 0) == 0 and c.debug_last_launch()["launches"] == 0       # nothing to do: no launch
        assert c.time_stats() == (0.0, 0)
        d_a.upload(np.full(2 * n * 2, 128, dtype=np.uint8)); d_b.upload(np.full(2 * n * 2, 128, dtype=np.uint8))
        assert call(A, n, Bp, n, n, O, n, 0) == 0
        # the output behind the inputs in one allocation, touching and not overlapping
        both.upload(np.full(4 * n * 4, 128, dtype=np.uint8))
        assert call(both.ptr, n, both.ptr + 2 * n * 2, n, n, both.ptr + 4 * n * 2, n, 0) == 0
        ms, calls = c.time_stats()
        assert calls == 2 and ms > 0.0 and c.debug_last_launch()["launches"] == 4 and c.get(1)["samples"] == 2 * n
        for d in (d_a, d_b, d_out, one_in, one_out, both):
            d.free()
    for kw in (dict(device=99), dict(window_log2=3), dict(window_log2=8), dict(format=4), dict(n_pairs=0)):
        with pytest.raises(nv.NvxError) as e:
            an.Canceller(**kw)
        assert e.value.code == ARG, kw


# ------------------------------------------------------------------------------------------------------------------ (j)
def test_seed_11_of_the_acceptance_case_on_the_device(nv, an, oracle):
    """The pair of seed 11 through the canceller on the device: the words are the CPU's.  Then the main and the cancelled row as
    two streams of a two-chain handle: the 490 message arrives from the cancelled row and not from the main row, and the bits
    of all four chains are the oracle's on the same words."""
    t490 = ac.text()
    a, b = ac.pair(nv, 11)
    n = len(a)
    want, ref = ar.cancel(a, b)
    d_rows = nv.DeviceBuffer(2 * n * 4); d_sense = nv.DeviceBuffer(n * 4)
    d_rows.upload(a); d_sense.upload(b)
    with an.Canceller(ar.CS16) as c:
        # the cancelled row goes behind the main row: row 1 of the handle's input
        c.resident(d_rows, n, d_sense, n, n, d_rows, n, out_first=n)
        got = d_rows.download(2 * n * 4, dtype=np.int16).reshape(2, n, 2)
        assert np.array_equal(got[0], a) and np.array_equal(got[1], want), _first_difference(got[1], want)
        assert c.get(0) == _status(ref) and ref.solved == n // B - 3 and ref.rejected == 0
        assert abs(ref.c[0] - ac.WEIGHT[0]) <= 40 and abs(ref.c[1] - ac.WEIGHT[1]) <= 40
    frames = n // nv.FRAME_IN
    with nv.Pipeline(n_streams=2, chain_mask=nv.CHAIN_518 | nv.CHAIN_490, max_frames=8) as p:
        for f0 in range(0, frames, 8):
            p.process_resident(d_rows, n, f0, min(8, frames - f0), hip_stream=p.hip_stream)
        p.fetch()
        bits = [(p.bits(s, 0), p.bits(s, 1)) for s in range(2)]
        msgs = [[m[3] for m in p.messages if m[0] == s and m[1] == 490] for s in range(2)]
    d_rows.free(); d_sense.free()
    cpu = [ac.delivered(oracle, row, nv.FRAME_IN) for row in (a, want)]
    for s in range(2):
        assert bits[s] == cpu[s][1] and msgs[s] == cpu[s][0], s
    assert msgs[1] == [t490] and msgs[0] != [t490]
