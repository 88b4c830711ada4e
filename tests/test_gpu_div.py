"""The diversity combiner (include/navtex_amd_div.h) on the GPU (-m gpu): output words and nvx_div_get equal to the restatement
(tests/div_ref.py) for every format in one call from position 0 on aligned and unaligned output rows, calls cut at and next to
the block and cell ends against one shot, a reset pair rejoining the others, block and cell ends at every offset class of a
tile from a position set through the hook, a lead flip and reason 1 inside one call, four targets, set_freq / set / HOLD /
TRACK between calls, positions beyond 2^32, 256 pairs, push against resident, the calls that are refused before anything is
launched, and the acceptance case's seed 11 through a two-stream handle.  Every comparison is ==, with sentinels around every
output row, and both input rows are full scale behind the samples of a call."""
from pathlib import Path

import numpy as np
import pytest

import div_cases as dc
import div_ref as dr

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FORMATS = (dr.CS16, dr.CU8, dr.CS8, dr.CF32)
FORMAT_IDS = ("cs16", "cu8", "cs8", "cf32")
SENTINEL = 0x5a5a1234
B, CELL = dr.BLOCK, dr.CELL
STEPS = (0, (1 << 32) // 512, dr.step_from_hz(-14000, 252000), 0x12345678)       # 0, a whole turn per two blocks, a negative one, any


@pytest.fixture(scope="module")
def dv(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_div.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.div
    return navtex_amd.div


def _run_resident(nv, c, pairs, cuts, pitch_extra=0, out_first=0):
    """The pairs ((main, second), [n, 2] each, all of one length) through nvx_div_resident in calls of `cuts` samples; every
    call's input is uploaded to the start of the input rows as whole rows: behind a call's n_in samples both rows are full
    scale up to the pitch, so a read behind n_in changes the output and the sums.  The second rows have a pitch of their own.
    Sentinels around every output row.  Returns int16 [pairs, targets, n, 2]."""
    ns, n, nt = len(pairs), len(pairs[0][0]), c.n_targets
    assert sum(cuts) == n and ns == c.n_pairs
    dt = pairs[0][0].dtype
    bps = dt.itemsize * 2
    pitch_out = out_first + n + pitch_extra
    pitch_main = (max(max(cuts), 1) + 7) // 8 * 8 + 8 * pitch_extra
    pitch_second = pitch_main + 8 * (pitch_extra + 1)
    d_main = nv.DeviceBuffer(ns * pitch_main * bps); d_second = nv.DeviceBuffer(ns * pitch_second * bps)
    d_out = nv.DeviceBuffer(ns * nt * pitch_out * 4)
    d_out.upload(np.full(ns * nt * pitch_out, SENTINEL, dtype=np.uint32))
    block_a = np.empty((ns, pitch_main, 2), dtype=dt); block_b = np.empty((ns, pitch_second, 2), dtype=dt)
    full = 1.0 if dt == np.float32 else np.iinfo(dt).max
    start = c.position(0)
    pos = 0
    for cut in cuts:
        block_a[:, cut:] = full; block_b[:, cut:] = full
        for s in range(ns):
            block_a[s, :cut] = pairs[s][0][pos:pos + cut]
            block_b[s, :cut] = pairs[s][1][pos:pos + cut]
        d_main.upload(block_a); d_second.upload(block_b)
        c.resident(d_main, pitch_main, d_second, pitch_second, cut, d_out, pitch_out, out_first + pos)
        pos += cut
    assert c.position(ns - 1) == start + n
    words = d_out.download(ns * nt * pitch_out * 4, dtype=np.uint32).reshape(ns * nt, pitch_out)
    d_main.free(); d_second.free(); d_out.free()
    assert np.all(words[:, :out_first] == SENTINEL) and np.all(words[:, out_first + n:] == SENTINEL), "words outside the span were written"
    return np.ascontiguousarray(words[:, out_first:out_first + n]).view(np.int16).reshape(ns, nt, n, 2)


def _first_difference(got, want):
    return int(np.argmax(np.any(got != want, axis=1)))


def _same(c, got, s, want, ref, where=None):
    """Pair s of the plan: every target's words and status are the restatement's."""
    for k in range(c.n_targets):
        assert np.array_equal(got[s][k], want[k]), (where, s, k, _first_difference(got[s][k], want[k]))
        if ref is not None:
            assert c.get(s, k) == ref.status(k), (where, s, k)


def _plan(dv, fmt, n_pairs, steps, window_log2):
    c = dv.Combiner(fmt, n_pairs=n_pairs, n_targets=len(steps), window_log2=window_log2)
    for k, step in enumerate(steps):
        c.set_freq(k, step)
    return c


# ------------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_two_pairs_of_two_targets_and_three_and_a_half_cells_in_every_format(nv, dv, fmt):
    """W = 1: the cells 1, 2 and 3 are solved.  Pitches larger than the data; out_first = 7 with an odd pitch (the unaligned
    stores) and 8 with a pitch that is a multiple of 4 (the aligned ones): the same words."""
    n = 3 * CELL + CELL // 2
    steps = STEPS[1:3]
    pairs = [dc.formatted_tones(n, 200 + 10 * fmt + s, steps, fmt) for s in range(2)]
    refs = [dr.combine(a, b, steps, fmt, 0) for a, b in pairs]
    assert all(t.solved == 3 and len({h[2] for h in t.history}) == 3 for _, ref in refs for t in ref.targets)
    for out_first in (7, 8):
        with _plan(dv, fmt, 2, steps, 0) as c:
            got = _run_resident(nv, c, pairs, [n], pitch_extra=3 + out_first % 2, out_first=out_first)
            for s in range(2):
                _same(c, got, s, refs[s][0], refs[s][1], out_first)


# ------------------------------------------------------------------------------------------------------------------ (b)
def test_one_shot_equals_calls_cut_at_the_block_and_cell_ends_and_a_reset_pair_rejoins(nv, dv):
    cuts = [CELL + 1, 1, 0, B - 1, B, CELL - 2 * B - 1, 100, B - 100, 3 * B + 7]
    n1 = 4 * CELL
    cuts = cuts + [n1 - sum(cuts)]
    tail = CELL + 777
    steps = [STEPS[2]]
    pairs = [dc.tones_pair(n1 + tail, 400 + s, steps) for s in range(3)]
    refs = [dr.combine(a, b, steps, dr.CS16, 0) for a, b in pairs]
    with _plan(dv, dr.CS16, 3, steps, 0) as c:
        got = _run_resident(nv, c, [(a[:n1], b[:n1]) for a, b in pairs], cuts)
        for s in range(3):
            assert np.array_equal(got[s][0], refs[s][0][0][:n1]), (s, _first_difference(got[s][0], refs[s][0][0][:n1]))
        c.reset(1)
        st = c.get(1)
        assert c.position(1) == 0 and c.position(0) == n1 and (st["weight"], st["lead"], st["coherence_q14"], st["sums"]) == ((0, 0), 0, 0, (0, 0, 0, 0))
        assert st["step"] == STEPS[2] and st["cells_solved"] == 3
        d = nv.DeviceBuffer(3 * 64 * 4); e = nv.DeviceBuffer(3 * 64 * 4); o = nv.DeviceBuffer(3 * 64 * 4)
        assert dv.lib.nvx_div_resident(c._h, d.ptr, 64, e.ptr, 64, 64, o.ptr, 64, 0, None) == nv._native.ERR_STATE
        assert b"same position" in dv.lib.nvx_div_last_error()
        d.free(); e.free(); o.free()
        # pair 1 starts anew on other data, alone and in calls of its own, up to where the others stand
        fresh = dr.Combiner(dr.CS16, 1, 0)
        fresh.set_freq(0, STEPS[2])
        other = dc.tones_pair(n1 + tail, 450, steps)
        pos = 0
        for cut in (CELL + 5, 1, CELL - 6, n1 - 2 * CELL):
            assert np.array_equal(c.push(1, other[0][pos:pos + cut], other[1][pos:pos + cut]), fresh.push(other[0][pos:pos + cut], other[1][pos:pos + cut])), pos
            pos += cut
        assert c.position(1) == n1
        got = _run_resident(nv, c, [(pairs[0][0][n1:], pairs[0][1][n1:]), (other[0][n1:], other[1][n1:]), (pairs[2][0][n1:], pairs[2][1][n1:])], [tail])
        assert np.array_equal(got[0][0], refs[0][0][0][n1:]) and np.array_equal(got[2][0], refs[2][0][0][n1:])
        assert np.array_equal(got[1][0], fresh.push(other[0][n1:], other[1][n1:])[0])
        assert c.get(0) == refs[0][1].status(0) and c.get(2) == refs[2][1].status(0)
        want = fresh.status(0)
        want["samples"] += n1
        want["cells_solved"] += 3
        assert c.get(1) == want


# ------------------------------------------------------------------------------------------------------------------ (c)
TILE_OFFSETS = (2048, 1, 3, 4, 255, 256, 257, 1023, 1024, 1028, 2047, 2052, 3072, 4092, 4095)


@pytest.mark.parametrize("fmt", [dr.CS16, dr.CU8, dr.CF32], ids=["cs16", "cu8", "cf32"])
def test_block_and_cell_ends_everywhere_in_a_tile(nv, dv, fmt):
    """From a position set through the hook, call i starts 4096 + TILE_OFFSETS[i] samples in front of a cell's end: the end lies
    that many samples into the call's second tile -- in every wave, on and beside the edges of a lane's group, a step and a
    wave's region --, and the call's first block has as many samples less than a multiple of 256.  W = 1 and paths that change
    every 50 000 samples: every cell has another weight, so a sample given the wrong cell's weight shows; a sample added to the
    wrong block changes the sums and the solves behind them."""
    start = 5 * CELL - 4096 - TILE_OFFSETS[0]
    starts = [(5 + i) * CELL - 4096 - off for i, off in enumerate(TILE_OFFSETS)]
    cuts = [y - x for x, y in zip(starts, starts[1:])] + [4096 + TILE_OFFSETS[-1] + 5000]
    n = sum(cuts)
    steps = [STEPS[2], STEPS[3]]
    pairs = [dc.formatted_tones(n, 900 + fmt, steps, fmt), dc.extremes(fmt, n, 910 + fmt)[2]]
    refs = [dr.Combiner(fmt, 2, 0, start) for _ in pairs]
    want = []
    for ref, (a, b) in zip(refs, pairs):
        for k, step in enumerate(steps):
            ref.set_freq(k, step)
        want.append(ref.push(a, b))
    weights = [(h[1], h[2]) for h in refs[0].targets[0].history]
    assert refs[0].targets[0].first == 5 and len(weights) == len(TILE_OFFSETS) - 1 and all(x != y for x, y in zip(weights, weights[1:]))
    with _plan(dv, fmt, 2, steps, 0) as c:
        c.debug_set_position(start)
        got = _run_resident(nv, c, pairs, cuts)
        for s in range(2):
            _same(c, got, s, want[s], refs[s])


# ------------------------------------------------------------------------------------------------------------------ (d)
def test_a_lead_flip_and_reason_one_inside_one_call(nv, dv):
    """Both rows silent for two cells, then a tone whose stronger branch changes: in one call of eight cells at W = 1 the cell
    starts 1 and 2 are rejected with reason 1, and both leads occur behind them."""
    n = 8 * CELL + 300
    a, b = dc.silence_then_tone(n, 17, STEPS[2], 2 * CELL)
    want, ref = dr.combine(a, b, [STEPS[2]], dr.CS16, 0)
    hist = ref.targets[0].history
    assert [h[4] for h in hist] == [1, 1, 0, 0, 0, 0, 0, 0] and {h[1] for h in hist[2:]} == {0, 1} and ref.targets[0].rejected == 2
    with _plan(dv, dr.CS16, 1, [STEPS[2]], 0) as c:
        got = _run_resident(nv, c, [(a, b)], [n])
        _same(c, got, 0, want, ref)


# ------------------------------------------------------------------------------------------------------------------ (e)
@pytest.mark.parametrize("fmt", [dr.CS16, dr.CS8], ids=["cs16", "cs8"])
def test_four_targets_on_tones_and_on_full_scale_rows(nv, dv, fmt):
    """The steps 0, 2^32 / 512, a negative one and an arbitrary one from one read of the input, W = 2; the second pair is full-scale
    random (the largest block sums there are)."""
    n = 4 * CELL + 12345
    pairs = [dc.formatted_tones(n, 300 + fmt, STEPS, fmt), dc.extremes(fmt, n, 310 + fmt)[2], dc.extremes(fmt, n, 320 + fmt)[0]]
    refs = [dr.combine(a, b, STEPS, fmt, 1) for a, b in pairs]
    assert all(t.solved + t.rejected == 3 for _, ref in refs for t in ref.targets)
    with _plan(dv, fmt, 3, STEPS, 1) as c:
        got = _run_resident(nv, c, pairs, [CELL + 11, n - CELL - 11], out_first=3)
        for s in range(3):
            _same(c, got, s, refs[s][0], refs[s][1])


# ------------------------------------------------------------------------------------------------------------------ (f)
def test_set_freq_set_hold_and_back_to_track_between_calls(nv, dv):
    n = 9 * CELL
    a, b = dc.tones_pair(n, 90, [STEPS[1], STEPS[2]])
    ref = dr.Combiner(dr.CS16, 2, 0)
    with dv.Combiner(dr.CS16, n_targets=2, window_log2=0) as c:
        def both(f):
            f(c); f(ref)

        def step(k):
            got = _run_resident(nv, c, [(a[step.pos:step.pos + k], b[step.pos:step.pos + k])], [k])
            want = ref.push(a[step.pos:step.pos + k], b[step.pos:step.pos + k])
            _same(c, got, 0, want, ref, step.pos)
            step.pos += k
        step.pos = 0
        both(lambda x: x.set_freq(0, STEPS[1])); both(lambda x: x.set_freq(1, STEPS[3]))
        both(lambda x: x.set(0, 1, -3000, 4000))                           # in front of the first sample: held until cell 1
        assert c.get(0, 0) == ref.status(0) and c.get(0, 0)["weight"] == (-3000, 4000)
        step(CELL // 2)
        step(2 * CELL)                                                     # cells 1 and 2 start: solved
        assert ref.targets[0].solved == 2
        both(lambda x: x.set_freq(1, STEPS[2]))                            # in mid-cell: target 1 anew, its first counted cell is 3
        assert c.get(0, 1) == ref.status(1) and ref.targets[1].first == 3
        step(CELL + 100)
        both(lambda x: x.set_mode(0, dr.HOLD))
        held = ref.targets[0].w
        step(CELL)
        assert ref.targets[0].w == held and ref.targets[0].solved == 3 and ref.targets[1].solved == 3
        both(lambda x: x.set(0, 0, 32767, -32767))                         # a calibrated set-up: set and hold, at the limits
        both(lambda x: x.set(1, 1, 100, 100)); both(lambda x: x.set_freq(1, STEPS[2]))     # a set that a restart drops
        assert c.get(0, 1) == ref.status(1) and c.get(0, 1)["weight"] == (0, 0)
        step(CELL + 17)
        assert ref.targets[0].w == (32767, -32767)
        both(lambda x: x.set_mode(0, dr.TRACK))
        step(n - step.pos)
        assert ref.targets[0].solved == 6 and c.get(0, 0)["mode"] == dv.TRACK
        ARG = nv._native.ERR_ARG
        for bad in ((0, 32768, 0), (0, 0, 32768), (0, -32768, 0), (0, 0, -32768), (2, 0, 0), (-1, 0, 0)):
            assert dv.lib.nvx_div_set(c._h, 0, 0, *bad) == ARG
        assert dv.lib.nvx_div_set_mode(c._h, 0, 0, 2) == ARG and dv.lib.nvx_div_set_mode(c._h, 0, 0, -1) == ARG
        assert dv.lib.nvx_div_set_mode(c._h, 1, 0, 0) == ARG and dv.lib.nvx_div_set(c._h, 0, 2, 0, 0, 0) == ARG and dv.lib.nvx_div_set_freq(c._h, 0, 2, 5) == ARG
        assert c.get(0, 0) == ref.status(0) and c.get(0, 1) == ref.status(1)


# ------------------------------------------------------------------------------------------------------------------ (g)
@pytest.mark.parametrize("position", [2 ** 32 - 1000, 2 ** 40 + 5])
def test_positions_beyond_32_bits(nv, dv, position):
    """Three cells in two calls from the position, then a cell and a half more: the NCO's phase is that of the 64-bit index, and
    the cell the position lies in is not counted."""
    n, more = 3 * CELL, CELL + CELL // 2
    steps = [STEPS[2], STEPS[3]]
    pairs = [dc.tones_pair(n + more, 80 + s, steps) for s in range(2)]
    refs = [dr.Combiner(dr.CS16, 2, 0, position) for _ in pairs]
    for ref in refs:
        for k, step in enumerate(steps):
            ref.set_freq(k, step)
    with _plan(dv, dr.CS16, 2, steps, 0) as c:
        c.debug_set_position(position)
        assert c.position(1) == position
        got = _run_resident(nv, c, [(a[:n], b[:n]) for a, b in pairs], [CELL + 9000, n - CELL - 9000])
        for s in range(2):
            _same(c, got, s, refs[s].push(pairs[s][0][:n], pairs[s][1][:n]), refs[s])
        got = _run_resident(nv, c, [(a[n:], b[n:]) for a, b in pairs], [more])
        for s in range(2):
            _same(c, got, s, refs[s].push(pairs[s][0][n:], pairs[s][1][n:]), refs[s])
            assert refs[s].targets[0].solved >= 2


# ------------------------------------------------------------------------------------------------------------------ (h)
def test_scale_256_pairs(nv, dv):
    """256 pairs x 1 target x 2.2 cells of unsigned 8-bit samples, sixteen different pairs among them, every pair checked.  Below
    1024 pairs the launch arithmetic spreads a pair over chunks of at least 8 tiles."""
    ns, n, kinds = 256, int(2.2 * CELL) // 8 * 8, 16
    steps = [STEPS[2]]
    pairs = [dc.formatted_tones(n, 7000 + k, steps, dr.CU8) for k in range(kinds)]
    refs = [dr.combine(a, b, steps, dr.CU8, 0) for a, b in pairs]
    d_main = nv.DeviceBuffer(ns * n * 2); d_second = nv.DeviceBuffer(ns * n * 2); d_out = nv.DeviceBuffer(ns * n * 4)
    block_a, block_b = np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])
    for s in range(0, ns, kinds):
        d_main.upload(block_a, s * n * 2); d_second.upload(block_b, s * n * 2)
    with _plan(dv, dr.CU8, ns, steps, 0) as c:
        c.resident(d_main, n, d_second, n, n, d_out, n)
        shape = c.debug_last_launch()
        assert shape == {"launches": 3, "chunks": 5, "tiles_per_chunk": 8, "records": n // B + 1, "form": 2} and (n + 4095) // 4096 == 36
        got = d_out.download(ns * n * 4, dtype=np.int16).reshape(ns, n, 2)
        status = {s: c.get(s) for s in (0, 127, 255)}
    d_main.free(); d_second.free(); d_out.free()
    bad = [s for s in range(ns) if not np.array_equal(got[s], refs[s % kinds][0][0])]
    assert not bad, bad[:10]
    assert all(st == refs[s % kinds][1].status(0) for s, st in status.items()) and refs[0][1].targets[0].solved == 2


# ------------------------------------------------------------------------------------------------------------------ (i)
@pytest.mark.parametrize("fmt", [dr.CS16, dr.CS8], ids=["cs16", "cs8"])
def test_push_equals_resident(nv, dv, fmt):
    n = 2 * CELL + 3000
    steps = STEPS[2:4]
    pairs = [dc.formatted_tones(2 * n, 120 + s, steps, fmt) for s in range(3)]
    refs = [dr.combine(a, b, steps, fmt, 0) for a, b in pairs]
    with _plan(dv, fmt, 3, steps, 0) as c:
        for s, cuts in enumerate(([n], [1, CELL - 1, n - CELL], [7, 0, CELL + 5000, 1, n - CELL - 5008])):
            pos, parts = 0, []
            for cut in cuts:
                parts.append(c.push(s, pairs[s][0][pos:pos + cut], pairs[s][1][pos:pos + cut])); pos += cut
            out = np.concatenate(parts, axis=1)
            assert out.dtype == np.int16 and out.shape == (2, n, 2) and np.array_equal(out, refs[s][0][:, :n]), s
            assert c.position(s) == n
        got = _run_resident(nv, c, [(a[n:], b[n:]) for a, b in pairs], [n])
        for s in range(3):
            _same(c, got, s, refs[s][0][:, n:], refs[s][1])


# ------------------------------------------------------------------------------------------------------------------ (j)
def test_span_alignment_overlap_and_position_errors_launch_nothing(nv, dv):
    ARG = nv._native.ERR_ARG
    n = 8192
    with dv.Combiner(dr.CU8, n_pairs=2, n_targets=2) as c:
        d_a = nv.DeviceBuffer(2 * n * 2); d_b = nv.DeviceBuffer(2 * n * 2); d_out = nv.DeviceBuffer(4 * n * 4)
        one_in = nv.DeviceBuffer(n * 2); three_out = nv.DeviceBuffer(3 * n * 4)
        both = nv.DeviceBuffer(6 * n * 4)                                     # inputs and output in one allocation
        c.timing(True)
        call = lambda *a: dv.lib.nvx_div_resident(c._h, *a, None)            # noqa: E731
        A, Bp, O = d_a.ptr, d_b.ptr, d_out.ptr
        bad = {"more samples than the main pitch": (A, n - 8, Bp, n, n, O, n, 0),
               "more samples than the second pitch": (A, n, Bp, n - 8, n, O, n, 0),
               "words beyond the pitch": (A, n, Bp, n, n, O, n - 1, 0),
               "out_first pushes them beyond it": (A, n, Bp, n, n, O, n, 1),
               "main rows for one pair": (one_in.ptr, n, Bp, n, n, O, n, 0),
               "second rows for one pair": (A, n, one_in.ptr, n, n, O, n, 0),
               "output rows for three of the four": (A, n, Bp, n, n, three_out.ptr, n, 0),
               "misaligned main": (A + 4, n, Bp, n, n - 8, O, n, 0),
               "misaligned second": (A, n, Bp + 8, n, n - 8, O, n, 0),
               "misaligned output": (A, n, Bp, n, n, O + 2, n, 0),
               "main rows not 16-byte aligned": (A, n - 3, Bp, n, n - 8, O, n, 0),
               "second rows not 16-byte aligned": (A, n, Bp, n - 3, n - 8, O, n, 0),
               "null main": (None, n, Bp, n, n, O, n, 0),
               "null second": (A, n, None, n, n, O, n, 0),
               "null output": (A, n, Bp, n, n, None, n, 0),
               "too many samples": (A, 2 ** 31, Bp, 2 ** 31, 2 ** 30 + 1, O, 2 ** 31, 0),
               "a main pitch that wraps": (A, 2 ** 63, Bp, n, n, O, n, 0),
               "a second pitch that wraps": (A, n, Bp, 2 ** 63, n, O, n, 0),
               "an output pitch that wraps": (A, n, Bp, n, n, O, 2 ** 62, 0),
               "out_first that wraps": (A, n, Bp, n, n, O, n, 2 ** 64 - 8),
               "the output on the main rows": (both.ptr, n, Bp, n, n, both.ptr, n, 0),
               "the output on the second rows": (A, n, both.ptr, n, n, both.ptr, n, 0),
               "the output's first row on the main rows' last": (both.ptr, n, Bp, n, n, both.ptr, n, n - 8),
               "the main rows inside the output's span": (both.ptr + 2 * n * 4, n, Bp, n, n, both.ptr, 2 * n, 0)}
        for name, args in bad.items():
            assert call(*args) == ARG, name
            assert dv.lib.nvx_div_last_error() != b""
        assert b"overlaps" in dv.lib.nvx_div_last_error()
        c.debug_set_position(2 ** 62 - 100)
        assert call(A, n, Bp, n, n, O, n, 0) == ARG and b"2^62" in dv.lib.nvx_div_last_error()
        assert dv.lib.nvx_div_debug_set_position(c._h, 0, 2 ** 62) == ARG and dv.lib.nvx_div_debug_set_position(c._h, 2, 0) == ARG
        assert dv.lib.nvx_div_reset(c._h, 2) == ARG and dv.lib.nvx_div_get(c._h, -1, 0, None) == ARG and dv.lib.nvx_div_get(c._h, 0, 0, None) == ARG
        assert dv.lib.nvx_div_get(c._h, 0, 2, None) == ARG
        assert c.time_stats() == (0.0, 0) and c.debug_last_launch()["launches"] == 0 and c.position(0) == 2 ** 62 - 100
        c.reset()
        assert call(A, n, Bp, n, 0, O, n, 0) == 0 and c.debug_last_launch()["launches"] == 0       # nothing to do: no launch
        assert c.time_stats() == (0.0, 0)
        d_a.upload(np.full(2 * n * 2, 128, dtype=np.uint8)); d_b.upload(np.full(2 * n * 2, 128, dtype=np.uint8))
        assert call(A, n, Bp, n, n, O, n, 0) == 0
        # the output behind the inputs in one allocation, touching and not overlapping
        both.upload(np.full(6 * n * 4, 128, dtype=np.uint8))
        assert call(both.ptr, n, both.ptr + 2 * n * 2, n, n, both.ptr + 4 * n * 2, n, 0) == 0
        ms, calls = c.time_stats()
        assert calls == 2 and ms > 0.0 and c.debug_last_launch()["launches"] == 6 and c.get(1, 1)["samples"] == 2 * n
        for d in (d_a, d_b, d_out, one_in, three_out, both):
            d.free()
    for kw in (dict(device=99), dict(window_log2=3), dict(window_log2=6), dict(format=4), dict(n_pairs=0), dict(n_targets=5)):
        with pytest.raises(nv.NvxError) as e:
            dv.Combiner(**kw)
        assert e.value.code == ARG, kw


# ------------------------------------------------------------------------------------------------------------------ (k)
def test_seed_11_of_the_acceptance_case_on_the_device(nv, dv, oracle):
    """The pair of seed 11 through the combiner on the device: the words are the CPU's.  Then the main and the combined row as two
    streams of a two-chain handle: the 490 message arrives from the combined row and not from the main row, and the bits of
    all four chains are the oracle's on the same words."""
    t490 = dc.text()
    a, b = dc.fading_pair(nv, 11)
    n = len(a)
    want, ref = dr.combine(a, b, [dc.STEP_490])
    d_rows = nv.DeviceBuffer(2 * n * 4); d_second = nv.DeviceBuffer(n * 4)
    d_rows.upload(a); d_second.upload(b)
    with _plan(dv, dr.CS16, 1, [dc.STEP_490], 2) as c:
        # the combined row goes behind the main row: row 1 of the handle's input
        c.resident(d_rows, n, d_second, n, n, d_rows, n, out_first=n)
        got = d_rows.download(2 * n * 4, dtype=np.int16).reshape(2, n, 2)
        assert np.array_equal(got[0], a) and np.array_equal(got[1], want[0]), _first_difference(got[1], want[0])
        assert c.get(0) == ref.status(0) and ref.targets[0].solved == n // CELL - 3 and ref.targets[0].rejected == 0
    frames = n // nv.FRAME_IN
    with nv.Pipeline(n_streams=2, chain_mask=nv.CHAIN_518 | nv.CHAIN_490, max_frames=8) as p:
        for f0 in range(0, frames, 8):
            p.process_resident(d_rows, n, f0, min(8, frames - f0), hip_stream=p.hip_stream)
        p.fetch()
        bits = [(p.bits(s, 0), p.bits(s, 1)) for s in range(2)]
        msgs = [[m[3] for m in p.messages if m[0] == s and m[1] == 490] for s in range(2)]
    d_rows.free(); d_second.free()
    cpu = [dc.delivered(oracle, row, nv.FRAME_IN) for row in (a, want[0])]
    for s in range(2):
        assert bits[s] == cpu[s][1] and msgs[s] == cpu[s][0], s
    assert msgs[1] == [t490] and msgs[0] != [t490]
