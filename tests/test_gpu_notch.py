"""The tone notch (include/navtex_amd_notch.h) on the GPU (-m gpu): output words equal to the restatement (tests/notch_ref.py)
for rows of several notches in every format, one shot against calls cut at and next to the block and tile ends, a reset row
rejoining the others, the rails and full-scale random input (float32 specials), the longest ring and delay line, set_freq /
disable / enable / measure / refine between calls, positions beyond 2^32, push against resident, 256 rows with the launch's
shape pinned, the calls that are refused before anything is launched, and the acceptance case's seed 11 through a two-chain
handle.  Every comparison is ==, with sentinels around every output row, and the input is full scale behind the samples of a
call.  R = 4 (D = 1280) unless said."""
from pathlib import Path

import numpy as np
import pytest

import notch_cases as nc
import notch_ref as nr

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FORMATS = (nr.CS16, nr.CU8, nr.CS8, nr.CF32)
FORMAT_IDS = ("cs16", "cu8", "cs8", "cf32")
SENTINEL = 0x5a5a1234
B = nr.BLOCK
R4 = 2                                      # width_log2 of R = 4


@pytest.fixture(scope="module")
def nt(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_notch.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.notch
    return navtex_amd.notch


def _run_resident(nv, c, rows, cuts, pitch_extra=0, out_first=0):
    """The rows ([n, 2] each, all of one length) through nvx_notch_resident in calls of `cuts` samples; every call's input is
    uploaded to the start of the input rows as whole rows: behind a call's n_in samples a row is full scale up to the pitch, so
    a read behind n_in changes the output and the sums.  Sentinels around every output row.  Returns int16 [rows, n, 2]."""
    ns, n = len(rows), len(rows[0])
    assert sum(cuts) == n and ns == c.n_rows
    dt = rows[0].dtype
    bps = dt.itemsize * 2
    pitch_out = out_first + n + pitch_extra
    pitch_in = (max(max(cuts), 1) + 7) // 8 * 8 + 8 * (pitch_extra + 1)
    d_in = nv.DeviceBuffer(ns * pitch_in * bps)
    d_out = nv.DeviceBuffer(ns * pitch_out * 4)
    d_out.upload(np.full(ns * pitch_out, SENTINEL, dtype=np.uint32))
    block = np.empty((ns, pitch_in, 2), dtype=dt)
    full = 1.0 if dt == np.float32 else np.iinfo(dt).max
    start = c.position(0)
    pos = 0
    for cut in cuts:
        block[:, cut:] = full
        for s in range(ns):
            block[s, :cut] = rows[s][pos:pos + cut]
        d_in.upload(block)
        c.resident(d_in, pitch_in, cut, d_out, pitch_out, out_first + pos)
        pos += cut
    assert c.position(ns - 1) == start + n
    words = d_out.download(ns * pitch_out * 4, dtype=np.uint32).reshape(ns, pitch_out)
    d_in.free(); d_out.free()
    assert np.all(words[:, :out_first] == SENTINEL) and np.all(words[:, out_first + n:] == SENTINEL), "words outside the span were written"
    return np.ascontiguousarray(words[:, out_first:out_first + n]).view(np.int16).reshape(ns, n, 2)


def _first_difference(got, want):
    return int(np.argmax(np.any(got != want, axis=1)))


def _set(c, ref, row, steps, disabled=()):
    """The same steps and flags on the device's row and on its restatement."""
    for k, step in enumerate(steps):
        c.set_freq(k, step, row=row); ref.set_freq(k, step)
        c.enable(k, k not in disabled, row=row); ref.enable(k, k not in disabled)


def _same(c, refs):
    for s, ref in enumerate(refs):
        for k in range(len(ref.tones)):
            assert c.get(k, s) == ref.get(k), (s, k)


# ------------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_three_rows_of_four_notches_in_every_format(nv, nt, fmt):
    """Each row with other steps and another notch disabled; out_first = 7 (the unaligned stores) and 8."""
    n = 20000
    made = [nc.busy_row(n, 300 + 10 * fmt + s, fmt) for s in range(3)]
    for out_first in (7, 8):
        refs = [nr.Notch(fmt, 4, R4) for _ in made]
        with nt.Notch(fmt, n_rows=3, n_notches=4, width_log2=R4) as c:
            assert c.delay() == 1280 == refs[0].delay()
            for s, (_, steps) in enumerate(made):
                _set(c, refs[s], s, steps, disabled=(3 - s,))
            got = _run_resident(nv, c, [row for row, _ in made], [n], pitch_extra=3 + out_first % 2, out_first=out_first)
            for s, (row, _) in enumerate(made):
                want = refs[s].push(row)
                assert np.array_equal(got[s], want), (out_first, s, _first_difference(got[s], want))
                assert want[1280 + 8 * B:].any() and not np.array_equal(want[1280:], row[:n - 1280])
            _same(c, refs)
            assert refs[0].get(0)["pairs"] == n // B - 2 * 4 + 1


# ------------------------------------------------------------------------------------------------------------------ (b)
def test_one_shot_equals_calls_cut_at_the_block_and_tile_ends_and_a_reset_row_rejoins(nv, nt):
    cuts = [257, 1, 0, 255, 256, 4095, 4097]
    n1 = 24000
    cuts = cuts + [n1 - sum(cuts)]
    tail = 3000
    made = [nc.busy_row(n1 + tail, 400 + s) for s in range(3)]
    refs = [nr.Notch(nr.CS16, 4, R4) for _ in made]
    with nt.Notch(nr.CS16, n_rows=3, n_notches=4, width_log2=R4) as c:
        for s, (_, steps) in enumerate(made):
            _set(c, refs[s], s, steps)
        wants = [ref.push(row) for ref, (row, _) in zip(refs, made)]            # one shot
        got = _run_resident(nv, c, [row[:n1] for row, _ in made], cuts)
        for s in range(3):
            assert np.array_equal(got[s], wants[s][:n1]), (s, _first_difference(got[s], wants[s][:n1]))
        c.reset(1)
        assert c.position(1) == 0 and c.position(0) == n1 and c.get(0, 1)["x"] == (0, 0) and c.get(0, 1)["pairs"] == 0
        d = nv.DeviceBuffer(3 * 64 * 4); o = nv.DeviceBuffer(3 * 64 * 4)
        assert nt.lib.nvx_notch_resident(c._h, d.ptr, 64, 64, o.ptr, 64, 0, None) == nv._native.ERR_STATE
        assert b"same position" in nt.lib.nvx_notch_last_error()
        d.free(); o.free()
        # row 1 starts anew on other data, alone and in calls of its own (the first of one sample), up to where the others stand
        other, steps = nc.busy_row(n1 + tail, 450)
        fresh = nr.Notch(nr.CS16, 4, R4)
        fresh.samples = n1                                                 # the row's counter runs on through a reset
        for k, step in enumerate(made[1][1]):
            fresh.set_freq(k, step); fresh.enable(k)
        pos = 0
        for cut in (1, 700, 1279, 5, n1 - 1985):
            assert np.array_equal(c.push(1, other[pos:pos + cut]), fresh.push(other[pos:pos + cut])), pos
            pos += cut
        assert c.position(1) == n1
        got = _run_resident(nv, c, [made[0][0][n1:], other[n1:], made[2][0][n1:]], [tail])
        assert np.array_equal(got[0], wants[0][n1:]) and np.array_equal(got[2], wants[2][n1:])
        assert np.array_equal(got[1], fresh.push(other[n1:]))
        _same(c, [refs[0], fresh, refs[2]])
        assert c.get(0, 1)["samples"] == 2 * n1 + tail


# ------------------------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_the_rails_and_full_scale_random_input(nv, nt, fmt):
    """The rails notched at 0 Hz (every product at its largest: the amplitude at 2^20 and a c at 2^35) and at a step that turns,
    and full-scale random rows."""
    n = 12000
    rows = [nc.rails(fmt, n), nc.rails(fmt, n), nc.full_scale(fmt, n, 500 + fmt)]
    steps = [[0, 0x40000000], [123456789, 0xfffff000], [0x12345678, 0x9abcdef0]]
    refs = [nr.Notch(fmt, 2, R4) for _ in rows]
    with nt.Notch(fmt, n_rows=3, n_notches=2, width_log2=R4) as c:
        for s in range(3):
            _set(c, refs[s], s, steps[s])
        got = _run_resident(nv, c, rows, [5000, n - 5000], out_first=3)
        for s in range(3):
            want = refs[s].push(rows[s])
            assert np.array_equal(got[s], want), (s, _first_difference(got[s], want))
        _same(c, refs)


# ------------------------------------------------------------------------------------------------------------------ (d)
def test_the_longest_ring_and_delay_line(nv, nt):
    """R = 64: D = 16640, 130 carried block sums per notch; 60 000 samples in three ragged calls."""
    n = 60000
    row, steps = nc.busy_row(n, 600, k=2)
    ref = nr.Notch(nr.CS16, 2, 6)
    with nt.Notch(nr.CS16, n_notches=2, width_log2=6) as c:
        assert c.delay() == 16640
        _set(c, ref, 0, steps)
        got = _run_resident(nv, c, [row], [16001, 27002, n - 43003])
        want = ref.push(row)
        assert np.array_equal(got[0], want), _first_difference(got[0], want)
        _same(c, [ref])
        assert ref.get(0)["pairs"] == n // B - 2 * 64 + 1


# ------------------------------------------------------------------------------------------------------------------ (e)
def test_set_freq_disable_enable_measure_and_refine_between_calls(nv, nt):
    n = 40000
    row, steps = nc.busy_row(n, 700, k=2)
    ref = nr.Notch(nr.CS16, 2, R4)
    with nt.Notch(nr.CS16, n_notches=2, width_log2=R4) as c:
        def step(k):
            got = _run_resident(nv, c, [row[step.pos:step.pos + k]], [k])
            want = ref.push(row[step.pos:step.pos + k])
            assert np.array_equal(got[0], want), (step.pos, _first_difference(got[0], want))
            _same(c, [ref])
            step.pos += k
        step.pos = 0
        step(3000)                                                         # nothing enabled: the delayed conversion
        _set(c, ref, 0, steps)
        step(5001)
        c.enable(1, False); ref.enable(1, False)
        step(2999)
        c.measure(0); ref.measure(0)
        assert c.get(0)["pairs"] == 0 and c.get(0)["x"] == (0, 0)
        step(7000)
        assert 0 < ref.get(0)["pairs"] < 7000 // B
        c.enable(1); ref.enable(1)
        c.set_freq(0, steps[0] + 5000); ref.set_freq(0, steps[0] + 5000)
        step(6000)
        # the first notch sits 3 Hz above its carrier: the readout points back down, the host's arithmetic to the step
        new = c.refine(0)
        assert abs(new - ref.refine(0)) <= 1 and new != steps[0] + 5000
        ref.set_freq(0, new)
        assert c.get(0)["step"] == new and c.get(0)["pairs"] == 0
        step(n - step.pos)
        ARG = nv._native.ERR_ARG
        assert nt.lib.nvx_notch_set_freq(c._h, 0, 2, 1) == ARG and nt.lib.nvx_notch_set_freq(c._h, 1, 0, 1) == ARG
        assert nt.lib.nvx_notch_enable(c._h, 0, -1, 1) == ARG and nt.lib.nvx_notch_measure(c._h, -2, 0) == ARG
        assert nt.lib.nvx_notch_refine(c._h, -1, 0, None) == ARG and nt.lib.nvx_notch_get(c._h, 0, 0, None) == ARG


# ------------------------------------------------------------------------------------------------------------------ (f)
@pytest.mark.parametrize("position", [2 ** 32 - 1000, 2 ** 40 + 5])
def test_positions_beyond_32_bits(nv, nt, position):
    """The block the position lies in sums only what it received, the words in front of the position are zero, and the phase
    wraps at 2^32 inside the first call."""
    n, more = 9000, 4000
    made = [nc.busy_row(n + more, 80 + s, k=2) for s in range(2)]
    refs = [nr.Notch(nr.CS16, 2, R4, position) for _ in made]
    with nt.Notch(nr.CS16, n_rows=2, n_notches=2, width_log2=R4) as c:
        c.debug_set_position(position)
        assert c.position(1) == position
        for s, (_, steps) in enumerate(made):
            _set(c, refs[s], s, steps)
        got = _run_resident(nv, c, [row[:n] for row, _ in made], [2345, n - 2345])
        for s in range(2):
            want = refs[s].push(made[s][0][:n])
            assert np.array_equal(got[s], want), (s, _first_difference(got[s], want))
            assert not want[:1280].any() and want[1280:].any()
        got = _run_resident(nv, c, [row[n:] for row, _ in made], [more])
        for s in range(2):
            want = refs[s].push(made[s][0][n:])
            assert np.array_equal(got[s], want), (s, _first_difference(got[s], want))
        _same(c, refs)


# ------------------------------------------------------------------------------------------------------------------ (g)
@pytest.mark.parametrize("fmt", [nr.CS16, nr.CS8], ids=["cs16", "cs8"])
def test_push_equals_resident(nv, nt, fmt):
    n = 9000
    made = [nc.busy_row(2 * n, 120 + s, fmt, k=2) for s in range(3)]
    refs = [nr.Notch(fmt, 2, R4) for _ in made]
    with nt.Notch(fmt, n_rows=3, n_notches=2, width_log2=R4) as c:
        for s, (_, steps) in enumerate(made):
            _set(c, refs[s], s, steps)
        wants = [ref.push(row) for ref, (row, _) in zip(refs, made)]
        for s, cuts in enumerate(([n], [1, B - 1, n - B], [7, 0, 1273, 1, n - 1281])):
            pos, parts = 0, []
            for cut in cuts:
                parts.append(c.push(s, made[s][0][pos:pos + cut])); pos += cut
            out = np.concatenate(parts)
            assert out.dtype == np.int16 and np.array_equal(out, wants[s][:n]), (s, _first_difference(out, wants[s][:n]))
            assert c.position(s) == n
        got = _run_resident(nv, c, [row[n:] for row, _ in made], [n])
        for s in range(3):
            assert np.array_equal(got[s], wants[s][n:]), s
        _same(c, refs)


# ------------------------------------------------------------------------------------------------------------------ (h)
def test_scale_256_rows(nv, nt):
    """256 rows x 40 000 unsigned 8-bit samples, sixteen different rows among them, every row checked.  Ten tiles a row, which
    the launch arithmetic spreads over two workgroups (below 1024 rows it aims at 2048 workgroups, in chunks of at least eight
    tiles)."""
    ns, n, kinds = 256, 40000, 16
    made = [nc.busy_row(n, 7000 + k, nr.CU8, k=2) for k in range(kinds)]
    refs = [nr.Notch(nr.CU8, 2, R4) for _ in made]
    d_in = nv.DeviceBuffer(ns * n * 2); d_out = nv.DeviceBuffer(ns * n * 4)
    block = np.stack([row for row, _ in made])
    for s in range(0, ns, kinds):
        d_in.upload(block, s * n * 2)
    with nt.Notch(nr.CU8, n_rows=ns, n_notches=2, width_log2=R4) as c:
        for s in range(ns):
            for k, st in enumerate(made[s % kinds][1]):
                c.set_freq(k, st, row=s); c.enable(k, row=s)
        c.resident(d_in, n, n, d_out, n)
        assert c.debug_last_launch() == {"launches": 3, "chunks": 2, "tiles_per_chunk": 8, "records": 157, "form": 2}
        got = d_out.download(ns * n * 4, dtype=np.int16).reshape(ns, n, 2)
        status = {s: [c.get(k, s) for k in range(2)] for s in (0, 127, 255)}
    d_in.free(); d_out.free()
    wants = []
    for ref, (row, steps) in zip(refs, made):
        for k, st in enumerate(steps):
            ref.set_freq(k, st); ref.enable(k)
        wants.append(ref.push(row))
    bad = [s for s in range(ns) if not np.array_equal(got[s], wants[s % kinds])]
    assert not bad, bad[:10]
    assert all(st == [refs[s % kinds].get(k) for k in range(2)] for s, st in status.items())


# ------------------------------------------------------------------------------------------------------------------ (i)
def test_span_alignment_overlap_and_position_errors_launch_nothing(nv, nt):
    ARG = nv._native.ERR_ARG
    n = 8192
    with nt.Notch(nr.CU8, n_rows=2) as c:
        d_a = nv.DeviceBuffer(2 * n * 2); d_out = nv.DeviceBuffer(2 * n * 4)
        one_in = nv.DeviceBuffer(n * 2); one_out = nv.DeviceBuffer(n * 4)
        both = nv.DeviceBuffer(4 * n * 4)                                     # input and output in one allocation
        c.timing(True)
        call = lambda *a: nt.lib.nvx_notch_resident(c._h, *a, None)          # noqa: E731
        A, O = d_a.ptr, d_out.ptr
        bad = {"more samples than the pitch": (A, n - 8, n, O, n, 0),
               "words beyond the pitch": (A, n, n, O, n - 1, 0),
               "out_first pushes them beyond it": (A, n, n, O, n, 1),
               "input rows for one row": (one_in.ptr, n, n, O, n, 0),
               "output rows for one row": (A, n, n, one_out.ptr, n, 0),
               "misaligned input": (A + 4, n, n - 8, O, n, 0),
               "misaligned output": (A, n, n, O + 2, n, 0),
               "input rows not 16-byte aligned": (A, n - 3, n - 8, O, n, 0),
               "null input": (None, n, n, O, n, 0),
               "null output": (A, n, n, None, n, 0),
               "too many samples": (A, 2 ** 31, 2 ** 30 + 1, O, 2 ** 31, 0),
               "an input pitch that wraps": (A, 2 ** 63, n, O, n, 0),
               "an output pitch that wraps": (A, n, n, O, 2 ** 62, 0),
               "out_first that wraps": (A, n, n, O, n, 2 ** 64 - 8),
               "the output on the input": (both.ptr, n, n, both.ptr, n, 0),
               "the output's first row on the input's last": (both.ptr, n, n, both.ptr, n, n - 8),
               "the input inside the output's span": (both.ptr + 2 * n * 4, n, n, both.ptr, 2 * n, 0)}
        for name, args in bad.items():
            assert call(*args) == ARG, name
            assert nt.lib.nvx_notch_last_error() != b""
        assert b"overlaps" in nt.lib.nvx_notch_last_error()
        c.debug_set_position(2 ** 62 - 100)
        assert call(A, n, n, O, n, 0) == ARG and b"2^62" in nt.lib.nvx_notch_last_error()
        assert nt.lib.nvx_notch_debug_set_position(c._h, 0, 2 ** 62) == ARG and nt.lib.nvx_notch_debug_set_position(c._h, 2, 0) == ARG
        assert nt.lib.nvx_notch_reset(c._h, 2) == ARG and nt.lib.nvx_notch_get(c._h, -1, 0, None) == ARG
        assert c.time_stats() == (0.0, 0) and c.debug_last_launch()["launches"] == 0 and c.position(0) == 2 ** 62 - 100
        c.reset()
        assert call(A, n, 0, O, n, 0) == 0 and c.debug_last_launch()["launches"] == 0         # nothing to do: no launch
        assert c.time_stats() == (0.0, 0)
        d_a.upload(np.full(2 * n * 2, 128, dtype=np.uint8))
        assert call(A, n, n, O, n, 0) == 0
        # the output behind the input in one allocation, touching and not overlapping
        both.upload(np.full(4 * n * 4, 128, dtype=np.uint8))
        assert call(both.ptr, n, n, both.ptr + 2 * n * 2, n, 0) == 0
        ms, calls = c.time_stats()
        assert calls == 2 and ms > 0.0 and c.debug_last_launch()["launches"] == 6 and c.get(0, 1)["samples"] == 2 * n
        for d in (d_a, d_out, one_in, one_out, both):
            d.free()
    for kw in (dict(device=99), dict(width_log2=1), dict(width_log2=7), dict(format=4), dict(n_rows=0), dict(n_notches=0), dict(n_notches=5)):
        with pytest.raises(nv.NvxError) as e:
            nt.Notch(**kw)
        assert e.value.code == ARG, kw


# ------------------------------------------------------------------------------------------------------------------ (j)
def test_seed_11_of_the_acceptance_case_on_the_device(nv, nt, oracle):
    """The row of seed 11 through two notches 1 Hz off at R = 32 on the device: the words are the CPU's.  Then the plain and the
    notched row as two streams of a two-chain handle: the 490 message arrives from the notched row and not from the plain row,
    and the bits of all four chains are the oracle's on the same words."""
    t490 = nc.text()
    a = nc.acceptance_row(nv, 11)
    n = len(a)
    want, ref = nr.notch(a, nc.steps(1.0), width_log2=5)
    d_rows = nv.DeviceBuffer(2 * n * 4)
    d_rows.upload(a)
    with nt.Notch(nr.CS16, n_notches=2, width_log2=5) as c:
        for k, step in enumerate(nc.steps(1.0)):
            c.set_freq(k, step); c.enable(k)
        # the notched row goes behind the plain row: row 1 of the handle's input
        c.resident(d_rows, n, n, d_rows, n, out_first=n)
        got = d_rows.download(2 * n * 4, dtype=np.int16).reshape(2, n, 2)
        assert np.array_equal(got[0], a) and np.array_equal(got[1], want), _first_difference(got[1], want)
        _same(c, [ref])
        assert ref.get(0)["pairs"] == nr.MAX_PAIRS
    frames = n // nv.FRAME_IN
    with nv.Pipeline(n_streams=2, chain_mask=nv.CHAIN_518 | nv.CHAIN_490, max_frames=8) as p:
        for f0 in range(0, frames, 8):
            p.process_resident(d_rows, n, f0, min(8, frames - f0), hip_stream=p.hip_stream)
        p.fetch()
        bits = [(p.bits(s, 0), p.bits(s, 1)) for s in range(2)]
        msgs = [[m[3] for m in p.messages if m[0] == s and m[1] == 490] for s in range(2)]
    d_rows.free()
    cpu = [nc.delivered(oracle, row, nv.FRAME_IN) for row in (a, want)]
    for s in range(2):
        assert bits[s] == cpu[s][1] and msgs[s] == cpu[s][0], s
    assert msgs[1] == [t490] and msgs[0] != [t490]
