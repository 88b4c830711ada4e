"""The spectrum monitor (include/navtex_amd_spec.h) on the GPU (-m gpu): level words and surveys equal to the restatement
(tests/spec_ref.py) for rows in every format with many lines to a call, one shot against calls cut at and next to H, N and a
line's hop with a reset row rejoining, N = 4096 (the new table), A = 1, zeros and the rails, measure between calls, positions
beyond 2^32, push against resident, a call in several batches, 256 rows with the launch's shape pinned, the calls that are
refused before anything is launched, and the acceptance case's seed 11: the device's survey, its two steps into the notch on
the device, and the plain and notched rows through a two-chain handle.  Every comparison is ==, with sentinels around every
output row, and the input is full scale behind the samples of a call."""
from pathlib import Path

import numpy as np
import pytest

import spec_cases as sc
import spec_ref as sr

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FORMATS = (sr.CS16, sr.CU8, sr.CS8, sr.CF32)
FORMAT_IDS = ("cs16", "cu8", "cs8", "cf32")
SENTINEL = 0xa5c3
GUARD = 64                                  # level words of sentinel in front of and behind the output: 128 bytes


@pytest.fixture(scope="module")
def sp(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_spec.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.spec
    return navtex_amd.spec


def _run_resident(nv, sp, c, rows, cuts, pitch_extra=0, spare_lines=1, levels=True):
    """The rows ([n, 2] each, all of one length) through nvx_spec_resident in calls of `cuts` samples; every call's input is
    uploaded to the start of the input rows as whole rows: behind a call's n_in samples a row is full scale up to the pitch, so
    a read behind n_in changes the lines.  The level words of a call go to [rows][line_cap][N] with line_cap `spare_lines`
    above what the call completes, sentinels in the spare lines and around the whole.  Returns uint16 [rows, lines, N]."""
    ns, n, N = len(rows), len(rows[0]), c.n
    assert sum(cuts) == n and ns == c.n_rows
    dt = rows[0].dtype
    bps = dt.itemsize * 2
    pitch_in = (max(max(cuts), 1) + 7) // 8 * 8 + 8 * (pitch_extra + 1)
    d_in = nv.DeviceBuffer(ns * pitch_in * bps)
    block = np.empty((ns, pitch_in, 2), dtype=dt)
    full = 1.0 if dt == np.float32 else np.iinfo(dt).max
    start = c.position(0)
    pos, parts = 0, [[] for _ in rows]
    for cut in cuts:
        block[:, cut:] = full
        for s in range(ns):
            block[s, :cut] = rows[s][pos:pos + cut]
        d_in.upload(block)
        lines = c.lines_for(cut)
        cap = lines + spare_lines
        words = 2 * GUARD + ns * cap * N
        d_lv = nv.DeviceBuffer(words * 2)
        d_lv.upload(np.full(words, SENTINEL, dtype=np.uint16))
        got = sp.lib.nvx_spec_resident(c._h, d_in.ptr, pitch_in, cut, d_lv.ptr + 2 * GUARD if levels else None, cap, None)
        assert got == lines, (got, lines, sp.lib.nvx_spec_last_error())
        out = d_lv.download(words * 2, dtype=np.uint16)
        d_lv.free()
        assert np.all(out[:GUARD] == SENTINEL) and np.all(out[-GUARD:] == SENTINEL), "words outside the level words were written"
        out = out[GUARD:-GUARD].reshape(ns, cap, N)
        assert np.all(out[:, lines if levels else 0:] == SENTINEL), "lines the call did not complete were written"
        for s in range(ns):
            parts[s].append(out[s, :lines].copy())
        pos += cut
    assert c.position(ns - 1) == start + n
    d_in.free()
    return [np.concatenate(p) for p in parts]


def _same_survey(c, refs, rows=None):
    for s, ref in enumerate(refs):
        row = s if rows is None else rows[s]
        p, re, im, lines = c.get(row)
        assert lines == ref.lines, (row, lines, ref.lines)
        assert np.array_equal(p, ref.sp) and np.array_equal(re, ref.sc_re) and np.array_equal(im, ref.sc_im), row


def _first_difference(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.argwhere(got != want)[:1].tolist()


# ------------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_three_rows_of_forty_lines_in_every_format(nv, sp, fmt):
    """N = 256, A = 2: forty workgroups a row in one call, so the fold's order matters; pitches larger than the data."""
    n = 39 * 256 + 384 + 50
    rows = [sc.busy(n, 300 + 10 * fmt + s, fmt) for s in range(3)]
    refs = [sr.Spectrum(fmt, 8, 2) for _ in rows]
    with sp.Spectrum(fmt, n_rows=3, n_log2=8, avg=2) as c:
        got = _run_resident(nv, sp, c, rows, [n], pitch_extra=3, spare_lines=2)
        for s, row in enumerate(rows):
            want = refs[s].push(row)
            assert want.shape == (40, 256) and np.array_equal(got[s], want), (s, _first_difference(got[s], want))
        _same_survey(c, refs)
        assert refs[0].lines == 40 and refs[0].sc_re.any() and len(refs[0].find_lines()) == len(c.find_lines(0)) >= 1


# ------------------------------------------------------------------------------------------------------------------ (b)
def test_one_shot_equals_calls_cut_at_h_n_and_a_hop_and_a_reset_row_rejoins(nv, sp):
    n_log2, avg = 9, 3
    N, H = 512, 256
    hop = avg * H
    cuts = [H - 1, 1, 0, N, hop + 1]
    n1 = 12 * hop + 100
    cuts = cuts + [n1 - sum(cuts)]
    tail = 3 * hop
    rows = [sc.busy(n1 + tail, 400 + s) for s in range(3)]
    refs = [sr.Spectrum(sr.CS16, n_log2, avg) for _ in rows]
    with sp.Spectrum(sr.CS16, n_rows=3, n_log2=n_log2, avg=avg) as c:
        wants = [ref.push(row) for ref, row in zip(refs, rows)]                 # one shot
        got = _run_resident(nv, sp, c, [row[:n1] for row in rows], cuts)
        k1 = sr.lines_at(n1, n_log2, avg)
        for s in range(3):
            assert np.array_equal(got[s], wants[s][:k1]), (s, _first_difference(got[s], wants[s][:k1]))
        c.reset(1)
        assert c.position(1) == 0 and c.position(0) == n1 and c.get(1)[3] == 0 and not c.get(1)[0].any()
        d = nv.DeviceBuffer(3 * 64 * 4)
        assert sp.lib.nvx_spec_resident(c._h, d.ptr, 64, 64, None, 0, None) == nv._native.ERR_STATE
        assert b"same position" in sp.lib.nvx_spec_last_error()
        d.free()
        # row 1 starts anew on other data, alone and in calls of its own (the first of one sample), up to where the others stand
        other = sc.busy(n1 + tail, 450)
        fresh = sr.Spectrum(sr.CS16, n_log2, avg)
        pos = 0
        for cut in (1, 700, N - 1, 5, n1 - 705 - N):
            assert np.array_equal(c.push(1, other[pos:pos + cut]), fresh.push(other[pos:pos + cut])), pos
            pos += cut
        assert c.position(1) == n1
        got = _run_resident(nv, sp, c, [rows[0][n1:], other[n1:], rows[2][n1:]], [tail])
        assert np.array_equal(got[0], wants[0][k1:]) and np.array_equal(got[2], wants[2][k1:])
        assert np.array_equal(got[1], fresh.push(other[n1:]))
        _same_survey(c, [refs[0], fresh, refs[2]])


# ------------------------------------------------------------------------------------------------------------------ (c)
def test_n_4096_reads_the_new_table(nv, sp):
    n_log2, avg = 12, 3
    n = 4 * avg * 2048 + 4 * 2048 + 33
    row = sc.busy(n, 500)
    ref = sr.Spectrum(sr.CS16, n_log2, avg)
    with sp.Spectrum(sr.CS16, n_log2=n_log2, avg=avg) as c:
        got = _run_resident(nv, sp, c, [row], [5000, n - 5000])
        want = ref.push(row)
        assert want.shape == (5, 4096) and np.array_equal(got[0], want), _first_difference(got[0], want)
        _same_survey(c, [ref])


# ------------------------------------------------------------------------------------------------------------------ (d)
def test_a_of_one_has_no_lag_products_and_the_finder_refuses(nv, sp):
    n = 6 * 1024 + 1024 + 9
    row = sc.busy(n, 600)
    ref = sr.Spectrum(sr.CS16, 11, 1)
    with sp.Spectrum(sr.CS16, n_log2=11, avg=1) as c:
        got = _run_resident(nv, sp, c, [row], [n])
        want = ref.push(row)
        assert want.shape == (6, 2048) and np.array_equal(got[0], want), _first_difference(got[0], want)
        _same_survey(c, [ref])
        p, re, im, lines = c.get()
        assert lines == 6 and p.any() and not re.any() and not im.any()
        with pytest.raises(sp.SpecError) as e:
            c.find_lines(min_lines=1)
        assert e.value.code == nv._native.ERR_ARG


# ------------------------------------------------------------------------------------------------------------------ (e)
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_zeros_and_the_rails(nv, sp, fmt):
    """Silence gives level 0 in every word (CU8 has no silence: its row is the format's lowest value like the rails); the
    rails and full-scale random rows (float32: the specials of the conversion) are the restatement's."""
    n = 9 * 256 + 384 + 3
    rows = [sc.zeros(fmt, n) if fmt != sr.CU8 else sc.rails(fmt, n), sc.rails(fmt, n), sc.full_scale(fmt, n, 700 + fmt)]
    refs = [sr.Spectrum(fmt, 8, 2) for _ in rows]
    with sp.Spectrum(fmt, n_rows=3, n_log2=8, avg=2) as c:
        got = _run_resident(nv, sp, c, rows, [1000, n - 1000])
        for s, row in enumerate(rows):
            want = refs[s].push(row)
            assert np.array_equal(got[s], want), (s, _first_difference(got[s], want))
        amp = float(abs(sr.rr.convert(rows[1][:1], fmt)[0, 0]))             # the format's lowest value, converted
        if fmt != sr.CU8:
            assert got[0].shape == (10, 256) and not got[0].any() and not c.get(0)[0].any()
        assert got[1][0, 128] == got[1].max() and abs(sr.level_db(got[1][0, 128]) - 10 * np.log10(2 * 2.0 * (amp * 128) ** 2)) < 0.2591 + 2 * 0.0118
        _same_survey(c, refs)


# ------------------------------------------------------------------------------------------------------------------ (f)
def test_measure_between_calls(nv, sp):
    n_log2, avg = 8, 3
    hop = avg * 128
    row = sc.busy(30 * hop, 800)
    ref = sr.Spectrum(sr.CS16, n_log2, avg)
    with sp.Spectrum(sr.CS16, n_log2=n_log2, avg=avg) as c:
        def step(k):
            got = _run_resident(nv, sp, c, [row[step.pos:step.pos + k]], [k])
            want = ref.push(row[step.pos:step.pos + k])
            assert np.array_equal(got[0], want), (step.pos, _first_difference(got[0], want))
            _same_survey(c, [ref])
            step.pos += k
        step.pos = 0
        step(5 * hop + 7)
        c.measure(); ref.measure()
        assert c.get()[3] == 0 and not c.get()[0].any()
        step(100)                                                          # completes nothing: the restart stays pending
        assert c.get()[3] == 0
        step(4 * hop)                                                      # its first line began in front of the restart: it does not count
        assert ref.lines == 2
        c.measure(0); ref.measure()
        step(hop - 107)                                                    # ends on a line's first sample
        c.measure(); ref.measure()
        step(30 * hop - step.pos)
        assert ref.lines == 30 - 10 - 1
        assert sp.lib.nvx_spec_measure(c._h, 1) == nv._native.ERR_ARG and sp.lib.nvx_spec_reset(c._h, -2) == nv._native.ERR_ARG


# ------------------------------------------------------------------------------------------------------------------ (g)
@pytest.mark.parametrize("position", [2 ** 32 - 1000, 2 ** 40 + 5])
def test_positions_beyond_32_bits(nv, sp, position):
    n, more = 3000, 2000
    rows = [sc.busy(n + more, 80 + s) for s in range(2)]
    refs = [sr.Spectrum(sr.CS16, 8, 2, position) for _ in rows]
    with sp.Spectrum(sr.CS16, n_rows=2, n_log2=8, avg=2) as c:
        c.debug_set_position(position)
        assert c.position(1) == position
        for part in ([r[:n] for r in rows], [r[n:] for r in rows]):
            got = _run_resident(nv, sp, c, part, [999, len(part[0]) - 999])
            for s in range(2):
                want = refs[s].push(part[s])
                assert want.shape[0] >= 7 and np.array_equal(got[s], want), (s, _first_difference(got[s], want))
        _same_survey(c, refs)
        assert c.position(0) == position + n + more


# ------------------------------------------------------------------------------------------------------------------ (h)
@pytest.mark.parametrize("fmt", [sr.CS16, sr.CS8], ids=["cs16", "cs8"])
def test_push_equals_resident_and_a_call_in_batches(nv, sp, fmt):
    n_log2, avg = 8, 2
    n = 20 * 256 + 384
    rows = [sc.busy(2 * n, 120 + s, fmt) for s in range(3)]
    refs = [sr.Spectrum(fmt, n_log2, avg) for _ in rows]
    with sp.Spectrum(fmt, n_rows=3, n_log2=n_log2, avg=avg) as c:
        wants = [ref.push(row) for ref, row in zip(refs, rows)]
        k = sr.lines_at(n, n_log2, avg)
        for s, cuts in enumerate(([n], [1, 127, n - 128], [7, 0, 377, 1, n - 385])):
            pos, parts = 0, []
            for cut in cuts:
                parts.append(c.push(s, rows[s][pos:pos + cut], levels=s != 1)); pos += cut
            out = np.concatenate(parts)
            if s != 1:
                assert out.dtype == np.uint16 and np.array_equal(out, wants[s][:k]), (s, _first_difference(out, wants[s][:k]))
            assert out.shape[0] == k and c.position(s) == n
        # the rest in batches of at most two lines of the three rows: 3 * 2 * 3 * 256 * 8 bytes of scratch rows
        c.debug_set_scratch(3 * 2 * 3 * 256 * 8)
        got = _run_resident(nv, sp, c, [row[n:] for row in rows], [n])
        lines = wants[0].shape[0] - k
        assert c.debug_last_launch()["batch_lines"] == 2 and c.debug_last_launch()["batches"] == (lines + 1) // 2 and lines % 2 == 1
        for s in range(3):
            assert np.array_equal(got[s], wants[s][k:]), s
        _same_survey(c, refs)


# ------------------------------------------------------------------------------------------------------------------ (i)
def test_scale_256_rows(nv, sp):
    """256 rows x 6 lines of N = 1024, A = 4, unsigned 8-bit samples, sixteen different rows among them, every row checked."""
    ns, kinds, n_log2, avg = 256, 16, 10, 4
    n = 5 * avg * 512 + 5 * 512
    made = [sc.busy(n, 7000 + k, sr.CU8) for k in range(kinds)]
    d_in = nv.DeviceBuffer(ns * n * 2); d_lv = nv.DeviceBuffer(ns * 6 * 1024 * 2)
    block = np.stack(made)
    for s in range(0, ns, kinds):
        d_in.upload(block, s * n * 2)
    with sp.Spectrum(sr.CU8, n_rows=ns, n_log2=n_log2, avg=avg) as c:
        assert c.lines_for(n) == 6 and c.resident(d_in, n, n, d_lv, 6) == 6
        assert c.debug_last_launch() == {"launches": 3, "lines": 6, "batch_lines": 6, "batches": 1, "carried": 0}
        got = d_lv.download(ns * 6 * 1024 * 2, dtype=np.uint16).reshape(ns, 6, 1024)
        surveys = {s: c.get(s) for s in (0, 127, 255)}
    d_in.free(); d_lv.free()
    refs = [sr.Spectrum(sr.CU8, n_log2, avg) for _ in made]
    wants = [ref.push(row) for ref, row in zip(refs, made)]
    bad = [s for s in range(ns) if not np.array_equal(got[s], wants[s % kinds])]
    assert not bad, bad[:10]
    for s, (p, re, im, lines) in surveys.items():
        ref = refs[s % kinds]
        assert lines == 6 and np.array_equal(p, ref.sp) and np.array_equal(re, ref.sc_re) and np.array_equal(im, ref.sc_im), s


# ------------------------------------------------------------------------------------------------------------------ (j)
def test_span_alignment_overlap_line_cap_and_position_errors_launch_nothing(nv, sp):
    ARG = nv._native.ERR_ARG
    n = 8192                                                            # N = 256, A = 2: 31 lines
    with sp.Spectrum(sr.CU8, n_rows=2, n_log2=8, avg=2) as c:
        cap = c.lines_for(n)
        assert cap == 31
        d_a = nv.DeviceBuffer(2 * n * 2); d_lv = nv.DeviceBuffer(2 * cap * 256 * 2)
        one_in = nv.DeviceBuffer(n * 2); one_lv = nv.DeviceBuffer(cap * 256 * 2)
        both = nv.DeviceBuffer(2 * n * 2 + 2 * (cap + 1) * 256 * 2)            # input and level words in one allocation
        c.timing(True)
        call = lambda *a: sp.lib.nvx_spec_resident(c._h, *a, None)         # noqa: E731
        A, O = d_a.ptr, d_lv.ptr
        bad = {"more samples than the pitch": (A, n - 8, n, O, cap),
               "input rows for one row": (one_in.ptr, n, n, O, cap),
               "level words for one row": (A, n, n, one_lv.ptr, cap),
               "more lines than line_cap": (A, n, n, O, cap - 1),
               "no line_cap at all": (A, n, n, O, 0),
               "misaligned input": (A + 4, n, n - 8, O, cap),
               "misaligned level words": (A, n, n, O + 2, cap),
               "input rows not 16-byte aligned": (A, n - 3, n - 8, O, cap),
               "null input": (None, n, n, O, cap),
               "too many samples": (A, 2 ** 31, 2 ** 30 + 1, O, cap),
               "an input pitch that wraps": (A, 2 ** 63, n, O, cap),
               "a line_cap that wraps": (A, n, n, O, 2 ** 62),
               "the level words on the input": (both.ptr, n, n, both.ptr, cap),
               "the level words' first lines on the input's last row": (both.ptr, n, n, both.ptr + 2 * n * 2 - 512, cap)}
        for name, args in bad.items():
            assert call(*args) == ARG, name
            assert sp.lib.nvx_spec_last_error() != b""
        assert b"overlap" in sp.lib.nvx_spec_last_error()
        c.debug_set_position(2 ** 62 - 100)
        assert call(A, n, n, O, cap) == ARG and b"2^62" in sp.lib.nvx_spec_last_error()
        assert sp.lib.nvx_spec_debug_set_position(c._h, 0, 2 ** 62) == ARG and sp.lib.nvx_spec_debug_set_position(c._h, 2, 0) == ARG
        assert sp.lib.nvx_spec_reset(c._h, 2) == ARG and sp.lib.nvx_spec_get(c._h, -1, None, None, None, None) == ARG
        assert sp.lib.nvx_spec_lines_for(c._h, 2, n) == ARG and sp.lib.nvx_spec_lines_for(c._h, 0, 2 ** 30 + 1) == ARG
        assert c.time_stats() == (0.0, 0) and c.debug_last_launch()["launches"] == 0 and c.position(0) == 2 ** 62 - 100
        c.reset()
        assert call(A, n, 0, O, cap) == 0 and c.debug_last_launch()["launches"] == 0          # nothing to do: no launch
        assert c.time_stats() == (0.0, 0)
        d_a.upload(np.full(2 * n * 2, 128, dtype=np.uint8))
        d_lv.upload(np.full(2 * cap * 256, SENTINEL, dtype=np.uint16))
        # survey only: no level word is written
        assert call(A, n, n, None, 0) == cap and c.get(1)[3] == cap
        assert np.all(d_lv.download(2 * cap * 256 * 2, dtype=np.uint16) == SENTINEL)
        # the level words behind the input in one allocation, touching and not overlapping
        both.upload(np.full(2 * n * 2 + 2 * (cap + 1) * 256 * 2, 128, dtype=np.uint8))
        assert call(both.ptr, n, n, both.ptr + 2 * n * 2, cap + 1) == 32 and c.get(0)[3] == 2 * cap + 1
        ms, calls = c.time_stats()
        assert calls == 2 and ms > 0.0 and c.debug_last_launch()["launches"] == 6
        for d in (d_a, d_lv, one_in, one_lv, both):
            d.free()
    for kw in (dict(device=99), dict(n_log2=7), dict(n_log2=13), dict(format=4), dict(n_rows=0), dict(avg=0), dict(avg=65)):
        with pytest.raises(nv.NvxError) as e:
            sp.Spectrum(**kw)
        assert e.value.code == ARG, kw


# ------------------------------------------------------------------------------------------------------------------ (k)
def test_seed_11_of_the_acceptance_case_on_the_device(nv, sp, oracle):
    """The row of seed 11 through the monitor at N = 4096, A = 8, survey only: the device's survey is the CPU's, and the finder,
    which is not told where the carriers are, names the two within a hertz.  Its two steps go into the tone notch on the device
    (R = 32, no refine); the plain and the notched row run as two streams of a two-chain handle: the 490 message arrives from
    the notched row and not from the plain row, and the bits of all four chains are the oracle's on the same words."""
    import navtex_amd.notch as nt
    t490 = sc.nc.text()
    a = sc.acceptance_row(nv, 11)
    n = len(a)
    _, ref = sr.spectrum(a, sr.CS16, 12, 8)
    d_rows = nv.DeviceBuffer(2 * n * 4)
    d_rows.upload(a)
    with sp.Spectrum(sr.CS16, n_log2=12, avg=8) as c:
        assert c.resident(d_rows, n, n) == ref.lines == 369
        _same_survey(c, [ref])
        hits = c.find_lines()
    assert len(hits) == 2 and sorted(h["bin"] for h in hits) == sorted(h["bin"] for h in ref.find_lines())
    for hz, _ in sc.CARRIERS:
        assert min(abs(f - hz) for f in sc.hits_hz(hits)) <= 1.0, (hz, sc.hits_hz(hits))
    with nt.Notch(nt.CS16, n_notches=2, width_log2=5) as notch:
        for k, h in enumerate(hits):
            notch.set_freq(k, h["step"]); notch.enable(k)
        # the notched row goes behind the plain row: row 1 of the handle's input
        notch.resident(d_rows, n, n, d_rows, n, out_first=n)
        got = d_rows.download(2 * n * 4, dtype=np.int16).reshape(2, n, 2)
    assert np.array_equal(got[0], a)
    frames = n // nv.FRAME_IN
    with nv.Pipeline(n_streams=2, chain_mask=nv.CHAIN_518 | nv.CHAIN_490, max_frames=8) as p:
        for f0 in range(0, frames, 8):
            p.process_resident(d_rows, n, f0, min(8, frames - f0), hip_stream=p.hip_stream)
        p.fetch()
        bits = [(p.bits(s, 0), p.bits(s, 1)) for s in range(2)]
        msgs = [[m[3] for m in p.messages if m[0] == s and m[1] == 490] for s in range(2)]
    d_rows.free()
    cpu = [sc.nc.delivered(oracle, row, nv.FRAME_IN) for row in (got[0], got[1])]
    for s in range(2):
        assert bits[s] == cpu[s][1] and msgs[s] == cpu[s][0], s
    assert msgs[1] == [t490] and msgs[0] != [t490]
