"""The IQ corrector (include/navtex_amd_iqc.h) on the GPU (-m gpu): output words equal to the restatement (tests/iqc_ref.py)
for every format and window in one call from position 0, W = 4 cut into calls at and next to the block ends against one shot,
a reset stream rejoining the others, the rails and full-scale random input (float32 specials) with the counters and the
window's sums, the rejection reasons 1, 2 and 4, the two launch shapes, positions beyond 2^32, set / HOLD / TRACK between calls,
push against resident, and the acceptance case's seed 11 through a two-chain handle.  Every comparison is ==, with sentinels
around every output row.  Where a block ends inside a tile, the longer windows across calls, form 2 beyond its one case here,
the apply at the limits of nvx_iqc_set and reason 3: tests/test_gpu_iqc_edges.py."""
from pathlib import Path

import numpy as np
import pytest

import iqc_cases as ic
import iqc_ref as ir
import resample_ref as rr
from iqc_cases import _extremes

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FORMATS = (ir.CS16, ir.CU8, ir.CS8, ir.CF32)
FORMAT_IDS = ("cs16", "cu8", "cs8", "cf32")
SENTINEL = 0x5a5a1234
B = ir.BLOCK


@pytest.fixture(scope="module")
def iq(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_iqc.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.iqc
    return navtex_amd.iqc


def _gain(fmt):
    return 3.0 if fmt in (ir.CU8, ir.CS8) else 1.0


def _run_resident(nv, c, rows, cuts, pitch_extra=0, out_first=0):
    """The rows ([n, 2] each, all of one length) through nvx_iqc_resident in calls of `cuts` samples; every call's input is
    uploaded to the start of the input rows as whole rows: behind a call's n_in samples the row is full scale up to the pitch,
    so a read behind n_in changes the output.  Sentinels around every output row.  Returns int16 [streams, n, 2]."""
    ns, n = len(rows), len(rows[0])
    assert sum(cuts) == n and ns == c.n_streams
    dt = rows[0].dtype
    bps = dt.itemsize * 2
    pitch_out = out_first + n + pitch_extra
    pitch_in = (max(max(cuts), 1) + 7) // 8 * 8 + 8 * pitch_extra
    d_in = nv.DeviceBuffer(ns * pitch_in * bps)
    d_out = nv.DeviceBuffer(ns * pitch_out * 4)
    d_out.upload(np.full(ns * pitch_out, SENTINEL, dtype=np.uint32))
    block = np.empty((ns, pitch_in, 2), dtype=dt)
    start = c.position(0)
    pos = 0
    for cut in cuts:
        block[:, cut:] = 1.0 if dt == np.float32 else np.iinfo(dt).max
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


def _status(ref):
    """What nvx_iqc_get returns, from the restatement."""
    return {"coefficients": tuple(int(v) for v in ref.coef), "mode": ref.mode, "last_reason": ref.reason, "sums": ref.sums(),
            "samples": ref.samples, "blocks_solved": ref.solved, "blocks_rejected": ref.rejected}


# ------------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_two_streams_of_six_and_a_half_blocks_in_every_format(nv, iq, fmt):
    """W = 4: blocks 4, 5 and 6 are solved.  A pitch larger than the data; out_first = 7 (the unaligned stores) and 8."""
    n = 6 * B + B // 2
    rows = [rr.to_format(ic.impaired_noise(n, 200 + 10 * fmt + s), fmt, gain=_gain(fmt)) for s in range(2)]
    refs = [ir.correct(row, fmt, 2) for row in rows]
    assert all(ref.solved == 3 and len({h[1] for h in ref.history}) == 3 for _, ref in refs)
    for out_first in (7, 8):
        with iq.Corrector(fmt, n_streams=2, window_log2=2) as c:
            got = _run_resident(nv, c, rows, [n], pitch_extra=3 + out_first % 2, out_first=out_first)
            for s in range(2):
                assert np.array_equal(got[s], refs[s][0]), (out_first, s, _first_difference(got[s], refs[s][0]))
                assert c.get(s) == _status(refs[s][1]), (out_first, s)


@pytest.mark.parametrize("window_log2,blocks", [(4, 18.3), (6, 66.2)], ids=["w16", "w64"])
def test_one_stream_through_the_longer_windows(nv, iq, window_log2, blocks):
    n = int(blocks * B)
    row = ic.impaired_noise(n, 300 + window_log2)
    want, ref = ir.correct(row, ir.CS16, window_log2)
    assert ref.solved == int(blocks) - (1 << window_log2) + 1 and ref.rejected == 0
    with iq.Corrector(ir.CS16, window_log2=window_log2) as c:
        got = _run_resident(nv, c, [row], [n], pitch_extra=5, out_first=7)
        assert np.array_equal(got[0], want), _first_difference(got[0], want)
        assert c.get(0) == _status(ref)
    assert c.window_log2 == window_log2


# ------------------------------------------------------------------------------------------------------------------ (b)
def test_one_shot_equals_calls_cut_at_the_block_ends_and_a_reset_stream_rejoins(nv, iq):
    cuts = [B + 1, 1, 0, B - 1, B]
    n1 = 8 * B + 20000
    cuts = cuts + [n1 - sum(cuts)]
    tail = 2 * B + 777
    rows = [ic.impaired_noise(n1 + tail, 400 + s) for s in range(3)]
    refs = [ir.correct(row, ir.CS16, 2) for row in rows]
    with iq.Corrector(ir.CS16, n_streams=3, window_log2=2) as c:
        got = _run_resident(nv, c, [row[:n1] for row in rows], cuts)
        for s in range(3):
            assert np.array_equal(got[s], refs[s][0][:n1]), (s, _first_difference(got[s], refs[s][0][:n1]))
        c.reset(1)
        assert c.position(1) == 0 and c.position(0) == n1 and c.get(1)["coefficients"] == ir.IDENTITY
        d = nv.DeviceBuffer(3 * 64 * 4); o = nv.DeviceBuffer(3 * 64 * 4)
        assert iq.lib.nvx_iqc_resident(c._h, d.ptr, 64, 64, o.ptr, 64, 0, None) == nv._native.ERR_STATE
        assert b"same position" in iq.lib.nvx_iqc_last_error()
        d.free(); o.free()
        # stream 1 starts anew on other data, alone and in calls of its own, up to where the others stand
        fresh = ir.Corrector(ir.CS16, 2)
        other = ic.impaired_noise(n1 + tail, 450)
        pos = 0
        for cut in (B + 5, 1, B - 6, n1 - 2 * B):
            assert np.array_equal(c.push(1, other[pos:pos + cut]), fresh.push(other[pos:pos + cut])), pos
            pos += cut
        assert c.position(1) == n1
        got = _run_resident(nv, c, [rows[0][n1:], other[n1:], rows[2][n1:]], [tail])
        assert np.array_equal(got[0], refs[0][0][n1:]) and np.array_equal(got[2], refs[2][0][n1:])
        assert np.array_equal(got[1], fresh.push(other[n1:]))
        assert c.get(0) == _status(refs[0][1]) and c.get(2) == _status(refs[2][1])
        st = c.get(1)
        assert st["coefficients"] == fresh.coef and st["sums"] == fresh.sums() and st["samples"] == 2 * n1 + tail


# ------------------------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_the_rails_and_full_scale_random_input_with_counters_and_sums(nv, iq, fmt):
    """Every product at its largest: I^2 + Q^2 = 2^31 and 2 I Q = 2^31 in every sample of the first row.  The counters and the
    window's five sums are the restatement's integers."""
    n = 5 * B + 21000
    rows = _extremes(fmt, n, 500 + fmt)
    refs = [ir.correct(row, fmt, 2) for row in rows]
    if fmt == ir.CS16:
        assert refs[0][1].sums()[2:] == (4 * B * 2 ** 30,) * 3 and np.array_equal(rows[0], ic.rails(n, False)) and np.array_equal(rows[1], ic.rails(n, True))
    assert refs[0][1].reason == 1 and refs[2][1].solved + refs[2][1].rejected == 2
    with iq.Corrector(fmt, n_streams=3, window_log2=2) as c:
        got = _run_resident(nv, c, rows, [2 * B + 11, n - 2 * B - 11], out_first=3)
        for s in range(3):
            assert np.array_equal(got[s], refs[s][0]), (s, _first_difference(got[s], refs[s][0]))
            assert c.get(s) == _status(refs[s][1]), s


# ------------------------------------------------------------------------------------------------------------------ (d)
def test_the_rejection_reasons(nv, iq):
    n = 5 * B + 100
    rows = [ic.silence_with_dc(n), ic.q_equals_i(n, 61), ic.q_three_i_rotated(n, 62)]
    refs = [ir.correct(row, ir.CS16, 2) for row in rows]
    assert [ref.reason for _, ref in refs] == [1, 2, 4] and all(ref.rejected == 2 and ref.solved == 0 for _, ref in refs)
    assert refs[0][1].coef == (ic.DC_I, ic.DC_Q, 0, 16384) and not refs[0][0][4 * B:].any()
    with iq.Corrector(ir.CS16, n_streams=3, window_log2=2) as c:
        got = _run_resident(nv, c, rows, [n])
        for s in range(3):
            assert np.array_equal(got[s], refs[s][0]), (s, _first_difference(got[s], refs[s][0]))
            assert c.get(s) == _status(refs[s][1]), s


# ------------------------------------------------------------------------------------------------------------------ (e)
def test_a_stream_spread_over_chunks(nv, iq):
    """1 stream x 40 blocks behind a first call of 777 samples: twenty workgroups of two blocks each, block ends inside tiles."""
    first, n = 777, 40 * B
    row = ic.impaired_noise(first + n, 70)
    want, ref = ir.correct(row, ir.CS16, 2)
    with iq.Corrector(ir.CS16, window_log2=2) as c:
        got = _run_resident(nv, c, [row], [first, n])
        assert c.debug_last_launch() == {"launches": 4, "chunks": 20, "tiles_per_chunk": 32, "records": 41, "form": 2}
        assert np.array_equal(got[0], want), _first_difference(got[0], want)
        assert c.get(0) == _status(ref) and ref.solved == 37


def test_scale_1024_streams_at_one_chunk_each(nv, iq):
    """1024 streams x 5.2 blocks of unsigned 8-bit samples, sixteen different rows among them."""
    ns, n, kinds = 1024, int(5.2 * B) // 8 * 8, 16
    rows = [rr.to_format(ic.impaired_noise(n, 7000 + k), ir.CU8, gain=3.0) for k in range(kinds)]
    refs = [ir.correct(row, ir.CU8, 2) for row in rows]
    d_in = nv.DeviceBuffer(ns * n * 2); d_out = nv.DeviceBuffer(ns * n * 4)
    block = np.stack(rows)
    for s in range(0, ns, kinds):
        d_in.upload(block, s * n * 2)
    with iq.Corrector(ir.CU8, n_streams=ns, window_log2=2) as c:
        c.resident(d_in, n, n, d_out, n)
        got = d_out.download(ns * n * 4, dtype=np.int16).reshape(ns, n, 2)
        shape = c.debug_last_launch()
        assert shape["chunks"] == 1 and shape["form"] == 1 and shape["records"] == 6 and shape["tiles_per_chunk"] == (n + 4095) // 4096
        status = {s: c.get(s) for s in (0, 511, 1023)}
    d_in.free(); d_out.free()
    bad = [s for s in range(ns) if not np.array_equal(got[s], refs[s % kinds][0])]
    assert not bad, bad[:10]
    assert all(st == _status(refs[s % kinds][1]) for s, st in status.items()) and refs[0][1].solved == 2


# ------------------------------------------------------------------------------------------------------------------ (f)
@pytest.mark.parametrize("position", [2 ** 32 - 1000, 2 ** 40 + 5])
def test_positions_beyond_32_bits(nv, iq, position):
    """Three blocks in two calls from the position, then a block and a half more: the block the position lies in counts as
    complete when it ends, with the samples it got."""
    n, more = 3 * B, B + B // 2
    rows = [ic.impaired_noise(n + more, 80 + s) for s in range(2)]
    refs = [ir.Corrector(ir.CS16, 2, position) for _ in rows]
    with iq.Corrector(ir.CS16, n_streams=2, window_log2=2) as c:
        c.debug_set_position(position)
        assert c.position(1) == position
        got = _run_resident(nv, c, [row[:n] for row in rows], [B + 9000, n - B - 9000])
        for s in range(2):
            want = refs[s].push(rows[s][:n])
            assert np.array_equal(got[s], want), (s, _first_difference(got[s], want))
            assert c.get(s) == _status(refs[s])
        got = _run_resident(nv, c, [row[n:] for row in rows], [more])
        for s in range(2):
            want = refs[s].push(rows[s][n:])
            assert np.array_equal(got[s], want), (s, _first_difference(got[s], want))
            assert c.get(s) == _status(refs[s]) and refs[s].solved >= 1


# ------------------------------------------------------------------------------------------------------------------ (g)
def test_set_hold_and_back_to_track_between_calls(nv, iq):
    n = 11 * B
    row = ic.impaired_noise(n, 90)
    ref = ir.Corrector(ir.CS16, 2)
    with iq.Corrector(ir.CS16, window_log2=2) as c:
        def step(k):
            got = _run_resident(nv, c, [row[step.pos:step.pos + k]], [k])
            want = ref.push(row[step.pos:step.pos + k])
            assert np.array_equal(got[0], want), (step.pos, _first_difference(got[0], want))
            assert c.get(0) == _status(ref), step.pos
            step.pos += k
        step.pos = 0
        c.set(-120, 45, 700, 15000); ref.set(-120, 45, 700, 15000)        # in front of the first sample: held until block 4
        step(2 * B + 100)
        assert ref.coef == (-120, 45, 700, 15000)
        step(3 * B)                                                        # blocks 4 and 5 start: solved
        assert ref.solved == 2
        c.set_mode(iq.HOLD); ref.set_mode(ir.HOLD)
        held = ref.coef
        step(2 * B)
        assert ref.coef == held and ref.solved == 2
        c.set(5, -5, -300, 17000); ref.set(5, -5, -300, 17000)             # a calibrated radio: set and hold
        step(B + 17)
        assert ref.coef == (5, -5, -300, 17000)
        c.set_mode(iq.TRACK); ref.set_mode(ir.TRACK)
        step(n - step.pos)
        assert ref.solved == 4 and c.get(0)["mode"] == iq.TRACK
        for bad in ((40000, 0, 0, 16384), (0, 0, 5463, 16384), (0, 0, 0, 12287), (0, 0, 0, 21846)):
            assert iq.lib.nvx_iqc_set(c._h, 0, *bad) == nv._native.ERR_ARG
        assert iq.lib.nvx_iqc_set_mode(c._h, 0, 2) == nv._native.ERR_ARG and iq.lib.nvx_iqc_set_mode(c._h, 1, 0) == nv._native.ERR_ARG
        assert c.get(0) == _status(ref)


# ------------------------------------------------------------------------------------------------------------------ (h)
@pytest.mark.parametrize("fmt", [ir.CS16, ir.CS8], ids=["cs16", "cs8"])
def test_push_equals_resident(nv, iq, fmt):
    n = 5 * B + 3000
    rows = [rr.to_format(ic.impaired_noise(2 * n, 120 + s), fmt, gain=_gain(fmt)) for s in range(3)]
    refs = [ir.correct(row, fmt, 2) for row in rows]
    with iq.Corrector(fmt, n_streams=3, window_log2=2) as c:
        for s, cuts in enumerate(([n], [1, B - 1, n - B], [7, 0, B + 5000, 1, n - B - 5008])):
            pos, parts = 0, []
            for cut in cuts:
                parts.append(c.push(s, rows[s][pos:pos + cut])); pos += cut
            out = np.concatenate(parts)
            assert out.dtype == np.int16 and np.array_equal(out, refs[s][0][:n]), s
            assert c.position(s) == n
        got = _run_resident(nv, c, [row[n:] for row in rows], [n])
        for s in range(3):
            assert np.array_equal(got[s], refs[s][0][n:]), s
            assert c.get(s) == _status(refs[s][1])


def test_span_and_position_errors_launch_nothing(nv, iq):
    ARG = nv._native.ERR_ARG
    n = 8192
    with iq.Corrector(ir.CU8, n_streams=2) as c:
        d_in = nv.DeviceBuffer(2 * n * 2); d_out = nv.DeviceBuffer(2 * n * 4)
        one_in = nv.DeviceBuffer(n * 2); one_out = nv.DeviceBuffer(n * 4)
        c.timing(True)
        call = lambda *a: iq.lib.nvx_iqc_resident(c._h, *a, None)            # noqa: E731
        bad = {"more samples than the pitch": (d_in.ptr, n - 8, n, d_out.ptr, n, 0),
               "words beyond the pitch": (d_in.ptr, n, n, d_out.ptr, n - 1, 0),
               "out_first pushes them beyond it": (d_in.ptr, n, n, d_out.ptr, n, 1),
               "input rows for one stream": (one_in.ptr, n, n, d_out.ptr, n, 0),
               "output rows for one stream": (d_in.ptr, n, n, one_out.ptr, n, 0),
               "misaligned input": (d_in.ptr + 4, n, n - 8, d_out.ptr, n, 0),
               "misaligned output": (d_in.ptr, n, n, d_out.ptr + 2, n, 0),
               "rows not 16-byte aligned": (d_in.ptr, n - 3, n - 8, d_out.ptr, n, 0),
               "null input": (None, n, n, d_out.ptr, n, 0),
               "null output": (d_in.ptr, n, n, None, n, 0),
               "too many samples": (d_in.ptr, 2 ** 31, 2 ** 30 + 1, d_out.ptr, 2 ** 31, 0),
               "a pitch that wraps": (d_in.ptr, 2 ** 63, n, d_out.ptr, n, 0),
               "an output pitch that wraps": (d_in.ptr, n, n, d_out.ptr, 2 ** 62, 0),
               "out_first that wraps": (d_in.ptr, n, n, d_out.ptr, n, 2 ** 64 - 8)}
        for name, args in bad.items():
            assert call(*args) == ARG, name
            assert iq.lib.nvx_iqc_last_error() != b""
        c.debug_set_position(2 ** 62 - 100)
        assert call(d_in.ptr, n, n, d_out.ptr, n, 0) == ARG and b"2^62" in iq.lib.nvx_iqc_last_error()
        assert iq.lib.nvx_iqc_debug_set_position(c._h, 0, 2 ** 62) == ARG and iq.lib.nvx_iqc_debug_set_position(c._h, 2, 0) == ARG
        assert iq.lib.nvx_iqc_reset(c._h, 2) == ARG and iq.lib.nvx_iqc_get(c._h, -1, None) == ARG and iq.lib.nvx_iqc_get(c._h, 0, None) == ARG
        assert c.time_stats() == (0.0, 0) and c.debug_last_launch()["launches"] == 0 and c.position(0) == 2 ** 62 - 100
        c.reset()
        assert call(d_in.ptr, n, 0, d_out.ptr, n, 0) == 0 and c.debug_last_launch()["launches"] == 0       # nothing to do: no launch
        d_in.upload(np.full(2 * n * 2, 128, dtype=np.uint8))
        assert call(d_in.ptr, n, n, d_out.ptr, n, 0) == 0
        ms, calls = c.time_stats()
        assert calls == 1 and ms > 0.0 and c.debug_last_launch()["launches"] == 2 and c.get(1)["samples"] == n
        for d in (d_in, d_out, one_in, one_out):
            d.free()
    for kw in (dict(device=99), dict(window_log2=3), dict(window_log2=8), dict(format=4), dict(n_streams=0)):
        with pytest.raises(nv.NvxError) as e:
            iq.Corrector(**kw)
        assert e.value.code == ARG, kw


# ------------------------------------------------------------------------------------------------------------------ (i)
def test_seed_11_of_the_acceptance_case_on_the_device(nv, iq, oracle):
    """The impaired row of seed 11 through the corrector on the device: the words are the CPU's.  Then the impaired and the
    corrected row as two streams of a two-chain handle: the 490 message arrives from the corrected row and not from the
    impaired one, and the bits of all four chains are the oracle's on the same words."""
    t518, t490 = ic.texts()
    y = ic.impair(ic.rows(nv, 11))
    n = len(y)
    want, ref = ir.correct(y)
    d_in = nv.DeviceBuffer(2 * n * 4)
    d_in.upload(y)
    with iq.Corrector(ir.CS16) as c:
        # the corrected row goes behind the impaired one: row 1 of the handle's input
        c.resident(d_in, n, n, d_in, n, out_first=n)
        got = d_in.download(2 * n * 4, dtype=np.int16).reshape(2, n, 2)
        assert np.array_equal(got[0], y) and np.array_equal(got[1], want), _first_difference(got[1], want)
        assert c.get(0) == _status(ref) and ref.solved > 60 and ref.rejected == 0
    frames = n // nv.FRAME_IN
    with nv.Pipeline(n_streams=2, chain_mask=nv.CHAIN_518 | nv.CHAIN_490, max_frames=8) as p:
        for f0 in range(0, frames, 8):
            p.process_resident(d_in, n, f0, min(8, frames - f0), hip_stream=p.hip_stream)
        p.fetch()
        bits = [(p.bits(s, 0), p.bits(s, 1)) for s in range(2)]
        msgs = [{f: [m[3] for m in p.messages if m[0] == s and m[1] == f] for f in (518, 490)} for s in range(2)]
    d_in.free()
    cpu = [ic.delivered(oracle, row, nv.FRAME_IN) for row in (y, want)]
    for s in range(2):
        assert bits[s] == cpu[s][1] and msgs[s] == cpu[s][0], s
    assert msgs[1][490] == [t490] and msgs[0][490] != [t490]
    assert msgs[0][518] == [t518] and msgs[1][518] == [t518]
