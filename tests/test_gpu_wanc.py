"""The multi-tap noise canceller (include/navtex_amd_wanc.h) on the GPU (-m gpu): output words equal to the restatement
(tests/wanc_ref.py) for every format at K = 8 and for K = 4 and 16, calls cut at and next to the block ends and shorter than the
halo against one shot, a reset pair rejoining the others, block ends everywhere in a tile, a pair spread over chunks, the rails
and full-scale random input with the counters and the window's sums, the rejection reasons 1, 2 and 3, set / HOLD / TRACK
between calls, positions beyond 2^32, 256 pairs, push against resident, the calls that are refused before anything is launched,
and the acceptance case's seed 11 through a two-chain handle.  Every comparison is ==, with sentinels around every output row,
and both input rows are full scale behind the samples of a call."""
from pathlib import Path

import numpy as np
import pytest

import anc_cases as ac
import anc_ref as ar
import wanc_cases as wc
import wanc_ref as wr

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FORMATS = (wr.CS16, wr.CU8, wr.CS8, wr.CF32)
FORMAT_IDS = ("cs16", "cu8", "cs8", "cf32")
SENTINEL = 0x5a5a1234
B = wr.BLOCK


@pytest.fixture(scope="module")
def wn(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_wanc.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.wanc
    return navtex_amd.wanc


def _run_resident(nv, c, pairs, cuts, pitch_extra=0, out_first=0):
    """The pairs ((main, sense), [n, 2] each, all of one length) through nvx_wanc_resident in calls of `cuts` samples; every
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
    """What nvx_wanc_get returns, from the restatement."""
    return {"weights": ref.w, "mode": ref.mode, "last_reason": ref.reason, "coherence_q14": ref.coherence, "sums": ref.sums(),
            "samples": ref.samples, "blocks_solved": ref.solved, "blocks_rejected": ref.rejected}


# ------------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("fmt,K", [(f, 8) for f in FORMATS] + [(wr.CS16, 4), (wr.CS16, 16)], ids=[f"{i}-k8" for i in FORMAT_IDS] + ["cs16-k4", "cs16-k16"])
def test_two_pairs_of_six_and_a_half_blocks(nv, wn, fmt, K):
    """W = 4: blocks 4, 5 and 6 are solved.  Pitches larger than the data; out_first = 7 (the unaligned stores) and 8."""
    n = 6 * B + B // 2
    pairs = [wc.formatted_pair(n, 200 + 10 * fmt + s, fmt) for s in range(2)]
    refs = [wr.cancel(a, b, fmt, K) for a, b in pairs]
    assert all(ref.solved == 3 and len({h[1] for h in ref.history}) == 3 for _, ref in refs)
    for out_first in (7, 8):
        with wn.Canceller(fmt, n_pairs=2, n_taps=K) as c:
            got = _run_resident(nv, c, pairs, [n], pitch_extra=3 + out_first % 2, out_first=out_first)
            for s in range(2):
                assert np.array_equal(got[s], refs[s][0]), (out_first, s, _first_difference(got[s], refs[s][0]))
                assert c.get(s) == _status(refs[s][1]), (out_first, s)


# ------------------------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("K", [4, 8, 16])
def test_one_shot_equals_calls_cut_at_the_block_ends_and_shorter_than_the_halo(nv, wn, K):
    """Calls that end on, one in front of and one behind a block end, calls of 1, K - 1 and G samples (shorter than the halo:
    the next call's halo comes from the carried words and the call's own), an empty call, and calls of K - 1 and 1 samples
    across a block end."""
    G = K // 2
    cuts = [B + 1, 1, 0, B - 1, K - 1, G, 1, 1, B - K - G - 2, B - (K - 1), K - 1, 1, G, B - G - 1]
    n = 7 * B + 1234
    cuts = cuts + [n - sum(cuts)]
    assert sum(cuts[:4]) == 2 * B + 1 and sum(cuts[:9]) == 3 * B and sum(cuts[:10]) == 4 * B - (K - 1) and sum(cuts[:14]) == 5 * B
    pairs = [wc.drifting_pair(n, 400 + K + s) for s in range(2)]
    refs = [wr.cancel(a, b, wr.CS16, K) for a, b in pairs]
    assert all(ref.solved == 4 for _, ref in refs)
    with wn.Canceller(wr.CS16, n_pairs=2, n_taps=K) as c:
        got = _run_resident(nv, c, pairs, cuts)
        for s in range(2):
            assert np.array_equal(got[s], refs[s][0]), (s, _first_difference(got[s], refs[s][0]))
            assert c.get(s) == _status(refs[s][1]), s


def test_a_reset_pair_rejoins(nv, wn):
    n1, tail = 5 * B, B + 777
    pairs = [wc.drifting_pair(n1 + tail, 430 + s) for s in range(3)]
    refs = [wr.cancel(a, b) for a, b in pairs]
    with wn.Canceller(wr.CS16, n_pairs=3) as c:
        got = _run_resident(nv, c, [(a[:n1], b[:n1]) for a, b in pairs], [2 * B + 5, n1 - 2 * B - 5])
        for s in range(3):
            assert np.array_equal(got[s], refs[s][0][:n1]), (s, _first_difference(got[s], refs[s][0][:n1]))
        c.reset(1)
        st = c.get(1)
        assert c.position(1) == 0 and c.position(0) == n1 and st["weights"] == ((0,) * 8, (0,) * 8) and st["coherence_q14"] == 0 and not any(st["sums"])
        d = nv.DeviceBuffer(3 * 64 * 4); e = nv.DeviceBuffer(3 * 64 * 4); o = nv.DeviceBuffer(3 * 64 * 4)
        assert wn.lib.nvx_wanc_resident(c._h, d.ptr, 64, e.ptr, 64, 64, o.ptr, 64, 0, None) == nv._native.ERR_STATE
        assert b"same position" in wn.lib.nvx_wanc_last_error()
        d.free(); e.free(); o.free()
        # pair 1 starts anew on other data, alone and in calls of its own, up to where the others stand: silence in front of it
        fresh = wr.Canceller(wr.CS16)
        other = wc.drifting_pair(n1 + tail, 450)
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
        assert st["weights"] == fresh.w and st["sums"] == fresh.sums() and st["samples"] == 2 * n1 + tail and st["coherence_q14"] == fresh.coherence


# ------------------------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_block_ends_everywhere_in_a_tile(nv, wn, fmt):
    """The IQ corrector's block-end sweep (iqc_cases.sweep_cuts: 35 blocks in 44 calls; the kernels share its tiles): a block
    ends 1, 3, 4, 255 ... 4092, 4095 samples into a call's first, second or third tile, calls end just behind the end in the same
    tile and on it.  Every window solves to other weights, so a sample given the wrong block's weights shows, and a sample added
    to the wrong block changes the sums and the solves behind them."""
    import iqc_cases as ic
    cuts = ic.sweep_cuts()
    n = sum(cuts)
    splits, ragged, exact = ic.sweep_coverage(cuts)
    assert set(splits) >= set(ic.SWEEP_N_A) and len(ragged) >= 5 and exact >= 5 and n == 35 * B + 777
    pairs = [wc.formatted_pair(n, 900 + fmt, fmt)]
    refs = [wr.cancel(a, b, fmt) for a, b in pairs]
    weights = [h[1] for h in refs[0][1].history]
    assert refs[0][1].solved == 32 and all(x != y for x, y in zip(weights, weights[1:]))
    with wn.Canceller(fmt, n_pairs=1) as c:
        got = _run_resident(nv, c, pairs, cuts)
        assert np.array_equal(got[0], refs[0][0]), _first_difference(got[0], refs[0][0])
        assert c.get(0) == _status(refs[0][1])


# ------------------------------------------------------------------------------------------------------------------ (d)
def test_a_pair_spread_over_chunks(nv, wn):
    """1 pair x 40 blocks behind a first call of 777 samples: twenty workgroups of two blocks each, block ends inside tiles, and
    every chunk's first tile takes its halo from the row."""
    first, n = 777, 40 * B
    a, b = wc.drifting_pair(first + n, 70)
    want, ref = wr.cancel(a, b)
    with wn.Canceller(wr.CS16) as c:
        got = _run_resident(nv, c, [(a, b)], [first, n])
        assert c.debug_last_launch() == {"launches": 6, "chunks": 20, "tiles_per_chunk": 32, "records": 41, "form": 2}
        assert np.array_equal(got[0], want), _first_difference(got[0], want)
        assert c.get(0) == _status(ref) and ref.solved == 37


# ------------------------------------------------------------------------------------------------------------------ (e)
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_the_rails_and_full_scale_random_input_with_counters_and_sums(nv, wn, fmt):
    """Every product at its largest: both rows at the lowest value make every real part 2^31 in CS16 (the one value the dot
    product wraps at).  The counters and the window's 4 K + 1 sums are the restatement's integers."""
    n = 5 * B + 21000
    pairs = ac.extremes(fmt, n, 500 + fmt)
    refs = [wr.cancel(a, b, fmt) for a, b in pairs]
    if fmt == wr.CS16:
        s = refs[0][1].sums()
        assert s[:8] == (4 * B * 2 ** 31,) * 8 and s[16:24] == (4 * B * 2 ** 31,) * 8 and s[32] == 4 * B * 2 ** 31 and not any(s[8:16]) and not any(s[24:32])
    assert all(ref.solved + ref.rejected == 2 for _, ref in refs)
    with wn.Canceller(fmt, n_pairs=3) as c:
        got = _run_resident(nv, c, pairs, [2 * B + 11, n - 2 * B - 11], out_first=3)
        for s in range(3):
            assert np.array_equal(got[s], refs[s][0]), (s, _first_difference(got[s], refs[s][0]))
            assert c.get(s) == _status(refs[s][1]), s


def test_the_rejection_reasons(nv, wn):
    """The CPU suite's rows on the device: a silent sense row (1), a strong sample at a window's edge (2, at block 6, behind two
    windows that hold it whole and want weights beyond the bounds), weights beyond the bounds (3), and a pair that solves."""
    n = 6 * B + 100
    pairs = [wc.silent_sense(n), wc.edge_sense(n), wc.weak_white_sense(n), wc.drifting_pair(n, 77)]
    refs = [wr.cancel(a, b) for a, b in pairs]
    assert [ref.reason for _, ref in refs] == [1, 2, 3, 0] and [ref.rejected for _, ref in refs] == [3, 3, 3, 0]
    assert [h[3] for h in refs[1][1].history] == [3, 3, 2] and refs[2][1].coherence > 16000
    with wn.Canceller(wr.CS16, n_pairs=4) as c:
        got = _run_resident(nv, c, pairs, [n])
        for s in range(4):
            assert np.array_equal(got[s], refs[s][0]), (s, _first_difference(got[s], refs[s][0]))
            assert c.get(s) == _status(refs[s][1]), s


# ------------------------------------------------------------------------------------------------------------------ (f)
@pytest.mark.parametrize("position", [2 ** 32 - 1000, 2 ** 40 + 5])
def test_positions_beyond_32_bits(nv, wn, position):
    """Three blocks in two calls from the position, then two and a half blocks more: the block the position lies in counts as
    complete when it ends, with the samples it got, and silence lies in front of it."""
    n, more = 3 * B, 2 * B + B // 2
    pairs = [wc.drifting_pair(n + more, 80 + s) for s in range(2)]
    refs = [wr.Canceller(wr.CS16, position=position) for _ in pairs]
    with wn.Canceller(wr.CS16, n_pairs=2) as c:
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
def test_set_hold_and_back_to_track_between_calls(nv, wn):
    n = 11 * B
    a, b = wc.drifting_pair(n, 90)
    ref = wr.Canceller(wr.CS16)
    some = ((100, -2000, 8192, 300, -40, 5, 0, -7), (0, 1500, -8192, 20, 3, -900, 1, 2))
    limit = ((32767, 0, 0, 0, 0, 0, 0, 0), (0, 0, 0, -32767, 0, 0, 0, 0))                   # L1 = 65534: the bound
    with wn.Canceller(wr.CS16) as c:
        def step(k):
            got = _run_resident(nv, c, [(a[step.pos:step.pos + k], b[step.pos:step.pos + k])], [k])
            want = ref.push(a[step.pos:step.pos + k], b[step.pos:step.pos + k])
            assert np.array_equal(got[0], want), (step.pos, _first_difference(got[0], want))
            assert c.get(0) == _status(ref), step.pos
            step.pos += k
        step.pos = 0
        c.set(*some); ref.set(*some)                                       # in front of the first sample: held until block 4
        step(2 * B + 100)
        assert ref.w == some
        step(3 * B)                                                        # blocks 4 and 5 start: solved
        assert ref.solved == 2
        c.set_mode(wn.HOLD); ref.set_mode(wr.HOLD)
        held = ref.w
        step(2 * B)
        assert ref.w == held and ref.solved == 2
        c.set(*limit); ref.set(*limit)                                     # a calibrated set-up: set and hold, at the limits
        step(B + 17)
        assert ref.w == limit
        c.set_mode(wn.TRACK); ref.set_mode(wr.TRACK)
        step(n - step.pos)
        assert ref.solved == 4 and c.get(0)["mode"] == wn.TRACK
        arr = lambda v: (wn.C.c_int32 * 8)(*v)                             # noqa: E731
        zero = (0,) * 8
        for bad in (((32768,) + zero[1:], zero), (zero, zero[:7] + (-32768,)), ((32767, 1) + zero[2:], (0, 0, 32767) + zero[3:]), ((8192,) * 8, (1,) + zero[1:])):
            assert wn.lib.nvx_wanc_set(c._h, 0, arr(bad[0]), arr(bad[1])) == nv._native.ERR_ARG, bad
        assert wn.lib.nvx_wanc_set(c._h, 0, None, arr(zero)) == nv._native.ERR_ARG and wn.lib.nvx_wanc_set(c._h, 0, arr(zero), None) == nv._native.ERR_ARG
        assert wn.lib.nvx_wanc_set_mode(c._h, 0, 2) == nv._native.ERR_ARG and wn.lib.nvx_wanc_set_mode(c._h, 0, -1) == nv._native.ERR_ARG
        assert wn.lib.nvx_wanc_set_mode(c._h, 1, 0) == nv._native.ERR_ARG and wn.lib.nvx_wanc_set(c._h, 1, arr(zero), arr(zero)) == nv._native.ERR_ARG
        assert c.get(0) == _status(ref)


# ------------------------------------------------------------------------------------------------------------------ (h)
def test_scale_256_pairs(nv, wn):
    """256 pairs x 1.5 blocks of unsigned 8-bit samples at W = 4 with set weights, sixteen different pairs among them, every pair
    checked.  Two calls: a block, which a workgroup per pair takes (form 1), and the rest."""
    ns, n, kinds = 256, (B + B // 2) // 8 * 8, 16
    w = ((-300, 4000, -6000, 900, 2000, -100, 50, 7), (200, -3000, 5000, 1000, -700, 60, -20, 3))
    pairs = [wc.formatted_pair(n, 7000 + k, wr.CU8) for k in range(kinds)]
    refs = []
    for a, b in pairs:
        ref = wr.Canceller(wr.CU8)
        ref.set(*w)
        refs.append((ref.push(a, b), ref))
    d_main = nv.DeviceBuffer(ns * n * 2); d_sense = nv.DeviceBuffer(ns * n * 2); d_out = nv.DeviceBuffer(ns * n * 4)
    block_a, block_b = np.stack([a for a, _ in pairs]), np.stack([b for _, b in pairs])
    for s in range(0, ns, kinds):
        d_main.upload(block_a, s * n * 2); d_sense.upload(block_b, s * n * 2)

    class At:
        def __init__(self, ptr):
            self.ptr = ptr

    with wn.Canceller(wr.CU8, n_pairs=ns) as c:
        c.set(*w)
        c.resident(d_main, n, d_sense, n, B, d_out, n)
        assert c.debug_last_launch() == {"launches": 3, "chunks": 1, "tiles_per_chunk": 16, "records": 1, "form": 1}
        rest = n - B
        c.resident(At(d_main.ptr + B * 2), n, At(d_sense.ptr + B * 2), n, rest, d_out, n, B)
        assert c.debug_last_launch() == {"launches": 6, "chunks": 1, "tiles_per_chunk": 8, "records": 1, "form": 1}
        got = d_out.download(ns * n * 4, dtype=np.int16).reshape(ns, n, 2)
        status = {s: c.get(s) for s in (0, 127, 255)}
    d_main.free(); d_sense.free(); d_out.free()
    bad = [s for s in range(ns) if not np.array_equal(got[s], refs[s % kinds][0])]
    assert not bad, bad[:10]
    assert all(st == _status(refs[s % kinds][1]) for s, st in status.items()) and refs[0][1].w == w and refs[0][1].complete == 1


# ------------------------------------------------------------------------------------------------------------------ (i)
@pytest.mark.parametrize("fmt", [wr.CS16, wr.CS8], ids=["cs16", "cs8"])
def test_push_equals_resident(nv, wn, fmt):
    n = 5 * B + 3000
    pairs = [wc.formatted_pair(2 * n, 120 + s, fmt) for s in range(3)]
    refs = [wr.cancel(a, b, fmt) for a, b in pairs]
    with wn.Canceller(fmt, n_pairs=3) as c:
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


# ------------------------------------------------------------------------------------------------------------------ (j)
def test_span_alignment_overlap_and_position_errors_launch_nothing(nv, wn):
    ARG = nv._native.ERR_ARG
    n = 8192
    with wn.Canceller(wr.CU8, n_pairs=2) as c:
        d_a = nv.DeviceBuffer(2 * n * 2); d_b = nv.DeviceBuffer(2 * n * 2); d_out = nv.DeviceBuffer(2 * n * 4)
        one_in = nv.DeviceBuffer(n * 2); one_out = nv.DeviceBuffer(n * 4)
        both = nv.DeviceBuffer(4 * n * 4)                                     # inputs and output in one allocation
        c.timing(True)
        call = lambda *a: wn.lib.nvx_wanc_resident(c._h, *a, None)           # noqa: E731
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
            assert wn.lib.nvx_wanc_last_error() != b""
        assert b"overlaps" in wn.lib.nvx_wanc_last_error()
        c.debug_set_position(2 ** 62 - 100)
        assert call(A, n, Bp, n, n, O, n, 0) == ARG and b"2^62" in wn.lib.nvx_wanc_last_error()
        assert wn.lib.nvx_wanc_debug_set_position(c._h, 0, 2 ** 62) == ARG and wn.lib.nvx_wanc_debug_set_position(c._h, 2, 0) == ARG
        assert wn.lib.nvx_wanc_reset(c._h, 2) == ARG and wn.lib.nvx_wanc_get(c._h, -1, None) == ARG and wn.lib.nvx_wanc_get(c._h, 0, None) == ARG
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
        assert calls == 2 and ms > 0.0 and c.debug_last_launch()["launches"] == 6 and c.get(1)["samples"] == 2 * n
        for d in (d_a, d_b, d_out, one_in, one_out, both):
            d.free()
    for kw in (dict(device=99), dict(window_log2=3), dict(format=4), dict(n_pairs=0), dict(n_taps=6), dict(n_taps=32), dict(load_log2=7), dict(load_log2=21)):
        with pytest.raises(nv.NvxError) as e:
            wn.Canceller(**kw)
        assert e.value.code == ARG, kw


# ------------------------------------------------------------------------------------------------------------------ (k)
def test_seed_11_of_the_acceptance_case_on_the_device(nv, wn, oracle):
    """The pair of seed 11 (the noise over three echoes) through both cancellers on the device: the words are the CPU's.  Then
    the single-weight row and the multi-tap row as two streams of a two-chain handle: the 490 message arrives from the multi-tap
    row and not from the single-weight one, and the bits of all four chains are the oracle's on the same words."""
    import navtex_amd.anc as an
    t490 = ac.text()
    a, b = wc.pair(nv, 11)
    n = len(a)
    want, ref = wr.cancel(a, b)
    single, _ = ar.cancel(a, b)
    d_main = nv.DeviceBuffer(n * 4); d_sense = nv.DeviceBuffer(n * 4); d_rows = nv.DeviceBuffer(2 * n * 4)
    d_main.upload(a); d_sense.upload(b)
    with an.Canceller(ar.CS16) as c1, wn.Canceller(wr.CS16) as c:
        c1.resident(d_main, n, d_sense, n, n, d_rows, n)                    # row 0 of the handle's input
        c.resident(d_main, n, d_sense, n, n, d_rows, n, out_first=n)        # row 1
        got = d_rows.download(2 * n * 4, dtype=np.int16).reshape(2, n, 2)
        assert np.array_equal(got[0], single) and np.array_equal(got[1], want), _first_difference(got[1], want)
        assert c.get(0) == _status(ref) and ref.solved == n // B - 3 and ref.rejected == 0
    frames = n // nv.FRAME_IN
    with nv.Pipeline(n_streams=2, chain_mask=nv.CHAIN_518 | nv.CHAIN_490, max_frames=8) as p:
        for f0 in range(0, frames, 8):
            p.process_resident(d_rows, n, f0, min(8, frames - f0), hip_stream=p.hip_stream)
        p.fetch()
        bits = [(p.bits(s, 0), p.bits(s, 1)) for s in range(2)]
        msgs = [[m[3] for m in p.messages if m[0] == s and m[1] == 490] for s in range(2)]
    d_main.free(); d_sense.free(); d_rows.free()
    cpu = [ac.delivered(oracle, row, nv.FRAME_IN) for row in (single, want)]
    for s in range(2):
        assert bits[s] == cpu[s][1] and msgs[s] == cpu[s][0], s
    assert msgs[1] == [t490] and msgs[0] != [t490]
