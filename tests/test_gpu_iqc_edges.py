"""The IQ corrector's unreached paths on the GPU (-m gpu), words == the restatement (tests/iqc_ref.py) throughout, sentinels
around every output row, the input at full scale behind every call's n_in, and nvx_iqc_get == the restatement's state
(coefficients, mode, last reason, the window's five sums, samples, both counters) behind every stage:
a. the block-end sweep in all four formats: one run of 35 blocks in 44 calls (iqc_cases.sweep_cuts) in which a block ends
   1, 3, 4, ... 4095 samples into a call's first, second or third tile -- on and next to every lane-group, step and region
   edge -- seven times with the call ending 1, 5 or 90 samples behind it in the same tile, and six times with the call
   ending on it; the cut plan's coverage is asserted by iqc_cases.block_ends_in_tiles, here and on the CPU (tests/test_iqc.py);
b. W = 16 and W = 64 cut into calls: a call that completes no block, one that completes more than W, the first solve from
   the carried ring alone and from the ring and the call's records, slots that wrap; set, HOLD and TRACK; a stream
   restarted, pushed up alone and rejoining;
c. form 2 with three streams, W = 16, in CS8 and CF32, the chunk borders moved through the block by a first call of P
   samples: a block's end in every chunk's first tile, chunks that start on a tile edge in mid-block, block ends in wave 1
   of the chunks' last tile; the third call's first solves read the carried ring from every workgroup that needs them; one
   stream held at set coefficients across it.  A form-2 call whose chunks are longer than 32 tiles needs more than 65 536
   tiles in the grid, about 268 M samples: it is left out on purpose, and varying P moves the chunk borders through the
   block at a fraction of the cost;
d. the apply at the corners nvx_iqc_set admits, the sum in front of the shift at 83 % of 2^31 on either sign;
e. rejection reason 3 beside the other three, at W = 4 and W = 16."""
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import iqc_cases as ic
import iqc_ref as ir
import resample_ref as rr
from iqc_cases import _extremes
from test_gpu_iqc import FORMAT_IDS, FORMATS, _first_difference, _gain, _run_resident, _status

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
B, TILE = ir.BLOCK, ic.TILE


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


def _stage(nv, c, refs, rows, at, cuts, what, **kw):
    """Samples [at, at + sum(cuts)) of every row through nvx_iqc_resident in calls of `cuts` (test_gpu_iqc._run_resident)
    and through the restatements: the same words, and the same state behind them.  Returns where the next stage starts."""
    n = sum(cuts)
    got = _run_resident(nv, c, [row[at:at + n] for row in rows], cuts, **kw)
    for s, ref in enumerate(refs):
        want = ref.push(rows[s][at:at + n])
        assert np.array_equal(got[s], want), (what, "stream", s, "first difference at sample", at + _first_difference(got[s], want))
        assert c.get(s) == _status(ref), (what, "stream", s)
    return at + n


# ------------------------------------------------------------------------------------------ a. where a block ends in a tile
@lru_cache(maxsize=None)
def _sweep(fmt):
    rows = ic.sweep_rows(fmt)
    return rows, [ir.correct(row, fmt, 2) for row in rows]


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_a_block_ends_at_every_seam_of_a_tile(nv, iq, fmt):
    """iqc_cases.sweep_cuts, W = 4, two streams.  Every window solves, and to other coefficients than the one in front of
    it, in both rows: a sample corrected with the other side's coefficients, or summed into the other block, differs.  The
    calls whose n_a is a multiple of 4 store 16 bytes at a time (out_first = 0, rows a multiple of 4 words), the others
    word by word."""
    cuts = ic.sweep_cuts()
    splits, ragged, exact = ic.sweep_coverage(cuts)
    assert set(splits) >= set(ic.SWEEP_N_A) and len(ragged) >= 5 and exact >= 5
    assert {(n_a + ic.SWEEP_SHORT[n_a]) % 8 == 0 for n_a in ragged} == {True, False}            # calls that end on a lane's group, and inside one
    rows, refs = _sweep(fmt)
    n = len(rows[0])
    for _, ref in refs:
        coefs = [h[1] for h in ref.history]
        assert ref.solved == n // B - 3 and ref.rejected == 0 and all(a != b for a, b in zip(coefs, coefs[1:]))
    with iq.Corrector(fmt, n_streams=2, window_log2=2) as c:
        got = _run_resident(nv, c, rows, cuts, pitch_extra=-n % 4)
        for s in range(2):
            assert np.array_equal(got[s], refs[s][0]), (s, _first_difference(got[s], refs[s][0]))
            assert c.get(s) == _status(refs[s][1]), s


# ------------------------------------------------------------------------------------------ b. the longer windows in calls
def test_w16_across_calls_hold_and_a_restarted_stream(nv, iq):
    """CU8, two streams from position 2^40 + 5 + 7 B: slot0 starts at 7 and wraps.  Calls of 3.3, 0.2 (no block completes:
    done == 0), 12.6 (the sixteenth block completes inside: the first solve from three ring slots and the call's records),
    1.0, 17.4 (done > W: the ring is replaced whole) and 5.5 blocks.  Then set and HOLD for two blocks, TRACK again; then
    stream 1 restarted -- nvx_iqc_reset, and the position hook, as 2^40 samples cannot be pushed -- and pushed up alone to
    where stream 0 stands, and a last call of both."""
    start = 2 ** 40 + 5 + 7 * B
    cuts = [int(3.3 * B) + 1, int(0.2 * B) + 3, int(12.6 * B) + 2, B, int(17.4 * B) + 5, int(5.5 * B) + 1]
    ends = np.cumsum([5] + cuts)
    assert [int(b // B - a // B) for a, b in zip(ends, ends[1:])] == [3, 0, 13, 1, 17, 6]
    hold, track, back, tail = 2 * B + 11, B + B // 2, 2 * B + 4321, B + 20000
    n = sum(cuts) + hold + track + tail
    rows = [rr.to_format(ic.impaired_noise(n, 930 + s, amp=6000 - 2500 * s), ir.CU8, gain=3.0) for s in range(2)]
    alone = rr.to_format(ic.impaired_noise(back, 935), ir.CU8, gain=3.0)
    refs = [ir.Corrector(ir.CU8, 4, start) for _ in rows]
    with iq.Corrector(ir.CU8, n_streams=2, window_log2=4) as c:
        c.debug_set_position(start)
        at = _stage(nv, c, refs, rows, 0, cuts, "six calls", pitch_extra=1, out_first=3)
        for ref in refs:                                       # block starts 16 .. 40 behind the position are solved
            assert ref.solved == (5 + at - 1) // B - 15 == 25 and ref.rejected == 0 and len({h[1] for h in ref.history}) == 25
        c.set(-77, 310, -900, 17500); c.set_mode(iq.HOLD)
        for ref in refs:
            ref.set(-77, 310, -900, 17500); ref.set_mode(ir.HOLD)
        at = _stage(nv, c, refs, rows, at, [hold], "HOLD")
        assert refs[0].coef == (-77, 310, -900, 17500) and refs[0].solved == 25
        c.set_mode(iq.TRACK)
        for ref in refs:
            ref.set_mode(ir.TRACK)
        at = _stage(nv, c, refs, rows, at, [track], "TRACK again")
        assert refs[0].solved == 26 and refs[0].coef != (-77, 310, -900, 17500)
        c.reset(1)
        assert c.position(1) == 0 and c.position(0) == start + at and c.get(1)["coefficients"] == ir.IDENTITY
        c.debug_set_position(start + at - back, stream=1)
        refs[1].reset(start + at - back)
        pos = 0
        for cut in (B - 7, 1, back - B + 6):
            got, want = c.push(1, alone[pos:pos + cut]), refs[1].push(alone[pos:pos + cut])
            assert np.array_equal(got, want), ("stream 1 alone", pos + _first_difference(got, want))
            pos += cut
        assert pos == back and c.position(1) == start + at and c.get(1) == _status(refs[1])
        at = _stage(nv, c, refs, rows, at, [tail], "both again", out_first=1)
        assert at == n and refs[1].coef == ir.IDENTITY and refs[0].solved > refs[1].solved


def test_w64_across_calls_the_first_solve_from_the_carried_ring_alone(nv, iq):
    """CS16, one stream, 70 blocks and 1234 samples: calls of 10.3, 0.5, 30 and 23.2 blocks up to the end of block 63, then block 64 as a
    call of its own -- its coefficients are solved from all 64 lanes of the carried ring -- then the rest, whose slots wrap
    past 64 and whose solves take ring slots and records together."""
    cuts = [int(10.3 * B) + 3, B // 2 + 1, 30 * B - 7]
    cuts += [64 * B - sum(cuts), B, 5 * B + 1234]
    n = sum(cuts)
    assert all(cut > 0 for cut in cuts) and sum(cuts[:4]) == 64 * B and n // B == 70
    row = ic.impaired_noise(n, 940)
    ref = ir.Corrector(ir.CS16, 6)
    with iq.Corrector(ir.CS16, window_log2=6) as c:
        _stage(nv, c, [ref], [row], 0, cuts, "six calls", pitch_extra=2, out_first=5)
    assert ref.solved == n // B - 64 + 1 == 7 and ref.rejected == 0 and len({h[1] for h in ref.history}) == 7


# ---------------------------------------------------------------------------------------------- c. form 2 beyond its case
FORM2_FIRST = {"block-end-in-first-tile": B - 100, "tile-edge-mid-block": 5 * TILE, "wave-1-of-last-tile": 2596}
FORM2_CALLS = (24 * B, 20 * B)


@lru_cache(maxsize=None)
def _form2_rows(fmt):
    n = max(FORM2_FIRST.values()) + sum(FORM2_CALLS)
    return [rr.to_format(ic.impaired_noise(n, 950 + 10 * fmt + s, amp=6000 - 2000 * s), fmt, gain=_gain(fmt)) for s in range(2)] + [_extremes(fmt, n, 955 + fmt)[2]]


@pytest.mark.parametrize("first", list(FORM2_FIRST), ids=list(FORM2_FIRST))
@pytest.mark.parametrize("fmt", [ir.CS8, ir.CF32], ids=["cs8", "cf32"])
def test_form_2_with_three_streams_and_the_chunk_borders_moved_through_the_block(nv, iq, fmt, first):
    """A call of P samples (one chunk: it is shorter than 33 tiles), then 24 blocks in 12 chunks and 20 blocks in 10, of 32
    tiles each.  The second call solves from its own records (block 16 of the stream on), the third from the first: its
    first sixteen blocks reach back into the carried ring, each from the workgroups that touch it.  In the first parameter
    set stream 1 is set and held in front of the third call.  A block counted twice or not at all across a chunk border
    shows in the counters."""
    P = FORM2_FIRST[first]
    ends = ic.block_ends_in_tiles(P, FORM2_CALLS[0])
    where = {((B - P % B + k * B) // TILE % 32, n_a) for k, (n_a, _) in enumerate(ends)}
    assert where == {"block-end-in-first-tile": {(0, 100), (16, 100)}, "tile-edge-mid-block": set(), "wave-1-of-last-tile": {(15, 1500), (31, 1500)}}[first]
    assert len(ends) == (0 if first == "tile-edge-mid-block" else 24)
    n = P + sum(FORM2_CALLS)
    rows = [row[:n] for row in _form2_rows(fmt)]
    refs = [ir.Corrector(fmt, 4) for _ in rows]
    form1 = {"chunks": 1, "tiles_per_chunk": (P + TILE - 1) // TILE, "records": 1, "form": 1}
    form2 = lambda chunks: {"chunks": chunks, "tiles_per_chunk": 32, "records": 2 * chunks + 1, "form": 2}     # noqa: E731
    with iq.Corrector(fmt, n_streams=3, window_log2=4) as c:
        at = _stage(nv, c, refs, rows, 0, [P], "the first call", pitch_extra=-n % 4)
        assert c.debug_last_launch() == dict(form1, launches=2)
        at = _stage(nv, c, refs, rows, at, [FORM2_CALLS[0]], "24 blocks")
        assert c.debug_last_launch() == dict(form2(12), launches=4)
        assert all(ref.solved + ref.rejected == (P + 24 * B - 1) // B - 15 for ref in refs)
        if first == "block-end-in-first-tile":
            c.set(150, -90, 1200, 15500, stream=1); c.set_mode(iq.HOLD, stream=1)
            refs[1].set(150, -90, 1200, 15500); refs[1].set_mode(ir.HOLD)
        held = refs[1].solved
        at = _stage(nv, c, refs, rows, at, [FORM2_CALLS[1]], "20 blocks", out_first=-at % 4)
        assert c.debug_last_launch() == dict(form2(10), launches=6)
    assert refs[0].solved + refs[0].rejected == (n - 1) // B - 15 and refs[0].solved >= 28
    assert (refs[1].solved == held and refs[1].coef == (150, -90, 1200, 15500)) == (first == "block-end-in-first-tile")


# ------------------------------------------------------------------------------------ d. the apply at its arithmetic limits
CORNERS = ((-32768, -32768, 5462, 21845), (32767, 32767, 5462, 21845), (-32768, 32767, -5462, 12288))


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_the_apply_at_the_corners_of_set(nv, iq, fmt):
    """HOLD; the lowest value throughout, the rails alternating and full-scale random input, each stream at one corner of
    what nvx_iqc_set admits, and the corners rotated over the streams.  With I = Q = 32767 and dI = dQ = -32768 the sum in
    front of the shift is 27 307 * 65 535 + 8192 = 1 789 572 437, both operands of either multiply 17 bits wide."""
    n = 3 * TILE + 5
    rows = _extremes(fmt, n, 600 + fmt)
    acc = []
    for turn in range(3):
        refs = [ir.Corrector(fmt, 2) for _ in rows]
        with iq.Corrector(fmt, n_streams=3, window_log2=2) as c:
            c.set_mode(iq.HOLD)
            for s, ref in enumerate(refs):
                dI, dQ, c_i, c_q = CORNERS[(s + turn) % 3]
                c.set(dI, dQ, c_i, c_q, stream=s)
                ref.set_mode(ir.HOLD); ref.set(dI, dQ, c_i, c_q)
                x = rr.convert(rows[s], fmt)
                acc.append(c_q * (x[:, 1] - dQ) + c_i * (x[:, 0] - dI) + 8192)
            _stage(nv, c, refs, rows, 0, [2 * TILE + 3, TILE + 2], ("corners turned by", turn), out_first=turn)
            assert all(ref.coef == CORNERS[(s + turn) % 3] and ref.solved + ref.rejected == 0 for s, ref in enumerate(refs))
    if fmt == ir.CS16:
        assert max(int(a.max()) for a in acc) == 1789572437 and min(int(a.min()) for a in acc) < -1789000000


# ------------------------------------------------------------------------------------------------ e. rejection reason 3
@pytest.mark.parametrize("window_log2", [2, 4], ids=["w4", "w16"])
def test_the_rejection_reasons_with_reason_3(nv, iq, window_log2):
    """The three rows of test_gpu_iqc.test_the_rejection_reasons and I = 5 i, Q = i, whose v is not positive: W + 1 blocks and
    100 samples in two calls, so that both solves read the carried ring."""
    W = 1 << window_log2
    n = (W + 1) * B + 100
    rows = [ic.silence_with_dc(n), ic.q_equals_i(n, 61), ic.q_three_i_rotated(n, 62), ic.q_fifth_of_i(n, 63)]
    refs = [ir.Corrector(ir.CS16, window_log2) for _ in rows]
    with iq.Corrector(ir.CS16, n_streams=4, window_log2=window_log2) as c:
        _stage(nv, c, refs, rows, 0, [W * B - 1000, n - W * B + 1000], "two calls")
    assert [ref.reason for ref in refs] == [1, 2, 4, 3] and all(ref.rejected == 2 and ref.solved == 0 and ref.coef[2:] == (0, 16384) for ref in refs)
