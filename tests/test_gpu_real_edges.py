"""The real-input converter's unreached paths on the GPU (-m gpu), words == the restatement (tests/real_ref.py) throughout,
sentinels around every output row and the input at full scale behind every call's n_in (real_cases._run_resident):
a. the 16-byte stores over three streams in every format -- every row's first word of the call 16-byte aligned and the pitch
   a multiple of 4 words, both asserted at the call -- at a length whose last pair lies in wave 2, inside a lane's group of
   loads (of 4 and of 8 pairs) and three words into a store group, which is then stored word by word; and at a multiple of 4
   that is none of 8.  Once in one call and once in two calls cut at an odd number of pairs: the second starts on a word
   that is not aligned and stores the same data word by word;
b. three chunks of 4, 4 and 1 tiles in every format: a later chunk's halo from the input (float32: the loads step by step),
   and a last chunk of one ragged tile;
c. calls of 1, 27, 28 and 29 pairs against the history of 28, and positions beyond 2^32, in unsigned 8-bit and float32."""
from functools import lru_cache
from pathlib import Path

import pytest

import real_cases as rc
import real_ref as rf
from real_cases import _run_resident, _same

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FORMATS = (rf.S16, rf.U8, rf.S8, rf.F32)
FORMAT_IDS = ("s16", "u8", "s8", "f32")
T = rc.TILE                               # outputs of a tile


@pytest.fixture(scope="module")
def rl(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_real.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.real
    assert navtex_amd.real.TILE == T
    return navtex_amd.real


# ------------------------------------------------------------------------------------------------------------------ (a)
@lru_cache(maxsize=None)
def _vec(fmt, n_out):
    rows = rc.vec_rows(fmt, n_out)
    return rows, [rf.convert_all(row, fmt)[0] for row in rows]


@pytest.mark.parametrize("n_out", rc.VEC_OUTPUTS, ids=["2T+2967", "2T+1028"])
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_the_16_byte_stores_over_three_streams_and_an_end_inside_wave_2(nv, rl, fmt, n_out):
    """3 streams x n_out outputs, out_first 0 and 4 and a pitch that is a multiple of 4 words.  2 T + 2967: the last pair in wave 2
    -- with 4 pairs per lane step 3, lane 37, three pairs into the group; with 8 step 1, lane 50, seven pairs in -- and the
    store group cut after 3 words.  2 T + 1028: the group of 8 pairs cut after 4, the store group whole."""
    spt = 8 if fmt in (rf.U8, rf.S8) else 4
    if n_out == 2 * T + 2967:
        assert rc.end_of_call(n_out, spt) == {4: ((2, 3, 37), 3, 3), 8: ((2, 1, 50), 7, 3)}[spt]
    else:
        assert rc.end_of_call(n_out, spt) == ((1, 0, 0), 4, 4) and n_out % 8 == 4
    assert rc.VEC_CUT % 2 == 1 and rc.end_of_call(rc.VEC_CUT, spt)[1] < spt
    rows, want = _vec(fmt, n_out)
    for out_first in (0, 4):
        pitch_extra = -(out_first + n_out) % 4 or 4
        for cuts, aligned in (([2 * n_out], [True]), ([2 * rc.VEC_CUT, 2 * (n_out - rc.VEC_CUT)], [True, False])):
            with rl.Converter(fmt, n_streams=rc.VEC_STREAMS) as c:
                got = _run_resident(nv, c, rows, cuts, pitch_extra=pitch_extra, out_first=out_first, aligned=aligned)
                assert c.debug_last_launch() == {"launches": len(cuts), "chunks": 1, "tiles_per_chunk": -(-(cuts[-1] // 2) // T), "form": 1}
                _same(got, want, (out_first, cuts))


# ------------------------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_two_streams_spread_over_three_chunks_in_every_format(nv, rl, fmt):
    """2 streams x (8 T + 5) outputs behind a first call of 38 samples: three workgroups a stream, of 4, 4 and 1 tiles; the
    second and third take their halo from the input, the third has one tile of five outputs."""
    first, n = 38, 2 * (8 * T + 5)
    rows = [rc.signal(fmt, first + n, 70 + 10 * fmt + s) for s in range(2)]
    want = [rf.convert_all(row, fmt)[0] for row in rows]
    with rl.Converter(fmt, n_streams=2) as c:
        got = _run_resident(nv, c, rows, [first, n], pitch_extra=1, out_first=1)
        assert c.debug_last_launch() == {"launches": 2, "chunks": 3, "tiles_per_chunk": 4, "form": 2}
        _same(got, want, "chunks")


# ------------------------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("fmt", [rf.U8, rf.F32], ids=["u8", "f32"])
def test_calls_shorter_and_longer_than_the_history_outside_s16(nv, rl, fmt):
    """Calls of 2, 54, 56, 58 and 0 samples and the rest: 1, 27, 28 and 29 pairs against a history of 28; the first two write
    the state row partly from the one read."""
    cuts = [2, 54, 56, 58, 0]
    n = 2 * (T + 77)
    cuts = cuts + [n - sum(cuts)]
    rows = [rc.signal(fmt, n, 410 + 10 * fmt + s) for s in range(3)]
    want = [rf.convert_all(row, fmt)[0] for row in rows]
    with rl.Converter(fmt, n_streams=3) as c:
        _same(_run_resident(nv, c, rows, cuts, out_first=1), want, "cuts")


@pytest.mark.parametrize("position", [2 ** 32 - 1000, 2 ** 40 + 6])
@pytest.mark.parametrize("fmt", [rf.U8, rf.F32], ids=["u8", "f32"])
def test_positions_beyond_32_bits_outside_s16(nv, rl, fmt, position):
    """60 samples in two calls of 11 and 19 pairs from the position: silence in front of it, both calls shorter than the
    history, and only the position's parity enters the sign.  Inverted for unsigned 8-bit at 2^40 + 6 and float32 at
    2^32 - 1000."""
    invert = int((fmt == rf.U8) == (position == 2 ** 40 + 6))
    rows = [rc.full_scale(fmt, 60, 80 + fmt), rc.signal(fmt, 60, 81 + fmt)]
    refs = [rf.Converter(fmt, invert, position) for _ in rows]
    with rl.Converter(fmt, n_streams=2, invert=invert) as c:
        c.debug_set_position(position)
        assert c.position(1) == (position, position // 2)
        got = _run_resident(nv, c, rows, [22, 38])
        _same(got, [refs[s].push(rows[s]) for s in range(2)], (position, invert))
