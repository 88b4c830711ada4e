"""The narrowband interpolator's unreached kernels and tap rows on the GPU (-m gpu), words == the restatement
(tests/narrow_ref.py) throughout, sentinels around every output row and the input at full scale behind every call's n_in
(narrow_cases._run_resident):
a. the eight kernels whose tap row is three 16-byte words (T = 18 .. 24), each at 72 000 S/s (T = 20: four zero taps in front
   of the row), at 67 200 S/s (T = 24: the row is full) and at one of 75 600, 70 000 and 73 332 S/s (T = 18, 22, 18; the last
   has the largest table a three-word row can have, 1000 rows, and a row step of 291 rows); 144 000 / 2, the plan of 72 000
   through rate_den 2; and the two paddings the other kernels never met: 84 000 S/s (T = 16, a full two-word row) and
   64 800 S/s (T = 26, six zero taps in front of a four-word row);
b. calls of 0, 1, T - 2, T - 1, T and more samples against one shot at T = 24 and T = 18, where the state row of T - 1 words is
   written partly from the one read; then one stream pushed alone;
c. the rails and full-scale random input at T = 24;
d. positions beyond 2^32 at T = 24, the first output at a phase that is not 0."""
from pathlib import Path

import numpy as np
import pytest

import narrow_cases as nc
import narrow_ref as nr
from narrow_cases import _first_difference, _run_resident, _same

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FORMAT_IDS = {nr.S16: "s16", nr.U8: "u8", nr.S8: "s8", nr.F32: "f32"}
KIND_IDS = {nr.IQ: "iq", nr.REAL: "real"}
RUNS = [(rate, fmt, kind) for rate, runs in nc.EDGE_RUNS.items() for fmt, kind in runs]


def _id(run):
    rate, fmt, kind = run
    return f"{rate[0]}_{rate[1]}-{FORMAT_IDS[fmt]}-{KIND_IDS[kind]}"


@pytest.fixture(scope="module")
def nb(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_narrow.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.narrow
    return navtex_amd.narrow


@pytest.fixture(scope="module")
def designs(nb):
    cache = {}
    def get(num, den=1):
        if (num, den) not in cache:
            cache[(num, den)] = nb.design(num, den)
        return cache[(num, den)]
    return get


def _lds_bytes(L, T):
    return L * (((T + 7) // 8) | 1) * 16 + (288 + 8200) * 4


# ------------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("run", RUNS, ids=_id)
def test_three_streams_of_three_tiles_and_a_ragged_fourth_at_the_unreached_rows(nv, nb, designs, run):
    """3 streams x (3 tiles + 37 samples), a seed each, spread over two workgroups.  A pitch larger than the data; out_first at
    each residue mod 4 (residue 0: the aligned 16-byte stores)."""
    rate, fmt, kind = run
    L, M, T, h = designs(*rate)
    assert (L, M, T) == nc.EDGE_PLANS[rate]
    rows = nc.edge_rows(rate, fmt, kind)
    n = len(rows[0])
    want = [nr.interpolate_all(row, h, L, M, fmt, kind)[0] for row in rows]
    with nb.Interpolator(*rate, format=fmt, kind=kind, n_streams=3) as c:
        assert (c.L, c.M, c.T) == (L, M, T)
        for out_first in (8, 5, 6, 7):
            c.reset()
            got = _run_resident(nv, c, rows, [n], pitch_extra=1 + out_first % 4, out_first=out_first)
            shape = c.debug_last_launch()
            assert (shape["chunks"], shape["tiles_per_chunk"], shape["form"], shape["windows"]) == (2, 2, 2, 256), shape
            assert shape["lds_bytes"] == _lds_bytes(L, T), shape
            _same(got, want, out_first)


# ------------------------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("fmt,kind", [(nr.S16, nr.IQ), (nr.U8, nr.REAL)], ids=["s16-iq", "u8-real"])
@pytest.mark.parametrize("rate", [(67200, 1), (75600, 1)], ids=["67200_T24", "75600_T18"])
def test_one_shot_equals_short_calls_and_push_equals_resident_at_three_word_rows(nv, nb, designs, rate, fmt, kind):
    """Calls of 0, 1, T - 2, T - 1, T, 1500, 0, 1 and 900 samples against one shot: the four calls behind the first are shorter
    than the T - 1 words of the state row, which is then written partly from the row read.  Then stream 1 pushed alone in
    calls of 1, 0, T - 1 and the rest."""
    L, M, T, h = designs(*rate)
    assert T == nc.EDGE_PLANS[rate][2]
    cuts = [0, 1, T - 2, T - 1, T, 1500, 0, 1, 900]
    n1, n2 = sum(cuts), 700
    rows = [nc.signal(fmt, kind, n1 + n2, 400 + 10 * fmt + s) for s in range(3)]
    want = [nr.interpolate_all(row, h, L, M, fmt, kind)[0] for row in rows]
    o1 = nr.outputs_after(n1, L, M)
    with nb.Interpolator(*rate, format=fmt, kind=kind, n_streams=3) as c:
        assert c.T == T
        got = _run_resident(nv, c, [row[:n1] for row in rows], cuts, pitch_extra=1, out_first=2)
        _same(got, [w[:o1] for w in want], "cuts")
        ref = nr.Interpolator(h, L, M, fmt, kind)
        assert np.array_equal(ref.push(rows[1][:n1]), want[1][:o1])
        pos = n1
        for cut in (1, 0, T - 1, n2 - T):
            out, exp = c.push(1, rows[1][pos:pos + cut]), ref.push(rows[1][pos:pos + cut])
            pos += cut
            assert out.dtype == np.int16 and np.array_equal(out, exp), (pos, cut, _first_difference(out, exp) if len(exp) else None)
            assert c.position(1) == (pos, nr.outputs_after(pos, L, M))
        assert pos == n1 + n2 and c.position(0) == (n1, o1)


# ------------------------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("fmt,kind", [(nr.S16, nr.IQ), (nr.F32, nr.REAL)], ids=["s16-iq", "f32-real"])
def test_the_rails_and_full_scale_random_input_at_a_full_three_word_row(nv, nb, designs, fmt, kind):
    """Windows matched in sign to the phase with the largest sum |h| (35 556 at 67 200 S/s), every second one and Q negated: the
    value before the clamp is +71 110 and -71 112 (float32 REAL: -70 328), beyond int16 on both sides by more than its width.
    And full-scale random input with the float32 specials.  Two calls cut at 301."""
    rate = (67200, 1)
    L, M, T, h = designs(*rate)
    assert T == 24
    rails = nc.rails(h, fmt, kind, 24)
    n = len(rails)
    rows = [rails, nc.full_scale(fmt, kind, n, 500 + fmt), nc.full_scale(fmt, kind, n, 600 + fmt)]
    refs = [nr.interpolate_all(row, h, L, M, fmt, kind) for row in rows]
    print("before the clamp:", refs[0][1].acc_max >> 14, refs[0][1].acc_min >> 14)
    assert refs[0][1].acc_max >> 14 > 70000 > 32767 and refs[0][1].acc_min >> 14 < -70000 < -32768
    assert refs[0][0][:, 0].max() == 32767 and refs[0][0][:, 0].min() == -32768
    if kind == nr.IQ:
        assert refs[0][0][:, 1].max() == 32767 and refs[0][0][:, 1].min() == -32768
    with nb.Interpolator(*rate, format=fmt, kind=kind, n_streams=3) as c:
        got = _run_resident(nv, c, rows, [301, n - 301], out_first=3)
        _same(got, [r[0] for r in refs], "rails")


# ------------------------------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("position", [2 ** 33 + 1001, 2 ** 40 + 6])
def test_positions_beyond_32_bits_at_a_full_three_word_row(nv, nb, designs, position):
    """600 samples in two calls from the position: silence in front of it, and the phase of its first output is the position's
    (M = 4: a position that is a multiple of 4, such as 2^32 - 1000, has phase 0; these have 1 and 2)."""
    rate = (67200, 1)
    L, M, T, h = designs(*rate)
    assert (nr.outputs_after(position, L, M) * M - position * L) % M != 0
    rows = [nc.signal(nr.S16, nr.IQ, 600, 80 + s) for s in range(2)]
    refs = [nr.Interpolator(h, L, M, position=position) for _ in rows]
    with nb.Interpolator(*rate, n_streams=2) as c:
        c.debug_set_position(position)
        assert c.position(1) == (position, nr.outputs_after(position, L, M))
        got = _run_resident(nv, c, rows, [222, 378])
        _same(got, [refs[s].push(rows[s]) for s in range(2)], position)
