"""The channel tap's unreached paths on the GPU (-m gpu), samples == the restatement (tests/tap_ref.py) throughout, sentinels
around every output row and the input at full scale behind every call's n_in (tap_cases._run_resident).  The tile of 128 outputs
in both forms (2000 S/s: taps wave-uniform; 2016 S/s: taps per lane) and the wave-uniform form with the audio filter of
T = 3602 (12 000 S/s REAL: 451 groups, 15 widenings, taps through SGPRs), none of which ran but one shot from a reset:
a. calls of 0, 1, T - 2, T - 1, T and more samples against one shot and against the restatement call by call, five calls in a row
   shorter than the history (the state loop copies state from state: 29 rounds of 128 threads at T = 3602), a last call of two
   tiles from a carried state; one input pushed alone, reset, brought back up and rejoining;
b. positions beyond 2^32 with odd shift and pitch steps, also at 12 000 S/s IQ (wave-uniform, T = 602);
c. the rails, a constant row at the negative rail and full-scale random input, also at 96 000 S/s (T = 32, G = 5: the row is
   mostly padding)."""
from pathlib import Path

import numpy as np
import pytest

import tap_cases as tc
import tap_ref as tr
from tap_cases import _flat, _run_resident, _same, _set_shifts

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
RAIL_SHIFTS = ((0.0, 14000.0), (0.0, -9000.0), (-14000.0, 5000.5), (60000.0, -100.0))     # per input and tap, Hz: k = 0 for the rails and the constant row


def _id(plan):
    return f"{'iq' if plan[1] == tr.IQ else 'real'}_{plan[0]}"


@pytest.fixture(scope="module")
def tp(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_tap.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.tap
    return navtex_amd.tap


@pytest.fixture(scope="module")
def designs(tp):
    cache = {}
    def get(fo, kind=tr.IQ):
        if (fo, kind) not in cache:
            cache[(fo, kind)] = tp.design(fo, kind)
        return cache[(fo, kind)]
    return get


def _assert_plan(c, fo, kind):
    """The last launch took the tile, the form and the filter length the case is about."""
    tile_out, form, T = tc.EDGE_PLANS[(fo, kind)]
    shape = c.debug_last_launch()
    assert (shape["tile_out"], shape["form"], shape["waves"], c.T) == (tile_out, form, tile_out // 64, T), shape
    return shape


# ------------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("plan", [(2000, tr.IQ), (2016, tr.IQ), (12000, tr.REAL)], ids=_id)
def test_cut_calls_the_carried_state_push_and_a_reset_input_rejoining(nv, tp, designs, plan):
    """2 inputs x 2 taps, a k = 0 and odd k among the shifts, an odd pitch step (REAL).  tap_cases.edge_cuts in resident calls
    against one shot and against the restatement call by call; then input 1 pushed alone in calls of 1, 0, T - 1 and 700
    samples; then reset, refused while it stands elsewhere, pushed back up on other data to where input 0 stands, and both in
    a resident call."""
    fo, kind = plan
    L, M, T, h = designs(fo, kind)
    tile_out = tc.EDGE_PLANS[plan][0]
    cuts = tc.edge_cuts(L, M, T, tile_out)
    n1, n2, n3 = sum(cuts), T + 700, T + 900
    assert n1 >= 3 * T + 9000 and all(cut < T - 1 for cut in cuts[6:11]) and tr.outputs_after(cuts[-1], L, M) > tile_out
    rows = tc.edge_rows(n1 + n2 + n3, fo)
    with tp.Tap(fo, kind, n_inputs=2, n_taps=2) as c:
        assert (c.L, c.M, c.T) == (L, M, T)
        ks, kps = _set_shifts(c, tc.EDGE_SHIFTS, kind, tc.EDGE_PITCHES)
        assert ks[0][0] == 0 and ks[0][1] % 2 == 1 and ks[1][0] % 2 == 1 and ks[1][1] % 2 == 1 and (kps is None or kps[0] % 2 == 1)
        refs = [tr.Tap(h, L, M, kind, ks[i], kps) for i in range(2)]
        one = [tr.tap_all(rows[i][:n1], h, L, M, kind, ks[i], kps)[0] for i in range(2)]
        got = _run_resident(nv, c, [row[:n1] for row in rows], cuts, pitch_extra=1, out_first=1)
        shape = _assert_plan(c, fo, kind)
        assert shape["tiles"] == 2 and shape["launches"] == sum(cut > 0 for cut in cuts)
        _same(got, _flat(one), "cuts against one shot")
        by_call = [[refs[i].push(rows[i][pos:pos + cut]) for pos, cut in zip(np.cumsum([0] + cuts), cuts)] for i in range(2)]
        _same(got, _flat([[np.concatenate([part[t] for part in by_call[i]]) for t in range(2)] for i in range(2)]), "cuts against the restatement call by call")
        # input 1 alone
        pos = n1
        for cut in (1, 0, T - 1, 700):
            _same(list(c.push(1, rows[1][pos:pos + cut])), refs[1].push(rows[1][pos:pos + cut]), ("pushed", pos))
            pos += cut
            assert c.position(1) == (pos, tr.outputs_after(pos, L, M))
        assert pos == n1 + n2 and c.position(0) == (n1, tr.outputs_after(n1, L, M))
        # reset: it stands elsewhere, the resident call is refused and launches nothing
        c.reset(1)
        assert c.position(1) == (0, 0) and c.get_shift(1, 1)[0] == ks[1][1]
        d = nv.DeviceBuffer(2 * 64 * 4); o = nv.DeviceBuffer(4 * 64 * 4)
        launches = c.debug_last_launch()["launches"]
        assert tp.lib.nvx_tap_resident(c._h, d.ptr, 64, 64, o.ptr, 64, 0, None, None) == nv._native.ERR_STATE
        assert b"same position" in tp.lib.nvx_tap_last_error() and c.debug_last_launch()["launches"] == launches
        d.free(); o.free()
        refs[1].reset()
        other = tc.signal(n1 + n3, 450 + fo)
        pos = 0
        for cut in (10, 1, 2000, n1 - 2011):
            _same(list(c.push(1, other[pos:pos + cut])), refs[1].push(other[pos:pos + cut]), ("back up", pos))
            pos += cut
        assert c.position(1) == c.position(0)
        tail = [rows[0][n1:n1 + n3], other[n1:]]
        got = _run_resident(nv, c, tail, [n3], out_first=2)
        _assert_plan(c, fo, kind)
        _same(got, _flat([refs[i].push(tail[i]) for i in range(2)]), "rejoined")


# ------------------------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("plan", [(2000, tr.IQ), (12000, tr.IQ), (12000, tr.REAL)], ids=_id)
@pytest.mark.parametrize("position", [2 ** 32 - 1000, 2 ** 40 + 6])
def test_positions_beyond_32_bits_at_the_small_tile_and_in_the_uniform_form(nv, tp, designs, position, plan):
    """T + 400 and 600 samples from the position, at least one output each: silence in front of it, the phase of its first
    output is the position's, and the mixer's and the pitch's indices are the true ones (odd steps)."""
    fo, kind = plan
    L, M, T, h = designs(fo, kind)
    cuts = [T + 400, 600]
    counts = [tr.outputs_after(position + sum(cuts[:j + 1]), L, M) - tr.outputs_after(position + sum(cuts[:j]), L, M) for j in range(2)]
    assert min(counts) >= 1
    rows = [tc.signal(sum(cuts), 80 + s + fo) for s in range(2)]
    with tp.Tap(fo, kind, n_inputs=2, n_taps=2) as c:
        ks, kps = _set_shifts(c, ((61.5, -20000.0), (922.9, 0.0)), kind, tc.EDGE_PITCHES)
        assert ks[0][0] % 2 == 1 and ks[1][0] % 2 == 1 and (kps is None or kps[0] % 2 == 1)
        refs = [tr.Tap(h, L, M, kind, ks[i], kps, position=position) for i in range(2)]
        c.debug_set_position(position)
        assert c.position(1) == (position, tr.outputs_after(position, L, M))
        got = _run_resident(nv, c, rows, cuts, out_first=1)
        _assert_plan(c, fo, kind)
        _same(got, _flat([refs[s].push(rows[s]) for s in range(2)]), position)


# ------------------------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("plan", [(2000, tr.IQ), (12000, tr.REAL), (96000, tr.IQ)], ids=_id)
def test_the_rails_a_constant_row_at_the_negative_rail_and_full_scale_random_input(nv, tp, designs, plan):
    """Four inputs x two taps in two calls cut at T + 301, out_first = 3: windows matched in sign to the phase with the largest
    sum |h|, every second one and Q negated, through k = 0 -- the value before the clamp is beyond int16 on both sides (+-59 900
    at 2000 S/s, +-53 100 at 12 kS/s REAL, +-49 200 at 96 kS/s), and for the long filters the sum needs more than 36 bits --;
    (-32768, -32768) throughout through k = 0, which makes every run of 256 low halves as large as it gets; and two full-scale
    random rows through shifted taps.  The largest run of 256 low halves, sum hl * 32768 (tap_cases.low_run, from the C
    design): 37 532 * 32768 = 1 229 848 576 at 2000 S/s, 49 490 * 32768 = 1 621 688 320 at 12 kS/s REAL, 4352 * 32768 =
    142 606 336 at 96 kS/s (32 taps), below 2^31 = 2 147 483 648 as tap_ref.check_split states.  At 96 kS/s six windows are 255
    samples, fewer than the first call: there the row has 24."""
    fo, kind = plan
    L, M, T, h = designs(fo, kind)
    rails = tc.rails(h, L, M, 6 if T > 32 else 24)
    n = len(rails)
    assert n > T + 301 + T
    rows = [rails, np.full((n, 2), -32768, dtype=np.int16), tc.full_scale(n, 500 + kind + fo), tc.full_scale(n, 600 + kind + fo)]
    run = tc.low_run(h) * 32768
    print("the largest run of 256 low halves:", tc.low_run(h), "* 32768 =", run)
    assert run < 2 ** 31
    with tp.Tap(fo, kind, n_inputs=4, n_taps=2) as c:
        ks, kps = _set_shifts(c, RAIL_SHIFTS, kind, (None, 2000.0))
        assert ks[0][0] == 0 and ks[1][0] == 0 and all(k != 0 for k in _flat(ks[2:]))
        refs = [tr.tap_all(rows[i], h, L, M, kind, ks[i], kps) for i in range(4)]
        print("before the clamp:", refs[0][1].acc_max >> 21, refs[0][1].acc_min >> 21)
        assert refs[0][1].acc_max >> 21 > 32767 and refs[0][1].acc_min >> 21 < -32768
        if T > 32:
            assert refs[0][1].acc_max > 1 << 36 and refs[1][1].acc_min <= -(1 << 36)
        if kind == tr.IQ:
            r0 = refs[0][0][0]
            assert {int(r0[:, 0].max()), int(r0[:, 0].min()), int(r0[:, 1].max()), int(r0[:, 1].min())} == {32767, -32768}
            assert int(refs[1][0][0].min()) == -32768
        got = _run_resident(nv, c, rows, [T + 301, n - T - 301], out_first=3)
        _assert_plan(c, fo, kind)
        _same(got, _flat([r[0] for r in refs]), "rails")
