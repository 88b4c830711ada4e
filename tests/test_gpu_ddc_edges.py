"""The down-converter bank's edges on the GPU (-m gpu): the shifts, shapes and plans tests/test_gpu_ddc.py does not reach.
The bank's kernel is a copy of the resampler's, not shared source, so tests/test_gpu_resample_edges.py protects none of it.
Every comparison is == on words against the restatement (tests/ddc_ref.py, run with the plan's own taps); the shape a case
is meant to launch is asserted on what the host handed the kernel (nvx_ddc_debug_last_launch), not on a copy of the host's
rule; every call goes through test_gpu_ddc._run (sentinels around the output rows, full scale behind n_in) or keeps its
discipline.

  a  a different shift in every cell of 3 inputs x 4 slices, set for all inputs and then cell by cell; push; one cell retuned
  b  every admissible shift as a slice of one input: 1963 slices at 96 kS/s, 4011 at 2.4 MS/s
  c  65535 rows: 255 inputs x 257 slices, a shift per cell
  d  the plan shapes the first file leaves out: the largest LDS launch, L = 1, L = 1008 and L = 630 with T = 30 from global memory
  e  the most workgroups a row can have: chunk indices up to 2047
  f  the bank's own conversion in front of the mixer: every float32 tie, all 256 values of both 8-bit formats
  g  the FIR accumulator at its extremes behind a mixing slice
  h  retunes with nothing in between: five calls on one stream without a host synchronisation"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import ddc_ref as dr
import resample_ref as rr
from test_gpu_ddc import FORMATS, FORMAT_IDS, SENTINEL, _At, _check, _random, _run, _same, _set_ks, _two_inputs, dd, rs            # noqa: F401  (dd, rs: the fixtures)
from test_gpu_resample_edges import _samples_for, _want_long, cf32_sweep_values, extreme_input, held

pytestmark = pytest.mark.gpu


def _hz(k, fi):
    return k * fi / dr.N                                                       # exact: N is a power of two


def _want_mixed_long(conv, taps, L, M, k):
    """dr.ddc of one long input from its reset: the restated mixer over the whole input, then the block-parallel resampler
    restatement of the mixed samples (they are int16 after the mixer's clamp)."""
    return _want_long(dr.mix(conv, k, 0).astype(np.int16), rr.CS16, taps, L, M)


# ---------------------------------------------------------------------------------------- a. a different shift in every cell
def _cell_shifts(fi):
    """(what set_shift(slice, hz) gives every input first, the [input][slice] shifts the single-cell calls leave).  Each
    of the four first values survives in exactly one input; every input has one k = 0, at a slice of its own; +k_range
    and -k_range stand in different inputs."""
    kr = dr.k_range(fi)
    base = (kr // 2, -(kr // 3), 37, -1)
    cells = [[0, base[1], base[2], kr],
             [base[0], 0, -kr, 64],
             [-(kr // 2) - 1, kr // 3 + 2, 0, base[3]]]
    return base, cells


@pytest.mark.parametrize("fi,fmt", [(2400000, rr.CU8), (250000, rr.CF32)], ids=["2400000-cu8", "250000-cf32"])
def test_a_different_shift_in_every_cell(nv, dd, rs, fi, fmt):
    """3 inputs x 4 slices, all three inputs carrying the SAME samples: the twelve rows differ only through k[input][slice],
    so a kernel that reads k[slice], or a push that forgets its input's row of k, gives some row another cell's words.  The
    nine shifts that are not 0 all differ; the three k = 0 cells (one per input, each at another slice: the bypass branch
    must be taken per cell too) give the same row by construction, and no other two rows are equal.  Then every input
    alone through nvx_ddc_push in cuts of its own (in the order 2, 0, 1; the inputs end on different history rows), then
    one cell of input 1 retuned and 5000 more samples resident: only that row follows the new k."""
    L, M, T, S, taps = rs.design(fi)
    n, more = 20011, 5000
    x = np.concatenate([_two_inputs(nv, fi, fmt, n, seed=61)[1], _random(fmt, more, np.random.default_rng(62))])
    conv = rr.convert(x, fmt)
    base, cells = _cell_shifts(fi)
    flat = [k for row in cells for k in row]
    assert flat.count(0) == 3 and len(set(flat)) == 10 and max(flat) == -min(flat) == dr.k_range(fi)
    assert len({row.index(0) for row in cells}) == 3

    def want(k, a, b):
        return dr.ddc(conv[a:b], taps, L, M, k, a, conv[:a])[0]
    first = {k: want(k, 0, n) for k in set(flat)}
    assert len({w.tobytes() for w in first.values()}) == 10, "two shifts give the same row: the case proves nothing"
    with dd.Ddc(fi, fmt, n_inputs=3, n_slices=4) as d:
        for s in range(4):
            assert d.set_shift(s, _hz(base[s], fi)) == _hz(base[s], fi)
        for i in range(3):
            for s in range(4):
                if cells[i][s] != base[s]:
                    assert d.set_shift(s, _hz(cells[i][s], fi), input=i) == _hz(cells[i][s], fi)
        for i in range(3):
            for s in range(4):
                assert d.get_shift(s, i) == (cells[i][s], _hz(cells[i][s], fi)), (i, s)
        got = _run(nv, d, [x[:n]] * 3, [n], pitch_extra=2, out_first=5)
        assert d.debug_last_launch()["inputs"] == 3 and d.debug_last_launch()["slices"] == 4
        for i in range(3):
            for s in range(4):
                _same(got[i, s], first[cells[i][s]], ("resident", i, s, cells[i][s]))
        # every input alone, from its reset
        d.reset()
        cuts = {2: (7, T - 1, n - T - 6), 0: (n - 4003, 4003), 1: (5000, 1, 3, n - 5004)}
        for i in (2, 0, 1):
            assert sum(cuts[i]) == n
            parts, pos = [], 0
            for c in cuts[i]:
                parts.append(d.push(i, x[pos:pos + c])); pos += c
            pushed = np.concatenate(parts, axis=1)
            assert d.debug_last_launch()["inputs"] == 1 and d.position(i)[0] == n
            for s in range(4):
                _same(pushed[s], got[i, s], ("push", i, s, cells[i][s]))
        # one cell of input 1 gets another shift; every other cell goes on as it was
        new_k = -777
        assert new_k not in flat and d.set_shift(3, _hz(new_k, fi), input=1) == _hz(new_k, fi)
        old_k, cells[1][3] = cells[1][3], new_k
        for i in range(3):
            for s in range(4):
                assert d.get_shift(s, i)[0] == cells[i][s], (i, s)
        rest = _run(nv, d, [x[n:]] * 3, [more], pitch_extra=1, out_first=2)
        for i in range(3):
            for s in range(4):
                _same(rest[i, s], want(cells[i][s], n, n + more), ("retuned", i, s, cells[i][s]))
        assert not np.array_equal(rest[1, 3], want(old_k, n, n + more))


# ------------------------------------------------------------------------------------------------ b. every admissible shift
@pytest.mark.parametrize("fi,fmt,n,slices,outs", [(96000, rr.CS16, 3300, 1963, 8663), (2400000, rr.CU8, 8200, 4011, 861)],
                         ids=["96000-cs16", "2400000-cu8"])
def test_every_admissible_shift(nv, dd, rs, fi, fmt, n, slices, outs):
    """One input, slice s at k = s - k_range: every value the index arithmetic j = (k (n mod N)) mod N, the half-turn
    negation and the padded LDS slot can be asked for, on full-scale random input, two tiles or more per row."""
    L, M, T, S, taps = rs.design(fi)
    kr = dr.k_range(fi)
    ks = tuple(range(-kr, kr + 1))
    assert len(ks) == slices and rr.outputs_after(n, L, M) == outs
    x = _random(fmt, n, np.random.default_rng(fi % 997))
    with dd.Ddc(fi, fmt, n_inputs=1, n_slices=slices) as d:
        _set_ks(d, ks, fi)
        got = _run(nv, d, [x], [n], pitch_extra=1, out_first=3)
        shape = d.debug_last_launch()
    assert (shape["slices"], shape["inputs"], shape["chunks"]) == (slices, 1, 1) and shape["tiles"] >= 2, shape
    conv = rr.convert(x, fmt)
    want = dr.ddc_slices(conv, taps, L, M, ks)
    for s in (0, 1, kr, kr + 1, slices - 1):                                   # the many-slice restatement is the per-slice one
        assert np.array_equal(want[s], dr.ddc(conv, taps, L, M, ks[s])[0]), s
    assert got.shape == (1,) + want.shape
    wrong = np.nonzero(np.any(got[0] != want, axis=(1, 2)))[0]
    assert len(wrong) == 0, (len(wrong), [ks[s] for s in wrong[:16]])


# ---------------------------------------------------------------------------------------------------------- c. 65535 rows
def test_65535_rows_with_a_shift_per_cell(nv, dd, rs):
    """The most rows a plan takes, 255 inputs x 257 slices at 96 kS/s, signed 8-bit: 200 samples per input under a seed of
    its own (525 outputs, one short tile), cell (i, s) at k = ((257 i + s) 37) mod 1963 - 981, sentinels around every row."""
    fi, fmt, ni, ns, n = 96000, rr.CS8, 255, 257, 200
    L, M, T, S, taps = rs.design(fi)
    kmax = dr.k_range(fi)
    ks = [[((i * ns + s) * 37) % (2 * kmax + 1) - kmax for s in range(ns)] for i in range(ni)]
    assert rr.outputs_after(n, L, M) == 525 and ni * ns == 65535 and len({k for row in ks for k in row}) == 2 * kmax + 1
    rows = [np.random.default_rng(9000 + i).integers(-128, 128, size=(n, 2), dtype=np.int8) for i in range(ni)]
    with dd.Ddc(fi, fmt, n_inputs=ni, n_slices=ns) as d:
        for i in range(ni):
            for s in range(ns):
                assert d.set_shift(s, _hz(ks[i][s], fi), input=i) == _hz(ks[i][s], fi)
        for i in range(ni):
            for s in range(ns):
                assert d.get_shift(s, i)[0] == ks[i][s], (i, s)
        got = _run(nv, d, rows, [n], pitch_extra=1, out_first=3)
        shape = d.debug_last_launch()
    assert (shape["slices"], shape["inputs"]) == (ns, ni) and shape["launches"] == 1, shape

    def check(i):
        want = dr.ddc_slices(rr.convert(rows[i], fmt), taps, L, M, ks[i])
        return [(i, int(s)) for s in np.nonzero(np.any(got[i] != want, axis=(1, 2)))[0]]
    with ThreadPoolExecutor(16) as ex:
        wrong = sum(ex.map(check, range(ni)), [])
    assert not wrong, (len(wrong), wrong[:10])
    for i, s in ((0, 0), (0, ns - 1), (1, 0), (127, 128), (ni - 1, ns - 1)):   # the many-slice restatement is the per-slice one
        assert np.array_equal(got[i, s], dr.ddc(rr.convert(rows[i], fmt), taps, L, M, ks[i][s])[0]), (i, s)


# --------------------------------------------------------------------------------------------------- d. the plan shapes
ALL_FORMATS = (100100, 1000250)
ONE_FORMAT = (2000000, 1920000, 1024000, 768000, 384000, 256000, 192000, 252000, 504000, 2016000, 1000400)
PLAN_CASES = [(fi, fmt) for fi in ALL_FORMATS for fmt in FORMATS] + [(fi, FORMATS[j % 4]) for j, fi in enumerate(ONE_FORMAT)]


@pytest.mark.parametrize("fi,fmt", PLAN_CASES, ids=[f"{fi}-{FORMAT_IDS[fmt]}" for fi, fmt in PLAN_CASES])
def test_the_plan_shapes_the_first_file_leaves_out(nv, dd, rs, fi, fmt):
    """The scheme of test_output_equals_the_restatement at the resampler's other rates: 100 100 S/s, the largest LDS
    launch (43 264 + 57 600 = 100 864 bytes: above the 64 KB a kernel has without nvx_ddc_prepare's attribute), 1 000 250
    and 1 000 400 S/s (T = 30, the taps from global memory, M of 4001 and 2501), L = 1 (the phase never advances), and the
    ordinary rates the first file does not run.  2 inputs x 3 slices, k at the end of the range, 0, and an odd one."""
    L, M, T, S, taps = rs.design(fi)
    n = 20011
    rows = _two_inputs(nv, fi, fmt, n, seed=fi % 1000 + fmt)
    kr = dr.k_range(fi)
    ks = (kr, 0, -(kr // 3) | 1)
    assert ks[2] % 2 == 1 and abs(ks[2] + kr / 3) <= 2
    with dd.Ddc(fi, fmt, n_inputs=2, n_slices=3) as d:
        assert (d.L, d.M, d.T) == (L, M, T)
        _set_ks(d, ks, fi)
        got = _run(nv, d, rows, [n - 4003, 4003], pitch_extra=3, out_first=7)
        shape = d.debug_last_launch()
    assert shape["launches"] == 2 and (shape["slices"], shape["inputs"]) == (3, 2), shape
    if fi == 100100:
        assert shape["taps_in_lds"] and shape["lds_bytes"] == 43264 + 57600, shape
    if fi in (1000250, 1000400):
        assert not shape["taps_in_lds"] and T == 30, shape
    if fi in (252000, 504000, 2016000):
        assert L == 1 and d.L == 1
    _check(got, rows, fmt, taps, L, M, ks)
    assert got[1, 1].any() and not np.array_equal(got[1, 0], got[1, 2])


# ------------------------------------------------------------------------------- e. the most workgroups a row can have
_memo = {}


def _length_for(n_out, L, M):
    """(samples, outputs) of the shortest input with at least n_out outputs.  At 96 kS/s a sample adds two or three
    outputs (L / M = 21 / 8), so not every count has a length: 4094 * 4096 + 100 and 1023 * 4096 + 100 have none, the
    next count has."""
    outs = rr.outputs_after(-(-n_out * M // L), L, M)
    assert 0 <= outs - n_out < -(-L // M)
    return _samples_for(outs, L, M), outs


def _long_row(rs, fi, n_out):
    """int16 full-scale random, the shortest input of at least n_out outputs at rate fi, and its conversion."""
    if fi not in _memo:
        L, M, T, S, taps = rs.design(fi)
        n, _ = _length_for(n_out, L, M)
        x = _random(rr.CS16, n, np.random.default_rng(71 + fi % 97))
        _memo[fi] = (x, rr.convert(x, rr.CS16))
    return _memo[fi]


LONG_96K, LONG_250K = 4094 * 4096 + 100, 2047 * 4096 + 100


@pytest.mark.parametrize("fi,n_out,shape_wanted", [(96000, LONG_96K, (16, 4095, 2, 2048)), (250000, LONG_250K, (16, 2048, 1, 2048))],
                         ids=["96000", "250000"])
def test_the_most_workgroups_a_row_can_have(nv, dd, rs, fi, n_out, shape_wanted):
    """1 input x 1 slice at k = k_range, int16: a one-row launch spreads its tiles over up to 2048 workgroups, and the
    chunk's start (q, r) comes from divmod<12>(r0 + blockIdx.x chunk_dr, L), built for exactly that bound.
    96 kS/s (the rate where an output costs the fewest input samples; 6.4 M samples): 4095 tiles of 4096 outputs over 2048
    workgroups of two tiles; the last workgroup holds one tile, and that tile is short (101 outputs).  The full length was
    taken, not the 2048-tile fallback: the reference -- the restated mixer over the whole input, then the block-parallel
    resampler restatement -- takes about 3 s.  At L = 21 the product blockIdx.x chunk_dr stays below 2^16 whatever the
    shape (chunk_dr = 16 here), and so it does at 100 100 S/s (4096 * 143 mod 360 = 8) and 1 000 250 S/s (16): a product
    cut to 16 bits passes all of them.
    250 kS/s (L = 126; 8.3 M samples): 2048 tiles, a workgroup each, chunk_dr = 4096 * 125 mod 126 = 62, the product up to
    126 914 and a carry out of r in every second workgroup."""
    fmt = rr.CS16
    L, M, T, S, taps = rs.design(fi)
    x, conv = _long_row(rs, fi, n_out)
    kr = dr.k_range(fi)
    outs = rr.outputs_after(len(x), L, M)
    assert outs == n_out + 1 == _length_for(n_out, L, M)[1]                    # n_out itself has no length at either rate
    with dd.Ddc(fi, fmt, n_inputs=1, n_slices=1) as d:
        _set_ks(d, (kr,), fi)
        got = _run(nv, d, [x], [len(x)], pitch_extra=1, out_first=1)
        shape = d.debug_last_launch()
    assert (shape["K"], shape["tiles"], shape["tiles_per_chunk"], shape["chunks"]) == shape_wanted, shape
    assert shape["tiles"] - (shape["chunks"] - 1) * shape["tiles_per_chunk"] == 1 and got.shape[2] % 4096 == 101
    _same(got[0, 0], _want_mixed_long(conv, taps, L, M, kr), "one slice")


def test_a_thousand_workgroups_for_each_of_two_rows(nv, dd, rs):
    """The first 1.6 M samples of the same input through two slices, k = 0 and -k_range: 1024 workgroups per row."""
    fi, fmt = 96000, rr.CS16
    L, M, T, S, taps = rs.design(fi)
    n, outs = _length_for(1023 * 4096 + 100, L, M)
    assert outs == 1023 * 4096 + 101
    x, conv = _long_row(rs, fi, LONG_96K)
    x, conv = x[:n], conv[:n]
    ks = (0, -dr.k_range(fi))
    with dd.Ddc(fi, fmt, n_inputs=1, n_slices=2) as d:
        _set_ks(d, ks, fi)
        got = _run(nv, d, [x], [n], pitch_extra=1, out_first=1)
        shape = d.debug_last_launch()
    assert shape["K"] == 16 and shape["chunks"] == 1024 and (shape["slices"], shape["inputs"]) == (2, 1), shape
    for s, k in enumerate(ks):
        _same(got[0, s], _want_mixed_long(conv, taps, L, M, k), (s, k))


# ---------------------------------------------------------------------------- f. the bank's own conversion in front of the mixer
def _quarter_turns(conv):
    """What the mixer makes of converted samples at k = 1024, from the header: the table steps through (32767, 0),
    (0, 32767), (-32767, 0), (0, -32767), so sample n comes out with its components swapped and signed by n mod 4, each as
    (v 32767 + 2^14) >> 15 (no clamp: |v| <= 32768 gives at most 32767)."""
    i, q = conv[:, 0], conv[:, 1]
    ph = np.arange(len(conv)) % 4
    r = lambda v: (v * 32767 + (1 << 14)) >> 15                                # noqa: E731
    return np.stack([np.select([ph == 0, ph == 1, ph == 2], [r(i), r(q), r(-i)], r(-q)),
                     np.select([ph == 0, ph == 1, ph == 2], [r(q), r(-i), r(-q)], r(i))], axis=1)


@pytest.mark.parametrize("fmt", [rr.CF32, rr.CU8, rr.CS8], ids=["cf32", "cu8", "cs8"])
def test_the_banks_own_conversion_in_front_of_the_mixer(nv, dd, rs, fmt):
    """unpack_group<FMT> exists only in the bank (v_perm_b32 for the 8-bit formats, cf32_to_i16 per component for CF32) and
    the resampler's conversion sweep does not pass through it.  252 kS/s in (L = M = 1): every float32 tie of the conversion
    with its neighbours and the special values, or all 256 values of an 8-bit format, each held for 16 samples, I in
    order and Q in reverse; slices at k = 0 (the resampler's conversion), 1024 and k_range.  At k = 1024 the mixer is a
    swap and a sign: the restatement's mixed samples are asserted to be that function of convert(value), so a wrong
    conversion is a wrong value there, not only a mismatch."""
    fi, hold = 252000, 16
    L, M, T, S, taps = rs.design(fi)
    assert (L, M) == (1, 1)
    if fmt == rr.CF32:
        values = cf32_sweep_values()
    else:
        values = np.arange(256).astype(np.uint8) if fmt == rr.CU8 else np.arange(-128, 128).astype(np.int8)
    x = held(values, hold)
    conv = rr.convert(x, fmt)
    assert np.array_equal(conv, np.repeat(rr.convert(np.stack([values, values[::-1]], axis=1), fmt), hold, axis=0))
    assert np.array_equal(dr.mix(conv, 1024, 0), _quarter_turns(conv))
    assert dr.table()[[0, 1024, 2048, 3072]].tolist() == [[32767, 0], [0, 32767], [-32767, 0], [0, -32767]]
    ks = (0, 1024, dr.k_range(fi))
    with dd.Ddc(fi, fmt, n_inputs=1, n_slices=3) as d:
        _set_ks(d, ks, fi)
        got = _run(nv, d, [x], [len(x)], pitch_extra=1, out_first=1)
        shape = d.debug_last_launch()
    assert shape["taps_in_lds"] and shape["slices"] == 3, shape
    for s, k in enumerate(ks):
        _same(got[0, s], _want_mixed_long(conv, taps, L, M, k), (s, k))


# ------------------------------------------------------------------------------ g. accumulator extremes behind the mixer
def _before_the_clamp(mixed, taps, L, M, at):
    """(acc + 2^14) >> 15 of the outputs `at` (all of the heaviest phase) from mixed samples [n, 2] int64; the accumulator
    asserted inside int32."""
    h = taps.astype(np.int64)
    ph = int(np.argmax(np.abs(h).sum(axis=1)))
    q = at * M // L
    assert np.all(at * M % L == ph)
    acc = np.zeros((len(at), 2), dtype=np.int64)
    for t in range(taps.shape[1]):
        acc += h[ph, t] * mixed[q - t]
    assert np.abs(acc).max() + (1 << (rr.S - 1)) < 2 ** 31
    return (acc + (1 << (rr.S - 1))) >> rr.S


def _turned_back(x, k):
    """int16 samples which the mixer at shift k turns into (about) x: exact for k = 1024, a swap and a sign with -(-32768)
    clipped to 32767; x e^(+2 pi i k n / N) in float64, rounded and clipped, otherwise."""
    i, q = x[:, 0].astype(np.int64), x[:, 1].astype(np.int64)
    n = np.arange(len(x), dtype=np.int64)
    if k == 1024:
        ph = n % 4
        y = np.stack([np.select([ph == 0, ph == 1, ph == 2], [i, -q, -i], q), np.select([ph == 0, ph == 1, ph == 2], [q, i, -q], -i)], axis=1)
    else:
        a = 2 * np.pi * ((k * n) % dr.N) / dr.N
        y = np.rint(np.stack([i * np.cos(a) - q * np.sin(a), q * np.cos(a) + i * np.sin(a)], axis=1)).astype(np.int64)
    return np.clip(y, -32768, 32767).astype(np.int16)


@pytest.mark.parametrize("fi", [100100, 3200000])
def test_accumulator_extremes_behind_the_mixer(nv, dd, rs, fi):
    """extreme_input's samples (rails matched in sign to the taps of the heaviest phase) as input 0, turned back by the
    k = 1024 sequence as input 1 and by k = 37 as input 2, through slices at k = (0, 1024, 37).  Cell (1, 1): the mixed
    windows stand within 2 of the rails, and the value before the clamp is beyond int16 on both sides in both components
    (asserted; 100 100 S/s: +-56 567 at all 280 outputs, |acc| 1.85e9 of int32's 2.147e9; 3.2 MS/s: +-41 662 at all 50).
    Cell (2, 2): rails on both components do not survive a rotation that is not a quarter turn -- the pre-rotated sample
    is clipped to the int16 square -- so it reaches less: 100 100 S/s -55 790 ... +55 256 with all 280 chosen outputs
    beyond int16, 3.2 MS/s -36 523 ... +36 523 with 41 of 50 beyond (computed on the CPU from the restatement); asserted
    only to pass int16 on at least one side.  The device equals the restatement in all nine cells, and in cell (0, 0) the
    resampler's extremes are met again."""
    fmt = rr.CS16
    L, M, T, S, taps = rs.design(fi)
    n = 40013
    x, at, before = extreme_input(fmt, taps, L, M, n, seed=fi % 997)
    assert len(at) >= 30
    ks = (0, 1024, 37)
    rows = [x, _turned_back(x, 1024), _turned_back(x, 37)]
    conv = [rr.convert(r, fmt) for r in rows]
    assert np.array_equal(_before_the_clamp(conv[0], taps, L, M, at), before)
    mixed = dr.mix(conv[1], 1024, 0)
    win = (at * M // L)[:, None] - np.arange(T)[None, :]
    assert np.all(np.minimum(32767 - mixed[win], mixed[win] + 32768) <= 2)
    b1 = _before_the_clamp(mixed, taps, L, M, at)
    assert np.all((b1 > 32767) | (b1 < -32768)) and (b1 > 32767).any(axis=0).all() and (b1 < -32768).any(axis=0).all(), b1
    b2 = _before_the_clamp(dr.mix(conv[2], 37, 0), taps, L, M, at)
    print(f"{fi}: k = 1024 |before| {np.abs(b1).min()} ... {np.abs(b1).max()}; k = 37 {b2.min()} ... {b2.max()}, "
          f"{int(np.any((b2 > 32767) | (b2 < -32768), axis=1).sum())} of {len(at)} outputs beyond int16")
    assert (b2 > 32767).any() or (b2 < -32768).any()
    want = [[dr.ddc(c, taps, L, M, k)[0] for k in ks] for c in conv]          # asserts every accumulator inside int32 itself
    assert np.array_equal(want[1][1][at], np.clip(b1, -32768, 32767)) and np.array_equal(want[0][0][at], np.clip(before, -32768, 32767))
    with dd.Ddc(fi, fmt, n_inputs=3, n_slices=3) as d:
        _set_ks(d, ks, fi)
        got = _run(nv, d, rows, [n], pitch_extra=1, out_first=1)
    for i in range(3):
        for s in range(3):
            _same(got[i, s], want[i][s], (i, s))


# ----------------------------------------------------------------------------------- h. retunes with nothing in between
@pytest.mark.parametrize("timed", [False, True], ids=["untimed", "timed"])
def test_retunes_with_nothing_in_between(nv, dd, rs, timed):
    """2.4 MS/s, int16, 1 input x 3 slices: the whole input uploaded once, then five resident calls of 40 004, 4, 20 004, 12
    and 30 004 samples on one non-null HIP stream, each reading at its offset (multiples of 4 samples: 16-byte aligned),
    all three shifts set anew before each, and no host synchronisation before the end.  Segment c of slice s equals the
    restatement with call c's k and the unmixed history carried.  upload_shifts must not rewrite the pinned row of shifts
    before the earlier asynchronous upload has read it (it waits on its k_uploaded event); this test cannot prove that
    protocol -- a copy that happens to be over in time passes without it -- but it is the only sequence in the suite whose
    result depends on it.  Sentinels in front of and behind the output rows; full scale behind the last call's input."""
    fi, fmt = 2400000, rr.CS16
    L, M, T, S, taps = rs.design(fi)
    calls = (40004, 4, 20004, 12, 30004)
    n = sum(calls)
    retunes = ((100, 0, -700), (-55, 300, 2005), (0, -2005, 64), (1, 0, -1), (1024, 37, 0))
    x = _random(fmt, n, np.random.default_rng(81))
    conv = rr.convert(x, fmt)
    total = rr.outputs_after(n, L, M)
    out_first, pitch_out = 3, total + 3 + 2
    d_in = nv.DeviceBuffer((n + 8) * 4); d_out = nv.DeviceBuffer(3 * pitch_out * 4)
    d_in.upload(np.concatenate([x, np.full((8, 2), 32767, dtype=np.int16)]))
    d_out.upload(np.full(3 * pitch_out, SENTINEL, dtype=np.uint32))
    with dd.Ddc(fi, fmt, n_inputs=1, n_slices=3) as d, nv.Pipeline(n_streams=1, chain_mask=nv.CHAIN_518, max_frames=1) as p:
        hs = p.hip_stream
        assert hs
        d.timing(timed)
        pos = made = 0
        for c, ks in zip(calls, retunes):
            for s, k in enumerate(ks):
                assert d.set_shift(s, _hz(k, fi)) == _hz(k, fi)
            assert pos % 4 == 0
            got = d.resident(_At(d_in.ptr + pos * 4), c, c, d_out, pitch_out, out_first + made, hip_stream=hs)
            assert got == rr.outputs_after(pos + c, L, M) - rr.outputs_after(pos, L, M)
            pos, made = pos + c, made + got
        assert made == total and d.debug_last_launch()["launches"] == 5 and d.position(0) == (n, total)
        nv.lib.nvx_device_sync(0)
        assert d.time_stats()[1] == (5 if timed else 0)
        words = d_out.download(3 * pitch_out * 4, dtype=np.uint32).reshape(3, pitch_out)
    d_in.free(); d_out.free()
    assert np.all(words[:, :out_first] == SENTINEL) and np.all(words[:, out_first + total:] == SENTINEL), "words outside the span were written"
    rows = np.ascontiguousarray(words[:, out_first:out_first + total]).view(np.int16).reshape(3, total, 2)
    for s in range(3):
        pos = made = 0
        hist = None
        for c, ks in zip(calls, retunes):
            want, hist = dr.ddc(conv[pos:pos + c], taps, L, M, ks[s], pos, hist)
            _same(rows[s, made:made + len(want)], want, ("call of", c, "slice", s, "k", ks[s]))
            pos, made = pos + c, made + len(want)
        assert made == total
