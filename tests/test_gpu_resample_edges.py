"""The resampler's edges on the GPU (-m gpu): the launch shapes, plans and magnitudes tests/test_gpu_resample.py does not reach.
Every comparison is == on words against the restatement (tests/resample_ref.py, run with the plan's own taps); the shape a
case is meant to launch is asserted on what the host handed the kernel (nvx_resample_debug_last_launch), not on a copy of
the host's rule.

  a  several tiles per workgroup in form 2, a shorter last chunk, about 1366 chunks; the same input in form 1 and cut in three
  b  every plan shape: K = 2, L = 1, the largest L, T = 30 with the taps in global memory, the largest LDS launch
  c  the accumulator at its extremes and the clamp on both sides
  d  every float32 rounding tie of CF32, its neighbours and the special values; all 256 values of CU8 and CS8
  e  a stream past position 2^32 in calls of 2^30 samples
  f  65535 streams
(g, nothing read behind n_in, is in _run_resident itself; h, the output-count limit, in test_span_errors_launch_nothing.)"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import resample_ref as rr
from test_gpu_resample import FORMATS, FORMAT_IDS, _inputs, _run_resident, _want, rs            # noqa: F401  (rs: the fixture)

pytestmark = pytest.mark.gpu
FORMS = pytest.mark.parametrize("form", [1, 2], ids=["per-stream", "spread"])


def _full_scale(fmt, n, seed):
    rng = np.random.default_rng(seed)
    if fmt == rr.CF32:
        return rng.uniform(-1.3, 1.3, size=(n, 2)).astype(np.float32)
    info = np.iinfo(rr.DTYPES[fmt])
    return rng.integers(info.min, info.max + 1, size=(n, 2), dtype=rr.DTYPES[fmt])


def _want_long(row, fmt, taps, L, M, block=1 << 19):
    """resample_all of one long stream, its blocks side by side: a block's history is the T-1 samples in front of it."""
    x = rr.convert(row, fmt)
    T = taps.shape[1]
    with ThreadPoolExecutor(16) as ex:
        parts = list(ex.map(lambda c: rr.resample(x[c:c + block], taps, L, M, c, x[max(0, c - (T - 1)):c])[0], range(0, len(x), block)))
    return np.concatenate(parts)


def _samples_for(n_out, L, M):
    """The most input samples that give exactly n_out outputs."""
    n = n_out * M // L
    while rr.outputs_after(n + 1, L, M) <= n_out:
        n += 1
    while rr.outputs_after(n, L, M) > n_out:
        n -= 1
    assert rr.outputs_after(n, L, M) == n_out
    return n


def _same(got, want, what=""):
    for s in range(len(want)):
        assert got[s].shape == want[s].shape and np.array_equal(got[s], want[s]), (what, s, int(np.argmax(np.any(got[s] != want[s], axis=1))))


# ------------------------------------------------------------------------------------------- a. several tiles per chunk
_memo = {}


def _memo_get(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def _case_i(nv, rs):
    fi, n, ns = 96000, 40013, 300
    L, M, T, S, taps = rs.design(fi)
    rows = [_inputs(nv, fi, rr.CS16, n, seed=s)[s % 4] for s in range(ns)]
    x = np.stack(rows)
    want = rr.resample_streams(rr.convert(x.reshape(-1, 2), rr.CS16).reshape(x.shape), taps, L, M, out_block=256)
    assert want.shape == (ns, 105035, 2)
    for s in (0, 1, 2, 3, ns - 1):                                             # the many-stream restatement is the per-stream one
        assert np.array_equal(want[s], rr.resample_all(rows[s], rr.CS16, taps, L, M))
    return rows, want


@pytest.mark.parametrize("cut", ["one-call", "three-calls"])
@FORMS
def test_several_tiles_per_chunk_300_streams(nv, rs, form, cut):
    """(i) 96 kS/s, int16, 300 streams of 40013 samples: 26 tiles of 4096 outputs over 7 workgroups of 4 tiles, the last of 2."""
    rows, want = _memo_get("i", lambda: _case_i(nv, rs))
    n = len(rows[0])
    chunks = [n] if cut == "one-call" else [10007, 5, n - 10012]
    with rs.Resampler(96000, rr.CS16, n_streams=len(rows)) as r:
        r.set_form(form)
        got = _run_resident(nv, r, rows, chunks, pitch_extra=1, out_first=3)
        last = r.debug_last_launch()
    if form == 2 and cut == "one-call":
        assert (last["K"], last["tiles"], last["tiles_per_chunk"], last["chunks"]) == (16, 26, 4, 7), last
        assert last["tiles"] % last["tiles_per_chunk"] == 2
    elif form == 2:
        assert last["tiles_per_chunk"] >= 2 and last["tiles"] % last["tiles_per_chunk"] != 0, last
    else:
        assert last["chunks"] == 1 and last["tiles_per_chunk"] == last["tiles"], last
    _same(got, want, (form, cut))


def _case_long(rs, fi, fmt, tiles, K, seed):
    L, M, T, S, taps = rs.design(fi)
    n = _samples_for(tiles * 256 * K, L, M)
    row = _full_scale(fmt, n, seed)
    return row, _want_long(row, fmt, taps, L, M)


@FORMS
def test_several_tiles_per_chunk_one_long_stream(nv, rs, form):
    """(ii) 2.048 MS/s, unsigned 8-bit, one stream of 4097 tiles (34.1 M samples): 3 tiles per workgroup, 1366 workgroups, the
    last of 2 tiles -- the chunk offset at block indices up to 1365."""
    row, want = _memo_get("ii", lambda: _case_long(rs, 2048000, rr.CU8, 4097, 4, 11))
    assert len(want) == 4195328
    with rs.Resampler(2048000, rr.CU8) as r:
        r.set_form(form)
        got = _run_resident(nv, r, [row], [len(row)])
        last = r.debug_last_launch()
    if form == 2:
        assert (last["K"], last["tiles"], last["tiles_per_chunk"], last["chunks"]) == (4, 4097, 3, 1366), last
        assert last["tiles"] % last["tiles_per_chunk"] == 2
    else:
        assert last["chunks"] == 1, last
    _same(got, [want], form)


def _case_iii(nv, rs):
    fi, ns, tiles = 252250, 40, 106
    L, M, T, S, taps = rs.design(fi)
    n = _samples_for(tiles * 4096 - 1234, L, M)
    rows = _inputs(nv, fi, rr.CS16, n, seed=3) + [_full_scale(rr.CS16, n, 100 + s) for s in range(4, ns)]
    with ThreadPoolExecutor(16) as ex:
        want = list(ex.map(lambda row: rr.resample_all(row, rr.CS16, taps, L, M), rows))
    return rows, want


@FORMS
def test_several_tiles_per_chunk_global_taps(nv, rs, form):
    """(iii) 252.25 kS/s (L = 1008, the tap table in global memory), int16, 40 streams of 106 tiles: 3 tiles per workgroup,
    the last of 1; the last tile short."""
    rows, want = _memo_get("iii", lambda: _case_iii(nv, rs))
    with rs.Resampler(252250, rr.CS16, n_streams=len(rows)) as r:
        r.set_form(form)
        got = _run_resident(nv, r, rows, [len(rows[0])])
        last = r.debug_last_launch()
    assert not last["taps_in_lds"] and last["tiles"] == 106, last
    if form == 2:
        assert last["tiles_per_chunk"] >= 3 and last["tiles"] % last["tiles_per_chunk"] != 0, last
    _same(got, want, form)


@FORMS
def test_several_tiles_per_chunk_k2(nv, rs, form):
    """(iv) 3.2 MS/s (K = 2), signed 8-bit, one stream of 2049 tiles: 2 tiles per workgroup, the last of 1."""
    row, want = _memo_get("iv", lambda: _case_long(rs, 3200000, rr.CS8, 2049, 2, 12))
    with rs.Resampler(3200000, rr.CS8) as r:
        r.set_form(form)
        got = _run_resident(nv, r, [row], [len(row)])
        last = r.debug_last_launch()
    assert last["K"] == 2 and last["tiles"] == 2049, last
    if form == 2:
        assert last["tiles_per_chunk"] >= 2 and last["tiles"] % last["tiles_per_chunk"] != 0, last
    _same(got, [want], form)


# ------------------------------------------------------------------------------------------------- b. every plan shape
ALL_FORMATS = (3200000, 1000250, 100100)
ONE_FORMAT = (2000000, 1920000, 1024000, 384000, 256000, 192000, 252000, 504000, 2016000, 1000400, 252250, 96250)
PLAN_CASES = [(fi, fmt) for fi in ALL_FORMATS for fmt in FORMATS] + [(fi, FORMATS[k % 4]) for k, fi in enumerate(ONE_FORMAT)]
GLOBAL_TAPS = (1000250, 1000400, 252250)


@FORMS
@pytest.mark.parametrize("fi,fmt", PLAN_CASES, ids=[f"{fi}-{FORMAT_IDS[fmt]}" for fi, fmt in PLAN_CASES])
def test_every_plan_shape(nv, rs, fi, fmt, form):
    """The scheme of test_output_equals_the_restatement at the rates it leaves out: the edge of the range (3.2 MS/s, K = 2,
    T = 92), L = 1 (the phase never advances), the largest L (1008), T = 30 with the taps read from global memory, and
    100.1 kS/s, the largest LDS launch (92416 bytes) with a tap at the int16 rail."""
    L, M, T, S, taps = rs.design(fi)
    n = 40013
    rows, want = _memo_get(("b", fi, fmt), lambda: (lambda rows: (rows, _want(rows, fmt, taps, L, M)))(_inputs(nv, fi, fmt, n, seed=fi % 1000 + fmt)))
    with rs.Resampler(fi, fmt, n_streams=len(rows)) as r:
        assert (r.L, r.M, r.T) == (L, M, T)
        r.set_form(form)
        got = _run_resident(nv, r, rows, [n], pitch_extra=3, out_first=7)
        last = r.debug_last_launch()
    assert last["launches"] == 1 and last["taps_in_lds"] == (fi not in GLOBAL_TAPS), last
    if fi == 3200000:
        assert last["K"] == 2 and T == 92, last
    if fi == 100100:
        assert last["lds_bytes"] == 34816 + 57600 and int(taps.max()) == 32767, last
    if fi in (1000250, 1000400):
        assert T == 30
    if fi in (252000, 504000, 2016000):
        assert L == 1
    if fi in (1000250, 252250):
        assert L == 1008
    _same(got, want, form)
    fill = rr.outputs_after(T - 1, L, M)
    assert np.all(want[3][fill:] == (128 if fmt == rr.CU8 else 0)) and want[1].any()


# ----------------------------------------------------------------------------------------- c. the accumulator's extremes
def extreme_input(fmt, taps, L, M, n, seed):
    """[n, 2] samples in fmt and the outputs that stand at the extremes: the phase with the largest sum of |taps|, and at
    outputs of that phase at least 2 T samples apart a window whose samples are the positive rail where the tap is positive
    and the negative rail elsewhere (every second window and Q the other way round); full-scale random in between.
    Returns (samples, the outputs' indices, their values before the clamp [k, 2])."""
    T = taps.shape[1]
    h = taps.astype(np.int64)
    ph = int(np.argmax(np.abs(h).sum(axis=1)))
    x = _full_scale(fmt, n, seed)
    info = np.iinfo(rr.DTYPES[fmt])
    n_out = rr.outputs_after(n, L, M)
    idx = np.arange(n_out, dtype=np.int64)
    q = idx * M // L
    cand = idx[(idx * M % L == ph) & (q >= T - 1)]
    chosen, last_q = [], -10 ** 9
    for k in cand:
        if q[k] - last_q >= 2 * T:
            chosen.append(int(k)); last_q = int(q[k])
    for j, k in enumerate(chosen):
        up = h[ph] > 0                                                         # tap t multiplies sample q - t
        if j % 2:
            up = ~up
        win = q[k] - np.arange(T)
        x[win, 0] = np.where(up, info.max, info.min)
        x[win, 1] = np.where(up, info.min, info.max)
    conv = rr.convert(x, fmt)
    chosen = np.array(chosen, dtype=np.int64)
    acc = np.zeros((len(chosen), 2), dtype=np.int64)
    for t in range(T):
        acc += h[ph, t] * conv[q[chosen] - t]
    assert np.abs(acc).max() + (1 << (rr.S - 1)) < 2 ** 31
    return x, chosen, (acc + (1 << (rr.S - 1))) >> rr.S


@pytest.mark.parametrize("fi,fmt", [(100100, rr.CS16), (3200000, rr.CS16), (252250, rr.CS16), (96000, rr.CS8)],
                         ids=["100100-cs16", "3200000-cs16", "252250-cs16", "96000-cs8"])
def test_accumulator_extremes_and_both_clamps(nv, rs, fi, fmt):
    """Input matched in sign to the taps of the heaviest phase: the value before the clamp is far outside int16 on both sides
    (+-56569 at 100.1 kS/s, |acc| 1.85e9 of int32's 2.147e9), the accumulator stays inside int32, and the device clamps as the
    restatement does."""
    L, M, T, S, taps = rs.design(fi)
    n = 40013
    x, at, before = extreme_input(fmt, taps, L, M, n, seed=fi % 997)
    assert len(at) >= 30
    assert np.all((before > 32767) | (before < -32768)), before
    assert (before > 32767).any(axis=0).all() and (before < -32768).any(axis=0).all()
    if fi == 100100:
        assert np.abs(before).min() >= 56000, np.abs(before).min()
    want = rr.resample_all(x, fmt, taps, L, M)                                 # asserts the accumulator inside int32 itself
    assert np.array_equal(want[at], np.clip(before, -32768, 32767))
    for form in (1, 2):
        with rs.Resampler(fi, fmt) as r:
            r.set_form(form)
            got = _run_resident(nv, r, [x], [n], pitch_extra=1, out_first=1)
        _same(got, [want], form)


# ------------------------------------------------------------------------------------------------ d. conversion sweeps
def cf32_sweep_values():
    """Every tie (k + 0.5) / 32768 of the conversion from below the negative clamp to above the positive one, each with its two
    float32 neighbours and k / 32768, and the special values, as float32 (NaNs as bit patterns)."""
    k = np.arange(-32770, 32770, dtype=np.float64)
    tie = ((k + 0.5) / 32768.0).astype(np.float32)
    assert np.array_equal(tie.astype(np.float64) * 32768.0, k + 0.5)           # exact in float32
    sweep = np.stack([np.nextafter(tie, np.float32(-np.inf)), tie, np.nextafter(tie, np.float32(np.inf)),
                      (k / 32768.0).astype(np.float32)], axis=1).reshape(-1)
    tiny = np.array([0x00000001, 0x80000001, 0x007fffff, 0x807fffff], dtype=np.uint32).view(np.float32)      # subnormals
    nans = np.array([0x7fc00000, 0xffc00000, 0x7fc00001, 0xffc12345, 0x7fffffff, 0xffffffff,                  # quiet
                     0x7f800001, 0xff800001, 0x7fa55555, 0xffbfffff, 0x7f812345], dtype=np.uint32).view(np.float32)   # signalling
    other = np.array([0.0, -0.0, 65536.0, -65536.0, 3.4e38, -3.4e38, np.inf, -np.inf], dtype=np.float32)
    return np.concatenate([sweep, other[:2], tiny, other[2:], nans])


def held(values, hold=16):
    """[len(values) * hold, 2]: every value held for `hold` samples, on I in order and on Q in reverse order."""
    x = np.empty((len(values) * hold, 2), dtype=values.dtype)
    x[:, 0] = np.repeat(values, hold)
    x[:, 1] = np.repeat(values[::-1], hold)
    return x


@pytest.mark.parametrize("fmt", [rr.CF32, rr.CU8, rr.CS8], ids=["cf32", "cu8", "cs8"])
def test_conversion_sweep_at_unit_ratio(nv, rs, fmt):
    """252 kS/s in, 252 kS/s out: L = M = 1, T = 10, and the one phase sums to 2^15, so a value held for 16 samples comes out as
    its own conversion, whatever the taps are."""
    fi, hold = 252000, 16
    L, M, T, S, taps = rs.design(fi)
    assert (L, M, T) == (1, 1, 10) and int(taps.astype(np.int64).sum()) == 1 << S
    if fmt == rr.CF32:
        values = cf32_sweep_values()
        assert len(values) == 4 * 65540 + 23 and np.isnan(values).sum() == 11
    else:
        values = np.arange(256).astype(rr.DTYPES[fmt]) if fmt == rr.CU8 else np.arange(-128, 128).astype(np.int8)
    x = held(values, hold)
    assert x[:, 0].tobytes() == np.repeat(values, hold).tobytes()              # bit patterns (NaN payloads) survived
    conv = rr.convert(np.stack([values, values[::-1]], axis=1), fmt)           # [values, 2]
    want = _want_long(x, fmt, taps, L, M)
    with rs.Resampler(fi, fmt) as r:
        got = _run_resident(nv, r, [x], [len(x)])[0]
        last = r.debug_last_launch()
    assert last["taps_in_lds"] and last["K"] == 16
    interior = got.reshape(len(values), hold, 2)[:, T - 1:, :]                 # outputs 16 j + 9 .. 16 j + 15 see the held value alone
    bad = np.nonzero(np.any(interior != conv[:, None, :], axis=(1, 2)))[0]
    assert len(bad) == 0, (bad[:10], values[bad[:10]], interior[bad[:3]], conv[bad[:3]])
    _same([got], [want])


# ------------------------------------------------------------------------------------------------------- e. past 2^32
def test_positions_past_2_to_32(nv, rs):
    """3.2 MS/s, unsigned 8-bit: 2^30, 2^30, 2^30 and 2^30 - 4099 samples from one 2 GiB device buffer (a 64 MiB random block
    32 times over), then two calls of 20011 fresh samples, the first of which crosses 2^32.  Counts and positions are exact
    after every call; the last 4096 outputs of the fourth call and both small calls equal the restatement run with the true
    64-bit position and the samples that stood in front."""
    fi, fmt = 3200000, rr.CU8
    L, M, T, S, taps = rs.design(fi)
    big, blk = 1 << 30, 1 << 25                                                # samples
    try:
        d_in = nv.DeviceBuffer(big * 2)
    except nv.NvxError as e:
        pytest.skip(f"no 2 GiB device buffer: {e}")
    block = _full_scale(fmt, blk, 21)
    for k in range(big // blk):
        d_in.upload(block, k * blk * 2)
    sample = lambda a, b: block[np.arange(a, b) % blk]                          # noqa: E731  samples [a, b) of the buffer
    calls = [big, big, big, big - 4099]
    cap = rs.out_count(fi, 0, big) + 1
    d_out = nv.DeviceBuffer(cap * 4)
    small_in = nv.DeviceBuffer(20016 * 2)
    with rs.Resampler(fi, fmt) as r:
        consumed = 0
        for c in calls:
            outs = r.resident(d_in, big, c, d_out, cap)
            assert outs == rs.out_count(fi, consumed, c) == rr.outputs_after(consumed + c, L, M) - rr.outputs_after(consumed, L, M)
            consumed += c
            assert r.position(0) == (consumed, rr.outputs_after(consumed, L, M))
        assert consumed == 2 ** 32 - 4099
        last = r.debug_last_launch()
        assert last["K"] == 2 and last["tiles_per_chunk"] > 1 and last["chunks"] > 1024, last
        tail = d_out.download(4096 * 4, offset=(outs - 4096) * 4, dtype=np.int16).reshape(-1, 2)
        m = 60000                                                              # the last m samples of the fourth call hold its last 4096 outputs
        c4 = calls[3]
        want, hist = rr.resample(rr.convert(sample(c4 - m, c4), fmt), taps, L, M, consumed - m, rr.convert(sample(c4 - m - (T - 1), c4 - m), fmt))
        assert len(want) > 4096 and np.array_equal(tail, want[-4096:]), int(np.argmax(np.any(tail != want[-4096:], axis=1)))
        for k in range(2):
            fresh = _full_scale(fmt, 20011, 30 + k)
            small_in.upload(np.concatenate([fresh, np.full((5, 2), 255, dtype=np.uint8)]))
            outs = r.resident(small_in, 20016, 20011, d_out, cap)
            assert outs == rs.out_count(fi, consumed, 20011)
            want, hist = rr.resample(rr.convert(fresh, fmt), taps, L, M, consumed, hist)
            consumed += 20011
            assert r.position(0) == (consumed, rr.outputs_after(consumed, L, M))
            got = d_out.download(outs * 4, dtype=np.int16).reshape(-1, 2)
            assert len(want) == outs and np.array_equal(got, want), (k, int(np.argmax(np.any(got != want, axis=1))))
        assert consumed > 2 ** 32
    for b in (d_in, d_out, small_in):
        b.free()


# --------------------------------------------------------------------------------------------------- f. 65535 streams
def test_65535_streams(nv, rs):
    """The most streams a plan takes (the grid's y limit): 2.048 MS/s, unsigned 8-bit, calls of 1031 and 1000 samples at pitch
    1032, every stream random under its own seed; every stream equals the restatement and the words outside the spans keep
    their sentinel."""
    fi, fmt, ns, pitch_in, calls = 2048000, rr.CU8, 65535, 1032, (1031, 1000)
    L, M, T, S, taps = rs.design(fi)
    n = sum(calls)

    def rows_of(s0):
        return np.stack([np.random.default_rng(70000 + s).integers(0, 256, size=(n, 2), dtype=np.uint8) for s in range(s0, min(ns, s0 + 4096))])
    with ThreadPoolExecutor(16) as ex:
        x = np.concatenate(list(ex.map(rows_of, range(0, ns, 4096))))
    total = rr.outputs_after(n, L, M)
    out_first, pitch_out, sentinel = 5, total + 5 + 3, 0x5a5a1234
    d_in = nv.DeviceBuffer(ns * pitch_in * 2); d_out = nv.DeviceBuffer(ns * pitch_out * 4)
    d_out.upload(np.full(ns * pitch_out, sentinel, dtype=np.uint32))
    block = np.empty((ns, pitch_in, 2), dtype=np.uint8)
    with rs.Resampler(fi, fmt, n_streams=ns) as r:
        pos = made = 0
        for c in calls:
            block[:, c:] = 255
            block[:, :c] = x[:, pos:pos + c]
            d_in.upload(block)
            got = r.resident(d_in, pitch_in, c, d_out, pitch_out, out_first + made)
            assert got == rs.out_count(fi, pos, c)
            pos, made = pos + c, made + got
        last = r.debug_last_launch()
        assert made == total and r.position(0) == r.position(ns - 1) == (n, total)
        assert last["launches"] == 2 and last["chunks"] == 1 and last["tiles"] == 1, last
    words = d_out.download(ns * pitch_out * 4, dtype=np.uint32).reshape(ns, pitch_out)
    d_in.free(); d_out.free()
    assert np.all(words[:, :out_first] == sentinel) and np.all(words[:, out_first + total:] == sentinel), "words outside the span were written"
    got = np.ascontiguousarray(words[:, out_first:out_first + total]).view(np.int16).reshape(ns, total, 2)

    def check(s0):
        part = x[s0:s0 + 4096]
        want = rr.resample_streams(rr.convert(part.reshape(-1, 2), fmt).reshape(part.shape), taps, L, M)
        return [s0 + int(s) for s in np.nonzero(np.any(got[s0:s0 + 4096] != want, axis=(1, 2)))[0]]
    with ThreadPoolExecutor(4) as ex:
        wrong = sum(ex.map(check, range(0, ns, 4096)), [])
    assert not wrong, (len(wrong), wrong[:10])
    for s in (0, 1, 4095, 4096, ns - 1):                                       # the many-stream restatement is the per-stream one
        assert np.array_equal(got[s], rr.resample_all(x[s], fmt, taps, L, M)), s
