"""The blanker's unreached paths on the GPU (-m gpu), words == the restatement (tests/blank_ref.py) throughout and every
launch shape asserted on what the host handed the kernel (nvx_blank_debug_last_launch) before a word is compared:
a. the chunked form in all four formats, at the block phases off = 1, 1024, 1023 and 7, at hold 1024, 32 and 0, with aligned
   and unaligned stores, on inputs that fail when a later chunk's pre-roll carries a ring slot, the open block's partial sum
   or a detection wrongly (tests/test_blank.py shows each input tripped by such a variant), and the call behind it, which
   reads the state row the last chunk wrote;  b. where the host changes form: 32 tiles against 33, 1023 streams against 1024;
c. single spikes on every seam of the kernel's walk at fourteen holds, and a hold that runs through four short calls;
d. the level's arithmetic on blocks of constant magnitude, with probes at the level and one above it;  e. 65 535 streams;
f. calls with no host synchronisation in between, and resets at either state-row parity;  g. a push that takes form 2.
Every resident call is uploaded as whole rows with full scale behind n_in, between sentinels, as in test_gpu_blank.py."""
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pytest

import blank_ref as br
import resample_ref as rr
from test_gpu_blank import SENTINEL, _At, _first_difference, _noise_with_bursts

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FORMAT_IDS = {br.CS16: "cs16", br.CU8: "cu8", br.CS8: "cs8", br.CF32: "cf32"}
TILE = br.TILE
FORM1 = {"chunks": 1, "preroll_blocks": 0, "form": 1}


@pytest.fixture(scope="module")
def bl(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_blank.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.blank
    return navtex_amd.blank


def _form2(chunks, blocks_per_chunk=128):
    return {"chunks": chunks, "blocks_per_chunk": blocks_per_chunk, "preroll_blocks": 8, "form": 2}


def _run(nv, b, rows, cuts, shapes, pitch_extra=0, out_first=0):
    """test_gpu_blank._run_resident, and the shape of every call's launch against `shapes` (a dict of the fields to hold, or
    None for a call that launches nothing): the rows ([n, 2] each, of one length) through nvx_blank_resident in calls of
    `cuts` samples, each uploaded to the start of the input rows as whole rows with full scale from n_in up to the pitch;
    sentinels around every output row; position() asserted.  Returns int16 [streams, n, 2]."""
    ns, n = len(rows), len(rows[0])
    assert sum(cuts) == n and ns == b.n_streams and len(shapes) == len(cuts)
    dt = rows[0].dtype
    bps = dt.itemsize * 2
    pitch_out = out_first + n + pitch_extra
    pitch_in = (max(max(cuts), 1) + 7) // 8 * 8 + 8 * pitch_extra
    d_in = nv.DeviceBuffer(ns * pitch_in * bps)
    d_out = nv.DeviceBuffer(ns * pitch_out * 4)
    d_out.upload(np.full(ns * pitch_out, SENTINEL, dtype=np.uint32))
    block = np.empty((ns, pitch_in, 2), dtype=dt)
    start = b.position(0)
    launches = b.debug_last_launch()["launches"]
    pos = 0
    for c, want in zip(cuts, shapes):
        block[:, c:] = 1.0 if dt == np.float32 else np.iinfo(dt).max
        for s in range(ns):
            block[s, :c] = rows[s][pos:pos + c]
        d_in.upload(block)
        b.resident(d_in, pitch_in, c, d_out, pitch_out, out_first + pos)
        pos += c
        shape = b.debug_last_launch()
        launches += want is not None
        assert shape["launches"] == launches and all(shape[k] == v for k, v in (want or {}).items()), (c, shape, want)
        assert b.position(ns - 1) == start + pos
    words = d_out.download(ns * pitch_out * 4, dtype=np.uint32).reshape(ns, pitch_out)
    d_in.free(); d_out.free()
    assert np.all(words[:, :out_first] == SENTINEL) and np.all(words[:, out_first + n:] == SENTINEL), "words outside the span were written"
    return np.ascontiguousarray(words[:, out_first:out_first + n]).view(np.int16).reshape(ns, n, 2)


def _same(got, want, what):
    assert np.array_equal(got, want), (what, "first difference at sample", _first_difference(got, want))


# -------------------------------------------------------------------- a. form 2: formats, phases, holds, the call behind
CELLS = br.form2_cells()


@pytest.mark.parametrize("cell", range(len(CELLS)), ids=[f"{FORMAT_IDS[c[0]]}-first{c[1]}-hold{c[2]}-out{c[3]}" for c in CELLS])
def test_form_2_across_formats_phases_and_holds_and_the_call_behind_it(nv, bl, cell):
    """Two streams of blank_ref.form2_trap_row, three calls: `first` samples set the phase, 64 * 4096 + 5 run as three
    chunks of 128 blocks behind pre-rolls of 8 (the last chunk a ragged tile of 5 samples), 3000 run as one and start from
    the state row the last chunk wrote out of its pre-roll.  Equal to the restatement, counters included, and to the same
    input through calls of at most 32 tiles, which take form 1."""
    fmt, first, hold, out_first = CELLS[cell]
    rows, infos, _ = br.form2_trap_rows(fmt, first, hold, cell)
    n = len(rows[0])
    assert n == first + br.FORM2_N2 + br.FORM2_N3
    refs = [br.blank(row, fmt, hold=hold) for row in rows]
    # the form-2 call's first word is 16-byte aligned and so is every row, except in the cells that name an odd out_first
    pitch_extra = 1
    if not out_first:
        out_first = -first % 4
        pitch_extra = -(out_first + n) % 4
    assert ((out_first + first) % 4 == 0 and (out_first + n + pitch_extra) % 4 == 0) == (CELLS[cell][3] == 0)
    with bl.Blanker(fmt, n_streams=2, hold=hold) as b:
        got = _run(nv, b, rows, [first, br.FORM2_N2, br.FORM2_N3], [FORM1, _form2(3), FORM1], pitch_extra=pitch_extra, out_first=out_first)
        stats = [b.stats(s) for s in range(2)]
    with bl.Blanker(fmt, n_streams=2, hold=hold) as b:
        one = _run(nv, b, rows, [first, 32 * TILE, 32 * TILE, 5, br.FORM2_N3], [FORM1] * 5)
    for s in range(2):
        want, ref = refs[s]
        for k, C in enumerate(infos[s]["starts"]):           # around each later chunk's start first: it names the chunk
            _same(got[s][C - 2 * TILE:C + 5 * br.NB], want[C - 2 * TILE:C + 5 * br.NB], ("stream", s, "around the start of chunk", k + 1))
        _same(got[s], want, ("stream", s))
        assert stats[s] == (n, ref.detections, ref.blanked), s
    _same(one.reshape(-1, 2), got.reshape(-1, 2), "calls of one chunk against form 2")


# ------------------------------------------------------------------------------------------------ b. the form decision
@pytest.mark.parametrize("n_in, shape", [(32 * TILE, FORM1), (32 * TILE + 1, _form2(2))], ids=["32-tiles", "32-tiles-and-1"])
def test_32_tiles_take_one_chunk_and_one_sample_more_takes_two(nv, bl, n_in, shape):
    """Two CS16 streams: 131 072 samples are 32 tiles, form 1; 131 073 are 33, two chunks, the second one sample long.  A
    call of 2000 samples follows each and reads the state either left."""
    n = n_in + 2000
    at = [(n_in - 2000, 300), (n_in - 30, 25), (n_in - 5000, 1024)]
    rows = [_noise_with_bursts(n, 500 + s, at=at) for s in range(2)]
    with bl.Blanker(br.CS16, n_streams=2) as b:
        got = _run(nv, b, rows, [n_in, 2000], [shape, FORM1])
        for s in range(2):
            want, ref = br.blank(rows[s])
            _same(got[s], want, s)
            assert ref.gone[n_in - 5:n_in + 20].all() and b.stats(s) == (n, ref.detections, ref.blanked)


def test_1023_streams_are_spread_and_1024_are_not(nv, bl):
    """1024 CS8 streams x 135 169 samples (33 tiles), a seed each, 0.83 GB of buffers: a 1024-stream plan takes them in form
    1, a 1023-stream plan rows 0 .. 1022 at the same pitch in form 2 with two chunks; the same words."""
    ns, n = 1024, 33 * TILE + 1
    pitch = (n + 7) // 8 * 8
    block = np.full((ns, pitch, 2), 127, dtype=np.int8)
    for s in range(ns):
        rng = np.random.default_rng(9000 + s)
        block[s, :n] = rng.integers(-6, 7, size=(n, 2), dtype=np.int8)
        for at in rng.integers(0, n - 300, 12).tolist() + [32 * TILE - 20 - s % 7, 32 * TILE - 3000]:
            block[s, at:at + int(rng.integers(1, 300))] = rng.integers(-120, 121, size=2)
    d_in = nv.DeviceBuffer(ns * pitch * 2); d_out = nv.DeviceBuffer((ns * n + 64) * 4)
    d_in.upload(block)
    got, stats = [], []
    for streams, shape in ((1024, FORM1), (1023, _form2(2))):
        d_out.upload(np.full(ns * n + 64, SENTINEL, dtype=np.uint32))
        with bl.Blanker(br.CS8, n_streams=streams) as b:
            b.resident(d_in, pitch, n, d_out, n)
            last = b.debug_last_launch()
            assert last["launches"] == 1 and all(last[k] == v for k, v in shape.items()), last
            assert b.position(streams - 1) == n
            stats.append([b.stats(s) for s in (0, 511, 1022)])
        words = d_out.download((ns * n + 64) * 4, dtype=np.uint32)
        assert np.all(words[streams * n:] == SENTINEL), "words behind the last row were written"
        got.append(words[:1023 * n].reshape(1023, n))
    d_in.free(); d_out.free()
    assert np.array_equal(got[0], got[1]), np.flatnonzero((got[0] != got[1]).any(axis=1))[:10]
    picked = np.linspace(0, 1022, 16).astype(int)
    assert picked[0] == 0 and picked[-1] == 1022
    want, det, gone = br.blank_streams(block[picked, :n], br.CS8)
    assert np.array_equal(got[1][picked], br.pack(want.reshape(-1, 2)).reshape(16, n)) and det.min() > 0
    assert stats[0] == stats[1] and stats[0][0] == (n, det[0], gone[0]) and stats[0][2] == (n, det[-1], gone[-1])


# ----------------------------------------------------------------- c. isolated spikes at every structural boundary
@pytest.mark.parametrize("hold", br.SPIKE_HOLDS)
@pytest.mark.parametrize("fmt", [br.CS16, br.CU8], ids=["cs16", "cu8"])
def test_single_spikes_on_every_seam_of_the_walk(nv, bl, fmt, hold):
    """blank_ref.spike_row behind its warm-up call: one chunk, single-sample spikes a tile and more apart on both sides of
    every lane, DPP row, broadcast, step, region, tile and block seam; each blanks hold + 1 samples and no neighbour hides
    a hold that is one short or long or a scan that loses the detection (tests/test_blank.py holds the input to that)."""
    x, at = br.spike_row(fmt, seed=3)
    rows = [x, x.copy()]
    rows[1][at[::2]] = rows[1][at[::2] + 2000]                # the second stream keeps every other spike
    with bl.Blanker(fmt, n_streams=2, hold=hold) as b:
        got = _run(nv, b, rows, [br.SPIKE_FIRST, len(x) - br.SPIKE_FIRST], [FORM1, FORM1])
        for s in range(2):
            want, ref = br.blank(rows[s], fmt, hold=hold)
            assert ref.detections == len(at) // (s + 1) and ref.blanked == ref.detections * (hold + 1)
            _same(got[s], want, (s, hold))
            assert b.stats(s) == (len(x), ref.detections, ref.blanked)


def test_a_hold_of_1024_runs_through_four_short_calls(nv, bl):
    """A spike on the last sample of a call, then calls of 1, 1000, 23 and 1 samples: the first three are blanked through
    (1024 samples), the fourth's only sample is the first to pass."""
    cuts = [6000, 1, 1000, 23, 1, 500]
    rows = []
    for s in range(2):
        x = np.random.default_rng(70 + s).integers(-200, 201, size=(sum(cuts), 2)).astype(np.int16)
        x[5999] = (-30000, 30000)
        rows.append(x)
    with bl.Blanker(br.CS16, n_streams=2, hold=1024) as b:
        got = _run(nv, b, rows, cuts, [FORM1] * 6)
        for s in range(2):
            want, ref = br.blank(rows[s], hold=1024)
            assert ref.detections == 1 and ref.gone[5999:7024].all() and not ref.gone[7024] and ref.blanked == 1025
            _same(got[s], want, s)
            assert b.stats(s) == (sum(cuts), 1, 1025)


# ------------------------------------------------------------------------------------------ d. the level's arithmetic
def _level_case(nv, bl, rows, position, **params):
    with bl.Blanker(br.CS16, n_streams=len(rows), hold=0, **params) as b:
        b.debug_set_position(position)
        got = _run(nv, b, rows, [len(rows[0])], [FORM1], out_first=position % 3)
        for s, row in enumerate(rows):
            want, ref = br.blank(row, hold=0, position=position, **params)
            _same(got[s], want, (s, position, params))
            assert b.stats(s) == (len(row), ref.detections, ref.blanked) and ref.detections == ref.blanked
    return ref


@pytest.mark.parametrize("position", br.LEVEL_POSITIONS)
@pytest.mark.parametrize("floor", br.LEVEL_FLOORS)
@pytest.mark.parametrize("thr_q8", br.LEVEL_THR)
def test_the_strict_compare_the_shift_the_floor_and_the_ring_slots(nv, bl, thr_q8, floor, position):
    """blank_ref.level_row: CS16 blocks of constant magnitude that straddle regions and tiles, in each a sample at the level
    (no detection) and one a unit above (a detection): the minimum in every ring slot, a block sum of 1024 c + 1023 against
    1024 (c + 1), six loud blocks behind quiet ones.  Stream 1 carries the same blocks with every sign turned."""
    x, at_level, above = br.level_row(position, thr_q8, floor, br.LEVEL_BLOCKS)
    y = np.where(x == -32768, x, -x).astype(np.int16)
    ref = _level_case(nv, bl, [x, y], position, thr_q8=thr_q8, floor=floor)
    assert len(above) >= 20 and ref.d[above].all() and not ref.d[at_level].any()


@pytest.mark.parametrize("position", br.LEVEL_POSITIONS)
def test_the_product_2_to_28_and_silence_with_no_floor(nv, bl, position):
    """Five blocks of (-32768, -32768) from the reset on at thr_q8 = 4096: thr_q8 * (ref >> 10) = 2^28, a level of 2^20,
    nothing detected in them or in the quiet block behind.  Silence with floor = 0: a level of 0, every non-zero sample
    detected and no zero one."""
    x, _, _ = br.level_row(position, 4096, 64, br.RAIL_BLOCKS)
    ref = _level_case(nv, bl, [x, x.copy()], position, thr_q8=4096)
    assert not ref.d[:6 * 1024 - position % 1024].any()
    x = br.silent_row(position)
    ref = _level_case(nv, bl, [x, br.silent_row(position, seed=6)], position, floor=0)
    assert ref.detections > 200


# ---------------------------------------------------------------------------------------------------- e. 65 535 streams
def test_65535_streams_an_amplitude_and_a_spike_each(nv, bl):
    """CS8, 65 535 rows of 5376 samples (five blocks and a quarter; 2.1 GB of buffers): row r has noise of its own amplitude
    (1 + r % 11) and a spike whose place and size follow from r, so a row taken for another differs.  grid.y beyond 1024,
    the stream offsets beyond 2^31 bytes; every row == blank_streams, sentinels behind the last."""
    ns, n = 65535, 5376
    r = np.arange(ns)
    rows = np.empty((ns, n, 2), dtype=np.int8)
    slab = 4096

    def make(r0):
        rng = np.random.default_rng(r0)
        k = min(slab, ns - r0)
        rows[r0:r0 + k] = rng.integers(-4, 5, size=(k, n, 2), dtype=np.int8) * (1 + r[r0:r0 + k] % 11).astype(np.int8)[:, None, None]
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(make, range(0, ns, slab)))
    place = 4096 + (r * 37) % 1200
    rows[r, place, 0] = 127 - r % 5
    rows[r, place, 1] = -128 + r % 3
    d_in = nv.DeviceBuffer(ns * n * 2); d_out = nv.DeviceBuffer((ns * n + 64) * 4)
    d_in.upload(rows)
    d_out.upload(np.full(64, SENTINEL, dtype=np.uint32), ns * n * 4)
    with bl.Blanker(br.CS8, n_streams=ns) as b:
        b.resident(d_in, n, n, d_out, n)
        last = b.debug_last_launch()
        assert last == {"launches": 1, "chunks": 1, "blocks_per_chunk": 8, "preroll_blocks": 0, "form": 1}, last
        assert b.position(0) == b.position(ns - 1) == n
        stats = [b.stats(s) for s in (0, 32767, 65534)]
    words = d_out.download((ns * n + 64) * 4, dtype=np.uint32)
    d_in.free(); d_out.free()
    assert np.all(words[ns * n:] == SENTINEL), "words behind the last row were written"
    got = words[:ns * n].view(np.int16).reshape(ns, n, 2)

    def check(r0):
        want, det, gone = br.blank_streams(rows[r0:r0 + slab], br.CS8)
        bad = np.flatnonzero((got[r0:r0 + slab] != want).any(axis=(1, 2)))
        return (r0 + bad).tolist(), det, gone
    with ThreadPoolExecutor(16) as ex:
        res = list(ex.map(check, range(0, ns, slab)))
    assert not sum((b_ for b_, _, _ in res), []), sum((b_ for b_, _, _ in res), [])[:10]
    det, gone = np.concatenate([d for _, d, _ in res]), np.concatenate([g for _, _, g in res])
    assert (det >= 1).all() and stats == [(n, det[s], gone[s]) for s in (0, 32767, 65534)]


# ------------------------------------------------------------------------------------------- f. ordering and resets
@pytest.mark.parametrize("timed", [False, True], ids=["untimed", "timed"])
def test_five_calls_alternating_forms_with_no_host_synchronisation(nv, bl, timed):
    """Two CS16 streams uploaded once, then five resident calls on one non-null HIP stream, form 2, 1, 2, 1, 2, each
    reading at its offset, and nothing waited for before the end.  Every launch reads the state row its predecessor wrote
    and writes the other: this is the only sequence in the suite whose result depends on the two state rows alternating
    between launches that are merely ordered on a stream.  It cannot prove that protocol -- launches that happen not to
    overlap pass without it."""
    cuts = [33 * TILE + 4, 3000, 33 * TILE + 8, 5000, 34 * TILE - 4]
    shapes = [_form2(2), FORM1, _form2(2), FORM1, _form2(2)]
    n = sum(cuts)
    rows = [_noise_with_bursts(n, 600 + s, at=[(sum(cuts[:k]) - 20 - s, 30) for k in range(1, 5)]) for s in range(2)]
    pitch_in, pitch_out = n + 8, n + 3
    d_in = nv.DeviceBuffer(2 * pitch_in * 4); d_out = nv.DeviceBuffer(2 * pitch_out * 4)
    block = np.full((2, pitch_in, 2), 32767, dtype=np.int16)
    block[:, :n] = rows
    d_in.upload(block)
    d_out.upload(np.full(2 * pitch_out, SENTINEL, dtype=np.uint32))
    with bl.Blanker(br.CS16, n_streams=2) as b, nv.Pipeline(n_streams=1, chain_mask=nv.CHAIN_518, max_frames=1) as p:
        hs = p.hip_stream
        assert hs
        b.timing(timed)
        pos = 0
        for k, (c, shape) in enumerate(zip(cuts, shapes)):
            assert pos % 4 == 0
            b.resident(_At(d_in.ptr + pos * 4), pitch_in, c, d_out, pitch_out, 1 + pos, hip_stream=hs)
            last = b.debug_last_launch()
            assert last["launches"] == k + 1 and all(last[f] == v for f, v in shape.items()), (k, last)
            pos += c
        assert b.position(1) == n
        nv.lib.nvx_device_sync(0)
        assert b.time_stats()[1] == (5 if timed else 0) and b.debug_last_launch()["launches"] == 5
        words = d_out.download(2 * pitch_out * 4, dtype=np.uint32).reshape(2, pitch_out)
        stats = [b.stats(s) for s in range(2)]
    d_in.free(); d_out.free()
    assert np.all(words[:, :1] == SENTINEL) and np.all(words[:, 1 + n:] == SENTINEL), "words outside the span were written"
    got = np.ascontiguousarray(words[:, 1:1 + n]).view(np.int16).reshape(2, n, 2)
    for s in range(2):
        want, ref = br.blank(rows[s])
        _same(got[s], want, s)
        assert stats[s] == (n, ref.detections, ref.blanked)


@pytest.mark.parametrize("how", ["reset-one", "reset-all", "set-position"])
@pytest.mark.parametrize("launches", [1, 2], ids=["after-one-launch", "after-two"])
def test_a_reset_at_either_state_row_parity(nv, bl, how, launches):
    """Three CS16 streams, one or two joint calls (the state row the next launch reads is row 1 or row 0), then stream 1
    restarted -- nvx_blank_reset(1), nvx_blank_reset(-1) for all three, or the position hook at a position that is 1023 mod
    1024 -- pushed alone up to where the others stand, and a joint call.  Every stream equals a restatement restarted at the
    same points; the counters run on across the restart."""
    cuts = [3000, 2000][:launches]
    P, tail = sum(cuts), 9000
    rows = [_noise_with_bursts(P + tail, 700 + 10 * launches + s, rate=900) for s in range(3)]
    refs = [br.Blanker() for _ in range(3)]
    with bl.Blanker(br.CS16, n_streams=3) as b:
        got = _run(nv, b, [row[:P] for row in rows], cuts, [FORM1] * launches)
        for s in range(3):
            _same(got[s], refs[s].push(rows[s][:P]), s)
        if how == "reset-all":
            b.reset(-1)
            for ref in refs:
                ref.reset()
            assert [b.position(s) for s in range(3)] == [0, 0, 0]
        else:
            start = 0 if how == "reset-one" else P - P % 1024 - 1
            assert start < P and (how == "reset-one" or start % 1024 == 1023)
            if how == "reset-one":
                b.reset(1)
            else:
                b.debug_set_position(start, stream=1)
            refs[1].reset(start)
            assert [b.position(s) for s in range(3)] == [P, start, P]
            alone = _noise_with_bursts(P - start + 4096, 760 + launches, rate=700)[-(P - start):]
            pos = 0
            for c in (1, (P - start) // 2, P - start - 1 - (P - start) // 2):
                if c:
                    _same(b.push(1, alone[pos:pos + c]), refs[1].push(alone[pos:pos + c]), ("stream 1 alone from", start + pos))
                pos += c
            assert pos == P - start and b.position(1) == P
        got = _run(nv, b, [row[P:] for row in rows], [tail], [FORM1])
        for s in range(3):
            _same(got[s], refs[s].push(rows[s][P:]), ("behind the restart", s))
            assert refs[s].detections > 0 and b.stats(s) == (refs[s].samples, refs[s].detections, refs[s].blanked), s


# --------------------------------------------------------------------------------------- g. a push that takes form 2
@pytest.mark.parametrize("fmt", [br.CS16, br.CF32], ids=["cs16", "cf32"])
def test_a_push_large_enough_for_form_2(nv, bl, fmt):
    """One push of 4 * 32 * 4096 + 777 samples: five chunks, the last of 777 samples; then one of 300 samples, which reuses
    the larger staging buffers and reads the state the fifth chunk wrote."""
    n = 4 * 32 * TILE + 777
    at = [(k * 32 * TILE - 20, 30) for k in range(1, 5)] + [(k * 32 * TILE - 6000 + 900 * j, 50) for k in range(1, 5) for j in range(6)]
    x = rr.to_format(_noise_with_bursts(n + 300, 800 + fmt, at=at + [(n - 10, 40)]), fmt)
    want, ref = br.blank(x, fmt)
    with bl.Blanker(fmt, n_streams=2) as b:
        first = b.push(1, x[:n])
        last = b.debug_last_launch()
        assert last == {"launches": 1, "chunks": 5, "blocks_per_chunk": 128, "preroll_blocks": 8, "form": 2}, last
        second = b.push(1, x[n:])
        last = b.debug_last_launch()
        assert last["launches"] == 2 and last["form"] == 1 and last["chunks"] == 1, last
        _same(first, want[:n], "the push of five chunks")
        _same(second, want[n:], "the push behind it")
        assert ref.gone[n - 10:n + 30].all()
        assert b.position(1) == n + 300 and b.position(0) == 0 and b.stats(1) == (n + 300, ref.detections, ref.blanked) and b.stats(0) == (0, 0, 0)
