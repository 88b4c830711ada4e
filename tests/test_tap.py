"""The channel tap (include/navtex_amd_tap.h) on the CPU: the header and the companion library's exports and argument safety,
L, M, T and every call's count against fractions.Fraction, the refusals of rates, shifts and pitches, the taps handed out held
to the project's two bars for thirteen designs, the table against the bank's, the launch arithmetic against 128-bit integers
(a stand-alone program under ASan + UBSan), the restatement (tests/tap_ref.py) against Python integers, on cuts anywhere, at
the rails and over a retune, the audio kind's fold, and end to end through the restatements and the oracle's character layer:
stations of a 252 kS/s row through taps of both kinds and back through the interpolator, each delivering exactly its text."""
import ctypes as C
import re
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import ddc_ref as dr
import signals
import tap_cases as tc
import tap_ref as tr

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "navtex_amd_tap.h"
PLAN = ROOT / "navtex_amd" / "tap" / "nvx_tap_plan.h"
SYMBOLS = ["nvx_tap_config_default", "nvx_tap_create", "nvx_tap_design", "nvx_tap_destroy", "nvx_tap_get_pitch", "nvx_tap_get_shift", "nvx_tap_grid",
           "nvx_tap_last_error", "nvx_tap_plan", "nvx_tap_position", "nvx_tap_push", "nvx_tap_reset", "nvx_tap_resident", "nvx_tap_set_pitch",
           "nvx_tap_set_shift", "nvx_tap_table", "nvx_tap_time_stats", "nvx_tap_timing"]
HOOKS = ["nvx_tap_debug_last_launch", "nvx_tap_debug_set_position"]


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


# ------------------------------------------------------------------------------------------------------------ interface
def test_header_compiles_as_plain_c_and_declares_the_entry_points(tmp_path):
    text = HEADER.read_text()
    assert sorted(set(re.findall(r"NVX_API\s+[\w\s\*]+?\b(\w+)\s*\(", text))) == SYMBOLS
    assert "252 kS/s row -> tap -> file" in text and "S = 21" in text and "2000 <= fo <= 96000" in text and "< 2^40" in text
    src = tmp_path / "t.c"
    src.write_text((ROOT / "tests" / "harness" / "null_args_tap.c").read_text())
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", f"-I{ROOT / 'include'}", str(src)], check=True)
    src.write_text('#include "navtex_amd_tap.h"\nint main(void){ nvx_tap_config c; c.kind = NVX_TAP_REAL; '
                   'return NVX_TAP_IQ == 0 && c.kind == 1 && NVX_TAP_SHIFT == 21 && NVX_TAP_GRID == 4096 && NVX_TAP_INPUT_RATE == 252000 '
                   '&& sizeof c == 24 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


@pytest.mark.parametrize("sym", SYMBOLS + HOOKS)
def test_symbol_is_exported(tp, sym):
    assert hasattr(tp.lib, sym), f"{sym} is declared but not exported"


def test_the_companion_links_no_other_library_of_the_project_and_no_test_infrastructure(tp):
    lib = ROOT / "navtex_amd" / "libnavtex_amd_tap.so"
    out = subprocess.run(["ldd", str(lib)], capture_output=True, text=True).stdout
    assert "libnavtex_amd" not in out and "oracle" not in out and "libamdhip64" in out
    # it defines nothing but its own interface and the tests' two hooks, and needs no nvx_ symbol from elsewhere
    nm = subprocess.run(["nm", "-D", str(lib)], capture_output=True, text=True, check=True).stdout
    defined = sorted(l.split()[-1] for l in nm.splitlines() if " T " in l and "nvx_" in l)
    assert defined == sorted(SYMBOLS + HOOKS) and all(d.startswith("nvx_tap_") for d in defined)
    assert not [h for h in HOOKS if h in HEADER.read_text()] and all(h in PLAN.read_text() for h in HOOKS)
    assert tp.lib.nvx_tap_debug_last_launch(None, None, None, None, None, None) < 0 and tp.lib.nvx_tap_debug_set_position(None, 0, 0) < 0
    assert not [l for l in nm.splitlines() if " U " in l and "nvx" in l]
    for path in (ROOT / "navtex_amd" / "tap").iterdir():
        text = path.read_text()
        assert "oracle" not in text and "nvxo_" not in text, path
    assert "oracle" not in HEADER.read_text() and "oracle" not in (ROOT / "navtex_amd" / "tap.py").read_text()
    assert C.sizeof(tp.Config) == 24


def test_null_nonsense_and_overflowing_arguments_are_errors_never_crashes(tp, tmp_path):
    src = ROOT / "tests" / "harness" / "null_args_tap.c"
    exe = tmp_path / "null_args_tap"
    lib = ROOT / "navtex_amd"
    subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib}", "-lnavtex_amd_tap",
                    f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "tap null-safety ok" in out.stdout, (out.stdout[-2500:], out.stderr[-500:])
    assert all(re.search(rf"\b{s}\(", src.read_text()) for s in SYMBOLS)


def test_create_returns_nodev_without_a_gpu_and_refuses_bad_parameters_first(nv, tp):
    if nv.device_count() > 0:
        pytest.skip("a GPU is present")
    cfg = tp.Config()
    tp.lib.nvx_tap_config_default(C.byref(cfg))
    h = C.c_void_p(1)
    assert tp.lib.nvx_tap_create(C.byref(cfg), C.byref(h)) == -2
    assert h.value is None and b"no CPU path" in tp.lib.nvx_tap_last_error()
    with pytest.raises(nv.NvxError) as e:
        tp.Tap(8000, kind=tp.REAL, n_inputs=4, n_taps=2)
    assert e.value.code == -2
    for kw in (dict(output_rate_hz=1999), dict(output_rate_hz=96001), dict(output_rate_hz=7999, kind=tp.REAL), dict(output_rate_hz=48001, kind=tp.REAL),
               dict(output_rate_hz=2001), dict(output_rate_hz=12000, kind=2), dict(output_rate_hz=12000, n_inputs=0), dict(output_rate_hz=12000, n_taps=0),
               dict(output_rate_hz=12000, n_inputs=65535, n_taps=2)):
        with pytest.raises(nv.NvxError) as e:
            tp.Tap(**kw)
        assert e.value.code == nv._native.ERR_ARG, kw


# ------------------------------------------------------------------------------------------- plans, counts and refusals
def test_l_m_t_and_the_refusals(nv, tp):
    for (fo, kind), (L, M, T) in tc.PLAN_OF.items():
        f = Fraction(fo, 252000)
        assert (f.numerator, f.denominator) == (L, M) == tr.ratio(fo) and tp.design(fo, kind, taps=False)[:3] == (L, M, T), (fo, kind)
        assert L * T <= 32768 and T % 2 == 0
    for fo, kind, word in ((1999, tr.IQ, b"outside"), (96001, tr.IQ, b"outside"), (7999, tr.REAL, b"outside"), (48001, tr.REAL, b"outside"),
                           (2001, tr.IQ, b"32768 taps"), (0, tr.IQ, b"outside"), (2 ** 32 - 1, tr.IQ, b"outside"), (12000, 2, b"kind"), (12000, -1, b"kind"),
                           (8001, tr.REAL, b"32768 taps")):
        assert tp.lib.nvx_tap_design(fo, kind, None, None, None, None, 0) == nv._native.ERR_ARG, (fo, kind)
        assert word in tp.lib.nvx_tap_last_error(), (fo, kind, tp.lib.nvx_tap_last_error())
    assert Fraction(2001, 252000).numerator == 667
    # every rate the library accepts keeps L T within the table
    for kind in (tr.IQ, tr.REAL):
        lo, hi = tr.RATE_RANGE[kind]
        for fo in range(lo, hi + 1, 250):
            if tp.lib.nvx_tap_design(fo, kind, None, None, None, None, 0) > 0:
                L, M, T, _ = tp.design(fo, kind, taps=False)
                assert L * T <= 32768 and T % 2 == 0 and (L, M) == tr.ratio(fo), fo


def test_shifts_and_pitches_on_their_grids_and_beyond_their_ranges(nv, tp):
    rng = np.random.default_rng(5)
    for fo, kind in ((12000, tr.IQ), (96000, tr.IQ), (2000, tr.IQ), (8000, tr.REAL)):
        fp = tr.edges(fo, kind)[0]
        limit = 126000 - fp
        for hz in [0.0, 14000.0, -14000.0, 30.76171875, 30.76, 30.77, 92.28515625, float(limit), -float(limit), float(limit) + 31.0, -float(limit) - 31.0,
                   float(limit) - 31.0, 126000.0] + [float(v) for v in rng.uniform(-126000, 126000, size=200)]:
            want = tr.grid(fo, kind, hz)
            k, applied = C.c_int(99999), C.c_double(-1.0)
            rc = tp.lib.nvx_tap_grid(fo, kind, hz, C.byref(k), C.byref(applied))
            if want is None:
                assert rc == nv._native.ERR_ARG and k.value == 99999 and b"pass band" in tp.lib.nvx_tap_last_error(), (fo, hz)
            else:
                assert rc == 0 and k.value == want and applied.value == want * 252000 / 4096 and abs(hz - applied.value) <= 30.77, (fo, hz)
        assert tr.grid(fo, kind, float(limit) + 31.0) is None and tr.grid(fo, kind, float(limit) - 31.0) is not None
    assert tr.grid(12000, tr.IQ, 30.76171875) == 0 and tr.grid(12000, tr.IQ, 92.28515625) == 2      # ties to even
    for hz in (float("nan"), float("inf"), -float("inf")):
        assert tp.lib.nvx_tap_grid(12000, tr.IQ, hz, None, None) == nv._native.ERR_ARG
    # the pitch rule has no entry point without a plan: the restatement's range, and the default inside it at every audio rate
    for fo in tc.REAL_RATES:
        kp = tr.pitch_grid(fo, tr.DEFAULT_PITCH_HZ)
        assert kp is not None and abs(kp * fo / 4096 - 1000) <= fo / 8192
        assert tr.pitch_grid(fo, 799 - fo / 8192) is None and tr.pitch_grid(fo, fo / 2 - 799 + fo / 8192) is None
        assert tr.pitch_grid(fo, 801 + fo / 8192) is not None and tr.pitch_grid(fo, fo / 2 - 801 - fo / 8192) is not None


@pytest.mark.parametrize("fo", [12000, 8000, 11025, 6250, 96000, 44100, 2000])
def test_every_calls_count_against_fractions_over_random_chunkings(tp, fo):
    """Positions up to 2^62; calls of zero and of one sample among them."""
    L, M = tr.ratio(fo)
    rng = np.random.default_rng(fo)
    for start in (0, 1, 12345, 2 ** 32 - 1000, 2 ** 40 + 6, 2 ** 62 - 10 ** 6):
        chunks = [0, 1, 1, 0, 2, 29, 30] + [int(c) for c in rng.integers(0, 5000, size=40)] + [1, 0]
        want = tr.exact_counts(fo, start, chunks)
        pos = start
        for c, w in zip(chunks, want):
            assert tp.out_count(L, M, pos, c) == w == tr.outputs_after(pos + c, L, M) - tr.outputs_after(pos, L, M), (start, pos, c)
            pos += c
        total = Fraction(pos) * Fraction(fo, 252000)
        assert tr.outputs_after(pos, L, M) == -(-total.numerator // total.denominator)
    assert tr.exact_counts(fo, 0, [0]) == [0] and tr.exact_counts(fo, 0, [1]) == [1]


# ----------------------------------------------------------------------------------------------------------------- taps
@pytest.fixture(scope="module")
def designs(tp):
    return {d: tp.design(*d) for d in tc.DESIGNS}


@pytest.mark.parametrize("design", tc.DESIGNS, ids=lambda d: f"{'iq' if d[1] == tr.IQ else 'real'}_{d[0]}")
def test_the_taps_handed_out_hold_the_two_bars(designs, design):
    """Every phase sums to exactly 2^21; sum |h >> 8| <= 65535 and sum |h| < 2^24; the pass band within +-0.1 dB from 0 to fp; at
    most -76 dB from the stop edge to L * 126000, on an FFT grid of 16 points per side lobe.  Recorded from the C design: sum |h|
    at most 1.84 * 2^21 (IQ) and 1.63 * 2^21 (REAL), sum |h >> 8| at most 15 542; pass band within 0.0005 dB; stop band between
    -87.8 and -90.8 dB (IQ) and between -81.5 and -83.8 dB (REAL)."""
    fo, kind = design
    L, M, T, h = designs[design]
    fp, fs = (float(v) for v in tr.edges(fo, kind))
    assert (L, M, T) == tc.PLAN_OF[design] and h.shape == (L, T) and h.dtype == np.int32
    h64 = h.astype(np.int64)
    assert np.all(h64.sum(axis=1) == 1 << 21)
    tr.check_split(h)
    f, db = tr.response_fft(h, L)
    assert f[-1] == L * 126000.0
    pass_db, stop_db = db[f <= fp], db[f >= fs]
    assert len(pass_db) >= 16 and len(stop_db) >= 16 * (T // 2)
    print(f"{fo} kind {kind}: L {L} M {M} T {T}, sum|h| <= {np.abs(h64).sum(axis=1).max() / 2 ** 21:.3f} * 2^21, sum|h >> 8| <= {int(np.abs(h64 >> 8).sum(axis=1).max())}, "
          f"pass band within {float(np.abs(pass_db).max()):.4f} dB, stop band at most {float(stop_db.max()):.1f} dB")
    assert np.abs(pass_db).max() <= 0.1
    assert stop_db.max() <= -76.0
    # the recipe restated in numpy gives the same numbers, but for the last bit of a rounding
    L2, M2, T2, h2 = tr.design(fo, kind)
    assert (L2, M2, T2) == (L, M, T) and np.abs(h2.astype(np.int64) - h64).max() <= 1


def test_int16_taps_would_miss_the_bar(designs):
    """The design fact behind S = 21: the 12 kS/s taps rounded to S = 15 leave the stop band above -76 dB."""
    L, M, T, h = designs[(12000, tr.IQ)]
    f, db = tr.response_fft(np.rint(h / 64.0), L)
    assert -70.0 < db[f >= 7200.0].max() < -55.0


def test_the_table_is_the_banks(tp):
    import navtex_amd.ddc as ddc
    w = tp.table()
    assert w.shape == (4096, 2) and w.dtype == np.int16 and np.array_equal(w, ddc.table()) and np.array_equal(w, dr.table())
    assert tp.lib.nvx_tap_table(None, 0) == 4096


def test_the_launch_arithmetic_against_128_bit_integers_under_asan_ubsan(tmp_path):
    """nvx_tap_plan.h's functions without a device (tests/harness/tap_launch_args.cpp): every output's (q, r), once, its window
    inside its tile's staged span and aligned, wave-uniform rows where the plan says so.  A stand-alone program under ASan +
    UBSan."""
    exe = tmp_path / "tap_launch_args"
    pkg = ROOT / "navtex_amd"
    subprocess.run(["g++", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    f"-I{ROOT / 'include'}", f"-I{pkg / 'csrc'}", f"-I{pkg / 'tap'}",
                    str(ROOT / "tests" / "harness" / "tap_launch_args.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env={"ASAN_OPTIONS": "detect_leaks=1", "PATH": "/usr/bin:/bin"})
    assert out.returncode == 0 and "tap launch args ok" in out.stdout, (out.stdout + out.stderr)[-3000:]


# ----------------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("design", [(12000, tr.IQ), (11025, tr.IQ), (96000, tr.IQ), (8000, tr.REAL)], ids=["12000", "11025", "96000", "real_8000"])
def test_the_numpy_restatement_equals_python_integers(designs, design):
    fo, kind = design
    L, M, T, h = designs[design]
    n = 2 * T + 40 * (M // L + 1)
    x = tc.full_scale(n, 1)
    k, kp = tr.grid(fo, kind, -20000.0), tr.pitch_grid(fo, 1234.5)
    (out,), _ = tr.tap_all(x, h, L, M, kind, [k], [kp])
    assert len(out) == tr.outputs_after(n, L, M)
    picks = list(range(0, 6)) + [len(out) // 2, len(out) - 2, len(out) - 1]
    ys = np.array([tr.output_int(x, h, L, M, i, k)[0] for i in picks], dtype=np.int64)
    if kind == tr.IQ:
        assert np.array_equal(out[picks], ys)
        assert np.array_equal(tr.pack(out).view(np.int16).reshape(-1, 2), out)
    else:
        for i, y in zip(picks, ys):
            assert out[i] == tr.pitch_turn(y[None, :], kp, i)[0], i


@pytest.mark.parametrize("kind", [tr.IQ, tr.REAL], ids=["iq", "real"])
def test_one_shot_equals_cuts_anywhere_and_a_reset_leaves_shifts_alone(designs, kind):
    fo = 11025 if kind == tr.IQ else 8000
    L, M, T, h = designs[(fo, kind)]
    n = 3 * T + 5000
    x = tc.signal(n, 5)
    ks, kps = [0, tr.grid(fo, kind, 14000.0)], [tr.pitch_grid(fo, 1000), tr.pitch_grid(fo, 2000)]
    one, ref = tr.tap_all(x, h, L, M, kind, ks, kps)
    assert ref.consumed == n and ref.produced == len(one[0]) == tr.outputs_after(n, L, M)
    c = tr.Tap(h, L, M, kind, ks, kps)
    pos, parts = 0, []
    for cut in [0, 1, T - 2, T - 1, T, 1, 0, 3500, 3, n - 3505 - 3 * T + 3]:
        parts.append(c.push(x[pos:pos + cut])); pos += cut
        assert c.consumed == pos and c.produced == tr.outputs_after(pos, L, M) == sum(len(p[0]) for p in parts)
    assert pos == n
    for t in range(2):
        assert np.array_equal(np.concatenate([p[t] for p in parts]), one[t])
    assert not np.array_equal(one[0], one[1])
    c.reset()
    again = c.push(x)
    assert all(np.array_equal(again[t], one[t]) for t in range(2)) and c.ks == ks


def test_a_constant_comes_out_as_the_constant_through_k_0_and_a_retune_reaches_the_carried_samples(designs):
    L, M, T, h = designs[(48000, tr.IQ)]
    x = np.tile(np.array([[12345, -32768]], dtype=np.int16), (3 * T + 400, 1))
    (out,), _ = tr.tap_all(x, h, L, M, tr.IQ, [0])
    settled = out[tr.outputs_after(T, L, M):]
    assert len(settled) > 100 and np.all(settled == (12345, -32768))
    # a new shift applies from the next call on, the carried samples included: the call after the retune equals a tap that had
    # the new shift all along, from its first output on
    y = tc.signal(3000, 9)
    k1, k2 = tr.grid(48000, tr.IQ, 5000.0), tr.grid(48000, tr.IQ, -7000.0)
    a = tr.Tap(h, L, M, tr.IQ, [k1])
    a.push(y[:1700])
    a.ks[0] = k2
    tail = a.push(y[1700:])[0]
    whole = tr.tap_all(y, h, L, M, tr.IQ, [k2])[0][0]
    assert np.array_equal(tail, whole[tr.outputs_after(1700, L, M):])
    assert not np.array_equal(tail, tr.tap_all(y, h, L, M, tr.IQ, [k1])[0][0][tr.outputs_after(1700, L, M):])


def test_the_rails_clamp_both_ways_and_the_sum_needs_more_than_32_bits(designs):
    """Windows matched in sign to the phase with the largest sum |h|: the value before the clamp is beyond int16 both ways."""
    for design in ((12000, tr.IQ), (8000, tr.IQ), (11025, tr.IQ)):
        L, M, T, h = designs[design]
        big = int(np.abs(h.astype(np.int64)).sum(axis=1).max())
        (out,), ref = tr.tap_all(tc.rails(h, L, M, 6), h, L, M, tr.IQ, [0])
        assert ref.acc_max >> 21 > 55000 and ref.acc_min >> 21 < -55000 and ref.acc_max <= big * 32768 and ref.acc_max > 1 << 36
        assert ref.acc_max >= (big - 2 * T) * 32767                              # the matched window: all of sum |h| but the zero taps' signs
        assert {int(out[:, 0].max()), int(out[:, 0].min()), int(out[:, 1].max()), int(out[:, 1].min())} == {32767, -32768}


# ------------------------------------------------------------------------------------- the GPU edge cases, without a GPU
class _StateMovedByOneWord(tr.Tap):
    """The restatement with one error: the carried row stands one word late."""

    def push(self, x):
        out = super().push(x)
        self.hist = np.concatenate([np.zeros((1, 2), dtype=np.int64), self.hist[:-1]])
        return out


@pytest.mark.parametrize("plan", [(2000, tr.IQ), (2016, tr.IQ), (12000, tr.REAL)], ids=["iq_2000", "iq_2016", "real_12000"])
def test_the_edge_cuts_tell_a_state_row_moved_by_one_word(tp, plan):
    """tests/test_gpu_tap_edges.py's cut plan and inputs through the restatement and through one whose state row is moved by one
    word behind every call: every call with outputs behind the first differs in every row -- the call of T samples, the one
    of 5000, and the last, whose first windows lie in the carried row."""
    fo, kind = plan
    L, M, T, h = tp.design(fo, kind)
    tile_out, _, t_want = tc.EDGE_PLANS[plan]
    assert T == t_want
    cuts = tc.edge_cuts(L, M, T, tile_out)
    assert sum(cuts) >= 3 * T + 9000 and all(cut < T - 1 for cut in cuts[6:11]) and tr.outputs_after(cuts[-1], L, M) > tile_out
    ks = [tr.grid(fo, kind, hz) for hz in tc.EDGE_SHIFTS[0]]
    kps = [tr.pitch_grid(fo, hz) for hz in tc.EDGE_PITCHES] if kind == tr.REAL else None
    assert ks[0] == 0 and ks[1] % 2 == 1 and (kps is None or kps[0] % 2 == 1)
    x = tc.edge_rows(sum(cuts), fo)[0]
    right, wrong = tr.Tap(h, L, M, kind, ks, kps), _StateMovedByOneWord(h, L, M, kind, ks, kps)
    differing, pos = [], 0
    for j, cut in enumerate(cuts):
        a, b = right.push(x[pos:pos + cut]), wrong.push(x[pos:pos + cut])
        pos += cut
        if len(a[0]) and all(not np.array_equal(a[t], b[t]) for t in range(2)):
            differing.append(j)
    assert {4, 5, len(cuts) - 1} <= set(differing), differing


# ------------------------------------------------------------------------------------------------------------ audio fold
def test_a_tone_two_pitches_below_the_station_stays_76_db_below_it_in_the_audio(designs):
    """The REAL kind at 8 kS/s, pitch 1000 Hz: a full-scale tone at hz lands at 1000 Hz in the audio.  One at hz - 2000 Hz would,
    through a filter open to 1000 Hz, be turned up to -1000 Hz and fold onto the station in the real part; the 800 Hz stop edge
    keeps it at least 76 dB down."""
    fo = 8000
    L, M, T, h = designs[(fo, tr.REAL)]
    k, kp = tr.grid(fo, tr.REAL, 14000.0), tr.pitch_grid(fo, 1000)
    hz = k * 252000 / 4096
    assert kp * fo / 4096 == 1000.0
    n = 252000 * 6 // 10
    t = np.arange(n)
    rms = []
    for f in (hz, hz - 2000.0):
        z = 32767 * np.exp(2j * np.pi * f * t / 252000)
        x = np.stack([np.rint(z.real), np.rint(z.imag)], axis=1).astype(np.int16)
        (a,), _ = tr.tap_all(x, h, L, M, tr.REAL, [k], [kp])
        a = a[tr.outputs_after(T, L, M):].astype(np.float64)
        rms.append(np.sqrt(np.mean(a * a)))
    db = 20 * np.log10(max(rms[1], 1e-9) / rms[0])
    print(f"station {rms[0]:.1f} rms, the tone two pitches below {rms[1]:.3f} rms: {db:.1f} dB")
    assert abs(rms[0] - 32767 / np.sqrt(2)) < 50 and db <= -76.0


# ------------------------------------------------------------------------------------------------------------ end to end
def _way_back(nv, case, y):
    """The tap's output of the case back at 252 kS/s: int16 [n, 2]."""
    import narrow_ref as nr
    import navtex_amd.narrow as nb
    import real_ref as rf
    c = tc.E2E[case]
    if c["back"] == "converter":
        L, M, T, h = nb.design(c["rate"], 2)
        return nr.interpolate_all(rf.convert_all(y[:len(y) // 2 * 2])[0], h, L, M, nr.S16, nr.IQ)[0]
    L, M, T, h = nb.design(c["rate"], 1)
    return nr.interpolate_all(y, h, L, M, nr.S16, nr.REAL if c["back"] == "real" else nr.IQ)[0]


def _decode(nv, back, tuned):
    import tune_ref as tu
    y1 = tu.front(back[:len(back) // nv.FRAME_IN * nv.FRAME_IN], False)
    return tu.messages(tu.decode(tu.chain(y1, 0, tu.k_of(tuned))))


@pytest.mark.parametrize("case", ["i", "ii", "iii", "iv"])
def test_stations_of_a_252k_row_through_taps_and_back_deliver_their_texts(nv, tp, oracle, case):
    """The row of the case (amplitude 8000 over noise 1500), a tap per station with the taps the library hands out, back
    through the interpolator's restatement, a chain tuned to what the tap left: the shift's residue, for audio on top of the
    pitch (and a quarter of the rate lower behind the real-input converter): exactly the text."""
    c = tc.E2E[case]
    fo, kind = c["rate"], c["kind"]
    L, M, T, h = tp.design(fo, kind)
    x = tc.row(nv, case)
    stations = list(c["stations"].items())
    ks = [tp.grid(fo, kind, hz)[0] for _, hz in stations]
    assert ks == [tr.grid(fo, kind, hz) for _, hz in stations]
    kps = [tr.pitch_grid(fo, tr.DEFAULT_PITCH_HZ)] * len(ks) if kind == tr.REAL else None
    ys, _ = tr.tap_all(x, h, L, M, kind, ks, kps)
    assert len(ys[0]) == tr.outputs_after(len(x), L, M)
    for t, (seed, hz) in enumerate(stations):
        tuned = tc.tuned_hz(case, hz, ks[t], kps[t] if kps else None)
        assert _decode(nv, _way_back(nv, case, ys[t]), tuned) == [signals.stream_text(seed)], (case, seed, tuned)


def test_a_tap_shifted_to_a_carrier_the_scan_found_delivers_its_text(nv, tp, oracle):
    """Case (v): a station 9371 Hz off the row's centre, where no chain is nominal.  The scan's restatement finds it; a tap is
    shifted to the offset found, and the chain behind the way back is tuned to the residue of that."""
    import scan_ref as sr
    c = tc.E2E["v"]
    (seed, hz), = c["stations"].items()
    x = tc.row(nv, "v")
    hits = sr.find(sr.scan(x[:8 * nv.FRAME_IN], False, n_frames=3, first_frame=4))
    found = hits[0]["offset_hz"]
    assert abs(found - hz) <= 5.0, hits
    L, M, T, h = tp.design(c["rate"], c["kind"])
    k, applied = tp.grid(c["rate"], c["kind"], found)
    (y,), _ = tr.tap_all(x, h, L, M, c["kind"], [k])
    assert _decode(nv, _way_back(nv, "v", y), found - applied) == [signals.stream_text(seed)]
