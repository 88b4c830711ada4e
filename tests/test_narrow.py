"""The narrowband interpolator (include/navtex_amd_narrow.h) on the CPU: the header and the companion library's exports and
argument safety, L, M and every call's count against fractions.Fraction, the refusals, the taps handed out held to the
project's two bars for twenty-six rates, the launch arithmetic against 128-bit integers (a stand-alone program under ASan +
UBSan), the restatement (tests/narrow_ref.py) against Python integers and on cuts anywhere, and end to end through the
restatement, the tuned chain's restatement and the oracle's character layer: six audio and low-rate IQ sources, each
delivering exactly its text."""
import ctypes as C
import re
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import narrow_cases as nc
import narrow_ref as nr
import signals

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "navtex_amd_narrow.h"
PLAN = ROOT / "navtex_amd" / "narrow" / "nvx_narrow_plan.h"
SYMBOLS = ["nvx_nb_config_default", "nvx_nb_create", "nvx_nb_design", "nvx_nb_destroy", "nvx_nb_last_error", "nvx_nb_plan", "nvx_nb_position",
           "nvx_nb_push", "nvx_nb_reset", "nvx_nb_resident", "nvx_nb_time_stats", "nvx_nb_timing"]
HOOKS = ["nvx_nb_debug_last_launch", "nvx_nb_debug_set_position"]


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


# ------------------------------------------------------------------------------------------------------------ interface
def test_header_compiles_as_plain_c_and_declares_the_entry_points(tmp_path):
    text = HEADER.read_text()
    assert sorted(set(re.findall(r"NVX_API\s+[\w\s\*]+?\b(\w+)\s*\(", text))) == SYMBOLS
    assert "audio / low-rate IQ -> (real ->) narrow -> scan -> tune -> decode" in text and "S = 14" in text and "2000 <= fi <= 96000" in text
    src = tmp_path / "t.c"
    src.write_text('#include "navtex_amd_narrow.h"\nint main(void){ nvx_nb_config c; c.format = NVX_NB_F32; c.kind = NVX_NB_REAL; '
                   'return NVX_NB_S16 == 0 && NVX_NB_U8 == 1 && NVX_NB_S8 == 2 && c.format == 3 && c.kind == 1 && NVX_NB_IQ == 0 && NVX_NB_SHIFT == 14 '
                   '&& sizeof c == 28 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


@pytest.mark.parametrize("sym", SYMBOLS + HOOKS)
def test_symbol_is_exported(nb, sym):
    assert hasattr(nb.lib, sym), f"{sym} is declared but not exported"


def test_the_companion_links_no_other_library_of_the_project_and_no_test_infrastructure(nb):
    lib = ROOT / "navtex_amd" / "libnavtex_amd_narrow.so"
    out = subprocess.run(["ldd", str(lib)], capture_output=True, text=True).stdout
    assert "libnavtex_amd" not in out and "oracle" not in out and "libamdhip64" in out
    # it defines nothing but its own interface and the tests' two hooks, and needs no nvx_ symbol from elsewhere
    nm = subprocess.run(["nm", "-D", str(lib)], capture_output=True, text=True, check=True).stdout
    defined = sorted(l.split()[-1] for l in nm.splitlines() if " T " in l and "nvx_" in l)
    assert defined == sorted(SYMBOLS + HOOKS) and all(d.startswith("nvx_nb_") for d in defined)
    assert not [h for h in HOOKS if h in HEADER.read_text()] and all(h in PLAN.read_text() for h in HOOKS)
    assert nb.lib.nvx_nb_debug_last_launch(None, None, None, None, None, None, None) < 0 and nb.lib.nvx_nb_debug_set_position(None, 0, 0) < 0
    assert not [l for l in nm.splitlines() if " U " in l and "nvx" in l]
    for path in (ROOT / "navtex_amd" / "narrow").iterdir():
        text = path.read_text()
        assert "oracle" not in text and "nvxo_" not in text, path
    assert "oracle" not in HEADER.read_text() and "oracle" not in (ROOT / "navtex_amd" / "narrow.py").read_text()
    assert C.sizeof(nb.Config) == 28


def test_null_nonsense_and_overflowing_arguments_are_errors_never_crashes(nb, tmp_path):
    src = ROOT / "tests" / "harness" / "null_args_narrow.c"
    exe = tmp_path / "null_args_narrow"
    lib = ROOT / "navtex_amd"
    subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib}", "-lnavtex_amd_narrow",
                    f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "narrow null-safety ok" in out.stdout, (out.stdout[-2500:], out.stderr[-500:])
    assert all(re.search(rf"\b{s}\(", src.read_text()) for s in SYMBOLS)


def test_create_returns_nodev_without_a_gpu_and_refuses_bad_parameters_first(nv, nb):
    if nv.device_count() > 0:
        pytest.skip("a GPU is present")
    cfg = nb.Config()
    nb.lib.nvx_nb_config_default(C.byref(cfg))
    h = C.c_void_p(1)
    assert nb.lib.nvx_nb_create(C.byref(cfg), C.byref(h)) == -2
    assert h.value is None and b"no CPU path" in nb.lib.nvx_nb_last_error()
    with pytest.raises(nv.NvxError) as e:
        nb.Interpolator(8000, format=nb.U8, kind=nb.REAL, n_streams=4)
    assert e.value.code == -2
    for kw in (dict(rate_num=1999), dict(rate_num=96001), dict(rate_num=12000, rate_den=0), dict(rate_num=12000, rate_den=3), dict(rate_num=2001),
               dict(rate_num=12000, kind=2), dict(rate_num=12000, format=4), dict(rate_num=12000, format=-1), dict(rate_num=12000, n_streams=0),
               dict(rate_num=12000, n_streams=65536), dict(rate_num=3999, rate_den=2)):
        with pytest.raises(nv.NvxError) as e:
            nb.Interpolator(**kw)
        assert e.value.code == nv._native.ERR_ARG, kw


# --------------------------------------------------------------------------------------------------------- rates, counts
def test_l_m_and_the_refusals(nv, nb):
    want = {(12000, 1): (21, 1), (8000, 1): (63, 2), (11025, 1): (160, 7), (11025, 2): (320, 7), (12500, 1): (504, 25), (96000, 1): (21, 8),
            (24000, 2): (21, 1), (2000, 1): (126, 1), (4000, 2): (126, 1), (192000, 2): (21, 8), (44100, 1): (40, 7), (7350, 1): (240, 7),
            (72000, 1): (7, 2), (67200, 1): (15, 4), (75600, 1): (10, 3), (70000, 1): (18, 5), (73332, 1): (1000, 291), (144000, 2): (7, 2),
            (84000, 1): (3, 1), (64800, 1): (35, 9)}
    for (num, den), (L, M) in want.items():
        f = Fraction(252000 * den, num)
        assert (f.numerator, f.denominator) == (L, M) == nr.ratio(num, den) == nb.design(num, den, taps=False)[:2], (num, den)
    for num, den, word in ((1999, 1, b"outside"), (96001, 1, b"outside"), (3999, 2, b"outside"), (192001, 2, b"outside"), (12000, 0, b"rate_den"),
                           (12000, 3, b"rate_den"), (2001, 1, b"1024 phases"), (0, 1, b"outside"), (2 ** 32 - 1, 1, b"outside")):
        assert nb.lib.nvx_nb_design(num, den, None, None, None, None, 0) == nv._native.ERR_ARG, (num, den)
        assert word in nb.lib.nvx_nb_last_error(), (num, den, nb.lib.nvx_nb_last_error())
    # every supported rate whose L fits: L T stays within the table
    for num in range(2000, 96001, 250):
        L, M, T, _ = nb.design(num, 1, taps=False)
        assert L <= 1024 and L * T <= 32768 and T % 2 == 0 and 12 <= T <= 30, num


@pytest.mark.parametrize("num,den", [(12000, 1), (8000, 1), (11025, 1), (11025, 2), (12500, 1), (96000, 1), (7350, 1)])
def test_every_calls_count_against_fractions_over_random_chunkings(nb, num, den):
    """Positions up to 2^62; calls of zero and of one sample among them."""
    L, M = nr.ratio(num, den)
    rng = np.random.default_rng(num + den)
    for start in (0, 1, 12345, 2 ** 32 - 1000, 2 ** 40 + 6, 2 ** 62 - 10 ** 6):
        chunks = [0, 1, 1, 0, 2, 29, 30] + [int(c) for c in rng.integers(0, 5000, size=40)] + [1, 0]
        want = nr.exact_counts(num, den, start, chunks)
        pos = start
        for c, w in zip(chunks, want):
            assert nb.out_count(L, M, pos, c) == w == nr.outputs_after(pos + c, L, M) - nr.outputs_after(pos, L, M), (start, pos, c)
            pos += c
        total = Fraction(pos) * Fraction(252000 * den, num)
        assert nr.outputs_after(pos, L, M) == -(-total.numerator // total.denominator)
    assert nr.exact_counts(num, den, 0, [0]) == [0] and nr.exact_counts(num, den, 0, [1])[0] == -(-L // M)


# ----------------------------------------------------------------------------------------------------------------- taps
@pytest.fixture(scope="module")
def designs(nb):
    return {rate: nb.design(*rate) for rate in nc.DESIGN_RATES}


@pytest.mark.parametrize("rate", nc.DESIGN_RATES, ids=lambda r: f"{r[0]}/{r[1]}")
def test_the_taps_handed_out_hold_the_two_bars(designs, rate):
    """Every phase sums to exactly 2^14; sum |h| <= 65535; the pass band within +-0.1 dB from 0 to fp; at most -76 dB from
    fi - fp to L fi / 2, on 8 points per side lobe.  Recorded from the C design: T = 30 (28 / 14 / 12 at 64 / 88.2 / 96 kS/s, and
    narrow_cases.T_OF_RATE's 16 .. 26 between 64.8 and 84 kS/s); sum |h| at most 37 892 (28 288 at 96 kS/s); pass band within
    0.0010 dB (84 kS/s, L = 3; 0.0006 dB elsewhere); stop band between -77.3 dB (72 kS/s, L = 7, T = 20: 1.3 dB inside the bar;
    -80.2 dB at 75.6 kS/s and -80.6 dB at 84 kS/s come next, then -80.8 dB at L = 21) and -90.1 dB."""
    num, den = rate
    L, M, T, h = designs[rate]
    fi = num / den
    fp = nr.pass_edge(Fraction(num, den))
    assert T == nc.T_OF_RATE.get(rate, 30) and h.shape == (L, T) and h.dtype == np.int16
    sums, abs_sums = h.astype(np.int64).sum(axis=1), np.abs(h.astype(np.int64)).sum(axis=1)
    assert np.all(sums == 1 << 14)
    pass_db = nr.response_db(h, L, fi, np.linspace(0.0, fp, 201))
    lobe = L * fi / (L * T)                                 # a side lobe of the window is about one bin of the prototype's length wide
    stop_f = np.arange(fi - fp, L * fi / 2, lobe / 8)
    stop_db = nr.response_db(h, L, fi, stop_f)
    print(f"{num}/{den}: L {L} M {M} T {T}, sum|h| <= {int(abs_sums.max())}, pass band within {float(np.abs(pass_db).max()):.4f} dB, "
          f"stop band at most {float(stop_db.max()):.1f} dB")
    assert abs_sums.max() <= 65535
    assert np.abs(pass_db).max() <= 0.1
    assert stop_db.max() <= -76.0
    # the recipe restated in numpy gives the same numbers, but for the last bit of a rounding
    L2, M2, T2, h2 = nr.design(num, den)
    assert (L2, M2, T2) == (L, M, T) and np.abs(h2.astype(np.int64) - h).max() <= 1


def test_the_launch_arithmetic_against_128_bit_integers_under_asan_ubsan(tmp_path):
    """nvx_narrow_plan.h's functions without a device (tests/harness/nb_launch_args.cpp): every output's (q, r), once, inside its
    tile's image; the staged span holds its window.  A stand-alone program under ASan + UBSan."""
    exe = tmp_path / "nb_launch_args"
    pkg = ROOT / "navtex_amd"
    subprocess.run(["g++", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    f"-I{ROOT / 'include'}", f"-I{pkg / 'csrc'}", f"-I{pkg / 'narrow'}",
                    str(ROOT / "tests" / "harness" / "nb_launch_args.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env={"ASAN_OPTIONS": "detect_leaks=1", "PATH": "/usr/bin:/bin"})
    assert out.returncode == 0 and "narrow launch args ok" in out.stdout, (out.stdout + out.stderr)[-3000:]


# ----------------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("rate", [(12000, 1), (11025, 1), (96000, 1)], ids=["12000", "11025", "96000"])
def test_the_numpy_restatement_equals_python_integers(designs, rate):
    L, M, T, h = designs[rate]
    x = nc.full_scale(nr.S16, nr.IQ, 120, 1)
    out, _ = nr.interpolate_all(x, h, L, M)
    c = nr.convert(x, nr.S16, nr.IQ)
    assert len(out) == nr.outputs_after(120, L, M)
    for n in list(range(0, 80)) + [len(out) // 2, len(out) - 1]:
        assert (int(out[n, 0]), int(out[n, 1])) == nr.output_int(c, h, L, M, n)[0], n
    assert np.array_equal(nr.pack(out).view(np.int16).reshape(-1, 2), out)


@pytest.mark.parametrize("kind", [nr.IQ, nr.REAL], ids=["iq", "real"])
def test_one_shot_equals_cuts_anywhere_and_real_is_iq_fed_zero_q(designs, kind):
    L, M, T, h = designs[(11025, 1)]
    n = 3000
    x = nc.signal(nr.S8, kind, n, 5)
    one, ref = nr.interpolate_all(x, h, L, M, nr.S8, kind)
    assert ref.consumed == n and ref.produced == len(one) == nr.outputs_after(n, L, M)
    c = nr.Interpolator(h, L, M, nr.S8, kind)
    pos, parts = 0, []
    for cut in [0, 1, T - 2, T - 1, T, 1, 0, 1500, 3, n - 1502 - 3 * T]:
        parts.append(c.push(x[pos:pos + cut])); pos += cut
        assert c.consumed == pos and c.produced == nr.outputs_after(pos, L, M) == sum(len(p) for p in parts)
    assert pos == n and np.array_equal(np.concatenate(parts), one)
    if kind == nr.REAL:
        assert not one[:, 1].any() and one[:, 0].any()
        iq = np.stack([x, np.zeros_like(x)], axis=1)
        assert np.array_equal(nr.interpolate_all(iq, h, L, M, nr.S8, nr.IQ)[0], one)


def test_the_rails_clamp_both_ways(designs):
    """Windows matched in sign to the phase with the largest sum |h|: the value before the clamp is beyond int16 both ways."""
    for rate in ((12000, 1), (8000, 1)):
        L, M, T, h = designs[rate]
        big = int(np.abs(h.astype(np.int64)).sum(axis=1).max())
        out, ref = nr.interpolate_all(nc.rails(h, nr.S16, nr.IQ, 8), h, L, M)
        assert ref.acc_max >> 14 > 70000 and ref.acc_min >> 14 < -70000 and ref.acc_max <= big * 32768
        assert out.max() == 32767 and out.min() == -32768
        assert {int(out[:, 0].max()), int(out[:, 0].min()), int(out[:, 1].max()), int(out[:, 1].min())} == {32767, -32768}


# ------------------------------------------------------------------------------------- the GPU edge cases, without a GPU
def test_the_edge_cases_reach_every_kernel_of_three_word_rows_and_tell_a_tap_row_shifted_by_one_entry():
    """What tests/test_gpu_narrow_edges.py reaches, from narrow_cases alone: for every format and kind at least three rates
    with ceil(T / 8) = 3, a full row (T = 24) and a padded one (T = 20) among them; and T = 16, 24 and 26.  And its inputs
    tell a wrong row from the right one: with every phase's taps moved by one entry, as a wrong number of zero taps in
    front of the row would have them, every stream of every case differs from the restatement."""
    runs = [(rate, fmt, kind) for rate, per_rate in nc.EDGE_RUNS.items() for fmt, kind in per_rate]
    for fmt in (nr.S16, nr.U8, nr.S8, nr.F32):
        for kind in (nr.IQ, nr.REAL):
            ts = [nc.EDGE_PLANS[rate][2] for rate, f, k in runs if (f, k) == (fmt, kind) and rate[1] == 1]
            three = [T for T in ts if (T + 7) // 8 == 3]
            assert len(three) >= 3 and 24 in three and 20 in three, (fmt, kind, ts)
    assert {16, 24, 26} <= {nc.EDGE_PLANS[rate][2] for rate, _, _ in runs}
    for rate, fmt, kind in runs:
        L, M, T, h = nr.design(*rate)
        assert (L, M, T) == nc.EDGE_PLANS[rate]
        moved = np.zeros_like(h)
        moved[:, 1:] = h[:, :-1]
        for row in nc.edge_rows(rate, fmt, kind):
            want, wrong = nr.interpolate_all(row, h, L, M, fmt, kind)[0], nr.interpolate_all(row, moved, L, M, fmt, kind)[0]
            assert (want != wrong).any(axis=1).mean() > 0.5, (rate, fmt, kind)


# ------------------------------------------------------------------------------------------------------------ end to end
def _decode(tr, y, nv, tuned):
    y1 = tr.front(y[:len(y) // nv.FRAME_IN * nv.FRAME_IN], False)
    k = tr.NOMINAL[0] if tuned is None else tr.k_of(tuned)
    return tr.messages(tr.decode(tr.chain(y1, 0, k)))


@pytest.mark.parametrize("seed", sorted(nc.E2E))
def test_audio_and_low_rate_iq_end_to_end_on_the_cpu(nv, nb, oracle, seed):
    """The source of the case at its own rate (amplitude 8000 over noise 1500), through the path of the case with the taps the
    library hands out, the chain tuned as the case says: exactly the text.  The REAL kind has Q = 0 and delivers nothing when
    the chain is tuned to the mirror."""
    import tune_ref as tr
    case = nc.E2E[seed]
    num, den, kind = nc.plan_of(seed)
    L, M, T, h = nb.design(num, den)
    src = nc.source(nv, seed)
    x = nc.interpolator_input(seed, src)
    y, _ = nr.interpolate_all(x, h, L, M, nr.S16, kind)
    assert len(y) == nr.outputs_after(len(x), L, M)
    assert _decode(tr, y, nv, case["tuned"]) == [signals.stream_text(seed)]
    if case["path"] == "real":
        assert not y[:, 1].any()
        assert _decode(tr, y, nv, -case["tuned"]) == []
