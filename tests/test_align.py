"""The row aligner (include/navtex_amd_align.h) on the CPU: the header and the companion library's exports and argument safety,
the shipped taps against the header's statements, the shared prototype's new variant, nvx_align_find against the restatement
(tests/align_ref.py) on tables made by the restatement, the launch arithmetic of both kernels against 128-bit integers (a
stand-alone program under ASan + UBSan), the restatement's own edges, the estimator's accuracy and the contrast's two sides,
and end to end through the oracle: the canceller's acceptance case with band-limited noise and a sense row 137.4 samples late,
twelve seeds, with and without the aligner."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import align_cases as alc
import align_ref as ar
import anc_cases as ac
import anc_ref

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "navtex_amd_align.h"
PLAN = ROOT / "navtex_amd" / "align" / "nvx_align_plan.h"
SYMBOLS = sorted(["nvx_align_config_default", "nvx_align_create", "nvx_align_destroy", "nvx_align_measure_resident", "nvx_align_window", "nvx_align_find",
                  "nvx_align_set_delay", "nvx_align_get_delay", "nvx_align_resident", "nvx_align_push", "nvx_align_reset", "nvx_align_position",
                  "nvx_align_plan", "nvx_align_delay", "nvx_align_taps", "nvx_align_timing", "nvx_align_time_stats", "nvx_align_last_error"])
HOOKS = ["nvx_align_debug_last_launch", "nvx_align_debug_set_position"]
T, G = ar.T, ar.G


@pytest.fixture(scope="module")
def al(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_align.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.align
    return navtex_amd.align


# ------------------------------------------------------------------------------------------------------------ interface
def test_header_compiles_as_plain_c_and_declares_the_entry_points(tmp_path):
    text = HEADER.read_text()
    assert sorted(set(re.findall(r"NVX_API\s+[\w\s\*]+?\b(\w+)\s*\(", text))) == SYMBOLS
    for name, want in (("NVX_ALIGN_PHASES", "32"), ("NVX_ALIGN_TAPS", "16"), ("NVX_ALIGN_GROUP_DELAY", "7"), ("NVX_ALIGN_MAX_DELAY_DEFAULT", "4096"),
                       ("NVX_ALIGN_MAX_DELAY_LIMIT", "1048576"), ("NVX_ALIGN_MIN_CONTRAST_DEFAULT", "64"), ("NVX_ALIGN_MAX_LAGS", "8192"),
                       ("NVX_ALIGN_MIN_WINDOW", "1024"), ("NVX_ALIGN_COHERENCE_ONE", "16384")):
        assert re.search(rf"#define {name}\s+{re.escape(want)}\b", text), name
    assert "Known limit" in text and "IQ-correct (each row) -> align -> cancel -> blank -> notch -> DDC / resample -> scan -> tune -> decode" in text
    src = tmp_path / "t.c"
    src.write_text('#include "navtex_amd_align.h"\nint main(void){ nvx_align_config c; nvx_align_estimate e; c.format = NVX_ALIGN_CF32; e.median_power = 0; '
                   'return NVX_ALIGN_CS16 == 0 && NVX_ALIGN_CU8 == 1 && NVX_ALIGN_CS8 == 2 && c.format == 3 && sizeof c == 24 && sizeof e == 32 && '
                   '!e.median_power ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


@pytest.mark.parametrize("sym", SYMBOLS + HOOKS)
def test_symbol_is_exported(al, sym):
    assert hasattr(al.lib, sym), f"{sym} is declared but not exported"


def test_the_companion_links_no_other_library_of_the_project_and_no_test_infrastructure(al):
    lib = ROOT / "navtex_amd" / "libnavtex_amd_align.so"
    out = subprocess.run(["ldd", str(lib)], capture_output=True, text=True).stdout
    assert "libnavtex_amd" not in out and "oracle" not in out and "libamdhip64" in out
    nm = subprocess.run(["nm", "-D", str(lib)], capture_output=True, text=True, check=True).stdout
    defined = sorted(l.split()[-1] for l in nm.splitlines() if " T " in l and "nvx_" in l)
    assert defined == sorted(SYMBOLS + HOOKS) and all(d.startswith("nvx_align_") for d in defined)
    assert not [h for h in HOOKS if h in HEADER.read_text()] and all(h in PLAN.read_text() for h in HOOKS)
    assert al.lib.nvx_align_debug_last_launch(None, None, None, None) < 0 and al.lib.nvx_align_debug_set_position(None, 0, 0) < 0
    assert not [l for l in nm.splitlines() if " U " in l and "nvx" in l]
    for path in (ROOT / "navtex_amd" / "align").iterdir():
        text = path.read_text()
        assert "oracle" not in text and "nvxo_" not in text, path
    assert "oracle" not in HEADER.read_text() and "oracle" not in (ROOT / "navtex_amd" / "align.py").read_text()
    assert C.sizeof(al.Config) == 24 and C.sizeof(al.Estimate) == 32
    assert (al.PHASES, al.TAPS, al.GROUP_DELAY, al.lib.nvx_align_delay()) == (32, 16, 7, 7)


def test_null_and_nonsense_arguments_are_errors_never_crashes(al, tmp_path):
    src = ROOT / "tests" / "harness" / "null_args_align.c"
    exe = tmp_path / "null_args_align"
    lib = ROOT / "navtex_amd"
    subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib}", "-lnavtex_amd_align",
                    f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "align null-safety ok" in out.stdout, (out.stdout[-2500:], out.stderr[-500:])
    assert all(re.search(rf"\b{s}\(", src.read_text()) for s in SYMBOLS)


def test_create_returns_nodev_without_a_gpu_and_refuses_bad_parameters_first(nv, al):
    for kw in (dict(max_delay=0), dict(max_delay=(1 << 20) + 1), dict(min_contrast=0), dict(format=4), dict(format=-1), dict(n_pairs=0), dict(n_pairs=65536)):
        with pytest.raises(nv.NvxError) as e:
            al.Aligner(**kw)
        assert e.value.code == nv._native.ERR_ARG, kw
    if nv.device_count() > 0:
        return                                                   # the rest is what a machine without a GPU answers
    cfg = al.Config()
    al.lib.nvx_align_config_default(C.byref(cfg))
    assert (cfg.struct_size, cfg.device, cfg.format, cfg.n_pairs, cfg.max_delay, cfg.min_contrast) == (24, 0, 0, 1, 4096, 64)
    h = C.c_void_p(1)
    assert al.lib.nvx_align_create(C.byref(cfg), C.byref(h)) == -2
    assert h.value is None and b"no CPU path" in al.lib.nvx_align_last_error()
    with pytest.raises(nv.NvxError) as e:
        al.Aligner(al.CU8, n_pairs=4)
    assert e.value.code == -2


def test_the_launch_arithmetic_against_128_bit_integers_under_asan_ubsan(tmp_path):
    """nvx_align_fill_args and nvx_align_fill_measure_args (navtex_amd/align/nvx_align_plan.h) without a device
    (tests/harness/align_launch_args.cpp).  A stand-alone program under ASan + UBSan."""
    exe = tmp_path / "align_launch_args"
    pkg = ROOT / "navtex_amd"
    subprocess.run(["g++", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT / 'include'}", f"-I{pkg / 'csrc'}", f"-I{pkg / 'align'}",
                    str(ROOT / "tests" / "harness" / "align_launch_args.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env={"ASAN_OPTIONS": "detect_leaks=1", "PATH": "/usr/bin:/bin"})
    assert out.returncode == 0 and "align launch args ok" in out.stdout, (out.stdout + out.stderr)[-3000:]


# ----------------------------------------------------------------------------------------------------------------- taps
def test_the_shipped_taps_phase_zero_the_sums_and_the_computed_response(al):
    """Phase 0 is the unit tap at G; every phase sums to exactly 2^14; sum |h| < 2 * 2^14 keeps the accumulator inside int32;
    over |f| <= 0.3 of the rate the gain stays within +-0.01 dB and the delay within 1/64 sample of G + f/32.  Computed:
    sum |h| <= 31 308, +-0.0024 dB, 0.0010 sample (the header and DESIGN 3.17 quote these)."""
    h = ar.taps()
    assert np.array_equal(h, al.taps().astype(np.int64)) and h.shape == (32, 16)
    assert h[0].tolist() == [0] * G + [16384] + [0] * (T - 1 - G)
    assert np.all(h.sum(axis=1) == 16384)
    sum_abs = int(np.abs(h).sum(axis=1).max())
    assert sum_abs < 2 * 16384 and sum_abs * 32768 + 8192 < 1 << 31
    assert np.array_equal(h[1:], h[:0:-1, ::-1])                  # phase f is phase 32 - f mirrored: the prototype is symmetric about its centre
    w = 2 * np.pi * np.linspace(-0.3, 0.3, 1201)
    k = np.arange(T)
    worst_db = worst_delay = 0.0
    for f in range(32):
        resp = (h[f][None, :] * np.exp(-1j * w[:, None] * k[None, :])).sum(axis=1) / 16384.0
        worst_db = max(worst_db, float(np.abs(20 * np.log10(np.abs(resp))).max()))
        phase = np.angle(resp * np.exp(1j * w * (G + f / 32)))
        nz = np.abs(w) > 1e-9
        worst_delay = max(worst_delay, float(np.abs(phase[nz] / w[nz]).max()), abs(float((h[f] * k).sum()) / 16384.0 - G - f / 32))
    print("sum |h|", sum_abs, "ripple", round(worst_db, 5), "dB, delay error", round(worst_delay, 5), "sample")
    assert worst_db <= 0.01 and worst_delay <= 1 / 64


def test_the_shared_prototype_is_a_call_of_the_variant_that_takes_the_centre(tmp_path):
    """nvx_pp_prototype(fc, L, T) equals nvx_pp_prototype_at(fc, L, T, (L T - 1) / 2) bit for bit, and the variant centred on
    a whole index gives a unit phase 0 at a Nyquist cut-off (tests/test_polyphase_design.py holds the three shipped designs)."""
    src = tmp_path / "pp.c"
    src.write_text('#include <string.h>\n#include <stdio.h>\n#include "nvx_polyphase_design.h"\n'
                   'int main(void){ long long *r1 = NULL, *r2 = NULL; int bad = 0;\n'
                   ' const struct { double fc; int L, T; } D[] = { { 0.5 / 63, 63, 58 }, { 0.0123, 21, 8 }, { 0.25, 1, 92 }, { 0.5 / 32, 32, 16 } };\n'
                   ' for (int i = 0; i < 4; i++) { double *a = nvx_pp_prototype(D[i].fc, D[i].L, D[i].T, &r1), *b = nvx_pp_prototype_at(D[i].fc, D[i].L, D[i].T, 0.5 * (D[i].L * D[i].T - 1), &r2);\n'
                   '  bad += memcmp(a, b, sizeof(double) * D[i].L * D[i].T) != 0; free(a); free(b); }\n'
                   ' double *p = nvx_pp_prototype_at(0.5 / 32, 32, 16, 256.0, &r1); int big; long long s = nvx_pp_phase(p, 32, 16, 0, 14, r1, &big);\n'
                   ' bad += !(s == 16384 && big == 8 && r1[8] == 16384); for (int k = 1; k < 256; k++) bad += p[256 - k] != p[256 + k]; free(p);\n'
                   ' printf("%d\\n", bad); return bad; }\n')
    exe = tmp_path / "pp"
    subprocess.run(["gcc", "-O1", "-Wall", "-Werror", "-ffp-contract=off", f"-I{ROOT / 'navtex_amd' / 'csrc'}", str(src), "-o", str(exe), "-lm"], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True).stdout.strip() == "0"


# ----------------------------------------------------------------------------------------------------------------- find
def _table(delay, seed, lag_first, n_lags=128, n=4096 + 400, **kw):
    a, b = alc.noise_pair(n, delay, seed, **kw)
    return ar.measure(a, b, ar.CS16, lag_first, n_lags)


@pytest.mark.parametrize("delay", [0.0, 3.0, -5.0, 17.25, -40.53125, 0.5, -0.5, 63 + 31 / 32, -(2 + 1 / 32)])
def test_find_equals_the_restatement_on_delays_of_both_signs(al, delay):
    lag_first = int(np.floor(delay)) - 60
    r, saa, sbb, n = _table(delay, 300 + int(abs(delay) * 32), lag_first)
    got, want = al.find(r, lag_first, n, saa, sbb), ar.find(r, lag_first, n, saa, sbb)
    assert got == want and got["reason"] == 0 and got["peak_lag"] in (int(np.floor(delay)), int(np.ceil(delay)))
    assert abs(got["delay_q5"] / 32 - delay) <= 1 / 32 and got["coherence_q14"] > 15000, got


def test_find_every_reason_and_the_first_admissible_lag(al):
    r, saa, sbb, n = _table(7.0, 5, -3)                      # the peak at index 10 = T/2 + 2: the first admissible
    for lag_first, reason in ((-3, 0), (-2, 2), (7 - 127 + 10, 0), (7 - 127 + 9, 2)):
        r, saa, sbb, n = _table(7.0, 5, lag_first)
        got = al.find(r, lag_first, n, saa, sbb)
        assert got == ar.find(r, lag_first, n, saa, sbb) and (got["reason"], got["peak_lag"]) == (reason, 7), (lag_first, got)
        assert (got["delay_q5"] == 7 * 32) == (reason == 0) and (got["median_power"] > 0) == (reason == 0)
    # reason 1: a silent row, on either side (SAA = N - 1 against N)
    assert al.find(r, -3, n, n - 1, sbb) == ar.find(r, -3, n, n - 1, sbb) and al.find(r, -3, n, n - 1, sbb)["reason"] == 1
    assert al.find(r, -3, n, saa, n - 1)["reason"] == 1 and al.find(r, -3, n, n, n)["reason"] != 1
    z = np.zeros((5000, 2), dtype=np.int16)
    rz, saa_z, sbb_z, nz = ar.measure(z, z, ar.CS16, -64, 128)
    assert (saa_z, sbb_z) == (0, 0) and al.find(rz, -64, nz, 0, 0) == ar.find(rz, -64, nz, 0, 0)
    # reason 3: a carrier the rows share, and rows that share nothing; min_contrast = 1 lets the latter through
    a, b = alc.carrier_pair(5000, 30, 1)
    rc, saa_c, sbb_c, nc = ar.measure(a, b, ar.CS16, -64, 128)
    got = al.find(rc, -64, nc, saa_c, sbb_c)
    assert got == ar.find(rc, -64, nc, saa_c, sbb_c) and got["reason"] == 3 and got["delay_q5"] == 0 and got["median_power"] > got["peak_power"] // 2
    a, b = alc.random_rows(ar.CS16, 5000, 2)
    rn, saa_n, sbb_n, nn = ar.measure(a, b, ar.CS16, -64, 128)
    assert al.find(rn, -64, nn, saa_n, sbb_n) == ar.find(rn, -64, nn, saa_n, sbb_n) and al.find(rn, -64, nn, saa_n, sbb_n)["reason"] in (2, 3)
    assert al.find(rn, -64, nn, saa_n, sbb_n, 1) == ar.find(rn, -64, nn, saa_n, sbb_n, 1)


def test_find_takes_the_first_of_equal_maxima(al):
    """(A, 0) at lag c and (0, A) at lag c + 1: P is equal at both (the coarse peak is the first), and the candidates of delay
    c and c + 1 both see the unit phase on one of the two: equal W, and the first in order of increasing delay wins.  The same
    at full scale, where the shift s is 23."""
    for amp in (1 << 20, (1 << 53) - 1):
        r = np.zeros((64, 2), dtype=np.int64)
        r[30, 0] = amp; r[31, 1] = amp
        got = al.find(r, -20, 4096, 1 << 40, 1 << 40)
        assert got == ar.find(r, -20, 4096, 1 << 40, 1 << 40) and (got["reason"], got["peak_lag"], got["delay_q5"]) == (0, 10, 320), got
        r[31, 1] = -amp - (1 if amp < 1 << 40 else 0)            # one more on the second: now it is the peak, and the delay c + 1
        got = al.find(r, -20, 4096, 1 << 40, 1 << 40)
        assert got == ar.find(r, -20, 4096, 1 << 40, 1 << 40)
        if amp < 1 << 40:
            assert (got["peak_lag"], got["delay_q5"]) == (11, 352), got


# ---------------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("fmt", (ar.CS16, ar.CU8, ar.CS8, ar.CF32))
def test_one_shot_equals_cuts_and_a_whole_delay_is_the_conversion_moved(fmt):
    import resample_ref as rr
    n = 3000
    a, b = alc.random_rows(fmt, n, 70 + fmt)
    ca, cb = rr.convert(a, fmt), rr.convert(b, fmt)
    for delay in (0, 32 * 9, -32 * 40, 5, -37, 32 * 40 - 1):
        one = ar.align(a, b, delay, fmt, 40)
        c = ar.Aligner(fmt, 40, delay)
        parts, pos = [], 0
        for cut in (0, 1, T - 1, T, 700, 1, n - 700 - 2 * T - 1):
            parts.append(c.push(a[pos:pos + cut], b[pos:pos + cut])); pos += cut
        assert pos == n and c.position == n
        assert np.array_equal(np.concatenate([p[0] for p in parts]), one[0]) and np.array_equal(np.concatenate([p[1] for p in parts]), one[1]), delay
        dm, ds, f = ar.split_delay(delay)
        assert 32 * dm - 32 * ds - f == delay
        assert np.array_equal(one[0][G + dm:], ca[:n - G - dm]) and not one[0][:G + dm].any()
        if f == 0:
            assert np.array_equal(one[1][G + ds:], cb[:n - G - ds]) and not one[1][:G + ds].any()


def test_a_delay_set_between_calls_reaches_into_the_carried_samples():
    a, b = alc.random_rows(ar.CS16, 2000, 3)
    c = ar.Aligner(ar.CS16, 100, 0)
    c.push(a[:1000], b[:1000])
    c.set_delay(32 * 90)
    out = c.push(a[1000:], b[1000:])
    assert np.array_equal(out[0], a[1000 - G - 90:2000 - G - 90]) and np.array_equal(out[1], b[1000 - G:2000 - G])


def test_the_aligned_rows_of_delayed_noise_cancel():
    """Common noise in 0.8 of the band, the sense row 20.3 samples late: behind the aligner the canceller's null is deeper
    than 25 dB; without it nothing is cancelled."""
    B = anc_ref.BLOCK
    a, b = alc.noise_pair(6 * B, 20.3, 9, own=0)
    r, saa, sbb, n = ar.measure(a[:B + 255], b[:B + 255], ar.CS16, -100, 256)
    e = ar.find(r, -100, n, saa, sbb)
    assert e["reason"] == 0 and abs(e["delay_q5"] / 32 - 20.3) <= 1 / 32
    ya, yb = ar.align(a, b, e["delay_q5"])
    depth = ac.power_db(anc_ref.cancel(ya, yb)[0][4 * B:], ya[4 * B:])
    plain = ac.power_db(anc_ref.cancel(a, b)[0][4 * B:], a[4 * B:])
    print("null depth behind the aligner", round(depth, 1), "dB, without it", round(plain, 1), "dB")
    assert depth <= -25.0 and plain >= -1.0


# ------------------------------------------------------------------------------------------------ accuracy and contrast
def test_the_estimators_accuracy_and_the_contrast_on_both_sides(al):
    """Twelve seeds, N = 65 536, 256 lags.  Common noise in 0.8 of the band, true delays anywhere: the estimate lies within
    1/32 sample (measured: at most 0.0174 off) and the contrast far above min_contrast = 64 (measured 1.6e4 .. 3.0e4).  Rows that share
    nothing stay far below it (measured 5.6 .. 16.2; the largest of 256 independent lags lies about 8 x above the median).  Noise
    that fills the whole band is outside the statement; its error is printed."""
    rng = np.random.default_rng(2024)
    errors, full_band, shared, nothing = [], [], [], []
    for seed in alc.SEEDS:
        delay = float(rng.uniform(-90, 90))
        lag_first = int(np.floor(delay)) - 128
        for band, sink in ((alc.BAND, errors), (1.0, full_band)):
            a, b = alc.noise_pair(65536 + 255, delay, seed, band=band)
            r, saa, sbb, n = ar.measure(a, b, ar.CS16, lag_first, 256)
            e = ar.find(r, lag_first, n, saa, sbb)
            assert n == 65536 and e["reason"] == 0 and e == al.find(r, lag_first, n, saa, sbb)
            sink.append(abs(e["delay_q5"] / 32 - delay))
            if band < 1.0:
                shared.append(e["peak_power"] / e["median_power"])
        a, b = alc.random_rows(ar.CS16, 65536 + 255, seed)
        r, saa, sbb, n = ar.measure(a, b, ar.CS16, -128, 256)
        e = ar.find(r, -128, n, saa, sbb, 1)
        nothing.append(e["peak_power"] / e["median_power"])
        assert ar.find(r, -128, n, saa, sbb)["reason"] in (2, 3)
    print("error in 0.8 of the band: max", round(max(errors), 4), "; full band: max", round(max(full_band), 4), "; contrast shared", round(min(shared)),
          "..", round(max(shared)), "; nothing shared", round(min(nothing), 1), "..", round(max(nothing), 1))
    assert max(errors) <= 1 / 32
    assert min(shared) >= 100 * ar.MIN_CONTRAST_DEFAULT and max(nothing) <= ar.MIN_CONTRAST_DEFAULT / 3


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def acceptance(nv, oracle):
    """The twelve seeds, once: what arrives from the canceller alone and from the canceller behind measure -> find -> align."""
    want = ac.text()
    got = {"plain": 0, "aligned": 0}
    found = []
    for seed in alc.SEEDS:
        a, b = alc.pair(nv, seed)
        r, saa, sbb, n = ar.measure(a[:alc.MEASURE_N], b[:alc.MEASURE_N], ar.CS16, alc.LAG_FIRST, alc.N_LAGS)
        e = ar.find(r, alc.LAG_FIRST, n, saa, sbb)
        ya, yb = ar.align(a, b, e["delay_q5"])
        y, ref = anc_ref.cancel(ya, yb)
        y0, ref0 = anc_ref.cancel(a, b)
        got["aligned"] += ac.delivered(oracle, y, nv.FRAME_IN)[0] == [want]
        got["plain"] += ac.delivered(oracle, y0, nv.FRAME_IN)[0] == [want]
        found.append((e, ref.c, ref.coherence, ref0.c, ref0.coherence))
    print("490 delivered: canceller alone", got["plain"], "behind the aligner", got["aligned"], "of 12;", [(f[0]["delay_q5"], f[2], f[4]) for f in found])
    return got, found


def test_the_acceptance_case_delivers_behind_the_aligner_only(acceptance):
    """The canceller's acceptance case (490 at -14 kHz, amplitude 300, common noise of +-6000, +-150 of each receiver's own, W = 4)
    with the common noise confined to 0.8 of the band and everything the sense antenna receives 137.4 samples late: the first
    values tried.  Measured: the canceller alone 0 of 12, restated measure -> find -> align -> cancel 12 of 12."""
    got, _ = acceptance
    assert got["plain"] == 0
    assert got["aligned"] == 12


def test_the_acceptance_cases_delay_and_coherence(acceptance):
    """The delay found is 137.4 to the grid (4397 / 32 = 137.406); behind the aligner the canceller sees the coherence of the
    sample-aligned case, without it none."""
    _, found = acceptance
    for e, c, coherence, c0, coherence0 in found:
        assert e["reason"] == 0 and abs(e["delay_q5"] - alc.DELAY * 32) <= 1 and e["peak_lag"] == 137, e
        assert coherence > 15000 and coherence0 < 100, (coherence, coherence0)
        assert abs(c[0] - ac.WEIGHT[0]) <= 60 and abs(c[1] - ac.WEIGHT[1]) <= 60, c
