"""The zoom bank (include/navtex_amd_zoom.h) on the CPU: the header and the companion library's exports and argument safety,
the grid rule, the taps and the filter's figures computed from them for every k, the launch arithmetic against 128-bit
integers (a stand-alone program under ASan + UBSan), the restatement (tests/zoom_ref.py) against Python integers, against
itself on cuts anywhere, at kz = 0 and across a retune, tones on FFT bins, and end to end through the oracle: the acceptance
case (three services from one 1.008 MS/s row, an interferer one output band beside the weak one, twelve seeds)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import zoom_cases as zc
import zoom_ref as zr

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "navtex_amd_zoom.h"
PLAN = ROOT / "navtex_amd" / "zoom" / "nvx_zoom_plan.h"
SYMBOLS = ["nvx_zoom_config_default", "nvx_zoom_create", "nvx_zoom_destroy", "nvx_zoom_get_shift", "nvx_zoom_grid", "nvx_zoom_last_error", "nvx_zoom_plan",
           "nvx_zoom_position", "nvx_zoom_push", "nvx_zoom_reset", "nvx_zoom_resident", "nvx_zoom_set_shift", "nvx_zoom_taps", "nvx_zoom_time_stats",
           "nvx_zoom_timing"]
HOOKS = ["nvx_zoom_debug_last_launch", "nvx_zoom_debug_set_position"]
TAPS = (10376, 3314, 1825, 1144, 745, 486, 310, 191, 111, 60, 30, 13, 4, 1)
FORMATS = (zr.CS16, zr.CU8, zr.CS8, zr.CF32)
KS = (1, 2, 3, 4, 5, 6)


@pytest.fixture(scope="module")
def zl(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_zoom.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.zoom
    return navtex_amd.zoom


# ------------------------------------------------------------------------------------------------------------ interface
def test_header_compiles_as_plain_c_and_declares_the_entry_points(tmp_path):
    text = HEADER.read_text()
    assert sorted(set(re.findall(r"NVX_API\s+[\w\s\*]+?\b(\w+)\s*\(", text))) == SYMBOLS
    assert ", ".join(str(t) for t in TAPS) in text and "decimate in the radio" in text
    assert "(real ->) zoom -> IQ-correct / blank / notch -> DDC / resample -> scan -> tune -> decode" in text
    assert "+-0.01 dB" in text and "-76 dB" in text and "-99.8 dBc" in text
    src = tmp_path / "t.c"
    src.write_text('#include "navtex_amd_zoom.h"\nint main(void){ nvx_zoom_config c; c.format = NVX_ZOOM_CF32; c.log2_decim = NVX_ZOOM_MAX_LOG2; '
                   'return NVX_ZOOM_CS16 == 0 && NVX_ZOOM_CU8 == 1 && NVX_ZOOM_CS8 == 2 && c.format == 3 && c.log2_decim == 6 && sizeof c == 24 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


@pytest.mark.parametrize("sym", SYMBOLS + HOOKS)
def test_symbol_is_exported(zl, sym):
    assert hasattr(zl.lib, sym), f"{sym} is declared but not exported"


def test_the_companion_links_no_other_library_of_the_project_and_no_test_infrastructure(zl):
    lib = ROOT / "navtex_amd" / "libnavtex_amd_zoom.so"
    out = subprocess.run(["ldd", str(lib)], capture_output=True, text=True).stdout
    assert "libnavtex_amd" not in out and "oracle" not in out and "libamdhip64" in out
    nm = subprocess.run(["nm", "-D", str(lib)], capture_output=True, text=True, check=True).stdout
    defined = sorted(l.split()[-1] for l in nm.splitlines() if " T " in l and "nvx_" in l)
    assert defined == sorted(SYMBOLS + HOOKS) and all(d.startswith("nvx_zoom_") for d in defined)
    assert not [h for h in HOOKS if h in HEADER.read_text()] and all(h in PLAN.read_text() for h in HOOKS)
    assert zl.lib.nvx_zoom_debug_last_launch(None, None, None, None, None, None) < 0 and zl.lib.nvx_zoom_debug_set_position(None, 0, 0) < 0
    assert not [l for l in nm.splitlines() if " U " in l and "nvx" in l]
    for path in (ROOT / "navtex_amd" / "zoom").iterdir():
        text = path.read_text()
        assert "oracle" not in text and "nvxo_" not in text, path
        # the taps and the table are included, not copied
        assert "10376" not in text and "32766" not in text, path
    assert "oracle" not in HEADER.read_text() and "oracle" not in (ROOT / "navtex_amd" / "zoom.py").read_text()
    assert C.sizeof(zl.Config) == 24


def test_the_headers_constants_and_formats_agree_with_the_mirror(zl):
    text = HEADER.read_text()
    define = lambda name: int(re.search(rf"#define {name}\s+\(?(-?\d+)\)?", text).group(1))      # noqa: E731
    assert (define("NVX_ZOOM_GRID"), define("NVX_ZOOM_KZ_MIN"), define("NVX_ZOOM_KZ_MAX")) == (zl.GRID, zl.KZ_MIN, zl.KZ_MAX) == (zr.N, zr.KZ_MIN, zr.KZ_MAX)
    assert (define("NVX_ZOOM_MAX_ZOOMS"), define("NVX_ZOOM_MIN_LOG2"), define("NVX_ZOOM_MAX_LOG2")) == (zl.MAX_ZOOMS, zl.MIN_LOG2, zl.MAX_LOG2) == (8, 1, 6)
    assert (define("NVX_ZOOM_STAGE_REACH"), define("NVX_ZOOM_STAGE_DELAY")) == (zl.STAGE_REACH, zl.STAGE_DELAY) == (zr.REACH, zr.DELAY)
    assert [define(f"NVX_ZOOM_{n}") for n in ("CS16", "CU8", "CS8", "CF32")] == [zl.CS16, zl.CU8, zl.CS8, zl.CF32] == list(FORMATS)
    assert int(re.search(r"#define NVX_ZOOM_BLOCK (\d+)", PLAN.read_text()).group(1)) == zl.BLOCK
    assert [zl.history(k) for k in KS] == [zr.history(k) for k in KS] == [53, 159, 371, 795, 1643, 3339]
    assert zl.BYTES_PER_SAMPLE == {zl.CS16: 4, zl.CU8: 2, zl.CS8: 2, zl.CF32: 8}


def test_null_and_nonsense_arguments_are_errors_never_crashes(zl, tmp_path):
    src = ROOT / "tests" / "harness" / "null_args_zoom.c"
    exe = tmp_path / "null_args_zoom"
    lib = ROOT / "navtex_amd"
    subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib}", "-lnavtex_amd_zoom",
                    f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-lm"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "zoom null-safety ok" in out.stdout, (out.stdout[-2500:], out.stderr[-500:])
    assert all(re.search(rf"\b{s}\(", src.read_text()) for s in SYMBOLS)


def test_create_refuses_bad_parameters_first_and_returns_nodev_without_a_gpu(nv, zl):
    for kw in (dict(log2_decim=0), dict(log2_decim=7), dict(log2_decim=2, format=4), dict(log2_decim=2, format=-1), dict(log2_decim=2, n_inputs=0),
               dict(log2_decim=2, n_zooms=0), dict(log2_decim=2, n_zooms=9), dict(log2_decim=2, n_inputs=65536), dict(log2_decim=2, n_inputs=32768, n_zooms=2)):
        with pytest.raises(nv.NvxError) as e:
            zl.Zoom(**kw)
        assert e.value.code == nv._native.ERR_ARG, kw
    if nv.device_count() == 0:                              # with a device the GPU files create plans
        cfg = zl.Config()
        zl.lib.nvx_zoom_config_default(C.byref(cfg))
        h = C.c_void_p(1)
        assert zl.lib.nvx_zoom_create(C.byref(cfg), C.byref(h)) == -2
        assert h.value is None and b"no CPU path" in zl.lib.nvx_zoom_last_error()
        with pytest.raises(nv.NvxError) as e:
            zl.Zoom(5, zl.CU8, n_inputs=4, n_zooms=3)
        assert e.value.code == -2


# ------------------------------------------------------------------------------------------------------- grid and taps
def test_the_taps_are_the_converters(nv, zl):
    import navtex_amd.real as rl
    assert zl.taps() == (TAPS, 53, 15) and zr.TAPS == TAPS and rl.taps()[0] == zl.taps()[0]
    assert zl.lib.nvx_zoom_taps((C.c_int16 * 13)(), 13, None, None) == nv._native.ERR_ARG and zl.lib.nvx_zoom_taps(None, 0, None, None) == 14


def test_the_grid_rounds_ties_to_even_and_refuses_what_leaves_the_range(nv, zl):
    # at a rate of 4096 a table step is 1 Hz: the ties are exact
    for hz, kz in ((0.5, 0), (1.5, 2), (2.5, 2), (-0.5, 0), (-1.5, -2), (-2.5, -2), (0.49, 0), (0.51, 1), (2047.5, None), (2047.49, 2047), (-2048.5, -2048),
                   (-2048.51, None), (2048.0, None)):
        assert zr.grid(4096, hz) == kz, hz
        if kz is None:
            with pytest.raises(zl.ZoomError) as e:
                zl.grid(4096, hz)
            assert e.value.code == nv._native.ERR_ARG
        else:
            assert zl.grid(4096, hz) == (kz, float(kz)), hz
    rng = np.random.default_rng(5)
    for rate in (1008000, 8064000, 10e6, 20e6, 64.8e6 / 2, 130e6 / 2, 2.4e6 + 0.5):
        for hz in list(rng.uniform(-0.49 * rate, 0.49 * rate, size=40)) + [0.0, rate / 8192, -rate / 8192, 3 * rate / 8192, rate / 4096]:
            kz, applied = zl.grid(rate, hz)
            assert kz == zr.grid(rate, hz) and applied == kz * rate / 4096 and abs(hz - applied) <= rate / 8192 * (1 + 1e-12), (rate, hz)
    for rate, hz in ((1e6, float("nan")), (1e6, float("inf")), (1e6, -float("inf")), (0.0, 1.0), (-1.0, 1.0), (float("nan"), 1.0), (float("inf"), 1.0)):
        assert zr.grid(rate, hz) is None
        with pytest.raises(zl.ZoomError):
            zl.grid(rate, hz)
    assert zc.centres() == ((-1219, -1219 * 1008000 / 4096), (1422, 1422 * 1008000 / 4096))


@pytest.mark.parametrize("k", KS)
def test_the_filters_figures_computed_from_the_taps(k):
    """The taps sum to 2^15 and their magnitudes to 53604; |acc| stays below 2^31 - 2^14; over the inner 80 % of the output band
    the ripple is within +-0.01 dB, and every folding path is at most -76 dB (computed: -0.0006 .. +0.0037 dB and -78.99 dB)."""
    h = zr.lowpass()
    assert len(h) == 55 and h.sum() == 1 << 15 and np.abs(h).sum() == 53604 == zr.ABS_SUM and h[27] == 1 << 14
    assert np.array_equal(h, h[::-1]) and not h[1:27:2].any() and [int(abs(v)) for v in h[28::2]] == list(TAPS)
    assert zr.ACC_MAX == 1756495872 < (1 << 31) - (1 << 14)
    lo, hi, fold = zr.ripple_and_folding_db(k)
    print("k", k, "ripple", round(lo, 5), "..", round(hi, 5), "dB; folding at most", round(fold, 2), "dB")
    assert -0.01 <= lo <= hi <= 0.01
    assert fold <= -76.0
    assert zr.delay(k) == 26 * ((1 << k) - 1) and zr.history(k) == 53 * ((1 << k) - 1)


def test_the_launch_arithmetic_against_128_bit_integers_under_asan_ubsan(tmp_path):
    """nvx_zoom_fill_args (navtex_amd/zoom/nvx_zoom_plan.h) without a device: positions up to 2^62, every k, call lengths around
    D, H, a tile and a chunk, every chunking -- each output in one group of one tile of one chunk, its window inside the state
    plus the call and inside what its chunk walked, the LDS planes' bounds, the state's writer, 16-byte stores only on aligned
    rows (tests/harness/zoom_launch_args.cpp).  A stand-alone program under ASan + UBSan."""
    exe = tmp_path / "zoom_launch_args"
    pkg = ROOT / "navtex_amd"
    subprocess.run(["g++", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT / 'include'}", f"-I{pkg / 'csrc'}", f"-I{pkg / 'zoom'}", f"-I{pkg / 'real'}",
                    str(ROOT / "tests" / "harness" / "zoom_launch_args.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env={"ASAN_OPTIONS": "detect_leaks=1", "PATH": "/usr/bin:/bin"})
    assert out.returncode == 0 and "zoom launch args ok" in out.stdout, (out.stdout + out.stderr)[-3000:]


# ----------------------------------------------------------------------------------------------------------- restatement
def test_the_numpy_restatement_equals_python_integers():
    x = zc.full_scale(zr.CS16, 2 * 400, 1)
    c = zr.rr.convert(x, zr.CS16)
    out, ref = zr.zoom_all(x, 1)
    for m in list(range(0, 60)) + [399]:
        assert (zr.stage_int(c[:, 0], m)[0], zr.stage_int(c[:, 1], m)[0]) == tuple(int(v) for v in out[0, m]), m
    # two stages: the second over the first's outputs
    out2, _ = zr.zoom_all(x, 2)
    u1 = out[0].astype(np.int64)
    for m in list(range(0, 40)) + [199]:
        assert zr.stage_int(u1[:, 0], m)[0] == int(out2[0, m, 0]), m
    assert ref.acc[0] < 0 < ref.acc[1]


@pytest.mark.parametrize("k", (1, 3, 6))
@pytest.mark.parametrize("fmt", FORMATS, ids=("cs16", "cu8", "cs8", "cf32"))
def test_one_shot_equals_cuts_anywhere_and_kz_0_equals_the_unmixed_stages(fmt, k):
    D = 1 << k
    n = D * 90 + 5
    x = zc.full_scale(fmt, n, 10 + fmt)
    kzs = (0, 37, -2048)
    one, ref1 = zr.zoom_all(x, k, kzs, fmt)
    assert one.shape == (3, n // D, 2) and ref1.consumed == n and ref1.produced == n // D and len(ref1.held) == n % D
    rng = np.random.default_rng(k)
    ref, parts, pos = zr.Zoom(k, kzs, fmt), [], 0
    for cut in [1, D - 1, D + 1, 3 * D + 2, 0] + list(rng.integers(0, 4 * D, size=30)) + [n]:
        cut = min(int(cut), n - pos)
        parts.append(ref.push(x[pos:pos + cut])); pos += cut
        assert ref.consumed == pos and ref.produced == pos // D
    assert np.array_equal(np.concatenate(parts, axis=1), one)
    # kz = 0: the stages on the converted samples themselves
    u = np.concatenate([np.zeros((zr.history(k), 2), dtype=np.int64), zr.rr.convert(x, fmt)[:n // D * D]])
    for _ in range(k):
        u = zr.stage(u[:zr.REACH], u[zr.REACH:])
    assert np.array_equal(u, one[0])
    assert not np.array_equal(one[0], one[1])


@pytest.mark.parametrize("k", (1, 3, 6))
def test_a_retune_is_as_if_the_zoom_always_had_it_from_the_next_call_on(k):
    D = 1 << k
    n1, n2 = D * 70, D * 50
    x = zc.signal(zr.CS16, n1 + n2, 20 + k)
    ref = zr.Zoom(k, (100,))
    before = ref.push(x[:n1])
    ref.set_shift(0, -731)
    after = ref.push(x[n1:])
    assert np.array_equal(before[0], zr.zoom_all(x[:n1], k, (100,))[0][0])
    assert np.array_equal(after[0], zr.zoom_all(x, k, (-731,))[0][0, n1 // D:])
    ref.reset()
    assert ref.kz == [-731] and ref.consumed == 0


# ----------------------------------------------------------------------------------------------------------------- tones
@pytest.mark.parametrize("b", zc.TONE_BINS)
@pytest.mark.parametrize("k,kz", ((1, 777), (3, -1500), (6, 2047)))
def test_a_tone_on_a_bin_has_unit_gain_and_what_folds_onto_it_is_below_76_dbc(k, kz, b):
    """A tone of amplitude 20 000 that comes out on bin b of 4096 outputs: its rms within 0.01 dB of the input's.  The same tone
    moved by a / D of the input rate, a = 1 .. D - 1 (at k = 6: the nearest, the one in the middle and the farthest aliases),
    folds onto the same bin: at most -76 dBc there (Blackman window)."""
    D = 1 << k
    out, _ = zr.zoom_all(zc.tone(k, kz, b), k, (kz,))
    gain_db, level_db = zc.tone_levels(out[0], b)
    print("k", k, "kz", kz, "bin", b, "gain by rms", round(gain_db, 4), "dB, on the bin", round(level_db, 4), "dB")
    assert abs(gain_db) <= 0.01
    assert abs(level_db) <= 0.01
    for a in sorted({1, D // 2, D - 1}):
        folded, _ = zr.zoom_all(zc.tone(k, kz, b, fold=a), k, (kz,))
        _, alias_db = zc.tone_levels(folded[0], b)
        naive_db = zc.tone_levels(zr.naive(zc.tone(k, kz, b, fold=a), k, kz), b)[1]
        print("   alias", a, "comes out at", round(alias_db, 1), "dBc; kept every", D, "th sample:", round(naive_db, 1), "dBc")
        assert alias_db <= -76.0
        assert naive_db > -1.0


# ------------------------------------------------------------------------------------------------------------ end to end
def test_the_acceptance_case(nv, oracle):
    """A row at 1.008 MS/s, k = 2: zoom A near -300 kHz has 518 (amplitude 8000) at +14 kHz and 490 (amplitude 300, under noise
    zc.NOISE) at -14 kHz of its applied centre; an interferer of amplitude zc.INTERFERER with a third text 252 kHz above the
    490 carrier; zoom B near +350 kHz has a fourth text at +14 kHz.  Twelve seeds.  Z: the restatement's rows decoded by the
    oracle's two chains; N: every fourth mixed sample of zoom A.  The rules that fix the two amplitudes: the noise starts at
    1500 and falls by 250 until Z delivers 490 twelve times of twelve (1500 does); the interferer starts at 8000 and doubles,
    to at most 12 000, until N delivers 490 from none of twelve (8000 does)."""
    t518, t490, t_int, t4209 = zc.texts()
    (ka, _), (kb, _) = zc.centres()
    assert zc.NOISE == 1500 and zc.INTERFERER == zc.AMP_518 == 8000 and len({t518, t490, t_int, t4209}) == 4
    got = {"A518": 0, "A490": 0, "B": 0, "N490": 0, "N_int": 0}
    for seed in zc.SEEDS:
        x = zc.wide_row(nv, seed)
        rows, _ = zr.zoom_all(x, zc.K, (ka, kb))
        assert rows.shape[1] % nv.FRAME_IN == 0
        a, _ = zc.delivered(oracle, rows[0], nv.FRAME_IN)
        b, _ = zc.delivered(oracle, rows[1], nv.FRAME_IN)
        n, _ = zc.delivered(oracle, zr.naive(x, zc.K, ka), nv.FRAME_IN)
        got["A518"] += a[518] == [t518]; got["A490"] += a[490] == [t490]; got["B"] += b[518] == [t4209]
        got["N490"] += n[490] == [t490]; got["N_int"] += n[490] == [t_int]
    print("noise", zc.NOISE, "interferer", zc.INTERFERER, "|", got)
    assert got["A490"] == 12                                # the rule that fixes zc.NOISE
    assert got["N490"] == 0                                 # the rule that fixes zc.INTERFERER
    assert got["A518"] == 12 and got["B"] == 12
