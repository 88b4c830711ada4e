"""The spectrum monitor (include/navtex_amd_spec.h) on the CPU: the header and the companion library's exports and argument
safety, the generated table against the band scan's, the launch arithmetic against 128-bit integers (a stand-alone program
under ASan + UBSan), the restatement (tests/spec_ref.py) on cuts at and next to H, N, a line's hop and a line's span, at every
averaging and size the kernels take another path for, on tones, zeros and the rails and through measure in mid-stream, and the
finder: nothing in noise, and the acceptance case (the notch's row: a weak 490 station and two carriers the finder is not told
of, twelve seeds) through the notch's restatement and the oracle."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import notch_ref as nr
import resample_ref as rr
import scan_ref
import spec_cases as sc
import spec_ref as sr

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "navtex_amd_spec.h"
PLAN = ROOT / "navtex_amd" / "spec" / "nvx_spec_plan.h"
SYMBOLS = ["nvx_spec_config_default", "nvx_spec_create", "nvx_spec_destroy", "nvx_spec_find_lines", "nvx_spec_get", "nvx_spec_last_error",
           "nvx_spec_lines_for", "nvx_spec_measure", "nvx_spec_params_default", "nvx_spec_plan", "nvx_spec_position", "nvx_spec_push", "nvx_spec_reset",
           "nvx_spec_resident", "nvx_spec_time_stats", "nvx_spec_timing"]
HOOKS = ["nvx_spec_debug_last_launch", "nvx_spec_debug_set_position", "nvx_spec_debug_set_scratch"]
FORMATS = (sr.CS16, sr.CU8, sr.CS8, sr.CF32)


@pytest.fixture(scope="module")
def sp(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_spec.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.spec
    return navtex_amd.spec


# ------------------------------------------------------------------------------------------------------------ interface
def test_header_compiles_as_plain_c_and_declares_the_entry_points(tmp_path):
    text = HEADER.read_text()
    assert sorted(set(re.findall(r"NVX_API\s+[\w\s\*]+?\b(\w+)\s*\(", text))) == SYMBOLS
    for name, want in (("NVX_SPEC_LOG2_MIN", "8"), ("NVX_SPEC_LOG2_MAX", "12"), ("NVX_SPEC_LOG2_DEFAULT", "11"), ("NVX_SPEC_AVG_DEFAULT", "8"),
                       ("NVX_SPEC_MAX_HOP", "65536")):
        assert re.search(rf"#define {name}\s+{re.escape(want)}\b", text), name
    assert "IQ-correct -> cancel -> blank -> [spectrum -> find_lines ->] notch -> DDC / resample -> scan -> tune -> decode" in text
    # the known limits are the header's to state
    assert "Known limits." in text
    for words in ("A carrier weaker than what else falls into its bin", "Below about 20 ms per", "names steady lines, not what they are",
                  "The level word is for display, not for arithmetic"):
        assert words in text, words
    src = tmp_path / "t.c"
    src.write_text('#include "navtex_amd_spec.h"\nint main(void){ nvx_spec_config c; nvx_spec_params p; nvx_spec_hit h; c.format = NVX_SPEC_CF32; p.min_lines = 0; h.bin = 0; '
                   'return NVX_SPEC_CS16 == 0 && NVX_SPEC_CU8 == 1 && NVX_SPEC_CS8 == 2 && c.format == 3 && sizeof c == 24 && sizeof p == 32 && sizeof h == 32 && '
                   'NVX_SPEC_LEVEL_ZERO == 253696 && NVX_SPEC_LEVEL_DB(8192) == 0.0 && NVX_SPEC_LEVEL_DB(8448) > 3.0102 && NVX_SPEC_LEVEL_DB(8448) < 3.0104 && '
                   '!p.min_lines && !h.bin ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


@pytest.mark.parametrize("sym", SYMBOLS + HOOKS)
def test_symbol_is_exported(sp, sym):
    assert hasattr(sp.lib, sym), f"{sym} is declared but not exported"


def test_the_companion_links_no_other_library_of_the_project_and_no_test_infrastructure(sp):
    lib = ROOT / "navtex_amd" / "libnavtex_amd_spec.so"
    out = subprocess.run(["ldd", str(lib)], capture_output=True, text=True).stdout
    assert "libnavtex_amd" not in out and "oracle" not in out and "libamdhip64" in out
    # it defines nothing but its own interface and the tests' three hooks, and needs no nvx_ symbol from elsewhere
    nm = subprocess.run(["nm", "-D", str(lib)], capture_output=True, text=True, check=True).stdout
    defined = sorted(l.split()[-1] for l in nm.splitlines() if " T " in l and "nvx_" in l)
    assert defined == sorted(SYMBOLS + HOOKS) and all(d.startswith("nvx_spec_") for d in defined)
    assert not [h for h in HOOKS if h in HEADER.read_text()] and all(h in PLAN.read_text() for h in HOOKS)
    assert sp.lib.nvx_spec_debug_last_launch(None, None, None, None, None) < 0 and sp.lib.nvx_spec_debug_set_position(None, 0, 0) < 0
    assert sp.lib.nvx_spec_debug_set_scratch(None, 0) < 0
    assert not [l for l in nm.splitlines() if " U " in l and "nvx" in l]
    for path in (ROOT / "navtex_amd" / "spec").iterdir():
        text = path.read_text()
        assert "oracle" not in text and "nvxo_" not in text, path
    assert "oracle" not in HEADER.read_text() and "oracle" not in (ROOT / "navtex_amd" / "spec.py").read_text()
    assert C.sizeof(sp.Config) == 24 and C.sizeof(sp.Params) == 32 and C.sizeof(sp.Hit) == 32
    # the kernels the header names are the ones the kernel file holds
    kernels = sorted(set(re.findall(r"__global__[^\n]*void (nvx_spec_\w+)", (ROOT / "navtex_amd" / "spec" / "nvx_spec.hip").read_text())))
    assert kernels == ["nvx_spec_carry", "nvx_spec_fold", "nvx_spec_line"] and all(k in HEADER.read_text() for k in kernels)


def test_null_and_nonsense_arguments_are_errors_never_crashes(sp, tmp_path):
    src = ROOT / "tests" / "harness" / "null_args_spec.c"
    exe = tmp_path / "null_args_spec"
    lib = ROOT / "navtex_amd"
    subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib}", "-lnavtex_amd_spec",
                    f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "spec null-safety ok" in out.stdout, (out.stdout[-2500:], out.stderr[-500:])
    assert all(re.search(rf"\b{s}\(", src.read_text()) for s in SYMBOLS)


def test_create_returns_nodev_without_a_gpu_and_refuses_bad_parameters_first(nv, sp):
    for kw in (dict(n_log2=7), dict(n_log2=13), dict(format=4), dict(format=-1), dict(n_rows=0), dict(n_rows=65536), dict(avg=0), dict(avg=65),
               dict(n_log2=12, avg=33), dict(n_log2=8, avg=513)):
        with pytest.raises(nv.NvxError) as e:
            sp.Spectrum(**kw)
        assert e.value.code == nv._native.ERR_ARG, kw
    if nv.device_count() > 0:
        return                                                   # the rest is what a machine without a GPU answers
    cfg = sp.Config()
    sp.lib.nvx_spec_config_default(C.byref(cfg))
    assert (cfg.struct_size, cfg.device, cfg.format, cfg.n_rows, cfg.n_log2, cfg.avg) == (24, 0, 0, 1, 11, 8)
    h = C.c_void_p(1)
    assert sp.lib.nvx_spec_create(C.byref(cfg), C.byref(h)) == -2
    assert h.value is None and b"no CPU path" in sp.lib.nvx_spec_last_error()
    with pytest.raises(nv.NvxError) as e:
        sp.Spectrum(sp.CU8, n_rows=4, n_log2=12, avg=32)
    assert e.value.code == -2


def test_the_new_table_holds_the_band_scans_bits_at_its_even_entries():
    """C_4096[2 j] = C_2048[j] and S likewise, bit for bit, so every N <= 2048 reads the scan's numbers; the quarter points are
    exact, and every entry is libm's value to 1e-15: half an ulp of the entry plus what rounding the argument 2 pi j / 4096, up to
    2 pi, to a double moves the function by (7e-16)."""
    C4, S4 = sr.table()
    C2, S2 = scan_ref.table()
    assert C4.shape == (4096,) and np.array_equal(C4[::2].view(np.uint64), np.asarray(C2).view(np.uint64))
    assert np.array_equal(S4[::2].view(np.uint64), np.asarray(S2).view(np.uint64))
    assert (C4[0], S4[0], C4[1024], S4[1024], C4[2048], S4[3072]) == (1.0, 0.0, 0.0, 1.0, -1.0, -1.0) and C4[512] == S4[512]
    j = np.arange(4096)
    assert np.abs(C4 - np.cos(2 * np.pi * j / 4096)).max() < 1e-15 and np.abs(S4 - np.sin(2 * np.pi * j / 4096)).max() < 1e-15
    # the generator writes the committed header
    text = (ROOT / "tools" / "gen_spec_table.py").read_text()
    assert "gen_tune_table" in text and "nvx_spec_cs" in text


def test_the_launch_arithmetic_against_128_bit_integers_under_asan_ubsan(tmp_path):
    """nvx_spec_fill_args (navtex_amd/spec/nvx_spec_plan.h) without a device: positions up to 2^62, calls cut at and next to H, N,
    a line's hop and span and of 2^30 samples -- the lines a call completes against the header's definition, every sample of its
    first and last lines in the ring or in the input where its absolute index says, the ring words a call leaves
    (tests/harness/spec_launch_args.cpp).  A stand-alone program under ASan + UBSan."""
    exe = tmp_path / "spec_launch_args"
    pkg = ROOT / "navtex_amd"
    subprocess.run(["g++", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT / 'include'}", f"-I{pkg / 'csrc'}", f"-I{pkg / 'spec'}",
                    str(ROOT / "tests" / "harness" / "spec_launch_args.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env={"ASAN_OPTIONS": "detect_leaks=1", "PATH": "/usr/bin:/bin"})
    assert out.returncode == 0 and "spec launch args ok" in out.stdout, (out.stdout + out.stderr)[-3000:]


# ----------------------------------------------------------------------------------------------------------- restatement
def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a.get()[:3], b.get()[:3])) and a.lines == b.lines and a.position == b.position and \
        np.array_equal(a.carry, b.carry)


@pytest.mark.parametrize("n_log2,avg", [(8, 1), (8, 2), (8, 5), (9, 3), (12, 2)])
def test_one_shot_equals_cuts_at_and_next_to_h_n_a_hop_and_a_span(n_log2, avg):
    N, H = 1 << n_log2, 1 << (n_log2 - 1)
    hop, span = avg * H, (avg + 1) * H
    n = 29 * hop + span + 77
    row = sc.busy(n, 40 + n_log2 + avg)
    one, ref = sr.spectrum(row, sr.CS16, n_log2, avg)
    assert one.shape == (30, N) and ref.lines == 30 and len(ref.carry) == n - 30 * hop and one.any()
    rng = np.random.default_rng(n)
    for trial in range(3):
        cuts = [H - 1, 1, 0, N, hop + 1, H, H + 1, N - 1, N + 1, hop - 1, hop, span - 1, span + 1]
        rest = n - sum(cuts)
        assert rest >= 0
        while rest:
            cut = int(min(rest, rng.choice([0, 1, H, N, hop, span, int(rng.integers(1, 2 * span))])))
            cuts.append(cut); rest -= cut
        if trial:
            rng.shuffle(cuts)
        got, cut_ref = sr.spectrum(row, sr.CS16, n_log2, avg, cuts=cuts)
        assert np.array_equal(got, one), trial
        assert _same(ref, cut_ref)
    if avg == 1:
        assert not ref.sc_re.any() and not ref.sc_im.any() and ref.find_lines() == sr.ERR_ARG      # no lag products: the finder refuses


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_format_converts_as_the_notch_does(fmt):
    """A full-scale row in the format == the CS16 row of its conversion, word for word."""
    n = 2000
    row = sc.full_scale(fmt, n, 30 + fmt)
    a, ra = sr.spectrum(row, fmt, 8, 2)
    b, rb = sr.spectrum(np.asarray(rr.convert(row, fmt), dtype=np.int16), sr.CS16, 8, 2)
    assert a.shape[0] == 7 and np.array_equal(a, b) and _same(ra, rb)


@pytest.mark.parametrize("n_log2", [8, 12])
def test_a_tone_on_a_bin_centre_and_half_way_between_bins(n_log2):
    """On a bin the Hann window puts the tone in three bins, 6 dB down at the neighbours; half-way it is in two equal ones.  The
    lag product's phase gives its place to a hundredth of a bin either way, and the level word is the power to 0.26 dB.  The tone
    stands 40 dB over the noise in its bin (amplitude^2 N (2/3) / sigma^2 = 10^4): the window's skirt four bins away, 47 dB down
    half-way between bins, stays under the floor, so the one line is the one hit.  With that ratio rho and M = 9 * 3 lag products the coherence is
    1 - 1 / rho less a scatter of sqrt(2 / (rho M)) = 0.003: above 0.99 at three times the scatter."""
    N, H, avg = 1 << n_log2, 1 << (n_log2 - 1), 4
    n = 9 * avg * H + H
    noise = 1000.0
    amp = float(np.sqrt(1e4 * (2 * noise ** 2 / 3) * 1.5 / N))
    for bins in (37.0, -20.5, 0.25 - N / 2):
        lv, ref = sr.spectrum(sc.tone(n, n_log2, bins, amp=amp, noise=noise), sr.CS16, n_log2, avg)
        i = int(np.floor(bins + 0.5)) + N // 2
        assert ref.lines == 9 and int(np.argmax(ref.sp)) in (i, i - 1 if bins % 1 else i)
        hits = ref.find_lines()
        assert len(hits) == 1 and abs(hits[0]["cycles_per_sample"] * N - bins) < 0.01 and hits[0]["coherence"] > 0.99, (bins, hits)
        assert hits[0]["step"] == int(np.rint((hits[0]["cycles_per_sample"] % 1.0) * 2 ** 32)) & 0xffffffff
        db = sr.level_db(lv[3])
        if bins == 37.0:
            assert abs(db[i] - 10 * np.log10(avg * (amp * N / 2) ** 2)) < 0.35 and abs(db[i] - db[i + 1] - 6.02) < 0.7 and abs(db[i] - db[i - 1] - 6.02) < 0.7
            assert db[i + 40] < db[i] - 30
        if bins == -20.5:
            assert abs(db[i] - db[i - 1]) < 0.7


def test_zeros_give_level_zero_and_the_rails_the_level_the_bound_predicts():
    """Silence: every power is 0.0 and every level word 0.  Every component at -32768: bin 0 of a segment is -32768 N/2 (1 + j),
    its power 2 (2^15 N/2)^2, a line's A times that: the level word is that power's, index N/2 holds it, and it stays below the
    header's bound of (64 + 32) * 256."""
    for fmt in (sr.CS16, sr.CS8, sr.CF32):
        lv, ref = sr.spectrum(sc.zeros(fmt, 3000), fmt, 8, 3)
        assert lv.shape == (7, 256) and not lv.any() and not ref.sp.any() and not ref.sc_re.any() and ref.lines == 7
    for n_log2, avg in ((8, 1), (8, 512), (12, 4)):
        N, H = 1 << n_log2, 1 << (n_log2 - 1)
        lv, ref = sr.spectrum(sc.rails(sr.CS16, (avg + 1) * H), sr.CS16, n_log2, avg)
        want = avg * 2.0 * (32768.0 * N / 2) ** 2
        assert lv.shape == (1, N) and abs(int(lv[0, H]) - int(sr.level_words(np.array([want]))[0])) <= 1 and lv.max() == lv[0, H] <= 96 * 256
        assert abs(sr.level_db(lv[0, H]) - 10 * np.log10(want)) < 0.2591 + 2 * 0.0118
        assert lv[0, 5] < lv[0, H] - 100 * 256 / 3.0103                   # a hundred dB down, away from the line
    for fmt in FORMATS:                                                   # bounds only
        sr.spectrum(sc.rails(fmt, 3000), fmt, 8, 2)
        sr.spectrum(sc.full_scale(fmt, 3000, 5), fmt, 8, 2)


def test_the_level_word_is_monotone_and_within_a_quarter_db():
    """Never above the true logarithm, and below it by at most the chord's sag of log2, 0.0861 octaves = 0.2591 dB, plus the
    truncation to eight mantissa bits, 1/256 octave = 0.0118 dB."""
    p = np.concatenate([[0.0, 1e-300, 2.0 ** -33, 2.0 ** -32], np.sort(np.random.default_rng(3).uniform(0, 62, 20000)) ** 1.0])
    p[4:] = 2.0 ** p[4:]
    lv = sr.level_words(p).astype(np.int64)
    assert list(lv[:4]) == [0, 0, 0, 0] and (np.diff(lv[3:]) >= 0).all() and lv[-1] < 96 * 256
    err = sr.level_db(lv[4:]) - 10 * np.log10(p[4:])
    assert err.max() <= 1e-9 and err.min() > -(0.2591 + 0.0118), (err.min(), err.max())


def test_measure_in_mid_stream_equals_a_fresh_survey_from_that_line_on():
    n_log2, avg = 8, 3
    H = 128
    hop = avg * H
    row = sc.busy(20 * hop, 9)
    for at in (5 * hop, 5 * hop + 1, 7 * hop - 1, 6 * hop + H):
        ref = sr.Spectrum(sr.CS16, n_log2, avg)
        a = ref.push(row[:at])
        before = ref.get()
        ref.measure()
        assert ref.lines == 0 and not ref.sp.any() and before[3] == sr.lines_at(at, n_log2, avg)
        b = ref.push(row[at:])
        one, whole = sr.spectrum(row, sr.CS16, n_log2, avg)
        assert np.array_equal(np.concatenate([a, b]), one)               # the lines go on as they were
        first = -(-at // hop)                                             # the first line that begins at or behind the restart
        fresh = sr.Spectrum(sr.CS16, n_log2, avg)
        fresh.push(row[first * hop:])
        assert ref.lines == fresh.lines == whole.lines - first and all(np.array_equal(x, y) for x, y in zip(ref.get()[:3], fresh.get()[:3]))


@pytest.mark.parametrize("position", [2 ** 32 - 1000, 2 ** 40 + 5])
def test_positions_beyond_32_bits(position):
    """From a position the samples in front of it are silence and the lines lie where the absolute index puts them: the row
    behind `position` == the same row behind as many zeros as the position is past a line's first sample, from zero."""
    n_log2, avg = 8, 2
    hop = avg * 128
    row = sc.busy(3000, 3)
    got, ref = sr.spectrum(row, sr.CS16, n_log2, avg, position=position)
    cut, cut_ref = sr.spectrum(row, sr.CS16, n_log2, avg, cuts=[999, 1, 1280, 720], position=position)
    lead = position - sr.lines_at(position, n_log2, avg) * hop
    want, low = sr.spectrum(np.concatenate([np.zeros((lead, 2), dtype=np.int16), row]), sr.CS16, n_log2, avg)
    assert np.array_equal(got, want) and np.array_equal(got, cut) and _same(ref, cut_ref) and ref.position == position + 3000
    skipped = -(-lead // hop)                                             # lines that begin in front of the position do not count
    assert ref.lines == low.lines - skipped and got.shape[0] == low.lines


# ---------------------------------------------------------------------------------------------------------------- finder
def test_noise_alone_gives_no_hit_and_a_coherence_near_a_sixth():
    n_log2, avg = 10, 8
    rng = np.random.default_rng(8)
    n = 40 * avg * 512 + 512
    row = np.stack([rng.uniform(-1500, 1500, n), rng.uniform(-1500, 1500, n)], axis=1).astype(np.int16)
    _, ref = sr.spectrum(row, sr.CS16, n_log2, avg)
    g = sr.coherence(ref.sp, ref.sc_re, ref.sc_im, avg)
    print("noise of +-1500, 40 lines of 8: coherence mean", round(float(g.mean()), 3), "max", round(float(g.max()), 3))
    assert ref.lines == 40 and ref.find_lines() == [] and ref.find_lines(min_score_db=0.0) == []
    assert 0.1 < g.mean() < 0.25 and g.max() < 0.5
    assert ref.find_lines(min_lines=41) == sr.ERR_ARG


def test_the_c_finder_agrees_with_the_restatement(sp):
    n_log2, avg = 9, 4
    n = 30 * avg * 256 + 256
    row = sc.busy(n, 17)
    _, ref = sr.spectrum(row, sr.CS16, n_log2, avg)
    want = ref.find_lines()
    got = sp.find_lines(ref.sp, ref.sc_re, ref.sc_im, n_log2, avg, ref.lines)
    assert len(want) == 3 and [h["bin"] for h in got] == [h["bin"] for h in want]
    for g, w in zip(got, want):
        assert abs(g["cycles_per_sample"] - w["cycles_per_sample"]) < 1e-12 and abs(g["step"] - w["step"]) <= 1
        assert abs(g["coherence"] - w["coherence"]) < 1e-12 and abs(g["score_db"] - w["score_db"]) < 1e-9
    assert len(sp.find_lines(ref.sp, ref.sc_re, ref.sc_im, n_log2, avg, ref.lines, cap=1)) == 1
    loose = dict(min_coherence=0.0, min_score_db=3.0, guard_bins=0)
    assert [h["bin"] for h in sp.find_lines(ref.sp, ref.sc_re, ref.sc_im, n_log2, avg, ref.lines, cap=512, **loose)] == [h["bin"] for h in ref.find_lines(**loose)]
    for bad in (dict(avg=1), dict(lines=7)):
        with pytest.raises(sp.SpecError):
            sp.find_lines(ref.sp, ref.sc_re, ref.sc_im, n_log2, **dict(dict(avg=avg, lines=ref.lines), **bad))


@pytest.fixture(scope="module")
def acceptance(nv, oracle):
    """The twelve seeds, once: the finder's hits on the whole row at N = 4096, A = 8, and what arrives from the plain row and
    from the row notched at the finder's two steps, R = 32, without refine."""
    want = sc.nc.text()
    got = {"plain": 0, "notched": 0, "hits": [], "errors": [], "coherence": []}
    for seed in sc.SEEDS:
        a = sc.acceptance_row(nv, seed)
        _, ref = sr.spectrum(a, sr.CS16, 12, 8)
        hits = ref.find_lines()
        got["hits"].append(len(hits))
        truth = [hz for hz, _ in sc.CARRIERS]
        got["errors"].append([min(abs(hz - t) for hz in sc.hits_hz(hits)) if hits else np.inf for t in truth])
        got["coherence"].append([round(h["coherence"], 4) for h in hits])
        got["plain"] += sc.nc.delivered(oracle, a, nv.FRAME_IN)[0] == [want]
        if len(hits) == 2:
            notch = nr.Notch(nr.CS16, 2, 5)
            for k, h in enumerate(hits):
                notch.set_freq(k, h["step"]); notch.enable(k)
            y = np.concatenate([notch.push(a[at:at + (1 << 20)]) for at in range(0, len(a), 1 << 20)])
            got["notched"] += sc.nc.delivered(oracle, y, nv.FRAME_IN)[0] == [want]
    print("hits per seed", got["hits"], "worst error in Hz", np.max(got["errors"]), "least coherence", min(min(c) for c in got["coherence"] if c))
    print("490 delivered: plain", got["plain"], "notched at the finder's steps (R = 32, no refine)", got["notched"], "of 12")
    return got


def test_the_acceptance_case_finds_exactly_the_two_carriers_within_a_hertz(acceptance):
    """A 490 station at amplitude 300, noise +-1500, carriers of 3000 and 6000 at +60 and -310 Hz from the chain's centre; the
    finder is not told where.  Measured: two hits on every seed, errors at most 0.04 Hz, coherence at least 0.997."""
    assert acceptance["hits"] == [2] * 12
    assert np.max(acceptance["errors"]) <= 1.0


def test_the_acceptance_case_delivers_from_the_row_notched_at_the_finders_steps_only(acceptance):
    """The two steps set on the notch's restatement at R = 32 without refine deliver the message 12 of 12; the plain rows at
    most 1 of 12 (the notch's recorded figure)."""
    assert acceptance["notched"] == 12
    assert acceptance["plain"] <= 1
