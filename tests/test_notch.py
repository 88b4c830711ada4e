"""The tone notch (include/navtex_amd_notch.h) on the CPU: the header and the companion library's exports and argument
safety, the launch arithmetic against 128-bit integers (a stand-alone program under ASan + UBSan), the restatement
(tests/notch_ref.py) on cuts at and next to the block and tile ends, with no notch enabled, through set_freq in mid-stream, at
positions beyond 2^32 and at the rails, and the signal measurements: the suppression table, white noise, the acceptance case (a
weak 490 station with two carriers inside its chain's passband, twelve seeds) through the oracle, and the refine path."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import notch_cases as nc
import notch_ref as nr
import resample_ref as rr

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "navtex_amd_notch.h"
PLAN = ROOT / "navtex_amd" / "notch" / "nvx_notch_plan.h"
SYMBOLS = ["nvx_notch_config_default", "nvx_notch_create", "nvx_notch_delay", "nvx_notch_destroy", "nvx_notch_enable", "nvx_notch_get",
           "nvx_notch_hz_from_step", "nvx_notch_last_error", "nvx_notch_measure", "nvx_notch_plan", "nvx_notch_position", "nvx_notch_push",
           "nvx_notch_refine", "nvx_notch_reset", "nvx_notch_resident", "nvx_notch_set_freq", "nvx_notch_step_from_hz", "nvx_notch_time_stats",
           "nvx_notch_timing"]
HOOKS = ["nvx_notch_debug_last_launch", "nvx_notch_debug_set_position"]
B = nr.BLOCK
FORMATS = (nr.CS16, nr.CU8, nr.CS8, nr.CF32)


@pytest.fixture(scope="module")
def nt(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_notch.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.notch
    return navtex_amd.notch


# ------------------------------------------------------------------------------------------------------------ interface
def test_header_compiles_as_plain_c_and_declares_the_entry_points(tmp_path):
    text = HEADER.read_text()
    assert sorted(set(re.findall(r"NVX_API\s+[\w\s\*]+?\b(\w+)\s*\(", text))) == SYMBOLS
    for name, want in (("NVX_NOTCH_BLOCK", "256"), ("NVX_NOTCH_MAX_NOTCHES", "4"), ("NVX_NOTCH_WIDTH_LOG2_MIN", "2"), ("NVX_NOTCH_WIDTH_LOG2_MAX", "6"),
                       ("NVX_NOTCH_WIDTH_LOG2_DEFAULT", "5"), ("NVX_NOTCH_MAX_PAIRS", "4096")):
        assert re.search(rf"#define {name}\s+{re.escape(want)}\b", text), name
    assert "Known limit" in text and "IQ-correct -> cancel -> blank -> notch -> DDC / resample -> scan -> tune -> decode" in text
    src = tmp_path / "t.c"
    src.write_text('#include "navtex_amd_notch.h"\nint main(void){ nvx_notch_config c; nvx_notch_status s; c.format = NVX_NOTCH_CF32; s.pairs = 0; '
                   'return NVX_NOTCH_CS16 == 0 && NVX_NOTCH_CU8 == 1 && NVX_NOTCH_CS8 == 2 && c.format == 3 && sizeof c == 24 && sizeof s == 40 && !s.pairs ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


@pytest.mark.parametrize("sym", SYMBOLS + HOOKS)
def test_symbol_is_exported(nt, sym):
    assert hasattr(nt.lib, sym), f"{sym} is declared but not exported"


def test_the_companion_links_no_other_library_of_the_project_and_no_test_infrastructure(nt):
    lib = ROOT / "navtex_amd" / "libnavtex_amd_notch.so"
    out = subprocess.run(["ldd", str(lib)], capture_output=True, text=True).stdout
    assert "libnavtex_amd" not in out and "oracle" not in out and "libamdhip64" in out
    # it defines nothing but its own interface and the tests' two hooks, and needs no nvx_ symbol from elsewhere
    nm = subprocess.run(["nm", "-D", str(lib)], capture_output=True, text=True, check=True).stdout
    defined = sorted(l.split()[-1] for l in nm.splitlines() if " T " in l and "nvx_" in l)
    assert defined == sorted(SYMBOLS + HOOKS) and all(d.startswith("nvx_notch_") for d in defined)
    assert not [h for h in HOOKS if h in HEADER.read_text()] and all(h in PLAN.read_text() for h in HOOKS)
    assert nt.lib.nvx_notch_debug_last_launch(None, None, None, None, None) < 0 and nt.lib.nvx_notch_debug_set_position(None, 0, 0) < 0
    assert not [l for l in nm.splitlines() if " U " in l and "nvx" in l]
    for path in (ROOT / "navtex_amd" / "notch").iterdir():
        text = path.read_text()
        assert "oracle" not in text and "nvxo_" not in text, path
    assert "oracle" not in HEADER.read_text() and "oracle" not in (ROOT / "navtex_amd" / "notch.py").read_text()
    assert C.sizeof(nt.Config) == 24 and C.sizeof(nt.Status) == 40
    # the table is the bank's, read from its header and not copied
    host = (ROOT / "navtex_amd" / "notch" / "nvx_notch_host.cpp").read_text()
    assert '#include "nvx_ddc_table.h"' in host and "nvx_ddc_w(" in host


def test_null_and_nonsense_arguments_are_errors_never_crashes(nt, tmp_path):
    src = ROOT / "tests" / "harness" / "null_args_notch.c"
    exe = tmp_path / "null_args_notch"
    lib = ROOT / "navtex_amd"
    subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib}", "-lnavtex_amd_notch",
                    f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "notch null-safety ok" in out.stdout, (out.stdout[-2500:], out.stderr[-500:])
    assert all(re.search(rf"\b{s}\(", src.read_text()) for s in SYMBOLS)


def test_create_returns_nodev_without_a_gpu_and_refuses_bad_parameters_first(nv, nt):
    for kw in (dict(width_log2=1), dict(width_log2=7), dict(format=4), dict(format=-1), dict(n_rows=0), dict(n_rows=65536), dict(n_notches=0),
               dict(n_notches=5)):
        with pytest.raises(nv.NvxError) as e:
            nt.Notch(**kw)
        assert e.value.code == nv._native.ERR_ARG, kw
    # the helpers need no device, and agree with the restatement's
    for hz in (0.0, 1000.0, -14310.0, 125999.0, -126000.0, 0.03):
        assert nt.step_from_hz(hz, 252000.0) == nr.step_from_hz(hz, 252000.0), hz
        assert abs(nt.hz_from_step(nt.step_from_hz(hz, 252000.0), 252000.0) - nr.hz_from_step(nr.step_from_hz(hz, 252000.0), 252000.0)) < 1e-9
    if nv.device_count() > 0:
        return                                                   # the rest is what a machine without a GPU answers
    cfg = nt.Config()
    nt.lib.nvx_notch_config_default(C.byref(cfg))
    assert (cfg.struct_size, cfg.device, cfg.format, cfg.n_rows, cfg.n_notches, cfg.width_log2) == (24, 0, 0, 1, 1, 5)
    h = C.c_void_p(1)
    assert nt.lib.nvx_notch_create(C.byref(cfg), C.byref(h)) == -2
    assert h.value is None and b"no CPU path" in nt.lib.nvx_notch_last_error()
    with pytest.raises(nv.NvxError) as e:
        nt.Notch(nt.CU8, n_rows=4, n_notches=2)
    assert e.value.code == -2


def test_the_launch_arithmetic_against_128_bit_integers_under_asan_ubsan(tmp_path):
    """nvx_notch_fill_args (navtex_amd/notch/nvx_notch_plan.h) without a device: positions up to 2^62, call lengths around half
    a block, a block, the delay, a tile and a chunk, every width and chunking -- each word in one tile of one chunk, its block's
    record, its two values of M among its tile's 18 and their block sums among the carried ones and the records, the NCOs'
    first samples, the layout of a row's state, 16-byte stores only on aligned rows (tests/harness/notch_launch_args.cpp).  A
    stand-alone program under ASan + UBSan."""
    exe = tmp_path / "notch_launch_args"
    pkg = ROOT / "navtex_amd"
    subprocess.run(["g++", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT / 'include'}", f"-I{pkg / 'csrc'}", f"-I{pkg / 'notch'}",
                    str(ROOT / "tests" / "harness" / "notch_launch_args.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env={"ASAN_OPTIONS": "detect_leaks=1", "PATH": "/usr/bin:/bin"})
    assert out.returncode == 0 and "notch launch args ok" in out.stdout, (out.stdout + out.stderr)[-3000:]


# ----------------------------------------------------------------------------------------------------------- restatement
def _state(ref):
    return [ref.get(k) for k in range(len(ref.tones))] + [ref.position]


def _fed(row, steps, cuts, fmt=nr.CS16, width_log2=2, position=0, disabled=()):
    ref = nr.Notch(fmt, len(steps), width_log2, position)
    for k, step in enumerate(steps):
        ref.set_freq(k, step); ref.enable(k, k not in disabled)
    pos, parts = 0, []
    for cut in cuts:
        parts.append(ref.push(row[pos:pos + cut])); pos += cut
    assert pos == len(row)
    return np.concatenate(parts), ref


@pytest.mark.parametrize("width_log2,n", [(2, 30000), (4, 41000)])
def test_one_shot_equals_cuts_at_and_next_to_the_block_and_tile_ends(width_log2, n):
    row, steps = nc.busy_row(n, 3 + width_log2)
    one, ref = _fed(row, steps, [n], width_log2=width_log2, disabled=(3,))
    D = ref.delay()
    assert not one[:D].any() and one[D:].any() and ref.get(0)["pairs"] == n // B - 2 * (1 << width_log2) + 1
    rng = np.random.default_rng(n)
    for trial in range(3):
        cuts = [0, 1, 127, 128, B - 1, B, B + 1, 4095, 4096, 4097, D - 1, 1, D]
        rest = n - sum(cuts)
        while rest:
            cut = int(min(rest, rng.choice([0, 1, B - 1, B, B + 1, int(rng.integers(1, 3000))])))
            cuts.append(cut); rest -= cut
        if trial:
            rng.shuffle(cuts)
        got, cut_ref = _fed(row, steps, cuts, width_log2=width_log2, disabled=(3,))
        assert np.array_equal(got, one), trial
        assert _state(cut_ref) == _state(ref)


@pytest.mark.parametrize("fmt", FORMATS)
def test_with_no_notch_enabled_the_output_is_the_conversion_delayed(fmt):
    """Steps set and sums running, nothing enabled: the conversion delayed by D, word for word, and zeros in front."""
    n = 9000
    row = nc.full_scale(fmt, n, 20 + fmt)
    out, ref = _fed(row, [0x12345678, 77], [4000, 5000], fmt=fmt, disabled=(0, 1))
    D = ref.delay()
    assert D == 1280 and not out[:D].any() and np.array_equal(out[D:], rr.convert(row, fmt)[:n - D].astype(np.int16))
    assert np.array_equal(nr.pack(out).view(np.int16).reshape(-1, 2), out) and ref.get(1)["pairs"] == n // B - 7
    for r in range(2, 7):
        assert nr.Notch(fmt, 1, r).delay() == ((1 << r) + 1) * 256


def test_set_freq_in_mid_stream_restarts_the_notch_and_ramps_in():
    """The pending D words are computed with the new step from sums that start at zero: the call behind a set_freq equals a
    notch that was reset there, on the same delay line; 2R blocks on the amplitude is whole."""
    n = 30000
    row = nc.tone(n, 1000.0)
    step = nr.step_from_hz(1000.0, nc.RATE)
    ref = nr.Notch(nr.CS16, 1, 2)
    ref.set_freq(0, nr.step_from_hz(5000.0, nc.RATE)); ref.enable(0)
    first = ref.push(row[:10001])
    assert nc.power_db(first[1280 + 2048:], row[2048:10001 - 1280]) > -0.1           # a notch 4 kHz away leaves the tone
    ref.set_freq(0, step)
    assert ref.get(0)["pairs"] == 0 and ref.get(0)["x"] == (0, 0)
    rest = ref.push(row[10001:])
    # the same samples through a notch whose sums start at 10001, the delay line aside: a fresh row at that position
    other = nr.Notch(nr.CS16, 1, 2, position=10001)
    other.set_freq(0, step); other.enable(0)
    other.line, other.start = ref.line * 0 + rr.convert(row[10001 - 1280:10001], nr.CS16), 0
    assert np.array_equal(rest, other.push(row[10001:])) and ref.get(0) == dict(other.get(0), samples=n)
    D, ramp = 1280, 2 * 4 * B
    assert nc.power_db(rest[:D], row[:D]) > -3.0                                     # at the restart the notch takes nothing yet
    assert nc.power_db(rest[D + ramp:], row[:len(rest) - D - ramp]) < -60.0          # 2R blocks on it takes all of it


@pytest.mark.parametrize("position", [2 ** 32 - 1000, 2 ** 40 + 5])
def test_positions_beyond_32_bits(position):
    """From a position the words in front of it are zero, the block it lies in sums what it received, and the phase is that of
    the absolute index: a tone generated with the phase it has at that index is notched as deep as from zero."""
    n = 20000
    phase = (position * (1000.0 / nc.RATE)) % 1.0
    row = nc._quantise(nc.carrier(n, 1000.0, 8000.0, phase=phase))
    step = nr.step_from_hz(1000.0, nc.RATE)
    one, ref = _fed(row, [step], [n], position=position)
    cut, cut_ref = _fed(row, [step], [999, 1, 1280, n - 2280], position=position)
    assert np.array_equal(one, cut) and _state(ref) == _state(cut_ref) and ref.position == position + n
    assert not one[:1280].any() and nc.power_db(one[1280 + 2048 + 256:], row[:n - 3584]) < -60.0
    assert ref.get(0)["pairs"] == (position + n) // B - -(-position // B) - 2 * 4 + 1


def test_the_rails_stay_within_every_asserted_bound():
    """All-rails DC notched at 0 Hz: B = 256 * 2^30 (re) per block, M = R^2 of it, the amplitude 2^20 less a table's worth, and
    what is left is (-2, -2).  Every width; the bounds are asserted inside the restatement."""
    for r in range(2, 7):
        R = 1 << r
        n = (3 * R + 3) * B + 77
        row = nc.rails(nr.CS16, n)
        out, ref = nr.notch(row, [0], width_log2=r)
        D = ref.delay()
        assert np.array_equal(out[D + 2 * R * B:], np.full((n - D - 2 * R * B, 2), -2, dtype=np.int16)), r
        assert ref.get(0)["pairs"] == n // B - 2 * R + 1
    # the rails turning at a quarter of the rate and at an odd step, all formats: bounds only
    for fmt in FORMATS:
        nr.notch(nc.rails(fmt, 6000), [0x40000000, 0xdeadbeef], fmt, 2)
        nr.notch(nc.full_scale(fmt, 6000, 9), [0x40000000, 0xdeadbeef], fmt, 2)


# ------------------------------------------------------------------------------------------------------- signal measurements
def test_the_suppression_table():
    """A pure tone of amplitude 8000 at 1000 Hz of 252 kS/s, the notch 0, 1, 2, 5 and 10 Hz above it, and 85 Hz above it (a
    station's other tone beside a notched one): the tone's attenuation behind the ramp.  Measured:
        R   0 Hz   1 Hz   2 Hz   5 Hz   10 Hz  85 Hz
        8  -67.0  -65.5  -59.7  -45.1  -33.2   -1.3
       16  -67.0  -59.7  -49.0  -33.3  -21.5   -0.4
       32  -67.0  -49.0  -37.1  -21.5  -10.4   -0.1
       64  -67.0  -37.1  -25.3  -10.4   -1.8    0.0"""
    table = {}
    for r in (3, 4, 5, 6):
        R = 1 << r
        D, ramp = (R + 1) * B, 2 * R * B
        n = D + ramp + 60000
        x = nc.tone(n, 1000.0)
        table[R] = []
        for off in (0.0, 1.0, 2.0, 5.0, 10.0, 85.0):
            y, _ = nr.notch(x, [nr.step_from_hz(1000.0 + off, nc.RATE)], width_log2=r)
            table[R].append(round(float(nc.power_db(y[D + ramp:], x[ramp:n - D])), 1))
        print("R", R, "attenuation in dB at 0 / 1 / 2 / 5 / 10 Hz off and 85 Hz beside:", table[R])
    assert table[16][0] <= -60.0 and table[16][3] <= -30.0
    assert all(table[R][0] <= -60.0 for R in table) and all(table[R][5] >= -2.0 for R in table)


def test_white_noise_passes_unchanged_in_power():
    n = 200000
    x = nc.white(n)
    for r in (4, 5):
        y, ref = nr.notch(x, [nr.step_from_hz(1000.0, nc.RATE)], width_log2=r)
        D = ref.delay()
        change = nc.power_db(y[D:], x[:n - D])
        print("R", 1 << r, "white noise of +-6000: power changed by", round(change, 4), "dB")
        assert abs(change) <= 0.01


def _notched(row, steps, width_log2):
    """The row through the restatement in calls of 2^20 samples."""
    ref = nr.Notch(nr.CS16, len(steps), width_log2)
    for k, step in enumerate(steps):
        ref.set_freq(k, step); ref.enable(k)
    return np.concatenate([ref.push(row[at:at + (1 << 20)]) for at in range(0, len(row), 1 << 20)]), ref


@pytest.fixture(scope="module")
def acceptance(nv, oracle):
    """The twelve seeds, once: what arrives from the plain row and from the row notched 1 Hz off at R = 32."""
    want = nc.text()
    got = {"plain": 0, "notched": 0}
    for seed in nc.SEEDS:
        a = nc.acceptance_row(nv, seed)
        y, _ = _notched(a, nc.steps(1.0), 5)
        got["plain"] += nc.delivered(oracle, a, nv.FRAME_IN)[0] == [want]
        # the notched row lags by D = 8448 samples, which the oracle takes as it takes any late start
        got["notched"] += nc.delivered(oracle, y, nv.FRAME_IN)[0] == [want]
    print("490 delivered: plain", got["plain"], "notched (1 Hz off, R = 32)", got["notched"], "of 12")
    return got


def test_the_acceptance_case_delivers_from_the_notched_row_only(acceptance):
    """490 at -14 kHz, amplitude 300, noise +-1500; a carrier of 3000 60 Hz above the chain's centre and one of 6000 310 Hz
    below it; two notches 1 Hz off at R = 32.  Measured: plain 0, notched 12 of 12."""
    assert acceptance["notched"] == 12
    assert acceptance["plain"] <= 1


def test_the_refine_path_lands_within_a_quarter_hertz(nv):
    """The notches 5 Hz off (what the scan gives), one second of the acceptance row, refine, the rest: the applied frequencies
    lie within 0.25 Hz of the true ones.  Measured 0.03 Hz."""
    a = nc.acceptance_row(nv, 11)[:4 * nc.RATE]
    for off in (5.0, -3.0, 1.0):
        ref = nr.Notch(nr.CS16, 2, 5)
        for k, step in enumerate(nc.steps(off)):
            ref.set_freq(k, step); ref.enable(k)
        ref.push(a[:nc.RATE])
        read = [ref.offset_hz(k, nc.RATE) for k in range(2)]
        errors = [nr.hz_from_step(ref.refine(k), nc.RATE) - hz for k, (hz, _) in enumerate(nc.CARRIERS)]
        print("set", off, "Hz off: the readout says", [round(-v, 2) for v in read], "Hz; after refine the notches are off by", [round(e, 3) for e in errors], "Hz")
        assert all(abs(e) <= 0.25 for e in errors), errors
        assert all(ref.get(k)["pairs"] == 0 for k in range(2))
        ref.push(a[nc.RATE:])                                    # the rest of the row: the bounds hold through the restart
