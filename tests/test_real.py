"""The real-input converter (include/navtex_amd_real.h) on the CPU: the header and the companion library's exports and
argument safety, the taps with their three properties and the response computed from them, the launch arithmetic against
128-bit integers (a stand-alone program under ASan + UBSan), the restatement (tests/real_ref.py) against Python integers, on
cuts anywhere including odd ones, in four formats, inverted and at the rails, tones on FFT bins, and end to end through the
oracle: the acceptance case (a weak 490 station 28 kHz below a strong 518 one in a real 504 kS/s row, twelve seeds)."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import real_cases as rc
import real_ref as rf

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "navtex_amd_real.h"
PLAN = ROOT / "navtex_amd" / "real" / "nvx_real_plan.h"
SYMBOLS = ["nvx_real_config_default", "nvx_real_create", "nvx_real_destroy", "nvx_real_last_error", "nvx_real_plan", "nvx_real_position",
           "nvx_real_push", "nvx_real_reset", "nvx_real_resident", "nvx_real_taps", "nvx_real_time_stats", "nvx_real_timing"]
HOOKS = ["nvx_real_debug_last_launch", "nvx_real_debug_set_position"]
TAPS = (10376, 3314, 1825, 1144, 745, 486, 310, 191, 111, 60, 30, 13, 4, 1)
FORMATS = (rf.S16, rf.U8, rf.S8, rf.F32)
T = 4096


@pytest.fixture(scope="module")
def rl(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_real.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.real
    return navtex_amd.real


# ------------------------------------------------------------------------------------------------------------ interface
def test_header_compiles_as_plain_c_and_declares_the_entry_points(tmp_path):
    text = HEADER.read_text()
    assert sorted(set(re.findall(r"NVX_API\s+[\w\s\*]+?\b(\w+)\s*\(", text))) == SYMBOLS
    assert ", ".join(str(t) for t in TAPS) in text and "K = 13, S = 14" in text
    assert "real -> (blank) -> DDC / resample -> scan -> tune -> decode" in text and "192 kS/s" in text and "6.4 MS/s" in text
    src = tmp_path / "t.c"
    src.write_text('#include "navtex_amd_real.h"\nint main(void){ nvx_real_config c; c.format = NVX_REAL_F32; c.invert = 1; '
                   'return NVX_REAL_S16 == 0 && NVX_REAL_U8 == 1 && NVX_REAL_S8 == 2 && c.format == 3 && c.invert && sizeof c == 20 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


@pytest.mark.parametrize("sym", SYMBOLS + HOOKS)
def test_symbol_is_exported(rl, sym):
    assert hasattr(rl.lib, sym), f"{sym} is declared but not exported"


def test_the_companion_links_no_other_library_of_the_project_and_no_test_infrastructure(rl):
    lib = ROOT / "navtex_amd" / "libnavtex_amd_real.so"
    out = subprocess.run(["ldd", str(lib)], capture_output=True, text=True).stdout
    assert "libnavtex_amd" not in out and "oracle" not in out and "libamdhip64" in out
    # it defines nothing but its own interface and the tests' two hooks, and needs no nvx_ symbol from elsewhere
    nm = subprocess.run(["nm", "-D", str(lib)], capture_output=True, text=True, check=True).stdout
    defined = sorted(l.split()[-1] for l in nm.splitlines() if " T " in l and "nvx_" in l)
    assert defined == sorted(SYMBOLS + HOOKS) and all(d.startswith("nvx_real_") for d in defined)
    assert not [h for h in HOOKS if h in HEADER.read_text()] and all(h in PLAN.read_text() for h in HOOKS)
    assert rl.lib.nvx_real_debug_last_launch(None, None, None, None) < 0 and rl.lib.nvx_real_debug_set_position(None, 0, 0) < 0
    assert not [l for l in nm.splitlines() if " U " in l and "nvx" in l]
    for path in (ROOT / "navtex_amd" / "real").iterdir():
        text = path.read_text()
        assert "oracle" not in text and "nvxo_" not in text, path
    assert "oracle" not in HEADER.read_text() and "oracle" not in (ROOT / "navtex_amd" / "real.py").read_text()
    assert C.sizeof(rl.Config) == 20


def test_null_nonsense_and_odd_arguments_are_errors_never_crashes(rl, tmp_path):
    src = ROOT / "tests" / "harness" / "null_args_real.c"
    exe = tmp_path / "null_args_real"
    lib = ROOT / "navtex_amd"
    subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib}", "-lnavtex_amd_real",
                    f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "real null-safety ok" in out.stdout, (out.stdout[-2500:], out.stderr[-500:])
    assert all(re.search(rf"\b{s}\(", src.read_text()) for s in SYMBOLS)


def test_create_returns_nodev_without_a_gpu_and_refuses_bad_parameters_first(nv, rl):
    if nv.device_count() > 0:
        pytest.skip("a GPU is present")
    cfg = rl.Config()
    rl.lib.nvx_real_config_default(C.byref(cfg))
    h = C.c_void_p(1)
    assert rl.lib.nvx_real_create(C.byref(cfg), C.byref(h)) == -2
    assert h.value is None and b"no CPU path" in rl.lib.nvx_real_last_error()
    with pytest.raises(nv.NvxError) as e:
        rl.Converter(rl.U8, n_streams=4)
    assert e.value.code == -2
    for kw in (dict(invert=2), dict(invert=-1), dict(format=4), dict(format=-1), dict(n_streams=0), dict(n_streams=65536)):
        with pytest.raises(nv.NvxError) as e:
            rl.Converter(**kw)
        assert e.value.code == nv._native.ERR_ARG, kw


# ----------------------------------------------------------------------------------------------------------------- taps
def test_the_taps_are_the_contracts_and_the_three_properties_hold(nv, rl):
    assert rl.taps() == (TAPS, 13, 14) and rf.TAPS == TAPS and (rf.K, rf.S) == (13, 14) and (rl.K, rl.S, rl.HISTORY) == (13, 14, 28)
    assert rl.lib.nvx_real_taps((C.c_int16 * 13)(), 13, None, None) == nv._native.ERR_ARG and rl.lib.nvx_real_taps(None, 0, None, None) == 14
    assert sum(a if j % 2 == 0 else -a for j, a in enumerate(TAPS)) == 1 << 13
    assert 2 * sum(TAPS) == 37220 <= 65535 and sum(TAPS) * 65535 == rf.ACC_MAX < 1 << 31
    # a real tone of amplitude a comes out as a complex tone of amplitude a: G(0) = 1, and the wanted sideband is (1 + G) / 2
    assert rf.gain([0.0])[0] == 1.0
    out = subprocess.run([sys.executable, str(ROOT / "tools" / "real_taps.py")], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.splitlines()[0] == ", ".join(str(t) for t in TAPS), out.stdout + out.stderr


def test_the_response_computed_from_the_taps():
    """Within +-0.01 dB for |f| <= 0.2 fr, at most -76 dB for |f| >= 0.3 fr (computed: 0.001 dB and -79.0 dB)."""
    inner = np.linspace(-0.2, 0.2, 8001)
    outer = np.concatenate([np.linspace(0.3, 0.5, 4001), np.linspace(-0.5, -0.3, 4001)])
    pass_db = 20 * np.log10(np.abs(1 + rf.gain(inner)) / 2)
    stop_db = 20 * np.log10(np.maximum(np.abs(1 + rf.gain(outer)) / 2, 1e-12))
    print("pass band within", float(np.abs(pass_db).max()), "dB; stop band at most", float(stop_db.max()), "dB")
    assert np.abs(pass_db).max() <= 0.01
    assert stop_db.max() <= -76.0
    # what folds onto +f is what lay at 1/2 - f: G(1/2 - f) = -G(f)
    assert np.allclose(rf.gain(0.5 - inner), -rf.gain(inner), atol=1e-12)


def test_the_launch_arithmetic_against_128_bit_integers_under_asan_ubsan(tmp_path):
    """nvx_real_fill_args (navtex_amd/real/nvx_real_plan.h) without a device: positions up to 2^62, call lengths around the
    history, a tile and a chunk, every chunking -- each output in one group of one tile of one chunk, halos inside the input,
    the LDS image's bounds, the sign, the state's writer, 16-byte stores only on aligned rows
    (tests/harness/real_launch_args.cpp).  A stand-alone program under ASan + UBSan."""
    exe = tmp_path / "real_launch_args"
    pkg = ROOT / "navtex_amd"
    subprocess.run(["g++", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT / 'include'}", f"-I{pkg / 'csrc'}", f"-I{pkg / 'real'}",
                    str(ROOT / "tests" / "harness" / "real_launch_args.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env={"ASAN_OPTIONS": "detect_leaks=1", "PATH": "/usr/bin:/bin"})
    assert out.returncode == 0 and "real launch args ok" in out.stdout, (out.stdout + out.stderr)[-3000:]


# ----------------------------------------------------------------------------------------------------------- restatement
def test_the_numpy_restatement_equals_python_integers():
    x = rc.full_scale(rf.S16, 600, 1)
    for invert in (0, 1):
        out, _ = rf.convert_all(x, rf.S16, invert)
        c = rf.convert(x, rf.S16)
        for m in list(range(0, 60)) + [150, 299]:
            i, q, _ = rf.output_int(c, m, invert)
            assert (int(out[m, 0]), int(out[m, 1])) == (i, q), (invert, m)
    assert len(out) == 300 and np.array_equal(rf.pack(out).view(np.int16).reshape(-1, 2), out)


@pytest.mark.parametrize("fmt", FORMATS)
def test_one_shot_equals_cuts_anywhere_through_the_push_rule(fmt):
    """Cuts at 0, 1, 2, 55, 56, 57 and mid-tile, in this order and in two others: odd cuts leave a sample waiting."""
    n = 2 * (2 * T + 300) + 1
    x = rc.signal(fmt, n, 10 + fmt)
    one, ref1 = rf.convert_all(x, fmt)
    assert len(one) == n // 2 and ref1.consumed == n and len(ref1.held) == 1
    rng = np.random.default_rng(n)
    for trial in range(3):
        cuts = [0, 1, 2, 55, 56, 57, T + 1234, T + 1233]
        rest = n - sum(cuts)
        while rest:
            cut = int(min(rest, rng.choice([0, 1, 2, 55, 56, 57, int(rng.integers(1, 2 * T))])))
            cuts.append(cut); rest -= cut
        if trial:
            rng.shuffle(cuts)
        c = rf.Converter(fmt)
        pos, parts = 0, []
        for cut in cuts:
            parts.append(c.push(x[pos:pos + cut])); pos += cut
            assert c.consumed == pos and c.produced == pos // 2
        assert pos == n and np.array_equal(np.concatenate(parts), one), trial


def test_four_formats_give_the_conversions_numbers():
    """The I branch is the converted even sample, delayed and signed; silence in front of the stream."""
    for fmt, raw, want in ((rf.S16, [-32768, -1, 0, 1, 32767, 12345], [-32768, -1, 0, 1, 32767, 12345]),
                           (rf.U8, [0, 1, 127, 128, 255, 200], [-32640, -32384, -128, 128, 32640, 18560]),
                           (rf.S8, [-128, -1, 0, 1, 127, 100], [-32768, -256, 0, 256, 32512, 25600]),
                           (rf.F32, [np.nan, np.inf, -np.inf, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.25, 0.999999, 3e38, -1.0, 1e-42],
                            [0, 32767, -32768, 0, 2, 2, -8192, 32767, 32767, -32768, 0])):
        assert [int(v) for v in rf.convert(np.array(raw, dtype=rf.DTYPES[fmt]), fmt)] == want, fmt
        x = np.zeros(2 * (len(raw) + rf.K), dtype=rf.DTYPES[fmt])
        if fmt == rf.U8:
            x[:] = 128                                          # 128 converts to +128, not to zero: the Q sum of a constant is zero
        x[0:2 * len(raw):2] = raw
        out, _ = rf.convert_all(x, fmt)
        m = np.arange(rf.K, rf.K + len(raw))
        s = np.where((m - rf.K) % 2 == 0, 1, -1)
        assert np.array_equal(out[m, 0], np.clip(s * np.array(want), -32768, 32767)), fmt
        assert not out[:rf.K, 0].any()


def test_invert_negates_q_and_nothing_else():
    x = rc.signal(rf.S16, 20000, 3)
    a, _ = rf.convert_all(x, rf.S16, 0)
    b, _ = rf.convert_all(x, rf.S16, 1)
    assert np.array_equal(a[:, 0], b[:, 0]) and np.abs(a[:, 1].astype(np.int64)).max() < 32767 and a[:, 1].any()
    assert np.array_equal(b[:, 1], -a[:, 1])


def test_the_rails_clamp_both_ways():
    n = 2 * 1000
    out, ref = rf.convert_all(rc.rails_low(n))
    # s * -32768: -32768 where s = +1, and +32768 clamped to 32767 where s = -1; a constant has no Q
    assert (out[rf.K::2, 0] == -32768).all() and (out[rf.K + 1::2, 0] == 32767).all() and not out[:rf.K, 0].any()
    assert not out[rf.HISTORY:, 1].any() and out[:rf.HISTORY, 1].any()          # the step from silence to the rail, and then nothing
    out, ref = rf.convert_all(rc.rails_step(n))
    assert (ref.acc_min, ref.acc_max) == (-rf.ACC_MAX, rf.ACC_MAX)
    assert out[:, 1].min() == -32768 and out[:, 1].max() == 32767 and set(out[rf.K:, 0].tolist()) == {-32768, 32767}
    inv, _ = rf.convert_all(rc.rails_step(n), rf.S16, 1)
    assert inv[:, 1].min() == -32768 and inv[:, 1].max() == 32767 and not np.array_equal(inv[:, 1], out[:, 1])
    c = rf.convert(rc.rails_step(n), rf.S16)
    hits = [m for m in range(30, 200) if abs(rf.output_int(c, m)[2]) == rf.ACC_MAX]
    assert hits and all(rf.output_int(c, m)[:2] == (int(out[m, 0]), int(out[m, 1])) for m in range(30, 200))


@pytest.mark.parametrize("b", rc.TONE_BINS)
def test_a_tone_on_a_bin_has_unit_gain_and_its_image_is_below_76_dbc(b):
    """A real tone of amplitude 20 000 that comes out on bin b of 16 384 outputs (Blackman window): the gain within 0.01 dB, the
    image at bin -b at most -76 dBc; without the Q branch the image is as strong as the tone."""
    x = rc.tone(b)
    out, _ = rf.convert_all(x)
    gain_db, image_dbc = rc.tone_levels(out, b)
    _, naive_dbc = rc.tone_levels(rc.naive(x), b)
    print("bin", b, "gain", round(gain_db, 4), "dB, image", round(image_dbc, 1), "dBc, naive image", round(naive_dbc, 1), "dBc")
    assert abs(gain_db) <= 0.01
    assert image_dbc <= -76.0
    assert naive_dbc > -10.0


# ------------------------------------------------------------------------------------- the GPU edge cases, without a GPU
@pytest.mark.parametrize("fmt", [rf.S16, rf.U8, rf.S8, rf.F32], ids=["s16", "u8", "s8", "f32"])
def test_the_vector_store_case_ends_off_the_first_lanes_and_tells_a_zeroed_last_pair(fmt):
    """tests/test_gpu_real_edges.py's lengths against the kernel's layout: the call's last pair in wave 2, inside a lane's
    group of loads and of stores.  And its rows tell a wrong load from the right one: with the last pair of the group that
    straddles the call's end read as zero, the call's last output differs in every stream -- for the one call, and for the
    first of two calls cut at VEC_CUT pairs."""
    spt = 8 if fmt in (rf.U8, rf.S8) else 4
    (wave, step, lane), pairs, words = rc.end_of_call(rc.VEC_OUTPUTS[0], spt)
    assert wave == 2 and (step, lane) != (0, 0) and 0 < pairs < spt and words == 3
    assert rc.end_of_call(rc.VEC_OUTPUTS[1], spt)[1:] == (4, 4) and rc.VEC_CUT % 2 == 1 and rc.end_of_call(rc.VEC_CUT, spt)[1] < spt
    for n_out in rc.VEC_OUTPUTS:
        for row in rc.vec_rows(fmt, n_out):
            want = rf.convert_all(row, fmt)[0]
            c = rf.convert(row, fmt)
            for n in (n_out, rc.VEC_CUT):
                zeroed = c.copy()
                zeroed[2 * n - 2:2 * n] = 0
                right, wrong = rf.output_int(c, n - 1)[:2], rf.output_int(zeroed, n - 1)[:2]
                assert right == tuple(int(v) for v in want[n - 1]) and wrong != right, (n_out, n)


# ------------------------------------------------------------------------------------------------------------ end to end
def test_the_acceptance_case(nv, oracle):
    """A real row at 504 kS/s: 518 at 140 kHz, amplitude 8000; 490 at 112 kHz, amplitude 300 under noise rc.NOISE; twelve seeds.
    R: the reference row (the same stations built as complex at 252 kS/s) decoded by the oracle's two chains; K: the real row
    through the converter; N: through `naive`.  The counts are in DESIGN 3.11."""
    t518, t490 = rc.texts()
    got = {name: {518: 0, 490: 0} for name in "RKN"}
    for seed in rc.SEEDS:
        x = rc.real_row(nv, seed)
        k, _ = rf.convert_all(x)
        assert len(k) % nv.FRAME_IN == 0
        for name, row in (("R", rc.reference_row(nv, seed)), ("K", k), ("N", rc.naive(x))):
            msgs, _ = rc.delivered(oracle, row, nv.FRAME_IN)
            got[name][518] += msgs[518] == [t518]
            got[name][490] += msgs[490] == [t490]
    print("noise", rc.NOISE, "| 490: reference", got["R"][490], "converted", got["K"][490], "naive", got["N"][490],
          "| 518:", got["R"][518], got["K"][518], got["N"][518])
    assert got["R"][490] == 12                              # the rule that fixes rc.NOISE
    assert got["K"][518] == 12
    assert got["K"][490] >= 10
    assert got["N"][490] <= got["K"][490] - 6
