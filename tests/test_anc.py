"""The antenna noise canceller (include/navtex_amd_anc.h) on the CPU: the header and the companion library's exports and
argument safety, the launch arithmetic against 128-bit integers (a stand-alone program under ASan + UBSan), the restatement
(tests/anc_ref.py) on cuts at the block ends, the zero weight, the three rejection reasons, the rails and full-scale random
rows in every format, and end to end through the oracle: the acceptance case (a weak 490 station under local noise that a
sense antenna hears too, twelve seeds), the null depth on pure common noise, and the known limit (b) -- a strong station
that is itself what the two rows share."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import anc_cases as ac
import anc_ref as ar
import resample_ref as rr

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "navtex_amd_anc.h"
PLAN = ROOT / "navtex_amd" / "anc" / "nvx_anc_plan.h"
SYMBOLS = ["nvx_anc_config_default", "nvx_anc_create", "nvx_anc_destroy", "nvx_anc_get", "nvx_anc_last_error", "nvx_anc_plan", "nvx_anc_position",
           "nvx_anc_push", "nvx_anc_reset", "nvx_anc_resident", "nvx_anc_set", "nvx_anc_set_mode", "nvx_anc_time_stats", "nvx_anc_timing"]
HOOKS = ["nvx_anc_debug_last_launch", "nvx_anc_debug_set_position"]
B = ar.BLOCK
FORMATS = (ar.CS16, ar.CU8, ar.CS8, ar.CF32)


@pytest.fixture(scope="module")
def an(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_anc.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.anc
    return navtex_amd.anc


# ------------------------------------------------------------------------------------------------------------ interface
def test_header_compiles_as_plain_c_and_declares_the_entry_points(tmp_path):
    text = HEADER.read_text()
    assert sorted(set(re.findall(r"NVX_API\s+[\w\s\*]+?\b(\w+)\s*\(", text))) == SYMBOLS
    for name, want in (("NVX_ANC_BLOCK", "65536"), ("NVX_ANC_WINDOW_LOG2_DEFAULT", "2"), ("NVX_ANC_C_ONE", "8192"), ("NVX_ANC_C_MAX", "32767"),
                       ("NVX_ANC_COHERENCE_ONE", "16384"), ("NVX_ANC_TRACK", "0"), ("NVX_ANC_HOLD", "1")):
        assert re.search(rf"#define {name}\s+{re.escape(want)}\b", text), name
    assert "Known limit" in text and "IQ-correct (each row) -> cancel -> blank -> DDC / resample -> scan -> tune -> decode" in text
    src = tmp_path / "t.c"
    src.write_text('#include "navtex_amd_anc.h"\nint main(void){ nvx_anc_config c; nvx_anc_status s; c.format = NVX_ANC_CF32; s.sums[3] = 0; '
                   'return NVX_ANC_CS16 == 0 && NVX_ANC_CU8 == 1 && NVX_ANC_CS8 == 2 && c.format == 3 && sizeof c == 20 && sizeof s == 80 && !s.sums[3] ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


@pytest.mark.parametrize("sym", SYMBOLS + HOOKS)
def test_symbol_is_exported(an, sym):
    assert hasattr(an.lib, sym), f"{sym} is declared but not exported"


def test_the_companion_links_no_other_library_of_the_project_and_no_test_infrastructure(an):
    lib = ROOT / "navtex_amd" / "libnavtex_amd_anc.so"
    out = subprocess.run(["ldd", str(lib)], capture_output=True, text=True).stdout
    assert "libnavtex_amd" not in out and "oracle" not in out and "libamdhip64" in out
    # it defines nothing but its own interface and the tests' two hooks, and needs no nvx_ symbol from elsewhere
    nm = subprocess.run(["nm", "-D", str(lib)], capture_output=True, text=True, check=True).stdout
    defined = sorted(l.split()[-1] for l in nm.splitlines() if " T " in l and "nvx_" in l)
    assert defined == sorted(SYMBOLS + HOOKS) and all(d.startswith("nvx_anc_") for d in defined)
    assert not [h for h in HOOKS if h in HEADER.read_text()] and all(h in PLAN.read_text() for h in HOOKS)
    assert an.lib.nvx_anc_debug_last_launch(None, None, None, None, None) < 0 and an.lib.nvx_anc_debug_set_position(None, 0, 0) < 0
    assert not [l for l in nm.splitlines() if " U " in l and "nvx" in l]
    for path in (ROOT / "navtex_amd" / "anc").iterdir():
        text = path.read_text()
        assert "oracle" not in text and "nvxo_" not in text, path
    assert "oracle" not in HEADER.read_text() and "oracle" not in (ROOT / "navtex_amd" / "anc.py").read_text()
    assert C.sizeof(an.Config) == 20 and C.sizeof(an.Status) == 80


def test_null_and_nonsense_arguments_are_errors_never_crashes(an, tmp_path):
    src = ROOT / "tests" / "harness" / "null_args_anc.c"
    exe = tmp_path / "null_args_anc"
    lib = ROOT / "navtex_amd"
    subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib}", "-lnavtex_amd_anc",
                    f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "anc null-safety ok" in out.stdout, (out.stdout[-2500:], out.stderr[-500:])
    assert all(re.search(rf"\b{s}\(", src.read_text()) for s in SYMBOLS)


def test_create_returns_nodev_without_a_gpu_and_refuses_bad_parameters_first(nv, an):
    for kw in (dict(window_log2=0), dict(window_log2=3), dict(window_log2=8), dict(format=4), dict(format=-1), dict(n_pairs=0), dict(n_pairs=65536)):
        with pytest.raises(nv.NvxError) as e:
            an.Canceller(**kw)
        assert e.value.code == nv._native.ERR_ARG, kw
    if nv.device_count() > 0:
        return                                                   # the rest is what a machine without a GPU answers
    cfg = an.Config()
    an.lib.nvx_anc_config_default(C.byref(cfg))
    assert (cfg.struct_size, cfg.device, cfg.format, cfg.n_pairs, cfg.window_log2) == (20, 0, 0, 1, 2)
    h = C.c_void_p(1)
    assert an.lib.nvx_anc_create(C.byref(cfg), C.byref(h)) == -2
    assert h.value is None and b"no CPU path" in an.lib.nvx_anc_last_error()
    with pytest.raises(nv.NvxError) as e:
        an.Canceller(an.CU8, n_pairs=4)
    assert e.value.code == -2


def test_the_launch_arithmetic_against_128_bit_integers_under_asan_ubsan(tmp_path):
    """nvx_anc_fill_args (navtex_amd/anc/nvx_anc_plan.h) without a device: positions up to 2^62, call lengths around a tile, a
    block and a chunk, every chunking and window -- each sample in one tile of one chunk and in the block the kernels take it
    for, a record for every block, the ring slot, 16-byte stores only on aligned rows (tests/harness/anc_launch_args.cpp).
    A stand-alone program under ASan + UBSan."""
    exe = tmp_path / "anc_launch_args"
    pkg = ROOT / "navtex_amd"
    subprocess.run(["g++", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT / 'include'}", f"-I{pkg / 'csrc'}", f"-I{pkg / 'anc'}",
                    str(ROOT / "tests" / "harness" / "anc_launch_args.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env={"ASAN_OPTIONS": "detect_leaks=1", "PATH": "/usr/bin:/bin"})
    assert out.returncode == 0 and "anc launch args ok" in out.stdout, (out.stdout + out.stderr)[-3000:]


# ----------------------------------------------------------------------------------------------------------- restatement
def _state(c):
    return (c.c, c.coherence, c.reason, c.sums(), c.samples, c.solved, c.rejected, c.history)


def _cut_everywhere(a, b, fmt, window_log2, one):
    """One shot == cuts at 0, 1, 65 535, 65 536, 65 537 and mid-block, in this order and in two others."""
    n = len(a)
    rng = np.random.default_rng(n)
    for trial in range(3):
        cuts = [0, 1, B - 1, B, B + 1, 30000]
        rest = n - sum(cuts)
        while rest:
            cut = int(min(rest, rng.choice([0, 1, B - 1, B, B + 1, int(rng.integers(1, 3 * B))])))
            cuts.append(cut); rest -= cut
        if trial:
            rng.shuffle(cuts)
        c = ar.Canceller(fmt, window_log2)
        pos, parts = 0, []
        for cut in cuts:
            parts.append(c.push(a[pos:pos + cut], b[pos:pos + cut])); pos += cut
        assert pos == n and np.array_equal(np.concatenate(parts), one[0]), trial
        assert _state(c) == _state(one[1])


@pytest.mark.parametrize("window_log2,blocks", [(2, 9.4), (4, 19.2)])
def test_one_shot_equals_cuts_at_and_next_to_the_block_ends(window_log2, blocks):
    a, b = ac.drifting_pair(int(blocks * B), 3 + window_log2)
    one = ar.cancel(a, b, ar.CS16, window_log2)
    assert one[1].solved == int(blocks) - (1 << window_log2) + 1 and len({h[1] for h in one[1].history}) == one[1].solved
    _cut_everywhere(a, b, ar.CS16, window_log2, one)


def test_nothing_is_cancelled_until_the_window_is_full_and_the_solve_behind_it():
    a, b = ac.noise_pair(6 * B, 6000, seed=7)
    out, ref = ar.cancel(a, b, ar.CS16, 2)
    assert np.array_equal(out[:4 * B], a[:4 * B]) and np.abs(out[4 * B:]).max() <= 3
    assert [h[0] for h in ref.history] == [4, 5] and all(h[3] == 0 for h in ref.history)
    assert all(abs(h[1][0] - ac.WEIGHT[0]) <= 2 and abs(h[1][1] - ac.WEIGHT[1]) <= 2 and h[2] >= 16380 for h in ref.history)
    assert ar.solve(ref.sums(), 2) == ar.solve(tuple(np.int64(v) for v in ref.sums()), 2)


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_zero_weight_is_the_main_rows_conversion(fmt):
    """HOLD from the first sample: the weight (0, 0) throughout gives the main row's conversion word for word, whatever the
    sense row holds; the sums go on."""
    n = 5 * B + 9
    (_, _), (_, _), (a, b) = ac.extremes(fmt, n, 20 + fmt)
    c = ar.Canceller(fmt, 2)
    c.set_mode(ar.HOLD)
    out = c.push(a, b)
    conv_a, conv_b = rr.convert(a, fmt), rr.convert(b, fmt)
    assert np.array_equal(out, conv_a.astype(np.int16)) and (c.samples, c.solved, c.rejected, c.c, c.coherence) == (n, 0, 0, (0, 0), 0)
    assert np.array_equal(ar.pack(out).view(np.int16).reshape(-1, 2), out)
    assert c.sums() == tuple(int(v) for v in ar.block_sums(conv_a[B:5 * B], conv_b[B:5 * B]))


def test_reason_one_a_silent_sense_row_and_reason_two_a_faint_one():
    n = 5 * B + 100
    a, b = ac.silent_sense(n)
    out, ref = ar.cancel(a, b, ar.CS16, 2)
    assert (ref.reason, ref.rejected, ref.solved, ref.c, ref.coherence) == (1, 2, 0, (0, 0), 0) and np.array_equal(out, a)
    assert ref.sums() == (4 * B * 2 ** 31, 0, 0, 0)
    a, b = ac.faint_sense(n)
    out, ref = ar.cancel(a, b, ar.CS16, 2)
    assert (ref.reason, ref.rejected, ref.solved, ref.c, ref.coherence) == (2, 2, 0, (0, 0), 0) and np.array_equal(out, a)
    assert ref.sums() == (4 * B * 2 ** 31, 4 * B * 32, -4 * B * 2 * 4 * 32768, 0)
    # one step up the sense row passes step 1, one step down it fails it: TBB = 16 N is (2, 2) on half the samples and (3, 3) ...
    b = np.full((n, 2), 2, dtype=np.int16)
    assert ar.cancel(a, b, ar.CS16, 2)[1].reason == 1                  # TBB = 8 N
    b = np.full((n, 2), 3, dtype=np.int16)
    assert ar.cancel(a, b, ar.CS16, 2)[1].reason == 2                  # TBB = 18 N, tbb = 4


def test_reason_three_against_the_sense_row_at_half_the_main_row():
    """The sense row at a quarter of the main row wants 4.0 = 32768 in Q13, one more than fits: reason 3, with the coherence
    of a perfect match.  At half it solves to (16384, 0), and nothing is left of the main row."""
    n = 5 * B + 100
    a, b = ac.quarter_sense(n)
    out, ref = ar.cancel(a, b, ar.CS16, 2)
    assert (ref.reason, ref.rejected, ref.solved, ref.c) == (3, 2, 0, (0, 0)) and ref.coherence == 16384 and np.array_equal(out, a)
    a, b = ac.half_sense(n)
    out, ref = ar.cancel(a, b, ar.CS16, 2)
    assert (ref.reason, ref.rejected, ref.solved, ref.c, ref.coherence) == (0, 0, 2, (16384, 0), 16384)
    assert np.array_equal(out[:4 * B], a[:4 * B]) and not out[4 * B:].any()


def test_both_rows_at_the_rails():
    """(-32768, -32768) in both rows: every product at its largest (each term 2^31, the window's sums 2^49), the weight
    (8192, 0), and p = r = 8192 * -32768 + 4096."""
    n = 6 * B + 5
    a = ac.rails(n)
    one = ar.cancel(a, a.copy(), ar.CS16, 2)
    assert one[1].sums() == (4 * B * 2 ** 31, 4 * B * 2 ** 31, 4 * B * 2 ** 31, 0)
    assert (one[1].c, one[1].coherence, one[1].reason, one[1].solved) == ((8192, 0), 16384, 0, 3) and not one[0][4 * B:].any()
    _cut_everywhere(a, a.copy(), ar.CS16, 2, one)
    # W = 64 at the rails: the largest sums there are, checked against the header's bounds inside solve()
    full = (64 * B * 2 ** 31,) * 3 + (0,)
    assert ar.solve(full, 6) == ((8192, 0), 16384, 0)
    # the largest weight against the largest sample: the bound of the apply, checked inside apply()
    hi = np.array([[-32768, -32768], [32767, -32768], [-32768, 32767]], dtype=np.int64)
    for c in ((32767, 32767), (-32767, 32767), (32767, -32767), (-32767, -32767)):
        ar.apply(hi, hi, c)


@pytest.mark.parametrize("fmt", FORMATS)
def test_full_scale_rows_in_every_format(fmt):
    """The lowest value throughout, the rails alternating in sign, and full-scale random rows (float32: NaN, infinities,
    denormals and the ties of the rounding among them): one shot equals the cut rows, and the sums are the direct ones."""
    n = 5 * B + 21000
    for k, (a, b) in enumerate(ac.extremes(fmt, n, 500 + fmt)):
        one = ar.cancel(a, b, fmt, 2)
        assert one[1].solved + one[1].rejected == 2, k
        ca, cb = rr.convert(a, fmt), rr.convert(b, fmt)
        assert one[1].sums() == tuple(int(v) for v in ar.block_sums(ca[B:5 * B], cb[B:5 * B])), k
        c = ar.Canceller(fmt, 2)
        parts = [c.push(a[:2 * B + 11], b[:2 * B + 11]), c.push(a[2 * B + 11:], b[2 * B + 11:])]
        assert np.array_equal(np.concatenate(parts), one[0]) and _state(c) == _state(one[1]), k
    if fmt == ar.CS16:
        (a, b) = ac.extremes(fmt, n, 500)[0]
        assert np.array_equal(a, ac.rails(n)) and np.array_equal(b, ac.rails(n))


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def acceptance(nv, oracle):
    """The twelve seeds, once: what arrives from the main row, the sense row and the cancelled row, and the last weight."""
    want = ac.text()
    got = {"main": 0, "sense": 0, "cancelled": 0}
    weights = []
    for seed in ac.SEEDS:
        a, b = ac.pair(nv, seed)
        y, ref = ar.cancel(a, b)
        assert ref.rejected == 0 and ref.solved == len(a) // B - 4 + 1 and ref.window_log2 == 2
        for name, row in (("main", a), ("sense", b), ("cancelled", y)):
            got[name] += ac.delivered(oracle, row, nv.FRAME_IN)[0] == [want]
        weights.append((ref.c, ref.coherence))
    print("490 delivered: main", got["main"], "sense", got["sense"], "cancelled", got["cancelled"], "of 12; last weights", weights)
    return got, weights


def test_the_acceptance_case_delivers_from_the_cancelled_row_only(acceptance):
    """490 at -14 kHz, amplitude 300, under common noise of +-6000 and +-150 of each receiver's own; the station reaches the
    sense antenna at 0.3 e^{j 0.7}, the noise at 0.8 e^{j 2.1}; W = 4.  Measured: main 0, sense 0, cancelled 12 of 12."""
    got, _ = acceptance
    assert got["cancelled"] == 12
    assert got["main"] <= 1 and got["sense"] <= 1


def test_the_acceptance_cases_weight_is_the_noise_paths(acceptance):
    """The exact weight is 8192 / (0.8 e^{j 2.1}) = (-5170, -8839); the station the two rows share moves the solved one by
    about (19, 4)."""
    _, weights = acceptance
    for (c_re, c_im), coherence in weights:
        assert abs(c_re - ac.WEIGHT[0]) <= 40 and abs(c_im - ac.WEIGHT[1]) <= 40, (c_re, c_im)
        assert coherence > 16000


def test_the_null_depth_on_pure_common_noise():
    """No station and no own noise, 8 blocks, W = 4: the output's power behind block 4 against the main row's.  What is left
    is the rounding of the int16 samples of the sense row times the weight's gain of 1.25, and of the weight itself.
    Measured -75.7 dB at +-6000 and -83.7 dB at +-20000."""
    depth = {}
    for amp in (6000, 20000):
        a, b = ac.noise_pair(8 * B, amp)
        y, ref = ar.cancel(a, b, ar.CS16, 2)
        depth[amp] = ac.power_db(y[4 * B:], a[4 * B:])
        assert ref.solved == 4 and ref.rejected == 0
    print("null depth", {k: round(v, 1) for k, v in depth.items()}, "dB")
    assert depth[6000] <= -70.0


def test_the_known_limit_a_station_that_is_what_the_rows_share(nv, oracle):
    """Known limit (b): the station at amplitude 8000 on both rows, +-1500 of own noise, no common noise.  The canceller
    takes the station for the noise.  The coherence says so, and that is all that is asserted; the station's drop in dB and
    whether it is still delivered are printed, and DESIGN 3.14 records them."""
    want = ac.text()
    for seed in ac.SEEDS[:2]:
        a, b = ac.limit_pair(nv, seed)
        y, ref = ar.cancel(a, b)
        s = ac.station(nv, seed, ac.LIMIT_AMP)[4 * B:]
        level = abs(np.vdot(s, y[4 * B:].astype(np.float64) @ (1, 1j)) / np.vdot(s, s))
        print("seed", seed, "coherence", ref.coherence, "weight", ref.c, "the station's level in the output", round(20 * np.log10(max(level, 1e-9)), 1),
              "dB, power", round(ac.power_db(y[4 * B:], a[4 * B:]), 1), "dB, delivered", ac.delivered(oracle, y, nv.FRAME_IN)[0] == [want])
        assert all(h[2] > 14000 for h in ref.history) and ref.rejected == 0
