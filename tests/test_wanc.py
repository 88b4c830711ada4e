"""The multi-tap noise canceller (include/navtex_amd_wanc.h) on the CPU: the header and the companion library's exports and
argument safety, the launch arithmetic against 128-bit integers and the solve's integer division against the processor's
(stand-alone programs under ASan + UBSan), the solve compiled for the host against the restatement (tests/wanc_ref.py), the
restatement on cuts at the block ends, the unfilled window, zero weights, the three rejection reasons, the rails and
full-scale random rows in every format, and end to end through the oracle: the acceptance case (the canceller's, with the noise
reaching the main antenna over three echoes, twelve seeds) and the null depth on pure common noise over the same paths."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import anc_cases as ac
import anc_ref as ar
import resample_ref as rr
import wanc_cases as wc
import wanc_ref as wr

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "navtex_amd_wanc.h"
PLAN = ROOT / "navtex_amd" / "wanc" / "nvx_wanc_plan.h"
SYMBOLS = ["nvx_wanc_config_default", "nvx_wanc_create", "nvx_wanc_destroy", "nvx_wanc_get", "nvx_wanc_last_error", "nvx_wanc_plan", "nvx_wanc_position",
           "nvx_wanc_push", "nvx_wanc_reset", "nvx_wanc_resident", "nvx_wanc_set", "nvx_wanc_set_mode", "nvx_wanc_time_stats", "nvx_wanc_timing"]
HOOKS = ["nvx_wanc_debug_last_launch", "nvx_wanc_debug_set_position"]
B = wr.BLOCK
FORMATS = (wr.CS16, wr.CU8, wr.CS8, wr.CF32)
SANITIZE = ["-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
SANITIZE_ENV = {"ASAN_OPTIONS": "detect_leaks=1", "PATH": "/usr/bin:/bin"}


@pytest.fixture(scope="module")
def wn(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_wanc.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.wanc
    return navtex_amd.wanc


# ------------------------------------------------------------------------------------------------------------ interface
def test_header_compiles_as_plain_c_and_declares_the_entry_points(tmp_path):
    text = HEADER.read_text()
    assert sorted(set(re.findall(r"NVX_API\s+[\w\s\*]+?\b(\w+)\s*\(", text))) == SYMBOLS
    for name, want in (("NVX_WANC_BLOCK", "65536"), ("NVX_WANC_WINDOW_LOG2_DEFAULT", "2"), ("NVX_WANC_TAPS_DEFAULT", "8"), ("NVX_WANC_TAPS_MAX", "16"),
                       ("NVX_WANC_LOAD_LOG2_DEFAULT", "12"), ("NVX_WANC_W_ONE", "8192"), ("NVX_WANC_W_MAX", "32767"), ("NVX_WANC_L1_MAX", "65534"),
                       ("NVX_WANC_COHERENCE_ONE", "16384"), ("NVX_WANC_TRACK", "0"), ("NVX_WANC_HOLD", "1")):
        assert re.search(rf"#define {name}\s+{re.escape(want)}\b", text), name
    assert "Known limit" in text and "IQ-correct (each row) -> align -> multi-tap cancel -> blank -> notch -> DDC / resample -> scan -> tune -> decode" in text
    src = tmp_path / "t.c"
    src.write_text('#include "navtex_amd_wanc.h"\nint main(void){ nvx_wanc_config c; nvx_wanc_status s; c.format = NVX_WANC_CF32; s.q_im[15] = 0; '
                   'return NVX_WANC_CS16 == 0 && NVX_WANC_CU8 == 1 && NVX_WANC_CS8 == 2 && c.format == 3 && sizeof c == 28 && sizeof s == 688 && !s.q_im[15] ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


@pytest.mark.parametrize("sym", SYMBOLS + HOOKS)
def test_symbol_is_exported(wn, sym):
    assert hasattr(wn.lib, sym), f"{sym} is declared but not exported"


def test_the_companion_links_no_other_library_of_the_project_and_no_test_infrastructure(wn):
    lib = ROOT / "navtex_amd" / "libnavtex_amd_wanc.so"
    out = subprocess.run(["ldd", str(lib)], capture_output=True, text=True).stdout
    assert "libnavtex_amd" not in out and "oracle" not in out and "libamdhip64" in out
    # it defines nothing but its own interface and the tests' two hooks, and needs no nvx_ symbol from elsewhere
    nm = subprocess.run(["nm", "-D", str(lib)], capture_output=True, text=True, check=True).stdout
    defined = sorted(l.split()[-1] for l in nm.splitlines() if " T " in l and "nvx_" in l)
    assert defined == sorted(SYMBOLS + HOOKS) and all(d.startswith("nvx_wanc_") for d in defined)
    assert not [h for h in HOOKS if h in HEADER.read_text()] and all(h in PLAN.read_text() for h in HOOKS)
    assert wn.lib.nvx_wanc_debug_last_launch(None, None, None, None, None) < 0 and wn.lib.nvx_wanc_debug_set_position(None, 0, 0) < 0
    assert not [l for l in nm.splitlines() if " U " in l and "nvx" in l]
    for path in (ROOT / "navtex_amd" / "wanc").iterdir():
        text = path.read_text()
        assert "oracle" not in text and "nvxo_" not in text, path
    assert "oracle" not in HEADER.read_text() and "oracle" not in (ROOT / "navtex_amd" / "wanc.py").read_text()
    assert C.sizeof(wn.Config) == 28 and C.sizeof(wn.Status) == 688


def test_null_and_nonsense_arguments_are_errors_never_crashes(wn, tmp_path):
    src = ROOT / "tests" / "harness" / "null_args_wanc.c"
    exe = tmp_path / "null_args_wanc"
    lib = ROOT / "navtex_amd"
    subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib}", "-lnavtex_amd_wanc",
                    f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "wanc null-safety ok" in out.stdout, (out.stdout[-2500:], out.stderr[-500:])
    assert all(re.search(rf"\b{s}\(", src.read_text()) for s in SYMBOLS)


def test_create_returns_nodev_without_a_gpu_and_refuses_bad_parameters_first(nv, wn):
    for kw in (dict(window_log2=0), dict(window_log2=3), dict(window_log2=8), dict(format=4), dict(format=-1), dict(n_pairs=0), dict(n_pairs=65536),
               dict(n_taps=0), dict(n_taps=2), dict(n_taps=12), dict(n_taps=32), dict(load_log2=7), dict(load_log2=21)):
        with pytest.raises(nv.NvxError) as e:
            wn.Canceller(**kw)
        assert e.value.code == nv._native.ERR_ARG, kw
    if nv.device_count() > 0:
        return                                                   # the rest is what a machine without a GPU answers
    cfg = wn.Config()
    wn.lib.nvx_wanc_config_default(C.byref(cfg))
    assert (cfg.struct_size, cfg.device, cfg.format, cfg.n_pairs, cfg.window_log2, cfg.n_taps, cfg.load_log2) == (28, 0, 0, 1, 2, 8, 12)
    h = C.c_void_p(1)
    assert wn.lib.nvx_wanc_create(C.byref(cfg), C.byref(h)) == -2
    assert h.value is None and b"no CPU path" in wn.lib.nvx_wanc_last_error()
    with pytest.raises(nv.NvxError) as e:
        wn.Canceller(wn.CU8, n_pairs=4, n_taps=16)
    assert e.value.code == -2


def test_the_launch_arithmetic_against_128_bit_integers_under_asan_ubsan(tmp_path):
    """nvx_wanc_fill_args (navtex_amd/wanc/nvx_wanc_plan.h) without a device: positions up to 2^62, call lengths from one sample
    to around a tile, a block and a chunk, every chunking, window and tap count -- each sample in one part of one tile of one
    chunk and in the block the kernels take it for, a record for every block, the ring slot, the halo's reads, the state row's
    layout, 16-byte stores only on aligned rows (tests/harness/wanc_launch_args.cpp).  A stand-alone program under ASan + UBSan."""
    exe = tmp_path / "wanc_launch_args"
    pkg = ROOT / "navtex_amd"
    subprocess.run(["g++", *SANITIZE, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT / 'include'}", f"-I{pkg / 'csrc'}", f"-I{pkg / 'wanc'}",
                    str(ROOT / "tests" / "harness" / "wanc_launch_args.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=SANITIZE_ENV)
    assert out.returncode == 0 and "wanc launch args ok" in out.stdout, (out.stdout + out.stderr)[-3000:]


@pytest.fixture(scope="module")
def solve_exe(tmp_path_factory):
    """navtex_amd/wanc/nvx_wanc_solve.h, the code the solve kernel runs per lane, compiled for the host under ASan + UBSan with
    the library's -ffp-contract=off (tests/harness/wanc_solve.cpp): a stand-alone program."""
    exe = tmp_path_factory.mktemp("wanc_solve") / "wanc_solve"
    pkg = ROOT / "navtex_amd"
    subprocess.run(["g++", *SANITIZE, "-ffp-contract=off", f"-I{ROOT / 'include'}", f"-I{pkg / 'csrc'}", f"-I{pkg / 'wanc'}",
                    str(ROOT / "tests" / "harness" / "wanc_solve.cpp"), "-o", str(exe)], check=True)
    return exe


def test_the_solves_integer_division_is_the_ieee_one(solve_exe):
    """The fp64 division instruction sequence is made of fused multiply-adds, which the solve is compiled without; its quotients
    are formed in integers.  Against the processor's division: corner cases and four million random operands, subnormal
    operands and results, overflow and near ties among them."""
    out = subprocess.run([str(solve_exe), "div"], capture_output=True, text=True, timeout=300, env=SANITIZE_ENV)
    assert out.returncode == 0 and "wanc div ok" in out.stdout, (out.stdout + out.stderr)[-3000:]


def _solve_lines(solve_exe, cases):
    """cases: (K, window_log2, load_log2, sums) -> what the host build of the kernel's solve prints for each."""
    text = "".join(f"{K} {wl} {ll} {s[4 * K]} " + " ".join(str(int(v)) for v in s[:4 * K]) + "\n" for K, wl, ll, s in cases)
    out = subprocess.run([str(solve_exe), "solve"], input=text, capture_output=True, text=True, timeout=300, env=SANITIZE_ENV)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    return [tuple(int(v) for v in line.split()) for line in out.stdout.splitlines()]


def test_the_kernels_solve_on_the_host_equals_the_restatement(solve_exe):
    """The windows of real rows in every tap count, window and loading, the rejection reasons' windows, the rails, and random sums
    that are no autocorrelation at all (most end in reason 2 or 3): reason, coherence and all 2 K weights."""
    cases = []
    for K in (4, 8, 16):
        for wl, ll, seed in ((2, 12, 1), (2, 8, 2), (2, 20, 3), (4, 16, 4)):
            n = ((1 << wl) + 2) * B + 5
            a, b = wc.drifting_pair(n, 40 + seed) if seed != 2 else wc.noise_pair(n, 150)
            ref = wr.cancel(a, b, wr.CS16, K, wl, ll)[1]
            assert ref.solved >= 2
            cases.append((K, wl, ll, ref.sums()))
        for a, b in (wc.silent_sense(5 * B), wc.edge_sense(6 * B + 1), wc.weak_white_sense(5 * B), (ac.rails(5 * B), ac.rails(5 * B))):
            cases.append((K, 2, 12, wr.cancel(a, b, wr.CS16, K)[1].sums()))
        rng = np.random.default_rng(K)
        for _ in range(40):
            s = rng.integers(-2 ** 40, 2 ** 40, size=wr.n_sums(K))
            s[0], s[K], s[4 * K] = abs(s[0]) * 64 + 2 ** 30, 0, abs(s[4 * K]) * 64
            cases.append((K, 2, int(rng.integers(8, 21)), tuple(int(v) for v in s)))
    got = _solve_lines(solve_exe, cases)
    assert len(got) == len(cases)
    reasons = set()
    for (K, wl, ll, s), line in zip(cases, got):
        (w_re, w_im), coherence, reason = wr.solve(s, K, wl, ll)
        assert line == (reason, coherence) + w_re + w_im, (K, wl, ll, s)
        reasons.add(reason)
    assert reasons == {0, 1, 2, 3}


# ----------------------------------------------------------------------------------------------------------- restatement
def _state(c):
    return (c.w, c.coherence, c.reason, c.sums(), c.samples, c.solved, c.rejected, c.history, c.hist_a.tolist(), c.hist_b.tolist())


def _cut_everywhere(a, b, fmt, K, window_log2, one):
    """One shot == cuts at 0, 1, 65 535, 65 536, 65 537 and mid-block, K - 1 and K / 2 samples, in this order and in two others."""
    n = len(a)
    rng = np.random.default_rng(n)
    for trial in range(3):
        cuts = [0, 1, B - 1, B, B + 1, 30000, K - 1, K // 2]
        rest = n - sum(cuts)
        while rest:
            cut = int(min(rest, rng.choice([0, 1, B - 1, B, B + 1, K - 1, int(rng.integers(1, 3 * B))])))
            cuts.append(cut); rest -= cut
        if trial:
            rng.shuffle(cuts)
        c = wr.Canceller(fmt, K, window_log2)
        pos, parts = 0, []
        for cut in cuts:
            parts.append(c.push(a[pos:pos + cut], b[pos:pos + cut])); pos += cut
        assert pos == n and np.array_equal(np.concatenate(parts), one[0]), trial
        assert _state(c) == _state(one[1])


@pytest.mark.parametrize("K,window_log2,blocks", [(8, 2, 9.4), (4, 2, 7.2), (16, 4, 19.2)])
def test_one_shot_equals_cuts_at_and_next_to_the_block_ends(K, window_log2, blocks):
    a, b = wc.drifting_pair(int(blocks * B), 3 + window_log2 + K)
    one = wr.cancel(a, b, wr.CS16, K, window_log2)
    assert one[1].solved == int(blocks) - (1 << window_log2) + 1 and len({h[1] for h in one[1].history}) == one[1].solved
    _cut_everywhere(a, b, wr.CS16, K, window_log2, one)


def test_one_sample_at_a_time_across_a_block_end():
    K = 8
    a, b = wc.drifting_pair(5 * B + 40, 21)
    out, one = wr.cancel(a, b)
    c = wr.Canceller()
    parts = [c.push(a[:5 * B - 20], b[:5 * B - 20])]
    for i in range(5 * B - 20, 5 * B + 40):
        parts.append(c.push(a[i:i + 1], b[i:i + 1]))
    assert np.array_equal(np.concatenate(parts), out) and _state(c) == _state(one) and one.solved == 2 and K == one.K


def test_nothing_is_cancelled_until_the_window_is_full_and_the_solve_behind_it():
    """Pure common noise without echoes: the float trial's null is -70 dB at load_log2 = 12 (known limit (b)); 10 dB are left
    for the exact arithmetic."""
    a, b = wc.noise_pair(6 * B, 0, seed=7, echoes=False)
    out, ref = wr.cancel(a, b)
    assert np.array_equal(out[:4 * B], wc.delayed(a, 4)[:4 * B])
    assert ac.power_db(out[4 * B:], wc.delayed(a, 4)[4 * B:]) < -60.0
    assert [h[0] for h in ref.history] == [4, 5] and all(h[3] == 0 and h[2] >= 16300 for h in ref.history)
    assert wr.solve(ref.sums(), 8, 2, 12) == wr.solve(tuple(np.int64(v) for v in ref.sums()), 8, 2, 12)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("K", [4, 8, 16])
def test_zero_weights_are_the_main_rows_conversion_delayed(fmt, K):
    """HOLD from the first sample: zero weights throughout give the main row's conversion G samples late, word for word,
    whatever the sense row holds; the sums go on."""
    n = 5 * B + 9
    (_, _), (_, _), (a, b) = ac.extremes(fmt, n, 20 + fmt)
    c = wr.Canceller(fmt, K)
    c.set_mode(wr.HOLD)
    out = c.push(a, b)
    conv_a, conv_b = rr.convert(a, fmt), rr.convert(b, fmt)
    assert np.array_equal(out, wc.delayed(conv_a, K // 2).astype(np.int16)) and (c.samples, c.solved, c.rejected, c.coherence) == (n, 0, 0, 0)
    assert c.w == ((0,) * K, (0,) * K)
    assert np.array_equal(wr.pack(out).view(np.int16).reshape(-1, 2), out)
    assert c.sums() == tuple(int(v) for v in wr.block_sums(wc.delayed(conv_a, K // 2)[B:5 * B], conv_b[B - (K - 1):5 * B], K))


def test_the_three_reasons_are_each_reached_by_a_constructed_pair():
    n = 6 * B + 100
    a, b = wc.silent_sense(n)
    out, ref = wr.cancel(a, b)
    assert (ref.reason, ref.rejected, ref.solved, ref.coherence) == (1, 3, 0, 0) and np.array_equal(out, wc.delayed(a, 4)) and not any(ref.w[0] + ref.w[1])
    assert ref.sums()[0] == 0 and ref.sums()[32] == 4 * B * 2 ** 31
    # one step up the sense row passes step 1: R0 = 16 N is (2, 2) on half the samples and (3, 3) ...
    assert wr.cancel(a, np.full((n, 2), 2, dtype=np.int16))[1].reason == 1                  # R0 = 8 N
    assert wr.cancel(a, np.full((n, 2), 3, dtype=np.int16))[1].reason != 1                  # R0 = 18 N
    a, b = wc.edge_sense(n)
    out, ref = wr.cancel(a, b)
    assert [h[3] for h in ref.history] == [3, 3, 2] and (ref.reason, ref.rejected, ref.coherence) == (2, 3, 0) and np.array_equal(out, wc.delayed(a, 4))
    s = ref.sums()
    assert abs(s[1]) > s[0] + (s[0] >> 12) + 1                  # |r[1]| > r[0] + lambda: no autocorrelation
    a, b = wc.weak_white_sense(n)
    out, ref = wr.cancel(a, b)
    assert (ref.reason, ref.rejected, ref.solved) == (3, 3, 0) and ref.coherence > 16000 and np.array_equal(out, wc.delayed(a, 4))
    # the same path within the bounds solves: 3.5 on tap G + 1, and nothing is left
    a = np.zeros((n, 2), dtype=np.int16); a[1:] = 7 * (b[:-1] // 2 * 2) // 2
    out, ref = wr.cancel(a, b, load_log2=20)
    assert (ref.reason, ref.solved) == (0, 3) and abs(ref.w[0][5] - 28672) <= 4 and sum(abs(v) for v in ref.w[0] + ref.w[1]) < 28672 + 60


def test_both_rows_at_the_rails_with_the_bounds_asserted():
    """(-32768, -32768) in both rows: every real part at 2^31, the one value a 32-bit dot product wraps at (the window's sums
    2^49), bounds asserted inside block_sums() and apply(); W = 64 at the rails has the largest sums there are; and the largest
    weights against the largest samples meet the bound of the apply."""
    n = 6 * B + 5
    a = ac.rails(n)
    one = wr.cancel(a, a.copy())
    s = one[1].sums()
    assert s[:8] == (4 * B * 2 ** 31,) * 8 and s[16:24] == (4 * B * 2 ** 31,) * 8 and s[32] == 4 * B * 2 ** 31 and not any(s[8:16]) and not any(s[24:32])
    assert one[1].reason == 0 and one[1].solved == 3 and one[1].w == ((1024,) * 8, (0,) * 8) and np.abs(one[0][4 * B:]).max() <= 4
    _cut_everywhere(a, a.copy(), wr.CS16, 8, 2, one)
    for K in (4, 8, 16):
        full = (64 * B * 2 ** 31,) * K + (0,) * K + (64 * B * 2 ** 31,) * K + (0,) * K + (64 * B * 2 ** 31,)
        assert max(full) == 1 << 53
        (w_re, w_im), coherence, reason = wr.solve(full, K, 6, 12)
        assert reason == 0 and w_re == (8192 // K,) * K and not any(w_im) and coherence >= 16380
    hi = np.array([[-32768, -32768]] * 20 + [[32767, -32768]] * 20 + [[-32768, 32767]] * 20, dtype=np.int64)
    for w in (((32767, -32767) + (0,) * 6, (0,) * 8), ((0,) * 8, (0,) * 6 + (-32767, 32767)), ((-8192,) * 4 + (0,) * 4, (8191,) * 3 + (8193,) + (0,) * 4)):
        assert sum(abs(v) for v in w[0] + w[1]) == wr.L1_MAX
        wr.apply(hi[7:], hi, w, 8)


@pytest.mark.parametrize("fmt", FORMATS)
def test_full_scale_rows_in_every_format(fmt):
    """The lowest value throughout, the rails alternating in sign, and full-scale random rows (float32: NaN, infinities,
    denormals and the ties of the rounding among them): one shot equals the cut rows, and the sums are the direct ones."""
    n = 5 * B + 21000
    for k, (a, b) in enumerate(ac.extremes(fmt, n, 500 + fmt)):
        one = wr.cancel(a, b, fmt)
        assert one[1].solved + one[1].rejected == 2, k
        ca, cb = rr.convert(a, fmt), rr.convert(b, fmt)
        assert one[1].sums() == tuple(int(v) for v in wr.block_sums(wc.delayed(ca, 4)[B:5 * B], cb[B - 7:5 * B], 8)), k
        c = wr.Canceller(fmt)
        parts = [c.push(a[:2 * B + 11], b[:2 * B + 11]), c.push(a[2 * B + 11:], b[2 * B + 11:])]
        assert np.array_equal(np.concatenate(parts), one[0]) and _state(c) == _state(one[1]), k


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def acceptance(nv, oracle):
    """The twelve seeds, once: what arrives from the main row, the single-weight canceller's row and the multi-tap row."""
    want = ac.text()
    got = {"main": 0, "single": 0, "multi": 0}
    rejected, nulls = 0, []
    for seed in wc.SEEDS:
        a, b = wc.pair(nv, seed)
        y, ref = wr.cancel(a, b, wr.CS16, 8, 2, 12)
        y1, _ = ar.cancel(a, b)
        assert ref.solved + ref.rejected == len(a) // B - 4 + 1
        rejected += ref.rejected
        for name, row in (("main", a), ("single", y1), ("multi", y)):
            got[name] += ac.delivered(oracle, row, nv.FRAME_IN)[0] == [want]
        nulls.append((round(ac.power_db(y[4 * B:], wc.delayed(a, 4)[4 * B:]), 1), round(ac.power_db(y1[4 * B:], a[4 * B:]), 1)))
    print("490 delivered: main", got["main"], "single weight", got["single"], "8 taps", got["multi"], "of 12; blocks rejected", rejected,
          "; power left (8 taps, single weight) dB", nulls)
    return got, rejected


def test_the_acceptance_case_delivers_from_the_multi_tap_row_only(acceptance):
    """The canceller's acceptance case (490 at -14 kHz, amplitude 300, common noise +-6000, own noise +-150, W = 4, seeds 11 .. 22)
    with the noise reaching the main antenna over three echoes and the sense antenna over one; K = 8, load_log2 = 12.
    Measured in the exact arithmetic: main 0, single weight 0 (its null is -4.5 dB), 8 taps 12 of 12 (-23.8 dB), no block
    rejected."""
    got, rejected = acceptance
    assert got["multi"] == 12
    assert got["main"] <= 1 and got["single"] <= 1
    assert rejected == 0


def test_the_null_depth_on_pure_common_noise_over_the_two_paths():
    """No station, 8 blocks, W = 4, the acceptance case's two paths, own noise 0 and +-150: the power left behind block 4 against
    the delayed main row's, broadband and inside +-500 Hz at -14 and +14 kHz, for K = 4, 8 and 16 and for the single-weight
    canceller; and without echoes at load_log2 = 12 and 16 (known limit (b)).  DESIGN 3.18 records the figures.  Asserted: with own
    noise +-150, 8 taps null at least 15 dB deeper than the single weight at both frequencies."""
    n = 8 * B
    table = {}
    for own in (0, 150):
        a, b = wc.noise_pair(n, own)
        y1, _ = ar.cancel(a, b)
        rows = {"single": (y1, a)}
        for K in (4, 8, 16):
            y, ref = wr.cancel(a, b, wr.CS16, K)
            assert ref.solved == 4 and ref.rejected == 0
            rows[f"K={K}"] = (y, wc.delayed(a, K // 2))
        for name, (y, against) in rows.items():
            table[(own, name)] = tuple(round(f, 1) for f in (ac.power_db(y[4 * B:], against[4 * B:]), wc.band_db(y[4 * B:], against[4 * B:], -14000.0),
                                                             wc.band_db(y[4 * B:], against[4 * B:], 14000.0)))
            print("own noise", own, name, "broadband, -14 kHz, +14 kHz (dB):", table[(own, name)])
    for ll in (12, 16):
        a, b = wc.noise_pair(n, 0, echoes=False)
        y, _ = wr.cancel(a, b, wr.CS16, 8, 2, ll)
        print("no echoes, no own noise, load_log2", ll, "broadband (dB):", round(ac.power_db(y[4 * B:], wc.delayed(a, 4)[4 * B:]), 1),
              "single weight:", round(ac.power_db(ar.cancel(a, b)[0][4 * B:], a[4 * B:]), 1))
    for f in (1, 2):
        assert table[(150, "K=8")][f] <= table[(150, "single")][f] - 15.0, table
