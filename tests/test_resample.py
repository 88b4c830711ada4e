"""The resampler (include/navtex_amd_resample.h) on the CPU: the header and the companion library's exports and argument
safety, the plan's launch arithmetic against 128-bit integers (a stand-alone program under ASan + UBSan), the rates and the
count rule against exact rational arithmetic, the taps nvx_resample_design hands out (their properties and the prototype's
response for the twelve rates of the header), the restatement (tests/resample_ref.py) on constants and at the rails, and
resample -> decode end to end through the restatements."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import resample_ref as rr
import signals

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "navtex_amd_resample.h"
SYMBOLS = ["nvx_resample_config_default", "nvx_resample_create", "nvx_resample_design", "nvx_resample_destroy",
           "nvx_resample_last_error", "nvx_resample_out_count", "nvx_resample_plan", "nvx_resample_position", "nvx_resample_push",
           "nvx_resample_reset", "nvx_resample_resident", "nvx_resample_set_form", "nvx_resample_time_stats", "nvx_resample_timing"]


@pytest.fixture(scope="module")
def rs(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_resample.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.resample
    return navtex_amd.resample


@pytest.fixture(scope="module")
def plans(rs):
    return {fi: rs.design(fi) for fi in rr.RATES}


# ------------------------------------------------------------------------------------------------------------ interface
def test_header_compiles_as_plain_c_and_declares_the_entry_points(tmp_path):
    text = HEADER.read_text()
    assert sorted(set(re.findall(r"NVX_API\s+[\w\s\*]+?\b(\w+)\s*\(", text))) == SYMBOLS
    for name, want in (("NVX_RS_OUTPUT_RATE", "252000"), ("NVX_RS_SHIFT", "15"), ("NVX_RS_MAX_RATE", "3200000"), ("NVX_RS_MIN_RATE", "96000"),
                       ("NVX_RS_MAX_PHASES", "1024"), ("NVX_RS_MAX_TAPS", "32768")):
        assert re.search(rf"#define {name}\s+{re.escape(want)}\b", text), name
    assert "out of scope" in text and "3.2 MS/s" in text
    src = tmp_path / "t.c"
    src.write_text('#include "navtex_amd_resample.h"\nint main(void){ nvx_resample_config c; c.format = NVX_RS_CF32; '
                   'return NVX_RS_CS16 == 0 && NVX_RS_CU8 == 1 && NVX_RS_CS8 == 2 && c.format == 3 && sizeof c == 20 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


@pytest.mark.parametrize("sym", SYMBOLS)
def test_symbol_is_exported(rs, sym):
    assert hasattr(rs.lib, sym), f"{sym} is declared in navtex_amd_resample.h but not exported"


def test_the_companion_links_neither_the_product_library_nor_test_infrastructure(rs):
    lib = ROOT / "navtex_amd" / "libnavtex_amd_resample.so"
    out = subprocess.run(["ldd", str(lib)], capture_output=True, text=True).stdout
    assert "libnavtex_amd.so" not in out and "libnavtex_amd_scan" not in out and "oracle" not in out and "libamdhip64" in out
    # it defines nothing but its own interface, and needs no nvx_ symbol from elsewhere
    nm = subprocess.run(["nm", "-D", str(lib)], capture_output=True, text=True, check=True).stdout
    defined = sorted(l.split()[-1] for l in nm.splitlines() if " T " in l and "nvx_" in l)
    hook = "nvx_resample_debug_last_launch"              # the tests' one hook: declared in nvx_resample_plan.h, not in the public header
    assert defined == sorted(SYMBOLS + [hook]) and hook not in HEADER.read_text()
    assert hook in (ROOT / "navtex_amd" / "resample" / "nvx_resample_plan.h").read_text() and rs.lib.nvx_resample_debug_last_launch(None, *[None] * 6) < 0
    assert not [l for l in nm.splitlines() if " U " in l and "nvx" in l]
    for path in (ROOT / "navtex_amd" / "resample").iterdir():
        text = path.read_text()
        assert "oracle" not in text and "nvxo_" not in text, path
    assert "oracle" not in HEADER.read_text() and "oracle" not in (ROOT / "navtex_amd" / "resample.py").read_text()


def test_null_and_nonsense_arguments_are_errors_never_crashes(rs, tmp_path):
    src = ROOT / "tests" / "harness" / "null_args_resample.c"
    exe = tmp_path / "null_args_resample"
    lib = ROOT / "navtex_amd"
    subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib}", "-lnavtex_amd_resample",
                    f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-lm"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "resample null-safety ok" in out.stdout, (out.stdout[-2500:], out.stderr[-500:])
    assert all(re.search(rf"\b{s}\(", src.read_text()) for s in SYMBOLS)


def test_create_returns_nodev_without_a_gpu(nv, rs):
    if nv.device_count() > 0:
        pytest.skip("a GPU is present")
    cfg = rs.Config()
    rs.lib.nvx_resample_config_default(C.byref(cfg))
    h = C.c_void_p(1)
    assert rs.lib.nvx_resample_create(C.byref(cfg), C.byref(h)) == -2
    assert h.value is None and b"no CPU path" in rs.lib.nvx_resample_last_error()
    with pytest.raises(nv.NvxError) as e:
        rs.Resampler(2400000, rs.CU8, n_streams=4)
    assert e.value.code == -2


def test_the_launch_arithmetic_against_128_bit_integers_under_asan_ubsan(tmp_path):
    """The plan's launch arithmetic (navtex_amd/resample/nvx_rs_host.h, which the down-converter bank compiles too) without
    a device: for five plans, positions up to 2^62, output counts around a tile and every chunking, the kernels' walk
    restated -- every output reached once, at its exact position and phase, inside the staged span, and the bounds the
    kernels' two divisions rely on (tests/harness/rs_launch_args.cpp).  A stand-alone program under ASan + UBSan."""
    exe = tmp_path / "rs_launch_args"
    pkg = ROOT / "navtex_amd"
    subprocess.run(["g++", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT / 'include'}", f"-I{pkg / 'csrc'}", f"-I{pkg / 'resample'}",
                    str(ROOT / "tests" / "harness" / "rs_launch_args.cpp"), "-x", "c", str(pkg / "resample" / "nvx_resample_design.c"),
                    "-o", str(exe), "-lm"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env={"ASAN_OPTIONS": "detect_leaks=1", "PATH": "/usr/bin:/bin"})
    assert out.returncode == 0 and "rs launch args ok" in out.stdout, (out.stdout + out.stderr)[-3000:]
    for rate in (2048000, 1000250, 252000, 96000, 100100):
        assert f"{rate} S/s: " in out.stdout


# ----------------------------------------------------------------------------------------------------- rates and counts
def test_rates_reduce_as_the_header_says(rs, plans):
    for fi, (L, M, T, S, taps) in plans.items():
        assert (L, M) == rr.ratio(fi) and L * fi == M * rr.OUTPUT_RATE and S == 15 and taps.shape == (L, T)
        assert T == rr.T_OF_RATE[fi] and L <= 1024 and L * T <= 32768
    assert plans[2048000][:2] == (63, 512) and plans[250000][:2] == (126, 125) and plans[96000][:2] == (21, 8)


@pytest.mark.parametrize("fi", rr.RATES + (252252, 100100))
def test_the_count_rule_against_exact_rational_arithmetic(rs, fi):
    """Random chunkings, from positions beyond 2^32 and near 2^62 too: every call's count, and the total ceil(N L / M)."""
    L, M = rr.ratio(fi)
    rng = np.random.default_rng(fi)
    for start in (0, 1, int(rng.integers(1, 1 << 20)), (1 << 32) + int(rng.integers(0, 1 << 20)), (1 << 62) - int(rng.integers(1 << 20, 1 << 30))):
        chunks = [int(c) for c in rng.choice([0, 1, 2, 7, 57, M - 1, M, M + 1, 4096, 65536, 655360], size=60)]
        want = rr.exact_counts(fi, [start] + chunks)[1:]
        pos = start
        for c, w in zip(chunks, want):
            assert rs.out_count(fi, pos, c) == w, (start, pos, c)
            pos += c
        assert sum(want) == rr.outputs_after(pos, L, M) - rr.outputs_after(start, L, M)
    if fi % 25 == 0:
        assert rs.out_count(fi, 0, fi * 8 // 25) == 80640 and rs.out_count(fi, 7 * (fi * 8 // 25), fi * 8 // 25) == 80640


@pytest.mark.parametrize("fi", [95999, 3200001, 10000000, 0, 251999, 2048001, 1260252, 2 ** 32 - 1])
def test_rates_outside_the_supported_range_are_refused(nv, rs, fi):
    assert rs.lib.nvx_resample_design(fi, None, None, None, None, None, 0) == nv._native.ERR_ARG
    assert rs.lib.nvx_resample_last_error() != b""
    assert rs.lib.nvx_resample_out_count(fi, 0, 1000) == -1
    with pytest.raises(nv.NvxError) as e:
        rs.design(fi)
    assert e.value.code == nv._native.ERR_ARG


# ------------------------------------------------------------------------------------------------------------------ taps
@pytest.mark.parametrize("fi", rr.RATES)
def test_tap_properties(plans, fi):
    L, M, T, S, taps = plans[fi]
    t = taps.astype(np.int64)
    assert taps.dtype == np.int16 and T % 2 == 0
    assert np.all(t.sum(axis=1) == 1 << S), "a phase does not sum to 2^S"
    assert np.abs(t).sum(axis=1).max() <= 65535, "the accumulator could leave int32"
    print(fi, "T", T, "largest sum of |h|", int(np.abs(t).sum(axis=1).max()))


@pytest.mark.parametrize("fi", rr.RATES)
def test_the_prototypes_response_meets_both_bars(plans, fi):
    """From the taps handed out, as the prototype at rate L fi, relative to DC: +-0.1 dB up to 25 kHz, <= -76 dB from
    min(fi, 252000) - 25000 up to L fi / 2, on a grid of 8 points per side lobe (a lobe of an N-tap window is fs / N wide)."""
    L, M, T, S, taps = plans[fi]
    fs = L * fi
    step = fs / (L * T) / 8
    stop = np.minimum(np.arange(rr.stop_edge(fi), fs / 2 + step, step), fs / 2)
    sb = rr.response_db(taps, L, fi, stop)
    pb = rr.response_db(taps, L, fi, np.linspace(0, rr.PASS_HZ, 201))
    print(fi, "worst stopband", round(float(sb.max()), 2), "dB at", int(stop[int(np.argmax(sb))]), "Hz; passband", round(float(np.abs(pb).max()), 5), "dB")
    assert np.abs(pb).max() <= rr.PASS_DB
    assert sb.max() <= rr.STOP_DB
    # the response is that of real taps: the same at -f
    assert np.allclose(rr.response_db(taps, L, fi, -stop[:64]), sb[:64], atol=1e-9)


# ----------------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("fi", rr.RATES)
def test_a_constant_returns_itself_and_the_rails_do_not_overflow(plans, fi):
    L, M, T, S, taps = plans[fi]
    n = 40 * M + 3 * T
    fill = rr.outputs_after(T - 1, L, M)                   # outputs whose window still reaches in front of the stream
    for c in (32767, -32768, 1, -1, 12345, 0):
        out = rr.resample(np.full((n, 2), c, dtype=np.int64), taps, L, M)[0]
        assert len(out) == rr.outputs_after(n, L, M) and np.all(out[fill:] == c), c
    # the worst case for every phase: each sample at the rail with its tap's sign -- the int32 assertion inside resample() holds
    rng = np.random.default_rng(fi)
    x = np.where(rng.integers(0, 2, size=(n, 2)) > 0, 32767, -32768)
    pos = np.arange(rr.outputs_after(n, L, M)) * M
    for k, r in enumerate(np.argsort(-np.abs(taps.astype(np.int64)).sum(axis=1))[:8]):      # the phases with the largest sum of |h|
        hit = np.flatnonzero((pos % L == r) & (pos // L >= (k + 1) * 2 * T))[0]
        x[pos[hit] // L - np.arange(T), :] = np.where(taps[r] >= 0, 32767, -32768)[:, None]
    out = rr.resample(x, taps, L, M)[0]
    assert out.max() == 32767 and out.min() >= -32768
    out = rr.resample(-x - 1, taps, L, M)[0]
    assert out.min() == -32768


def test_the_conversions():
    assert rr.convert(np.array([[0, 255], [127, 128]], dtype=np.uint8), rr.CU8).tolist() == [[-32640, 32640], [-128, 128]]
    assert rr.convert(np.array([[-128, 127], [0, 1]], dtype=np.int8), rr.CS8).tolist() == [[-32768, 32512], [0, 256]]
    f = np.array([[np.nan, np.inf], [-np.inf, 0.5 / 32768], [1.5 / 32768, 2.5 / 32768], [-0.5 / 32768, -1.5 / 32768], [1.0, -1.0],
                  [32767.5 / 32768, 1e-42], [3e38, -3e38]], dtype=np.float32)
    assert rr.convert(f, rr.CF32).tolist() == [[0, 32767], [-32768, 0], [2, 2], [0, -2], [32767, -32768], [32767, 0], [32767, -32768]]


def test_chunked_restatement_is_the_one_shot():
    fi = 2400000
    L, M = rr.ratio(fi)
    rng = np.random.default_rng(2)
    T = 68
    taps = rng.integers(-400, 400, size=(L, T)).astype(np.int16)
    x = rng.integers(-32768, 32768, size=(20000, 2))
    one = rr.resample(x, taps, L, M)[0]
    parts, hist, pos = [], None, 0
    for c in [0, 1, T - 2, T - 1, 1, 5000, 0, 3, 20000 - 5002 - 2 * T]:
        out, hist = rr.resample(x[pos:pos + c], taps, L, M, pos, hist)
        parts.append(out); pos += c
    assert pos == len(x) and np.array_equal(np.concatenate(parts), one)


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("fmt", [rr.CS16, rr.CU8], ids=["cs16", "cu8"])
@pytest.mark.parametrize("fi", [2048000, 250000])
def test_resample_then_decode_end_to_end_on_the_cpu(nv, rs, oracle, fi, fmt):
    """A message at +14 kHz, amplitude 8000 over noise 1500, generated at fi (for CU8 requantised to 8 bits with the
    amplitude raised threefold, the carrier spanning some ninety counts), resampled by the restatement with the plan's
    taps and decoded by the oracle: exactly that message."""
    L, M, T, S, taps = rs.design(fi)
    text = signals.stream_text(17)
    bits = nv.sitor_encode(text, 40)
    n = (len(bits) + 300) * (fi // 100)
    src = rr.to_format(rr.cpfsk(bits, fi, n, freq_hz=14000, amplitude=8000, noise_amp=1500, seed=17), fmt, gain=3.0 if fmt == rr.CU8 else 1.0)
    y = rr.resample_all(src, fmt, taps, L, M)
    assert len(y) == rr.outputs_after(n, L, M)
    ref = oracle.Pipe(chain_mask=1)
    ref.push(y[:len(y) // nv.FRAME_IN * nv.FRAME_IN])
    assert [m[2] for m in ref.messages] == [text]
