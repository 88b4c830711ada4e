"""The band scan (include/navtex_amd_scan.h) on the CPU: the header and the companion library's exports and argument
safety, the generated twiddle table, the restatement's transform against numpy's FFT, the detector in C against the
restatement (tests/scan_ref.py), the detection cases, and scan -> tune -> decode end to end through the restatements.

The synthetic streams here keep noise_amp > 0.  With noise_amp 0 the generator's own spurs at multiples of 1 kHz, 34 dB
below a carrier, are real lines above an empty floor, and the detector finds them: that is the generator, not a fault."""
import ctypes as C
import re
import subprocess
from decimal import Decimal, getcontext
from pathlib import Path

import numpy as np
import pytest

import scan_ref as sr
import signals
import tune_ref as tr

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "navtex_amd_scan.h"
SYMBOLS = ["nvx_scan_find", "nvx_scan_iq", "nvx_scan_last_error", "nvx_scan_params_default", "nvx_scan_resident",
           "nvx_scan_set_form", "nvx_scan_time_stats", "nvx_scan_timing"]
HOOK = "nvx_scan_debug_last_launch"        # the tests' one hook: declared in nvx_scan_kernels.h, not in the public header


@pytest.fixture(scope="module")
def sc(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_scan.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.scan
    return navtex_amd.scan


# ------------------------------------------------------------------------------------------------------------ interface
def test_header_compiles_as_plain_c_and_declares_the_entry_points(tmp_path):
    text = HEADER.read_text()
    assert sorted(set(re.findall(r"NVX_API\s+[\w\s\*]+?\b(\w+)\s*\(", text))) == SYMBOLS
    for name, want in (("NVX_SCAN_FFT", "2048"), ("NVX_SCAN_BIN_HZ", "30.76171875"), ("NVX_SCAN_SLOTS_PER_FRAME", "9")):
        assert re.search(rf"#define {name}\s+{re.escape(want)}\b", text), name
    src = tmp_path / "t.c"
    src.write_text('#include "navtex_amd_scan.h"\nint main(void){ return NVX_SCAN_FFT * NVX_SCAN_BIN_HZ == 63000.0 && '
                   'NVX_SCAN_SLOTS_PER_FRAME * NVX_SCAN_SLOT_OUTPUTS == 20160 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


@pytest.mark.parametrize("sym", SYMBOLS + [HOOK])
def test_symbol_is_exported(sc, sym):
    assert hasattr(sc.lib, sym), f"{sym} is declared in navtex_amd_scan.h but not exported"


def test_the_companion_links_neither_the_product_library_nor_test_infrastructure(sc):
    out = subprocess.run(["ldd", str(ROOT / "navtex_amd" / "libnavtex_amd_scan.so")], capture_output=True, text=True).stdout
    assert "libnavtex_amd.so" not in out and "oracle" not in out and "libamdhip64" in out


def test_the_hook_is_internal_and_the_library_defines_nothing_else(sc):
    nm = subprocess.run(["nm", "-D", str(ROOT / "navtex_amd" / "libnavtex_amd_scan.so")], capture_output=True, text=True, check=True).stdout
    defined = sorted(l.split()[-1] for l in nm.splitlines() if " T " in l and "nvx_" in l)
    assert defined == sorted(SYMBOLS + [HOOK]) and HOOK not in HEADER.read_text()
    assert HOOK in (ROOT / "navtex_amd" / "scan" / "nvx_scan_kernels.h").read_text()
    assert sc.lib.nvx_scan_debug_last_launch(None, None, None, None) >= 0 and set(sc.debug_last_launch()) == {"launches", "form", "grid", "scratch_bytes"}


def test_null_and_nonsense_arguments_are_errors_never_crashes(sc, tmp_path):
    src = ROOT / "tests" / "harness" / "null_args_scan.c"
    exe = tmp_path / "null_args_scan"
    lib = ROOT / "navtex_amd"
    subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib}", "-lnavtex_amd_scan",
                    f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-lm"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "scan null-safety ok" in out.stdout, (out.stdout[-2500:], out.stderr[-500:])
    assert all(re.search(rf"\b{s}\(", src.read_text()) for s in SYMBOLS + [HOOK])


def test_device_entry_points_return_nodev_without_a_gpu(nv, sc):
    if nv.device_count() > 0:
        pytest.skip("a GPU is present")
    iq = np.zeros((nv.FRAME_IN, 2), dtype=np.int16)
    row = np.zeros(sc.FFT)
    used = C.c_int(-1)
    assert sc.lib.nvx_scan_iq(0, iq.ctypes.data_as(C.c_void_p), iq.shape[0], 0, 1, row.ctypes.data_as(C.c_void_p), C.byref(used)) == -2
    assert used.value == -1 and b"no CPU path" in sc.lib.nvx_scan_last_error()
    assert sc.lib.nvx_scan_resident(0, C.c_void_p(0x100000), nv.FRAME_IN, 0, 1, 1, 0, 1, C.c_void_p(0x200000), None) == -2
    with pytest.raises(nv.NvxError) as e:
        sc.scan_iq(iq, False)
    assert e.value.code == -2


# ---------------------------------------------------------------------------------------------------------------- table
def test_the_table_is_the_generator_output(tmp_path):
    out = tmp_path / "t.h"
    subprocess.run(["python3", str(ROOT / "tools" / "gen_scan_table.py"), str(out)], check=True)
    assert out.read_text() == sr.HEADER.read_text()


def test_octant_is_correctly_rounded_against_decimal():
    """Every stored value is within half an ulp of cos / sin evaluated in decimal at 70 digits, by a code path of its own."""
    getcontext().prec = 70

    def atan_inv(x):
        total = term = Decimal(1) / x
        k, x2 = 1, x * x
        while True:
            term /= -x2
            nxt = total + term / (2 * k + 1)
            if nxt == total:
                return total
            total, k = nxt, k + 1
    pi = 4 * (4 * atan_inv(5) - atan_inv(239))
    oc = sr.octant()
    assert len(oc) == 257 and oc[0] == (1.0, 0.0) and oc[256][0] == oc[256][1]
    for j, (c, s) in enumerate(oc):
        x = 2 * pi * j / sr.N
        cs, ss, term, n = Decimal(1), Decimal(0), Decimal(1), 0
        while True:
            n += 1
            term = term * x / n
            if term == 0 or abs(term) < Decimal(10) ** -68:
                break
            if n % 2:
                ss += term if n % 4 == 1 else -term
            else:
                cs += term if n % 4 == 0 else -term
        for got, exact in ((c, cs), (s, ss)):
            ulp = np.spacing(abs(got)) if got != 0 else np.spacing(0.0)
            assert abs(Decimal(got) - exact) <= Decimal(float(ulp)) / 2, (j, got, exact)


def test_the_full_turn_follows_by_exact_symmetries():
    c, s = sr.table()
    n, q = sr.N, sr.N // 4
    j = np.arange(n)
    assert c[0] == 1.0 and s[0] == 0.0 and c[q] == 0.0 and s[q] == 1.0 and c[2 * q] == -1.0 and s[2 * q] == 0.0 and s[3 * q] == -1.0
    assert np.array_equal(c[(n - j) % n], c) and np.array_equal(s[(n - j) % n], -s)
    assert np.array_equal(c[(j + 2 * q) % n], -c) and np.array_equal(s[(j + 2 * q) % n], -s)
    assert np.array_equal(c[(q - j) % n], s)
    assert np.max(np.abs(c - np.cos(2 * np.pi * j / n))) < 2e-15 and np.max(np.abs(s - np.sin(2 * np.pi * j / n))) < 2e-15     # libm on a rounded argument
    # the window the header states: one rounding
    w = 0.5 - 0.5 * c
    assert w[0] == 0.0 and w[1024] == 1.0 and np.array_equal(w[1:], w[:0:-1])


# ------------------------------------------------------------------------------------------------- transform restatement
FFT_MEASURED = 3.4e-16          # the worst max|X - numpy.fft(x)| / max|X| seen on the inputs below (real segments: 1.9e-16)


def test_the_restated_transform_is_numpys_fft(nv):
    """The explicit radix-2 stages against numpy.fft.fft (pocketfft: other factorisation, other twiddles), on windowed
    segments of real FIR1 output and on full-scale random input.  Measured: 1.9e-16 (segments) and 3.3e-16 (random) of the
    largest bin -- a 2048-point transform in fp64, eleven stages of rounding at 1.1e-16 each, errors adding like a random
    walk -- asserted with a fourfold margin."""
    st, _ = signals.stream_params(nv, 3, nv.RATE_IN)
    iq = nv.synth_host(st, nv.RATE_IN, 2 * nv.FRAME_IN)
    xr, xi = sr.window(sr.segments(sr.front(iq, False), 0, 2))
    rng = np.random.default_rng(7)
    z = rng.integers(-32768, 32768, size=(16, sr.N, 2)).astype(np.float64)
    for name, (ar, ai) in (("segments", (xr, xi)), ("random", (z[..., 0], z[..., 1]))):
        fr, fi = sr.fft(ar, ai)
        ref = np.fft.fft(ar + 1j * ai, axis=-1)
        dev = np.max(np.abs((fr + 1j * fi) - ref)) / np.max(np.abs(ref))
        print(name, "worst relative deviation", dev)
        assert dev <= 4 * FFT_MEASURED, (name, dev)


@pytest.mark.parametrize("f0", [1, 2])
@pytest.mark.parametrize("raw,s0", [(True, 1), (True, 3), (False, 1)], ids=["raw", "raw-cic3", "252k"])
def test_the_restatement_on_a_cut_is_the_restatement_on_the_whole_stream(nv, raw, s0, f0):
    """The header's lead-in claim, which the GPU tests of long rows lean on: frames [f0, f0 + 2) restated from the samples
    of those frames alone equal, word for word, the same frames restated from the stream's reset -- with full-scale noise
    in front of the cut and behind it, so that anything the filters carried across a frame's first sample would show."""
    frame = nv.FRAME_RAW if raw else nv.FRAME_IN
    rate = nv.RATE_RAW if raw else nv.RATE_IN
    rng = np.random.default_rng(100 * f0 + s0 + raw)
    st, _ = signals.stream_params(nv, 31 + f0, rate, freq_hz=-7001)
    iq = rng.integers(-32768, 32768, size=((f0 + 3) * frame, 2)).astype(np.int16)
    iq[f0 * frame:(f0 + 2) * frame] = nv.synth_host(st, rate, 2 * frame, f0 * frame)
    whole = sr.power_row(sr.front(iq, raw, s0), f0, 2)
    cut = sr.power_row_of_cut(iq[f0 * frame:], raw, s0, 2)
    assert whole.any() and np.array_equal(whole.view(np.uint64), cut.view(np.uint64))
    for k in (0, 1):                                                 # and frame by frame
        one = sr.power_row_of_cut(iq[(f0 + k) * frame:], raw, s0, 1)
        assert np.array_equal(one.view(np.uint64), sr.power_row(sr.front(iq, raw, s0), f0 + k, 1).view(np.uint64))


def test_a_synthetic_carrier_at_plus_14000_lands_at_plus_14000(nv):
    """The sign convention: row index i is (i - 1024) * 30.76 Hz with the sign of the generator's freq_hz and
    nvx_set_carrier's offset_hz."""
    for f in (14000, -14000):
        st, _ = signals.stream_params(nv, 1, nv.RATE_IN, freq_hz=f)
        p = sr.scan(nv.synth_host(st, nv.RATE_IN, nv.FRAME_IN), False)
        assert abs((int(np.argmax(p)) - 1024) * sr.BIN_HZ - f) < 100 + sr.BIN_HZ


# --------------------------------------------------------------------------------------------------------------- signals
CARRIERS = (14000, -14000, 1000, -5003, 19012)


def _multi(nv, rate, frames, carriers, amplitudes, noise_amp=1500, seed=21):
    car = [dict(freq_hz=f, bits=nv.sitor_encode(signals.stream_text(10 + i), 40), bit_offset=(37 * i + 11) % (rate // 100),
                phase0=977 * i + 5, amplitude=a) for i, (f, a) in enumerate(zip(carriers, amplitudes))]
    frame = nv.FRAME_RAW if rate == nv.RATE_RAW else nv.FRAME_IN
    return nv.synth_host(nv.make_stream(car, seed=seed, noise_amp=noise_amp), rate, frames * frame)


def _noise(nv, rate, frames, seed):
    frame = nv.FRAME_RAW if rate == nv.RATE_RAW else nv.FRAME_IN
    return nv.synth_host(nv.make_stream([], seed=seed, noise_amp=1500), rate, frames * frame)


def _same_hits(c_hits, ref_hits):
    assert len(c_hits) == len(ref_hits) and [h["bin"] for h in c_hits] == [h["bin"] for h in ref_hits]
    for a, b in zip(c_hits, ref_hits):
        for k in ("offset_hz", "score_db", "shift_hz", "band_power_db"):
            assert abs(a[k] - b[k]) <= 1e-9 * max(1.0, abs(b[k])), (k, a, b)


@pytest.mark.parametrize("amplitude", [8000, 200])
@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("raw,s0", [(True, 1), (True, 3), (False, 1)], ids=["raw", "raw-cic3", "252k"])
def test_five_carriers_are_found_within_5_hz(nv, sc, raw, s0, frames, amplitude):
    iq = _multi(nv, nv.RATE_RAW if raw else nv.RATE_IN, frames, CARRIERS, [amplitude] * 5)
    row = sr.scan(iq, raw, s0)
    hits = sc.find(row)
    _same_hits(hits, sr.find(row))
    assert len(hits) == 5, hits
    assert [h["score_db"] for h in hits] == sorted((h["score_db"] for h in hits), reverse=True)
    for f in CARRIERS:
        h = min(hits, key=lambda x: abs(x["offset_hz"] - f))
        print(raw, s0, frames, amplitude, f, round(h["offset_hz"] - f, 2), round(h["shift_hz"], 1), round(h["score_db"], 1))
        assert abs(h["offset_hz"] - f) <= 5.0 and abs(h["shift_hz"] - 170.0) <= 15.0, (f, h)
        assert abs((h["bin"] - 1024) * sr.BIN_HZ - f) <= 13 * sr.BIN_HZ


def test_noise_silence_and_dc_give_no_hits(nv, sc):
    for raw in (False, True):
        rate = nv.RATE_RAW if raw else nv.RATE_IN
        for seed in range(4):
            for frames in (1, 3):
                row = sr.scan(_noise(nv, rate, frames, 100 + seed), raw)
                assert sc.find(row) == [] and sr.find(row) == [], (raw, seed, frames)
        silent = np.zeros(((nv.FRAME_RAW if raw else nv.FRAME_IN), 2), dtype=np.int16)
        row = sr.scan(silent, raw)
        assert not row.any() and sc.find(row) == [] and sr.find(row) == []
        # a DC offset on top of the noise: the strongest line of the row, at the centre, and no station
        for frames in (1, 3):
            dc = (_noise(nv, rate, frames, 5).astype(np.int32) + np.array([3000, -2000])).astype(np.int16)
            row = sr.scan(dc, raw)
            assert abs(int(np.argmax(row)) - 1024) <= 1
            assert sc.find(row) == [] and sr.find(row) == [], (raw, frames)


def test_a_carrier_at_the_centre_is_not_taken_for_a_dc_offset(nv, sc):
    row = sr.scan(_multi(nv, nv.RATE_IN, 1, [0], [8000]), False)
    hits = sc.find(row)
    assert len(hits) == 1 and abs(hits[0]["offset_hz"]) <= 5.0 and abs(hits[0]["shift_hz"] - 170.0) <= 15.0, hits


@pytest.mark.parametrize("sep", [500, -500])
@pytest.mark.parametrize("frames", [1, 3])
def test_neighbours(nv, sc, sep, frames):
    """A carrier 20 dB below a neighbour 500 Hz away is found; 26 dB or more below it may be missing (the neighbour's own
    side lobes are as strong there), but nothing spurious appears."""
    row = sr.scan(_multi(nv, nv.RATE_IN, frames, [3000, 3000 + sep], [8000, 800], seed=9), False)
    hits = sc.find(row)
    _same_hits(hits, sr.find(row))
    assert len(hits) == 2 and abs(hits[0]["offset_hz"] - 3000) <= 5.0 and abs(hits[1]["offset_hz"] - (3000 + sep)) <= 5.0, hits
    for amp in (401, 253, 80):                       # 26, 30 and 40 dB below
        row = sr.scan(_multi(nv, nv.RATE_IN, frames, [3000, 3000 + sep], [8000, amp], seed=9), False)
        hits = sc.find(row)
        _same_hits(hits, sr.find(row))
        assert 1 <= len(hits) <= 2 and abs(hits[0]["offset_hz"] - 3000) <= 5.0, (amp, hits)
        assert all(min(abs(h["offset_hz"] - 3000), abs(h["offset_hz"] - 3000 - sep)) <= 5.0 for h in hits), (amp, hits)


def test_detector_in_c_is_the_restatement_on_awkward_rows(sc):
    """Rows that are no spectra: random powers with planted lines, ties, zeros among the neighbours of a peak, a peak on
    the wrap-around, parameters away from the defaults."""
    rng = np.random.default_rng(3)
    rows = []
    for k in range(12):
        row = rng.exponential(1.0, sr.N)
        for _ in range(k):
            c = int(rng.integers(0, sr.N))
            row[(c - 3) % sr.N] += 10.0 ** rng.uniform(1, 5)
            row[(c + 3) % sr.N] += 10.0 ** rng.uniform(1, 5)
        rows.append(row)
    flat = np.ones(sr.N); flat[[2, 8, 2040, 2046]] = 500.0; rows.append(flat)                    # ties, and a pair across the wrap
    sparse = np.zeros(sr.N); sparse[::2] = 1.0; sparse[[700, 706]] = 1e4; rows.append(sparse)     # zeros beside the tones
    for row in rows:
        _same_hits(sc.find(row), sr.find(row))
        p = sc.default_params()
        p.band_half, p.floor_half, p.guard_bins, p.min_score_db, p.max_offset_hz, p.refine_iters = 3, 20, 8, 4.0, 31000.0, 2
        _same_hits(sc.find(row, p), sr.find(row, band_half=3, floor_half=20, guard_bins=8, min_score_db=4.0, max_offset_hz=31000.0, refine_iters=2))
    many = rows[11]
    assert len(sc.find(many, cap=2)) == 2 and sc.lib.nvx_scan_find(many.ctypes.data_as(C.c_void_p), None, None, 0) == len(sr.find(many)) > 2


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("freq_hz", [1000, -5003])
def test_scan_tune_decode_end_to_end_on_the_cpu(nv, sc, freq_hz):
    """scan -> k_of(offset) -> the tuned chain -> decode -> the transmitted message, all through the restatements; the same
    signal through the nominal mixer gives no message."""
    text = "ZCZC SC01\nFOUND BY THE BAND SCAN\nNNNN\n"
    st, _ = signals.stream_params(nv, 5, nv.RATE_IN, freq_hz=freq_hz, text=text)
    iq = nv.synth_host(st, nv.RATE_IN, 40 * nv.FRAME_IN)
    y1 = tr.front(iq, False)
    hits = sc.find(sr.power_row(y1, 0, 3))
    assert len(hits) == 1 and abs(hits[0]["offset_hz"] - freq_hz) <= 5.0, hits
    k = tr.k_of(hits[0]["offset_hz"])
    assert abs(k * tr.STEP_HZ - freq_hz) <= 5.0 + tr.STEP_HZ / 2
    assert tr.messages(tr.decode(tr.chain(y1, 0, k))) == [text]
    assert tr.messages(tr.decode(tr.chain(y1, 0, tr.NOMINAL[0]))) == []
