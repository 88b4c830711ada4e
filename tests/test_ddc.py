"""The down-converter bank (include/navtex_amd_ddc.h) on the CPU: the header and the companion library's exports and
argument safety, the grid rule against exact rational arithmetic, the mixer table against its generator and its symmetries,
the restatement (tests/ddc_ref.py) against the resampler's for k = 0, the mixer's spurs, and one wide input -> three slices
-> scan / tune / decode end to end through the restatements."""
import ctypes as C
import re
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import ddc_cases as cases
import ddc_ref as dr
import resample_ref as rr
import scan_ref as sr
import tune_ref as tr

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "navtex_amd_ddc.h"
PLAN = ROOT / "navtex_amd" / "ddc" / "nvx_ddc_plan.h"
SYMBOLS = ["nvx_ddc_config_default", "nvx_ddc_create", "nvx_ddc_destroy", "nvx_ddc_get_shift", "nvx_ddc_grid", "nvx_ddc_last_error",
           "nvx_ddc_plan", "nvx_ddc_position", "nvx_ddc_push", "nvx_ddc_reset", "nvx_ddc_resident", "nvx_ddc_set_shift", "nvx_ddc_table",
           "nvx_ddc_time_stats", "nvx_ddc_timing"]
HOOKS = ["nvx_ddc_debug_last_launch", "nvx_ddc_debug_set_position"]     # the tests' hooks: declared in nvx_ddc_plan.h only


def _build_if_missing():
    if not (ROOT / "navtex_amd" / "libnavtex_amd_ddc.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()


@pytest.fixture(scope="module")
def dd(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    _build_if_missing()
    import navtex_amd.ddc
    return navtex_amd.ddc


# ------------------------------------------------------------------------------------------------------------ interface
def test_header_compiles_as_plain_c_and_declares_the_entry_points(tmp_path):
    text = HEADER.read_text()
    assert sorted(set(re.findall(r"NVX_API\s+[\w\s\*]+?\b(\w+)\s*\(", text))) == SYMBOLS
    for name, want in (("NVX_DDC_OUTPUT_RATE", "252000"), ("NVX_DDC_GRID", "4096"), ("NVX_DDC_SCALE", "32767"), ("NVX_DDC_GUARD_HZ", "25000")):
        assert re.search(rf"#define {name}\s+{re.escape(want)}\b", text), name
    assert "NOT continuous across a retune" in text and "bypasses the mixer" in text
    src = tmp_path / "t.c"
    src.write_text('#include "navtex_amd_ddc.h"\nint main(void){ nvx_ddc_config c; c.format = NVX_DDC_CF32; '
                   'return NVX_DDC_CS16 == 0 && NVX_DDC_CU8 == 1 && NVX_DDC_CS8 == 2 && c.format == 3 && sizeof c == 24 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


@pytest.mark.parametrize("sym", SYMBOLS + HOOKS)
def test_symbol_is_exported(dd, sym):
    assert hasattr(dd.lib, sym), f"{sym} is declared but not exported"


def test_the_library_exports_only_its_interface_and_links_none_of_the_others(dd):
    lib = ROOT / "navtex_amd" / "libnavtex_amd_ddc.so"
    out = subprocess.run(["ldd", str(lib)], capture_output=True, text=True).stdout
    assert "libnavtex_amd" not in out and "oracle" not in out and "libamdhip64" in out
    nm = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    defined = sorted(l.split()[-1] for l in nm.splitlines() if l.split()[-2] in "TDBR" and not l.split()[-1].startswith(("_init", "_fini", "__hip", "_Z")))
    assert defined == sorted(SYMBOLS + HOOKS), defined
    assert not [l for l in nm.splitlines() if "nvx_rs_" in l or "nvx_resample" in l], "the tap design's symbols are to stay hidden"
    und = subprocess.run(["nm", "-D", "--undefined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    assert "nvx" not in und
    header, plan = HEADER.read_text(), PLAN.read_text()
    for hook in HOOKS:
        assert hook not in header and hook in plan
    assert dd.lib.nvx_ddc_debug_last_launch(None, *[None] * 8) < 0 and dd.lib.nvx_ddc_debug_set_position(None, 0, 0) < 0
    for path in (ROOT / "navtex_amd" / "ddc").iterdir():
        text = path.read_text()
        assert "oracle" not in text and "nvxo_" not in text, path
    assert "oracle" not in header and "oracle" not in (ROOT / "navtex_amd" / "ddc.py").read_text()


def test_null_and_nonsense_arguments_are_errors_never_crashes(dd, tmp_path):
    src = ROOT / "tests" / "harness" / "null_args_ddc.c"
    exe = tmp_path / "null_args_ddc"
    lib = ROOT / "navtex_amd"
    subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib}", "-lnavtex_amd_ddc",
                    f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib", "-lm"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ddc null-safety ok" in out.stdout, (out.stdout[-2500:], out.stderr[-500:])
    assert all(re.search(rf"\b{s}\(", src.read_text()) for s in SYMBOLS)


def test_create_needs_a_device_and_says_so_without_one(nv, dd):
    cfg = dd.Config()
    dd.lib.nvx_ddc_config_default(C.byref(cfg))
    h = C.c_void_p(1)
    rc = dd.lib.nvx_ddc_create(C.byref(cfg), C.byref(h))
    if nv.device_count() > 0:
        assert rc == 0 and h.value
        dd.lib.nvx_ddc_destroy(h)
        return
    assert rc == -2 and h.value is None and b"no CPU path" in dd.lib.nvx_ddc_last_error()
    with pytest.raises(nv.NvxError) as e:
        dd.Ddc(2400000, dd.CU8, n_inputs=2, n_slices=4)
    assert e.value.code == -2


# ------------------------------------------------------------------------------------------------------- grid and table
@pytest.mark.parametrize("fi", rr.RATES)
def test_the_grid_rule_against_exact_rational_arithmetic(nv, dd, fi):
    """Random requests (as the doubles they are), the exact grid points and the midpoints between them, +-range and one
    grid step beyond: k, the applied frequency, and the refusals."""
    ARG = nv._native.ERR_ARG
    rng = np.random.default_rng(fi)
    kmax = dr.k_range(fi)
    assert abs(Fraction(kmax * fi, dr.N)) <= Fraction(fi, 2) - dr.GUARD_HZ < abs(Fraction((kmax + 1) * fi, dr.N))
    reqs = [float(h) for h in rng.uniform(-fi / 2, fi / 2, size=300)]
    ks = [int(k) for k in rng.integers(-kmax - 2, kmax + 3, size=40)] + [0, 1, -1, kmax, -kmax, kmax + 1, -kmax - 1]
    reqs += [k * fi / dr.N for k in ks] + [(2 * k + 1) * fi / (2 * dr.N) for k in ks]             # grid points; midpoints (ties) where exact
    reqs += [np.nextafter((2 * k + 1) * fi / (2 * dr.N), s) for k in ks[:10] for s in (-np.inf, np.inf)]
    k, applied = C.c_int(), C.c_double()
    refused = 0
    for hz in reqs:
        want = dr.grid(fi, hz)
        rc = dd.lib.nvx_ddc_grid(fi, hz, C.byref(k), C.byref(applied))
        if want is None:
            refused += 1
            assert rc == ARG and dd.lib.nvx_ddc_last_error() != b"", hz
        else:
            assert rc == 0 and k.value == want and applied.value == want * fi / dr.N, (hz, want, k.value)
            assert abs(Fraction(hz) - Fraction(want * fi, dr.N)) <= Fraction(fi, 2 * dr.N)
    assert refused >= 2
    assert dd.grid(fi, kmax * fi / dr.N)[0] == kmax and dd.grid(fi, -kmax * fi / dr.N)[0] == -kmax
    for hz in ((kmax + 1) * fi / dr.N, -(kmax + 1) * fi / dr.N):
        with pytest.raises(nv.NvxError) as e:
            dd.grid(fi, hz)
        assert e.value.code == ARG
    if fi == 96000:
        assert kmax == 981 and kmax * fi / dr.N <= 23000.0 < (kmax + 1) * fi / dr.N      # the range at 96 kS/s is +-23 kHz


def test_the_table_equals_its_generator_and_is_symmetric(dd, tmp_path):
    w = dd.table().astype(np.int64)
    assert np.array_equal(w, dr.table()), "the library's table is not the decimal one"
    n = dr.N
    assert np.array_equal(w[(np.arange(n) + n // 2) % n], -w)
    assert np.array_equal(w[(np.arange(n) + n // 4) % n], np.stack([-w[:, 1], w[:, 0]], axis=1))
    assert np.array_equal(w[(-np.arange(n)) % n], np.stack([w[:, 0], -w[:, 1]], axis=1))
    assert w.min() == -32767 and w.max() == 32767 and w[0].tolist() == [32767, 0] and w[n // 8].tolist() == [23170, 23170]
    # the committed header is what the generator writes
    out = tmp_path / "table.h"
    subprocess.run(["python3", str(ROOT / "tools" / "gen_ddc_table.py"), str(out)], check=True)
    assert out.read_text() == (ROOT / "navtex_amd" / "ddc" / "nvx_ddc_table.h").read_text()


# ----------------------------------------------------------------------------------------------------------- restatement
def test_the_k0_restatement_is_the_resamplers(dd):
    import navtex_amd.resample as rs
    for fi, fmt in ((2400000, rr.CU8), (250000, rr.CS16)):
        L, M, T, S, taps = rs.design(fi)
        rng = np.random.default_rng(fi)
        info = np.iinfo(rr.DTYPES[fmt])
        x = rng.integers(info.min, info.max + 1, size=(30000, 2)).astype(rr.DTYPES[fmt])
        want = rr.resample_all(x, fmt, taps, L, M)
        assert np.array_equal(dr.ddc_all(x, fmt, taps, L, M, 0), want)
        # ... and in two calls, the history carried unmixed
        a, hist = dr.ddc(rr.convert(x[:12345], fmt), taps, L, M, 0)
        b, _ = dr.ddc(rr.convert(x[12345:], fmt), taps, L, M, 0, 12345, hist)
        assert np.array_equal(np.concatenate([a, b]), want)


def test_the_restatement_does_not_depend_on_the_cut_and_clamps_at_the_rails():
    fi = 2400000
    L, M = rr.ratio(fi)
    rng = np.random.default_rng(3)
    T = 68
    taps = rng.integers(-400, 400, size=(L, T)).astype(np.int16)
    x = rng.integers(-32768, 32768, size=(20000, 2))
    for k in (37, -1365):
        one = dr.ddc(x, taps, L, M, k)[0]
        parts, hist, pos = [], None, 0
        for c in [0, 1, T - 2, T - 1, 1, 5000, 0, 3, 20000 - 5002 - 2 * T]:
            out, hist = dr.ddc(x[pos:pos + c], taps, L, M, k, pos, hist)
            parts.append(out); pos += c
        assert pos == len(x) and np.array_equal(np.concatenate(parts), one)
    # both components at the rail, rotated by 45 degrees: 46340 before the clamp
    rails = np.array([[32767, 32767], [-32768, -32768], [32767, -32768], [-32768, 32767]] * 4)
    m = dr.mix(rails, 512, 1)                              # j = 512 for the first sample: 45 degrees
    assert m[0].tolist() == [32767, 0] and m.max() == 32767 and m.min() == -32768
    assert np.array_equal(dr.mix(rails, 0, 5), rails)


@pytest.mark.parametrize("amplitude", [8000, 32000])
@pytest.mark.parametrize("k", [512, -1365, 37])
def test_the_mixers_spurs_stay_below_the_front_ends_bar(k, amplitude):
    """A clean tone at 2.4 MS/s through the restated mixer alone: 2^18-point Blackman spectrum, +-64 bins around the peak
    excluded, the worst line relative to the carrier."""
    fs, n, f0 = 2400000, 1 << 18, 123456.7
    ph = 2 * np.pi * f0 / fs * np.arange(n)
    x = np.rint(amplitude * np.stack([np.cos(ph), np.sin(ph)], axis=1)).astype(np.int64)
    y = dr.mix(x, k, 0)
    spec = np.abs(np.fft.fft((y[:, 0] + 1j * y[:, 1]) * np.blackman(n)))
    peak = int(np.argmax(spec))
    want = (f0 - k * fs / dr.N) % fs
    assert abs(peak * fs / n - want) <= fs / n, "the tone did not move by k fi / N"
    keep = np.ones(n, dtype=bool)
    keep[(peak + np.arange(-64, 65)) % n] = False
    worst = 20 * np.log10(spec[keep].max() / spec[peak])
    print(f"k {k} amplitude {amplitude}: worst line {worst:.1f} dBc")
    assert worst <= -76.0


@pytest.mark.parametrize("k", [1, -1, 37, 512, -1365, dr.k_range(2400000)])
def test_the_restated_mixer_against_a_plain_rotation_in_long_double(k):
    """The restatement is exact integer arithmetic; this holds it against something that is not: (32767 / 32768) x
    e^(-2 pi i j / N) in np.longdouble on 200 000 full-scale random samples from sample 12 345 on.  Where neither component
    of the rotation comes within 68 of a rail (or beyond one), both components of dr.mix lie within 1.5 of it: 0.5 from the
    rounding shift, plus (|I| + |Q|) 0.5 / 32768 <= 1.0 from the table's rounding (each of c and s is off by at most 0.5,
    and |I|, |Q| <= 32768).  Measured: 1.282 at the worst of the six shifts (k = 2005); the bound asserted is the derived one."""
    n, first = 200000, 12345
    x = np.random.default_rng(5000 + k).integers(-32768, 32768, size=(n, 2))
    j = (k * (first + np.arange(n, dtype=np.int64))) % dr.N                  # the index reduced exactly: the angle stays below one turn
    ang = 2 * np.longdouble(np.pi) * j.astype(np.longdouble) / dr.N
    assert np.finfo(np.longdouble).eps <= 2.0 ** -52
    c, s = np.cos(ang), np.sin(ang)
    xi, xq = x[:, 0].astype(np.longdouble), x[:, 1].astype(np.longdouble)
    g = np.longdouble(32767) / np.longdouble(32768)
    want = np.stack([g * (xi * c + xq * s), g * (xq * c - xi * s)], axis=1)
    inside = np.all((want >= -32768 + 68) & (want <= 32767 - 68), axis=1)
    assert inside.sum() > n // 4
    got = dr.mix(x, k, first)
    worst = float(np.abs(got[inside].astype(np.longdouble) - want[inside]).max())
    print(f"k {k}: {int(inside.sum())} samples away from the rails, worst |mix - rotation| {worst:.3f}")
    assert worst <= 1.5


def test_every_table_index_at_the_rails_is_exact_in_32_bits():
    """The header's "the sums are exact in 32 bits": for all 4096 j and the four rail pairs of (I, Q) both mixer sums with
    their rounding constant stay below 2^31 in size, counted in Python integers from the decimal table; and the restated
    mixer gives the clamp of that exact value."""
    w = dr._table_tuple()
    assert len(w) == dr.N
    largest = 0
    for i, q in ((32767, 32767), (-32768, -32768), (32767, -32768), (-32768, 32767)):
        want = []
        for c, s in w:
            si, sq = i * c + q * s + (1 << 14), q * c - i * s + (1 << 14)
            largest = max(largest, abs(si), abs(sq))
            want.append((min(max(si >> 15, -32768), 32767), min(max(sq >> 15, -32768), 32767)))
        got = dr.mix(np.full((dr.N, 2), (i, q), dtype=np.int64), 1, 0)       # k = 1 from sample 0: j = n
        assert np.array_equal(got, np.array(want, dtype=np.int64)), (i, q)
        assert got.max() == 32767 and got.min() == -32768                    # the clamp is reached on both sides
    assert 2 ** 30 < largest < 2 ** 31, largest


def test_the_block_route_for_many_slices_is_the_restatement_slice_by_slice():
    """dr.ddc_slices, the reference of the GPU tests with thousands of slices, against dr.ddc: random taps of the 2.4 MS/s
    shape, 2 inputs x 40 slices (k = 0 and both ends of the range among them), blocks of 256 and of 7 slices."""
    fi = 2400000
    L, M = rr.ratio(fi)
    rng = np.random.default_rng(17)
    taps = rng.integers(-400, 400, size=(L, 68)).astype(np.int16)
    kmax = dr.k_range(fi)
    ks = [0, 1, -1, kmax, -kmax, 1024, 2048 - 64] + [int(k) for k in rng.integers(-kmax, kmax + 1, size=33)]
    assert len(ks) == 40
    for seed in (1, 2):
        x = np.random.default_rng(seed).integers(-32768, 32768, size=(3001, 2))
        got = dr.ddc_slices(x, taps, L, M, ks)
        assert got.dtype == np.int16 and got.shape == (40, rr.outputs_after(3001, L, M), 2)
        for s, k in enumerate(ks):
            assert np.array_equal(got[s], dr.ddc(x, taps, L, M, k)[0]), (seed, s, k)
        assert np.array_equal(dr.ddc_slices(x, taps, L, M, ks, block=7), got)
        assert len({got[s].tobytes() for s in range(40)}) == 40


# ------------------------------------------------------------------------------------------------------------ end to end
def test_one_wide_input_three_stations_end_to_end_on_the_cpu(nv, dd, oracle):
    """One 2.4 MS/s unsigned 8-bit input holds three stations with different texts (tests/ddc_cases.py); three slices
    shifted to -400 000, 0 and +612 345 Hz bring each to +-14 kHz plus the grid's residue.  Slice 1 (k = 0) is decoded by
    the oracle as it stands, slice 0 tuned to +14 kHz plus its residue, and slice 2's carrier is found by the restated scan
    and nvx_scan_find within 5 Hz of -14 kHz plus the residue nvx_ddc_grid reported, then decoded tuned to what was found."""
    import navtex_amd.scan as sc
    (_, frames), (ys, ks, residues) = cases.source(), cases.slices()
    texts = [t for _, _, t in cases.STATIONS]
    assert ys.shape == (3, frames * nv.FRAME_IN, 2) and ks == (-683, 0, 1045)
    assert residues[1] == 0.0 and abs(residues[0]) > 100.0                  # slice 0 needs the tuned chain: 195 Hz off
    ref = oracle.Pipe(chain_mask=1)
    ref.push(ys[1])
    assert [m[2] for m in ref.messages] == [texts[1]]
    y1 = tr.front(ys[0], False)
    assert tr.messages(tr.decode(tr.chain(y1, 0, tr.k_of(14000 + residues[0])))) == [texts[0]]
    y1 = tr.front(ys[2], False)
    hits = sc.find(sr.power_row(y1, 0, 3))
    assert hits and abs(hits[0]["offset_hz"] - (-14000 + residues[2])) <= 5.0, (hits[:2], residues[2])
    assert tr.messages(tr.decode(tr.chain(y1, 0, tr.k_of(hits[0]["offset_hz"])))) == [texts[2]]
