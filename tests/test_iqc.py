"""The IQ corrector (include/navtex_amd_iqc.h) on the CPU: the header and the companion library's exports and argument
safety, the launch arithmetic against 128-bit integers (a stand-alone program under ASan + UBSan), the restatement
(tests/iqc_ref.py) on cuts at the block ends, the identity, the four rejection reasons and the rails, the cut plan of the GPU
suite's block-end sweep (tests/test_gpu_iqc_edges.py) against a model of the kernels' tiles, and end to end through the
oracle: the acceptance case (a weak 490 station under the image of a strong 518 one, twelve seeds), the image of a tone
before and behind the corrector, and the known limit -- two strong stations at mirrored frequencies."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import iqc_cases as ic
import iqc_ref as ir
import resample_ref as rr

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "navtex_amd_iqc.h"
PLAN = ROOT / "navtex_amd" / "iqc" / "nvx_iqc_plan.h"
SYMBOLS = ["nvx_iqc_config_default", "nvx_iqc_create", "nvx_iqc_destroy", "nvx_iqc_get", "nvx_iqc_last_error", "nvx_iqc_plan", "nvx_iqc_position",
           "nvx_iqc_push", "nvx_iqc_reset", "nvx_iqc_resident", "nvx_iqc_set", "nvx_iqc_set_mode", "nvx_iqc_time_stats", "nvx_iqc_timing"]
HOOKS = ["nvx_iqc_debug_last_launch", "nvx_iqc_debug_set_position"]
B = ir.BLOCK


@pytest.fixture(scope="module")
def iq(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_iqc.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.iqc
    return navtex_amd.iqc


# ------------------------------------------------------------------------------------------------------------ interface
def test_header_compiles_as_plain_c_and_declares_the_entry_points(tmp_path):
    text = HEADER.read_text()
    assert sorted(set(re.findall(r"NVX_API\s+[\w\s\*]+?\b(\w+)\s*\(", text))) == SYMBOLS
    for name, want in (("NVX_IQC_BLOCK", "65536"), ("NVX_IQC_WINDOW_LOG2_DEFAULT", "4"), ("NVX_IQC_CQ_IDENTITY", "16384"), ("NVX_IQC_CQ_MIN", "12288"),
                       ("NVX_IQC_CQ_MAX", "21845"), ("NVX_IQC_CI_MAX", "5462"), ("NVX_IQC_TRACK", "0"), ("NVX_IQC_HOLD", "1")):
        assert re.search(rf"#define {name}\s+{re.escape(want)}\b", text), name
    assert "Known limit" in text and "IQ-correct -> blank -> DDC / resample -> scan -> tune -> decode" in text
    src = tmp_path / "t.c"
    src.write_text('#include "navtex_amd_iqc.h"\nint main(void){ nvx_iqc_config c; nvx_iqc_status s; c.format = NVX_IQC_CF32; s.sums[4] = 0; '
                   'return NVX_IQC_CS16 == 0 && NVX_IQC_CU8 == 1 && NVX_IQC_CS8 == 2 && c.format == 3 && sizeof c == 20 && sizeof s == 88 && !s.sums[4] ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


@pytest.mark.parametrize("sym", SYMBOLS + HOOKS)
def test_symbol_is_exported(iq, sym):
    assert hasattr(iq.lib, sym), f"{sym} is declared but not exported"


def test_the_companion_links_no_other_library_of_the_project_and_no_test_infrastructure(iq):
    lib = ROOT / "navtex_amd" / "libnavtex_amd_iqc.so"
    out = subprocess.run(["ldd", str(lib)], capture_output=True, text=True).stdout
    assert "libnavtex_amd" not in out and "oracle" not in out and "libamdhip64" in out
    # it defines nothing but its own interface and the tests' two hooks, and needs no nvx_ symbol from elsewhere
    nm = subprocess.run(["nm", "-D", str(lib)], capture_output=True, text=True, check=True).stdout
    defined = sorted(l.split()[-1] for l in nm.splitlines() if " T " in l and "nvx_" in l)
    assert defined == sorted(SYMBOLS + HOOKS) and all(d.startswith("nvx_iqc_") for d in defined)
    assert not [h for h in HOOKS if h in HEADER.read_text()] and all(h in PLAN.read_text() for h in HOOKS)
    assert iq.lib.nvx_iqc_debug_last_launch(None, None, None, None, None) < 0 and iq.lib.nvx_iqc_debug_set_position(None, 0, 0) < 0
    assert not [l for l in nm.splitlines() if " U " in l and "nvx" in l]
    for path in (ROOT / "navtex_amd" / "iqc").iterdir():
        text = path.read_text()
        assert "oracle" not in text and "nvxo_" not in text, path
    assert "oracle" not in HEADER.read_text() and "oracle" not in (ROOT / "navtex_amd" / "iqc.py").read_text()
    assert C.sizeof(iq.Config) == 20 and C.sizeof(iq.Status) == 88


def test_null_and_nonsense_arguments_are_errors_never_crashes(iq, tmp_path):
    src = ROOT / "tests" / "harness" / "null_args_iqc.c"
    exe = tmp_path / "null_args_iqc"
    lib = ROOT / "navtex_amd"
    subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib}", "-lnavtex_amd_iqc",
                    f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "iqc null-safety ok" in out.stdout, (out.stdout[-2500:], out.stderr[-500:])
    assert all(re.search(rf"\b{s}\(", src.read_text()) for s in SYMBOLS)


def test_create_returns_nodev_without_a_gpu_and_refuses_bad_parameters_first(nv, iq):
    if nv.device_count() > 0:
        pytest.skip("a GPU is present")
    cfg = iq.Config()
    iq.lib.nvx_iqc_config_default(C.byref(cfg))
    h = C.c_void_p(1)
    assert iq.lib.nvx_iqc_create(C.byref(cfg), C.byref(h)) == -2
    assert h.value is None and b"no CPU path" in iq.lib.nvx_iqc_last_error()
    with pytest.raises(nv.NvxError) as e:
        iq.Corrector(iq.CU8, n_streams=4)
    assert e.value.code == -2
    for kw in (dict(window_log2=0), dict(window_log2=3), dict(window_log2=8), dict(format=4), dict(format=-1), dict(n_streams=0), dict(n_streams=65536)):
        with pytest.raises(nv.NvxError) as e:
            iq.Corrector(**kw)
        assert e.value.code == nv._native.ERR_ARG, kw


def test_the_launch_arithmetic_against_128_bit_integers_under_asan_ubsan(tmp_path):
    """nvx_iqc_fill_args (navtex_amd/iqc/nvx_iqc_plan.h) without a device: positions up to 2^62, call lengths around a tile, a
    block and a chunk, every chunking and window -- each sample in one tile of one chunk and in the block the kernels take it
    for, a record for every block, the ring slot, 16-byte stores only on aligned rows (tests/harness/iqc_launch_args.cpp).
    A stand-alone program under ASan + UBSan."""
    exe = tmp_path / "iqc_launch_args"
    pkg = ROOT / "navtex_amd"
    subprocess.run(["g++", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT / 'include'}", f"-I{pkg / 'csrc'}", f"-I{pkg / 'iqc'}",
                    str(ROOT / "tests" / "harness" / "iqc_launch_args.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env={"ASAN_OPTIONS": "detect_leaks=1", "PATH": "/usr/bin:/bin"})
    assert out.returncode == 0 and "iqc launch args ok" in out.stdout, (out.stdout + out.stderr)[-3000:]


# ----------------------------------------------------------------------------------------------------------- restatement
def _cut_everywhere(x, fmt, window_log2, one):
    """One shot == cuts at 0, 1, 65 535, 65 536, 65 537 and mid-block, in this order and in two others."""
    n = len(x)
    rng = np.random.default_rng(n)
    for trial in range(3):
        cuts = [0, 1, B - 1, B, B + 1, 30000]
        rest = n - sum(cuts)
        while rest:
            cut = int(min(rest, rng.choice([0, 1, B - 1, B, B + 1, int(rng.integers(1, 3 * B))])))
            cuts.append(cut); rest -= cut
        if trial:
            rng.shuffle(cuts)
        c = ir.Corrector(fmt, window_log2)
        pos, parts = 0, []
        for cut in cuts:
            parts.append(c.push(x[pos:pos + cut])); pos += cut
        assert pos == n and np.array_equal(np.concatenate(parts), one[0]), trial
        assert (c.coef, c.reason, c.sums(), c.samples, c.solved, c.rejected, c.history) == \
               (one[1].coef, one[1].reason, one[1].sums(), n, one[1].solved, one[1].rejected, one[1].history)


@pytest.mark.parametrize("window_log2,blocks", [(2, 9.4), (4, 19.2)])
def test_one_shot_equals_cuts_at_the_block_ends(window_log2, blocks):
    x = ic.impaired_noise(int(blocks * B), 3 + window_log2)
    one = ir.correct(x, ir.CS16, window_log2)
    assert one[1].solved == int(blocks) - (1 << window_log2) + 1 and len({h[1] for h in one[1].history}) == one[1].solved
    _cut_everywhere(x, ir.CS16, window_log2, one)


def test_the_identity_until_the_window_is_full_and_the_solve_behind_it():
    x = ic.impaired_noise(6 * B, 5)
    out, ref = ir.correct(x, ir.CS16, 2)
    assert np.array_equal(out[:4 * B], x[:4 * B]) and not np.array_equal(out[4 * B:4 * B + 100], x[4 * B:4 * B + 100])
    assert [h[0] for h in ref.history] == [4, 5] and all(h[2] == 0 for h in ref.history)
    dI, dQ, c_i, c_q = ref.history[0][1]
    # the impairment's own numbers: the offsets, -tan(3 deg), 1 / (1.05 cos(3 deg))
    assert abs(dI - ic.DC_I) < 40 and abs(dQ - ic.DC_Q) < 40
    assert abs(c_i / 16384 + np.tan(np.deg2rad(3.0))) < 0.004 and abs(c_q / 16384 - 1 / (1.05 * np.cos(np.deg2rad(3.0)))) < 0.004
    assert ir.solve(ref.sums(), 2) == ir.solve(tuple(np.int64(v) for v in ref.sums()), 2)


@pytest.mark.parametrize("fmt", [ir.CS16, ir.CU8, ir.CS8, ir.CF32])
def test_bypass_is_the_conversion(fmt):
    """HOLD from the first sample: the identity throughout, and the identity is the conversion word for word."""
    rng = np.random.default_rng(fmt)
    n = 5 * B + 9
    if fmt == ir.CF32:
        x = rng.uniform(-1.3, 1.3, size=(n, 2)).astype(np.float32)
        x[:6, 0] = [np.nan, np.inf, -np.inf, 0.5 / 32768, 1.5 / 32768, 1e-42]
    else:
        info = np.iinfo(rr.DTYPES[fmt])
        x = rng.integers(info.min, info.max + 1, size=(n, 2)).astype(rr.DTYPES[fmt])
    c = ir.Corrector(fmt, 2)
    c.set_mode(ir.HOLD)
    out = c.push(x)
    assert np.array_equal(out, rr.convert(x, fmt).astype(np.int16)) and (c.samples, c.solved, c.rejected, c.coef) == (n, 0, 0, ir.IDENTITY)
    assert np.array_equal(ir.pack(out).view(np.int16).reshape(-1, 2), out)
    conv = rr.convert(x, fmt)
    assert c.sums() == tuple(int(v) for v in ir.block_sums(conv[B:5 * B]))


def test_silence_is_too_little_signal_and_its_offset_goes_all_the_same():
    n = 6 * B
    out, ref = ir.correct(ic.silence_with_dc(n), ir.CS16, 2)
    assert ref.reason == 1 and ref.rejected == 2 and ref.solved == 0 and ref.coef == (ic.DC_I, ic.DC_Q, 0, 16384)
    assert not out[4 * B:].any() and (out[:4 * B] == (ic.DC_I, ic.DC_Q)).all()
    for fmt, z in ((ir.CU8, 128), (ir.CS8, 0), (ir.CF32, 0.0)):
        _, ref = ir.correct(np.full((5 * B, 2), z, dtype=rr.DTYPES[fmt]), fmt, 2)
        assert ref.reason == 1 and ref.coef[2:] == (0, 16384), fmt


def test_the_rejection_reasons_two_and_four():
    n = 5 * B + 100
    out, ref = ir.correct(ic.q_equals_i(n, 61), ir.CS16, 2)
    assert ref.reason == 2 and ref.rejected == 2 and ref.coef[2:] == (0, 16384)
    x = ic.q_three_i_rotated(n, 62)
    out, ref = ir.correct(x, ir.CS16, 2)
    assert ref.reason == 4 and ref.rejected == 2 and ref.coef[2:] == (0, 16384)
    dI, dQ = ref.history[0][1][:2]                           # the offset goes all the same
    assert np.array_equal(out[4 * B:5 * B], x[4 * B:5 * B].astype(np.int64) - (dI, dQ)) and np.array_equal(out[:4 * B], x[:4 * B])
    # unrotated, three times the level is reason 2: the coherence comes first
    i = x[:, 0]
    assert ir.correct(np.stack([i, 3 * (i // 3)], axis=1).astype(np.int16), ir.CS16, 2)[1].reason == 2


def test_reason_three_what_is_left_of_q_is_not_positive():
    """I = 5 i, Q = i: a = -1/5 passes step 7, and v = CQQ + 2 a CIQ + a^2 CII is nothing but rounding: reason 3, the identity
    gain, the offset removed all the same."""
    n = 5 * B + 100
    x = ic.q_fifth_of_i(n, 63)
    out, ref = ir.correct(x, ir.CS16, 2)
    assert ref.reason == 3 and ref.rejected == 2 and ref.solved == 0 and ref.coef[2:] == (0, 16384)
    assert [h[2] for h in ref.history] == [3, 3]
    dI, dQ = ref.history[0][1][:2]
    assert np.array_equal(out[4 * B:5 * B], x[4 * B:5 * B].astype(np.int64) - (dI, dQ)) and np.array_equal(out[:4 * B], x[:4 * B])
    for y in (x * (1, -1), np.stack([8 * (x[:, 1] // 2), x[:, 1] // 2], axis=1)):            # Q = -i; I = 8 i
        assert ir.correct(y.astype(np.int16), ir.CS16, 2)[1].reason == 3
    assert ir.correct(ic.q_fifth_of_i(17 * B + 100, 63), ir.CS16, 4)[1].history[-1][2] == 3


# ------------------------------------------------------------------------------------ the block-end sweep's cut plan
def test_the_tile_model_against_the_blocks_sample_by_sample():
    """iqc_cases.block_ends_in_tiles against the header's definition taken literally: sample k of a call at `position` lies
    in block (position + k) div 65 536 and in tile k div 4096."""
    rng = np.random.default_rng(8)
    cases = [(0, 5 * B), (B - 1, 2), (B - 1, 1), (B - 4096, 4096), (B - 4096, 4097), (B - 4095, 4096), (2 ** 40 + 5, 3 * B), (7, B - 7), (7, B - 6)]
    cases += [(int(rng.integers(0, 2 ** 41)), int(rng.integers(1, 3 * B))) for _ in range(40)]
    for position, n_in in cases:
        k = np.arange(n_in, dtype=np.int64)
        block, tile = (position + k) // B, k // 4096
        want = []
        for t in np.unique(tile[1:][block[1:] != block[:-1]]):       # the tiles in which a sample is the first of its block ...
            mine = block[tile == t]
            if mine[0] != mine[-1]:                                  # ... and not the tile's first
                want.append((int((mine == mine[0]).sum()), int((tile == t).sum()) == 4096))
        assert ic.block_ends_in_tiles(position, n_in) == want, (position, n_in)
    assert ic.block_ends_in_tiles(B - 100, 200) == [(100, False)] and ic.block_ends_in_tiles(B - 100, 100) == []


def test_the_sweeps_cut_plan_reaches_every_block_end_and_both_call_ends():
    cuts = ic.sweep_cuts()
    splits, ragged, exact = ic.sweep_coverage(cuts)
    assert min(cuts) > 0 and len(cuts) == 44 and sum(cuts) == 35 * B + 777
    assert set(splits) >= set(ic.SWEEP_N_A) and len(ic.SWEEP_N_A) == 24
    # the call ends 1, 5 or 90 samples behind the block's end, in the same tile: on the edge of a lane's group, and inside one
    assert sorted(ragged) == sorted(ic.SWEEP_SHORT) and len(ragged) >= 5 and {ic.SWEEP_SHORT[n_a] for n_a in ragged} == {1, 5, 90}
    assert {(n_a + ic.SWEEP_SHORT[n_a]) % 8 == 0 for n_a in ragged} == {True, False}
    # the call ends on the block's end, and the next one starts a block
    assert exact == len(ic.SWEEP_EXACT) >= 5
    # from block 5 on every block's end is aimed at: it lies in the first three tiles of a call, or is the call's end
    pos, aimed = 0, set()
    for cut in cuts:
        for e in range(pos // B + 1, (pos + cut) // B + 1):
            if e * B - pos < 3 * 4096 or e * B == pos + cut:
                aimed.add(e)
        pos += cut
    assert aimed == set(range(ic.SWEEP_FIRST_END, 35))


@pytest.mark.parametrize("fmt", [ir.CS16, ir.CU8, ir.CS8, ir.CF32])
def test_the_restatement_in_the_sweeps_cuts_equals_one_shot(fmt):
    cuts = ic.sweep_cuts()
    for x in ic.sweep_rows(fmt):
        one, ref = ir.correct(x, fmt, 2)
        coefs = [h[1] for h in ref.history]
        assert ref.solved == 32 and ref.rejected == 0 and all(a != b for a, b in zip(coefs, coefs[1:]))
        c = ir.Corrector(fmt, 2)
        pos, parts = 0, []
        for cut in cuts:
            parts.append(c.push(x[pos:pos + cut])); pos += cut
        assert pos == len(x) and np.array_equal(np.concatenate(parts), one)
        assert (c.coef, c.reason, c.sums(), c.samples, c.solved, c.rejected, c.history) == (ref.coef, ref.reason, ref.sums(), len(x), 32, 0, ref.history)


def test_the_rails():
    """Every sample at (-32768, -32768): the largest sums there are, and no signal once the offset is out.  The rails alternating
    in sign: full-scale squares on both branches, coherent enough to be refused."""
    n = 6 * B + 5
    x = ic.rails(n, False)
    one = ir.correct(x, ir.CS16, 2)
    assert one[1].sums() == (-4 * B * 32768, -4 * B * 32768, 4 * B * 2 ** 30, 4 * B * 2 ** 30, 4 * B * 2 ** 30)
    assert one[1].reason == 1 and one[1].coef == (-32768, -32768, 0, 16384) and not one[0][4 * B:].any()
    _cut_everywhere(x, ir.CS16, 2, one)
    x = ic.rails(n, True)
    one = ir.correct(x, ir.CS16, 2)
    assert one[1].rejected == 3 and one[1].sums()[2] == 4 * B * (2 ** 30 + 32767 ** 2) // 2
    assert (np.abs(one[0][4 * B:].astype(np.int64)) >= 32767).all()                  # +-65535 about the middle: clamped both ways
    _cut_everywhere(x, ir.CS16, 2, one)
    # W = 64 at the rails: the largest intermediate of the solve, checked against 2^63 inside solve()
    full = (-(64 * B) * 32768, (64 * B) * 32767, 64 * B * 2 ** 30, 64 * B * 32767 ** 2, -(64 * B) * 32768 * 32767)
    assert ir.solve(full, 6)[1] == 1


# ------------------------------------------------------------------------------------------------------------ end to end
def test_the_acceptance_case(nv, oracle):
    """518 at +14 kHz, amplitude 8000; 490 at -14 kHz, amplitude 300 over noise 1500; twelve seeds.  C: decoded from the clean
    rows; H: through the impairment (gain 1.05, 3 degrees, offsets 300 and -200); K: those through the corrector at its
    defaults.  Measured: the 490 message C = 12, H = 0, K = 12 of 12, the 518 message 12 in all three."""
    t518, t490 = ic.texts()
    got = {name: {518: 0, 490: 0} for name in "CHK"}
    for seed in ic.SEEDS:
        x = ic.rows(nv, seed)
        y = ic.impair(x)
        z, ref = ir.correct(y)
        assert ref.rejected == 0 and ref.solved == len(y) // B - 16 + 1
        for name, row in (("C", x), ("H", y), ("K", z)):
            msgs, _ = ic.delivered(oracle, row, nv.FRAME_IN)
            got[name][518] += msgs[518] == [t518]
            got[name][490] += msgs[490] == [t490]
    print("490: clean", got["C"][490], "impaired", got["H"][490], "corrected", got["K"][490],
          "| 518:", got["C"][518], got["H"][518], got["K"][518])
    assert got["C"][490] == 12
    assert got["K"][490] >= got["H"][490] + 6
    assert got["K"][490] >= 10
    assert got["C"][518] == got["K"][518] == 12


def test_the_image_of_a_tone_goes_from_29_to_below_60_dbc():
    """A noise-free tone on bin 3641 of 65 536, amplitude 8000: its image in a Hann-windowed FFT of a block behind the window.
    Measured -28.9 dBc impaired and -93.9 dBc corrected; Q14 coefficients bound it near -90."""
    x = ic.tone(20 * B)
    y = ic.impair(x)
    z, ref = ir.correct(y)
    clean, impaired, corrected = (ic.image_dbc(r[18 * B:19 * B]) for r in (x, y, z))
    print("image: clean", round(clean, 1), "impaired", round(impaired, 1), "corrected", round(corrected, 1), "dBc", ref.history[-1])
    assert ref.rejected == 0 and -30.0 < impaired < -28.0
    assert corrected <= -60.0


def test_two_strong_stations_at_mirrored_frequencies_are_both_delivered(nv, oracle):
    """The known limit: both stations at amplitude 8000 on clean input.  Their coherence over a finite window is taken for the
    radio's, and the coefficients wander; both messages arrive all the same.  The scatter goes into DESIGN 3.10."""
    t518, t490 = ic.texts()
    for seed in ic.SEEDS[:3]:
        x = ic.rows(nv, seed, amp_490=ic.AMP_518)
        for window_log2 in (4, 2):
            z, ref = ir.correct(x, ir.CS16, window_log2)
            ci = [h[1][2] for h in ref.history]
            cq = [h[1][3] - 16384 for h in ref.history]
            print("seed", seed, "W", 1 << window_log2, "c_i", min(ci), "..", max(ci), "c_q - 16384", min(cq), "..", max(cq), "rejected", ref.rejected)
            if window_log2 == 4:
                msgs, _ = ic.delivered(oracle, z, nv.FRAME_IN)
                assert msgs[518] == [t518] and msgs[490] == [t490], seed
                assert max(map(abs, ci)) < 1000 and max(map(abs, cq)) < 1000
