"""The diversity combiner (include/navtex_amd_div.h) on the CPU: the header and the companion library's exports and argument
safety, the solve (navtex_amd/div/nvx_div_solve.h as a stand-alone program under ASan + UBSan) against the restatement's Python
integers line for line, the launch arithmetic against 128-bit integers (likewise stand-alone), the restatement
(tests/div_ref.py) on cuts at block ends, cell ends, mid-block and one-sample calls, reason 1, a lead flip, the rails and
full-scale random rows in every format, set_freq in mid-cell, HOLD and set, the steps 0, negative and 2^32/512, and end to end
through the oracle: the acceptance case (a 490 station that fades on two antennas in quadrature, twelve seeds), the weight on
a static pair, and the known limit (d) -- a fade faster than the window."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import div_cases as dc
import div_ref as dr
import resample_ref as rr

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "navtex_amd_div.h"
PLAN = ROOT / "navtex_amd" / "div" / "nvx_div_plan.h"
SYMBOLS = ["nvx_div_config_default", "nvx_div_create", "nvx_div_destroy", "nvx_div_get", "nvx_div_hz_from_step", "nvx_div_last_error", "nvx_div_plan",
           "nvx_div_position", "nvx_div_push", "nvx_div_reset", "nvx_div_resident", "nvx_div_set", "nvx_div_set_freq", "nvx_div_set_mode",
           "nvx_div_step_from_hz", "nvx_div_time_stats", "nvx_div_timing"]
HOOKS = ["nvx_div_debug_last_launch", "nvx_div_debug_set_position"]
B, CELL = dr.BLOCK, dr.CELL
FORMATS = (dr.CS16, dr.CU8, dr.CS8, dr.CF32)
STEPS = (0, (1 << 32) // 512, dr.step_from_hz(-14000, 252000), 0x12345678)       # 0, a whole turn per two blocks, a negative one, any


@pytest.fixture(scope="module")
def dv(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_div.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.div
    return navtex_amd.div


# ------------------------------------------------------------------------------------------------------------ interface
def test_header_compiles_as_plain_c_and_declares_the_entry_points(tmp_path):
    text = HEADER.read_text()
    assert sorted(set(re.findall(r"NVX_API\s+[\w\s\*]+?\b(\w+)\s*\(", text))) == SYMBOLS
    for name, want in (("NVX_DIV_BLOCK", "256"), ("NVX_DIV_CELL", "65536"), ("NVX_DIV_MAX_TARGETS", "4"), ("NVX_DIV_WINDOW_LOG2_DEFAULT", "2"),
                       ("NVX_DIV_W_ONE", "8192"), ("NVX_DIV_W_MAX", "32767"), ("NVX_DIV_COHERENCE_ONE", "16384"), ("NVX_DIV_TRACK", "0"), ("NVX_DIV_HOLD", "1")):
        assert re.search(rf"#define {name}\s+{re.escape(want)}\b", text), name
    assert "Known limits" in text and all(f"({k})" in text for k in "abcdef")
    assert "IQ-correct (each row) -> align -> (blank / notch / DDC / resample, each row alike) -> combine -> scan -> tune -> decode" in text
    # the reciprocal pointers
    assert "navtex_amd_div.h" in (ROOT / "include" / "navtex_amd_anc.h").read_text()
    src = tmp_path / "t.c"
    src.write_text('#include "navtex_amd_div.h"\nint main(void){ nvx_div_config c; nvx_div_status s; c.format = NVX_DIV_CF32; s.sums[3] = 0; '
                   'return NVX_DIV_CS16 == 0 && NVX_DIV_CU8 == 1 && NVX_DIV_CS8 == 2 && c.format == 3 && sizeof c == 24 && sizeof s == 88 && !s.sums[3] ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


@pytest.mark.parametrize("sym", SYMBOLS + HOOKS)
def test_symbol_is_exported(dv, sym):
    assert hasattr(dv.lib, sym), f"{sym} is declared but not exported"


def test_the_companion_links_no_other_library_of_the_project_and_no_test_infrastructure(dv):
    lib = ROOT / "navtex_amd" / "libnavtex_amd_div.so"
    out = subprocess.run(["ldd", str(lib)], capture_output=True, text=True).stdout
    assert "libnavtex_amd" not in out and "oracle" not in out and "libamdhip64" in out
    # it defines nothing but its own interface and the tests' two hooks, and needs no nvx_ symbol from elsewhere
    nm = subprocess.run(["nm", "-D", str(lib)], capture_output=True, text=True, check=True).stdout
    defined = sorted(l.split()[-1] for l in nm.splitlines() if " T " in l and "nvx_" in l)
    assert defined == sorted(SYMBOLS + HOOKS) and all(d.startswith("nvx_div_") for d in defined)
    assert not [h for h in HOOKS if h in HEADER.read_text()] and all(h in PLAN.read_text() for h in HOOKS)
    assert dv.lib.nvx_div_debug_last_launch(None, None, None, None, None) < 0 and dv.lib.nvx_div_debug_set_position(None, 0, 0) < 0
    assert not [l for l in nm.splitlines() if " U " in l and "nvx" in l]
    for path in (ROOT / "navtex_amd" / "div").iterdir():
        text = path.read_text()
        assert "oracle" not in text and "nvxo_" not in text, path
    assert "oracle" not in HEADER.read_text() and "oracle" not in (ROOT / "navtex_amd" / "div.py").read_text()
    assert C.sizeof(dv.Config) == 24 and C.sizeof(dv.Status) == 88
    # the two formulas are the restatement's
    for hz in (-14000.0, 0.0, 490.0, 125999.0, -126000.0, 1e7):
        assert dv.step_from_hz(hz, 252000.0) == dr.step_from_hz(hz, 252000.0), hz
    assert dv.hz_from_step(STEPS[2], 252000.0) == dr.hz_from_step(STEPS[2], 252000.0) and abs(dv.hz_from_step(STEPS[2], 252000.0) + 14000) < 1e-3


def test_null_and_nonsense_arguments_are_errors_never_crashes(dv, tmp_path):
    src = ROOT / "tests" / "harness" / "null_args_div.c"
    exe = tmp_path / "null_args_div"
    lib = ROOT / "navtex_amd"
    subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib}", "-lnavtex_amd_div",
                    f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "div null-safety ok" in out.stdout, (out.stdout[-2500:], out.stderr[-500:])
    assert all(re.search(rf"\b{s}\(", src.read_text()) for s in SYMBOLS)


def test_create_returns_nodev_without_a_gpu_and_refuses_bad_parameters_first(nv, dv):
    for kw in (dict(window_log2=3), dict(window_log2=6), dict(window_log2=-1), dict(format=4), dict(format=-1), dict(n_pairs=0), dict(n_pairs=65536),
               dict(n_targets=0), dict(n_targets=5)):
        with pytest.raises(nv.NvxError) as e:
            dv.Combiner(**kw)
        assert e.value.code == nv._native.ERR_ARG, kw
    if nv.device_count() > 0:
        return                                                   # the rest is what a machine without a GPU answers
    cfg = dv.Config()
    dv.lib.nvx_div_config_default(C.byref(cfg))
    assert (cfg.struct_size, cfg.device, cfg.format, cfg.n_pairs, cfg.n_targets, cfg.window_log2) == (24, 0, 0, 1, 1, 2)
    h = C.c_void_p(1)
    assert dv.lib.nvx_div_create(C.byref(cfg), C.byref(h)) == -2
    assert h.value is None and b"no CPU path" in dv.lib.nvx_div_last_error()
    with pytest.raises(nv.NvxError) as e:
        dv.Combiner(dv.CU8, n_pairs=4, n_targets=2)
    assert e.value.code == -2


def _sanitized(tmp_path, name, extra=()):
    exe = tmp_path / name
    pkg = ROOT / "navtex_amd"
    subprocess.run(["g++", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT / 'include'}", f"-I{pkg / 'csrc'}", f"-I{pkg / 'div'}", *extra,
                    str(ROOT / "tests" / "harness" / (name + ".cpp")), "-o", str(exe)], check=True)
    return exe


def test_the_launch_arithmetic_against_128_bit_integers_under_asan_ubsan(tmp_path):
    """nvx_div_fill_args (navtex_amd/div/nvx_div_plan.h) without a device: positions up to 2^62, call lengths around a block, a
    tile, a cell and a chunk, every chunking and window -- each sample in one tile of one chunk, in the block the sums kernel and
    the cell the apply kernel take it for, a record for every block and a weight for every cell, the fold's blocks of every
    cell, 16-byte stores only on aligned rows (tests/harness/div_launch_args.cpp).  A stand-alone program under ASan + UBSan."""
    exe = _sanitized(tmp_path, "div_launch_args")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env={"ASAN_OPTIONS": "detect_leaks=1", "PATH": "/usr/bin:/bin"})
    assert out.returncode == 0 and "div launch args ok" in out.stdout, (out.stdout + out.stderr)[-3000:]


def _solve_rows():
    """A few thousand rows of sums: the extremes, perfect squares +-1 under the square root, and random rows of every size
    with |TRE|, |TIM| <= max(TAA, TBB), as the sums of real rows have them."""
    top = 1 << 59
    rows = [(top, top, top, top), (top, top, -top, -top), (top, top, 0, 0), (top, 0, 0, 0), (0, top, 0, 0), (top, 1, -top, top), (1, top, top, -top),
            (512, 511, 0, 0), (512, 512, 0, 0), (1023, 0, 0, 0), (0, 1024, 0, 0), (0, 0, 0, 0), (1024, 0, 0, 0), (600, 600, 600, 0), (600, 600, 0, -600),
            (5000, 5000, 0, 0), (1 << 40, 1 << 40, 0, 0), (1 << 28, 1 << 28, 1 << 28, 0), ((1 << 29) - 1, (1 << 29) - 1, (1 << 29) - 1, (1 << 29) - 1),
            (1 << 29, 1 << 29, -(1 << 29), -(1 << 29)), (top - 1, top - 1, top - 1, -(top - 1))]
    # d^2 + 4 tre^2 a perfect square (d, 2 tre, k a Pythagorean triple), and next to one: d one off, tim = 1
    for d, e in ((3, 2), (5, 6), (65, 36), (119, 60), (300000, 200000), (3 << 25, 1 << 26)):
        assert (d * d + 4 * e * e) == int(round((d * d + 4 * e * e) ** 0.5)) ** 2
        for dd in (d - 1, d, d + 1):
            for tim in (0, 1):
                rows += [(dd + e + 1000, e + 1000, e, tim), (e + 1000, dd + e + 1000, -e, -tim)]
    for k in (5, 1000, 46341, (1 << 20) + 3, (1 << 29) - 1):              # q = k^2 exactly: tre = tim = 0, d = k
        rows += [(k + 2000, 2000, 0, 0), (2000, k + 2000, 0, 0), (k + 2000, 2000, 0, 1), (k + 2000, 2001, 0, 0)]
    rng = np.random.default_rng(59)
    for bits in range(1, 60):
        for _ in range(60):
            hi = 1 << bits
            taa, tbb = int(rng.integers(0, hi)) + (hi >> 1) * int(rng.integers(0, 2)), int(rng.integers(0, hi))
            if rng.integers(0, 2):
                taa, tbb = tbb, taa
            m = min(max(taa, tbb), top)
            rows.append((min(taa, top), min(tbb, top), int(rng.integers(-m, m + 1)), int(rng.integers(-m, m + 1))))
    return rows


def test_the_solve_on_the_host_under_asan_ubsan_equals_the_restatement_line_for_line(tmp_path):
    """navtex_amd/div/nvx_div_solve.h -- the code the fold kernel runs -- compiled for the host as a stand-alone program: its
    lead, weight, coherence and reason on every row are the Python integers'."""
    rows = _solve_rows()
    assert len(rows) > 3000
    (tmp_path / "rows.txt").write_text("".join("%d %d %d %d\n" % r for r in rows))
    exe = _sanitized(tmp_path, "div_solve")
    out = subprocess.run([str(exe), str(tmp_path / "rows.txt")], capture_output=True, text=True, timeout=600, env={"ASAN_OPTIONS": "detect_leaks=1", "PATH": "/usr/bin:/bin"})
    assert out.returncode == 0 and f"div solve ok: {len(rows)} rows" in out.stderr, (out.stdout[-500:] + out.stderr)[-3000:]
    got = out.stdout.splitlines()
    want = [dr.solve_line(r) for r in rows]
    bad = [(r, g, w) for r, g, w in zip(rows, got, want) if g != w]
    assert len(got) == len(want) and not bad, bad[:5]
    # what the extremes are
    assert dr.solve((1023, 0, 0, 0)) == (0, (0, 0), 0, 1) and dr.solve((0, 1024, 0, 0)) == (1, (0, 0), 0, 0)
    assert dr.solve((5000, 5000, 0, 0)) == (0, (0, 0), 0, 0)                # d = 0 and no correlation: den = 0
    assert dr.solve((1 << 59,) * 2 + (1 << 59, 0)) == (0, (8192, 0), 16384, 0)
    assert dr.solve((600, 600, 0, -600)) == (0, (0, -8192), 16384, 0) and dr.solve((0, 0, 0, 0))[3] == 1
    reasons = [int(w.split()[4]) for w in want]
    leads = [int(w.split()[0]) for w in want]
    assert 0 < sum(reasons) < len(rows) // 4 and len(rows) // 4 < sum(leads) < 3 * len(rows) // 4


# ----------------------------------------------------------------------------------------------------------- restatement
def _state(c):
    return [(c.status(k), t.first, t.complete, t.history, tuple(t.cell), tuple(t.block)) for k, t in enumerate(c.targets)]


def _cut_everywhere(a, b, steps, fmt, window_log2, one):
    """One shot == cuts at block ends, cell ends, next to both, mid-block and one-sample calls, in this order and in two others."""
    n = len(a)
    rng = np.random.default_rng(n)
    for trial in range(3):
        cuts = [0, 1, B - 1, B, 1, CELL - 2 * B - 1, CELL, CELL + 1, B - 1, 30000, 1, 1, 1]
        rest = n - sum(cuts)
        assert rest >= 0
        while rest:
            cut = int(min(rest, rng.choice([0, 1, B - 1, B, B + 1, CELL, int(rng.integers(1, 2 * CELL))])))
            cuts.append(cut); rest -= cut
        if trial:
            rng.shuffle(cuts)
        c = dr.Combiner(fmt, len(steps), window_log2)
        for k, step in enumerate(steps):
            c.set_freq(k, step)
        pos, parts = 0, []
        for cut in cuts:
            parts.append(c.push(a[pos:pos + cut], b[pos:pos + cut])); pos += cut
        assert pos == n and np.array_equal(np.concatenate(parts, axis=1), one[0]), trial
        assert _state(c) == _state(one[1])


@pytest.mark.parametrize("window_log2,cells", [(0, 4.4), (2, 7.3)])
def test_one_shot_equals_cuts_at_and_next_to_the_block_and_cell_ends(window_log2, cells):
    steps = STEPS[1:3]
    a, b = dc.tones_pair(int(cells * CELL), 3 + window_log2, steps)
    one = dr.combine(a, b, steps, dr.CS16, window_log2)
    for t in one[1].targets:
        assert t.solved == int(cells) - (1 << window_log2) + 1 and len({h[2] for h in t.history}) == t.solved
    _cut_everywhere(a, b, steps, dr.CS16, window_log2, one)


def test_a_lead_flip_within_a_row_and_the_stronger_row_is_the_output():
    """The stronger branch changes from window to window at W = 1: both leads occur, and where the weight is (0, 0) with lead 1
    the output is the second row's conversion."""
    a, b = dc.tones_pair(9 * CELL, 17, [STEPS[2]])
    out, ref = dr.combine(a, b, [STEPS[2]], dr.CS16, 0)
    leads = [h[1] for h in ref.targets[0].history]
    assert len(leads) == 8 and 0 in leads and 1 in leads and any(x != y for x, y in zip(leads, leads[1:]))
    assert np.array_equal(out[0][:CELL], a[:CELL])
    c = dr.Combiner(dr.CS16, 1, 0)
    c.set(0, 1, 0, 0)
    c.set_mode(0, dr.HOLD)
    assert np.array_equal(c.push(a[:1000], b[:1000])[0], b[:1000])


def test_reason_one_silence_in_the_band():
    """Both rows all zero for three cells at W = 2: the cell starts 2 and 3 are rejected with reason 1 and the weight (0, 0), the
    next ones solve.  TAA + TBB = 1023 is reason 1, 1024 is not."""
    n = 6 * CELL + 100
    a, b = dc.silence_then_tone(n, 5, STEPS[2], 3 * CELL)
    out, ref = dr.combine(a, b, [STEPS[2]], dr.CS16, 1)
    t = ref.targets[0]
    assert [(h[0], h[4]) for h in t.history] == [(2, 1), (3, 1), (4, 0), (5, 0), (6, 0)] and (t.rejected, t.solved) == (2, 3)
    assert t.history[1][1:4] == (0, (0, 0), 0) and np.array_equal(out[0][:4 * CELL], a[:4 * CELL])
    assert dr.solve((1000, 23, 5, 5))[3] == 1 and dr.solve((1000, 24, 5, 5))[3] == 0


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_zero_weight_is_the_main_rows_conversion(fmt):
    """HOLD from the first sample: the weight (0, 0) with lead 0 throughout gives the main row's conversion word for word,
    whatever the second row holds; the sums go on."""
    n = 3 * CELL + 9
    a, b = dc.extremes(fmt, n, 20 + fmt)[2]
    c = dr.Combiner(fmt, 1, 1)
    c.set_freq(0, STEPS[3])
    c.set_mode(0, dr.HOLD)
    out = c.push(a, b)
    assert np.array_equal(out[0], rr.convert(a, fmt).astype(np.int16))
    st = c.status(0)
    assert (st["samples"], st["cells_solved"], st["cells_rejected"], st["weight"], st["lead"], st["mode"]) == (n, 0, 0, (0, 0), 0, dr.HOLD)
    assert st["sums"][0] > 0 and st["sums"][1] > 0 and c.targets[0].complete == 2


@pytest.mark.parametrize("fmt", FORMATS)
def test_rails_and_full_scale_rows_in_every_format_clamp_and_cut_alike(fmt):
    """The lowest value throughout, the rails alternating in sign, and full-scale random rows (float32: NaN, infinities,
    denormals and the ties of the rounding among them), four targets: one shot equals the cut rows, every bound of the header
    holds (asserted inside the restatement), and the sum of two full-scale rows clamps."""
    n = 3 * CELL + 21000
    for k, (a, b) in enumerate(dc.extremes(fmt, n, 500 + fmt)):
        one = dr.combine(a, b, STEPS, fmt, 0)
        assert all(t.solved + t.rejected == 3 for t in one[1].targets), k
        c = dr.Combiner(fmt, 4, 0)
        for j, step in enumerate(STEPS):
            c.set_freq(j, step)
        parts = [c.push(a[:CELL + 11], b[:CELL + 11]), c.push(a[CELL + 11:], b[CELL + 11:])]
        assert np.array_equal(np.concatenate(parts, axis=1), one[0]) and _state(c) == _state(one[1]), k
        if k == 0:
            # both rows at the lowest value: at step 0 they are equal and coherent, the weight is (8192, 0) and the sum clamps
            t = one[1].targets[0]
            assert (t.lead, t.w, t.coherence, t.reason) == (0, (8192, 0), 16384, 0) and (one[0][0][CELL:] == -32768).all()
        if k == 2:
            # the largest weight a set takes, on full-scale rows: |p|, |r'| < 2^31 (asserted inside apply), and most sums clamp
            c = dr.Combiner(fmt, 1, 0)
            c.set(0, 1, 32767, -32767)
            c.set_mode(0, dr.HOLD)
            o = c.push(a[:20000], b[:20000])[0]
            assert int(((o == 32767) | (o == -32768)).sum()) > 10000


def test_set_freq_in_mid_cell_starts_the_target_anew_and_leaves_the_other():
    """set_freq at 2.4 cells at W = 1: the first counted cell is 3, so the first solve behind it is at cell 4; cell 3 goes out with
    the weight (0, 0), and the samples of cell 2 behind the restart are not summed.  The other target is as without it."""
    n = 6 * CELL
    at = 2 * CELL + 26000
    a, b = dc.tones_pair(n, 31, [STEPS[1], STEPS[2]])
    plain = dr.combine(a, b, [STEPS[1], STEPS[2]], dr.CS16, 0)
    c = dr.Combiner(dr.CS16, 2, 0)
    c.set_freq(0, STEPS[1]); c.set_freq(1, STEPS[3])
    first = c.push(a[:at], b[:at])
    c.set_freq(1, STEPS[2])
    assert c.targets[1].first == 3 and c.status(1)["weight"] == (0, 0) and c.status(1)["sums"] == (0, 0, 0, 0) and c.status(1)["step"] == STEPS[2]
    rest = c.push(a[at:], b[at:])
    out = np.concatenate([first, rest], axis=1)
    assert np.array_equal(out[0], plain[0][0]) and c.status(0) == plain[1].status(0)
    t = c.targets[1]
    assert [h[0] for h in t.history] == [4, 5] and t.solved + t.rejected == 4 and np.array_equal(out[1][at:4 * CELL], a[at:4 * CELL])     # the counters stay
    # from cell 4 on the target is what one started at cell 3 is: the same sums, the same weights
    fresh = dr.Combiner(dr.CS16, 1, 0, position=3 * CELL)
    fresh.set_freq(0, STEPS[2])
    tail = fresh.push(a[3 * CELL:], b[3 * CELL:])
    assert np.array_equal(tail[0], out[1][3 * CELL:]) and fresh.targets[0].history == t.history


def test_hold_and_set_between_calls():
    n = 7 * CELL
    a, b = dc.tones_pair(n, 41, [STEPS[2]])
    c = dr.Combiner(dr.CS16, 1, 0)
    c.set_freq(0, STEPS[2])
    c.set(0, 1, -3000, 4000)
    out = [c.push(a[:CELL // 2], b[:CELL // 2])]                          # the set weight, until the first solve
    assert np.array_equal(out[0][0], dr.apply(a[:CELL // 2].astype(np.int64), b[:CELL // 2].astype(np.int64), 1, (-3000, 4000)))
    out.append(c.push(a[CELL // 2:2 * CELL + 5], b[CELL // 2:2 * CELL + 5]))
    assert c.targets[0].solved == 2
    held = (c.targets[0].lead, c.targets[0].w)
    c.set_mode(0, dr.HOLD)
    out.append(c.push(a[2 * CELL + 5:4 * CELL], b[2 * CELL + 5:4 * CELL]))
    assert (c.targets[0].lead, c.targets[0].w) == held and c.targets[0].solved == 2
    c.set(0, 0, 32767, -32767)
    out.append(c.push(a[4 * CELL:5 * CELL + 1], b[4 * CELL:5 * CELL + 1]))
    assert c.status(0)["weight"] == (32767, -32767)
    c.set_mode(0, dr.TRACK)
    out.append(c.push(a[5 * CELL + 1:], b[5 * CELL + 1:]))
    assert c.targets[0].solved == 3 and [h[0] for h in c.targets[0].history] == [1, 2, 6]


# ------------------------------------------------------------------------------------------------------------ end to end
def _acceptance(nv, oracle, window_log2, period_s, rows=("main", "second", "combined")):
    want = dc.text()
    got = dict.fromkeys(rows, 0)
    for seed in dc.SEEDS:
        a, b = dc.fading_pair(nv, seed, period_s=period_s)
        y, ref = dr.combine(a, b, [dc.STEP_490], dr.CS16, window_log2)
        assert ref.targets[0].rejected == 0 and ref.targets[0].solved == len(a) // CELL - (1 << window_log2) + 1
        for name, row in (("main", a), ("second", b), ("combined", y[0])):
            if name in rows:
                got[name] += dc.delivered(oracle, row, nv.FRAME_IN)[0] == [want]
    return got


def test_the_acceptance_case_delivers_from_the_combined_row_only(nv, oracle):
    """490 at -14 kHz, amplitude 300, with the gains cos(2 pi t / 8 s) e^{j 0.7} and sin(2 pi t / 8 s) e^{j 2.1} on the two
    antennas, under own noise of +-1500 on each; W = 4.  Measured with the integer restatement: main 0, second 0, combined 12
    of 12."""
    got = _acceptance(nv, oracle, 2, dc.FADE_S)
    print("490 delivered: main", got["main"], "second", got["second"], "combined", got["combined"], "of 12")
    assert got["combined"] == 12
    assert got["main"] <= 1 and got["second"] <= 1


def test_the_weight_follows_the_paths(nv):
    """A static pair with the gains 1 and 0.5 e^{j 1.0}: lead 0 and the weight within 40 of rint(8192 * 0.5 e^{-j 1.0}); with the
    rows swapped the lead is 1, and the weight the same."""
    a, b = dc.static_pair(nv, 11)
    for rows, lead in (((a, b), 0), ((b, a), 1)):
        _, ref = dr.combine(*rows, [dc.STEP_490], dr.CS16, 2)
        t = ref.targets[0]
        assert t.solved >= 2 and t.rejected == 0
        for h in t.history:
            assert h[1] == lead and abs(h[2][0] - dc.STATIC_WEIGHT[0]) <= 40 and abs(h[2][1] - dc.STATIC_WEIGHT[1]) <= 40, h
            assert h[3] > 15000
    assert dc.STATIC_WEIGHT == tuple(int(v) for v in np.rint(8192 * np.array([np.conj(dc.STATIC_GAIN).real, np.conj(dc.STATIC_GAIN).imag])))


def test_the_known_limit_a_fade_faster_than_the_window(nv, oracle):
    """Known limit (d): the acceptance case with a period of 3 s.  At W = 4 the causal one-second window lags the fade.  Nothing
    is asserted: the count is printed, and DESIGN 3.20 records it beside W = 1's."""
    for window_log2 in (2, 0):
        got = _acceptance(nv, oracle, window_log2, 3.0, rows=("combined",))
        print("3 s period, W =", 1 << window_log2, ": combined", got["combined"], "of 12")
