"""The impulse noise blanker (include/navtex_amd_blank.h) on the CPU: the header and the companion library's exports and
argument safety, the launch arithmetic against 128-bit integers (a stand-alone program under ASan + UBSan), the restatement
(tests/blank_ref.py) on cuts, clean signal, silence, the rails, the bypass, sustained loud input and the counters, and the
acceptance case: a weak message under impulsive interference, decoded through the restatements with and without the
blanker, at 252 kS/s and at 768 kS/s in front of the resampler; blank_streams (many rows at once) against blank() row by
row; and the trap inputs of tests/test_gpu_blank_edges.py: each is shown to carry its feature on the restatement and to change
words under a deliberately wrong variant of it (_variant: a ring of three, the three newest sums, the partial sum dropped at
a chunk start, hold +- 1, >= for >, the reference not shifted)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import blank_cases as bc
import blank_ref as br
import resample_ref as rr

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "navtex_amd_blank.h"
PLAN = ROOT / "navtex_amd" / "blank" / "nvx_blank_plan.h"
SYMBOLS = ["nvx_blank_config_default", "nvx_blank_create", "nvx_blank_destroy", "nvx_blank_last_error", "nvx_blank_plan", "nvx_blank_position",
           "nvx_blank_push", "nvx_blank_reset", "nvx_blank_resident", "nvx_blank_stats", "nvx_blank_time_stats", "nvx_blank_timing"]
HOOKS = ["nvx_blank_debug_last_launch", "nvx_blank_debug_set_position"]


@pytest.fixture(scope="module")
def bl(nv):
    """The companion library's binding; builds the libraries first when the companion is missing."""
    if not (ROOT / "navtex_amd" / "libnavtex_amd_blank.so").exists():
        import importlib.util
        spec = importlib.util.spec_from_file_location("nvx_build", ROOT / "navtex_amd" / "build.py")
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        build.build_lib()
    import navtex_amd.blank
    return navtex_amd.blank


def _noise(n, seed, amp=1500):
    return np.random.default_rng(seed).integers(-amp, amp + 1, size=(n, 2)).astype(np.int16)


# ------------------------------------------------------------------------------------------------------------ interface
def test_header_compiles_as_plain_c_and_declares_the_entry_points(tmp_path):
    text = HEADER.read_text()
    assert sorted(set(re.findall(r"NVX_API\s+[\w\s\*]+?\b(\w+)\s*\(", text))) == SYMBOLS
    for name, want in (("NVX_BLANK_BLOCK", "1024"), ("NVX_BLANK_THR_MIN", "256"), ("NVX_BLANK_THR_MAX", "4096"), ("NVX_BLANK_THR_DEFAULT", "1024"),
                       ("NVX_BLANK_HOLD_MAX", "1024"), ("NVX_BLANK_HOLD_DEFAULT", "32"), ("NVX_BLANK_FLOOR_MAX", "65535"),
                       ("NVX_BLANK_FLOOR_DEFAULT", "64")):
        assert re.search(rf"#define {name}\s+{re.escape(want)}\b", text), name
    assert "no look-ahead" in text and "Out of scope" in text
    assert "4.0 detects 2e-5 of the\n *            samples, 5.0 detects none in 4 M, and 3.0 detects 0.2 %" in text
    src = tmp_path / "t.c"
    src.write_text('#include "navtex_amd_blank.h"\nint main(void){ nvx_blank_config c; c.format = NVX_BLANK_CF32; '
                   'return NVX_BLANK_CS16 == 0 && NVX_BLANK_CU8 == 1 && NVX_BLANK_CS8 == 2 && c.format == 3 && sizeof c == 28 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


@pytest.mark.parametrize("sym", SYMBOLS + HOOKS)
def test_symbol_is_exported(bl, sym):
    assert hasattr(bl.lib, sym), f"{sym} is declared but not exported"


def test_the_companion_links_no_other_library_of_the_project_and_no_test_infrastructure(bl):
    lib = ROOT / "navtex_amd" / "libnavtex_amd_blank.so"
    out = subprocess.run(["ldd", str(lib)], capture_output=True, text=True).stdout
    assert "libnavtex_amd" not in out and "oracle" not in out and "libamdhip64" in out
    # it defines nothing but its own interface and the tests' two hooks, and needs no nvx_ symbol from elsewhere
    nm = subprocess.run(["nm", "-D", str(lib)], capture_output=True, text=True, check=True).stdout
    defined = sorted(l.split()[-1] for l in nm.splitlines() if " T " in l and "nvx_" in l)
    assert defined == sorted(SYMBOLS + HOOKS) and all(d.startswith("nvx_blank_") for d in defined)
    assert not [h for h in HOOKS if h in HEADER.read_text()] and all(h in PLAN.read_text() for h in HOOKS)
    assert bl.lib.nvx_blank_debug_last_launch(None, None, None, None, None) < 0 and bl.lib.nvx_blank_debug_set_position(None, 0, 0) < 0
    assert not [l for l in nm.splitlines() if " U " in l and "nvx" in l]
    for path in (ROOT / "navtex_amd" / "blank").iterdir():
        text = path.read_text()
        assert "oracle" not in text and "nvxo_" not in text, path
    assert "oracle" not in HEADER.read_text() and "oracle" not in (ROOT / "navtex_amd" / "blank.py").read_text()


def test_null_and_nonsense_arguments_are_errors_never_crashes(bl, tmp_path):
    src = ROOT / "tests" / "harness" / "null_args_blank.c"
    exe = tmp_path / "null_args_blank"
    lib = ROOT / "navtex_amd"
    subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib}", "-lnavtex_amd_blank",
                    f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "blank null-safety ok" in out.stdout, (out.stdout[-2500:], out.stderr[-500:])
    assert all(re.search(rf"\b{s}\(", src.read_text()) for s in SYMBOLS)


def test_create_returns_nodev_without_a_gpu_and_refuses_bad_parameters_first(nv, bl):
    if nv.device_count() > 0:
        pytest.skip("a GPU is present")
    cfg = bl.Config()
    bl.lib.nvx_blank_config_default(C.byref(cfg))
    h = C.c_void_p(1)
    assert bl.lib.nvx_blank_create(C.byref(cfg), C.byref(h)) == -2
    assert h.value is None and b"no CPU path" in bl.lib.nvx_blank_last_error()
    with pytest.raises(nv.NvxError) as e:
        bl.Blanker(bl.CU8, n_streams=4)
    assert e.value.code == -2
    for kw in (dict(thr_q8=255), dict(thr_q8=4097), dict(hold=1025), dict(floor=65536), dict(format=4), dict(n_streams=0)):
        with pytest.raises(nv.NvxError) as e:
            bl.Blanker(**kw)
        assert e.value.code == nv._native.ERR_ARG, kw


def test_the_launch_arithmetic_against_128_bit_integers_under_asan_ubsan(tmp_path):
    """nvx_blank_fill_args (navtex_amd/blank/nvx_blank_plan.h) without a device: positions up to 2^62, call lengths around a
    tile and a chunk, every chunking -- each sample in one live tile of one chunk, pre-rolls of whole tiles inside the call
    with five whole blocks in them, block ends on the stream's blocks, 16-byte stores only on aligned rows
    (tests/harness/blank_launch_args.cpp).  A stand-alone program under ASan + UBSan."""
    exe = tmp_path / "blank_launch_args"
    pkg = ROOT / "navtex_amd"
    subprocess.run(["g++", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT / 'include'}", f"-I{pkg / 'csrc'}", f"-I{pkg / 'blank'}",
                    str(ROOT / "tests" / "harness" / "blank_launch_args.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env={"ASAN_OPTIONS": "detect_leaks=1", "PATH": "/usr/bin:/bin"})
    assert out.returncode == 0 and "blank launch args ok" in out.stdout, (out.stdout + out.stderr)[-3000:]


# ----------------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("hold", [0, 32, 1024])
def test_one_shot_equals_random_cuts(hold):
    n = 60000
    rng = np.random.default_rng(hold)
    x = _noise(n, 3)
    for s in rng.integers(4096, n - 400, 25):
        x[s:s + int(rng.integers(1, 400))] = rng.integers(-30000, 30000, size=2)
    one, ref = br.blank(x, hold=hold)
    assert ref.detections > 0
    for trial in range(4):
        cuts = [0, 1, 1023, 1024, 1025, max(hold - 1, 0), hold, hold + 1]
        rest = n - sum(cuts)
        while rest:
            c = int(min(rest, rng.choice([0, 1, 1023, 1024, 1025, hold + 1, int(rng.integers(1, 9000))])))
            cuts.append(c); rest -= c
        if trial:
            rng.shuffle(cuts)
        b = br.Blanker(hold=hold)
        pos, parts = 0, []
        for c in cuts:
            parts.append(b.push(x[pos:pos + c])); pos += c
        assert pos == n and np.array_equal(np.concatenate(parts), one), trial
        assert (b.samples, b.detections, b.blanked) == (n, ref.detections, ref.blanked)


@pytest.mark.parametrize("amplitude", [8000, 300])
def test_a_clean_signal_changes_in_no_sample(nv, amplitude):
    import signals
    bits = nv.sitor_encode(signals.stream_text(3), 8)
    x = rr.cpfsk(bits, 252000, 400000, amplitude=amplitude, seed=amplitude)
    out, ref = br.blank(x)
    assert np.array_equal(out, x) and (ref.samples, ref.detections, ref.blanked) == (len(x), 0, 0)


@pytest.mark.parametrize("floor", [0, 64])
def test_silence_blanks_nothing(floor):
    for fmt, z in ((br.CS16, 0), (br.CU8, 128), (br.CS8, 0), (br.CF32, 0.0)):
        x = np.full((20000, 2), z, dtype=rr.DTYPES[fmt])
        out, ref = br.blank(x, fmt, floor=floor)
        assert np.array_equal(out, rr.convert(x, fmt)) and ref.detections == 0 and ref.blanked == 0, fmt


def test_the_first_four_blocks_are_never_blanked_even_at_the_rails():
    x = _noise(12000, 5, amp=100)
    x[:4096:7] = (-32768, 32767)                            # dense in the first four blocks, sparse behind them
    x[3:4096:11] = (-32768, -32768)
    x[4096::500] = (32767, -32768)
    for thr in (256, 1024, 4096):
        out, ref = br.blank(x, thr_q8=thr, hold=1024, floor=0)
        assert np.array_equal(out[:4096], x[:4096]) and not ref.gone[:4096].any() and not ref.d[:4096].any()
        assert ref.d[4096:].any() and not np.array_equal(out[4096:], x[4096:])


def test_the_largest_magnitude_is_judged_correctly_at_the_largest_threshold():
    """(-32768, -32768) gives m = 65536.  At thr_q8 = 4096 (16.0) the level is 16 times the reference mean: a mean of 4095
    gives 65520 < 65536, detected; a mean of 4096 gives exactly 65536, which m does not exceed."""
    for mean, detected in ((4095, True), (4096, False)):
        x = np.zeros((6000, 2), dtype=np.int16)
        x[:, 0] = mean
        x[5000] = (-32768, -32768)
        out, ref = br.blank(x, thr_q8=4096, hold=0)
        assert br.level_of(mean * 1024, 4096, 64) == 16 * mean
        assert bool(ref.d[5000]) == detected and ref.detections == int(detected)
        assert (out[5000].tolist() == [0, 0]) == detected


@pytest.mark.parametrize("fmt", [br.CS16, br.CU8, br.CS8, br.CF32])
def test_bypass_is_the_conversion(fmt):
    rng = np.random.default_rng(fmt)
    if fmt == br.CF32:
        x = rng.uniform(-1.3, 1.3, size=(9000, 2)).astype(np.float32)
        x[:6, 0] = [np.nan, np.inf, -np.inf, 0.5 / 32768, 1.5 / 32768, 1e-42]
    else:
        info = np.iinfo(rr.DTYPES[fmt])
        x = rng.integers(info.min, info.max + 1, size=(9000, 2)).astype(rr.DTYPES[fmt])
    x[5000:5200] = x[0] * 0 + (1 if fmt != br.CF32 else 0.9)
    out, ref = br.blank(x, fmt, thr_q8=0)
    assert np.array_equal(out, rr.convert(x, fmt).astype(np.int16)) and (ref.samples, ref.detections, ref.blanked) == (9000, 0, 0)
    assert np.array_equal(br.pack(out).view(np.int16).reshape(-1, 2), out)


def test_four_loud_blocks_in_a_row_raise_the_level():
    """A strong signal that stays: blanked for the four blocks it takes the minimum of four to rise, passed from then on.  A
    burst shorter than that never raises the level it is judged by."""
    x = _noise(20 * 1024, 8, amp=300)
    on = 8 * 1024
    x[on:] = np.where(np.arange(len(x) - on)[:, None] % 2, 20000, -20000)
    out, ref = br.blank(x, hold=0)
    first_full = 8                                         # the first loud block
    assert ref.gone[on:(first_full + 4) * 1024].all(), "blanked until four loud blocks are complete"
    assert not ref.gone[(first_full + 4) * 1024:].any(), "and passed from the next block on"
    assert np.array_equal(out[(first_full + 4) * 1024:], x[(first_full + 4) * 1024:])
    y = _noise(20 * 1024, 8, amp=300)
    y[on + 100:on + 100 + 3 * 1024] = 20000                # in four blocks, but not four loud blocks
    _, ref = br.blank(y, hold=0)
    assert ref.gone[on + 100:on + 100 + 3 * 1024].all() and ref.blanked == 3 * 1024


def test_the_counters_and_the_hold():
    x = _noise(9000, 9, amp=200)
    x[6000] = (30000, 30000); x[6010] = (30000, 30000); x[8990] = (-30000, 0)
    out, ref = br.blank(x, hold=32)
    assert (ref.samples, ref.detections) == (9000, 3) and ref.blanked == 10 + 33 + 10
    assert ref.gone[6000:6043].all() and not ref.gone[5999] and not ref.gone[6043] and ref.gone[8990:].all()
    assert not out[6000:6043].any() and np.array_equal(out[:6000], x[:6000])
    b = br.Blanker(hold=32)
    b.push(x[:8995]); b.reset(); b.push(x[8995:])          # a reset forgets the detection: its hold does not run on
    assert not b.gone.any() and (b.samples, b.detections) == (9000, 3)


# ------------------------------------------------------------------------------------------------------------ end to end
def test_the_acceptance_case(nv, oracle):
    """A message at +14 kHz, amplitude 300 over noise 1500, twelve seeds.  C: decoded from the clean rows; H: with 40 bursts
    a second of 100 .. 300 samples of +-30000; B: those through the blanker at its defaults.  Measured: C = 12, H = 0,
    B = 12, 3.6 % of the samples blanked, and the clean rows pass the blanker unchanged."""
    text = bc.text()
    bits = nv.sitor_encode(text, 40)
    C_, H, B, part = 0, 0, 0, []
    for seed in bc.SEEDS:
        x, y = bc.rows(nv.FRAME_IN, bits, seed)
        out, ref = br.blank(y)
        C_ += bc.delivered(oracle, x, nv.FRAME_IN)[0] == [text]
        H += bc.delivered(oracle, y, nv.FRAME_IN)[0] == [text]
        B += bc.delivered(oracle, out, nv.FRAME_IN)[0] == [text]
        part.append(ref.blanked / ref.samples)
    print("C", C_, "H", H, "B", B, "blanked", round(float(np.mean(part)), 4))
    assert C_ == 12 and B >= H + 6 and B >= 10
    assert 0.02 < np.mean(part) < 0.06
    assert np.array_equal(br.blank(x)[0], x)               # the last seed's clean row


def test_the_chain_at_768k_delivers_with_the_blanker_and_not_without(nv, bl, oracle):
    """blanker -> the restated resampler with the plan's taps -> oracle, seed 12, bursts of 300 .. 900 samples, hold = 96."""
    import navtex_amd.resample as rs
    text = bc.text()
    bits = nv.sitor_encode(text, 40)
    L, M, T, S, taps = rs.design(bc.CHAIN_RATE)
    x, y = bc.chain_rows(bits)
    without = rr.resample_all(y, rr.CS16, taps, L, M)
    out, ref = br.blank(y, hold=bc.CHAIN_HOLD)
    with_ = rr.resample_all(out, rr.CS16, taps, L, M)
    got = [bc.delivered(oracle, r, nv.FRAME_IN)[0] for r in (without, with_)]
    print("without", got[0] == [text], "with", got[1] == [text], "blanked", round(ref.blanked / ref.samples, 4))
    assert got[1] == [text] and got[0] != [text]


# ------------------------------------------------------------------------------- the restatement for many rows at once
@pytest.mark.parametrize("fmt", [br.CS16, br.CU8])
def test_blank_streams_equals_blank_row_by_row(fmt):
    rng = np.random.default_rng(fmt)
    n, position = 9000, 2 ** 33 + 777
    rows = rng.integers(-900, 901, size=(32, n, 2))
    for s in range(32):
        for at in rng.integers(0, n - 200, 6):
            rows[s, at:at + int(rng.integers(1, 200))] = rng.integers(-30000, 30000, size=2)
        rows[s, 5000 + s:5050 + 2 * s] = (30000, -30000)
    rows = np.stack([rr.to_format(r.astype(np.int16), fmt, gain=3.0 if fmt == br.CU8 else 1.0) for r in rows])
    for params in (dict(), dict(thr_q8=300, hold=1024, floor=0), dict(hold=0, floor=2000), dict(thr_q8=0)):
        out, det, gone = br.blank_streams(rows, fmt, position=position, batch=5 * n, **params)
        for s in range(32):
            want, ref = br.blank(rows[s], fmt, position=position, **params)
            assert np.array_equal(out[s], want) and (det[s], gone[s]) == (ref.detections, ref.blanked), (params, s)
        assert (det > 0).all() or params.get("thr_q8") == 0


# ------------------------------------------------------- the trap inputs of tests/test_gpu_blank_edges.py discriminate
def _variant(x, fmt, thr_q8=br.THR_DEFAULT, hold=br.HOLD_DEFAULT, floor=br.FLOOR_DEFAULT, position=0, ring=4, need=4, hold_delta=0, ge=False,
             shift=10, drop_at=()):
    """The restatement once more in one shot, with a fault to choose: a ring of `ring` sums judged from `need` complete
    blocks on, the hold off by hold_delta, >= for >, the reference not shifted, and the open block's sum in front of the
    samples drop_at forgotten (what a chunk would see whose pre-roll lost the partial sum).  Returns int16 [n, 2]."""
    c = rr.convert(x, fmt)
    m = np.abs(c[:, 0]) + np.abs(c[:, 1])
    idx = position + np.arange(len(c), dtype=np.int64)
    b = idx // br.NB - position // br.NB
    s = np.bincount(b, weights=m).astype(np.int64)
    for at in drop_at:
        lo = max((position // br.NB + int(b[at])) * br.NB - position, 0)
        s[b[at]] -= int(m[lo:at].sum())
    level = np.full(len(s), -1, dtype=np.int64)
    for k in range(need, len(s)):
        level[k] = max((thr_q8 * (int(s[k - ring:k].min()) >> shift)) >> 8, floor)
    lv = level[b]
    d = (lv >= 0) & ((m >= lv) if ge else (m > lv))
    latest = np.maximum.accumulate(np.where(d, idx, np.int64(-1) << 40))
    return np.where((idx - latest <= hold + hold_delta)[:, None], 0, c).astype(np.int16)


RING_OF_THREE, THREE_NEWEST, NO_SHIFT, GE = dict(ring=3, need=3), dict(ring=3), dict(shift=0), dict(ge=True)


@pytest.mark.parametrize("cell", range(len(br.form2_cells())))
def test_form_2_trap_inputs_discriminate(cell):
    """Case a's rows: the design's detections are the restatement's, every trap's feature is there, and each of the wrong
    variants a pre-roll could amount to changes words."""
    fmt, first, hold, _ = br.form2_cells()[cell]
    rows, infos, slots = br.form2_trap_rows(fmt, first, hold, cell)
    assert sorted(sl for ss in slots for sl in ss) == [0, 1, 2, 3]
    for s in range(2):
        x, info = rows[s], infos[s]
        assert len(x) == first + 64 * 4096 + 5 + 3000 and info["starts"] == [first + 32 * 4096, first + 64 * 4096]
        out, ref = br.blank(x, fmt, hold=hold)
        assert np.array_equal(_variant(x, fmt, hold=hold), out)
        assert np.array_equal(ref.d, info["det"]), "the detections are the designed ones and no other"
        for C in info["starts"]:
            assert ref.d[C - hold] and ref.gone[C] and not ref.gone[C + 1]                 # trap 1
            assert not ref.d[C - hold - 1] and not ref.d[C - hold + 1:C + 2].any()       # no other whose hold ends at C or C + 1
        assert ref.d[info["probes"]].all() and not ref.gone[info["quiet"]].any() and (len(info["quiet"]) == 4) == (info["off"] == 1023)
        wrong = [dict(hold_delta=1)] + ([dict(hold_delta=-1)] if hold else []) + ([dict(drop_at=info["starts"])] if info["off"] < 1024 else [])
        if 0 in slots[s]:                                      # the smallest sum in the oldest slot
            wrong += [RING_OF_THREE, THREE_NEWEST]
        for v in wrong:
            got = _variant(x, fmt, hold=hold, **v)
            assert not np.array_equal(got, out), v
            if "hold_delta" in v:                              # ... at the chunk's first two samples
                C = info["starts"][0]
                assert not np.array_equal(got[C:C + 2], out[C:C + 2]), v
            if "drop_at" in v and info["off"] == 1023:         # one sample's sum: only the probes at the level see it
                q = info["quiet"]
                assert not got[q].any() and out[q].any()


@pytest.mark.parametrize("fmt", [br.CS16, br.CU8], ids=["cs16", "cu8"])
def test_spike_inputs_discriminate(fmt):
    """Case c's rows: as many detections as spikes, each blanking exactly hold + 1 samples; a hold one off changes words."""
    x, at = br.spike_row(fmt, seed=3)
    assert (at - br.SPIKE_FIRST - 4096 * (2 + np.arange(len(at)))).tolist() == br.spike_offsets(fmt) and len(at) == 16
    assert at[br.spike_offsets(fmt).index(br.SPIKE_OFF)] % 1024 == 0 and at[br.spike_offsets(fmt).index(br.SPIKE_OFF - 1)] % 1024 == 1023
    for hold in br.SPIKE_HOLDS:
        out, ref = br.blank(x, fmt, hold=hold)
        assert ref.detections == len(at) and ref.d[at].all() and ref.blanked == len(at) * (hold + 1)
        for a in at:
            assert ref.gone[a:a + hold + 1].all() and not ref.gone[a + hold + 1] and not ref.gone[a - 1]
        assert np.array_equal(_variant(x, fmt, hold=hold), out)
        for delta in (1, -1) if hold else (1,):
            assert not np.array_equal(_variant(x, fmt, hold=hold, hold_delta=delta), out), (hold, delta)


@pytest.mark.parametrize("position", br.LEVEL_POSITIONS)
def test_level_inputs_discriminate(position):
    """Case d's rows: a probe at the level is no detection and one a unit above it is; >= for >, an unshifted reference and
    a ring that loses its oldest sum change words."""
    for thr in br.LEVEL_THR:
        for floor in br.LEVEL_FLOORS:
            x, at_level, above = br.level_row(position, thr, floor, br.LEVEL_BLOCKS)
            out, ref = br.blank(x, thr_q8=thr, hold=0, floor=floor, position=position)
            assert len(above) >= 20 and ref.d[above].all() and not ref.d[at_level].any(), (thr, floor)
            kw = dict(thr_q8=thr, hold=0, floor=floor, position=position)
            assert np.array_equal(_variant(x, br.CS16, **kw), out)
            for v in [GE] + ([NO_SHIFT, RING_OF_THREE, THREE_NEWEST] if floor <= 64 else []):
                assert not np.array_equal(_variant(x, br.CS16, **kw, **v), out), (thr, floor, v)
    # ref >> 10: the block of 1024 * 700 + 1023 gives the level of 700, the one of 1024 * 701 that of 701
    x, at_level, _ = br.level_row(position, 256, 0, br.LEVEL_BLOCKS)
    m = np.abs(x.astype(np.int64)).sum(axis=1)
    assert {700, 701} <= set(m[at_level].tolist())
    # four loud blocks, then passed
    x, _, _ = br.level_row(position, 1024, 64, br.LEVEL_BLOCKS)
    _, ref = br.blank(x, hold=0, position=position)
    loud = [k for k, blk in enumerate(br.LEVEL_BLOCKS) if blk[0] == 20000]
    per_block = [int(ref.d[k * 1024 - position % 1024:(k + 1) * 1024 - position % 1024].sum()) for k in loud]
    assert per_block == [1024] * 4 + [0] * 2
    # 2^28: five blocks at (-32768, -32768) from the reset on, thr_q8 = 4096: nothing in them, nothing in the quiet block behind
    x, _, _ = br.level_row(position, 4096, 64, br.RAIL_BLOCKS)
    _, ref = br.blank(x, thr_q8=4096, hold=0, position=position)
    assert not ref.d[:6 * 1024 - position % 1024].any() and (x[:4096] == -32768).all()
    assert br.level_of(1024 * 65536, 4096, 0) == 1 << 20 and 4096 * ((1024 * 65536) >> 10) == 1 << 28
    # silence with floor = 0: every non-zero sample behind the first four blocks, and no zero one
    x = br.silent_row(position)
    _, ref = br.blank(x, hold=0, floor=0, position=position)
    behind = np.arange(len(x)) >= 4 * 1024 - position % 1024
    assert np.array_equal(ref.d, behind & x.any(axis=1)) and ref.detections > 200
