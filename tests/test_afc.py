"""Automatic frequency control (include/navtex_amd_afc.h) on the CPU: the header, its symbols, struct layouts and
null-argument safety; the law's host twin nvx_afc_step_host against the restatement (tests/afc_ref.py) on random records
and on the corners, again as a stand-alone program under ASan + UBSan; and the loop closed on the CPU through the
restatements of tuning (tune_ref) and of the signal report (signal_ref): a carrier that drifts 90 Hz is followed, and the
message sent behind the drift decodes with the tracked k and not with a constant one."""
import ctypes as C
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import afc_ref as ar
import oracle_binding as ob
import signal_ref as sr
import tune_ref as tr

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "navtex_amd_afc.h").read_text()
LAW = ROOT / "navtex_amd" / "csrc" / "nvx_afc_law.h"


def _symbols():
    return sorted(set(re.findall(r"NVX_API\s+[\w\s\*]+?\b(\w+)\s*\(", HEADER)))


def test_header_compiles_as_plain_c_and_declares_its_entry_points(tmp_path):
    assert _symbols() == sorted(["nvx_afc_config_default", "nvx_afc_enable", "nvx_afc_disable", "nvx_afc_read", "nvx_afc_trace",
                                 "nvx_group_afc_enable", "nvx_group_afc_disable", "nvx_group_afc_read", "nvx_group_afc_trace"])
    src = tmp_path / "t.c"
    src.write_text('#include "navtex_amd_afc.h"\nint main(void){ nvx_afc_config c; nvx_afc_config_default(&c);\n'
                   '  return NVX_AFC_C > 22.9183118 && NVX_AFC_C < 22.9183119 && NVX_AFC_TRACE_KEEP == 1024 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", "-c", str(src), "-o", str(tmp_path / "t.o")], check=True)
    # the constant is one hexadecimal double literal, the double nearest to 900 / (4 pi 3.125); the law's copy is the same
    assert float(ar.C) == 900.0 / (4.0 * math.pi * 3.125)
    assert re.search(r"#define NVX_AFC_LAW_C\s+(\S+)", LAW.read_text()).group(1) == re.search(r"#define NVX_AFC_C\s+(\S+)", HEADER).group(1)
    # both headers say what a tracking chain's signal report measures
    assert "against the k that launch" in HEADER and "navtex_amd_afc.h" in (ROOT / "include" / "navtex_amd_signal.h").read_text()


@pytest.mark.parametrize("sym", _symbols() + ["nvx_afc_step_host"])
def test_symbol_is_exported(nv, sym):
    assert hasattr(nv.lib, sym), f"{sym} is declared in navtex_amd_afc.h but not exported"


def test_null_objects_are_errors_and_struct_layouts_match_the_binding(nv, tmp_path):
    src = ROOT / "tests" / "harness" / "null_args_afc.c"
    exe = tmp_path / "null_args_afc"
    lib = ROOT / "navtex_amd"
    subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib}", "-lnavtex_amd",
                    f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "afc null-safety ok" in out.stdout, (out.stdout[-1500:], out.stderr[-500:])
    assert all(re.search(rf"\b{s}\(", src.read_text()) for s in _symbols())
    got = {}
    for t, f, off, size in re.findall(r"^layout (\w+)\.?(\S*) (\d+) (\d+)$", out.stdout.replace(" * ", ". "), flags=re.M):
        got.setdefault(t, {})[f] = (int(off), int(size))
    for name, st in (("nvx_afc_config", nv._native.AfcConfig), ("nvx_afc_status", nv._native.AfcStatus)):
        want = {f: (getattr(st, f).offset, getattr(st, f).size) for f, _ in st._fields_}
        want[""] = (0, C.sizeof(st))
        assert got[name] == want, (name, got[name], want)
    c = nv.afc_config()
    assert (c.struct_size, c.gain_shift, c.max_step, c.range_k, c.min_samples, c.contrast_min) == (C.sizeof(c), 1, 8, 48, 256, 0.7)
    assert {k: getattr(c, k) for k in ar.DEFAULTS} == ar.DEFAULTS


def test_without_a_device_there_is_no_tracking_and_bad_arguments_are_errors(nv):
    """Tracking is turned on for a handle, and there is none without a device (NVX_ERR_NODEV, no CPU path); with one, every
    argument out of range is NVX_ERR_ARG and a wideband handle NVX_ERR_STATE."""
    if nv.device_count() == 0:
        with pytest.raises(nv.NvxError) as e:
            nv.Pipeline()
        assert e.value.code == nv._native.ERR_NODEV
        return
    E = nv._native
    with nv.Pipeline(n_streams=2, chain_masks=[1, 3], char_layer=False) as p:
        for args in ((0, 1), (2, 0), (-1, 0), (0, 2), (0, -1)):
            assert nv.lib.nvx_afc_enable(p._h, *args, None) == E.ERR_ARG, args
            assert nv.lib.nvx_afc_disable(p._h, *args, 0) == E.ERR_ARG, args
            assert nv.lib.nvx_afc_read(p._h, *args, C.byref(E.AfcStatus())) == E.ERR_ARG, args
            assert nv.lib.nvx_afc_trace(p._h, *args, (C.c_int32 * 4)(), 4) == E.ERR_ARG, args
        assert nv.lib.nvx_afc_read(p._h, 0, 0, None) == E.ERR_ARG and nv.lib.nvx_afc_trace(p._h, 0, 0, None, 4) == E.ERR_ARG
        for bad in (dict(gain_shift=-1), dict(gain_shift=5), dict(max_step=0), dict(max_step=65), dict(range_k=0), dict(range_k=321),
                    dict(min_samples=-1), dict(contrast_min=-0.01), dict(contrast_min=1.01), dict(contrast_min=float("nan")), dict(struct_size=28)):
            assert nv.lib.nvx_afc_enable(p._h, 0, 0, C.byref(nv.afc_config(**bad))) == E.ERR_ARG, bad
        for ok in (dict(gain_shift=0, max_step=1, range_k=1, min_samples=0, contrast_min=0.0), dict(gain_shift=4, max_step=64, range_k=320, contrast_min=1.0)):
            p.afc_enable(1, 1, **ok)
        assert p.afc_status(1, 1)["enabled"] == 1 and p.afc_status(0, 0)["enabled"] == 0 and p.afc_trace(0, 0) == []
    with nv.Pipeline(n_streams=1, wideband=True, raw_rate=True, char_layer=False) as p:
        assert nv.lib.nvx_afc_enable(p._h, 0, 0, None) == E.ERR_STATE and nv.lib.nvx_afc_read(p._h, 0, 0, C.byref(E.AfcStatus())) == E.ERR_STATE


def test_the_binding_applies_fields_on_top_of_a_given_config(nv):
    """afc_enable(s, c, cfg, field=...): the fields go on top of a copy of cfg (the caller's struct stays), without a cfg on
    top of the defaults, and an unknown field is a TypeError."""
    seen = []

    def fn(h, stream, chain, cfg):
        c = cfg._obj if cfg is not None else None
        seen.append(None if c is None else (c.struct_size, c.gain_shift, c.max_step, c.range_k, c.min_samples, c.contrast_min))
        return 0
    mine = nv.afc_config(range_k=7, contrast_min=0.5)
    nv._afc_enable(fn, None, 0, 0, mine, dict(max_step=1), "t")
    nv._afc_enable(fn, None, 0, 0, None, dict(max_step=2), "t")
    nv._afc_enable(fn, None, 0, 0, mine, {}, "t")
    nv._afc_enable(fn, None, 0, 0, None, {}, "t")
    size = C.sizeof(mine)
    assert seen == [(size, 1, 1, 7, 256, 0.5), (size, 1, 2, 48, 256, 0.7), (size, 1, 8, 7, 256, 0.5), None] and mine.max_step == 8
    with pytest.raises(TypeError):
        nv._afc_enable(fn, None, 0, 0, mine, dict(max_steps=1), "t")


# ---- the law: host twin == restatement
def _case(par=None, kc=4480, k0=None, k1=None, samples=288, nb=144, sb=0.0, sy=0.0, hi=9.0, lo=1.0):
    p = dict(ar.DEFAULTS, **(par or {}))
    k1 = kc if k1 is None else k1
    return p, kc, (k1 if k0 is None else k0), k1, dict(samples=samples, b_samples=nb, sum_dphi_b=sb, sum_dphi_y=sy, sum_mf_hi=hi, sum_mf_lo=lo)


def corners():
    """(case, what the header's text says it gives: K[L+2] - K[L+1] and flags, or None = whatever the restatement gives)."""
    nan, inf, U, CL = float("nan"), float("inf"), ar.UPDATE, ar.CLAMP
    g0 = dict(gain_shift=0)
    out = [
        (_case(nb=0), (0, 0)), (_case(nb=288), (0, 0)), (_case(samples=0, nb=0, par=dict(min_samples=0)), (0, 0)),   # nb = 0, ny = 0; 0 / 0 holds
        (_case(samples=256, nb=128), (0, U)), (_case(samples=255, nb=128), (0, 0)),                                  # samples = / below min_samples
        (_case(samples=800, nb=100), (0, U)), (_case(samples=800, nb=99), (0, 0)),                                   # 8 nb = / below samples
        (_case(samples=800, nb=700), (0, U)), (_case(samples=800, nb=701), (0, 0)),                                  # 8 ny = / below samples
        (_case(par=dict(contrast_min=0.5), hi=3.0, lo=1.0), (0, U)),                                                 # hi - lo = c (hi + lo) exactly
        (_case(par=dict(contrast_min=0.5), hi=3.0, lo=np.nextafter(1.0, 2.0)), (0, 0)),
        (_case(par=dict(contrast_min=0.0), hi=1.0, lo=1.0), (0, U)), (_case(par=dict(contrast_min=1.0), hi=1.0, lo=0.0), (0, U)),
        # r exactly at a tie (e = 0, r = -(K[L+1] - K[L]), gain_shift 1): -1.5 -> -2, 0.5 -> 0, -2.5 -> -2, 1.5 -> 2, -0.5 -> 0
        (_case(k0=4480, k1=4483), (-2, U)), (_case(k0=4481, k1=4480), (0, U)), (_case(k0=4480, k1=4485), (-2, U)),
        (_case(k0=4483, k1=4480), (2, U)), (_case(k0=4480, k1=4481), (0, U)),
        (_case(par=dict(gain_shift=2), k0=4480, k1=4486), (-2, U)), (_case(par=dict(gain_shift=2), k0=4480, k1=4490), (-2, U)),   # -1.5, -2.5
        # max_step at its edge: d = +-8 passes, +-9 is cut
        (_case(par=g0, k0=4488, k1=4480), (8, U)), (_case(par=g0, k0=4489, k1=4480), (8, U | CL)),
        (_case(par=g0, k0=4472, k1=4480), (-8, U)), (_case(par=g0, k0=4471, k1=4480), (-8, U | CL)),
        # the range about the centre at its edge
        (_case(par=g0, k0=4528, k1=4527), (1, U)), (_case(par=g0, k0=4529, k1=4527), (1, U | CL)),
        (_case(par=g0, k0=4432, k1=4433), (-1, U)), (_case(par=g0, k0=4431, k1=4433), (-1, U | CL)),
        # +-25 kHz at its edge (the centre 10 below it, the range beyond)
        (_case(par=g0, kc=7990, k0=8000, k1=7999), (1, U)), (_case(par=g0, kc=7990, k0=8001, k1=7999), (1, U | CL)),
        (_case(par=g0, kc=-7990, k0=-8000, k1=-7999), (-1, U)), (_case(par=g0, kc=-7990, k0=-8001, k1=-7999), (-1, U | CL)),
        # a measured offset: mean tone frequency +10 Hz = 3.2 k -> rint(1.6) = 2
        (_case(sb=144 * (2 * math.pi * 95 / 900), sy=144 * (2 * math.pi * -75 / 900)), (2, U)),
        (_case(sb=1e300, sy=1e300, nb=1, samples=8, par=dict(min_samples=0)), (8, U | CL)),                         # huge but finite: cut to max_step
    ]
    for field in ("sb", "sy", "hi", "lo"):                                                                           # NaN and inf sums
        for v in (nan, inf, -inf):
            want = (0, 0)
            if field == "hi" and v in (inf, -inf): want = (0, U)      # inf >= c inf, -inf >= c (-inf): the gate passes as written, e = 0
            if field == "lo" and v == -inf: want = (0, U)             # hi - (-inf) = inf >= c * (-inf)
            out.append((_case(**{field: v}), want))
    out.append((_case(hi=inf, lo=inf), (0, 0)))                       # inf - inf
    return out


def _host(nv, case):
    p, kc, k0, k1, r = case
    f = C.c_uint(77)
    k2 = nv.lib.nvx_afc_step_host(p["gain_shift"], p["max_step"], p["range_k"], p["min_samples"], p["contrast_min"], kc, k0, k1,
                                  r["samples"], r["b_samples"], r["sum_dphi_b"], r["sum_dphi_y"], r["sum_mf_hi"], r["sum_mf_lo"], C.byref(f))
    return k2, f.value


def random_cases(n, seed=20):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        par = dict(gain_shift=int(rng.integers(0, 5)), max_step=int(rng.integers(1, 65)), range_k=int(rng.integers(1, 321)),
                   min_samples=int(rng.choice([0, 100, 256, 280, 288, 1000])), contrast_min=float(rng.choice([0.0, 0.5, 0.7, 1.0, rng.random()])))
        kc = int(rng.integers(-8000, 8001))
        k1 = int(np.clip(kc + rng.integers(-par["range_k"], par["range_k"] + 1), -8000, 8000))
        k0 = int(np.clip(k1 + rng.integers(-70, 71), -8000, 8000))
        samples = int(rng.choice([0, 8, 255, 256, 280, 288, 864, 3456, int(rng.integers(0, 5000))]))
        nb = int(rng.choice([0, samples // 8, (samples + 7) // 8, samples // 2, samples - samples // 8, samples, int(rng.integers(0, samples + 1))]))
        mean_b, mean_y = rng.normal(0.3, 0.4), rng.normal(-0.3, 0.4)           # radians a sample: +-40 Hz around the two tones, and far beyond
        lo = float(rng.random() * 1e6)
        hi = float(lo * rng.choice([1.0, 3.0, 5.6667, 1.0 + 10 * rng.random()]))
        out.append((par, kc, k0, k1, dict(samples=samples, b_samples=nb, sum_dphi_b=float(mean_b * nb * rng.choice([1, 1, 1, 30])),
                                           sum_dphi_y=float(mean_y * (samples - nb)), sum_mf_hi=hi, sum_mf_lo=lo)))
    return out


def test_the_host_twin_is_the_restatement_on_the_corners(nv):
    for case, want in corners():
        k2, flags = ar.step(*case)
        assert (k2 - case[3], flags) == want, ("the restatement against the header's text", case, k2, flags)
        assert _host(nv, case) == (k2, flags), (case, k2, flags)


def test_the_host_twin_is_the_restatement_on_random_records(nv):
    seen = set()
    for case in random_cases(10_000):
        want = ar.step(*case)
        assert _host(nv, case) == want, case
        seen.add(want[1])
    assert seen == {0, ar.UPDATE, ar.UPDATE | ar.CLAMP}


def test_the_law_alone_under_asan_and_ubsan_on_the_same_cases(tmp_path):
    """navtex_amd/csrc/nvx_afc_law.h in a stand-alone host program (tests/harness/afc_law_corners.cpp) built with
    -fsanitize=address,undefined: the corner table and 2000 of the random records, answers == the restatement's."""
    cases = [c for c, _ in corners()] + random_cases(2000)
    def lit(v):
        return "nan" if math.isnan(v) else ("inf" if v > 0 else "-inf") if math.isinf(v) else float(v).hex()
    lines = []
    for p, kc, k0, k1, r in cases:
        k2, flags = ar.step(p, kc, k0, k1, r)
        lines.append(" ".join(str(x) for x in (p["gain_shift"], p["max_step"], p["range_k"], p["min_samples"], lit(p["contrast_min"]), kc, k0, k1,
                                                r["samples"], r["b_samples"], lit(r["sum_dphi_b"]), lit(r["sum_dphi_y"]), lit(r["sum_mf_hi"]), lit(r["sum_mf_lo"]), k2, flags)))
    table = tmp_path / "cases.txt"
    table.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "afc_law_corners"
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    f"-I{ROOT / 'navtex_amd' / 'csrc'}", str(ROOT / "tests" / "harness" / "afc_law_corners.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), str(table)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and f"afc law corners ok {len(cases)}" in out.stdout, (out.stdout[-1500:], out.stderr[-1500:])


# ---- the loop, closed on the CPU
def test_a_drifting_carrier_is_followed_and_its_message_decodes_only_with_the_tracked_k(nv):
    """252 kS/s, amplitude 8000, noise_amp 1500: the carriers drift 0 -> +90 Hz over 30 frames and hold while MESSAGE is
    sent.  Launch by launch (a frame each) tune_ref.chain runs frame f with K[f], signal_ref.report gives the frame's
    record and the law K[f + 2].  The FIR histories a frame needs lie within the frame in front of it (nvx_kernels.h: 530
    mixer outputs), so each frame is restated from a two-frame window; the decode at the end runs over the whole stream."""
    iq, ramp, frames = ar.drift_then_hold(nv, nv.RATE_IN)
    y1 = tr.front(iq, False)
    fR, fI = ob.bitfilter_table()
    for ch in (0, 1):
        kc = tr.NOMINAL[ch]
        K = [kc, kc]
        for f in range(frames):
            a = max(0, f - 1)
            y3 = tr.chain(y1[a * tr.N:(f + 1) * tr.N], ch, K[a:f + 1])
            rec = sr.report(y3, ob.decode(y3)[1], fR, fI, start=(f - a) * nv.FRAME_Y3)
            K.append(ar.step(ar.DEFAULTS, kc, K[f], K[f + 1], rec)[0])
        K = K[:frames]
        tail = np.array(K[ramp + 10:]) - kc
        assert np.all(np.abs(tail * ar.STEP_HZ - ar.DRIFT_HZ) <= sr.OFFSET_TOL), (ch, tail)
        assert max(abs(b - a) for a, b in zip(K, K[1:])) <= ar.DEFAULTS["max_step"]
        assert tr.messages(tr.decode(tr.chain(y1, ch, K))) == [ar.MESSAGE], (ch, K)
        assert tr.messages(tr.decode(tr.chain(y1, ch, kc))) == [], ch           # the same message, a constant centre
