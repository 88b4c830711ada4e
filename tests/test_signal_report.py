"""Per-chain signal reports (include/navtex_amd_signal.h) on CPU: the header and its null-argument safety, the numpy
restatement (tests/signal_ref.py) against the bit-timing restatement's decisions, what the estimator says about known
signals -- on the oracle's y3 and delta-phi with the device's atan2 -- and the resources the report's sums leave the
demodulator kernels."""
import ctypes as C
import functools
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle_binding as ob
import signal_ref as sr
import timing_ref as tr

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "navtex_amd_signal.h").read_text()


def _symbols():
    return sorted(set(re.findall(r"NVX_API\s+[\w\s\*]+?\b(\w+)\s*\(", HEADER)))


def test_header_compiles_as_plain_c_and_declares_both_entry_points(tmp_path):
    assert _symbols() == ["nvx_enable_signal_report", "nvx_signal_report_read"]
    src = tmp_path / "t.c"
    src.write_text('#include "navtex_amd_signal.h"\nint main(void){ nvx_signal_report r; r.samples = 0; return (int)r.samples; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True)


def test_struct_layout_matches_the_binding(nv):
    assert C.sizeof(nv._native.SignalReport) == 2 * 8 + 14 * 8
    fields = re.findall(r"^\s+(?:uint64_t|double)\s+([\w, ]+);", HEADER[HEADER.index("typedef struct nvx_signal_report"):], flags=re.M)
    names = [f.strip() for group in fields for f in group.split(",")]
    assert names == [f for f, _ in nv._native.SignalReport._fields_]


@pytest.mark.parametrize("sym", _symbols())
def test_symbol_is_exported(nv, sym):
    assert hasattr(nv.lib, sym), f"{sym} is declared in navtex_amd_signal.h but not exported"


def test_null_objects_are_errors_never_crashes(nv, tmp_path):
    src = ROOT / "tests" / "harness" / "null_args_signal.c"
    exe = tmp_path / "null_args_signal"
    lib = ROOT / "navtex_amd"
    subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib}", "-lnavtex_amd",
                    f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "signal null-safety ok" in out.stdout, (out.stdout[-1500:], out.stderr[-500:])
    assert all(re.search(rf"\b{s}\(", src.read_text()) for s in _symbols())


@functools.lru_cache(maxsize=None)
def _oracle_reports(nv, rate, delta=0, amp=8000, noise=1500, carrier=True):
    """Both chains' reports on the oracle's y3 and delta-phi (device atan2), the whole stream."""
    iq, frames = sr.synth(nv, rate, delta, amp, noise, carrier)
    p = ob.Pipe(chain_mask=3, charlayer=False, tap_y3=frames * nv.FRAME_Y3)
    p.push_raw(iq) if rate == nv.RATE_RAW else p.push(iq)
    fR, fI = ob.bitfilter_table()
    atan = C.cast(nv.lib.nvx_atan2_host, C.c_void_p)
    out = []
    for chain in (0, 1):
        y3 = p.y3(chain)
        assert y3.shape[0] == frames * nv.FRAME_Y3
        r = sr.report(y3, ob.decode_taps(y3, atan)["dphi"], fR, fI)
        out.append({**r, **sr.derive(r)})
    return tuple(out)


@pytest.mark.parametrize("rate", [252000, 2016000])
def test_restated_decisions_are_the_bit_timing_restatements(nv, rate):
    iq, frames = sr.synth(nv, rate, secs=2)
    p = ob.Pipe(chain_mask=3, charlayer=False, tap_y3=frames * nv.FRAME_Y3)
    p.push_raw(iq) if rate == nv.RATE_RAW else p.push(iq)
    fR, fI = ob.bitfilter_table()
    for chain in (0, 1):
        y3 = p.y3(chain)
        B, Y = sr.energies(y3, fR, fI)
        assert B.dtype == np.float32 and np.array_equal((B > Y).astype(np.uint8), tr.decisions(y3, fR, fI))
        P, phi, d, hi, lo = sr.terms(y3, np.zeros(y3.shape[0]), fR, fI)
        assert P.shape[0] == y3.shape[0] - sr.G_DAB and np.all(hi >= lo) and 0 < d.sum() < d.shape[0]


@pytest.mark.parametrize("rate", [252000, 2016000])
def test_estimator_on_known_signals(nv, rate):
    def reports(chain, **kw):
        return _oracle_reports(nv, rate, **kw)[chain]
    sr.check_physics(reports)
    base = reports(0)
    assert base["samples"] == sr.SECONDS * rate // (nv.FRAME_RAW if rate == nv.RATE_RAW else nv.FRAME_IN) * nv.FRAME_Y3 - sr.G_DAB
    assert 0.0 <= base["contrast"] <= 1.0 and base["shift_hz"] > 0          # 'B' is the upper tone


def _demod_meta(tmp_path):
    spec = __import__("importlib.util").util.spec_from_file_location("nvx_build_sig", ROOT / "navtex_amd" / "build.py")
    mod = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = tmp_path / "demod.s"
    subprocess.run(["/opt/rocm/bin/hipcc", f"--offload-arch={mod.ARCH}", "-std=c++17", *mod.COMMON, "--cuda-device-only", "-S",
                    str(ROOT / "navtex_amd" / "csrc" / "nvx_demod.hip"), "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels"):]
    kernels = {}
    for block in re.split(r"\n\s+- \.", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            kernels[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(group_segment_fixed_size|private_segment_fixed_size|vgpr_count|vgpr_spill_count):\s+(\d+)", block)}
    return kernels


def test_demod_kernels_keep_their_lds_occupancy_and_no_scratch(tmp_path):
    """The report's sums cost the front kernels no scratch, the walk form stays within 16 KB of LDS (room beside the next
    launch's cascade grid) and within 96 VGPRs (five waves per SIMD, as before the sums)."""
    k = _demod_meta(tmp_path)
    demod = {n: v for n, v in k.items() if "nvx_demod" in n}
    assert len(demod) == 4, sorted(k)
    for n, v in demod.items():
        assert v["private_segment_fixed_size"] == 0 and v.get("vgpr_spill_count", 0) == 0, (n, v)
        if "front" in n:
            assert v["group_segment_fixed_size"] <= 16384 or "tiles" in n, (n, v)
    walk = next(v for n, v in demod.items() if n == "_Z15nvx_demod_front14nvx_demod_args")
    assert walk["vgpr_count"] <= 96, walk
