"""Guards on the generated gfx950 code of the demodulator kernels with the soft values in them (hipcc cross-compiles
without a GPU): no scratch, no fused multiply-add in the soft arithmetic, and the registers the FSM kernel may take.

The soft values are computed in nvx_demod_fsm, which had no floating-point multiply before: it must hold NO fused
multiply-add of any kind.  The three front kernels keep the FMAs they always had and no other: the explicit error-free
transformations of nvx_atan2 and the expansion of IEEE division (nvx_demod.hip's header comment: the discriminator's
atan2, and the one division of the arg-max margin statistics), fp64 only -- counted here on two probe kernels, one that
calls nvx_atan2 once and one that divides once, times the instantiations of the per-sample code in each front (the walk
and the head are compiled with and without the signal report's sums: two; the tiles: one)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")

FSM = "_Z13nvx_demod_fsm14nvx_demod_args"
FRONTS = {"_Z15nvx_demod_front14nvx_demod_args": 2, "_Z20nvx_demod_front_head14nvx_demod_args": 2, "_Z21nvx_demod_front_tiles14nvx_demod_argsi": 1}
# Registers of nvx_demod_fsm as compiled (recorded: 106; 53 before the soft pass).  Its waves run beside the NEXT launch's
# cascade grid, which leaves one wave's room per CU: with the cascade kernels at up to 192 VGPRs, two to a SIMD, 128
# still fit (2 * 192 + 128 = 512).
FSM_VGPRS_RECORDED, FSM_VGPRS_MAX = 106, 128
PROBE = r'''
#include <hip/hip_runtime.h>
#include "nvx_atan2.h"
__global__ void probe_atan2(const double *y, const double *x, double *o) { o[threadIdx.x] = nvx_atan2(y[threadIdx.x], x[threadIdx.x]); }
__global__ void probe_div(const double *y, const double *x, double *o) { o[threadIdx.x] = y[threadIdx.x] / x[threadIdx.x]; }
'''


def _compile(src: Path, out: Path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("nvx_build_soft_isa", ROOT / "navtex_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    subprocess.run([HIPCC, f"--offload-arch={mod.ARCH}", "-std=c++17", *mod.COMMON, "--cuda-device-only", "-S", str(src), "-o", str(out)],
                   check=True, capture_output=True)
    text = out.read_text()
    kernels = {m.group(1): m.group(0) for m in re.finditer(r"^(_Z\w+):.*?\.end_amdhsa_kernel", text, flags=re.S | re.M)}
    meta = {}
    for block in re.split(r"\n\s+- \.", text[text.index("amdhsa.kernels"):])[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            meta[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(group_segment_fixed_size|private_segment_fixed_size|vgpr_count|vgpr_spill_count|sgpr_spill_count):\s+(\d+)", block)}
    return kernels, meta


@pytest.fixture(scope="module")
def demod(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("soft_isa")
    kernels, meta = _compile(ROOT / "navtex_amd" / "csrc" / "nvx_demod.hip", tmp / "demod.s")
    probe = tmp / "probe.hip"
    probe.write_text(PROBE)
    pk, _ = _compile(probe, tmp / "probe.s")
    return kernels, meta, pk


def _fma(body: str, pattern: str) -> int:
    return len(re.findall(rf"^\s+(?:{pattern})\b", body, flags=re.M))


def test_the_four_demodulator_kernels_and_no_scratch(demod):
    kernels, meta, _ = demod
    names = {k for k in meta if "nvx_demod" in k}
    assert names == {FSM, *FRONTS}, sorted(meta)
    for n in names:
        assert meta[n]["private_segment_fixed_size"] == 0 and meta[n].get("vgpr_spill_count", 0) == 0, (n, meta[n])
        assert "scratch_" not in kernels[n], n
    print({n: meta[n]["vgpr_count"] for n in sorted(names)})


def test_the_soft_arithmetic_holds_no_fused_multiply_add(demod):
    kernels, _, probe = demod
    fsm = kernels[FSM]
    assert _fma(fsm, r"v_fma_f32|v_fma_f64|v_fmac_f32\w*|v_fmac_f64\w*|v_pk_fma_f32|v_mad_f32|v_mac_f32\w*") == 0
    # the soft pass is there: five taps x four accumulators, products and sums apart (one window at a time: at least once)
    assert _fma(fsm, r"v_mul_f32\w*") >= 10 and _fma(fsm, r"v_mul_f64\w*") >= 20 and _fma(fsm, r"v_add_f64\w*") >= 40
    assert _fma(fsm, r"v_sub_f32\w*") >= 1                       # soft = Brot - Yrot, float32
    f64 = r"v_fma_f64|v_fmac_f64\w*"
    per_instance = _fma(next(v for k, v in probe.items() if "probe_atan2" in k), f64) + _fma(next(v for k, v in probe.items() if "probe_div" in k), f64)
    assert per_instance > 0
    for name, instances in FRONTS.items():
        body = kernels[name]
        assert _fma(body, r"v_fma_f32|v_fmac_f32\w*|v_pk_fma_f32|v_mad_f32|v_mac_f32\w*") == 0, name
        assert _fma(body, f64) == instances * per_instance, (name, _fma(body, f64), per_instance)


def test_fsm_kernel_registers(demod):
    _, meta, _ = demod
    got = meta[FSM]["vgpr_count"]
    print("nvx_demod_fsm VGPRs:", got, "(recorded:", FSM_VGPRS_RECORDED, ")")
    assert got <= FSM_VGPRS_MAX, got
    assert meta[FSM]["group_segment_fixed_size"] == 29568       # the 29 KB table, nothing else in LDS
