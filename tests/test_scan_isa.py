"""Guards on the band scan's generated gfx950 code (navtex_amd/scan/nvx_scan.hip, cross-compiled with the shipped
flags): exactly its three kernels, no scratch, no fused multiply-add (the header's arithmetic is products and sums
rounded one by one), the LDS per workgroup DESIGN 3.6 states, and registers for three workgroups per CU."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")

SCAN_KERNELS = ["nvx_scan_fold", "nvx_scan_frame", "nvx_scan_stream"]
LDS_BYTES = 8256 * 4 + 1024 * 16          # the slot's samples as int16 pairs (the transform reuses them) + the twiddles: 49408


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    import importlib.util
    spec = importlib.util.spec_from_file_location("nvx_build_for_scan_isa", ROOT / "navtex_amd" / "build.py")
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    tmp = tmp_path_factory.mktemp("scan_isa")
    kernels, meta = {}, ""
    for name in build.SCAN_HIP_SOURCES:
        out = tmp / (name + ".s")
        subprocess.run([HIPCC, f"--offload-arch={build.ARCH}", "-std=c++17", *build.COMMON, f"-I{build.SCAN}", "--cuda-device-only", "-S",
                        str(build.SCAN / name), "-o", str(out)], check=True, capture_output=True)
        text = out.read_text()
        for m in re.finditer(r"^(_Z\w+|nvx_\w+):.*?s_endpgm", text, flags=re.S | re.M):
            kernels[m.group(1)] = m.group(0)
        meta += text[text.index("amdhsa.kernels"):]
    assert "-ffp-contract=off" in build.COMMON
    return kernels, meta



def _meta(meta):
    out = {}
    for block in meta.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        short = re.sub(r"^void |\(.*$", "", subprocess.run(["c++filt", name], capture_output=True, text=True, check=True).stdout.strip())
        out[short] = {f: int(re.search(rf"\.{f}:\s*(\d+)", block).group(1))
                      for f in ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count")}
    return out


def test_the_scan_library_holds_exactly_its_three_kernels(isa):
    _, meta = isa
    assert sorted(_meta(meta)) == SCAN_KERNELS


def test_no_scratch_and_no_fused_multiply_add(isa):
    kernels, meta = isa
    assert len(kernels) == 3
    for name, body in kernels.items():
        assert not re.search(r"v_fma_f64|v_fmac_f64|v_fma_f32|v_fmac_f32|v_pk_fma", body), f"{name}: FMA breaks the header's rounding"
        assert "scratch_" not in body, name
    for name, m in _meta(meta).items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)


def test_lds_and_registers_allow_three_workgroups_per_cu(isa):
    _, meta = isa
    m = _meta(meta)
    assert m["nvx_scan_stream"]["group_segment_fixed_size"] == LDS_BYTES == 49408
    assert m["nvx_scan_frame"]["group_segment_fixed_size"] == LDS_BYTES
    assert m["nvx_scan_fold"]["group_segment_fixed_size"] == 0
    assert 3 * LDS_BYTES <= 160 * 1024
    for k in ("nvx_scan_stream", "nvx_scan_frame"):     # 4 waves per workgroup, one per SIMD: three workgroups need 3 x VGPRs <= 512
        assert m[k]["vgpr_count"] <= 168, (k, m[k])


def test_fir1_and_the_transform_are_fully_unrolled_fp64(isa):
    """FIR1: 8 outputs x 37 taps x 2 components per thread, each a product and a sum of its own; sixteen-byte LDS reads
    (the used dwords read in pairs would run at a quarter of that rate)."""
    kernels, _ = isa
    for name, body in kernels.items():
        if "fold" in name:
            continue
        assert body.count("v_mul_f64") >= 8 * 37 * 2 + 8 * 2, name
        assert body.count("ds_read_b128") >= 80 and "ds_read2_b32" not in body, name
        assert "global_atomic" not in body and "ds_add" not in body
