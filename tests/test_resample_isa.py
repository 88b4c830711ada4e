"""Guards on the resampler's generated gfx950 code (navtex_amd/resample/nvx_resample.hip, cross-compiled with the shipped
flags): exactly its eight kernels, no scratch, no spills, no fp64, no fused multiply-add, no atomics, the dot-product
instruction and the 8-byte LDS reads in the FIR loop, and the LDS and registers behind the occupancy DESIGN 3.7 states."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")

# nvx_resample<format, taps in the LDS>: CS16, CU8, CS8, CF32, each with the tap table in the LDS and in global memory
RESAMPLE_KERNELS = sorted(f"nvx_resample<{fmt}, {lds}>" for fmt in range(4) for lds in ("true", "false"))
PLANE_BYTES = 2 * 8704 * 2                # two planes of 8704 int16: 34816
TAPS_LDS_MAX = 60 * 1024
VGPR_MAX = 64                             # 512 / 64 = 8 waves per SIMD: registers never limit the occupancy


@pytest.fixture(scope="module")
def build():
    import importlib.util
    spec = importlib.util.spec_from_file_location("nvx_build_for_resample_isa", ROOT / "navtex_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def isa(build, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("resample_isa")
    kernels, meta = {}, ""
    for name in build.RESAMPLE_HIP_SOURCES:
        out = tmp / (name + ".s")
        subprocess.run([HIPCC, f"--offload-arch={build.ARCH}", "-std=c++17", *build.COMMON, f"-I{build.RESAMPLE}", "--cuda-device-only", "-S",
                        str(build.RESAMPLE / name), "-o", str(out)], check=True, capture_output=True)
        text = out.read_text()
        for m in re.finditer(r"^(_Z\w+|nvx_\w+):.*?s_endpgm", text, flags=re.S | re.M):
            kernels[_short(m.group(1))] = m.group(0)
        meta += text[text.index("amdhsa.kernels"):]
    assert "-ffp-contract=off" in build.COMMON
    return kernels, meta


def _short(mangled):
    name = subprocess.run(["c++filt", mangled], capture_output=True, text=True, check=True).stdout.strip()
    return re.sub(r"^void |\(.*$", "", name)


def _meta(meta):
    out = {}
    for block in meta.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[_short(name)] = {f: int(re.search(rf"\.{f}:\s*(\d+)", block).group(1))
                             for f in ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count")}
    return out


def test_the_library_holds_exactly_its_eight_kernels(isa):
    kernels, meta = isa
    assert sorted(_meta(meta)) == RESAMPLE_KERNELS and sorted(kernels) == RESAMPLE_KERNELS


def test_no_scratch_no_spills_no_fp64_no_fma_no_atomics(isa):
    kernels, meta = isa
    for name, body in kernels.items():
        assert not re.search(r"v_\w+_f64", body), f"{name}: fp64"
        assert not re.search(r"v_fma_|v_fmac_|v_pk_fma|v_mad_f|v_mac_f", body), f"{name}: a fused or chained multiply-add"
        assert "scratch_" not in body and "atomic" not in body and not re.search(r"ds_(add|sub|inc|dec|min|max|and|or|xor|cmpst)", body), name
        floats = re.findall(r"\bv_\w+_f32\w*", body)
        if not name.startswith("nvx_resample<3"):
            assert not floats, f"{name}: float32 outside CF32's conversion: {sorted(set(floats))}"
    for name, m in _meta(meta).items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)


def test_the_fir_loop_is_dot_products_from_eight_byte_lds_reads(isa):
    """Per loop step three ds_read_b64 (taps, I, Q; taps from global memory in the other form) and four v_dot2(c)_i32_i16;
    no ds_read2 pairing (half the rate), and the staged planes are written sixteen bytes at a time."""
    kernels, _ = isa
    for name, body in kernels.items():
        dots = len(re.findall(r"v_dot2c?_i32_i16", body))
        assert dots >= 8 and dots % 4 == 0, (name, dots)
        assert "ds_read2" not in body and "ds_read_b32" not in body, name
        reads = body.count("ds_read_b64")
        assert reads == (dots // 4) * (3 if name.endswith("true>") else 2), (name, reads, dots)
        assert body.count("ds_write_b128") >= 2, name
        assert re.search(r"global_load_dwordx4 .* nt", body), f"{name}: the input is not read with non-temporal 16-byte loads"


def test_lds_and_registers_allow_the_occupancy_design_states(isa, build):
    """The LDS is dynamic: the planes plus the plan's tap table.  At 2.048 MS/s (L = 63, T = 58) that is 69088 bytes, two
    workgroups per CU of 160 KB; the largest launch is the planes plus a 60 KB table, one workgroup."""
    _, meta = isa
    plan = (build.RESAMPLE / "nvx_resample_plan.h").read_text()
    assert re.search(r"#define NVX_RS_PLANE 8704\b", plan) and re.search(r"#define NVX_RS_TAPS_LDS_MAX \(60 \* 1024\)", plan)
    for name, m in _meta(meta).items():
        assert m["group_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] <= VGPR_MAX, (name, m)
    L, T = 63, 58
    tp = (T + 3 + 3) // 4 * 4
    table = 4 * L * (tp // 2 + (2 if tp // 4 % 2 == 0 else 0)) * 4
    assert tp == 64 and table == 34272 and PLANE_BYTES + table == 69088
    assert 2 * (PLANE_BYTES + table) <= 160 * 1024 < 3 * (PLANE_BYTES + table)
    assert PLANE_BYTES + TAPS_LDS_MAX <= 160 * 1024
