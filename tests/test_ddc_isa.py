"""Guards on the down-converter bank's generated gfx950 code (navtex_amd/ddc/nvx_ddc.hip, cross-compiled with the shipped
flags): exactly the eight kernels DESIGN 3.8 lists, no scratch, no spills, no fp64, no fused multiply-add, no atomics,
float32 only in the CF32 instances, the FIR loop's three 8-byte LDS reads per four dot products, and the registers and LDS
behind the two workgroups per CU at 2.048 MS/s."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# nvx_ddc_bank<format, taps in the LDS>: CS16, CU8, CS8, CF32, each with the tap table in the LDS and in global memory
DDC_KERNELS = sorted(f"nvx_ddc_bank<{fmt}, {lds}>" for fmt in range(4) for lds in ("true", "false"))
PLANE_BYTES = 2 * 8704 * 2                # two planes of 8704 int16: 34816
TABLE_BYTES = (2048 + 2048 // 32) * 4     # the half turn, one word of padding per 32: 8448
HALF_CU = 80 * 1024
VGPR_MAX = 64                             # 512 / 64 = 8 waves per SIMD: registers never limit the occupancy


@pytest.fixture(scope="module")
def build():
    import importlib.util
    spec = importlib.util.spec_from_file_location("nvx_build_for_ddc_isa", ROOT / "navtex_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def isa(build, tmp_path_factory):
    assert Path(HIPCC).exists(), "hipcc is needed to look at the generated code"
    tmp = tmp_path_factory.mktemp("ddc_isa")
    kernels, meta = {}, ""
    for name in build.DDC_HIP_SOURCES:
        out = tmp / (name + ".s")
        subprocess.run([HIPCC, f"--offload-arch={build.ARCH}", "-std=c++17", *build.COMMON, f"-I{build.DDC}", f"-I{build.RESAMPLE}",
                        "--cuda-device-only", "-S", str(build.DDC / name), "-o", str(out)], check=True, capture_output=True)
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


def _blocks(body):
    """The kernel's basic blocks: the text between labels."""
    return re.split(r"^\.LBB\d+_\d+:.*$", body, flags=re.M)


def test_the_library_holds_exactly_the_kernels_design_lists(isa):
    kernels, meta = isa
    assert sorted(_meta(meta)) == DDC_KERNELS and sorted(kernels) == DDC_KERNELS
    design = (ROOT / "DESIGN.md").read_text()
    assert "nvx_ddc_bank<format, taps in the LDS>" in design


def test_no_scratch_no_spills_no_fp64_no_fma_no_atomics(isa):
    kernels, meta = isa
    for name, body in kernels.items():
        assert not re.search(r"v_\w+_f64", body), f"{name}: fp64"
        assert not re.search(r"v_fma_|v_fmac_|v_pk_fma|v_mad_f|v_mac_f", body), f"{name}: a fused or chained multiply-add"
        assert "scratch_" not in body and "atomic" not in body and not re.search(r"ds_(add|sub|inc|dec|min|max|and|or|xor|cmpst)", body), name
        floats = re.findall(r"\bv_\w+_f32\w*", body)
        if not name.startswith("nvx_ddc_bank<3"):
            assert not floats, f"{name}: float32 outside CF32's conversion: {sorted(set(floats))}"
    for name, m in _meta(meta).items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)


def test_the_fir_loop_is_dot_products_from_eight_byte_lds_reads(isa):
    """The 8-byte LDS reads belong to the FIR loop alone (the mixer's table reads are 4 bytes wide): in every block that
    has them, three ds_read_b64 (taps, I, Q; two with the taps in global memory) per four dot products, never paired into
    ds_read2; the mixer's dot products sit in blocks of their own, and the planes are written sixteen bytes at a time."""
    kernels, _ = isa
    for name, body in kernels.items():
        per_fir = 3 if name.endswith("true>") else 2
        assert "ds_read2" not in body, name
        fir_blocks = mixer_dots = 0
        for block in _blocks(body):
            reads, dots = block.count("ds_read_b64"), len(re.findall(r"v_dot2c?_i32_i16", block))
            if reads:
                fir_blocks += 1
                assert dots and dots % 4 == 0 and reads == (dots // 4) * per_fir, (name, reads, dots)
                assert "ds_read_b32" not in block, name
            else:
                mixer_dots += dots
        assert fir_blocks >= 1, name
        # a staged group of 8: sixteen mixer dot products, eight table reads; the edge path: two and one
        assert mixer_dots >= 18 and mixer_dots % 2 == 0 and body.count("ds_read_b32") == mixer_dots // 2, (name, mixer_dots)
        assert body.count("ds_write_b128") >= 2, name
        assert re.search(r"global_load_dwordx4", body) and not re.search(r"global_load_dwordx4 .* nt", body), \
            f"{name}: the input is to be read with plain 16-byte loads (the sibling slices share it through the caches)"


def test_lds_and_registers_allow_two_workgroups_per_cu_at_2048000(isa, build):
    """The LDS is dynamic: the planes, the half turn of the mixer table and the plan's tap table.  At 2.048 MS/s (L = 63,
    T = 58) that is 77536 bytes: two workgroups per CU of 160 KB, as the resampler has."""
    _, meta = isa
    plan = (build.DDC / "nvx_ddc_plan.h").read_text()
    rs_plan = (build.RESAMPLE / "nvx_resample_plan.h").read_text()
    assert re.search(r"#define NVX_RS_PLANE 8704\b", rs_plan) and re.search(r"#define NVX_RS_TAPS_LDS_MAX \(60 \* 1024\)", rs_plan)
    assert re.search(r"#define NVX_DDC_TAB_DW \(NVX_DDC_HALF \+ NVX_DDC_HALF / 32\)", plan) and re.search(r"#define NVX_DDC_HALF \(NVX_DDC_GRID / 2\)", plan)
    for name, m in _meta(meta).items():
        assert m["group_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] <= VGPR_MAX, (name, m)
    L, T = 63, 58
    tp = (T + 3 + 3) // 4 * 4
    taps = 4 * L * (tp // 2 + (2 if tp // 4 % 2 == 0 else 0)) * 4
    assert taps == 34272 and PLANE_BYTES + TABLE_BYTES + taps == 77536 <= HALF_CU
    assert PLANE_BYTES + TABLE_BYTES + 60 * 1024 <= 160 * 1024
