"""Guards on the zoom bank's generated gfx950 code (navtex_amd/zoom/nvx_zoom.hip, cross-compiled with the shipped flags):
exactly its four kernels, no scratch and no spills, at most 72 vector registers, 20 480 bytes of static LDS (the 16 KB table
and the block's 4 KB of converted samples; the stages' lines are dynamic), v_dot2_i32_i16 for the mixer and the stages,
16-byte non-temporal loads of the input, 16-byte non-temporal stores of the output, 8-byte LDS reads of the odd samples.
Positive properties only: what the kernels are meant to contain."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")

KERNELS = [f"nvx_zoom_bank<{fmt}>" for fmt in range(4)]                # CS16, CU8, CS8, CF32
# reached: 67 (CS16) and 69; 72 is seven waves per SIMD, and the LDS (29 KB at k = 5 with one zoom) allows five workgroups per CU
VGPR_MAX = 72
LDS_STATIC = 4096 * 4 + 1024 * 4


@pytest.fixture(scope="module")
def build():
    import importlib.util
    spec = importlib.util.spec_from_file_location("nvx_build_for_zoom_isa", ROOT / "navtex_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _short(mangled):
    name = subprocess.run(["c++filt", mangled], capture_output=True, text=True, check=True).stdout.strip()
    return re.sub(r"^void |\(.*$", "", name)


@pytest.fixture(scope="module")
def isa(build, tmp_path_factory):
    """(the kernels' bodies, the metadata of every kernel)."""
    tmp = tmp_path_factory.mktemp("zoom_isa")
    kernels, meta = {}, {}
    for name in build.ZOOM_HIP_SOURCES:
        out = tmp / (name + ".s")
        subprocess.run([HIPCC, f"--offload-arch={build.ARCH}", "-std=c++17", *build.COMMON, f"-I{build.ZOOM}", f"-I{build.RESAMPLE}", f"-I{build.DDC}",
                        f"-I{build.REAL}", "--cuda-device-only", "-S", str(build.ZOOM / name), "-o", str(out)], check=True, capture_output=True)
        text = out.read_text()
        for m in re.finditer(r"^(_Z\w+):.*?^\.Lfunc_end\d+:", text, flags=re.S | re.M):      # the whole body: a kernel may end in several places
            if "s_endpgm" in m.group(0):
                kernels[_short(m.group(1))] = m.group(0)
        for block in text[text.index("amdhsa.kernels"):].split("  - .agpr_count")[1:]:
            kernel = _short(re.search(r"\.name:\s+(\S+)", block).group(1))
            meta[kernel] = {f: int(re.search(rf"\.{f}:\s*(\d+)", block).group(1))
                            for f in ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count")}
    return kernels, meta


def test_the_library_holds_exactly_its_four_kernels(isa, build):
    kernels, meta = isa
    assert sorted(meta) == sorted(KERNELS) and sorted(kernels) == sorted(KERNELS)
    assert build.ZOOM_LIB.name == "libnavtex_amd_zoom.so" and build.ZOOM_CXX_SOURCES == ["nvx_zoom_host.cpp"]


def test_no_scratch_no_spills_the_register_ceiling_and_the_static_lds(isa):
    _, meta = isa
    for name, m in sorted(meta.items()):
        print(name, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= VGPR_MAX, (name, m)
        assert m["group_segment_fixed_size"] == LDS_STATIC, (name, m)
    plan = (ROOT / "navtex_amd" / "zoom" / "nvx_zoom_plan.h").read_text()
    assert "#define NVX_ZOOM_LDS_STATIC (NVX_ZOOM_GRID * 4 + NVX_ZOOM_BLOCK * 4)" in plan and "#define NVX_ZOOM_BLOCK 1024" in plan


def test_the_kernels_use_the_dot_product_sixteen_byte_loads_and_stores(isa):
    kernels, _ = isa
    for fmt, name in enumerate(KERNELS):
        body = kernels[name]
        # v_dot2_i32_i16 (or the form that adds into its destination, v_dot2c_i32_i16): two per mixed sample of a thread's four,
        # fourteen per stage output of a group's four, I and Q
        assert len(re.findall(r"v_dot2c?_i32_i16", body)) >= 2 * 4 + 14 * 4 * 2, name
        assert len(re.findall(r"global_load_dwordx4 .* nt", body)) >= (2 if fmt == 3 else 1), name       # the call's input
        assert len(re.findall(r"global_store_dwordx4 .* nt", body)) >= 1, name
        assert len(re.findall(r"ds_read_b64", body)) >= 16, name                                          # the odd samples: 8 a component
        assert len(re.findall(r"v_med3_i32", body)) >= 2 * 4 + 8, name                                    # the clamps
        assert "s_barrier" in body, name
