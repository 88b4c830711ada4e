"""Guards on the noise canceller's generated gfx950 code (navtex_amd/anc/nvx_anc.hip, cross-compiled with the shipped flags):
exactly its eight kernels, no scratch and no spills, at most 64 VGPRs (eight waves per SIMD by registers), v_dot2_i32_i16 in
both kernels, 16-byte loads of both rows and 64-bit atomics in the sums kernels, v_med3_i32 and 16-byte non-temporal stores in
the apply kernels.  Positive properties only: what the kernels are meant to contain."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")

SUMS_KERNELS = [f"nvx_anc_sums<{fmt}>" for fmt in range(4)]           # CS16, CU8, CS8, CF32
APPLY_KERNELS = [f"nvx_anc_apply<{fmt}>" for fmt in range(4)]
VGPR_MAX = 64                             # 512 / 64 = 8 waves per SIMD: the vector registers never limit the occupancy


@pytest.fixture(scope="module")
def build():
    import importlib.util
    spec = importlib.util.spec_from_file_location("nvx_build_for_anc_isa", ROOT / "navtex_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _short(mangled):
    name = subprocess.run(["c++filt", mangled], capture_output=True, text=True, check=True).stdout.strip()
    return re.sub(r"^void |\(.*$", "", name)


@pytest.fixture(scope="module")
def isa(build, tmp_path_factory):
    """(the kernels' bodies, the metadata of every kernel)."""
    tmp = tmp_path_factory.mktemp("anc_isa")
    kernels, meta = {}, {}
    for name in build.ANC_HIP_SOURCES:
        out = tmp / (name + ".s")
        subprocess.run([HIPCC, f"--offload-arch={build.ARCH}", "-std=c++17", *build.COMMON, f"-I{build.ANC}", f"-I{build.RESAMPLE}", "--cuda-device-only",
                        "-S", str(build.ANC / name), "-o", str(out)], check=True, capture_output=True)
        text = out.read_text()
        for m in re.finditer(r"^(_Z\w+):.*?^\.Lfunc_end\d+:", text, flags=re.S | re.M):      # the whole body: a kernel may end in several places
            if "s_endpgm" in m.group(0):
                kernels[_short(m.group(1))] = m.group(0)
        for block in text[text.index("amdhsa.kernels"):].split("  - .agpr_count")[1:]:
            kernel = _short(re.search(r"\.name:\s+(\S+)", block).group(1))
            meta[kernel] = {f: int(re.search(rf"\.{f}:\s*(\d+)", block).group(1))
                            for f in ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count")}
    return kernels, meta


def test_the_library_holds_exactly_its_eight_kernels(isa):
    kernels, meta = isa
    assert sorted(meta) == sorted(SUMS_KERNELS + APPLY_KERNELS) and sorted(kernels) == sorted(SUMS_KERNELS + APPLY_KERNELS)


def test_no_scratch_no_spills_and_eight_waves_by_vector_registers(isa):
    _, meta = isa
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= VGPR_MAX, (name, m)
        assert m["group_segment_fixed_size"] <= 64, (name, m)


def test_the_sums_kernels_use_the_dot_product_sixteen_byte_loads_and_64_bit_atomics(isa):
    kernels, _ = isa
    for name in SUMS_KERNELS:
        body = kernels[name]
        # v_dot2_i32_i16 in the form that adds into its destination (v_dot2c_i32_i16, gfx950's): three per sample, sixteen samples a thread
        assert len(re.findall(r"v_dot2c?_i32_i16", body)) >= 48, name
        assert len(re.findall(r"v_mul_i32_i24|v_mad_i32_i24", body)) >= 32, name      # Q1 I2 and I1 Q2
        assert "global_atomic_add_x2" in body, name
        assert len(re.findall(r"global_load_dwordx4", body)) >= 4, name                # both rows


def test_the_apply_kernels_use_the_dot_product_med3_and_sixteen_byte_non_temporal_stores(isa):
    kernels, _ = isa
    for name in APPLY_KERNELS:
        body = kernels[name]
        assert len(re.findall(r"v_dot2c?_i32_i16", body)) >= 32, name                  # two per sample
        assert len(re.findall(r"v_med3_i32", body)) >= 32, name
        assert len(re.findall(r"global_load_dwordx4 .* nt", body)) >= 4, name
        assert len(re.findall(r"global_store_dwordx4 .* nt", body)) >= 2, name
