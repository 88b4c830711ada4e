"""Guards on the diversity combiner's generated gfx950 code (navtex_amd/div/nvx_div.hip, cross-compiled with the shipped flags):
exactly its nine kernels, no scratch and no spills, at most 64 VGPRs (eight waves per SIMD by registers), the 16 KB table in
the LDS of the sums kernels, v_dot2_i32_i16 in the sums and the apply kernels, 16-byte loads of both rows in the sums kernels,
v_med3_i32, 16-byte non-temporal loads and 16-byte non-temporal stores in the apply kernels.  Positive properties only: what the
kernels are meant to contain."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")

SUMS_KERNELS = [f"nvx_div_sums<{fmt}>" for fmt in range(4)]           # CS16, CU8, CS8, CF32
APPLY_KERNELS = [f"nvx_div_apply<{fmt}>" for fmt in range(4)]
FOLD_KERNEL = "nvx_div_fold"
VGPR_MAX = 64                             # 512 / 64 = 8 waves per SIMD: the vector registers never limit the occupancy
SAMPLES_PER_LANE = {0: 4, 1: 8, 2: 8, 3: 4}                           # of one step, by format


@pytest.fixture(scope="module")
def build():
    import importlib.util
    spec = importlib.util.spec_from_file_location("nvx_build_for_div_isa", ROOT / "navtex_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _short(mangled):
    name = subprocess.run(["c++filt", mangled], capture_output=True, text=True, check=True).stdout.strip()
    return re.sub(r"^void |\(.*$", "", name)


@pytest.fixture(scope="module")
def isa(build, tmp_path_factory):
    """(the kernels' bodies, the metadata of every kernel)."""
    tmp = tmp_path_factory.mktemp("div_isa")
    kernels, meta = {}, {}
    for name in build.DIV_HIP_SOURCES:
        out = tmp / (name + ".s")
        subprocess.run([HIPCC, f"--offload-arch={build.ARCH}", "-std=c++17", *build.COMMON, f"-I{build.DIV}", f"-I{build.RESAMPLE}", f"-I{build.DDC}",
                        "--cuda-device-only", "-S", str(build.DIV / name), "-o", str(out)], check=True, capture_output=True)
        text = out.read_text()
        for m in re.finditer(r"^(_Z\w+):.*?^\.Lfunc_end\d+:", text, flags=re.S | re.M):      # the whole body: a kernel may end in several places
            if "s_endpgm" in m.group(0):
                kernels[_short(m.group(1))] = m.group(0)
        for block in text[text.index("amdhsa.kernels"):].split("  - .agpr_count")[1:]:
            kernel = _short(re.search(r"\.name:\s+(\S+)", block).group(1))
            meta[kernel] = {f: int(re.search(rf"\.{f}:\s*(\d+)", block).group(1))
                            for f in ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count")}
    return kernels, meta


def test_the_library_holds_exactly_its_nine_kernels(isa):
    kernels, meta = isa
    want = sorted(SUMS_KERNELS + APPLY_KERNELS + [FOLD_KERNEL])
    assert sorted(meta) == want and sorted(kernels) == want


def test_no_scratch_no_spills_and_eight_waves_by_vector_registers(isa):
    _, meta = isa
    print({name: (m["vgpr_count"], m["group_segment_fixed_size"]) for name, m in meta.items()})
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= VGPR_MAX, (name, m)
    for name in SUMS_KERNELS:
        assert meta[name]["group_segment_fixed_size"] == 4096 * 4, name               # the table, and nothing else
    for name in APPLY_KERNELS:
        assert meta[name]["group_segment_fixed_size"] == 0, name
    assert meta[FOLD_KERNEL]["group_segment_fixed_size"] == 16 * 4 * 8                # the ring of W = 16 cells


def test_the_sums_kernels_mix_down_with_the_dot_product_from_sixteen_byte_loads(isa):
    kernels, _ = isa
    for fmt, name in enumerate(SUMS_KERNELS):
        body = kernels[name]
        # four per sample of a lane's group and target: both rows against (c, s) and against (-s, c); the v_dot2c_i32_i16 form
        # adds into its destination
        assert len(re.findall(r"v_dot2c?_i32_i16", body)) >= 4 * SAMPLES_PER_LANE[fmt], name
        assert len(re.findall(r"global_load_dwordx4", body)) >= 2, name                # both rows (and the table's words)
        assert len(re.findall(r"ds_read_b32|ds_read2_b32", body)) >= SAMPLES_PER_LANE[fmt] // 2, name      # the table from the LDS
        assert "global_atomic_add_x2" in body and "global_store_dwordx4" in body, name  # both ways to the records


def test_the_apply_kernels_use_the_dot_product_med3_and_sixteen_byte_non_temporal_accesses(isa):
    kernels, _ = isa
    for name in APPLY_KERNELS:
        body = kernels[name]
        assert len(re.findall(r"v_dot2c?_i32_i16", body)) >= 32, name                  # two per sample, sixteen samples a thread and tile
        assert len(re.findall(r"v_med3_i32", body)) >= 32, name
        assert len(re.findall(r"global_load_dwordx4 .* nt", body)) >= 4, name
        assert len(re.findall(r"global_store_dwordx4 .* nt", body)) >= 2, name
