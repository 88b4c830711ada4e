"""Guards on the tone notch's generated gfx950 code (navtex_amd/notch/nvx_notch.hip, cross-compiled with the shipped flags):
exactly its nine kernels, no scratch and no spills, at most 64 (sums, update) and 104 (apply) vector registers, the 16 KB table in the LDS of the sums
and the apply kernels, v_dot2_i32_i16 and 16-byte loads in the sums kernels, 16-byte loads, v_med3_i32 and 16-byte non-temporal
stores in the apply kernels.  Positive properties only: what the kernels are meant to contain."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")

SUMS_KERNELS = [f"nvx_notch_sums<{fmt}>" for fmt in range(4)]         # CS16, CU8, CS8, CF32
APPLY_KERNELS = [f"nvx_notch_apply<{fmt}>" for fmt in range(4)]
UPDATE_KERNEL = "nvx_notch_update"
# the ceilings reached, by kernel: the sums kernels 38 (CS16, CF32) and 58 (8-bit), the update kernel 56, the apply kernels 90 and 102:
# 64 is eight waves per SIMD, 104 four (four workgroups per CU by registers, of which the 17 KB of LDS allow nine)
VGPR_MAX = {"sums": 64, "update": 64, "apply": 104}
TABLE_BYTES = 4096 * 4


@pytest.fixture(scope="module")
def build():
    import importlib.util
    spec = importlib.util.spec_from_file_location("nvx_build_for_notch_isa", ROOT / "navtex_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _short(mangled):
    name = subprocess.run(["c++filt", mangled], capture_output=True, text=True, check=True).stdout.strip()
    return re.sub(r"^void |\(.*$", "", name)


@pytest.fixture(scope="module")
def isa(build, tmp_path_factory):
    """(the kernels' bodies, the metadata of every kernel)."""
    tmp = tmp_path_factory.mktemp("notch_isa")
    kernels, meta = {}, {}
    for name in build.NOTCH_HIP_SOURCES:
        out = tmp / (name + ".s")
        subprocess.run([HIPCC, f"--offload-arch={build.ARCH}", "-std=c++17", *build.COMMON, f"-I{build.NOTCH}", f"-I{build.RESAMPLE}", f"-I{build.DDC}",
                        "--cuda-device-only", "-S", str(build.NOTCH / name), "-o", str(out)], check=True, capture_output=True)
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
    want = sorted(SUMS_KERNELS + APPLY_KERNELS + [UPDATE_KERNEL])
    assert sorted(meta) == want and sorted(kernels) == want


def test_no_scratch_no_spills_and_the_register_ceiling(isa):
    _, meta = isa
    for name, m in sorted(meta.items()):
        print(name, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= VGPR_MAX[name.split("_")[2].split("<")[0]], (name, m)
    for name in SUMS_KERNELS:
        assert meta[name]["group_segment_fixed_size"] == TABLE_BYTES, name
    for name in APPLY_KERNELS:                                         # the table and 4 x 18 values of M, 16 bytes each
        assert meta[name]["group_segment_fixed_size"] == TABLE_BYTES + 4 * 18 * 16, name
    assert meta[UPDATE_KERNEL]["group_segment_fixed_size"] == 0


def test_the_sums_kernels_use_the_dot_product_and_sixteen_byte_loads(isa):
    kernels, _ = isa
    for fmt, name in enumerate(SUMS_KERNELS):
        body = kernels[name]
        spt = 8 if fmt in (1, 2) else 4
        # v_dot2_i32_i16 (or the form that adds into its destination, v_dot2c_i32_i16): two per sample of a lane's group
        assert len(re.findall(r"v_dot2c?_i32_i16", body)) >= 2 * spt, name
        assert "global_load_dwordx4" in body and "ds_read_b32" in body, name
        assert "global_atomic_add_x2" in body and "global_store_dwordx4" in body, name      # the two ways a record is written
        assert len(re.findall(r"v_add_u32_dpp|v_mov_b32_dpp", body)) >= 6, name            # the wave reduction


def test_the_apply_kernels_use_sixteen_byte_loads_med3_and_non_temporal_stores(isa):
    kernels, _ = isa
    for fmt, name in enumerate(APPLY_KERNELS):
        body = kernels[name]
        spt = 8 if fmt in (1, 2) else 4
        assert len(re.findall(r"v_med3_i32", body)) >= 2 * spt, name
        assert len(re.findall(r"global_load_dwordx4 .* nt", body)) >= 1, name              # the call's input
        assert len(re.findall(r"global_load_dwordx4", body)) >= 2, name                    # ... and the delay line
        assert len(re.findall(r"global_store_dwordx4 .* nt", body)) >= spt // 4, name
        assert "ds_read_b128" in body or "ds_read2_b64" in body, name                      # the values of M
