"""Guards on the row aligner's generated gfx950 code (navtex_amd/align/nvx_align.hip, cross-compiled with the shipped flags):
exactly its eight kernels, no scratch and no spills, at most 64 vector registers (eight waves per SIMD), the static LDS of each
kernel, v_dot2_i32_i16 for the correlator and for the filter, 16-byte LDS reads in both, 16-byte non-temporal stores of both
output rows, 64-bit atomics for the tables.  Positive properties only: what the kernels are meant to contain."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")

MEASURE = [f"nvx_align_measure<{fmt}>" for fmt in range(4)]            # CS16, CU8, CS8, CF32
APPLY = [f"nvx_align_apply<{fmt}>" for fmt in range(4)]
# reached: 52 (measure) and 63 or 64 (apply); 64 is eight waves per SIMD
VGPR_MAX = 64
LDS_MEASURE = 1024 * 2 * 4 + 4 * (1024 + 64 + 16) * 4                  # the main row's two words per sample, four copies of the sense span
LDS_APPLY = (4096 + 16) * 4 + 8 * 4                                    # the sense row's window of a tile, the phase's tap words


@pytest.fixture(scope="module")
def build():
    import importlib.util
    spec = importlib.util.spec_from_file_location("nvx_build_for_align_isa", ROOT / "navtex_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _short(mangled):
    name = subprocess.run(["c++filt", mangled], capture_output=True, text=True, check=True).stdout.strip()
    return re.sub(r"^void |\(.*$", "", name)


@pytest.fixture(scope="module")
def isa(build, tmp_path_factory):
    """(the kernels' bodies, the metadata of every kernel)."""
    tmp = tmp_path_factory.mktemp("align_isa")
    kernels, meta = {}, {}
    for name in build.ALIGN_HIP_SOURCES:
        out = tmp / (name + ".s")
        subprocess.run([HIPCC, f"--offload-arch={build.ARCH}", "-std=c++17", *build.COMMON, f"-I{build.ALIGN}", f"-I{build.RESAMPLE}",
                        "--cuda-device-only", "-S", str(build.ALIGN / name), "-o", str(out)], check=True, capture_output=True)
        text = out.read_text()
        for m in re.finditer(r"^(_Z\w+):.*?^\.Lfunc_end\d+:", text, flags=re.S | re.M):      # the whole body: a kernel may end in several places
            if "s_endpgm" in m.group(0):
                kernels[_short(m.group(1))] = m.group(0)
        for block in text[text.index("amdhsa.kernels"):].split("  - .agpr_count")[1:]:
            kernel = _short(re.search(r"\.name:\s+(\S+)", block).group(1))
            meta[kernel] = {f: int(re.search(rf"\.{f}:\s*(\d+)", block).group(1))
                            for f in ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count")}
    return kernels, meta


def test_the_library_holds_exactly_its_eight_kernels(isa, build):
    kernels, meta = isa
    assert sorted(meta) == sorted(MEASURE + APPLY) and sorted(kernels) == sorted(MEASURE + APPLY)
    assert build.ALIGN_LIB.name == "libnavtex_amd_align.so" and build.ALIGN_CXX_SOURCES == ["nvx_align_host.cpp"] and build.ALIGN_C_SOURCES == ["nvx_align_find.c"]


def test_no_scratch_no_spills_the_register_ceiling_and_the_static_lds(isa):
    _, meta = isa
    for name, m in sorted(meta.items()):
        print(name, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= VGPR_MAX, (name, m)
        assert m["group_segment_fixed_size"] == (LDS_MEASURE if name in MEASURE else LDS_APPLY), (name, m)


def test_the_correlator_uses_the_dot_product_sixteen_byte_lds_reads_and_atomics(isa):
    kernels, _ = isa
    for name in MEASURE:
        body = kernels[name]
        # v_dot2_i32_i16 (or the form that adds into its destination): eight per four samples, the loop unrolled eight times, and
        # the two power sums
        assert len(re.findall(r"v_dot2c?_i32_i16", body)) >= 8 * 8 + 2, name
        assert len(re.findall(r"ds_read_b128", body)) >= 3 * 8, name              # per four samples: two of the main row, one of the sense copy
        assert len(re.findall(r"global_atomic_add_x2", body)) >= 4, name          # the lag's two sums, SAA and SBB
        assert "s_barrier" in body, name


def test_the_filter_uses_the_dot_product_sixteen_byte_lds_reads_and_stores(isa):
    kernels, _ = isa
    for name in APPLY:
        body = kernels[name]
        # per step: four outputs x two components x eight tap words, in the whole tile's form and in the last tile's
        assert len(re.findall(r"v_dot2c?_i32_i16", body)) >= 2 * 64, name
        assert len(re.findall(r"ds_read_b128", body)) >= 2 * 5, name               # the twenty words behind four outputs
        assert len(re.findall(r"global_store_dwordx4 .* nt", body)) >= 2, name     # both output rows
        assert len(re.findall(r"v_med3_i32", body)) >= 8, name                     # the clamps
        assert len(re.findall(r"v_perm_b32", body)) >= 36, name                    # the I pairs and the Q pairs
        assert "s_barrier" in body, name
