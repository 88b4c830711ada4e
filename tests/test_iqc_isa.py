"""Guards on the IQ corrector's generated gfx950 code (navtex_amd/iqc/nvx_iqc.hip, cross-compiled with the shipped flags):
exactly its eight kernels, no scratch, no spills, no fp64, float32 only in the CF32 instances (the solve's division and
square root are shifts and subtractions), v_dot2_i32_i16 and 64-bit atomics in the sums kernels, v_mad_i32_i24, v_med3_i32
and 16-byte non-temporal stores in the apply kernels, and the registers behind eight waves per SIMD."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")

SUMS_KERNELS = [f"nvx_iqc_sums<{fmt}>" for fmt in range(4)]           # CS16, CU8, CS8, CF32
APPLY_KERNELS = [f"nvx_iqc_apply<{fmt}>" for fmt in range(4)]
VGPR_MAX = 64                             # 512 / 64 = 8 waves per SIMD: registers never limit the occupancy


@pytest.fixture(scope="module")
def build():
    import importlib.util
    spec = importlib.util.spec_from_file_location("nvx_build_for_iqc_isa", ROOT / "navtex_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def isa(build, tmp_path_factory):
    """(the kernels' bodies, every function's body -- the solve's helpers are functions of their own --, the metadata)."""
    tmp = tmp_path_factory.mktemp("iqc_isa")
    kernels, functions, meta = {}, {}, ""
    for name in build.IQC_HIP_SOURCES:
        out = tmp / (name + ".s")
        subprocess.run([HIPCC, f"--offload-arch={build.ARCH}", "-std=c++17", *build.COMMON, f"-I{build.IQC}", f"-I{build.RESAMPLE}", "--cuda-device-only",
                        "-S", str(build.IQC / name), "-o", str(out)], check=True, capture_output=True)
        text = out.read_text()
        for m in re.finditer(r"^(_Z\w+):.*?^\.Lfunc_end\d+:", text, flags=re.S | re.M):      # the whole body: a kernel may end in several places
            (kernels if "s_endpgm" in m.group(0) else functions)[_short(m.group(1))] = m.group(0)
        meta += text[text.index("amdhsa.kernels"):]
    return kernels, functions, meta


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
    kernels, _, meta = isa
    assert sorted(_meta(meta)) == sorted(SUMS_KERNELS + APPLY_KERNELS) and sorted(kernels) == sorted(SUMS_KERNELS + APPLY_KERNELS)


def test_no_scratch_no_spills_no_fp64_and_float32_only_for_cf32(isa):
    kernels, functions, meta = isa
    for name, body in list(kernels.items()) + list(functions.items()):
        assert not re.search(r"v_\w+_f64", body), f"{name}: fp64"
        assert "scratch_" not in body and "v_writelane" not in body, name
        floats = re.findall(r"\bv_\w+_f32\w*", body)
        if name not in ("nvx_iqc_sums<3>", "nvx_iqc_apply<3>"):
            assert not floats, f"{name}: float32 outside CF32's conversion: {sorted(set(floats))}"
        else:
            assert floats and not re.search(r"v_(div|rcp|sqrt|exp|log)\w*_f32", body), sorted(set(floats))
    for name, m in _meta(meta).items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= VGPR_MAX, (name, m)


def test_the_sums_kernels_use_the_dot_product_and_64_bit_atomics(isa):
    kernels, _, _ = isa
    for name in SUMS_KERNELS:
        body = kernels[name]
        # v_dot2_i32_i16 in the form that adds into its destination (v_dot2c_i32_i16, gfx950's): two per sample, sixteen samples a thread
        assert len(re.findall(r"v_dot2c?_i32_i16", body)) >= 32, name
        assert "v_mul_i32_i24" in body, name
        assert "global_atomic_add_x2" in body, name
        assert len(re.findall(r"global_load_dwordx4", body)) >= 2, name
        assert "global_store" not in body and "flat_" not in body and "buffer_" not in body, name


def test_the_apply_kernels_use_24_bit_multiply_adds_and_sixteen_byte_non_temporal_stores(isa):
    kernels, _, _ = isa
    for name in APPLY_KERNELS:
        body = kernels[name]
        assert len(re.findall(r"v_mad_i32_i24", body)) >= 32, name             # two per sample
        assert len(re.findall(r"v_med3_i32", body)) >= 32, name
        assert len(re.findall(r"global_load_dwordx4 .* nt", body)) >= 2, name
        assert len(re.findall(r"global_store_dwordx4 .* nt", body)) >= 2, name
        assert "flat_load" not in body and "flat_store" not in body and "buffer_" not in body, name
        assert m_lds(isa, name) <= 64


def m_lds(isa, name):
    return _meta(isa[2])[name]["group_segment_fixed_size"]
