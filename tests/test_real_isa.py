"""Guards on the real-input converter's generated gfx950 code (navtex_amd/real/nvx_real.hip, cross-compiled with the shipped
flags): exactly its four kernels, no scratch, no spills, no fp64, float32 only in the F32 instance, the int16 dot products
of the Q sum, 8-byte LDS reads, 16-byte non-temporal loads and stores, and the registers behind eight waves per SIMD."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")

KERNELS = [f"nvx_real<{fmt}>" for fmt in range(4)]              # S16, U8, S8, F32
VGPR_MAX = 64                             # 512 / 64 = 8 waves per SIMD: registers never limit the occupancy
LDS_BYTES = 2 * 2 * (32 + 4096)           # two int16 rows of a halo slot and a tile: nine workgroups fit a CU's 160 KiB


@pytest.fixture(scope="module")
def build():
    import importlib.util
    spec = importlib.util.spec_from_file_location("nvx_build_for_real_isa", ROOT / "navtex_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def isa(build, tmp_path_factory):
    """(the kernels' bodies, every other function's body, the metadata)."""
    tmp = tmp_path_factory.mktemp("real_isa")
    kernels, functions, meta = {}, {}, ""
    for name in build.REAL_HIP_SOURCES:
        out = tmp / (name + ".s")
        subprocess.run([HIPCC, f"--offload-arch={build.ARCH}", "-std=c++17", *build.COMMON, f"-I{build.REAL}", f"-I{build.RESAMPLE}", "--cuda-device-only",
                        "-S", str(build.REAL / name), "-o", str(out)], check=True, capture_output=True)
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


def test_the_library_holds_exactly_its_four_kernels(isa):
    kernels, functions, meta = isa
    assert sorted(_meta(meta)) == sorted(KERNELS) and sorted(kernels) == sorted(KERNELS) and not functions


def test_no_scratch_no_spills_no_fp64_and_float32_only_for_f32(isa):
    kernels, _, meta = isa
    for name, body in kernels.items():
        assert not re.search(r"v_\w+_f64", body), f"{name}: fp64"
        assert "scratch_" not in body and "v_writelane" not in body, name
        floats = re.findall(r"\bv_\w+_f32\w*", body)
        if name != "nvx_real<3>":
            assert not floats, f"{name}: float32 outside F32's conversion: {sorted(set(floats))}"
        else:
            assert floats and not re.search(r"v_(div|rcp|sqrt|exp|log)\w*_f32", body), sorted(set(floats))
    for name, m in _meta(meta).items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= VGPR_MAX, (name, m)
        assert m["group_segment_fixed_size"] == LDS_BYTES, (name, m)


def test_the_q_sum_runs_on_the_int16_dot_product(isa):
    kernels, _, _ = isa
    for name in KERNELS:
        body = kernels[name]
        # fourteen per output, four outputs a group, four groups a tile; the whole tile and the call's last are two bodies
        assert len(re.findall(r"v_dot2c?_i32_i16", body)) == 2 * 4 * 4 * 14, name
        assert not re.findall(r"v_mul_lo_u32|v_mad_u64_u32|v_mul_hi", body), name       # no 32-bit multiplies: the taps meet packed int16
        assert len(re.findall(r"v_med3_i32", body)) >= 2 * 4 * 4, name                  # the clamps
        assert len(re.findall(r"\bds_read_b64\b", body)) >= 2 * 4 * 8 and "ds_read2_b64" not in body, name
        assert len(re.findall(r"s_barrier", body)) == 4, name


def test_sixteen_byte_non_temporal_loads_and_stores(isa):
    kernels, _, _ = isa
    for name in KERNELS:
        body = kernels[name]
        assert len(re.findall(r"global_load_dwordx4 .* nt", body)) >= 2, name
        assert len(re.findall(r"global_store_dwordx4 .* nt", body)) >= 2 * 4, name
        assert "flat_load" not in body and "flat_store" not in body and "buffer_" not in body and "global_atomic" not in body, name
