"""Guards on the blanker's generated gfx950 code (navtex_amd/blank/nvx_blank.hip, cross-compiled with the shipped flags):
exactly its four kernels, no scratch, no spills, no fp64, no fused multiply-add, float32 only in the CF32 instance, 16-byte
non-temporal loads and 16-byte stores, the DPP steps of the sums and the scan, two barriers per tile, and the LDS and
registers behind the occupancy DESIGN 3.9 states."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")

BLANK_KERNELS = sorted(f"nvx_blank<{fmt}>" for fmt in range(4))      # CS16, CU8, CS8, CF32
LDS_BYTES = 84                            # per wave two sums and its latest detection; five levels; four fronts: 21 words
VGPR_MAX = 64                             # 512 / 64 = 8 waves per SIMD: registers never limit the occupancy


@pytest.fixture(scope="module")
def build():
    import importlib.util
    spec = importlib.util.spec_from_file_location("nvx_build_for_blank_isa", ROOT / "navtex_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def isa(build, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("blank_isa")
    kernels, meta = {}, ""
    for name in build.BLANK_HIP_SOURCES:
        out = tmp / (name + ".s")
        subprocess.run([HIPCC, f"--offload-arch={build.ARCH}", "-std=c++17", *build.COMMON, f"-I{build.BLANK}", f"-I{build.RESAMPLE}", "--cuda-device-only",
                        "-S", str(build.BLANK / name), "-o", str(out)], check=True, capture_output=True)
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


def test_the_library_holds_exactly_its_four_kernels(isa):
    kernels, meta = isa
    assert sorted(_meta(meta)) == BLANK_KERNELS and sorted(kernels) == BLANK_KERNELS


def test_no_scratch_no_spills_no_fp64_no_fma_and_float32_only_for_cf32(isa):
    kernels, meta = isa
    for name, body in kernels.items():
        assert not re.search(r"v_\w+_f64", body), f"{name}: fp64"
        assert not re.search(r"v_fma_|v_fmac_|v_pk_fma|v_mad_f|v_mac_f", body), f"{name}: a fused or chained multiply-add"
        assert "scratch_" not in body and "v_writelane" not in body, name
        floats = re.findall(r"\bv_\w+_f32\w*", body)
        if name != "nvx_blank<3>":
            assert not floats, f"{name}: float32 outside CF32's conversion: {sorted(set(floats))}"
        else:
            assert floats and not re.search(r"v_(div|rcp|sqrt|exp|log)\w*_f32", body), sorted(set(floats))
    for name, m in _meta(meta).items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)


def test_sixteen_byte_non_temporal_loads_and_sixteen_byte_stores(isa):
    """Every tile is read with global_load_dwordx4 ... nt; the words go out as global_store_dwordx4: ... nt on aligned rows, and
    unaligned (no nt: the stores of neighbouring lanes share cache lines) on the others.  Narrower vector loads and stores
    exist only on the sample-by-sample path of a call's last tile and for the state row."""
    kernels, _ = isa
    for name, body in kernels.items():
        assert len(re.findall(r"global_load_dwordx4 .* nt", body)) >= 2, name
        assert len(re.findall(r"global_store_dwordx4 .* nt", body)) >= 2, name
        assert "buffer_load" not in body and "flat_load" not in body and "flat_store" not in body, name


def test_the_reductions_are_dpp_and_a_tile_has_two_barriers(isa):
    """Per tile two sums and a max-scan per step inside the wave: row_shr 1, 2, 4, 8, row_bcast 15 and 31 (and wave_shr 1 for
    the scan's exclusive form); no ds_bpermute or ds_swizzle; the waves meet twice per tile through 84 bytes of LDS."""
    kernels, _ = isa
    for name, body in kernels.items():
        for ctrl in ("row_shr:1", "row_shr:2", "row_shr:4", "row_shr:8", "row_bcast:15", "row_bcast:31", "wave_shr:1"):
            assert ctrl in body, (name, ctrl)
        assert "ds_bpermute" not in body and "ds_permute" not in body and "ds_swizzle" not in body, name
        # two barriers in every copy of the tile's code (the whole-tile loop, which the compiler may peel, and the last, ragged tile)
        assert body.count("s_barrier") >= 4 and body.count("s_barrier") % 2 == 0, (name, body.count("s_barrier"))
        assert not re.search(r"ds_(add|sub|inc|dec|min|max|and|or|xor|cmpst)", body), name


def test_lds_and_registers_allow_eight_waves_per_simd(isa, build):
    _, meta = isa
    plan = (build.BLANK / "nvx_blank_plan.h").read_text()
    assert re.search(rf"#define NVX_BLANK_LDS_BYTES {LDS_BYTES}\b", plan) and re.search(r"#define NVX_BLANK_THREADS 256\b", plan)
    for name, m in _meta(meta).items():
        assert m["group_segment_fixed_size"] == LDS_BYTES, (name, m)
        assert m["vgpr_count"] <= VGPR_MAX, (name, m)
