"""Guards on the multi-tap canceller's generated gfx950 code (navtex_amd/wanc/nvx_wanc.hip, cross-compiled with the shipped
flags): exactly its twenty-seven kernels (sums and apply per format and tap count, the solve per tap count), no scratch and no
spills, v_dot2_i32_i16 and 64-bit atomics in the sums kernels, v_dot2_i32_i16, v_med3_i32 and 16-byte non-temporal stores in the
apply kernels, fp64 multiplies and no fused multiply-add in the solve kernels.  Positive properties and the one the header's
rounding rests on: what the kernels are meant to contain."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")

TAPS = (4, 8, 16)
SUMS_KERNELS = [f"nvx_wanc_sums<{fmt}, {k}>" for fmt in range(4) for k in TAPS]           # CS16, CU8, CS8, CF32
APPLY_KERNELS = [f"nvx_wanc_apply<{fmt}, {k}>" for fmt in range(4) for k in TAPS]
SOLVE_KERNELS = [f"nvx_wanc_solve_blocks<{k}>" for k in TAPS]
LDS_STAGED = 4 * (16 + 4096 + 4096)       # a tile of both rows as packed words, and the sense halo


@pytest.fixture(scope="module")
def build():
    import importlib.util
    spec = importlib.util.spec_from_file_location("nvx_build_for_wanc_isa", ROOT / "navtex_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _short(mangled):
    name = subprocess.run(["c++filt", mangled], capture_output=True, text=True, check=True).stdout.strip()
    return re.sub(r"^void |\(.*$", "", name)


@pytest.fixture(scope="module")
def isa(build, tmp_path_factory):
    """(the kernels' bodies, the metadata of every kernel)."""
    tmp = tmp_path_factory.mktemp("wanc_isa")
    kernels, meta = {}, {}
    for name in build.WANC_HIP_SOURCES:
        out = tmp / (name + ".s")
        subprocess.run([HIPCC, f"--offload-arch={build.ARCH}", "-std=c++17", *build.COMMON, f"-I{build.WANC}", f"-I{build.RESAMPLE}", "--cuda-device-only",
                        "-S", str(build.WANC / name), "-o", str(out)], check=True, capture_output=True)
        text = out.read_text()
        for m in re.finditer(r"^(_Z\w+):.*?^\.Lfunc_end\d+:", text, flags=re.S | re.M):      # the whole body: a kernel may end in several places
            if "s_endpgm" in m.group(0):
                kernels[_short(m.group(1))] = m.group(0)
        for block in text[text.index("amdhsa.kernels"):].split("  - .agpr_count")[1:]:
            kernel = _short(re.search(r"\.name:\s+(\S+)", block).group(1))
            meta[kernel] = {f: int(re.search(rf"\.{f}:\s*(\d+)", block).group(1))
                            for f in ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count")}
    return kernels, meta


def test_the_library_holds_exactly_its_kernels(isa):
    kernels, meta = isa
    want = sorted(SUMS_KERNELS + APPLY_KERNELS + SOLVE_KERNELS)
    assert sorted(meta) == want and sorted(kernels) == want


def test_no_scratch_and_no_spills(isa):
    _, meta = isa
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 512, (name, m)
        if "solve" not in name:
            assert m["group_segment_fixed_size"] == LDS_STAGED, (name, m)
        else:
            assert m["group_segment_fixed_size"] <= 48 * 1024, (name, m)


def test_the_sums_kernels_use_the_dot_product_and_64_bit_atomics(isa):
    kernels, _ = isa
    for name in SUMS_KERNELS:
        body = kernels[name]
        k = int(re.search(r", (\d+)>", name).group(1))
        # v_dot2_i32_i16 (v_dot2c_i32_i16 where it adds into its destination): two real parts per sample and tap and one power, four samples a step
        assert len(re.findall(r"v_dot2c?_i32_i16", body)) >= 4 * (2 * k + 1), name
        assert len(re.findall(r"v_mul_i32_i24|v_mad_i32_i24", body)) >= 4 * 2 * k, name       # the imaginary parts
        assert "global_atomic_add_x2" in body, name
        assert len(re.findall(r"global_load_dwordx4", body)) >= 4, name                        # both rows
        assert len(re.findall(r"ds_read_b128|ds_read2_b64", body)) >= 2, name


def test_the_apply_kernels_use_the_dot_product_med3_and_sixteen_byte_non_temporal_stores(isa):
    kernels, _ = isa
    for name in APPLY_KERNELS:
        body = kernels[name]
        k = int(re.search(r", (\d+)>", name).group(1))
        assert len(re.findall(r"v_dot2c?_i32_i16", body)) >= 4 * 2 * k, name                   # two per sample and tap
        assert len(re.findall(r"v_med3_i32", body)) >= 8, name
        assert len(re.findall(r"global_load_dwordx4 .* nt", body)) >= 4, name
        assert len(re.findall(r"global_store_dwordx4 .* nt", body)) >= 1, name


def test_the_solve_kernels_round_every_product_and_sum_on_its_own(isa):
    kernels, _ = isa
    for name in SOLVE_KERNELS:
        body = kernels[name]
        assert not re.search(r"v_fma_f64|v_fmac_f64", body), f"{name}: FMA breaks the header's rounding"
        assert body.count("v_mul_f64") >= 20 and body.count("v_add_f64") >= 15, name
        assert "v_rndne_f64" in body and "global_atomic_add_x2" in body, name
