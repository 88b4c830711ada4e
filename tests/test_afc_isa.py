"""Guards on the generated gfx950 code of the AFC update kernel (navtex_amd/afc/nvx_afc.hip, cross-compiled with the shipped
flags): exactly its one kernel, no scratch, no spills, no LDS, no atomics, plain vector stores, and no fused fp64
multiply-add in the law's arithmetic -- the only ones are the five of each of the two IEEE divisions' own refinement
(v_div_scale .. v_div_fixup), whose result is the correctly rounded quotient.  The register counts are recorded."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")

KERNEL = "nvx_afc_update"
VGPR_MAX, SGPR_MAX = 64, 48               # recorded: 40 VGPRs, 22 SGPRs -- far from limiting a kernel of one lane per slot
DIVISIONS = 2                             # sum_dphi_b / nb and sum_dphi_y / ny
FMA_PER_DIVISION = 5                      # the refinement steps between v_rcp_f64 and v_div_fmas_f64


@pytest.fixture(scope="module")
def build():
    import importlib.util
    spec = importlib.util.spec_from_file_location("nvx_build_for_afc_isa", ROOT / "navtex_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def isa(build, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("afc_isa")
    kernels, meta = {}, ""
    for name in build.AFC_HIP_SOURCES:
        out = tmp / (name + ".s")
        subprocess.run([HIPCC, f"--offload-arch={build.ARCH}", "-std=c++17", *build.COMMON, "--cuda-device-only",
                        "-S", str(build.AFC / name), "-o", str(out)], check=True, capture_output=True)
        text = out.read_text()
        for m in re.finditer(r"^(_Z\w+|nvx_\w+):.*?s_endpgm", text, flags=re.S | re.M):
            kernels[_short(m.group(1))] = m.group(0)
        meta += text[text.index("amdhsa.kernels"):]
    assert "-ffp-contract=off" in build.COMMON
    assert "nvx_afc.hip" in build.AFC_HIP_SOURCES and "nvx_afc.cpp" in build.CXX_SOURCES
    return kernels, meta


def _short(mangled):
    name = subprocess.run(["c++filt", mangled], capture_output=True, text=True, check=True).stdout.strip()
    return re.sub(r"^void |\(.*$", "", name)


def _meta(meta):
    out = {}
    for block in meta.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[_short(name)] = {f: int(re.search(rf"\.{f}:\s*(\d+)", block).group(1))
                             for f in ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count")}
    return out


def test_one_kernel_no_scratch_no_lds_no_spills_and_its_registers(isa):
    kernels, meta = isa
    assert sorted(kernels) == [KERNEL] and sorted(_meta(meta)) == [KERNEL]
    m = _meta(meta)[KERNEL]
    print(f"{KERNEL}: {m['vgpr_count']} VGPRs, {m['sgpr_count']} SGPRs")
    assert m["private_segment_fixed_size"] == 0 and m["group_segment_fixed_size"] == 0, m
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert m["vgpr_count"] <= VGPR_MAX and m["sgpr_count"] <= SGPR_MAX, m
    body = kernels[KERNEL]
    assert "scratch_" not in body and "v_writelane" not in body and not re.search(r"\bds_\w+", body) and "s_barrier" not in body


def test_plain_vector_stores_and_no_atomics(isa):
    """K[L+2] (4 bytes) and the note (8 bytes) leave through global_store; every load of device memory is a vector load
    (the scalar loads are the kernel's arguments); nothing atomic, nothing flat, no buffer instruction."""
    body = isa[0][KERNEL]
    stores = re.findall(r"^\s+(global_store_\w+)", body, flags=re.M)
    assert sorted(stores) == ["global_store_dword", "global_store_dwordx2"], stores
    assert not re.search(r"atomic|\bflat_|\bbuffer_", body)
    assert len(re.findall(r"^\s+global_load_", body, flags=re.M)) >= 4
    for line in re.findall(r"^\s+(s_load_\w+\s+.*)$", body, flags=re.M):
        assert re.search(r"s\[\d+:\d+\], (0x[0-9a-f]+|\d+)\s*$", line.split(";")[0].strip()), line      # kernarg segment: base pair + immediate


def test_no_fused_fp64_multiply_add_in_the_laws_arithmetic(isa):
    """The law's products and sums are v_mul_f64 / v_add_f64, rint is v_rndne_f64, ldexp v_ldexp_f64.  The fused
    instructions present are exactly those of the two divisions' expansion, all between the first v_rcp_f64 and the last
    v_div_fixup_f64."""
    body = isa[0][KERNEL]
    lines = [l.strip().split()[0] for l in body.splitlines() if l.strip() and not l.strip().startswith((";", ".", "//")) and not l.rstrip().endswith(":")]
    fused = [i for i, op in enumerate(lines) if re.match(r"v_(fma|fmac|mad|mac|pk_fma)\w*_f(16|32|64)", op)]      # (integer mads are address arithmetic)
    assert all(re.match(r"v_fmac?_f64", lines[i]) for i in fused), [lines[i] for i in fused]
    assert sum(op.startswith("v_div_fixup_f64") for op in lines) == DIVISIONS and sum(op.startswith("v_rcp_f64") for op in lines) == DIVISIONS
    assert sum(op.startswith("v_div_fmas_f64") for op in lines) == DIVISIONS and sum(op.startswith("v_div_scale_f64") for op in lines) == 2 * DIVISIONS
    assert len(fused) == FMA_PER_DIVISION * DIVISIONS, [lines[i] for i in fused]
    first_rcp = min(i for i, op in enumerate(lines) if op.startswith("v_rcp_f64"))
    last_fix = max(i for i, op in enumerate(lines) if op.startswith("v_div_fixup_f64"))
    assert all(first_rcp < i < last_fix for i in fused)
    assert sum(op.startswith("v_rndne_f64") for op in lines) == 1 and sum(op.startswith("v_ldexp_f64") for op in lines) == 1
    # contrast_min * (hi + lo) and (mb + my) * C, beside the one product inside each division
    assert sum(op.startswith("v_mul_f64") for op in lines) == 2 + DIVISIONS
    assert not any(re.match(r"v_\w+_f32", op) for op in lines)
