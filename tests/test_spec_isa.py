"""Guards on the spectrum monitor's generated gfx950 code (navtex_amd/spec/nvx_spec.hip, cross-compiled with the shipped
flags): exactly the kernels the header names -- nvx_spec_line for four formats and five sizes, nvx_spec_fold, nvx_spec_carry for
four formats --, no scratch and no spills, at most 96 vector registers in the line kernels (1024 threads leave 128), 24 N bytes
of LDS, 16-byte non-temporal loads of the input and 16-byte non-temporal stores of the level words, 16-byte LDS reads of the
twiddles and 8-byte ones of the data, and fp64 products and sums with no fused multiply-add among them.  Positive properties
only: what the kernels are meant to contain."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")

SIZES = (8, 9, 10, 11, 12)
LINE_KERNELS = [f"nvx_spec_line<{fmt}, {l}>" for fmt in range(4) for l in SIZES]        # CS16, CU8, CS8, CF32
CARRY_KERNELS = [f"nvx_spec_carry<{fmt}>" for fmt in range(4)]
FOLD_KERNEL = "nvx_spec_fold"
# the ceilings reached: the line kernels 77 .. 90 (the most at N = 4096), the fold and carry kernels 8 .. 15
VGPR_MAX = {"line": 96, "fold": 16, "carry": 16}


@pytest.fixture(scope="module")
def build():
    import importlib.util
    spec = importlib.util.spec_from_file_location("nvx_build_for_spec_isa", ROOT / "navtex_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _short(mangled):
    name = subprocess.run(["c++filt", mangled], capture_output=True, text=True, check=True).stdout.strip()
    return re.sub(r"^void |\(.*$", "", name)


@pytest.fixture(scope="module")
def isa(build, tmp_path_factory):
    """(the kernels' bodies, the metadata of every kernel)."""
    tmp = tmp_path_factory.mktemp("spec_isa")
    kernels, meta = {}, {}
    for name in build.SPEC_HIP_SOURCES:
        out = tmp / (name + ".s")
        subprocess.run([HIPCC, f"--offload-arch={build.ARCH}", "-std=c++17", *build.COMMON, f"-I{build.SPEC}", f"-I{build.RESAMPLE}",
                        "--cuda-device-only", "-S", str(build.SPEC / name), "-o", str(out)], check=True, capture_output=True)
        text = out.read_text()
        for m in re.finditer(r"^(_Z\w+):.*?^\.Lfunc_end\d+:", text, flags=re.S | re.M):      # the whole body: a kernel may end in several places
            if "s_endpgm" in m.group(0):
                kernels[_short(m.group(1))] = m.group(0)
        for block in text[text.index("amdhsa.kernels"):].split("  - .agpr_count")[1:]:
            kernel = _short(re.search(r"\.name:\s+(\S+)", block).group(1))
            meta[kernel] = {f: int(re.search(rf"\.{f}:\s*(\d+)", block).group(1))
                            for f in ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                                      "max_flat_workgroup_size")}
    return kernels, meta


def test_the_library_holds_exactly_the_kernels_the_header_names(isa):
    kernels, meta = isa
    want = sorted(LINE_KERNELS + CARRY_KERNELS + [FOLD_KERNEL])
    assert sorted(meta) == want and sorted(kernels) == want
    header = (ROOT / "include" / "navtex_amd_spec.h").read_text()
    assert all(k in header for k in ("nvx_spec_line<format, n_log2>", "nvx_spec_fold", "nvx_spec_carry<format>"))


def test_no_scratch_no_spills_the_register_ceiling_and_the_lds(isa):
    _, meta = isa
    for name, m in sorted(meta.items()):
        print(name, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= VGPR_MAX[name.split("_")[2].split("<")[0]], (name, m)
    for fmt in range(4):
        for l in SIZES:
            m = meta[f"nvx_spec_line<{fmt}, {l}>"]
            # re[N], im[N] and (cos, -sin)[N / 2] in fp64: 96 KB at N = 4096, one workgroup to a CU's 160 KB; N / 4 threads
            assert m["group_segment_fixed_size"] == 24 << l and m["max_flat_workgroup_size"] == (1 << l) // 4, (fmt, l, m)
    for name in CARRY_KERNELS + [FOLD_KERNEL]:
        assert meta[name]["group_segment_fixed_size"] == 0, name


def test_the_line_kernels_stream_sixteen_bytes_and_multiply_without_fusing(isa):
    kernels, _ = isa
    for name in LINE_KERNELS:
        body = kernels[name]
        fmt = int(name[len("nvx_spec_line<")])
        assert len(re.findall(r"global_load_dwordx4 .* nt", body)) >= (2 if fmt == 3 else 1), name      # the call's input (float32: two to a group)
        assert len(re.findall(r"global_store_dwordx4 .* nt", body)) >= 1, name                          # the level words
        assert "global_store_dwordx2" in body, name                                                      # P_line and C_line to the scratch row
        # the header's arithmetic: products and sums of their own.  A butterfly is four products and six sums; the powers and
        # the lag products of a thread's four bins are twenty-four products
        assert len(re.findall(r"v_mul_f64", body)) >= 24 + 4 * 4 and len(re.findall(r"v_add_f64", body)) >= 6 * 4, name
        assert "ds_read_b128" in body or "ds_read2_b64" in body, name                                    # a twiddle: (cos, -sin) at once
        # the data: re[] and im[] apart, 8 bytes each (a position's two in one ds_*2st64_b64 where the compiler pairs them)
        assert re.search(r"ds_read(2st64|2)?_b64", body) and re.search(r"ds_write(2st64|2)?_b64", body), name
        assert "v_cvt_f64_i32" in body and "v_bfrev_b32" in body, name                                   # int16 -> fp64, the bit reversal
        if "8>" not in name:                                                                             # N = 256 is one wave: no barrier needed
            assert "s_barrier" in body, name


def test_the_fold_adds_in_order_and_the_carry_converts(isa):
    kernels, _ = isa
    body = kernels[FOLD_KERNEL]
    assert "v_add_f64" in body and "global_load_dwordx2" in body and "global_store_dwordx2" in body
    for name in CARRY_KERNELS:
        assert "global_store_dword" in kernels[name], name
    assert "v_cvt" in kernels["nvx_spec_carry<3>"] and "v_med3_f32" in kernels["nvx_spec_carry<3>"]      # float32: times 32768, rounded, clamped
