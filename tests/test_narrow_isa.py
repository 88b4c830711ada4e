"""Guards on the narrowband interpolator's generated gfx950 code (navtex_amd/narrow/nvx_narrow.hip, cross-compiled with the
shipped flags): exactly its kernel family (four formats x two kinds x three lengths of a tap row), no scratch, no spills, no
fp64, no FMA, no atomics, float32 only in the F32 instances, and the loop property of the window-stationary form: the window is in registers, so the filter reads the LDS once
-- 16 bytes of taps -- per eight dot products (IQ) or four (REAL); and the registers and LDS DESIGN 3.12 states."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")

IQ, REAL = 0, 1
ROWS = (2, 3, 4)                          # 16-byte words of a tap row: T up to 16, 24 and 32
KERNELS = [f"nvx_nb<{fmt}, {kind}, {tq}>" for fmt in range(4) for kind in (IQ, REAL) for tq in ROWS]      # S16, U8, S8, F32 x IQ, REAL x rows
# the window is 4 tq registers per component; 512 / 72 = 7 waves per SIMD for the IQ kind at T = 30, 8 elsewhere
VGPR_MAX = {(IQ, 2): 48, (IQ, 3): 60, (IQ, 4): 72, (REAL, 2): 40, (REAL, 3): 48, (REAL, 4): 56}


@pytest.fixture(scope="module")
def build():
    import importlib.util
    spec = importlib.util.spec_from_file_location("nvx_build_for_narrow_isa", ROOT / "navtex_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def isa(build, tmp_path_factory):
    """(the kernels' bodies, every other function's body, the metadata)."""
    tmp = tmp_path_factory.mktemp("narrow_isa")
    kernels, functions, meta = {}, {}, ""
    for name in build.NARROW_HIP_SOURCES:
        out = tmp / (name + ".s")
        subprocess.run([HIPCC, f"--offload-arch={build.ARCH}", "-std=c++17", *build.COMMON, f"-I{build.NARROW}", f"-I{build.RESAMPLE}", "--cuda-device-only",
                        "-S", str(build.NARROW / name), "-o", str(out)], check=True, capture_output=True)
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


def _kind(name):
    return int(name[-5])


def _rows(name):
    return int(name[-2])


def test_the_library_holds_exactly_its_kernel_family(isa):
    kernels, functions, meta = isa
    assert sorted(_meta(meta)) == sorted(KERNELS) and sorted(kernels) == sorted(KERNELS) and not functions


def test_no_scratch_no_spills_no_fp64_no_fma_no_atomics_and_float32_only_for_f32(isa):
    kernels, _, meta = isa
    for name, body in kernels.items():
        assert not re.search(r"v_\w+_f64", body), f"{name}: fp64"
        assert "scratch_" not in body and "v_writelane" not in body, name
        assert not re.search(r"v_(pk_)?(fma|mac|mad|fmac)\w*_f(16|32)", body), f"{name}: a fused multiply-add"
        assert "atomic" not in body and not re.search(r"\bds_\w*(add|sub|inc|dec|min|max|and|or|xor|cmpst|wrxchg)\w*", body), f"{name}: an atomic"
        floats = re.findall(r"\bv_\w+_f32\w*", body)
        if not name.startswith("nvx_nb<3,"):
            assert not floats, f"{name}: float32 outside F32's conversion: {sorted(set(floats))}"
        else:
            assert floats and not re.search(r"v_(div|rcp|sqrt|exp|log)\w*_f32", body), sorted(set(floats))
    for name, m in _meta(meta).items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= VGPR_MAX[(_kind(name), _rows(name))], (name, m)
        assert m["group_segment_fixed_size"] == 0, (name, m)        # all of the LDS is the launch's: the table, the stage, the image


def test_the_filter_reads_sixteen_bytes_of_taps_per_eight_dot_products(isa):
    """Per 16-byte word of a tap row the IQ kind has 4 dot products for I and 4 for Q, the REAL kind 4.  Besides the row's reads a
    kernel reads 16 bytes once more: the output image, in the store.  The window is read once per tile, word by word, and
    split by one v_perm_b32 per register; nothing reads 8 bytes or less than a word."""
    kernels, _, _ = isa
    for name in KERNELS:
        body = kernels[name]
        tq, per_word = _rows(name), 8 if _kind(name) == IQ else 4
        assert len(re.findall(r"v_dot2c?_i32_i16", body)) == tq * per_word, name
        assert len(re.findall(r"\bds_read_b128\b", body)) == tq + 1, name
        assert not re.findall(r"\bds_read2?_b64\b", body) and not re.findall(r"\bds_read_[ui](8|16)\b", body), name
        # the window: 8 words per row word
        assert 2 * len(re.findall(r"\bds_read2_b32\b", body)) + len(re.findall(r"\bds_read_b32\b", body)) >= 8 * tq, name
        assert len(re.findall(r"v_perm_b32", body)) >= tq * per_word, name
        assert len(re.findall(r"v_med3_i32", body)) == (2 if _kind(name) == IQ else 1), name      # the clamps
        assert len(re.findall(r"s_barrier", body)) == 2, name
        assert len(re.findall(r"global_store_dwordx4 .* nt", body)) == 1, name
        assert "flat_load" not in body and "flat_store" not in body and "buffer_" not in body, name
