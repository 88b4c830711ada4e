"""Guards on the channel tap's generated gfx950 code (navtex_amd/tap/nvx_tap.hip, cross-compiled with the shipped flags): exactly
its kernel family (two kinds x two forms), no scratch, no spills, no fp64, no float, no atomics, no static LDS, and the loop
property of the output-stationary form DESIGN 3.13 describes: per 8-byte LDS read of samples four dot products (a group of 8
taps is four reads and sixteen dot products), the taps through the scalar cache in the wave-uniform form and through 16-byte
vector loads in the per-lane form; and the registers DESIGN 3.13 states."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not Path(HIPCC).exists(), reason="hipcc not available")

IQ, REAL = 0, 1
KERNELS = [f"nvx_tap_kernel<{kind}, {form}>" for kind in (IQ, REAL) for form in ("false", "true")]      # form true: taps wave-uniform
# 8 waves per SIMD at up to 64 registers; the uniform form keeps its taps in SGPRs
VGPR_MAX = {"false": 64, "true": 40}
MIXER_DOTS = 4                            # the staging loop mixes two samples per turn, two dot products each


@pytest.fixture(scope="module")
def build():
    import importlib.util
    spec = importlib.util.spec_from_file_location("nvx_build_for_tap_isa", ROOT / "navtex_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def isa(build, tmp_path_factory):
    """(the kernels' bodies, every other function's body, the metadata)."""
    tmp = tmp_path_factory.mktemp("tap_isa")
    kernels, functions, meta = {}, {}, ""
    for name in build.TAP_HIP_SOURCES:
        out = tmp / (name + ".s")
        subprocess.run([HIPCC, f"--offload-arch={build.ARCH}", "-std=c++17", *build.COMMON, f"-I{build.TAP}", f"-I{build.RESAMPLE}", f"-I{build.DDC}",
                        "--cuda-device-only", "-S", str(build.TAP / name), "-o", str(out)], check=True, capture_output=True)
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
    return int(name[len("nvx_tap_kernel<")])


def _form(name):
    return name[name.index(", ") + 2:-1]


def test_the_library_holds_exactly_its_kernel_family(isa):
    kernels, functions, meta = isa
    assert sorted(_meta(meta)) == sorted(KERNELS) and sorted(kernels) == sorted(KERNELS) and not functions


def test_no_scratch_no_spills_no_fp64_no_float_no_atomics_no_static_lds(isa):
    kernels, _, meta = isa
    for name, body in kernels.items():
        assert not re.search(r"v_\w+_f64", body), f"{name}: fp64"
        assert not re.findall(r"\bv_\w+_f(16|32)\w*", body) and "v_cvt" not in body, f"{name}: float"
        assert "scratch_" not in body and "v_writelane" not in body, name
        assert "atomic" not in body and not re.search(r"\bds_\w*(add|sub|inc|dec|min|max|and|or|xor|cmpst|wrxchg)\w*", body), f"{name}: an atomic"
    for name, m in _meta(meta).items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= VGPR_MAX[_form(name)], (name, m)
        assert m["group_segment_fixed_size"] == 0, (name, m)        # all of the LDS is the launch's: the two planes


def test_four_dot_products_per_sample_read_and_the_taps_by_the_form(isa):
    """Besides the mixer's (and the audio kind's one for the pitch) every dot product belongs to the filter: four per ds_read_b64,
    and nothing else reads the LDS.  The wave-uniform form loads no taps through the vector cache; the per-lane form loads two
    16-byte words per four sample reads."""
    kernels, _, _ = isa
    for name in KERNELS:
        body = kernels[name]
        dots = len(re.findall(r"v_dot2c?_i32_i16", body)) - MIXER_DOTS - (1 if _kind(name) == REAL else 0)
        reads = len(re.findall(r"\bds_read_b64\b", body))
        assert reads >= 4 and dots == 4 * reads, (name, dots, reads)
        assert not re.findall(r"\bds_read(?!_b64\b)\w*", body), name
        wide = len(re.findall(r"\bglobal_load_dwordx4\b", body))
        if _form(name) == "true":
            assert wide == 0 and len(re.findall(r"\bs_load_dwordx(8|16)\b", body)) >= 2, name
        else:
            assert 2 * wide == reads, (name, wide, reads)
        assert len(re.findall(r"s_barrier", body)) == 1, name
        assert "flat_load" not in body and "flat_store" not in body and "buffer_" not in body, name
