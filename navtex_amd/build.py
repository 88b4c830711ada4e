"""Build helper: compiles libnavtex_amd.so (HIP kernels for gfx950 + host C/C++) and its
companions libnavtex_amd_scan.so (the band scan, navtex_amd/scan/), libnavtex_amd_resample.so (the resampler,
navtex_amd/resample/), libnavtex_amd_ddc.so (the down-converter bank, navtex_amd/ddc/), libnavtex_amd_blank.so (the
impulse noise blanker, navtex_amd/blank/), libnavtex_amd_iqc.so (the IQ corrector, navtex_amd/iqc/), libnavtex_amd_real.so
(the real-input converter, navtex_amd/real/), libnavtex_amd_narrow.so (the narrowband interpolator, navtex_amd/narrow/),
libnavtex_amd_tap.so (the channel tap, navtex_amd/tap/), libnavtex_amd_anc.so (the antenna noise canceller,
navtex_amd/anc/), libnavtex_amd_notch.so (the tone notch, navtex_amd/notch/), libnavtex_amd_zoom.so (the zoom bank,
navtex_amd/zoom/), libnavtex_amd_align.so (the row aligner, navtex_amd/align/), libnavtex_amd_wanc.so (the multi-tap noise
canceller, navtex_amd/wanc/), libnavtex_amd_div.so (the diversity combiner, navtex_amd/div/) and libnavtex_amd_spec.so (the
spectrum monitor, navtex_amd/spec/) in-tree with hipcc, and -- for tests only -- the oracle library and the compiled
reference seams via oracle/Makefile.

    python navtex_amd/build.py            # product library
    python navtex_amd/build.py --oracle   # + oracle (and reference seams when /root/reference exists)

Run it as a script (or load it by path): importing the navtex_amd package itself
requires the library to exist already.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from pathlib import Path

PKG = Path(__file__).resolve().parent
ROOT = PKG.parent
CSRC = PKG / "csrc"
OBJ = PKG / "_obj"
LIB = PKG / "libnavtex_amd.so"
ARCH = "gfx950"

C_SOURCES = ["nvx_sitor.c", "nvx_wav.c", "nvx_synth_host.c", "nvx_store.c"]
HIP_SOURCES = ["nvx_cascade.hip", "nvx_fir3.hip", "nvx_demod.hip", "nvx_channelise.hip", "nvx_wideband_fused.hip", "nvx_synth.hip"]
# the companion library (include/navtex_amd_scan.h): its own directory, objects and link; the same flags
SCAN = PKG / "scan"
SCAN_LIB = PKG / "libnavtex_amd_scan.so"
SCAN_C_SOURCES = ["nvx_scan_find.c"]
SCAN_HIP_SOURCES = ["nvx_scan.hip"]
SCAN_CXX_SOURCES = ["nvx_scan_host.cpp"]
# the second companion (include/navtex_amd_resample.h), built the same way
RESAMPLE = PKG / "resample"
RESAMPLE_LIB = PKG / "libnavtex_amd_resample.so"
RESAMPLE_C_SOURCES = ["nvx_resample_design.c"]
RESAMPLE_HIP_SOURCES = ["nvx_resample.hip"]
RESAMPLE_CXX_SOURCES = ["nvx_resample_host.cpp"]
# the third companion (include/navtex_amd_ddc.h): its own sources, plus the resampler's tap design compiled in (the object
# the resampler links too: -fvisibility=hidden keeps its symbols out of both libraries' exports)
DDC = PKG / "ddc"
DDC_LIB = PKG / "libnavtex_amd_ddc.so"
DDC_HIP_SOURCES = ["nvx_ddc.hip"]
DDC_CXX_SOURCES = ["nvx_ddc_host.cpp"]
DDC_SHARED_C_SOURCES = ["nvx_resample_design.c"]           # of RESAMPLE
# the fourth companion (include/navtex_amd_blank.h): its own sources; its kernel includes the resampler's nvx_rs_device.h for
# the formats' loads and conversions, through nvx_stream_device.h beside it (the same-rate companions' streaming helpers),
# and links nothing of either
BLANK = PKG / "blank"
BLANK_LIB = PKG / "libnavtex_amd_blank.so"
BLANK_HIP_SOURCES = ["nvx_blank.hip"]
BLANK_CXX_SOURCES = ["nvx_blank_host.cpp"]
# the fifth companion (include/navtex_amd_iqc.h), built as the fourth is: nvx_stream_device.h again, and nothing linked
IQC = PKG / "iqc"
IQC_LIB = PKG / "libnavtex_amd_iqc.so"
IQC_HIP_SOURCES = ["nvx_iqc.hip"]
IQC_CXX_SOURCES = ["nvx_iqc_host.cpp"]
# the sixth companion (include/navtex_amd_real.h), built as the fourth and fifth are, on the same two headers
REAL = PKG / "real"
REAL_LIB = PKG / "libnavtex_amd_real.so"
REAL_HIP_SOURCES = ["nvx_real.hip"]
REAL_CXX_SOURCES = ["nvx_real_host.cpp"]
# the seventh companion (include/navtex_amd_narrow.h): its own design, kernel and host side; nvx_rs_device.h once more
NARROW = PKG / "narrow"
NARROW_LIB = PKG / "libnavtex_amd_narrow.so"
NARROW_C_SOURCES = ["nvx_narrow_design.c"]
NARROW_HIP_SOURCES = ["nvx_narrow.hip"]
NARROW_CXX_SOURCES = ["nvx_narrow_host.cpp"]
# the eighth companion (include/navtex_amd_tap.h), built as the seventh is; it also reads the bank's table header nvx_ddc_table.h
TAP = PKG / "tap"
TAP_LIB = PKG / "libnavtex_amd_tap.so"
TAP_C_SOURCES = ["nvx_tap_design.c"]
TAP_HIP_SOURCES = ["nvx_tap.hip"]
TAP_CXX_SOURCES = ["nvx_tap_host.cpp"]
# the antenna noise canceller (include/navtex_amd_anc.h), built as the fifth is: nvx_stream_device.h, and nothing linked
ANC = PKG / "anc"
ANC_LIB = PKG / "libnavtex_amd_anc.so"
ANC_HIP_SOURCES = ["nvx_anc.hip"]
ANC_CXX_SOURCES = ["nvx_anc_host.cpp"]
# the tone notch (include/navtex_amd_notch.h), built as the canceller is, nvx_stream_device.h included; it also reads the bank's
# table header nvx_ddc_table.h
NOTCH = PKG / "notch"
NOTCH_LIB = PKG / "libnavtex_amd_notch.so"
NOTCH_HIP_SOURCES = ["nvx_notch.hip"]
NOTCH_CXX_SOURCES = ["nvx_notch_host.cpp"]
# the zoom bank (include/navtex_amd_zoom.h), built as the notch is; it reads the bank's table header nvx_ddc_table.h and the
# real-input converter's taps nvx_real_taps.h
ZOOM = PKG / "zoom"
ZOOM_LIB = PKG / "libnavtex_amd_zoom.so"
ZOOM_HIP_SOURCES = ["nvx_zoom.hip"]
ZOOM_CXX_SOURCES = ["nvx_zoom_host.cpp"]
# the row aligner (include/navtex_amd_align.h), built as the canceller is, nvx_stream_device.h included; its host-only parts
# (the estimate, and the taps from csrc/nvx_polyphase_design.h) are plain C
ALIGN = PKG / "align"
ALIGN_LIB = PKG / "libnavtex_amd_align.so"
ALIGN_C_SOURCES = ["nvx_align_find.c"]
ALIGN_HIP_SOURCES = ["nvx_align.hip"]
ALIGN_CXX_SOURCES = ["nvx_align_host.cpp"]
# the multi-tap noise canceller (include/navtex_amd_wanc.h), built as the canceller is: nvx_stream_device.h, and nothing linked
WANC = PKG / "wanc"
WANC_LIB = PKG / "libnavtex_amd_wanc.so"
WANC_HIP_SOURCES = ["nvx_wanc.hip"]
WANC_CXX_SOURCES = ["nvx_wanc_host.cpp"]
# the diversity combiner (include/navtex_amd_div.h), built as the notch is: nvx_stream_device.h and the bank's table header
# nvx_ddc_table.h, and nothing linked
DIV = PKG / "div"
DIV_LIB = PKG / "libnavtex_amd_div.so"
DIV_HIP_SOURCES = ["nvx_div.hip"]
DIV_CXX_SOURCES = ["nvx_div_host.cpp"]
# the spectrum monitor (include/navtex_amd_spec.h), built as the notch is: nvx_stream_device.h for the formats' loads, its own
# generated table nvx_spec_table.h, a host-only finder in plain C, and nothing linked
SPEC = PKG / "spec"
SPEC_LIB = PKG / "libnavtex_amd_spec.so"
SPEC_C_SOURCES = ["nvx_spec_find.c"]
SPEC_HIP_SOURCES = ["nvx_spec.hip"]
SPEC_CXX_SOURCES = ["nvx_spec_host.cpp"]
CXX_SOURCES = ["nvx_api.cpp", "nvx_push.cpp", "nvx_shim.cpp", "nvx_capture.cpp", "nvx_wideband.cpp", "nvx_synth_dev.cpp", "nvx_fsm_host.cpp", "nvx_group.cpp",
               "nvx_tune.cpp", "nvx_afc.cpp"]
# automatic frequency control (include/navtex_amd_afc.h): its update kernel is part of libnavtex_amd.so, in a directory of
# its own beside csrc (the law it runs, csrc/nvx_afc_law.h, is shared with the host)
AFC = PKG / "afc"
AFC_HIP_SOURCES = ["nvx_afc.hip"]

# -ffp-contract=off is part of the numerical contract: FIR products and sums are
# rounded separately, exactly as the reference's x86-64 build does.
COMMON = ["-O3", "-fPIC", "-ffp-contract=off", "-fvisibility=hidden",
          f"-I{ROOT / 'include'}", f"-I{CSRC}"] + os.environ.get("NVX_EXTRA_CFLAGS", "").split()


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError("hipcc not found: the HIP toolchain is required (there is no CPU build of this library)")


def _run(cmd):
    print(" ".join(str(c) for c in cmd), file=sys.stderr, flush=True)
    subprocess.run([str(c) for c in cmd], check=True, stdout=sys.stderr)


def _stale(out: Path, deps) -> bool:
    if not out.exists():
        return True
    t = out.stat().st_mtime
    return any(Path(d).stat().st_mtime > t for d in deps)


def _companion_jobs(hipcc: str, force: bool, src_dir: Path, c_sources, hip_sources, cxx_sources, also=()):
    """(objects, compile jobs) of a companion library: csrc headers are on its include path (FIR1's taps, and
    nvx_companion.h: what the companions' host sides share), and the directories in `also` (another companion's internal
    headers: the bank compiles the resampler's nvx_rs_host.h and nvx_rs_device.h)."""
    headers = list(src_dir.glob("*.h")) + list(CSRC.glob("*.h")) + list((ROOT / "include").glob("*.h")) + [Path(__file__)]
    flags = [*COMMON, f"-I{src_dir}"]
    for d in also:
        headers += list(d.glob("*.h"))
        flags.append(f"-I{d}")
    objs, jobs = [], []
    for srcs, cmd in ((c_sources, [hipcc, "-x", "c", "-std=gnu11", "-Wall", "-Wextra"]),
                      (hip_sources, [hipcc, f"--offload-arch={ARCH}", "-std=c++17"]),
                      (cxx_sources, [hipcc, "-x", "hip", "--offload-arch=" + ARCH, "-std=c++17", "-Wall"])):
        for src in srcs:
            o = OBJ / (src + ".o")
            if force or _stale(o, [src_dir / src] + headers):
                jobs.append([*cmd, *flags, "-c", src_dir / src, "-o", o])
            objs.append(o)
    return objs, jobs


def _scan_jobs(hipcc: str, force: bool):
    return _companion_jobs(hipcc, force, SCAN, SCAN_C_SOURCES, SCAN_HIP_SOURCES, SCAN_CXX_SOURCES)


def _resample_jobs(hipcc: str, force: bool):
    return _companion_jobs(hipcc, force, RESAMPLE, RESAMPLE_C_SOURCES, RESAMPLE_HIP_SOURCES, RESAMPLE_CXX_SOURCES)


def _ddc_jobs(hipcc: str, force: bool):
    objs, jobs = _companion_jobs(hipcc, force, DDC, [], DDC_HIP_SOURCES, DDC_CXX_SOURCES, also=(RESAMPLE,))
    return objs + [OBJ / (src + ".o") for src in DDC_SHARED_C_SOURCES], jobs


def _blank_jobs(hipcc: str, force: bool):
    return _companion_jobs(hipcc, force, BLANK, [], BLANK_HIP_SOURCES, BLANK_CXX_SOURCES, also=(RESAMPLE,))


def _iqc_jobs(hipcc: str, force: bool):
    return _companion_jobs(hipcc, force, IQC, [], IQC_HIP_SOURCES, IQC_CXX_SOURCES, also=(RESAMPLE,))


def _real_jobs(hipcc: str, force: bool):
    return _companion_jobs(hipcc, force, REAL, [], REAL_HIP_SOURCES, REAL_CXX_SOURCES, also=(RESAMPLE,))


def _narrow_jobs(hipcc: str, force: bool):
    return _companion_jobs(hipcc, force, NARROW, NARROW_C_SOURCES, NARROW_HIP_SOURCES, NARROW_CXX_SOURCES, also=(RESAMPLE,))


def _tap_jobs(hipcc: str, force: bool):
    return _companion_jobs(hipcc, force, TAP, TAP_C_SOURCES, TAP_HIP_SOURCES, TAP_CXX_SOURCES, also=(RESAMPLE, DDC))


def _anc_jobs(hipcc: str, force: bool):
    return _companion_jobs(hipcc, force, ANC, [], ANC_HIP_SOURCES, ANC_CXX_SOURCES, also=(RESAMPLE,))


def _notch_jobs(hipcc: str, force: bool):
    return _companion_jobs(hipcc, force, NOTCH, [], NOTCH_HIP_SOURCES, NOTCH_CXX_SOURCES, also=(RESAMPLE, DDC))


def _zoom_jobs(hipcc: str, force: bool):
    return _companion_jobs(hipcc, force, ZOOM, [], ZOOM_HIP_SOURCES, ZOOM_CXX_SOURCES, also=(RESAMPLE, DDC, REAL))


def _align_jobs(hipcc: str, force: bool):
    return _companion_jobs(hipcc, force, ALIGN, ALIGN_C_SOURCES, ALIGN_HIP_SOURCES, ALIGN_CXX_SOURCES, also=(RESAMPLE,))


def _wanc_jobs(hipcc: str, force: bool):
    return _companion_jobs(hipcc, force, WANC, [], WANC_HIP_SOURCES, WANC_CXX_SOURCES, also=(RESAMPLE,))


def _div_jobs(hipcc: str, force: bool):
    return _companion_jobs(hipcc, force, DIV, [], DIV_HIP_SOURCES, DIV_CXX_SOURCES, also=(RESAMPLE, DDC))


def _spec_jobs(hipcc: str, force: bool):
    return _companion_jobs(hipcc, force, SPEC, SPEC_C_SOURCES, SPEC_HIP_SOURCES, SPEC_CXX_SOURCES, also=(RESAMPLE,))


def _link(hipcc: str, lib: Path, objs, libs=()) -> None:
    # link beside the target and rename: another process (a second rank, a test runner) never maps a half-written file
    tmp = lib.with_name(lib.name + f".tmp{os.getpid()}")
    _run([hipcc, "-shared", "-fPIC", f"--offload-arch={ARCH}", *objs, "-o", tmp, *libs])
    os.replace(tmp, lib)


def build_lib(force: bool = False) -> Path:
    from concurrent.futures import ThreadPoolExecutor
    hipcc = _hipcc()
    OBJ.mkdir(exist_ok=True)
    headers = list(CSRC.glob("*.h")) + list((ROOT / "include").glob("*.h")) + [Path(__file__)]
    objs, jobs = [], []
    scan_objs, scan_jobs = _scan_jobs(hipcc, force)
    jobs += scan_jobs
    resample_objs, resample_jobs = _resample_jobs(hipcc, force)
    jobs += resample_jobs
    ddc_objs, ddc_jobs = _ddc_jobs(hipcc, force)
    jobs += ddc_jobs
    blank_objs, blank_jobs = _blank_jobs(hipcc, force)
    jobs += blank_jobs
    iqc_objs, iqc_jobs = _iqc_jobs(hipcc, force)
    jobs += iqc_jobs
    real_objs, real_jobs = _real_jobs(hipcc, force)
    jobs += real_jobs
    narrow_objs, narrow_jobs = _narrow_jobs(hipcc, force)
    jobs += narrow_jobs
    tap_objs, tap_jobs = _tap_jobs(hipcc, force)
    jobs += tap_jobs
    anc_objs, anc_jobs = _anc_jobs(hipcc, force)
    jobs += anc_jobs
    notch_objs, notch_jobs = _notch_jobs(hipcc, force)
    jobs += notch_jobs
    zoom_objs, zoom_jobs = _zoom_jobs(hipcc, force)
    jobs += zoom_jobs
    align_objs, align_jobs = _align_jobs(hipcc, force)
    jobs += align_jobs
    wanc_objs, wanc_jobs = _wanc_jobs(hipcc, force)
    jobs += wanc_jobs
    div_objs, div_jobs = _div_jobs(hipcc, force)
    jobs += div_jobs
    spec_objs, spec_jobs = _spec_jobs(hipcc, force)
    jobs += spec_jobs
    for src in C_SOURCES:
        o = OBJ / (src + ".o")
        if force or _stale(o, [CSRC / src] + headers):
            jobs.append([hipcc, "-x", "c", "-std=gnu11", "-Wall", "-Wextra", *COMMON, "-c", CSRC / src, "-o", o])
        objs.append(o)
    for src in HIP_SOURCES:
        o = OBJ / (src + ".o")
        if force or _stale(o, [CSRC / src] + headers):
            jobs.append([hipcc, f"--offload-arch={ARCH}", "-std=c++17", *COMMON, "-c", CSRC / src, "-o", o])
        objs.append(o)
    for src in AFC_HIP_SOURCES:
        o = OBJ / (src + ".o")
        if force or _stale(o, [AFC / src] + headers):
            jobs.append([hipcc, f"--offload-arch={ARCH}", "-std=c++17", *COMMON, "-c", AFC / src, "-o", o])
        objs.append(o)
    for src in CXX_SOURCES:
        o = OBJ / (src + ".o")
        if force or _stale(o, [CSRC / src] + headers):
            jobs.append([hipcc, "-x", "hip", "--offload-arch=" + ARCH, "-std=c++17", "-Wall", "-Wno-unused-value", "-Wno-unused-result", *COMMON, "-c", CSRC / src, "-o", o])
        objs.append(o)
    # the translation units are independent: compile them side by side (the cascade's twelve kernels dominate)
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        list(pool.map(_run, jobs))
    if force or _stale(LIB, objs):
        _link(hipcc, LIB, objs, ["-lpthread", "-ldl"])
    if force or _stale(SCAN_LIB, scan_objs):
        _link(hipcc, SCAN_LIB, scan_objs, ["-lpthread", "-lm"])
    if force or _stale(RESAMPLE_LIB, resample_objs):
        _link(hipcc, RESAMPLE_LIB, resample_objs, ["-lpthread", "-lm"])
    if force or _stale(DDC_LIB, ddc_objs):
        _link(hipcc, DDC_LIB, ddc_objs, ["-lpthread", "-lm"])
    if force or _stale(BLANK_LIB, blank_objs):
        _link(hipcc, BLANK_LIB, blank_objs, ["-lpthread"])
    if force or _stale(IQC_LIB, iqc_objs):
        _link(hipcc, IQC_LIB, iqc_objs, ["-lpthread"])
    if force or _stale(REAL_LIB, real_objs):
        _link(hipcc, REAL_LIB, real_objs, ["-lpthread"])
    if force or _stale(NARROW_LIB, narrow_objs):
        _link(hipcc, NARROW_LIB, narrow_objs, ["-lpthread", "-lm"])
    if force or _stale(TAP_LIB, tap_objs):
        _link(hipcc, TAP_LIB, tap_objs, ["-lpthread", "-lm"])
    if force or _stale(ANC_LIB, anc_objs):
        _link(hipcc, ANC_LIB, anc_objs, ["-lpthread"])
    if force or _stale(NOTCH_LIB, notch_objs):
        _link(hipcc, NOTCH_LIB, notch_objs, ["-lpthread", "-lm"])
    if force or _stale(ZOOM_LIB, zoom_objs):
        _link(hipcc, ZOOM_LIB, zoom_objs, ["-lpthread", "-lm"])
    if force or _stale(ALIGN_LIB, align_objs):
        _link(hipcc, ALIGN_LIB, align_objs, ["-lpthread", "-lm"])
    if force or _stale(WANC_LIB, wanc_objs):
        _link(hipcc, WANC_LIB, wanc_objs, ["-lpthread"])
    if force or _stale(DIV_LIB, div_objs):
        _link(hipcc, DIV_LIB, div_objs, ["-lpthread", "-lm"])
    if force or _stale(SPEC_LIB, spec_objs):
        _link(hipcc, SPEC_LIB, spec_objs, ["-lpthread", "-lm"])
    return LIB


def build_variant(name: str, flags, sources=("nvx_cascade.hip", "nvx_wideband_fused.hip")) -> Path:
    """TEST INFRASTRUCTURE: another build of the same library -- the named kernel sources recompiled with extra flags,
    everything else the product's own objects -- as tests/_variants/libnavtex_amd_<name>.so; load it with
    NAVTEX_AMD_LIB.  `inject` (-DNVX_INJECT_STALE=n) is the fault-injection build of the state hand-over's seal."""
    hipcc = _hipcc()
    build_lib()
    out_dir = ROOT / "tests" / "_variants"
    out_dir.mkdir(exist_ok=True)
    headers = list(CSRC.glob("*.h")) + list((ROOT / "include").glob("*.h")) + [Path(__file__)]
    objs, jobs = [], []
    for src in C_SOURCES + HIP_SOURCES + CXX_SOURCES:
        if src in sources:
            o = out_dir / f"{src}.{name}.o"
            if _stale(o, [CSRC / src] + headers):
                lang = ["-x", "c", "-std=gnu11"] if src in C_SOURCES else (["-x", "hip"] if src in CXX_SOURCES else []) + [f"--offload-arch={ARCH}", "-std=c++17"]
                jobs.append([hipcc, *lang, *COMMON, *flags, "-c", CSRC / src, "-o", o])
            objs.append(o)
        else:
            objs.append(OBJ / (src + ".o"))
    objs += [OBJ / (src + ".o") for src in AFC_HIP_SOURCES]
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=2) as pool:
        list(pool.map(_run, jobs))
    lib = out_dir / f"libnavtex_amd_{name}.so"
    if _stale(lib, objs):
        tmp = lib.with_name(lib.name + f".tmp{os.getpid()}")
        _run([hipcc, "-shared", "-fPIC", f"--offload-arch={ARCH}", *objs, "-o", tmp, "-lpthread", "-ldl"])
        os.replace(tmp, lib)
    return lib


INJECT_FLAGS = ["-DNVX_INJECT_STALE=5"]


def build_oracle() -> None:
    """Test infrastructure: our CPU restatement, and the reference itself when its
    sources are present (build container only)."""
    _run(["make", "-s", "-C", ROOT / "oracle", "oracle"])
    if os.path.isdir("/root/reference/receiver"):   # False, not an error, where the directory exists but cannot be read
        _run(["make", "-s", "-C", ROOT / "oracle", "ref"])


if __name__ == "__main__":
    build_lib(force="--force" in sys.argv)
    if "--oracle" in sys.argv:
        build_oracle()
    # the fault-injection variant shares every object but two with the product: once it exists it is kept in step with
    # it (a variant left over from before an ABI change is refused by nvx_create, and the GPU suite's injection test with it)
    if "--inject" in sys.argv or (ROOT / "tests" / "_variants" / "libnavtex_amd_inject.so").exists():
        build_variant("inject", INJECT_FLAGS)
    if "--variant" in sys.argv:               # --variant NAME FLAG... [--sources a.hip,b.cpp]: A/B builds (tests/_variants/)
        rest = sys.argv[sys.argv.index("--variant") + 1:]
        srcs = ("nvx_cascade.hip", "nvx_wideband_fused.hip")
        if "--sources" in rest:
            k = rest.index("--sources"); srcs = tuple(rest[k + 1].split(",")); rest = rest[:k] + rest[k + 2:]
        print(build_variant(rest[0], rest[1:], srcs))
