#!/usr/bin/env python3
"""Instruction-level comparison of the cascade kernels between two source trees.

    python tools/isa_diff.py <git rev> [kernel regex] [--all]

Compiles navtex_amd/csrc/nvx_cascade.hip of <git rev> and of the working tree for gfx950 (device only, -S) and compares
the instruction streams of the kernels whose demangled names match in both (labels and comments removed).  With --all:
every device translation unit of libnavtex_amd.so (navtex_amd/csrc/*.hip), of the scan library (navtex_amd/scan/*.hip), of
the resampler (navtex_amd/resample/*.hip), of the down-converter bank (navtex_amd/ddc/*.hip), of the blanker
(navtex_amd/blank/*.hip), of the IQ corrector (navtex_amd/iqc/*.hip), of the real-input converter (navtex_amd/real/*.hip), of
the narrowband interpolator (navtex_amd/narrow/*.hip), of the channel tap (navtex_amd/tap/*.hip), of the noise canceller
(navtex_amd/anc/*.hip), of the tone notch (navtex_amd/notch/*.hip) and of the zoom bank (navtex_amd/zoom/*.hip; all with the
resampler's, the bank's and the converter's directories on their include path), each where the revision has it.  That is how a feature that lives in a library of its own shows that it left
the other kernels alone (profiles/resample_isa_identical.txt, profiles/ddc_isa_identical.txt,
profiles/blank_isa_identical.txt, profiles/iqc_isa_identical.txt, profiles/real_isa_identical.txt,
profiles/zoom_isa_identical.txt), and how
a change that moves code between these files shows that no kernel changed (profiles/rs_shared_isa_identical.txt,
profiles/stream_device_isa_identical.txt).  Used in
round 5 to show that pruning the A/B alternates out of the roofline kernel changed no instruction of the kernels that
ship (profiles/r05/a0_prune_isa_identical.txt); hipcc cross-compiles, no GPU needed."""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
COMPANIONS = ("navtex_amd/scan", "navtex_amd/resample", "navtex_amd/ddc", "navtex_amd/blank", "navtex_amd/iqc", "navtex_amd/real",
              "navtex_amd/narrow", "navtex_amd/tap", "navtex_amd/anc", "navtex_amd/notch", "navtex_amd/zoom")


def compile_tree(tree: Path, out: Path, everything: bool = False) -> dict:
    csrc = tree / "navtex_amd" / "csrc"
    sources = [csrc / "nvx_cascade.hip"]
    if everything:
        sources = sorted(csrc.glob("*.hip")) + [src for d in COMPANIONS for src in sorted((tree / d).glob("*.hip"))]
    text = ""
    for src in sources:
        subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", f"-I{tree / 'include'}", f"-I{csrc}",
                        f"-I{src.parent}", f"-I{tree / 'navtex_amd' / 'resample'}", f"-I{tree / 'navtex_amd' / 'ddc'}", f"-I{tree / 'navtex_amd' / 'real'}", "-cuid=same", "--cuda-device-only", "-S", str(src), "-o", str(out)], check=True, capture_output=True)
        text += out.read_text()
    kernels = {}
    for sym in re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, flags=re.M):         # the kernels, not the data symbols
        m = re.search(rf"^{re.escape(sym)}:.*?s_endpgm", text, flags=re.S | re.M)
        name = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
        name = re.sub(r"^void |\(.*$", "", name)
        body = [re.sub(r"\.LBB\d+_\d+", "L", re.sub(r";.*", "", l)).strip() for l in m.group(0).splitlines()
                if l.startswith("\t") and not l.strip().startswith((".", ";"))]
        kernels[name] = body
    return kernels


def canonical(name: str) -> str:
    # round-4 trees carried two more template parameters (passes of prefetch, non-temporal loads): <RAW, NCH, 1, true>
    return re.sub(r"nvx_fir_cascade<(\w+), (\d), 1, true>", r"nvx_fir_cascade<\1, \2>", name)


def main():
    everything = "--all" in sys.argv
    args = [a for a in sys.argv[1:] if a != "--all"]
    rev = args[0]
    pat = re.compile(args[1] if len(args) > 1 else ".")
    with tempfile.TemporaryDirectory() as td:
        old = Path(td) / "old"
        old.mkdir()
        extra = [d for d in COMPANIONS if everything and
                 subprocess.run(["git", "-C", str(ROOT), "cat-file", "-e", f"{rev}:{d}"], capture_output=True).returncode == 0]
        tar = subprocess.run(["git", "-C", str(ROOT), "archive", rev, "navtex_amd/csrc", *extra, "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "x", "-C", str(old)], input=tar, check=True)
        a = {canonical(k): v for k, v in compile_tree(old, Path(td) / "a.s", everything).items()}
        b = compile_tree(ROOT, Path(td) / "b.s", everything)
    print(f"{rev}: {len(a)} kernels; working tree: {len(b)} kernels")
    same = True
    for name in sorted(b):
        if not pat.search(name):
            continue
        if name not in a:
            print(f"  {name}: not in {rev}"); continue
        eq = a[name] == b[name]
        same &= eq
        print(f"  {name}: {len(a[name])} / {len(b[name])} instructions, {'IDENTICAL' if eq else 'DIFFERENT'}")
    print("only in", rev + ":", sorted(set(a) - set(b)))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
