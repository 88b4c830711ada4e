"""The polyphase design the rate changers share (navtex_amd/csrc/nvx_polyphase_design.h) on the CPU: a stand-alone program under
ASan + UBSan walks the resampler's, the narrowband interpolator's and the channel tap's designs, which all stand on it."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "navtex_amd"


def test_the_three_designs_keep_their_headers_promises_under_asan_ubsan(tmp_path):
    """For the rates the tests name (resample_ref.RATES with 252252 and 100100, narrow_cases.DESIGN_RATES, tap_cases.DESIGNS) and
    the rates at the edges of each range (L = 1008, L * T = 32760 / 30240 / 32756, the longest phase, the ends): every phase
    sums to exactly 2^S, the taps lie in int16 or below 2^24, a phase's absolute sum stays within 65535 or below 2^24 and the
    tap's high halves within 65535, T is even, L * T fits the table, and ceil(n L / M) equals its restatement by quotient and
    remainder at positions up to 2^62 (tests/harness/polyphase_design_core.c).  The taps lie in allocations of exactly L * T
    entries.  No device, no HIP, no Python in the process."""
    exe = tmp_path / "polyphase_design_core"
    subprocess.run(["gcc", "-std=gnu11", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", f"-I{ROOT / 'include'}", f"-I{PKG / 'csrc'}", f"-I{PKG / 'resample'}",
                    f"-I{PKG / 'narrow'}", f"-I{PKG / 'tap'}", str(ROOT / "tests" / "harness" / "polyphase_design_core.c"),
                    str(PKG / "resample" / "nvx_resample_design.c"), str(PKG / "narrow" / "nvx_narrow_design.c"), str(PKG / "tap" / "nvx_tap_design.c"),
                    "-o", str(exe), "-lm"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env={"ASAN_OPTIONS": "detect_leaks=1", "PATH": "/usr/bin:/bin"})
    assert out.returncode == 0 and "polyphase design core ok" in out.stdout, (out.stdout + out.stderr)[-3000:]


def test_the_design_header_is_c99_alone():
    """The header is pure C with no HIP: it compiles as C99 on its own, with nothing else on the include path."""
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", str(PKG / "csrc" / "nvx_polyphase_design.h")], check=True)
