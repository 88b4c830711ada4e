"""The launch arithmetic the same-rate companions share (navtex_amd/csrc/nvx_stream_plan.h) on the CPU: a stand-alone program
under ASan + UBSan walks it against arithmetic restated there."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_chunk_split_wanted_rule_and_row_alignment_against_restated_arithmetic(tmp_path):
    """nvx_stream_chunks for every number of tiles in 0..300, chunks wanted in -1..40, 683 and 2048 and shortest chunks of
    1, 4 and 32 tiles -- each tile in exactly one chunk, no chunk empty, no more chunks than wanted, every chunk but the last
    whole, none below the shortest where there are several, no tiles one chunk; nvx_stream_wanted around 1024 rows; and
    nvx_stream_rows_aligned16 row by row (tests/harness/stream_plan_core.cpp).  No device, no HIP."""
    exe = tmp_path / "stream_plan_core"
    subprocess.run(["g++", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    f"-I{ROOT / 'navtex_amd' / 'csrc'}", str(ROOT / "tests" / "harness" / "stream_plan_core.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env={"ASAN_OPTIONS": "detect_leaks=1", "PATH": "/usr/bin:/bin"})
    assert out.returncode == 0 and "stream plan core ok" in out.stdout, (out.stdout + out.stderr)[-3000:]


def test_the_pure_header_is_c():
    """The header is read by C as well: it compiles as C with no HIP on the include path."""
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", str(ROOT / "navtex_amd" / "csrc" / "nvx_stream_plan.h")],
                   check=True)
