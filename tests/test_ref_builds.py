"""Which BUILDS of the reference the parity claims cover (build container only: needs /root/reference and g++).

The committed vectors (tests/golden/golden.json) come from the reference compiled the way its autotools set-up compiles
it on x86-64: `-g -O2`, no -march, no fast-math -- so no FMA contraction (configure.ac:1-12 sets no CXXFLAGS;
receiver/configure.ac:3-4 would set -O3 if the receiver were configured stand-alone).  Here the same sources are compiled
again, into scratch directories, with the flags of other plausible builds, and the whole golden record is regenerated from
each:

  -O3                         every field identical, byte for byte: the fp64 seam claims hold for both optimisation levels
                              the reference's build files can produce on x86-64;
  -O2 -march=haswell -mfma    what GCC does by default where the ISA has fused multiply-add (the aarch64 boards such a
                              receiver usually runs on contract the same way): every fp64 seam of every signal-bearing
                              case CHANGES -- seam-level bit-exactness is a statement about the no-FMA build -- while every
                              bit string, message, decoder output and character-layer trace stays the same: decision-level
                              parity holds for FMA-contracted builds too.
"""
import json
import os
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
REF_SRC = Path("/root/reference/receiver")
GOLDEN = ROOT / "tests" / "golden" / "golden.json"

pytestmark = [pytest.mark.ref,
              pytest.mark.skipif(not os.path.isdir(REF_SRC) or shutil.which("g++") is None, reason="needs the reference's sources and g++ (build container only)")]

SEAMS = ("y1", "y2_518", "y2_490", "y3_518", "y3_490")


def _cpu_has_fma() -> bool:
    try:
        return " fma " in Path("/proc/cpuinfo").read_text().replace("\n", " ")
    except OSError:
        return False


def _regenerate(tmp_path, flags):
    """oracle/Makefile's own `ref` recipe with other REFFLAGS, objects and seam binaries under tmp_path only."""
    out = tmp_path / "ref"
    subprocess.run(["make", "-s", "-C", str(ROOT / "oracle"), "ref", f"OUT={out}", f"REFFLAGS={flags} -I{REF_SRC}"], check=True, capture_output=True)
    sys.path.insert(0, str(ROOT / "tests" / "golden"))
    import make_golden
    return make_golden.generate(ref_dir=out, verbose=False)


def test_o3_build_reproduces_the_golden_vectors_byte_for_byte(tmp_path):
    got = _regenerate(tmp_path, "-g -O3")
    assert json.dumps(got, indent=1) == GOLDEN.read_text()


@pytest.mark.skipif(not _cpu_has_fma(), reason="this host cannot run an FMA build")
def test_fma_contracted_build_changes_every_seam_and_no_decision(tmp_path):
    got = _regenerate(tmp_path, "-g -O2 -march=haswell -mfma")
    gold = json.loads(GOLDEN.read_text())
    changed, same = [], []
    for name, rec in gold["iq"].items():
        new = got["iq"][name]
        for field in ("bits518", "bits490", "stdout_sha256", "iq_sha256"):
            assert new[field] == rec[field], f"{name}.{field}"
        assert [list(m) for m in new["messages"]] == [list(m) for m in rec["messages"]], name
        for seam in SEAMS:
            assert new[seam]["n_doubles"] == rec[seam]["n_doubles"]
            (same if new[seam]["sha256"] == rec[seam]["sha256"] else changed).append(f"{name}.{seam}")
    # every seam that carries signal moves; all-zero input stays all-zero under any rounding
    assert sorted(same) == sorted(f"silence.{s}" for s in SEAMS), same
    assert len(changed) == (len(gold["iq"]) - 1) * len(SEAMS)
    for name, rec in gold["decoder"].items():
        assert got["decoder"][name]["bits"] == rec["bits"], name
    for name, rec in gold["charlayer"].items():
        assert got["charlayer"][name]["stdout"] == rec["stdout"] and [list(m) for m in got["charlayer"][name]["messages"]] == [list(m) for m in rec["messages"]], name
    assert got["wav"] == gold["wav"] and got["tables"] == gold["tables"]
