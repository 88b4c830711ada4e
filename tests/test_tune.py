"""Per-chain carrier tuning (include/navtex_amd_tune.h) on CPU: the header and its null-argument safety, the generated
mixer table (correctly rounded, exact symmetries), and the restatement (tests/tune_ref.py): bit-identical to the
oracle's own pipeline at the nominal carriers, and the one that decodes a carrier the reference mixer cannot."""
import re
import subprocess
from decimal import Decimal, getcontext
from pathlib import Path

import numpy as np
import pytest

import oracle_binding as ob
import signals
import tune_ref as tr

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "navtex_amd_tune.h").read_text()


def _symbols():
    return sorted(set(re.findall(r"NVX_API\s+[\w\s\*]+?\b(\w+)\s*\(", HEADER)))


def test_header_compiles_as_plain_c_and_declares_the_four_entry_points(tmp_path):
    assert _symbols() == ["nvx_get_carrier", "nvx_group_get_carrier", "nvx_group_set_carrier", "nvx_set_carrier"]
    for name, want in (("NVX_TUNE_N", "20160"), ("NVX_TUNE_STEP_HZ", "3.125"), ("NVX_TUNE_MAX_HZ", "25000.0")):
        assert re.search(rf"#define {name}\s+{re.escape(want)}\b", HEADER), name
    src = tmp_path / "t.c"
    src.write_text('#include "navtex_amd_tune.h"\nint main(void){ return NVX_TUNE_N * NVX_TUNE_STEP_HZ == 63000.0 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(tmp_path / "t")], check=True)
    assert subprocess.run([str(tmp_path / "t")]).returncode == 0


@pytest.mark.parametrize("sym", _symbols())
def test_symbol_is_exported(nv, sym):
    assert hasattr(nv.lib, sym), f"{sym} is declared in navtex_amd_tune.h but not exported"


def test_null_objects_are_errors_never_crashes(nv, tmp_path):
    src = ROOT / "tests" / "harness" / "null_args_tune.c"
    exe = tmp_path / "null_args_tune"
    lib = ROOT / "navtex_amd"
    subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib}", "-lnavtex_amd",
                    f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "tune null-safety ok" in out.stdout, (out.stdout[-1500:], out.stderr[-500:])
    assert all(re.search(rf"\b{s}\(", src.read_text()) for s in _symbols())


def test_the_table_is_the_generator_output():
    import importlib.util
    import tempfile
    spec = importlib.util.spec_from_file_location("gen_tune_table", ROOT / "tools" / "gen_tune_table.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with tempfile.TemporaryDirectory() as d:
        out = Path(d) / "t.h"
        subprocess.run(["python3", str(ROOT / "tools" / "gen_tune_table.py"), str(out)], check=True)
        assert out.read_text() == tr.HEADER.read_text()


def test_octant_is_correctly_rounded_against_decimal():
    """Every stored value is within half an ulp of cos / sin evaluated in decimal at 60 digits."""
    getcontext().prec = 70
    # pi to 70 digits by Machin's formula, independent of the generator's code path
    def atan_inv(x):
        total = term = Decimal(1) / x
        k, x2 = 1, x * x
        while True:
            term /= -x2
            nxt = total + term / (2 * k + 1)
            if nxt == total:
                return total
            total, k = nxt, k + 1
    pi = 4 * (4 * atan_inv(5) - atan_inv(239))
    for j, (c, s) in enumerate(tr.octant()):
        x = 2 * pi * j / tr.N
        # cos and sin by their series
        cs, ss, term, n = Decimal(1), Decimal(0), Decimal(1), 0
        while True:
            n += 1
            term = term * x / n
            if term == 0 or abs(term) < Decimal(10) ** -68:
                break
            if n % 2:
                ss += term if n % 4 == 1 else -term
            else:
                cs += term if n % 4 == 0 else -term
        for got, exact in ((c, cs), (s, ss)):
            ulp = np.spacing(abs(got)) if got != 0 else np.spacing(0.0)
            assert abs(Decimal(got) - exact) <= Decimal(ulp) / 2, (j, got, exact)


def test_the_full_turn_follows_by_exact_symmetries():
    cr, ci = tr.table()
    n, q = tr.N, tr.N // 4
    j = np.arange(n)
    assert cr[0] == 1.0 and ci[0] == 0.0 and cr[q] == 0.0 and ci[q] == -1.0 and cr[2 * q] == -1.0 and cr[3 * q] == 0.0 and ci[3 * q] == 1.0
    assert np.array_equal(cr[(n - j) % n], cr) and np.array_equal(ci[(n - j) % n], -ci)          # conjugate symmetry
    assert np.array_equal(cr[(j + 2 * q) % n], -cr) and np.array_equal(ci[(j + 2 * q) % n], -ci)   # half turn
    assert np.array_equal(cr[(q - j) % n], -ci)                                                    # cos(pi/2 - x) = sin x
    assert np.max(np.abs(cr - np.cos(2 * np.pi * j / n))) < 2e-15 and np.max(np.abs(ci + np.sin(2 * np.pi * j / n))) < 2e-15


def _stream(nv, freq_hz, text, rate, frames, seed=3):
    st, _ = signals.stream_params(nv, seed, rate, freq_hz=freq_hz, text=text)
    frame = nv.FRAME_RAW if rate == nv.RATE_RAW else nv.FRAME_IN
    return nv.synth_host(st, rate, frames * frame)


@pytest.mark.parametrize("raw", [False, True], ids=["252k", "raw"])
def test_nominal_restatement_is_the_oracles_pipeline(nv, raw):
    """At k = +-4480 the restatement runs the oracle's own mixer: its bits are the oracle pipe's.  And the tuned mixer at
    k = +-4480 (T's entries instead of the reference's libm table) changes y3 only in the last bits, not one bit."""
    rate = nv.RATE_RAW if raw else nv.RATE_IN
    frames = 3 if raw else 12
    car = [dict(freq_hz=14000, bits=nv.sitor_encode("ZCZC EA01\nNOMINAL\nNNNN\n", 40), bit_offset=301, phase0=5),
           dict(freq_hz=-14000, bits=nv.sitor_encode("ZCZC GB42\nNOMINAL TOO\nNNNN\n", 40), bit_offset=777, phase0=9)]
    frame = nv.FRAME_RAW if raw else nv.FRAME_IN
    iq = nv.synth_host(nv.make_stream(car, seed=11, noise_amp=1500), rate, frames * frame)
    pipe = ob.Pipe(chain_mask=3, charlayer=False, tap_y3=frames * nv.FRAME_Y3)
    (pipe.push_raw if raw else pipe.push)(iq)
    y1 = tr.front(iq, raw)
    for ch in (0, 1):
        y3 = tr.chain(y1, ch, tr.NOMINAL[ch])
        assert np.array_equal(y3.view(np.uint64), pipe.y3(ch)[:y3.shape[0]].view(np.uint64))
        assert tr.decode(y3) == pipe.bits(ch)
        y3t = ob.fir3(ob.fir2(tr.mix_tuned(y1, tr.NOMINAL[ch])))
        assert np.max(np.abs(y3t - y3)) <= 1e-14 * np.max(np.abs(y3))
        assert tr.decode(y3t) == tr.decode(y3)


def test_a_carrier_150_hz_off_decodes_only_through_the_tuned_mixer(nv):
    text = "ZCZC AB12\nTUNED CARRIER TEST\nNNNN\n"
    iq = _stream(nv, 14150, text, nv.RATE_IN, 40)
    y1 = tr.front(iq, False)
    assert tr.messages(tr.decode(tr.chain(y1, 0, tr.NOMINAL[0]))) == []
    k = tr.k_of(14150)
    assert k == 4528
    assert tr.messages(tr.decode(tr.chain(y1, 0, k))) == [text]
