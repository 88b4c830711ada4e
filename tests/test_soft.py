"""Soft-decision SITOR-B decoding (include/navtex_amd_soft.h) without a GPU: the header and its symbols, the restated
soft values (tests/soft_ref.py) against the oracle's bits, the soft character layer of nvx_sitor.c against its Python
restatement, and the acceptance case -- what the soft rule is for -- counted on the oracle's own 900 S/s samples."""
import ctypes as C
import functools
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import cases
import oracle_binding as ob
import signals
import soft_ref

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "navtex_amd_soft.h").read_text()
GOLD = json.loads((Path(__file__).parent / "golden" / "golden.json").read_text())


def _symbols():
    return sorted(set(re.findall(r"NVX_API\s+[\w\s\*]+?\b(\w+)\s*\(", HEADER)))


def test_header_compiles_as_plain_c_and_declares_the_entry_points(tmp_path):
    assert _symbols() == ["nvx_enable_soft", "nvx_poll_soft", "nvx_set_soft_message_fn", "nvx_sitor_receive_soft", "nvx_sitor_set_soft",
                          "nvx_soft_count"]
    assert "nvx_group_member" in HEADER                      # says how a group's members are reached
    src = tmp_path / "t.c"
    src.write_text('#include "navtex_amd_soft.h"\nint main(void){ return NVX_SOFT_DECODE + NVX_SOFT_KEEP - 3; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", "-c", str(src), "-o", str(tmp_path / "t.o")],
                   check=True)


@pytest.mark.parametrize("sym", _symbols())
def test_symbol_is_exported(nv, sym):
    assert hasattr(nv.lib, sym), f"{sym} is declared in navtex_amd_soft.h but not exported"
    assert nv.SOFT_DECODE == 1 and nv.SOFT_KEEP == 2


def test_null_objects_are_errors_or_no_ops_never_crashes(nv, tmp_path):
    src = ROOT / "tests" / "harness" / "null_args_soft.c"
    exe = tmp_path / "null_args_soft"
    lib = ROOT / "navtex_amd"
    subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib}", "-lnavtex_amd",
                    f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "soft null-safety ok" in out.stdout, (out.stdout[-1500:], out.stderr[-500:])
    assert all(re.search(rf"\b{s}\(", src.read_text()) for s in _symbols())


def test_without_a_device_there_is_no_soft_path_either(nv):
    """A handle is what soft decoding is turned on for, and there is none without a device (NVX_ERR_NODEV, no CPU path);
    with a device the three modes are accepted and anything else is NVX_ERR_ARG."""
    if nv.device_count() == 0:
        with pytest.raises(nv.NvxError) as e:
            nv.Pipeline()
        assert e.value.code == nv._native.ERR_NODEV
        return
    with nv.Pipeline() as p:
        for mode in (1, 3, 1, 0, 3, 0):
            p.enable_soft(mode)
        for bad in (2, 4, -1):
            assert nv.lib.nvx_enable_soft(p._h, bad) == nv._native.ERR_ARG


# ---- the values ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two_carrier", "weak_518", "offset_490", "ragged_length"])
def test_restated_values_carry_the_oracles_bits(nv, name):
    """On the goldens' signal-bearing IQ cases: as many values as bits, and soft > 0 exactly where the bit is 'B' -- the
    oracle's bits, which are the compiled reference's (golden)."""
    rec = GOLD["iq"][name]
    iq = cases.make_iq(nv, rec["spec"])
    p = ob.Pipe(chain_mask=3, charlayer=False, tap_y3=iq.shape[0] // 280 + 8)
    p.push(iq)
    fR, fI = ob.bitfilter_table()
    for chain, tag in ((0, "518"), (1, "490")):
        y3 = p.y3(chain)
        taps = ob.decode_taps(y3)
        assert taps["bits"] == p.bits(chain) == rec[f"bits{tag}"]
        v = soft_ref.values(y3, fR, fI, taps["bit_at"])
        assert v.dtype == np.float32 and v.shape[0] == len(taps["bits"]) > 0
        assert "".join("B" if x > 0 else "Y" for x in v) == taps["bits"]


# ---- the character layer ---------------------------------------------------------------------------------------------
def _as_values(bits: str, weight=1.0) -> np.ndarray:
    return np.array([weight if b == "B" else -weight for b in bits], dtype=np.float32)


@pytest.mark.parametrize("name", sorted(GOLD["charlayer"]))
def test_soft_off_is_receive_bits_on_the_signs(nv, name):
    """All 14 golden character-layer cases through nvx_sitor_receive_soft with the soft rule off: the reference's messages
    and its complete trace, whatever the magnitudes."""
    assert len(GOLD["charlayer"]) == 14
    rec = GOLD["charlayer"][name]
    bits = cases.make_bits(nv, rec["spec"])
    rng = np.random.default_rng(len(bits))
    v = _as_values(bits) * rng.uniform(1e-30, 1e30, len(bits)).astype(np.float32)
    s = nv.Sitor(518, trace=True)
    s.feed_soft(v)
    assert [list(m) for m in s.messages] == rec["messages"]
    assert s.trace() == rec["stdout"]
    # ... and the restatement with the rule off is the same machine
    r = soft_ref.SoftLayer(518, soft=False)
    r.feed(v)
    assert [list(m) for m in r.messages] == rec["messages"] and "".join(r.trace) == rec["stdout"]


@pytest.mark.parametrize("i", [0, 7, 31, 57, 99, 700])
def test_soft_mode_on_clean_unit_values_is_the_hard_layer(nv, i):
    text = signals.stream_text(i)
    bits = nv.sitor_encode(text, 40)
    hard = nv.Sitor(518, trace=True)
    hard.feed(bits)
    soft = nv.Sitor(518, soft=True, trace=True)
    soft.feed_soft(_as_values(bits))
    assert soft.messages == hard.messages == [(518, text[5:9], text)]
    assert soft.trace() == hard.trace()
    again = nv.Sitor(518, soft=True)                          # hard bits into a soft layer weigh +-1
    again.feed(bits)
    assert again.messages == hard.messages


def _both(nv, v):
    c = nv.Sitor(518, soft=True, trace=True)
    c.feed_soft(v)
    r = soft_ref.SoftLayer(518)
    r.feed(v)
    return c, r


@pytest.mark.parametrize("seed", range(12))
def test_c_layer_equals_the_restatement_on_random_metric_streams(nv, seed):
    """Two transmissions with noise on the metrics: continuous values, values on a half-integer grid (exact ties between
    the seven sums, exact zeros -- a zero is a 'Y'), or small integers (ties between sp and sd).  Messages and the whole
    trace (every printed character's mark, every line added to a message, every event) compared with ==."""
    rng = np.random.default_rng(1000 + seed)
    bits = nv.sitor_encode(signals.stream_text(seed), 40) + "B" * 50 + nv.sitor_encode(signals.stream_text(seed + 50), 12)
    sigma = (0.3, 0.45, 0.6)[seed % 3] * (0.6 if seed % 4 in (1, 2) else 1.0)       # (a grid adds its own rounding noise)
    v = _as_values(bits) * rng.uniform(0.5, 1.5, len(bits)) + rng.normal(0.0, sigma, len(bits))
    if seed % 4 == 1:
        v = np.round(v * 2) / 2
    if seed % 4 == 2:
        v = np.round(v * 2)
    v = v.astype(np.float32)
    c, r = _both(nv, v)
    assert c.messages == r.messages
    assert c.trace() == "".join(r.trace)
    assert "phasing detected\n" in r.trace and len(r.printed) > 50
    if seed % 4 in (1, 2):
        assert (v == 0).sum() > 10


def test_c_layer_equals_the_restatement_with_phasing_cut_at_every_bit_offset(nv):
    """The input starts k bits into the phasing run, k = 0 .. 27 (two codes): whichever slot and bit the layer wakes up on,
    the phasing pairs print nothing, and C and restatement agree."""
    text = "ZCZC CU00\nCUT\nNNNN\n"
    bits = nv.sitor_encode(text, 40)
    rng = np.random.default_rng(5)
    for k in range(28):
        v = (_as_values(bits[k:]) * rng.uniform(0.8, 1.2, len(bits) - k)).astype(np.float32)
        c, r = _both(nv, v)
        assert c.messages == r.messages == [(518, "CU00", text)], k
        assert c.trace() == "".join(r.trace), k
        assert "".join(r.printed) == text.replace("\n", ""), k          # nothing printed through the phasing run


def test_the_phasing_hypothesis_is_what_keeps_the_phasing_run_silent():
    """Clean phasing pairs (DX = beta, RX = alpha) under the data hypothesis alone would print a character; sp > sd there."""
    alpha = [-1.0 if (soft_ref.ALPHA >> (6 - i)) & 1 else 1.0 for i in range(7)]
    beta = [-1.0 if (soft_ref.BETA >> (6 - i)) & 1 else 1.0 for i in range(7)]
    assert soft_ref.soft_code(alpha, beta) == soft_ref.ALPHA
    e = [-1.0 if (0x4A >> (6 - i)) & 1 else 1.0 for i in range(7)]
    assert soft_ref.soft_code(e, e) == 0x4A
    assert soft_ref.soft_code([0.0] * 7, [0.0] * 7) == 0x70           # all tied: the three earliest bits are 'Y'; sp == sd is data


# ---- the acceptance case -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _acceptance(nv, amplitude, noise_amp):
    """Per seed: (the reference rule's messages on the oracle's bits, the product's soft layer's on the restated values)."""
    fR, fI = ob.bitfilter_table()
    out = []
    for seed in soft_ref.ACCEPT_SEEDS:
        st, frames, want = soft_ref.accept_stream(nv, seed, amplitude, noise_amp)
        iq = nv.synth_host(st, nv.RATE_IN, frames * nv.FRAME_IN)
        p = ob.Pipe(chain_mask=1, charlayer=False, tap_y3=frames * nv.FRAME_Y3)
        p.push(iq)
        y3 = p.y3(0)
        taps = ob.decode_taps(y3)
        assert taps["bits"] == p.bits(0)
        hard = ob.CharLayer(518)
        hard.feed(taps["bits"])
        soft = nv.Sitor(518, soft=True)
        soft.feed_soft(soft_ref.values(y3, fR, fI, taps["bit_at"]))
        out.append((hard.messages, soft.messages, (518,) + want))
    return out


def test_acceptance_weak_carrier_soft_rule_delivers_where_the_reference_rule_does_not(nv):
    """Amplitude 300, noise_amp 6000, seeds 11 .. 22: H = runs in which the reference's rule delivers exactly ('HA07',
    text), S = the same for the soft layer.  Asserted: S >= H + 6.  Counted here: H = 1, S = 12."""
    runs = _acceptance(nv, 300, 6000)
    H = sum(h == [want] for h, s, want in runs)
    S = sum(s == [want] for h, s, want in runs)
    print(f"acceptance at noise_amp 6000: H = {H}, S = {S} of {len(runs)}")
    assert len(runs) == 12 and S >= H + 6, (H, S)


def test_acceptance_strong_carrier_both_rules_deliver_everything(nv):
    runs = _acceptance(nv, 8000, 1500)
    for h, s, want in runs:
        assert h == s == [want]
