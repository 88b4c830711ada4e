"""Restatement of soft-decision SITOR-B decoding (include/navtex_amd_soft.h), written from the header's definition, not from
the kernels or from nvx_sitor.c.

1. The values.  soft = Brot - Yrot, one float32 subtraction of the two float32 energies (signal_ref.energies, the
   restatement of receiver/decoder.C:115-132) of the five-sample window ENDING on the sample where the bit FSM decided a
   bit -- the samples where oracle_binding.decode_taps(...)["bit_at"] is non-zero.
2. The soft character layer: the reference's byte_state_machine (receiver/nav_b_sm.C) with one change, the character
   printed in the RX slot, which is decided from the soft values of the RX code and of its DX twin.  Control (phasing
   detector, slot tracking, end of emission, error window, mute) runs on the hard bits, the sign of the values."""
from __future__ import annotations

import re

import numpy as np

import signal_ref

ALPHA, BETA = 0x07, 0x4C
PHASING = "BBBBBBYYYYBBYYBBBBBBYYYYBBYYBB"
MUTE_BITS, ERRWIN, ERRMAX = 1100, 20, 12
SOM = re.compile(r"(CZC|Z.ZC|ZC.C|ZCZ.) +([A-Z][A-Z])([0-9][0-9])", re.S)
EOM = re.compile(r"NNN|N.NN|NN.N", re.S)
LINE_MAX = 4999
# CCIR-476 code -> character, letters and figures (nav_b_sm.h:60-83): 34 of the 35 codes with three 'Y' bits (0x54 is
# unassigned: the layer prints '_' for it, as the reference's table reads) plus 0x5C, which the reference decodes as a blank
LTRS = {0x0B: "J", 0x0D: "W", 0x0E: "A", 0x13: "F", 0x15: "Y", 0x16: "S", 0x19: "-", 0x1A: "D", 0x1C: "Z", 0x23: "C", 0x25: "P",
        0x26: "I", 0x29: "G", 0x2A: "R", 0x2C: "L", 0x31: "M", 0x32: "N", 0x34: "H", 0x38: "O", 0x43: "K", 0x45: "Q", 0x46: "U",
        0x4A: "E", 0x51: "X", 0x58: "B", 0x5C: " ", 0x61: "V", 0x62: " ", 0x68: "T"}
FIGS = {0x0B: "b", 0x0D: "2", 0x0E: "-", 0x13: "*", 0x15: "6", 0x16: "'", 0x19: "-", 0x1A: "%", 0x1C: "+", 0x23: ":", 0x25: "0",
        0x26: "8", 0x29: "*", 0x2A: "4", 0x2C: ")", 0x31: ".", 0x32: ",", 0x34: "*", 0x38: "9", 0x43: "(", 0x45: "1", 0x46: "7",
        0x4A: "3", 0x51: "/", 0x58: "?", 0x5C: " ", 0x61: "=", 0x62: " ", 0x68: "5"}
CONTROL = {0x07: "alpha", 0x4C: "beta", 0x49: "figs", 0x52: "ltrs", 0x64: "lf", 0x70: "cr"}
VALID = set(LTRS) | set(CONTROL)


def values(y3: np.ndarray, fR, fI, bit_at: np.ndarray) -> np.ndarray:
    """float32 soft values of a chain whose samples since reset are y3, for the bits decided where bit_at != 0."""
    B, Y = signal_ref.energies(y3, fR, fI)
    assert B.dtype == np.float32 and Y.dtype == np.float32
    return (B - Y)[np.asarray(bit_at) != 0]


def soft_code(rx, dx) -> int:
    """The code printed for an RX code with metrics rx and its DX twin with metrics dx (python floats = double)."""
    m = [float(r) + float(d) for r, d in zip(rx, dx)]
    total = 0.0
    for v in m:
        total += v
    order = sorted(range(7), key=lambda i: (m[i], i))     # the three smallest, ties to the earlier bit
    ys = set(order[:3])
    three = 0.0
    for i in range(7):
        if i in ys:
            three += m[i]
    sd = total - 2.0 * three
    sp_rx = sp_dx = 0.0
    for i in range(7):
        sp_rx += -float(rx[i]) if (ALPHA >> (6 - i)) & 1 else float(rx[i])
    for i in range(7):
        sp_dx += -float(dx[i]) if (BETA >> (6 - i)) & 1 else float(dx[i])
    if sp_rx + sp_dx > sd:
        return ALPHA
    return sum(1 << (6 - i) for i in ys)


class SoftLayer:
    """The soft character layer: feed(values) -> self.messages [(freq, bbbb, text)], self.printed (every character and
    '*' appended to a line, in order: the emitted text) and self.trace (what the reference prints on its way, nav_b_sm.C:
    the text nvx_sitor_set_trace hands out)."""

    def __init__(self, freq: int = 518, soft: bool = True):
        self.freq, self.soft = freq, soft
        self.messages, self.printed, self.trace = [], [], []
        self.acc, self.cur = 0, [0.0] * 7
        self._reset()

    def _reset(self):
        self.matched = self.mute = self.nbits = 0
        self.enabled = False
        self.slot = "search"
        self.figures = False
        self.dx, self.dxm, self.dx_pos, self.dx_full = [0, 0, 0], [None, None, None], 0, False
        self.idle_run, self.prev_dx_idle = 0, False
        self.errs = []
        self.err_count = 0
        self.line, self.text, self.bbbb, self.in_message = "", "", "", False

    def _abort(self):
        self.trace.append("message abort\n")
        if self.in_message:
            self.messages.append((self.freq, self.bbbb, self.text))
        self._reset()

    def _append_line(self, ch):
        self.printed.append(ch)
        if len(self.line) < LINE_MAX:
            self.line += ch

    def _line_feed(self):
        if self.in_message:
            self.text = (self.text + self.line)[:LINE_MAX]
            self.text = (self.text + "\n")[:LINE_MAX]
            self.trace.append(f"line added: {self.line}\n")
        m = SOM.search(self.line)
        if m:
            self.text = (self.line[:LINE_MAX] + "\n")[:LINE_MAX]
            self.bbbb = (self.bbbb + m.group(2) + m.group(3))[:4]
            self.in_message = True
            self.trace.append("============START OF MESSAGE============ \n")
        elif EOM.search(self.line):
            if self.in_message:
                self.messages.append((self.freq, self.bbbb, self.text))
            self.text, self.bbbb, self.in_message = "", "", False
            self.trace.append("============ END OF MESSAGE ============\n")
        self.line = ""

    def _emit(self, code):
        if code == 0:
            self.trace.append("*")
            self._append_line("*")
            return
        kind = CONTROL.get(code)
        if kind == "ltrs":
            self.figures = False
        elif kind == "figs":
            self.figures = True
        elif kind == "lf":
            self._line_feed()
        elif kind is None:
            self.trace.append(".;")
            self._append_line((FIGS if self.figures else LTRS).get(code, "_"))

    def _code(self, code):
        if self.slot == "search":
            if code == ALPHA:
                self.slot = "dx"
            if code == BETA:
                self.slot = "rx"
        elif self.slot == "dx":
            self.dx[self.dx_pos], self.dxm[self.dx_pos] = code, list(self.cur)
            self.dx_pos += 1
            if self.dx_pos == 3:
                self.dx_pos, self.dx_full = 0, True
            ended = False
            if code == ALPHA:
                self.trace.append("\n alpha received in DX position\n")
                if self.prev_dx_idle:
                    self.idle_run += 1
                    if self.idle_run == 2:
                        self.trace.append("\nend of emission detected\n\nstopping reception\n")
                        self._abort()
                        ended = True
                if not ended:
                    self.prev_dx_idle = True
            else:
                self.prev_dx_idle = False
            if not ended:
                self.slot = "rx"
        else:
            if self.dx_full:
                twin = self.dx[self.dx_pos]
                if self.soft:
                    self._emit(soft_code(self.cur, self.dxm[self.dx_pos]))
                elif code in VALID:
                    self._emit(code)
                elif twin in VALID:
                    self._emit(twin)
                else:
                    self._emit(0)
            self.slot = "dx"
        bad = code not in VALID
        if len(self.errs) == ERRWIN:
            self.err_count -= self.errs.pop(0)
        self.errs.append(int(bad))
        self.err_count += int(bad)
        if self.err_count > ERRMAX:
            self._emit(0)
            self.trace.append("\n error th exceeded \n")
            self._abort()

    def feed(self, soft) -> None:
        for v in np.asarray(soft, dtype=np.float32):
            bit = "B" if v > 0 else "Y"
            if self.enabled:
                self.cur[self.nbits] = float(v)
                self.acc = ((self.acc << 1) | (bit == "Y")) & 0xFF
                self.nbits += 1
                if self.nbits == 7:
                    code = self.acc & 0x7F
                    self._code(code)
                    self.nbits, self.acc = 0, 0
            if self.mute:
                self.mute -= 1
                if self.mute == 0:
                    self.trace.append("phase det disable timer expired\n")
                continue
            if self.matched == 29:
                if bit == "B":
                    self.enabled, self.nbits, self.acc = True, 0, 0
                    self.trace.append("phasing detected\n")
                    self.mute = MUTE_BITS
                self.matched = 0
            elif bit == PHASING[self.matched]:
                self.matched += 1
            elif self.matched != 6:
                self.matched = 0


# ---- the acceptance case of the soft decoder: one weak carrier, twelve noise seeds ----------------------------------
ACCEPT_SEEDS = tuple(range(11, 23))
ACCEPT_ID = 7


def accept_stream(nv, seed: int, amplitude: int, noise_amp: int):
    """(SynthStream, frames at 252 kS/s, (bbbb, text)) of one acceptance run."""
    import signals
    text = signals.stream_text(ACCEPT_ID)
    bits = nv.sitor_encode(text, 40)
    secs = (len(bits) + 400) / 100
    frames = int(secs * 252000) // nv.FRAME_IN + 1
    st = nv.make_stream([dict(freq_hz=14000, bits=bits, bit_offset=301, phase0=5, amplitude=amplitude)], seed=seed, noise_amp=noise_amp)
    return st, frames, ("HA07", text)
