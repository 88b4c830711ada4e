#!/usr/bin/env python3
"""Where the real-input converter's fourteen taps come from (include/navtex_amd_real.h; navtex_amd/real/nvx_real_taps.h holds
the numbers, and the numbers are the contract: this script documents them and must reproduce them).

  1. a half-band low-pass of 55 taps: h[n] = sinc(n / 2) / 2 for n = -27 .. 27, times numpy.kaiser(55, 8.25).  Its even
     taps but the centre are zero; the centre tap (1/2) is the I branch, a delay;
  2. the side taps h[2 j + 1], j = 0 .. 13, doubled (the filter has gain 2: a real tone of amplitude a leaves as a complex
     tone of amplitude a) and taken by magnitude: their signs (-1)^j are what the shift by fs/4 removes;
  3. normalised so that the alternating sum  a[0] - a[1] + a[2] - ...  is 1/2: unity gain at the band centre, and a zero at
     its image;
  4. rounded at 2^14;
  5. the residue 2^13 - (A[0] - A[1] + ...) put on A[0], so that the alternating sum is 2^13 exactly.

Prints the list, K and S, and with --response the pass-band ripple and the stop-band rejection computed from the integers.

    python tools/real_taps.py [--response]"""
import sys

import numpy as np

K, S = 13, 14
CONTRACT = (10376, 3314, 1825, 1144, 745, 486, 310, 191, 111, 60, 30, 13, 4, 1)


def design():
    n = np.arange(-27, 28)
    h = np.sinc(n / 2.0) / 2.0 * np.kaiser(55, 8.25)
    a = 2.0 * np.abs(h[27 + 1::2])                          # h[1], h[3], .. h[27]
    sign = (-1.0) ** np.arange(len(a))
    a *= 0.5 / float((sign * a).sum())
    A = [int(v) for v in np.rint(a * (1 << S))]
    A[0] += (1 << (S - 1)) - sum(v if j % 2 == 0 else -v for j, v in enumerate(A))
    return A


def response_db(taps, f):
    """The half-band filter's gain in dB at frequency f behind the shift, in units of the input rate fr, |f| <= 0.5.  A real
    tone at fr/4 + f comes out as (1 + G) / 2 of a tone at +f and (1 - G) / 2 of one at -f, with
    G(f) = sum (-1)^j A[j] cos(2 pi f (2 j + 1)) / 2^(S-1); G(1/2 - f) = -G(f), so the image of f is the filter's gain at
    1/2 - f: what lies at |f| >= 0.3 fr folds onto |f| <= 0.2 fr."""
    f = np.asarray(f, dtype=np.float64)
    j = np.arange(len(taps))
    g = (((-1.0) ** j * np.asarray(taps, dtype=np.float64))[None, :] * np.cos(2 * np.pi * f[:, None] * (2 * j[None, :] + 1))).sum(axis=1) / (1 << (S - 1))
    return 20 * np.log10(np.maximum(np.abs(1 + g) / 2, 1e-12))


def main():
    A = design()
    print(", ".join(str(v) for v in A))
    print(f"K = {K}, S = {S}, alternating sum {sum(v if j % 2 == 0 else -v for j, v in enumerate(A))}, 2 * sum {2 * sum(A)}")
    if "--response" in sys.argv:
        inner = np.linspace(-0.2, 0.2, 4001)
        outer = np.linspace(0.3, 0.5, 2001)
        print(f"|f| <= 0.2 fr: within {np.abs(response_db(A, inner)).max():.5f} dB; |f| >= 0.3 fr: at most {response_db(A, outer).max():.2f} dB")
    return 0 if tuple(A) == CONTRACT else 1


if __name__ == "__main__":
    sys.exit(main())
