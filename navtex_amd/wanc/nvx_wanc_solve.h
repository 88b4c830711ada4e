/* nvx_wanc_solve.h -- steps 1 .. 7 of the multi-tap canceller's solve (include/navtex_amd_wanc.h), as one function that the
 * solve kernel (nvx_wanc.hip) runs per lane and tests/harness/wanc_solve.cpp runs on the host.  Its working numbers live in
 * memory the caller hands over, `stride` doubles apart (a lane's column of the LDS; 1 on the host), so that nothing is
 * indexed in registers.  The quotients are formed in integers (nvx_wanc_div): the processor's fp64 division is a sequence of
 * fused multiply-adds, and this file is compiled without any; the result is the IEEE one bit for bit.  Internal. */
#ifndef NVX_WANC_SOLVE_H
#define NVX_WANC_SOLVE_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "navtex_amd_wanc.h"

#if defined(__HIPCC__)
#define NVX_WANC_HD __host__ __device__ __forceinline__
#else
#define NVX_WANC_HD static inline
#endif

/* the doubles a solve works in: rr, ri, qr, qi, d, e, xr, xi (K each), then Lr and Li (K (K - 1) / 2 each, row i from
 * i (i - 1) / 2 on) */
#define NVX_WANC_WS_DOUBLES(k) (8 * (k) + (k) * ((k) - 1))

NVX_WANC_HD uint64_t nvx_wanc_bits(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }
NVX_WANC_HD double nvx_wanc_from_bits(uint64_t b) { double v; memcpy(&v, &b, 8); return v; }

/* a finite, non-zero magnitude as m * 2^(e - 1075) with 2^52 <= m < 2^53 */
NVX_WANC_HD void nvx_wanc_split(uint64_t mag, uint64_t *m, int *e)
{
    *e = (int)(mag >> 52); *m = mag & 0xfffffffffffffull;
    if (*e == 0) { const int sh = __builtin_clzll(*m) - 11; *m <<= sh; *e = 1 - sh; }
    else *m |= 1ull << 52;
}

/* n / d for a finite or infinite n (a NaN is returned as it is) and a finite d > 0: the IEEE quotient, round to nearest even,
 * subnormal results and overflow included, by long division of the significands. */
NVX_WANC_HD double nvx_wanc_div(double n, double d)
{
    const uint64_t nb = nvx_wanc_bits(n), sign = nb & 0x8000000000000000ull, mag = nb & 0x7fffffffffffffffull;
    if (mag == 0 || (mag >> 52) == 0x7ff) return n;
    uint64_t mn, md;
    int en, ed;
    nvx_wanc_split(mag, &mn, &en);
    nvx_wanc_split(nvx_wanc_bits(d), &md, &ed);
    int e = en - ed;
    if (mn < md) { mn <<= 1; e -= 1; }                      /* 1 <= mn / md < 2 */
    uint64_t q = 0, rem = mn;
    for (int i = 0; i < 55; i++) {                          /* 55 bits of the quotient, the first one set */
        q <<= 1;
        if (rem >= md) { rem -= md; q |= 1; }
        rem <<= 1;
    }
    int sticky = rem != 0;
    const int E = e + 1023;                                 /* the biased exponent, before rounding */
    if (E >= 2047) return nvx_wanc_from_bits(sign | 0x7ff0000000000000ull);
    if (E <= 0) {                                           /* subnormal: 1 - E more bits go */
        const int sh = 1 - E;
        if (sh > 56) { q = 0; sticky = 1; }
        else { sticky |= (q & ((1ull << sh) - 1)) != 0; q >>= sh; }
    }
    const uint64_t m = q >> 2;
    const int up = (q & 2) && ((q & 1) || sticky || (m & 1));
    const uint64_t bits = (E >= 1 ? ((uint64_t)(E - 1) << 52) : 0) + m + (uint64_t)up;     /* a carry moves into the exponent */
    return nvx_wanc_from_bits(sign | bits);
}

/* Steps 1 .. 7.  `ws`: rr, ri, qr, qi filled in by the caller (fp64 of the window's sums), the rest scratch.  `w`: K words of
 * w_re, then K of w_im, `wstride` apart.  Returns the reason; *coherence as the header says. */
NVX_WANC_HD int nvx_wanc_solve(int K, int window_log2, int load_log2, int64_t R0, int64_t TAA, double *ws, int stride, int32_t *w, int wstride,
                               int32_t *coherence)
{
#define WS(i) ws[(size_t)(i) * (size_t)stride]
    const int RR = 0, RI = K, QR = 2 * K, QI = 3 * K, D = 4 * K, E = 5 * K, XR = 6 * K, XI = 7 * K, LR = 8 * K, LI = 8 * K + K * (K - 1) / 2;
    *coherence = 0;
    for (int k = 0; k < 2 * K; k++) w[(size_t)k * wstride] = 0;
    if (R0 < ((int64_t)16 << (16 + window_log2))) return 1;
    const double diag = (double)(R0 + ((R0 >> load_log2) + 1));
    for (int j = 0; j < K; j++) {
        const int rj = j * (j - 1) / 2;
        double s = diag;
        for (int m = 0; m < j; m++) {
            const double lr = WS(LR + rj + m), li = WS(LI + rj + m);
            const double a = lr * lr, b = li * li, t = a + b, u = t * WS(D + m);
            s = s - u;
        }
        WS(D + j) = s;
        if (!(s > 0.0 && s < __builtin_inf())) return 2;
        const double e = nvx_wanc_div(1.0, s);
        WS(E + j) = e;
        for (int i = j + 1; i < K; i++) {
            const int ri = i * (i - 1) / 2;
            double sr = WS(RR + i - j), si = WS(RI + i - j);
            for (int m = 0; m < j; m++) {
                const double ar = WS(LR + ri + m), ai = WS(LI + ri + m), br = WS(LR + rj + m), bi = WS(LI + rj + m), dm = WS(D + m);
                const double p1 = ar * br, p2 = ai * bi, ur = p1 + p2;
                const double p3 = ai * br, p4 = ar * bi, ui = p3 - p4;
                const double t1 = ur * dm, t2 = ui * dm;
                sr = sr - t1; si = si - t2;
            }
            WS(LR + ri + j) = sr * e; WS(LI + ri + j) = si * e;
        }
    }
    for (int j = 0; j < K; j++) {                           /* L z = Q: z in xr, xi */
        const int rj = j * (j - 1) / 2;
        double zr = WS(QR + j), zi = WS(QI + j);
        for (int m = 0; m < j; m++) {
            const double lr = WS(LR + rj + m), li = WS(LI + rj + m), vr = WS(XR + m), vi = WS(XI + m);
            const double p1 = lr * vr, p2 = li * vi, ur = p1 - p2;
            const double p3 = lr * vi, p4 = li * vr, ui = p3 + p4;
            zr = zr - ur; zi = zi - ui;
        }
        WS(XR + j) = zr; WS(XI + j) = zi;
    }
    for (int j = 0; j < K; j++) { WS(XR + j) = WS(XR + j) * WS(E + j); WS(XI + j) = WS(XI + j) * WS(E + j); }
    for (int j = K - 1; j >= 0; j--) {                      /* L^H x = y, in place */
        double xr = WS(XR + j), xi = WS(XI + j);
        for (int i = j + 1; i < K; i++) {
            const int ri = i * (i - 1) / 2;
            const double lr = WS(LR + ri + j), li = WS(LI + ri + j), vr = WS(XR + i), vi = WS(XI + i);
            const double p1 = lr * vr, p2 = li * vi, ur = p1 + p2;
            const double p3 = lr * vi, p4 = li * vr, ui = p3 - p4;
            xr = xr - ur; xi = xi - ui;
        }
        WS(XR + j) = xr; WS(XI + j) = xi;
    }
    double c = 0.0;
    for (int k = 0; k < K; k++) {
        const double p1 = WS(XR + k) * WS(QR + k), p2 = WS(XI + k) * WS(QI + k), u = p1 + p2;
        c = c + u;
    }
    if (TAA > 0) {
        const double num = 16384.0 * c, v = nvx_wanc_div(num, (double)TAA);
        *coherence = !(v >= 1.0) ? 0 : (v >= 16384.0 ? 16384 : (int32_t)v);
    }
    int64_t l1 = 0;
    int bad = 0;
    for (int k = 0; k < 2 * K; k++) {
        const double v = __builtin_rint(8192.0 * WS(XR + k));       /* xi lies behind xr */
        if (!(v >= -32767.0 && v <= 32767.0)) { bad = 1; continue; }
        const int32_t iv = (int32_t)v;
        w[(size_t)k * wstride] = iv;
        l1 += iv < 0 ? -iv : iv;
    }
    if (bad || l1 > NVX_WANC_L1_MAX) {
        for (int k = 0; k < 2 * K; k++) w[(size_t)k * wstride] = 0;
        return 3;
    }
    return 0;
#undef WS
}

#endif
