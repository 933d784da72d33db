// The formulas of include/aefft.h that several host-check programs (tools/*_hostcheck.cpp) compare a kernel against, restated once in 64-bit
// integers: the floor division, the two taps and the weight of a LINEAR axis, the overlap of an AREA axis, and the pixel rule without roundf.
// For the checks only: nothing under autoencoder-fft_amd/ includes this header, and it shares nothing with the kernels or with resize_taps.h.
#pragma once
#include <math.h>

typedef long long i64;
static i64 fdiv(i64 a, i64 b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
// destination index i of N on a source axis of S: the taps s0, s1 and the weight w of s1 in 1/2048
static void linear_axis(int i, int S, int N, int* s0, int* s1, int* w)
{
    const i64 n = (2LL * i + 1) * S - N, den = 2LL * N;
    i64 s = fdiv(n, den), r = n - s * den, ww = (4096 * r + den) / (2 * den);
    if (s < 0) { s = 0; ww = 0; }
    if (s >= S - 1) { s = S - 1; ww = 0; }
    *s0 = (int)s; *s1 = (int)(s + 1 < S - 1 ? s + 1 : S - 1); *w = (int)ww;
}
// what destination cell i of N and source cell k of S share, in units of 1 / (S N) of the axis
static i64 overlap(int i, int k, int S, int N)
{
    const i64 hi = (i + 1LL) * S < (k + 1LL) * N ? (i + 1LL) * S : (k + 1LL) * N, lo = (i64)i * S > (i64)k * N ? (i64)i * S : (i64)k * N;
    return hi > lo ? hi - lo : 0;
}
// the reference's own rounding, without roundf: clamp, halves away from zero, NaN -> 0
static unsigned px_ref(float v)
{
    if (!(v > 0.f)) return 0;
    if (v >= 255.f) return 255;
    return (unsigned)floor((double)v + 0.5);
}
