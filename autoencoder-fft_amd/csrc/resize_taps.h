// The per-axis taps of the integer resizes (include/aefft.h, AEFFT_RESIZE_LINEAR / AEFFT_RESIZE_AREA), stated ONCE for every kernel that resizes:
// resize_kernels.hip (image -> frames) and present_kernels.hip (frames -> image, map -> image).  Both filters are separable sums with taps of one
// form: destination index i reads source indices lo .. lo + cnt - 1 with weight wf on the first, wl on the last (cnt > 1) and N, the destination
// size, on those between:
//   LINEAR  lo = x0, cnt = 1 or 2, wf = 2048 - w, wl = w                       AREA  lo = floor(i S / N), the overlaps o(i, lo), N, .., N, o(i, hi)
// What the tile bodies do with the taps -- the sums over a staged band and the roundings -- is stated once as well, in resize_tile.h, which
// includes this header.
// Plain C++: the including file defines RZ_HD (the function qualifiers); tools/resize_hostcheck.cpp and tools/present_hostcheck.cpp compile this
// header for the host.
#pragma once

namespace aefft {

constexpr int RZ_LINEAR = 0, RZ_AREA = 1;        // == AEFFT_RESIZE_LINEAR / AEFFT_RESIZE_AREA
RZ_HD int rz_min(int a, int b) { return a < b ? a : b; }
RZ_HD int rz_max(int a, int b) { return a > b ? a : b; }

struct RzTap { int lo, cnt, wf, wl; };
// the taps of destination index i on an axis of S source and N destination samples (all products below 2^28: S, N <= 8192)
RZ_HD RzTap rz_tap(int mode, int i, int S, int N)
{
    RzTap t;
    if (mode == RZ_LINEAR) {
        const int n = (2 * i + 1) * S - N, den = 2 * N;
        int s = n >= 0 ? n / den : -((-n + den - 1) / den);                      // floor
        int w = (4096 * (n - s * den) + den) / (2 * den);                       // round(2048 r / den), halves up
        if (s < 0) { s = 0; w = 0; }
        if (s >= S - 1) { s = S - 1; w = 0; }
        t.lo = s; t.cnt = rz_min(s + 1, S - 1) - s + 1; t.wf = 2048 - w; t.wl = w;
    } else {
        const int a = i * S, b = a + S;                                          // the cell [i S, (i + 1) S) in units of 1 / N source pixels
        const int lo = a / N, hi = (b - 1) / N;
        t.lo = lo; t.cnt = hi - lo + 1; t.wf = rz_min(b, (lo + 1) * N) - a; t.wl = b - hi * N;
    }
    return t;
}
// weight of source index k for a tap (0 outside it); mid = the destination size of the axis
RZ_HD int rz_weight(const RzTap& t, int k, int mid)
{
    const int r = k - t.lo;
    if (r < 0 || r >= t.cnt) return 0;
    return r == 0 ? t.wf : (r == t.cnt - 1 ? t.wl : mid);
}

}  // namespace aefft
