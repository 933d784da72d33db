// The formulas of include/aefft.h that several host-check programs (tools/*_hostcheck.cpp) compare a kernel against, restated once in 64-bit
// integers: the floor division, the two taps and the weight of a LINEAR axis, the overlap of an AREA axis, the pixel rule without roundf, and the
// two resizes built from them (image -> frames, frames -> image) with the image side at any pitch and stride.
// For the checks only: nothing under autoencoder-fft_amd/ includes this header, and it shares nothing with the kernels, with resize_taps.h or
// with resize_tile.h.
#pragma once
#include <math.h>
#include <stddef.h>

#include <vector>

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

// aefft_image_resize_to_frames: B images of H rows of W interleaved pixels (row y of image b at img + b stride + y pitch) -> want [B][D][Nx][Ny] as
// the 8-bit pixel or, float frames, q (value = q * 2^-16).  mode 0 LINEAR, 1 AREA
static void image_to_frames_ref(const unsigned char* img, size_t pitch, size_t stride, int W, int H, int mode, bool f32, int B, int D, int Nx, int Ny,
                                std::vector<unsigned>& want)
{
    want.assign((size_t)B * D * Nx * Ny, 0);
    std::vector<std::vector<i64>> ox(Nx, std::vector<i64>(W, 0)), oy(Ny, std::vector<i64>(H, 0));
    if (mode == 1) {
        for (int i = 0; i < Nx; ++i) for (int k = 0; k < W; ++k) ox[i][k] = overlap(i, k, W, Nx);
        for (int j = 0; j < Ny; ++j) for (int k = 0; k < H; ++k) oy[j][k] = overlap(j, k, H, Ny);
    }
    for (int b = 0; b < B; ++b)
        for (int d = 0; d < D; ++d)
            for (int i = 0; i < Nx; ++i)
                for (int j = 0; j < Ny; ++j) {
                    const unsigned char* p = img + b * stride + d;
                    unsigned out;
                    if (mode == 0) {
                        int x0, x1, wx, y0, y1, wy;
                        linear_axis(i, W, Nx, &x0, &x1, &wx);
                        linear_axis(j, H, Ny, &y0, &y1, &wy);
                        const i64 v = (2048LL - wy) * ((2048LL - wx) * p[y0 * pitch + x0 * D] + (i64)wx * p[y0 * pitch + x1 * D]) +
                                      (i64)wy * ((2048LL - wx) * p[y1 * pitch + x0 * D] + (i64)wx * p[y1 * pitch + x1 * D]);
                        out = f32 ? (unsigned)((v + 32) >> 6) : (unsigned)((v + (1LL << 21)) >> 22);
                    } else {
                        i64 num = 0;
                        for (int y = 0; y < H; ++y) {
                            if (!oy[j][y]) continue;
                            i64 row = 0;
                            for (int x = 0; x < W; ++x)
                                if (ox[i][x]) row += ox[i][x] * p[y * pitch + x * D];
                            num += oy[j][y] * row;
                        }
                        const i64 wh = (i64)W * H;
                        out = f32 ? (unsigned)((65536 * num + wh / 2) / wh) : (unsigned)((2 * num + wh) / (2 * wh));
                    }
                    want[(((size_t)b * D + d) * Nx + i) * Ny + j] = out;
                }
}

// aefft_frames_resize_to_image: the frames' pixels px [B][D][Nx][Ny] -> the live bytes of B images of H rows of W interleaved pixels (row y of image
// b at img + b stride + y pitch; every other byte is left as it was): the same formulas with the roles swapped.  mode 0 LINEAR, 1 AREA
static void frames_to_image_ref(const unsigned char* px, int B, int D, int Nx, int Ny, int mode, int W, int H, unsigned char* img, size_t pitch, size_t stride)
{
    std::vector<std::vector<i64>> ox(W, std::vector<i64>(Nx, 0)), oy(H, std::vector<i64>(Ny, 0));
    if (mode == 1) {
        for (int i = 0; i < W; ++i) for (int k = 0; k < Nx; ++k) ox[i][k] = overlap(i, k, Nx, W);
        for (int j = 0; j < H; ++j) for (int k = 0; k < Ny; ++k) oy[j][k] = overlap(j, k, Ny, H);
    }
    for (int b = 0; b < B; ++b)
        for (int d = 0; d < D; ++d) {
            const unsigned char* p = px + ((size_t)b * D + d) * Nx * Ny;         // p[x * Ny + y]
            for (int j = 0; j < H; ++j)
                for (int i = 0; i < W; ++i) {
                    i64 out;
                    if (mode == 0) {
                        int x0, x1, wx, y0, y1, wy;
                        linear_axis(i, Nx, W, &x0, &x1, &wx);
                        linear_axis(j, Ny, H, &y0, &y1, &wy);
                        const i64 v = (2048LL - wy) * ((2048LL - wx) * p[(size_t)x0 * Ny + y0] + (i64)wx * p[(size_t)x1 * Ny + y0]) +
                                      (i64)wy * ((2048LL - wx) * p[(size_t)x0 * Ny + y1] + (i64)wx * p[(size_t)x1 * Ny + y1]);
                        out = (v + (1LL << 21)) >> 22;
                    } else {
                        i64 num = 0;
                        for (int x = 0; x < Nx; ++x) {
                            if (!ox[i][x]) continue;
                            i64 col = 0;
                            for (int y = 0; y < Ny; ++y)
                                if (oy[j][y]) col += oy[j][y] * p[(size_t)x * Ny + y];
                            num += ox[i][x] * col;
                        }
                        const i64 nn = (i64)Nx * Ny;
                        out = (2 * num + nn) / (2 * nn);
                    }
                    img[b * stride + j * pitch + (size_t)i * D + d] = (unsigned char)out;
                }
        }
}
