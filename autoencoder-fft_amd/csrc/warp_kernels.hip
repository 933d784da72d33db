// Geometric alignment of interleaved 8-bit images (aefft_image_warp_affine, aefft_image_remap, gfx950; include/aefft.h has the definition, DESIGN.md
// section 30 the route and the measurement).  Both calls reduce to a pair (tx, ty) of signed 32-bit integers for every destination pixel, the source
// position times 2048; from there on they are one sampler: the taps of the interpolation, the border rule on each tap and axis, the resize's weights
// and rounding.
//   warp_affine_kernel<D>   (tx, ty) from an affine in Q24, one for the batch or one for each image.  The image index and with it the affine are the
//                           same in every lane of a workgroup: the six coefficients are loaded once an image.  U and V are exact 64-bit integers,
//                           so a lane forms them at its first pixel and adds a[0] and a[3] from pixel to pixel: increments are the definition.
//   warp_remap_kernel<D>    (tx, ty) from the table int [Hd][Wd][2], which the batch shares: a workgroup keeps the taps, the weights and the
//                           verdicts of the border rule of its pixels in registers and walks the images with them, so the 8 bytes a pixel of table
//                           are read once for its share of the batch, not once an image.
//   work     a workgroup of 256 lanes owns a tile of 32 x 32 destination pixels -- compact in both directions, so that under a rotation the taps
//            of neighbouring lanes still meet in the same cache lines --, a lane four neighbouring pixels of a row (WP_PX): the 4 D bytes from
//            column x0 = 4 k on are D whole dwords of the row whatever D is.  Workgroup (tile, c) takes the images c, c + gridDim.y, ...
//   taps     gathers through the vector cache: every index has passed wp_index, so whatever the table or the coefficients hold, no byte outside
//            the B source images is read; a CONSTANT tap outside the image is not loaded at all.  The two taps of a source row are neighbouring
//            pixels, 2 D <= 8 contiguous bytes: where 8 bytes from the first tap on are live bytes of the row, ONE load of 8 bytes at any
//            alignment brings both (NEAREST: one of 4 bytes), single bytes at the borders and the row's end -- 2 loads a pixel instead of 4 D.
//   stores   pointer, pitch and stride multiples of 4: the lane's D dwords (the four pixels that cross the row's end Wd: the live bytes one by one);
//            bytes otherwise.  The same bytes on either route.  Bytes beyond Wd D of a row are never written.
// No LDS, no atomics, no barrier: every destination byte is a function of the arguments alone.
// tools/warp_hostcheck.cpp compiles this file for the host (AEFFT_HOSTCHECK: tools/hostlanes.h supplies the launch variables and WP_HD).
#ifndef AEFFT_HOSTCHECK
#include "internal.h"
#define WP_HD __device__ __forceinline__
#endif

namespace aefft {

constexpr int WP_NEAREST = 0, WP_LINEAR = 1;                                     // AEFFT_WARP_NEAREST, AEFFT_WARP_LINEAR
constexpr int WP_CONSTANT = 0, WP_REPLICATE = 1, WP_REFLECT = 2;                 // AEFFT_BORDER_CONSTANT, _REPLICATE, _REFLECT
constexpr int WP_LANES = 256;
constexpr int WP_PX = 4;                                                         // pixels of a lane, neighbours in a row
constexpr int WP_TX = 32, WP_TY = 32;                                            // the tile: WP_TX / WP_PX lanes along a row x WP_TY rows
constexpr int WP_SIZE = 8192;                                                    // the largest side of an image
constexpr int WP_REMAP_GROUPS = 2048;                                            // workgroups a remap launch aims at: the batch is split until the tiles reach it
constexpr unsigned WP_GRID_Y = 65535;
static_assert(WP_TX / WP_PX * WP_TY == WP_LANES, "a lane owns WP_PX pixels of the tile");

typedef long long wp_i64;
typedef unsigned long long wp_u64;

struct WpAffine { wp_i64 a[6]; };                                                // aefft_affine: Q24, 48 bytes

struct WpArgs {
    const unsigned char* src; size_t spitch, sstride;                            // B images each (the strides are 0 for B == 1)
    unsigned char* dst; size_t dpitch, dstride;
    const WpAffine* m;                                                           // affine: nm of them
    const int* map;                                                              // remap: [Hd][Wd][2], x first
    int Ws, Hs, Wd, Hd, B, nm;
    int interp, border;
    unsigned bval;                                                               // CONSTANT: channel d's byte at bits 8 d
    int tiles_x;                                                                 // tiles along a destination row
    int dst_words;                                                               // dst, dpitch and dstride are multiples of 4
};

// the border rule on one tap and one axis: the index the tap reads, in 0 .. S-1 whatever s is; `live` is false for a CONSTANT tap outside the image
WP_HD int wp_index(int s, int S, int border, bool* live)
{
    *live = true;
    if ((unsigned)s < (unsigned)S) return s;
    if (border == WP_REFLECT) {
        if (S == 1) return 0;
        const int P = 2 * (S - 1);
        int r = s % P;                                                           // (|s| <= 2^20 + 1)
        r = r < 0 ? r + P : r;
        return r < S ? r : P - r;
    }
    *live = border != WP_CONSTANT;
    return s < 0 ? 0 : S - 1;
}

// a pixel's taps: the byte offsets of the two rows and the two columns inside a source image, the weights and the border rule's four verdicts
struct WpTaps {
    size_t r0, r1;                                                               // sy pitch, (sy + 1) pitch after the border rule
    int c0, c1;                                                                  // sx D, (sx + 1) D after the border rule
    unsigned w;                                                                  // wx | wy << 12 | live x0, x1, y0, y1 at bits 24..27 | WP_PAIR | WP_QUAD
};
constexpr unsigned WP_X0 = 1u << 24, WP_X1 = 1u << 25, WP_Y0 = 1u << 26, WP_Y1 = 1u << 27;
constexpr unsigned WP_PAIR = 1u << 28, WP_QUAD = 1u << 29;                           // 8 (LINEAR: both taps of a row) / 4 (NEAREST) live bytes of the row from c0 on

WP_HD WpTaps wp_taps(int tx, int ty, const WpArgs& g, int D)
{
    int sx, sy;
    unsigned wx = 0, wy = 0;
    if (g.interp == WP_NEAREST) {
        sx = (int)(((wp_i64)tx + 1024) >> 11);                                   // halves up; 64 bits: tx + 1024 may pass 2^31
        sy = (int)(((wp_i64)ty + 1024) >> 11);
    } else {
        sx = tx >> 11; wx = (unsigned)tx & 2047u;
        sy = ty >> 11; wy = (unsigned)ty & 2047u;
    }
    bool x0, x1, y0, y1;
    const int ix0 = wp_index(sx, g.Ws, g.border, &x0), ix1 = wp_index(sx + 1, g.Ws, g.border, &x1);
    const int iy0 = wp_index(sy, g.Hs, g.border, &y0), iy1 = wp_index(sy + 1, g.Hs, g.border, &y1);
    WpTaps t;
    t.r0 = (size_t)iy0 * g.spitch; t.r1 = (size_t)iy1 * g.spitch;
    t.c0 = ix0 * D; t.c1 = ix1 * D;
    t.w = wx | wy << 12 | (x0 ? WP_X0 : 0u) | (x1 ? WP_X1 : 0u) | (y0 ? WP_Y0 : 0u) | (y1 ? WP_Y1 : 0u);
    const int rowbytes = g.Ws * D;                                               // (bytes of a row beyond Ws D are never read)
    if (x0 && x1 && ix1 == ix0 + 1 && t.c0 + 8 <= rowbytes) t.w |= WP_PAIR;
    if (x0 && t.c0 + 4 <= rowbytes) t.w |= WP_QUAD;
    return t;
}

// one tap of channel d: the source byte, or the constant where the border rule says so (then nothing is loaded)
WP_HD unsigned wp_tap(const unsigned char* row, int c, int d, bool live, unsigned bval)
{
    return live ? (unsigned)row[(size_t)(c + d)] : (bval >> (8 * d)) & 255u;
}

// the two taps of one source row, all channels.  WP_PAIR: the taps are neighbours inside the row and 8 bytes from the first one on are live bytes
// of the row, so one load of 8 bytes at any alignment (a copy of 8 bytes: the back end picks the instruction) holds both pixels; single bytes
// otherwise, which is the route at the borders and at a row's last pixels
template <int D> WP_HD void wp_two(const unsigned char* row, const WpTaps& t, bool ylive, unsigned bval, unsigned (&p0)[D], unsigned (&p1)[D])
{
    if (ylive && (t.w & WP_PAIR)) {
        wp_u64 v;
        __builtin_memcpy(&v, row + t.c0, 8);
#pragma unroll
        for (int d = 0; d < D; ++d) { p0[d] = (unsigned)(v >> (8 * d)) & 255u; p1[d] = (unsigned)(v >> (8 * (D + d))) & 255u; }
        return;
    }
#pragma unroll
    for (int d = 0; d < D; ++d) {
        p0[d] = wp_tap(row, t.c0, d, ylive && (t.w & WP_X0), bval);
        p1[d] = wp_tap(row, t.c1, d, ylive && (t.w & WP_X1), bval);
    }
}

// the pixel's D bytes into the lane's dwords: byte n = k D + d of the lane at bits 8 (n & 3) of word n >> 2
template <int D> WP_HD void wp_pixel(const unsigned char* img, const WpTaps& t, const WpArgs& g, int k, unsigned (&word)[D])
{
    unsigned v[D];
    if (g.interp == WP_NEAREST) {
        const bool live = (t.w & WP_X0) && (t.w & WP_Y0);
        if (live && (t.w & WP_QUAD)) {                                            // (4 live bytes of the row from the tap on: one load)
            unsigned q;
            __builtin_memcpy(&q, img + t.r0 + t.c0, 4);
#pragma unroll
            for (int d = 0; d < D; ++d) v[d] = (q >> (8 * d)) & 255u;
        } else {
#pragma unroll
            for (int d = 0; d < D; ++d) v[d] = wp_tap(img + t.r0, t.c0, d, live, g.bval);
        }
    } else {
        unsigned p00[D], p01[D], p10[D], p11[D];
        wp_two<D>(img + t.r0, t, t.w & WP_Y0, g.bval, p00, p01);
        wp_two<D>(img + t.r1, t, t.w & WP_Y1, g.bval, p10, p11);
        const unsigned wx = t.w & 2047u, wy = (t.w >> 12) & 2047u;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const unsigned acc = (2048u - wy) * ((2048u - wx) * p00[d] + wx * p01[d]) + wy * ((2048u - wx) * p10[d] + wx * p11[d]);   // < 2^30
            v[d] = (acc + (1u << 21)) >> 22;
        }
    }
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const int n = k * D + d;
        word[n >> 2] |= v[d] << (8 * (n & 3));
    }
}

// the lane's `live` (1..4) pixels leave: row points at the first one's first byte
template <int D> WP_HD void wp_store(unsigned char* row, const unsigned (&word)[D], int live, int words)
{
    if (words && live == WP_PX) {
#pragma unroll
        for (int i = 0; i < D; ++i) reinterpret_cast<unsigned*>(row)[i] = word[i];
        return;
    }
#pragma unroll
    for (int n = 0; n < WP_PX * D; ++n)
        if (n < live * D) row[n] = (unsigned char)(word[n >> 2] >> (8 * (n & 3)));
}

// the lane's place: its row y, its first column x0 and its live pixels (0: the lane has nothing to do)
WP_HD int wp_place(const WpArgs& g, unsigned tile, unsigned lane, int* x0, int* y)
{
    const int tx = (int)(tile % (unsigned)g.tiles_x), ty = (int)(tile / (unsigned)g.tiles_x);
    *x0 = tx * WP_TX + (int)(lane % (WP_TX / WP_PX)) * WP_PX;
    *y = ty * WP_TY + (int)(lane / (WP_TX / WP_PX));
    if (*y >= g.Hd || *x0 >= g.Wd) return 0;
    const int left = g.Wd - *x0;
    return left < WP_PX ? left : WP_PX;
}

// tx of the definition out of U: clamp((U + 2^12) >> 13) with U wrapping in 64 bits
WP_HD int wp_q11(wp_u64 U)
{
    const wp_i64 t = (wp_i64)(U + 4096ull) >> 13;
    return t < -2147483647LL - 1 ? (int)(-2147483647LL - 1) : t > 2147483647LL ? 2147483647 : (int)t;
}

template <int D> WP_HD void warp_affine_body(const WpArgs& g, unsigned tile, unsigned first, unsigned step, unsigned lane)
{
    int x0, y;
    const int live = wp_place(g, tile, lane, &x0, &y);
    if (!live) return;
    for (unsigned b = first; b < (unsigned)g.B; b += step) {
        const WpAffine& m = g.m[g.nm == 1 ? 0u : b];                              // (the same in every lane)
        const wp_u64 a0 = (wp_u64)m.a[0], a3 = (wp_u64)m.a[3];
        wp_u64 U = a0 * (wp_u64)x0 + (wp_u64)m.a[1] * (wp_u64)y + (wp_u64)m.a[2];
        wp_u64 V = a3 * (wp_u64)x0 + (wp_u64)m.a[4] * (wp_u64)y + (wp_u64)m.a[5];
        const unsigned char* img = g.src + (size_t)b * g.sstride;
        unsigned word[D];
#pragma unroll
        for (int i = 0; i < D; ++i) word[i] = 0;
#pragma unroll
        for (int k = 0; k < WP_PX; ++k) {
            if (k < live) wp_pixel<D>(img, wp_taps(wp_q11(U), wp_q11(V), g, D), g, k, word);
            U += a0; V += a3;
        }
        wp_store<D>(g.dst + (size_t)b * g.dstride + (size_t)y * g.dpitch + (size_t)x0 * D, word, live, g.dst_words);
    }
}

template <int D> WP_HD void warp_remap_body(const WpArgs& g, unsigned tile, unsigned first, unsigned step, unsigned lane)
{
    int x0, y;
    const int live = wp_place(g, tile, lane, &x0, &y);
    if (!live) return;
    WpTaps t[WP_PX];
    const int* e = g.map + ((size_t)y * g.Wd + x0) * 2;
#pragma unroll
    for (int k = 0; k < WP_PX; ++k) {
        const bool in = k < live;                                                 // (past the row's end: nothing of the table is read)
        t[k] = wp_taps(in ? e[2 * k] : 0, in ? e[2 * k + 1] : 0, g, D);
    }
    for (unsigned b = first; b < (unsigned)g.B; b += step) {
        const unsigned char* img = g.src + (size_t)b * g.sstride;
        unsigned word[D];
#pragma unroll
        for (int i = 0; i < D; ++i) word[i] = 0;
#pragma unroll
        for (int k = 0; k < WP_PX; ++k)
            if (k < live) wp_pixel<D>(img, t[k], g, k, word);
        wp_store<D>(g.dst + (size_t)b * g.dstride + (size_t)y * g.dpitch + (size_t)x0 * D, word, live, g.dst_words);
    }
}

// what both launchers take; false for what the kernels do not serve.  grid->x: the tiles; the caller sets grid->y
static inline bool wp_geometry(const unsigned char* src, size_t spitch, size_t sstride, int Ws, int Hs, int interp, int border, unsigned bval, unsigned char* dst,
                               size_t dpitch, size_t dstride, int Wd, int Hd, int B, int D, WpArgs* g, unsigned* tiles)
{
    const auto side = [](int v) { return v >= 1 && v <= WP_SIZE; };
    if (!src || !dst || !side(Ws) || !side(Hs) || !side(Wd) || !side(Hd) || B < 1 || D < 1 || D > 4 || (interp != WP_NEAREST && interp != WP_LINEAR) ||
        border < WP_CONSTANT || border > WP_REFLECT || spitch < (size_t)Ws * D || dpitch < (size_t)Wd * D)
        return false;
    *g = WpArgs();
    g->src = src; g->spitch = spitch; g->sstride = B > 1 ? sstride : 0; g->Ws = Ws; g->Hs = Hs;
    g->dst = dst; g->dpitch = dpitch; g->dstride = B > 1 ? dstride : 0; g->Wd = Wd; g->Hd = Hd;
    g->B = B; g->interp = interp; g->border = border; g->bval = bval;
    g->tiles_x = (Wd + WP_TX - 1) / WP_TX;
    g->dst_words = ((reinterpret_cast<uintptr_t>(dst) | dpitch | g->dstride) & 3u) == 0;
    *tiles = (unsigned)g->tiles_x * (unsigned)((Hd + WP_TY - 1) / WP_TY);         // (at most 256 x 256)
    return true;
}
// the images a remap workgroup walks are every wp_remap_split-th: the batch is split until the launch has WP_REMAP_GROUPS workgroups
static inline unsigned wp_remap_split(unsigned tiles, int B)
{
    const unsigned want = (WP_REMAP_GROUPS + tiles - 1) / tiles;
    return want < (unsigned)B ? want : (unsigned)B;
}

#ifndef AEFFT_HOSTCHECK
template <int D> __global__ __launch_bounds__(WP_LANES) void warp_affine_kernel(const WpArgs g) { warp_affine_body<D>(g, blockIdx.x, blockIdx.y, gridDim.y, threadIdx.x); }
template <int D> __global__ __launch_bounds__(WP_LANES) void warp_remap_kernel(const WpArgs g) { warp_remap_body<D>(g, blockIdx.x, blockIdx.y, gridDim.y, threadIdx.x); }

static_assert(sizeof(WpAffine) == sizeof(aefft_affine) && sizeof(WpAffine) == 48, "aefft_affine is six Q24 coefficients of 64 bits");

hipError_t launch_image_warp_affine(const unsigned char* src, size_t spitch, size_t sstride, int Ws, int Hs, const aefft_affine* m, int nm, int interp, int border,
                                    unsigned bval, unsigned char* dst, size_t dpitch, size_t dstride, int Wd, int Hd, int B, int D, hipStream_t st)
{
    WpArgs g;
    unsigned tiles = 0;
    if (!m || (nm != 1 && nm != B) || !wp_geometry(src, spitch, sstride, Ws, Hs, interp, border, bval, dst, dpitch, dstride, Wd, Hd, B, D, &g, &tiles))
        return hipErrorInvalidValue;
    g.m = reinterpret_cast<const WpAffine*>(m); g.nm = nm;
    const dim3 grid(tiles, (unsigned)B < WP_GRID_Y ? (unsigned)B : WP_GRID_Y), block(WP_LANES);
    switch (D) {
        case 1: warp_affine_kernel<1><<<grid, block, 0, st>>>(g); break;
        case 2: warp_affine_kernel<2><<<grid, block, 0, st>>>(g); break;
        case 3: warp_affine_kernel<3><<<grid, block, 0, st>>>(g); break;
        default: warp_affine_kernel<4><<<grid, block, 0, st>>>(g); break;
    }
    return hipGetLastError();
}

hipError_t launch_image_remap(const unsigned char* src, size_t spitch, size_t sstride, int Ws, int Hs, const int* map, int interp, int border, unsigned bval,
                              unsigned char* dst, size_t dpitch, size_t dstride, int Wd, int Hd, int B, int D, hipStream_t st)
{
    WpArgs g;
    unsigned tiles = 0;
    if (!map || !wp_geometry(src, spitch, sstride, Ws, Hs, interp, border, bval, dst, dpitch, dstride, Wd, Hd, B, D, &g, &tiles)) return hipErrorInvalidValue;
    g.map = map;
    const dim3 grid(tiles, wp_remap_split(tiles, B)), block(WP_LANES);
    switch (D) {
        case 1: warp_remap_kernel<1><<<grid, block, 0, st>>>(g); break;
        case 2: warp_remap_kernel<2><<<grid, block, 0, st>>>(g); break;
        case 3: warp_remap_kernel<3><<<grid, block, 0, st>>>(g); break;
        default: warp_remap_kernel<4><<<grid, block, 0, st>>>(g); break;
    }
    return hipGetLastError();
}
#endif

}  // namespace aefft
