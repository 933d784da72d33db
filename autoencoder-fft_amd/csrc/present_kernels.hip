// The way out of the net (gfx950): aefft_frames_resize_to_image and aefft_map_overlay_image -- the reference loop's SpinToImage_C + imshow
// (autoencoder.cpp:217-223) for frames of ANY size, and a per-tile heat map blended onto the camera image, one launch each.
//   frames_resize_kernel<D, F32, MODE>   frames [B][D][Nx][Ny] (8-bit, or float through px_u8) -> B images of H rows of W interleaved pixels;
//                                        MODE 0 LINEAR, 1 AREA: the taps of resize_taps.h with the roles swapped (source Nx, Ny; destination W, H)
//   map_overlay_kernel<D>                map [B][Mx][My] -> k0 = px_u8((m - lo) inv) -> LINEAR taps (or the pixel's tile) -> lut -> alpha blend, in place
// All-integer arithmetic behind px_u8 (include/aefft.h states the formulas): every route gives the same bytes as a numpy restatement.
// Both kernels share one tiling.  A workgroup (256 threads) owns a tile of TX destination columns x TY destination rows x
// all D channels of one image; TX is a multiple of 4, so a tile row starts on a dword of its image row whatever D is.  Full tiles are
// 64 / D (rounded down to 4) x 32 for frames_resize (rows of 64, 64, 60, 64 bytes) and up to 256 / D x 32 for map_overlay.  When an axis REDUCES by a ratio r the launcher divides that side of the
// tile by ceil(r) (at least 4 columns, 1 row): the source footprint of a tile stays about one full tile's, and a large reduction still has
// workgroups to spread over.  grid.x: the tiles of an image; grid.y x grid.z: the images.  Per tile:
//   1. TX + TY lanes write the tile's taps to LDS (rz_tap: the divisions, once per tile).
//   2. frames_resize: the source footprint -- for every source column x in [xs, xe) and channel d the run frames[b][d][x][ya .. ye) -- is staged
//      in LDS in FRAME order, as bytes, run n = (x - xb) D + d at dword n P (P odd): consecutive lanes load consecutive dwords of a run (float4
//      of float frames, px_u8 on the way in) when Ny % 4 == 0, single elements otherwise, then the next run.  In bands of XB source columns
//      when the footprint exceeds PR_BAND_WORDS, the lanes' sums running across the bands.
//      map_overlay: the map entries [xs, xe) x [ys, ye) are quantised to k0 bytes in LDS, and the colour table (256 D bytes) beside them.
//   3. frames_resize: a lane owns ONE byte column c = i D + d of the tile row (its column tap in registers) and up to 8 rows; a wave's 64 lanes
//      are the 64 byte columns of the same rows, so the rows' taps are the same in the whole wave.  For every source column of its tap the
//      lane forms, per row, the vertical sum over the run (consecutive LDS bytes) and adds it times the column's weight: 32-bit sums for LINEAR
//      (< 2^30), 64-bit for AREA.  Banks: the 32 lanes of an LDS lane group read, at ONE byte offset into their runs, the runs
//      n(c) = (lo(i) - xb) D + d for 32 consecutive c.  Run n lies on bank n P + const (mod 32), P odd: a bijection of n mod 32.  Enlarging or
//      same size (Nx <= W): lo(i + 1) - lo(i) is 0 or 1, so the lanes' n are within 32 consecutive values -- different banks, or the same
//      address (a broadcast).  Reducing by r: up to ceil(r) lanes per bank.
//      The finished bytes go to a tile image in LDS (row slot x 64 bytes, image order).
//      map_overlay: a lane owns one dword of an image row (one byte on the unaligned route): it loads it, blends its bytes and stores it.
//   4. frames_resize: the tile image leaves with the accesses that are contiguous on the image side: a lane per dword when image_d, pitch and
//      image_stride are multiples of 4 (the dword that crosses the row's end W D split into its live bytes), a lane per byte otherwise.
// No scratch, no atomics, no workspace.  The kernel bodies are plain C++ over (threadIdx, blockIdx, gridDim, __syncthreads) and an LDS pointer:
// tools/present_hostcheck.cpp compiles this file for the host, threads as lanes, under the sanitizers (AEFFT_HOSTCHECK: tools/hostlanes.h supplies
// those names and px_u8, and leaves the launchers out).
#include <type_traits>
#ifndef AEFFT_HOSTCHECK
#include "internal.h"
#include "fft_common.h"
#define RZ_HD __host__ __device__ __forceinline__
#define RZ_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)
#endif
#include "resize_taps.h"
#include "resize_tile.h"                         // fr_stage_runs, fr_band_sums, fr_round_tile: steps 2 and 3, shared with yuv_out_kernels.hip

namespace aefft {

// (the tile constants PR_TY, PR_CW, PR_NH, PR_RPL, pr_ceil_div and pr_div_u8: resize_tile.h)
constexpr int PR_BAND_WORDS = 8704;              // dwords of staged runs a workgroup holds (34 KiB: one column of D runs of 8192 + 3 bytes fits)
RZ_HD int pr_tx_full(int D) { return (PR_CW / D) & ~3; }   // destination columns of a full tile: 64, 32, 20, 16
// the tile for source sizes (Sx, Sy) -> destination sizes (W, H): a full tile (txf x tyf), each side divided by the axis' reduction ratio (rounded up)
RZ_HD void pr_tile(int txf, int tyf, int Sx, int Sy, int W, int H, int* TX, int* TY)
{
    *TX = rz_max(4, (txf / pr_ceil_div(Sx, W)) & ~3);
    *TY = rz_max(1, tyf / pr_ceil_div(Sy, H));
}
// map_overlay's full tile: rows of up to 256 bytes (at most 128 columns: TX + TY lanes compute the taps) x 32 rows, 8 dwords per lane -- it stages
// next to nothing per tile, so a larger tile only spreads the taps and the colour table over more pixels
constexpr int OV_TY = 32;
RZ_HD int ov_tx_full(int D) { return rz_min(128, 256 / D) & ~3; }   // 128, 128, 84, 64

// ---- frames -> image ------------------------------------------------------------------------------
struct FrArgs {
    const void* frames; unsigned char* image; size_t pitch, stride;
    int Nx, Ny, W, H;                            // source (frame) and destination (image) sizes
    int TX, TY, tx, ty, B;                       // the tile; tiles per image along x and y; images
    int P, XB;                                   // dwords of a staged run (odd); source columns of a band
    int ush;                                     // log2 of the lanes a run gets while staging: the least power of two that holds its dwords (or elements)
    bool img_words, frm_words;
};
// LDS of a launch, in dwords: the taps (TX + TY of 4), the finished tile in image order (PR_TY row slots of PR_CW bytes) and the band
RZ_HD int fr_lds_words(int D, const FrArgs& g) { return 4 * (g.TX + g.TY) + PR_CW / 4 * PR_TY + D * g.XB * g.P; }

template <int D, bool F32, int MODE>
__device__ __forceinline__ void frames_resize_body(const FrArgs& a, unsigned* lds)
{
    typedef typename std::conditional<MODE == RZ_AREA, unsigned long long, unsigned>::type acc_t;
    RzTap* xt = reinterpret_cast<RzTap*>(lds);
    RzTap* yt = xt + a.TX;
    unsigned* tile = lds + 4 * (a.TX + a.TY);
    unsigned char* tileb = reinterpret_cast<unsigned char*>(tile);
    unsigned* band = tile + PR_CW / 4 * PR_TY;
    const unsigned char* bandb = reinterpret_cast<const unsigned char*>(band);
    const int tid = (int)threadIdx.x;
    const int ty_i = (int)blockIdx.x / a.tx;
    const int i0 = ((int)blockIdx.x - ty_i * a.tx) * a.TX, j0 = ty_i * a.TY;
    const int ncols = rz_min(a.W - i0, a.TX), nrows = rz_min(a.H - j0, a.TY);
    if (tid < ncols) xt[tid] = rz_tap(MODE, i0 + tid, a.Nx, a.W);
    else if (tid >= a.TX && tid < a.TX + nrows) yt[tid - a.TX] = rz_tap(MODE, j0 + tid - a.TX, a.Ny, a.H);
    __syncthreads();
    // source columns [xs, xe) and rows [ys, ye) of the tile (the same in every lane); ya: the first staged row (a dword of the run on the dword route)
    const int xs = RZ_UNIFORM(xt[0].lo), xe = RZ_UNIFORM(xt[ncols - 1].lo + xt[ncols - 1].cnt);
    const int ys = RZ_UNIFORM(yt[0].lo), ye = RZ_UNIFORM(yt[nrows - 1].lo + yt[nrows - 1].cnt);
    const int ya = a.frm_words ? ys & ~3 : ys;
    const int nyb = ye - ya, nwy = (nyb + 3) >> 2;                               // (nwy <= P: the launcher sized P over every tile)
    const int rowlive = ncols * D, nw = (rowlive + 3) >> 2;                      // bytes and dwords of a tile row (at most 64 and 16)
    // the lane: byte column c = i D + d of the tile row (lanes run along c: ONE column tap per lane, in registers) x the rows h, h + 4, .., h + 28.
    // h is the same in a wave, so a row's taps are too: the loops over a run's rows are scalar loops.  The sums carry NO predicate that stays
    // the same from band to band (each would hold a pair of scalar registers across the whole loop nest): a lane beyond the row's live bytes
    // sums its last live column again, a row slot beyond the tile's rows sums the last row again, and a tap's last weight is 0 when it is
    // also its first.  Every lane writes its eight results to its own places of the finished tile -- row slot 8 h + k, column c -- and the
    // copy-out reads the live ones.
    const int c = tid % PR_CW, h = RZ_UNIFORM(tid / PR_CW);
    const int cc = rz_min(c, rowlive - 1), d = cc % D;
    const int nru = a.frm_words ? nwy : nyb;                                     // units of a staged run: dwords, or elements
    const RzTap X = xt[cc / D];
    // grid.y, grid.z: the images (a loop over them here would keep everything above in registers across the whole loop nest)
    const size_t b = (size_t)blockIdx.z * gridDim.y + blockIdx.y;
    if (b >= (size_t)a.B) return;
    {
        acc_t acc[PR_RPL];
#pragma unroll
        for (int k = 0; k < PR_RPL; ++k) acc[k] = 0;
        for (int xb = xs; xb < xe; xb += a.XB) {
            const int nxb = rz_min(a.XB, xe - xb);
            fr_stage_runs<D, F32>(tid, a.frames, b, a.Nx, a.Ny, xb, nxb, ya, nru, a.ush, a.frm_words, a.P, band);
            __syncthreads();
            fr_band_sums<D, MODE>(X, yt, bandb, a.P, d, h, nrows, xb, nxb, ya, a.W, a.H, acc);
            __syncthreads();
        }
        // the finished bytes to the tile in image order, then out with the accesses that are contiguous on the image side
        fr_round_tile<MODE>(acc, (unsigned long long)a.Nx * a.Ny, tileb, h, c);
        __syncthreads();
        unsigned char* img = a.image + b * a.stride + (size_t)j0 * a.pitch + (size_t)i0 * D;
        // a lane per dword of a row when image_d, pitch and image_stride are multiples of 4, per byte otherwise
        for (int idx = tid; idx < nrows * (a.img_words ? PR_CW / 4 : PR_CW); idx += 256) {
            const int r = a.img_words ? idx / (PR_CW / 4) : idx / PR_CW, u = a.img_words ? idx % (PR_CW / 4) : idx % PR_CW;
            const int slot = (r % PR_NH) * PR_RPL + r / PR_NH;                   // row r = 4 k + h lies in slot PR_RPL h + k
            if (u >= (a.img_words ? nw : rowlive)) continue;
            if (a.img_words) {
                const int n = rowlive - 4 * u;                                   // live bytes of the dword (>= 1)
                unsigned char* p = img + (size_t)r * a.pitch + 4 * u;
                const unsigned v = tile[PR_CW / 4 * slot + u];
                if (n >= 4) *reinterpret_cast<unsigned*>(p) = v;
                else
                    for (int e = 0; e < n; ++e) p[e] = (unsigned char)(v >> (8 * e));   // (the dword that crosses the row's end W D: its live bytes)
            } else img[(size_t)r * a.pitch + u] = tileb[PR_CW * slot + u];
        }
    }
}

// the launch geometry: the tile, the run's dwords P (the tallest tile's footprint, made odd) and the band's columns XB (the widest tile's footprint,
// or what PR_BAND_WORDS holds of it).  Exact, from the same rz_tap the kernel uses, over every tile's end taps.
static inline FrArgs fr_geometry(const void* frames, int Nx, int Ny, int mode, unsigned char* image, size_t pitch, size_t stride, int W, int H, int B, int D)
{
    FrArgs g;
    g.frames = frames; g.image = image; g.pitch = pitch; g.stride = B > 1 ? stride : 0;
    g.Nx = Nx; g.Ny = Ny; g.W = W; g.H = H; g.B = B;
    pr_tile(pr_tx_full(D), PR_TY, Nx, Ny, W, H, &g.TX, &g.TY);
    g.tx = pr_ceil_div(W, g.TX); g.ty = pr_ceil_div(H, g.TY);
    g.img_words = ((reinterpret_cast<uintptr_t>(image) | pitch | g.stride) & 3u) == 0;
    g.frm_words = (Ny & 3) == 0;
    int nx = 1, nyb = 1;
    for (int t = 0; t < g.tx; ++t) {
        const RzTap f = rz_tap(mode, t * g.TX, Nx, W), l = rz_tap(mode, rz_min(t * g.TX + g.TX, W) - 1, Nx, W);
        nx = rz_max(nx, l.lo + l.cnt - f.lo);
    }
    for (int t = 0; t < g.ty; ++t) {
        const RzTap f = rz_tap(mode, t * g.TY, Ny, H), l = rz_tap(mode, rz_min(t * g.TY + g.TY, H) - 1, Ny, H);
        nyb = rz_max(nyb, l.lo + l.cnt - (g.frm_words ? f.lo & ~3 : f.lo));
    }
    g.P = ((nyb + 3) >> 2) | 1;
    for (g.ush = 0; (1 << g.ush) < (g.frm_words ? (nyb + 3) >> 2 : nyb); ++g.ush) {}
    g.XB = rz_max(1, rz_min(nx, PR_BAND_WORDS / (D * g.P)));
    return g;
}

// ---- map -> image ---------------------------------------------------------------------------------
struct OvArgs {
    const float* map; const unsigned char* lut; unsigned char* image; size_t pitch, stride;
    int Mx, My, W, H;
    float lo, inv;                               // k0 = px_u8((m - lo) * inv)
    int smooth, alpha;
    int TX, TY, tx, ty, B;
    int NI, PJ;                                  // staged map columns at most; bytes of a staged map column
    bool img_words;
};
// the taps of image index i on a map axis of S entries: LINEAR's, or the tile the pixel lies in with the whole weight (v = k0 << 22: k = k0)
RZ_HD RzTap ov_tap(int smooth, int i, int S, int N)
{
    if (smooth) return rz_tap(RZ_LINEAR, i, S, N);
    RzTap t;
    t.lo = i * S / N; t.cnt = 1; t.wf = 2048; t.wl = 0;                          // (i S < 2^23)
    return t;
}
// LDS of a launch, in dwords: the taps, the colour table, the k0 bytes
RZ_HD int ov_lds_words(int D, const OvArgs& g) { return 4 * (g.TX + g.TY) + 64 * D + ((g.NI * g.PJ + 3) >> 2); }

template <int D>
__device__ __forceinline__ void map_overlay_body(const OvArgs& a, unsigned* lds)
{
    RzTap* xt = reinterpret_cast<RzTap*>(lds);
    RzTap* yt = xt + a.TX;
    unsigned char* lut = reinterpret_cast<unsigned char*>(lds + 4 * (a.TX + a.TY));
    unsigned char* kq = lut + 256 * D;
    const int tid = (int)threadIdx.x;
    const int ty_i = (int)blockIdx.x / a.tx;
    const int i0 = ((int)blockIdx.x - ty_i * a.tx) * a.TX, j0 = ty_i * a.TY;
    const int ncols = rz_min(a.W - i0, a.TX), nrows = rz_min(a.H - j0, a.TY);
    if (tid < ncols) xt[tid] = ov_tap(a.smooth, i0 + tid, a.Mx, a.W);
    else if (tid >= a.TX && tid < a.TX + nrows) yt[tid - a.TX] = ov_tap(a.smooth, j0 + tid - a.TX, a.My, a.H);
    for (int idx = tid; idx < 256 * D; idx += 256) lut[idx] = a.lut[idx];
    __syncthreads();
    const int xs = RZ_UNIFORM(xt[0].lo), xe = RZ_UNIFORM(xt[ncols - 1].lo + xt[ncols - 1].cnt);
    const int ys = RZ_UNIFORM(yt[0].lo), ye = RZ_UNIFORM(yt[nrows - 1].lo + yt[nrows - 1].cnt);
    const int nys = ye - ys;                                                     // (<= PJ, and xe - xs <= NI: the launcher sized them over every tile)
    const int rowlive = ncols * D;
    const int unit = a.img_words ? 4 : 1, nu = (rowlive + unit - 1) / unit;      // a lane's bytes of a row; lanes of a row
    const int ush = a.img_words ? 6 : 8;                                         // a row's lanes are counted off in 64 dwords / 256 bytes: no division
    const size_t b = (size_t)blockIdx.z * gridDim.y + blockIdx.y;               // grid.y, grid.z: the images
    if (b >= (size_t)a.B) return;
    {
        for (int idx = tid; idx < (xe - xs) * nys; idx += 256) {
            const int I = idx / nys, J = idx - I * nys;
            const float m = a.map[(b * a.Mx + xs + I) * (size_t)a.My + ys + J];
            const float t = m - a.lo;                                            // (each operation rounds on its own: nothing here can contract)
            kq[I * a.PJ + J] = (unsigned char)px_u8(t * a.inv);
        }
        __syncthreads();
        for (int item = tid; item < (nrows << ush); item += 256) {
            const int r = item >> ush, u = item & ((1 << ush) - 1), c0 = u * unit, n = rz_min(unit, rowlive - c0);
            if (u >= nu) continue;
            unsigned char* p = a.image + b * a.stride + (size_t)(j0 + r) * a.pitch + (size_t)i0 * D + c0;
            unsigned v = 0;
            if (n >= 4) v = *reinterpret_cast<const unsigned*>(p);
            else
                for (int e = 0; e < n; ++e) v |= (unsigned)p[e] << (8 * e);      // (a single byte, or the dword that crosses the row's end: its live bytes only)
            const RzTap Y = yt[r];
            unsigned out = 0, k = 0;
            for (int e = 0; e < n; ++e) {
                const int c = c0 + e, i = c / D, d = c - i * D;
                if (e == 0 || d == 0) {                                          // a new pixel: its table index
                    const RzTap X = xt[i];
                    const unsigned char* q = kq + (X.lo - xs) * a.PJ + (Y.lo - ys);
                    unsigned t0 = (unsigned)Y.wf * q[0], t1 = 0;
                    if (Y.cnt > 1) t0 += (unsigned)Y.wl * q[1];
                    if (X.cnt > 1) {
                        t1 = (unsigned)Y.wf * q[a.PJ];
                        if (Y.cnt > 1) t1 += (unsigned)Y.wl * q[a.PJ + 1];
                    }
                    k = ((unsigned)X.wf * t0 + (unsigned)X.wl * t1 + (1u << 21)) >> 22;
                }
                const unsigned old = (v >> (8 * e)) & 255u;
                out |= (((unsigned)a.alpha * lut[k * D + d] + (unsigned)(256 - a.alpha) * old + 128u) >> 8) << (8 * e);
            }
            if (n >= 4) *reinterpret_cast<unsigned*>(p) = out;
            else
                for (int e = 0; e < n; ++e) p[e] = (unsigned char)(out >> (8 * e));
        }
    }
}

static inline OvArgs ov_geometry(const float* map, int Mx, int My, float lo, float inv, int smooth, const unsigned char* lut, int alpha,
                                 unsigned char* image, size_t pitch, size_t stride, int W, int H, int B, int D)
{
    OvArgs g;
    g.map = map; g.lut = lut; g.image = image; g.pitch = pitch; g.stride = B > 1 ? stride : 0;
    g.Mx = Mx; g.My = My; g.W = W; g.H = H; g.lo = lo; g.inv = inv; g.smooth = smooth ? 1 : 0; g.alpha = alpha; g.B = B;
    pr_tile(ov_tx_full(D), OV_TY, Mx, My, W, H, &g.TX, &g.TY);
    g.tx = pr_ceil_div(W, g.TX); g.ty = pr_ceil_div(H, g.TY);
    g.img_words = ((reinterpret_cast<uintptr_t>(image) | pitch | g.stride) & 3u) == 0;
    g.NI = 1; g.PJ = 1;
    for (int t = 0; t < g.tx; ++t) {
        const RzTap f = ov_tap(g.smooth, t * g.TX, Mx, W), l = ov_tap(g.smooth, rz_min(t * g.TX + g.TX, W) - 1, Mx, W);
        g.NI = rz_max(g.NI, l.lo + l.cnt - f.lo);
    }
    for (int t = 0; t < g.ty; ++t) {
        const RzTap f = ov_tap(g.smooth, t * g.TY, My, H), l = ov_tap(g.smooth, rz_min(t * g.TY + g.TY, H) - 1, My, H);
        g.PJ = rz_max(g.PJ, l.lo + l.cnt - f.lo);
    }
    return g;
}

#ifndef AEFFT_HOSTCHECK
template <int D, bool F32, int MODE>
__global__ __launch_bounds__(256) void frames_resize_kernel(const FrArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned pr_lds[];
    frames_resize_body<D, F32, MODE>(a, pr_lds);
}

template <int D>
__global__ __launch_bounds__(256) void map_overlay_kernel(const OvArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned pr_lds[];
    map_overlay_body<D>(a, pr_lds);
}

// grid.x: the tiles of an image (at most 2^22); grid.y x grid.z: the images, image b = z grid.y + y (workgroups beyond B return at once)
static dim3 pr_grid(int tx, int ty, int B)
{
    const unsigned by = (unsigned)B < 65535u ? (unsigned)B : 65535u;
    return dim3((unsigned)tx * (unsigned)ty, by, ((unsigned)B + by - 1) / by);
}
static bool pr_image_ok(const void* image, size_t pitch, int W, int H, int B, int D)
{
    const auto in = [](int v) { return v >= 1 && v <= 8192; };
    return image && B >= 1 && D >= 1 && D <= 4 && in(W) && in(H) && pitch >= (size_t)W * D;
}

hipError_t launch_frames_resize(const void* frames, bool f32, int Nx, int Ny, int mode, unsigned char* image, size_t pitch, size_t stride,
                                int W, int H, int B, int D, hipStream_t st)
{
    if (!frames || !pr_image_ok(image, pitch, W, H, B, D) || Nx < 1 || Nx > 8192 || Ny < 1 || Ny > 8192) return hipErrorInvalidValue;
    if (mode != RZ_LINEAR && mode != RZ_AREA) return hipErrorInvalidValue;
    if (mode == RZ_AREA && (W > Nx || H > Ny)) return hipErrorInvalidValue;
    const FrArgs g = fr_geometry(frames, Nx, Ny, mode, image, pitch, stride, W, H, B, D);
    const dim3 gr = pr_grid(g.tx, g.ty, B), bl(256);
    const size_t lds = 4 * (size_t)fr_lds_words(D, g);
    if (lds > 65536) return hipErrorInvalidValue;                                // (cannot happen: at most 37 KiB by PR_BAND_WORDS)
#define FR_CASE(DD, FF, MM) case ((DD) * 4 + (FF) * 2 + (MM)): frames_resize_kernel<DD, FF != 0, MM><<<gr, bl, lds, st>>>(g); break;
#define FR_CASES(DD) FR_CASE(DD, 0, 0) FR_CASE(DD, 0, 1) FR_CASE(DD, 1, 0) FR_CASE(DD, 1, 1)
    switch (D * 4 + (f32 ? 2 : 0) + mode) {
        FR_CASES(1) FR_CASES(2) FR_CASES(3) FR_CASES(4)
        default: return hipErrorInvalidValue;
    }
#undef FR_CASES
#undef FR_CASE
    return hipGetLastError();
}

hipError_t launch_map_overlay(const float* map, int Mx, int My, float lo, float inv, int smooth, const unsigned char* lut, int alpha,
                              unsigned char* image, size_t pitch, size_t stride, int W, int H, int B, int D, hipStream_t st)
{
    if (!map || !lut || !pr_image_ok(image, pitch, W, H, B, D) || Mx < 1 || Mx > 1024 || My < 1 || My > 1024 || alpha < 0 || alpha > 256) return hipErrorInvalidValue;
    const OvArgs g = ov_geometry(map, Mx, My, lo, inv, smooth, lut, alpha, image, pitch, stride, W, H, B, D);
    const dim3 gr = pr_grid(g.tx, g.ty, B), bl(256);
    const size_t lds = 4 * (size_t)ov_lds_words(D, g);
    if (lds > 65536) return hipErrorInvalidValue;                                // (cannot happen: at most 1026 x 34 k0 bytes, the table and the taps)
    switch (D) {
        case 1: map_overlay_kernel<1><<<gr, bl, lds, st>>>(g); break;
        case 2: map_overlay_kernel<2><<<gr, bl, lds, st>>>(g); break;
        case 3: map_overlay_kernel<3><<<gr, bl, lds, st>>>(g); break;
        default: map_overlay_kernel<4><<<gr, bl, lds, st>>>(g); break;
    }
    return hipGetLastError();
}
#endif

}  // namespace aefft
