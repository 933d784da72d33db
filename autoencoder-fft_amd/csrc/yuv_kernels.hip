// aefft_yuv_to_image and aefft_yuv_resize_to_frames (gfx950): NV12, I420 and YUYV video -- what a hardware decoder, a software decoder and a V4L2
// webcam deliver -- to interleaved 8-bit images and, fused with the resize + ImageToSpin_C of resize_kernels.hip, to the planar frames every 8-bit
// net call takes, one launch each.  All-integer (include/aefft.h states table and formula): with c = Y - yoff, u = U - 128, v = V - 128
//   p[y][x][d] = clamp((ky c + a_d u + b_d v + 2^19) >> 20, 0, 255),      chroma of pixel (x, y) = the sample at (x >> 1, y >> 1)  (YUYV: (x >> 1, y))
// The D coefficient rows (a_d, b_d) come in as arguments in the order the channels are stored: matrix and channel order are data, not
// instantiations.  D = 3 (BGR, RGB) or D = 1 (GRAY: no chroma byte is loaded from a chroma plane).
//   yuv_resize_kernel<FMT, D, F32, MODE>   the tile body of resize_kernel with another staging phase: a lane takes an ITEM -- 4 pixels of a luma
//                                          row pair (NV12, I420: one chroma row serves both rows) or of one row (YUYV) --, loads its 2 luma dwords
//                                          and its chroma (one dword NV12, two halves I420; YUYV two dwords in all), YV_MLP items' loads issued
//                                          before the first conversion, converts, and writes 4 D interleaved bytes per row as D dwords into the
//                                          SAME band layout (byte 4 r P + x D + d - a0, a0 = (xs & ~3) D: a 4-pixel group is D whole dwords).
//                                          Lanes run along the groups of a row (consecutive dwords of Y, of NV12 chroma): the items are counted off
//                                          in rows of 2^lw >= the widest tile's groups (the launcher's choice), 256 per pass.  Behind the band
//                                          everything is the resize's arithmetic, from resize_tile.h (see yuv_body).
//   yuv_image_kernel<FMT, D>               element-wise, no LDS: a lane owns one item, so each chroma sample is loaded once, and stores 4 D bytes
//                                          per row -- D dwords when image_d, pitch and image_stride are multiples of 4, bytes otherwise.
// Loads: dwords (halves for I420 chroma) when every used plane pointer, pitch and stride is a multiple of 4, bytes otherwise, and bytes for the
// group that crosses a row's end: nothing beyond a row's live bytes is read.  Both routes give the same bytes.
// The 8-bit value is clamped in Q20 BEFORE the shift and packed with shifts and masks (the other order selected a packed
// shift-and-saturate instruction whose device bytes were wrong).
// Plain C++ over (threadIdx, blockIdx, gridDim, __syncthreads) and an LDS pointer: tools/yuv_hostcheck.cpp compiles this file for the host, threads
// as lanes, under the sanitizers (AEFFT_HOSTCHECK: tools/hostlanes.h supplies those names and leaves the launchers out).
#include <type_traits>
#ifndef AEFFT_HOSTCHECK
#include "internal.h"
#define RZ_HD __host__ __device__ __forceinline__
#define RZ_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)
#endif
#include "resize_taps.h"                         // RzTap, rz_tap, rz_weight: the tap formulas of every kernel that resizes
#include "resize_tile.h"                         // rz_band_sums, rz_store_block: the phases behind the staging, shared with resize_kernels.hip

namespace aefft {

constexpr int YV_NV12 = 0, YV_I420 = 1, YV_YUYV = 2;     // == AEFFT_YUV_NV12 / _I420 / _YUYV
constexpr int YV_TJ = 16;                        // destination rows of a tile, TI = 64 / D columns, as resize_kernels.hip
constexpr int YV_MLP = 2;                        // items (2 x 4 pixels, 3 loads) a lane has in flight while staging
constexpr int YV_BAND_WORDS = 8704;              // dwords of staged rows a workgroup holds (a row of 8192 x 3 bytes fits)

// the conversion's constants: yoff, ky and the D rows (a_d, b_d) in the order the channels are stored
struct YvCoef { int yoff, ky, a[3], b[3]; };
// include/aefft.h's table: rows (R, G, B) of BT601, BT709, JPEG; order 0 BGR, 1 RGB, 2 GRAY (no rows)
static inline YvCoef yv_coef(int matrix, int order)
{
    static const int T[3][8] = {{16, 1220945, 0, 1673555, -410793, -852458, 2115221, 0},
                                {16, 1220945, 0, 1879825, -223607, -558796, 2215014, 0},
                                {0, 1048576, 0, 1470104, -360853, -748826, 1858077, 0}};
    YvCoef k = {T[matrix][0], T[matrix][1], {0, 0, 0}, {0, 0, 0}};
    for (int d = 0; d < 3 && order != 2; ++d) {
        const int row = order == 0 ? 2 - d : d;
        k.a[d] = T[matrix][2 + 2 * row]; k.b[d] = T[matrix][3 + 2 * row];
    }
    return k;
}

// the source of both kernels: plane k of image b starts at plane[k] + b * stride[k] (stride 0 for B == 1)
struct YvSrc {
    const unsigned char* plane[3]; size_t pitch[3], stride[3];
    int W, H;
    bool words;                                  // every used pointer, pitch and stride is a multiple of 4
    YvCoef k;
};
static inline YvSrc yv_source(int fmt, const unsigned char* const* plane, const size_t* pitch, const size_t* stride, int W, int H, int matrix, int order, int B)
{
    YvSrc s;
    const int used = order == 2 || fmt == YV_YUYV ? 1 : (fmt == YV_NV12 ? 2 : 3);
    uintptr_t bits = 0;
    for (int k = 0; k < 3; ++k) {
        s.plane[k] = k < used ? plane[k] : nullptr; s.pitch[k] = k < used ? pitch[k] : 0; s.stride[k] = k < used && B > 1 ? stride[k] : 0;
        bits |= reinterpret_cast<uintptr_t>(s.plane[k]) | s.pitch[k] | s.stride[k];
    }
    s.W = W; s.H = H; s.words = (bits & 3u) == 0;
    s.k = yv_coef(matrix, order);
    return s;
}

// N (4 or 2) bytes at p, the first n >= 1 of them live.  FAST: all N are live and p is aligned -- one load; otherwise single bytes (a dead byte
// re-reads byte 0 and is masked: no branch)
template <int N, bool FAST>
RZ_HD unsigned yv_ld(const unsigned char* p, int n)
{
    if (FAST) return N == 4 ? *reinterpret_cast<const unsigned*>(p) : (unsigned)*reinterpret_cast<const unsigned short*>(p);
    unsigned v = 0;
#pragma unroll
    for (int e = 0; e < N; ++e) v |= (e < n ? (unsigned)p[e < n ? e : 0] : 0u) << (8 * e);
    return v;
}

// an item: pixels x .. x + 3 (x a multiple of 4, x < W) of luma rows 2 p, 2 p + 1 (NV12, I420) or of row p (YUYV), as loaded.
//   NV12  y[r] = the row's 4 Y bytes, c0 = U V U V        I420  c0 = U U, c1 = V V (two bytes each)        YUYV  y[0] = Y U Y V, c0 = Y U Y V
struct YvItem { unsigned y[2], c0, c1; };
// whether an item at x loads whole dwords: the words route, and its 4 pixels exist (then so do its 2 chroma pairs, whole)
RZ_HD bool yv_fast(const YvSrc& s, int x) { return s.words && s.W - x >= 4; }
// pl: the image's three plane bases.  A luma row outside [ylo, yhi) is replaced by the nearest one inside (loaded, never used): no branch
template <int FMT, int D, bool FAST>
RZ_HD YvItem yv_load(const YvSrc& s, const unsigned char* const* pl, int x, int p, int ylo, int yhi)
{
    YvItem it = {{0u, 0u}, 0u, 0u};
    if (FMT == YV_YUYV) {
        const unsigned char* r = pl[0] + (size_t)p * s.pitch[0] + 2 * x;
        const int n = 2 * (s.W - x);                                             // live bytes from here (W is even: at least 4)
        it.y[0] = yv_ld<4, FAST>(r, n);
        it.c0 = yv_ld<4, FAST>(r + (n > 4 ? 4 : 0), n - 4);                      // (n == 4: no second pair; every byte masked)
    } else {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int y = rz_min(rz_max(2 * p + r, ylo), yhi - 1);
            it.y[r] = yv_ld<4, FAST>(pl[0] + (size_t)y * s.pitch[0] + x, s.W - x);
        }
        if (D == 3) {
            const int Wc = (s.W + 1) >> 1;
            if (FMT == YV_NV12) it.c0 = yv_ld<4, FAST>(pl[1] + (size_t)p * s.pitch[1] + x, 2 * Wc - x);
            else {
                it.c0 = yv_ld<2, FAST>(pl[1] + (size_t)p * s.pitch[1] + (x >> 1), Wc - (x >> 1));
                it.c1 = yv_ld<2, FAST>(pl[2] + (size_t)p * s.pitch[2] + (x >> 1), Wc - (x >> 1));
            }
        }
    }
    return it;
}
// a coefficient (|k| < 2^23) times c, u or v (9 bits and a sign): both fit 24 bits and the product 32, so the device multiplies at the full rate
// (v_mul_i32_i24 / v_mad_i32_i24; the 32-bit v_mul_lo_u32 runs at a quarter of it) with the same bits
RZ_HD int yv_mul(int k, int x)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __mul24(k, x);
#else
    return k * x;
#endif
}
// row r of an item -> its 4 D interleaved bytes as D dwords (pixels beyond W: whatever the zero bytes give; they are never used)
template <int FMT, int D>
RZ_HD void yv_convert(const YvCoef& k, const YvItem& it, int r, unsigned* out)
{
#pragma unroll
    for (int n = 0; n < D; ++n) out[n] = 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        int Y, U = 128, V = 128;
        if (FMT == YV_YUYV) {
            const unsigned w = e < 2 ? it.y[0] : it.c0;
            Y = (int)((w >> (16 * (e & 1))) & 255u); U = (int)((w >> 8) & 255u); V = (int)(w >> 24);
        } else {
            Y = (int)((it.y[r] >> (8 * e)) & 255u);
            if (FMT == YV_NV12) { U = (int)((it.c0 >> (16 * (e >> 1))) & 255u); V = (int)((it.c0 >> (16 * (e >> 1) + 8)) & 255u); }
            else { U = (int)((it.c0 >> (8 * (e >> 1))) & 255u); V = (int)((it.c1 >> (8 * (e >> 1))) & 255u); }
        }
        const int base = yv_mul(k.ky, Y - k.yoff) + (1 << 19), u = U - 128, v = V - 128;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int t = D == 3 ? base + yv_mul(k.a[d], u) + yv_mul(k.b[d], v) : base;   // |t| < 2^30
            const unsigned px = (unsigned)(t < 0 ? 0 : t > 0xfffffff ? 0xfffffff : t) >> 20;   // clamped in Q20, then shifted
            const int n = e * D + d;
            out[n >> 2] |= px << (8 * (n & 3));
        }
    }
}

// ---- yuv -> image ----------------------------------------------------------------------------------
struct YiArgs {
    YvSrc s;
    unsigned char* image; size_t pitch, stride;
    int B, gx, gy;                               // images; blocks of 64 groups along a row, blocks of 4 item rows
    bool img_words;
};

template <int FMT, int D>
__device__ __forceinline__ void yuv_image_body(const YiArgs& a)
{
    constexpr int RSH = FMT == YV_YUYV ? 0 : 1;                                  // luma rows of an item: 1 << RSH
    const int tid = (int)threadIdx.x;
    const int by = (int)blockIdx.x / a.gx, bx = (int)blockIdx.x - by * a.gx;
    const int x = 4 * (bx * 64 + (tid & 63)), p = by * 4 + (tid >> 6);
    if (x >= a.s.W || (p << RSH) >= a.s.H) return;
    const int live = rz_min(4, a.s.W - x) * D;                                   // bytes of the group that exist
    // grid.y: the images, folded (a folded grid loops)
    for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
        const unsigned char* pl[3] = {a.s.plane[0] + (size_t)b * a.s.stride[0], a.s.plane[1] + (size_t)b * a.s.stride[1], a.s.plane[2] + (size_t)b * a.s.stride[2]};
        const YvItem it = yv_fast(a.s, x) ? yv_load<FMT, D, true>(a.s, pl, x, p, 0, a.s.H) : yv_load<FMT, D, false>(a.s, pl, x, p, 0, a.s.H);
#pragma unroll
        for (int r = 0; r <= RSH; ++r) {
            const int y = (p << RSH) + r;
            if (y >= a.s.H) continue;
            unsigned out[D];
            yv_convert<FMT, D>(a.s.k, it, r, out);
            unsigned char* o = a.image + (size_t)b * a.stride + (size_t)y * a.pitch + (size_t)x * D;
            if (a.img_words && live == 4 * D) {
#pragma unroll
                for (int n = 0; n < D; ++n) reinterpret_cast<unsigned*>(o)[n] = out[n];
            } else {
#pragma unroll
                for (int n = 0; n < 4 * D; ++n)
                    if (n < live) o[n] = (unsigned char)(out[n >> 2] >> (8 * (n & 3)));
            }
        }
    }
}

static inline YiArgs yi_geometry(const YvSrc& s, int fmt, unsigned char* image, size_t pitch, size_t stride, int B)
{
    YiArgs g;
    g.s = s; g.image = image; g.pitch = pitch; g.stride = B > 1 ? stride : 0; g.B = B;
    const int groups = (s.W + 3) / 4, prows = fmt == YV_YUYV ? s.H : (s.H + 1) / 2;
    g.gx = (groups + 63) / 64; g.gy = (prows + 3) / 4;
    g.img_words = ((reinterpret_cast<uintptr_t>(image) | pitch | g.stride) & 3u) == 0;
    return g;
}

// ---- yuv -> resize -> frames -------------------------------------------------------------------------
RZ_HD int yv_ti(int D) { return 64 / D; }        // destination columns of a tile: 64 (GRAY), 21
struct YvArgs {
    YvSrc s;
    void* frames;
    int Nx, Ny;
    int tx, ty, B;                               // tiles per image along x and y; images
    int P, RB;                                   // dwords of a staged row (odd); rows of a band
    int lw;                                      // 2^lw >= the widest tile's groups of 4 pixels: the staging's items are counted off in rows of 2^lw
    bool frm_words;
};
constexpr int YV_ARG_WORDS = (int)((sizeof(YvArgs) + 15) / 16) * 4;               // dwords of the arguments' copy in LDS
// LDS of a launch, in dwords: the taps (TI + TJ of 4), the arguments' copy and the band
RZ_HD int yv_lds_words(int D, int P, int RB) { return 4 * (yv_ti(D) + YV_TJ) + YV_ARG_WORDS + P * RB; }

// rows [yb, yb + nr) x the groups of pixels [xs & ~3, xe) of image b, converted, into the band.  `a` is the workgroup's copy of the arguments in
// LDS: read from there, planes, pitches, strides and coefficients are in vector registers for the staging only.  The scalar file is the tile
// body's tight resource, and 29 more dwords of kernel arguments kept in it spilled up to 52 scalar registers.
template <int FMT, int D>
__device__ __forceinline__ void yuv_stage(const YvArgs& a, int b, int xs, int xe, int yb, int nr, unsigned* rows)
{
    const YvSrc& s = a.s;
    constexpr int RSH = FMT == YV_YUYV ? 0 : 1;
    const int tid = (int)threadIdx.x;
    const int x0 = xs & ~3, ng = (xe - x0 + 3) >> 2;                             // (ng D <= P: the launcher sized P over every tile)
    const int p0 = yb >> RSH, p1 = ((yb + nr - 1) >> RSH) + 1;                   // the item rows that meet the band
    const int total = (p1 - p0) << a.lw, gmask = (1 << a.lw) - 1;                // item t: row p0 + (t >> lw), group t & gmask (live below ng)
    const unsigned char* pl[3] = {s.plane[0] + (size_t)b * s.stride[0], s.plane[1] + (size_t)b * s.stride[1], s.plane[2] + (size_t)b * s.stride[2]};
#pragma unroll 1
    for (int t = tid; t < total; t += 256 * YV_MLP) {
        // every load of the lane's YV_MLP items before the first conversion; an item beyond the band or the tile's groups repeats the nearest live
        // one (loaded, never used), so the loads take no branch but the one between whole dwords and bytes
        YvItem it[YV_MLP];
        int pk[YV_MLP], gk[YV_MLP];
        bool fast = true;
#pragma unroll
        for (int k = 0; k < YV_MLP; ++k) {
            const int tk = rz_min(t + 256 * k, total - 1);
            pk[k] = p0 + (tk >> a.lw); gk[k] = rz_min(tk & gmask, ng - 1);
            fast = fast && yv_fast(s, x0 + 4 * gk[k]);
        }
        if (fast) {
#pragma unroll
            for (int k = 0; k < YV_MLP; ++k) it[k] = yv_load<FMT, D, true>(s, pl, x0 + 4 * gk[k], pk[k], yb, yb + nr);
        } else {
#pragma unroll
            for (int k = 0; k < YV_MLP; ++k) it[k] = yv_load<FMT, D, false>(s, pl, x0 + 4 * gk[k], pk[k], yb, yb + nr);
        }
#pragma unroll
        for (int k = 0; k < YV_MLP; ++k) {
            if (t + 256 * k >= total || ((t + 256 * k) & gmask) >= ng) continue;
#pragma unroll
            for (int r = 0; r <= RSH; ++r) {
                const int y = (pk[k] << RSH) + r - yb;
                if ((unsigned)y >= (unsigned)nr) continue;                       // (a row of another band)
                unsigned out[D];
                yv_convert<FMT, D>(s.k, it[k], r, out);
#pragma unroll
                for (int n = 0; n < D; ++n) rows[y * a.P + gk[k] * D + n] = out[n];
            }
        }
    }
}

// The tile body: resize_body's (resize_kernels.hip; DESIGN.md section 20 has the argument for each step) with yuv_stage as its staging and the
// arguments' copy in LDS.  The taps, the lane's block and the band loop are this body's own, as they are there; the arithmetic behind the
// staging -- the LINEAR / AREA sums over a band, the roundings and the stores -- is resize_tile.h's rz_band_sums and rz_store_block, which both
// bodies call with scalars (DESIGN.md section 23 has the register tables before and after).  The composition test (tests/test_gpu_yuv.py: fused ==
// yuv_to_image -> image_resize_to_frames, bit for bit) holds the two stagings to the same band layout.
template <int FMT, int D, bool F32, int MODE>
__device__ __forceinline__ void yuv_body(const YvArgs& a, unsigned* lds)
{
    typedef typename std::conditional<MODE == RZ_AREA, unsigned long long, unsigned>::type acc_t;
    constexpr int TI = 64 / D;
    RzTap* xt = reinterpret_cast<RzTap*>(lds);
    RzTap* yt = xt + TI;
    unsigned* args = lds + 4 * (TI + YV_TJ);
    unsigned* rows = args + YV_ARG_WORDS;
    const unsigned char* rowb = reinterpret_cast<const unsigned char*>(rows);
    const int tid = (int)threadIdx.x;
    if (tid < (int)(sizeof(YvArgs) / 4)) args[tid] = reinterpret_cast<const unsigned*>(&a)[tid];   // (visible behind the taps' barrier)
    // grid.x: the tx ty tiles of an image (at most 2^18), grid.y: the images, folded onto at most 2^20 workgroups (uniform: a folded grid loops)
    for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
        const int ty_i = (int)blockIdx.x / a.tx;
        const int i0 = ((int)blockIdx.x - ty_i * a.tx) * TI, j0 = ty_i * YV_TJ;
        const int ncols = rz_min(a.Nx - i0, TI), nrows = rz_min(a.Ny - j0, YV_TJ);
        if (tid < ncols) xt[tid] = rz_tap(MODE, i0 + tid, a.s.W, a.Nx);
        else if (tid >= TI && tid < TI + nrows) yt[tid - TI] = rz_tap(MODE, j0 + tid - TI, a.s.H, a.Ny);
        __syncthreads();
        // source columns [xs, xe) and rows [ys, ye) of the tile (the same in every lane; the rows, which bound the band loop, in scalar registers)
        const int xs = xt[0].lo, xe = xt[ncols - 1].lo + xt[ncols - 1].cnt;
        const int ys = RZ_UNIFORM(yt[0].lo), ye = RZ_UNIFORM(yt[nrows - 1].lo + yt[nrows - 1].cnt);
        const int a0 = (xs & ~3) * D;                                            // first staged byte of a row: a whole group of 4 pixels
        // the lane's block: column c = i D + d (lanes run along c), rows 4 q .. 4 q + 3 of the tile
        const int tc = ncols * D;
        const int q = tid / tc, c = tid - q * tc, i = c / D, d = c - i * D;
        const bool own = 4 * q < nrows;
        const RzTap X = xt[i];
        const unsigned char* col = rowb + (X.lo * D + d - a0);
        acc_t acc[4] = {0, 0, 0, 0};
        for (int yb = ys; yb < ye; yb += a.RB) {
            const int nr = rz_min(a.RB, ye - yb);
            yuv_stage<FMT, D>(*reinterpret_cast<const YvArgs*>(args), b, xs, xe, yb, nr, rows);
            __syncthreads();
            rz_band_sums<D, MODE>(X, yt, col, a.P, q, nrows, own, yb, nr, a.Nx, a.Ny, acc);
            __syncthreads();
        }
        if (!own) continue;
        const size_t o = (((size_t)b * D + d) * a.Nx + (i0 + i)) * (size_t)a.Ny + (j0 + 4 * q);
        rz_store_block<F32, MODE>(acc[0], acc[1], acc[2], acc[3], (unsigned long long)a.s.W * a.s.H, a.frames, o, a.frm_words, q, nrows);
    }
}

// the launch geometry: tiles, the staged row's dwords P (the widest tile's groups x D, made odd), the lanes per staged row and the band's rows RB
// (the tallest tile's footprint, or what YV_BAND_WORDS holds of it).  Exact, from the same rz_tap the kernel uses.
static inline YvArgs yv_geometry(const YvSrc& s, int mode, void* frames, int B, int D, int Nx, int Ny)
{
    YvArgs g;
    g.s = s; g.frames = frames; g.Nx = Nx; g.Ny = Ny; g.B = B;
    const int TI = yv_ti(D);
    g.tx = (Nx + TI - 1) / TI; g.ty = (Ny + YV_TJ - 1) / YV_TJ;
    g.frm_words = (Ny & 3) == 0;
    int ng = 1, nr = 1;
    for (int t = 0; t < g.tx; ++t) {
        const RzTap f = rz_tap(mode, t * TI, s.W, Nx), l = rz_tap(mode, rz_min(t * TI + TI, Nx) - 1, s.W, Nx);
        ng = rz_max(ng, (l.lo + l.cnt - (f.lo & ~3) + 3) >> 2);
    }
    for (int t = 0; t < g.ty; ++t) {
        const RzTap f = rz_tap(mode, t * YV_TJ, s.H, Ny), l = rz_tap(mode, rz_min(t * YV_TJ + YV_TJ, Ny) - 1, s.H, Ny);
        nr = rz_max(nr, l.lo + l.cnt - f.lo);
    }
    g.P = (ng * D) | 1;
    g.RB = rz_max(1, rz_min(nr, YV_BAND_WORDS / g.P));
    g.lw = 0;
    while ((1 << g.lw) < ng) ++g.lw;
    return g;
}

#ifndef AEFFT_HOSTCHECK
template <int FMT, int D>
__global__ __launch_bounds__(256) void yuv_image_kernel(const YiArgs a) { yuv_image_body<FMT, D>(a); }

template <int FMT, int D, bool F32, int MODE>
__global__ __launch_bounds__(256) void yuv_resize_kernel(const YvArgs a)
{
    extern __shared__ unsigned yv_lds[];
    yuv_body<FMT, D, F32, MODE>(a, yv_lds);
}

static bool yv_args_ok(int fmt, const unsigned char* const* plane, const size_t* pitch, int W, int H, int matrix, int order, int B)
{
    const auto in = [](int v) { return v >= 1 && v <= 8192; };
    if (fmt < 0 || fmt > 2 || matrix < 0 || matrix > 2 || order < 0 || order > 2 || !plane || !pitch || B < 1 || !in(W) || !in(H)) return false;
    if (fmt == YV_YUYV) return plane[0] && (W & 1) == 0 && pitch[0] >= (size_t)2 * W;
    const size_t Wc = (size_t)(W + 1) / 2;
    if (!plane[0] || pitch[0] < (size_t)W) return false;
    if (order == 2) return true;
    if (fmt == YV_NV12) return plane[1] && pitch[1] >= 2 * Wc;
    return plane[1] && plane[2] && pitch[1] >= Wc && pitch[2] >= Wc;
}
// GRAY reads the luma plane only, which NV12 and I420 lay out alike: one set of D = 1 kernels serves both
static int yv_kernel_fmt(int fmt, int order) { return order == 2 && fmt == YV_I420 ? YV_NV12 : fmt; }

hipError_t launch_yuv_image(int fmt, const unsigned char* const* plane, const size_t* pitch, const size_t* stride, int W, int H, int matrix, int order,
                            unsigned char* image, size_t ipitch, size_t istride, int B, hipStream_t st)
{
    const int D = order == 2 ? 1 : 3;
    if (!yv_args_ok(fmt, plane, pitch, W, H, matrix, order, B) || !image || ipitch < (size_t)W * D || (B > 1 && !stride)) return hipErrorInvalidValue;
    const YiArgs g = yi_geometry(yv_source(fmt, plane, pitch, stride, W, H, matrix, order, B), fmt, image, ipitch, istride, B);
    const unsigned tpi = (unsigned)(g.gx * g.gy);                                // at most 32 x 2048 blocks per image
    const dim3 gr(tpi, (unsigned)B < 65535u ? (unsigned)B : 65535u), bl(256);
#define YI_CASE(FF, DD) case ((FF) * 2 + ((DD) == 3)): yuv_image_kernel<FF, DD><<<gr, bl, 0, st>>>(g); break;
    switch (yv_kernel_fmt(fmt, order) * 2 + (D == 3)) {
        YI_CASE(0, 1) YI_CASE(0, 3) YI_CASE(1, 3) YI_CASE(2, 1) YI_CASE(2, 3)
        default: return hipErrorInvalidValue;
    }
#undef YI_CASE
    return hipGetLastError();
}

hipError_t launch_yuv_resize(int fmt, const unsigned char* const* plane, const size_t* pitch, const size_t* stride, int W, int H, int matrix, int order,
                             int mode, void* frames, bool f32, int B, int Nx, int Ny, hipStream_t st)
{
    const auto in = [](int v) { return v >= 1 && v <= 8192; };
    const int D = order == 2 ? 1 : 3;
    if (!yv_args_ok(fmt, plane, pitch, W, H, matrix, order, B) || !frames || !in(Nx) || !in(Ny) || (B > 1 && !stride)) return hipErrorInvalidValue;
    if (mode != RZ_LINEAR && mode != RZ_AREA) return hipErrorInvalidValue;
    if (mode == RZ_AREA && (Nx > W || Ny > H)) return hipErrorInvalidValue;
    const YvArgs g = yv_geometry(yv_source(fmt, plane, pitch, stride, W, H, matrix, order, B), mode, frames, B, D, Nx, Ny);
    const unsigned tpi = (unsigned)(g.tx * g.ty), by = (1u << 20) / tpi < 65535u ? (1u << 20) / tpi : 65535u;
    const dim3 gr(tpi, (unsigned)B < by ? (unsigned)B : by), bl(256);
    const size_t lds = 4 * (size_t)yv_lds_words(D, g.P, g.RB);
#define YV_CASE(FF, DD, TT, MM) case ((FF) * 8 + ((DD) == 3) * 4 + (TT) * 2 + (MM)): yuv_resize_kernel<FF, DD, TT != 0, MM><<<gr, bl, lds, st>>>(g); break;
#define YV_CASES(FF, DD) YV_CASE(FF, DD, 0, 0) YV_CASE(FF, DD, 0, 1) YV_CASE(FF, DD, 1, 0) YV_CASE(FF, DD, 1, 1)
    switch (yv_kernel_fmt(fmt, order) * 8 + (D == 3) * 4 + (f32 ? 2 : 0) + mode) {
        YV_CASES(0, 1) YV_CASES(0, 3) YV_CASES(1, 3) YV_CASES(2, 1) YV_CASES(2, 3)
        default: return hipErrorInvalidValue;
    }
#undef YV_CASES
#undef YV_CASE
    return hipGetLastError();
}
#endif

}  // namespace aefft
