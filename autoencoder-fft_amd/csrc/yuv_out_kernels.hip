// aefft_image_to_yuv and aefft_frames_resize_to_yuv (gfx950): video OUT -- interleaved 8-bit images, or the planar frames a net writes, to the NV12
// surface a hardware encoder takes, the I420 planes of a software encoder or the YUYV buffer of a V4L2 sink, one launch each.  The mirror of
// yuv_kernels.hip.  All-integer (include/aefft.h states tables and formulas): with R, G, B a pixel's channels
//   Y = yoff + ((yr R + yg G + yb B + 2^19) >> 20)                                             one per pixel, in range without a clamp
//   U = clamp(128 + ((ur S_R + ug S_G + ub S_B + (n << 19)) >> (20 + log2 n)), 0, 255)         S: the channel sums over the sample's n LIVE pixels
// (V likewise): the block (2x'..2x'+1, 2y'..2y'+1) cut to the image for NV12 and I420 (n = 4, 2, 1), the pair (2x', 2x'+1) of a row for YUYV.
// Both kernels REPLICATE the nearest live pixel into a dead one (a column beyond W, a row beyond H) instead of masking it: the sum over the full
// block is then S 4 / n (YUYV: twice the pair's sum, S 4 / n again), and
//   (k S (4 / n) + 2^21) >> 22  ==  (k S + (n << 19)) >> (20 + log2 n)           (numerator and denominator times 4 / n: the same floor),
// so every sample takes ONE formula with a constant shift and no branch.  The 128 is carried inside the shift (128 << 22), so the sum is clamped
// in Q22 BEFORE the shift and the bytes are packed with shifts and masks (DESIGN.md sections 22-23: the other order selected a packed
// shift-and-saturate instruction whose device bytes were wrong).  Coefficients are below 2^23 and sums at most 1020: 24-bit multiplies are exact.
// The D coefficient columns come in as arguments in the order the channels are stored: matrix and channel order are data, not instantiations.
// D = 3 (BGR, RGB) or D = 1 (GRAY: Y from ky alone, every chroma sample 128).
//   image_yuv_kernel<FMT, D>               element-wise, no LDS, the ITEM scheme of yuv_image_kernel: a lane owns 4 pixels of a luma row pair (NV12,
//                                          I420) or of one row (YUYV), loads each row's 4 D bytes as D dwords (bytes when the image pointer, pitch
//                                          or stride is no multiple of 4, and for the group that crosses the row's end), forms the 8 (4) Y and the
//                                          2 chroma samples and stores one Y dword per row plus one chroma dword (NV12), two halves (I420), or two
//                                          dwords in all (YUYV).
//   frames_yuv_kernel<FMT, D, F32, MODE>   the tile body of frames_resize_kernel (present_kernels.hip) with another step 4: the lanes read the
//                                          finished tile image from LDS an item each, convert and store plane rows.  Its tiles have an even
//                                          number of rows for NV12 and I420, so that a chroma block lies in one tile.
// Stores: whole dwords (halves for I420 chroma) when every used plane pointer, pitch and stride is a multiple of 4, bytes otherwise and for the
// group that crosses a row's end: nothing beyond a row's live bytes is written, nothing is read from the destination.  Both routes give the same bytes.
// Plain C++ over (threadIdx, blockIdx, gridDim, __syncthreads) and an LDS pointer: tools/yuv_out_hostcheck.cpp compiles this file for the host,
// threads as lanes, under the sanitizers (AEFFT_HOSTCHECK: tools/hostlanes.h supplies those names and px_u8, and leaves the launchers out).
#include <type_traits>
#ifndef AEFFT_HOSTCHECK
#include "internal.h"
#include "fft_common.h"
#define RZ_HD __host__ __device__ __forceinline__
#define RZ_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)
#endif
#include "resize_taps.h"                         // RzTap, rz_tap, rz_weight: the tap formulas of every kernel that resizes
#include "resize_tile.h"                         // fr_stage_runs, fr_band_sums, fr_round_tile and the tile constants, shared with present_kernels.hip

namespace aefft {

constexpr int YO_NV12 = 0, YO_I420 = 1, YO_YUYV = 2;     // == AEFFT_YUV_NV12 / _I420 / _YUYV

// the conversion's constants: yoff, ky and the coefficients of Y, U and V for channel d as stored
struct YoCoef { int yoff, ky, y[3], u[3], v[3]; };
// include/aefft.h's table: rows BT601, BT709, JPEG; yoff, ky, then (r, g, b) of Y, U and V; order 0 BGR, 1 RGB, 2 GRAY (Y from ky, no chroma)
static inline YoCoef yo_coef(int matrix, int order)
{
    static const int T[3][11] = {{16, 900542, 269262, 528618, 102662, -155423, -305128, 460551, 460551, -385654, -74897},
                                 {16, 900542, 191455, 644068, 65019, -105533, -355018, 460551, 460551, -418321, -42230},
                                 {0, 1048576, 313524, 615514, 119538, -176932, -347356, 524288, 524288, -439026, -85262}};
    YoCoef k = {T[matrix][0], T[matrix][1], {T[matrix][1], 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int d = 0; d < 3 && order != 2; ++d) {
        const int ch = order == 0 ? 2 - d : d;
        k.y[d] = T[matrix][2 + ch]; k.u[d] = T[matrix][5 + ch]; k.v[d] = T[matrix][8 + ch];
    }
    return k;
}

// the destination of both kernels: plane k of image b starts at plane[k] + b * stride[k] (stride 0 for B == 1); every plane of the format is written
struct YoDst {
    unsigned char* plane[3]; size_t pitch[3], stride[3];
    int W, H;
    bool words;                                  // every used pointer, pitch and stride is a multiple of 4
    YoCoef k;
};
static inline int yo_planes(int fmt) { return fmt == YO_I420 ? 3 : (fmt == YO_NV12 ? 2 : 1); }
static inline YoDst yo_dest(int fmt, unsigned char* const* plane, const size_t* pitch, const size_t* stride, int W, int H, int matrix, int order, int B)
{
    YoDst s;
    const int used = yo_planes(fmt);
    uintptr_t bits = 0;
    for (int k = 0; k < 3; ++k) {
        s.plane[k] = k < used ? plane[k] : nullptr; s.pitch[k] = k < used ? pitch[k] : 0; s.stride[k] = k < used && B > 1 ? stride[k] : 0;
        bits |= reinterpret_cast<uintptr_t>(s.plane[k]) | s.pitch[k] | s.stride[k];
    }
    s.W = W; s.H = H; s.words = (bits & 3u) == 0;
    s.k = yo_coef(matrix, order);
    return s;
}

// a coefficient (|k| < 2^23) times a channel or a sum of four (at most 1020): both fit 24 bits and the product 32, so the device multiplies at the
// full rate with the same bits
RZ_HD int yo_mul(int k, int x)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __mul24(k, x);
#else
    return k * x;
#endif
}

// an item's pixels as loaded: row r's 4 D interleaved bytes as D dwords, dead pixels and a dead row holding the nearest live pixel.  Out: NV12, I420
// yw[r] = the row's 4 Y bytes; NV12 cw[0] = U V U V; I420 cw[0] = U U, cw[1] = V V (two bytes each); YUYV cw[0], cw[1] = Y U Y V each
template <int FMT, int D>
RZ_HD void yo_convert(const YoCoef& k, const unsigned (*in)[D], unsigned* yw, unsigned* cw)
{
    constexpr int ROWS = FMT == YO_YUYV ? 1 : 2;
    constexpr int SH = 20 + ROWS;                                                // the chroma shift: the sums run over 2 ROWS pixels
    int S[2][D];
    unsigned Y[ROWS][4];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int d = 0; d < D; ++d) S[c][d] = 0;
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int t = 1 << 19;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const int n = e * D + d, ch = (int)((in[r][n >> 2] >> (8 * (n & 3))) & 255u);
                t += yo_mul(k.y[d], ch);                                         // (positive coefficients: 0 <= t < 2^29, Y in range without a clamp)
                S[e >> 1][d] += ch;
            }
            Y[r][e] = (unsigned)k.yoff + ((unsigned)t >> 20);
        }
    unsigned U[2] = {128u, 128u}, V[2] = {128u, 128u};
    if (D == 3) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            int tu = (1 << (SH - 1)) + (128 << SH), tv = tu;                     // the rounding, and the 128 inside the shift: 0 < t <= 2^30
#pragma unroll
            for (int d = 0; d < D; ++d) { tu += yo_mul(k.u[d], S[c][d]); tv += yo_mul(k.v[d], S[c][d]); }
            const int hi = (256 << SH) - 1;                                      // clamped in Q(SH), then shifted
            U[c] = (unsigned)(tu < 0 ? 0 : tu > hi ? hi : tu) >> SH;
            V[c] = (unsigned)(tv < 0 ? 0 : tv > hi ? hi : tv) >> SH;
        }
    }
    if (FMT == YO_YUYV) {
        cw[0] = Y[0][0] | U[0] << 8 | Y[0][1] << 16 | V[0] << 24;
        cw[1] = Y[0][2] | U[1] << 8 | Y[0][3] << 16 | V[1] << 24;
        yw[0] = 0u;
    } else {
#pragma unroll
        for (int r = 0; r < ROWS; ++r) yw[r] = Y[r][0] | Y[r][1] << 8 | Y[r][2] << 16 | Y[r][3] << 24;
        if (FMT == YO_NV12) { cw[0] = U[0] | V[0] << 8 | U[1] << 16 | V[1] << 24; cw[1] = 0u; }
        else { cw[0] = U[0] | U[1] << 8; cw[1] = V[0] | V[1] << 8; }
    }
}

// n (at most N) live bytes of the N in w to o; FAST: all N are live and o is aligned -- one store
template <int N, bool FAST>
RZ_HD void yo_st(unsigned char* o, unsigned w, int n)
{
    if (FAST) {
        if (N == 4) *reinterpret_cast<unsigned*>(o) = w;
        else *reinterpret_cast<unsigned short*>(o) = (unsigned short)w;
        return;
    }
#pragma unroll
    for (int e = 0; e < N; ++e)
        if (e < n) o[e] = (unsigned char)(w >> (8 * e));
}
// the item at pixels x .. x + 3 (x a multiple of 4, `live` = min(4, W - x) of them exist) of luma rows 2 p, 2 p + 1 (YUYV: of row p) into the planes
// pl of one image.  FAST: the words route and live == 4 (then the item's chroma samples are whole too)
template <int FMT, bool FAST>
RZ_HD void yo_store(const YoDst& s, unsigned char* const* pl, int x, int p, int live, const unsigned* yw, const unsigned* cw)
{
    if (FMT == YO_YUYV) {
        unsigned char* o = pl[0] + (size_t)p * s.pitch[0] + 2 * (size_t)x;
        yo_st<4, FAST>(o, cw[0], 2 * live);                                      // (W is even: live is 2 or 4)
        if (live > 2) yo_st<4, FAST>(o + 4, cw[1], 2 * live - 4);
        return;
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
        if (2 * p + r < s.H) yo_st<4, FAST>(pl[0] + (size_t)(2 * p + r) * s.pitch[0] + x, yw[r], live);
    const int lc = (live + 1) >> 1;                                              // chroma samples of the item that exist
    if (FMT == YO_NV12) yo_st<4, FAST>(pl[1] + (size_t)p * s.pitch[1] + x, cw[0], 2 * lc);
    else {
        yo_st<2, FAST>(pl[1] + (size_t)p * s.pitch[1] + (x >> 1), cw[0], lc);
        yo_st<2, FAST>(pl[2] + (size_t)p * s.pitch[2] + (x >> 1), cw[1], lc);
    }
}

// ---- image -> yuv ----------------------------------------------------------------------------------
struct YoArgs {
    YoDst s;
    const unsigned char* image; size_t pitch, stride;
    int B, gx, gy;                               // images; blocks of 64 groups along a row, blocks of 4 item rows
    bool img_words;
};

template <int FMT, int D>
__device__ __forceinline__ void image_yuv_body(const YoArgs& a)
{
    constexpr int RSH = FMT == YO_YUYV ? 0 : 1;                                  // luma rows of an item: 1 << RSH
    const int tid = (int)threadIdx.x;
    const int by = (int)blockIdx.x / a.gx, bx = (int)blockIdx.x - by * a.gx;
    const int x = 4 * (bx * 64 + (tid & 63)), p = by * 4 + (tid >> 6);
    if (x >= a.s.W || (p << RSH) >= a.s.H) return;
    const int live = rz_min(4, a.s.W - x);                                       // pixels of the group that exist
    // grid.y: the images, folded (a folded grid loops)
    for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
        unsigned in[RSH + 1][D];
#pragma unroll
        for (int r = 0; r <= RSH; ++r) {
            const int y = rz_min((p << RSH) + r, a.s.H - 1);                     // (a row beyond H: the last one again)
            const unsigned char* row = a.image + (size_t)b * a.stride + (size_t)y * a.pitch + (size_t)x * D;
            if (a.img_words && live == 4) {
#pragma unroll
                for (int n = 0; n < D; ++n) in[r][n] = reinterpret_cast<const unsigned*>(row)[n];
            } else {
#pragma unroll
                for (int n = 0; n < D; ++n) in[r][n] = 0u;
#pragma unroll
                for (int n = 0; n < 4 * D; ++n) {                                // (a pixel beyond W: the last one again -- no branch per pixel)
                    const int e = n / D, d = n - e * D;
                    in[r][n >> 2] |= (unsigned)row[rz_min(e, live - 1) * D + d] << (8 * (n & 3));
                }
            }
        }
        unsigned yw[2], cw[2];
        yo_convert<FMT, D>(a.s.k, in, yw, cw);
        unsigned char* pl[3] = {a.s.plane[0] + (size_t)b * a.s.stride[0], a.s.plane[1] + (size_t)b * a.s.stride[1], a.s.plane[2] + (size_t)b * a.s.stride[2]};
        if (a.s.words && live == 4) yo_store<FMT, true>(a.s, pl, x, p, live, yw, cw);
        else yo_store<FMT, false>(a.s, pl, x, p, live, yw, cw);
    }
}

static inline YoArgs yo_geometry(const YoDst& s, int fmt, const unsigned char* image, size_t pitch, size_t stride, int B)
{
    YoArgs g;
    g.s = s; g.image = image; g.pitch = pitch; g.stride = B > 1 ? stride : 0; g.B = B;
    const int groups = (s.W + 3) / 4, prows = fmt == YO_YUYV ? s.H : (s.H + 1) / 2;
    g.gx = (groups + 63) / 64; g.gy = (prows + 3) / 4;
    g.img_words = ((reinterpret_cast<uintptr_t>(image) | pitch | g.stride) & 3u) == 0;
    return g;
}

// ---- frames -> resize -> yuv -------------------------------------------------------------------------
// (the tile is frames_resize_kernel's: PR_TY, PR_CW, PR_NH, PR_RPL and pr_ceil_div of resize_tile.h)
constexpr int FY_BAND_WORDS = 8704;              // dwords of staged runs a workgroup holds (34 KiB: one column of D runs of 8192 + 3 bytes fits)

struct FyArgs {
    const void* frames;
    YoDst s;                                     // (s.W, s.H: the destination sizes)
    int Nx, Ny;                                  // the source (frame) sizes
    int TX, TY, tx, ty, B;                       // the tile; tiles per image along x and y; images
    int P, XB;                                   // dwords of a staged run (odd); source columns of a band
    int ush;                                     // log2 of the lanes a run gets while staging
    bool frm_words;
};
// LDS of a launch, in dwords: the taps (TX + TY of 4), the finished tile in image order (PR_TY row slots of PR_CW bytes) and the band
RZ_HD int fy_lds_words(int D, const FyArgs& g) { return 4 * (g.TX + g.TY) + PR_CW / 4 * PR_TY + D * g.XB * g.P; }

// The tile body: frames_resize_body's (present_kernels.hip; DESIGN.md section 21 has the argument for each step) with another step 4.  The taps (step 1),
// the lane and the band loop are this body's own, as they are there; steps 2 and 3 -- the run staging, the sums over a band and the rounding into the
// tile image in LDS -- are resize_tile.h's fr_stage_runs, fr_band_sums and fr_round_tile, which both bodies call with scalars (DESIGN.md section 23 has the
// register tables before and after).  One difference in the lane: beyond the row's live bytes it sums the LAST PIXEL's channel d again (not the
// last byte), and a row slot beyond the tile's rows the last row (as there), so that the tile image holds replicated pixels wherever an item
// reaches beyond the image.  Step 4 is this file's.
template <int FMT, int D, bool F32, int MODE>
__device__ __forceinline__ void frames_yuv_body(const FyArgs& a, unsigned* lds)
{
    typedef typename std::conditional<MODE == RZ_AREA, unsigned long long, unsigned>::type acc_t;
    constexpr int RSH = FMT == YO_YUYV ? 0 : 1;
    const int W = a.s.W, H = a.s.H;
    RzTap* xt = reinterpret_cast<RzTap*>(lds);
    RzTap* yt = xt + a.TX;
    unsigned* tile = lds + 4 * (a.TX + a.TY);
    unsigned char* tileb = reinterpret_cast<unsigned char*>(tile);
    unsigned* band = tile + PR_CW / 4 * PR_TY;
    const unsigned char* bandb = reinterpret_cast<const unsigned char*>(band);
    const int tid = (int)threadIdx.x;
    const int ty_i = (int)blockIdx.x / a.tx;
    const int i0 = ((int)blockIdx.x - ty_i * a.tx) * a.TX, j0 = ty_i * a.TY;     // (NV12, I420: TY is even, so j0 is)
    const int ncols = rz_min(W - i0, a.TX), nrows = rz_min(H - j0, a.TY);
    if (tid < ncols) xt[tid] = rz_tap(MODE, i0 + tid, a.Nx, W);
    else if (tid >= a.TX && tid < a.TX + nrows) yt[tid - a.TX] = rz_tap(MODE, j0 + tid - a.TX, a.Ny, H);
    __syncthreads();
    // source columns [xs, xe) and rows [ys, ye) of the tile (the same in every lane); ya: the first staged row (a dword of the run on the dword route)
    const int xs = RZ_UNIFORM(xt[0].lo), xe = RZ_UNIFORM(xt[ncols - 1].lo + xt[ncols - 1].cnt);
    const int ys = RZ_UNIFORM(yt[0].lo), ye = RZ_UNIFORM(yt[nrows - 1].lo + yt[nrows - 1].cnt);
    const int ya = a.frm_words ? ys & ~3 : ys;
    const int nyb = ye - ya, nwy = (nyb + 3) >> 2;                               // (nwy <= P: the launcher sized P over every tile)
    const int rowlive = ncols * D;                                               // bytes of a tile row (at most 64)
    // the lane: byte column c = i D + d of the tile row x the rows h, h + 4, .., h + 28 (h the same in a wave)
    const int c = tid % PR_CW, h = RZ_UNIFORM(tid / PR_CW);
    const int cc = c < rowlive ? c : rowlive - D + c % D, d = cc % D;            // (beyond the live bytes: the last pixel's channel again)
    const int nru = a.frm_words ? nwy : nyb;                                     // units of a staged run: dwords, or elements
    const RzTap X = xt[cc / D];
    // grid.y, grid.z: the images
    const size_t b = (size_t)blockIdx.z * gridDim.y + blockIdx.y;
    if (b >= (size_t)a.B) return;
    acc_t acc[PR_RPL];
#pragma unroll
    for (int k = 0; k < PR_RPL; ++k) acc[k] = 0;
    for (int xb = xs; xb < xe; xb += a.XB) {
        const int nxb = rz_min(a.XB, xe - xb);
        fr_stage_runs<D, F32>(tid, a.frames, b, a.Nx, a.Ny, xb, nxb, ya, nru, a.ush, a.frm_words, a.P, band);
        __syncthreads();
        fr_band_sums<D, MODE>(X, yt, bandb, a.P, d, h, nrows, xb, nxb, ya, W, H, acc);
        __syncthreads();
    }
    // the finished bytes to the tile in image order: row r = 4 k + h in slot PR_RPL h + k, all PR_TY slots and PR_CW columns of it written
    fr_round_tile<MODE>(acc, (unsigned long long)a.Nx * a.Ny, tileb, h, c);
    __syncthreads();
    // 4. a lane per item -- group g of 4 pixels (D whole dwords of a tile row) x item row pp, the groups counted off in 16 --: its rows from LDS,
    //    the conversion, and the stores of image_yuv_kernel
    unsigned char* pl[3] = {a.s.plane[0] + b * a.s.stride[0], a.s.plane[1] + b * a.s.stride[1], a.s.plane[2] + b * a.s.stride[2]};
    const int ng = (ncols + 3) >> 2, np = (nrows + RSH) >> RSH;
    for (int idx = tid; idx < np * (PR_CW / 4); idx += 256) {
        const int g = idx % (PR_CW / 4), pp = idx / (PR_CW / 4);
        if (g >= ng) continue;
        unsigned in[RSH + 1][D];
#pragma unroll
        for (int r = 0; r <= RSH; ++r) {
            const int row = (pp << RSH) + r, slot = (row % PR_NH) * PR_RPL + row / PR_NH;   // (row <= nrows <= 31: a slot beyond the rows holds the last row)
#pragma unroll
            for (int n = 0; n < D; ++n) in[r][n] = tile[PR_CW / 4 * slot + g * D + n];
        }
        unsigned yw[2], cw[2];
        yo_convert<FMT, D>(a.s.k, in, yw, cw);
        const int live = rz_min(4, ncols - 4 * g);
        if (a.s.words && live == 4) yo_store<FMT, true>(a.s, pl, i0 + 4 * g, (j0 >> RSH) + pp, live, yw, cw);
        else yo_store<FMT, false>(a.s, pl, i0 + 4 * g, (j0 >> RSH) + pp, live, yw, cw);
    }
}

// the launch geometry: fr_geometry's (present_kernels.hip) with the tile's rows made even for NV12 and I420 -- at least 2, where the present
// kernel's tile is ONE row high when the y axis reduces by more than 32 --, so that the two luma rows of a chroma block lie in one tile
static inline FyArgs fy_geometry(const YoDst& s, int fmt, const void* frames, int Nx, int Ny, int mode, int B, int D)
{
    FyArgs g;
    g.frames = frames; g.s = s; g.Nx = Nx; g.Ny = Ny; g.B = B;
    const int W = s.W, H = s.H;
    g.TX = rz_max(4, (((PR_CW / D) & ~3) / pr_ceil_div(Nx, W)) & ~3);
    g.TY = rz_max(1, PR_TY / pr_ceil_div(Ny, H));
    if (fmt != YO_YUYV) g.TY = rz_max(2, g.TY & ~1);
    g.tx = pr_ceil_div(W, g.TX); g.ty = pr_ceil_div(H, g.TY);
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
    g.XB = rz_max(1, rz_min(nx, FY_BAND_WORDS / (D * g.P)));
    return g;
}

#ifndef AEFFT_HOSTCHECK
template <int FMT, int D>
__global__ __launch_bounds__(256) void image_yuv_kernel(const YoArgs a) { image_yuv_body<FMT, D>(a); }

template <int FMT, int D, bool F32, int MODE>
__global__ __launch_bounds__(256) void frames_yuv_kernel(const FyArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned fy_lds[];
    frames_yuv_body<FMT, D, F32, MODE>(a, fy_lds);
}

static bool yo_args_ok(int fmt, unsigned char* const* plane, const size_t* pitch, const size_t* stride, int W, int H, int matrix, int order, int B)
{
    const auto in = [](int v) { return v >= 1 && v <= 8192; };
    if (fmt < 0 || fmt > 2 || matrix < 0 || matrix > 2 || order < 0 || order > 2 || !plane || !pitch || (B > 1 && !stride) || B < 1 || !in(W) || !in(H)) return false;
    if (fmt == YO_YUYV) return plane[0] && (W & 1) == 0 && pitch[0] >= (size_t)2 * W;
    const size_t Wc = (size_t)(W + 1) / 2;
    if (!plane[0] || pitch[0] < (size_t)W) return false;
    if (fmt == YO_NV12) return plane[1] && pitch[1] >= 2 * Wc;
    return plane[1] && plane[2] && pitch[1] >= Wc && pitch[2] >= Wc;
}

// (GRAY has kernels of its own for every format: on the way out I420 fills two chroma planes where NV12 fills one, so it cannot borrow NV12's)
hipError_t launch_image_yuv(const unsigned char* image, size_t ipitch, size_t istride, int order, int fmt, unsigned char* const* plane, const size_t* pitch,
                            const size_t* stride, int W, int H, int matrix, int B, hipStream_t st)
{
    const int D = order == 2 ? 1 : 3;
    if (!yo_args_ok(fmt, plane, pitch, stride, W, H, matrix, order, B) || !image || ipitch < (size_t)W * D) return hipErrorInvalidValue;
    const YoArgs g = yo_geometry(yo_dest(fmt, plane, pitch, stride, W, H, matrix, order, B), fmt, image, ipitch, istride, B);
    const unsigned tpi = (unsigned)(g.gx * g.gy);                                // at most 32 x 2048 blocks per image
    const dim3 gr(tpi, (unsigned)B < 65535u ? (unsigned)B : 65535u), bl(256);
#define YO_CASE(FF, DD) case ((FF) * 2 + ((DD) == 3)): image_yuv_kernel<FF, DD><<<gr, bl, 0, st>>>(g); break;
    switch (fmt * 2 + (D == 3)) {
        YO_CASE(0, 1) YO_CASE(0, 3) YO_CASE(1, 1) YO_CASE(1, 3) YO_CASE(2, 1) YO_CASE(2, 3)
        default: return hipErrorInvalidValue;
    }
#undef YO_CASE
    return hipGetLastError();
}

hipError_t launch_frames_yuv(const void* frames, bool f32, int Nx, int Ny, int mode, int order, int fmt, unsigned char* const* plane, const size_t* pitch,
                             const size_t* stride, int W, int H, int matrix, int B, hipStream_t st)
{
    const auto in = [](int v) { return v >= 1 && v <= 8192; };
    const int D = order == 2 ? 1 : 3;
    if (!yo_args_ok(fmt, plane, pitch, stride, W, H, matrix, order, B) || !frames || !in(Nx) || !in(Ny)) return hipErrorInvalidValue;
    if (mode != RZ_LINEAR && mode != RZ_AREA) return hipErrorInvalidValue;
    if (mode == RZ_AREA && (W > Nx || H > Ny)) return hipErrorInvalidValue;
    const FyArgs g = fy_geometry(yo_dest(fmt, plane, pitch, stride, W, H, matrix, order, B), fmt, frames, Nx, Ny, mode, B, D);
    // grid.x: the tiles of an image (at most 2^22); grid.y x grid.z: the images, image b = z grid.y + y (workgroups beyond B return at once)
    const unsigned by = (unsigned)B < 65535u ? (unsigned)B : 65535u;
    const dim3 gr((unsigned)g.tx * (unsigned)g.ty, by, ((unsigned)B + by - 1) / by), bl(256);
    const size_t lds = 4 * (size_t)fy_lds_words(D, g);
    if (lds > 65536) return hipErrorInvalidValue;                                // (cannot happen: at most 37 KiB by FY_BAND_WORDS)
#define FY_CASE(FF, DD, TT, MM) case ((FF) * 8 + ((DD) == 3) * 4 + (TT) * 2 + (MM)): frames_yuv_kernel<FF, DD, TT != 0, MM><<<gr, bl, lds, st>>>(g); break;
#define FY_CASES(FF, DD) FY_CASE(FF, DD, 0, 0) FY_CASE(FF, DD, 0, 1) FY_CASE(FF, DD, 1, 0) FY_CASE(FF, DD, 1, 1)
    switch (fmt * 8 + (D == 3) * 4 + (f32 ? 2 : 0) + mode) {
        FY_CASES(0, 1) FY_CASES(0, 3) FY_CASES(1, 1) FY_CASES(1, 3) FY_CASES(2, 1) FY_CASES(2, 3)
        default: return hipErrorInvalidValue;
    }
#undef FY_CASES
#undef FY_CASE
    return hipGetLastError();
}
#endif

}  // namespace aefft
