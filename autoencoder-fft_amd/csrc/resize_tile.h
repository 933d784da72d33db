// The phases that the four tile bodies which resize through a staged band in LDS have in common, stated ONCE: the defining integer arithmetic of
// include/aefft.h (the band sums and both roundings) in device code.
//   way in   resize_body (resize_kernels.hip, image -> frames) and yuv_body (yuv_kernels.hip, YUV -> frames): everything behind the staging of a
//            band -- rz_band_sums, the LINEAR / AREA loops of a lane's block over one band, and rz_store_block, the rounding and the stores
//   way out  frames_resize_body (present_kernels.hip, frames -> image) and frames_yuv_body (yuv_out_kernels.hip, frames -> YUV): steps 2 and 3
//            of present_kernels.hip's head, behind the taps -- fr_stage_runs, the runs of a band from the frames; fr_band_sums, a lane's sums over one band; fr_round_tile, the
//            rounding into the tile image -- with the tile constants PR_* and pr_div_u8 / pr_ceil_div
// Each body keeps its own staging (way in), its own step 4 (way out), its control flow, its argument struct and its geometry; the helpers are
// function templates over scalars the bodies already hold in registers -- no template over the staging, no functor, no shared argument struct --
// and are inlined into the bodies (DESIGN.md sections 20 and 21 have the argument for each step, section 23 the register tables before and after).
// Plain C++ over what the including file brings: RZ_HD and RZ_UNIFORM (its qualifier macros), and from HIP -- or, for the four host-check programs
// (tools/resize_, yuv_, present_, yuv_out_hostcheck.cpp), from tools/hostlanes.h -- __device__, __forceinline__, float4 / make_float4 and px_u8
// (fft_common.h, included here unless AEFFT_HOSTCHECK is defined).  No helper reads threadIdx or blockIdx: the lane comes in as a scalar.
#pragma once
#ifndef AEFFT_HOSTCHECK
#include "fft_common.h"                          // px_u8
#endif
#include "resize_taps.h"

namespace aefft {

// ---- way in: a band of source rows in IMAGE order -> a lane's block of 4 destination rows --------------
// The lane's block is column c = i D + d (tap X; col: the column's first byte of the band's row 0) x rows 4 q .. 4 q + 3 of the tile (taps yt, nrows
// of them live; own: the block has a live row).  The band holds the source rows [yb, yb + nr) at P dwords each.  acc runs across the bands.
template <int D, int MODE, typename acc_t>
__device__ __forceinline__ void rz_band_sums(const RzTap& X, const RzTap* yt, const unsigned char* col, int P, int q, int nrows, bool own, int yb, int nr,
                                             int Nx, int Ny, acc_t (&acc)[4])
{
    if (MODE == RZ_LINEAR) {
        // LINEAR: a destination row has one or two source rows.  The lane takes its four destination rows one after the other; the horizontal
        // sum of a source row is formed once and kept for the next destination row when that starts on the same source row (y1 = y0')
        int h_row = -1;
        unsigned h = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const RzTap Y = yt[rz_min(4 * q + k, nrows - 1)];
            const int cnt = 4 * q + k < nrows ? Y.cnt : 0;                       // (a row beyond the tile, a lane without a block: no trips)
#pragma unroll 1
            for (int r = 0; r < cnt; ++r) {
                const int y = Y.lo + r - yb;
                const bool in = (unsigned)y < (unsigned)nr;                      // (false: a row of another band)
                if (in && y != h_row) {
                    const unsigned char* p = col + 4 * y * P;
                    h = (unsigned)X.wf * p[0];
                    if (X.cnt > 1) h += (unsigned)X.wl * p[D];
                    h_row = y;
                }
                acc[k] += (acc_t)(!in ? 0u : (r == 0 ? (unsigned)Y.wf : (unsigned)Y.wl)) * h;
            }
        }
    } else {
        // AREA: the lane runs ONCE over the source rows of its block; a row's horizontal sum goes to the one or two destination rows it overlaps
        RzTap Y[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) Y[k] = yt[rz_min(4 * q + k, nrows - 1)];
        const int y_first = Y[0].lo, y_end = own ? Y[3].lo + Y[3].cnt : 0;       // (Y[3]: the block's last live row)
#pragma unroll
        for (int k = 1; k < 4; ++k)
            if (4 * q + k >= nrows) Y[k].cnt = 0;
#pragma unroll 1
        for (int y = rz_max(y_first, yb); y < rz_min(y_end, yb + nr); ++y) {
            const unsigned char* p = col + 4 * (y - yb) * P;
            unsigned h = (unsigned)X.wf * p[0];
#pragma unroll 1
            for (int x = 1; x < X.cnt - 1; ++x) h += (unsigned)Nx * p[x * D];
            if (X.cnt > 1) h += (unsigned)X.wl * p[(X.cnt - 1) * D];
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] += (acc_t)(unsigned)rz_weight(Y[k], y, Ny) * h;
        }
    }
}

// the block's four sums, rounded (wh = W H, the AREA divisor), to frames[o .. o + 3]: one dword of 8-bit pixels or one float4 when Ny % 4 == 0
// (frm_words), the live rows as single elements otherwise.  (The sums by VALUE: taken as a reference to the body's array, the select chain around
// the one 64-bit division cost every AREA kernel 8 instructions more than with the text in the body)
template <bool F32, int MODE, typename acc_t>
__device__ __forceinline__ void rz_store_block(acc_t acc0, acc_t acc1, acc_t acc2, acc_t acc3, unsigned long long wh, void* frames, size_t o, bool frm_words,
                                               int q, int nrows)
{
    const acc_t acc[4] = {acc0, acc1, acc2, acc3};
    unsigned px[4] = {0u, 0u, 0u, 0u};                                           // 8-bit frames: the pixel; float frames: value * 2^16 (< 2^24)
    if (MODE == RZ_LINEAR) {
#pragma unroll
        for (int k = 0; k < 4; ++k) px[k] = F32 ? (unsigned)((acc[k] + 32u) >> 6) : (unsigned)((acc[k] + (1u << 21)) >> 22);
    } else {
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {                                            // (one copy of the 64-bit division; the selects keep acc and px in registers)
            const unsigned long long num = k == 0 ? acc[0] : k == 1 ? acc[1] : k == 2 ? acc[2] : acc[3];
            const unsigned v = F32 ? (unsigned)((65536ull * num + wh / 2) / wh) : (unsigned)((2 * num + wh) / (2 * wh));
            px[0] = k == 0 ? v : px[0]; px[1] = k == 1 ? v : px[1]; px[2] = k == 2 ? v : px[2]; px[3] = k == 3 ? v : px[3];
        }
    }
    if (F32) {
        float* f = static_cast<float*>(frames) + o;
        const float s = 1.0f / 65536.0f;
        if (frm_words) *reinterpret_cast<float4*>(f) = make_float4((float)px[0] * s, (float)px[1] * s, (float)px[2] * s, (float)px[3] * s);
        else
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * q + k < nrows) f[k] = (float)px[k] * s;
    } else {
        unsigned char* f = static_cast<unsigned char*>(frames) + o;
        if (frm_words) *reinterpret_cast<unsigned*>(f) = px[0] | px[1] << 8 | px[2] << 16 | px[3] << 24;
        else
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * q + k < nrows) f[k] = (unsigned char)px[k];
    }
}

// ---- way out: a band of source columns in FRAME order -> a lane's byte column of the tile image --------
constexpr int PR_TY = 32;                        // destination rows of a full tile
constexpr int PR_CW = 64;                        // bytes of a full tile row: a wave's lanes, one byte column each
constexpr int PR_NH = 256 / PR_CW;               // waves of the workgroup: wave h owns the rows h, h + 4, h + 8, ...
constexpr int PR_RPL = PR_TY / PR_NH;            // rows of the tile a lane owns: 8
RZ_HD int pr_ceil_div(int a, int b) { return (a + b - 1) / b; }
// 0 <= q = floor(n / den) <= 255 without a 64-bit division: a float estimate (off by one at most), then corrected exactly
RZ_HD unsigned pr_div_u8(unsigned long long n, unsigned long long den)
{
    unsigned q = (unsigned)((float)n / (float)den);
    q = q > 255u ? 255u : q;
    while ((unsigned long long)q * den > n) --q;
    while ((unsigned long long)(q + 1) * den <= n) ++q;
    return q;
}

// run n = (x - xb) D + d of the band: the bytes frames[b][d][x][ya ..] of the source columns [xb, xb + nxb) at dword n P.  Consecutive lanes:
// consecutive units of a run -- a dword (a float4 of float frames, px_u8 on the way in) when Ny % 4 == 0 (frm_words), an element otherwise; nru
// of them, counted off in 2^ush --, then the next run
template <int D, bool F32>
__device__ __forceinline__ void fr_stage_runs(int tid, const void* frames, size_t b, int Nx, int Ny, int xb, int nxb, int ya, int nru, int ush, bool frm_words,
                                              int P, unsigned* band)
{
    unsigned char* bandb_w = reinterpret_cast<unsigned char*>(band);
#pragma unroll 2
    for (int idx = tid; idx < (D * nxb) << ush; idx += 256) {
        const int run = idx >> ush, u = idx & ((1 << ush) - 1), x = run / D, dd = run - x * D;
        if (u >= nru) continue;
        const size_t o = ((b * D + dd) * Nx + (xb + x)) * (size_t)Ny + ya + (frm_words ? 4 * u : u);   // (dwords: ya + 4 u + 3 < Ny, a multiple of 4)
        if (frm_words) {
            unsigned v;
            if (F32) {
                const float4 f = *reinterpret_cast<const float4*>(static_cast<const float*>(frames) + o);
                v = px_u8(f.x) | px_u8(f.y) << 8 | px_u8(f.z) << 16 | px_u8(f.w) << 24;
            } else v = *reinterpret_cast<const unsigned*>(static_cast<const unsigned char*>(frames) + o);
            band[run * P + u] = v;
        } else bandb_w[4 * run * P + u] = F32 ? (unsigned char)px_u8(static_cast<const float*>(frames)[o]) : static_cast<const unsigned char*>(frames)[o];
    }
}

// the lane's byte column (tap X, channel d) x the PR_RPL rows h, h + PR_NH, .. of the tile (taps yt, nrows of them live; h the same in a wave, so
// a row's taps are too: the loops over a run's rows are scalar loops) over the band's source columns [xb, xb + nxb).  For every source column of
// its tap the lane forms, per row, the vertical sum over the run (consecutive LDS bytes from row ya) and adds it times the column's weight.  The
// sums carry NO predicate that stays the same from band to band: a row slot beyond the tile's rows sums the last row again, and a tap's last
// weight is 0 when it is also its first.  W, H: the destination sizes (the weight of a tap's inner source indices).  acc runs across the bands.
// (X by VALUE: taken by reference, the x loop of every LINEAR kernel kept both range tests of rz_weight, 2-5 instructions more than with the text
// in the body; rz_band_sums compiles to fewer instructions with the reference)
template <int D, int MODE, typename acc_t>
__device__ __forceinline__ void fr_band_sums(const RzTap X, const RzTap* yt, const unsigned char* bandb, int P, int d, int h, int nrows, int xb, int nxb, int ya,
                                             int W, int H, acc_t (&acc)[PR_RPL])
{
    const int x_end = rz_min(X.lo + X.cnt, xb + nxb);
#pragma unroll 1
    for (int x = rz_max(X.lo, xb); x < x_end; ++x) {
        const unsigned char* run = bandb + 4 * ((x - xb) * D + d) * P - ya;
        const unsigned wx = (unsigned)rz_weight(X, x, W);
#pragma unroll
        for (int k = 0; k < PR_RPL; ++k) {
            const RzTap Y = yt[rz_min(PR_NH * k + h, nrows - 1)];                 // (the same in every lane of the wave)
            const int lo = Y.lo, cnt = MODE == RZ_AREA ? RZ_UNIFORM(Y.cnt) : Y.cnt, wf = Y.wf, wl = cnt > 1 ? Y.wl : 0;
            const unsigned char* p = run + lo;
            unsigned v = (unsigned)wf * p[0];                                    // the vertical sum of the run: at most 255 * 8192
            if (MODE == RZ_AREA)
#pragma unroll 1
                for (int y = 1; y < cnt - 1; ++y) v += (unsigned)H * p[y];
            v += (unsigned)wl * p[cnt - 1];
            acc[k] += (acc_t)wx * v;
        }
    }
}

// the lane's PR_RPL sums, rounded (nn = Nx Ny, the AREA divisor), to the tile image in LDS: row r = PR_NH k + h in slot PR_RPL h + k, column c
template <int MODE, typename acc_t>
__device__ __forceinline__ void fr_round_tile(const acc_t (&acc)[PR_RPL], unsigned long long nn, unsigned char* tileb, int h, int c)
{
#pragma unroll
    for (int k = 0; k < PR_RPL; ++k) {
        const unsigned px = MODE == RZ_LINEAR ? (unsigned)((acc[k] + (1u << 21)) >> 22) : pr_div_u8(2 * (unsigned long long)acc[k] + nn, 2 * nn);
        tileb[PR_CW * (h * PR_RPL + k) + c] = (unsigned char)px;
    }
}

}  // namespace aefft
