// aefft_image_resize_to_frames (gfx950): the reference loop's `resize(rgb, imgC, Size(Nx, Ny))` + ImageToSpin_C (autoencoder.cpp:124-125) in one
// launch -- B images of H rows of interleaved pixels, any W x H, to the library's planar [B][D][Nx][Ny] frames (y contiguous), 8-bit or float.
//   resize_kernel<D, F32, MODE>    MODE 0 LINEAR (cv::resize's default geometry, weights in 1/2048), MODE 1 AREA (the exact box average)
// All-integer arithmetic (include/aefft.h states the formulas): every route gives the same bits as a numpy restatement.
// Both filters are separable sums with per-axis taps of ONE form (rz_tap): destination index i reads source indices lo .. lo + cnt - 1 with
// weight wf on the first, wl on the last (cnt > 1) and N, the destination size, on those between:
//   LINEAR  lo = x0, cnt = 1 or 2, wf = 2048 - w, wl = w                       AREA  lo = floor(i S / N), the overlaps o(i, lo), N, .., N, o(i, hi)
// so one kernel serves both; the modes differ in rz_tap, the loop over a block's source rows, the accumulator's width (32 / 64 bits) and the rounding.
// A workgroup (256 threads) owns a tile of TI = 64 / D destination columns x 16 destination rows x all D channels of one image (DESIGN.md
// section 20).  Per tile: TI + 16 lanes write the tile's taps to LDS (once per tile, not per pixel); the source rows the tile needs, bytes
// [xs D, xe D) of each, are staged in LDS in IMAGE order with coalesced loads -- dwords when image_d, pitch and image_stride are multiples of 4
// (the dword that would cross the row's end W D is split into its live bytes), bytes otherwise -- in bands of RB rows: one band when the
// footprint fits the launch's LDS, several for large reduction ratios, the lanes' sums running across them.  A lane owns a block of 4 destination
// rows j of one column c = i D + d: it forms a source row's horizontal sum out of LDS once and adds it to the one or two rows j it belongs to
// (LINEAR: row by row of the destination, a shared source row kept; AREA: one run over the block's source rows); then it stores the 4 results as one dword of 8-bit pixels or one float4 when Ny % 4 == 0,
// as single elements otherwise.  Lanes run along c: the 32 lanes of an LDS lane group read ONE staged row at byte offsets lo(i) D + d, an
// ascending run of at most 32 r bytes (r = W / Nx), so the dwords they touch are consecutive and on different banks up to r = 4 whatever the LDS
// pitch (section 20 has the argument and what happens beyond).  No scratch, no atomics, no global byte gather on the aligned route.
// The kernel body is plain C++ over (threadIdx, blockIdx, gridDim, __syncthreads) and an LDS pointer: tools/resize_hostcheck.cpp compiles this
// file for the host, threads as lanes, under the sanitizers (AEFFT_HOSTCHECK: tools/hostlanes.h supplies those names and leaves the launcher out).
#include <type_traits>
#ifndef AEFFT_HOSTCHECK
#include "internal.h"
#define RZ_HD __host__ __device__ __forceinline__
#define RZ_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)
#endif
#include "resize_taps.h"                         // RzTap, rz_tap, rz_weight: the tap formulas, shared with present_kernels.hip
#include "resize_tile.h"                         // rz_band_sums, rz_store_block: the phases behind the staging, shared with yuv_kernels.hip

namespace aefft {

constexpr int RZ_TJ = 16;                        // destination rows of a tile: 4 blocks of 4, so TI D * 4 <= 256 blocks, one per lane
constexpr int RZ_MLP = 8;                        // source rows a wave has in flight while staging
constexpr int RZ_BAND_WORDS = 8704;              // dwords of staged source rows a workgroup holds (34 KiB: a row of 8192 x 4 bytes + its slack fits)
RZ_HD int rz_ti(int D) { return 64 / D; }        // destination columns of a tile: 64, 32, 21, 16

struct RzArgs {
    const unsigned char* image; size_t pitch, stride; void* frames;
    int W, H, Nx, Ny;
    int tx, ty, B;                               // tiles per image along x and y; images
    int P, RB;                                   // dwords of a staged row (odd); rows of a band
    bool img_words, frm_words;
};
// LDS of a launch, in dwords: the taps (TI + TJ of 4) and the band
RZ_HD int rz_lds_words(int D, int P, int RB) { return 4 * (rz_ti(D) + RZ_TJ) + P * RB; }

template <int D, bool F32, int MODE>
__device__ __forceinline__ void resize_body(const RzArgs& a, unsigned* lds)
{
    typedef typename std::conditional<MODE == RZ_AREA, unsigned long long, unsigned>::type acc_t;
    constexpr int TI = 64 / D;
    RzTap* xt = reinterpret_cast<RzTap*>(lds);
    RzTap* yt = xt + TI;
    unsigned* rows = lds + 4 * (TI + RZ_TJ);
    const unsigned char* rowb = reinterpret_cast<const unsigned char*>(rows);
    unsigned char* rowb_w = reinterpret_cast<unsigned char*>(rows);
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int rowlive = a.W * D;                                                 // bytes of a source row that may be read
    // grid.x: the tx ty tiles of an image (at most 2^18), grid.y: the images, folded onto at most 2^20 workgroups (uniform: a folded grid loops)
    for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
        const int ty_i = (int)blockIdx.x / a.tx;
        const int i0 = ((int)blockIdx.x - ty_i * a.tx) * TI, j0 = ty_i * RZ_TJ;
        const int ncols = rz_min(a.Nx - i0, TI), nrows = rz_min(a.Ny - j0, RZ_TJ);
        if (tid < ncols) xt[tid] = rz_tap(MODE, i0 + tid, a.W, a.Nx);
        else if (tid >= TI && tid < TI + nrows) yt[tid - TI] = rz_tap(MODE, j0 + tid - TI, a.H, a.Ny);
        __syncthreads();
        // source columns [xs, xe) and rows [ys, ye) of the tile (the same in every lane; the rows, which bound the band loop, in scalar registers)
        const int xs = xt[0].lo, xe = xt[ncols - 1].lo + xt[ncols - 1].cnt;
        const int ys = RZ_UNIFORM(yt[0].lo), ye = RZ_UNIFORM(yt[nrows - 1].lo + yt[nrows - 1].cnt);
        const int a0 = a.img_words ? (xs * D) & ~3 : xs * D;                     // first staged byte of a row
        const int nbytes = xe * D - a0, nw = (nbytes + 3) >> 2;                  // (nw <= P: the launcher sized P over every tile)
        const unsigned char* src = a.image + (size_t)b * a.stride + a0;
        // the lane's block: column c = i D + d (lanes run along c), rows 4 q .. 4 q + 3 of the tile
        const int tc = ncols * D;
        const int q = tid / tc, c = tid - q * tc, i = c / D, d = c - i * D;
        const bool own = 4 * q < nrows;
        const RzTap X = xt[i];
        const unsigned char* col = rowb + (X.lo * D + d - a0);
        acc_t acc[4] = {0, 0, 0, 0};
        for (int yb = ys; yb < ye; yb += a.RB) {
            const int nr = rz_min(a.RB, ye - yb);
            // a wave per staged row, its lanes along the row: consecutive lanes load consecutive dwords (bytes).  A wave takes RZ_MLP rows at a
            // time, all their loads issued before the first LDS store, so that a row's latency is paid once per RZ_MLP rows (rows beyond the band
            // repeat its last row: the same value to the same place)
            if (a.img_words) {
                const int nwf = rz_min(nw, (rowlive - a0) >> 2);                 // whole dwords of a row; at most one more crosses the row's end W D
#pragma unroll 1
                for (int r0 = wave; r0 < nr; r0 += 4 * RZ_MLP) {
#pragma unroll 1
                    for (int w = lane; w < nwf; w += 64) {
                        unsigned v[RZ_MLP];
#pragma unroll
                        for (int k = 0; k < RZ_MLP; ++k) v[k] = *reinterpret_cast<const unsigned*>(src + (size_t)(yb + rz_min(r0 + 4 * k, nr - 1)) * a.pitch + 4 * w);
#pragma unroll
                        for (int k = 0; k < RZ_MLP; ++k) rows[rz_min(r0 + 4 * k, nr - 1) * a.P + w] = v[k];
                    }
                }
                if (nwf < nw) {                                                  // (that dword: its live bytes only)
                    const int live = rowlive - a0 - 4 * nwf;
#pragma unroll 1
                    for (int rr = tid; rr < nr; rr += 256) {
                        const unsigned char* p = src + (size_t)(yb + rr) * a.pitch + 4 * nwf;
                        unsigned v = 0;
                        for (int e = 0; e < live; ++e) v |= (unsigned)p[e] << (8 * e);
                        rows[rr * a.P + nwf] = v;
                    }
                }
            } else {
#pragma unroll 1
                for (int r0 = wave; r0 < nr; r0 += 4 * RZ_MLP) {
#pragma unroll 1
                    for (int cb = lane; cb < nbytes; cb += 64) {
                        unsigned char v[RZ_MLP];
#pragma unroll
                        for (int k = 0; k < RZ_MLP; ++k) v[k] = src[(size_t)(yb + rz_min(r0 + 4 * k, nr - 1)) * a.pitch + cb];
#pragma unroll
                        for (int k = 0; k < RZ_MLP; ++k) rowb_w[4 * rz_min(r0 + 4 * k, nr - 1) * a.P + cb] = v[k];
                    }
                }
            }
            __syncthreads();
            rz_band_sums<D, MODE>(X, yt, col, a.P, q, nrows, own, yb, nr, a.Nx, a.Ny, acc);
            __syncthreads();
        }
        if (!own) continue;
        const size_t o = (((size_t)b * D + d) * a.Nx + (i0 + i)) * (size_t)a.Ny + (j0 + 4 * q);
        rz_store_block<F32, MODE>(acc[0], acc[1], acc[2], acc[3], (unsigned long long)a.W * a.H, a.frames, o, a.frm_words, q, nrows);
    }
}

// the launch geometry: tiles, the staged row's dwords P (the widest tile's, made odd) and the band's rows RB (the tallest tile's footprint, or what
// RZ_BAND_WORDS holds of it).  Exact, from the same rz_tap the kernel uses: at most 8192 / TI + 8192 / 16 tiles' end taps.
static inline RzArgs rz_geometry(const unsigned char* image, size_t pitch, size_t stride, int W, int H, int mode, void* frames, int B, int D, int Nx, int Ny)
{
    RzArgs g;
    g.image = image; g.pitch = pitch; g.stride = B > 1 ? stride : 0; g.frames = frames;
    g.W = W; g.H = H; g.Nx = Nx; g.Ny = Ny;
    const int TI = rz_ti(D);
    g.tx = (Nx + TI - 1) / TI; g.ty = (Ny + RZ_TJ - 1) / RZ_TJ;
    g.B = B;
    g.img_words = ((reinterpret_cast<uintptr_t>(image) | pitch | g.stride) & 3u) == 0;
    g.frm_words = (Ny & 3) == 0;
    int nw = 1, nr = 1;
    for (int t = 0; t < g.tx; ++t) {
        const RzTap f = rz_tap(mode, t * TI, W, Nx), l = rz_tap(mode, rz_min(t * TI + TI, Nx) - 1, W, Nx);
        const int a0 = g.img_words ? (f.lo * D) & ~3 : f.lo * D;
        nw = rz_max(nw, ((l.lo + l.cnt) * D - a0 + 3) >> 2);
    }
    for (int t = 0; t < g.ty; ++t) {
        const RzTap f = rz_tap(mode, t * RZ_TJ, H, Ny), l = rz_tap(mode, rz_min(t * RZ_TJ + RZ_TJ, Ny) - 1, H, Ny);
        nr = rz_max(nr, l.lo + l.cnt - f.lo);
    }
    g.P = nw | 1;
    g.RB = rz_max(1, rz_min(nr, RZ_BAND_WORDS / g.P));
    return g;
}

#ifndef AEFFT_HOSTCHECK
template <int D, bool F32, int MODE>
__global__ __launch_bounds__(256) void resize_kernel(const RzArgs a)
{
    extern __shared__ unsigned rz_lds[];
    resize_body<D, F32, MODE>(a, rz_lds);
}

hipError_t launch_image_resize(const unsigned char* image, size_t pitch, size_t stride, int W, int H, int mode, void* frames, bool f32,
                               int B, int D, int Nx, int Ny, hipStream_t st)
{
    const auto in = [](int v) { return v >= 1 && v <= 8192; };
    if (!image || !frames || B < 1 || D < 1 || D > 4 || !in(W) || !in(H) || !in(Nx) || !in(Ny) || pitch < (size_t)W * D) return hipErrorInvalidValue;
    if (mode != RZ_LINEAR && mode != RZ_AREA) return hipErrorInvalidValue;
    if (mode == RZ_AREA && (Nx > W || Ny > H)) return hipErrorInvalidValue;
    const RzArgs g = rz_geometry(image, pitch, stride, W, H, mode, frames, B, D, Nx, Ny);
    const unsigned tpi = (unsigned)(g.tx * g.ty), by = (1u << 20) / tpi < 65535u ? (1u << 20) / tpi : 65535u;
    const dim3 gr(tpi, (unsigned)B < by ? (unsigned)B : by), bl(256);
    const size_t lds = 4 * (size_t)rz_lds_words(D, g.P, g.RB);
#define RZ_CASE(DD, FF, MM) case ((DD) * 4 + (FF) * 2 + (MM)): resize_kernel<DD, FF != 0, MM><<<gr, bl, lds, st>>>(g); break;
#define RZ_CASES(DD) RZ_CASE(DD, 0, 0) RZ_CASE(DD, 0, 1) RZ_CASE(DD, 1, 0) RZ_CASE(DD, 1, 1)
    switch (D * 4 + (f32 ? 2 : 0) + mode) {
        RZ_CASES(1) RZ_CASES(2) RZ_CASES(3) RZ_CASES(4)
        default: return hipErrorInvalidValue;
    }
#undef RZ_CASES
#undef RZ_CASE
    return hipGetLastError();
}
#endif

}  // namespace aefft
