// Error and SSIM maps of two interleaved 8-bit images at the image's own resolution (aefft_image_compare_map, gfx950; include/aefft.h has the
// definition, DESIGN.md section 26 the layout and the measurement).  Two images a, b of W x H pixels of D channels are compared cell by cell on a
// grid of Mx x My cells -- cell I holds the columns [ceil(I W / Mx), ceil((I+1) W / Mx)), the pixels x with floor(x Mx / W) = I, which is what
// aefft_map_overlay_image(smooth = 0) colours with entry I --:
//   compare_map_kernel<D, METRIC>   the two images -> map [B][Mx][My]: the mean squared error, or the mean over the channels of the SSIM, of each cell
//   compare_score_kernel            map -> score [B]: the pixel-weighted mean of the map as stored, added in one fixed order in double
// A streaming reduction: every byte of both images is read once, all sums are integers (any order of adding gives the same value), and the handful of
// double operations behind them is stated in the header, so tests/compare_ref.py gives the same bits.
//   work     a workgroup owns cell row J of one image (at most 64 image rows) and a span of `cpw` neighbouring cells.  A lane owns ONE dword of ONE
//            cell -- bytes 4 w .. 4 w + 3 of the row, counted from the row's first byte -- over every rg-th row: the lanes of a workgroup run along
//            the contiguous bytes of a row, `items` = cpw nwc of them, and the 256 / items lane groups take the rows in turn.  A cell starts at
//            an arbitrary byte, so the dword on a boundary is loaded by a lane of either cell and each keeps its own bytes (a per-lane mask that
//            the rows share); the second load comes out of the cache.  For SSIM the mask splits once more by channel -- the channel of row byte o
//            is o mod D, for D = 3 a pattern with a period of three dwords --, so a lane keeps D x 5 integer moments and each is one
//            v_dot4_u32_u8 per row: Sx = dot(x & m, 0x01010101), Sxx = dot(x & m, x & m), Sxr = dot(x & m, r & m).  MSE keeps
//            sum x^2 + sum r^2 and sum x r and forms e = (sum x^2 + sum r^2) - 2 sum x r once (modulo 2^32: e itself is below 2^31).
//   loads    each image on its own: ALIGNED dwords when its pointer, pitch and stride are multiples of 4 (then every row starts on a dword), single
//            bytes put together in the same order otherwise; the dword that crosses the row's end is read byte by byte up to W D on either route,
//            so bytes beyond W D of a row are never read and every combination of routes gives the same bits.
//   sums     no atomics anywhere: every lane leaves its sums in LDS ([k][lane]: consecutive lanes, consecutive banks), behind a barrier ONE lane
//            adds up sum k of cell c from the cell's nwc x rg lanes (at most 4096 x 65025 < 2^32), and behind a second one lane a (cell, channel)
//            forms the channel's SSIM -- the signed 64-bit factors of the header, four conversions, two products and one division in double --;
//            for D > 1 the channels of a cell meet in LDS once more and one lane a cell adds them in ascending d and stores the entry.  A cell
//            belongs to one workgroup.  LDS: 256 x (5 D or 1) words for the lanes + at most 128 (D = 1: 256) x (5 D or 1) for the cells, 30 KiB
//            at D = 4.
//   score    one workgroup an image: lane I adds m[I][J] n_IJ along J in double (each product is exact), lane 0 adds the r_I along I.
// tools/compare_hostcheck.cpp compiles this file for the host, threads as lanes, under the sanitizers (AEFFT_HOSTCHECK: tools/hostlanes.h supplies
// the launch variables and the barrier; the dot product has its host form below).
#ifndef AEFFT_HOSTCHECK
#include "internal.h"
#include "fft_common.h"
#define CM_HD __device__ __forceinline__
#endif

namespace aefft {

constexpr int CM_MSE = 0, CM_SSIM = 1;                                           // AEFFT_COMPARE_MSE, AEFFT_COMPARE_SSIM
constexpr int CM_SIDE = 64;                                                      // the largest side of a cell
constexpr int CM_CELLS = 1024;                                                   // the most cells along an axis
constexpr int CM_LANES = 256;
constexpr int CM_MOMENTS = 5;                                                    // Sx, Sr, Sxx, Srr, Sxr

#ifndef AEFFT_HOSTCHECK
CM_HD unsigned cm_dot4(unsigned a, unsigned b, unsigned c) { return __builtin_amdgcn_udot4(a, b, c, false); }   // c + sum of the four byte products
#else
CM_HD unsigned cm_dot4(unsigned a, unsigned b, unsigned c)
{
    for (int k = 0; k < 4; ++k) c += ((a >> (8 * k)) & 255u) * ((b >> (8 * k)) & 255u);
    return c;
}
#endif

struct CmArgs {
    const unsigned char *a, *b; size_t a_pitch, a_stride, b_pitch, b_stride;     // B images each (the strides are 0 for B == 1)
    float* map;                                                                  // [B][Mx][My]
    int W, H, Mx, My;
    int nwc;                                                                     // the dwords a cell's bytes can touch at most
    int cpw, spans;                                                              // cells of a workgroup, workgroups along a cell row (grid.x)
    int items, rg;                                                               // cpw nwc lanes along a row, 256 / items lane groups over the rows
    int units;                                                                   // the B My cell rows (grid.y x grid.z)
    int a_words, b_words;
};

// the first column (row) of cell I of M on an axis of W: ceil(I W / M); I W <= 2^23
CM_HD int cm_edge(int I, int W, int M) { return (I * W + M - 1) / M; }

template <int D, int METRIC> struct CmLds {
    static constexpr int ACC = METRIC == CM_SSIM ? CM_MOMENTS * D : 1;           // sums of a lane, and of a cell
    static constexpr int PART = CM_LANES * ACC;                                  // the lanes' sums, [k][lane]; later the channels' SSIM as doubles
    static constexpr int CPW = CM_LANES / ((D + 2) / 4 + 1);                     // cells of a workgroup at most: a cell has D bytes or more, nwc >= (D + 2) / 4 + 1
    static constexpr int WORDS = PART + CPW * ACC;                               // ... + the cells' sums, [k][cell]
};

// row bytes o .. o + 3, of which n (>= 1) lie inside the row: one aligned dword, or the live bytes one by one
CM_HD unsigned cm_load(const unsigned char* p, int n, int words)
{
    if (words && n >= 4) return *reinterpret_cast<const unsigned*>(p);
    unsigned v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < n) v |= (unsigned)p[k] << (8 * k);
    return v;
}

// one channel's SSIM of a cell of n pixels from its five sums: the signed 64-bit factors of the header, four conversions, two products, one division
CM_HD double cm_ssim(long long n, long long Sx, long long Sr, long long Sxx, long long Srr, long long Sxr)
{
    const long long K1 = 65025, K2 = 585225;                                      // 10000 C1, 10000 C2 at a data range of 255
    const long long A1 = 20000 * Sx * Sr + K1 * n * n, A2 = 20000 * (n * Sxr - Sx * Sr) + K2 * n * n;
    const long long B1 = 10000 * (Sx * Sx + Sr * Sr) + K1 * n * n, B2 = 10000 * (n * Sxx - Sx * Sx + n * Srr - Sr * Sr) + K2 * n * n;
    return ((double)A1 * (double)A2) / ((double)B1 * (double)B2);
}

template <int D, int METRIC>
CM_HD void compare_map_body(const CmArgs& g, unsigned span, unsigned unit, unsigned* lds)
{
    typedef CmLds<D, METRIC> L;
    constexpr int ACC = L::ACC;
    const int tid = (int)threadIdx.x;
    const unsigned bi = unit / (unsigned)g.My;
    const int J = (int)(unit - bi * g.My), y0 = cm_edge(J, g.H, g.My), y1 = cm_edge(J + 1, g.H, g.My);
    const int I0 = (int)span * g.cpw, nc = g.Mx - I0 < g.cpw ? g.Mx - I0 : g.cpw;
    const int grp = tid / g.items, item = tid - grp * g.items, ci = item / g.nwc, w = item - ci * g.nwc;
    unsigned acc[ACC];
#pragma unroll
    for (int k = 0; k < ACC; ++k) acc[k] = 0;
    if (grp < g.rg && ci < nc) {
        const int c0 = cm_edge(I0 + ci, g.W, g.Mx) * D, c1 = cm_edge(I0 + ci + 1, g.W, g.Mx) * D;      // the cell's bytes of a row
        const int o = 4 * ((c0 >> 2) + w);                                       // this lane's dword
        if (o < c1) {
            unsigned cell = 0;                                                    // the bytes of the dword that are the cell's
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (o + k >= c0 && o + k < c1) cell |= 255u << (8 * k);
            const int n = g.W * D - o;                                            // (>= 1: o < c1 <= W D)
            const unsigned char* pa = g.a + (size_t)bi * g.a_stride + (size_t)o;
            const unsigned char* pb = g.b + (size_t)bi * g.b_stride + (size_t)o;
            if constexpr (METRIC == CM_MSE) {
                unsigned cross = 0;
#pragma unroll 4
                for (int y = y0 + grp; y < y1; y += g.rg) {
                    const unsigned x = cm_load(pa + (size_t)y * g.a_pitch, n, g.a_words) & cell, r = cm_load(pb + (size_t)y * g.b_pitch, n, g.b_words) & cell;
                    acc[0] = cm_dot4(x, x, acc[0]);
                    acc[0] = cm_dot4(r, r, acc[0]);
                    cross = cm_dot4(x, r, cross);
                }
                acc[0] -= 2u * cross;
            } else {
                unsigned m[D];                                                    // ... and of channel d: row byte o + k has channel (o + k) mod D
                const int ph = o % D;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    m[d] = 0;
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if ((ph + k) % D == d) m[d] |= 255u << (8 * k);
                    m[d] &= cell;
                }
#pragma unroll 4
                for (int y = y0 + grp; y < y1; y += g.rg) {
                    const unsigned x = cm_load(pa + (size_t)y * g.a_pitch, n, g.a_words), r = cm_load(pb + (size_t)y * g.b_pitch, n, g.b_words);
#pragma unroll
                    for (int d = 0; d < D; ++d) {
                        const unsigned xd = x & m[d], rd = r & m[d];
                        acc[CM_MOMENTS * d + 0] = cm_dot4(xd, 0x01010101u, acc[CM_MOMENTS * d + 0]);
                        acc[CM_MOMENTS * d + 1] = cm_dot4(rd, 0x01010101u, acc[CM_MOMENTS * d + 1]);
                        acc[CM_MOMENTS * d + 2] = cm_dot4(xd, xd, acc[CM_MOMENTS * d + 2]);
                        acc[CM_MOMENTS * d + 3] = cm_dot4(rd, rd, acc[CM_MOMENTS * d + 3]);
                        acc[CM_MOMENTS * d + 4] = cm_dot4(xd, rd, acc[CM_MOMENTS * d + 4]);
                    }
                }
            }
        }
    }
    // every lane leaves its sums (zeros where it had no bytes), sum k of lane t at [k][t]; then sum k of cell c is added up by ONE lane, into [k][c]
#pragma unroll
    for (int k = 0; k < ACC; ++k) lds[k * CM_LANES + tid] = acc[k];
    __syncthreads();
    unsigned* sums = lds + L::PART;
    for (int t = tid; t < nc * ACC; t += CM_LANES) {
        const int k = t / nc, c = t - k * nc;
        const unsigned* q = lds + k * CM_LANES + c * g.nwc;
        unsigned s = 0;
        for (int gr = 0; gr < g.rg; ++gr)
            for (int i = 0; i < g.nwc; ++i) s += q[gr * g.items + i];
        sums[t] = s;
    }
    __syncthreads();
    const long long ny = y1 - y0;
    float* out = g.map + (size_t)bi * g.Mx * (size_t)g.My + J;                    // entry (I, J) of this image at out[I My]
    if constexpr (METRIC == CM_MSE) {
        for (int c = tid; c < nc; c += CM_LANES) {
            const long long n = (cm_edge(I0 + c + 1, g.W, g.Mx) - cm_edge(I0 + c, g.W, g.Mx)) * ny;   // the cell's pixels, <= 4096
            out[(size_t)(I0 + c) * g.My] = (float)((double)sums[c] / (double)(D * n));
        }
    } else {
        double* ssim = reinterpret_cast<double*>(lds);                            // (the lanes' sums are spent) [cell][d]: one lane a channel
        for (int t = tid; t < nc * D; t += CM_LANES) {
            const int c = t / D, d = t - c * D;
            const long long n = (cm_edge(I0 + c + 1, g.W, g.Mx) - cm_edge(I0 + c, g.W, g.Mx)) * ny;
            const unsigned* q = sums + CM_MOMENTS * d * nc + c;
            const double v = cm_ssim(n, q[0], q[nc], q[2 * nc], q[3 * nc], q[4 * nc]);
            if constexpr (D == 1) out[(size_t)(I0 + c) * g.My] = (float)v;
            else ssim[t] = v;
        }
        if constexpr (D > 1) {
            __syncthreads();
            for (int c = tid; c < nc; c += CM_LANES) {
                double s = ssim[c * D];
#pragma unroll
                for (int d = 1; d < D; ++d) s += ssim[c * D + d];
                out[(size_t)(I0 + c) * g.My] = (float)(s / (double)D);
            }
        }
    }
}

// score[b] = (float)(S / (W H)), S = ((r_0 + r_1) + ...) along I, r_I = ((m[I][0] n_I0 + m[I][1] n_I1) + ...) along J, n_IJ the pixels of cell (I, J);
// lds: CM_CELLS doubles (the r_I) and CM_CELLS ints (the rows of the cells along J)
CM_HD void compare_score_body(const float* map, float* score, int W, int H, int Mx, int My, unsigned bi, double* lds)
{
    const int tid = (int)threadIdx.x;
    int* rows = reinterpret_cast<int*>(lds + CM_CELLS);
    for (int J = tid; J < My; J += CM_LANES) rows[J] = cm_edge(J + 1, H, My) - cm_edge(J, H, My);
    __syncthreads();
    for (int I = tid; I < Mx; I += CM_LANES) {
        const int nx = cm_edge(I + 1, W, Mx) - cm_edge(I, W, Mx);
        const float* m = map + ((size_t)bi * Mx + I) * (size_t)My;
        double r = (double)m[0] * (double)(nx * rows[0]);                         // (every product is exact: 24 bits by 13)
#pragma unroll 8
        for (int J = 1; J < My; ++J) r += (double)m[J] * (double)(nx * rows[J]);
        lds[I] = r;
    }
    __syncthreads();
    if (tid == 0) {
        double S = lds[0];
        for (int I = 1; I < Mx; ++I) S += lds[I];
        score[bi] = (float)(S / (double)(W * H));
    }
}

// the launch geometry; false for what the kernels do not serve
static inline bool cm_geometry(const unsigned char* a, size_t a_pitch, size_t a_stride, const unsigned char* b, size_t b_pitch, size_t b_stride, int W, int H,
                               int B, int D, int Mx, int My, float* map, CmArgs* g)
{
    if (!a || !b || !map || W < 1 || W > 8192 || H < 1 || H > 8192 || B < 1 || D < 1 || D > 4 || Mx < 1 || Mx > W || Mx > CM_CELLS || My < 1 || My > H ||
        My > CM_CELLS) return false;
    const int sx = (W + Mx - 1) / Mx, sy = (H + My - 1) / My;
    if (sx > CM_SIDE || sy > CM_SIDE || a_pitch < (size_t)W * D || b_pitch < (size_t)W * D || (long long)B * My > 0x7fffffffLL) return false;
    g->a = a; g->a_pitch = a_pitch; g->a_stride = B > 1 ? a_stride : 0;
    g->b = b; g->b_pitch = b_pitch; g->b_stride = B > 1 ? b_stride : 0;
    g->map = map; g->W = W; g->H = H; g->Mx = Mx; g->My = My;
    g->nwc = (sx * D + 2) / 4 + 1;                                               // sx D bytes from an arbitrary byte on: at most 65 dwords
    const int most = CM_LANES / g->nwc < Mx ? CM_LANES / g->nwc : Mx;            // (>= 3) cells whose dwords fit the workgroup's lanes ...
    g->spans = (Mx + most - 1) / most;
    g->cpw = (Mx + g->spans - 1) / g->spans;                                     // ... levelled over the spans
    g->items = g->cpw * g->nwc;
    g->rg = CM_LANES / g->items;
    g->units = B * My;
    g->a_words = ((reinterpret_cast<uintptr_t>(a) | a_pitch | g->a_stride) & 3u) == 0;
    g->b_words = ((reinterpret_cast<uintptr_t>(b) | b_pitch | g->b_stride) & 3u) == 0;
    return true;
}
static inline unsigned cm_grid_y(const CmArgs& g) { return (unsigned)(g.units < 65535 ? g.units : 65535); }   // unit = z grid.y + y (workgroups beyond return at once)
static inline unsigned cm_grid_z(const CmArgs& g) { return ((unsigned)g.units + cm_grid_y(g) - 1) / cm_grid_y(g); }

#ifndef AEFFT_HOSTCHECK
template <int D, int METRIC>
__global__ __launch_bounds__(CM_LANES) void compare_map_kernel(const CmArgs g)
{
    __shared__ __attribute__((aligned(16))) unsigned lds[CmLds<D, METRIC>::WORDS];   // (doubles live in it too)
    const unsigned u = blockIdx.z * gridDim.y + blockIdx.y;
    if (u < (unsigned)g.units) compare_map_body<D, METRIC>(g, blockIdx.x, u, lds);
}

__global__ __launch_bounds__(CM_LANES) void compare_score_kernel(const float* map, float* score, int W, int H, int Mx, int My)
{
    __shared__ double lds[CM_CELLS + CM_CELLS / 2];
    compare_score_body(map, score, W, H, Mx, My, blockIdx.x, lds);
}

hipError_t launch_compare_map(const unsigned char* a, size_t a_pitch, size_t a_stride, const unsigned char* b, size_t b_pitch, size_t b_stride, int W, int H,
                              int B, int D, int metric, int Mx, int My, float* map, hipStream_t st)
{
    CmArgs g;
    if ((metric != CM_MSE && metric != CM_SSIM) || !cm_geometry(a, a_pitch, a_stride, b, b_pitch, b_stride, W, H, B, D, Mx, My, map, &g)) return hipErrorInvalidValue;
    const dim3 gr((unsigned)g.spans, cm_grid_y(g), cm_grid_z(g)), bl(CM_LANES);
    switch (D * 2 + metric) {
        case 2: compare_map_kernel<1, CM_MSE><<<gr, bl, 0, st>>>(g); break;
        case 3: compare_map_kernel<1, CM_SSIM><<<gr, bl, 0, st>>>(g); break;
        case 4: compare_map_kernel<2, CM_MSE><<<gr, bl, 0, st>>>(g); break;
        case 5: compare_map_kernel<2, CM_SSIM><<<gr, bl, 0, st>>>(g); break;
        case 6: compare_map_kernel<3, CM_MSE><<<gr, bl, 0, st>>>(g); break;
        case 7: compare_map_kernel<3, CM_SSIM><<<gr, bl, 0, st>>>(g); break;
        case 8: compare_map_kernel<4, CM_MSE><<<gr, bl, 0, st>>>(g); break;
        default: compare_map_kernel<4, CM_SSIM><<<gr, bl, 0, st>>>(g); break;
    }
    return hipGetLastError();
}

hipError_t launch_compare_score(const float* map, float* score, int W, int H, int B, int Mx, int My, hipStream_t st)
{
    if (!map || !score || B < 1 || W < 1 || H < 1 || Mx < 1 || Mx > CM_CELLS || Mx > W || My < 1 || My > H) return hipErrorInvalidValue;
    compare_score_kernel<<<dim3((unsigned)B), dim3(CM_LANES), 0, st>>>(map, score, W, H, Mx, My);
    return hipGetLastError();
}
#endif

}  // namespace aefft
