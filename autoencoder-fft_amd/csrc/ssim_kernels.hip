// Block SSIM of the reconstruction (aefft_net_ssim_map, gfx950): the two small kernels beside the SSIM epilogue of the inverse row passes
// (fft_kernels.hip c2r_rows_kernel<.., SCORE = 5 / 6>, fft_mixed_kernels.hip mix_c2r_rows_kernel<.., SCORE = 5 / 6>).  A STRIP is two rows x
// tile columns of one channel; the row passes leave FIVE floats per strip -- the sums of x', r', x'^2, r'^2, x'r' with x' = x - pivot,
// r' = r - pivot -- in strips [5][B*D*Nx/2][Ny/tile]: one plane per moment, each laid out as aefft_net_score_map's strip buffer.
//   ssim_diff_kernel    the same strips from a STORED float reconstruction, for the routes whose reconstruction does not come out of one of
//                       the two row kernels (the spatial net, the chirp-z transforms)
//   ssim_finish_kernel  per channel a window's tile/2 strips of each moment added in double, the SSIM formula in double, the channels'
//                       mean, one float per map entry
// No atomics anywhere: a map entry is one fixed sequence of operations on its own pixels.
#include "internal.h"
#include "device_util.h"

namespace aefft {

// score_map_diff_kernel's wave per row pair, lane per column, butterfly per tile -- with five sums, in double, each rounded to float once.
template <bool U8>
__global__ __launch_bounds__(256) void ssim_diff_kernel(const void* __restrict__ ref, const float* __restrict__ recon, float* __restrict__ strips,
                                                        long npairs, int n, int lt, float pivot)
{
    const long pair = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= npairs) return;                                         // (whole waves)
    const int lane = threadIdx.x & 63;
    const long first = pair * 2 * n;
    const int ns = n >> lt;
    const long ms = npairs * ns;                                        // floats of one moment's plane
    for (int c0 = 0; c0 < n; c0 += 64) {                                // (uniform)
        const int c = c0 + lane;
        double m[SSIM_MOMENTS] = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (c < n) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const long i = first + (long)r * n + c;
                const float rv = __builtin_nontemporal_load(&recon[i]);
                float x;
                if constexpr (U8) x = (float)__builtin_nontemporal_load(&static_cast<const unsigned char*>(ref)[i]);
                else x = __builtin_nontemporal_load(&static_cast<const float*>(ref)[i]);
                const double a = (double)x - (double)pivot, b = (double)rv - (double)pivot;
                m[0] += a; m[1] += b; m[2] += a * a; m[3] += b * b; m[4] += a * b;
            }
        }
#pragma unroll
        for (int k = 0; k < SSIM_MOMENTS; ++k) {
#pragma unroll
            for (int l = 0; l < 6; ++l)
                if (l < lt) m[k] += __shfl_xor(m[k], 1 << l, 64);
        }
        if ((lane & ((1 << lt) - 1)) == 0 && c < n) {
#pragma unroll
            for (int k = 0; k < SSIM_MOMENTS; ++k) strips[k * ms + pair * ns + (c >> lt)] = (float)m[k];
        }
    }
}

// One thread per map entry (b, I, J).  Per channel d: the window's strips are rows (b D + d) Nx/2 + I tile/2 + p of every moment's plane
// [..][nJ], column J, added over p in double; then, with n = tile^2 pixels,
//   mx' = Sx/n, mr' = Sr/n (means less the pivot), vx = max(Sxx/n - mx'^2, 0), vr = max(Srr/n - mr'^2, 0), c = Sxr/n - mx' mr',
//   ssim = (2 mx mr + C1)(2 c + C2) / ((mx^2 + mr^2 + C1)(vx + vr + C2)),  mx = mx' + pivot, mr = mr' + pivot;
// the channels are added in order, scaled by 1/D and rounded once.
__global__ __launch_bounds__(64) void ssim_finish_kernel(const float* __restrict__ strips, float* __restrict__ map, long entries, long ms, int D, int hx /* Nx/2 */,
                                                          int nI, int nJ, int hp /* tile/2 */, double inv_n, double pivot, double C1, double C2)
{
    const long e = (long)blockIdx.x * 64 + threadIdx.x;        // (one wave per workgroup: a tile-64 map has few entries, each a long chain of loads -- spread over the CUs)
    if (e >= entries) return;
    const int J = (int)(e % nJ);
    const long bi = e / nJ;
    const int I = (int)(bi % nI);
    const long b = bi / nI;
    double acc = 0.0;
    for (int d = 0; d < D; ++d) {
        const float* p = strips + (((b * D + d) * hx + (long)I * hp) * nJ + J);
        // (row pair outer, moment inner: five independent loads per step, and each moment's strips still added in row-pair order)
        double s[SSIM_MOMENTS] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
        for (int q = 0; q < hp; ++q) {
#pragma unroll
            for (int k = 0; k < SSIM_MOMENTS; ++k) s[k] += (double)p[k * ms + (long)q * nJ];
        }
#pragma unroll
        for (int k = 0; k < SSIM_MOMENTS; ++k) s[k] *= inv_n;
        const double vx = fmax(s[2] - s[0] * s[0], 0.0), vr = fmax(s[3] - s[1] * s[1], 0.0), cv = s[4] - s[0] * s[1];
        const double mx = s[0] + pivot, mr = s[1] + pivot;
        acc += (2.0 * mx * mr + C1) * (2.0 * cv + C2) / ((mx * mx + mr * mr + C1) * (vx + vr + C2));
    }
    map[e] = (float)(acc / (double)D);
}

hipError_t launch_ssim_diff(const void* ref, bool u8, const float* recon, float* strips, long npairs, int n, int tile, float pivot, hipStream_t st)
{
    const int lt = score_tile_log2(tile);
    if (!ref || !recon || !strips || npairs < 1 || n < 1 || lt < 0 || n % tile) return hipErrorInvalidValue;
    const long blocks = (npairs + 3) / 4;
    if (blocks >= (1L << 31)) return hipErrorInvalidValue;
    if (u8) ssim_diff_kernel<true><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(ref, recon, strips, npairs, n, lt, pivot);
    else ssim_diff_kernel<false><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(ref, recon, strips, npairs, n, lt, pivot);
    return hipGetLastError();
}

hipError_t launch_ssim_finish(const float* strips, float* map, int B, int D, int Nx, int Ny, int tile, float data_range, float pivot, hipStream_t st)
{
    if (!strips || !map || B < 1 || D < 1 || score_tile_log2(tile) < 0 || Nx < tile || Ny < tile || Nx % tile || Ny % tile || !(data_range > 0.f)) return hipErrorInvalidValue;
    const int nI = Nx / tile, nJ = Ny / tile;
    const long entries = (long)B * nI * nJ, blocks = (entries + 63) / 64;
    if (blocks >= (1L << 31)) return hipErrorInvalidValue;
    const long ms = (long)B * D * (Nx / 2) * nJ;
    const double L = (double)data_range, C1 = (0.01 * L) * (0.01 * L), C2 = (0.03 * L) * (0.03 * L);
    ssim_finish_kernel<<<dim3((unsigned)blocks), dim3(64), 0, st>>>(strips, map, entries, ms, D, Nx / 2, nI, nJ, tile / 2, 1.0 / ((double)tile * tile), (double)pivot, C1, C2);
    return hipGetLastError();
}

}  // namespace aefft
