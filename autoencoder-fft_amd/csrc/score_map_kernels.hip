// Per-tile reconstruction error (aefft_net_score_map, gfx950): the two small kernels beside the mapping epilogue of the inverse row passes
// (fft_kernels.hip c2r_rows_kernel<.., SCORE = 3 / 4>, fft_mixed_kernels.hip mix_c2r_rows_kernel<.., SCORE = 3 / 4>).  A STRIP is two rows x
// tile columns of one channel; the row passes leave one float per strip in strips [B*D*Nx/2][Ny/tile].
//   score_map_diff_kernel    the same strips from a STORED float reconstruction, for the routes whose reconstruction does not come out of one
//                            of the two row kernels (the spatial net, the chirp-z transforms)
//   score_map_finish_kernel  a map entry's D * tile/2 strips added in double, scaled, one float per entry
// No atomics anywhere: a map entry is one fixed sequence of additions over its own pixels.
#include "internal.h"
#include "device_util.h"

namespace aefft {

// One wave per row pair (rows 2k, 2k+1: 2n consecutive floats).  Lane i takes columns i, i + 64, .. of both rows, in double; for each of them the
// tile's columns are an aligned segment of `tile` lanes (tile divides 64 and n), reduced by a butterfly of lt levels; a segment beyond the row
// adds zeros and writes nothing.  Each strip is rounded to float once.
template <bool U8>
__global__ __launch_bounds__(256) void score_map_diff_kernel(const void* __restrict__ frames, const float* __restrict__ recon, float* __restrict__ strips,
                                                             long npairs, int n, int lt)
{
    const long pair = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= npairs) return;                                         // (whole waves)
    const int lane = threadIdx.x & 63;
    const long first = pair * 2 * n;
    const int ns = n >> lt;
    for (int c0 = 0; c0 < n; c0 += 64) {                                // (uniform)
        const int c = c0 + lane;
        double acc = 0.0;
        if (c < n) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const long i = first + (long)r * n + c;
                const float rv = __builtin_nontemporal_load(&recon[i]);
                float x;
                if constexpr (U8) x = (float)__builtin_nontemporal_load(&static_cast<const unsigned char*>(frames)[i]);
                else x = __builtin_nontemporal_load(&static_cast<const float*>(frames)[i]);
                const float d = x - rv;
                acc += (double)d * (double)d;
            }
        }
#pragma unroll
        for (int l = 0; l < 6; ++l)
            if (l < lt) acc += __shfl_xor(acc, 1 << l, 64);
        if ((lane & ((1 << lt) - 1)) == 0 && c < n) strips[pair * ns + (c >> lt)] = (float)acc;
    }
}

// One thread per map entry (b, I, J): its strips are rows (b D + d) Nx/2 + I tile/2 + p of strips [..][nJ], column J -- d outer, the tile row's
// row pairs p inner, in double; scaled by 1 / (D tile tile) and rounded once.
__global__ __launch_bounds__(256) void score_map_finish_kernel(const float* __restrict__ strips, float* __restrict__ map, long entries, int D, int hx /* Nx/2 */,
                                                               int nI, int nJ, int hp /* tile/2 */, double scale)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= entries) return;
    const int J = (int)(e % nJ);
    const long bi = e / nJ;
    const int I = (int)(bi % nI);
    const long b = bi / nI;
    double acc = 0.0;
    for (int d = 0; d < D; ++d) {
        const float* p = strips + (((b * D + d) * hx + (long)I * hp) * nJ + J);
        for (int k = 0; k < hp; ++k) acc += (double)p[(long)k * nJ];
    }
    map[e] = (float)(acc * scale);
}

hipError_t launch_score_map_diff(const void* frames, bool u8, const float* recon, float* strips, long npairs, int n, int tile, hipStream_t st)
{
    const int lt = score_tile_log2(tile);
    if (!frames || !recon || !strips || npairs < 1 || n < 1 || lt < 0 || n % tile) return hipErrorInvalidValue;
    const long blocks = (npairs + 3) / 4;
    if (blocks >= (1L << 31)) return hipErrorInvalidValue;
    if (u8) score_map_diff_kernel<true><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(frames, recon, strips, npairs, n, lt);
    else score_map_diff_kernel<false><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(frames, recon, strips, npairs, n, lt);
    return hipGetLastError();
}

hipError_t launch_score_map_finish(const float* strips, float* map, int B, int D, int Nx, int Ny, int tile, hipStream_t st)
{
    if (!strips || !map || B < 1 || D < 1 || score_tile_log2(tile) < 0 || Nx < tile || Ny < tile || Nx % tile || Ny % tile) return hipErrorInvalidValue;
    const int nI = Nx / tile, nJ = Ny / tile;
    const long entries = (long)B * nI * nJ, blocks = (entries + 255) / 256;
    if (blocks >= (1L << 31)) return hipErrorInvalidValue;
    score_map_finish_kernel<<<dim3((unsigned)blocks), dim3(256), 0, st>>>(strips, map, entries, D, Nx / 2, nI, nJ, tile / 2, 1.0 / ((double)D * tile * tile));
    return hipGetLastError();
}

}  // namespace aefft
