// Per-frame reconstruction error (aefft_net_score, gfx950): the two small kernels beside the scoring epilogue of the inverse row passes
// (fft_kernels.hip c2r_rows_kernel<.., SCORE>, fft_mixed_kernels.hip mix_c2r_rows_kernel<.., SCORE>).
//   score_diff_kernel    the row-pair partial sums of (x - r)^2 from a STORED float reconstruction, for the routes whose reconstruction does
//                        not come out of one of the two row kernels (the spatial net, the chirp-z transforms)
//   score_finish_kernel  a frame's partials added in double, scaled, one float per frame
// No atomics anywhere: a frame's score is one fixed sequence of additions over its own pixels.
#include "internal.h"
#include "device_util.h"

namespace aefft {

// the sum over the 64 lanes of a wave, in every lane: a butterfly, both partners add the same two numbers at every level
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One wave per row pair: rows 2k, 2k+1 of a frame's `rows` rows are 2n consecutive floats (an odd last row: n).  Lane i takes elements i, i + 64, ..
// in order, in double (the kernel is bound by its two reads), then the butterfly; the partial is rounded to float once.
template <bool U8>
__global__ __launch_bounds__(256) void score_diff_kernel(const void* __restrict__ frames, const float* __restrict__ recon, float* __restrict__ part,
                                                         long npairs, long npf, long rows, int n)
{
    const long pair = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= npairs) return;
    const int lane = threadIdx.x & 63;
    const long b = pair / npf, k = pair - b * npf;
    const long first = (b * rows + 2 * k) * n;                          // first element of the pair
    const long len = (2 * k + 1 < rows ? 2L : 1L) * n;
    double acc = 0.0;
    for (long i = lane; i < len; i += 64) {
        const float r = __builtin_nontemporal_load(&recon[first + i]);
        float x;
        if constexpr (U8) x = (float)__builtin_nontemporal_load(&static_cast<const unsigned char*>(frames)[first + i]);
        else x = __builtin_nontemporal_load(&static_cast<const float*>(frames)[first + i]);
        const float d = x - r;
        acc += (double)d * (double)d;
    }
    acc = wave_sum(acc);
    if (lane == 0) part[pair] = (float)acc;
}

// One wave per frame: lane i adds partials i, i + 64, .. of the frame in index order, then the butterfly, all in double
__global__ __launch_bounds__(64) void score_finish_kernel(const float* __restrict__ part, float* __restrict__ score, long npf, double scale)
{
    const float* p = part + (long)blockIdx.x * npf;
    double acc = 0.0;
    for (long i = threadIdx.x; i < npf; i += 64) acc += (double)p[i];
    acc = wave_sum(acc);
    if (threadIdx.x == 0) score[blockIdx.x] = (float)(acc * scale);
}

hipError_t launch_score_diff(const void* frames, bool u8, const float* recon, float* part, int B, long rows, int n, hipStream_t st)
{
    if (!frames || !recon || !part || B < 1 || rows < 1 || n < 1) return hipErrorInvalidValue;
    const long npf = (rows + 1) / 2, npairs = (long)B * npf, blocks = (npairs + 3) / 4;
    if (blocks >= (1L << 31)) return hipErrorInvalidValue;
    if (u8) score_diff_kernel<true><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(frames, recon, part, npairs, npf, rows, n);
    else score_diff_kernel<false><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(frames, recon, part, npairs, npf, rows, n);
    return hipGetLastError();
}

hipError_t launch_score_finish(const float* part, float* score, int B, long npf, double scale, hipStream_t st)
{
    if (!part || !score || B < 1 || npf < 1) return hipErrorInvalidValue;
    score_finish_kernel<<<dim3((unsigned)B), dim3(64), 0, st>>>(part, score, npf, scale);
    return hipGetLastError();
}

}  // namespace aefft
