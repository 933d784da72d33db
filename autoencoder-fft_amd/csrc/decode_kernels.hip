// Decode (aefft_net_decode, gfx950): frames from a stored hidden layer, in the operator forms.
//
// The FFT-mode network is linear, and every pooling crop between a hidden layer and the innermost pair discards the bins outside the
// coarsest grid; every decoder output is zero outside that grid's image (decoder_compact, net_step.hip).  The remainder of autoenc_fft
// from layer 2l+2 (fft_backproplib.cu:1331-1376, loop index n = l+1 onward) is therefore ONE affine operator per bin t of the coarsest grid:
//       O_0,b[t] = T^_l[t] [h_b[t]; 1]          h_b = the code's spectrum on grid l, cropped to the coarsest grid (the R2C's fused crop)
//       T^_l     = (F_0/dD_0) (F_1/dD_1) ... (F_{L-1}/dD_{L-1}) (C_{L-1}/dM_{L-1}) ... (C_{l+1}/dM_{l+1})      [D][dM_l], each factor read
//                  at the bin of its own grid that t maps to (map_up: pool_fft's row and Nyquist-column map, compositions keep its form),
// and the affine column collects every bias below, each times its layer's own Nx*Ny, on the DC bin (conv_k, :162-189; the un-pooling
// steps carry no amplitude factor, :154-155).  decode_op_kernel forms T^_l once per weight set and pair, decode_apply_kernel applies it.
#include "../../include/aefft.h"
#include "internal.h"
#include "device_util.h"
#include "opform_device.h"

namespace aefft {

__device__ __forceinline__ void dec_cfma(float2& acc, float2 a, float2 b) { acc.x = fmaf(a.x, b.x, acc.x); acc.x = fmaf(-a.y, b.y, acc.x); acc.y = fmaf(a.x, b.y, acc.y); acc.y = fmaf(a.y, b.x, acc.y); }

// ------------------------------------------------------------------------------------------
// T^_l, row by row: thread = (bin t, output channel d).  The row vector r = e_d^T F_0/dD_0 ... is carried through the stages left to
// right, r' = r W / div with W [K][M] row-major at the stage's bin, affine' = affine + (r . bias) Nx Ny [t == 0].  A row is up to
// 513 complex long: it lives in the thread's own column of a two-halved workspace ws [2][D][maxW][NT] (lane-contiguous, so every access
// is coalesced; a thread reads back only what it wrote itself), the last stage writes T [D][M+1][Pc].  NT threads stride over the bins;
// the workgroup is 64 bins x D rows.
// (Runs once per weight set and pair: the gathers of W -- K*M per stage and thread -- are what it costs.)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void decode_op_kernel(const DecodeOpArgs g)
{
    const int tid = blockIdx.x * 64 + threadIdx.x;
    const int d = threadIdx.y;                 // (blockDim.y == D)
    if (tid >= g.NT) return;
    for (long t = tid; t < g.Pc; t += g.NT) {
        const bool dc = t == 0;
        for (int s = 0; s < g.nst; ++s) {
            const DecodeStage& st = g.st[s];
            const int K = st.K, M = st.M;
            const long u = map_up(t, g.NxC, g.NyC, st.Nx, st.Ny);
            const bool last = s == g.nst - 1;
            float2* out = last ? g.T + (long)d * (M + 1) * g.Pc + t : g.ws + ((long)(s & 1) * g.D + d) * g.maxW * g.NT + tid;
            const long os = last ? g.Pc : g.NT;
            if (s == 0) {        // r = row d of F_0 / dD_0, affine = p_0[d] Nx Ny
                for (int m = 0; m < M; ++m) out[m * os] = pk_scale(st.inv, st.W[((long)d * M + m) * st.P + u]);
                out[M * os] = make_float2(dc ? st.bias[d] * st.nn : 0.f, 0.f);
                continue;
            }
            const float2* in = g.ws + ((long)((s - 1) & 1) * g.D + d) * g.maxW * g.NT + tid;
            float2 aff = in[(long)K * g.NT];
            if (dc)
                for (int c = 0; c < K; ++c) { const float2 r = in[(long)c * g.NT]; const float bn = st.bias[c] * st.nn; aff.x = fmaf(r.x, bn, aff.x); aff.y = fmaf(r.y, bn, aff.y); }
            for (int m = 0; m < M; ++m) {
                float2 acc = make_float2(0.f, 0.f);
                for (int c = 0; c < K; ++c) dec_cfma(acc, in[(long)c * g.NT], st.W[((long)c * M + m) * st.P + u]);
                out[m * os] = pk_scale(st.inv, acc);
            }
            out[M * os] = aff;
        }
    }
}

hipError_t launch_decode_op(const DecodeOpArgs& g, hipStream_t st)
{
    if (g.nst < 1 || g.nst > DEC_MAX_STAGES || g.D < 1 || g.D > 4 || g.Pc < 1 || g.NT < 1 || g.NT % 64 || g.maxW < 2 || !g.T || !g.ws) return hipErrorInvalidValue;
    for (int s = 0; s < g.nst; ++s) {
        const DecodeStage& q = g.st[s];
        const bool last = s == g.nst - 1;
        // every row a stage writes -- M elements and the affine one -- fits the column of what was allocated: the workspace (stride maxW), or T for
        // the last stage (Tw rows); a stage's input is the stage before's output; stage 0 reads row d < D of F_0 and no row
        if (q.K < 1 || q.M < 1 || q.M + 1 > (last ? g.Tw : g.maxW) || (s > 0 && q.K != g.st[s - 1].M) || (s == 0 && q.K != g.D)) return hipErrorInvalidValue;
        if (q.Nx < g.NxC || q.Ny < g.NyC || q.P != (long)q.Nx * (q.Ny / 2 + 1)) return hipErrorInvalidValue;
    }
    decode_op_kernel<<<dim3((unsigned)(g.NT / 64)), dim3(64, g.D), 0, st>>>(g);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// out[b][d][t] = sum_m T[d][m][t] h[b][m][t] + T[d][K][t]: a skinny per-bin product (K = dM_l up to 513, DD <= 3 rows).
// Bins across the 64 lanes (every load and store one contiguous 512-byte piece per wave); the four waves of a workgroup split K, each
// keeps its T[.][m][t] in registers across its FPT frames (DD + FPT loads feed DD * FPT complex multiply-adds), and the partial sums
// meet in LDS.  The grid's second axis runs over groups of FPT frames.
// ------------------------------------------------------------------------------------------
template <int DD, int FPT>
__global__ __launch_bounds__(256) void decode_apply_kernel(const float2* __restrict__ T, const float2* __restrict__ h, float2* __restrict__ out,
                                                           int B, int K, long Pc)
{
    __shared__ float2 red[3][FPT * DD][64];
    const long t = min((long)blockIdx.x * 64 + threadIdx.x, Pc - 1);      // (clamped: the lanes past the end load valid addresses and store nothing)
    const bool live = (long)blockIdx.x * 64 + threadIdx.x < Pc;
    const int b0 = blockIdx.y * FPT;
    const int y = threadIdx.y;
    float2 acc[FPT][DD];
#pragma unroll
    for (int f = 0; f < FPT; ++f)
#pragma unroll
        for (int d = 0; d < DD; ++d) acc[f][d] = make_float2(0.f, 0.f);
    const float2* hb[FPT];
#pragma unroll
    for (int f = 0; f < FPT; ++f) hb[f] = h + (long)min(b0 + f, B - 1) * K * Pc + t;
#pragma unroll 2
    for (int m = y; m < K; m += 4) {
        float2 tv[DD], hv[FPT];
#pragma unroll
        for (int d = 0; d < DD; ++d) tv[d] = T[((long)d * (K + 1) + m) * Pc + t];
#pragma unroll
        for (int f = 0; f < FPT; ++f) hv[f] = hb[f][(long)m * Pc];
#pragma unroll
        for (int f = 0; f < FPT; ++f)
#pragma unroll
            for (int d = 0; d < DD; ++d) dec_cfma(acc[f][d], tv[d], hv[f]);
    }
    if (y > 0) {
#pragma unroll
        for (int f = 0; f < FPT; ++f)
#pragma unroll
            for (int d = 0; d < DD; ++d) red[y - 1][f * DD + d][threadIdx.x] = acc[f][d];
    }
    __syncthreads();
    if (y > 0 || !live) return;
#pragma unroll
    for (int d = 0; d < DD; ++d) {
        const float2 aff = T[((long)d * (K + 1) + K) * Pc + t];
#pragma unroll
        for (int f = 0; f < FPT; ++f) {
            if (b0 + f >= B) continue;
            float2 v = acc[f][d];
#pragma unroll
            for (int w = 0; w < 3; ++w) { const float2 p = red[w][f * DD + d][threadIdx.x]; v.x += p.x; v.y += p.y; }
            out[((long)(b0 + f) * DD + d) * Pc + t] = make_float2(v.x + aff.x, v.y + aff.y);
        }
    }
}

template <int DD> static hipError_t decode_apply_d(const float2* T, const float2* h, float2* out, int B, int K, long Pc, hipStream_t st)
{
    const long bx = (Pc + 63) / 64;
    // eight frames per thread halve the re-reads of T; four where that leaves fewer than two workgroups per compute unit
    if (bx * ((B + 7) / 8) >= 512) decode_apply_kernel<DD, 8><<<dim3((unsigned)bx, (unsigned)((B + 7) / 8)), dim3(64, 4), 0, st>>>(T, h, out, B, K, Pc);
    else decode_apply_kernel<DD, 4><<<dim3((unsigned)bx, (unsigned)((B + 3) / 4)), dim3(64, 4), 0, st>>>(T, h, out, B, K, Pc);
    return hipGetLastError();
}

hipError_t launch_decode_apply(const float2* T, const float2* h, float2* out, int B, int D, int K, long Pc, hipStream_t st)
{
    if (B < 1 || K < 1 || Pc < 1 || (B + 3) / 4 > 65535 || (Pc + 63) / 64 >= (1L << 31)) return hipErrorInvalidValue;
    switch (D) {
    case 1: return decode_apply_d<1>(T, h, out, B, K, Pc, st);
    case 2: return decode_apply_d<2>(T, h, out, B, K, Pc, st);
    case 3: return decode_apply_d<3>(T, h, out, B, K, Pc, st);
    default: return hipErrorInvalidValue;      // (the operator forms take at most OPC - 1 = 3 input channels)
    }
}

}  // namespace aefft
