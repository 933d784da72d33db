// Training toward a target frame (aefft_net_step_grad_target, gfx950).  gradient_k_io (fft_backproplib.cu:395-475) reads
// the expected output only in the error O - T, and every output of it is linear in that error; with N_b = X_0,b - T_b (the spectrum of
// pool(x_b - t_b) on pair 0's grid, exactly zero when the target is the frame) pair 0's error is (O - X) + N, and the target enters as
//   target_terms_kernel   S_0 += sum_b N_b X_b^H,  es_0 += sum_b N_b(0,0)  behind the launch that completes them; it also leaves
//                         K = sum_b N_b [X_b; 1]^H (D x (D+1) per bin) and n2 = sum_b |N_b|^2 for the post-update MSE
//   target_mse_kernel     |T - O'|^2 = |E|^2 - 2 Re(E^H N) + |N|^2 with E = X - O' = R [X; 1], R = [I - G'_0 | -beta^]: the step's own launches
//                         sum |E|^2, this one adds -2 Re tr(R K^H) + n2 into pair 0's slots
// Neither reads a frame twice, and nothing of the plain step's kernels changes.
#include "internal.h"
#include "device_util.h"

namespace aefft {

// batch slices per workgroup (one wave each), by the LDS their partial sums take: 8 x 12 x 64 complex = 48 KB at D = 3
template <int D> struct TargetTile { static constexpr int SL = D <= 3 ? 8 : 4, NK = D * (D + 1); };

// Workgroup = 64 consecutive bins x SL waves; lane = bin (consecutive lanes, consecutive bins, 8-byte loads), wave w takes frames w, w + SL, ..
// Phase A: every wave sums its frames' terms in registers, in frame order.  Phase B: the SL partial sums of every element go through LDS and
// are added in wave order 0 .. SL-1 by the wave that owns the element's plane -- a fixed order, no atomics: the same inputs give the same bits.
// Lanes past P0 load the last bin and store nothing; a wave with no frame (B < SL) adds zeros.
template <int D>
__global__ __launch_bounds__(64 * TargetTile<D>::SL) void target_terms_kernel(const float2* __restrict__ Xf, const float2* __restrict__ Tf, float2* __restrict__ S,
                                                                               float* __restrict__ es /* nullable */, float2* __restrict__ K, float* __restrict__ n2,
                                                                               int B, long P0)
{
    constexpr int SL = TargetTile<D>::SL, NK = TargetTile<D>::NK;
    __shared__ float2 pk[SL][NK][64];
    __shared__ float pn[SL][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long s = (long)blockIdx.x * 64 + lane;
    const bool ok = s < P0;
    const long sc = ok ? s : P0 - 1;
    float2 acc[NK];
#pragma unroll
    for (int e = 0; e < NK; ++e) acc[e] = make_float2(0.f, 0.f);
    float an = 0.f;
#pragma unroll 2
    for (int b = w; b < B; b += SL) {
        float2 x[D], t[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            x[d] = Xf[((long)b * D + d) * P0 + sc];
            t[d] = Tf[((long)b * D + d) * P0 + sc];
        }
#pragma unroll
        for (int a = 0; a < D; ++a) {
            const float2 nv = make_float2(x[a].x - t[a].x, x[a].y - t[a].y);
#pragma unroll
            for (int j = 0; j < D; ++j) {            // N[a] conj(X[j])
                acc[a * (D + 1) + j].x += nv.x * x[j].x + nv.y * x[j].y;
                acc[a * (D + 1) + j].y += nv.y * x[j].x - nv.x * x[j].y;
            }
            acc[a * (D + 1) + D].x += nv.x; acc[a * (D + 1) + D].y += nv.y;
            an += nv.x * nv.x + nv.y * nv.y;
        }
    }
#pragma unroll
    for (int e = 0; e < NK; ++e) pk[w][e][lane] = acc[e];
    pn[w][lane] = an;
    __syncthreads();
    for (int e = w; e < NK; e += SL) {               // (uniform per wave)
        float2 v = pk[0][e][lane];
#pragma unroll
        for (int k = 1; k < SL; ++k) { const float2 u = pk[k][e][lane]; v.x += u.x; v.y += u.y; }
        if (!ok) continue;
        K[(long)e * P0 + s] = v;
        const int a = e / (D + 1), j = e - a * (D + 1);
        if (j < D) {
            float2* p = S + ((long)a * D + j) * P0 + s;      // (mk_S layout: [error channel][input channel][bin]; the element is this lane's alone)
            float2 o = *p;
            o.x += v.x; o.y += v.y;
            *p = o;
        } else if (s == 0 && es) {
            es[2 * a] += v.x; es[2 * a + 1] += v.y;
        }
    }
    if (w == NK % SL) {
        float v = pn[0][lane];
#pragma unroll
        for (int k = 1; k < SL; ++k) v += pn[k][lane];
        if (ok) n2[s] = v;
    }
}

// One bin per thread, 256 consecutive bins per workgroup.  G' = F'.C'/(dM D) of the UPDATED weights is read ([D][D] planes, where a route left
// it) or formed from the planar spectra C' [dM][D][P], F' [D][dM][P]; the difference to the identity is taken on the matrix elements, as the
// step's own MSE kernels take it.  The bias column of R is -beta^ at the DC bin, beta^ = Nx Ny (p' + F'(0,0) b' / D).  Interior columns of the
// Hermitian half-plane count twice (calc_mse, fft_backproplib.cu:480-498); block sum, one add into pair 0's slots (launch_mse_finish sums them).
template <int D>
__global__ __launch_bounds__(256) void target_mse_kernel(const TargetMseArgs q)
{
    __shared__ float red[4];
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    const bool ok = s < q.P;
    const long sc = ok ? s : q.P - 1;
    float2 k[D * (D + 1)];
#pragma unroll
    for (int e = 0; e < D * (D + 1); ++e) k[e] = q.K[(long)e * q.P + sc];
    float part = q.n2[sc];
    float2 g[D * D];
    if (q.G) {
#pragma unroll
        for (int e = 0; e < D * D; ++e) g[e] = q.G[(long)e * q.P + sc];
    } else {
#pragma unroll
        for (int e = 0; e < D * D; ++e) g[e] = make_float2(0.f, 0.f);
        for (int m = 0; m < q.dM; ++m) {
            float2 f[D], c[D];
#pragma unroll
            for (int d = 0; d < D; ++d) {
                f[d] = q.F[((long)d * q.dM + m) * q.P + sc];
                c[d] = q.C[((long)m * D + d) * q.P + sc];
            }
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    g[a * D + d].x += f[a].x * c[d].x - f[a].y * c[d].y;
                    g[a * D + d].y += f[a].x * c[d].y + f[a].y * c[d].x;
                }
        }
        const float inv = 1.0f / ((float)q.dM * (float)D);
#pragma unroll
        for (int e = 0; e < D * D; ++e) { g[e].x *= inv; g[e].y *= inv; }
    }
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const float rx = (a == j ? 1.f : 0.f) - g[a * D + j].x, ry = -g[a * D + j].y;      // (I - G')[a][j]
            const float2 kv = k[a * (D + 1) + j];
            part -= 2.f * (rx * kv.x + ry * kv.y);
        }
    if (s == 0) {
        const float NN = (float)q.Nx * (float)q.Ny;
#pragma unroll
        for (int a = 0; a < D; ++a) {
            // beta[a] = p'[a] + sum_m F'[a][m](0,0) b'[m] / D  (F' at the DC bin is real: the sum of the taps)
            float acc = 0.f;
            for (int m = 0; m < q.dM; ++m) acc = fmaf(q.Fdc[((long)a * q.dM + m) * q.fdc_stride].x, q.b[m], acc);
            part += 2.f * (q.p[a] + acc / (float)D) * NN * k[a * (D + 1) + D].x;
        }
    }
    {
        const int nyr = q.Ny / 2 + 1;
        const int j = (int)(sc % nyr);
        part *= !ok ? 0.f : ((j > 0 && j < nyr - 1) ? 2.f : 1.f);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float tot = (red[0] + red[1]) + (red[2] + red[3]);
        if (tot != 0.f) atomicAdd(q.slots + (blockIdx.x % MSE_SLOTS) * MSE_SLOT_STRIDE, tot * q.scale);
    }
}

template <int D>
static hipError_t terms_launch(const float2* Xf, const float2* Tf, float2* S, float* es, float2* K, float* n2, int B, long P0, hipStream_t st)
{
    const long blocks = (P0 + 63) / 64;
    if (blocks >= (1L << 31)) return hipErrorInvalidValue;
    target_terms_kernel<D><<<dim3((unsigned)blocks), dim3(64 * TargetTile<D>::SL), 0, st>>>(Xf, Tf, S, es, K, n2, B, P0);
    return hipGetLastError();
}

hipError_t launch_target_terms(const float2* Xf, const float2* Tf, float2* S, float* es, float2* K, float* n2, int B, int D, long P0, hipStream_t st)
{
    if (!Xf || !Tf || !S || !K || !n2 || B < 1 || P0 < 1) return hipErrorInvalidValue;
    switch (D) {
    case 1: return terms_launch<1>(Xf, Tf, S, es, K, n2, B, P0, st);
    case 2: return terms_launch<2>(Xf, Tf, S, es, K, n2, B, P0, st);
    case 3: return terms_launch<3>(Xf, Tf, S, es, K, n2, B, P0, st);
    case 4: return terms_launch<4>(Xf, Tf, S, es, K, n2, B, P0, st);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_target_mse(const TargetMseArgs& q, int D, hipStream_t st)
{
    if (!q.K || !q.n2 || !q.slots || !q.Fdc || !q.b || !q.p || (!q.G && (!q.C || !q.F)) || q.dM < 1 || q.P < 1) return hipErrorInvalidValue;
    const long blocks = (q.P + 255) / 256;
    if (blocks >= (1L << 31)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(256);
    switch (D) {
    case 1: target_mse_kernel<1><<<grid, block, 0, st>>>(q); break;
    case 2: target_mse_kernel<2><<<grid, block, 0, st>>>(q); break;
    case 3: target_mse_kernel<3><<<grid, block, 0, st>>>(q); break;
    case 4: target_mse_kernel<4><<<grid, block, 0, st>>>(q); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace aefft
