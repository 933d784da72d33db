// Mixed-radix (2, 3, 4, 5, 8) passes of the batched 2-D R2C / C2R for sizes whose only prime factors are 2, 3 and 5 -- the camera
// frames the reference is fed (640 x 480 = 2^7 5 x 2^5 3 5, 1280 x 720, 320 x 240): cufftPlanMany takes them (fft_backproplib.cu:773-779).
//
// The four kernels mirror the power-of-two ones of fft_kernels.hip and share their contract (internal.h launch_r2c / launch_c2r):
//   R2C rows  : two real rows packed as one complex row, one n-point FFT in LDS, Hermitian split into the half-spectra of both rows;
//               DC and Nyquist share packed column 0, so `mid` is [planes][Nx][Nys/2] as on the power-of-two path
//   R2C cols  : CW-column tiles of `mid`, Nx-point FFTs, the spectral crop to Nxs rows fused into the store, column 0 unpacked
//   C2R cols  : the zero-pad from Nxi rows fused into the load, the self-conjugate columns Hermitian-symmetrised (pocketfft semantics)
//   C2R rows  : packed half-spectra (Wc columns, the rest zero) -> two real rows, times `scale`
// so each axis picks its kernel on its own size (640 x 512: mixed columns, power-of-two rows).
//
// One n-point transform is computed by T threads (T = 16 .. 256, the smallest with 8 T >= n): Stockham passes (decimation in frequency,
// auto-sort), in place in LDS (padded index n + n/8), one barrier pair per pass.  The size is not a template parameter: the radix sequence
// travels in the kernel arguments (MixPlan, 4 bits per pass) and the twiddles come from a per-size table, computed on the host in double
// precision and uploaded once per (device, n).  Pass i of radix R at stride S (product of the earlier radices) has n/R butterflies; butterfly
// ib = p*S + q reads elements ib + j*(n/R), j < R, and after the R-point DFT multiplies output u by W_{n/S}^(p u), read from the table at
// off_i + p*(R-1) + u-1 (off_i: the sum of (n/S_j/R_j)*(R_j-1) over the earlier passes).  A thread holds at most ceil(8/R) butterflies.
#include "internal.h"
#include "device_util.h"
#include "fft_common.h"
#include "score_device.h"
#include <hip/hip_ext.h>
#include <math.h>
#include <map>
#include <mutex>
#include <vector>

namespace aefft {

// ------------------------------------------------------------------------------------------
// radix-3 and radix-5 butterflies (packed helpers of fft_common.h)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float2 splat(float c) { return make_float2(c, c); }

// X1,2 = a0 - (a1 + a2)/2 +- DIR i sqrt(3)/2 (a1 - a2)
template <int DIR> struct Dft<3, DIR> {
    static __device__ __forceinline__ void run(float2* a)
    {
        const float2 s = cadd(a[1], a[2]), d = csub(a[1], a[2]);
        const float2 m = csub(a[0], splat(0.5f) * s), e = splat(0.86602540378443864676f) * d;
        a[0] = cadd(a[0], s);
        a[1] = add_muli<DIR>(m, e);
        a[2] = sub_muli<DIR>(m, e);
    }
};

// W = exp(DIR 2 pi i / 5), c_k = cos(2 pi k / 5), s_k = sin(2 pi k / 5):
// X1,4 = a0 + c1 (a1 + a4) + c2 (a2 + a3) +- DIR i (s1 (a1 - a4) + s2 (a2 - a3)),  X2,3 = a0 + c2 (a1 + a4) + c1 (a2 + a3) +- DIR i (s2 (a1 - a4) - s1 (a2 - a3))
template <int DIR> struct Dft<5, DIR> {
    static __device__ __forceinline__ void run(float2* a)
    {
        const float c1 = 0.30901699437494742410f, c2 = -0.80901699437494742410f;
        const float s1 = 0.95105651629515357212f, s2 = 0.58778525229247312917f;
        const float2 b1 = cadd(a[1], a[4]), b2 = cadd(a[2], a[3]), d1 = csub(a[1], a[4]), d2 = csub(a[2], a[3]);
        const float2 m1 = a[0] + splat(c1) * b1 + splat(c2) * b2, m2 = a[0] + splat(c2) * b1 + splat(c1) * b2;
        const float2 e1 = splat(s1) * d1 + splat(s2) * d2, e2 = splat(s2) * d1 - splat(s1) * d2;
        a[0] = a[0] + b1 + b2;
        a[1] = add_muli<DIR>(m1, e1); a[4] = sub_muli<DIR>(m1, e1);
        a[2] = add_muli<DIR>(m2, e2); a[3] = sub_muli<DIR>(m2, e2);
    }
};

// ------------------------------------------------------------------------------------------
// the LDS transform
// ------------------------------------------------------------------------------------------
constexpr int MIX_MAXP = 8;          // passes (1458 = 3^6 2: 7)
struct MixPlan {
    const float2* tw;                // twiddles of every pass, forward sign (the inverse conjugates)
    int n, np;
    unsigned rad;                    // radix of pass i in bits 4i .. 4i+3
};

// T <= 64: a transform lives inside one wave, whose LDS requests are served in order (fft_kernels.hip pass_sync)
template <int T> __device__ __forceinline__ void mix_sync()
{
    if constexpr (T <= 64) __builtin_amdgcn_wave_barrier();
    else __syncthreads();
}

template <int T, int R, int DIR>
__device__ __forceinline__ void mix_pass(float2* s, int t, int n, int S, const float2* __restrict__ tw)
{
    constexpr int NV = (8 + R - 1) / R;       // butterflies per thread (n <= 8 T)
    const int nb = n / R;
    const bool twiddled = n / S > R;
    float2 a[NV * R], w[NV * (R - 1)];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int ib = t + T * v;
        if (ib < nb) {
            const int p = ib / S;
#pragma unroll
            for (int j = 0; j < R; ++j) a[v * R + j] = s[pad_idx(ib + j * nb)];
            if (twiddled) {
#pragma unroll
                for (int u = 1; u < R; ++u) w[v * (R - 1) + u - 1] = tw[p * (R - 1) + u - 1];
            }
        }
    }
    mix_sync<T>();
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int ib = t + T * v;
        if (ib < nb) {
            const int p = ib / S, q = ib - p * S;
            Dft<R, DIR>::run(&a[v * R]);
            if (twiddled) {
#pragma unroll
                for (int u = 1; u < R; ++u) {
                    float2 x = w[v * (R - 1) + u - 1];
                    if (DIR > 0) x.y = -x.y;
                    a[v * R + u] = cmul(a[v * R + u], x);
                }
            }
#pragma unroll
            for (int u = 0; u < R; ++u) s[pad_idx(q + S * (R * p + u))] = a[v * R + u];
        }
    }
    mix_sync<T>();
}

// Caller has issued __syncthreads() after filling `s`; on return the result is in `s` (natural order) and visible to the workgroup.
template <int T, int DIR> __device__ __forceinline__ void mix_fft(float2* s, int t, const MixPlan& pl)
{
    const int n = pl.n;
    int S = 1, off = 0;
    for (int i = 0; i < pl.np; ++i) {
        const int R = (pl.rad >> (4 * i)) & 15;
        const float2* tw = pl.tw + off;
        switch (R) {
        case 2: mix_pass<T, 2, DIR>(s, t, n, S, tw); break;
        case 3: mix_pass<T, 3, DIR>(s, t, n, S, tw); break;
        case 4: mix_pass<T, 4, DIR>(s, t, n, S, tw); break;
        case 5: mix_pass<T, 5, DIR>(s, t, n, S, tw); break;
        default: mix_pass<T, 8, DIR>(s, t, n, S, tw); break;
        }
        off += (n / S / R) * (R - 1);
        S *= R;
    }
    __syncthreads();     // the results are read across transforms
}

template <int T> struct MixRowCfg {
    static constexpr int NT = T >= 256 ? T : 256;
    static constexpr int G = NT / T;          // row PAIRS per workgroup
};

// ------------------------------------------------------------------------------------------
// row passes
// ------------------------------------------------------------------------------------------
// forward: in [npairs*2][n] real (floats, or 8-bit pixels when U8) -> mid [npairs*2][Wc] packed half spectra.  Two pixels per load (n is
// even: every row starts on a 2-element boundary, so no load crosses into the next row whatever n % 4 is).
template <int T, bool U8>
__global__ __launch_bounds__(MixRowCfg<T>::NT) void mix_r2c_rows_kernel(const void* __restrict__ in_v, float2* __restrict__ mid, long npairs,
                                                                         int Wc, const MixPlan pl)
{
    constexpr int NT = MixRowCfg<T>::NT, G = MixRowCfg<T>::G;
    extern __shared__ float2 s[];
    const int N = pl.n, H = N / 2, PL = pad_len(N);
    const int tid = threadIdx.x, g = tid / T, t = tid % T;
    const long pair0 = (long)blockIdx.x * G;
    const int live = npairs - pair0 < G ? (int)(npairs - pair0) : G;
    for (int it = tid; it < live * H; it += NT) {
        const int gg = it / H, c = it - gg * H;
        const long ra = (pair0 + gg) * 2 * H + c;                        // element pair c of row A; row B follows H pairs later
        float2 va, vb;
        if constexpr (U8) {
            const unsigned short* src = static_cast<const unsigned short*>(in_v);
            const unsigned wa = src[ra], wb = src[ra + H];
            va = make_float2((float)(wa & 255u), (float)(wa >> 8));
            vb = make_float2((float)(wb & 255u), (float)(wb >> 8));
        } else {
            const float2* src = static_cast<const float2*>(in_v);
            va = ld_stream(&src[ra]);                                   // (frames are read once)
            vb = ld_stream(&src[ra + H]);
        }
        float2* z = s + gg * PL;
        z[pad_idx(2 * c)] = make_float2(va.x, vb.x);
        z[pad_idx(2 * c + 1)] = make_float2(va.y, vb.y);
    }
    __syncthreads();
    mix_fft<T, -1>(s + g * PL, t, pl);

    // Hermitian split of Z = FFT(a + i b): A[k] = (Z[k] + conj Z[N-k]) / 2, B[k] = (Z[k] - conj Z[N-k]) / 2i; column 0 carries DC + i Nyquist
    for (int it = tid; it < live * Wc; it += NT) {
        const int gg = it / Wc, k = it - gg * Wc;
        const float2* z = s + gg * PL;
        float2 a, b;
        if (k == 0) {
            const float2 z0 = z[pad_idx(0)], zh = z[pad_idx(H)];
            a = make_float2(z0.x, zh.x); b = make_float2(z0.y, zh.y);
        } else {
            const float2 zk = z[pad_idx(k)], zn = z[pad_idx(N - k)];
            a = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y)); b = make_float2(0.5f * (zk.y + zn.y), -0.5f * (zk.x - zn.x));
        }
        float2* dst = mid + (pair0 + gg) * 2 * Wc + k;
        dst[0] = a;
        dst[Wc] = b;
    }
}

// inverse: mid [npairs*2][Wc] packed half spectra (the columns from Wc to n/2 are zero) -> out [npairs*2][n] real, times scale
// U8: ... -> unsigned char [npairs*2][n] by SpinToImage_C's rule (px_u8, fft_common.h), two pixels per 16-bit store (n is even: every row
// starts on a 2-byte boundary whatever n % 4 is, as on the forward pass's load)
// SCORE (1..6, score_device.h; as c2r_rows_kernel's): thread t of row pair g takes the element pairs t, t + T, .. of ITS pair (at most four:
// n <= 8 T) -- the reference's two pixels of both rows requested behind the spectrum's loads -- and one block behind the passes forms the
// rounded rows (stored as well when `out` is non-null), the lane's sums, and their reduction over a strip or over the pair's T threads.
template <int T, bool U8 = false, int SCORE = 0>
__global__ __launch_bounds__(MixRowCfg<T>::NT) void mix_c2r_rows_kernel(const float2* __restrict__ mid, void* __restrict__ out, long npairs,
                                                                         int Wc, float scale, const MixPlan pl, const typename ScoreParam<SCORE>::type sc)
{
    static_assert(!(U8 && SCORE), "the scoring epilogue has no 8-bit reconstruction");
    constexpr int NT = MixRowCfg<T>::NT, G = MixRowCfg<T>::G;
    extern __shared__ float2 s[];
    const int N = pl.n, H = N / 2, PL = pad_len(N);
    const int tid = threadIdx.x, g = tid / T, t = tid % T;
    const long pair0 = (long)blockIdx.x * G;
    const int live = npairs - pair0 < G ? (int)(npairs - pair0) : G;
    if (Wc < H) {
        for (int it = tid; it < G * PL; it += NT) s[it] = make_float2(0.f, 0.f);
        __syncthreads();
    }
    for (int it = tid; it < live * Wc; it += NT) {
        const int gg = it / Wc, k = it - gg * Wc;
        const float2* src = mid + (pair0 + gg) * 2 * Wc + k;
        const float2 A = src[0], B = src[Wc];
        float2* z = s + gg * PL;
        if (k == 0) {
            z[pad_idx(0)] = make_float2(A.x, B.x);          // DC of both rows (imaginary parts ignored)
            z[pad_idx(H)] = make_float2(A.y, B.y);          // Nyquist, carried in .y of the packed column
        } else {
            z[pad_idx(k)] = make_float2(A.x - B.y, A.y + B.x);          // A + i B
            z[pad_idx(N - k)] = make_float2(A.x + B.y, -A.y + B.x);     // conj(A) + i conj(B)
        }
    }
    constexpr int NJ = 4;                                           // element pairs of a row per thread: H <= 4 T
    using Tr = ScoreTraits<SCORE>;
    [[maybe_unused]] ScoreRef<2, Tr::F32> ref[NJ];
    if constexpr (SCORE != 0) {
        const long r0 = (pair0 + (g < live ? g : 0)) * 2 * H;     // (a row pair that does not exist re-reads pair 0; an element pair beyond the row, pair 0 of it)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = t + j * T < H ? t + j * T : 0;
            ref[j].load(sc.frames, r0 + c, r0 + H + c);
        }
    }
    __syncthreads();
    mix_fft<T, +1>(s + g * PL, t, pl);

    if constexpr (SCORE != 0) {
        float* const orow = static_cast<float*>(out) + (pair0 + g) * 2 * N;      // (read under `store` only)
        const bool store = out != nullptr;
        const float2* z = s + g * PL;
        // a strip's sums are one position's; a row pair's run over the lane's positions, its terms in order
        constexpr int NA = Tr::STRIP ? NJ : 1;
        ScoreAcc<Tr::NS> acc[NA];
        if constexpr (!Tr::STRIP) acc[0].clear();
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = t + j * T;
            ScoreAcc<Tr::NS>& a = acc[Tr::STRIP ? j : 0];
            if constexpr (Tr::STRIP) a.clear();
            if (g < live && c < H)
                score_position(z + pad_idx(2 * c), scale, ref[j], score_pivot(sc), store, orow + 2 * c, orow + N + 2 * c, a);
        }
        if constexpr (Tr::STRIP) {
            // the map: element pair e = t + j T is two columns of both rows; a strip is tile/2 consecutive element pairs, i.e. for a FIXED j an aligned
            // segment of tile/2 lanes (T is a power of two, and T >= tile/2 for every smooth n a tile divides; the launcher checks) -- a butterfly
            // per j, never a sum over j.  Lanes with e >= H add 0; they lie in whole segments (tile | n) and write nothing.
            const int lw = sc.lt - 1, ns = N >> sc.lt;                  // log2 of a strip's lanes; strips of a row pair
            const long ms = npairs * ns;                                // floats of one moment's plane
            float* const prow = sc.part + (pair0 + g) * ns;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int c = t + j * T;
                score_strip_reduce<5>(acc[j], lw, (t & ((1 << lw) - 1)) == 0 && g < live && c < H, prow + (c >> lw), ms);
            }
            return;
        }
        const float sum = acc[0].m[0];
        if constexpr (T <= 64) {
            const float v = score_seg_sum<T>(sum);
            if (t == 0 && g < live) sc.part[pair0 + g] = v;
        } else {
            __shared__ float red[NT / 64];
            const float v = score_seg_sum<64>(sum);
            if ((tid & 63) == 0) red[tid >> 6] = v;
            __syncthreads();
            if (t == 0 && g < live) {
                float w = red[tid >> 6];
#pragma unroll
                for (int k = 1; k < T / 64; ++k) w += red[(tid >> 6) + k];
                sc.part[pair0 + g] = w;
            }
        }
        return;
    }
    if constexpr (U8) {
        unsigned short* const o8 = static_cast<unsigned short*>(out);
        for (int it = tid; it < live * H; it += NT) {
            const int gg = it / H, c = it - gg * H;
            const float2* z = s + gg * PL;
            const float2 z0 = z[pad_idx(2 * c)], z1 = z[pad_idx(2 * c + 1)];
            const long ra = (pair0 + gg) * 2 * H + c;
            __builtin_nontemporal_store((unsigned short)(px_u8(z0.x * scale) | px_u8(z1.x * scale) << 8), &o8[ra]);
            __builtin_nontemporal_store((unsigned short)(px_u8(z0.y * scale) | px_u8(z1.y * scale) << 8), &o8[ra + H]);
        }
        return;
    }
    float2* const o = static_cast<float2*>(out);
    for (int it = tid; it < live * H; it += NT) {
        const int gg = it / H, c = it - gg * H;
        const float2* z = s + gg * PL;
        const float2 z0 = z[pad_idx(2 * c)], z1 = z[pad_idx(2 * c + 1)];
        const long ra = (pair0 + gg) * 2 * H + c;
        st_stream(&o[ra], make_float2(z0.x * scale, z1.x * scale));          // (the images are not read again)
        st_stream(&o[ra + H], make_float2(z0.y * scale, z1.y * scale));
    }
}

// ------------------------------------------------------------------------------------------
// column passes: a workgroup transforms CW columns of one plane (blockDim = CW * T; the last tile of a plane may be narrower)
// ------------------------------------------------------------------------------------------
// forward: mid [planes][n][Wc] -> out [planes][Nxs][Wc+1]
template <int T>
__global__ __launch_bounds__(1024) void mix_fwd_cols_kernel(const float2* __restrict__ mid, float2* __restrict__ out, int Wc, int Nxs, int CW,
                                                             const MixPlan pl)
{
    extern __shared__ float2 s[];
    const int N = pl.n, PL = pad_len(N), NT = blockDim.x;
    const int tid = threadIdx.x;
    const long plane = blockIdx.x;
    const int c0 = blockIdx.y * CW, cw = min(CW, Wc - c0);
    const float2* src = mid + plane * N * (long)Wc + c0;
    for (int it = tid; it < N * cw; it += NT) {
        const int r = it / cw, c = it - r * cw;
        s[c * PL + pad_idx(r)] = src[(long)r * Wc + c];
    }
    __syncthreads();
    mix_fft<T, -1>(s + (tid / T) * PL, tid % T, pl);

    const int Nyrs = Wc + 1;
    float2* dst = out + plane * Nxs * (long)Nyrs;
    for (int it = tid; it < Nxs * cw; it += NT) {
        const int i = it / cw, c = it - i * cw;
        const int si = crop_row(i, N, Nxs);
        const float2 z = s[c * PL + pad_idx(si)];
        const int col = c0 + c;
        if (col == 0) {
            // column 0 carries DC + i*Nyquist of the row pass: split by Hermitian symmetry along x
            const float2 zn = s[pad_idx((N - si) % N)];
            dst[(long)i * Nyrs] = make_float2(0.5f * (z.x + zn.x), 0.5f * (z.y - zn.y));
            dst[(long)i * Nyrs + Wc] = make_float2(0.5f * (z.y + zn.y), -0.5f * (z.x - zn.x));
        } else {
            dst[(long)i * Nyrs + col] = z;
        }
    }
}

// inverse: in [planes][Nxi][Wc+1] (rows zero-padded to n) -> mid [planes][n][Wc]
// OPIN: the input spectra are not stored but evaluated on load from the reconstruction's operator (opin_load, fft_common.h), as in the
// power-of-two inv_cols_kernel; `in` is not read.  Its own instantiation: the stored-spectra kernel keeps its load loop.
struct MixNoOp {};
template <bool OPIN> struct MixOpArg { typedef MixNoOp type; };
template <> struct MixOpArg<true> { typedef OpIn type; };
template <int T, bool OPIN>
__global__ __launch_bounds__(1024) void mix_inv_cols_kernel(const float2* __restrict__ in, float2* __restrict__ mid, int Wc, int Nxi, int CW,
                                                             const MixPlan pl, const typename MixOpArg<OPIN>::type op)
{
    extern __shared__ float2 s[];
    const int N = pl.n, PL = pad_len(N), NT = blockDim.x;
    const int tid = threadIdx.x;
    const long plane = blockIdx.x;
    const int c0 = blockIdx.y * CW, cw = min(CW, Wc - c0);
    const int Nyri = Wc + 1;
    const float2* src = in + plane * Nxi * (long)Nyri;
    float2* dcs = s + CW * PL;                                        // [Nxi] column 0 (DC) and [Nxi] Nyquist column, when c0 == 0
    float2* nys = dcs + Nxi;
    if (Nxi < N) {
        for (int it = tid; it < CW * PL; it += NT) s[it] = make_float2(0.f, 0.f);
        __syncthreads();
    }
    for (int it = tid; it < Nxi * cw; it += NT) {
        const int sr = it / cw, c = it - sr * cw;
        float2 v, vn = make_float2(0.f, 0.f);
        if constexpr (OPIN) {
            v = opin_load(op, plane, sr * Nyri + c0 + c, Nxi, 2 * Wc);
            if (c0 + c == 0) vn = opin_load(op, plane, sr * Nyri + Wc, Nxi, 2 * Wc);
        } else {
            v = src[(long)sr * Nyri + c0 + c];
            if (c0 + c == 0) vn = src[(long)sr * Nyri + Wc];
        }
        if (c0 + c == 0) { dcs[sr] = v; nys[sr] = vn; }
        else {
            const int r = Nxi == N ? sr : (sr < Nxi / 2 ? sr : (sr == Nxi / 2 ? N / 2 : sr + N - Nxi));    // inverse of padsrc_row
            s[c * PL + pad_idx(r)] = v;
        }
    }
    if (c0 == 0) {
        __syncthreads();
        for (int r = tid; r < N; r += NT) {
            // Hermitian-symmetrise the two self-conjugate columns and pack them as DC + i*Nyquist
            const int sr = padsrc_row(r, N, Nxi), sm = padsrc_row((N - r) % N, N, Nxi);
            const float2 zz = make_float2(0.f, 0.f);
            const float2 d0 = sr >= 0 ? dcs[sr] : zz, n0 = sr >= 0 ? nys[sr] : zz, d1 = sm >= 0 ? dcs[sm] : zz, n1 = sm >= 0 ? nys[sm] : zz;
            const float2 dc = make_float2(0.5f * (d0.x + d1.x), 0.5f * (d0.y - d1.y));
            const float2 ny = make_float2(0.5f * (n0.x + n1.x), 0.5f * (n0.y - n1.y));
            s[pad_idx(r)] = make_float2(dc.x - ny.y, dc.y + ny.x);
        }
    }
    __syncthreads();
    mix_fft<T, +1>(s + (tid / T) * PL, tid % T, pl);

    float2* dst = mid + plane * N * (long)Wc + c0;
    for (int it = tid; it < N * cw; it += NT) {
        const int r = it / cw, c = it - r * cw;
        dst[(long)r * Wc + c] = s[c * PL + pad_idx(r)];
    }
}

// ------------------------------------------------------------------------------------------
// host side: plans, twiddle tables, launches
// ------------------------------------------------------------------------------------------
bool fft_size_mixed(int n)
{
    if (n < 8 || n > 2048 || (n & 1)) return false;
    while (n % 2 == 0) n /= 2;
    while (n % 3 == 0) n /= 3;
    while (n % 5 == 0) n /= 5;
    return n == 1;
}
bool fft_size_smooth(int n) { return n >= 10 && (n & (n - 1)) != 0 && fft_size_mixed(n); }

// radix sequence: the fives and threes, then eights, then one four or two
static std::vector<int> mix_radices(int n)
{
    std::vector<int> r;
    while (n % 5 == 0) { r.push_back(5); n /= 5; }
    while (n % 3 == 0) { r.push_back(3); n /= 3; }
    while (n % 8 == 0) { r.push_back(8); n /= 8; }
    if (n % 4 == 0) { r.push_back(4); n /= 4; }
    if (n % 2 == 0) { r.push_back(2); n /= 2; }
    return r;
}

struct MixKey { int dev, n; bool operator<(const MixKey& o) const { return dev != o.dev ? dev < o.dev : n < o.n; } };
static std::mutex g_mix_mu;
static std::map<MixKey, float2*> g_mix_tw;     // per (device, n) for the life of the process (at most 2 * 2048 entries each)

// the plan of an n-point transform on the current device; the twiddle table is built on first use (blocking upload)
static hipError_t mix_plan(int n, MixPlan* pl)
{
    if (!fft_size_mixed(n)) return hipErrorInvalidValue;
    const std::vector<int> r = mix_radices(n);
    if ((int)r.size() > MIX_MAXP) return hipErrorInvalidValue;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    pl->n = n; pl->np = (int)r.size(); pl->rad = 0;
    for (size_t i = 0; i < r.size(); ++i) pl->rad |= (unsigned)r[i] << (4 * i);
    std::lock_guard<std::mutex> lock(g_mix_mu);
    auto it = g_mix_tw.find(MixKey{dev, n});
    if (it == g_mix_tw.end()) {
        std::vector<float2> host;
        int S = 1;
        for (int R : r) {
            const int ncur = n / S;
            for (int p = 0; p < ncur / R; ++p)
                for (int u = 1; u < R; ++u) {
                    const double a = -2.0 * M_PI * (double)((long)p * u) / (double)ncur;
                    host.push_back(make_float2((float)cos(a), (float)sin(a)));
                }
            S *= R;
        }
        float2* d = nullptr;
        e = hipMalloc(&d, sizeof(float2) * std::max<size_t>(host.size(), 1));
        if (e != hipSuccess) return e;
        if (!host.empty()) e = hipMemcpy(d, host.data(), sizeof(float2) * host.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(d); return e; }
        it = g_mix_tw.emplace(MixKey{dev, n}, d).first;
    }
    pl->tw = it->second;
    return hipSuccess;
}
hipError_t fft_mixed_prepare(int n) { MixPlan pl; return mix_plan(n, &pl); }

static int mix_threads(int n) { int t = 16; while (8 * t < n) t *= 2; return t; }

template <typename K> static hipError_t mix_allow_lds(K kernel, size_t bytes)
{
    if (bytes <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

#define AEFFT_T_SWITCH(t, CALL)                  \
    switch (t) {                                  \
    case 16: { constexpr int TT = 16; CALL; }     \
    case 32: { constexpr int TT = 32; CALL; }     \
    case 64: { constexpr int TT = 64; CALL; }     \
    case 128: { constexpr int TT = 128; CALL; }   \
    case 256: { constexpr int TT = 256; CALL; }   \
    default: e = hipErrorInvalidValue;            \
    }

template <int T> static hipError_t run_mix_r2c_rows(const void* in, float2* mid, long npairs, int Wc, const MixPlan& pl, hipStream_t st, bool u8)
{
    using Cfg = MixRowCfg<T>;
    const size_t lds = sizeof(float2) * (size_t)Cfg::G * pad_len(pl.n);
    const long blocks = (npairs + Cfg::G - 1) / Cfg::G;
    if (blocks >= (1L << 31)) return hipErrorInvalidValue;
    if (u8) mix_r2c_rows_kernel<T, true><<<dim3((unsigned)blocks), dim3(Cfg::NT), lds, st>>>(in, mid, npairs, Wc, pl);
    else mix_r2c_rows_kernel<T, false><<<dim3((unsigned)blocks), dim3(Cfg::NT), lds, st>>>(in, mid, npairs, Wc, pl);
    return hipGetLastError();
}
template <int T> static hipError_t run_mix_c2r_rows(const float2* mid, void* out, long npairs, int Wc, float scale, const MixPlan& pl, hipStream_t st, bool u8,
                                                    const ScoreArg* score)
{
    using Cfg = MixRowCfg<T>;
    const size_t lds = sizeof(float2) * (size_t)Cfg::G * pad_len(pl.n);
    const long blocks = (npairs + Cfg::G - 1) / Cfg::G;
    if (blocks >= (1L << 31)) return hipErrorInvalidValue;
    if (score) {
        // (T >= tile/2: a strip's element pairs are lanes of ONE row pair.  Every smooth n a tile divides has it; n = 64, 128 with tile 64 would
        // not, and reaches the power-of-two pass instead: a net's pooled grids are >= 8, so its packed width is a power of two >= 4)
        if (score->tile / 2 > T) return hipErrorInvalidValue;
        return score_dispatch(*score, pl.n, u8, [&](auto S, const auto& dev) {
            mix_c2r_rows_kernel<T, false, decltype(S)::value><<<dim3((unsigned)blocks), dim3(Cfg::NT), lds, st>>>(mid, out, npairs, Wc, scale, pl, dev);
            return hipGetLastError();
        });
    }
    if (u8) mix_c2r_rows_kernel<T, true><<<dim3((unsigned)blocks), dim3(Cfg::NT), lds, st>>>(mid, out, npairs, Wc, scale, pl, ScoreNone{});
    else mix_c2r_rows_kernel<T, false><<<dim3((unsigned)blocks), dim3(Cfg::NT), lds, st>>>(mid, out, npairs, Wc, scale, pl, ScoreNone{});
    return hipGetLastError();
}

// column tile: at most 16 columns, 1024 threads and 64 KB of LDS, and not wider than the plane's Wc columns need
static int mix_cw(int n, int T, int Wc, size_t extra)
{
    int cw = std::min(16, 1024 / T);
    while (cw > 1 && sizeof(float2) * ((size_t)cw * pad_len(n)) + extra > 64 * 1024) cw /= 2;
    while (cw > 1 && cw / 2 >= Wc) cw /= 2;
    return cw;
}
template <int T> static hipError_t run_mix_fwd_cols(const float2* mid, float2* out, long planes, int Wc, int Nxs, const MixPlan& pl, hipStream_t st, hipEvent_t done)
{
    const int cw = mix_cw(pl.n, T, Wc, 0);
    const size_t lds = sizeof(float2) * ((size_t)cw * pad_len(pl.n));
    const dim3 grid((unsigned)planes, (unsigned)((Wc + cw - 1) / cw));
    // `done`: recorded by this dispatch's own completion signal (a side stream forks here)
    if (done) hipExtLaunchKernelGGL((mix_fwd_cols_kernel<T>), grid, dim3(cw * T), lds, st, nullptr, done, 0, mid, out, Wc, Nxs, cw, pl);
    else mix_fwd_cols_kernel<T><<<grid, dim3(cw * T), lds, st>>>(mid, out, Wc, Nxs, cw, pl);
    return hipGetLastError();
}
template <int T> static hipError_t run_mix_inv_cols(const float2* in, float2* mid, long planes, int Wc, int Nxi, const MixPlan& pl, hipStream_t st, const OpIn* op)
{
    const size_t extra = sizeof(float2) * 2 * (size_t)Nxi;
    const int cw = mix_cw(pl.n, T, Wc, extra);
    const size_t lds = sizeof(float2) * ((size_t)cw * pad_len(pl.n)) + extra;
    hipError_t e = op ? mix_allow_lds(mix_inv_cols_kernel<T, true>, lds) : mix_allow_lds(mix_inv_cols_kernel<T, false>, lds);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)planes, (unsigned)((Wc + cw - 1) / cw));
    if (op) mix_inv_cols_kernel<T, true><<<grid, dim3(cw * T), lds, st>>>(in, mid, Wc, Nxi, cw, pl, *op);
    else mix_inv_cols_kernel<T, false><<<grid, dim3(cw * T), lds, st>>>(in, mid, Wc, Nxi, cw, pl, MixNoOp{});
    return hipGetLastError();
}

hipError_t launch_mix_r2c_rows(const void* in, float2* mid, long npairs, int Ny, int Wc, hipStream_t st, bool in_u8)
{
    MixPlan pl;
    hipError_t e = mix_plan(Ny, &pl);
    if (e != hipSuccess) return e;
    if (Wc < 1 || 2 * Wc > Ny) return hipErrorInvalidValue;
    AEFFT_T_SWITCH(mix_threads(Ny), e = run_mix_r2c_rows<TT>(in, mid, npairs, Wc, pl, st, in_u8); break)
    return e;
}
hipError_t launch_mix_c2r_rows(const float2* mid, void* out, long npairs, int Ny, int Wc, float scale, hipStream_t st, bool out_u8, const ScoreArg* score)
{
    MixPlan pl;
    hipError_t e = mix_plan(Ny, &pl);
    if (e != hipSuccess) return e;
    if (Wc < 1 || 2 * Wc > Ny) return hipErrorInvalidValue;
    AEFFT_T_SWITCH(mix_threads(Ny), e = run_mix_c2r_rows<TT>(mid, out, npairs, Wc, scale, pl, st, out_u8, score); break)
    return e;
}
hipError_t launch_mix_fwd_cols(const float2* mid, float2* out, long planes, int Nx, int Wc, int Nxs, hipStream_t st, hipEvent_t done)
{
    MixPlan pl;
    hipError_t e = mix_plan(Nx, &pl);
    if (e != hipSuccess) return e;
    if (Wc < 1 || Nxs < 2 || Nxs > Nx || (Nxs & 1) || planes >= (1L << 31)) return hipErrorInvalidValue;
    AEFFT_T_SWITCH(mix_threads(Nx), e = run_mix_fwd_cols<TT>(mid, out, planes, Wc, Nxs, pl, st, done); break)
    return e;
}
hipError_t launch_mix_inv_cols(const float2* in, float2* mid, long planes, int Nx, int Wc, int Nxi, hipStream_t st, const OpIn* opin)
{
    MixPlan pl;
    hipError_t e = mix_plan(Nx, &pl);
    if (e != hipSuccess) return e;
    if (Wc < 1 || Nxi < 2 || Nxi > Nx || (Nxi & 1) || planes >= (1L << 31)) return hipErrorInvalidValue;
    if ((opin != nullptr) == (in != nullptr)) return hipErrorInvalidValue;      // stored spectra or the operator, not both
    // (the operator's bin index and plane products in 32 bits, as opin_load forms them)
    if (opin && (opin->D0 < 1 || opin->D0 > OPIN_COLS - 1 || (long)Nxi * (Wc + 1) >= (1L << 31))) return hipErrorInvalidValue;
    AEFFT_T_SWITCH(mix_threads(Nx), e = run_mix_inv_cols<TT>(in, mid, planes, Wc, Nxi, pl, st, opin); break)
    return e;
}

}  // namespace aefft
