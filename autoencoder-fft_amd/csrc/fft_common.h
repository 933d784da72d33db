// Device helpers shared by the power-of-two (fft_kernels.hip) and mixed-radix (fft_mixed_kernels.hip) transforms: packed complex
// arithmetic, the small DFT butterflies, the padded LDS index and the row maps of the fused spectral crop / zero-pad.
#pragma once
#include <hip/hip_runtime.h>
#include "internal.h"

namespace aefft {

// complex arithmetic on the native 2-vector, two floats per lane and issue slot (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32).  The row and
// column kernels are co-limited by their VALU instruction stream (rocprofv3 --pmc: VALUBusy 51-55 %), and what hipcc makes of a
// complex product or of a rotation by +-i written on float2 is the packed arithmetic PLUS v_mov / v_xor instructions that build the swapped and
// negated operand (92 of the 363 vector instructions of the 512-point row pass).  The VOP3P modifiers do that inside the arithmetic instruction --
// op_sel / op_sel_hi pick which half of each source feeds the low / high result, neg_lo / neg_hi negate it -- so the products and the
// rotate-and-add forms below are written as the instructions themselves: a complex product is two instructions, a +- i b is one.
typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2f tov(float2 a) { return __builtin_bit_cast(v2f, a); }
__device__ __forceinline__ float2 tof(v2f a) { return __builtin_bit_cast(float2, a); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return a + b; }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return a - b; }
__device__ __forceinline__ float2 cmul(float2 a, float2 b)
{
    v2f t, r;
    const v2f av = tov(a), bv = tov(b);
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1]" : "=v"(t) : "v"(av), "v"(bv));                                        // (a.x b.x, a.x b.y)
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]" : "=v"(r) : "v"(av), "v"(bv), "v"(t));       // + (-a.y b.y, a.y b.x)
    return tof(r);
}
__device__ __forceinline__ float2 cconj(float2 a) { return make_float2(a.x, -a.y); }
// multiply by exp(DIR*i*pi/2): -i for the forward transform, +i for the inverse
template <int DIR> __device__ __forceinline__ float2 mul_i(float2 a)
{
    return DIR < 0 ? make_float2(a.y, -a.x) : make_float2(-a.y, a.x);
}
// a + mul_i<DIR>(b) and a - mul_i<DIR>(b) in one instruction each
template <int DIR> __device__ __forceinline__ float2 add_muli(float2 a, float2 b)
{
    v2f r;
    const v2f av = tov(a), bv = tov(b);
    if (DIR < 0) asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(av), "v"(bv));             // (a.x + b.y, a.y - b.x)
    else asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(av), "v"(bv));                     // (a.x - b.y, a.y + b.x)
    return tof(r);
}
template <int DIR> __device__ __forceinline__ float2 sub_muli(float2 a, float2 b) { return add_muli<-DIR>(a, b); }

template <int R, int DIR> struct Dft;
template <int DIR> struct Dft<2, DIR> {
    static __device__ __forceinline__ void run(float2* a)
    {
        float2 t = a[0];
        a[0] = cadd(t, a[1]);
        a[1] = csub(t, a[1]);
    }
};
template <int DIR> struct Dft<4, DIR> {
    static __device__ __forceinline__ void run(float2* a)
    {
        const float2 t0 = cadd(a[0], a[2]), t1 = csub(a[0], a[2]);
        const float2 t2 = cadd(a[1], a[3]), d = csub(a[1], a[3]);
        a[0] = cadd(t0, t2); a[2] = csub(t0, t2);
        a[1] = add_muli<DIR>(t1, d); a[3] = sub_muli<DIR>(t1, d);
    }
};
template <int DIR> struct Dft<8, DIR> {
    static __device__ __forceinline__ void run(float2* a)
    {
        float2 e[4] = {a[0], a[2], a[4], a[6]};
        float2 o[4] = {a[1], a[3], a[5], a[7]};
        Dft<4, DIR>::run(e);
        Dft<4, DIR>::run(o);
        const float c = 0.70710678118654752440f;
        // o[u] *= w8^u, w8 = exp(DIR*i*pi/4)
        // w8 = (1 -+ i)/sqrt2, w8^3 = (-1 -+ i)/sqrt2:  o*w8 = c*(o + mul_i(o)),  o*w8^3 = -c*(o - mul_i(o)),  o*w8^2 = mul_i(o) (folded into the sums)
        const float2 cc = make_float2(c, c), nc = make_float2(-c, -c);
        const float2 o1 = cc * add_muli<DIR>(o[1], o[1]);
        const float2 o3 = nc * sub_muli<DIR>(o[3], o[3]);
        a[0] = cadd(e[0], o[0]); a[4] = csub(e[0], o[0]);
        a[1] = cadd(e[1], o1);   a[5] = csub(e[1], o1);
        a[2] = add_muli<DIR>(e[2], o[2]); a[6] = sub_muli<DIR>(e[2], o[2]);
        a[3] = cadd(e[3], o3);   a[7] = csub(e[3], o3);
    }
};

__host__ __device__ constexpr int pad_idx(int n) { return n + (n >> 3); }
__host__ __device__ constexpr int pad_len(int n) { return n + (n >> 3) + 2; }

// SpinToImage_C's pixel rule (netlib.cpp:66-68): clamp((int)round(v), 0, 255), halves away from zero (roundf, not v + 0.5: the sum rounds
// 0.49999997 up to 1), NaN -> 0 (the comparison is false)
__device__ __forceinline__ unsigned px_u8(float v) { return v > 0.f ? (unsigned)fminf(roundf(v), 255.f) : 0u; }

// source row of destination row i when the spectrum is cropped from Nx to Nxs rows (fft.cu:102-104)
__device__ __forceinline__ int crop_row(int i, int Nx, int Nxs)
{
    if (Nxs == Nx || i < Nxs / 2) return i;
    if (i == Nxs / 2) return Nx / 2;
    return i + Nx - Nxs;
}
// source row (of Nxi) feeding destination row r (of Nx) under zero-pad up-sampling (fft.cu:119-133); -1 = zero
__device__ __forceinline__ int padsrc_row(int r, int Nx, int Nxi)
{
    if (Nx == Nxi) return r;
    if (r < Nxi / 2) return r;
    if (r > Nx - Nxi / 2) return r - Nx + Nxi;
    if (r == Nx / 2) return Nxi / 2;
    return -1;
}

// Operator-form input of the reconstruction's inverse transform (opform_kernels.hip): the spectrum of plane (b, d) is not
// stored but evaluated where it is read, O_b[d][t] = A[OPC-1][d][t] + sum_j A[j][d][t] x_b[j][u(t)] (u: the bin of the input grid
// that bin t of this grid maps to) -- 4 loads and 3 complex FMAs per element instead of a launch that writes the planes out.
__device__ __forceinline__ float2 opin_load(const OpIn& o, long plane, int t, int Nxi, int Nyi)
{
    const int b = (int)(plane / o.D0), d = (int)(plane - (long)b * o.D0);
    const long Pc = (long)Nxi * (Nyi / 2 + 1), P0 = (long)o.Nx0 * (o.Ny0 / 2 + 1);
    const unsigned nyr = Nyi / 2 + 1, NyrB = o.Ny0 / 2 + 1;
    const unsigned i = (unsigned)t / nyr, j = (unsigned)t - i * nyr;
    const unsigned bi = i < (unsigned)Nxi / 2 ? i : (i == (unsigned)Nxi / 2 ? (unsigned)o.Nx0 / 2 : i + o.Nx0 - Nxi);
    const unsigned bj = j < nyr - 1 ? j : NyrB - 1;
    const long u = (long)bi * NyrB + bj;
    float2 acc = o.A[((long)(OPIN_COLS - 1) * o.D0 + d) * Pc + t];
    for (int jj = 0; jj < o.D0; ++jj) {
        const float2 a = o.A[((long)jj * o.D0 + d) * Pc + t], x = o.Xf[((long)b * o.D0 + jj) * P0 + u];
        acc.x += a.x * x.x - a.y * x.y; acc.y += a.x * x.y + a.y * x.x;
    }
    return acc;
}

}  // namespace aefft
