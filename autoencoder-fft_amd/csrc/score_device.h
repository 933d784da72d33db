// The scoring epilogue of the inverse row passes (c2r_rows_kernel<.., SCORE> in fft_kernels.hip, mix_c2r_rows_kernel<.., SCORE> in
// fft_mixed_kernels.hip): what a SCORE value means, the lane's reference pixels, its sums, one position's work, the strip reduction -- and the
// host's one way from a ScoreArg (internal.h) to an instantiation.  Both kernels build their single scoring block from these.
#pragma once
#include <type_traits>
#include "device_util.h"
#include "fft_common.h"

namespace aefft {

// SCORE 0: none.  1 / 2: one float per ROW PAIR (aefft_net_score); 3 / 4: one float per STRIP -- two rows x `tile` columns of one channel,
// tile = 1 << lt in 8..64 -- (aefft_net_score_map); 5 / 6: five floats per strip (aefft_net_ssim_map).  Odd: the reference pixels are floats;
// even: 8-bit.
template <int SCORE> struct ScoreTraits {
    static constexpr bool F32 = (SCORE & 1) != 0;                     // the reference is float (else 8-bit pixels)
    static constexpr int NS = SCORE >= 5 ? SSIM_MOMENTS : 1;          // sums per lane position
    static constexpr bool STRIP = SCORE >= 3;                         // the reduction stops at a strip (else it runs over the row pair)
};

// Only a scoring instantiation carries the argument: the others take the empty ScoreNone, so their argument loads and their code are what
// they were.  part: [npairs] (ScoreDev), [npairs][n >> lt] (ScoreMapDev), [SSIM_MOMENTS][npairs][n >> lt], one plane per moment (ScoreSsimDev).
// The tile is a run-time value (no template axis over it).
struct ScoreNone {};
struct ScoreDev { const void* frames; float* part; };
struct ScoreMapDev { const void* frames; float* part; int lt; };
struct ScoreSsimDev { const void* frames; float* part; int lt; float pivot; };
template <int SCORE> struct ScoreParam { typedef ScoreDev type; };
template <> struct ScoreParam<0> { typedef ScoreNone type; };
template <> struct ScoreParam<3> { typedef ScoreMapDev type; };
template <> struct ScoreParam<4> { typedef ScoreMapDev type; };
template <> struct ScoreParam<5> { typedef ScoreSsimDev type; };
template <> struct ScoreParam<6> { typedef ScoreSsimDev type; };
__device__ __forceinline__ float score_pivot(const ScoreDev&) { return 0.f; }
__device__ __forceinline__ float score_pivot(const ScoreMapDev&) { return 0.f; }
__device__ __forceinline__ float score_pivot(const ScoreSsimDev& s) { return s.pivot; }

// The reconstructed pixel is the ROUNDED product z * scale, the value the float row pass stores.  Passing it through an empty asm makes it a
// value of its own: the back end cannot contract the product into the subtraction that follows (x - z * scale as one fma would make the score
// a function of the unrounded product, and a trained net's small residual is where that shows).
__device__ __forceinline__ float score_px(float z, float scale) { float r = z * scale; asm("" : "+v"(r)); return r; }
__device__ __forceinline__ float score_sq(float x, float r) { const float d = x - r; return d * d; }
// one pixel's five terms, in this order: sum x', r', x'^2, r'^2, x'r' with x' = x - pivot, r' = r - pivot (x the reference pixel, r the rounded
// reconstruction).  The pivot (half the data range) keeps the float sums of squares small where the window is flat; variances and the
// covariance do not depend on it, the finish adds it back to the means.
__device__ __forceinline__ void ssim_acc(float (&m)[SSIM_MOMENTS], float x, float r, float pivot)
{
    const float a = x - pivot, b = r - pivot;
    m[0] += a; m[1] += b; m[2] += a * a; m[3] += b * b; m[4] += a * b;
}
// a lane's sums: one of (x - r)^2, or SSIM's five
template <int NS> struct ScoreAcc {
    float m[NS];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int k = 0; k < NS; ++k) m[k] = 0.f;
    }
    __device__ __forceinline__ void add(float x, float r, float pivot)
    {
        if constexpr (NS == 1) m[0] += score_sq(x, r);
        else ssim_acc(m, x, r, pivot);
    }
};

// The lane's reference pixels for W columns of both rows of its pair: a float4 / float2, or one 32-bit / 16-bit word of 8-bit pixels, per row.
// Read once: streaming loads.
template <int W, bool F32> struct ScoreWord;
template <> struct ScoreWord<4, true> { typedef float4 type; };
template <> struct ScoreWord<2, true> { typedef float2 type; };
template <> struct ScoreWord<4, false> { typedef unsigned type; };
template <> struct ScoreWord<2, false> { typedef unsigned short type; };
__device__ __forceinline__ void score_unpack(float4 v, float (&x)[4]) { x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w; }
__device__ __forceinline__ void score_unpack(float2 v, float (&x)[2]) { x[0] = v.x; x[1] = v.y; }
__device__ __forceinline__ void score_unpack(unsigned v, float (&x)[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = (float)((v >> (8 * k)) & 255u);
}
__device__ __forceinline__ void score_unpack(unsigned short v, float (&x)[2]) { x[0] = (float)(v & 255u); x[1] = (float)(v >> 8); }
// `frames` from pixel px on, in the reference's type
template <bool F32> __device__ __forceinline__ const void* score_rows(const void* frames, long px)
{
    if constexpr (F32) return static_cast<const float*>(frames) + px;
    else return static_cast<const unsigned char*>(frames) + px;
}
template <int W, bool F32> struct ScoreRef {
    typedef typename ScoreWord<W, F32>::type Word;
    Word a, b;      // rows A and B
    // ia, ib: the lane's words of row A and of row B, counted from `rows` in words of W pixels (in the caller's index type: a 32-bit lane
    // offset from a uniform base, or a long)
    template <typename I> __device__ __forceinline__ void load(const void* rows, I ia, I ib)
    {
        const Word* src = static_cast<const Word*>(rows);
        if constexpr (F32) { a = ld_stream(&src[ia]); b = ld_stream(&src[ib]); }
        else { a = __builtin_nontemporal_load(&src[ia]); b = __builtin_nontemporal_load(&src[ib]); }
    }
};
__device__ __forceinline__ void score_store(float* p, const float (&r)[4]) { st_stream(reinterpret_cast<float4*>(p), make_float4(r[0], r[1], r[2], r[3])); }
__device__ __forceinline__ void score_store(float* p, const float (&r)[2]) { st_stream(reinterpret_cast<float2*>(p), make_float2(r[0], r[1])); }

// W pixels of one row into the sums, in column order
template <int W, int NS> __device__ __forceinline__ void score_row(ScoreAcc<NS>& acc, const float (&x)[W], const float (&r)[W], float pivot)
{
    static_assert(W == 2 || W == 4, "two or four pixels per lane and row");
    acc.add(x[0], r[0], pivot); acc.add(x[1], r[1], pivot);
    if constexpr (W == 4) { acc.add(x[2], r[2], pivot); acc.add(x[3], r[3], pivot); }
}

// One position of a lane: z[0 .. W) are W consecutive complex elements of the row pair's transform in LDS (adjacent in the padded layout), their
// real parts W pixels of row A, their imaginary parts of row B.  Forms the rounded reconstruction, stores it to oa / ob when `store` (uniform),
// and feeds the sums: row A's W pixels in column order, then row B's.
// The order of the statements is part of the result's bits.  Under -ffp-contract=fast a fresh sum's first addition t0 + t1 has two products and
// the back end fuses ONE of them into it -- the one the optimiser ranks first, and it ranks a term by where its inputs appear in the code.  With
// the reference unpacked first and both rows' pixels formed per element, every instantiation fuses the product it always has (the first
// column's, but for the x'^2 sum of the mixed-radix kernel's 8-bit SSIM instantiations): checked per instantiation in the optimised IR.
template <int W, bool F32, int NS>
__device__ __forceinline__ void score_position(const float2* z, float scale, const ScoreRef<W, F32>& ref, float pivot, bool store, float* oa, float* ob,
                                               ScoreAcc<NS>& acc)
{
    float2 v[W];
    float ra[W], rb[W], xa[W], xb[W];
    score_unpack(ref.a, xa);
    score_unpack(ref.b, xb);
#pragma unroll
    for (int k = 0; k < W; ++k) v[k] = z[k];
#pragma unroll
    for (int k = 0; k < W; ++k) { ra[k] = score_px(v[k].x, scale); rb[k] = score_px(v[k].y, scale); }
    score_row(acc, xa, ra, pivot);
    score_row(acc, xb, rb, pivot);
    if (store) {
        score_store(oa, ra);
        score_store(ob, rb);
    }
}

// the sum over an aligned segment of W lanes of a wave (W a power of two), in every lane of it: a butterfly, whose two partners add the same
// two numbers at every level -- one fixed order, the same bits in every lane
template <int W> __device__ __forceinline__ float score_seg_sum(float v)
{
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// the sum over an aligned segment of 1 << lw lanes of a wave (lw uniform, at most LMAX), in every lane of it: score_seg_sum's butterfly from the
// nearest partner outwards, as many levels as the segment has (a loop with a uniform bound)
template <int LMAX> __device__ __forceinline__ float score_seg_sum_rt(float v, int lw)
{
#pragma unroll
    for (int l = 0; l < LMAX; ++l)
        if (l < lw) v += __shfl_xor(v, 1 << l, 64);
    return v;
}
// The strip reduction (SCORE 3..6): a strip's positions lie in 1 << lw consecutive lanes, aligned; each of the lane's sums goes through the
// butterfly and the strip's first lane (`first`) writes it to dst[k * ms], ms the floats of one moment's plane.  Every lane of the wave calls it.
template <int LMAX, int NS> __device__ __forceinline__ void score_strip_reduce(const ScoreAcc<NS>& acc, int lw, bool first, float* dst, long ms)
{
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const float v = score_seg_sum_rt<LMAX>(acc.m[k], lw);
        if (first) dst[k * ms] = v;
    }
}

// Host: from a ScoreArg to f(std::integral_constant<int, SCORE>, the device struct of ScoreParam<SCORE>), the argument checked once.  n: the
// row length; out_u8: the caller asked for 8-bit rows, which no scoring instantiation writes.
template <typename F> hipError_t score_dispatch(const ScoreArg& a, int n, bool out_u8, F&& f)
{
    if (out_u8 || !a.frames) return hipErrorInvalidValue;
    if (!a.tile) {
        if (!a.part) return hipErrorInvalidValue;
        const ScoreDev d{a.frames, a.part};
        return a.u8 ? f(std::integral_constant<int, 2>{}, d) : f(std::integral_constant<int, 1>{}, d);
    }
    const int lt = score_tile_log2(a.tile);
    if (!a.strips || lt < 0 || n % a.tile) return hipErrorInvalidValue;
    if (a.ssim) {
        const ScoreSsimDev d{a.frames, a.strips, lt, a.pivot};
        return a.u8 ? f(std::integral_constant<int, 6>{}, d) : f(std::integral_constant<int, 5>{}, d);
    }
    const ScoreMapDev d{a.frames, a.strips, lt};
    return a.u8 ? f(std::integral_constant<int, 4>{}, d) : f(std::integral_constant<int, 3>{}, d);
}

}  // namespace aefft
