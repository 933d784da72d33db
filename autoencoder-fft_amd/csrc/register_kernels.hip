// Translation by phase correlation: the three kernels around the two transforms of aefft_frames_register / aefft_frames_register_ref (gfx950;
// include/aefft.h has the definition, DESIGN.md section 31 the route and the measurement).  n = Nx Ny cells of a frame, cell p = i Ny + j;
// Nyr = Ny / 2 + 1 bins of a spectrum row.  Nx and Ny are even, so n is a multiple of 4 and every plane starts on 16 bytes.
//   register_prepare_kernel  g[b][i][j] = wx[i] wy[j] sum_d p[b][d][i][j].  A lane owns four consecutive elements of a row pair (2 Ny contiguous
//                            elements, a multiple of 4: one 16-byte load a channel from float frames, one dword from 8-bit ones, one 16-byte
//                            store); 256 lanes a workgroup pass, the passes grid-strided.  The two Hann tables are built once a workgroup in LDS.
//   register_cross_kernel    a lane owns a bin: Q = A conj(B) / (|A| |B|) over the kept bins, 0 elsewhere, written over the image spectrum.  The
//                            kept-bin rule is two compares on indices.  Each modulus by rsqrt and one Newton step, so that no product of two
//                            moduli is formed (|A|^2 |B|^2 leaves the float range for 8-bit frames of 2048 x 2048).
//   register_peak1_kernel    ceil(n / 4096) workgroups an image: every lane keeps the largest 64-bit key {order-preserving image of s : ~p} of its
//                            sixteen cells (four 16-byte loads ahead of their compares), the keys meet in LDS by a tree of integer max, one
//                            partial a workgroup.  The largest key is the largest value at the smallest index.
//   register_peak2_kernel    a workgroup an image: the partials meet the same way, 25 lanes gather the 5 x 5 circular neighbourhood, lane 0 forms
//                            the centroid in double in a fixed order and writes the shift and, where asked for, the affine.
// No atomics, no workgroup waits for another; every result is a function of the inputs alone.
// tools/register_hostcheck.cpp compiles this file for the host (AEFFT_HOSTCHECK: tools/hostlanes.h supplies the launch variables and the barrier).
#ifndef AEFFT_HOSTCHECK
#include "internal.h"
#define RG_HD __device__ __forceinline__
#endif

namespace aefft {

constexpr int RG_HANN = 0, RG_NOWINDOW = 1;                                      // AEFFT_REGISTER_HANN, AEFFT_REGISTER_NOWINDOW
constexpr int RG_LANES = 256;
constexpr int RG_CHUNK = 4096;                                                   // cells of a stage-one workgroup: 16 a lane
constexpr int RG_MAX_GRID = 2048;                                                // workgroups of the prepare launch at the most
constexpr int RG_PEAK_WORDS = 2 * RG_LANES + 32;                                 // LDS of the peak kernels, in words: a key a lane, the neighbourhood

typedef unsigned long long rg_u64;
struct __attribute__((aligned(8))) rg_f2 { float x, y; };
struct RgShift { float dx, dy, response; int cell; };                            // aefft_shift
struct RgAffine { long long a[6]; };                                             // aefft_affine

struct RgArgs {
    const void* frames;                                                          // prepare: [B][D][Nx][Ny], 8-bit or float
    float* planes;                                                               // prepare: [B][Nx][Ny]
    rg_f2* spec;                                                                 // cross: [B][Nx][Nyr], the image spectra in, Q out
    const rg_f2* ref;                                                            // cross: [nref][Nx][Nyr]
    const float* surf;                                                           // peak: [B][Nx][Ny]
    rg_u64* part;                                                                // peak: [B][nparts]
    RgShift* shift;                                                              // [B]
    RgAffine* affine;                                                            // [B] or null
    int B, D, Nx, Ny, window, nref;
    int umax, vmax, low;                                                         // kept: |u| <= umax, |v| <= vmax, not (|u| <= low and |v| <= low)
    int nparts;
    float min_response;
    double sx, sy;
};

RG_HD float rg_float(unsigned u) { float v; __builtin_memcpy(&v, &u, 4); return v; }
RG_HD unsigned rg_bits(float v) { unsigned u; __builtin_memcpy(&u, &v, 4); return u; }
// the order-preserving image of a float's bits among unsigned ints (calib_kernels.hip's cb_ord, restated)
RG_HD unsigned rg_ord(unsigned u) { return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u); }

// the periodic Hann window
RG_HD float rg_hann(int n, int N) { return 0.5f - 0.5f * __builtin_cosf(6.283185307179586f * (float)n / (float)N); }

// 1 / sqrt(x) for x > 0: the back end's estimate and one Newton step
#ifndef AEFFT_HOSTCHECK
RG_HD float rg_rsqrt0(float x) { return __builtin_amdgcn_rsqf(x); }
#else
RG_HD float rg_rsqrt0(float x) { return 1.0f / __builtin_sqrtf(x); }
#endif
RG_HD float rg_rsqrt(float x)
{
    const float r = rg_rsqrt0(x);
    return r * (1.5f - 0.5f * x * r * r);
}

// ---- prepare --------------------------------------------------------------------------------
template <int D, bool U8> RG_HD void register_prepare_body(const RgArgs& g, unsigned blk, unsigned nblk, unsigned* lds)
{
    const int t = (int)threadIdx.x, Nx = g.Nx, Ny = g.Ny;
    float* wx = reinterpret_cast<float*>(lds);                                   // [Nx], then wy [Ny]
    float* wy = wx + Nx;
    const bool hann = g.window == RG_HANN;
    if (hann) {
        for (int n = t; n < Nx + Ny; n += RG_LANES) wx[n] = n < Nx ? rg_hann(n, Nx) : rg_hann(n - Nx, Ny);
        __syncthreads();
    }
    const unsigned hq = (unsigned)Ny / 2, hx = (unsigned)Nx / 2;                   // quads of a row pair, row pairs of an image
    const unsigned total = (unsigned)g.B * hx * hq;                              // (B Nx Ny / 4 < 2^29)
    for (unsigned q = blk * RG_LANES + (unsigned)t; q < total; q += nblk * RG_LANES) {
        const unsigned rp = q / hq, e = 4 * (q - rp * hq);                       // the row pair over the batch; the quad's first element in it
        const unsigned b = rp / hx, i0 = 2 * (rp - b * hx);
        float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const size_t off = (((size_t)b * D + d) * Nx + i0) * Ny + e;         // (a multiple of 4)
            if (U8) {
                const unsigned w = *reinterpret_cast<const unsigned*>(static_cast<const unsigned char*>(g.frames) + off);
                s[0] += (float)(w & 255u); s[1] += (float)((w >> 8) & 255u); s[2] += (float)((w >> 16) & 255u); s[3] += (float)(w >> 24);
            } else {
                const float4 v = *reinterpret_cast<const float4*>(static_cast<const float*>(g.frames) + off);
                s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
            }
        }
        if (hann) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const unsigned up = e + c >= (unsigned)Ny ? 1u : 0u;               // (Ny = 2 mod 4: a quad may straddle the pair's two rows)
                s[c] = (wx[i0 + up] * wy[e + c - up * Ny]) * s[c];
            }
        }
        *reinterpret_cast<float4*>(g.planes + ((size_t)b * Nx + i0) * Ny + e) = make_float4(s[0], s[1], s[2], s[3]);
    }
}

// ---- cross-power ----------------------------------------------------------------------------
// bpi: the workgroups of an image
RG_HD void register_cross_body(const RgArgs& g, unsigned blk, unsigned bpi)
{
    const int Nx = g.Nx, Nyr = g.Ny / 2 + 1;
    const unsigned b = blk / bpi, bin = (blk - b * bpi) * RG_LANES + threadIdx.x;
    if (bin >= (unsigned)(Nx * Nyr)) return;
    const int i = (int)(bin / (unsigned)Nyr), v = (int)bin - i * Nyr;              // (v = |v|: the half spectrum holds j <= Ny / 2)
    const int u = i < Nx - i ? i : Nx - i;
    const size_t at = (size_t)b * Nx * Nyr + bin;
    rg_f2 q = {0.f, 0.f};
    if (u <= g.umax && v <= g.vmax && !(u <= g.low && v <= g.low)) {
        const rg_f2 a = g.spec[at], r = g.ref[(g.nref == 1 ? (size_t)0 : (size_t)b * Nx * Nyr) + bin];
        const float na = a.x * a.x + a.y * a.y, nr = r.x * r.x + r.y * r.y;
        if (na > 0.f && nr > 0.f && na < 3.0e38f && nr < 3.0e38f) {              // (a NaN or an infinity: Q = 0)
            const float k = rg_rsqrt(na) * rg_rsqrt(nr);
            q.x = (a.x * r.x + a.y * r.y) * k;
            q.y = (a.y * r.x - a.x * r.y) * k;
        }
    }
    g.spec[at] = q;
}

// ---- peak -----------------------------------------------------------------------------------
// the lanes' keys meet: the largest in key[0], seen by every lane
RG_HD rg_u64 rg_meet(rg_u64* key, int t, rg_u64 mine)
{
    key[t] = mine;
    __syncthreads();
    for (int d = RG_LANES / 2; d >= 1; d >>= 1) {
        if (t < d) { const rg_u64 a = key[t], c = key[t + d]; key[t] = a > c ? a : c; }
        __syncthreads();
    }
    return key[0];
}

RG_HD rg_u64 rg_key(float v, unsigned p)
{
    unsigned u = rg_bits(v);
    if (u == 0x80000000u) u = 0;                                                 // -0 counts as +0
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0;                               // NaN: below every cell's key (the image of -inf is 0x007FFFFF)
    return ((rg_u64)rg_ord(u) << 32) | (unsigned)~p;
}

RG_HD void register_peak1_body(const RgArgs& g, unsigned blk, unsigned* lds)
{
    const int t = (int)threadIdx.x;
    const unsigned n = (unsigned)(g.Nx * g.Ny), b = blk / (unsigned)g.nparts, part = blk - b * (unsigned)g.nparts;
    const float* s = g.surf + (size_t)b * n;
    float4 v[4];
    unsigned p[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        p[k] = part * RG_CHUNK + 4u * (unsigned)(k * RG_LANES + t);
        v[k] = p[k] < n ? *reinterpret_cast<const float4*>(s + p[k]) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    rg_u64 best = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (p[k] >= n) continue;
        const float c[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const rg_u64 mine = rg_key(c[e], p[k] + e);
            best = mine > best ? mine : best;
        }
    }
    best = rg_meet(reinterpret_cast<rg_u64*>(lds), t, best);
    if (t == 0) g.part[blk] = best;
}

// rint(v) as an offset of the affine: a whole number of at most 2^39 in magnitude, or 0 for what is none (a NaN out of non-finite frames)
RG_HD long long rg_offset(double v)
{
    const double r = __builtin_rint(v);
    return r >= -549755813888.0 && r <= 549755813888.0 ? (long long)r : 0;
}

RG_HD void register_peak2_body(const RgArgs& g, unsigned b, unsigned* lds)
{
    const int t = (int)threadIdx.x, Nx = g.Nx, Ny = g.Ny;
    const float* s = g.surf + (size_t)b * Nx * Ny;
    float* nb = reinterpret_cast<float*>(lds + 2 * RG_LANES);                    // the neighbourhood [5][5]
    rg_u64 best = 0;
    for (int k = t; k < g.nparts; k += RG_LANES) {
        const rg_u64 c = g.part[(size_t)b * g.nparts + k];
        best = c > best ? c : best;
    }
    const rg_u64 win = rg_meet(reinterpret_cast<rg_u64*>(lds), t, best);
    const int p = win ? (int)~(unsigned)win : 0;                                 // (a surface of NaN only: cell 0)
    const int pi = p / Ny, pj = p - pi * Ny;
    if (t < 25) {
        const int di = t / 5 - 2, dj = t % 5 - 2;
        const int i = (pi + di + Nx) % Nx, j = (pj + dj + Ny) % Ny;              // (Nx, Ny >= 8)
        nb[t] = s[i * Ny + j];
    }
    __syncthreads();
    if (t != 0) return;
    double sw = 0.0, si = 0.0, sj = 0.0;                                         // ascending di, then dj; w di is exact, so fused or not, the same bits
    for (int k = 0; k < 25; ++k) {
        const double w = nb[k] > 0.f ? (double)nb[k] : 0.0;
        sw = sw + w;
        si = si + w * (double)(k / 5 - 2);
        sj = sj + w * (double)(k % 5 - 2);
    }
    double dx = (double)pi + (sw > 0.0 ? si / sw : 0.0), dy = (double)pj + (sw > 0.0 ? sj / sw : 0.0);
    if (dx >= (double)(Nx / 2)) dx -= (double)Nx;
    if (dy >= (double)(Ny / 2)) dy -= (double)Ny;
    RgShift out;
    out.dx = (float)dx; out.dy = (float)dy; out.response = nb[12]; out.cell = p;
    g.shift[b] = out;
    if (!g.affine) return;
    RgAffine a = {{16777216, 0, 0, 0, 16777216, 0}};
    if (out.response >= g.min_response) {                                        // (false for NaN)
        a.a[2] = rg_offset((double)out.dx * g.sx * 16777216.0);
        a.a[5] = rg_offset((double)out.dy * g.sy * 16777216.0);
    }
    g.affine[b] = a;
}

// ---- sizes (host arithmetic) ----------------------------------------------------------------
// a size the per-bin ops take: a power of two in 8..2048 or an even smooth size in 10..2048
static inline bool rg_size(int n)
{
    if (n < 8 || n > 2048 || (n & 1)) return false;
    while (n % 2 == 0) n /= 2;
    while (n % 3 == 0) n /= 3;
    while (n % 5 == 0) n /= 5;
    return n == 1;
}
static inline size_t rg_round16(size_t v) { return (v + 15) & ~(size_t)15; }
static inline int rg_parts(int Nx, int Ny) { return (Nx * Ny + RG_CHUNK - 1) / RG_CHUNK; }
// the workspace: the planes (later the surface) | the image spectra | the peak partials; 0 for what the calls do not take
static inline size_t rg_workspace(int Nx, int Ny, int B, size_t* spec_at = nullptr, size_t* part_at = nullptr)
{
    if (!rg_size(Nx) || !rg_size(Ny) || B < 1 || (long long)B * Nx * Ny > 0x1fffffffLL) return 0;
    const size_t planes = rg_round16((size_t)4 * B * Nx * Ny), spec = rg_round16((size_t)8 * B * Nx * (Ny / 2 + 1));
    if (spec_at) *spec_at = planes;
    if (part_at) *part_at = planes + spec;
    return planes + spec + rg_round16((size_t)8 * B * rg_parts(Nx, Ny));
}
// the kept bins of the FULL Nx x Ny spectrum and the index limits the cross-power kernel compares with; -1 for a cutoff outside (0, 1]
static inline long long rg_kept(int Nx, int Ny, int window, float cutoff, int* umax, int* vmax, int* low)
{
    if (!(cutoff > 0.f) || !(cutoff <= 1.f)) return -1;
    const int um = (int)((double)cutoff * Nx / 2.0), vm = (int)((double)cutoff * Ny / 2.0);      // 2 |u| <= cutoff Nx (the product is exact)
    const int lw = window == RG_HANN ? 1 : 0;
    auto count = [](int m, int N) { return (long long)(m >= N / 2 ? N : 2 * m + 1); };           // the indices of an axis with |u| <= m
    *umax = um; *vmax = vm; *low = lw;
    return count(um, Nx) * count(vm, Ny) - count(um < lw ? um : lw, Nx) * count(vm < lw ? vm : lw, Ny);
}

#ifndef AEFFT_HOSTCHECK
template <int D, bool U8> __global__ __launch_bounds__(RG_LANES) void register_prepare_kernel(const RgArgs g)
{
    extern __shared__ __attribute__((aligned(16))) unsigned rg_lds[];
    register_prepare_body<D, U8>(g, blockIdx.x, gridDim.x, rg_lds);
}
__global__ __launch_bounds__(RG_LANES) void register_cross_kernel(const RgArgs g, unsigned bpi) { register_cross_body(g, blockIdx.x, bpi); }
__global__ __launch_bounds__(RG_LANES) void register_peak1_kernel(const RgArgs g)
{
    __shared__ __attribute__((aligned(16))) unsigned lds[RG_PEAK_WORDS];
    register_peak1_body(g, blockIdx.x, lds);
}
__global__ __launch_bounds__(RG_LANES) void register_peak2_kernel(const RgArgs g)
{
    __shared__ __attribute__((aligned(16))) unsigned lds[RG_PEAK_WORDS];
    register_peak2_body(g, blockIdx.x, lds);
}

static_assert(sizeof(RgShift) == sizeof(aefft_shift) && sizeof(RgAffine) == sizeof(aefft_affine), "the kernels' structures are the header's");

size_t register_workspace(int Nx, int Ny, int B, size_t* spec_at, size_t* part_at) { return rg_workspace(Nx, Ny, B, spec_at, part_at); }
long long register_kept(int Nx, int Ny, int window, float cutoff, int* umax, int* vmax, int* low) { return rg_kept(Nx, Ny, window, cutoff, umax, vmax, low); }

static bool rg_geometry(int Nx, int Ny, int B, int window, RgArgs* g)
{
    if (!rg_workspace(Nx, Ny, B) || (window != RG_HANN && window != RG_NOWINDOW)) return false;
    *g = RgArgs();
    g->B = B; g->Nx = Nx; g->Ny = Ny; g->window = window; g->nparts = rg_parts(Nx, Ny);
    return true;
}

template <int D> static void rg_prepare(const RgArgs& g, int u8, unsigned grid, size_t lds, hipStream_t st)
{
    if (u8) register_prepare_kernel<D, true><<<dim3(grid), dim3(RG_LANES), lds, st>>>(g);
    else register_prepare_kernel<D, false><<<dim3(grid), dim3(RG_LANES), lds, st>>>(g);
}

hipError_t launch_register_prepare(const void* frames, int frames_u8, float* planes, int B, int D, int Nx, int Ny, int window, hipStream_t st)
{
    RgArgs g;
    if (!frames || !planes || D < 1 || D > 4 || !rg_geometry(Nx, Ny, B, window, &g) || (long long)B * D * Nx * Ny > 0x7fffffffLL) return hipErrorInvalidValue;
    g.frames = frames; g.planes = planes; g.D = D;
    const unsigned passes = (unsigned)(((size_t)B * Nx * Ny / 4 + RG_LANES - 1) / RG_LANES);
    const unsigned grid = passes < (unsigned)RG_MAX_GRID ? passes : (unsigned)RG_MAX_GRID;
    const size_t lds = window == RG_HANN ? (size_t)4 * (Nx + Ny) : 0;            // (at most 16 KB)
    switch (D) {
    case 1: rg_prepare<1>(g, frames_u8, grid, lds, st); break;
    case 2: rg_prepare<2>(g, frames_u8, grid, lds, st); break;
    case 3: rg_prepare<3>(g, frames_u8, grid, lds, st); break;
    default: rg_prepare<4>(g, frames_u8, grid, lds, st); break;
    }
    return hipGetLastError();
}

hipError_t launch_register_cross(float2* spec, const float2* ref, int nref, int B, int Nx, int Ny, int window, int umax, int vmax, int low, hipStream_t st)
{
    RgArgs g;
    if (!spec || !ref || (nref != 1 && nref != B) || !rg_geometry(Nx, Ny, B, window, &g)) return hipErrorInvalidValue;
    g.spec = reinterpret_cast<rg_f2*>(spec); g.ref = reinterpret_cast<const rg_f2*>(ref); g.nref = nref;
    g.umax = umax; g.vmax = vmax; g.low = low;
    const unsigned bpi = (unsigned)((Nx * (Ny / 2 + 1) + RG_LANES - 1) / RG_LANES);   // (B bpi < 2^31: B Nx Ny < 2^29)
    register_cross_kernel<<<dim3((unsigned)B * bpi), dim3(RG_LANES), 0, st>>>(g, bpi);
    return hipGetLastError();
}

hipError_t launch_register_peak(const float* surf, void* part, int B, int Nx, int Ny, float min_response, double scale_x, double scale_y, aefft_shift* shift,
                                aefft_affine* affine, hipStream_t st)
{
    RgArgs g;
    if (!surf || !part || !shift || !rg_geometry(Nx, Ny, B, RG_HANN, &g)) return hipErrorInvalidValue;
    g.surf = surf; g.part = static_cast<rg_u64*>(part); g.shift = reinterpret_cast<RgShift*>(shift); g.affine = reinterpret_cast<RgAffine*>(affine);
    g.min_response = min_response; g.sx = scale_x; g.sy = scale_y;
    register_peak1_kernel<<<dim3((unsigned)(B * g.nparts)), dim3(RG_LANES), 0, st>>>(g);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    register_peak2_kernel<<<dim3((unsigned)B), dim3(RG_LANES), 0, st>>>(g);
    return hipGetLastError();
}
#endif

}  // namespace aefft
