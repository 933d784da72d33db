// The degraded input of target training (gfx950): aefft_frames_degrade -- frames [B][D][Nx][Ny] (8-bit, or float through px_u8) -> the binomial blur of
// radius R in 0..4, the Irwin-Hall noise and the impulses keyed by Philox4x32-10 on (seed, first_frame + b, the element's linear index) -> frames of the
// same shape, 8-bit or float, in one launch.  All-integer arithmetic behind the two quantisations of dg_quantise (include/aefft.h states the formulas):
// every route gives the same bytes as a numpy restatement.
//   degrade_kernel<R, SF32, DF32, WORDS>   R: the blur's radius; SF32 / DF32: a float source / destination; WORDS: Ny % 4 == 0, the frame side moves
//                                          dwords (float4 of float frames), single elements otherwise
// A lane owns a QUAD: four elements that follow each other along j.
//   R == 0   element-wise, no LDS, no barrier.  The quads are counted off along the frame's linear index n, so a quad starts on a multiple of 4 of n
//            on both routes and two Philox calls (counters n/2 and n/2 + 1) serve it.  grid.x: 256 quads each; grid.y x grid.z: the frames.
//   R > 0    a workgroup (256 threads) owns a tile of DG_TI = 32 rows (i) x DG_TJ = 64 columns (j) of one plane.  grid.x: D x the tiles of a plane.
//     1. The source rows i0 - R .. i0 + 32 + R (clamped to the plane: edges replicated) are staged in LDS as bytes, 72 per row: the columns
//        j0 - 4 .. j0 + 68 (clamped), 18 dwords -- a dword of the frame each when WORDS (a float4 through px_u8; beyond the plane's columns the
//        edge byte of the nearest dword, replicated), built from single elements otherwise.  A lane loads its three dwords before it stores one.
//     2. Along i: a lane owns one staged dword column of one row, item = 18 i + w: tap k is the dword at item + 18 k, so the 64 lanes of a wave read
//        64 consecutive dwords -- no bank conflict on the [i][j] tile whatever R is.  The four bytes are summed as two packed 16-bit pairs
//        (255 * 4^R < 2^16) and leave as four dwords H[i][4 w ..], one 16-byte store.
//     3. Along j: a lane owns a quad of one row, reads the 4 + 2 R dwords it needs of H[i][4 q .. 4 q + 12) (consecutive lanes: consecutive
//        16-byte groups) and forms its four sums v <= 255 * 16^R < 2^24; u = v << (16 - 4 R).
//     With WORDS a quad starts on a multiple of 4 of n (two Philox calls); otherwise its n has any parity and every element makes its own call.
// The noise of one element: T = the sum of six bytes - 765 (two packed byte sums), u += T m; the impulse replaces it when c >> 16 < t.  The key
// schedule and the counter's frame words are the same in the whole launch: scalar registers.  Each round's two products are one 32 x 32 -> 64-bit
// multiply each.  When m == 0 and t == 0 (a blur alone, or the copy) the launch makes no Philox call at all.
// No scratch, no atomics, no workspace.  The kernel bodies are plain C++ over (threadIdx, blockIdx, gridDim, __syncthreads) and an LDS pointer:
// tools/degrade_hostcheck.cpp compiles this file for the host, threads as lanes, under the sanitizers (AEFFT_HOSTCHECK: tools/hostlanes.h and the program supply those
// names, px_u8 and the byte sum, and leaves the launcher out).
#include <math.h>
#ifndef AEFFT_HOSTCHECK
#include "internal.h"
#include "fft_common.h"
#define DG_HD __device__ __forceinline__
#define DG_BYTESUM(x, acc) __builtin_amdgcn_sad_u8((x), 0u, (acc))     // acc + the sum of the four bytes of x (v_sad_u8 against 0)
#endif

namespace aefft {

constexpr int DG_TI = 32;                        // rows (i) of a tile
constexpr int DG_TJ = 64;                        // columns (j) of a tile: 16 quads
constexpr int DG_SW = DG_TJ / 4 + 2;             // staged dwords of a row: the tile's and one on either side (the halo, R <= 4)
constexpr int DG_HP = 4 * DG_SW;                 // dwords of a row of H: one per staged byte

struct DgArgs {
    const void* src; void* dst;
    int B, D, Nx, Ny;
    unsigned P;                                  // elements of a frame, D Nx Ny (<= 2^28)
    int tj, tiles;                               // tiles along j; tiles of a plane
    int m, t;                                    // the noise's multiplier and the impulses' threshold (dg_quantise)
    unsigned k0, k1;                             // the key: seed's low and high word
    unsigned long long first;                    // frame b is frame first + b of the stream (wrapping)
};
// LDS of a launch with R > 0, in dwords: the staged rows and H
constexpr int dg_lds_words(int R) { return R == 0 ? 0 : (DG_TI + 2 * R) * DG_SW + DG_TI * DG_HP; }

// the host's two quantisations (include/aefft.h steps 4 and 5): sigma in 0..255 -> m <= 92322, impulse in 0..1 -> t in 0..65536
static inline void dg_quantise(float sigma, float impulse, int* m, int* t)
{
    *m = (int)floor(((double)sigma * 65536.0) / sqrt(32767.5) + 0.5);
    *t = (int)floor((double)impulse * 65536.0 + 0.5);
}

struct DgWords { unsigned x, y, z, w; };
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC11): counter (c0, c1, c2, c3), key (k0, k1)
DG_HD DgWords dg_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;                                    // (the same in every lane)
    }
    DgWords o;
    o.x = c0; o.y = c1; o.z = c2; o.w = c3;
    return o;
}
// steps 4 and 5 for one element with its words (a, c)
DG_HD int dg_disturb(int u, unsigned a, unsigned c, int m, int t)
{
    const int T = (int)DG_BYTESUM(a, DG_BYTESUM(c & 0xffffu, 0u)) - 765;
    u += T * m;                                                                  // (|u| < 2^27)
    if ((int)(c >> 16) < t) u = (a & 1u) ? 255 << 16 : 0;
    return u;
}
// steps 3 to 5 for the quad n0 .. n0 + 3 of frame (g0, g1), `live` of them inside the frame.  PAIRS: n0 % 4 == 0
template <bool PAIRS>
DG_HD void dg_disturb4(int* u, unsigned n0, int live, const DgArgs& a, unsigned g0, unsigned g1)
{
    if ((a.m | a.t) == 0) return;
    if (PAIRS) {
        const DgWords x = dg_philox(n0 >> 1, 0u, g0, g1, a.k0, a.k1), y = dg_philox((n0 >> 1) + 1u, 0u, g0, g1, a.k0, a.k1);
        u[0] = dg_disturb(u[0], x.x, x.y, a.m, a.t);
        u[1] = dg_disturb(u[1], x.z, x.w, a.m, a.t);
        u[2] = dg_disturb(u[2], y.x, y.y, a.m, a.t);
        u[3] = dg_disturb(u[3], y.z, y.w, a.m, a.t);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e >= live) break;
            const unsigned n = n0 + (unsigned)e;
            const DgWords x = dg_philox(n >> 1, 0u, g0, g1, a.k0, a.k1);
            u[e] = dg_disturb(u[e], (n & 1u) ? x.z : x.x, (n & 1u) ? x.w : x.y, a.m, a.t);
        }
    }
}
// clamp((u + 32768) >> 16, 0, 255).  The clamp is taken in Q16, BEFORE the shift: the byte is then bits 16..23 of a non-negative value, and the
// four bytes of a quad are packed by plain shifts and masks
DG_HD unsigned dg_px(int u)
{
    const int v = u + 32768;
    const unsigned c = (unsigned)(v < 0 ? 0 : v > 0xffffff ? 0xffffff : v);
    return c >> 16;
}
// the source quad at element offset o as four bytes of a dword; WORDS: o is a multiple of 4 and the four are live
template <bool SF32, bool WORDS>
DG_HD unsigned dg_load4(const void* src, size_t o, int live)
{
    if (WORDS) {
        if (SF32) {
            const float4 f = *reinterpret_cast<const float4*>(static_cast<const float*>(src) + o);
            return px_u8(f.x) | px_u8(f.y) << 8 | px_u8(f.z) << 16 | px_u8(f.w) << 24;
        }
        return *reinterpret_cast<const unsigned*>(static_cast<const unsigned char*>(src) + o);
    }
    unsigned v = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (e < live) v |= (SF32 ? px_u8(static_cast<const float*>(src)[o + e]) : (unsigned)static_cast<const unsigned char*>(src)[o + e]) << (8 * e);
    return v;
}
// step 6 for a quad
template <bool DF32, bool WORDS>
DG_HD void dg_store4(void* dst, size_t o, int live, const int* u)
{
    if (DF32) {
        float* p = static_cast<float*>(dst) + o;
        if (WORDS) {
            float4 f;
            f.x = (float)u[0] * (1.0f / 65536.0f); f.y = (float)u[1] * (1.0f / 65536.0f);
            f.z = (float)u[2] * (1.0f / 65536.0f); f.w = (float)u[3] * (1.0f / 65536.0f);
            *reinterpret_cast<float4*>(p) = f;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < live) p[e] = (float)u[e] * (1.0f / 65536.0f);
        }
    } else {
        unsigned char* p = static_cast<unsigned char*>(dst) + o;
        if (WORDS) *reinterpret_cast<unsigned*>(p) = dg_px(u[0]) | dg_px(u[1]) << 8 | dg_px(u[2]) << 16 | dg_px(u[3]) << 24;
        else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < live) p[e] = (unsigned char)dg_px(u[e]);
        }
    }
}

// ---- R == 0: element-wise -------------------------------------------------------------------------
template <bool SF32, bool DF32, bool WORDS>
__device__ __forceinline__ void degrade_flat_body(const DgArgs& a)
{
    const size_t b = (size_t)blockIdx.z * gridDim.y + blockIdx.y;               // grid.y, grid.z: the frames
    if (b >= (size_t)a.B) return;
    const unsigned n0 = 4u * ((unsigned)blockIdx.x * 256u + (unsigned)threadIdx.x);   // (at most 2^28 + 1024)
    if (n0 >= a.P) return;
    const int live = a.P - n0 < 4u ? (int)(a.P - n0) : 4;                        // (4 when WORDS: P is a multiple of 4)
    const size_t o = b * (size_t)a.P + n0;
    const unsigned long long g = a.first + b;
    const unsigned p = dg_load4<SF32, WORDS>(a.src, o, live);
    int u[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) u[e] = (int)((p >> (8 * e)) & 255u) << 16;
    dg_disturb4<true>(u, n0, live, a, (unsigned)g, (unsigned)(g >> 32));
    dg_store4<DF32, WORDS>(a.dst, o, live, u);
}

// ---- R > 0: the blur in LDS -----------------------------------------------------------------------
// w_k = C(2 R, k)
DG_HD unsigned dg_weight(int R, int k)
{
    unsigned w = 1;
    for (int s = 0; s < k; ++s) w = w * (unsigned)(2 * R - s) / (unsigned)(s + 1);
    return w;
}
DG_HD int dg_clamp(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

template <int R, bool SF32, bool DF32, bool WORDS>
__device__ __forceinline__ void degrade_tile_body(const DgArgs& a, unsigned* lds)
{
    unsigned* S = lds;                                                           // [DG_TI + 2 R][DG_SW]: byte jj of a row is column j0 - 4 + jj
    unsigned* H = lds + (DG_TI + 2 * R) * DG_SW;                                 // [DG_TI][DG_HP]
    const int tid = (int)threadIdx.x;
    const int d = (int)blockIdx.x / a.tiles, tile = (int)blockIdx.x - d * a.tiles;
    const int ti = tile / a.tj, i0 = ti * DG_TI, j0 = (tile - ti * a.tj) * DG_TJ;
    const size_t b = (size_t)blockIdx.z * gridDim.y + blockIdx.y;               // grid.y, grid.z: the frames
    if (b >= (size_t)a.B) return;
    const size_t plane = (b * a.D + d) * (size_t)a.Nx * a.Ny;
    // 1. the staged rows: a lane's (at most three) dwords are ALL loaded before the first goes to LDS -- no branch on the way, so the loads are in
    // flight together (one trip to memory per tile, not one per dword).  A dword beyond the plane's columns is the nearest dword inside with its
    // edge byte replicated; a lane beyond the items loads the last item again and stores nothing
    constexpr int ITEMS = (DG_TI + 2 * R) * DG_SW, NS = (ITEMS + 255) / 256;
    unsigned sv[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int idx = tid + 256 * s < ITEMS ? tid + 256 * s : ITEMS - 1;
        const int ii = idx / DG_SW, w = idx - ii * DG_SW;
        const int j = j0 - 4 + 4 * w;
        const size_t row = plane + (size_t)dg_clamp(i0 - R + ii, a.Nx - 1) * a.Ny;
        unsigned v;
        if (WORDS) {                                                             // (Ny and j multiples of 4: a dword is wholly inside or wholly outside)
            v = dg_load4<SF32, true>(a.src, row + dg_clamp(j, a.Ny - 4), 4);
            unsigned edge = j < 0 ? v & 255u : v >> 24;
            edge |= edge << 8; edge |= edge << 16;
            v = j < 0 || j >= a.Ny ? edge : v;
        } else {
            v = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) v |= dg_load4<SF32, false>(a.src, row + dg_clamp(j + e, a.Ny - 1), 1) << (8 * e);
        }
        sv[s] = v;
    }
#pragma unroll
    for (int s = 0; s < NS; ++s)
        if (tid + 256 * s < ITEMS) S[tid + 256 * s] = sv[s];
    __syncthreads();
    // 2. along i: bytes 0 and 2 of the dword in one packed sum, bytes 1 and 3 in the other (each at most 255 * 4^R < 2^16)
    for (int idx = tid; idx < DG_TI * DG_SW; idx += 256) {
        unsigned e02 = 0, e13 = 0;
#pragma unroll
        for (int k = 0; k <= 2 * R; ++k) {
            const unsigned v = S[idx + DG_SW * k], w = dg_weight(R, k);
            e02 += w * (v & 0x00ff00ffu);
            e13 += w * ((v >> 8) & 0x00ff00ffu);
        }
        unsigned* h = H + 4 * idx;
        h[0] = e02 & 0xffffu; h[1] = e13 & 0xffffu; h[2] = e02 >> 16; h[3] = e13 >> 16;
    }
    __syncthreads();
    // 3. along j, and steps 3 to 6
    const unsigned long long g = a.first + b;
    for (int it = tid; it < DG_TI * (DG_TJ / 4); it += 256) {
        const int i = it / (DG_TJ / 4), q = it - i * (DG_TJ / 4);
        const unsigned* h = H + i * DG_HP + 4 * q;                               // h[4 + e + l - R]: column j0 + 4 q + e + l - R
        unsigned hh[12];
#pragma unroll
        for (int s = 0; s < 12; ++s) hh[s] = h[s];
        int u[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            unsigned v = 0;
#pragma unroll
            for (int l = 0; l <= 2 * R; ++l) v += dg_weight(R, l) * hh[4 + e + l - R];
            u[e] = (int)(v << (16 - 4 * R));
        }
        const int gi = i0 + i, gj = j0 + 4 * q;
        if (gi >= a.Nx || gj >= a.Ny) continue;
        const int live = a.Ny - gj < 4 ? a.Ny - gj : 4;
        const unsigned n0 = ((unsigned)d * a.Nx + gi) * (unsigned)a.Ny + gj;
        dg_disturb4<WORDS>(u, n0, live, a, (unsigned)g, (unsigned)(g >> 32));
        dg_store4<DF32, WORDS>(a.dst, plane + (size_t)gi * a.Ny + gj, live, u);
    }
}

static inline DgArgs dg_geometry(const void* src, void* dst, int B, int D, int Nx, int Ny, float sigma, float impulse,
                                 unsigned long long seed, unsigned long long first_frame)
{
    DgArgs g;
    g.src = src; g.dst = dst; g.B = B; g.D = D; g.Nx = Nx; g.Ny = Ny;
    g.P = (unsigned)D * (unsigned)Nx * (unsigned)Ny;
    g.tj = (Ny + DG_TJ - 1) / DG_TJ; g.tiles = g.tj * ((Nx + DG_TI - 1) / DG_TI);
    dg_quantise(sigma, impulse, &g.m, &g.t);
    g.k0 = (unsigned)seed; g.k1 = (unsigned)(seed >> 32); g.first = first_frame;
    return g;
}
// grid.x of a launch: 256 quads each for R == 0, D x the tiles of a plane otherwise (at most 2^18 and 2^17)
static inline unsigned dg_grid_x(int R, const DgArgs& g) { return R == 0 ? (g.P / 4u + (g.P % 4u ? 1u : 0u) + 255u) / 256u : (unsigned)g.D * (unsigned)g.tiles; }

#ifndef AEFFT_HOSTCHECK
template <int R, bool SF32, bool DF32, bool WORDS>
__global__ __launch_bounds__(256) void degrade_kernel(const DgArgs a)
{
    if constexpr (R == 0) degrade_flat_body<SF32, DF32, WORDS>(a);
    else {
        __shared__ __attribute__((aligned(16))) unsigned dg_lds[dg_lds_words(R)];
        degrade_tile_body<R, SF32, DF32, WORDS>(a, dg_lds);
    }
}

hipError_t launch_degrade(const void* src, bool src_f32, void* dst, bool dst_f32, int B, int D, int Nx, int Ny, int blur, float sigma, float impulse,
                          unsigned long long seed, unsigned long long first_frame, hipStream_t st)
{
    if (!src || !dst || B < 1 || D < 1 || D > 4 || Nx < 1 || Nx > 8192 || Ny < 1 || Ny > 8192 || blur < 0 || blur > 4) return hipErrorInvalidValue;
    if (!(sigma >= 0.f && sigma <= 255.f) || !(impulse >= 0.f && impulse <= 1.f)) return hipErrorInvalidValue;
    if (dst == src && (blur != 0 || src_f32 != dst_f32)) return hipErrorInvalidValue;
    const DgArgs g = dg_geometry(src, dst, B, D, Nx, Ny, sigma, impulse, seed, first_frame);
    const unsigned by = (unsigned)B < 65535u ? (unsigned)B : 65535u;             // frame b = z grid.y + y (workgroups beyond B return at once)
    const dim3 gr(dg_grid_x(blur, g), by, ((unsigned)B + by - 1) / by), bl(256);
    const bool words = (Ny & 3) == 0;
#define DG_CASE(RR, SS, DD, WW) case ((RR) * 8 + (SS) * 4 + (DD) * 2 + (WW)): degrade_kernel<RR, SS != 0, DD != 0, WW != 0><<<gr, bl, 0, st>>>(g); break;
#define DG_CASES(RR) DG_CASE(RR, 0, 0, 0) DG_CASE(RR, 0, 0, 1) DG_CASE(RR, 0, 1, 0) DG_CASE(RR, 0, 1, 1) DG_CASE(RR, 1, 0, 0) DG_CASE(RR, 1, 0, 1) DG_CASE(RR, 1, 1, 0) DG_CASE(RR, 1, 1, 1)
    switch (blur * 8 + (src_f32 ? 4 : 0) + (dst_f32 ? 2 : 0) + (words ? 1 : 0)) {
        DG_CASES(0) DG_CASES(1) DG_CASES(2) DG_CASES(3) DG_CASES(4)
        default: return hipErrorInvalidValue;
    }
#undef DG_CASES
#undef DG_CASE
    return hipGetLastError();
}
#endif

}  // namespace aefft
