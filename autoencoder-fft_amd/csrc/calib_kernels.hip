// Calibration of a per-cell baseline from maps of nominal footage, and the per-image peak (aefft_map_stats_update / _merge / _finish, aefft_map_peak,
// gfx950; include/aefft.h has the definition, DESIGN.md section 29 the route and the measurement).  n = Mx My cells, cell p = I My + J.
// The state is caller-owned, planar, and all-zero bytes when empty:
//   [0, 8n) double S1[n] | [8n, 16n) double S2[n] | [16n, 32n) float hi[4][n] | [32n, 48n) float lo[4][n] | [48n, 52n) int c[n]
// hi[0] >= hi[1] >= ... are the largest values seen, lo[0] <= lo[1] <= ... the smallest; only the first min(c, 4) slots are live, the others hold
// +0.0f.  In registers a dead slot is -inf (hi) or +inf (lo), so that one insertion rule serves every fill level; no counted value is infinite.
//   calib_update_kernel   a lane owns a cell and walks b = 0 .. B-1 in ascending order (the order of the sums is the definition: nothing reduces over
//                         b in parallel); the loads of CB_AHEAD images are issued before their adds, because the loop is latency-bound.  Read-modify-
//                         write of the lane's own 52 bytes: no atomics, no LDS.
//   calib_merge_kernel    a lane owns a cell: one addition for S1, S2 and c, src's live extremes inserted into dst's.
//   calib_finish_kernel   a lane owns a cell: hi[r-1] / lo[r-1] (RANK), or mean + k sd in double, each operation rounded once (SIGMA).
//   calib_peak_kernel     a workgroup of 1024 lanes owns an image: every lane keeps the largest 64-bit key {order-preserving image of v (complemented
//                         for BELOW) : ~p} of its cells, eight loads ahead of their compares, and the keys meet in LDS by a tree of integer max.  The
//                         winner is the peak at the smallest index.
// Exactness.  (double)x * (double)x is exact (48 bits), so S2's bits do not depend on whether the back end fuses the product into the addition
// (-ffp-contract=fast does).  The two products of finish that feed an addition or subtraction ARE rounded by the definition: cb_own makes each a value
// of its own, which the back end cannot contract (score_device.h's score_px does the same for floats).  The square root is the back end's, finished
// by cb_sqrt_fix: the candidate or one of its neighbours, chosen by the exact residual fma(-s, s, x), so the result is the correctly rounded root
// whenever the candidate is within one ulp.  No atomics anywhere; the result of every call is a function of its inputs alone.
// tools/calib_hostcheck.cpp compiles this file for the host (AEFFT_HOSTCHECK: tools/hostlanes.h supplies the launch variables and the barrier).
#ifndef AEFFT_HOSTCHECK
#include "internal.h"
#define CB_HD __device__ __forceinline__
#else
#define CB_HD static inline
#endif

namespace aefft {

constexpr int CB_SIGMA = 0, CB_RANK = 1;                                         // AEFFT_CALIB_SIGMA, AEFFT_CALIB_RANK
constexpr int CB_ABOVE = 0, CB_BELOW = 1;                                        // AEFFT_REGIONS_ABOVE, AEFFT_REGIONS_BELOW
constexpr int CB_LANES = 256;
constexpr int CB_SLOTS = 4;                                                      // the extremes kept on each side
constexpr int CB_AHEAD = 4;                                                      // images whose loads the update issues ahead of their adds
constexpr int CB_PEAK_AHEAD = 8;                                                 // cells a lane of the peak loads ahead of their compares
constexpr int CB_CELLS = 1024;                                                   // the most cells along an axis
constexpr int CB_CELL_BYTES = 52;                                                // 8 + 8 + 16 + 16 + 4
constexpr int CB_PEAK_LANES = 1024;                                              // the peak's workgroup: an image's cells meet in one, so it is the largest
constexpr int CB_PEAK_KEY_WORDS = 2;                                             // LDS of the peak kernel, in words a lane: its key

typedef unsigned long long cb_u64;

struct CbArgs {
    const float *map, *ref_in;                                                   // [B][Mx][My]; the peak's baseline [Mx][My] or null
    void* state;                                                                 // update, finish: the state; merge: dst
    const void* src;                                                             // merge: the state that is only read
    float* ref_out;                                                              // finish: [Mx][My]
    float* peak;                                                                 // [B]
    int* cell;                                                                   // [B]
    int n, B;                                                                    // n = Mx My
    int mode, sense, rank;
    float k, empty;
};

CB_HD float cb_float(unsigned u) { float v; __builtin_memcpy(&v, &u, 4); return v; }
CB_HD unsigned cb_bits(float v) { unsigned u; __builtin_memcpy(&u, &v, 4); return u; }
CB_HD double cb_double(cb_u64 u) { double v; __builtin_memcpy(&v, &u, 8); return v; }
CB_HD cb_u64 cb_bits64(double v) { cb_u64 u; __builtin_memcpy(&u, &v, 8); return u; }
// the order-preserving image of a float's bits among unsigned ints, and back (regions_kernels.hip's rg_ord, restated)
CB_HD unsigned cb_ord(unsigned u) { return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
CB_HD unsigned cb_unord(unsigned o) { return o ^ ((o >> 31) ? 0x80000000u : 0xFFFFFFFFu); }

// a rounded intermediate as a value of its own: what consumes it cannot be contracted with what produced it
#ifndef AEFFT_HOSTCHECK
CB_HD double cb_own(double v) { asm("" : "+v"(v)); return v; }
#else
CB_HD double cb_own(double v) { volatile double t = v; return t; }
#endif

// the planes of a state of n cells
struct CbPlanes { double *S1, *S2; float *hi, *lo; int* c; };
CB_HD CbPlanes cb_planes(void* state, int n)
{
    unsigned char* b = static_cast<unsigned char*>(state);
    CbPlanes s;
    s.S1 = reinterpret_cast<double*>(b); s.S2 = reinterpret_cast<double*>(b + (size_t)8 * n);
    s.hi = reinterpret_cast<float*>(b + (size_t)16 * n); s.lo = reinterpret_cast<float*>(b + (size_t)32 * n);
    s.c = reinterpret_cast<int*>(b + (size_t)48 * n);
    return s;
}

// a cell's state in registers
struct CbCell { double s1, s2; float h[CB_SLOTS], l[CB_SLOTS]; int c; };

CB_HD CbCell cb_load(const CbPlanes& s, int n, int p)
{
    CbCell x;
    x.s1 = s.S1[p]; x.s2 = s.S2[p]; x.c = s.c[p];
#pragma unroll
    for (int k = 0; k < CB_SLOTS; ++k) {
        const float h = s.hi[(size_t)k * n + p], l = s.lo[(size_t)k * n + p];
        x.h[k] = k < x.c ? h : cb_float(0xFF800000u);                            // dead: -inf
        x.l[k] = k < x.c ? l : cb_float(0x7F800000u);                            // dead: +inf
    }
    return x;
}

CB_HD void cb_store(const CbPlanes& s, int n, int p, const CbCell& x)
{
    s.S1[p] = x.s1; s.S2[p] = x.s2; s.c[p] = x.c;
#pragma unroll
    for (int k = 0; k < CB_SLOTS; ++k) {
        s.hi[(size_t)k * n + p] = k < x.c ? x.h[k] : 0.0f;
        s.lo[(size_t)k * n + p] = k < x.c ? x.l[k] : 0.0f;
    }
}

// v (finite, or a dead slot's infinity) enters the sorted slots where it belongs; what falls off the end is dropped.  Equal values keep their
// multiplicity, and with -0 counted as +0 equal values have equal bits: the slots are a function of the multiset
CB_HD void cb_insert(CbCell& x, float vh, float vl)
{
#pragma unroll
    for (int k = 0; k < CB_SLOTS; ++k) {
        const float a = x.h[k], b = x.l[k];
        const bool keep_h = a >= vh, keep_l = b <= vl;
        x.h[k] = keep_h ? a : vh; vh = keep_h ? vh : a;
        x.l[k] = keep_l ? b : vl; vl = keep_l ? vl : b;
    }
}

// one value of the footage
CB_HD void cb_count(CbCell& x, float v)
{
    unsigned u = cb_bits(v);
    if ((u & 0x7F800000u) == 0x7F800000u) return;                                // NaN, +-inf: skipped, not counted
    if (u == 0x80000000u) u = 0;                                                 // -0 counts as +0
    v = cb_float(u);
    const double d = (double)v;
    x.s1 = x.s1 + d;
    x.s2 = x.s2 + d * d;                                                         // (the product is exact: fused or not, the same bits)
    x.c = x.c + 1;
    cb_insert(x, v, v);
}

CB_HD void calib_update_body(const CbArgs& g, unsigned id)
{
    if (id >= (unsigned)g.n) return;
    const int n = g.n, p = (int)id;
    const CbPlanes s = cb_planes(g.state, n);
    CbCell x = cb_load(s, n, p);
    for (int b0 = 0; b0 < g.B; b0 += CB_AHEAD) {
        float v[CB_AHEAD];
#pragma unroll
        for (int k = 0; k < CB_AHEAD; ++k) v[k] = b0 + k < g.B ? g.map[(size_t)(b0 + k) * n + p] : cb_float(0x7FC00000u);    // (past the batch: skipped as NaN)
#pragma unroll
        for (int k = 0; k < CB_AHEAD; ++k) cb_count(x, v[k]);
    }
    cb_store(s, n, p, x);
}

CB_HD void calib_merge_body(const CbArgs& g, unsigned id)
{
    if (id >= (unsigned)g.n) return;
    const int n = g.n, p = (int)id;
    const CbPlanes d = cb_planes(g.state, n), s = cb_planes(const_cast<void*>(g.src), n);      // (src is only read)
    CbCell x = cb_load(d, n, p);
    const CbCell y = cb_load(s, n, p);
    x.s1 = x.s1 + y.s1;
    x.s2 = x.s2 + y.s2;
    x.c = x.c + y.c;
#pragma unroll
    for (int k = 0; k < CB_SLOTS; ++k) cb_insert(x, y.h[k], y.l[k]);              // (a dead slot's infinity falls off the end or lands in a dead slot)
    cb_store(d, n, p, x);
}

// the correctly rounded root of x out of a candidate s within one ulp of it: r = x - s^2 is exact in fma; s is right exactly when the root lies
// between the midpoints to its neighbours, (s - u'/2)^2 < x < (s + u/2)^2 with u = up - s, u' = s - dn, that is -s u' + u'^2/4 < r < s u + u^2/4.
// r, s u and s u' are whole multiples of u'^2 (s = k u, x a double near k^2 u^2), so the quarter terms decide nothing but the ties:
// r > s u moves up, r <= -s u' moves down.  s u and s u' are exact (a power of two times s).  x <= 0, a NaN or an infinity pass through, and so
// does x < 2^-600, where the products would leave the normal range (a variance of counted floats cannot get there: the square of the smallest
// float is 2^-298, the difference of two sums of such a whole multiple of 2^-351, and c - 1 < 2^31).
CB_HD double cb_sqrt_fix(double x, double s)
{
    if (!(x >= 0x1p-600) || !(s > 0.0) || cb_bits64(s) >= 0x7FF0000000000000ull) return s;
    const double r = __builtin_fma(-s, s, x);
    const double up = cb_double(cb_bits64(s) + 1), dn = cb_double(cb_bits64(s) - 1);
    const double su = cb_own(s * (up - s)), sd = cb_own(s * (s - dn));
    if (r > su) return up;
    if (r <= -sd) return dn;
    return s;
}
CB_HD double cb_sqrt(double x) { return cb_sqrt_fix(x, __builtin_sqrt(x)); }

CB_HD void calib_finish_body(const CbArgs& g, unsigned id)
{
    if (id >= (unsigned)g.n) return;
    const int n = g.n, p = (int)id;
    const CbPlanes s = cb_planes(g.state, n);
    const int c = s.c[p];
    float ref = g.empty;
    if (c > 0 && g.mode == CB_RANK) {
        const int r = (g.rank < c ? g.rank : c) - 1;                              // (rank in 1..4: r in 0..3)
        ref = (g.sense == CB_BELOW ? s.lo : s.hi)[(size_t)r * n + p];
    } else if (c > 0) {
        const double s1 = s.S1[p], s2 = s.S2[p];
        const double mean = s1 / (double)c;
        double sd = 0.0;
        if (c > 1) {
            const double pr = cb_own(s1 * mean);
            double d = s2 - pr;
            d = d < 0.0 ? 0.0 : d;
            const double var = d / (double)(c - 1);
            sd = cb_sqrt(var);
        }
        const double t = cb_own((double)g.k * sd);
        ref = (float)(mean + t);
    }
    g.ref_out[p] = ref;
}

// LANES: the lanes of the workgroup (CB_PEAK_LANES on the device; the host check runs the same body with the 256 its harness has)
template <int LANES> CB_HD void calib_peak_body(const CbArgs& g, unsigned b, unsigned* lds)
{
    cb_u64* key = reinterpret_cast<cb_u64*>(lds);
    const int t = (int)threadIdx.x, n = g.n;
    const float* m = g.map + (size_t)b * n;
    const bool below = g.sense == CB_BELOW;
    cb_u64 best = 0;                                                              // (no cell's key is 0: the image of -inf is 0x007FFFFF)
    for (int p0 = t; p0 < n; p0 += LANES * CB_PEAK_AHEAD) {
        float v[CB_PEAK_AHEAD], r[CB_PEAK_AHEAD];
#pragma unroll
        for (int k = 0; k < CB_PEAK_AHEAD; ++k) {
            const int p = p0 + k * LANES;
            v[k] = p < n ? m[p] : cb_float(0x7FC00000u);                          // (past the image: skipped as NaN)
            r[k] = g.ref_in && p < n ? g.ref_in[p] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < CB_PEAK_AHEAD; ++k) {
            const int p = p0 + k * LANES;
            unsigned u = cb_bits(g.ref_in ? v[k] - r[k] : v[k]);                  // one rounding
            if (u == 0x80000000u) u = 0;                                          // -0 counts as +0
            if ((u & 0x7FFFFFFFu) > 0x7F800000u) continue;                        // NaN
            const unsigned o = cb_ord(u);
            const cb_u64 mine = ((cb_u64)(below ? ~o : o) << 32) | (unsigned)~p;
            best = mine > best ? mine : best;
        }
    }
    key[t] = best;
    __syncthreads();
    for (int d = LANES / 2; d >= 1; d >>= 1) {
        if (t < d) { const cb_u64 a = key[t], c = key[t + d]; key[t] = a > c ? a : c; }
        __syncthreads();
    }
    if (t == 0) {
        const cb_u64 win = key[0];
        const unsigned o = (unsigned)(win >> 32);
        g.peak[b] = cb_float(win ? cb_unord(below ? ~o : o) : 0x7FC00000u);        // an image of NaN only: the quiet NaN
        g.cell[b] = win ? (int)~(unsigned)win : -1;
    }
}

// the state in bytes; 0 for sizes the calls do not take
static inline size_t calib_state_bytes(int Mx, int My)
{
    if (Mx < 1 || Mx > CB_CELLS || My < 1 || My > CB_CELLS) return 0;
    return ((size_t)CB_CELL_BYTES * Mx * My + 15) & ~(size_t)15;
}

// the sizes every launcher takes; false for what the kernels do not serve
static inline bool cb_geometry(int Mx, int My, int B, CbArgs* g)
{
    if (!calib_state_bytes(Mx, My) || B < 1 || (long long)B * Mx * My > 0x7fffffffLL) return false;
    *g = CbArgs();
    g->n = Mx * My; g->B = B;
    return true;
}
static inline unsigned cb_grid(const CbArgs& g) { return (unsigned)((g.n + CB_LANES - 1) / CB_LANES); }

#ifndef AEFFT_HOSTCHECK
__global__ __launch_bounds__(CB_LANES) void calib_update_kernel(const CbArgs g) { calib_update_body(g, blockIdx.x * CB_LANES + threadIdx.x); }
__global__ __launch_bounds__(CB_LANES) void calib_merge_kernel(const CbArgs g) { calib_merge_body(g, blockIdx.x * CB_LANES + threadIdx.x); }
__global__ __launch_bounds__(CB_LANES) void calib_finish_kernel(const CbArgs g) { calib_finish_body(g, blockIdx.x * CB_LANES + threadIdx.x); }
__global__ __launch_bounds__(CB_PEAK_LANES) void calib_peak_kernel(const CbArgs g)
{
    __shared__ __attribute__((aligned(16))) unsigned lds[CB_PEAK_KEY_WORDS * CB_PEAK_LANES];
    calib_peak_body<CB_PEAK_LANES>(g, blockIdx.x, lds);
}

size_t map_stats_bytes(int Mx, int My) { return calib_state_bytes(Mx, My); }

hipError_t launch_map_stats_update(const float* map, int Mx, int My, int B, void* stats, hipStream_t st)
{
    CbArgs g;
    if (!map || !stats || !cb_geometry(Mx, My, B, &g)) return hipErrorInvalidValue;
    g.map = map; g.state = stats;
    calib_update_kernel<<<dim3(cb_grid(g)), dim3(CB_LANES), 0, st>>>(g);
    return hipGetLastError();
}

hipError_t launch_map_stats_merge(void* dst, const void* src, int Mx, int My, hipStream_t st)
{
    CbArgs g;
    if (!dst || !src || !cb_geometry(Mx, My, 1, &g)) return hipErrorInvalidValue;
    g.state = dst; g.src = src;
    calib_merge_kernel<<<dim3(cb_grid(g)), dim3(CB_LANES), 0, st>>>(g);
    return hipGetLastError();
}

hipError_t launch_map_stats_finish(const void* stats, int Mx, int My, int mode, int sense, float k, int rank, float empty, float* ref, hipStream_t st)
{
    CbArgs g;
    if (!stats || !ref || !cb_geometry(Mx, My, 1, &g) || (mode != CB_SIGMA && mode != CB_RANK) || (sense != CB_ABOVE && sense != CB_BELOW) || rank < 1 ||
        rank > CB_SLOTS)
        return hipErrorInvalidValue;
    g.state = const_cast<void*>(stats); g.ref_out = ref;                          // (the finish only reads the state)
    g.mode = mode; g.sense = sense; g.rank = rank; g.k = k; g.empty = empty;
    calib_finish_kernel<<<dim3(cb_grid(g)), dim3(CB_LANES), 0, st>>>(g);
    return hipGetLastError();
}

hipError_t launch_map_peak(const float* map, const float* ref, int Mx, int My, int B, int sense, float* peak, int* cell, hipStream_t st)
{
    CbArgs g;
    if (!map || !peak || !cell || !cb_geometry(Mx, My, B, &g) || (sense != CB_ABOVE && sense != CB_BELOW)) return hipErrorInvalidValue;
    g.map = map; g.ref_in = ref; g.peak = peak; g.cell = cell; g.sense = sense;
    calib_peak_kernel<<<dim3((unsigned)B), dim3(CB_PEAK_LANES), 0, st>>>(g);
    return hipGetLastError();
}
#endif

}  // namespace aefft
