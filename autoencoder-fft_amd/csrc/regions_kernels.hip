// Anomaly regions from a score map (aefft_map_regions, gfx950; include/aefft.h has the definition, DESIGN.md section 27 the route and the measurement):
// hysteresis threshold, connected components under 4- or 8-connectivity, a label map, per-region boxes with area and peak, a per-image count.  A tiled
// union-find in six launches on one stream; a cell is (I, J) of image b, its index p = I My + J inside the image, g = b Mx My + p in the batch.
//   regions_tile_kernel     a workgroup owns a tile of 16 x 16 cells: value and foreground of each cell, the rows' foreground masks in LDS, every cell
//                           starts at the first cell of its run along J, the runs of neighbouring rows unite in LDS (one union a pair of touching runs),
//                           and the area and the peak key of every tile component meet at its root in LDS.  labels[g] = the tile root's g (-1:
//                           background); slot[g] = {key, area} at a tile root, zeros elsewhere.
//   regions_border_kernel   the cells on a tile's edge unite with their foreground neighbours of the tile before (up, left and, under 8-connectivity,
//                           the two upper diagonals: every pair of neighbours once), an atomicMin union on labels.  Only roots are ever relinked.
//   regions_flatten_kernel  every tile root finds its component's root, points at it and adds its area and its key to the root's slot.  The other cells
//                           keep pointing at their tile root: two hops from any cell to its root.
//   regions_count_kernel    a workgroup owns 1024 consecutive cells of one image and counts its kept roots (a root: labels[g] == g; kept: a strong
//                           peak and area >= min_area) into the aux word of slot[b Mx My + block].
//   regions_rank_kernel     the same blocks: a kept root's number is 1 + the kept roots before it -- the counts of the blocks before, a scan over the
//                           lanes, the lane's own four cells in order.  The root's slot receives the number (0: dropped), regions[number - 1] the root's
//                           cell as bounds, the area and the peak; count[b] the image's total.
//   regions_final_kernel    tiles again: a tile root reads its root's number, the cells of a tile component meet their bounds at the tile root in LDS,
//                           the tile root carries them to the region by integer min / max, every cell stores its number.
// Determinism: every union links the LARGER root under the SMALLER, so the root of a component is its smallest index whatever the interleaving; the sums
// are integer add, min and max and ONE 64-bit max on the key {order-preserving image of v (complemented for BELOW) : ~p}, whose winner is the peak at the
// smallest index; there is no float atomic and no result depends on an arrival order.
// Termination: (find) a cell's parent is never above the cell -- lab[x] <= x holds at every moment, also for a stale read --, so a find loop follows
// strictly decreasing indices and ends after at most x steps; (union) an iteration ends the union unless its atomicMin LOST, that is returned a
// parent old < a that somebody else had stored, and then it goes on with old in place of a: the pair (a, b) decreases strictly, at most a + b
// iterations; (scan) 8 doubling steps; (offsets) at most 1024 block counts an image, four a lane.  No workgroup waits for another one: there is no
// flag, no spinning and no cooperative launch; a launch boundary is the only ordering between workgroups, and within a launch every access that can
// race is an atomic whose operation commutes, or a read of a word whose every possible value is right (a parent link, a bound that only grows).
// The atomics are plain HIP atomics on LDS and global memory (vector instructions).  tools/regions_hostcheck.cpp compiles this file for the host,
// threads as lanes and the workgroups one after another (legal because none waits), under the sanitizers (AEFFT_HOSTCHECK: tools/hostlanes.h supplies
// the launch variables and the barrier; the atomics have their host forms below).
#ifndef AEFFT_HOSTCHECK
#include "internal.h"
#define RG_HD __device__ __forceinline__
#else
#define RG_HD static inline
#endif

namespace aefft {

constexpr int RG_ABOVE = 0, RG_BELOW = 1;                                        // AEFFT_REGIONS_ABOVE, AEFFT_REGIONS_BELOW
constexpr int RG_T = 16;                                                         // the side of a tile
constexpr int RG_LANES = 256;                                                    // = RG_T RG_T: a lane a cell
constexpr int RG_PER = 4, RG_CHUNK = RG_LANES * RG_PER;                          // consecutive cells of a lane, and of a workgroup, when ranking
constexpr int RG_CELLS = 1024;                                                   // the most cells along an axis
constexpr int RG_MAX_REGIONS = 65536;
constexpr int RG_WORDS = 8;                                                      // the ints of an aefft_region: i0, j0, i1, j1, area, peak_i, peak_j, peak

struct RgSlot { unsigned long long key; int area, aux; };                        // the 16 workspace bytes of a cell

typedef unsigned long long rg_u64;

#ifndef AEFFT_HOSTCHECK
RG_HD int rg_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
RG_HD int rg_min(int* p, int v) { return atomicMin(p, v); }                     // (all return-less but this one: a union needs what it displaced)
RG_HD void rg_max(int* p, int v) { atomicMax(p, v); }
RG_HD void rg_add(int* p, int v) { atomicAdd(p, v); }
RG_HD void rg_or(unsigned* p, unsigned v) { atomicOr(p, v); }
RG_HD void rg_max64(rg_u64* p, rg_u64 v) { atomicMax(p, v); }
RG_HD int rg_clz(unsigned v) { return __clz((int)v); }
#else
RG_HD int rg_ld(const int* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
RG_HD int rg_min(int* p, int v)
{
    int o = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (o > v && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return o;
}
RG_HD void rg_max(int* p, int v)
{
    int o = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (o < v && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
}
RG_HD void rg_add(int* p, int v) { __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
RG_HD void rg_or(unsigned* p, unsigned v) { __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
RG_HD void rg_max64(rg_u64* p, rg_u64 v)
{
    rg_u64 o = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (o < v && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
}
RG_HD int rg_clz(unsigned v) { return __builtin_clz(v); }
#endif

struct RgArgs {
    const float *map, *ref;                                                      // [B][Mx][My]; [Mx][My] or null
    int* labels;                                                                 // [B][Mx][My]
    RgSlot* slot;                                                                // [B][Mx][My]: the workspace
    int* regions;                                                                // [B][max_regions][RG_WORDS] or null
    int* count;                                                                  // [B]
    int Mx, My, B, cells;                                                        // cells = Mx My
    int tx, ty;                                                                  // tiles along I and J
    int nblk;                                                                    // ranking blocks of an image
    unsigned tiles, flat, blocks;                                                // the three grids: B tx ty, ceil(B cells / 256), B nblk
    int sense, conn8, min_area, max_regions;
    float lo, hi;
};

// the order-preserving image of a float's bits among unsigned ints, and back
RG_HD unsigned rg_ord(unsigned u) { return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
RG_HD unsigned rg_unord(unsigned o) { return o ^ ((o >> 31) ? 0x80000000u : 0xFFFFFFFFu); }
RG_HD float rg_float(unsigned u) { float v; __builtin_memcpy(&v, &u, 4); return v; }
RG_HD unsigned rg_bits(float v) { unsigned u; __builtin_memcpy(&u, &v, 4); return u; }

// the peak's value bits of a key, and is that peak strong?
RG_HD unsigned rg_peak_bits(rg_u64 key, int sense) { const unsigned o = (unsigned)(key >> 32); return rg_unord(sense == RG_BELOW ? ~o : o); }
RG_HD bool rg_strong(rg_u64 key, int sense, float hi) { const float v = rg_float(rg_peak_bits(key, sense)); return sense == RG_BELOW ? v <= hi : v >= hi; }

// the root of x: parents never lie above their children, so the indices fall strictly
RG_HD int rg_find(const int* lab, int x)
{
    for (;;) {
        const int p = rg_ld(lab + x);
        if (p == x) return x;
        x = p;
    }
}

// one component out of a's and b's: the larger root goes under the smaller.  Another round only when the atomicMin lost to a smaller parent, which it
// then unites with b
RG_HD void rg_union(int* lab, int a, int b)
{
    for (;;) {
        a = rg_find(lab, a);
        b = rg_find(lab, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = rg_min(lab + a, b);
        if (old == a) return;
        a = old;
    }
}

// LDS of the tile kernel, in words: the keys [256] (two words each), the parents [256], the areas [256], the rows' masks [16]
constexpr int RG_TILE_WORDS = 4 * RG_LANES + RG_T;
// ... of the final kernel: the numbers [256], the largest I, the smallest J and the largest J [256 each]
constexpr int RG_FINAL_WORDS = 4 * RG_LANES;
// ... of the rank kernel: the scan [256], the counts before and in all [2]
constexpr int RG_RANK_WORDS = RG_LANES + 2;

struct RgCell { int b, tI, tJ, I, J, g; bool in; };
// lane t of tile `tile`
RG_HD RgCell rg_cell(const RgArgs& g, unsigned tile, int t)
{
    RgCell c;
    const unsigned per = (unsigned)(g.tx * g.ty), rem = tile % per;
    c.b = (int)(tile / per); c.tI = (int)(rem / (unsigned)g.ty); c.tJ = (int)(rem % (unsigned)g.ty);
    c.I = c.tI * RG_T + (t >> 4); c.J = c.tJ * RG_T + (t & 15);
    c.in = c.I < g.Mx && c.J < g.My;
    c.g = c.in ? c.b * g.cells + c.I * g.My + c.J : 0;
    return c;
}

RG_HD void regions_tile_body(const RgArgs& g, unsigned tile, unsigned* lds)
{
    rg_u64* key = reinterpret_cast<rg_u64*>(lds);
    int* lab = reinterpret_cast<int*>(lds + 2 * RG_LANES);
    int* area = lab + RG_LANES;
    unsigned* rows = lds + 4 * RG_LANES;
    const int t = (int)threadIdx.x, ti = t >> 4, tj = t & 15;
    const RgCell c = rg_cell(g, tile, t);
    bool fg = false;
    rg_u64 mine = 0;
    if (c.in) {
        const int p = c.I * g.My + c.J;
        float v = g.map[c.g];
        if (g.ref) v = v - g.ref[p];                                              // one rounding
        unsigned u = rg_bits(v);
        if (u == 0x80000000u) u = 0;                                              // -0 counts as +0
        v = rg_float(u);
        fg = g.sense == RG_BELOW ? v <= g.lo : v >= g.lo;                         // (NaN: false)
        const unsigned o = rg_ord(u);
        mine = ((rg_u64)(g.sense == RG_BELOW ? ~o : o) << 32) | (unsigned)~p;
    }
    key[t] = 0; area[t] = 0;
    if (t < RG_T) rows[t] = 0;
    __syncthreads();
    if (fg) rg_or(rows + ti, 1u << tj);
    __syncthreads();
    const unsigned m = rows[ti], up = ti ? rows[ti - 1] : 0u;
    const unsigned below = (1u << tj) - 1u, gap = ~m & below;                     // the background cells of the row before this one
    lab[t] = fg ? ti * RG_T + (gap ? 32 - rg_clz(gap) : 0) : -1;                  // the first cell of the run
    __syncthreads();
    if (fg && ti) {
        // a pair of touching runs unites once: a neighbour above is skipped where the cell before (behind) unites the same two runs
        const bool upfg = (up >> tj) & 1u, leftfg = tj > 0 && ((m >> (tj - 1)) & 1u), rightfg = tj < 15 && ((m >> (tj + 1)) & 1u);
        const bool ulfg = tj > 0 && ((up >> (tj - 1)) & 1u), urfg = tj < 15 && ((up >> (tj + 1)) & 1u);
        if (upfg && !(leftfg && ulfg)) rg_union(lab, t, t - RG_T);
        if (g.conn8) {
            if (ulfg && !upfg && !leftfg) rg_union(lab, t, t - RG_T - 1);
            if (urfg && !upfg && !rightfg) rg_union(lab, t, t - RG_T + 1);
        }
    }
    __syncthreads();
    const int lr = fg ? rg_find(lab, t) : -1;
    if (fg) {
        rg_add(area + lr, 1);
        rg_max64(key + lr, mine);
    }
    __syncthreads();
    if (c.in) {
        g.labels[c.g] = fg ? c.b * g.cells + (c.tI * RG_T + (lr >> 4)) * g.My + c.tJ * RG_T + (lr & 15) : -1;
        RgSlot s;
        s.key = fg && lr == t ? key[t] : 0; s.area = fg && lr == t ? area[t] : 0; s.aux = 0;
        g.slot[c.g] = s;
    }
}

// a cell on a tile's edge and its foreground neighbours in the tiles before it
RG_HD void regions_border_body(const RgArgs& g, unsigned id)
{
    const unsigned total = (unsigned)g.B * (unsigned)g.cells;
    if (id >= total) return;
    const int x = (int)id, p = (int)(id % (unsigned)g.cells), I = p / g.My, J = p - I * g.My, My = g.My;
    const bool ti0 = (I & 15) == 0 && I > 0, tj0 = (J & 15) == 0 && J > 0, tj15 = (J & 15) == 15 && J < My - 1 && I > 0;
    if (!(ti0 || tj0 || tj15)) return;
    int* L = g.labels;
    if (L[x] < 0) return;
    const bool upfg = I > 0 && L[x - My] >= 0, leftfg = J > 0 && L[x - 1] >= 0, rightfg = J < My - 1 && L[x + 1] >= 0;
    const bool ulfg = I > 0 && J > 0 && L[x - My - 1] >= 0, urfg = I > 0 && J < My - 1 && L[x - My + 1] >= 0;
    // (skipped where a neighbour's pair, inside a tile or on this list, unites the same two components)
    if (ti0 && upfg && !(leftfg && ulfg && (J & 15) != 0)) rg_union(L, x, x - My);
    if (tj0 && leftfg && !(upfg && ulfg && (I & 15) != 0)) rg_union(L, x, x - 1);
    if (g.conn8) {
        if ((ti0 || tj0) && ulfg && !upfg && !leftfg) rg_union(L, x, x - My - 1);
        if ((ti0 || tj15) && urfg && !upfg && !rightfg) rg_union(L, x, x - My + 1);
    }
}

// a tile root joins its component's root
RG_HD void regions_flatten_body(const RgArgs& g, unsigned id)
{
    if (id >= (unsigned)g.B * (unsigned)g.cells) return;
    const int x = (int)id;
    if (g.labels[x] < 0) return;
    const int part = g.slot[x].area;
    if (part <= 0) return;                                                        // not a tile root
    const int r = rg_find(g.labels, x);
    if (r == x) return;
    const rg_u64 k = g.slot[x].key;                                               // (this slot is no root's: nobody adds to it)
    g.labels[x] = r;
    rg_add(&g.slot[r].area, part);
    rg_max64(&g.slot[r].key, k);
}

// is cell x a kept root?  (its slot then holds the component's area and key)
RG_HD bool rg_kept(const RgArgs& g, int x, RgSlot* s)
{
    if (g.labels[x] != x) return false;
    *s = g.slot[x];
    return s->area >= g.min_area && rg_strong(s->key, g.sense, g.hi);
}

RG_HD void regions_count_body(const RgArgs& g, unsigned block, unsigned* lds)
{
    const int t = (int)threadIdx.x, b = (int)(block / (unsigned)g.nblk), blk = (int)(block % (unsigned)g.nblk);
    int* sum = reinterpret_cast<int*>(lds);
    if (t == 0) sum[0] = 0;
    __syncthreads();
    int c = 0;
#pragma unroll
    for (int k = 0; k < RG_PER; ++k) {
        const int p = blk * RG_CHUNK + t * RG_PER + k;
        RgSlot s;
        if (p < g.cells && rg_kept(g, b * g.cells + p, &s)) ++c;
    }
    if (c) rg_add(sum, c);
    __syncthreads();
    if (t == 0) g.slot[b * g.cells + blk].aux = sum[0];                           // (blk < nblk <= cells)
}

RG_HD void regions_rank_body(const RgArgs& g, unsigned block, unsigned* lds)
{
    const int t = (int)threadIdx.x, b = (int)(block / (unsigned)g.nblk), blk = (int)(block % (unsigned)g.nblk);
    int* sc = reinterpret_cast<int*>(lds);
    int* sums = sc + RG_LANES;                                                    // the kept roots of the blocks before this one, and of the image
    RgSlot s[RG_PER];
    bool kept[RG_PER];
    int c = 0;
#pragma unroll
    for (int k = 0; k < RG_PER; ++k) {
        const int p = blk * RG_CHUNK + t * RG_PER + k;
        kept[k] = p < g.cells && rg_kept(g, b * g.cells + p, &s[k]);
        c += kept[k];
    }
    sc[t] = c;
    if (t < 2) sums[t] = 0;
    __syncthreads();
    for (int d = 1; d < RG_LANES; d <<= 1) {
        const int v = t >= d ? sc[t - d] : 0;
        __syncthreads();
        sc[t] += v;
        __syncthreads();
    }
    int before = 0, all = 0;
    for (int j = t; j < g.nblk; j += RG_LANES) {
        const int a = g.slot[b * g.cells + j].aux;
        all += a;
        if (j < blk) before += a;
    }
    if (before) rg_add(sums, before);
    if (all) rg_add(sums + 1, all);
    __syncthreads();
    int rank = sums[0] + sc[t] - c;
#pragma unroll
    for (int k = 0; k < RG_PER; ++k) {
        const int p = blk * RG_CHUNK + t * RG_PER + k;
        if (p >= g.cells) break;
        const int x = b * g.cells + p;
        if (g.labels[x] != x) continue;
        if (!kept[k]) { g.slot[x].area = 0; continue; }
        ++rank;
        g.slot[x].area = rank;                                                    // (the area moves on to the region: from here the word is the number)
        if (rank <= g.max_regions) {
            int* R = g.regions + ((size_t)b * g.max_regions + (rank - 1)) * RG_WORDS;
            const int I = p / g.My, J = p - I * g.My, pp = (int)~(unsigned)s[k].key, pi = pp / g.My;
            R[0] = I; R[1] = J; R[2] = I; R[3] = J; R[4] = s[k].area; R[5] = pi; R[6] = pp - pi * g.My; R[7] = (int)rg_peak_bits(s[k].key, g.sense);
        }
    }
    if (blk == 0 && t == 0) g.count[b] = sums[1];
}

RG_HD void regions_final_body(const RgArgs& g, unsigned tile, unsigned* lds)
{
    int* rk = reinterpret_cast<int*>(lds);
    int *hiI = rk + RG_LANES, *loJ = hiI + RG_LANES, *hiJ = loJ + RG_LANES;
    const int t = (int)threadIdx.x;
    const RgCell c = rg_cell(g, tile, t);
    const int x = c.in ? g.labels[c.g] : -1;                                      // the component's root (a tile root's), the tile root, or -1
    const bool root = x >= 0 && (x == c.g || g.slot[c.g].area > 0);               // a tile root: its slot kept its part, or, a root's, holds the number
    rk[t] = root ? g.slot[x].area : 0;
    hiI[t] = -1; loJ[t] = RG_CELLS; hiJ[t] = -1;
    __syncthreads();
    int at = t;                                                                   // the tile root's lane
    if (x >= 0 && !root) {
        const int xp = x - c.b * g.cells, xI = xp / g.My;
        at = (xI - c.tI * RG_T) * RG_T + (xp - xI * g.My - c.tJ * RG_T);
    }
    const int rank = x >= 0 ? rk[at] : 0;
    const bool boxed = rank >= 1 && rank <= g.max_regions;
    if (boxed) {
        rg_max(hiI + at, c.I);
        rg_min(loJ + at, c.J);
        rg_max(hiJ + at, c.J);
    }
    __syncthreads();
    if (root && boxed) {
        int* R = g.regions + ((size_t)c.b * g.max_regions + (rank - 1)) * RG_WORDS;    // (i0 is the root's I: the smallest index has the smallest I)
        if (rg_ld(R + 2) < hiI[t]) rg_max(R + 2, hiI[t]);                         // (a bound only grows: a stale read costs an atomic, never a result)
        if (rg_ld(R + 1) > loJ[t]) rg_min(R + 1, loJ[t]);
        if (rg_ld(R + 3) < hiJ[t]) rg_max(R + 3, hiJ[t]);
    }
    if (c.in) g.labels[c.g] = rank;
}

// the workspace in bytes; 0 for sizes the call does not take
static inline size_t regions_workspace(int Mx, int My, int B)
{
    if (Mx < 1 || Mx > RG_CELLS || My < 1 || My > RG_CELLS || B < 1 || (long long)B * Mx * My > 0x7fffffffLL) return 0;
    return sizeof(RgSlot) * (size_t)B * Mx * My;
}

// the launch geometry; false for what the kernels do not serve
static inline bool rg_geometry(const float* map, const float* ref, int Mx, int My, int B, int sense, float lo, float hi, int connectivity, int min_area,
                               int* labels, int* regions, int max_regions, int* count, void* work, RgArgs* g)
{
    if (!map || !labels || !count || !work || !regions_workspace(Mx, My, B) || (sense != RG_ABOVE && sense != RG_BELOW) ||
        (connectivity != 4 && connectivity != 8) || min_area < 1 || max_regions < 0 || max_regions > RG_MAX_REGIONS || (regions == nullptr) != (max_regions == 0))
        return false;
    g->map = map; g->ref = ref; g->labels = labels; g->slot = static_cast<RgSlot*>(work); g->regions = regions; g->count = count;
    g->Mx = Mx; g->My = My; g->B = B; g->cells = Mx * My;
    g->tx = (Mx + RG_T - 1) / RG_T; g->ty = (My + RG_T - 1) / RG_T;
    g->nblk = (g->cells + RG_CHUNK - 1) / RG_CHUNK;
    g->tiles = (unsigned)B * (unsigned)(g->tx * g->ty);                          // (each at most B Mx My < 2^31)
    g->flat = (unsigned)(((long long)B * g->cells + RG_LANES - 1) / RG_LANES);
    g->blocks = (unsigned)B * (unsigned)g->nblk;
    g->sense = sense; g->conn8 = connectivity == 8; g->min_area = min_area; g->max_regions = max_regions; g->lo = lo; g->hi = hi;
    return true;
}

#ifndef AEFFT_HOSTCHECK
static_assert(sizeof(aefft_region) == RG_WORDS * sizeof(int) && sizeof(RgSlot) == 16, "the layouts the kernels write");

__global__ __launch_bounds__(RG_LANES) void regions_tile_kernel(const RgArgs g)
{
    __shared__ __attribute__((aligned(16))) unsigned lds[RG_TILE_WORDS];
    regions_tile_body(g, blockIdx.x, lds);
}
__global__ __launch_bounds__(RG_LANES) void regions_border_kernel(const RgArgs g) { regions_border_body(g, blockIdx.x * RG_LANES + threadIdx.x); }
__global__ __launch_bounds__(RG_LANES) void regions_flatten_kernel(const RgArgs g) { regions_flatten_body(g, blockIdx.x * RG_LANES + threadIdx.x); }
__global__ __launch_bounds__(RG_LANES) void regions_count_kernel(const RgArgs g)
{
    __shared__ unsigned lds[1];
    regions_count_body(g, blockIdx.x, lds);
}
__global__ __launch_bounds__(RG_LANES) void regions_rank_kernel(const RgArgs g)
{
    __shared__ unsigned lds[RG_RANK_WORDS];
    regions_rank_body(g, blockIdx.x, lds);
}
__global__ __launch_bounds__(RG_LANES) void regions_final_kernel(const RgArgs g)
{
    __shared__ unsigned lds[RG_FINAL_WORDS];
    regions_final_body(g, blockIdx.x, lds);
}

size_t map_regions_workspace(int Mx, int My, int B) { return regions_workspace(Mx, My, B); }

hipError_t launch_map_regions(const float* map, const float* ref, int Mx, int My, int B, int sense, float lo, float hi, int connectivity, int min_area,
                              int* labels, aefft_region* regions, int max_regions, int* count, void* work, hipStream_t st)
{
    RgArgs g;
    if (!rg_geometry(map, ref, Mx, My, B, sense, lo, hi, connectivity, min_area, labels, reinterpret_cast<int*>(regions), max_regions, count, work, &g))
        return hipErrorInvalidValue;
    const dim3 bl(RG_LANES);
    regions_tile_kernel<<<dim3(g.tiles), bl, 0, st>>>(g);
    regions_border_kernel<<<dim3(g.flat), bl, 0, st>>>(g);
    regions_flatten_kernel<<<dim3(g.flat), bl, 0, st>>>(g);
    regions_count_kernel<<<dim3(g.blocks), bl, 0, st>>>(g);
    regions_rank_kernel<<<dim3(g.blocks), bl, 0, st>>>(g);
    regions_final_kernel<<<dim3(g.tiles), bl, 0, st>>>(g);
    return hipGetLastError();
}
#endif

}  // namespace aefft
