// Tiled inference at the image boundary (aefft_tile_plan_make / aefft_image_tiles_to_frames / aefft_frames_tiles_to_image, gfx950; include/aefft.h has
// the definition, DESIGN.md section 24 the layout).  An image of W x H interleaved pixels is cut into overlapping tiles of the net's frame size
// Nx x Ny (reflected beyond the image's edge) and the tiles are blended back with integer ramp weights that sum to a constant:
//   tile_gather_kernel<D, F32>   image rows -> tile frames [T][D][Nx][Ny] (unsigned char, or float when F32: (float)pixel)
//   tile_blend_kernel<D, F32>    tile frames -> image rows (float frames through px_u8 first)
// Both are LDS-tiled transposing copies in the manner of image_kernels.hip: a block of 64 image columns x 64 image rows, all D
// channels, staged in LDS in IMAGE order; each side moves it with the accesses that are contiguous on that side.
//   gather   a workgroup owns a 64 x 64 block of ONE tile.  Its source rows go through a reflection map (64 entries in LDS, a plain ramp in the
//            interior).  Its source columns are a span of at most 64 columns of the image, in order or -- on the image's left or right edge --
//            folded by the reflection.  Image side: a lane loads one ALIGNED dword of a source row -- the span starts at an arbitrary byte of the
//            row, so the LDS row keeps the row's own dword phase (one dword more than 64 D bytes).  Frame side: as image_unpack -- a lane owns 4
//            columns c = i D + d x 4 rows j and stores 4 pixels along j (one dword / one float4), 16 consecutive lanes on one run of 64 pixels; it
//            takes its 4 x 4 bytes out of two neighbouring LDS dwords per row with a funnel shift and transposes them in registers, or, in a
//            folded block, reads them one by one through the column map.
//   blend    pixel-centric: a workgroup owns 64 image columns x the up to 64 image rows whose PRIMARY tile row is ty and whose row k in that tile
//            lies in one 64-aligned chunk -- so the primary tile's samples of a lane's 4 rows are one aligned dword / float4 of the frame (Ny a
//            multiple of 4).  The primary tile of a coordinate is the last one whose kept area has begun; in its left ramp the previous tile
//            contributes too (single elements: its phase along j is S mod 4).  A lane gathers the one, two or four samples of each of its 16
//            pixels, forms acc = sum wx wy p and floor((2 acc + den) / (2 den)) by a multiply-shift (tl_div: exact for every n < 2^31), and
//            writes the bytes to LDS in image order; the image side stores aligned dwords of the rows.  Every pixel is written once: no atomics,
//            the image is never read.
// Either side falls back ON ITS OWN to single elements when its condition fails (image pointer, pitch or stride not a multiple of 4; Ny not a
// multiple of 4): every accepted argument gives the same bytes.
// LDS: an LDS row is RWP = 16 D + 1 dwords, four rows form a super-row of SR = 4 RWP + 2 = 64 D + 6 dwords.  The frame side's lanes q = 0..15 of a
// run read dword g of rows 4 q + k: banks 6 q + g + const (mod 32), and 6 q runs through all 16 even residues, so the 32 lanes of a ds_read_b32 /
// ds_write_b32 lane group (q = 0..15 x two neighbouring g) are on 32 different banks.  16 SR + 192 map words: 17.2 KiB at D = 4.  No scratch.
// tools/tiles_hostcheck.cpp compiles this file for the host, threads as lanes, under the sanitizers (AEFFT_HOSTCHECK: tools/hostlanes.h supplies the
// launch variables, the barrier, float4 and px_u8).
#ifndef AEFFT_HOSTCHECK
#include "internal.h"
#include "fft_common.h"
#define TL_HD __device__ __forceinline__
#define TL_MHD static __device__ __forceinline__                              // (a member function)
#endif

namespace aefft {

constexpr int TL_TILE = 64;                                                      // image columns and image rows of a block

// one axis of the plan (include/aefft.h): image size W, tile N, rim M, ramp R, step S, n tiles, tile 0 at o0, den = 2 R or 1
struct TlAxis { int W, N, M, R, S, n, o0, den; };
static inline bool tl_axis(int W, int N, int V, int M, TlAxis* a)
{
    if (W < 1 || W > 8192 || N < 2 || N > 2048 || V < 0 || V > N / 2 || M < 0 || M > V / 2) return false;   // (2 V <= N, 2 M <= V without the products)
    a->W = W; a->N = N; a->M = M; a->S = N - V; a->R = V - 2 * M;
    const int num = W - N + 2 * M;
    a->n = num <= 0 ? 1 : (num + a->S - 1) / a->S + 1;
    const int E = (a->n - 1) * a->S + N - 2 * M - W;
    a->o0 = -M - E / 2;
    a->den = a->R > 0 ? 2 * a->R : 1;
    return true;
}
bool tile_plan(const aefft_tile_desc* d, aefft_tile_plan* p)
{
    TlAxis x, y;
    if (!d || !p || !tl_axis(d->W, d->Nx, d->overlap_x, d->rim_x, &x) || !tl_axis(d->H, d->Ny, d->overlap_y, d->rim_y, &y)) return false;
    p->ntx = x.n; p->nty = y.n; p->ox0 = x.o0; p->oy0 = y.o0; p->step_x = x.S; p->step_y = y.S; p->ramp_x = x.R; p->ramp_y = y.R;
    return true;
}

struct TlArgs {
    const unsigned char* image; size_t pitch, stride;                            // B images (the blend writes through them)
    void* frames;                                                                // [T][D][Nx][Ny]
    TlAxis x, y;
    int bx, by;                                                                  // gather: blocks of a tile along i, j; blend: along the image's columns, a tile's rows
    int units;                                                                   // gather: the T tiles; blend: the B nty tile rows (grid.y x grid.z; grid.x = bx by)
    int img_words, frm_words;
    unsigned long long mul; int shift;                                           // blend: floor(n / (2 denx deny)) = (n * mul) >> shift for n < 2^31
};

// floor(n / dv) for n < 2^31 as a multiply-shift: l = ceil(log2 dv), shift = 32 + l, mul = floor(2^shift / dv) + 1 <= 2^33 (round-up method:
// mul dv - 2^shift <= dv <= 2^l); n mul < 2^64
static inline void tl_magic(unsigned dv, unsigned long long* mul, int* shift)
{
    int l = 0;
    while ((1ull << l) < dv) ++l;
    *shift = 32 + l;
    *mul = (1ull << *shift) / dv + 1;
}
TL_HD unsigned tl_div(unsigned n, unsigned long long mul, int shift) { return (unsigned)(((unsigned long long)n * mul) >> shift); }

TL_HD int tl_min(int a, int b) { return a < b ? a : b; }
TL_HD int tl_max(int a, int b) { return a > b ? a : b; }
// reflection without repeating the edge pixel, iterated: defined for any x
TL_HD int tl_reflect(int x, int W)
{
    if (W == 1) return 0;
    const int P = 2 * (W - 1);
    int m = x % P;
    if (m < 0) m += P;
    return m < W ? m : P - m;
}

// the least and the largest value tl_reflect takes on [x, x + n): the triangle wave has its minima 0 at the multiples of P and its maxima W - 1
// half a period further, and is monotone in between -- the image of an interval is an interval of at most n columns
TL_HD void tl_reflect_range(int x, int n, int W, int* lo, int* hi)
{
    *lo = *hi = 0;
    if (W == 1) return;
    const int P = 2 * (W - 1), ra = tl_reflect(x, W), rb = tl_reflect(x + n - 1, W);
    int ma = x % P, mb = (x - (W - 1)) % P;
    if (ma < 0) ma += P;
    if (mb < 0) mb += P;
    *lo = (ma == 0 || ma + n - 1 >= P) ? 0 : tl_min(ra, rb);
    *hi = (mb == 0 || mb + n - 1 >= P) ? W - 1 : tl_max(ra, rb);
}

template <int D> struct TlLds {
    static constexpr int RW = TL_TILE * D / 4;                                   // dwords of 64 pixels
    static constexpr int RWP = RW + 1;                                           // dwords of an LDS row: the source row's dword phase costs one more
    static constexpr int SR = 4 * RWP + 2;                                       // dwords of a super-row (four rows + the pad)
    static constexpr int WORDS = TL_TILE / 4 * SR;
    static constexpr int TOTAL = WORDS + 3 * TL_TILE;                            // + the maps (gather: rows, columns; blend: tile, column, weight)
    TL_MHD int word(int j, int w) { return (j >> 2) * SR + (j & 3) * RWP + w; }
    TL_MHD int byte(int j, int c) { return 4 * word(j, 0) + c; }
};

// first element of frame row (d, i) of frame f at row j
TL_HD size_t tl_frame_at(long f, int D, int d, int i, int j, int Nx, int Ny) { return (((size_t)f * D + d) * Nx + i) * (size_t)Ny + j; }

template <int D, bool F32>
TL_HD void tile_gather_body(const TlArgs& a, unsigned t, unsigned f, unsigned* lds)
{
    typedef TlLds<D> L;
    int* ymap = reinterpret_cast<int*>(lds + L::WORDS);
    int* xmap = ymap + TL_TILE;
    const int Nx = a.x.N, Ny = a.y.N, tid = (int)threadIdx.x;
    const unsigned bj = t / (unsigned)a.bx, fr = f / (unsigned)a.x.n, b = fr / (unsigned)a.y.n;   // block t of tile f = (b nty + ty) ntx + tx
    const int i0 = (int)(t - bj * a.bx) * TL_TILE, j0 = (int)bj * TL_TILE, tx = (int)(f - fr * a.x.n), ty = (int)(fr - b * a.y.n);
    const int ncols = tl_min(Nx - i0, TL_TILE), nrows = tl_min(Ny - j0, TL_TILE);
    const int xs = a.x.o0 + tx * a.x.S + i0, ys = a.y.o0 + ty * a.y.S + j0;      // the block's first column and row in image coordinates
    // the source columns of the block are the span [xlo, xhi] of at most 64 columns, in order (the block lies inside the image) or folded
    int xlo, xhi;
    tl_reflect_range(xs, ncols, a.x.W, &xlo, &xhi);
    const bool folded = xs < 0 || xs + ncols > a.x.W;
    if (tid < TL_TILE) ymap[tid] = tl_reflect(ys + tid, a.y.W);
    else if (tid < 2 * TL_TILE) xmap[tid - TL_TILE] = tl_reflect(xs + tid - TL_TILE, a.x.W) - xlo;      // column i of the block is column xmap[i] of the span
    __syncthreads();
    const unsigned char* img = a.image + (size_t)b * a.stride;
    const int nb = (xhi - xlo + 1) * D;                                          // bytes of the span
    int s = 0;                                                                   // byte phase of the span's first column within its LDS row
    if (a.img_words) {
        s = (xlo * D) & 3;
        const int a0 = xlo * D - s, nw = (s + nb + 3) >> 2, live = a.x.W * D;
        for (int idx = tid; idx < nrows * L::RWP; idx += 256) {
            const int j = idx / L::RWP, w = idx - j * L::RWP;
            if (w >= nw) continue;
            const unsigned char* p = img + (size_t)ymap[j] * a.pitch + a0 + 4 * w;
            const int n = live - (a0 + 4 * w);
            unsigned v = 0;
            if (n >= 4) v = *reinterpret_cast<const unsigned*>(p);
            else
                for (int k = 0; k < n; ++k) v |= (unsigned)p[k] << (8 * k);      // (the dword that crosses the row's end: its live bytes only)
            lds[L::word(j, w)] = v;
        }
    } else {
        unsigned char* lb = reinterpret_cast<unsigned char*>(lds);
        for (int idx = tid; idx < nrows * (TL_TILE * D); idx += 256) {
            const int j = idx / (TL_TILE * D), c = idx - j * (TL_TILE * D);
            if (c < nb) lb[L::byte(j, c)] = img[(size_t)ymap[j] * a.pitch + (size_t)xlo * D + c];
        }
    }
    __syncthreads();
    if (a.frm_words && folded) {                                                  // a block on the image's left or right edge: its bytes one by one out of the span
        const unsigned char* lb = reinterpret_cast<const unsigned char*>(lds);
        for (int blk = tid; blk < 16 * L::RW; blk += 256) {
            const int q = blk & 15, g = blk >> 4;
            if (4 * q >= nrows) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = 4 * g + e, i = c / D, d = c - i * D;
                if (i >= ncols) continue;
                const int at = L::byte(4 * q, s + xmap[i] * D + d);
                const unsigned p0 = lb[at], p1 = lb[at + 4 * L::RWP], p2 = lb[at + 8 * L::RWP], p3 = lb[at + 12 * L::RWP];
                const size_t o = tl_frame_at(f, D, d, i0 + i, j0 + 4 * q, Nx, Ny);
                if constexpr (F32) {
                    float4 v; v.x = (float)p0; v.y = (float)p1; v.z = (float)p2; v.w = (float)p3;
                    *reinterpret_cast<float4*>(static_cast<float*>(a.frames) + o) = v;
                } else *reinterpret_cast<unsigned*>(static_cast<unsigned char*>(a.frames) + o) = p0 | p1 << 8 | p2 << 16 | p3 << 24;
            }
        }
    } else if (a.frm_words) {
        for (int blk = tid; blk < 16 * L::RW; blk += 256) {
            const int q = blk & 15, g = blk >> 4;
            if (4 * q >= nrows) continue;                                         // (Ny is a multiple of 4: a block of four rows is live or not)
            unsigned rr[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned lo = lds[q * L::SR + k * L::RWP + g], hi = lds[q * L::SR + k * L::RWP + g + 1];
                rr[k] = (unsigned)((((unsigned long long)hi << 32) | lo) >> (8 * s));
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = 4 * g + e, i = c / D, d = c - i * D;
                if (i >= ncols) continue;
                const unsigned p0 = (rr[0] >> (8 * e)) & 255u, p1 = (rr[1] >> (8 * e)) & 255u, p2 = (rr[2] >> (8 * e)) & 255u, p3 = (rr[3] >> (8 * e)) & 255u;
                const size_t o = tl_frame_at(f, D, d, i0 + i, j0 + 4 * q, Nx, Ny);
                if constexpr (F32) {
                    float4 v; v.x = (float)p0; v.y = (float)p1; v.z = (float)p2; v.w = (float)p3;
                    *reinterpret_cast<float4*>(static_cast<float*>(a.frames) + o) = v;
                } else *reinterpret_cast<unsigned*>(static_cast<unsigned char*>(a.frames) + o) = p0 | p1 << 8 | p2 << 16 | p3 << 24;
            }
        }
    } else {
        const unsigned char* lb = reinterpret_cast<const unsigned char*>(lds);
        for (int idx = tid; idx < TL_TILE * D * TL_TILE; idx += 256) {
            const int j = idx & 63, c = idx >> 6, i = c / D, d = c - i * D;
            if (j >= nrows || i >= ncols) continue;
            const unsigned char v = lb[L::byte(j, s + xmap[i] * D + d)];
            const size_t o = tl_frame_at(f, D, d, i0 + i, j0 + j, Nx, Ny);
            if constexpr (F32) static_cast<float*>(a.frames)[o] = (float)v;
            else static_cast<unsigned char*>(a.frames)[o] = v;
        }
    }
}

// the pixels of elements o .. o + 3 of the frames: all four at once (WORDS: o is a multiple of 4), or those whose weight is not zero
template <bool F32, bool WORDS>
TL_HD void tl_load4(const void* frames, size_t o, const int* w, unsigned* p)
{
    if constexpr (WORDS) {
        if constexpr (F32) {
            const float4 v = *reinterpret_cast<const float4*>(static_cast<const float*>(frames) + o);
            p[0] = px_u8(v.x); p[1] = px_u8(v.y); p[2] = px_u8(v.z); p[3] = px_u8(v.w);
        } else {
            const unsigned v = *reinterpret_cast<const unsigned*>(static_cast<const unsigned char*>(frames) + o);
            p[0] = v & 255u; p[1] = (v >> 8) & 255u; p[2] = (v >> 16) & 255u; p[3] = v >> 24;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            p[k] = 0;
            if (w[k] == 0) continue;
            if constexpr (F32) p[k] = px_u8(static_cast<const float*>(frames)[o + k]);
            else p[k] = static_cast<const unsigned char*>(frames)[o + k];
        }
    }
}

// sum over the tile rows of wy p for rows k .. k + 3 of column (d, i) of the tile at column tx: the primary tile row ty and, where wb is set, ty - 1
template <int D, bool F32, bool WORDS>
TL_HD void tl_column(const TlArgs& a, long frow, int tx, int d, int i, int k, const int* wa, const int* wb, bool anyb, unsigned* acc)
{
    unsigned p[4];
    tl_load4<F32, WORDS>(a.frames, tl_frame_at(frow + tx, D, d, i, k, a.x.N, a.y.N), wa, p);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = (unsigned)wa[e] * p[e];
    if (anyb) {
        tl_load4<F32, false>(a.frames, tl_frame_at(frow - a.x.n + tx, D, d, i, k + a.y.S, a.x.N, a.y.N), wb, p);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += (unsigned)wb[e] * p[e];
    }
}

template <int D, bool F32, bool WORDS>
TL_HD void tile_blend_lanes(const TlArgs& a, long frow, int ty, int kb, int rlo, int rhi, int nc, unsigned* lds)
{
    typedef TlLds<D> L;
    const int* ctx = reinterpret_cast<const int*>(lds + L::WORDS);
    const int *ckx = ctx + TL_TILE, *cwx = ckx + TL_TILE;
    const unsigned dd = (unsigned)a.x.den * (unsigned)a.y.den;
    for (int blk = (int)threadIdx.x; blk < 16 * L::RW; blk += 256) {
        const int q = blk & 15, g = blk >> 4, k = kb + 4 * q;
        if (4 * q + 3 < rlo || 4 * q >= rhi) continue;
        int wa[4], wb[4];
        bool anyb = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int kk = k + e, row = 4 * q + e;
            const bool live = row >= rlo && row < rhi;
            wa[e] = !live ? 0 : (ty > 0 && kk < a.y.M + a.y.R) ? 2 * (kk - a.y.M) + 1 : a.y.den;
            wb[e] = live ? a.y.den - wa[e] : 0;
            anyb = anyb || wb[e] != 0;
        }
        unsigned out[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int c = 4 * g + s, i = c / D, d = c - i * D;
            if (i >= nc) continue;                                                // (columns beyond the image: bytes the image side never stores)
            const int tx = ctx[i], kx = ckx[i], wx = cwx[i];
            unsigned acc[4];
            tl_column<D, F32, WORDS>(a, frow, tx, d, kx, k, wa, wb, anyb, acc);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] *= (unsigned)wx;
            if (wx != a.x.den) {                                                  // the left ramp of tile column tx: the one before it contributes
                unsigned acc2[4];
                tl_column<D, F32, WORDS>(a, frow, tx - 1, d, kx + a.x.S, k, wa, wb, anyb, acc2);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] += acc2[e] * (unsigned)(a.x.den - wx);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) out[e] |= tl_div(2u * acc[e] + dd, a.mul, a.shift) << (8 * s);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) lds[q * L::SR + e * L::RWP + g] = out[e];
    }
}

template <int D, bool F32>
TL_HD void tile_blend_body(const TlArgs& a, unsigned t, unsigned u, unsigned* lds)
{
    typedef TlLds<D> L;
    int* ctx = reinterpret_cast<int*>(lds + L::WORDS);
    int *ckx = ctx + TL_TILE, *cwx = ckx + TL_TILE;
    const int tid = (int)threadIdx.x;
    const unsigned m = t / (unsigned)a.bx, b = u / (unsigned)a.y.n;              // block t of tile row u = b nty + ty
    const int X0 = (int)(t - m * a.bx) * TL_TILE, kb = (int)m * TL_TILE, ty = (int)(u - b * a.y.n);
    const int nc = tl_min(a.x.W - X0, TL_TILE), oy = a.y.o0 + ty * a.y.S;
    // the rows whose primary tile row is ty: k in [M, M + S) (the last tile row: to N - M), inside the image
    const int klo = tl_max(a.y.M, -oy), khi = tl_min(ty == a.y.n - 1 ? a.y.N - a.y.M : a.y.M + a.y.S, a.y.W - oy);
    const int rlo = tl_max(klo - kb, 0), rhi = tl_min(khi - kb, TL_TILE);
    if (rlo >= rhi) return;                                                       // (uniform: this chunk of the tile row holds no row of its own)
    if (tid < nc) {
        const int u = X0 + tid - a.x.o0, tx = tl_min(a.x.n - 1, (u - a.x.M) / a.x.S), kx = u - tx * a.x.S;
        ctx[tid] = tx; ckx[tid] = kx;
        cwx[tid] = (tx > 0 && kx < a.x.M + a.x.R) ? 2 * (kx - a.x.M) + 1 : a.x.den;
    }
    __syncthreads();
    const long frow = (long)u * a.x.n;                                            // the first frame of tile row ty of image b
    if (a.frm_words) tile_blend_lanes<D, F32, true>(a, frow, ty, kb, rlo, rhi, nc, lds);
    else tile_blend_lanes<D, F32, false>(a, frow, ty, kb, rlo, rhi, nc, lds);
    __syncthreads();
    unsigned char* img = const_cast<unsigned char*>(a.image) + (size_t)b * a.stride + (size_t)X0 * D;   // column X0 of image b's row 0
    const int nb = nc * D, nr = rhi - rlo, y0 = oy + kb;                         // block row j is image row y0 + j (>= 0 from rlo on)
    if (a.img_words) {
        for (int idx = tid; idx < nr * L::RW; idx += 256) {
            const int j = rlo + idx / L::RW, w = idx % L::RW, n = nb - 4 * w;
            if (n <= 0) continue;
            unsigned char* p = img + (size_t)(y0 + j) * a.pitch + 4 * w;
            const unsigned v = lds[L::word(j, w)];
            if (n >= 4) *reinterpret_cast<unsigned*>(p) = v;
            else
                for (int k = 0; k < n; ++k) p[k] = (unsigned char)(v >> (8 * k));
        }
    } else {
        const unsigned char* lb = reinterpret_cast<const unsigned char*>(lds);
        for (int idx = tid; idx < nr * (TL_TILE * D); idx += 256) {
            const int j = rlo + idx / (TL_TILE * D), c = idx % (TL_TILE * D);
            if (c < nb) img[(size_t)(y0 + j) * a.pitch + c] = lb[L::byte(j, c)];
        }
    }
}

// the launch geometry: grid.x = the blocks of a unit, the units (at most 2^31 - 1) on grid.y x grid.z
static inline bool tl_geometry(const aefft_tile_desc* desc, const unsigned char* image, size_t pitch, size_t stride, void* frames, int B, bool blend, TlArgs* g)
{
    if (!desc || !tl_axis(desc->W, desc->Nx, desc->overlap_x, desc->rim_x, &g->x) || !tl_axis(desc->H, desc->Ny, desc->overlap_y, desc->rim_y, &g->y)) return false;
    g->image = image; g->pitch = pitch; g->stride = B > 1 ? stride : 0; g->frames = frames;
    g->by = (g->y.N + TL_TILE - 1) / TL_TILE;
    if (blend) {
        g->bx = (g->x.W + TL_TILE - 1) / TL_TILE;
        g->units = B * g->y.n;
    } else {
        g->bx = (g->x.N + TL_TILE - 1) / TL_TILE;
        g->units = B * g->y.n * g->x.n;                                          // (the entry point has checked that it fits)
    }
    g->img_words = ((reinterpret_cast<uintptr_t>(image) | pitch | g->stride) & 3u) == 0;
    g->frm_words = (g->y.N & 3) == 0;
    tl_magic(2u * (unsigned)g->x.den * (unsigned)g->y.den, &g->mul, &g->shift);
    return true;
}
static inline unsigned tl_grid_y(const TlArgs& g) { return (unsigned)(g.units < 65535 ? g.units : 65535); }   // unit = z grid.y + y (workgroups beyond return at once)
static inline unsigned tl_grid_z(const TlArgs& g) { return ((unsigned)g.units + tl_grid_y(g) - 1) / tl_grid_y(g); }

#ifndef AEFFT_HOSTCHECK
template <int D, bool F32>
__global__ __launch_bounds__(256) void tile_gather_kernel(const TlArgs a)
{
    __shared__ unsigned lds[TlLds<D>::TOTAL];
    const unsigned u = blockIdx.z * gridDim.y + blockIdx.y;
    if (u < (unsigned)a.units) tile_gather_body<D, F32>(a, blockIdx.x, u, lds);
}

template <int D, bool F32>
__global__ __launch_bounds__(256) void tile_blend_kernel(const TlArgs a)
{
    __shared__ unsigned lds[TlLds<D>::TOTAL];
    const unsigned u = blockIdx.z * gridDim.y + blockIdx.y;
    if (u < (unsigned)a.units) tile_blend_body<D, F32>(a, blockIdx.x, u, lds);
}

#define TL_LAUNCH(KERNEL)                                                                                 \
    do {                                                                                                  \
        const dim3 gr((unsigned)(g.bx * g.by), tl_grid_y(g), tl_grid_z(g)), bl(256);                                                             \
        switch (D * 2 + (f32 ? 1 : 0)) {                                                                  \
            case 2: KERNEL<1, false><<<gr, bl, 0, st>>>(g); break;                                       \
            case 3: KERNEL<1, true><<<gr, bl, 0, st>>>(g); break;                                        \
            case 4: KERNEL<2, false><<<gr, bl, 0, st>>>(g); break;                                       \
            case 5: KERNEL<2, true><<<gr, bl, 0, st>>>(g); break;                                        \
            case 6: KERNEL<3, false><<<gr, bl, 0, st>>>(g); break;                                       \
            case 7: KERNEL<3, true><<<gr, bl, 0, st>>>(g); break;                                        \
            case 8: KERNEL<4, false><<<gr, bl, 0, st>>>(g); break;                                       \
            default: KERNEL<4, true><<<gr, bl, 0, st>>>(g); break;                                       \
        }                                                                                                 \
    } while (0)

static bool tl_args_ok(const void* image, size_t pitch, const void* frames, const aefft_tile_desc* desc, int B, int D)
{
    return image && frames && desc && B >= 1 && D >= 1 && D <= 4 && desc->W >= 1 && pitch >= (size_t)desc->W * D;
}

hipError_t launch_tile_gather(const unsigned char* image, size_t pitch, size_t stride, const aefft_tile_desc* desc, void* frames, bool f32, int B, int D, hipStream_t st)
{
    TlArgs g;
    if (!tl_args_ok(image, pitch, frames, desc, B, D) || !tl_geometry(desc, image, pitch, stride, frames, B, false, &g)) return hipErrorInvalidValue;
    TL_LAUNCH(tile_gather_kernel);
    return hipGetLastError();
}

hipError_t launch_tile_blend(const void* frames, bool f32, const aefft_tile_desc* desc, unsigned char* image, size_t pitch, size_t stride, int B, int D, hipStream_t st)
{
    TlArgs g;
    if (!tl_args_ok(image, pitch, frames, desc, B, D) || !tl_geometry(desc, image, pitch, stride, const_cast<void*>(frames), B, true, &g)) return hipErrorInvalidValue;
    TL_LAUNCH(tile_blend_kernel);
    return hipGetLastError();
}
#endif

}  // namespace aefft
