// aefft_raw_to_image (gfx950): the raw samples of an industrial camera -- a Bayer mosaic or a mono sensor, 8 bits, 9..16 bits in 16-bit words, or
// GenICam's packed 10p / 12p rows -- to the interleaved 8-bit images every image call takes, one launch.  All-integer behind the host's
// quantisations (include/aefft.h states every step): linearise (black level, gain, clip: Q16 grey levels), demosaic (BILINEAR or the
// Malvar-He-Cutler 5 x 5 filters in sixteenths, reflected borders), colour matrix in Q10, then the byte or the 4096-entry table.
//   bayer_kernel<CONT, METHOD>   a workgroup owns a tile of BA_TW x BA_TH destination pixels.  STAGING: the tile plus the groups of 4 samples that
//                                hold its 2-pixel halo -- BA_SW x BA_SH samples from (x0 - 4, y0 - 2) -- are loaded, unpacked and linearised to Q16
//                                dwords in LDS, each exactly once.  A lane takes an ITEM, 4 samples of a row from x = 0 mod 4 (U8: one dword, U16: two,
//                                PACKED: the two aligned dwords that hold its 5 or 6 bytes), both of a lane's items loaded before the first is
//                                converted.  The container and the word / byte route differ HERE only.  DEMOSAIC: a lane owns a 2 x 2 quad, so every
//                                lane does one site of each type; which is which (the pattern: the parity of the R site) is uniform, and the
//                                branches on it are scalar.  The 6 x 6 window is written as 18 aligned pairs (BA_SW is even), so that a half-wave
//                                -- one row of quads -- can read 64 consecutive dwords, one bank row, with one 64-bit read; the compiler drops the
//                                samples a method never uses and emits 64-bit reads for the whole pairs and 32-bit ones for the rest (DESIGN.md
//                                section 28 has the mix: the 32-bit ones are two-way conflicted at this lane stride of 2 dwords).
//                                OUTPUT: the quad's 12 bytes go to a second LDS region laid out as the tile's image rows (192 bytes each), and behind
//                                a barrier the workgroup stores them as dwords along the rows -- or as bytes where the image is not word-aligned and
//                                for the dword that crosses a row's end.
//   mono_kernel<CONT>            element-wise, no LDS: a lane owns one item and stores its 4 bytes as one dword (or bytes, as above).
// Loads: whole dwords when the data pointer, the pitch and the stride are multiples of 4 and the item lies inside the row, single samples
// (bytes; U16: halves, its pointers are even) otherwise -- the same two-route rule as yuv_kernels.hip's yv_ld.  A sample outside the image is the
// reflected one (the edge not repeated); a staged sample that no destination pixel needs is clamped into the image (loaded, never used).  Nothing
// beyond a row's live bytes is read.  Both routes give the same bytes.
// The 8-bit value is clamped in Q18 BEFORE the shift and packed with shifts and masks, as in yuv_kernels.hip.
// Plain C++ over (threadIdx, blockIdx, gridDim, __syncthreads) and an LDS pointer: tools/bayer_hostcheck.cpp compiles this file for the host, threads
// as lanes, under the sanitizers (AEFFT_HOSTCHECK: tools/hostlanes.h supplies those names and leaves the launchers out).  Every lane reaches every
// barrier: the tile body has no early return.
#include <math.h>
#ifndef AEFFT_HOSTCHECK
#include "internal.h"
#define BA_HD __host__ __device__ __forceinline__
#endif

namespace aefft {

constexpr int BA_RGGB = 0, BA_GRBG = 1, BA_GBRG = 2, BA_BGGR = 3, BA_MONO = 4;   // == AEFFT_RAW_RGGB .. AEFFT_RAW_MONO
constexpr int BA_U8 = 0, BA_U16 = 1, BA_PACKED = 2;                              // == AEFFT_RAW_U8 / _U16 / _PACKED
constexpr int BA_BILINEAR = 0, BA_MHC = 1;                                       // == AEFFT_DEMOSAIC_BILINEAR / _MHC
constexpr int BA_TW = 64, BA_TH = 16;            // destination pixels of a tile: 32 x 8 quads, one per lane
constexpr int BA_SW = BA_TW + 8, BA_SH = BA_TH + 4;   // staged samples: columns x0 - 4 .. x0 + 67 (whole groups of 4), rows y0 - 2 .. y0 + 17
constexpr int BA_GROUPS = BA_SW / 4;             // items of a staged row
constexpr int BA_ITEMS = BA_GROUPS * BA_SH;      // 360: at most 2 a lane
constexpr int BA_OUT_WORDS = BA_TW * 3 * BA_TH / 4;   // the tile's image rows: 16 rows of 48 dwords
constexpr int BA_LDS_WORDS = BA_SW * BA_SH + BA_OUT_WORDS;
constexpr unsigned BA_FULL = 255u << 16;         // 255 grey levels in Q16

BA_HD int ba_min(int a, int b) { return a < b ? a : b; }
BA_HD int ba_max(int a, int b) { return a > b ? a : b; }
// reflection without repeating the edge (-1 -> 1, n -> n - 2), exact for the reach of 2 the filters have (n >= 4); an index further out -- a staged
// sample no pixel needs -- ends up clamped
BA_HD int ba_reflect(int i, int n)
{
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return ba_min(ba_max(i, 0), n - 1);
}

// the source: image b at data + b * stride (stride 0 for B == 1); m, cap per colour R, G, B (MONO: entry 0)
struct BaSrc {
    const unsigned char* data; size_t pitch, stride;
    int W, H, bits, black;
    unsigned mask;                               // 2^bits - 1
    unsigned live;                               // bytes of a row that hold samples
    unsigned m[3], cap[3];                       // the multiplier and the clamp of s in front of it: min(s, cap) m < 2^32, same bits
    bool words;                                  // pointer, pitch and stride are multiples of 4
};
// include/aefft.h step 1, the host's part: m = floor(gain 255 65536 / (white - black) + 1/2) in double (the caller checks m <= 2^30)
static inline double ba_multiplier(float gain, int black, int white) { return floor((double)gain * 255.0 * 65536.0 / (double)(white - black) + 0.5); }
static inline unsigned ba_row_bytes(int container, int bits, int W) { return container == BA_U8 ? (unsigned)W : container == BA_U16 ? 2u * W : ((unsigned)W * bits + 7u) >> 3; }
static inline BaSrc ba_source(int container, int bits, int W, int H, const void* data, size_t pitch, size_t stride, int black, int white, const float* gain, int ngain, int B)
{
    BaSrc s;
    s.data = static_cast<const unsigned char*>(data); s.pitch = pitch; s.stride = B > 1 ? stride : 0;
    s.W = W; s.H = H; s.bits = bits; s.black = black; s.mask = (1u << bits) - 1u; s.live = ba_row_bytes(container, bits, W);
    for (int c = 0; c < 3; ++c) {
        const unsigned long long m = (unsigned long long)ba_multiplier(gain[c < ngain ? c : 0], black, white);
        s.m[c] = (unsigned)m;
        const unsigned long long cap = m ? (BA_FULL + m - 1) / m : 65535ull;      // ceil((255 << 16) / m): cap m >= 255 << 16, (cap - 1) m < 255 << 16
        s.cap[c] = (unsigned)(cap < 65535ull ? cap : 65535ull);
    }
    s.words = ((reinterpret_cast<uintptr_t>(data) | pitch | s.stride) & 3u) == 0;
    return s;
}

// an item as loaded: the 4 samples of a group.  U8: w0 = 4 bytes.  U16: w0, w1 = 2 halves each.  PACKED: bits sh .. sh + 4 bits - 1 of w1:w0
struct BaItem { unsigned w0, w1; int sh; };
// whether the item at x (a multiple of 4, maybe outside the row) loads whole dwords: the words route, its 4 samples exist and, PACKED, the two
// aligned dwords around its bytes lie inside the row's live bytes
template <int CONT>
BA_HD bool ba_fast(const BaSrc& s, int x)
{
    if (!s.words || x < 0 || x + 4 > s.W) return false;
    return CONT != BA_PACKED || (unsigned)((((x >> 2) * (s.bits >> 1)) & ~3) + 8) <= s.live;
}
// row: the first byte of the (reflected) source row
template <int CONT, bool FAST>
BA_HD BaItem ba_load(const BaSrc& s, const unsigned char* row, int x)
{
    BaItem it = {0u, 0u, 0};
    if (FAST) {
        if (CONT == BA_U8) it.w0 = *reinterpret_cast<const unsigned*>(row + x);
        else if (CONT == BA_U16) {
            const unsigned* p = reinterpret_cast<const unsigned*>(row + 2 * x);
            it.w0 = p[0]; it.w1 = p[1];
        } else {
            const int off = (x >> 2) * (s.bits >> 1);                            // a group of 4 samples is bits / 2 bytes
            const unsigned* p = reinterpret_cast<const unsigned*>(row + (off & ~3));
            it.w0 = p[0]; it.w1 = p[1]; it.sh = 8 * (off & 3);                   // (sh + 4 bits <= 64)
        }
    } else {
        unsigned r[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int xe = ba_reflect(x + e, s.W);
            if (CONT == BA_U8) r[e] = row[xe];
            else if (CONT == BA_U16) r[e] = *reinterpret_cast<const unsigned short*>(row + 2 * xe);
            else {
                const int bit = xe * s.bits;                                     // (a sample spans exactly two bytes, both live)
                const unsigned char* p = row + (bit >> 3);
                r[e] = (((unsigned)p[0] | (unsigned)p[1] << 8) >> (bit & 7)) & s.mask;
            }
        }
        if (CONT == BA_U8) it.w0 = r[0] | r[1] << 8 | r[2] << 16 | r[3] << 24;
        else if (CONT == BA_U16) { it.w0 = r[0] | r[1] << 16; it.w1 = r[2] | r[3] << 16; }
        else {
            const unsigned long long v = (unsigned long long)r[0] | (unsigned long long)r[1] << s.bits | (unsigned long long)r[2] << (2 * s.bits) |
                                         (unsigned long long)r[3] << (3 * s.bits);
            it.w0 = (unsigned)v; it.w1 = (unsigned)(v >> 32);
        }
    }
    return it;
}
// sample e of an item (bits above `bits` of a 16-bit word are dropped)
template <int CONT>
BA_HD unsigned ba_raw(const BaSrc& s, const BaItem& it, int e)
{
    if (CONT == BA_U8) return (it.w0 >> (8 * e)) & 255u;
    if (CONT == BA_U16) return ((e < 2 ? it.w0 : it.w1) >> (16 * (e & 1))) & s.mask;
    const unsigned long long v = ((unsigned long long)it.w1 << 32 | it.w0) >> it.sh;
    return (unsigned)(v >> (s.bits * e)) & s.mask;
}
// include/aefft.h step 1: u = min(max(r - black, 0) m, 255 << 16), the product in 32 bits behind the clamp of s
BA_HD unsigned ba_linear(int black, unsigned m, unsigned cap, unsigned r)
{
    const int d = (int)r - black;
    unsigned sv = d < 0 ? 0u : (unsigned)d;
    sv = sv < cap ? sv : cap;
    const unsigned u = sv * m;
    return u < BA_FULL ? u : BA_FULL;
}
// a Q10 coefficient (|c| < 2^13) times q (< 2^17): both fit 24 bits and the product 32, so the device multiplies at the full rate
BA_HD int ba_mul(int c, int q)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __mul24(c, q);
#else
    return c * q;
#endif
}
// include/aefft.h step 5: the byte of o (Q18), straight or through the table
BA_HD unsigned ba_byte(int o, const unsigned char* lut)
{
    if (lut) {
        const int t = o + (1 << 13);
        return lut[(unsigned)(t < 0 ? 0 : t > (4080 << 14) ? (4080 << 14) : t) >> 14];
    }
    const int t = o + (1 << 17);
    return (unsigned)(t < 0 ? 0 : t > 0x3ffffff ? 0x3ffffff : t) >> 18;         // clamped in Q18, then shifted
}

struct BaArgs {
    BaSrc s;
    int rx, ry;                                  // the parity of the R site: R at (x, y) with x = rx, y = ry (mod 2)
    int ccm[9];                                  // Q10, the rows in the order the channels are stored (BGR: the matrix's rows reversed)
    const unsigned char* lut;
    unsigned char* image; size_t pitch, stride;
    int B, gx, gy;                               // images; tiles (MONO: blocks of 64 groups, of 4 rows) along x and y
    bool img_words;
};

// ---- the demosaic ------------------------------------------------------------------------------
BA_HD int ba_clampq(int v) { return v < 0 ? 0 : v > (int)BA_FULL ? (int)BA_FULL : v; }
// the three colours (R, G, B) at the site w[cy][cx] of a window of Q16 samples.  is_g: a G site, r_row: its row holds R (so E, W are R and N, S are
// B); is_r: an R site (else a B site).  The three flags are uniform.
template <int METHOD>
BA_HD void ba_site(const int (&w)[6][6], int cx, int cy, bool is_g, bool r_row, bool is_r, int* rgb)
{
    const int c = w[cy][cx], N = w[cy - 1][cx], S = w[cy + 1][cx], E = w[cy][cx + 1], W = w[cy][cx - 1];
    const int diag = w[cy - 1][cx - 1] + w[cy - 1][cx + 1] + w[cy + 1][cx - 1] + w[cy + 1][cx + 1];
    const int v2 = w[cy - 2][cx] + w[cy + 2][cx], h2 = w[cy][cx - 2] + w[cy][cx + 2];
    if (!is_g) {
        int g, o;
        if (METHOD == BA_BILINEAR) { g = (N + S + E + W + 2) >> 2; o = (diag + 2) >> 2; }
        else {
            g = ba_clampq((8 * c + 4 * (N + S + E + W) - 2 * (v2 + h2) + 8) >> 4);
            o = ba_clampq((12 * c + 4 * diag - 3 * (v2 + h2) + 8) >> 4);
        }
        rgb[0] = is_r ? c : o; rgb[1] = g; rgb[2] = is_r ? o : c;
    } else {
        int h, v;
        if (METHOD == BA_BILINEAR) { h = (E + W + 1) >> 1; v = (N + S + 1) >> 1; }
        else {
            h = ba_clampq((10 * c + 8 * (E + W) - 2 * h2 + v2 - 2 * diag + 8) >> 4);
            v = ba_clampq((10 * c + 8 * (N + S) - 2 * v2 + h2 - 2 * diag + 8) >> 4);
        }
        rgb[0] = r_row ? h : v; rgb[1] = c; rgb[2] = r_row ? v : h;
    }
}

struct __attribute__((aligned(8))) BaPair { unsigned a, b; };

template <int CONT, int METHOD>
__device__ __forceinline__ void bayer_body(const BaArgs& a, unsigned* lds)
{
    unsigned* tile = lds;                                                        // [BA_SH][BA_SW] Q16 samples
    unsigned* outw = lds + BA_SW * BA_SH;                                        // [BA_TH][48] dwords: the tile's image rows
    const BaSrc& s = a.s;
    const int tid = (int)threadIdx.x;
    const int ty = (int)blockIdx.x / a.gx, x0 = ((int)blockIdx.x - ty * a.gx) * BA_TW, y0 = ty * BA_TH;
    // grid.y: the images, folded (uniform: a folded grid loops)
    for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
        const unsigned char* img = s.data + (size_t)b * s.stride;
        // staging: both items' loads before the first conversion; a lane without a second item repeats the last one (loaded, never used)
        {
            BaItem it[2];
            int row[2], grp[2];
            bool fast = true;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int idx = ba_min(tid + 256 * k, BA_ITEMS - 1);
                row[k] = idx / BA_GROUPS; grp[k] = idx - row[k] * BA_GROUPS;
                fast = fast && ba_fast<CONT>(s, x0 - 4 + 4 * grp[k]);
            }
            if (fast) {
#pragma unroll
                for (int k = 0; k < 2; ++k) it[k] = ba_load<CONT, true>(s, img + (size_t)ba_reflect(y0 - 2 + row[k], s.H) * s.pitch, x0 - 4 + 4 * grp[k]);
            } else {
#pragma unroll
                for (int k = 0; k < 2; ++k) it[k] = ba_load<CONT, false>(s, img + (size_t)ba_reflect(y0 - 2 + row[k], s.H) * s.pitch, x0 - 4 + 4 * grp[k]);
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (tid + 256 * k >= BA_ITEMS) continue;
                const int pb = (row[k] ^ a.ry) & 1;                              // (x0 - 4 and y0 - 2 are even: the staged indices carry the parity)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int pa = (e ^ a.rx) & 1, c = pa == pb ? 2 * pa : 1;    // R, G or B
                    const unsigned m = c == 0 ? s.m[0] : c == 1 ? s.m[1] : s.m[2], cap = c == 0 ? s.cap[0] : c == 1 ? s.cap[1] : s.cap[2];
                    tile[row[k] * BA_SW + 4 * grp[k] + e] = ba_linear(s.black, m, cap, ba_raw<CONT>(s, it[k], e));
                }
            }
        }
        __syncthreads();
        // the lane's quad: pixels (x0 + 2 qx + i, y0 + 2 qy + j); its window w[r][c] is the sample at (x0 + 2 qx - 2 + c, y0 + 2 qy - 2 + r)
        const int qx = tid & 31, qy = tid >> 5;
        int w[6][6];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const BaPair* p = reinterpret_cast<const BaPair*>(tile + (2 * qy + r) * BA_SW + 2 * qx + 2);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const BaPair v = p[c];
                w[r][2 * c] = (int)v.a; w[r][2 * c + 1] = (int)v.b;
            }
        }
        unsigned short* o16 = reinterpret_cast<unsigned short*>(outw);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            unsigned by[6];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const bool is_g = ((i ^ j ^ a.rx ^ a.ry) & 1) != 0, r_row = ((j ^ a.ry) & 1) == 0, is_r = ((i ^ a.rx) & 1) == 0;
                int rgb[3];
                ba_site<METHOD>(w, 2 + i, 2 + j, is_g, r_row, is_r, rgb);
                const int q0 = (rgb[0] + 128) >> 8, q1 = (rgb[1] + 128) >> 8, q2 = (rgb[2] + 128) >> 8;
#pragma unroll
                for (int d = 0; d < 3; ++d)
                    by[3 * i + d] = ba_byte(ba_mul(a.ccm[3 * d], q0) + ba_mul(a.ccm[3 * d + 1], q1) + ba_mul(a.ccm[3 * d + 2], q2), a.lut);   // |o| < 2^30
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) o16[(2 * qy + j) * (BA_TW * 3 / 2) + 3 * qx + k] = (unsigned short)(by[2 * k] | by[2 * k + 1] << 8);
        }
        __syncthreads();
        // the tile's rows as dwords along the rows (x0 * 3 is a multiple of 4); the dword that crosses the row's end, and every dword of an image
        // that is not word-aligned, as bytes
        const int live = ba_min(BA_TW, s.W - x0) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int idx = tid + 256 * k, r = idx / (BA_TW * 3 / 4), off = 4 * (idx - r * (BA_TW * 3 / 4));
            if (y0 + r >= s.H || off >= live) continue;
            const unsigned v = outw[idx];
            unsigned char* o = a.image + (size_t)b * a.stride + (size_t)(y0 + r) * a.pitch + (size_t)x0 * 3 + off;
            if (a.img_words && live - off >= 4) *reinterpret_cast<unsigned*>(o) = v;
            else {
#pragma unroll
                for (int n = 0; n < 4; ++n)
                    if (off + n < live) o[n] = (unsigned char)(v >> (8 * n));
            }
        }
        __syncthreads();                                                         // (the next image's staging overwrites the tile)
    }
}

// ---- mono ----------------------------------------------------------------------------------------
template <int CONT>
__device__ __forceinline__ void mono_body(const BaArgs& a)
{
    const BaSrc& s = a.s;
    const int tid = (int)threadIdx.x;
    const int by = (int)blockIdx.x / a.gx, bx = (int)blockIdx.x - by * a.gx;
    const int x = 4 * (bx * 64 + (tid & 63)), y = by * 4 + (tid >> 6);
    if (x >= s.W || y >= s.H) return;
    const int live = ba_min(4, s.W - x);
    for (int b = blockIdx.y; b < a.B; b += gridDim.y) {
        const unsigned char* row = s.data + (size_t)b * s.stride + (size_t)y * s.pitch;
        const BaItem it = ba_fast<CONT>(s, x) ? ba_load<CONT, true>(s, row, x) : ba_load<CONT, false>(s, row, x);
        unsigned out = 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int q = (int)((ba_linear(s.black, s.m[0], s.cap[0], ba_raw<CONT>(s, it, e)) + 128u) >> 8);
            out |= ba_byte(q << 10, a.lut) << (8 * e);
        }
        unsigned char* o = a.image + (size_t)b * a.stride + (size_t)y * a.pitch + x;
        if (a.img_words && live == 4) *reinterpret_cast<unsigned*>(o) = out;
        else {
#pragma unroll
            for (int n = 0; n < 4; ++n)
                if (n < live) o[n] = (unsigned char)(out >> (8 * n));
        }
    }
}

// the arguments and the launch geometry of either kernel.  ccm: null (the identity) or 9 floats, row-major, out = ccm * (R, G, B); quantised to Q10
// with floor(x 1024 + 1/2) and stored with the rows in the channels' order (order 0 BGR: reversed)
static inline BaArgs ba_geometry(int pattern, int container, int bits, int W, int H, const void* data, size_t pitch, size_t stride, int black, int white,
                                 const float* gain, const float* ccm, const unsigned char* lut, int order, unsigned char* image, size_t ipitch, size_t istride, int B)
{
    BaArgs g;
    const bool mono = pattern == BA_MONO;
    g.s = ba_source(container, bits, W, H, data, pitch, stride, black, white, gain, mono ? 1 : 3, B);
    g.rx = pattern == BA_GRBG || pattern == BA_BGGR; g.ry = pattern == BA_GBRG || pattern == BA_BGGR;
    for (int d = 0; d < 3; ++d)
        for (int j = 0; j < 3; ++j) {
            const int i = order == 0 ? 2 - d : d;                                // the matrix row stored as channel d
            g.ccm[3 * d + j] = ccm ? (int)floor((double)ccm[3 * i + j] * 1024.0 + 0.5) : (i == j ? 1024 : 0);
        }
    g.lut = lut; g.image = image; g.pitch = ipitch; g.stride = B > 1 ? istride : 0; g.B = B;
    if (mono) { g.gx = ((W + 3) / 4 + 63) / 64; g.gy = (H + 3) / 4; }
    else { g.gx = (W + BA_TW - 1) / BA_TW; g.gy = (H + BA_TH - 1) / BA_TH; }
    g.img_words = ((reinterpret_cast<uintptr_t>(image) | ipitch | g.stride) & 3u) == 0;
    return g;
}

#ifndef AEFFT_HOSTCHECK
template <int CONT, int METHOD>
__global__ __launch_bounds__(256) void bayer_kernel(const BaArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned ba_lds[BA_LDS_WORDS];
    bayer_body<CONT, METHOD>(a, ba_lds);
}

template <int CONT>
__global__ __launch_bounds__(256) void mono_kernel(const BaArgs a) { mono_body<CONT>(a); }

double raw_multiplier(float gain, int black, int white) { return ba_multiplier(gain, black, white); }

hipError_t launch_raw_image(const aefft_raw_desc& d, int order, unsigned char* image, size_t ipitch, size_t istride, int B, hipStream_t st)
{
    const bool mono = d.pattern == BA_MONO;
    const auto in = [](int v) { return v >= 4 && v <= 8192; };
    if (d.pattern < 0 || d.pattern > BA_MONO || d.container < 0 || d.container > BA_PACKED || (d.method != BA_BILINEAR && d.method != BA_MHC)) return hipErrorInvalidValue;
    if (d.container == BA_U8 ? d.bits != 8 : d.container == BA_U16 ? (d.bits < 9 || d.bits > 16) : (d.bits != 10 && d.bits != 12)) return hipErrorInvalidValue;
    if (!in(d.W) || !in(d.H) || B < 1 || !d.data || !image || d.black < 0 || d.black >= d.white || d.white > (1 << d.bits) - 1) return hipErrorInvalidValue;
    if (d.pitch < ba_row_bytes(d.container, d.bits, d.W) || ipitch < (size_t)d.W * (mono ? 1 : 3) || (!mono && order != 0 && order != 1)) return hipErrorInvalidValue;
    if (d.container == BA_U16 && ((reinterpret_cast<uintptr_t>(d.data) | d.pitch | (B > 1 ? d.stride : 0)) & 1u)) return hipErrorInvalidValue;
    const BaArgs g = ba_geometry(d.pattern, d.container, d.bits, d.W, d.H, d.data, d.pitch, d.stride, d.black, d.white, d.gain, mono ? nullptr : d.ccm, d.lut_d, order,
                                 image, ipitch, istride, B);
    const dim3 gr((unsigned)(g.gx * g.gy), (unsigned)B < 65535u ? (unsigned)B : 65535u), bl(256);   // at most 128 x 512 tiles (MONO: 32 x 2048 blocks) an image
#define BA_CASE(CC, MM) case ((CC) * 2 + (MM)): bayer_kernel<CC, MM><<<gr, bl, 0, st>>>(g); break;
#define MONO_CASE(CC) case (CC): mono_kernel<CC><<<gr, bl, 0, st>>>(g); break;
    if (mono) {
        switch (d.container) {
            MONO_CASE(0) MONO_CASE(1) MONO_CASE(2)
            default: return hipErrorInvalidValue;
        }
    } else {
        switch (d.container * 2 + d.method) {
            BA_CASE(0, 0) BA_CASE(0, 1) BA_CASE(1, 0) BA_CASE(1, 1) BA_CASE(2, 0) BA_CASE(2, 1)
            default: return hipErrorInvalidValue;
        }
    }
#undef MONO_CASE
#undef BA_CASE
    return hipGetLastError();
}
#endif

}  // namespace aefft
