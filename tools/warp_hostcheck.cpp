// aefft_image_warp_affine and aefft_image_remap without a device: the kernel source itself --
// autoencoder-fft_amd/csrc/warp_kernels.hip, the two bodies and the launch geometry -- compiled for the HOST, 256 threads as the lanes of a
// workgroup, under the sanitizers, with the source images, the destination images, the affines and the table allocated at exactly their live
// extent (a read or a write one byte outside any of them stops the program), against a scalar C restatement of include/aefft.h's definition that
// shares nothing with the kernels: one pixel and one channel at a time, 128-bit arithmetic reduced modulo 2^64 for U and V, the border rule by a
// loop that walks the reflection, the taps and weights straight from the header's formulas.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Wno-unknown-pragmas
//       -o warp_hostcheck tools/warp_hostcheck.cpp   (one line),   then   ./warp_hostcheck   (./warp_hostcheck quick: the small sweep)
//
// A stand-alone program: it is not loaded into Python and does not touch a GPU.  Exit status 0 and "all N runs exact" when every run is
// byte-exact on every byte of the destination buffer, the bytes between the rows and the images included.
#include "hostlanes.h"
#include "../autoencoder-fft_amd/csrc/warp_kernels.hip"

using namespace aefft;

// ---- the definition, restated -----------------------------------------------------------------------
static long long ref_floor_div(long long a, long long b) { long long q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }

// the index of a tap at s on an axis of S under the border rule; false: the tap has the constant
static bool ref_border(long long s, int S, int border, int* idx)
{
    if (s >= 0 && s < S) { *idx = (int)s; return true; }
    if (border == 0) { *idx = 0; return false; }
    if (border == 1) { *idx = s < 0 ? 0 : S - 1; return true; }
    if (S == 1) { *idx = 0; return true; }
    const long long P = 2 * (S - 1);
    long long m = s - ref_floor_div(s, P) * P;                                    // s mod P, non-negative
    *idx = (int)(m < S ? m : P - m);
    return true;
}

static unsigned ref_tap(const unsigned char* img, size_t pitch, int Ws, int Hs, int D, long long sy, long long sx, int d, int border, unsigned bval)
{
    int ix, iy;
    const bool lx = ref_border(sx, Ws, border, &ix), ly = ref_border(sy, Hs, border, &iy);
    return lx && ly ? img[(size_t)iy * pitch + (size_t)ix * D + d] : (bval >> (8 * d)) & 255u;
}

static unsigned char ref_sample(const unsigned char* img, size_t pitch, int Ws, int Hs, int D, long long tx, long long ty, int d, int interp, int border, unsigned bval)
{
    if (interp == 0) return (unsigned char)ref_tap(img, pitch, Ws, Hs, D, ref_floor_div(ty + 1024, 2048), ref_floor_div(tx + 1024, 2048), d, border, bval);
    const long long sx = ref_floor_div(tx, 2048), sy = ref_floor_div(ty, 2048), wx = tx - sx * 2048, wy = ty - sy * 2048;
    const long long p00 = ref_tap(img, pitch, Ws, Hs, D, sy, sx, d, border, bval), p01 = ref_tap(img, pitch, Ws, Hs, D, sy, sx + 1, d, border, bval);
    const long long p10 = ref_tap(img, pitch, Ws, Hs, D, sy + 1, sx, d, border, bval), p11 = ref_tap(img, pitch, Ws, Hs, D, sy + 1, sx + 1, d, border, bval);
    const long long v = (2048 - wy) * ((2048 - wx) * p00 + wx * p01) + wy * ((2048 - wx) * p10 + wx * p11);
    return (unsigned char)ref_floor_div(v + (1LL << 21), 1LL << 22);
}

// tx of the affine: U modulo 2^64 as a signed value, (U + 2^12) modulo 2^64 likewise, the floor of its 2^13-th, clamped to int32
static long long ref_wrap(__int128 v)
{
    const __int128 M = (__int128)1 << 64;
    v %= M;
    if (v < 0) v += M;
    if (v >= M / 2) v -= M;
    return (long long)v;
}
static long long ref_q11(const long long* a, int x, int y)
{
    const long long U = ref_wrap((__int128)a[0] * x + (__int128)a[1] * y + (__int128)a[2]);
    const long long t = ref_floor_div(ref_wrap((__int128)U + 4096), 8192);
    return t < -2147483648LL ? -2147483648LL : t > 2147483647LL ? 2147483647LL : t;
}

// ---- the buffers, at their exact extent ---------------------------------------------------------------
struct Image {
    unsigned char *base, *p; size_t pitch, stride, extent; int W, H, B, D;
};
// `off`: the bytes the pointer stands behind a 16-byte boundary; `pad`: the bytes of a row beyond W D; `gap`: the bytes between two images
static Image image(int W, int H, int B, int D, int off, int pad, int gap)
{
    Image m;
    m.W = W; m.H = H; m.B = B; m.D = D;
    m.pitch = (size_t)W * D + pad;
    m.stride = (size_t)(H - 1) * m.pitch + (size_t)W * D + gap;
    m.extent = (size_t)(B - 1) * m.stride + (size_t)(H - 1) * m.pitch + (size_t)W * D;
    void* q = nullptr;
    if (posix_memalign(&q, 16, m.extent + off)) abort();
    m.base = (unsigned char*)q; m.p = m.base + off;
    return m;
}

static long long rnd64() { unsigned long long v = 0; for (int k = 0; k < 8; ++k) v = v << 8 | rnd(); return (long long)v; }
static int rnd_in(int lo, int hi) { return lo + (int)(((rnd() << 8 | rnd()) * (unsigned)(hi - lo + 1)) >> 16); }

// a run: the launch exactly as the launcher sizes it, every byte of the destination buffer against the restatement (0xEE where nothing is written)
static void check(const char* name, const Image& s, const Image& d, const WpAffine* m, int nm, const int* map, int interp, int border, unsigned bval)
{
    ++runs;
    WpArgs g;
    unsigned tiles = 0;
    if (!wp_geometry(s.p, s.pitch, s.stride, s.W, s.H, interp, border, bval, d.p, d.pitch, d.stride, d.W, d.H, d.B, d.D, &g, &tiles)) abort();
    g.m = m; g.nm = nm; g.map = map;
    memset(d.base, 0xEE, d.extent + (size_t)(d.p - d.base));
    const unsigned gy = map ? wp_remap_split(tiles, d.B) : (unsigned)d.B;
    launch(tiles, gy, 1, 0, [&](unsigned*) {
        switch (d.D) {
            case 1: map ? warp_remap_body<1>(g, blockIdx.x, blockIdx.y, gridDim.y, threadIdx.x) : warp_affine_body<1>(g, blockIdx.x, blockIdx.y, gridDim.y, threadIdx.x); break;
            case 2: map ? warp_remap_body<2>(g, blockIdx.x, blockIdx.y, gridDim.y, threadIdx.x) : warp_affine_body<2>(g, blockIdx.x, blockIdx.y, gridDim.y, threadIdx.x); break;
            case 3: map ? warp_remap_body<3>(g, blockIdx.x, blockIdx.y, gridDim.y, threadIdx.x) : warp_affine_body<3>(g, blockIdx.x, blockIdx.y, gridDim.y, threadIdx.x); break;
            default: map ? warp_remap_body<4>(g, blockIdx.x, blockIdx.y, gridDim.y, threadIdx.x) : warp_affine_body<4>(g, blockIdx.x, blockIdx.y, gridDim.y, threadIdx.x); break;
        }
    });
    std::vector<unsigned char> want(d.extent, 0xEE);
    for (int b = 0; b < d.B; ++b)
        for (int y = 0; y < d.H; ++y)
            for (int x = 0; x < d.W; ++x) {
                long long tx, ty;
                if (map) { tx = map[((size_t)y * d.W + x) * 2]; ty = map[((size_t)y * d.W + x) * 2 + 1]; }
                else { const long long* a = m[nm == 1 ? 0 : b].a; tx = ref_q11(a, x, y); ty = ref_q11(a + 3, x, y); }
                for (int c = 0; c < d.D; ++c)
                    want[(size_t)b * d.stride + (size_t)y * d.pitch + (size_t)x * d.D + c] =
                        ref_sample(s.p + (size_t)b * s.stride, s.pitch, s.W, s.H, s.D, tx, ty, c, interp, border, bval);
            }
    size_t bad = 0;
    for (size_t i = 0; i < d.extent; ++i) bad += d.p[i] != want[i];
    for (unsigned char* q = d.base; q < d.p; ++q) bad += *q != 0xEE;
    if (bad) {
        ++failures;
        printf("MISMATCH %s: %dx%d -> %dx%d D %d B %d nm %d interp %d border %d words %d: %zu bytes differ\n", name, s.W, s.H, d.W, d.H, d.D, d.B, nm, interp, border,
               g.dst_words, bad);
    }
}

static WpAffine q24(double m0, double m1, double m2, double m3, double m4, double m5)
{
    const double m[6] = {m0, m1, m2, m3, m4, m5};
    WpAffine a;
    for (int k = 0; k < 6; ++k) a.a[k] = (long long)nearbyint(m[k] * 16777216.0);
    return a;
}

// every affine and every table of the sweep on one pair of shapes
static void run(int Ws, int Hs, int Wd, int Hd, int D, int B, bool aligned, bool quick, int pick)
{
    Image s = image(Ws, Hs, B, D, aligned ? 0 : 1, aligned ? (-(Ws * D) & 3) : 5, aligned ? 8 : 3);
    Image d = image(Wd, Hd, B, D, aligned ? 0 : 1, aligned ? (-(Wd * D) & 3) + 4 : 5, aligned ? (-(Wd * D) & 3) + 4 : 7);
    for (size_t i = 0; i < s.extent; ++i) s.p[i] = (unsigned char)rnd();
    const unsigned bval = 0x44332211u + (unsigned)pick;
    const double c30 = 0.8 * 0.8660254037844386, s30 = 0.8 * 0.5;
    std::vector<WpAffine> af = {
        q24(1, 0, 0, 0, 1, 0), q24(1, 0, -3, 0, 1, 2), q24(0, 1, 0, -1, 0, Hs - 1), q24(0, -1, Ws - 1, 1, 0, 0), q24(-1, 0, Ws - 1, 0, 1, 0),
        q24(c30, -s30, 0.31 * Ws, s30, c30, -0.2 * Hs), q24(3.7, 0, 0.4, 0, 3.7, -0.3), q24(1, 0, 0.5, 0, 1, 0.5), q24(1, 0, 20000, 0, 1, -20000),
        q24(32, -32, 32768, -32, 32, -32768), q24(0.25, 0.01, -0.6, -0.02, 0.3, Hs - 0.7)};
    for (int k = 0; k < 3; ++k) {                                                 // any bit pattern: the wrap and the clamp
        WpAffine a;
        for (int e = 0; e < 6; ++e) a.a[e] = k == 0 ? rnd64() : k == 1 ? (e % 3 == 2 ? rnd64() >> 20 : (long long)1 << (62 - e)) : (rnd64() >> (8 * e));
        af.push_back(a);
    }
    WpAffine* per = (WpAffine*)malloc(sizeof(WpAffine) * B);                      // (exactly nm of them)
    WpAffine* one = (WpAffine*)malloc(sizeof(WpAffine));
    int turn = pick;
    for (size_t k = 0; k < af.size(); ++k) {
        if (quick && (k + pick) % 3) continue;
        for (int interp = 0; interp < 2; ++interp)
            for (int border = 0; border < 3; ++border) {
                if (quick && (turn++ % 4)) continue;
                *one = af[k];
                check("affine", s, d, one, 1, nullptr, interp, border, bval);
                if (B > 1 && border == (int)(k % 3)) {
                    for (int b = 0; b < B; ++b) per[b] = af[(k + b) % af.size()];
                    check("affines", s, d, per, B, nullptr, interp, border, bval);
                }
            }
    }
    // the tables: the identity, positions inside the image, any int32, the extremes and just outside each edge
    int* map = (int*)malloc(sizeof(int) * 2 * Wd * Hd);
    for (int kind = 0; kind < 4; ++kind) {
        for (int y = 0; y < Hd; ++y)
            for (int x = 0; x < Wd; ++x) {
                int* e = map + ((size_t)y * Wd + x) * 2;
                if (kind == 0) { e[0] = 2048 * x; e[1] = 2048 * y; }
                else if (kind == 1) { e[0] = rnd_in(0, 2048 * (Ws - 1)); e[1] = rnd_in(0, 2048 * (Hs - 1)); }
                else if (kind == 2) { e[0] = (int)rnd64(); e[1] = (int)rnd64(); }
                else {
                    const int xs[8] = {-2147483647 - 1, 2147483647, -1, -1024, -1025, 2048 * (Ws - 1) + 1, 2048 * Ws - 1024, 2048 * Ws};
                    const int ys[8] = {-2147483647 - 1, 2147483647, -1, -1024, -1025, 2048 * (Hs - 1) + 1, 2048 * Hs - 1024, 2048 * Hs};
                    e[0] = xs[rnd() % 8]; e[1] = rnd() & 1 ? ys[rnd() % 8] : rnd_in(0, 2048 * (Hs - 1));
                }
            }
        for (int interp = 0; interp < 2; ++interp)
            for (int border = 0; border < 3; ++border) {
                if (quick && (turn++ % 4)) continue;
                check("remap", s, d, nullptr, 0, map, interp, border, bval);
            }
    }
    free(map); free(per); free(one); free(s.base); free(d.base);
}

int main(int argc, char** argv)
{
    const bool quick = argc > 1 && !strcmp(argv[1], "quick");
    // the tile is 32 x 32 and a lane owns 4 pixels: one pixel, a row end inside a lane's four, a tile and a bit in both directions, two tiles and a bit
    struct Shape { int Ws, Hs, Wd, Hd; };
    std::vector<Shape> shapes = {{1, 1, 1, 1}, {1, 9, 17, 5}, {53, 37, 65, 33}, {7, 1, 4, 3}};
    if (!quick) shapes.insert(shapes.end(), {{96, 64, 130, 67}, {2, 2, 33, 1}, {64, 48, 64, 48}, {3, 129, 1, 70}});
    int pick = 0;
    for (const Shape& sh : shapes)
        for (int D = 1; D <= 4; ++D)
            for (int B = 1; B <= 3; B += 2) {
                if (quick && (pick + D + B) % 3) { ++pick; continue; }
                run(sh.Ws, sh.Hs, sh.Wd, sh.Hd, D, B, (pick & 1) != 0, quick, pick);
                if (!quick) run(sh.Ws, sh.Hs, sh.Wd, sh.Hd, D, B, (pick & 1) == 0, quick, pick + 1);
                ++pick;
            }
    // a batch past the remap's split: more images than workgroups along y (the full sweep only: 2048 workgroups a launch)
    if (!quick) run(40, 30, 33, 9, 3, 2500, true, true, 7);
    return report();
}
