// aefft_raw_to_image without a device: the kernel source itself -- autoencoder-fft_amd/csrc/bayer_kernels.hip, both bodies and
// the launch geometry -- compiled for the HOST, 256 threads as the lanes of a workgroup and a barrier for __syncthreads, under the sanitizers, with
// the source, the table, the image and the LDS allocated at exactly their live extent, against a scalar C restatement of include/aefft.h in 64-bit
// integers (its own unpacking bit by bit, its own 64-bit linearisation, its own filter tables and reflection: it shares nothing with the kernel).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -pthread -Wno-unknown-pragmas
//       -o bayer_hostcheck tools/bayer_hostcheck.cpp   (one line),   then   ./bayer_hostcheck          (minutes: a barrier of 256 threads is slow)
//   ./bayer_hostcheck quick   runs the three smallest sizes with one layout a case (seconds; tests/test_raw_abi.py builds and runs this form)
//
// A stand-alone program: it is not loaded into Python and does not touch a GPU.  Exit status 0 and "all N runs exact" when every run is byte-exact,
// every byte of the destination's pixels was written and nothing beside them.
#include "hostlanes.h"
#include "../autoencoder-fft_amd/csrc/bayer_kernels.hip"
#include "hostcheck_ref.h"

using namespace aefft;

// ---- include/aefft.h, restated -----------------------------------------------------------------
static const i64 FULLQ = 255LL << 16;
// [dy + 2][dx + 2], sixteenths
static const int F_G[5][5] = {{0, 0, -2, 0, 0}, {0, 0, 4, 0, 0}, {-2, 4, 8, 4, -2}, {0, 0, 4, 0, 0}, {0, 0, -2, 0, 0}};
static const int F_ROW[5][5] = {{0, 0, 1, 0, 0}, {0, -2, 0, -2, 0}, {-2, 8, 10, 8, -2}, {0, -2, 0, -2, 0}, {0, 0, 1, 0, 0}};
static const int F_DIAG[5][5] = {{0, 0, -3, 0, 0}, {0, 4, 0, 4, 0}, {-3, 0, 12, 0, -3}, {0, 4, 0, 4, 0}, {0, 0, -3, 0, 0}};
// the colour (0 R, 1 G, 2 B) at (x, y) of the four patterns: the name spells pixels (0,0), (1,0), (0,1), (1,1)
static int colour_at(int pattern, int x, int y)
{
    static const int T[4][4] = {{0, 1, 1, 2}, {1, 0, 2, 1}, {1, 2, 0, 1}, {2, 1, 1, 0}};
    return T[pattern][2 * (y & 1) + (x & 1)];
}
static int refl(int i, int n) { if (i < 0) i = -i; if (i >= n) i = 2 * (n - 1) - i; return i; }

struct Raw { const unsigned char* data; size_t pitch, stride; int container, bits, W, H; };
static i64 sample_ref(const Raw& s, int b, int x, int y)
{
    const unsigned char* row = s.data + b * s.stride + y * s.pitch;
    if (s.container == 0) return row[x];
    if (s.container == 1) return (row[2 * x] | row[2 * x + 1] << 8) & ((1 << s.bits) - 1);
    i64 v = 0;
    for (int k = 0; k < s.bits; ++k) {
        const int pos = x * s.bits + k;
        v |= (i64)((row[pos >> 3] >> (pos & 7)) & 1) << k;
    }
    return v;
}
// the pixels [B][H][W][D], tight
static void image_ref(const Raw& s, int pattern, int black, int white, const float* gain, int method, const float* ccm, const unsigned char* lut, int order, int B,
                      std::vector<unsigned char>& px)
{
    const int W = s.W, H = s.H, D = pattern == 4 ? 1 : 3;
    i64 m[3], cq[3][3];
    for (int c = 0; c < 3; ++c) m[c] = (i64)floor((double)gain[pattern == 4 ? 0 : c] * 255.0 * 65536.0 / (double)(white - black) + 0.5);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) cq[i][j] = ccm ? (i64)floor((double)ccm[3 * i + j] * 1024.0 + 0.5) : (i == j ? 1024 : 0);
    px.assign((size_t)B * H * W * D, 0);
    std::vector<i64> u((size_t)W * H);
    for (int b = 0; b < B; ++b) {
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                i64 sv = sample_ref(s, b, x, y) - black;
                if (sv < 0) sv = 0;
                const i64 t = sv * m[pattern == 4 ? 0 : colour_at(pattern, x, y)];
                u[(size_t)y * W + x] = t < FULLQ ? t : FULLQ;
            }
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                i64 o[3];
                if (pattern == 4) o[0] = 1024 * ((u[(size_t)y * W + x] + 128) >> 8);
                else {
                    const int here = colour_at(pattern, x, y);
                    i64 v[3];
                    for (int c = 0; c < 3; ++c) {
                        if (c == here) { v[c] = u[(size_t)y * W + x]; continue; }
                        // the filter that produces colour c at this site
                        const bool same_row = colour_at(pattern, x + 1, y) == c, same_col = colour_at(pattern, x, y + 1) == c;
                        i64 sum = 0;
                        for (int dy = -2; dy <= 2; ++dy)
                            for (int dx = -2; dx <= 2; ++dx) {
                                const i64 t = u[(size_t)refl(y + dy, H) * W + refl(x + dx, W)];
                                int k;
                                if (method == 1) k = c == 1 ? F_G[dy + 2][dx + 2] : same_row ? F_ROW[dy + 2][dx + 2] : same_col ? F_ROW[dx + 2][dy + 2] : F_DIAG[dy + 2][dx + 2];
                                else {
                                    const bool near = dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1;
                                    const bool cross = near && (dx == 0) != (dy == 0), dg = near && dx != 0 && dy != 0;
                                    k = c == 1 ? cross : same_row ? (near && dy == 0 && dx != 0) : same_col ? (near && dx == 0 && dy != 0) : dg;
                                }
                                sum += k * t;
                            }
                        if (method == 1) { sum = (sum + 8) >> 4; v[c] = sum < 0 ? 0 : sum > FULLQ ? FULLQ : sum; }
                        else v[c] = (c == 1 || (!same_row && !same_col)) ? (sum + 2) >> 2 : (sum + 1) >> 1;
                    }
                    for (int i = 0; i < 3; ++i) {
                        o[i] = 0;
                        for (int j = 0; j < 3; ++j) o[i] += cq[i][j] * ((v[j] + 128) >> 8);
                    }
                }
                for (int d = 0; d < D; ++d) {
                    const i64 oo = o[D == 1 ? 0 : order == 0 ? 2 - d : d];
                    i64 by;
                    if (lut) { i64 k = (oo + (1 << 13)) >> 14; by = lut[k < 0 ? 0 : k > 4080 ? 4080 : k]; }
                    else { by = (oo + (1 << 17)) >> 18; by = by < 0 ? 0 : by > 255 ? 255 : by; }
                    px[(((size_t)b * H + y) * W + x) * D + d] = (unsigned char)by;
                }
            }
    }
}

// ---- the bodies the launcher chooses between -----------------------------------------------------
typedef void (*bayer_fn)(const BaArgs&, unsigned*);
typedef void (*mono_fn)(const BaArgs&);
template <int C, int M> static void bbody(const BaArgs& a, unsigned* lds) { bayer_body<C, M>(a, lds); }
template <int C> static void mbody(const BaArgs& a) { mono_body<C>(a); }
static const bayer_fn BBODY[3][2] = {{bbody<0, 0>, bbody<0, 1>}, {bbody<1, 0>, bbody<1, 1>}, {bbody<2, 0>, bbody<2, 1>}};
static const mono_fn MBODY[3] = {mbody<0>, mbody<1>, mbody<2>};

struct Case { int B, W, H, pattern, container, bits, method, order, kind, ikind, black, white; float gain[3]; bool ccm, lut; unsigned grid_y; };

// kind 0 tight, 1 pitch rounded up to 64, 2 pitch + 5 (U16: + 6) from a base off by one byte (U16: two): the byte route; ikind: the image's layout alike.
// Every allocation ends with its last live byte
static void run(const Case& c)
{
    const int D = c.pattern == 4 ? 1 : 3;
    const size_t live = ba_row_bytes(c.container, c.bits, c.W);
    size_t pitch = live, off = 0;
    if (c.kind == 1) pitch = (pitch + 63) / 64 * 64;
    if (c.kind == 2) { pitch += c.container == 1 ? 6 : 5; off = c.container == 1 ? 2 : 1; }
    const size_t stride = c.H * pitch + (c.kind == 2 ? (c.container == 1 ? 6 : 7) : 16), sext = (size_t)(c.B - 1) * stride + (size_t)(c.H - 1) * pitch + live;
    void* sp = nullptr;
    if (posix_memalign(&sp, 16, off + sext)) abort();
    unsigned char* salloc = (unsigned char*)sp;
    for (size_t i = 0; i < off + sext; ++i) salloc[i] = (unsigned char)rnd();
    size_t ipitch = (size_t)c.W * D, ioff = 0;
    if (c.ikind == 1) ipitch = (ipitch + 63) / 64 * 64;
    if (c.ikind == 2) { ipitch += 5; ioff = 1; }
    const size_t istride = c.H * ipitch + (c.ikind == 2 ? 3 : 8), iext = (size_t)(c.B - 1) * istride + (size_t)(c.H - 1) * ipitch + (size_t)c.W * D;
    void* ip = nullptr;
    if (posix_memalign(&ip, 16, ioff + iext)) abort();
    unsigned char* ialloc = (unsigned char*)ip;
    memset(ialloc, 0xEE, ioff + iext);
    unsigned char* lut = nullptr;
    if (c.lut) {
        lut = (unsigned char*)malloc(4081);                                      // entries above 4080 are never read
        for (int k = 0; k <= 4080; ++k) lut[k] = (unsigned char)((k * 37 + (k >> 3)) & 255);
    }
    const float ccm[9] = {1.6f, -0.45f, -0.15f, -0.3f, 1.55f, -0.25f, 0.05f, -0.7f, 1.65f};
    const BaArgs g = ba_geometry(c.pattern, c.container, c.bits, c.W, c.H, salloc + off, pitch, stride, c.black, c.white, c.gain, c.ccm ? ccm : nullptr, lut, c.order,
                                 ialloc + ioff, ipitch, istride, c.B);
    const unsigned gy = c.grid_y ? c.grid_y : (unsigned)c.B;
    if (c.pattern == 4) { const mono_fn body = MBODY[c.container]; launch((unsigned)(g.gx * g.gy), gy, 1u, 0, [&](unsigned*) { body(g); }); }
    else { const bayer_fn body = BBODY[c.container][c.method]; launch((unsigned)(g.gx * g.gy), gy, 1u, BA_LDS_WORDS, [&](unsigned* lds) { body(g, lds); }); }
    const Raw raw = {salloc + off, pitch, stride, c.container, c.bits, c.W, c.H};
    std::vector<unsigned char> px;
    image_ref(raw, c.pattern, c.black, c.white, c.gain, c.method, c.ccm ? ccm : nullptr, lut, c.order, c.B, px);
    std::vector<unsigned char> want(ioff + iext, 0xEE);
    for (int b = 0; b < c.B; ++b)
        for (int y = 0; y < c.H; ++y) memcpy(&want[ioff + b * istride + y * ipitch], &px[((size_t)b * c.H + y) * c.W * D], (size_t)c.W * D);
    size_t bad = 0;
    for (size_t k = 0; k < ioff + iext; ++k) bad += ialloc[k] != want[k];
    ++runs;
    if (bad) {
        ++failures;
        printf("MISMATCH B=%d %dx%d pattern=%d container=%d bits=%d method=%d order=%d kind=%d ikind=%d black=%d white=%d ccm=%d lut=%d: %zu of %zu differ (words src=%d img=%d)\n",
               c.B, c.W, c.H, c.pattern, c.container, c.bits, c.method, c.order, c.kind, c.ikind, c.black, c.white, (int)c.ccm, (int)c.lut, bad, ioff + iext, (int)g.s.words,
               (int)g.img_words);
    }
    free(lut); free(ialloc); free(salloc);
}

int main(int argc, char** argv)
{
    const bool quick = argc > 1 && !strcmp(argv[1], "quick");
    // the device test's sizes and beyond: the smallest, odd ones, a tile and its halo plus two, several tiles with remainders, a row of 8192, a column of tiles
    const int shapes[][3] = {{1, 4, 4}, {2, 5, 7}, {1, 66, 18}, {3, 131, 37}, {1, 64, 16}, {1, 8192, 4}, {1, 6, 300}, {2, 257, 5}};
    const int conts[][2] = {{0, 8}, {1, 10}, {1, 12}, {1, 16}, {2, 10}, {2, 12}};
    int n = 0, cse = 0;
    for (const auto& s : shapes) {
        if (quick && &s - shapes >= 3) break;
        for (const auto& ct : conts)
            for (int pattern = 0; pattern < 5; ++pattern)
                for (int method = 0; method < 2; ++method) {
                    if (pattern == 4 && method == 0) continue;
                    const bool big = (size_t)s[0] * s[1] * s[2] > 20000;
                    ++cse;
                    for (int kind = 0; kind < 3; ++kind) {
                        if ((big || quick) && kind != cse % 3) continue;        // (one layout, all three over the cases)
                        ++n;
                        const int top = (1 << ct[1]) - 1;
                        // levels and gains in turn: the identity; a black level and a white below the top with gains that reach both clamps
                        Case c = {s[0], s[1], s[2], pattern, ct[0], ct[1], method, n & 1, kind, (kind + n) % 3, 0, top, {1.f, 1.f, 1.f}, false, false, 0u};
                        if (n % 3 == 1) { c.black = top / 16; c.white = top - top / 8; c.gain[0] = 1.9f; c.gain[1] = 1.f; c.gain[2] = 1.4f; }
                        if (n % 3 == 2) { c.black = top / 3; c.white = top / 3 + 3; c.gain[0] = 0.f; c.gain[1] = 64.f; c.gain[2] = 0.37f; }
                        c.ccm = n % 4 >= 2; c.lut = n % 5 >= 3;
                        run(c);
                    }
                }
    }
    // a folded grid: five images on two rows of workgroups
    for (int pattern = 0; pattern < 5; pattern += 4) run(Case{5, 70, 9, pattern, 2, 12, 1, 0, 2, 2, 100, 3000, {1.5f, 1.f, 1.25f}, true, true, 2u});
    return report();
}
