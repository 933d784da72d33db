// aefft_frames_degrade without a device: the kernel source itself -- autoencoder-fft_amd/csrc/degrade_kernels.hip, both
// bodies and their launch geometry -- compiled for the HOST, 256 threads as the lanes of a workgroup and a barrier for __syncthreads, under the
// sanitizers, with the source, destination and LDS buffers allocated at exactly their live extent, against a scalar C restatement of
// include/aefft.h's formulas (its own Philox with the products split into halves, its own blur on 64-bit integers: it shares nothing with the
// kernel).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Wno-unknown-pragmas
//       -o degrade_hostcheck tools/degrade_hostcheck.cpp   (one line),   then   ./degrade_hostcheck
//
// A stand-alone program: it is not loaded into Python and does not touch a GPU.  Exit status 0 and "all N runs exact" when every run is
// bit-exact on every element of the destination.
#include "hostlanes.h"
static inline unsigned dg_bytesum(unsigned x, unsigned acc) { return acc + (x & 255u) + ((x >> 8) & 255u) + ((x >> 16) & 255u) + (x >> 24); }
#define DG_BYTESUM(x, acc) dg_bytesum((x), (acc))
#include "../autoencoder-fft_amd/csrc/degrade_kernels.hip"
#include "hostcheck_ref.h"

using namespace aefft;

// ---- the formulas of include/aefft.h, restated -------------------------------------------------
typedef unsigned long long u64;
static void ref_mulhilo(uint32_t a, uint32_t b, uint32_t* hi, uint32_t* lo)
{
    const uint32_t a0 = a & 0xffff, a1 = a >> 16, b0 = b & 0xffff, b1 = b >> 16;
    const uint32_t ll = a0 * b0, lh = a0 * b1, hl = a1 * b0, hh = a1 * b1;
    const uint32_t mid = (ll >> 16) + (lh & 0xffff) + (hl & 0xffff);
    *lo = (ll & 0xffff) | (mid << 16);
    *hi = hh + (lh >> 16) + (hl >> 16) + (mid >> 16);
}
static void ref_philox(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4])
{
    uint32_t c[4] = {ctr[0], ctr[1], ctr[2], ctr[3]}, k[2] = {key[0], key[1]};
    for (int r = 0; r < 10; ++r) {
        uint32_t hi0, lo0, hi1, lo1;
        ref_mulhilo(0xD2511F53u, c[0], &hi0, &lo0);
        ref_mulhilo(0xCD9E8D57u, c[2], &hi1, &lo1);
        const uint32_t n[4] = {hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0};
        memcpy(c, n, sizeof n);
        k[0] += 0x9E3779B9u; k[1] += 0xBB67AE85u;
    }
    memcpy(out, c, sizeof c);
}
static i64 binom(int n, int k) { i64 r = 1; for (int s = 1; s <= k; ++s) r = r * (n - k + s) / s; return r; }
static int clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

typedef void (*dg_fn)(const DgArgs&, unsigned*);
template <int R, bool SF32, bool DF32, bool WORDS> static void dg_body(const DgArgs& a, unsigned* lds)
{
    if constexpr (R == 0) degrade_flat_body<SF32, DF32, WORDS>(a);
    else degrade_tile_body<R, SF32, DF32, WORDS>(a, lds);
}
#define DG_ROW(R) {{{dg_body<R, false, false, false>, dg_body<R, false, false, true>}, {dg_body<R, false, true, false>, dg_body<R, false, true, true>}}, \
                   {{dg_body<R, true, false, false>, dg_body<R, true, false, true>}, {dg_body<R, true, true, false>, dg_body<R, true, true, true>}}}
static const dg_fn DG_BODIES[5][2][2][2] = {DG_ROW(0), DG_ROW(1), DG_ROW(2), DG_ROW(3), DG_ROW(4)};
static const int DG_LDS[5] = {dg_lds_words(0), dg_lds_words(1), dg_lds_words(2), dg_lds_words(3), dg_lds_words(4)};

static const float SPECIAL[] = {NAN, INFINITY, -INFINITY, -3.f, 300.f, 0.5f, 1.5f, 254.5f, 0.49999997f, 255.5f, 2.5f};

struct Shape { int B, D, Nx, Ny; };
static void run(const Shape& s, int R, float sigma, float impulse, bool sf32, bool df32, bool in_place, u64 seed, u64 first, unsigned grid_y = 0)
{
    const int B = s.B, D = s.D, Nx = s.Nx, Ny = s.Ny;
    const size_t P = (size_t)D * Nx * Ny, n = (size_t)B * P, ss = sf32 ? 4 : 1, ds = df32 ? 4 : 1;
    void *sp = nullptr, *dp = nullptr;
    if (posix_memalign(&sp, 16, n * ss)) abort();                                // 16-byte aligned, exactly n elements
    if (in_place) dp = sp;
    else if (posix_memalign(&dp, 16, n * ds)) abort();
    std::vector<unsigned char> px(n);
    for (size_t k = 0; k < n; ++k) {
        if (sf32) {
            const float v = k % 7 == 3 ? SPECIAL[(k / 7) % (sizeof SPECIAL / sizeof *SPECIAL)] : (float)rnd() + (float)rnd() / 256.f - 0.25f;
            ((float*)sp)[k] = v; px[k] = (unsigned char)px_ref(v);
        } else ((unsigned char*)sp)[k] = px[k] = (unsigned char)rnd();
    }
    if (!in_place) memset(dp, 0xEE, n * ds);
    const DgArgs g = dg_geometry(sp, dp, B, D, Nx, Ny, sigma, impulse, seed, first);
    const bool words = (Ny & 3) == 0;
    launch(dg_grid_x(R, g), grid_y ? grid_y : (unsigned)B, grid_y ? ((unsigned)B + grid_y - 1) / grid_y : 1u, (size_t)DG_LDS[R],
           [&](unsigned* lds) { DG_BODIES[R][sf32][df32][words](g, lds); });
    // the expected result, element by element
    const i64 m = (i64)floor(((double)sigma * 65536.0) / sqrt(32767.5) + 0.5), t = (i64)floor((double)impulse * 65536.0 + 0.5);
    if (m != g.m || t != g.t) { printf("QUANTISATION MISMATCH sigma=%g impulse=%g\n", sigma, impulse); ++failures; }
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    size_t bad = 0;
    for (int b = 0; b < B; ++b) {
        const u64 gf = first + (u64)b;
        for (int d = 0; d < D; ++d) {
            const unsigned char* p = px.data() + ((size_t)b * D + d) * Nx * Ny;
            for (int i = 0; i < Nx; ++i)
                for (int j = 0; j < Ny; ++j) {
                    i64 v = 0;
                    for (int l = 0; l <= 2 * R; ++l) {
                        i64 h = 0;
                        const int jj = clampi(j + l - R, Ny - 1);
                        for (int k = 0; k <= 2 * R; ++k) h += binom(2 * R, k) * p[(size_t)clampi(i + k - R, Nx - 1) * Ny + jj];
                        v += binom(2 * R, l) * h;
                    }
                    i64 u = v * (1LL << (16 - 4 * R));
                    const u64 nn = ((u64)d * Nx + i) * Ny + j;
                    const uint32_t ctr[4] = {(uint32_t)(nn >> 1), 0u, (uint32_t)gf, (uint32_t)(gf >> 32)};
                    uint32_t x[4];
                    ref_philox(ctr, key, x);
                    const uint32_t a = x[2 * (nn & 1)], c = x[2 * (nn & 1) + 1];
                    const i64 T = (i64)(a & 255) + ((a >> 8) & 255) + ((a >> 16) & 255) + (a >> 24) + (c & 255) + ((c >> 8) & 255) - 765;
                    u += T * m;
                    if ((i64)(c >> 16) < t) u = (a & 1) ? 255LL << 16 : 0;
                    const size_t o = (size_t)b * P + (size_t)nn;
                    if (df32) {
                        const float want = (float)(int32_t)u * (1.0f / 65536.0f), got = ((float*)dp)[o];
                        bad += memcmp(&want, &got, 4) != 0;
                    } else {
                        i64 q = (u + 32768) / 65536;                             // floor division for a negative u, without a shift
                        if ((u + 32768) % 65536 < 0) --q;
                        q = q < 0 ? 0 : q > 255 ? 255 : q;
                        bad += ((unsigned char*)dp)[o] != (unsigned char)q;
                    }
                }
        }
    }
    ++runs;
    if (bad) {
        ++failures;
        printf("MISMATCH B=%d D=%d %dx%d R=%d sigma=%g impulse=%g sf32=%d df32=%d in_place=%d: %zu elements differ\n", B, D, Nx, Ny, R, sigma, impulse, (int)sf32,
               (int)df32, (int)in_place, bad);
    }
    if (!in_place) free(dp);
    free(sp);
}

int main()
{
    // the three published known answers, on the kernel's own Philox and on the restatement's
    {
        const uint32_t KAT[3][10] = {
            {0, 0, 0, 0, 0, 0, 0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u},
            {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu},
            {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u, 0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}};
        for (const auto& k : KAT) {
            const DgWords w = dg_philox(k[0], k[1], k[2], k[3], k[4], k[5]);
            uint32_t x[4];
            ref_philox(k, k + 4, x);
            ++runs;
            if (w.x != k[6] || w.y != k[7] || w.z != k[8] || w.w != k[9] || memcmp(x, k + 6, 16)) { ++failures; printf("PHILOX known answer MISMATCH\n"); }
        }
    }
    const std::vector<Shape> shapes = {{1, 1, 8, 8}, {2, 3, 16, 12}, {1, 3, 10, 6}, {1, 2, 9, 7}, {1, 1, 1, 1}, {2, 4, 64, 64}, {1, 3, 130, 70},
                                       // beyond the device tests: one row, one column, a tile and one more either way, fewer than R rows
                                       {1, 1, 1, 200}, {1, 2, 200, 1}, {1, 1, 33, 65}, {2, 1, 3, 68}, {1, 4, 2, 3}};
    const float NOISE[5][2] = {{0.f, 0.f}, {1.5f, 0.f}, {25.f, 0.02f}, {255.f, 0.f}, {0.f, 1.f}};
    const u64 seed = 0x9e3779b97f4a7c15ULL, first = 0xffffffffULL;               // (B = 2: the carry into the counter's fourth word)
    int pick = 0;
    for (const Shape& s : shapes)
        for (int R = 0; R <= 4; ++R)
            for (int sf = 0; sf < 2; ++sf)
                for (int df = 0; df < 2; ++df) {
                    const float* nz = NOISE[pick++ % 5];
                    run(s, R, nz[0], nz[1], sf != 0, df != 0, false, seed, first);
                    if (R == 0 && sf == df) run(s, 0, NOISE[2][0], NOISE[2][1], sf != 0, df != 0, true, seed + 1, first);
                }
    // every noise setting on both routes of both kernels
    for (const auto& nz : NOISE)
        for (int R = 0; R <= 4; R += 2) {
            run(Shape{2, 3, 16, 12}, R, nz[0], nz[1], false, false, false, 7, 0);
            run(Shape{1, 2, 9, 7}, R, nz[0], nz[1], true, true, false, 7, ~0ULL);          // (the largest frame number)
        }
    // the frames on grid.y x grid.z: five frames as 2 x 3, the sixth workgroup returns at once
    for (int R = 0; R <= 1; ++R) run(Shape{5, 3, 9, 11}, R, 25.f, 0.02f, false, false, false, 3, ~0ULL - 1, 2);
    return report();
}
