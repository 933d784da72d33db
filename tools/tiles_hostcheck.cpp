// aefft_image_tiles_to_frames / aefft_frames_tiles_to_image without a device: the kernel source itself --
// autoencoder-fft_amd/csrc/tile_kernels.hip, both bodies, the plan and the launch geometry -- compiled for the HOST, 256 threads as the lanes of a
// workgroup and a barrier for __syncthreads, under the sanitizers, with the image, frame and LDS buffers allocated at exactly their live extent,
// against a plain C++ restatement of include/aefft.h's formulas (its own plan, its own reflection, the weights of EVERY tile summed per pixel in
// 64 bits and a real division: it shares nothing with the kernel).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Wno-unknown-pragmas
//       -o tiles_hostcheck tools/tiles_hostcheck.cpp   (one line),   then   ./tiles_hostcheck
//
// A stand-alone program: it is not loaded into Python and does not touch a GPU.  Exit status 0 and "all N runs exact" when every run is
// bit-exact on every byte of the destination, the bytes around it included.
#include "../include/aefft.h"
#include "hostlanes.h"
#include "../autoencoder-fft_amd/csrc/tile_kernels.hip"
#include "hostcheck_ref.h"

using namespace aefft;

// ---- the formulas of include/aefft.h, restated -------------------------------------------------
struct RefAxis { int W, N, V, M, S, R, n, o0; i64 den; };
static bool ref_axis(int W, int N, int V, int M, RefAxis* a)
{
    if (W < 1 || W > 8192 || N < 2 || N > 2048 || V < 0 || 2 * V > N || M < 0 || 2 * M > V) return false;
    a->W = W; a->N = N; a->V = V; a->M = M; a->S = N - V; a->R = V - 2 * M;
    const double c = ceil((double)(W - N + 2 * M) / (double)a->S);
    a->n = (int)c + 1 < 1 ? 1 : (int)c + 1;
    const int E = (a->n - 1) * a->S + N - 2 * M - W;
    a->o0 = -M - (int)floor(E / 2.0);
    a->den = a->R > 0 ? 2 * a->R : 1;
    return E >= 0;
}
static int ref_reflect(i64 x, int W)
{
    if (W == 1) return 0;
    const i64 P = 2 * (W - 1);
    const i64 m = ((x % P) + P) % P;
    return (int)(m < W ? m : P - m);
}
static i64 ref_weight(const RefAxis& a, int t, int x)
{
    const int k = x - (a.o0 + t * a.S);
    if (k < a.M || k >= a.N - a.M) return 0;
    if (t > 0 && k < a.M + a.R) return 2 * (k - a.M) + 1;
    if (t < a.n - 1 && k >= a.N - a.M - a.R) return 2 * (a.N - a.M - 1 - k) + 1;
    return a.den;
}

// ---- the units on grid.y x grid.z as the kernels take them: a workgroup past the last unit returns at once ----
template <class K> static void launch_units(const TlArgs& g, unsigned fold, size_t lds_words, K kernel)
{
    launch(g.bx * g.by, fold ? fold : tl_grid_y(g), fold ? (g.units + fold - 1) / fold : tl_grid_z(g), lds_words, [&](unsigned* lds) {
        const unsigned u = blockIdx.z * gridDim.y + blockIdx.y;
        if (u < g.units) kernel(g, blockIdx.x, u, lds);
    });
}

typedef void (*tl_fn)(const TlArgs&, unsigned, unsigned, unsigned*);
#define TL_ROW(K) {{K<1, false>, K<1, true>}, {K<2, false>, K<2, true>}, {K<3, false>, K<3, true>}, {K<4, false>, K<4, true>}}
static const tl_fn GATHER[4][2] = TL_ROW(tile_gather_body);
static const tl_fn BLEND[4][2] = TL_ROW(tile_blend_body);
static const size_t LDS_WORDS[4] = {TlLds<1>::TOTAL, TlLds<2>::TOTAL, TlLds<3>::TOTAL, TlLds<4>::TOTAL};

static const float SPECIAL[] = {NAN, INFINITY, -INFINITY, -3.f, 300.f, 0.5f, 1.5f, 254.5f, 0.49999997f, 255.5f, 2.5f};

struct Case { int W, H, Nx, Ny, Vx, Vy, Mx, My; };
// an image buffer of exactly the live extent behind `skew` bytes (skew 0: the dword route when pitch and stride allow; 1: the byte route)
struct Image {
    size_t pitch, stride, extent; unsigned char *base, *p;
    Image(int W, int H, int D, int B, size_t pad, size_t gap, size_t skew)
    {
        pitch = (size_t)W * D + pad; stride = (size_t)(H - 1) * pitch + (size_t)W * D + gap;
        extent = (size_t)(B - 1) * stride + (size_t)(H - 1) * pitch + (size_t)W * D;
        void* q = nullptr;
        if (posix_memalign(&q, 16, skew + extent)) abort();
        base = (unsigned char*)q; p = base + skew;                               // the live extent ends at the allocation's end
    }
    ~Image() { free(base); }
};

// layout 0: image, pitch and stride multiples of 4, as tight as that allows (the dword route; a dword may cross the row's end); 1: the same with
// a wider pad; 2: an odd pitch; 3: layout 0 behind a skewed pointer (2 and 3: the byte route)
static void run(const Case& c, int D, int B, bool f32, int layout, unsigned fold)
{
    const size_t fill = (size_t)(-c.W * D) & 3u, pad = layout == 1 ? fill + 4 : layout == 2 ? 1 + ((c.W * D) & 1) : fill, gap = layout == 1 ? fill + 8 : layout == 2 ? 5 : fill,
                 skew = layout == 3 ? 1 : 0;
    aefft_tile_desc desc = {c.W, c.H, c.Nx, c.Ny, c.Vx, c.Vy, c.Mx, c.My};
    aefft_tile_plan plan;
    RefAxis ax, ay;
    ++runs;
    if (!ref_axis(c.W, c.Nx, c.Vx, c.Mx, &ax) || !ref_axis(c.H, c.Ny, c.Vy, c.My, &ay) || !tile_plan(&desc, &plan)) { ++failures; printf("PLAN REFUSED\n"); return; }
    if (plan.ntx != ax.n || plan.nty != ay.n || plan.ox0 != ax.o0 || plan.oy0 != ay.o0 || plan.step_x != ax.S || plan.step_y != ay.S || plan.ramp_x != ax.R ||
        plan.ramp_y != ay.R) { ++failures; printf("PLAN MISMATCH W=%d H=%d\n", c.W, c.H); return; }
    // the weights: their sum, the two-tile bound and the cover
    for (int axis = 0; axis < 2; ++axis) {
        const RefAxis& a = axis ? ay : ax;
        for (int x = 0; x < a.W; ++x) {
            i64 sum = 0; int nz = 0;
            for (int t = 0; t < a.n; ++t) { const i64 w = ref_weight(a, t, x); sum += w; nz += w != 0; }
            if (sum != a.den || nz < 1 || nz > 2) { ++failures; printf("WEIGHTS W=%d N=%d V=%d M=%d x=%d: sum %lld over %d tiles\n", a.W, a.N, a.V, a.M, x, sum, nz); return; }
        }
    }
    const size_t T = (size_t)B * ax.n * ay.n, P = (size_t)D * c.Nx * c.Ny, es = f32 ? 4 : 1;
    Image src(c.W, c.H, D, B, pad, gap, skew), dst(c.W, c.H, D, B, pad, gap, skew);
    for (size_t k = 0; k < src.extent; ++k) src.p[k] = (unsigned char)rnd();
    void* fr = nullptr;
    if (posix_memalign(&fr, 16, T * P * es)) abort();                             // 16-byte aligned, exactly T frames
    memset(fr, 0xEE, T * P * es);
    TlArgs g;
    size_t bad = 0;
    // gather
    if (!tl_geometry(&desc, src.p, src.pitch, src.stride, fr, B, false, &g)) abort();
    launch_units(g, fold, LDS_WORDS[D - 1], GATHER[D - 1][f32]);
    for (size_t f = 0; f < T; ++f) {
        const int tx = (int)(f % ax.n), ty = (int)(f / ax.n % ay.n);
        const size_t b = f / ax.n / ay.n;
        for (int d = 0; d < D; ++d)
            for (int i = 0; i < c.Nx; ++i)
                for (int j = 0; j < c.Ny; ++j) {
                    const int x = ref_reflect((i64)ax.o0 + (i64)tx * ax.S + i, c.W), y = ref_reflect((i64)ay.o0 + (i64)ty * ay.S + j, c.H);
                    const unsigned char want = src.p[b * src.stride + (size_t)y * src.pitch + (size_t)x * D + d];
                    const size_t o = f * P + ((size_t)d * c.Nx + i) * c.Ny + j;
                    bad += f32 ? ((float*)fr)[o] != (float)want : ((unsigned char*)fr)[o] != want;
                }
    }
    // blend(gather) is the image, pad bytes untouched
    std::vector<unsigned char> before(dst.extent);
    for (size_t k = 0; k < dst.extent; ++k) before[k] = dst.p[k] = (unsigned char)rnd();
    if (!tl_geometry(&desc, dst.p, dst.pitch, dst.stride, fr, B, true, &g)) abort();
    launch_units(g, fold, LDS_WORDS[D - 1], BLEND[D - 1][f32]);
    for (size_t k = 0; k < dst.extent; ++k) {
        const size_t in = k % dst.stride, col = in % dst.pitch;
        const bool live = in < (size_t)(c.H - 1) * dst.pitch + (size_t)c.W * D && col < (size_t)c.W * D;
        bad += dst.p[k] != (live ? src.p[k] : before[k]);
    }
    // blend of random tiles (float: special values too) against the sum over EVERY tile
    std::vector<unsigned char> px(T * P);
    for (size_t k = 0; k < T * P; ++k) {
        if (f32) {
            const float v = k % 7 == 3 ? SPECIAL[(k / 7) % (sizeof SPECIAL / sizeof *SPECIAL)] : (float)rnd() + (float)rnd() / 256.f - 0.25f;
            ((float*)fr)[k] = v; px[k] = (unsigned char)px_ref(v);
        } else ((unsigned char*)fr)[k] = px[k] = (unsigned char)rnd();
    }
    for (size_t k = 0; k < dst.extent; ++k) before[k] = dst.p[k] = (unsigned char)rnd();
    launch_units(g, fold, LDS_WORDS[D - 1], BLEND[D - 1][f32]);
    std::vector<unsigned char> want(before);
    const i64 dd = ax.den * ay.den;
    for (int b = 0; b < B; ++b)
        for (int y = 0; y < c.H; ++y)
            for (int x = 0; x < c.W; ++x)
                for (int d = 0; d < D; ++d) {
                    i64 acc = 0;
                    for (int ty = 0; ty < ay.n; ++ty)
                        for (int tx = 0; tx < ax.n; ++tx) {
                            const i64 w = ref_weight(ax, tx, x) * ref_weight(ay, ty, y);
                            if (!w) continue;
                            const size_t f = ((size_t)b * ay.n + ty) * ax.n + tx;
                            acc += w * px[f * P + ((size_t)d * c.Nx + (x - ax.o0 - tx * ax.S)) * c.Ny + (y - ay.o0 - ty * ay.S)];
                        }
                    want[(size_t)b * dst.stride + (size_t)y * dst.pitch + (size_t)x * D + d] = (unsigned char)((2 * acc + dd) / (2 * dd));
                }
    for (size_t k = 0; k < dst.extent; ++k) bad += dst.p[k] != want[k];
    if (bad) {
        ++failures;
        printf("MISMATCH W=%d H=%d N=%dx%d V=%d,%d M=%d,%d D=%d B=%d f32=%d pad=%zu gap=%zu skew=%zu: %zu bytes differ\n", c.W, c.H, c.Nx, c.Ny, c.Vx, c.Vy, c.Mx,
               c.My, D, B, (int)f32, pad, gap, skew, bad);
    }
    free(fr);
}

int main()
{
    // the multiply-shift division against the real one: every den product of small ramps and the largest, n over its whole range
    for (unsigned dx = 1; dx <= 2048; dx = dx < 64 ? dx + 1 : dx * 2)
        for (unsigned dy : {1u, 2u, 3u, 4u, 5u, 6u, 7u, 8u, 34u, 138u, 554u, 2048u}) {
            const unsigned dv = 2 * dx * dy;
            unsigned long long mul; int shift;
            tl_magic(dv, &mul, &shift);
            ++runs;
            bool ok = true;
            for (unsigned p = 0; p <= 255 && ok; ++p) {
                const unsigned lo = 2 * p * dx * dy + dx * dy;                   // acc = p dd, and its neighbours on either side of a multiple of dv
                for (unsigned n : {lo, lo - (lo % dv), lo - (lo % dv) + dv - 1, lo + dv - 1 - (lo % dv) + 1, 511u * dx * dy}) ok = ok && tl_div(n, mul, shift) == n / dv;
            }
            for (int k = 0; k < 2000 && ok; ++k) {
                const unsigned n = (rnd() << 24 | rnd() << 16 | rnd() << 8 | rnd()) & 0x7fffffffu;
                ok = tl_div(n, mul, shift) == n / dv;
            }
            if (!ok) { ++failures; printf("DIVISION MISMATCH dv=%u\n", dv); }
        }
    const std::vector<Case> cases = {{13, 9, 8, 8, 4, 4, 1, 1}, {5, 3, 8, 8, 4, 4, 1, 1}, {9, 9, 8, 8, 4, 4, 2, 2}, {16, 8, 8, 8, 0, 0, 0, 0}, {8, 8, 8, 8, 0, 0, 0, 0},
                                     {37, 29, 16, 8, 6, 4, 1, 2}, {23, 17, 10, 6, 4, 3, 1, 1}, {130, 70, 32, 32, 8, 8, 2, 2}, {1, 1, 2, 2, 0, 0, 0, 0},
                                     // beyond the device tests: blocks of 64 and one more either way, a tile larger than the block in one axis, the largest overlap, a long reflection
                                     {200, 3, 68, 4, 34, 2, 17, 1}, {3, 150, 4, 132, 1, 66, 0, 0}, {70, 66, 65, 63, 3, 31, 1, 15}, {2, 2, 64, 64, 32, 32, 16, 16},
                                     {131, 67, 128, 64, 5, 3, 2, 1}};
    int pick = 0;
    for (const Case& c : cases)
        for (int D = 1; D <= 4; ++D)
            for (int f32 = 0; f32 < 2; ++f32) {
                const int v = pick++ % 4;
                run(c, D, 1 + (v & 1), f32 != 0, v, 0);
                if (v >= 2) run(c, D, 2 - (v & 1), f32 != 0, v - 2, 0);           // (every shape, D and element type on the dword route too)
            }
    // each layout on one shape, and the units on a grid.y of three
    for (int v = 0; v < 4; ++v) run(cases[0], 3, 2, false, v, v == 0 ? 3 : 0);
    for (int v = 0; v < 4; ++v) run(cases[7], 3, 2, v & 1, v, v == 0 ? 3 : 0);
    return report();
}
