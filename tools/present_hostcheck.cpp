// aefft_frames_resize_to_image and aefft_map_overlay_image without a device: the kernel source itself --
// autoencoder-fft_amd/csrc/present_kernels.hip, both bodies and their launch geometry -- compiled for the HOST, 256 threads as the lanes of a
// workgroup and a barrier for __syncthreads, under the sanitizers, with the frame, map, table, image and LDS buffers allocated at exactly their
// live extent, against a scalar C restatement of include/aefft.h's formulas in 64-bit integers (which shares nothing with the kernel's taps).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Wno-unknown-pragmas
//       -o present_hostcheck tools/present_hostcheck.cpp   (one line),   then   ./present_hostcheck
//
// A stand-alone program: it is not loaded into Python and does not touch a GPU.  Exit status 0 and "all N runs exact" when every run is
// byte-exact on the live bytes of the image and every other byte of the image's allocation is as it was.
#include "hostlanes.h"
#include "../autoencoder-fft_amd/csrc/present_kernels.hip"
#include "hostcheck_ref.h"

using namespace aefft;

struct Layout { size_t pitch, stride, off, extent; };
// kind 0 tight, 1 pitch rounded up to 64, 2 pitch W D + 5 from a base off by one byte, 3 a region of interest at (3, 5) of a larger batch
static Layout layout(int kind, int B, int D, int W, int H)
{
    Layout l;
    l.pitch = (size_t)W * D; l.off = 0;
    if (kind == 1) l.pitch = (l.pitch + 63) / 64 * 64;
    if (kind == 2) { l.pitch += 5; l.off = 1; }
    l.stride = (size_t)H * l.pitch;
    if (kind == 3) { l.pitch = (size_t)(W + 9) * D; l.stride = (size_t)(H + 7) * l.pitch; l.off = 3 * l.pitch + 5 * D; }
    l.extent = (size_t)(B - 1) * l.stride + (size_t)(H - 1) * l.pitch + (size_t)W * D;   // the LAST byte the call may touch is at off + extent - 1
    return l;
}

// ---- frames -> image ----------------------------------------------------------------------------
typedef void (*fr_fn)(const FrArgs&, unsigned*);
template <int D, bool F32, int MODE> static void fr_body(const FrArgs& a, unsigned* lds) { frames_resize_body<D, F32, MODE>(a, lds); }
#define FR_ROW(D) {{fr_body<D, false, 0>, fr_body<D, false, 1>}, {fr_body<D, true, 0>, fr_body<D, true, 1>}}
static const fr_fn FR_BODIES[4][2][2] = {FR_ROW(1), FR_ROW(2), FR_ROW(3), FR_ROW(4)};

static const float SPECIAL[] = {NAN, INFINITY, -INFINITY, -3.f, 300.f, 0.5f, 1.5f, 254.5f, 0.49999997f, 255.5f, 2.5f};

struct Shape { int B, D, Nx, Ny, W, H; };
static void run_resize(const Shape& s, int kind, int mode, bool f32, unsigned grid_y = 0)
{
    const int B = s.B, D = s.D, Nx = s.Nx, Ny = s.Ny, W = s.W, H = s.H;
    const Layout l = layout(kind, B, D, W, H);
    std::vector<unsigned char> before(l.off + l.extent);
    for (auto& v : before) v = (unsigned char)rnd();
    unsigned char* alloc = (unsigned char*)malloc(l.off + l.extent);
    memcpy(alloc, before.data(), l.off + l.extent);
    const size_t n = (size_t)B * D * Nx * Ny, es = f32 ? 4 : 1;
    void* fp = nullptr;
    if (posix_memalign(&fp, 16, n * es)) abort();                                // 16-byte aligned, exactly n elements
    std::vector<unsigned char> px(n);
    for (size_t k = 0; k < n; ++k) {
        if (f32) {
            const float v = k % 7 == 3 ? SPECIAL[(k / 7) % (sizeof SPECIAL / sizeof *SPECIAL)] : (float)rnd() + (float)rnd() / 256.f - 0.25f;
            ((float*)fp)[k] = v; px[k] = (unsigned char)px_ref(v);
        } else ((unsigned char*)fp)[k] = px[k] = (unsigned char)rnd();
    }
    const FrArgs g = fr_geometry(fp, Nx, Ny, mode, alloc + l.off, l.pitch, l.stride, W, H, B, D);
    launch((unsigned)(g.tx * g.ty), grid_y ? grid_y : (unsigned)B, grid_y ? ((unsigned)B + grid_y - 1) / grid_y : 1u, (size_t)fr_lds_words(D, g), [&](unsigned* lds) { FR_BODIES[D - 1][f32][mode](g, lds); });
    // the expected image over a copy of the allocation as it was: every byte outside the live pixels must be unchanged
    frames_to_image_ref(px.data(), B, D, Nx, Ny, mode, W, H, before.data() + l.off, l.pitch, l.stride);
    const size_t bad = [&] { size_t c = 0; for (size_t k = 0; k < l.off + l.extent; ++k) c += before[k] != alloc[k]; return c; }();
    ++runs;
    if (bad) {
        ++failures;
        printf("RESIZE MISMATCH B=%d D=%d %dx%d -> %dx%d kind=%d mode=%d f32=%d: %zu bytes differ (words img=%d frm=%d TX=%d TY=%d P=%d XB=%d)\n", B, D, Nx, Ny, W, H, kind,
               mode, (int)f32, bad, (int)g.img_words, (int)g.frm_words, g.TX, g.TY, g.P, g.XB);
    }
    free(fp);
    free(alloc);
}

// ---- map -> image -------------------------------------------------------------------------------
typedef void (*ov_fn)(const OvArgs&, unsigned*);
template <int D> static void ov_body(const OvArgs& a, unsigned* lds) { map_overlay_body<D>(a, lds); }
static const ov_fn OV_BODIES[4] = {ov_body<1>, ov_body<2>, ov_body<3>, ov_body<4>};

struct MapShape { int B, D, Mx, My, W, H; };
static void run_overlay(const MapShape& s, int kind, int smooth, int alpha, float lo, float hi)
{
    const int B = s.B, D = s.D, Mx = s.Mx, My = s.My, W = s.W, H = s.H;
    const Layout l = layout(kind, B, D, W, H);
    std::vector<unsigned char> before(l.off + l.extent);
    for (auto& v : before) v = (unsigned char)rnd();
    unsigned char* alloc = (unsigned char*)malloc(l.off + l.extent);
    memcpy(alloc, before.data(), l.off + l.extent);
    unsigned char* lut = (unsigned char*)malloc(256 * D + 1) + 1;                 // (any alignment: off by one byte)
    for (int k = 0; k < 256 * D; ++k) lut[k] = (unsigned char)rnd();
    const size_t n = (size_t)B * Mx * My;
    void* mp = nullptr;
    if (posix_memalign(&mp, 16, n * 4)) abort();
    float* map = (float*)mp;
    const float inv = 255.0f / (hi - lo);
    std::vector<unsigned char> k0(n);
    for (size_t k = 0; k < n; ++k) {
        float v = lo + (hi - lo) * ((float)rnd() - 20.f) / 215.f;                  // below lo and above hi included
        if (k % 5 == 2) v = SPECIAL[(k / 5) % 3];
        if (k % 5 == 4) v = lo + ((float)(rnd() % 255) + 0.5f) / inv;             // on or next to a rounding half
        map[k] = v;
        volatile float t = v - lo;
        volatile float u = t * inv;
        k0[k] = (unsigned char)px_ref(u);
    }
    const OvArgs g = ov_geometry(map, Mx, My, lo, inv, smooth, lut, alpha, alloc + l.off, l.pitch, l.stride, W, H, B, D);
    launch((unsigned)(g.tx * g.ty), (unsigned)B, 1u, (size_t)ov_lds_words(D, g), [&](unsigned* lds) { OV_BODIES[D - 1](g, lds); });
    for (int b = 0; b < B; ++b)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const unsigned char* q = k0.data() + (size_t)b * Mx * My;
                unsigned k;
                if (!smooth) k = q[(size_t)((i64)x * Mx / W) * My + (i64)y * My / H];
                else {
                    int x0, x1, wx, y0, y1, wy;
                    linear_axis(x, Mx, W, &x0, &x1, &wx);
                    linear_axis(y, My, H, &y0, &y1, &wy);
                    const i64 v = (2048LL - wy) * ((2048LL - wx) * q[(size_t)x0 * My + y0] + (i64)wx * q[(size_t)x1 * My + y0]) +
                                  (i64)wy * ((2048LL - wx) * q[(size_t)x0 * My + y1] + (i64)wx * q[(size_t)x1 * My + y1]);
                    k = (unsigned)((v + (1LL << 21)) >> 22);
                }
                for (int d = 0; d < D; ++d) {
                    unsigned char& p = before[l.off + b * l.stride + y * l.pitch + (size_t)x * D + d];
                    p = (unsigned char)((alpha * lut[k * D + d] + (256 - alpha) * p + 128) >> 8);
                }
            }
    const size_t bad = [&] { size_t c = 0; for (size_t k = 0; k < l.off + l.extent; ++k) c += before[k] != alloc[k]; return c; }();
    ++runs;
    if (bad) {
        ++failures;
        printf("OVERLAY MISMATCH B=%d D=%d map %dx%d image %dx%d kind=%d smooth=%d alpha=%d lo=%g hi=%g: %zu bytes differ (words=%d TX=%d TY=%d NI=%d PJ=%d)\n", B, D, Mx, My, W,
               H, kind, smooth, alpha, lo, hi, bad, (int)g.img_words, g.TX, g.TY, g.NI, g.PJ);
    }
    free(mp);
    free(lut - 1);
    free(alloc);
}

int main(int argc, char** argv)
{
    const bool big = argc > 1 && !strcmp(argv[1], "--big");                      // also the two large shapes of the device tests (minutes under the sanitizers)
    std::vector<Shape> shapes = {{1, 1, 8, 8, 8, 8}, {2, 3, 8, 8, 11, 9}, {1, 3, 16, 8, 7, 5}, {2, 4, 64, 64, 32, 32}, {1, 3, 66, 34, 130, 70}, {1, 2, 200, 150, 10, 12},
                                 // beyond the device tests: one destination pixel, one source pixel, runs that need bands (down to one column per band), 2 -> 3
                                 {1, 1, 1, 1, 37, 29}, {1, 4, 5, 3, 1, 1}, {1, 4, 40, 2500, 4, 16}, {3, 2, 2, 2, 3, 3}, {1, 1, 3, 8192, 3, 2}, {1, 4, 2, 8192, 1, 1},
                                 {1, 3, 700, 36, 5, 9}};
    if (big) { shapes.push_back({2, 3, 256, 256, 640, 480}); shapes.push_back({1, 1, 8192, 2064, 8, 6}); }
    for (const Shape& s : shapes)
        for (int kind = 0; kind < 4; ++kind)
            for (int mode = 0; mode < 2; ++mode) {
                if (mode == 1 && (s.W > s.Nx || s.H > s.Ny)) continue;
                if (s.Nx * s.Ny > 4000000 && (mode == 0 || kind > 1)) continue;  // (the 64-bit sum: AREA, two layouts)
                for (int f32 = 0; f32 < 2; ++f32) run_resize(s, kind, mode, f32 != 0);
            }
    // the images on grid.y x grid.z: five images as 2 x 3, the sixth workgroup returns at once
    for (int mode = 0; mode < 2; ++mode) run_resize(Shape{5, 3, 9, 11, 8, 8}, 2, mode, false, 2);
    std::vector<MapShape> maps = {{1, 1, 1, 1, 8, 8}, {2, 3, 4, 4, 11, 9}, {1, 3, 8, 6, 130, 70}, {2, 4, 32, 32, 64, 64},
                                  // beyond the device tests: a map larger than the image, one pixel, a long thin map
                                  {1, 2, 100, 70, 9, 5}, {2, 3, 1024, 3, 1, 1}, {1, 1, 3, 1024, 5, 300}};
    if (big) maps.push_back({1, 3, 32, 32, 640, 480});
    const int alphas[] = {0, 1, 128, 255, 256};
    for (const MapShape& s : maps)
        for (int kind = 0; kind < 4; ++kind)
            for (int smooth = 0; smooth < 2; ++smooth) {
                const int a = alphas[(runs + kind) % 5];
                run_overlay(s, kind, smooth, a, 0.25f, 7.5f);
                run_overlay(s, kind, smooth, kind == 0 ? 256 : alphas[(runs + 2) % 5], 1.0f, -0.125f);   // hi < lo: the inverted scale
            }
    return report();
}
