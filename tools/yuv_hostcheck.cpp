// aefft_yuv_to_image and aefft_yuv_resize_to_frames without a device: the kernel source itself --
// autoencoder-fft_amd/csrc/yuv_kernels.hip, both bodies and both launch geometries -- compiled for the HOST, 256 threads as the lanes of a workgroup
// and a barrier for __syncthreads, under the sanitizers, with every source plane, the image, the frames and the LDS allocated at exactly their
// live extent, against a scalar C restatement of include/aefft.h in 64-bit integers (its own coefficient table, its own chroma gather, and
// hostcheck_ref.h's resize: it shares nothing with the kernel, resize_taps.h and resize_tile.h included).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Wno-unknown-pragmas
//       -o yuv_hostcheck tools/yuv_hostcheck.cpp   (one line),   then   ./yuv_hostcheck
//
// A stand-alone program: it is not loaded into Python and does not touch a GPU.  Exit status 0 and "all N runs exact" when every run is
// byte-exact (float frames compared as bits) and every byte/element of the destination was written, and nothing beside it.
#include "hostlanes.h"
#include "../autoencoder-fft_amd/csrc/yuv_kernels.hip"
#include "hostcheck_ref.h"

using namespace aefft;

// ---- include/aefft.h, restated -----------------------------------------------------------------
// rows R, G, B: (a, b); then yoff, ky
static const i64 TABLE[3][8] = {{0, 1673555, -410793, -852458, 2115221, 0, 16, 1220945},
                                {0, 1879825, -223607, -558796, 2215014, 0, 16, 1220945},
                                {0, 1470104, -360853, -748826, 1858077, 0, 0, 1048576}};
struct Planes { const unsigned char* p[3]; size_t pitch[3], stride[3]; };
// the pixels p[b][y][x][d], tight
static void convert_ref(int fmt, const Planes& s, int W, int H, int matrix, int order, int B, std::vector<unsigned char>& px)
{
    const int D = order == 2 ? 1 : 3;
    px.assign((size_t)B * H * W * D, 0);
    for (int b = 0; b < B; ++b)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                i64 Y, U = 128, V = 128;
                if (fmt == 2) {
                    const unsigned char* r = s.p[0] + b * s.stride[0] + y * s.pitch[0];
                    Y = r[2 * x]; U = r[4 * (x / 2) + 1]; V = r[4 * (x / 2) + 3];
                } else {
                    Y = s.p[0][b * s.stride[0] + y * s.pitch[0] + x];
                    if (order != 2 && fmt == 0) { const unsigned char* r = s.p[1] + b * s.stride[1] + (y / 2) * s.pitch[1]; U = r[2 * (x / 2)]; V = r[2 * (x / 2) + 1]; }
                    if (order != 2 && fmt == 1) { U = s.p[1][b * s.stride[1] + (y / 2) * s.pitch[1] + x / 2]; V = s.p[2][b * s.stride[2] + (y / 2) * s.pitch[2] + x / 2]; }
                }
                const i64* T = TABLE[matrix];
                for (int d = 0; d < D; ++d) {
                    const int ch = order == 0 ? 2 - d : d;                       // BGR: (B, G, R) at d = 0, 1, 2
                    i64 v = T[7] * (Y - T[6]) + (order == 2 ? 0 : T[2 * ch] * (U - 128) + T[2 * ch + 1] * (V - 128));
                    v = fdiv(v + (1LL << 19), 1LL << 20);
                    px[(((size_t)b * H + y) * W + x) * D + d] = (unsigned char)(v < 0 ? 0 : v > 255 ? 255 : v);
                }
            }
}
// ---- the bodies the launchers choose between ---------------------------------------------------
typedef void (*resize_fn)(const YvArgs&, unsigned*);
typedef void (*image_fn)(const YiArgs&);
template <int F, int D> static void ibody(const YiArgs& a) { yuv_image_body<F, D>(a); }
template <int F, int D, bool T, int M> static void rbody(const YvArgs& a, unsigned* lds) { yuv_body<F, D, T, M>(a, lds); }
#define RROW(F, D) {{rbody<F, D, false, 0>, rbody<F, D, false, 1>}, {rbody<F, D, true, 0>, rbody<F, D, true, 1>}}
// [format][D == 3][f32][mode]; GRAY reads the luma plane only, which NV12 and I420 lay out alike: the launcher sends I420 GRAY to the NV12 kernels
static const resize_fn RBODY[3][2][2][2] = {{RROW(0, 1), RROW(0, 3)}, {RROW(0, 1), RROW(1, 3)}, {RROW(2, 1), RROW(2, 3)}};
static const image_fn IBODY[3][2] = {{ibody<0, 1>, ibody<0, 3>}, {ibody<0, 1>, ibody<1, 3>}, {ibody<2, 1>, ibody<2, 3>}};


// the source planes of a run, each in an allocation of its own that ends with the plane's last live byte
struct Source {
    Planes pl; std::vector<unsigned char*> allocs;
    ~Source() { for (unsigned char* a : allocs) free(a); }
};
// kind 0 tight, 1 pitch rounded up to 64, 2 pitch + 5 from a base off by one byte (the byte route); B > 1: a batch stride that is not the plane's size
static void make_source(Source& s, int fmt, int W, int H, int order, int B, int kind)
{
    const size_t Wc = (W + 1) / 2, Hc = (H + 1) / 2;
    const size_t live[3] = {fmt == 2 ? 2 * (size_t)W : (size_t)W, fmt == 0 ? 2 * Wc : Wc, Wc}, rows[3] = {(size_t)H, Hc, Hc};
    const int used = order == 2 || fmt == 2 ? 1 : (fmt == 0 ? 2 : 3);
    for (int k = 0; k < 3; ++k) {
        s.pl.p[k] = nullptr; s.pl.pitch[k] = s.pl.stride[k] = 0;
        if (k >= used) continue;
        size_t pitch = live[k], off = 0;
        if (kind == 1) pitch = (pitch + 63) / 64 * 64;
        if (kind == 2) { pitch += 5; off = 1; }
        const size_t stride = rows[k] * pitch + (kind == 2 ? 7 : 16);
        const size_t extent = (size_t)(B - 1) * stride + (rows[k] - 1) * pitch + live[k];
        unsigned char* a = (unsigned char*)malloc(off + extent);
        for (size_t i = 0; i < off + extent; ++i) a[i] = (unsigned char)rnd();
        s.allocs.push_back(a);
        s.pl.p[k] = a + off; s.pl.pitch[k] = pitch; s.pl.stride[k] = stride;
    }
}

struct Shape { int B, W, H, Nx, Ny; };

static void run_resize(const Shape& sh, int fmt, int matrix, int order, int kind, int mode, bool f32, unsigned grid_y = 0)
{
    const int B = sh.B, W = sh.W, H = sh.H, Nx = sh.Nx, Ny = sh.Ny, D = order == 2 ? 1 : 3;
    Source src;
    make_source(src, fmt, W, H, order, B, kind);
    const size_t n = (size_t)B * D * Nx * Ny, es = f32 ? 4 : 1;
    void* fp = nullptr;
    if (posix_memalign(&fp, 16, n * es)) abort();                                // 16-byte aligned, exactly n elements
    unsigned char* frames = (unsigned char*)fp;
    memset(frames, 0xEE, n * es);
    const YvArgs g = yv_geometry(yv_source(fmt, src.pl.p, src.pl.pitch, src.pl.stride, W, H, matrix, order, B), mode, frames, B, D, Nx, Ny);
    const resize_fn body = RBODY[fmt][D == 3][f32][mode];
    launch((unsigned)(g.tx * g.ty), grid_y ? grid_y : (unsigned)B, 1u, (size_t)yv_lds_words(D, g.P, g.RB), [&](unsigned* lds) { body(g, lds); });
    std::vector<unsigned char> px;
    std::vector<unsigned> want;
    convert_ref(fmt, src.pl, W, H, matrix, order, B, px);
    image_to_frames_ref(px.data(), (size_t)W * D, (size_t)W * D * H, W, H, mode, f32, B, D, Nx, Ny, want);   // (from the tight pixels)
    size_t bad = 0;
    for (size_t k = 0; k < n; ++k) {
        if (f32) {
            const float w = (float)want[k] * (1.0f / 65536.0f);
            bad += memcmp(&w, frames + 4 * k, 4) != 0;
        } else bad += frames[k] != (unsigned char)want[k];
    }
    ++runs;
    if (bad) {
        ++failures;
        printf("MISMATCH resize B=%d %dx%d -> %dx%d fmt=%d matrix=%d order=%d kind=%d mode=%d f32=%d: %zu of %zu differ (words=%d P=%d RB=%d lw=%d)\n", B, W, H, Nx, Ny, fmt,
               matrix, order, kind, mode, (int)f32, bad, n, (int)g.s.words, g.P, g.RB, g.lw);
    }
    free(frames);
}

// ikind: the image's layout, as kind; the image allocation ends with its last live byte, pad bytes must stay as they were
static void run_image(int B, int W, int H, int fmt, int matrix, int order, int kind, int ikind, unsigned grid_y = 0)
{
    const int D = order == 2 ? 1 : 3;
    Source src;
    make_source(src, fmt, W, H, order, B, kind);
    size_t pitch = (size_t)W * D, off = 0;
    if (ikind == 1) pitch = (pitch + 63) / 64 * 64;
    if (ikind == 2) { pitch += 5; off = 1; }
    const size_t stride = H * pitch + (ikind == 2 ? 3 : 8), extent = (size_t)(B - 1) * stride + (size_t)(H - 1) * pitch + (size_t)W * D;
    unsigned char* alloc = (unsigned char*)malloc(off + extent);
    memset(alloc, 0xEE, off + extent);
    unsigned char* image = alloc + off;
    const YiArgs g = yi_geometry(yv_source(fmt, src.pl.p, src.pl.pitch, src.pl.stride, W, H, matrix, order, B), fmt, image, pitch, stride, B);
    const image_fn body = IBODY[fmt][D == 3];
    launch((unsigned)(g.gx * g.gy), grid_y ? grid_y : (unsigned)B, 1u, 0, [&](unsigned*) { body(g); });
    std::vector<unsigned char> px;
    convert_ref(fmt, src.pl, W, H, matrix, order, B, px);
    std::vector<unsigned char> want(off + extent, 0xEE);
    for (int b = 0; b < B; ++b)
        for (int y = 0; y < H; ++y) memcpy(&want[off + b * stride + y * pitch], &px[((size_t)b * H + y) * W * D], (size_t)W * D);
    size_t bad = 0;
    for (size_t k = 0; k < off + extent; ++k) bad += alloc[k] != want[k];
    ++runs;
    if (bad) {
        ++failures;
        printf("MISMATCH image B=%d %dx%d fmt=%d matrix=%d order=%d kind=%d ikind=%d: %zu of %zu differ (words src=%d img=%d)\n", B, W, H, fmt, matrix, order, kind, ikind, bad,
               off + extent, (int)g.s.words, (int)g.img_words);
    }
    free(alloc);
}

int main()
{
    // the conversion: every (Y, U, V) of a sparse lattice plus the extremes through the kernel's yv_convert against the table above, every matrix and order
    for (int matrix = 0; matrix < 3; ++matrix)
        for (int order = 0; order < 3; ++order) {
            const YvCoef k = yv_coef(matrix, order);
            const int D = order == 2 ? 1 : 3;
            size_t bad = 0;
            for (int Y = 0; Y < 256; Y += (Y < 20 || Y > 230) ? 1 : 5)
                for (int U = 0; U < 256; U += (U < 3 || U > 251) ? 1 : 7)
                    for (int V = 0; V < 256; V += (V < 3 || V > 251) ? 1 : 7) {
                        YvItem it = {{(unsigned)Y * 0x01010101u, 0u}, (unsigned)(U | V << 8) * 0x00010001u, 0u};
                        unsigned out[3] = {0, 0, 0};
                        if (D == 3) yv_convert<YV_NV12, 3>(k, it, 0, out); else yv_convert<YV_NV12, 1>(k, it, 0, out);
                        for (int d = 0; d < D; ++d) {
                            const int ch = order == 0 ? 2 - d : d;
                            i64 v = TABLE[matrix][7] * (Y - TABLE[matrix][6]) + (order == 2 ? 0 : TABLE[matrix][2 * ch] * (U - 128) + TABLE[matrix][2 * ch + 1] * (V - 128));
                            v = fdiv(v + (1LL << 19), 1LL << 20);
                            v = v < 0 ? 0 : v > 255 ? 255 : v;
                            bad += ((out[d >> 2] >> (8 * (d & 3))) & 255u) != (unsigned)v;
                        }
                    }
            ++runs;
            if (bad) { ++failures; printf("MISMATCH convert matrix=%d order=%d: %zu\n", matrix, order, bad); }
        }
    // yuv -> image: the device test's shapes and beyond (one pixel, one pair, a row of 8192, one column), every format, source and image layout
    const int ishapes[][3] = {{1, 8, 8}, {2, 11, 9}, {2, 12, 9}, {1, 130, 70}, {1, 1, 1}, {1, 2, 1}, {3, 5, 2}, {1, 8192, 2}, {1, 2, 300}, {2, 257, 3}};
    for (const auto& s : ishapes)
        for (int fmt = 0; fmt < 3; ++fmt) {
            if (fmt == 2 && (s[1] & 1)) continue;
            for (int kind = 0; kind < 3; ++kind)
                for (int ikind = 0; ikind < 3; ++ikind) run_image(s[0], s[1], s[2], fmt, (kind + ikind) % 3, 0, kind, ikind);
            run_image(s[0], s[1], s[2], fmt, 0, 1, 0, 0);
            for (int kind = 0; kind < 3; kind += 2) run_image(s[0], s[1], s[2], fmt, 1, 2, kind, kind);
        }
    for (int fmt = 0; fmt < 3; ++fmt) run_image(5, 12, 9, fmt, 0, 0, 2, 2, 2);       // a folded grid: five images on two rows of workgroups
    // yuv -> frames: the device test's shapes and beyond (one destination pixel, one source pixel / pair, rows so wide that a band is a few rows,
    // more than 256 groups of 4 pixels in a tile's footprint)
    const Shape shapes[] = {{1, 8, 8, 8, 8}, {2, 11, 9, 8, 8}, {1, 6, 4, 16, 8}, {2, 64, 64, 32, 32}, {1, 130, 70, 66, 34}, {1, 200, 150, 10, 12},
                            {2, 640, 480, 256, 256}, {1, 1920, 1080, 64, 64},
                            {1, 37, 29, 1, 1}, {1, 1, 1, 5, 3}, {1, 2, 1, 5, 3}, {1, 2500, 40, 16, 4}, {3, 3, 3, 2, 2}, {1, 8192, 3, 2, 3}, {1, 8192, 2, 1, 1}};
    for (const Shape& s : shapes)
        for (int fmt = 0; fmt < 3; ++fmt) {
            if (fmt == 2 && (s.W & 1)) continue;
            const bool big = (size_t)s.W * s.H * s.B > 100000;                   // (the large ones: both routes, not every layout and frame type)
            for (int kind = 0; kind < 3; ++kind)
                for (int mode = 0; mode < 2; ++mode) {
                    if (mode == 1 && (s.Nx > s.W || s.Ny > s.H)) continue;
                    if (big && kind == 1) continue;
                    for (int f32 = 0; f32 < 2; ++f32) {
                        if (big && f32 != (kind == 2)) continue;
                        run_resize(s, fmt, (kind + mode) % 3, 0, kind, mode, f32 != 0);
                    }
                    if (!big) run_resize(s, fmt, 0, 2, kind, mode, mode != 0);   // GRAY
                }
            if (!big) run_resize(s, fmt, 1, 1, 0, 0, false);                     // RGB
        }
    for (int fmt = 0; fmt < 3; ++fmt)
        for (int mode = 0; mode < 2; ++mode) run_resize(Shape{5, 12, 10, 8, 8}, fmt, 0, 0, 2, mode, false, 2);   // a folded grid
    return report();
}
