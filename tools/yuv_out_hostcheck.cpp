// aefft_image_to_yuv and aefft_frames_resize_to_yuv without a device: the kernel source itself --
// autoencoder-fft_amd/csrc/yuv_out_kernels.hip, both bodies and both launch geometries -- compiled for the HOST, 256 threads as the lanes of a
// workgroup and a barrier for __syncthreads, under the sanitizers, with every destination plane, the source image, the frames and the LDS in
// allocations of their own that end at the last live byte, against a scalar C restatement of include/aefft.h in 64-bit integers (its own
// coefficient table, its own chroma blocks with their live counts, and hostcheck_ref.h's resize: it shares nothing with the kernels, resize_taps.h
// and resize_tile.h included).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Wno-unknown-pragmas
//       -o yuv_out_hostcheck tools/yuv_out_hostcheck.cpp   (one line),   then   ./yuv_out_hostcheck
//
// A stand-alone program: it is not loaded into Python and does not touch a GPU.  Exit status 0 and "all N runs exact" when in every run every
// byte of every plane's allocation is what the restatement says: the live bytes converted, every other byte as it was.
#include "hostlanes.h"
#include "../autoencoder-fft_amd/csrc/yuv_out_kernels.hip"
#include "hostcheck_ref.h"

using namespace aefft;

// ---- include/aefft.h, restated -----------------------------------------------------------------
// yoff, ky, then (r, g, b) of Y, of U, of V
static const i64 TABLE[3][11] = {{16, 900542, 269262, 528618, 102662, -155423, -305128, 460551, 460551, -385654, -74897},
                                 {16, 900542, 191455, 644068, 65019, -105533, -355018, 460551, 460551, -418321, -42230},
                                 {0, 1048576, 313524, 615514, 119538, -176932, -347356, 524288, 524288, -439026, -85262}};
// channel ch (0 R, 1 G, 2 B) of the tight pixel at px
static i64 chan(const unsigned char* px, int order, int ch) { return order == 2 ? px[0] : px[order == 0 ? 2 - ch : ch]; }
static unsigned char luma_ref(const unsigned char* px, int matrix, int order)
{
    const i64* T = TABLE[matrix];
    const i64 t = order == 2 ? T[1] * px[0] : T[2] * chan(px, order, 0) + T[3] * chan(px, order, 1) + T[4] * chan(px, order, 2);
    return (unsigned char)(T[0] + fdiv(t + (1LL << 19), 1LL << 20));
}
// the chroma sample over columns [x0, x0 + 2) x rows [y0, y0 + fy) of image b, cut to the image: which = 0 U, 1 V
static unsigned char chroma_ref(const unsigned char* img, int W, int H, int D, int b, int x0, int y0, int fy, int matrix, int order, int which)
{
    if (order == 2) return 128;
    i64 S[3] = {0, 0, 0}, n = 0;
    for (int y = y0; y < y0 + fy && y < H; ++y)
        for (int x = x0; x < x0 + 2 && x < W; ++x, ++n)
            for (int ch = 0; ch < 3; ++ch) S[ch] += chan(img + (((size_t)b * H + y) * W + x) * D, order, ch);
    const i64 lg = n == 4 ? 2 : n == 2 ? 1 : 0;
    const i64* k = TABLE[matrix] + 5 + 3 * which;
    const i64 v = 128 + fdiv(k[0] * S[0] + k[1] * S[1] + k[2] * S[2] + (n << 19), 1LL << (20 + lg));
    return (unsigned char)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// ---- the bodies the launchers choose between ---------------------------------------------------
typedef void (*image_fn)(const YoArgs&);
typedef void (*frames_fn)(const FyArgs&, unsigned*);
template <int F, int D> static void ibody(const YoArgs& a) { image_yuv_body<F, D>(a); }
template <int F, int D, bool T, int M> static void fbody(const FyArgs& a, unsigned* lds) { frames_yuv_body<F, D, T, M>(a, lds); }
#define FROW(F, D) {{fbody<F, D, false, 0>, fbody<F, D, false, 1>}, {fbody<F, D, true, 0>, fbody<F, D, true, 1>}}
// [format][D == 3] and [format][D == 3][f32][mode]
static const image_fn IBODY[3][2] = {{ibody<0, 1>, ibody<0, 3>}, {ibody<1, 1>, ibody<1, 3>}, {ibody<2, 1>, ibody<2, 3>}};
static const frames_fn FBODY[3][2][2][2] = {{FROW(0, 1), FROW(0, 3)}, {FROW(1, 1), FROW(1, 3)}, {FROW(2, 1), FROW(2, 3)}};

// the destination planes of a run, each in an allocation of its own that ends with the plane's last live byte, pre-filled with 0xEE, and what the
// restatement says each allocation holds afterwards
struct Dest {
    unsigned char* p[3]; size_t pitch[3], stride[3];
    std::vector<unsigned char*> allocs;
    std::vector<std::vector<unsigned char>> want;
    ~Dest() { for (unsigned char* a : allocs) free(a); }
};
// kind 0 tight, 1 pitch rounded up to 64, 2 pitch + 5 from a base off by one byte (the byte route); B > 1: a batch stride that is not the plane's size
static void make_dest(Dest& s, int fmt, int W, int H, int B, int kind, const unsigned char* img, int D, int matrix, int order)
{
    const size_t Wc = (W + 1) / 2, Hc = (H + 1) / 2;
    const size_t live[3] = {fmt == 2 ? 2 * (size_t)W : (size_t)W, fmt == 0 ? 2 * Wc : Wc, Wc}, rows[3] = {(size_t)H, Hc, Hc};
    const int used = fmt == 2 ? 1 : (fmt == 0 ? 2 : 3);
    for (int k = 0; k < 3; ++k) {
        s.p[k] = nullptr; s.pitch[k] = s.stride[k] = 0;
        if (k >= used) continue;
        size_t pitch = live[k], off = 0;
        if (kind == 1) pitch = (pitch + 63) / 64 * 64;
        if (kind == 2) { pitch += 5; off = 1; }
        const size_t stride = rows[k] * pitch + (kind == 2 ? 7 : 16);
        const size_t extent = (size_t)(B - 1) * stride + (rows[k] - 1) * pitch + live[k];
        unsigned char* a = (unsigned char*)malloc(off + extent);
        memset(a, 0xEE, off + extent);
        s.allocs.push_back(a);
        s.p[k] = a + off; s.pitch[k] = pitch; s.stride[k] = stride;
        std::vector<unsigned char> w(off + extent, 0xEE);
        for (int b = 0; b < B; ++b)
            for (size_t r = 0; r < rows[k]; ++r) {
                unsigned char* o = &w[off + b * stride + r * pitch];
                for (size_t c = 0; c < live[k]; ++c) {
                    const unsigned char* px = img + (((size_t)b * H + r) * W) * D;   // (row r of the image: for luma planes)
                    if (fmt == 2) o[c] = c % 2 == 0 ? luma_ref(px + (c / 2) * D, matrix, order) : chroma_ref(img, W, H, D, b, (int)(c / 4) * 2, (int)r, 1, matrix, order, (c % 4) == 3);
                    else if (k == 0) o[c] = luma_ref(px + c * D, matrix, order);
                    else if (fmt == 0) o[c] = chroma_ref(img, W, H, D, b, (int)(c / 2) * 2, (int)r * 2, 2, matrix, order, (int)(c & 1));
                    else o[c] = chroma_ref(img, W, H, D, b, (int)c * 2, (int)r * 2, 2, matrix, order, k - 1);
                }
            }
        s.want.push_back(w);
    }
}
static size_t dest_mismatches(const Dest& s)
{
    size_t bad = 0;
    for (size_t k = 0; k < s.allocs.size(); ++k)
        for (size_t i = 0; i < s.want[k].size(); ++i) bad += s.allocs[k][i] != s.want[k][i];
    return bad;
}

// ikind: the image's layout, as kind; its allocation ends with its last live byte, pad bytes random
static void run_image(int B, int W, int H, int fmt, int matrix, int order, int kind, int ikind, unsigned grid_y = 0)
{
    const int D = order == 2 ? 1 : 3;
    std::vector<unsigned char> tight((size_t)B * H * W * D);
    for (auto& v : tight) v = (unsigned char)rnd();
    size_t pitch = (size_t)W * D, off = 0;
    if (ikind == 1) pitch = (pitch + 63) / 64 * 64;
    if (ikind == 2) { pitch += 5; off = 1; }
    const size_t stride = H * pitch + (ikind == 2 ? 3 : 8), extent = (size_t)(B - 1) * stride + (size_t)(H - 1) * pitch + (size_t)W * D;
    unsigned char* alloc = (unsigned char*)malloc(off + extent);
    for (size_t i = 0; i < off + extent; ++i) alloc[i] = (unsigned char)rnd();
    for (int b = 0; b < B; ++b)
        for (int y = 0; y < H; ++y) memcpy(alloc + off + b * stride + y * pitch, &tight[((size_t)b * H + y) * W * D], (size_t)W * D);
    Dest dst;
    make_dest(dst, fmt, W, H, B, kind, tight.data(), D, matrix, order);
    const YoArgs g = yo_geometry(yo_dest(fmt, dst.p, dst.pitch, dst.stride, W, H, matrix, order, B), fmt, alloc + off, pitch, stride, B);
    const image_fn body = IBODY[fmt][D == 3];
    launch((unsigned)(g.gx * g.gy), grid_y ? grid_y : (unsigned)B, 1u, 0, [&](unsigned*) { body(g); });
    const size_t bad = dest_mismatches(dst);
    ++runs;
    if (bad) {
        ++failures;
        printf("MISMATCH image B=%d %dx%d fmt=%d matrix=%d order=%d kind=%d ikind=%d: %zu differ (words dst=%d img=%d)\n", B, W, H, fmt, matrix, order, kind, ikind, bad,
               (int)g.s.words, (int)g.img_words);
    }
    free(alloc);
}

struct Shape { int B, Nx, Ny, W, H; };

static void run_frames(const Shape& sh, int fmt, int matrix, int order, int kind, int mode, bool f32, unsigned gy = 0, unsigned gz = 1)
{
    const int B = sh.B, W = sh.W, H = sh.H, Nx = sh.Nx, Ny = sh.Ny, D = order == 2 ? 1 : 3;
    const size_t n = (size_t)B * D * Nx * Ny;
    std::vector<unsigned char> px(n);
    for (auto& v : px) v = (unsigned char)rnd();
    void* fp = nullptr;
    if (posix_memalign(&fp, 16, n * (f32 ? 4 : 1))) abort();                     // 16-byte aligned, exactly n elements
    for (size_t k = 0; k < n; ++k) {
        if (f32) ((float*)fp)[k] = (float)px[k] + ((rnd() & 1) ? 0.25f : -0.25f);   // (float frames holding the same pixels)
        else ((unsigned char*)fp)[k] = px[k];
    }
    std::vector<unsigned char> img((size_t)B * H * W * D);                      // the image [B][H][W][D], tight
    frames_to_image_ref(px.data(), B, D, Nx, Ny, mode, W, H, img.data(), (size_t)W * D, (size_t)W * D * H);
    Dest dst;
    make_dest(dst, fmt, W, H, B, kind, img.data(), D, matrix, order);
    const FyArgs g = fy_geometry(yo_dest(fmt, dst.p, dst.pitch, dst.stride, W, H, matrix, order, B), fmt, fp, Nx, Ny, mode, B, D);
    const frames_fn body = FBODY[fmt][D == 3][f32][mode];
    launch((unsigned)(g.tx * g.ty), gy ? gy : (unsigned)B, gz, (size_t)fy_lds_words(D, g), [&](unsigned* lds) { body(g, lds); });
    const size_t bad = dest_mismatches(dst);
    ++runs;
    if (bad) {
        ++failures;
        printf("MISMATCH frames B=%d %dx%d -> %dx%d fmt=%d matrix=%d order=%d kind=%d mode=%d f32=%d: %zu differ (words=%d TX=%d TY=%d P=%d XB=%d)\n", B, Nx, Ny, W, H, fmt,
               matrix, order, kind, mode, (int)f32, bad, (int)g.s.words, g.TX, g.TY, g.P, g.XB);
    }
    free(fp);
}

int main()
{
    // the conversion at the ends of every clamp: four equal pixels of every (R, B) lattice point at the G values 0 and 255, through the kernel's
    // yo_convert against the table above, every matrix
    for (int matrix = 0; matrix < 3; ++matrix) {
        const YoCoef k = yo_coef(matrix, 1);
        size_t bad = 0;
        for (int R = 0; R < 256; R += (R < 3 || R > 251) ? 1 : 7)
            for (int G = 0; G < 256; G += 255)
                for (int Bc = 0; Bc < 256; Bc += (Bc < 3 || Bc > 251) ? 1 : 7) {
                    const unsigned char px[3] = {(unsigned char)R, (unsigned char)G, (unsigned char)Bc};
                    unsigned char row[12];
                    for (int e = 0; e < 4; ++e) memcpy(row + 3 * e, px, 3);
                    unsigned in[2][3], yw[2], cw[2];
                    memcpy(in[0], row, 12); memcpy(in[1], row, 12);
                    yo_convert<YO_NV12, 3>(k, in, yw, cw);
                    bad += (yw[0] & 255u) != luma_ref(px, matrix, 1);
                    bad += (cw[0] & 255u) != chroma_ref(px, 1, 1, 3, 0, 0, 0, 2, matrix, 1, 0);
                    bad += ((cw[0] >> 8) & 255u) != chroma_ref(px, 1, 1, 3, 0, 0, 0, 2, matrix, 1, 1);
                }
        ++runs;
        if (bad) { ++failures; printf("MISMATCH convert matrix=%d: %zu\n", matrix, bad); }
    }
    // image -> yuv: the device test's shapes and beyond (one pixel, one pair, one column, a row of 8192), every format, destination and image layout
    const int ishapes[][3] = {{2, 8, 8}, {2, 11, 9}, {2, 12, 9}, {2, 130, 70}, {1, 1, 1}, {1, 2, 1}, {1, 1, 2}, {3, 5, 2}, {1, 2, 300}, {2, 257, 3}, {1, 8192, 2}};
    for (const auto& s : ishapes)
        for (int fmt = 0; fmt < 3; ++fmt) {
            if (fmt == 2 && (s[1] & 1)) continue;
            for (int kind = 0; kind < 3; ++kind)
                for (int ikind = 0; ikind < 3; ++ikind) run_image(s[0], s[1], s[2], fmt, (kind + ikind) % 3, 0, kind, ikind);
            run_image(s[0], s[1], s[2], fmt, 0, 1, 0, 0);
            for (int kind = 0; kind < 3; kind += 2) run_image(s[0], s[1], s[2], fmt, 1 + kind / 2, 2, kind, kind);
        }
    for (int fmt = 0; fmt < 3; ++fmt) run_image(5, 12, 9, fmt, 0, 0, 2, 2, 2);       // a folded grid: five images on two rows of workgroups
    // frames -> yuv: the device test's shapes and beyond: one destination pixel (pair), one source pixel, a y-reduction beyond 32 (the even-tile
    // rule) also to an odd height, 3 x 3 -> 2 x 2, Ny % 4 != 0 (the element route on the frame side)
    const Shape shapes[] = {{1, 8, 8, 8, 8}, {2, 8, 8, 11, 9}, {2, 8, 8, 12, 9}, {1, 16, 8, 6, 4}, {2, 32, 32, 64, 64}, {1, 66, 34, 130, 70}, {1, 64, 64, 10, 12}, {1, 64, 512, 10, 12},
                            {2, 256, 256, 640, 480}, {1, 64, 64, 1920, 1080},
                            {1, 37, 29, 1, 1}, {1, 37, 29, 2, 1}, {1, 1, 1, 5, 3}, {1, 1, 1, 6, 3}, {1, 9, 700, 4, 3}, {1, 9, 700, 5, 7}, {3, 3, 3, 2, 2}};
    for (const Shape& s : shapes)
        for (int fmt = 0; fmt < 3; ++fmt) {
            if (fmt == 2 && (s.W & 1)) continue;
            const bool big = (size_t)s.W * s.H * s.B > 100000;                   // (the large ones: both routes, not every layout and frame type)
            for (int kind = 0; kind < 3; ++kind)
                for (int mode = 0; mode < 2; ++mode) {
                    if (mode == 1 && (s.W > s.Nx || s.H > s.Ny)) continue;
                    if (big && kind == 1) continue;
                    for (int f32 = 0; f32 < 2; ++f32) {
                        if (big && f32 != (kind == 2)) continue;
                        run_frames(s, fmt, (kind + mode) % 3, 0, kind, mode, f32 != 0);
                    }
                    if (!big) run_frames(s, fmt, 0, 2, kind, mode, mode != 0);   // GRAY
                }
            if (!big) run_frames(s, fmt, 1, 1, 0, 0, false);                     // RGB
        }
    for (int fmt = 0; fmt < 3; ++fmt)
        for (int mode = 0; mode < 2; ++mode) run_frames(Shape{5, 16, 12, 12, 10}, fmt, 0, 0, 2, mode, false, 2, 3);   // a folded grid: b = 2 z + y, one workgroup row beyond B
    return report();
}
