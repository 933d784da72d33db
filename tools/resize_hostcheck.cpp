// aefft_image_resize_to_frames without a device: the kernel source itself -- autoencoder-fft_amd/csrc/resize_kernels.hip,
// body and launch geometry -- compiled for the HOST, 256 threads as the lanes of a workgroup and a barrier for __syncthreads, under the
// sanitizers, with the source, frame and LDS buffers allocated at exactly their live extent, against a C restatement of include/aefft.h's
// formulas in 64-bit integers (hostcheck_ref.h's image_to_frames_ref, which shares nothing with the kernel's taps).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Wno-unknown-pragmas
//       -o resize_hostcheck tools/resize_hostcheck.cpp   (one line),   then   ./resize_hostcheck
//
// A stand-alone program: it is not loaded into Python and does not touch a GPU.  Exit status 0 and "all N runs exact" when every run is
// byte-exact (float frames compared as bits) and every byte/element of the frames was written.
#include "hostlanes.h"
#include "../autoencoder-fft_amd/csrc/resize_kernels.hip"
#include "hostcheck_ref.h"

using namespace aefft;

// ---- the bodies the launcher chooses between ----------------------------------------------------
typedef void (*body_fn)(const RzArgs&, unsigned*);
template <int D, bool F32, int MODE> static void body(const RzArgs& a, unsigned* lds) { resize_body<D, F32, MODE>(a, lds); }
#define ROW(D) {{body<D, false, 0>, body<D, false, 1>}, {body<D, true, 0>, body<D, true, 1>}}
static const body_fn BODIES[4][2][2] = {ROW(1), ROW(2), ROW(3), ROW(4)};

struct Shape { int B, D, W, H, Nx, Ny; };

// kind 0 tight, 1 pitch rounded up to 64, 2 pitch W D + 5 from a base off by one byte, 3 a region of interest at (3, 5) of a larger batch
static void run(const Shape& s, int kind, int mode, bool f32, unsigned grid_y = 0)
{
    const int B = s.B, D = s.D, W = s.W, H = s.H, Nx = s.Nx, Ny = s.Ny;
    size_t pitch = (size_t)W * D, stride, off = 0;
    if (kind == 1) pitch = (pitch + 63) / 64 * 64;
    if (kind == 2) { pitch += 5; off = 1; }
    stride = (size_t)H * pitch;
    if (kind == 3) { pitch = (size_t)(W + 9) * D; stride = (size_t)(H + 7) * pitch; off = 3 * pitch + 5 * D; }
    const size_t extent = (size_t)(B - 1) * stride + (size_t)(H - 1) * pitch + (size_t)W * D;   // the LAST byte the call may read is at off + extent - 1
    unsigned char* alloc = (unsigned char*)malloc(off + extent);
    for (size_t k = 0; k < off + extent; ++k) alloc[k] = (unsigned char)rnd();
    const unsigned char* img = alloc + off;
    const size_t n = (size_t)B * D * Nx * Ny, es = f32 ? 4 : 1;
    void* fp = nullptr;
    if (posix_memalign(&fp, 16, n * es)) abort();                                // 16-byte aligned, exactly n elements
    unsigned char* frames = (unsigned char*)fp;
    memset(frames, 0xEE, n * es);
    const RzArgs g = rz_geometry(img, pitch, stride, W, H, mode, frames, B, D, Nx, Ny);
    launch((unsigned)(g.tx * g.ty), grid_y ? grid_y : (unsigned)B, 1u, (size_t)rz_lds_words(D, g.P, g.RB), [&](unsigned* lds) { BODIES[D - 1][f32][mode](g, lds); });
    std::vector<unsigned> want;
    image_to_frames_ref(img, pitch, stride, W, H, mode, f32, B, D, Nx, Ny, want);      // [B][D][Nx][Ny] as the 8-bit pixel or, float frames, q
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
        printf("MISMATCH B=%d D=%d %dx%d -> %dx%d kind=%d mode=%d f32=%d: %zu of %zu differ (words img=%d frm=%d P=%d RB=%d)\n", B, D, W, H, Nx, Ny, kind, mode, (int)f32, bad, n,
               (int)g.img_words, (int)g.frm_words, g.P, g.RB);
    }
    free(frames);
    free(alloc);
}

int main()
{
    const Shape shapes[] = {{1, 1, 8, 8, 8, 8}, {2, 3, 11, 9, 8, 8}, {1, 3, 7, 5, 16, 8}, {2, 4, 64, 64, 32, 32}, {1, 3, 130, 70, 66, 34},
                            {1, 2, 200, 150, 10, 12}, {2, 3, 640, 480, 256, 256}, {1, 3, 1920, 1080, 64, 64},
                            // beyond the device tests: one destination pixel, one source pixel, wide rows that need several bands (down to one row per band), 3 -> 2
                            {1, 1, 37, 29, 1, 1}, {1, 4, 1, 1, 5, 3}, {1, 4, 2500, 40, 16, 4}, {3, 2, 3, 3, 2, 2}, {1, 1, 8192, 3, 2, 3}, {1, 4, 8192, 2, 1, 1}};
    for (const Shape& s : shapes)
        for (int kind = 0; kind < 4; ++kind)
            for (int mode = 0; mode < 2; ++mode) {
                if (mode == 1 && (s.Nx > s.W || s.Ny > s.H)) continue;
                for (int f32 = 0; f32 < 2; ++f32) run(s, kind, mode, f32 != 0);
            }
    // a folded grid: five images on two rows of workgroups
    for (int mode = 0; mode < 2; ++mode) run(Shape{5, 3, 11, 9, 8, 8}, 2, mode, false, 2);
    return report();
}
