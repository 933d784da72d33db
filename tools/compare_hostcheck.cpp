// aefft_image_compare_map without a device: the kernel source itself -- autoencoder-fft_amd/csrc/compare_kernels.hip, both
// bodies and the launch geometry -- compiled for the HOST, 256 threads as the lanes of a workgroup and a barrier for __syncthreads, under the
// sanitizers, with both images, the map, the score and the LDS allocated at exactly their live extent, against a plain C++ restatement of
// include/aefft.h's formulas (pixel by pixel with floor(x Mx / W) as the cell rule, its own sums in 64 bits: it shares nothing with the kernel).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Wno-unknown-pragmas
//       -o compare_hostcheck tools/compare_hostcheck.cpp   (one line),   then   ./compare_hostcheck
//
// A stand-alone program: it is not loaded into Python and does not touch a GPU.  Exit status 0 and "all N runs exact" when every run is
// bit-exact on every entry of the map and the score.
#include "hostlanes.h"
#include "../autoencoder-fft_amd/csrc/compare_kernels.hip"

using namespace aefft;
typedef long long i64;

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
    unsigned char& at(int b, int y, int x, int D, int d) { return p[(size_t)b * stride + (size_t)y * pitch + (size_t)x * D + d]; }
};
// layout 0: pointer, pitch and stride multiples of 4, as tight as that allows (the dword route; a dword may cross the row's end); 1: the same
// with a wider pad; 2: an odd pitch; 3: layout 0 behind a skewed pointer (2 and 3: the byte route)
static Image* make_image(int W, int H, int D, int B, int layout)
{
    const size_t fill = (size_t)(-W * D) & 3u, pad = layout == 1 ? fill + 4 : layout == 2 ? 1 + ((W * D) & 1) : fill, gap = layout == 1 ? fill + 8 : layout == 2 ? 5 : fill;
    return new Image(W, H, D, B, pad, gap, layout == 3 ? 1 : 0);
}

// ---- the definition, restated: every pixel into its cell floor(x Mx / W), floor(y My / H) --------
struct Moments { i64 n, e, Sx[4], Sr[4], Sxx[4], Srr[4], Sxr[4]; };
static float ref_entry(const Moments& m, int D, int metric)
{
    if (metric == 0) return (float)((double)m.e / (double)(D * m.n));
    double s = 0;
    for (int d = 0; d < D; ++d) {
        const i64 n = m.n, K1 = 65025, K2 = 585225;
        const i64 A1 = 20000 * m.Sx[d] * m.Sr[d] + K1 * n * n, A2 = 20000 * (n * m.Sxr[d] - m.Sx[d] * m.Sr[d]) + K2 * n * n;
        const i64 B1 = 10000 * (m.Sx[d] * m.Sx[d] + m.Sr[d] * m.Sr[d]) + K1 * n * n, B2 = 10000 * (n * m.Sxx[d] - m.Sx[d] * m.Sx[d] + n * m.Srr[d] - m.Sr[d] * m.Sr[d]) + K2 * n * n;
        const double q = ((double)A1 * (double)A2) / ((double)B1 * (double)B2);
        s = d ? s + q : q;
    }
    return (float)(s / (double)D);
}

struct Case { int W, H, Mx, My, D; };
// fill: 0 random bytes; 1 a all 0 and b all 255 (the largest sums); 2 b == a except one cell; 3 the same buffer for both
static void run(const Case& c, int B, int la, int lb, int fill, unsigned fold)
{
    ++runs;
    const int W = c.W, H = c.H, D = c.D, Mx = c.Mx, My = c.My;
    Image* A = make_image(W, H, D, B, la);
    Image* Bm = fill == 3 ? A : make_image(W, H, D, B, lb);
    for (size_t k = 0; k < A->extent; ++k) A->p[k] = (unsigned char)rnd();
    if (fill != 3) for (size_t k = 0; k < Bm->extent; ++k) Bm->p[k] = (unsigned char)rnd();
    for (int b = 0; b < B && (fill == 1 || fill == 2); ++b)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                for (int d = 0; d < D; ++d) {
                    if (fill == 1) { A->at(b, y, x, D, d) = 0; Bm->at(b, y, x, D, d) = 255; }
                    else Bm->at(b, y, x, D, d) = A->at(b, y, x, D, d) ^ (((i64)x * Mx / W == Mx / 2 && (i64)y * My / H == My / 2) ? 0x55 : 0);
                }
    const size_t cells = (size_t)B * Mx * My;
    void *mp = nullptr, *sp = nullptr;
    if (posix_memalign(&mp, 16, cells * 4) || posix_memalign(&sp, 16, (size_t)B * 4)) abort();   // exactly the map and the score
    float *map = (float*)mp, *score = (float*)sp;
    size_t bad = 0;
    for (int metric = 0; metric < 2; ++metric) {
        memset(map, 0xEE, cells * 4); memset(score, 0xEE, (size_t)B * 4);
        CmArgs g;
        if (!cm_geometry(A->p, A->pitch, A->stride, Bm->p, Bm->pitch, Bm->stride, W, H, B, D, Mx, My, map, &g)) abort();
        const bool words_a = la < 2, words_b = fill == 3 ? words_a : lb < 2;
        if ((g.a_words != 0) != words_a || (g.b_words != 0) != words_b) { ++bad; printf("ROUTE a=%d b=%d\n", g.a_words, g.b_words); }
        const size_t lds_words = (size_t)(CM_LANES + g.cpw) * (metric ? 5 * D : 1);   // what a workgroup of cpw cells touches (the kernel declares the most cells)
        launch(g.spans, fold ? fold : cm_grid_y(g), fold ? (g.units + fold - 1) / fold : cm_grid_z(g), lds_words, [&](unsigned* lds) {
            const unsigned u = blockIdx.z * gridDim.y + blockIdx.y;
            if (u >= (unsigned)g.units) return;
            switch (D * 2 + metric) {
                case 2: compare_map_body<1, 0>(g, blockIdx.x, u, lds); break;
                case 3: compare_map_body<1, 1>(g, blockIdx.x, u, lds); break;
                case 4: compare_map_body<2, 0>(g, blockIdx.x, u, lds); break;
                case 5: compare_map_body<2, 1>(g, blockIdx.x, u, lds); break;
                case 6: compare_map_body<3, 0>(g, blockIdx.x, u, lds); break;
                case 7: compare_map_body<3, 1>(g, blockIdx.x, u, lds); break;
                case 8: compare_map_body<4, 0>(g, blockIdx.x, u, lds); break;
                default: compare_map_body<4, 1>(g, blockIdx.x, u, lds); break;
            }
        });
        launch(B, 1, 1, 2 * (size_t)CM_CELLS + My, [&](unsigned* lds) { compare_score_body(map, score, W, H, Mx, My, blockIdx.x, (double*)lds); });
        std::vector<Moments> mom(cells);
        memset(mom.data(), 0, cells * sizeof(Moments));
        for (int b = 0; b < B; ++b)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    Moments& m = mom[((size_t)b * Mx + (size_t)((i64)x * Mx / W)) * My + (size_t)((i64)y * My / H)];
                    ++m.n;
                    for (int d = 0; d < D; ++d) {
                        const i64 xv = A->at(b, y, x, D, d), rv = Bm->at(b, y, x, D, d);
                        m.e += (xv - rv) * (xv - rv);
                        m.Sx[d] += xv; m.Sr[d] += rv; m.Sxx[d] += xv * xv; m.Srr[d] += rv * rv; m.Sxr[d] += xv * rv;
                    }
                }
        for (int b = 0; b < B; ++b) {
            double S = 0;
            for (int I = 0; I < Mx; ++I) {
                double r = 0;
                for (int J = 0; J < My; ++J) {
                    const size_t k = ((size_t)b * Mx + I) * My + J;
                    const float want = ref_entry(mom[k], D, metric);
                    bad += memcmp(&want, &map[k], 4) != 0;
                    if (fill == 3) bad += map[k] != (metric ? 1.0f : 0.0f);
                    if (fill == 2 && metric == 0) bad += (map[k] != 0.0f) != (I == Mx / 2 && J == My / 2);
                    const double p = (double)map[k] * (double)mom[k].n;
                    r = J ? r + p : p;
                }
                S = I ? S + r : r;
            }
            const float want = (float)(S / (double)((i64)W * H));
            bad += memcmp(&want, &score[b], 4) != 0;
        }
    }
    if (bad) {
        ++failures;
        printf("MISMATCH W=%d H=%d M=%dx%d D=%d B=%d layouts %d,%d fill=%d: %zu entries differ\n", W, H, Mx, My, D, B, la, lb, fill, bad);
    }
    free(mp); free(sp);
    if (Bm != A) delete Bm;
    delete A;
}

int main()
{
    // the device tests' shapes, then: the largest cells at D = 1..3, cells one dword wide, a span of three cells of 65 dwords, the most cells along x,
    // a single cell, a row shorter than a dword
    const std::vector<Case> cases = {{13, 9, 4, 3, 3}, {5, 5, 5, 5, 1}, {128, 64, 2, 1, 4}, {130, 70, 3, 2, 3}, {65, 67, 5, 7, 2}, {641, 37, 11, 1, 3},
                                     {256, 256, 32, 32, 3}, {64, 64, 1, 1, 1}, {127, 33, 2, 1, 2}, {190, 5, 3, 1, 3}, {23, 11, 23, 11, 4}, {448, 3, 7, 3, 4},
                                     {1030, 2, 1024, 1, 1}, {3, 1, 1, 1, 1}, {1, 1, 1, 1, 3}, {77, 40, 9, 2, 1}};
    int pick = 0;
    for (const Case& c : cases)
        for (int la = 0; la < 4; ++la) {
            const int lb = (la + pick++) % 4;                                     // every layout of a, against a layout of b that moves on
            run(c, 1 + (pick & 1), la, lb, 0, 0);
        }
    for (int la = 0; la < 4; ++la)                                                // every pair of layouts on the shape with straddling dwords
        for (int lb = 0; lb < 4; ++lb) run(cases[0], 2, la, lb, 0, la == lb ? 3 : 0);
    for (const Case& c : cases) {
        run(c, 1, 0, 2, 1, 0);
        run(c, 2, 3, 0, 2, 0);
        run(c, 2, pick++ % 4, 0, 3, 0);
    }
    // the cell rows folded onto grid.y x grid.z as for B My > 65535: unit = z grid.y + y, the workgroups beyond the last unit return at once
    run(cases[0], 2, 0, 2, 0, 4);                                                 // 6 units on 4 x 2
    run(cases[0], 2, 3, 1, 0, 7);                                                 // 6 units on 7 x 1
    run(cases[4], 3, 1, 0, 0, 4);                                                 // 21 units on 4 x 6
    run({1920, 1080, 120, 68, 3}, 1, 0, 0, 0, 0);                                 // rows in cells of 15 and 16
    return report();
}
