// aefft_map_regions without a device: the kernel source itself -- autoencoder-fft_amd/csrc/regions_kernels.hip, the six
// bodies and the launch geometry -- compiled for the HOST, 256 threads as the lanes of a workgroup and a barrier for __syncthreads, the workgroups
// of a launch one after another (legal because no workgroup ever waits for another one), under the sanitizers, with the map, the baseline, the
// labels, the regions, the counts, the workspace and the LDS allocated at exactly their live extent, against a plain C++ flood fill that restates
// include/aefft.h's definition (it shares nothing with the kernels: no union-find, no keys).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Wno-unknown-pragmas
//       -o regions_hostcheck tools/regions_hostcheck.cpp   (one line),   then   ./regions_hostcheck
//
// A stand-alone program: it is not loaded into Python and does not touch a GPU.  Exit status 0 and "all N runs exact" when every run is
// bit-exact on every label, every count and every byte of the regions (the untouched tail included).
#include "hostlanes.h"
#include "../autoencoder-fft_amd/csrc/regions_kernels.hip"

using namespace aefft;

struct Region { int i0, j0, i1, j1, area, peak_i, peak_j; float peak; };
static_assert(sizeof(Region) == 4 * RG_WORDS, "aefft_region");

template <class T> static T* exact(size_t n)
{
    void* q = nullptr;
    if (posix_memalign(&q, 16, n ? n * sizeof(T) : 1)) abort();
    return (T*)q;
}

// ---- the definition, restated: a flood fill in scan order -----------------------------------------
struct Want { std::vector<int> labels, count; std::vector<Region> regions; };
static Want reference(const float* map, const float* ref, int Mx, int My, int B, int sense, float lo, float hi, int conn, int min_area, int max_regions,
                      const std::vector<Region>& fill)
{
    const int cells = Mx * My;
    Want w;
    w.labels.assign((size_t)B * cells, 0); w.count.assign(B, 0); w.regions = fill;
    std::vector<float> v(cells);
    std::vector<char> fg(cells), seen(cells);
    for (int b = 0; b < B; ++b) {
        for (int p = 0; p < cells; ++p) {
            volatile float d = ref ? map[(size_t)b * cells + p] - ref[p] : map[(size_t)b * cells + p];
            float x = d;
            if (x == 0.0f) x = 0.0f * 0.0f;                                       // +0
            v[p] = x;
            fg[p] = sense ? x <= lo : x >= lo;
            seen[p] = 0;
        }
        int n = 0;
        for (int p = 0; p < cells; ++p) {
            if (!fg[p] || seen[p]) continue;
            std::vector<int> comp, stack{p};
            seen[p] = 1;
            while (!stack.empty()) {
                const int q = stack.back();
                stack.pop_back();
                comp.push_back(q);
                const int I = q / My, J = q % My;
                for (int di = -1; di <= 1; ++di)
                    for (int dj = -1; dj <= 1; ++dj) {
                        if ((!di && !dj) || (conn == 4 && di && dj)) continue;
                        const int a = I + di, c = J + dj;
                        if (a < 0 || a >= Mx || c < 0 || c >= My || !fg[a * My + c] || seen[a * My + c]) continue;
                        seen[a * My + c] = 1;
                        stack.push_back(a * My + c);
                    }
            }
            bool strong = false;
            Region r{Mx, My, -1, -1, (int)comp.size(), 0, 0, 0.f};
            int peak_p = -1;
            for (int q : comp) {
                const int I = q / My, J = q % My;
                strong |= sense ? v[q] <= hi : v[q] >= hi;
                r.i0 = I < r.i0 ? I : r.i0; r.i1 = I > r.i1 ? I : r.i1; r.j0 = J < r.j0 ? J : r.j0; r.j1 = J > r.j1 ? J : r.j1;
                const bool better = peak_p < 0 || (sense ? v[q] < v[peak_p] : v[q] > v[peak_p]) || (v[q] == v[peak_p] && q < peak_p);
                if (better) peak_p = q;
            }
            if (!strong || r.area < min_area) continue;
            ++n;
            r.peak_i = peak_p / My; r.peak_j = peak_p % My; r.peak = v[peak_p];
            for (int q : comp) w.labels[(size_t)b * cells + q] = n;
            if (n <= max_regions) w.regions[(size_t)b * max_regions + n - 1] = r;
        }
        w.count[b] = n;
    }
    return w;
}

// ---- the patterns: 1 = foreground -----------------------------------------------------------------
enum { EMPTY, FULL, SPIRAL, U_SHAPE, COMB, RING, DIAG, ANTIDIAG, CHECKER, BARS, RANDOM30, RANDOM50, RANDOM60, NPATTERNS };
// a track one cell wide that winds inwards with a gap of one cell: it crosses every tile, and its cells lie far from its first one
static const std::vector<char>& spiral(int Mx, int My)
{
    static std::vector<char> m;
    static int mx = 0, my = 0;
    if (mx == Mx && my == My) return m;
    mx = Mx; my = My;
    m.assign((size_t)Mx * My, 0);
    auto in = [&](int i, int j) { return i >= 0 && i < Mx && j >= 0 && j < My; };
    int i = 0, j = 0, di = 0, dj = 1, turned = 0;
    m[0] = 1;
    while (turned < 2) {
        const int ni = i + di, nj = j + dj;
        if (in(ni, nj) && !m[ni * My + nj] && !(in(ni + di, nj + dj) && m[(ni + di) * My + nj + dj])) { i = ni; j = nj; m[i * My + j] = 1; turned = 0; }
        else { const int t = di; di = dj; dj = -t; ++turned; }
    }
    return m;
}

static bool pattern(int kind, int I, int J, int Mx, int My)
{
    switch (kind) {
        case EMPTY: return false;
        case FULL: return true;
        case SPIRAL: return spiral(Mx, My)[I * My + J];
        case U_SHAPE: return J == 0 || J == My - 1 || I == Mx - 1;                // the arms meet at the far end
        case COMB: return I == Mx - 1 || J % 2 == 0;                              // teeth along I joined by the last row
        case RING: return (I == 0 || I == Mx - 1 || J == 0 || J == My - 1) || (Mx > 4 && My > 4 && I == Mx / 2 && J == My / 2);
        case DIAG: return I % My == J || J % Mx == I;
        case ANTIDIAG: return (I + J) % std::max(Mx, My) == std::max(Mx, My) - 1;
        case CHECKER: return (I + J) % 2 == 0;
        case BARS: return I % 3 == 0 || (J % 19 == 5);                            // bars across every tile in both directions
        default: return false;
    }
}

struct Case { int Mx, My; };
static void run(const Case& c, int B, int kind, int sense, int conn, int mode, int min_area, int max_regions)
{
    ++runs;
    const int Mx = c.Mx, My = c.My, cells = Mx * My;
    const size_t total = (size_t)B * cells;
    float *map = exact<float>(total), *ref = (mode & 1) ? exact<float>(cells) : nullptr;
    // mode bit 0: a baseline; bit 1: special values (NaN, +-inf, -0) sprinkled in; bit 2: raw random floats (the subtraction rounds); bit 3: lo == hi
    float lo = sense ? 0.5f : 0.5f, hi = sense ? 0.25f : 0.75f;
    if (mode & 8) hi = lo;
    const float q = 1.0f / 32.0f;
    for (int p = 0; ref && p < cells; ++p) ref[p] = (mode & 4) ? (float)rnd() / 255.0f * 0.37f : (float)(rnd() % 8) * q;
    for (int b = 0; b < B; ++b)
        for (int p = 0; p < cells; ++p) {
            const int I = p / My, J = p % My;
            bool f = kind >= RANDOM30 ? (int)rnd() < (kind == RANDOM30 ? 77 : kind == RANDOM50 ? 128 : 154) : pattern(kind, I, J, Mx, My);
            if (b == 1 && kind < RANDOM30) f = pattern(kind, Mx - 1 - I, My - 1 - J, Mx, My);          // the second image: the pattern turned round
            float v;
            if (mode & 4) v = f ? (sense ? 0.5f - (float)rnd() / 512.0f : 0.5f + (float)rnd() / 512.0f) : (sense ? 0.51f + (float)rnd() / 512.0f : 0.49f - (float)rnd() / 512.0f);
            else {
                const int k = (int)(rnd() % 8);                                   // values on a grid of 1/32: equal peaks are common
                v = sense ? (f ? 0.5f - k * q * 1.2f : 0.5f + (k + 1) * q) : (f ? 0.5f + k * q * 1.2f : 0.5f - (k + 1) * q);
                if (f && (mode & 16)) v = sense ? 0.5f - (k & 1) * 8 * q : 0.5f + (k & 1) * 8 * q;   // two values only
            }
            if ((mode & 2) && rnd() < 20) {
                const unsigned s = rnd() % 4;
                v = s == 0 ? NAN : s == 1 ? INFINITY : s == 2 ? -INFINITY : -0.0f;
            }
            map[(size_t)b * cells + p] = ref ? v + ref[p] : v;
        }
    if (mode & 32) {                                                              // zeros of both signs around a threshold at zero
        lo = sense ? 0.0f : -1.0f; hi = sense ? -0.25f : 0.0f;
        for (size_t k = 0; k < total; ++k) { const unsigned s = rnd() % 4; map[k] = (s == 0 ? -0.0f : s == 1 ? 0.0f : s == 2 ? -0.5f : 0.5f) + (ref ? ref[k % cells] : 0.0f); }
    }
    int *labels = exact<int>(total), *count = exact<int>(B);
    Region* regions = max_regions ? exact<Region>((size_t)B * max_regions) : nullptr;
    std::vector<Region> fill((size_t)B * max_regions);
    if (!fill.empty()) memset(fill.data(), 0xEE, fill.size() * sizeof(Region));
    const size_t wb = regions_workspace(Mx, My, B);
    if (wb != 16 * total) abort();
    size_t bad = 0;
    const Want want = reference(map, ref, Mx, My, B, sense, lo, hi, conn, min_area, max_regions, fill);
    std::vector<int> first_labels;
    for (int rep = 0; rep < (runs % 4 == 0 ? 2 : 1); ++rep) {                     // every fourth run twice: the same bytes whatever the workspace held
        unsigned char* work = exact<unsigned char>(wb);
        memset(work, rep ? 0xFF : 0x11, wb);
        memset(labels, 0xEE, total * 4); memset(count, 0xEE, (size_t)B * 4);
        if (regions) memcpy(regions, fill.data(), fill.size() * sizeof(Region));
        RgArgs g;
        if (!rg_geometry(map, ref, Mx, My, B, sense, lo, hi, conn, min_area, labels, (int*)regions, max_regions, count, work, &g)) abort();
        launch(g.tiles, 1, 1, RG_TILE_WORDS, [&](unsigned* lds) { regions_tile_body(g, blockIdx.x, lds); });
        launch(g.flat, 1, 1, 0, [&](unsigned*) { regions_border_body(g, blockIdx.x * RG_LANES + threadIdx.x); });
        launch(g.flat, 1, 1, 0, [&](unsigned*) { regions_flatten_body(g, blockIdx.x * RG_LANES + threadIdx.x); });
        launch(g.blocks, 1, 1, 1, [&](unsigned* lds) { regions_count_body(g, blockIdx.x, lds); });
        launch(g.blocks, 1, 1, RG_RANK_WORDS, [&](unsigned* lds) { regions_rank_body(g, blockIdx.x, lds); });
        launch(g.tiles, 1, 1, RG_FINAL_WORDS, [&](unsigned* lds) { regions_final_body(g, blockIdx.x, lds); });
        for (size_t k = 0; k < total; ++k) bad += labels[k] != want.labels[k];
        for (int b = 0; b < B; ++b) bad += count[b] != want.count[b];
        if (regions) bad += memcmp(regions, want.regions.data(), fill.size() * sizeof(Region)) != 0;
        free(work);
    }
    if (bad) {
        ++failures;
        printf("MISMATCH %dx%d B=%d pattern %d sense %d conn %d mode %d min_area %d max_regions %d: %zu differ (count %d, want %d)\n", Mx, My, B, kind, sense, conn,
               mode, min_area, max_regions, bad, count[0], want.count[0]);
    }
    free(map); free(ref); free(labels); free(count); free(regions);
}

int main()
{
    // T = 16: one cell, one row, one column, a tile, a tile and a cell, three tiles by a short one, four and more tiles in both directions, long and thin
    const std::vector<Case> cases = {{1, 1}, {1, 7}, {7, 1}, {16, 16}, {17, 17}, {33, 15}, {50, 67}, {3, 200}, {200, 3}, {32, 32}};
    int pick = 0;
    for (const Case& c : cases)
        for (int kind = 0; kind < NPATTERNS; ++kind)
            for (int conn = 4; conn <= 8; conn += 4) {
                if (kind != DIAG && kind != ANTIDIAG && kind != CHECKER && conn != (pick % 2 ? 4 : 8)) { ++pick; continue; }   // (the others: connectivities in turn)
                const int sense = (pick >> 1) & 1, B = 1 + 2 * ((pick >> 2) & 1);
                // hysteresis and ties on every run; every fourth a plain threshold, every third a baseline, min_area 1..3, regions short of the count now and then
                run(c, B, kind, sense, conn, ((pick % 3) == 0 ? 1 : 0) | ((pick % 4) == 3 ? 8 : 0), 1 + pick % 3, pick % 5 == 0 ? 3 : 64);
                ++pick;
            }
    for (const Case& c : {cases[4], cases[6]})
        for (int sense = 0; sense < 2; ++sense)
            for (int conn = 4; conn <= 8; conn += 4) {
                run(c, 3, RANDOM50, sense, conn, 2, 1, 4096);                     // NaN, +-inf, -0
                run(c, 2, RANDOM60, sense, conn, 1 | 2, 2, 4096);
                run(c, 2, RANDOM60, sense, conn, 1 | 4, 1, 4096);                 // raw floats minus a baseline
                run(c, 1, RANDOM30, sense, conn, 4, 1, 0);                        // no regions at all
                run(c, 2, RANDOM60, sense, conn, 16, 1, 4096);                    // equal peaks throughout
                run(c, 2, RANDOM50, sense, conn, 32, 1, 4096);                    // zeros of both signs
                run(c, 2, RANDOM50, sense, conn, 32 | 1, 1, 4096);
                run(c, 1, CHECKER, sense, conn, 8, 1, 7);                         // more components than regions
            }
    run({130, 70}, 1, RANDOM60, 0, 8, 0, 1, 4096);                                // more than one ranking block an image (9100 cells)
    run({130, 70}, 2, RANDOM50, 1, 4, 0, 2, 4096);
    run({130, 70}, 1, SPIRAL, 0, 4, 0, 1, 16);
    return report();
}
