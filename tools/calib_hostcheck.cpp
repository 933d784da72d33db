// aefft_map_stats_update / _merge / _finish and aefft_map_peak without a device: the kernel source itself --
// autoencoder-fft_amd/csrc/calib_kernels.hip, the four bodies and the launch geometry -- compiled for the HOST, 256 threads as the lanes of a
// workgroup and a barrier for __syncthreads, under the sanitizers, with the maps, the states, the baseline, the peaks, the cells and the LDS
// allocated at exactly their live extent, against a scalar C restatement of include/aefft.h's definition that shares nothing with the kernels: it
// keeps every counted value of a cell in a list, adds in order through volatile doubles (nothing contracts), sorts the list for the extremes and
// takes the peak in a plain loop (no keys).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Wno-unknown-pragmas
//       -o calib_hostcheck tools/calib_hostcheck.cpp   (one line),   then   ./calib_hostcheck   (./calib_hostcheck quick: the small grids only)
//
// A stand-alone program: it is not loaded into Python and does not touch a GPU.  Exit status 0 and "all N runs exact" when every run is
// bit-exact on every byte of the states (the padding included), of the baselines, of the peaks and of the cells.
#include "hostlanes.h"
#include "../autoencoder-fft_amd/csrc/calib_kernels.hip"

#include <algorithm>

using namespace aefft;

// the harness runs 256 lanes a workgroup: the peak's body is generic in its lanes (1024 on the device), its LDS a key a lane
constexpr int HOST_LANES = 256, HOST_PEAK_WORDS = CB_PEAK_KEY_WORDS * HOST_LANES;
static_assert(HOST_LANES == CB_LANES, "the other bodies' launches use the kernels' own block");

template <class T> static T* exact(size_t n)
{
    void* q = nullptr;
    if (posix_memalign(&q, 16, n ? n * sizeof(T) : 1)) abort();
    return (T*)q;
}

static float from_bits(unsigned u) { float v; memcpy(&v, &u, 4); return v; }
static unsigned to_bits(float v) { unsigned u; memcpy(&u, &v, 4); return u; }

// ---- the definition, restated -----------------------------------------------------------------------
struct RefCell {
    double s1 = 0.0, s2 = 0.0;
    std::vector<float> seen;                                                      // every counted value, in arrival order
};

static void ref_count(RefCell& c, float x)
{
    if (!isfinite(x)) return;
    if (x == 0.0f) x = 0.0f * 0.0f;                                               // +0
    volatile double d = (double)x, sq = d * d, a = c.s1 + d, b = c.s2 + sq;
    c.s1 = a; c.s2 = b;
    c.seen.push_back(x);
}

// the bytes of a state of n cells out of the restated cells; `bytes` is the state's size, the padding zero
static std::vector<unsigned char> ref_state(const std::vector<RefCell>& cells, size_t bytes)
{
    const size_t n = cells.size();
    std::vector<unsigned char> out(bytes, 0);
    for (size_t p = 0; p < n; ++p) {
        const RefCell& c = cells[p];
        memcpy(&out[8 * p], &c.s1, 8);
        memcpy(&out[8 * n + 8 * p], &c.s2, 8);
        std::vector<float> s = c.seen;
        std::sort(s.begin(), s.end());
        for (size_t k = 0; k < 4 && k < s.size(); ++k) {
            memcpy(&out[16 * n + 4 * (k * n + p)], &s[s.size() - 1 - k], 4);
            memcpy(&out[32 * n + 4 * (k * n + p)], &s[k], 4);
        }
        const int cnt = (int)s.size();
        memcpy(&out[48 * n + 4 * p], &cnt, 4);
    }
    return out;
}

static RefCell ref_merge(const RefCell& a, const RefCell& b)
{
    RefCell m;
    volatile double s1 = a.s1 + b.s1, s2 = a.s2 + b.s2;
    m.s1 = s1; m.s2 = s2;
    m.seen = a.seen;
    m.seen.insert(m.seen.end(), b.seen.begin(), b.seen.end());
    return m;
}

static float ref_finish(const RefCell& c, int mode, int sense, float k, int rank, float empty)
{
    const int cnt = (int)c.seen.size();
    if (!cnt) return empty;
    if (mode == 1) {
        std::vector<float> s = c.seen;
        std::sort(s.begin(), s.end());
        const int r = std::min(rank, cnt);
        return sense ? s[r - 1] : s[cnt - r];
    }
    volatile double mean = c.s1 / (double)cnt, sd = 0.0;
    if (cnt > 1) {
        volatile double p = c.s1 * mean;
        volatile double d = c.s2 - p;
        if (d < 0.0) d = 0.0;
        volatile double var = d / (double)(cnt - 1);
        sd = sqrt(var);
    }
    volatile double t = (double)k * sd;
    volatile double r = mean + t;
    return (float)r;
}

static void ref_peak(const float* map, const float* ref, int n, int sense, float* peak, int* cell)
{
    int at = -1;
    float best = 0.0f;
    for (int p = 0; p < n; ++p) {
        volatile float d = ref ? map[p] - ref[p] : map[p];
        float v = d;
        if (v != v) continue;
        if (v == 0.0f) v = 0.0f * 0.0f;
        if (at < 0 || (sense ? v < best : v > best)) { at = p; best = v; }
    }
    *peak = at < 0 ? from_bits(0x7FC00000u) : best;
    *cell = at;
}

// ---- the values ---------------------------------------------------------------------------------------
enum { WIDE, UNIT, GRID, NKINDS };
static float value(int kind)
{
    const unsigned r24 = (rnd() << 16) | (rnd() << 8) | rnd();
    if (kind == WIDE) return (float)r24 / 16777216.0f * 65025.0f;
    if (kind == UNIT) return (float)r24 / 8388608.0f - 1.0f;
    return (float)((int)(rnd() % 16) - 4) / 32.0f;                                // ties are common
}
static float special()
{
    const unsigned s = rnd() % 5;
    return s == 0 ? from_bits(0x7FC00000u) : s == 1 ? INFINITY : s == 2 ? -INFINITY : s == 3 ? -0.0f : 0.0f;
}

// B maps of n cells: with `specials` NaN, +-inf and +-0 are planted, cell 0 is never finite and the last cell is constant (its d may come out
// negative before the clamp)
static void fill(float* map, int n, int B, int kind, bool specials)
{
    for (int b = 0; b < B; ++b)
        for (int p = 0; p < n; ++p) {
            float v = value(kind);
            if (specials && rnd() < 24) v = special();
            if (specials && p == 0) v = rnd() & 1 ? from_bits(0xFFC00001u) : INFINITY;
            if (specials && p == n - 1 && n > 1) v = 0.1f;
            map[(size_t)b * n + p] = v;
        }
}

static void run_update(CbArgs g, const float* map, int B, void* state)
{
    g.map = map; g.B = B; g.state = state;
    launch(cb_grid(g), 1, 1, 0, [&](unsigned*) { calib_update_body(g, blockIdx.x * CB_LANES + threadIdx.x); });
}

static size_t differ(const void* got, const std::vector<unsigned char>& want) { return memcmp(got, want.data(), want.size()) != 0; }

// the whole chain on one grid: updates of `Bs` maps in a row, the same footage split in two and merged, every finish, every peak
static void run(int Mx, int My, const std::vector<int>& Bs, int kind, bool specials, bool quick)
{
    ++runs;
    const int n = Mx * My;
    const size_t bytes = calib_state_bytes(Mx, My);
    if (bytes != (((size_t)52 * n + 15) & ~(size_t)15)) abort();
    CbArgs g0;
    if (!cb_geometry(Mx, My, 1, &g0)) abort();
    size_t bad = 0;
    unsigned char *whole = exact<unsigned char>(bytes), *first = exact<unsigned char>(bytes), *second = exact<unsigned char>(bytes);
    memset(whole, 0, bytes); memset(first, 0, bytes); memset(second, 0, bytes);
    std::vector<RefCell> rw(n), r1(n), r2(n);
    std::vector<float*> maps;
    for (size_t u = 0; u < Bs.size(); ++u) {
        const int B = Bs[u];
        float* map = exact<float>((size_t)B * n);
        fill(map, n, B, kind, specials);
        maps.push_back(map);
        run_update(g0, map, B, whole);
        run_update(g0, map, B, u == 0 ? first : second);                          // the split: the first update here, the others there
        for (int p = 0; p < n; ++p)
            for (int b = 0; b < B; ++b) {
                ref_count(rw[p], map[(size_t)b * n + p]);
                ref_count(u == 0 ? r1[p] : r2[p], map[(size_t)b * n + p]);
            }
        bad += differ(whole, ref_state(rw, bytes));                               // after every update
    }
    bad += differ(first, ref_state(r1, bytes)) + differ(second, ref_state(r2, bytes));
    // merge: second enters first; the restated merge of the restated halves, and hi / lo / c of the unsplit run
    {
        const std::vector<unsigned char> keep(second, second + bytes);
        CbArgs g = g0;
        g.state = first; g.src = second;
        launch(cb_grid(g), 1, 1, 0, [&](unsigned*) { calib_merge_body(g, blockIdx.x * CB_LANES + threadIdx.x); });
        std::vector<RefCell> rm(n);
        for (int p = 0; p < n; ++p) rm[p] = ref_merge(r1[p], r2[p]);
        bad += differ(first, ref_state(rm, bytes)) + differ(second, keep);
        bad += memcmp(first + (size_t)16 * n, whole + (size_t)16 * n, (size_t)36 * n) != 0;
        // finish, on the merged state (its sums are the merge's) and on the unsplit one
        float *ref = exact<float>(n), *want = exact<float>(n);
        int pick = runs;
        for (int which = 0; which < 2; ++which) {
            if (quick && which != (runs & 1)) continue;                               // (the quick form: the two states in turn)
            for (int mode = 0; mode < 2; ++mode)
                for (int sense = 0; sense < 2; ++sense)
                    for (int v = 0; v < (mode ? 4 : 3); ++v) {
                        const float ks[3] = {0.0f, 3.0f, -2.5f};
                        const float k = mode ? 3.0f : ks[v], empty = (pick++ & 1) ? INFINITY : 0.0f;
                        const int rank = mode ? v + 1 : 1 + pick % 4;
                        CbArgs f = g0;
                        f.state = which ? whole : first; f.ref_out = ref; f.mode = mode; f.sense = sense; f.rank = rank; f.k = k; f.empty = empty;
                        memset(ref, 0xEE, (size_t)n * 4);
                        launch(cb_grid(f), 1, 1, 0, [&](unsigned*) { calib_finish_body(f, blockIdx.x * CB_LANES + threadIdx.x); });
                        for (int p = 0; p < n; ++p) want[p] = ref_finish(which ? rw[p] : rm[p], mode, sense, k, rank, empty);
                        const bool off = memcmp(ref, want, (size_t)n * 4) != 0;
                        if (off) printf("  finish which %d mode %d sense %d k %g rank %d differs\n", which, mode, sense, k, rank);
                        bad += off;
                    }
        }
        // peak: the last maps, with and without the RANK-1 baseline of the sense
        const int B = Bs.back();
        float* peak = exact<float>(B);
        int* cell = exact<int>(B);
        for (int sense = 0; sense < 2; ++sense)
            for (int with = 0; with < 2; ++with) {
                for (int p = 0; p < n; ++p) want[p] = ref_finish(rw[p], 1, sense, 0.0f, 2, specials ? -INFINITY : 0.25f);
                CbArgs k = g0;
                k.map = maps.back(); k.ref_in = with ? want : nullptr; k.B = B; k.sense = sense; k.peak = peak; k.cell = cell;
                memset(peak, 0xEE, (size_t)B * 4); memset(cell, 0xEE, (size_t)B * 4);
                launch((unsigned)B, 1, 1, HOST_PEAK_WORDS, [&](unsigned* lds) { calib_peak_body<HOST_LANES>(k, blockIdx.x, lds); });
                for (int b = 0; b < B; ++b) {
                    float wp; int wc;
                    ref_peak(maps.back() + (size_t)b * n, with ? want : nullptr, n, sense, &wp, &wc);
                    const bool off = to_bits(wp) != to_bits(peak[b]) || wc != cell[b];
                    if (off) printf("  peak sense %d ref %d image %d: %08x at %d, want %08x at %d\n", sense, with, b, to_bits(peak[b]), cell[b], to_bits(wp), wc);
                    bad += off;
                }
            }
        free(ref); free(want); free(peak); free(cell);
    }
    if (bad) {
        ++failures;
        printf("MISMATCH %dx%d kind %d specials %d updates %zu: %zu checks differ\n", Mx, My, kind, (int)specials, Bs.size(), bad);
    }
    for (float* m : maps) free(m);
    free(whole); free(first); free(second);
}

// an image of NaN only, and ties: the smallest index wins
static void run_peak_edges()
{
    ++runs;
    const int Mx = 15, My = 17, n = Mx * My, B = 3;
    CbArgs g;
    if (!cb_geometry(Mx, My, B, &g)) abort();
    float *map = exact<float>((size_t)B * n), *peak = exact<float>(B);
    int* cell = exact<int>(B);
    for (int p = 0; p < n; ++p) {
        map[p] = from_bits(p & 1 ? 0x7FC00000u : 0xFFFFFFFFu);                    // NaN of both signs
        map[n + p] = p % 50 == 37 ? 2.0f : p % 7 == 3 ? -3.0f : 1.0f;             // the peak at 37, 87, ...; the trough at 3, 10, ...
        map[2 * n + p] = p == n - 1 ? -0.0f : 0.0f;                               // all equal once -0 counts as +0
    }
    size_t bad = 0;
    for (int sense = 0; sense < 2; ++sense) {
        g.map = map; g.sense = sense; g.peak = peak; g.cell = cell;
        launch((unsigned)B, 1, 1, HOST_PEAK_WORDS, [&](unsigned* lds) { calib_peak_body<HOST_LANES>(g, blockIdx.x, lds); });
        bad += to_bits(peak[0]) != 0x7FC00000u || cell[0] != -1;
        bad += sense ? (peak[1] != -3.0f || cell[1] != 3) : (peak[1] != 2.0f || cell[1] != 37);
        bad += to_bits(peak[2]) != 0 || cell[2] != 0;
    }
    if (bad) { ++failures; printf("MISMATCH peak edges: %zu\n", bad); }
    free(map); free(peak); free(cell);
}

// cb_sqrt_fix turns a candidate one ulp off, on either side, into the correctly rounded root, and leaves the right one alone
static void run_sqrt_fix()
{
    ++runs;
    size_t bad = 0;
    auto check = [&](double x) {
        const double s = sqrt(x);
        unsigned long long u;
        memcpy(&u, &s, 8);
        for (int off = -1; off <= 1; ++off) {
            const unsigned long long v = u + (unsigned long long)(long long)off;
            double cand;
            memcpy(&cand, &v, 8);
            if (!(cand > 0.0) || !isfinite(cand)) continue;
            bad += cb_sqrt_fix(x, cand) != s;
        }
    };
    for (int i = 0; i < 200000; ++i) {
        const unsigned long long m = ((unsigned long long)rnd() << 48) | ((unsigned long long)rnd() << 40) | ((unsigned long long)rnd() << 32) |
                                     ((unsigned long long)rnd() << 24) | (rnd() << 16) | (rnd() << 8) | rnd();
        const unsigned long long e = 1023 - 300 + (rnd() * 600ull) / 255;         // 2^-300 .. 2^300
        const unsigned long long u = (e << 52) | (m & 0xFFFFFFFFFFFFFull);
        double x;
        memcpy(&x, &u, 8);
        check(x);
    }
    for (double x : {1.0, 2.0, 4.0, 0.25, 9.0, 1e-180, 1e300, 4.0 - 0x1p-51, 1.0 + 0x1p-52, 1.0 - 0x1p-53, 0x1p-600, 65025.0 * 65025.0}) check(x);
    for (int k = 1; k < 4000; ++k) { check((double)k * (double)k); check((double)k * (double)k + 0x1p-30); check((double)k / 1024.0); }
    if (cb_sqrt_fix(0.0, 0.0) != 0.0 || cb_sqrt_fix(0x1p-700, 0x1p-350) != 0x1p-350 || !signbit(cb_sqrt_fix(-0.0, -0.0))) ++bad;
    if (bad) { ++failures; printf("MISMATCH sqrt fix: %zu\n", bad); }
}

int main(int argc, char** argv)
{
    const bool quick = argc > 1 && !strcmp(argv[1], "quick");
    run_sqrt_fix();
    run_peak_edges();
    // 256 lanes a workgroup: one cell, a row, one cell short of a block, a block, a block and a cell; then more blocks, long rows, the common map
    struct Grid { int Mx, My; };
    std::vector<Grid> grids = {{1, 1}, {1, 7}, {15, 17}, {16, 16}, {1, 257}};
    if (!quick) grids.insert(grids.end(), {{50, 67}, {3, 1024}, {240, 135}});
    int pick = 0;
    for (const Grid& gr : grids)
        for (int kind = 0; kind < NKINDS; ++kind) {
            const std::vector<std::vector<int>> rows = {{1, 3}, {5, 9}, {3, 1, 5}, {9, 2}};
            run(gr.Mx, gr.My, rows[pick % 4], kind, true, quick);
            if (!quick) run(gr.Mx, gr.My, rows[(pick + 1) % 4], kind, false, quick);
            ++pick;
        }
    return report();
}
