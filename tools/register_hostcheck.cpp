// aefft_frames_register's three kernels without a device: the kernel source itself --
// autoencoder-fft_amd/csrc/register_kernels.hip, the prepare, cross-power and two peak bodies and the size arithmetic -- compiled for the HOST,
// 256 threads as the lanes of a workgroup and a barrier for __syncthreads, under the sanitizers, with the frames, the planes, the spectra, the
// surfaces, the partials, the shifts, the affines and the LDS allocated at exactly their live extent, against a scalar C restatement of
// include/aefft.h's definition: plain loops over signed frequencies for the kept bins and their count, a division by the modulus in double for
// the cross-power, a plain scan for the peak (no keys), the centroid in double.  The transforms are not run: surfaces and spectra are random.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Wno-unknown-pragmas
//       -o register_hostcheck tools/register_hostcheck.cpp   (one line),   then   ./register_hostcheck   (./register_hostcheck quick: a thinned sweep)
//
// A stand-alone program: it is not loaded into Python and does not touch a GPU.  Exit status 0 and "all N runs exact" when every run agrees:
// the planes bit for bit, Q within 1e-5, the kept count, the peak cell (tie rule included), the response's bits and the affine exactly, the
// centroid within 1e-6.
#include "hostlanes.h"
#include "../autoencoder-fft_amd/csrc/register_kernels.hip"

using namespace aefft;

template <class T> static T* exact(size_t n)
{
    void* q = nullptr;
    if (posix_memalign(&q, 16, n ? n * sizeof(T) : 1)) abort();
    return (T*)q;
}
static float from_bits(unsigned u) { float v; memcpy(&v, &u, 4); return v; }
static float unit() { return (float)(int)(rnd() * 256u + rnd()) / 65536.0f; }     // [0, 1)

static void fail_run(const char* what, int Nx, int Ny, int B, int k)
{
    if (failures < 20) printf("FAILED %s: Nx %d Ny %d B %d (%d)\n", what, Nx, Ny, B, k);
}

// ---- prepare ------------------------------------------------------------------------------------
static float ref_window(int n, int N, int window) { return window == RG_HANN ? 0.5f - 0.5f * cosf(6.283185307179586f * (float)n / (float)N) : 1.0f; }

template <int D, bool U8> static void run_prepare(int Nx, int Ny, int B, int window, unsigned nblk)
{
    const size_t n = (size_t)Nx * Ny, nf = (size_t)B * D * n;
    unsigned char* f8 = exact<unsigned char>(U8 ? nf : 0);
    float* f32 = exact<float>(U8 ? 0 : nf);
    float* planes = exact<float>((size_t)B * n);
    for (size_t k = 0; k < nf; ++k) {
        if (U8) f8[k] = (unsigned char)rnd();
        else f32[k] = 255.0f * unit() - 20.0f;
    }
    RgArgs g = RgArgs();
    g.frames = U8 ? (const void*)f8 : (const void*)f32; g.planes = planes; g.B = B; g.D = D; g.Nx = Nx; g.Ny = Ny; g.window = window;
    launch(nblk, 1, 1, window == RG_HANN ? (size_t)(Nx + Ny) : 0, [&](unsigned* lds) { register_prepare_body<D, U8>(g, blockIdx.x, gridDim.x, lds); });
    int bad = 0;
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < Nx; ++i)
            for (int j = 0; j < Ny; ++j) {
                float s = 0.f;
                for (int d = 0; d < D; ++d) {
                    const size_t at = (((size_t)b * D + d) * Nx + i) * Ny + j;
                    s += U8 ? (float)f8[at] : f32[at];
                }
                const float want = window == RG_HANN ? (ref_window(i, Nx, window) * ref_window(j, Ny, window)) * s : s;
                bad += memcmp(&want, &planes[((size_t)b * Nx + i) * Ny + j], 4) != 0;
            }
    ++runs;
    if (bad) { ++failures; fail_run("prepare", Nx, Ny, B, bad); }
    free(f8); free(f32); free(planes);
}

// ---- cross-power --------------------------------------------------------------------------------
static bool ref_kept(int i, int j, int Nx, int Ny, int window, float cutoff)
{
    const int u = i <= Nx / 2 ? i : i - Nx, v = j <= Ny / 2 ? j : j - Ny;         // signed frequencies
    if (!(2.0 * abs(u) <= (double)cutoff * Nx && 2.0 * abs(v) <= (double)cutoff * Ny)) return false;
    return window == RG_HANN ? !(abs(u) <= 1 && abs(v) <= 1) : !(u == 0 && v == 0);
}

static void run_cross(int Nx, int Ny, int B, int nref, int window, float cutoff)
{
    const int Nyr = Ny / 2 + 1;
    const size_t per = (size_t)Nx * Nyr;
    rg_f2* spec = exact<rg_f2>((size_t)B * per);
    rg_f2* ref = exact<rg_f2>((size_t)nref * per);
    std::vector<rg_f2> in((size_t)B * per);
    for (size_t k = 0; k < (size_t)B * per; ++k) {
        const float scale = rnd() < 8 ? 3.0e9f : 100.0f;                          // (moduli whose squares' product would leave the float range)
        spec[k] = rnd() < 16 ? rg_f2{0.f, 0.f} : rg_f2{scale * (unit() - 0.5f), scale * (unit() - 0.5f)};
        in[k] = spec[k];
    }
    for (size_t k = 0; k < (size_t)nref * per; ++k) ref[k] = rnd() < 16 ? rg_f2{0.f, 0.f} : rg_f2{3.0e9f * (unit() - 0.5f), 50.0f * (unit() - 0.5f)};
    RgArgs g = RgArgs();
    g.spec = spec; g.ref = ref; g.nref = nref; g.B = B; g.Nx = Nx; g.Ny = Ny; g.window = window;
    const long long K = rg_kept(Nx, Ny, window, cutoff, &g.umax, &g.vmax, &g.low);
    long long count = 0;
    for (int i = 0; i < Nx; ++i)
        for (int j = 0; j < Ny; ++j) count += ref_kept(i, j, Nx, Ny, window, cutoff);
    const unsigned bpi = (unsigned)((per + RG_LANES - 1) / RG_LANES);
    launch((unsigned)B * bpi, 1, 1, 0, [&](unsigned*) { register_cross_body(g, blockIdx.x, bpi); });
    int bad = K != count;
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < Nx; ++i)
            for (int j = 0; j < Nyr; ++j) {
                const size_t at = (size_t)b * per + (size_t)i * Nyr + j;
                const rg_f2 a = in[at], r = ref[(nref == 1 ? 0 : (size_t)b * per) + (size_t)i * Nyr + j];
                const double rx = (double)a.x * r.x + (double)a.y * r.y, ry = (double)a.y * r.x - (double)a.x * r.y, m = sqrt(rx * rx + ry * ry);
                double qx = 0.0, qy = 0.0;
                if (ref_kept(i, j, Nx, Ny, window, cutoff) && m > 0.0) { qx = rx / m; qy = ry / m; }
                bad += !(fabs(spec[at].x - qx) <= 1e-5 && fabs(spec[at].y - qy) <= 1e-5);
            }
    ++runs;
    if (bad) { ++failures; fail_run("cross", Nx, Ny, B, bad); }
    free(spec); free(ref);
}

// ---- peak ---------------------------------------------------------------------------------------
// kind 0: smooth random values; 1: a few levels only (ties everywhere); 2: with NaN, -0 and infinities; 3: NaN only
static void run_peak(int Nx, int Ny, int B, int kind, bool with_affine, float min_response, double sx, double sy)
{
    const size_t n = (size_t)Nx * Ny;
    const int nparts = rg_parts(Nx, Ny);
    float* surf = exact<float>((size_t)B * n);
    rg_u64* part = exact<rg_u64>((size_t)B * nparts);
    RgShift* shift = exact<RgShift>(B);
    RgAffine* aff = exact<RgAffine>(with_affine ? B : 0);
    for (size_t k = 0; k < (size_t)B * n; ++k) {
        float v = kind == 1 ? (float)(rnd() & 3) * 0.25f - 0.25f : 2.0f * unit() - 1.2f;
        if (kind == 2 && rnd() < 40) { const unsigned odd[4] = {0x7FC00000u, 0x80000000u, 0xFF800000u, 0xFFC00001u}; v = from_bits(odd[rnd() & 3]); }
        if (kind == 3) v = from_bits(0x7FC00000u);
        surf[k] = v;
    }
    RgArgs g = RgArgs();
    g.surf = surf; g.part = part; g.shift = shift; g.affine = with_affine ? aff : nullptr; g.B = B; g.Nx = Nx; g.Ny = Ny; g.nparts = nparts;
    g.min_response = min_response; g.sx = sx; g.sy = sy;
    launch((unsigned)(B * nparts), 1, 1, RG_PEAK_WORDS, [&](unsigned* lds) { register_peak1_body(g, blockIdx.x, lds); });
    launch((unsigned)B, 1, 1, RG_PEAK_WORDS, [&](unsigned* lds) { register_peak2_body(g, blockIdx.x, lds); });
    int bad = 0;
    for (int b = 0; b < B; ++b) {
        const float* s = surf + (size_t)b * n;
        int cell = 0; bool any = false;
        for (size_t p = 0; p < n; ++p)
            if (!isnan(s[p]) && (!any || s[p] > s[cell])) { cell = (int)p; any = true; }      // (strictly larger: the first of equals stays; -0 == +0)
        const int pi = cell / Ny, pj = cell % Ny;
        double sw = 0, si = 0, sj = 0;
        for (int di = -2; di <= 2; ++di)
            for (int dj = -2; dj <= 2; ++dj) {
                const float v = s[((pi + di + Nx) % Nx) * Ny + (pj + dj + Ny) % Ny];
                const double w = v > 0.f ? (double)v : 0.0;
                sw += w; si += w * di; sj += w * dj;
            }
        double dx = pi + (sw > 0 ? si / sw : 0.0), dy = pj + (sw > 0 ? sj / sw : 0.0);
        if (dx >= Nx / 2) dx -= Nx;
        if (dy >= Ny / 2) dy -= Ny;
        const RgShift o = shift[b];
        bad += o.cell != cell || memcmp(&o.response, &s[cell], 4) != 0 || !(fabs(o.dx - dx) <= 1e-6 * (1.0 + fabs(dx))) || !(fabs(o.dy - dy) <= 1e-6 * (1.0 + fabs(dy)));
        bad += o.cell < 0 || o.cell >= (int)n;
        if (with_affine) {
            long long want[6] = {16777216, 0, 0, 0, 16777216, 0};
            if (o.response >= min_response) {
                want[2] = (long long)nearbyint((double)o.dx * sx * 16777216.0);
                want[5] = (long long)nearbyint((double)o.dy * sy * 16777216.0);
            }
            bad += memcmp(want, aff[b].a, 48) != 0;
        }
    }
    ++runs;
    if (bad) { ++failures; fail_run("peak", Nx, Ny, B, bad); }
    free(surf); free(part); free(shift); free(aff);
}

int main(int argc, char** argv)
{
    const bool quick = argc > 1 && !strcmp(argv[1], "quick");
    // (12, 10) and (10, 12): a quad of the prepare straddles a row pair's two rows when Ny = 2 mod 4; (96, 128): three stage-one workgroups
    const int grids[][2] = {{16, 16}, {32, 8}, {12, 10}, {48, 40}, {10, 12}, {64, 64}, {96, 128}, {8, 2048}};
    const int ngrids = quick ? 4 : 8;
    for (int gi = 0; gi < ngrids; ++gi) {
        const int Nx = grids[gi][0], Ny = grids[gi][1];
        if (!rg_size(Nx) || !rg_size(Ny) || !rg_workspace(Nx, Ny, 3)) { ++runs; ++failures; continue; }
        for (int B = 1; B <= 3; B += 2) {
            for (int window = 0; window < 2; ++window) {
                const unsigned nblk = 1 + rnd() % 3;                              // (fewer workgroups than passes: the grid stride runs)
                run_prepare<1, true>(Nx, Ny, B, window, nblk); run_prepare<3, false>(Nx, Ny, B, window, nblk);
                if (!quick || gi == 2) {
                    run_prepare<2, true>(Nx, Ny, B, window, nblk); run_prepare<3, true>(Nx, Ny, B, window, nblk); run_prepare<4, true>(Nx, Ny, B, window, nblk);
                    run_prepare<1, false>(Nx, Ny, B, window, nblk); run_prepare<2, false>(Nx, Ny, B, window, nblk); run_prepare<4, false>(Nx, Ny, B, window, nblk);
                }
                const float cutoffs[] = {1.0f, 0.5f, 0.3f, 0.07f};
                for (int c = 0; c < (quick ? 2 : 4); ++c) {
                    int um, vm, lw;
                    if (rg_kept(Nx, Ny, window, cutoffs[c], &um, &vm, &lw) <= 0) continue;
                    run_cross(Nx, Ny, B, 1, window, cutoffs[c]);
                    run_cross(Nx, Ny, B, B, window, cutoffs[c]);
                }
            }
            for (int kind = 0; kind < 4; ++kind)
                for (int rep = 0; rep < (quick ? 1 : 4); ++rep) {
                    run_peak(Nx, Ny, B, kind, false, 0.f, 1.0, 1.0);
                    run_peak(Nx, Ny, B, kind, true, rep & 1 ? 0.6f : -10.0f, rep & 2 ? 2.0 : 1.0, rep & 2 ? 1.5 : 32.0);
                }
        }
    }
    // the size arithmetic at its limits
    int um, vm, lw;
    const bool sizes = !rg_size(6) && rg_size(8) && rg_size(10) && !rg_size(14) && rg_size(2048) && !rg_size(2050) && !rg_size(15) && rg_workspace(16, 16, 1) == 1024 + 1152 + 16 &&
                       !rg_workspace(2048, 2048, 128) && rg_kept(16, 16, RG_HANN, 1.0f, &um, &vm, &lw) == 247 && rg_kept(16, 16, RG_NOWINDOW, 0.01f, &um, &vm, &lw) == 0 &&
                       rg_kept(16, 16, RG_HANN, 0.0f, &um, &vm, &lw) < 0 && rg_kept(16, 16, RG_HANN, from_bits(0x7FC00000u), &um, &vm, &lw) < 0 &&
                       rg_kept(16, 16, RG_HANN, 1.5f, &um, &vm, &lw) < 0;
    ++runs;
    if (!sizes) { ++failures; printf("FAILED sizes\n"); }
    return report();
}
