// C-ABI layer (include/aefft.h), registration: aefft_frames_register_ref and aefft_frames_register -- translation by phase correlation on the
// library's own transforms.  Host code only: the calls check their arguments, join a deferred reconstruction and chain the launchers of
// register_kernels.hip with do_r2c / do_c2r.  A unit of its own because it is the one image-boundary call that takes the context's transform
// workspace (image_ops.hip takes none).
#include "host.h"
#include <climits>
#include <cmath>

using namespace aefft;

namespace {
// a rejection is AEFFT_EINVAL with "<call>: <rule>" as the context's last error; nothing is enqueued
struct Reject {
    aefft_ctx* ctx; const char* fn;
    int operator()(const char* rule) const { return fail(ctx, AEFFT_EINVAL, (std::string(fn) + ": " + rule).c_str()); }
};
struct Range { const void* p; size_t n; bool out; };
bool meet(const Range& a, const Range& b)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a.p), b0 = reinterpret_cast<uintptr_t>(b.p);
    return a.n && b.n && a0 < b0 + b.n && b0 < a0 + a.n;
}
// no output meets an input or another output (a null pointer has no range)
bool outputs_clear(const Range* r, int n)
{
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
            if ((r[i].out || r[j].out) && r[i].p && r[j].p && meet(r[i], r[j])) return false;
    return true;
}
// the rules the two calls share: the frames, the grid, the window and the workspace; `need`, `spec_at`, `part_at` receive the workspace's layout
int chk_register(const Reject& bad, const void* frames_d, int count, const char* count_rule, int D, int Nx, int Ny, int window, const void* work_d,
                 size_t work_bytes, size_t* need, size_t* spec_at, size_t* part_at)
{
    if (D < 1 || D > 4) return bad("D must be 1..4");
    if (!net_size(Nx) || !net_size(Ny)) return bad("Nx, Ny must be powers of two in 8..2048, or even sizes in 10..2048 with no prime factor above 5");
    if (count < 1 || (long long)count * Nx * Ny >= (1LL << 29)) return bad(count_rule);
    if (window != AEFFT_REGISTER_HANN && window != AEFFT_REGISTER_NOWINDOW) return bad("window must be AEFFT_REGISTER_HANN or AEFFT_REGISTER_NOWINDOW");
    if (!aligned16(frames_d) || !aligned16(work_d)) return bad("frames_d, the spectra, the outputs and work_d must be 16-byte aligned");
    *need = register_workspace(Nx, Ny, count, spec_at, part_at);
    if (!*need || work_bytes < *need) return bad("work_bytes is below aefft_register_workspace(Nx, Ny, B) (nref for B in aefft_frames_register_ref)");
    return AEFFT_OK;
}
}  // namespace

extern "C" size_t aefft_register_spec_floats(int Nx, int Ny) { return net_size(Nx) && net_size(Ny) ? (size_t)2 * Nx * (Ny / 2 + 1) : 0; }
extern "C" size_t aefft_register_workspace(int Nx, int Ny, int B) { return register_workspace(Nx, Ny, B); }

extern "C" int aefft_frames_register_ref(aefft_ctx* ctx, const void* frames_d, int frames_u8, int nref, int D, int Nx, int Ny, int window, float* spec_d,
                                         void* work_d, size_t work_bytes)
{
    const Reject bad{ctx, "aefft_frames_register_ref"};
    if (!ctx || !frames_d || !spec_d || !work_d) return bad("null context, frames, spectra or workspace");
    size_t need = 0, spec_at = 0, part_at = 0;
    RET_IF(chk_register(bad, frames_d, nref, "nref must be >= 1 and nref * Nx * Ny below 2^29", D, Nx, Ny, window, work_d, work_bytes, &need, &spec_at, &part_at));
    if (!aligned16(spec_d)) return bad("frames_d, the spectra, the outputs and work_d must be 16-byte aligned");
    const size_t cells = (size_t)Nx * Ny, fb = (size_t)nref * D * cells * (frames_u8 ? 1 : 4), sb = (size_t)nref * bins(Nx, Ny) * 8;
    const Range r[3] = {{frames_d, fb, false}, {spec_d, sb, true}, {work_d, need, true}};
    if (!outputs_clear(r, 3)) return bad("the spectra and the workspace overlap the frames or each other");
    RET_IF(join_recon(ctx));                          // (frames_d may be a reconstruction that is still on the side stream)
    float* planes = static_cast<float*>(work_d);
    RET_IF(launch_or_fail(ctx, KID_IMAGE, (double)fb + 4.0 * nref * cells, "register_prepare",
                          [&] { return launch_register_prepare(frames_d, frames_u8, planes, nref, D, Nx, Ny, window, ctx->cur); }));
    return do_r2c(ctx, planes, F2(spec_d), nref, Nx, Ny, Nx, Ny);
}

extern "C" int aefft_frames_register(aefft_ctx* ctx, const void* frames_d, int frames_u8, int B, int D, int Nx, int Ny, int window, const float* ref_spec_d,
                                     int nref, float cutoff, float min_response, double scale_x, double scale_y, aefft_shift* shift_d, aefft_affine* affine_d,
                                     void* work_d, size_t work_bytes)
{
    const Reject bad{ctx, "aefft_frames_register"};
    if (!ctx || !frames_d || !ref_spec_d || !shift_d || !work_d) return bad("null context, frames, reference spectra, shifts or workspace");
    size_t need = 0, spec_at = 0, part_at = 0;
    RET_IF(chk_register(bad, frames_d, B, "B must be >= 1 and B * Nx * Ny below 2^29", D, Nx, Ny, window, work_d, work_bytes, &need, &spec_at, &part_at));
    if (nref != 1 && nref != B) return bad("nref must be 1 (one reference for the batch) or B (one per image)");
    int umax = 0, vmax = 0, low = 0;
    const long long K = register_kept(Nx, Ny, window, cutoff, &umax, &vmax, &low);
    if (K < 0) return bad("cutoff must be in (0, 1]");
    if (K == 0) return bad("the cutoff keeps no bin (K = 0)");
    if (!(scale_x > 0.0) || !(scale_x <= 32.0) || !(scale_y > 0.0) || !(scale_y <= 32.0)) return bad("scale_x and scale_y must be in (0, 32]");
    if (!aligned16(ref_spec_d) || !aligned16(shift_d) || !aligned16(affine_d)) return bad("frames_d, the spectra, the outputs and work_d must be 16-byte aligned");
    const size_t cells = (size_t)Nx * Ny, fb = (size_t)B * D * cells * (frames_u8 ? 1 : 4), sb = (size_t)bins(Nx, Ny) * 8;
    const Range r[5] = {{frames_d, fb, false}, {ref_spec_d, (size_t)nref * sb, false}, {shift_d, (size_t)B * sizeof(aefft_shift), true},
                        {affine_d, (size_t)B * sizeof(aefft_affine), true}, {work_d, need, true}};
    if (!outputs_clear(r, 5)) return bad("the shifts, the affines and the workspace overlap an input or each other");
    RET_IF(join_recon(ctx));                          // (frames_d may be a reconstruction that is still on the side stream)
    unsigned char* work = static_cast<unsigned char*>(work_d);
    float* planes = reinterpret_cast<float*>(work);                              // the windowed planes, later the surface
    float2* spec = reinterpret_cast<float2*>(work + spec_at);
    RET_IF(launch_or_fail(ctx, KID_IMAGE, (double)fb + 4.0 * B * cells, "register_prepare",
                          [&] { return launch_register_prepare(frames_d, frames_u8, planes, B, D, Nx, Ny, window, ctx->cur); }));
    RET_IF(do_r2c(ctx, planes, spec, B, Nx, Ny, Nx, Ny));
    RET_IF(launch_or_fail(ctx, KID_IMAGE, (double)sb * (2.0 * B + nref), "register_cross",
                          [&] { return launch_register_cross(spec, CF2(ref_spec_d), nref, B, Nx, Ny, window, umax, vmax, low, ctx->cur); }));
    RET_IF(do_c2r(ctx, spec, planes, B, Nx, Ny, Nx, Ny, (float)(1.0 / (double)K)));
    return launch_or_fail(ctx, KID_IMAGE, 4.0 * B * cells + B * (16.0 + (affine_d ? 48.0 : 0.0)), "register_peak", [&] {
        return launch_register_peak(planes, work + part_at, B, Nx, Ny, min_response, scale_x, scale_y, shift_d, affine_d, ctx->cur);
    });
}
