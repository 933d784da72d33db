// C-ABI layer (include/aefft.h), the read-outs of the frozen-weight reconstruction: aefft_net_score, aefft_net_score_map, aefft_net_ssim_map and
// the _target variants of the first two.  Each is aefft_net_infer's forward with a ScoreArg handed to the reconstruction's row pass (or, where the
// reconstruction does not come out of a row pass, a *_diff launch on the stored one) and a finish; they differ in the ReadOut they describe.
#include "net.h"

#include <cmath>
#include <initializer_list>
#include <string>

using namespace aefft;

// One read-out.  arg.tile and arg.ssim say which of the three kinds it is; the buffer the sums go to is filled in by readout_sums.
struct ReadOut {
    const char* who;        // the entry point, for messages
    const char* noun;       // what the refusals say is formed from the stored reconstruction: "score" or "map"
    int kid;                // profiler id of the kind's own launches
    ScoreArg arg;           // handed to launch_recon: the pixels the reconstruction is compared with -- the frames themselves or a target of the
                            // same shape -- and the tile, SSIM's flag and pivot
    float L;                // SSIM: data_range
    float *map_d, *score_d; // the call's outputs (score_d optional beside a map; map_d null for aefft_net_score)
};

// Where the row pass (or the diff launch) leaves its sums: the net's buffer of the read-out's kind.  The first SSIM call of a net allocates its
// strip buffer, behind the refusals: not under stream capture, include/aefft.h.
static int readout_sums(aefft_net* n, ScoreArg& a)
{
    if (!a.tile) { a.part = n->score_part; return AEFFT_OK; }
    a.strips = n->map_part;
    if (!a.ssim) return AEFFT_OK;
    if (!n->ssim_part) RET_IF(net_alloc_t(n, &n->ssim_part, (size_t)SSIM_MOMENTS * score_map_strips(n)));
    a.strips = n->ssim_part;
    return AEFFT_OK;
}

// the same sums from the STORED float reconstruction (routes whose reconstruction does not come out of one of the two row kernels)
static int readout_diff(aefft_net* n, const ReadOut& r, const float* recon_d)
{
    aefft_ctx* ctx = n->ctx;
    const ScoreArg& a = r.arg;
    const long npairs = (long)n->B * n->D * n->Nx / 2;
    return launch_or_fail(ctx, r.kid, (double)n->B * n->D * n->Nx * n->Ny * 8.0, !a.tile ? "score_diff" : a.ssim ? "ssim_diff" : "score_map_diff", [&] {
        if (!a.tile) return launch_score_diff(a.frames, false, recon_d, a.part, n->B, (long)n->D * n->Nx, n->Ny, ctx->cur);
        return a.ssim ? launch_ssim_diff(a.frames, false, recon_d, a.strips, npairs, n->Ny, a.tile, a.pivot, ctx->cur)
                      : launch_score_map_diff(a.frames, false, recon_d, a.strips, npairs, n->Ny, a.tile, ctx->cur);
    });
}

// The finish.  Score: a frame's row-pair partials added up (score_finish_kernel), score_d[b] = sum / (D Nx Ny).  Map and SSIM: the strips made
// into the map (score_map_finish_kernel / ssim_finish_kernel), then, when asked for, a frame's map entries averaged (score_finish_kernel with the
// map as the partials).
static int readout_finish(aefft_net* n, const ReadOut& r)
{
    aefft_ctx* ctx = n->ctx;
    const ScoreArg& a = r.arg;
    if (!a.tile) {
        const long npf = score_pairs_per_frame(n);
        return launch_or_fail(ctx, KID_SCORE, (double)n->B * (npf + 1) * 4.0, "score_finish",
                              [&] { return launch_score_finish(a.part, r.score_d, n->B, npf, 1.0 / ((double)n->D * n->Nx * n->Ny), ctx->cur); });
    }
    const int tile = a.tile;
    const long epf = (long)(n->Nx / tile) * (n->Ny / tile);        // map entries per frame
    if (a.ssim) {
        const double px = (double)n->B * n->D * n->Nx * n->Ny;
        RET_IF(launch_or_fail(ctx, KID_SSIM, (SSIM_MOMENTS * px / 2 / tile + (double)n->B * epf) * 4.0, "ssim_finish",
                              [&] { return launch_ssim_finish(a.strips, r.map_d, n->B, n->D, n->Nx, n->Ny, tile, r.L, a.pivot, ctx->cur); }));
    } else {
        RET_IF(launch_or_fail(ctx, KID_SCORE_MAP, ((double)n->B * n->D * n->Nx / 2 * (n->Ny / tile) + (double)n->B * epf) * 4.0, "score_map_finish",
                              [&] { return launch_score_map_finish(a.strips, r.map_d, n->B, n->D, n->Nx, n->Ny, tile, ctx->cur); }));
    }
    if (!r.score_d) return AEFFT_OK;
    return launch_or_fail(ctx, KID_SCORE, (double)n->B * (epf + 1) * 4.0, "score_finish",
                          [&] { return launch_score_finish(r.map_d, r.score_d, n->B, epf, 1.0 / (double)epf, ctx->cur); });
}

// aefft_net_infer's body with the read-out's argument handed to the reconstruction, then the finish launch.  The net reads frames_d.
static int readout_body(aefft_net* n, ReadOut r, const void* frames_d, bool frames_u8, float* recon_d)
{
    aefft_ctx* ctx = n->ctx;
    const std::string w(r.who), noun(r.noun);
    if (n->spatial) {
        if (frames_u8 || r.arg.u8) return sp_refuse(n, (w + " with 8-bit frames").c_str());
        if (!recon_d) return fail(ctx, AEFFT_EINVAL, (w + ": a spatial net's reconstruction is written by its last convolution, not by an inverse transform's row pass -- the " + noun + " is formed from the stored reconstruction, so recon_d must be given").c_str());
        RET_IF(readout_sums(n, r.arg));
        RET_IF(sp_forward(n, static_cast<const float*>(frames_d), recon_d));
        RET_IF(readout_diff(n, r, recon_d));
        RET_IF(readout_finish(n, r));
        return mark_step_point(n);
    }
    if (!recon_d && !c2r_scores_in_rows(n->Nx, n->Ny))
        return fail(ctx, AEFFT_EINVAL, (w + ": under AEFFT_F_CHIRPZ this grid's reconstruction comes out of the chirp-z transforms, not of an inverse row pass -- the " + noun + " is formed from the stored reconstruction, so recon_d must be given").c_str());
    RET_IF(readout_sums(n, r.arg));
    const bool op = op_eligible(n);
    RET_IF(net_forward(n, static_cast<const float*>(frames_d), frames_u8, nullptr, true, op, true));
    RET_IF(launch_recon(n, recon_d, WS_MID, false, &r.arg));
    RET_IF(readout_finish(n, r));
    return mark_step_point(n);
}

// The entry points' argument checks, in the order of their messages: the net; the pointers the call cannot do without (`missing`; `needed` names
// them); 16-byte alignment of every pointer, optional ones included (null passes); the tile (null: the call has none).
static int readout_args(aefft_net* n, const char* who, bool missing, const char* needed, std::initializer_list<const void*> ptrs, const int* tile)
{
    if (!n) return AEFFT_EINVAL;
    aefft_ctx* ctx = n->ctx;
    const std::string w(who);
    if (missing) return fail(ctx, AEFFT_EINVAL, (w + ": null " + needed).c_str());
    for (const void* p : ptrs)
        if (!aligned16p(p)) return fail(ctx, AEFFT_EINVAL, (w + ": pointers must be 16-byte aligned").c_str());
    if (tile && !(score_tile_log2(*tile) >= 0 && n->Nx % *tile == 0 && n->Ny % *tile == 0))
        return fail(ctx, AEFFT_EINVAL, (w + ": tile must be 8, 16, 32 or 64 and divide both Nx and Ny").c_str());
    return AEFFT_OK;
}

// ------------------------------------------------------------------------------------------
// per-frame reconstruction error (include/aefft.h aefft_net_score)
// ------------------------------------------------------------------------------------------
extern "C" int aefft_net_score(aefft_net* n, const void* frames_d, int frames_u8, float* score_d, float* recon_d)
{
    RET_IF(readout_args(n, "aefft_net_score", !frames_d || !score_d, "frames or score", {frames_d, score_d, recon_d}, nullptr));
    return readout_body(n, ReadOut{"aefft_net_score", "score", KID_SCORE, ScoreArg{frames_d, frames_u8 != 0, nullptr}, 0.f, nullptr, score_d}, frames_d, frames_u8 != 0, recon_d);
}

extern "C" int aefft_net_score_target(aefft_net* n, const void* frames_d, int frames_u8, const void* targets_d, int targets_u8, float* score_d, float* recon_d)
{
    RET_IF(readout_args(n, "aefft_net_score_target", !frames_d || !targets_d || !score_d, "frames, targets or score", {frames_d, targets_d, score_d, recon_d}, nullptr));
    return readout_body(n, ReadOut{"aefft_net_score_target", "score", KID_SCORE, ScoreArg{targets_d, targets_u8 != 0, nullptr}, 0.f, nullptr, score_d}, frames_d, frames_u8 != 0, recon_d);
}

// ------------------------------------------------------------------------------------------
// per-tile reconstruction error (include/aefft.h aefft_net_score_map): the tile in the score argument, the row pass leaves strips
// ------------------------------------------------------------------------------------------
extern "C" int aefft_net_score_map(aefft_net* n, const void* frames_d, int frames_u8, int tile, float* map_d, float* score_d, float* recon_d)
{
    RET_IF(readout_args(n, "aefft_net_score_map", !frames_d || !map_d, "frames or map", {frames_d, map_d, score_d, recon_d}, &tile));
    return readout_body(n, ReadOut{"aefft_net_score_map", "map", KID_SCORE_MAP, ScoreArg{frames_d, frames_u8 != 0, nullptr, tile}, 0.f, map_d, score_d}, frames_d, frames_u8 != 0, recon_d);
}

extern "C" int aefft_net_score_map_target(aefft_net* n, const void* frames_d, int frames_u8, const void* targets_d, int targets_u8, int tile, float* map_d,
                                          float* score_d, float* recon_d)
{
    RET_IF(readout_args(n, "aefft_net_score_map_target", !frames_d || !targets_d || !map_d, "frames, targets or map", {frames_d, targets_d, map_d, score_d, recon_d}, &tile));
    return readout_body(n, ReadOut{"aefft_net_score_map_target", "map", KID_SCORE_MAP, ScoreArg{targets_d, targets_u8 != 0, nullptr, tile}, 0.f, map_d, score_d}, frames_d, frames_u8 != 0, recon_d);
}

// ------------------------------------------------------------------------------------------
// block SSIM of the reconstruction (include/aefft.h aefft_net_ssim_map): five sums per strip, pivot = data_range / 2
// ------------------------------------------------------------------------------------------
extern "C" int aefft_net_ssim_map(aefft_net* n, const void* frames_d, int frames_u8, const void* targets_d, int targets_u8, int tile, float data_range,
                                  float* map_d, float* score_d, float* recon_d)
{
    RET_IF(readout_args(n, "aefft_net_ssim_map", !frames_d || !map_d, "frames or map", {frames_d, targets_d, map_d, score_d, recon_d}, &tile));
    if (!std::isfinite(data_range) || !(data_range > 0.f)) return fail(n->ctx, AEFFT_EINVAL, "aefft_net_ssim_map: data_range must be finite and greater than 0 (255 for 8-bit images)");
    const void* ref = targets_d ? targets_d : frames_d;
    const bool ref_u8 = targets_d ? targets_u8 != 0 : frames_u8 != 0;
    return readout_body(n, ReadOut{"aefft_net_ssim_map", "map", KID_SSIM, ScoreArg{ref, ref_u8, nullptr, tile, nullptr, true, 0.5f * data_range}, data_range, map_d, score_d},
                        frames_d, frames_u8 != 0, recon_d);
}
