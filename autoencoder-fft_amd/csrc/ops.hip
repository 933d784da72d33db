// C-ABI layer (include/aefft.h), op level: the internal op helpers -- transform routes and size checks, contractions and their
// descriptors, the gradient, the kernel-support transforms, the update -- which the network units (net.hip, net_step.hip) build on,
// and the op-level and spatial entry points.  (The image-boundary entry points are in image_ops.hip.)
#include "host.h"

#include <algorithm>
#include <cmath>

using namespace aefft;

// ------------------------------------------------------------------------------------------
// internal op helpers (all enqueue on ctx->cur)
// ------------------------------------------------------------------------------------------
long aefft::bins(int Nx, int Ny) { return (long)Nx * (Ny / 2 + 1); }

int aefft::chk_size(aefft_ctx* ctx, int Nx, int Ny)
{
    if (!fft_size_supported(Nx) || !fft_size_supported(Ny)) return fail(ctx, AEFFT_EINVAL, "Nx, Ny must be powers of two in 8..2048");
    return AEFFT_OK;
}

static int chk_size_any(aefft_ctx* ctx, int Nx, int Ny)
{
    if ((fft_size_supported(Nx) && fft_size_supported(Ny)) || (fft_size_supported_any(Nx) && fft_size_supported_any(Ny) && Nx <= 1024 && Ny <= 1024)) return AEFFT_OK;
    return fail(ctx, AEFFT_EINVAL, "Nx, Ny must be powers of two in 8..2048, or even sizes in 8..1024");
}
static bool pow2_sizes(int Nx, int Ny) { return fft_size_supported(Nx) && fft_size_supported(Ny); }
// the per-bin ops and the network: powers of two, or smooth sizes (even, 10..2048, no prime factor above 5) on the mixed-radix transforms
bool aefft::net_size(int n) { return fft_size_supported(n) || fft_size_smooth(n); }
static int chk_size_smooth(aefft_ctx* ctx, int Nx, int Ny)
{
    if (!net_size(Nx) || !net_size(Ny)) return fail(ctx, AEFFT_EINVAL, "Nx, Ny must be powers of two in 8..2048, or even sizes in 10..2048 with no prime factor above 5");
    return AEFFT_OK;
}
// the transforms take the mixed-radix passes (fft_mixed_kernels.hip) on grids with a smooth axis whose other axis has no prime factor above 5
// either, unless AEFFT_F_CHIRPZ sends sizes Bluestein serves (<= 1024) there.  A power-of-two grid keeps its routes whatever the crop / pad:
// the power-of-two passes, or Bluestein + resize for a crop to a size that is not a power of two (op-level pooling by 3, 5, ...)
static bool mixed_route(int Nx, int Ny)
{
    return (fft_size_smooth(Nx) || fft_size_smooth(Ny)) && fft_size_mixed(Nx) && fft_size_mixed(Ny) && !(flag(AEFFT_F_CHIRPZ) && Nx <= 1024 && Ny <= 1024);
}

// sizes that are not powers of two (fft_backproplib.cu:773-779: cufftPlanMany takes any): Bluestein rows + transposes (fft_kernels.hip);
// the spectral crop / zero-pad as a separate resize
static int do_r2c_any(aefft_ctx* ctx, const float* x, float2* X, long planes, int Nx, int Ny, int Nxs, int Nys)
{
    const size_t el = fft_any_ws_elems(planes, Nx, Ny);
    void *w1, *w2, *w3 = nullptr;
    RET_IF(ws_get(ctx, WS_MID, sizeof(float2) * el, &w1));
    RET_IF(ws_get(ctx, WS_MID2, sizeof(float2) * el, &w2));
    const bool crop = Nxs != Nx || Nys != Ny;
    if (crop) RET_IF(ws_get(ctx, WS_MID3, sizeof(float2) * el, &w3));
    {
        Bracket br(ctx, KID_R2C_ROWS, (double)planes * ((double)Nx * Ny * 4.0 + (double)bins(Nx, Ny) * 8.0));
        hipError_t e = launch_r2c_any(x, crop ? (float2*)w3 : X, (float2*)w1, (float2*)w2, planes, Nx, Ny, ctx->cur);
        if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "r2c (any size)", e);
    }
    return crop ? do_resize(ctx, (const float2*)w3, X, planes, Nx, Ny, Nxs, Nys) : AEFFT_OK;
}
static int do_c2r_any(aefft_ctx* ctx, const float2* X, float* x, long planes, int Nxi, int Nyi, int Nx, int Ny, float scale)
{
    const size_t el = fft_any_ws_elems(planes, Nx, Ny);
    void *w1, *w2, *w3 = nullptr;
    RET_IF(ws_get(ctx, WS_MID, sizeof(float2) * el, &w1));
    RET_IF(ws_get(ctx, WS_MID2, sizeof(float2) * el, &w2));
    const bool pad = Nxi != Nx || Nyi != Ny;
    if (pad) {
        RET_IF(ws_get(ctx, WS_MID3, sizeof(float2) * el, &w3));
        RET_IF(do_resize(ctx, X, (float2*)w3, planes, Nxi, Nyi, Nx, Ny));
    }
    Bracket br(ctx, KID_C2R_ROWS, (double)planes * ((double)Nx * Ny * 4.0 + (double)bins(Nx, Ny) * 8.0));
    hipError_t e = launch_c2r_any(pad ? (const float2*)w3 : X, x, (float2*)w1, (float2*)w2, planes, Nx, Ny, scale, ctx->cur);
    if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "c2r (any size)", e);
    return AEFFT_OK;
}

// R2C (+ fused crop to Nxs x Nys).  The two kernels are bracketed separately for profiling.
// u8: x holds 8-bit pixels (the frame transforms of aefft_net_step_grad_u8 / aefft_net_forward_u8 only; every other transform reads floats)
int aefft::do_r2c(aefft_ctx* ctx, const float* x, float2* X, long planes, int Nx, int Ny, int Nxs, int Nys, int ws_id, hipEvent_t done, bool u8)
{
    if ((!pow2_sizes(Nx, Ny) || !pow2_sizes(Nxs, Nys)) && !mixed_route(Nx, Ny)) {
        if (u8) return fail(ctx, AEFFT_EINVAL, "r2c: 8-bit frames need power-of-two sizes");
        RET_IF(chk_size_any(ctx, Nx, Ny));
        if (Nx > 1024 || Ny > 1024) return fail(ctx, AEFFT_EINVAL, "r2c: a crop to a size that is not a power of two needs a grid of at most 1024 x 1024");
        if (!aligned16(x) || !aligned16(X)) return fail(ctx, AEFFT_EINVAL, "r2c: pointers must be 16-byte aligned");
        return do_r2c_any(ctx, x, X, planes, Nx, Ny, Nxs, Nys);
    }
    if (!aligned16(x) || !aligned16(X)) return fail(ctx, AEFFT_EINVAL, "r2c: pointers must be 16-byte aligned");
    if (Nxs > Nx || Nys > Ny || Nxs < 2 || Nys < 2 || (Nxs & 1) || (Nys & 1)) return fail(ctx, AEFFT_EINVAL, "r2c: cropped size must be even and inside the grid");
    void* mid;
    RET_IF(ws_get(ctx, ws_id, sizeof(float2) * fft_mid_elems(planes, Nx, Nys / 2), &mid));
    // launch_r2c issues rows then cols; bracket as two launches by splitting the byte accounting:
    // rows: read planes*Nx*Ny*4, write mid; cols: read mid, write out.
    const double b_in = (double)planes * Nx * Ny * (u8 ? 1 : 4), b_mid = (double)planes * Nx * (Nys / 2) * 8, b_out = (double)planes * bins(Nxs, Nys) * 8;
    hipError_t e;
    {
        // The row and column kernels are launched inside launch_r2c; to time them separately we call it in two halves.
        Bracket br(ctx, KID_R2C_ROWS, b_in + b_mid);
        e = launch_r2c(x, nullptr, (float2*)mid, planes, Nx, Ny, Nxs, Nys, ctx->cur, nullptr, u8);
    }
    if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "r2c rows", e);
    {
        Bracket br(ctx, KID_R2C_COLS, b_mid + b_out);
        e = launch_r2c(nullptr, X, (float2*)mid, planes, Nx, Ny, Nxs, Nys, ctx->cur, done);
    }
    if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "r2c cols", e);
    return AEFFT_OK;
}

// (every pair's grid of a net on a power-of-two frame grid is a power of two: the frame grid decides)
bool aefft::c2r_scores_in_rows(int Nx, int Ny) { return pow2_sizes(Nx, Ny) || mixed_route(Nx, Ny); }

int aefft::do_c2r(aefft_ctx* ctx, const float2* X, void* x, long planes, int Nxi, int Nyi, int Nx, int Ny, float scale, int ws_id, const OpIn* opin,
                  bool out_u8, const ScoreArg* score)
{
    if (score && out_u8) return fail(ctx, AEFFT_EINVAL, "c2r: the scoring row pass writes no 8-bit pixels");
    if (!opin && (!pow2_sizes(Nx, Ny) || !pow2_sizes(Nxi, Nyi)) && !mixed_route(Nx, Ny)) {
        if (out_u8) return fail(ctx, AEFFT_EINVAL, "c2r: 8-bit output needs a power-of-two or smooth grid");
        if (score && !x) return fail(ctx, AEFFT_EINVAL, "c2r: on the any-size route the score is formed from the stored reconstruction, which was not asked for");
        RET_IF(chk_size_any(ctx, Nx, Ny));
        if (Nx > 1024 || Ny > 1024) return fail(ctx, AEFFT_EINVAL, "c2r: a zero-pad from a size that is not a power of two needs a grid of at most 1024 x 1024");
        if (!aligned16(x) || !aligned16(X)) return fail(ctx, AEFFT_EINVAL, "c2r: pointers must be 16-byte aligned");
        RET_IF(do_c2r_any(ctx, X, static_cast<float*>(x), planes, Nxi, Nyi, Nx, Ny, scale));
        if (!score) return AEFFT_OK;
        // (planes * Nx rows taken two at a time: Nx is even, so the pairs are the row pass's)
        if (score->tile && score->ssim)
            return launch_or_fail(ctx, KID_SSIM, (double)planes * Nx * Ny * (score->u8 ? 5.0 : 8.0), "ssim_diff", [&] {
                return launch_ssim_diff(score->frames, score->u8, static_cast<const float*>(x), score->strips, planes * Nx / 2, Ny, score->tile, score->pivot, ctx->cur);
            });
        if (score->tile)
            return launch_or_fail(ctx, KID_SCORE_MAP, (double)planes * Nx * Ny * (score->u8 ? 5.0 : 8.0), "score_map_diff", [&] {
                return launch_score_map_diff(score->frames, score->u8, static_cast<const float*>(x), score->strips, planes * Nx / 2, Ny, score->tile, ctx->cur);
            });
        return launch_or_fail(ctx, KID_SCORE, (double)planes * Nx * Ny * (score->u8 ? 5.0 : 8.0), "score_diff",
                              [&] { return launch_score_diff(score->frames, score->u8, static_cast<const float*>(x), score->part, 1, planes * Nx, Ny, ctx->cur); });
    }
    if (!aligned16(x) || (!opin && !aligned16(X))) return fail(ctx, AEFFT_EINVAL, "c2r: pointers must be 16-byte aligned");
    if (Nxi > Nx || Nyi > Ny || Nxi < 2 || Nyi < 2 || (Nxi & 1) || (Nyi & 1)) return fail(ctx, AEFFT_EINVAL, "c2r: padded-from size must be even and inside the grid");
    void* mid;
    RET_IF(ws_get(ctx, ws_id, sizeof(float2) * fft_mid_elems(planes, Nx, Nyi / 2), &mid));
    const double b_in = (double)planes * bins(Nxi, Nyi) * 8, b_mid = (double)planes * Nx * (Nyi / 2) * 8;
    // (the scoring row pass reads the frames, writes one float per row pair, and the rows only when they were asked for)
    const double b_out = (double)planes * Nx * Ny * (out_u8 ? 1 : (x ? 4 : 0)) + (score ? (double)planes * Nx * Ny * (score->u8 ? 1 : 4) + (double)planes * Nx * 2 * (score->tile ? Ny / score->tile : 1) * (score->ssim ? SSIM_MOMENTS : 1) : 0.0);
    hipError_t e;
    {
        Bracket br(ctx, KID_C2R_COLS, b_in + b_mid);
        e = launch_c2r(X, nullptr, (float2*)mid, planes, Nxi, Nyi, Nx, Ny, scale, ctx->cur, opin);
    }
    if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "c2r cols", e);
    {
        Bracket br(ctx, KID_C2R_ROWS, b_mid + b_out);
        e = launch_c2r(nullptr, x, (float2*)mid, planes, Nxi, Nyi, Nx, Ny, scale, ctx->cur, nullptr, out_u8, score);
    }
    if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "c2r rows", e);
    return AEFFT_OK;
}

// algorithmic bytes of one contraction = UNIQUE tensors entering + leaving: A (R*K planes) + B (K*C planes) + Out (R*C planes),
// 8 B per bin; an operand that is the same tensor as another one (X X^H; the MSE epilogue's T = B) counts once; A2 counts.
double aefft::contract_bytes(const Contract& q)
{
    const bool self = q.A == q.B && q.a_r == q.b_c && q.a_k == q.b_k && q.R == q.C;
    double planes = (double)q.R * q.K + (self ? 0.0 : (double)q.K * q.C);
    if (q.A2 && q.A2 != q.B) planes += (double)q.R * q.K;
    if (!q.mse.acc) planes += (double)q.R * q.C;
    return planes * q.P * 8.0;
}

Contract aefft::bc(const aefft_ctx* ctx, Contract q) { if (q.bias) q.biasColP1 = ctx->biasColP1; return q; }

int aefft::do_contract(aefft_ctx* ctx, const Contract& q0)
{
    const Contract q = bc(ctx, q0);
    const double bytes = contract_bytes(q);
    Bracket br(ctx, KID_CONTRACT, bytes);
    hipError_t e = launch_contract(q, ctx->cur);
    if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "contract", e);
    return AEFFT_OK;
}

static int do_contract2(aefft_ctx* ctx, const Contract& q0, const Contract& q1)
{
    const double bytes = contract_bytes(q0) + contract_bytes(q1);
    Contract2 qq{};
    qq.q[0] = bc(ctx, q0); qq.q[1] = bc(ctx, q1); qq.n = 2;
    Bracket br(ctx, KID_CONTRACT, bytes);
    hipError_t e = launch_contract2(qq, ctx->cur);
    if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "contract2", e);
    return AEFFT_OK;
}

// ---- contraction descriptors (shared by the single-problem and the grouped launches) ----
static Contract mk_conv(const float2* X, const float2* W, const float* bias, float2* O, int B, int R, int K, int Nx, int Ny)
{
    const long P = bins(Nx, Ny);
    Contract q{};
    q.A = W; q.a_r = (long)K * P; q.a_k = P;
    q.B = X; q.b_k = P; q.b_c = (long)K * P;
    q.Out = O; q.o_r = P; q.o_c = (long)R * P;
    q.R = R; q.C = B; q.K = K; q.P = P;
    q.preDivB = (float)R;                       // in_t /= dM   (fft_backproplib.cu:176-177)
    q.bias = bias; q.biasScale = (float)Nx * (float)Ny; q.biasAfterFirst = true;
    return q;
}
float aefft::grad_norm(int dM, int dD, int Nx, int Ny)
{
    const float norm = (float)Nx * (float)Ny;                 // fft_backproplib.cu:398
    return norm * 2 * dM * dD * Nx * Ny;                      // :399 (float arithmetic, left to right)
}
Contract aefft::mk_S(const float2* Xin, const float2* T, const float2* O, float2* S, int B, int dD, long P)
{
    Contract q{};
    q.A = O; q.A2 = T; q.a_r = P; q.a_k = (long)dD * P;
    q.B = Xin; q.b_k = (long)dD * P; q.b_c = P; q.conjB = true;
    q.Out = S; q.o_r = (long)dD * P; q.o_c = P;
    q.R = dD; q.C = dD; q.K = B; q.P = P;
    return q;
}
// The same S when O is stored on the support of the up-sampled spectra only (Oc[b][d][s], s on the small grid):
//   S = -sum_b X_b X_b^H  on every bin,   S[map(s)] += sum_b Oc_b[s] X_b[map(s)]^H  on the support.
Contract aefft::mk_XXneg(const float2* X, float2* S, int B, int dD, long P)
{
    Contract q{};
    q.A = X; q.a_r = P; q.a_k = (long)dD * P;
    q.B = X; q.b_k = (long)dD * P; q.b_c = P; q.conjB = true;
    q.Out = S; q.o_r = (long)dD * P; q.o_c = P;
    q.R = dD; q.C = dD; q.K = B; q.P = P;
    q.postDiv = -1.0f;
    return q;
}
Contract aefft::mk_OX(const float2* Oc, const float2* X, float2* S, int B, int dD, long P, long Pc, int Nx, int Ny, int NxC, int NyC)
{
    Contract q{};
    q.A = Oc; q.a_r = Pc; q.a_k = (long)dD * Pc;
    q.B = X; q.b_k = (long)dD * P; q.b_c = P; q.conjB = true;
    q.Out = S; q.o_r = (long)dD * P; q.o_c = P;
    q.R = dD; q.C = dD; q.K = B; q.P = Pc;
    q.gdNx = Nx; q.gdNy = Ny; q.gdNxs = NxC; q.gdNys = NyC; q.gdMask = 2 | 4;
    q.accumulate = true;
    return q;
}
Contract aefft::mk_dc(const float2* F, const float2* S, float2* dc, int B, int dM, int dD, long P, float Norm)
{
    Contract q{};
    q.A = F; q.a_r = P; q.a_k = (long)dM * P; q.conjA = true;
    q.B = S; q.b_k = (long)dD * P; q.b_c = P;
    q.Out = dc; q.o_r = (long)dD * P; q.o_c = P;
    q.R = dM; q.C = dD; q.K = dD; q.P = P;
    q.postDiv = Norm * (float)B;
    return q;
}
Contract aefft::mk_df(const float2* C, const float2* S, float2* df, int B, int dM, int dD, long P, float Norm)
{
    Contract r{};
    r.A = S; r.a_r = (long)dD * P; r.a_k = P;
    r.B = C; r.b_k = P; r.b_c = (long)dD * P; r.conjB = true;
    r.Out = df; r.o_r = (long)dM * P; r.o_c = P;
    r.R = dD; r.C = dM; r.K = dD; r.P = P;
    r.postDiv = Norm * (float)B;
    return r;
}
// Re-forward of one pair for its MSE only (fft_backproplib.cu:1460-1463 when nothing else consumes H and O): the two
// conv_k collapse per bin into G[d'][d] = sum_m F[d'][m] C[m][d] / (dM*dD) (no batch dimension) ...
Contract aefft::mk_G(const float2* F, const float2* C, float2* G, int dM, int dD, long P)
{
    Contract q{};
    q.A = F; q.a_r = (long)dM * P; q.a_k = P;
    q.B = C; q.b_k = (long)dD * P; q.b_c = P;
    q.Out = G; q.o_r = (long)dD * P; q.o_c = P;
    q.R = dD; q.C = dD; q.K = dM; q.P = P;
    q.postDiv = (float)dM * (float)dD;
    return q;
}
// ... and O_b = G X_b (+ the bias terms at DC) is compared with X_b inside the contraction's epilogue: H and O never exist.
Contract aefft::mk_gmse(const float2* G, const float2* X, const float2* F, const float* b, const float* p, float* mse_slot,
                        int B, int dM, int dD, int Nx, int Ny)
{
    const long P = bins(Nx, Ny);
    Contract q{};
    q.A = G; q.a_r = (long)dD * P; q.a_k = P;
    q.B = X; q.b_k = P; q.b_c = (long)dD * P;
    q.R = dD; q.C = B; q.K = dD; q.P = P;
    q.mse.acc = mse_slot; q.mse.F = F; q.mse.b = b; q.mse.p = p; q.mse.dM = dM; q.mse.Nyr = Ny / 2 + 1;
    q.mse.nfull = (float)dD * Nx * Ny;
    q.mse.scale = 1.0f / ((float)(2 * dM) * (float)Nx * (float)Ny * (float)B);        // as do_diff_mse
    q.mse.norm = (float)Nx * (float)Ny;
    return q;
}
// n independent contractions of class cls (see ContractN) in one launch; falls back to one launch each
int aefft::do_contract_group(aefft_ctx* ctx, const Contract* qs, int n, int nA, int cls)
{
    if (n <= 8 && n > 1 && !flag(AEFFT_F_NOGROUP)) {
        ContractN g{};
        double bytes = 0;
        for (int i = 0; i < n; ++i) { g.q[i] = bc(ctx, qs[i]); bytes += contract_bytes(qs[i]); }
        g.n = n; g.nA = nA;
        const int rc = launch_or_decline(ctx, KID_CONTRACT, bytes, "contract(group)", [&] { return launch_contract_group(g, cls, ctx->cur); });
        if (rc != DECLINED) return rc;
    }
    for (int i = 0; i < n; ++i) RET_IF(do_contract(ctx, qs[i]));
    return AEFFT_OK;
}

// pool_fft(conv_k(X)) without the full-resolution conv output (fft_backproplib.cu:1346-1348 when only the pooled
// layer is consumed): Xs[b][r] on the [Nxs][Nys/2+1] grid.  *done = false: the kernel declined the shapes.
int aefft::do_conv_pooled(aefft_ctx* ctx, const float2* X, const float2* W, const float* bias, float2* Xs, int B, int R, int K,
                          int Nx, int Ny, int Nxs, int Nys, bool* done)
{
    *done = false;
    const long P = bins(Nx, Ny), Ps = bins(Nxs, Nys);
    Contract q{};
    q.A = W; q.a_r = (long)K * P; q.a_k = P;
    q.B = X; q.b_k = P; q.b_c = (long)K * P;
    q.Out = Xs; q.o_r = Ps; q.o_c = (long)R * Ps;
    q.R = R; q.C = B; q.K = K; q.P = Ps;
    q.preDivB = (float)R;
    q.bias = bias; q.biasScale = (float)Nx * (float)Ny; q.biasAfterFirst = true;
    q.gdNx = Nx; q.gdNy = Ny; q.gdNxs = Nxs; q.gdNys = Nys; q.gdMask = 3;
    q = bc(ctx, q);
    const int rc = launch_or_decline(ctx, KID_CONTRACT, ((double)R * K + (double)K * B + (double)R * B) * Ps * 8.0, "contract(pooled)",
                                     [&] { return launch_contract(q, ctx->cur); });
    *done = rc == AEFFT_OK;
    return rc == DECLINED ? AEFFT_OK : rc;
}

// conv_k over a batch: O[b][r] = sum_k (X[b][k]/R) * W[r][k] (+ bias[r]*Nx*Ny at DC)
int aefft::do_conv(aefft_ctx* ctx, const float2* X, const float2* W, const float* bias, float2* O, int B, int R, int K, int Nx, int Ny,
                   float2* Ocrop, int Nxs, int Nys)
{
    Contract q = mk_conv(X, W, bias, O, B, R, K, Nx, Ny);
    if (Ocrop) { q.Out2 = Ocrop; q.dnNx = Nx; q.dnNy = Ny; q.dnNxs = Nxs; q.dnNys = Nys; }
    return do_contract(ctx, q);
}

// conv_k whose input is the zero-pad up-sampling (pool_fft with negative scale, fft_backproplib.cu:1360 of the
// previous decoder) of Xs [B][K][sNx][sNy/2+1]: the up-sampled tensor is never materialised.
int aefft::do_conv_up(aefft_ctx* ctx, const float2* Xs, const float2* W, const float* bias, float2* O, int B, int R, int K,
                      int Nx, int Ny, int sNx, int sNy)
{
    if (sNx == Nx && sNy == Ny) return do_conv(ctx, Xs, W, bias, O, B, R, K, Nx, Ny);
    const long P = bins(Nx, Ny), Ps = bins(sNx, sNy);
    Contract q{};
    q.A = W; q.a_r = (long)K * P; q.a_k = P;
    q.B = Xs; q.b_k = Ps; q.b_c = (long)K * Ps;
    q.Out = O; q.o_r = P; q.o_c = (long)R * P;
    q.R = R; q.C = B; q.K = K; q.P = P;
    q.preDivB = (float)R;
    q.bias = bias; q.biasScale = (float)Nx * (float)Ny; q.biasAfterFirst = true;
    q.upNx = Nx; q.upNy = Ny; q.upNxs = sNx; q.upNys = sNy;
    q = bc(ctx, q);
    // algorithmic bytes: the SMALL input, the weights on the support, the full output
    const double bytes = ((double)K * B * Ps + (double)R * K * Ps + (double)R * B * P) * 8.0;
    Bracket br(ctx, KID_CONTRACT, bytes);
    hipError_t e = launch_contract(q, ctx->cur);
    if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "contract(up)", e);
    return AEFFT_OK;
}

int aefft::do_resize(aefft_ctx* ctx, const float2* in, float2* out, long planes, int Nx, int Ny, int Nxs, int Nys)
{
    Bracket br(ctx, KID_RESIZE, (double)planes * (std::min(bins(Nx, Ny), bins(Nxs, Nys)) + bins(Nxs, Nys)) * 8.0);
    hipError_t e = launch_resize(in, out, planes, Nx, Ny, Nxs, Nys, ctx->cur);
    if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "resize", e);
    return AEFFT_OK;
}

static void pooled(int Nx, int Ny, int scale, int* Nxs, int* Nys)
{
    // fft_backproplib.cu:980-984 with power-of-two scales (exact in float)
    if (scale > 0) { *Nxs = Nx / scale; *Nys = Ny / scale; }
    else { *Nxs = Nx * (-scale); *Nys = Ny * (-scale); }
}

// E = O - T (optional), mse (optional, ACCUMULATED into *mse: caller zeroes), es (optional, accumulated),
// mean over B:  scale = 1/(2*dM*Nx*Ny*B)
int aefft::do_diff_mse(aefft_ctx* ctx, const float2* T, const float2* O, float2* E, float* mse, float* es, int B, int dM, int dD, int Nx, int Ny)
{
    const float scale = 1.0f / ((float)(2 * dM) * (float)Nx * (float)Ny * (float)B);
    Bracket br(ctx, KID_DIFFMSE, (double)B * dD * bins(Nx, Ny) * 8.0 * (E ? 3 : 2));
    hipError_t e = launch_diff_mse(T, O, E, mse, es, B, dD, Nx, Ny, scale, ctx->cur);
    if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "diff_mse", e);
    return AEFFT_OK;
}

// gradient_k_io over a batch (fft_backproplib.cu:395-475); T = spectrum of the expected output, E = O - T.
// The reference's four per-bin sums are re-associated so that the batch is contracted FIRST:
//     S[d][d1]  = sum_b  (O_b[d] - T_b[d]) * conj(X_b[d1])            (dD x dD per bin; the subtraction is fused)
//     dc[m][d]  = sum_d1 conj(F[d1][m]) * S[d1][d]      / (Norm*B)   (== conj(X) * sum_d1 E conj(F), :421-439)
//     df[d][m]  = sum_d1 S[d][d1] * conj(C[m][d1])      / (Norm*B)   (== E * conj(sum_d1 C X),      :426-455)
//     df[d][m](0,0) += es[d] * b[m]*Nx*Ny / (Norm*B),  es[d] = sum_b E_b[d](0,0)   (the b0 term, :448-455)
// Same sums, different order (float32 rounding only); neither E nor the B*dM-plane intermediates of the
// literal form are materialised.  S: workspace [dD][dD][P].  dc and df are produced by ONE launch.
int aefft::do_gradient(aefft_ctx* ctx, const float2* Xin, const float2* T, const float2* O, const float2* C, const float2* F,
                       const float* b, float2* S, float2* dc, float2* df, float* db, float* dp, int B, int dM, int dD, int Nx, int Ny)
{
    const long P = bins(Nx, Ny);
    const float norm = (float)Nx * (float)Ny;                 // fft_backproplib.cu:398
    const float Norm = grad_norm(dM, dD, Nx, Ny);
    RET_IF(do_contract(ctx, mk_S(Xin, T, O, S, B, dD, P)));
    RET_IF(do_contract2(ctx, mk_dc(F, S, dc, B, dM, dD, P, Norm), mk_df(C, S, df, B, dM, dD, P, Norm)));
    {
        Bracket br(ctx, KID_BIASGRAD, ((double)(dM * dD + dM + dD) + 2.0 * B * dD) * 8.0);
        hipError_t e = launch_bias_grad(O, T, F, b, df, db, dp, B, dM, dD, P, norm, Norm, ctx->cur);
        if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "bias_grad", e);
    }
    return AEFFT_OK;
}

// unnormalised C2R of a gradient spectrum sampled on the kernel support: g[planes][Nk][Nl]
// (== shrink_k(cufftExecC2R(d)), fft_backproplib.cu:1219-1226).  Direct pruned evaluation when the
// support is 3x3/5x5/7x7, generic C2R + shrink otherwise.
int aefft::do_c2r_shrink(aefft_ctx* ctx, const float2* dspec, float* gk, float* realws, float* part, long planes, int Nx, int Ny, int Nk, int Nl, float scale)
{
    if (pruned_supported(Nk, Nl, Nx, Ny)) {
        Bracket br(ctx, KID_KGRAD, (double)planes * (bins(Nx, Ny) * 8.0 + Nk * Nl * 4.0));
        hipError_t e = launch_kgrad(dspec, gk, part, ctx->tw, planes, Nx, Ny, Nk, Nl, scale, ctx->cur);
        if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "kgrad", e);
        return AEFFT_OK;
    }
    RET_IF(do_c2r(ctx, dspec, realws, planes, Nx, Ny, Nx, Ny, scale));
    Bracket br(ctx, KID_SHRINK, (double)planes * Nk * Nl * 8.0);
    hipError_t e = launch_shrink(realws, gk, planes, Nx, Ny, Nk, Nl, 1.0f, ctx->cur);
    if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "shrink", e);
    return AEFFT_OK;
}

// pad + R2C: kernel [planes][Nk][Nl] -> spectrum [planes][Nx][Nyr]  (fft_backproplib.cu:1274-1282 / 1150-1152)
int aefft::do_pad_r2c(aefft_ctx* ctx, const float* k, float2* K, float* realws, long planes, int Nx, int Ny, int Nk, int Nl)
{
    if (pruned_supported(Nk, Nl, Nx, Ny)) {
        Bracket br(ctx, KID_KSPEC, (double)planes * (bins(Nx, Ny) * 8.0 + Nk * Nl * 4.0));
        hipError_t e = launch_kspec(k, K, ctx->tw, planes, Nx, Ny, Nk, Nl, ctx->cur);
        if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "kspec", e);
        return AEFFT_OK;
    }
    {
        Bracket br(ctx, KID_PAD, (double)planes * ((double)Nx * Ny + Nk * Nl) * 4.0);
        hipError_t e = launch_pad(k, realws, planes, Nx, Ny, Nk, Nl, ctx->cur);
        if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "pad", e);
    }
    return do_r2c(ctx, realws, K, planes, Nx, Ny, Nx, Ny);
}

// the coordinate-space part of `backprop` (fft_backproplib.cu:1229-1272) on already shrunk gradients
int aefft::do_update(aefft_ctx* ctx, float* c, float* f, float* b, float* p, const float* dck, const float* dfk, const float* db,
                     const float* dp, Momentum mo, int dM, int dD, int Nk, int Nl, float del, int maxdiff, int sym, float gscale,
                     float* zero)
{
    UpdateArgs a{};
    a.zero = zero;
    a.c = c; a.f = f; a.b = b; a.p = p;
    a.dck = dck; a.dfk = dfk; a.db = db; a.dp = dp;
    a.Dc = mo.Dc; a.Df = mo.Df; a.Db = mo.Db; a.Dp = mo.Dp;
    a.dM = dM; a.dD = dD; a.Nk = Nk; a.Nl = Nl;
    a.del = del; a.alpha = 0.9f; a.w0 = 1.f; a.w1 = 10.f;      // fft_backproplib.cu:608,1252
    a.gscale = sym ? 0.5f * gscale : gscale; a.sym = sym;
    if (maxdiff) {
        const size_t nk = (size_t)dM * dD * Nk * Nl;
        void *small, *den;
        RET_IF(ws_get(ctx, WS_SMALL, sizeof(float) * (2 * nk + dM + dD + 64), &small));
        RET_IF(ws_get(ctx, WS_DEN, sizeof(float) * gradient_diff_ws_floats(dM, dD, Nk, Nl), &den));
        float* cd = (float*)small; float* fd = cd + nk; float* bd = fd + nk; float* pd = bd + dM;
        {
            Bracket br(ctx, KID_GDIFF, (double)nk * 16.0);
            hipError_t e = launch_gradient_diff(c, f, b, p, cd, fd, bd, pd, (float*)den, dM, dD, Nk, Nl, ctx->cur);
            if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "gradient_diff", e);
        }
        a.cd = cd; a.fd = fd; a.bd = bd; a.pd = pd;
    }
    Bracket br(ctx, KID_UPDATE, (double)dM * dD * Nk * Nl * 4.0 * 8);
    hipError_t e = launch_update(a, ctx->cur);
    if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "update", e);
    return AEFFT_OK;
}

UpdateArgs aefft::mk_update(float* c, float* f, float* b, float* p, const float* dck, const float* dfk, const float* db, const float* dp,
                            Momentum mo, int dM, int dD, int Nk, int Nl, float del, int sym, float gscale, float* zero)
{
    UpdateArgs a{};
    a.zero = zero;
    a.c = c; a.f = f; a.b = b; a.p = p;
    a.dck = dck; a.dfk = dfk; a.db = db; a.dp = dp;
    a.Dc = mo.Dc; a.Df = mo.Df; a.Db = mo.Db; a.Dp = mo.Dp;
    a.dM = dM; a.dD = dD; a.Nk = Nk; a.Nl = Nl;
    a.del = del; a.alpha = 0.9f; a.w0 = 1.f; a.w1 = 10.f;      // fft_backproplib.cu:608,1252
    a.gscale = sym ? 0.5f * gscale : gscale; a.sym = sym;
    return a;
}

// ------------------------------------------------------------------------------------------
// op-level C entry points
// ------------------------------------------------------------------------------------------

extern "C" int aefft_r2c(aefft_ctx* ctx, const float* x_d, float* X_d, long planes, int Nx, int Ny)
{
    if (!ctx || !x_d || !X_d || planes < 0) return fail(ctx, AEFFT_EINVAL, "aefft_r2c: bad argument");
    return do_r2c(ctx, x_d, F2(X_d), planes, Nx, Ny, Nx, Ny);
}

extern "C" int aefft_c2r(aefft_ctx* ctx, const float* X_d, float* x_d, long planes, int Nx, int Ny, float scale)
{
    if (!ctx || !x_d || !X_d || planes < 0) return fail(ctx, AEFFT_EINVAL, "aefft_c2r: bad argument");
    return do_c2r(ctx, CF2(X_d), x_d, planes, Nx, Ny, Nx, Ny, scale);
}

// op level: any integer scale, sized as the reference sizes it (fft_backproplib.cu:980-984: l = scale or 1/|scale| as FLOAT, Nxs = int(Nx / l) --
// exact for powers of two, SURVEY B-4, and for the other scales whatever that float arithmetic gives); the resized grid must be even (the
// index rules of `resize`, :98-153, are written for even sizes) and a size the transforms serve
static int chk_scale(aefft_ctx* ctx, int Nx, int Ny, int scale, int* Nxs, int* Nys)
{
    if (scale == 0) return fail(ctx, AEFFT_EINVAL, "pooling scale must be non-zero");
    const float l = scale > 0 ? (float)scale : -1.0f / (float)scale;
    *Nxs = (int)((float)Nx / l); *Nys = (int)((float)Ny / l);
    if ((*Nxs & 1) || (*Nys & 1)) return fail(ctx, AEFFT_EINVAL, "pooled size must be even");
    if (*Nxs < 8 || *Nys < 8 || *Nxs > 2048 || *Nys > 2048) return fail(ctx, AEFFT_EINVAL, "pooled size out of range 8..2048");
    return AEFFT_OK;
}

extern "C" int aefft_pool(aefft_ctx* ctx, const float* X_d, float* Xs_d, long planes, int Nx, int Ny, int scale, int* Nxs, int* Nys)
{
    if (!ctx || !X_d || !Xs_d || planes < 0) return fail(ctx, AEFFT_EINVAL, "aefft_pool: bad argument");
    if (!(net_size(Nx) && net_size(Ny))) RET_IF(chk_size_any(ctx, Nx, Ny));      // (only a resize: smooth sizes up to 2048 as well)
    int nx, ny;
    RET_IF(chk_scale(ctx, Nx, Ny, scale, &nx, &ny));
    if (Nxs) *Nxs = nx;
    if (Nys) *Nys = ny;
    if (scale == 1 || scale == -1) {   // fft_backproplib.cu:977: nothing happens
        HIPCHK(ctx, hipMemcpyAsync(Xs_d, X_d, sizeof(float2) * planes * bins(Nx, Ny), hipMemcpyDeviceToDevice, ctx->stream));
        return AEFFT_OK;
    }
    return do_resize(ctx, CF2(X_d), F2(Xs_d), planes, Nx, Ny, nx, ny);
}

extern "C" int aefft_r2c_pool(aefft_ctx* ctx, const float* x_d, float* Xs_d, long planes, int Nx, int Ny, int scale)
{
    if (!ctx || !x_d || !Xs_d || planes < 0 || scale < 1) return fail(ctx, AEFFT_EINVAL, "aefft_r2c_pool: bad argument");
    int nx, ny;
    RET_IF(chk_scale(ctx, Nx, Ny, scale, &nx, &ny));
    return do_r2c(ctx, x_d, F2(Xs_d), planes, Nx, Ny, nx, ny);
}

extern "C" int aefft_unpool_c2r(aefft_ctx* ctx, const float* Xs_d, float* x_d, long planes, int Nxs, int Nys, int scale, float out_scale)
{
    if (!ctx || !x_d || !Xs_d || planes < 0 || scale > -1) return fail(ctx, AEFFT_EINVAL, "aefft_unpool_c2r: scale must be <= -1");
    int nx, ny;
    RET_IF(chk_scale(ctx, Nxs, Nys, scale, &nx, &ny));
    return do_c2r(ctx, CF2(Xs_d), x_d, planes, Nxs, Nys, nx, ny, out_scale);
}

extern "C" int aefft_kernel_spectrum(aefft_ctx* ctx, const float* k_d, float* K_d, int nA, int nB, int Nk, int Nl, int Nx, int Ny)
{
    if (!ctx || !k_d || !K_d || nA <= 0 || nB <= 0 || Nk <= 0 || Nl <= 0 || Nk > Nx || Nl > Ny) return fail(ctx, AEFFT_EINVAL, "aefft_kernel_spectrum: bad argument");
    RET_IF(chk_size_smooth(ctx, Nx, Ny));
    const long planes = (long)nA * nB;
    void* real = nullptr;
    if (!pruned_supported(Nk, Nl, Nx, Ny)) RET_IF(ws_get(ctx, WS_REAL, sizeof(float) * planes * Nx * Ny, &real));
    return do_pad_r2c(ctx, k_d, F2(K_d), (float*)real, planes, Nx, Ny, Nk, Nl);
}

extern "C" int aefft_kernel_export(aefft_ctx* ctx, const float* K_d, float* k_d, int nA, int nB, int Nk, int Nl, int Nx, int Ny)
{
    if (!ctx || !k_d || !K_d || nA <= 0 || nB <= 0 || Nk <= 0 || Nl <= 0 || Nk > Nx || Nl > Ny) return fail(ctx, AEFFT_EINVAL, "aefft_kernel_export: bad argument");
    RET_IF(chk_size_smooth(ctx, Nx, Ny));
    const long planes = (long)nA * nB;
    void *real = nullptr, *part = nullptr;
    if (pruned_supported(Nk, Nl, Nx, Ny)) RET_IF(ws_get(ctx, WS_PART, sizeof(float) * kgrad_partial_floats(planes, Nx, Ny, Nk, Nl), &part));
    else RET_IF(ws_get(ctx, WS_REAL, sizeof(float) * planes * Nx * Ny, &real));
    // kfft_inv: C2R then * 1/(Nx*Ny) (fft_backproplib.cu:948), then kernel_invpad
    return do_c2r_shrink(ctx, CF2(K_d), k_d, (float*)real, (float*)part, planes, Nx, Ny, Nk, Nl, 1.0f / ((float)Nx * (float)Ny));
}

extern "C" int aefft_conv(aefft_ctx* ctx, const float* X_d, const float* C_d, const float* bias_d, float* O_d, int B, int dM, int dD, int Nx, int Ny)
{
    if (!ctx || !X_d || !C_d || !O_d || B <= 0 || dM <= 0 || dD <= 0) return fail(ctx, AEFFT_EINVAL, "aefft_conv: bad argument");
    RET_IF(chk_size_smooth(ctx, Nx, Ny));
    if (!aligned16(X_d) || !aligned16(C_d) || !aligned16(O_d)) return fail(ctx, AEFFT_EINVAL, "aefft_conv: pointers must be 16-byte aligned");
    return do_conv(ctx, CF2(X_d), CF2(C_d), bias_d, F2(O_d), B, dM, dD, Nx, Ny);
}

extern "C" int aefft_gradient(aefft_ctx* ctx, const float* Xin_d, const float* Xout_d, const float* O_d, const float* C_d,
                              const float* F_d, const float* b_d, float* dc_d, float* df_d, float* db_d, float* dp_d,
                              int B, int dM, int dD, int Nx, int Ny)
{
    if (!ctx || !Xin_d || !Xout_d || !O_d || !C_d || !F_d || !b_d || !dc_d || !df_d || !db_d || !dp_d || B <= 0 || dM <= 0 || dD <= 0)
        return fail(ctx, AEFFT_EINVAL, "aefft_gradient: bad argument");
    RET_IF(chk_size_smooth(ctx, Nx, Ny));
    const long P = bins(Nx, Ny);
    void* S;
    RET_IF(ws_get(ctx, WS_S, sizeof(float2) * dD * dD * P, &S));
    return do_gradient(ctx, CF2(Xin_d), CF2(Xout_d), CF2(O_d), CF2(C_d), CF2(F_d), b_d, (float2*)S, F2(dc_d), F2(df_d), db_d, dp_d, B, dM, dD, Nx, Ny);
}

extern "C" int aefft_mse(aefft_ctx* ctx, const float* T_d, const float* O_d, float* mse_d, int B, int dM, int dD, int Nx, int Ny)
{
    if (!ctx || !T_d || !O_d || !mse_d || B <= 0) return fail(ctx, AEFFT_EINVAL, "aefft_mse: bad argument");
    HIPCHK(ctx, hipMemsetAsync(mse_d, 0, sizeof(float), ctx->stream));
    return do_diff_mse(ctx, CF2(T_d), CF2(O_d), nullptr, mse_d, nullptr, B, dM, dD, Nx, Ny);
}

extern "C" int aefft_update(aefft_ctx* ctx, float* c_d, float* f_d, float* b_d, float* p_d, float* C_d, float* F_d,
                            const float* dc_d, const float* df_d, const float* db_d, const float* dp_d,
                            float* Dc_d, float* Df_d, float* Db_d, float* Dp_d,
                            int dM, int dD, int Nx, int Ny, int Nk, int Nl, float del, int maxdiff)
{
    if (!ctx || !c_d || !f_d || !b_d || !p_d || !C_d || !F_d || !dc_d || !df_d || !db_d || !dp_d || !Dc_d || !Df_d || !Db_d || !Dp_d)
        return fail(ctx, AEFFT_EINVAL, "aefft_update: null pointer");
    RET_IF(chk_size_smooth(ctx, Nx, Ny));
    const long planes = (long)dM * dD;
    const size_t nk = (size_t)planes * Nk * Nl;
    void *real = nullptr, *tmp, *part = nullptr;
    if (pruned_supported(Nk, Nl, Nx, Ny)) RET_IF(ws_get(ctx, WS_PART, sizeof(float) * kgrad_partial_floats(planes, Nx, Ny, Nk, Nl), &part));
    else RET_IF(ws_get(ctx, WS_REAL, sizeof(float) * planes * Nx * Ny, &real));
    RET_IF(ws_get(ctx, WS_TMP, sizeof(float) * 2 * nk, &tmp));
    float* dck = (float*)tmp; float* dfk = dck + nk;
    RET_IF(do_c2r_shrink(ctx, CF2(dc_d), dck, (float*)real, (float*)part, planes, Nx, Ny, Nk, Nl));
    RET_IF(do_c2r_shrink(ctx, CF2(df_d), dfk, (float*)real, (float*)part, planes, Nx, Ny, Nk, Nl));
    RET_IF(do_update(ctx, c_d, f_d, b_d, p_d, dck, dfk, db_d, dp_d, Momentum{Dc_d, Df_d, Db_d, Dp_d}, dM, dD, Nk, Nl, del, maxdiff, 0, 1.0f));
    RET_IF(do_pad_r2c(ctx, c_d, F2(C_d), (float*)real, planes, Nx, Ny, Nk, Nl));
    RET_IF(do_pad_r2c(ctx, f_d, F2(F_d), (float*)real, planes, Nx, Ny, Nk, Nl));
    return AEFFT_OK;
}

// spatial mode ------------------------------------------------------------------------------
static void spatial_geom(int Nk, int Nl, int cpu_semantics, int* ak, int* al, int* lo)
{
    if (cpu_semantics == 1) { *ak = (Nk - 1) / 2 - 1; *al = (Nl - 1) / 2 - 1; *lo = 1; }     // netlib.cpp:325-326,344
    else { *ak = ((Nk - 1) / 2 - 1) / 2; *al = ((Nl - 1) / 2 - 1) / 2; *lo = 0; }             // backproplib.cu:123-124,95
}

extern "C" int aefft_conv_spatial(aefft_ctx* ctx, const float* in_d, float* out_d, const float* c_d, const float* b_d,
                                  int B, int dD, int dM, int Nx, int Ny, int Nk, int Nl, int cpu_semantics)
{
    if (!ctx || !in_d || !out_d || !c_d || !b_d || B <= 0 || dD <= 0 || dM <= 0 || Nx <= 0 || Ny <= 0 || Nk <= 0 || Nl <= 0)
        return fail(ctx, AEFFT_EINVAL, "aefft_conv_spatial: bad argument");
    int ak, al, lo;
    spatial_geom(Nk, Nl, cpu_semantics, &ak, &al, &lo);
    Bracket br(ctx, KID_SPATIAL, ((double)B * (dD + dM) * Nx * Ny + (double)dM * dD * Nk * Nl) * 4.0);
    hipError_t e = launch_conv_spatial(in_d, out_d, c_d, b_d, B, dD, dM, Nx, Ny, Nk, Nl, ak, al, cpu_semantics == 1 ? 1.f : (float)dM, lo, ctx->stream);
    if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "conv_spatial", e);
    return AEFFT_OK;
}

extern "C" int aefft_pool_conv_spatial(aefft_ctx* ctx, const float* in_d, float* pooled_d, float* out_d, const float* c_d, const float* b_d,
                                       int B, int dD, int dM, int Nx, int Ny, int scale, int Nk, int Nl, int cpu_semantics)
{
    if (!ctx || !in_d || !out_d || !c_d || !b_d || B <= 0 || dD <= 0 || dM <= 0 || Nx <= 0 || Ny <= 0 || Nk <= 0 || Nl <= 0 || scale < 1)
        return fail(ctx, AEFFT_EINVAL, "aefft_pool_conv_spatial: bad argument");
    int ak, al, lo;
    spatial_geom(Nk, Nl, cpu_semantics, &ak, &al, &lo);
    Bracket br(ctx, KID_SPATIAL, ((double)B * dD * Nx * Ny * scale * scale + (double)B * (dM + (pooled_d ? dD : 0)) * Nx * Ny + (double)dM * dD * Nk * Nl) * 4.0);
    hipError_t e = launch_conv_spatial(in_d, out_d, c_d, b_d, B, dD, dM, Nx, Ny, Nk, Nl, ak, al, cpu_semantics == 1 ? 1.f : (float)dM, lo, ctx->stream, scale, pooled_d);
    if (e == hipErrorInvalidValue) { (void)hipGetLastError(); return fail(ctx, AEFFT_EINVAL, "aefft_pool_conv_spatial: kernel shape not served by the fused kernel"); }
    if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "pool_conv_spatial", e);
    return AEFFT_OK;
}

extern "C" int aefft_pool_spatial(aefft_ctx* ctx, const float* in_d, float* out_d, long planes, int Nxi, int Nyi, int Nxo, int Nyo, int scale)
{
    if (!ctx || !in_d || !out_d || planes <= 0 || Nxi <= 0 || Nyi <= 0 || Nxo <= 0 || Nyo <= 0 || scale == 0)
        return fail(ctx, AEFFT_EINVAL, "aefft_pool_spatial: bad argument");
    Bracket br(ctx, KID_SPATIAL, (double)planes * ((double)Nxi * Nyi + (double)Nxo * Nyo) * 4.0);
    hipError_t e = launch_pool_spatial(in_d, out_d, planes, Nxi, Nyi, Nxo, Nyo, scale, ctx->stream);
    if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "pool_spatial", e);
    return AEFFT_OK;
}

static int backprop_spatial_impl(aefft_ctx* ctx, const float* in_d, const float* out_d, const float* hin_d,
                                 float* c_d, float* b_d, float* f_d, float* p_d,
                                 float* dc_d, float* db_d, float* df_d, float* dp_d,
                                 float* ddc_d, float* ddb_d, float* ddf_d, float* ddp_d,
                                 int B, int dD, int dM, int Nx, int Ny, int Nk, int Nl,
                                 float delmax, float alpha, int tied, int cpu_semantics, bool hin_is_conv)
{
    if (!ctx || !in_d || !out_d || !hin_d || !c_d || !b_d || !f_d || !p_d || !dc_d || !db_d || !df_d || !dp_d || B <= 0)
        return fail(ctx, AEFFT_EINVAL, "aefft_backprop_spatial: bad argument");
    const size_t nk = (size_t)dM * dD * Nk * Nl;
    void *ws, *small;
    RET_IF(ws_get(ctx, WS_REAL, sizeof(float) * (size_t)B * dM * Nx * Ny, &ws));
    const size_t nrq = spatial_rq_floats(dD, Nk, Nl);
    RET_IF(ws_get(ctx, WS_TMP, sizeof(float) * (2 * nk + dM + dD + nrq), &small));
    SpatialGradArgs a{};
    a.in = in_d; a.out = out_d; a.hin = hin_d; a.f = f_d;
    a.gc = (float*)small; a.gf = a.gc + nk; a.gb = a.gf + nk; a.gp = a.gb + dM;
    a.ws = (float*)ws;
    a.rq = a.gp + dD;
    {
        const size_t pf = spatial_partial_floats(B, dD, dM, Nx, Ny, Nk, Nl);
        void* part = nullptr;
        if (pf) RET_IF(ws_get(ctx, WS_PART, sizeof(float) * pf, &part));
        a.part = (float*)part;
    }
    a.B = B; a.dD = dD; a.dM = dM; a.Nx = Nx; a.Ny = Ny; a.Nk = Nk; a.Nl = Nl;
    spatial_geom(Nk, Nl, cpu_semantics, &a.ak, &a.al, &a.lo);
    a.Norm = (float)(dD * dM * Nk * Nl * Nx * Ny);            // backproplib.cu:303
    if (tied) a.Norm = (float)(2 * dD * dM * Nk * Nl * Nx * Ny);   // :533
    a.tied = tied;
    if (hin_is_conv && spatial_regions_ok(a)) {
        // the hidden layer is this call's own Conv_gpu(in; c, b): dF and dP come out of the error-input region sums as dC and dB do, the
        // hidden layer is not read again (the weights are read before the update below changes them: stream order)
        a.c1 = c_d; a.b1 = b_d; a.div1 = cpu_semantics == 1 ? 1.f : (float)dM;
    }
    {
        Bracket br(ctx, KID_SPATIAL, (double)B * ((a.c1 ? 2.0 : 3.0) * dD + (a.c1 ? 0.0 : 1.0) * dM) * Nx * Ny * 4.0);
        hipError_t e = launch_spatial_grad(a, ctx->stream);
        if (e == hipSuccess && cpu_semantics == 2) e = launch_spatial_compat(a, ctx->stream);      // Appendix B-11: bug-compatible gf, gb
        if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "spatial_grad", e);
    }
    UpdateArgs u{};
    u.c = c_d; u.f = f_d; u.b = b_d; u.p = p_d;
    u.dck = a.gc; u.dfk = a.gf; u.db = a.gb; u.dp = a.gp;
    u.Dc = dc_d; u.Df = df_d; u.Db = db_d; u.Dp = dp_d;
    u.dM = dM; u.dD = dD; u.Nk = Nk; u.Nl = Nl;
    u.del = delmax; u.alpha = alpha; u.w0 = 1.f; u.w1 = 0.f; u.gscale = 1.f; u.sym = tied;
    u.ddc = ddc_d; u.ddf = tied ? nullptr : ddf_d; u.ddb = ddb_d; u.ddp = ddp_d;   // adapt_rate records the gradient (backproplib.cu:33)
    {
        Bracket br(ctx, KID_UPDATE, (double)nk * 4.0 * 8);
        hipError_t e = launch_update(u, ctx->stream);
        if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "update", e);
    }
    return AEFFT_OK;
}

extern "C" int aefft_backprop_spatial(aefft_ctx* ctx, const float* in_d, const float* out_d, const float* hin_d,
                                      float* c_d, float* b_d, float* f_d, float* p_d,
                                      float* dc_d, float* db_d, float* df_d, float* dp_d,
                                      float* ddc_d, float* ddb_d, float* ddf_d, float* ddp_d,
                                      int B, int dD, int dM, int Nx, int Ny, int Nk, int Nl,
                                      float delmax, float alpha, int tied, int cpu_semantics)
{
    return backprop_spatial_impl(ctx, in_d, out_d, hin_d, c_d, b_d, f_d, p_d, dc_d, db_d, df_d, dp_d, ddc_d, ddb_d, ddf_d, ddp_d,
                                 B, dD, dM, Nx, Ny, Nk, Nl, delmax, alpha, tied, cpu_semantics, false);
}

extern "C" int aefft_step_spatial(aefft_ctx* ctx, const float* in_d, float* hin_d, float* out_d,
                                  float* c_d, float* b_d, float* f_d, float* p_d,
                                  float* dc_d, float* db_d, float* df_d, float* dp_d,
                                  float* ddc_d, float* ddb_d, float* ddf_d, float* ddp_d,
                                  int B, int dD, int dM, int Nx, int Ny, int Nk, int Nl,
                                  float delmax, float alpha, int tied, int cpu_semantics)
{
    if (!ctx || !in_d || !out_d || !hin_d || cpu_semantics < 0 || cpu_semantics > 1) return fail(ctx, AEFFT_EINVAL, "aefft_step_spatial: bad argument");
    RET_IF(aefft_conv_spatial(ctx, in_d, hin_d, c_d, b_d, B, dD, dM, Nx, Ny, Nk, Nl, cpu_semantics));
    RET_IF(aefft_conv_spatial(ctx, hin_d, out_d, f_d, p_d, B, dM, dD, Nx, Ny, Nk, Nl, cpu_semantics));
    return backprop_spatial_impl(ctx, in_d, out_d, hin_d, c_d, b_d, f_d, p_d, dc_d, db_d, df_d, dp_d, ddc_d, ddb_d, ddf_d, ddp_d,
                                 B, dD, dM, Nx, Ny, Nk, Nl, delmax, alpha, tied, cpu_semantics, true);
}
