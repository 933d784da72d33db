// C-ABI layer (include/aefft.h), the spatial net: an aefft_net created with AEFFT_NET_SPATIAL trains the reference's coordinate-space
// mode (autoencoder.cpp:135-150 Pool -> Conv_gpu per encoder, Conv_gpu -> Pool(-s) per decoder, then backprop_gpu[_cc] per pair,
// :161-178) over a batch, every pair per step, split into step_grad / all-reduce / step_apply like the FFT nets.  The public entry
// points in net.hip, net_forward.hip, net_score.hip and net_step.hip hand a spatial net over to the functions here.  DESIGN.md section 12.
//
// Layers (autoencoder.cpp:109-120 ordering), pair l on the grid G_l = G_{l-1} / s_l:
//   2l+1     Pool(layer 2l, s_l)         q.Lin   written by the encoder's convolution (Pool on load, pooled_out)
//   2l+2     Conv_gpu(2l+1; c_l, b_l)    q.Lhid
//   4L-1-2l  Conv_gpu(4L-2-2l; f_l, p_l) q.Lout  reads pair l+1's Lout up-sampled on load (layer 4L-2-2l is never stored)
//   4L-2l    Pool(4L-1-2l, -s_l)         formed on request (layer 4L: also the reconstruction written by pair 0's decoder)
#include "net.h"

#include <algorithm>
#include <string>
#include <vector>

using namespace aefft;

// GPU semantics of Conv_gpu / backprop_gpu (backproplib.cu:123-124,95): tap offset -2*ak-1+k, range test '>= 0'
static void sp_geom(const Pair& q, int* ak, int* al)
{
    *ak = ((q.Nk - 1) / 2 - 1) / 2;
    *al = ((q.Nl - 1) / 2 - 1) / 2;
}

static float sp_norm(const Pair& q) { return (float)((double)q.dD * q.dM * q.Nk * q.Nl * q.Nx * q.Ny); }     // backproplib.cu:303

int aefft::sp_refuse(aefft_net* n, const char* entry)
{
    const std::string msg = std::string(entry) + ": does not apply to a spatial net (AEFFT_NET_SPATIAL)";
    return fail(n->ctx, AEFFT_EINVAL, msg.c_str());
}

int aefft::sp_create(aefft_ctx* ctx, const aefft_net_desc* d, aefft_net** out)
{
    if (d->Nx <= 0 || d->Ny <= 0) return fail(ctx, AEFFT_EINVAL, "aefft_net_create_ex (AEFFT_NET_SPATIAL): bad frame size");
    aefft_net* n = new aefft_net();
    n->ctx = ctx; n->D = d->D; n->Nx = d->Nx; n->Ny = d->Ny; n->L = d->npairs; n->B = d->batch; n->Bc = n->B;
    n->spatial = true; n->compact = false; n->pruned = false;
    n->pr.resize(n->L);
    const size_t B = (size_t)n->B;
    int dD = d->D, nx = d->Nx, ny = d->Ny;
    size_t goff = 0, maxWs = 0, maxPart = 0, maxRq = 0, maxUp = 0;
    int rc = AEFFT_OK;
    for (int l = 0; l < n->L && rc == AEFFT_OK; ++l) {
        Pair& q = n->pr[l];
        q.dD = dD; q.dM = d->maps[l]; q.Nk = d->Nk[l]; q.Nl = d->Nl[l]; q.s = d->scale[l];
        q.Nxin = nx; q.Nyin = ny;
        if (q.dM <= 0 || q.Nk <= 0 || q.Nl <= 0 || q.s < 1) { rc = fail(ctx, AEFFT_EINVAL, "aefft_net_create_ex (AEFFT_NET_SPATIAL): bad pair parameters"); break; }
        // Pool(-s) with a remainder reads past its input in the reference (netlib.cpp:141-162): exact division only
        if (nx % q.s || ny % q.s) {
            const std::string msg = "aefft_net_create_ex (AEFFT_NET_SPATIAL): every pair's scale must divide its input grid exactly (pair " + std::to_string(l) +
                                    ": " + std::to_string(nx) + " x " + std::to_string(ny) + " by " + std::to_string(q.s) + ")";
            rc = fail(ctx, AEFFT_EINVAL, msg.c_str());
            break;
        }
        q.Nx = nx / q.s; q.Ny = ny / q.s;
        if (q.Nx < q.Nk || q.Ny < q.Nl) {
            const std::string msg = "aefft_net_create_ex (AEFFT_NET_SPATIAL): every pooled grid must be at least the pair's kernel support (pair " + std::to_string(l) +
                                    ": " + std::to_string(q.Nx) + " x " + std::to_string(q.Ny) + " for " + std::to_string(q.Nk) + " x " + std::to_string(q.Nl) + ")";
            rc = fail(ctx, AEFFT_EINVAL, msg.c_str());
            break;
        }
        q.P = 0;
        const size_t nk = q.nk(), px = (size_t)q.Nx * q.Ny;
        q.goff = goff; goff += 2 * nk + q.dM + q.dD;
        if ((rc = net_alloc_t(n, &q.c, 2 * nk)) || (rc = net_alloc_t(n, &q.Dc, 2 * nk))) break;
        q.f = q.c + nk; q.Df = q.Dc + nk;
        if ((rc = net_alloc_t(n, &q.b, q.dM)) || (rc = net_alloc_t(n, &q.Db, q.dM)) || (rc = net_alloc_t(n, &q.p, q.dD)) || (rc = net_alloc_t(n, &q.Dp, q.dD))) break;
        if ((rc = net_alloc_t(n, &q.Lin, B * q.dD * px)) || (rc = net_alloc_t(n, &q.Lhid, B * q.dM * px)) || (rc = net_alloc_t(n, &q.Lout, B * q.dD * px))) break;
        maxWs = std::max(maxWs, B * q.dM * px);
        maxPart = std::max(maxPart, spatial_partial_floats(n->B, q.dD, q.dM, q.Nx, q.Ny, q.Nk, q.Nl));
        maxRq = std::max(maxRq, spatial_rq_floats(q.dD, q.Nk, q.Nl));
        if (l > 0) maxUp = std::max(maxUp, B * n->pr[l - 1].dM * (size_t)n->pr[l - 1].Nx * n->pr[l - 1].Ny);   // decoder l-1's up-sampled input
        dD = q.dM; nx = q.Nx; ny = q.Ny;
    }
    if (rc == AEFFT_OK && (rc = net_alloc_t(n, &n->grad, goff + 2 * (size_t)n->L)) == AEFFT_OK && (rc = net_alloc_t(n, &n->sp_ws, maxWs)) == AEFFT_OK &&
        (rc = net_alloc_t(n, &n->sp_rq, maxRq)) == AEFFT_OK && (rc = net_alloc_t(n, &n->sp_sqd, (size_t)SQD_MAX * SQD_BLOCKS)) == AEFFT_OK &&
        (rc = net_alloc_t(n, &n->score_part, B * score_pairs_per_frame(n))) == AEFFT_OK && (rc = net_alloc_t(n, &n->map_part, score_map_strips(n))) == AEFFT_OK &&
        (maxPart == 0 || (rc = net_alloc_t(n, &n->sp_part, maxPart)) == AEFFT_OK) && (maxUp == 0 || (rc = net_alloc_t(n, &n->sp_up, maxUp)) == AEFFT_OK))
        n->grad_n = goff;
    if (rc != AEFFT_OK) { aefft_net_destroy(n); return rc; }
    // zero weights and momentum, and the MSE tail with the L floats behind it (zero before the first step)
    hipError_t e = hipMemsetAsync(n->grad + n->grad_n, 0, sizeof(float) * 2 * n->L, ctx->stream);
    for (const Pair& q : n->pr) {
        if (e == hipSuccess) e = hipMemsetAsync(q.c, 0, 2 * q.nk() * 4, ctx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(q.b, 0, q.dM * 4, ctx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(q.p, 0, q.dD * 4, ctx->stream);
    }
    if (e != hipSuccess) { aefft_net_destroy(n); return fail(ctx, AEFFT_EHIP, "memset weights", e); }
    *out = n;
    return aefft_net_reset_momentum(n);
}

// The forward: per encoder ONE launch (Pool on load, the pooled layer published), per decoder ONE launch (the inner decoder's output
// up-sampled on load; pair 0's also writes the reconstruction).  Shapes the tiled convolutions do not serve decline the fused launch and
// run Pool / Pool(-s) as launches of their own around the plain convolution.
// first > 0 (aefft_net_decode): the encoders from pair `first` on, reading the stored layer 2*first (pair first-1's hidden layer); no frames.
static int sp_run_forward(aefft_net* n, const float* frames_d, float* recon_d, int first = 0)
{
    aefft_ctx* ctx = n->ctx;
    const int L = n->L, B = n->B;
    if (!frames_d && first == 0) return fail(ctx, AEFFT_EINVAL, "aefft_net_forward / step_grad: null frames");
    const float* x = first ? n->pr[first - 1].Lhid : frames_d;
    for (int l = first; l < L; ++l) {
        Pair& q = n->pr[l];
        int ak, al;
        sp_geom(q, &ak, &al);
        const long pin = (long)B * q.dD * q.Nxin * q.Nyin, pout = (long)B * q.Nx * q.Ny;
        const double bytes = ((double)pin + (double)pout * (q.dD + q.dM) + 2.0 * q.nk()) * 4.0;
        const int r = launch_or_decline(ctx, KID_SPATIAL, bytes, "spatial net encoder", [&] {
            return launch_conv_spatial(x, q.Lhid, q.c, q.b, B, q.dD, q.dM, q.Nx, q.Ny, q.Nk, q.Nl, ak, al, (float)q.dM, 0, ctx->cur, q.s, q.Lin);
        });
        if (r == DECLINED) {
            RET_IF(launch_or_fail(ctx, KID_SPATIAL, bytes, "spatial net pool", [&] {
                return launch_pool_spatial(x, q.Lin, (long)B * q.dD, q.Nxin, q.Nyin, q.Nx, q.Ny, q.s, ctx->cur);
            }));
            RET_IF(launch_or_fail(ctx, KID_SPATIAL, bytes, "spatial net encoder", [&] {
                return launch_conv_spatial(q.Lin, q.Lhid, q.c, q.b, B, q.dD, q.dM, q.Nx, q.Ny, q.Nk, q.Nl, ak, al, (float)q.dM, 0, ctx->cur);
            }));
        } else RET_IF(r);
        x = q.Lhid;
    }
    for (int l = L - 1; l >= 0; --l) {
        Pair& q = n->pr[l];
        int ak, al;
        sp_geom(q, &ak, &al);
        const bool inner = l == L - 1;
        const float* in = inner ? q.Lhid : n->pr[l + 1].Lout;        // layer 4L-2-2l: pair l+1's decoder output, up-sampled by s_{l+1} on load
        const int up = inner ? 0 : n->pr[l + 1].s;
        float* rec = l == 0 ? recon_d : nullptr;                      // layer 4L: the same values replicated s_0 x s_0
        const long px = (long)B * q.Nx * q.Ny;
        const double bytes = ((double)px * q.dM / (up ? (double)up * up : 1.0) + (double)px * q.dD * (rec ? 1.0 + (double)q.s * q.s : 1.0) + 2.0 * q.nk()) * 4.0;
        const int r = launch_or_decline(ctx, KID_SPATIAL, bytes, "spatial net decoder", [&] {
            return launch_conv_spatial(in, q.Lout, q.f, q.p, B, q.dM, q.dD, q.Nx, q.Ny, q.Nk, q.Nl, ak, al, (float)q.dD, 0, ctx->cur, 0, nullptr, up, rec, rec ? q.s : 0);
        });
        if (r != DECLINED) { RET_IF(r); continue; }
        if (up > 1) {
            RET_IF(launch_or_fail(ctx, KID_SPATIAL, bytes, "spatial net up-sampling", [&] {
                return launch_pool_spatial(in, n->sp_up, (long)B * q.dM, q.Nx / up, q.Ny / up, q.Nx, q.Ny, -up, ctx->cur);
            }));
            in = n->sp_up;
        }
        RET_IF(launch_or_fail(ctx, KID_SPATIAL, bytes, "spatial net decoder", [&] {
            return launch_conv_spatial(in, q.Lout, q.f, q.p, B, q.dM, q.dD, q.Nx, q.Ny, q.Nk, q.Nl, ak, al, (float)q.dD, 0, ctx->cur);
        }));
        if (rec)
            RET_IF(launch_or_fail(ctx, KID_SPATIAL, bytes, "spatial net reconstruction", [&] {
                return launch_pool_spatial(q.Lout, rec, (long)B * q.dD, q.Nx, q.Ny, q.Nxin, q.Nyin, -q.s, ctx->cur);
            }));
    }
    n->last_frames = frames_d;
    n->last_frames_u8 = false;
    n->have_forward = first == 0;
    return AEFFT_OK;
}

int aefft::sp_forward(aefft_net* n, const float* frames_d, float* recon_d) { return sp_run_forward(n, frames_d, recon_d); }

// aefft_net_decode: the code becomes the stored layer 2l+2 and the coordinate-space sequence runs from there.  No frame stands behind the
// call: a pending step_grad ends and the layer exports wait for the next forward.
int aefft::sp_decode(aefft_net* n, int l, const float* code_d, float* recon_d)
{
    aefft_ctx* ctx = n->ctx;
    const Pair& q = n->pr[l];
    HIPCHK(ctx, hipMemcpyAsync(q.Lhid, code_d, sizeof(float) * n->B * q.dM * q.Nx * q.Ny, hipMemcpyDeviceToDevice, ctx->cur));
    n->have_grad = false;
    return sp_run_forward(n, nullptr, recon_d, l + 1);
}

// forward, then per pair backprop_gpu's batch-mean gradients (in = layer 2l+1, out = layer 4L-1-2l, hin = layer 2l+2) straight into the
// pair's slice of the packed buffer, then the per-pair MSE into the buffer's tail
int aefft::sp_step_grad(aefft_net* n, const float* frames_d, float* recon_d)
{
    aefft_ctx* ctx = n->ctx;
    RET_IF(sp_run_forward(n, frames_d, recon_d));
    const int L = n->L, B = n->B;
    std::vector<int> standalone;       // pairs whose MSE is not formed by their gradient launch
    for (int l = 0; l < L; ++l) {
        Pair& q = n->pr[l];
        const GradSeg gs = q.grads(n->grad);
        SpatialGradArgs a{};
        a.in = q.Lin; a.out = q.Lout; a.hin = q.Lhid; a.f = q.f;
        a.gc = gs.dck; a.gf = gs.dfk; a.gb = gs.db; a.gp = gs.dp;
        a.ws = n->sp_ws;
        a.part = spatial_partial_floats(B, q.dD, q.dM, q.Nx, q.Ny, q.Nk, q.Nl) ? n->sp_part : nullptr;
        a.rq = n->sp_rq;
        a.B = B; a.dD = q.dD; a.dM = q.dM; a.Nx = q.Nx; a.Ny = q.Ny; a.Nk = q.Nk; a.Nl = q.Nl;
        sp_geom(q, &a.ak, &a.al);
        a.lo = 0;
        a.Norm = sp_norm(q);           // untied: step_apply(sym = 1) halves (backproplib.cu:533)
        a.tied = 0;
        // every hidden layer is its pair's own Conv_gpu of the pair's input: dF, dP from the error-input region sums
        // ... and the region launch, which stages s0 = out - in once per pixel, sums the pair's MSE into the tail slot as well
        if (spatial_regions_ok(a)) { a.c1 = q.c; a.b1 = q.b; a.div1 = (float)q.dM; a.mse = n->grad + n->grad_n + l; }
        else standalone.push_back(l);
        const double px = (double)B * q.Nx * q.Ny;
        RET_IF(launch_or_fail(ctx, KID_SPATIAL, px * ((a.c1 ? 2.0 : 3.0) * q.dD + (a.c1 ? 0.0 : 1.0) * q.dM) * 4.0, "spatial net gradient",
                              [&] { return launch_spatial_grad(a, ctx->cur); }));
    }
    // tail: sum (in - out)^2 / Norm / B per pair (backproplib.cu:346-356), before the update as the reference forms it; the pairs off the
    // region route by a standalone fixed-order reduction (their gradient launches read s0 as a GEMM operand, once per tap-shifted column block
    // and block of hidden maps: no launch reads each pixel once)
    const int ns = (int)standalone.size();
    for (int k0 = 0; k0 < ns; k0 += SQD_MAX) {
        SqdiffGroup g{};
        g.count = std::min(SQD_MAX, ns - k0);
        double bytes = 0;
        for (int k = 0; k < g.count; ++k) {
            const int l = standalone[k0 + k];
            const Pair& q = n->pr[l];
            g.a[k] = q.Lin; g.b[k] = q.Lout; g.n[k] = (long)B * q.dD * q.Nx * q.Ny;
            g.scale[k] = (float)(1.0 / ((double)sp_norm(q) * B));
            g.dst[k] = n->grad + n->grad_n + l;
            bytes += 8.0 * g.n[k];
        }
        RET_IF(launch_or_fail(ctx, KID_DIFFMSE, bytes, "spatial net mse", [&] { return launch_sqdiff_group(g, n->sp_sqd, ctx->cur); }));
    }
    n->have_grad = true;
    return AEFFT_OK;
}

// backprop_gpu's update of every pair from the (all-reduced) buffer: g = buffer * grad_scale (x 1/2 with sym), del0 as delmax directly
// (autoencoder.cpp:87,178); the tail is scaled by the same factor in place (as FFT nets leave it, an all-reduce of it times 1/world gives
// the global mean), saved behind the buffer and written to mse_d
int aefft::sp_step_apply(aefft_net* n, float del0, int maxdiff, int sym, float grad_scale, float* mse_d)
{
    aefft_ctx* ctx = n->ctx;
    if (maxdiff) return fail(ctx, AEFFT_EINVAL, "aefft_net_step_apply: maxdiff != 0 -- the spatial mode has no multiobjective term");
    if (!n->have_grad) return fail(ctx, AEFFT_ESTATE, "aefft_net_step_apply: call aefft_net_step_grad first");
    const int L = n->L;
    const float gs = sym ? 0.5f * grad_scale : grad_scale;
    RET_IF(launch_or_fail(ctx, KID_UPDATE, 12.0 * L, "spatial net mse tail", [&] {
        return launch_scale_tail(n->grad + n->grad_n, n->grad + n->grad_n + L, mse_d, L, gs, ctx->cur);
    }));
    for (int l0 = 0; l0 < L; l0 += 8) {
        UpdateGroup ug{};
        ug.n = std::min(8, L - l0);
        double bytes = 0;
        for (int k = 0; k < ug.n; ++k) {
            Pair& q = n->pr[l0 + k];
            const GradSeg g = q.grads(n->grad);
            ug.a[k] = mk_update(q.c, q.f, q.b, q.p, g.dck, g.dfk, g.db, g.dp, Momentum{q.Dc, q.Df, q.Db, q.Dp}, q.dM, q.dD, q.Nk, q.Nl, del0, sym,
                                grad_scale, nullptr);
            ug.a[k].alpha = n->alpha;
            bytes += (double)q.nk() * 4.0 * 8;
        }
        RET_IF(launch_or_fail(ctx, KID_UPDATE, bytes, "spatial net update", [&] { return launch_update_group(ug, ctx->cur); }));
    }
    n->have_grad = false;
    return AEFFT_OK;
}

int aefft::sp_last_mse(aefft_net* n, float* mse_d)
{
    HIPCHK(n->ctx, hipMemcpyAsync(mse_d, n->grad + n->grad_n + n->L, sizeof(float) * n->L, hipMemcpyDeviceToDevice, n->ctx->stream));
    return AEFFT_OK;
}

// every layer 0..4L of the last forward / step_grad; the up-sampled decoder layers 4L-2l by the Pool(-s) kernel from the stored 4L-1-2l
int aefft::sp_get_layer(aefft_net* n, int layer, float* out_d, int* ch, int* nx, int* ny)
{
    aefft_ctx* ctx = n->ctx;
    const int L = n->L;
    int c, x, y;
    const float* src = nullptr;
    const Pair* up = nullptr;
    if (layer == 0) { c = n->D; x = n->Nx; y = n->Ny; src = n->last_frames; }
    else if (layer <= 2 * L) {
        const Pair& q = n->pr[(layer - 1) / 2];
        x = q.Nx; y = q.Ny;
        if (layer & 1) { c = q.dD; src = q.Lin; } else { c = q.dM; src = q.Lhid; }
    } else if (layer & 1) {
        const Pair& q = n->pr[(4 * L - 1 - layer) / 2];
        c = q.dD; x = q.Nx; y = q.Ny; src = q.Lout;
    } else {
        const Pair& q = n->pr[(4 * L - layer) / 2];
        c = q.dD; x = q.Nxin; y = q.Nyin; up = &q;
    }
    if (ch) *ch = c;
    if (nx) *nx = x;
    if (ny) *ny = y;
    if (!out_d) return AEFFT_OK;
    if (!n->have_forward) return fail(ctx, AEFFT_ESTATE, "aefft_net_get_layer: no forward pass yet");
    if (up)
        return launch_or_fail(ctx, KID_SPATIAL, (double)n->B * c * ((double)up->Nx * up->Ny + (double)x * y) * 4.0, "get_layer: up-sampling", [&] {
            return launch_pool_spatial(up->Lout, out_d, (long)n->B * c, up->Nx, up->Ny, x, y, -up->s, ctx->stream);
        });
    HIPCHK(ctx, hipMemcpyAsync(out_d, src, sizeof(float) * n->B * c * x * y, hipMemcpyDeviceToDevice, ctx->stream));
    return AEFFT_OK;
}

extern "C" int aefft_net_set_inertia(aefft_net* n, float alpha)
{
    if (!n) return AEFFT_EINVAL;
    if (!n->spatial) return fail(n->ctx, AEFFT_EINVAL, "aefft_net_set_inertia: only a spatial net (AEFFT_NET_SPATIAL) has an inertia weight");
    if (!(alpha >= 0.f && alpha <= 1.f)) return fail(n->ctx, AEFFT_EINVAL, "aefft_net_set_inertia: alpha must lie in [0, 1]");
    n->alpha = alpha;
    return AEFFT_OK;
}
