// C-ABI layer (include/aefft.h), the resident network in training: bursts (aefft_net_train_pair), the gradient half (grads_grouped) and
// the update half (apply_grouped, the post-update MSE) of the training step, input prefetch, and the aefft_net_step_* / set_input_ready /
// last_mse / grad_buffer entry points.  The forward they start from is in net_forward.hip.
#include "net.h"

#include <algorithm>

using namespace aefft;

// every pair has pair 0's kernel support (Nk, Nl), and a pruned transform of it
static bool shared_supports(const aefft_net* n)
{
    for (const Pair& q : n->pr) if (!pruned_supported(q.Nk, q.Nl, q.Nx, q.Ny)) return false;
    return same_supports(n);
}

// G'_l = F_l.C_l / (dM dD) [dD][dD][P] of the STORED weights of every pair, into Pair::G: the spectrum of the (2Nk-1)^2-tap kernel f (*) c, taps
// formed inside the transforming workgroups (gspec_gbody).  false: shapes not served.
static int gprime_from_taps(aefft_net* n, bool* done)
{
    *done = false;
    aefft_ctx* ctx = n->ctx;
    if (n->L > 8 || !qpath_support(n->pr[0].Nk, n->pr[0].Nl) || !same_supports(n)) return AEFFT_OK;
    PrunedGroup pg{};
    GtapsGroup tg{};
    double bytes = 0;
    const int TT = (2 * n->pr[0].Nk - 1) * (2 * n->pr[0].Nk - 1);
    bool chunked = false;                                  // some plane is transformed by several row-chunk workgroups: the taps are formed once, in a launch in front
    for (int l = 0; l < n->L; ++l) {
        Pair& q = n->pr[l];
        if (!pruned_supported(q.Nk, q.Nl, q.Nx, q.Ny) || (double)q.dD * q.dD * q.P * 8.0 >= 4294967296.0) return AEFFT_OK;
        pg.q[l] = PrunedProb{nullptr, q.G, (long)q.dD * q.dD, q.Nx, q.Ny, 1.0f, 0, 0};
        pg.gsrc[l] = GtapSrc{q.c, q.f, q.dM, q.dD, 1.0f / ((float)q.dM * (float)q.dD)};
        bytes += (double)q.dD * q.dD * q.P * 8.0 + 2.0 * q.dM * q.dD * q.Nk * q.Nl * 4.0;
        chunked = chunked || q.Nx > 64;
    }
    if (chunked) {
        // taps once per plane, then their spectra as an ordinary pruned transform of (2Nk-1)^2-tap kernels (its own kernel instantiation:
        // the planar-spectra launch keeps its code)
        if (!n->gtaps) {
            size_t nt = 0;
            for (const Pair& q : n->pr) nt += (size_t)q.dD * q.dD * TT;
            RET_IF(net_alloc_t(n, &n->gtaps, nt));
        }
        PrunedGroup pt{};
        float* o = n->gtaps;
        for (int l = 0; l < n->L; ++l) {
            const Pair& q = n->pr[l];
            tg.gs[l] = pg.gsrc[l]; tg.out[l] = o;
            pt.q[l] = PrunedProb{o, q.G, (long)q.dD * q.dD, q.Nx, q.Ny, 1.0f, 0, 0};
            o += (size_t)q.dD * q.dD * TT;
        }
        tg.n = pt.n = n->L;
        const int rc = launch_or_decline(ctx, KID_KSPEC, bytes, "G'(stored taps)", [&] {
            const hipError_t e = launch_gtaps_group(tg, n->pr[0].Nk, ctx->cur);
            return e == hipSuccess ? launch_kspec_group_taps(pt, ctx->tw, 2 * n->pr[0].Nk - 1, ctx->cur) : e;
        });
        *done = rc == AEFFT_OK;
        if (rc != DECLINED) return rc;
        // (shapes these launches do not serve: taps formed in the transforming workgroups, below)
    }
    pg.n = n->L;
    const int rc = launch_or_decline(ctx, KID_KSPEC, bytes, "G'(taps)",
                                     [&] { return launch_kspec_group(pg, ctx->tw, n->pr[0].Nk, n->pr[0].Nl, ctx->cur, nullptr, nullptr); });
    *done = rc == AEFFT_OK;
    return rc == DECLINED ? AEFFT_OK : rc;
}

// Does the post-update MSE take G' = F.C/(dM dD) from the stored taps (gprime_from_taps)?  HBM-sized kernel spectra (no pooling): the MSE
// would read all 2*dM*dD planes of C|F back (6 GB at cfg3-P1), while the spectrum of the (2Nk-1)^2-tap kernel f (*) c (weight_kernels.hip)
// reads the kernels and writes dD*dD planes, read once.  Cache-sized ones: a per-bin contraction of the spectra (measured faster there).
static bool gprime_taps_pay(const aefft_net* n)
{
    if (flag(AEFFT_F_NOQPATH)) return false;
    double cf_bytes = 0;
    for (const Pair& q : n->pr) cf_bytes += 2.0 * q.dM * q.dD * q.P * 8.0;
    return cf_bytes > 256e6 || flag(AEFFT_F_GTAPS);
}

// expand a decoder output that the training-step forward kept on its support only
static int ensure_O(aefft_net* n, Pair& q)
{
    if (!q.O_stale) return AEFFT_OK;
    RET_IF(do_resize(n->ctx, q.Oc, q.O, (long)n->B * q.dD, n->NxC, n->NyC, q.Nx, q.Ny));
    q.O_stale = false;
    return AEFFT_OK;
}

// The slot sums of the last step's post-update MSE when aefft_net_step_apply was told not to deliver them (mse_d == NULL): they ride as a
// trailing workgroup of the next step's gradient launch (grads_grouped); anything else that needs them first calls this.
static int mse_flush(aefft_net* n)
{
    if (!n->mse_pending) return AEFFT_OK;
    aefft_ctx* ctx = n->ctx;
    RET_IF(launch_or_fail(ctx, KID_DIFFMSE, 4.0 * n->L * MSE_SLOTS, "mse_finish(deferred)", [&] {
        return launch_mse_finish(n->mse_slots, n->mse_post, nullptr, n->L, ctx->cur, nullptr, n->grad + n->grad_n, n->mse_pending_scale);
    }));
    n->mse_pending = false;
    return AEFFT_OK;
}

// dc|df spectra of pair q -> its dck|dfk taps (inverse transform and shrink to the kernel support)
static int shrink_dcdf(aefft_net* n, const Pair& q)
{
    aefft_ctx* ctx = n->ctx;
    const GradSeg gs = q.grads(n->grad);
    const long planes = (long)q.dM * q.dD;
    if (q.part && pruned_supported(q.Nk, q.Nl, q.Nx, q.Ny)) return do_c2r_shrink(ctx, q.dc, gs.dck, nullptr, q.part, 2 * planes, q.Nx, q.Ny, q.Nk, q.Nl);   // dc|df -> dck|dfk, one launch
    RET_IF(do_c2r_shrink(ctx, q.dc, gs.dck, n->real, nullptr, planes, q.Nx, q.Ny, q.Nk, q.Nl));
    return do_c2r_shrink(ctx, q.df, gs.dfk, n->real, nullptr, planes, q.Nx, q.Ny, q.Nk, q.Nl);
}

// gradient half of one loop-body iteration on pair q: needs X (= T, autoencoder.cpp:194) and the current O.
static int pair_grad(aefft_net* n, Pair& q)
{
    const GradSeg gs = q.grads(n->grad);
    RET_IF(ensure_O(n, q));
    RET_IF(do_gradient(n->ctx, q.X, q.X, q.O, q.C, q.F, q.b, q.S, q.dc, q.df, gs.db, gs.dp, n->B, q.dM, q.dD, q.Nx, q.Ny));
    return shrink_dcdf(n, q);
}

// update half: weights, new spectra, re-forward of the pair alone, post-update MSE accumulated into *mse_slot (pre-zeroed)
static int pair_apply(aefft_net* n, Pair& q, float del, int maxdiff, int sym, float gscale, float* mse_slot)
{
    aefft_ctx* ctx = n->ctx;
    const GradSeg gs = q.grads(n->grad);
    RET_IF(do_update(ctx, q.c, q.f, q.b, q.p, gs.dck, gs.dfk, gs.db, gs.dp, Momentum{q.Dc, q.Df, q.Db, q.Dp},
                     q.dM, q.dD, q.Nk, q.Nl, del, maxdiff, sym, gscale, n->burst ? nullptr : mse_slot));
    RET_IF(pair_spectra(n, q));
    // re-forward of this pair alone (fft_backproplib.cu:1460-1461) and its MSE (:1463)
    RET_IF(do_conv(ctx, q.X, q.C, q.b, q.H, n->B, q.dM, q.dD, q.Nx, q.Ny));
    RET_IF(do_conv(ctx, q.H, q.F, q.p, q.O, n->B, q.dD, q.dM, q.Nx, q.Ny));
    if (mse_slot) RET_IF(do_diff_mse(ctx, q.X, q.O, nullptr, mse_slot, nullptr, n->B, q.dM, q.dD, q.Nx, q.Ny));
    return AEFFT_OK;
}

extern "C" int aefft_net_train_pair(aefft_net* n, int l, int n_iter, float del0, int maxdiff, int sym, float* mse_h)
{
    if (!n || l < 0 || l >= n->L || n_iter < 0) return fail(n ? n->ctx : nullptr, AEFFT_EINVAL, "aefft_net_train_pair: bad argument");
    if (n->spatial) return sp_refuse(n, "aefft_net_train_pair");
    n->upd_after_fwd = false;
    aefft_ctx* ctx = n->ctx;
    if (!n->have_forward) return fail(ctx, AEFFT_ESTATE, "aefft_net_train_pair: run aefft_net_forward first (the burst trains on its layers)");
    RET_IF(mse_flush(n));
    RET_IF(join_recon(ctx));
    RET_IF(ensure_frames(n));
    Pair& q = n->pr[l];
    RET_IF(ensure_spectra(n, q));
    RET_IF(ensure_O(n, q));
    if ((size_t)(n_iter + 1) > n->mse_cap) {
        float* nm;
        RET_IF(net_alloc_t(n, &nm, (size_t)n_iter + 1));
        n->mse_dev = nm; n->mse_cap = (size_t)n_iter + 1;
    }
    const size_t nk = q.nk();
    // momentum lives only inside the burst (fft_backproplib.cu:1420-1423)
    HIPCHK(ctx, hipMemsetAsync(q.Dc, 0, nk * 4, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(q.Df, 0, nk * 4, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(q.Db, 0, q.dM * 4, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(q.Dp, 0, q.dD * 4, ctx->stream));
    const float del = 0.1f * del0;                      // :1445
    HIPCHK(ctx, hipMemsetAsync(n->mse_dev, 0, sizeof(float) * (n_iter + 1), ctx->stream));
    RET_IF(do_diff_mse(ctx, q.X, q.O, nullptr, n->mse_dev, nullptr, n->B, q.dM, q.dD, q.Nx, q.Ny));     // :1440
    n->burst = true;
    int rcb = AEFFT_OK;
    for (int it = 0; it < n_iter && rcb == AEFFT_OK; ++it) {
        rcb = pair_grad(n, q);
        if (rcb == AEFFT_OK) rcb = pair_apply(n, q, del, maxdiff, sym, 1.0f, n->mse_dev + it + 1);
    }
    n->burst = false;
    RET_IF(rcb);
    n->have_grad = false;
    if (mse_h) {
        HIPCHK(ctx, hipMemcpyAsync(mse_h, n->mse_dev, sizeof(float) * (n_iter + 1), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    weights_changed(n, &q);         // the burst changed this pair's weights (and used S)
    return mark_step_point(n);
}

// The spectra that stand in gradient_k_io's EXPECTED-OUTPUT role for pair q in the per-frame form: the pair's input (expout = in,
// autoencoder.cpp:194), or for pair 0 of a target step the targets' spectra (aefft_net_step_grad_target)
static const float2* expected_out(const aefft_net* n, const Pair& q) { return (n->target_step && &q == n->pr.data()) ? n->Tf : q.X; }

// Target step: the targets' spectra on pair 0's grid (the input transform with the crop fused, on the context stream: never prefetched),
// then S_0 += sum_b N_b X_b^H with N_b = X_0,b - T_b -- behind the launch that completes S_0 (opform_moments / support_terms), in front of
// its first consumer -- and, for the post-update MSE, K and n2 (target_kernels.hip).  es_0 takes its correction here in the operator
// form only: the per-frame DC-bin workgroups form O - T themselves from expected_out().
static int target_terms(aefft_net* n, const void* targets_d, bool u8)
{
    aefft_ctx* ctx = n->ctx;
    Pair& q = n->pr[0];
    RET_IF(do_r2c(ctx, static_cast<const float*>(targets_d), n->Tf, (long)n->B * n->D, n->Nx, n->Ny, q.Nx, q.Ny, WS_MID, nullptr, u8));
    const double bytes = (2.0 * n->B * n->D + 2.0 * n->D * n->D + (double)n->D * (n->D + 1)) * q.P * 8.0 + q.P * 4.0;
    return launch_or_fail(ctx, KID_TARGET, bytes, "target_terms", [&] {
        return launch_target_terms(n->Xf, n->Tf, q.S, op_mode(n) ? q.es : nullptr, n->tgtK, n->tgtN2, n->B, n->D, q.P, ctx->cur);
    });
}

// Target step: pair 0's post-update MSE is mse_fft(T, O') = |E|^2 - 2 Re(E^H N) + |N|^2 with E = X - O' the residual the step's own
// launches sum; the other two terms go into the pair's slots here, in front of whichever launch sums them.  G (nullable): G'_0 of the
// UPDATED weights where a route left it, else it is formed from the pair's planar spectra; Fdc: F' at the DC bin.
static int target_mse(aefft_net* n, const float2* G, const float2* Fdc, long fdc_stride)
{
    aefft_ctx* ctx = n->ctx;
    Pair& q = n->pr[0];
    TargetMseArgs a{};
    a.G = G; a.Fdc = Fdc; a.fdc_stride = fdc_stride;
    if (!G) {
        RET_IF(ensure_spectra(n, q));
        a.C = q.C; a.F = q.F; a.Fdc = q.F; a.fdc_stride = q.P;
    }
    a.b = q.b; a.p = q.p; a.K = n->tgtK; a.n2 = n->tgtN2; a.slots = mse_slot(n, 0);
    a.dM = q.dM; a.Nx = q.Nx; a.Ny = q.Ny; a.P = q.P;
    a.scale = 1.0f / ((float)(2 * q.dM) * (float)q.Nx * (float)q.Ny * (float)n->B) / ((float)q.dD * q.Nx * q.Ny);   // as mk_gmse
    const double bytes = ((G ? (double)q.dD * q.dD : 2.0 * q.dM * q.dD) + (double)q.dD * (q.dD + 1)) * q.P * 8.0 + q.P * 4.0;
    return launch_or_fail(ctx, KID_TARGET, bytes, "target_mse", [&] { return launch_target_mse(a, q.dD, ctx->cur); });
}

// Step mode runs the same per-pair sequences as pair_grad / pair_apply, phase by phase over ALL pairs, so that
// the independent contractions of a phase (4 x S, 4 x dc + 4 x df, 4 + 4 re-forward convs) go out as one launch each.
static int bias_and_kgrad(aefft_net* n, Pair& q)
{
    RET_IF(ensure_O(n, q));
    aefft_ctx* ctx = n->ctx;
    const GradSeg gs = q.grads(n->grad);
    const float norm = (float)q.Nx * (float)q.Ny, Norm = grad_norm(q.dM, q.dD, q.Nx, q.Ny);
    RET_IF(launch_or_fail(ctx, KID_BIASGRAD, ((double)(q.dM * q.dD + q.dM + q.dD) + 2.0 * n->B * q.dD) * 8.0, "bias_grad",
                          [&] { return launch_bias_grad(q.O, expected_out(n, q), q.F, q.b, q.df, gs.db, gs.dp, n->B, q.dM, q.dD, q.P, norm, Norm, ctx->cur); }));
    return shrink_dcdf(n, q);
}

// dc | df of every pair, four pairs (8 problems) per launch
static int dcdf_batch(aefft_net* n)
{
    Contract qs[8];
    for (int l0 = 0; l0 < n->L; l0 += 4) {
        const int m = std::min(4, n->L - l0);
        for (int i = 0; i < m; ++i) {
            Pair& q = n->pr[l0 + i];
            const float Norm = grad_norm(q.dM, q.dD, q.Nx, q.Ny);
            qs[i] = mk_dc(q.F, q.S, q.dc, n->B, q.dM, q.dD, q.P, Norm);
            qs[m + i] = mk_df(q.C, q.S, q.df, n->B, q.dM, q.dD, q.P, Norm);
        }
        RET_IF(do_contract_group(n->ctx, qs, 2 * m, m, 2));
    }
    return AEFFT_OK;
}

// operator form: the batch moments, S_l = sum_b (O_b - X_b) X_b^H and the DC error sums of every pair from the operators: one launch
static int opform_moments(aefft_net* n)
{
    aefft_ctx* ctx = n->ctx;
    SgradGroup sg{};
    double bytes = ((double)n->B * n->D + (double)OPC * OPC) * n->pr[0].P * 8.0;      // the input spectra in, the moments out
    for (int l = 0; l < n->L; ++l) {
        Pair& q = n->pr[l];
        const OpView ov = op_view(n, l);
        const int nxo = ov.nxo, nyo = ov.nyo;
        sg.q[l] = OpPair{ov.A, ov.O, q.S, q.es, q.dD, q.Nx, q.Ny, nxo, nyo, q.P, bins(nxo, nyo)};
        bytes += ((double)OPC * q.dD * (q.P + bins(nxo, nyo)) + (double)q.dD * q.dD * q.P) * 8.0;
    }
    sg.n = n->L; sg.Xf = n->Xf; sg.Mout = n->Mhat; sg.B = n->B; sg.D0 = n->D; sg.Nx0 = n->pr[0].Nx; sg.Ny0 = n->pr[0].Ny; sg.P0 = n->pr[0].P;
    return launch_or_fail(ctx, KID_SGRAD, bytes, "sgrad", [&] { return launch_msgrad_group(sg, ctx->cur); });
}

// per-frame form: S_l = sum_b (O_b - X_b) X_b^H of every pair, four pairs per launch.  With decoder outputs on the coarsest grid's
// support it is -sum_b X X^H + sum_b Oc X^H, and the forward may have launched either term already (xx_done, ox_done).
static int support_terms(aefft_net* n)
{
    aefft_ctx* ctx = n->ctx;
    Contract qs[8];
    bool comp = false;
    for (int l = 0; l < n->L; ++l) comp = comp || n->pr[l].O_stale;
    for (int l0 = 0; l0 < n->L; l0 += 4) {
        const int m = std::min(4, n->L - l0);
        if (!comp) {
            for (int i = 0; i < m; ++i) { Pair& q = n->pr[l0 + i]; qs[i] = mk_S(q.X, q.X, q.O, q.S, n->B, q.dD, q.P); }
            RET_IF(do_contract_group(ctx, qs, m, m, 1));
            continue;
        }
        if (!n->xx_done) {
            for (int i = 0; i < m; ++i) { Pair& q = n->pr[l0 + i]; qs[i] = mk_XXneg(q.X, q.S, n->B, q.dD, q.P); }
            RET_IF(do_contract_group(ctx, qs, m, m, 1));
        }
        int mo = 0;
        for (int i = 0; i < m; ++i) {
            Pair& q = n->pr[l0 + i];
            if (n->xx_done && (n->ox_done >> (l0 + i) & 1u)) continue;          // rode along with a decoder launch of the forward
            qs[mo++] = mk_OX(n, q, n->B);
        }
        if (mo == 1) RET_IF(do_contract(ctx, qs[0]));
        else if (mo > 1) RET_IF(do_contract_group(ctx, qs, mo, mo, 1));
    }
    return AEFFT_OK;
}

// the DC-bin terms of every pair for the grouped launches (on the Q path they also read the DC error sums es)
static int fill_bias_grads(aefft_net* n, bool op, bool qpath, BiasGradGroup& bg, double* bytes)
{
    for (int l = 0; l < n->L; ++l) {
        Pair& q = n->pr[l];
        const GradSeg gs = q.grads(n->grad);
        const float Norm = grad_norm(q.dM, q.dD, q.Nx, q.Ny);
        const OutView v = out_view(n, q);
        bg.a[l] = BiasGradArgs{v.O, expected_out(n, q), q.F, q.b, qpath ? nullptr : q.df, gs.db, gs.dp, n->B, q.dM, q.dD, q.P,
                               (float)q.Nx * (float)q.Ny, Norm, v.P, qpath ? q.es : nullptr, op ? q.es : nullptr};
        if (!q.spectra_valid) {
            // (operator form: the step left the planar spectra stale; F at the DC bin is record 0 of the
            // bin-major copy -- element (d1*dM + m) of the pair's F segment, stride 1.  Only F is read through P in this form.)
            if (!(op && qpath && n->Wp && n->packed_valid)) return fail(n->ctx, AEFFT_ESTATE, "gradient: stale kernel spectra");
            bg.a[l].F = n->Wp + n->pack.seg[2 * n->L - 1 - l].off;      // (segments: C_0 .. C_{L-1}, F_{L-1} .. F_0)
            bg.a[l].P = 1;
        }
        *bytes += ((double)(q.dM * q.dD + q.dM + q.dD) + 2.0 * n->B * q.dD) * 8.0;
    }
    bg.n = n->L;
    return AEFFT_OK;
}

// grouped weight gradients through Q = pruned inverse transform of S on the (2Nk-1)^2 offsets (weight_kernels.hip): no dc|df spectra
static int wgrads_qpath(aefft_net* n, bool op)
{
    aefft_ctx* ctx = n->ctx;
    BiasGradGroup bg{};
    PrunedGroup pg{};
    WgradGroup wg{};
    double bbytes = 0, kbytes = 0, wbytes = 0;
    RET_IF(fill_bias_grads(n, op, true, bg, &bbytes));
    const int T = 2 * n->pr[0].Nk - 1;
    for (int l = 0; l < n->L; ++l) {
        Pair& q = n->pr[l];
        const GradSeg gs = q.grads(n->grad);
        const size_t nk = q.nk();
        const float Norm = grad_norm(q.dM, q.dD, q.Nx, q.Ny);
        pg.q[l] = PrunedProb{q.S, q.Q, (long)q.dD * q.dD, q.Nx, q.Ny, 1.0f};
        pg.chunks[l] = q.Qn;
        wg.q[l] = WgradProb{q.c, q.f, q.Q, q.es, q.b, gs.dck, gs.dfk, q.dM, q.dD, 1.0f / (Norm * (float)n->B), (float)q.Nx * (float)q.Ny, 1};
        kbytes += (double)q.dD * q.dD * (q.P * 8.0 + T * T * 4.0);
        wbytes += (2.0 * nk + (double)q.dD * q.dD * T * T) * 4.0 + 2.0 * nk * 4.0;
    }
    pg.n = wg.n = n->L;
    // (the DC-bin terms ride along as extra workgroups)
    RET_IF(launch_or_fail(ctx, KID_KGRAD, kbytes + bbytes, "kgrad(group)", [&] { return launch_kgrad_group_taps(pg, ctx->tw, T, ctx->cur, &bg); }));
    for (int l = 0; l < n->L; ++l) wg.q[l].nq = pg.chunks[l];
    if (n->mse_pending) {      // the previous step's MSE sums: one more workgroup of this launch (they reach the packed buffer's tail before the all-reduce)
        wg.fin_slots = n->mse_slots; wg.fin_out = n->mse_post; wg.fin_tail = n->grad + n->grad_n; wg.fin_L = n->L; wg.fin_scale = n->mse_pending_scale;
    }
    RET_IF(launch_or_fail(ctx, KID_WGRAD, wbytes, "wgrad(group)", [&] { return launch_wgrad_taps_group(wg, n->pr[0].Nk, ctx->cur); }));
    n->mse_pending = false;
    return AEFFT_OK;
}

// grouped weight gradients through the dc|df spectra: their contractions, the DC-bin terms, then one pruned inverse transform of
// every pair (pair by pair where that launch declines)
static int wgrads_dcdf(aefft_net* n, bool op)
{
    aefft_ctx* ctx = n->ctx;
    BiasGradGroup bg{};
    PrunedGroup pg{};
    double bbytes = 0, kbytes = 0;
    RET_IF(fill_bias_grads(n, op, false, bg, &bbytes));
    for (int l = 0; l < n->L; ++l) {
        Pair& q = n->pr[l];
        pg.q[l] = PrunedProb{q.dc, q.grads(n->grad).dck, 2L * q.dM * q.dD, q.Nx, q.Ny, 1.0f};
        kbytes += 2.0 * q.dM * q.dD * (q.P * 8.0 + q.Nk * q.Nl * 4.0);
    }
    pg.n = n->L;
    RET_IF(dcdf_batch(n));
    RET_IF(launch_or_fail(ctx, KID_BIASGRAD, bbytes, "bias_grad(group)", [&] { return launch_bias_grad_group(bg, ctx->cur); }));
    const int rc = launch_or_decline(ctx, KID_KGRAD, kbytes, "kgrad(group)",
                                     [&] { return launch_kgrad_group(pg, ctx->tw, n->pr[0].Nk, n->pr[0].Nl, ctx->cur); });
    if (rc != DECLINED) return rc;
    for (const Pair& q : n->pr) RET_IF(shrink_dcdf(n, q));          // bias terms are done; only the transforms pair by pair
    return AEFFT_OK;
}

static int grads_grouped(aefft_net* n, const void* targets_d, bool targets_u8)
{
    const bool op = op_mode(n);
    RET_IF(op ? opform_moments(n) : support_terms(n));
    n->xx_done = false; n->ox_done = 0;
    if (targets_d) RET_IF(target_terms(n, targets_d, targets_u8));
    // DC-bin terms and the pruned inverse transforms of all pairs: one launch each when the pairs share (Nk, Nl)
    const bool same = (op || (n->L > 1 && n->L <= 8 && !flag(AEFFT_F_NOGROUP))) && shared_supports(n);
    if (!same) {
        // pairs with different kernel supports: dc | df per group of pairs, then pair by pair
        RET_IF(dcdf_batch(n));
        for (int l = 0; l < n->L; ++l) RET_IF(bias_and_kgrad(n, n->pr[l]));
        return AEFFT_OK;
    }
    bool qpath = op || (!flag(AEFFT_F_NOQPATH) && qpath_support(n->pr[0].Nk, n->pr[0].Nl));
    for (const Pair& q : n->pr) qpath = qpath && q.Q != nullptr;
    return qpath ? wgrads_qpath(n, op) : wgrads_dcdf(n, op);
}

// post-update MSE of pair q on the current frames (fft_backproplib.cu:1460-1463).  Step mode never reads the
// re-forward's H and O again (the next forward overwrites them), so they are not materialised: G = F.C per bin
// (into the dead S workspace), then one pass over X with the MSE epilogue.  Falls back to conv, conv, diff_mse
// for shapes the lean kernel does not serve (dD == 1 or B == 1).
// With a target, pair 0's fused pass still sums |X - O'|^2 (the caller adds the target's terms: target_mse); the conv, conv, diff_mse
// route compares O' with the target's spectra directly.
static int reforward_mse(aefft_net* n, Pair& q, float* mse_slots, bool* g_left_in_S = nullptr)
{
    if (g_left_in_S) *g_left_in_S = false;
    aefft_ctx* ctx = n->ctx;
    const bool nofuse = flag(AEFFT_F_NOFUSEMSE);
    if (!nofuse && q.dD >= 2 && n->B >= 2) {
        RET_IF(do_contract(ctx, mk_G(q.F, q.C, q.G, q.dM, q.dD, q.P)));
        const Contract m = mk_gmse(q.G, q.X, q.F, q.b, q.p, mse_slots, n->B, q.dM, q.dD, q.Nx, q.Ny);
        const int rc = launch_or_decline(ctx, KID_CONTRACT, contract_bytes(m), "contract(mse)", [&] { return launch_contract(m, ctx->cur); });
        if (rc == AEFFT_OK && g_left_in_S) *g_left_in_S = true;
        if (rc != DECLINED) return rc;
    }
    RET_IF(join_recon(ctx));                                                  // a deferred reconstruction may still be reading q.O (== Oc when P == Pc)
    RET_IF(do_conv(ctx, q.X, q.C, q.b, q.H, n->B, q.dM, q.dD, q.Nx, q.Ny));   // :1460
    RET_IF(do_conv(ctx, q.H, q.F, q.p, q.O, n->B, q.dD, q.dM, q.Nx, q.Ny));   // :1461
    return do_diff_mse(ctx, expected_out(n, q), q.O, nullptr, n->mse_post + (&q - n->pr.data()), nullptr, n->B, q.dM, q.dD, q.Nx, q.Ny);   // :1463
}

// The routes of one aefft_net_step_apply, decided in front of its first launch.  A declined spectra launch drops fused_upd and gp_route.
struct ApplyRoute {
    bool grouped;      // the update and the spectra of every pair in grouped launches
    bool ride;         // operator form: the spectra launch also writes the bin-major copy Wp
    bool fused_upd;    // the tap half of the update rides in the tail launch (opmse)
    bool gp_route;     // the spectra launch writes G' = F'.C'/(dM dD) for every pair but the innermost
    bool skip_inner;   // the spectra launch leaves out the innermost pair's planar spectra
};

static ApplyRoute apply_route(const aefft_net* n, int maxdiff, int sym)
{
    const aefft_ctx* ctx = n->ctx;
    ApplyRoute r{};
    // (with maxdiff: kernel supports the grouped multiobjective launch serves)
    const int kl = n->pr[0].Nk * n->pr[0].Nl;
    r.grouped = n->L > 1 && n->L <= 8 && !flag(AEFFT_F_NOGROUP) && shared_supports(n) && (!maxdiff || kl == 9 || kl == 25 || kl == 49);
    if (!r.grouped) return r;
    r.ride = op_mode(n) && n->Wp != nullptr;                  // the bin-major copy for the next step's chain: same taps, same launch
    // Fused update (operator form, plain gradients): no update launch.  The spectra launch reads every tap THROUGH the pending
    // update (w - clip_step(g, D): TapUpd) and carries the bias half as a trailing workgroup per pair; the taps and their momentum
    // are stored in place by trailing workgroups of the tail launch (tail_kernel) -- nothing in between reads them.
    r.fused_upd = r.ride && !sym && !maxdiff && !flag(AEFFT_F_NOFUSEUPD) && !ctx->prof;
    const Pair& qi = n->pr[n->L - 1];
    const bool inner_on_record = qi.P == n->pack.Pc && qi.dD <= CH_VMAX && qi.dM <= CH_VMAX;
    // Operator form with the chain launch: NO planar spectra are written.  The next step's chain reads the bin-major record Wp
    // and the compact planes Cc_l (C_l where the next pair's grid lands); the post-update MSE reads G'_l = F'_l.C'_l/(dM dD) --
    // dD*dD planes per pair, the spectrum of the (2Nk-1)^2 kernel f' (*) c' whose taps the transforming workgroups form
    // themselves (gspec_gbody) -- and the innermost pair from Wp.  Planar C|F are formed when something else asks (ensure_spectra).
    r.gp_route = r.ride && n->pr[0].Cc != nullptr && 2 * (n->L - 1) <= 8 && chain_form(n) && inner_on_record;
    // Without the compact planes: the innermost pair's PLANAR spectra are not written (the chain, the post-update MSE and the
    // DC-bin gradient terms take that pair from the bin-major record)
    r.skip_inner = !r.gp_route && r.ride && inner_on_record && !flag(AEFFT_F_NOCHAIN) && !flag(AEFFT_F_NOFUSEUPD) && !ctx->prof;
    return r;
}

// multiobjective terms (fft_backproplib.cu:709-753) of every pair in one grouped launch; their outputs and the chunk partial sums
// live in per-net buffers (allocated the first time maxdiff is asked for)
static int gdiff_grouped(aefft_net* n, GdiffGroup& gd)
{
    aefft_ctx* ctx = n->ctx;
    const int kl = n->pr[0].Nk * n->pr[0].Nl;
    if (!n->gd_out) {
        size_t no = 0, np_ = 0;
        for (const Pair& q : n->pr) { no += 2 * (size_t)q.dM * q.dD * kl + q.dM + q.dD; np_ += gradient_diff_ws_floats(q.dM, q.dD, q.Nk, q.Nl); }
        RET_IF(net_alloc_t(n, &n->gd_out, no));
        RET_IF(net_alloc_t(n, &n->gd_part, np_));
    }
    float *o = n->gd_out, *pw = n->gd_part;
    double gbytes = 0;
    for (int l = 0; l < n->L; ++l) {
        Pair& q = n->pr[l];
        const size_t nk = (size_t)q.dM * q.dD * kl;
        gd.q[l] = GdiffProb{q.c, q.f, q.b, q.p, o, o + nk, o + 2 * nk, o + 2 * nk + q.dM, pw, q.dM, q.dD, 0, 0};
        o += 2 * nk + q.dM + q.dD; pw += gradient_diff_ws_floats(q.dM, q.dD, q.Nk, q.Nl);
        gbytes += (double)nk * 16.0;
    }
    gd.n = n->L;
    return launch_or_fail(ctx, KID_GDIFF, gbytes, "gradient_diff(group)", [&] { return launch_gradient_diff_group(gd, n->pr[0].Nk, n->pr[0].Nl, ctx->cur); });
}

// the grouped update of every pair (gd: with the multiobjective terms); returns its bytes
static double fill_update(aefft_net* n, const GdiffGroup* gd, float del, int sym, float gscale, UpdateGroup& ug)
{
    double bytes = 0;
    for (int l = 0; l < n->L; ++l) {
        Pair& q = n->pr[l];
        const GradSeg gs = q.grads(n->grad);
        ug.a[l] = mk_update(q.c, q.f, q.b, q.p, gs.dck, gs.dfk, gs.db, gs.dp, Momentum{q.Dc, q.Df, q.Db, q.Dp},
                            q.dM, q.dD, q.Nk, q.Nl, del, sym, gscale, n->mse_post + l);
        if (gd) { ug.a[l].cd = gd->q[l].cd; ug.a[l].fd = gd->q[l].fd; ug.a[l].bd = gd->q[l].bd; ug.a[l].pd = gd->q[l].pd; }
        bytes += (double)q.nk() * 4.0 * 8;
    }
    ug.n = n->L;
    return bytes;
}

// problems of the grouped spectra launch: C'|F' of every pair (but the innermost with skip_inner), or on the G' route G'_l and
// the compact planes Cc_l of every pair but the innermost; returns their bytes
static double fill_spectra(aefft_net* n, const ApplyRoute& rt, const TapUpd* tu, PrunedGroup& pg)
{
    double kbytes = 0;
    if (rt.gp_route) {
        int k = 0;
        for (int l = 0; l + 1 < n->L; ++l) {
            Pair& q = n->pr[l];
            pg.q[k] = PrunedProb{nullptr, q.G, (long)q.dD * q.dD, q.Nx, q.Ny, 1.0f, 0, 0};
            pg.gsrc[k] = GtapSrc{q.c, q.f, q.dM, q.dD, 1.0f / ((float)q.dM * (float)q.dD)};
            pg.upd[k] = tu[l];
            kbytes += (double)q.dD * q.dD * q.P * 8.0 + 2.0 * q.dM * q.dD * q.Nk * q.Nl * 4.0;
            ++k;
        }
        const int k0 = k;
        pg.n = cc_problems(n, pg, k0, &kbytes);
        for (int l = 0; l + 1 < n->L; ++l) pg.upd[k0 + l] = tu[l];
        return kbytes;
    }
    for (int l = 0; l < n->L; ++l) {
        Pair& q = n->pr[l];
        pg.q[l] = PrunedProb{q.c, q.C, 2L * q.dM * q.dD, q.Nx, q.Ny, 1.0f};
        pg.upd[l] = tu[l];
        kbytes += 2.0 * q.dM * q.dD * (q.P * 8.0 + q.Nk * q.Nl * 4.0);
    }
    pg.n = n->L;
    if (rt.skip_inner) {
        const Pair& qi = n->pr[n->L - 1];
        pg.n = n->L - 1;
        kbytes -= 2.0 * qi.dM * qi.dD * (qi.P * 8.0 + qi.Nk * qi.Nl * 4.0);
    }
    return kbytes;
}

// the grouped update and the spectra launch of the new weights; a declined spectra launch falls back to the separate update
// and the pair-by-pair transforms
static int update_and_spectra(aefft_net* n, ApplyRoute& rt, UpdateGroup& ug, double ubytes)
{
    aefft_ctx* ctx = n->ctx;
    BiasUpdGroup bu{};
    TapUpd tu[8] = {};
    if (rt.fused_upd) {
        // the taps of every pair are read through TapUpd by the spectra launch, which also applies the bias half (BiasUpd)
        for (int l = 0; l < n->L; ++l) {
            Pair& q = n->pr[l];
            const GradSeg gs = q.grads(n->grad);
            tu[l] = TapUpd{gs.dck, q.Dc, ug.a[l].del, ug.a[l].alpha, ug.a[l].gscale};        // (c|f, dck|dfk, Dc|Df: each pair contiguous)
            bu.a[l] = BiasUpd{q.b, q.p, q.Db, q.Dp, gs.db, gs.dp, n->mse_post + l, q.dM, q.dD};
        }
        bu.n = n->L; bu.del = ug.a[0].del; bu.alpha = ug.a[0].alpha; bu.gscale = ug.a[0].gscale;
        n->pack.upd = 1; n->pack.upd_del = ug.a[0].del; n->pack.upd_alpha = ug.a[0].alpha; n->pack.upd_gscale = ug.a[0].gscale;
    } else {
        n->pack.upd = 0;
        RET_IF(launch_or_fail(ctx, KID_UPDATE, ubytes, "update(group)", [&] { return launch_update_group(ug, ctx->cur); }));
    }
    PrunedGroup pg{};
    const double kbytes = fill_spectra(n, rt, tu, pg);
    const int rc = launch_or_decline(ctx, KID_KSPEC, kbytes + ((op_mode(n) && n->Wp) ? (double)n->pack.Pc * n->pack.E * 8.0 : 0.0), "kspec(group)", [&] {
        return launch_kspec_group(pg, ctx->tw, n->pr[0].Nk, n->pr[0].Nl, ctx->cur, rt.ride ? &n->pack : nullptr, rt.fused_upd ? &bu : nullptr);
    });
    n->pack.upd = 0;
    if (rc == AEFFT_OK) {
        if (rt.ride) n->packed_valid = true;
        if (rt.skip_inner) n->pr[n->L - 1].spectra_valid = false;
        if (rt.gp_route) for (auto& q : n->pr) q.spectra_valid = false;
        else for (int l = 0; l < pg.n; ++l) n->pr[l].spectra_valid = true;
        return AEFFT_OK;
    }
    if (rc != DECLINED) return rc;
    rt.gp_route = false;
    if (rt.fused_upd) {                                               // declined before anything ran: the separate update after all
        rt.fused_upd = false;
        hipError_t e = launch_update_group(ug, ctx->cur);
        if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "update(group)", e);
    }
    for (int l = 0; l < n->L; ++l) RET_IF(pair_spectra(n, n->pr[l]));
    for (auto& q : n->pr) q.spectra_valid = true;
    return AEFFT_OK;
}

static int update_per_pair(aefft_net* n, float del, int maxdiff, int sym, float gscale)
{
    for (int l = 0; l < n->L; ++l) {
        Pair& q = n->pr[l];
        const GradSeg gs = q.grads(n->grad);
        RET_IF(do_update(n->ctx, q.c, q.f, q.b, q.p, gs.dck, gs.dfk, gs.db, gs.dp, Momentum{q.Dc, q.Df, q.Db, q.Dp},
                         q.dM, q.dD, q.Nk, q.Nl, del, maxdiff, sym, gscale, n->mse_post + l));
        RET_IF(pair_spectra(n, q));
        q.spectra_valid = true;
    }
    return AEFFT_OK;
}

// the operator-form MSE problem of every pair: from G'_l where the spectra launch (gp_route) or gprime_from_taps (g_taps) left it,
// else from the updated spectra; the innermost pair from the bin-major copy when that is current
static int fill_opmse(aefft_net* n, bool gp_route, bool g_taps, OpMseGroup& og, double* bytes)
{
    const bool inner_packed = n->Wp && n->packed_valid && n->pr[n->L - 1].P == n->pack.Pc;
    for (int l = 0; l < n->L; ++l) {
        Pair& q = n->pr[l];
        const float scale = 1.0f / ((float)(2 * q.dM) * (float)q.Nx * (float)q.Ny * (float)n->B) / ((float)q.dD * q.Nx * q.Ny);   // as mk_gmse
        OpMsePair o{};
        o.A = op_view(n, l).A; o.C = q.C; o.F = q.F; o.b = q.b; o.p = q.p;
        o.slots = mse_slot(n, l);
        o.dD = q.dD; o.dM = q.dM; o.Nx = q.Nx; o.Ny = q.Ny; o.P = q.P; o.scale = scale;
        if (gp_route && l + 1 < n->L) {
            o.G = q.G; o.Fdc = n->Wp + n->pack.seg[2 * n->L - 1 - l].off; o.fdc_stride = 1;      // (F' at the DC bin: record 0 of the bin-major copy)
            *bytes += ((double)q.dD * q.dD + (double)OPC * q.dD + (double)OPC * OPC) * q.P * 8.0;
        } else if (g_taps && !(l == n->L - 1 && inner_packed)) {
            RET_IF(ensure_spectra(n, q));
            o.G = q.G; o.Fdc = q.F; o.fdc_stride = q.P;                                            // (the planar F', DC bin)
            *bytes += ((double)q.dD * q.dD + (double)OPC * q.dD + (double)OPC * OPC) * q.P * 8.0;
        } else {
            if (!(l == n->L - 1 && inner_packed)) RET_IF(ensure_spectra(n, q));
            *bytes += (2.0 * q.dM * q.dD + (double)OPC * q.dD + (double)OPC * OPC) * q.P * 8.0;
        }
        og.q[l] = o;
    }
    og.n = n->L; og.Mhat = n->Mhat; og.Nx0 = n->pr[0].Nx; og.Ny0 = n->pr[0].Ny; og.P0 = n->pr[0].P;
    if (inner_packed) {      // the innermost pair reads the bin-major copy the kspec launch just refreshed
        og.Wp = n->Wp; og.E = n->pack.E;
        og.offC = n->pack.seg[n->L - 1].off; og.offF = n->pack.seg[n->L].off;
    }
    return AEFFT_OK;
}

// post-update MSE (fft_backproplib.cu:1460-1463) in operator form: R = A - F'(C' A / dM + b^) / dD - p^ per bin, then
// sum_a R[a] M^ R[a]^H; the updated spectra (or their product G') are read once, nothing is stored (opform_kernels.hip).
// wupd: the fused update's tap half, stored by this launch.
static int opform_mse(aefft_net* n, const ApplyRoute& rt, const UpdateGroup* wupd, float gscale, float* mse_d)
{
    aefft_ctx* ctx = n->ctx;
    bool g_taps = false;                                   // G' of EVERY pair at hand (operator form without the chain launch, HBM-sized spectra)
    if (!rt.gp_route && !rt.fused_upd /* the taps are stored */ && gprime_taps_pay(n)) RET_IF(gprime_from_taps(n, &g_taps));
    OpMseGroup og{};
    double bytes = 0;
    RET_IF(fill_opmse(n, rt.gp_route, g_taps, og, &bytes));
    // The NEXT step's operator chain depends on the updated weights only (the record Wp and the planes Cc the spectra launch has just
    // written): it shares this launch, writing the other set of operator buffers, and the next aefft_net_step_grad starts from it.
    const bool ahead = n->op_chain && n->packed_valid && chain_form(n) && !flag(AEFFT_F_NOAHEAD);
    ChainArgs ca{};
    if (ahead) fill_chain(n, ca, n->op_set ^ 1, &bytes);
    RET_IF(launch_or_fail(ctx, KID_OPMSE, bytes, "opmse", [&] { return launch_opmse_group(og, ctx->cur, ahead ? &ca : nullptr, wupd, &n->tail_route); }));
    if (ahead) { n->op_set ^= 1; n->chain_valid = true; }
    // (target step: behind the tail launch -- a fused update stores the taps there, and planar spectra formed on request read them -- and
    // in front of whatever sums the slots)
    if (n->target_step) RET_IF(target_mse(n, og.q[0].G, og.q[0].Fdc, og.q[0].fdc_stride));
    if (!mse_d && !ctx->prof && !flag(AEFFT_F_NOLAZYMSE)) {
        // nobody asked for the sums now: they are formed by one more workgroup of the next step's gradient launch (before its
        // all-reduce), by aefft_net_last_mse, or by whatever needs the slots next -- not by a launch of their own
        n->mse_pending = true; n->mse_pending_scale = gscale;
        return AEFFT_OK;
    }
    return launch_or_fail(ctx, KID_DIFFMSE, 4.0 * n->L * MSE_SLOTS, "mse_finish",
                          [&] { return launch_mse_finish(n->mse_slots, n->mse_post, mse_d, n->L, ctx->cur, nullptr, n->grad + n->grad_n, gscale); });
}

// the re-forward MSE of every pair into its slots: G = F.C of the first 8 pairs the fused form serves in one launch (or from the
// taps), their passes over X in one launch, the other pairs (all of them if that launch declines) through reforward_mse.
// *inner_g: the innermost pair's G belongs to the updated weights.
static int reforward_mse_all(aefft_net* n, bool* inner_g)
{
    aefft_ctx* ctx = n->ctx;
    const bool nofuse = flag(AEFFT_F_NOFUSEMSE), nogroup = flag(AEFFT_F_NOGROUP);
    auto fusable = [&](const Pair& q) { return !nofuse && !nogroup && q.dD >= 2 && n->B >= 2; };
    Contract gq[8], mq[8];
    int m = 0;
    for (int l = 0; l < n->L && m < 8; ++l) {
        Pair& q = n->pr[l];
        if (!fusable(q)) continue;
        gq[m] = mk_G(q.F, q.C, q.G, q.dM, q.dD, q.P);
        mq[m] = mk_gmse(q.G, q.X, q.F, q.b, q.p, mse_slot(n, l), n->B, q.dM, q.dD, q.Nx, q.Ny);
        ++m;
    }
    bool grouped = false;
    if (m > 1) {
        bool gtaps = false;
        if (m == n->L && gprime_taps_pay(n)) RET_IF(gprime_from_taps(n, &gtaps));
        if (!gtaps) RET_IF(do_contract_group(ctx, gq, m, m, 0));
        ContractN g{};
        double bytes = 0;
        for (int i = 0; i < m; ++i) { g.q[i] = mq[i]; bytes += contract_bytes(mq[i]); }
        g.n = m;
        const int rc = launch_or_decline(ctx, KID_CONTRACT, bytes, "contract(mse group)", [&] { return launch_contract_mfma(g, ctx->cur); });
        if (rc != AEFFT_OK && rc != DECLINED) return rc;
        grouped = rc == AEFFT_OK;
    }
    int k = 0;                                 // fusable pairs so far: the first 8 are in the group
    for (int l = 0; l < n->L; ++l) {
        Pair& q = n->pr[l];
        const bool in_group = grouped && fusable(q) && k++ < 8;
        bool left = in_group;
        if (!in_group) RET_IF(reforward_mse(n, q, mse_slot(n, l), &left));
        if (l == n->L - 1) *inner_g = left;
        // (target step: pair 0 went through G'_0 = q.G and summed |X - O'|^2; the cross term and |N|^2 into the same slots)
        if (l == 0 && left && n->target_step) RET_IF(target_mse(n, q.G, q.F, q.P));
    }
    return AEFFT_OK;
}

// post-update MSE (fft_backproplib.cu:1460-1463): G = F.C of every eligible pair in one launch, then every pair's pass
// over X with the MSE epilogue in one launch; pairs the fused form does not serve (dD == 1, B == 1) go pair by pair
static int frame_mse(aefft_net* n, float gscale, float* mse_d)
{
    aefft_ctx* ctx = n->ctx;
    bool inner_g = false;
    RET_IF(reforward_mse_all(n, &inner_g));
    Bracket br(ctx, KID_DIFFMSE, 4.0 * n->L * MSE_SLOTS);
    Pair& ql = n->pr[n->L - 1];
    BetaArgs ba{ql.beta, ql.F, ql.b, ql.p, ql.dM, ql.dD, ql.P};
    const bool want_beta = inner_g && ql.beta && ql.dD <= 256;
    hipError_t e = launch_mse_finish(n->mse_slots, n->mse_post, mse_d, n->L, ctx->cur, want_beta ? &ba : nullptr, n->grad + n->grad_n, gscale);     // also the copy-out to mse_d and to the packed buffer's tail
    ql.G_valid = want_beta && e == hipSuccess;
    if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "mse_finish", e);
    return AEFFT_OK;
}

static int apply_grouped(aefft_net* n, float del, int maxdiff, int sym, float gscale, float* mse_d)
{
    weights_changed(n, nullptr);          // ... are about to (the routes below re-derive what they leave current, and mark it)
    ApplyRoute rt = apply_route(n, maxdiff, sym);
    UpdateGroup ug{};
    if (rt.grouped) {
        GdiffGroup gd{};
        if (maxdiff) RET_IF(gdiff_grouped(n, gd));
        const double ubytes = fill_update(n, maxdiff ? &gd : nullptr, del, sym, gscale, ug);
        RET_IF(update_and_spectra(n, rt, ug, ubytes));
    } else RET_IF(update_per_pair(n, del, maxdiff, sym, gscale));
    if (op_mode(n) && n->Wp) RET_IF(ensure_packed(n));     // the next step's chain reads the bin-major copy of the NEW weights
    if (op_mode(n)) return opform_mse(n, rt, rt.fused_upd ? &ug : nullptr, gscale, mse_d);
    if (rt.fused_upd) return fail(n->ctx, AEFFT_ESTATE, "apply: fused update without the operator-form tail");      // (cannot happen: fused_upd implies op_state)
    return frame_mse(n, gscale, mse_d);
}

// input prefetch bookkeeping: everything of step k that reads this step's input-spectra buffer has been enqueued
int aefft::mark_step_point(aefft_net* n)
{
    if (!n->input_ready || !n->ev_end[0]) return AEFFT_OK;
    HIPCHK(n->ctx, hipEventRecord(n->ev_end[n->step_no & 1], n->ctx->stream));
    n->ev_end_valid[n->step_no & 1] = true;
    return AEFFT_OK;
}

extern "C" int aefft_net_set_input_ready(aefft_net* n, int enable)
{
    if (!n) return AEFFT_EINVAL;
    if (n->spatial) return enable ? sp_refuse(n, "aefft_net_set_input_ready(1)") : AEFFT_OK;
    aefft_ctx* ctx = n->ctx;
    if (enable && !n->X0alt) {
        const Pair& q = n->pr[0];
        RET_IF(net_alloc_t(n, &n->X0alt, (size_t)n->B * q.dD * q.P));
        // (queue-to-queue events of this library only: device scope, host.h AEFFT_X_QUEUE_EVENT_FLAGS)
        for (int i = 0; i < 2; ++i) HIPCHK(ctx, hipEventCreateWithFlags(&n->ev_end[i], AEFFT_X_QUEUE_EVENT_FLAGS));
        HIPCHK(ctx, hipEventCreateWithFlags(&n->ev_r2c, AEFFT_X_QUEUE_EVENT_FLAGS));
        HIPCHK(ctx, hipEventCreateWithFlags(&n->ev_mid, AEFFT_X_QUEUE_EVENT_FLAGS));
    }
    n->input_ready = enable != 0;
    return AEFFT_OK;
}

// targets_d (nullable): the step trains pair 0 toward these frames (aefft_net_step_grad_target)
static int step_grad(aefft_net* n, const float* frames_d, bool u8, float* recon_d, const void* targets_d = nullptr, bool targets_u8 = false)
{
    aefft_ctx* ctx = n->ctx;
    ++n->step_no;
    n->target_step = false;
    RET_IF(net_forward(n, frames_d, u8, recon_d, true, op_eligible(n)));
    n->target_step = targets_d != nullptr;
    {
        int rcg = grads_grouped(n, targets_d, targets_u8);
        if (rcg == AEFFT_OK) rcg = mse_flush(n);      // (a gradient route without the wgrad launch: the deferred MSE sums as their own launch after all)
        if (rcg != AEFFT_OK) { n->recon_deferred = nullptr; return rcg; }
    }
    if (n->recon_deferred) {
        // The reconstruction's inverse FFT starts HERE: where a data-parallel run waits for its all-reduce the GPU is otherwise
        // idle, and what follows on this stream (update, spectra, MSE) is latency-bound.  Joined by aefft_net_step_apply,
        // aefft_sync or the next call on this net.
        float* recon = n->recon_deferred;
        n->recon_deferred = nullptr;
        HIPCHK(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->aux[0], ctx->ev_fork, 0));
        {
            OnStream on(ctx, ctx->aux[0]);
            RET_IF(launch_recon(n, recon, WS_MID3));
        }
        HIPCHK(ctx, hipEventRecord(ctx->ev_join[0], ctx->aux[0]));
        ctx->recon_join = true;
    }
    if (n->recon_pending) {
        // the documented default: recon_d is complete, in stream order on the context stream, when this call's work is
        // (include/aefft.h; the pipelined mode relaxes it).  Joining later -- behind the update half -- was measured: see DESIGN.md 6.
        HIPCHK(ctx, hipEventRecord(ctx->ev_join[0], ctx->aux[0]));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join[0], 0));
        n->recon_pending = false;
    }
    n->have_grad = true;
    if (n->input_ready && n->ev_mid) { HIPCHK(ctx, hipEventRecord(n->ev_mid, ctx->stream)); n->ev_mid_valid = true; }
    return mark_step_point(n);
}

extern "C" int aefft_net_step_grad(aefft_net* n, const float* frames_d, float* recon_d)
{
    if (n && n->spatial) return sp_step_grad(n, frames_d, recon_d);
    return n ? step_grad(n, frames_d, false, recon_d) : AEFFT_EINVAL;
}

// 8-bit frames: the input transform converts on load (fft_kernels.hip r2c_rows_kernel<N, true>); nothing else reads the frames
extern "C" int aefft_net_step_grad_u8(aefft_net* n, const unsigned char* frames_d, float* recon_d)
{
    if (n && n->spatial) return sp_refuse(n, "aefft_net_step_grad_u8");
    return n ? step_grad(n, reinterpret_cast<const float*>(frames_d), true, recon_d) : AEFFT_EINVAL;
}

extern "C" int aefft_net_step_grad_target(aefft_net* n, const void* frames_d, int frames_u8, const void* targets_d, int targets_u8, float* recon_d)
{
    if (!n) return AEFFT_EINVAL;
    aefft_ctx* ctx = n->ctx;
    if (!frames_d || !targets_d) return fail(ctx, AEFFT_EINVAL, "aefft_net_step_grad_target: null frames or targets");
    if (!aligned16p(frames_d) || !aligned16p(targets_d) || !aligned16p(recon_d)) return fail(ctx, AEFFT_EINVAL, "aefft_net_step_grad_target: pointers must be 16-byte aligned");
    if (n->spatial) return sp_refuse(n, "aefft_net_step_grad_target");
    if (n->D > 4) return fail(ctx, AEFFT_EINVAL, "aefft_net_step_grad_target: frames are images of 1 to 4 channels (grey, BGR, BGRA): D must be at most 4");
    if (!n->Tf) {
        // (the first target call of a net: not under stream capture, include/aefft.h)
        const Pair& q = n->pr[0];
        float2 *tf = nullptr, *k = nullptr;
        RET_IF(net_alloc_t(n, &tf, (size_t)n->B * n->D * q.P));
        RET_IF(net_alloc_t(n, &k, (size_t)n->D * (n->D + 1) * q.P));
        RET_IF(net_alloc_t(n, &n->tgtN2, (size_t)q.P));
        n->tgtK = k; n->Tf = tf;
    }
    return step_grad(n, static_cast<const float*>(frames_d), frames_u8 != 0, recon_d, targets_d, targets_u8 != 0);
}

extern "C" int aefft_net_step_form(aefft_net* n)
{
    if (!n) return -1;
    if (n->spatial) return AEFFT_FORM_SPATIAL;
    if (!op_eligible(n)) return AEFFT_FORM_PER_FRAME;
    return chain_form(n) ? AEFFT_FORM_OPERATOR_CHAIN : AEFFT_FORM_OPERATOR;
}

extern "C" int aefft_net_tail_route(aefft_net* n) { return n ? n->tail_route : -1; }

extern "C" int aefft_net_grad_buffer(aefft_net* n, float** buf_d, size_t* nfloats)
{
    if (!n) return AEFFT_EINVAL;
    if (buf_d) *buf_d = n->grad;
    if (nfloats) *nfloats = n->grad_n + (size_t)n->L;
    return AEFFT_OK;
}

extern "C" int aefft_net_last_mse(aefft_net* n, float* mse_d)
{
    if (!n || !mse_d) return AEFFT_EINVAL;
    if (n->spatial) return sp_last_mse(n, mse_d);
    aefft_ctx* ctx = n->ctx;
    RET_IF(mse_flush(n));
    HIPCHK(ctx, hipMemcpyAsync(mse_d, n->mse_post, sizeof(float) * n->L, hipMemcpyDeviceToDevice, ctx->stream));
    return AEFFT_OK;
}

extern "C" int aefft_net_step_apply(aefft_net* n, float del0, int maxdiff, int sym, float grad_scale, float* mse_d)
{
    if (!n) return AEFFT_EINVAL;
    if (n->spatial) return sp_step_apply(n, del0, maxdiff, sym, grad_scale, mse_d);
    aefft_ctx* ctx = n->ctx;
    if (!n->have_grad) return fail(ctx, AEFFT_ESTATE, "aefft_net_step_apply: call aefft_net_step_grad first");
    RET_IF(mse_flush(n));
    const float del = 0.1f * del0;
    RET_IF(apply_grouped(n, del, maxdiff, sym, grad_scale, mse_d));
    n->have_grad = false;
    n->target_step = false;
    n->upd_after_fwd = true;
    RET_IF(join_recon(ctx));
    return mark_step_point(n);
}
