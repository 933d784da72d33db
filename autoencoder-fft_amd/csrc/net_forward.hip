// C-ABI layer (include/aefft.h), the resident network's forward: net_forward and its stages, the operator chain and the bin-major record it
// reads (ensure_packed, fill_chain), the reconstruction (launch_recon), the per-frame expansion of an operator-form step (ensure_frames), and
// the entry points that only run forward: aefft_net_forward*, aefft_net_infer, aefft_net_decode.  The read-outs of the reconstruction
// (aefft_net_score and its kin): net_score.hip.  Bursts and the training step: net_step.hip.
#include "net.h"

#include <algorithm>

using namespace aefft;

// problems of the spectra launch that serve the operator chain: Cc_l for l < L-1 (C sampled where the next pair's grid lands)
int aefft::cc_problems(aefft_net* n, PrunedGroup& pg, int first, double* bytes)
{
    int k = first;
    for (int l = 0; l + 1 < n->L; ++l) {
        Pair& q = n->pr[l];
        const Pair& nx = n->pr[l + 1];
        pg.q[k] = PrunedProb{q.c, q.Cc, (long)q.dM * q.dD, nx.Nx, nx.Ny, 1.0f, q.Nx, q.Ny};
        if (bytes) *bytes += (double)q.dM * q.dD * (nx.P * 8.0 + q.Nk * q.Nl * 4.0);
        ++k;
    }
    return k;
}

// the bin-major record Wp (and the compact Cc planes) of the CURRENT weights
int aefft::ensure_packed(aefft_net* n)
{
    if (!n->Wp || n->packed_valid) return AEFFT_OK;
    aefft_ctx* ctx = n->ctx;
    double bytes = (double)n->pack.Pc * n->pack.E * 8.0;
    PrunedGroup pg{};
    if (n->pr[0].Cc) {
        pg.n = cc_problems(n, pg, 0, &bytes);
        n->pack.upd = 0;
    }
    RET_IF(launch_or_fail(ctx, KID_KSPEC, bytes, "kspec_packed", [&] {
        return n->pr[0].Cc ? launch_kspec_group(pg, ctx->tw, n->pr[0].Nk, n->pr[0].Nl, ctx->cur, &n->pack, nullptr) : launch_kspec_packed(n->pack, ctx->cur);
    }));
    n->packed_valid = true;
    return AEFFT_OK;
}

// the training step's forward runs as ONE chain launch on the basis frames (chain_kernel): with the bin-major record, decoder outputs on the coarsest grid's support, and under these switches
bool aefft::chain_form(const aefft_net* n) { return n->Wp && (n->compact || n->L == 1) && !(dev_flags & (AEFFT_F_NOCHAIN | AEFFT_F_NOLAZY | AEFFT_F_NOCOMPACT | AEFFT_F_NOGROUP | AEFFT_F_NOMFMA | AEFFT_F_NOFUSECROP)); }

// The training step runs in operator form (opform_kernels.hip) when every pair has the Q-path gradient (equal square 3x3 / 5x5
// supports with pruned transforms) and the input has at most OPC-1 channels.
bool aefft::op_eligible(const aefft_net* n)
{
    // (op_shapes with its channel limits: a launch declined in the middle of step_apply would leave a fused update half applied)
    if (flag(AEFFT_F_NOOPFORM) || flag(AEFFT_F_NOQPATH) || !n->A0hat || !op_shapes(n)) return false;
    // (grids with a smooth axis: only on a net created with AEFFT_NET_SMOOTH_OPFORM -- the record and the reconstruction then take N-point
    // phase tables and the mixed-radix column pass -- and, by pruned_supported, not under AEFFT_F_NOPRUNESMOOTH)
    for (const Pair& q : n->pr)
        if (!q.Q || !(pruned_pow2(q.Nx, q.Ny) || n->smooth_opform) || !pruned_supported(q.Nk, q.Nl, q.Nx, q.Ny)) return false;
    return true;
}

// operator form: pair l's operators of the step in progress -- the chain form's own buffers, or the activation buffers
OpView aefft::op_view(const aefft_net* n, int l)
{
    const Pair& q = n->pr[l];
    if (n->op_chain) return OpView{l == 0 ? n->A0hat : q.opA[n->op_fwd], q.opO[n->op_fwd], n->NxC, n->NyC, n->Pc};
    const OutView v = out_view(n, q);
    return OpView{q.X, v.O, v.nx, v.ny, v.P};
}
void aefft::fill_chain(aefft_net* n, ChainArgs& ca, int set, double* bytes)
{
    const int L = n->L;
    const bool cc = L == 1 || n->pr[0].Cc != nullptr;
    for (int l = 0; l < L; ++l) {
        Pair& q = n->pr[l];
        ca.lv[l] = ChainLevel{q.C, q.F, q.b, q.p, l == 0 ? n->A0hat : q.opA[set], q.opO[set], q.dD, q.dM, q.Nx, q.Ny, q.P, cc ? q.Cc : nullptr};
        const double cb = (l + 1 < L) ? (double)n->pr[l + 1].P : (double)q.P;
        if (bytes) *bytes += ((double)q.dM * q.dD * (cb + n->Pc) + (double)OPC * q.dD * (q.P + n->Pc)) * 8.0;
    }
    ca.L = L; ca.D0 = n->D; ca.Pc = n->Pc; ca.Wp = n->Wp; ca.E = n->pack.E;
}

// the reconstruction's inverse FFT (fft_backproplib.cu:1373) on ctx->cur; operator form: the per-frame spectra are expanded first
// out_u8: recon_d is unsigned char, written as 8-bit pixels by the row pass
// score: the row pass (or, behind the any-size transforms, score_diff_kernel) leaves the row-pair sums of the squared difference to score->frames
int aefft::launch_recon(aefft_net* n, void* recon_d, int wsid, bool out_u8, const ScoreArg* score)
{
    aefft_ctx* ctx = n->ctx;
    Pair& q = n->pr[0];
    const OutView fv = out_view(n, q);
    const OpView ov = op_mode(n) ? op_view(n, 0) : OpView{nullptr, fv.O, fv.nx, fv.ny, 0};
    const float2* src = ov.O;
    const int nxo = ov.nxo, nyo = ov.nyo;
    if (op_mode(n)) {
        static_assert(OPIN_COLS == OPC, "operator width");
        const long PO = bins(nxo, nyo);
        if ((double)n->B * q.dD * PO * 8.0 > AEFFT_X_RECON_EXPAND_BYTES) {
            // large supports (no pooling: the decoder output lives on the whole grid): the per-frame spectra O_0,b = O^_0 [x_b; 1] are
            // written out once by a coalesced pass (7 plane-ordered loads per output) and the inverse transform reads them back.  Evaluated
            // inside the column pass instead, the same 7 loads are strided 128-byte pieces: 1.1 ms against 0.2 ms at cfg3-P1.
            // (sized at creation for the grid the default routes leave O^_0 on; a development switch that moves it to a larger grid on a live
            // net grows the buffer here, once)
            const size_t need = (size_t)n->B * q.dD * PO;
            if (need > n->recon_exp_n) { RET_IF(net_alloc_t(n, &n->recon_exp, need)); n->recon_exp_n = need; }
            RET_IF(launch_or_fail(ctx, KID_OPFORM, ((double)OPC * q.dD * PO + (double)n->B * q.dD * PO + (double)n->B * q.dD * q.P) * 8.0, "recon_expand",
                                  [&] { return launch_recon_expand(src, n->Xf, n->recon_exp, n->B, q.dD, q.Nx, q.Ny, nxo, nyo, ctx->cur); }));
            return do_c2r(ctx, n->recon_exp, recon_d, (long)n->B * q.dD, nxo, nyo, n->Nx, n->Ny, 1.0f / ((float)n->Nx * (float)n->Ny), wsid, nullptr, out_u8, score);
        }
        // small supports: O_0,b = O^_0 [x_b; 1] is evaluated inside the column pass of the inverse transform (no stored planes)
        const OpIn op{src, n->Xf, q.dD, q.Nx, q.Ny};
        return do_c2r(ctx, nullptr, recon_d, (long)n->B * q.dD, nxo, nyo, n->Nx, n->Ny, 1.0f / ((float)n->Nx * (float)n->Ny), wsid, &op, out_u8, score);
    }
    return do_c2r(ctx, src, recon_d, (long)n->B * q.dD, nxo, nyo, n->Nx, n->Ny, 1.0f / ((float)n->Nx * (float)n->Ny), wsid, nullptr, out_u8, score);
}

// How net_forward runs, decided in front of its first launch.
struct FwdPlan {
    bool chain;        // the whole network on the basis frames in one launch (chain_kernel)
    bool chain_cc;     // ... reading the bin-major record Wp and the compact Cc planes only
    bool need_chain;   // ... and the operators of the current weights are not at hand (first step, weights set from outside)
    bool prefetch;     // the input transform runs on the side stream aux[1] (aefft_net_set_input_ready)
    bool async;        // the reconstruction runs on the side stream aux[0]
    bool defer;        // ... launched by aefft_net_step_grad after the gradient half (pipelined mode)
    bool want_fork;    // ... forked behind the last launch in front of the gradient kernels
};

// infer: frozen-weight inference (aefft_net_infer) -- everything on the context stream, whatever the pipelining switches say
static FwdPlan forward_plan(const aefft_net* n, bool recon, bool lazy, bool op, bool infer)
{
    const aefft_ctx* ctx = n->ctx;
    FwdPlan f{};
    // the whole network on the basis frames in one launch (chain_kernel): hidden layers not materialised, decoder outputs on the
    // coarsest grid's support, operators in their own buffers
    f.chain = op && lazy && chain_form(n);
    // (the chain launch reads the bin-major record Wp and the compact Cc planes only: planar spectra that a training step in operator
    // form does not refresh are formed when something else asks for them)
    f.chain_cc = f.chain && (n->L == 1 || n->pr[0].Cc != nullptr);
    f.need_chain = f.chain && !n->chain_valid;
    f.prefetch = lazy && n->input_ready && n->X0alt && ctx->aux[1] != nullptr && !ctx->prof && !flag(AEFFT_F_NOPREFETCH);
    // (reconstructions beyond ~256 MB -- 32 frames of 1024^2 -- stay on the context stream: beside their row pass the pruned inverse transform
    // of S stretches from 42 to 145 us and the side stream costs more than it hides, 1.084 vs 1.057 ms per cfg5 step; at cfg3 it saves 15 of 203 us)
    // ... and reconstructions below ~8 MB (cfg2: one 256^2 frame, 11 us of kernels) stay there as well: the fork and join packets cost more than the
    // two kernels they would hide (0.074 vs 0.076 ms per cfg2 step)
    const double recon_bytes = (double)n->B * n->D * n->Nx * n->Ny * 4.0;
    const bool overlap_pays = recon_bytes <= 256e6 && (recon_bytes >= 8e6 || flag(AEFFT_F_SMALLOVERLAP));
    f.async = lazy && ctx->aux[0] != nullptr && !flag(AEFFT_F_NOOVERLAP) && overlap_pays && !ctx->prof;
    f.defer = f.async && n->input_ready && !flag(AEFFT_F_NODEFER);
    // the reconstruction's side stream forks behind the last launch in front of the gradient kernels -- the input transform's column
    // pass, or the chain launch when the operators of the current weights are not at hand (first step, weights set from outside) --
    // through that dispatch's own completion signal
    f.want_fork = f.chain && recon && f.async && !f.defer && ctx->cur == ctx->stream;
    if (infer) f.prefetch = f.async = f.defer = f.want_fork = false;
    return f;
}

// R2C of the frames fused with pair 0's pooling, into the input spectra Xf.  *forked: ctx->ev_fork is recorded behind it.
static int forward_input(aefft_net* n, const float* frames_d, bool u8, const FwdPlan& plan, bool* forked)
{
    aefft_ctx* ctx = n->ctx;
    const long planes = (long)n->B * n->D;
    const Pair& q0 = n->pr[0];
    if (!plan.prefetch) {
        const bool fork_r2c = plan.want_fork && !plan.need_chain;
        RET_IF(do_r2c(ctx, frames_d, n->Xf, planes, n->Nx, n->Ny, q0.Nx, q0.Ny, WS_MID, fork_r2c ? ctx->ev_fork : nullptr, u8));
        *forked = fork_r2c;
        return AEFFT_OK;
    }
    // The caller guarantees the frames are complete: their R2C goes to a side stream and may overlap the tail of the previous
    // step.  It writes the OTHER input-spectra buffer (the current one is still read by that tail), which was last read two
    // steps ago: wait for that step's end only.
    std::swap(n->Xf, n->X0alt);
    if (n->ev_end_valid[n->step_no & 1]) HIPCHK(ctx, hipStreamWaitEvent(ctx->aux[1], n->ev_end[n->step_no & 1], 0));
    // not earlier than the end of the previous step's gradient half: that is where a data-parallel run waits for its
    // all-reduce (an otherwise idle gap), and what follows on this stream (update, spectra, MSE) is latency-bound
    if (n->ev_mid_valid) HIPCHK(ctx, hipStreamWaitEvent(ctx->aux[1], n->ev_mid, 0));
    {
        OnStream on(ctx, ctx->aux[1]);
        RET_IF(do_r2c(ctx, frames_d, n->Xf, planes, n->Nx, n->Ny, q0.Nx, q0.Ny, WS_MID2, nullptr, u8));
    }
    HIPCHK(ctx, hipEventRecord(n->ev_r2c, ctx->aux[1]));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, n->ev_r2c, 0));
    return AEFFT_OK;
}

// the chain launch, unless the previous step's tail launch already ran it on the current weights
static int forward_chain(aefft_net* n, const FwdPlan& plan, bool* forked)
{
    if (plan.need_chain) {
        aefft_ctx* ctx = n->ctx;
        RET_IF(ensure_packed(n));
        ChainArgs ca{};
        double bytes = 0;
        fill_chain(n, ca, n->op_set, &bytes);
        const bool fork_here = plan.want_fork && !*forked;
        RET_IF(launch_or_fail(ctx, KID_CHAIN, bytes, "chain", [&] { return launch_chain(ca, ctx->cur, fork_here ? ctx->ev_fork : nullptr); }));
        *forked = *forked || fork_here;
        n->chain_valid = true;
    }
    n->op_fwd = n->op_set;
    for (Pair& q : n->pr) { q.H_stale = true; q.O_stale = q.P != n->Pc; }      // (what ensure_frames leaves in the activation buffers)
    return AEFFT_OK;
}

// pool -> conv per pair; B columns of the activation buffers
// first: the pair to start at, its input X already in place (aefft_net_decode: no frame stands behind the call, so the innermost pair
// does not take the collapsed operator's route either -- that launch also forms gradient terms of EVERY pair's input)
static int forward_encoder(aefft_net* n, int B, bool lazy, bool op, int first = 0)
{
    aefft_ctx* ctx = n->ctx;
    const int L = n->L;
    for (int l = first; l < L; ++l) {
        Pair& q = n->pr[l];
        // the next pair's spectral down-sampling (pool_fft, :1346) is written by this conv's epilogue: no resize launch
        const bool fuse = (l + 1 < L) && n->pr[l + 1].s != 1 && n->fuse_crop && !flag(AEFFT_F_NOFUSECROP);
        q.H_stale = false;
        if (lazy && !op && first == 0 && l == L - 1 && q.G_valid && !flag(AEFFT_F_NOGFWD)) {
            // innermost pair of a training step: its hidden layer feeds only its own decoder conv, and the previous step left
            // the collapsed operator of the CURRENT weights behind (G = F.C/(dM dD) in S, DC bias in beta): O = G X + beta below,
            // a quarter of the arithmetic and bytes of conv_k o conv_k, no H.
            q.H_stale = true;
            continue;
        }
        if (fuse && lazy) {
            const bool nolazy = flag(AEFFT_F_NOLAZY);
            const Pair& nx = n->pr[l + 1];
            bool done = false;
            if (!nolazy) RET_IF(do_conv_pooled(ctx, q.X, q.C, q.b, nx.X, B, q.dM, q.dD, q.Nx, q.Ny, nx.Nx, nx.Ny, &done));
            if (done) { q.H_stale = true; continue; }
        }
        if (fuse) { const Pair& nx = n->pr[l + 1]; RET_IF(do_conv(ctx, q.X, q.C, q.b, q.H, B, q.dM, q.dD, q.Nx, q.Ny, nx.X, nx.Nx, nx.Ny)); }
        else RET_IF(do_conv(ctx, q.X, q.C, q.b, q.H, B, q.dM, q.dD, q.Nx, q.Ny));
        if (!fuse && l + 1 < L && n->pr[l + 1].s != 1) {
            const Pair& nx = n->pr[l + 1];
            RET_IF(do_resize(ctx, q.H, nx.X, (long)B * nx.dD, nx.Nxin, nx.Nyin, nx.Nx, nx.Ny));
        }
    }
    return AEFFT_OK;
}

// innermost decoder output on the G route: O = G X + beta, one contraction
static int decoder_inner_g(aefft_net* n, int B, bool compact)
{
    Pair& q = n->pr[n->L - 1];
    Contract k{};
    k.A = q.G; k.a_r = (long)q.dD * q.P; k.a_k = q.P;
    k.B = q.X; k.b_k = q.P; k.b_c = (long)q.dD * q.P;
    k.Out = q.O; k.o_r = q.P; k.o_c = (long)q.dD * q.P;
    k.R = q.dD; k.C = B; k.K = q.dD; k.P = q.P;
    k.bias = q.beta; k.biasScale = (float)q.Nx * (float)q.Ny; k.biasAfterFirst = true;
    // the batch-first gradient term S = -sum_b X X^H needs only the encoder outputs: it shares this launch
    // (the decoder chain that follows is a sequence of small dependent launches)
    n->xx_done = false; n->ox_done = 0;
    if (compact && n->pr[0].P != n->Pc && n->L + 1 <= 8 && !flag(AEFFT_F_NOGROUP)) {
        Contract qs[8];
        qs[0] = k;
        for (int l2 = 0; l2 < n->L; ++l2) { Pair& q2 = n->pr[l2]; qs[1 + l2] = mk_XXneg(q2.X, q2.S, B, q2.dD, q2.P); }
        RET_IF(do_contract_group(n->ctx, qs, n->L + 1, n->L + 1, 0));
        n->xx_done = true;
        return AEFFT_OK;
    }
    return do_contract(n->ctx, k);
}

// Up-sampled spectra are zero outside the image of the coarsest grid, and conv_k maps zero to zero (the bias sits on
// the DC bin, inside it): every decoder output lives on those Pc bins.  The training step computes and stores only them:
//   Oc_l[b][d][s] = sum_m F_l[d][m][map_l(s)] * Oc_{l+1}[b][m][s] / dD + p[d] Nx Ny [s == 0]
// DECLINED: shapes the contraction does not serve.
static int decoder_compact(aefft_net* n, int l, int B, bool op)
{
    aefft_ctx* ctx = n->ctx;
    Pair& q = n->pr[l];
    const Pair& in = n->pr[l + 1];
    Contract k{};
    k.A = q.F; k.a_r = (long)q.dM * q.P; k.a_k = q.P;
    k.B = in.Oc; k.b_k = n->Pc; k.b_c = (long)q.dM * n->Pc;
    k.Out = q.Oc; k.o_r = n->Pc; k.o_c = (long)q.dD * n->Pc;
    k.R = q.dD; k.C = B; k.K = q.dM; k.P = n->Pc;
    k.preDivB = (float)q.dD;
    k.bias = q.p; k.biasScale = (float)q.Nx * (float)q.Ny; k.biasAfterFirst = true;
    k.gdNx = q.Nx; k.gdNy = q.Ny; k.gdNxs = n->NxC; k.gdNys = n->NyC; k.gdMask = 1;
    if (n->xx_done && !op && !flag(AEFFT_F_NOGROUP) && !flag(AEFFT_F_NOMFMA)) {
        // S = -sum_b X X^H is already out: the support term of the NEXT-inner pair (its decoder output is final) rides along
        Pair& qi = n->pr[l + 1];
        Contract qs[2] = {k, mk_OX(n, qi, B)};
        RET_IF(do_contract_group(ctx, qs, 2, 2, 0));
        n->ox_done |= 1u << (l + 1);
        return AEFFT_OK;
    }
    return launch_or_decline(ctx, KID_CONTRACT, ((double)k.R * k.K + (double)k.K * k.C + (double)k.R * k.C) * k.P * 8.0, "contract(compact decoder)",
                             [&] { return launch_contract(bc(ctx, k), ctx->cur); });
}

// decoder (:1356-1361): conv then zero-pad up-sampling.  The up-sampled tensor is never stored: the next
// decoder conv (and the final C2R) read the small spectrum through the zero-pad index map.
static int forward_decoder(aefft_net* n, int B, bool lazy, bool op)
{
    aefft_ctx* ctx = n->ctx;
    const int L = n->L;
    const bool nocompact = flag(AEFFT_F_NOCOMPACT);
    bool compact = lazy && n->compact && !nocompact && L > 1;
    Pair& qi = n->pr[L - 1];
    qi.O_stale = false;
    if (qi.H_stale) RET_IF(decoder_inner_g(n, B, compact));      // (set by the encoder: G route)
    else RET_IF(do_conv(ctx, qi.H, qi.F, qi.p, qi.O, B, qi.dD, qi.dM, qi.Nx, qi.Ny));
    for (int l = L - 2; l >= 0; --l) {
        Pair& q = n->pr[l];
        const Pair& in = n->pr[l + 1];
        q.O_stale = false;
        if (compact && q.P != n->Pc) {
            const int rc = decoder_compact(n, l, B, op);
            if (rc == AEFFT_OK) { q.O_stale = true; continue; }
            if (rc != DECLINED) return rc;
            // declined: from here down the full-grid decoder; the levels already done are expanded first
            n->compact = compact = false;
            for (int l2 = L - 2; l2 > l; --l2) {
                Pair& q2 = n->pr[l2];
                RET_IF(do_resize(ctx, q2.Oc, q2.O, (long)B * q2.dD, n->NxC, n->NyC, q2.Nx, q2.Ny));
                q2.O_stale = false;
            }
        }
        RET_IF(do_conv_up(ctx, in.O, q.F, q.p, q.O, B, q.dD, q.dM, q.Nx, q.Ny, in.Nx, in.Ny));
    }
    return AEFFT_OK;
}

// :1373 fft_inv of the up-sampled last output, fused zero-pad
static int forward_recon(aefft_net* n, float* recon_d, const FwdPlan& plan, bool forked)
{
    aefft_ctx* ctx = n->ctx;
    n->recon_deferred = nullptr;
    if (plan.defer) {
        // pipelined loop (aefft_net_set_input_ready): launched by aefft_net_step_grad after the gradient half instead
        n->recon_deferred = recon_d;
        return AEFFT_OK;
    }
    if (plan.async) {
        // training step: nothing downstream reads the reconstruction, so its (bandwidth-bound) inverse FFT runs on a side
        // stream underneath the latency-bound gradient contractions; aefft_net_step_grad joins it before returning
        if (!forked) HIPCHK(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->aux[0], ctx->ev_fork, 0));
    }
    {
        // (a side-stream transform has its own column/row workspace: the main stream's FFTs of non-pruned kernel supports use WS_MID)
        OnStream on(ctx, plan.async ? ctx->aux[0] : ctx->cur);
        RET_IF(launch_recon(n, recon_d, plan.async ? WS_MID3 : WS_MID));
    }
    n->recon_pending = plan.async;
    return AEFFT_OK;
}

// lazy: encoder outputs that are only consumed through pool_fft are computed on the pooled grid alone (the bins the crop
// discards are never formed; aefft_net_get_layer recomputes such a layer on demand).  The training step uses it.
// op: run the network on the OPC basis frames (the activation buffers then hold the per-bin operators A_l, O^_l) -- the
// frames themselves only go through the input transform, the second moments and the reconstruction.
// u8: the frames are 8-bit pixels (the input transform converts on load).
// infer: the call is aefft_net_infer's -- no side streams, and in the operator form without the chain launch the layers are not evaluated
// again while the activation buffers still hold the operators of the current weights (ops_valid).
int aefft::net_forward(aefft_net* n, const float* frames_d, bool u8, float* recon_d, bool lazy, bool op, bool infer)
{
    if (!n || !frames_d) return fail(n ? n->ctx : nullptr, AEFFT_EINVAL, "aefft_net_forward: bad argument");
    aefft_ctx* ctx = n->ctx;
    const int B = op ? (int)OPC : n->B;        // columns of the activation buffers
    BiasColGuard bias_col(ctx, op ? (int)OPC : 0);     // conv_k biases: the affine column only
    RET_IF(join_recon(ctx));
    n->xx_done = false; n->ox_done = 0;
    n->upd_after_fwd = false;
    const FwdPlan plan = forward_plan(n, recon_d != nullptr, lazy, op, infer);
    const bool reuse_ops = infer && op && !plan.chain && n->ops_valid && n->op_state;
    n->ops_valid = false;
    n->op_state = op && !plan.chain;
    n->op_chain = plan.chain;
    n->act_stale = plan.chain;
    for (int l = 0; l < n->L; ++l) if (!(plan.chain_cc || (plan.chain && l == n->L - 1 && n->L > 1))) RET_IF(ensure_spectra(n, n->pr[l]));
    // encoder (fft_backproplib.cu:1340-1357): R2C fused with pair 0's pooling, then pool -> conv per pair
    bool forked = false;
    RET_IF(forward_input(n, frames_d, u8, plan, &forked));
    n->pr[0].X = n->op_state ? n->A0hat : n->Xf;
    if (plan.chain) RET_IF(forward_chain(n, plan, &forked));
    else if (!reuse_ops) {
        RET_IF(forward_encoder(n, B, lazy, op));
        RET_IF(forward_decoder(n, B, lazy, op));
    }
    n->ops_valid = n->op_state;        // (the operators of the weights as they are now)
    if (recon_d) RET_IF(forward_recon(n, recon_d, plan, forked));
    n->last_frames = frames_d; n->last_frames_u8 = u8;
    n->have_forward = true; n->have_grad = false;
    return AEFFT_OK;
}

// Layer exports and bursts read per-frame spectra: after a training step in operator form the activation buffers hold operators,
// so the per-frame forward of the same frames is run first (with the CURRENT weights; the step's gradient state is kept).
int aefft::ensure_frames(aefft_net* n)
{
    if (n->op_chain && n->act_stale) {
        // chain mode: X_l,b = A_l [x_b; 1], O_l,b = O^_l [x_b; 1] from the RESIDENT input spectra and the operators of the last
        // step_grad (set op_fwd: intact until the step after next's tail launch) -- neither the caller's frame buffer nor the
        // current (possibly updated) weights enter.  Hidden layers stay to be formed on request (H_stale).
        aefft_ctx* ctx = n->ctx;
        const Pair& q0 = n->pr[0];
        for (int l = 0; l < n->L; ++l) {
            Pair& q = n->pr[l];
            const double rows = (double)OPC * q.dD + (double)n->B * (q.dD + n->D);
            if (l > 0)
                RET_IF(launch_or_fail(ctx, KID_OPFORM, rows * q.P * 8.0, "op_expand",
                                      [&] { return launch_op_expand(q.opA[n->op_fwd], n->Xf, q.X, n->B, n->D, q.dD, q0.Nx, q0.Ny, q.Nx, q.Ny, ctx->cur); }));
            RET_IF(launch_or_fail(ctx, KID_OPFORM, rows * n->Pc * 8.0, "op_expand", [&] {
                return launch_op_expand(q.opO[n->op_fwd], n->Xf, q.P != n->Pc ? q.Oc : q.O, n->B, n->D, q.dD, q0.Nx, q0.Ny, n->NxC, n->NyC, ctx->cur);
            }));
            q.H_stale = true; q.O_stale = q.P != n->Pc;
        }
        n->pr[0].X = n->Xf;
        n->act_stale = false;
        return AEFFT_OK;
    }
    if (!n->op_state) return AEFFT_OK;
    // (operator form without the chain launch: the activation buffers hold the operators themselves; the per-frame forward of the
    // same frames is run -- the caller's frame buffer must still hold them, include/aefft.h)
    const bool hg = n->have_grad;
    RET_IF(net_forward(n, n->last_frames, n->last_frames_u8, nullptr, false, false));
    n->have_grad = hg;
    return AEFFT_OK;
}

extern "C" int aefft_net_forward(aefft_net* n, const float* frames_d, float* recon_d)
{
    if (n && n->spatial) return sp_forward(n, frames_d, recon_d);
    RET_IF(net_forward(n, frames_d, false, recon_d, false));
    return mark_step_point(n);
}

// 8-bit frames: the same calls with the input transform converting on load (fft_kernels.hip r2c_rows_kernel<N, true>); nothing else reads the frames
extern "C" int aefft_net_forward_u8(aefft_net* n, const unsigned char* frames_d, float* recon_d)
{
    if (!n) return AEFFT_EINVAL;
    if (n->spatial) return sp_refuse(n, "aefft_net_forward_u8");
    RET_IF(net_forward(n, reinterpret_cast<const float*>(frames_d), true, recon_d, false));
    return mark_step_point(n);
}

// ------------------------------------------------------------------------------------------
// frozen-weight inference (include/aefft.h aefft_net_infer)
// ------------------------------------------------------------------------------------------
// Pair l's hidden layer of all B frames in the operator form: H^_l = C_l A_l / dM + bias is formed once per weight set and pair (Hhat), the
// frames' planes are H^_l [x_b; 1] (launch_op_expand into the pair's own hidden buffer) and go through the inverse transform.
static int infer_hidden_op(aefft_net* n, int l, float* hidden_d)
{
    aefft_ctx* ctx = n->ctx;
    Pair& q = n->pr[l];
    const Pair& q0 = n->pr[0];
    if (!n->hid_valid || n->hid_pair != l) {
        // the planar encoder spectrum: where the step keeps the planar spectra stale (spectra_valid false) the buffer is free, and stays
        // marked stale -- the step's own choice between the planar F and the bin-major record is not touched
        if (!q.spectra_valid) RET_IF(do_pad_r2c(ctx, q.c, q.C, nullptr, (long)q.dM * q.dD, q.Nx, q.Ny, q.Nk, q.Nl));
        n->hid_valid = false;
        RET_IF(launch_or_fail(ctx, KID_OPFORM, ((double)q.dM * q.dD + (double)OPC * (q.dD + q.dM)) * q.P * 8.0, "hidden_op",
                              [&] { return launch_hidden_op(q.C, op_view(n, l).A, q.b, n->Hhat, q.dM, q.dD, q.Nx, q.Ny, ctx->cur); }));
        n->hid_pair = l; n->hid_valid = true;
    }
    // (operator form without the chain launch: a next pair that is not pooled keeps its input operator in this buffer)
    if (n->op_state && l + 1 < n->L && n->pr[l + 1].X == q.H) n->ops_valid = false;
    RET_IF(launch_or_fail(ctx, KID_OPFORM, ((double)OPC * q.dM + (double)n->B * (q.dM + n->D)) * q.P * 8.0, "op_expand(hidden)",
                          [&] { return launch_op_expand(n->Hhat, n->Xf, q.H, n->B, n->D, q.dM, q0.Nx, q0.Ny, q.Nx, q.Ny, ctx->cur); }));
    q.H_stale = true;          // (a later layer export forms the layer from the pair's input as usual)
    return do_c2r(ctx, q.H, hidden_d, (long)n->B * q.dM, q.Nx, q.Ny, q.Nx, q.Ny, 1.0f / ((float)q.Nx * (float)q.Ny));
}

extern "C" int aefft_net_infer(aefft_net* n, const void* frames_d, int frames_u8, void* recon_d, int recon_u8, int hidden_pair, float* hidden_d)
{
    if (!n) return AEFFT_EINVAL;
    aefft_ctx* ctx = n->ctx;
    if (!frames_d || (!recon_d && !hidden_d)) return fail(ctx, AEFFT_EINVAL, "aefft_net_infer: null frames, or neither output asked for");
    if (hidden_d && (hidden_pair < 0 || hidden_pair >= n->L)) return fail(ctx, AEFFT_EINVAL, "aefft_net_infer: hidden_pair outside 0..L-1");
    if (!aligned16p(frames_d) || !aligned16p(recon_d) || !aligned16p(hidden_d)) return fail(ctx, AEFFT_EINVAL, "aefft_net_infer: pointers must be 16-byte aligned");
    if (n->spatial) {
        if (frames_u8 || recon_u8) return sp_refuse(n, "aefft_net_infer with 8-bit frames or pixels");
        RET_IF(sp_forward(n, static_cast<const float*>(frames_d), static_cast<float*>(recon_d)));
        if (hidden_d) {
            const Pair& q = n->pr[hidden_pair];
            HIPCHK(ctx, hipMemcpyAsync(hidden_d, q.Lhid, sizeof(float) * n->B * q.dM * q.Nx * q.Ny, hipMemcpyDeviceToDevice, ctx->cur));
        }
        return mark_step_point(n);
    }
    // the form the training step runs in (aefft_net_step_form): operators of the current weights where they are at hand, the frames
    // through the input transform and the inverse transform alone; the per-frame forward in its lazy form otherwise
    const bool op = op_eligible(n);
    RET_IF(net_forward(n, static_cast<const float*>(frames_d), frames_u8 != 0, nullptr, true, op, true));
    if (recon_d) RET_IF(launch_recon(n, recon_d, WS_MID, recon_u8 != 0));
    if (hidden_d) {
        if (op) RET_IF(infer_hidden_op(n, hidden_pair, hidden_d));
        else RET_IF(aefft_net_get_layer(n, 2 * hidden_pair + 2, hidden_d, nullptr, nullptr, nullptr));      // formed on request from the pair's input
    }
    return mark_step_point(n);
}

// ------------------------------------------------------------------------------------------
// decode (include/aefft.h aefft_net_decode): layer 4L from a stored layer 2l+2
// ------------------------------------------------------------------------------------------
// T^_l of the CURRENT weights (decode_kernels.hip), cached until the weights or the pair change
static int ensure_decode_op(aefft_net* n, int l)
{
    if (n->dec_valid && n->dec_pair == l) return AEFFT_OK;
    aefft_ctx* ctx = n->ctx;
    const int L = n->L;
    if (!n->That || !n->dec_ws) return fail(ctx, AEFFT_ESTATE, "aefft_net_decode: operator form on a net created without the decode buffers");      // (cannot happen: net_create sizes them by op_shapes, which op_eligible holds)
    // the planar spectra: where the step keeps them stale (spectra_valid false) the buffers are free, and stay marked stale -- the step's own
    // choice between the planar spectra and the bin-major record is not touched (as infer_hidden_op)
    for (int j = 0; j < L; ++j) if (!n->pr[j].spectra_valid) RET_IF(pair_spectra(n, n->pr[j]));
    DecodeOpArgs g{};
    double bytes = 0;
    for (int j = 0; j < L; ++j) {            // e_d^T F_0 F_1 .. F_{L-1}
        const Pair& q = n->pr[j];
        g.st[g.nst++] = DecodeStage{q.F, q.p, q.dD, q.dM, q.Nx, q.Ny, q.P, 1.0f / (float)q.dD, (float)q.Nx * (float)q.Ny};
    }
    for (int j = L - 1; j > l; --j) {        // .. C_{L-1} .. C_{l+1}
        const Pair& q = n->pr[j];
        g.st[g.nst++] = DecodeStage{q.C, q.b, q.dM, q.dD, q.Nx, q.Ny, q.P, 1.0f / (float)q.dM, (float)q.Nx * (float)q.Ny};
    }
    for (int s = 0; s < g.nst; ++s) bytes += (double)g.st[s].K * g.st[s].M * n->Pc * 8.0;
    // (stride, thread count and rows of T as net_create allocated them: launch_decode_op holds every stage's row against these)
    g.T = n->That; g.ws = n->dec_ws; g.D = n->D; g.NxC = n->NxC; g.NyC = n->NyC; g.Pc = n->Pc; g.NT = n->dec_nt; g.maxW = n->dec_w; g.Tw = n->dec_w;
    n->dec_valid = false;
    RET_IF(launch_or_fail(ctx, KID_OPFORM, bytes + (double)n->D * (n->pr[l].dM + 1) * n->Pc * 8.0, "decode_op", [&] { return launch_decode_op(g, ctx->cur); }));
    n->dec_pair = l; n->dec_valid = true;
    return AEFFT_OK;
}

// OPERATOR / OPERATOR_CHAIN: R2C of the code cropped to the coarsest grid (into the pair's own hidden buffer), T^_l applied per bin into
// pair 0's compact decoder output, the reconstruction's sparse inverse transform: five launches
static int decode_operator(aefft_net* n, int l, const float* code_d, void* recon_d, bool out_u8)
{
    aefft_ctx* ctx = n->ctx;
    Pair& q = n->pr[l];
    Pair& q0 = n->pr[0];
    RET_IF(ensure_decode_op(n, l));
    RET_IF(do_r2c(ctx, code_d, q.H, (long)n->B * q.dM, q.Nx, q.Ny, n->NxC, n->NyC));
    RET_IF(launch_or_fail(ctx, KID_OPFORM, ((double)n->D * (q.dM + 1) + (double)n->B * (q.dM + n->D)) * n->Pc * 8.0, "decode_apply",
                          [&] { return launch_decode_apply(n->That, q.H, q0.Oc, n->B, n->D, q.dM, n->Pc, ctx->cur); }));
    // (the two activation buffers written: in the operator form without the chain launch they held operators of the current weights;
    // the chain form's operator sets are buffers of their own)
    n->ops_valid = false;
    return do_c2r(ctx, q0.Oc, recon_d, (long)n->B * n->D, n->NxC, n->NyC, n->Nx, n->Ny, 1.0f / ((float)n->Nx * (float)n->Ny), WS_MID, nullptr, out_u8);
}

// PER_FRAME: R2C of the code straight onto the next pair's grid (its pooling is the transform's fused crop), the lazy per-frame forward
// from there, the reconstruction
static int decode_per_frame(aefft_net* n, int l, const float* code_d, void* recon_d, bool out_u8)
{
    aefft_ctx* ctx = n->ctx;
    const int L = n->L;
    Pair& q = n->pr[l];
    BiasColGuard bias_col(ctx, 0);
    n->xx_done = false; n->ox_done = 0;
    n->op_state = false; n->op_chain = false; n->act_stale = false; n->ops_valid = false;
    for (int j = 0; j < L; ++j) RET_IF(ensure_spectra(n, n->pr[j]));
    if (l + 1 < L) {
        const Pair& nx = n->pr[l + 1];       // (scale 1: nx.X is q.H and the grids are equal)
        RET_IF(do_r2c(ctx, code_d, nx.X, (long)n->B * q.dM, q.Nx, q.Ny, nx.Nx, nx.Ny));
        q.H_stale = nx.X != q.H;
        RET_IF(forward_encoder(n, n->B, true, false, l + 1));
    } else {
        RET_IF(do_r2c(ctx, code_d, q.H, (long)n->B * q.dM, q.Nx, q.Ny, q.Nx, q.Ny));
        q.H_stale = false;
    }
    RET_IF(forward_decoder(n, n->B, true, false));
    return launch_recon(n, recon_d, WS_MID, out_u8);
}

extern "C" int aefft_net_decode(aefft_net* n, int hidden_pair, const float* code_d, void* recon_d, int recon_u8)
{
    if (!n) return AEFFT_EINVAL;
    aefft_ctx* ctx = n->ctx;
    if (!code_d || !recon_d) return fail(ctx, AEFFT_EINVAL, "aefft_net_decode: null code or reconstruction");
    if (hidden_pair < 0 || hidden_pair >= n->L) return fail(ctx, AEFFT_EINVAL, "aefft_net_decode: hidden_pair outside 0..L-1");
    if (!aligned16p(code_d) || !aligned16p(recon_d)) return fail(ctx, AEFFT_EINVAL, "aefft_net_decode: pointers must be 16-byte aligned");
    if (n->spatial) {
        if (recon_u8) return sp_refuse(n, "aefft_net_decode with 8-bit pixels");
        return sp_decode(n, hidden_pair, code_d, static_cast<float*>(recon_d));
    }
    RET_IF(join_recon(ctx));
    // no frame stands behind the call: a pending step_grad ends, and the layer exports wait for the next forward
    n->have_grad = false; n->have_forward = false;
    n->recon_deferred = nullptr;
    if (op_eligible(n)) RET_IF(decode_operator(n, hidden_pair, code_d, recon_d, recon_u8 != 0));
    else RET_IF(decode_per_frame(n, hidden_pair, code_d, recon_d, recon_u8 != 0));
    // (the call reads no input spectra; the end-of-step event is recorded behind it all the same, as aefft_net_infer does, so that a
    // decode that one day does cannot race the prefetched input transform)
    return mark_step_point(n);
}
