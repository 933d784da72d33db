// C-ABI layer (include/aefft.h), resident network: create / destroy, the weight and spectra accessors, the operator chain's set-up
// (build_chain_items) and the layer exports (aefft_net_get_layer*, aefft_net_layers_layout, aefft_magnitude).  The forward, inference
// and decode are in net_forward.hip, the read-outs of the reconstruction in net_score.hip, the bursts and the training step in net_step.hip.
#include "net.h"

#include <algorithm>
#include <string>
#include <vector>

using namespace aefft;

static bool pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }

// ------------------------------------------------------------------------------------------
// resident network
// ------------------------------------------------------------------------------------------
int aefft::net_alloc(aefft_net* n, void** p, size_t bytes)
{
    hipError_t e = hipMalloc(p, std::max<size_t>(bytes, 256));
    if (e != hipSuccess) return fail(n->ctx, AEFFT_ENOMEM, "hipMalloc(net)", e);
    if (flag(AEFFT_F_POISON)) { (void)hipMemset(*p, 0xFF, std::max<size_t>(bytes, 256)); (void)hipDeviceSynchronize(); }
    n->allocs.push_back(*p);
    return AEFFT_OK;
}

// chain_kernel (opform_kernels.hip) runs the network on the basis frames in one launch; its coarsest-grid workgroups read a
// bin-major copy of the kernel spectra (kspec_packed_kernel).  Served when the coarsest grid is small (large ones stream better
// layer by layer) and the channel counts fit the kernel's LDS tiles.
static int build_chain_items(aefft_net* n)
{
    const int L = n->L;
    bool dims_ok = true;
    for (const Pair& q : n->pr) dims_ok = dims_ok && q.dD <= 128 && q.dM <= 128;
    for (int l = 0; l + 1 < L; ++l) dims_ok = dims_ok && 2 * n->pr[l].dM * (int)OPC * 8 <= 6144;
    if (!dims_ok || n->pr[L - 1].P > 16384) return AEFFT_OK;
    // the bin-major copy for the coarsest-grid items: C_0 .. C_{L-1}, F_{L-1} .. F_0 in chain order, segments padded to even sizes
    bool pk = qpath_support(n->pr[0].Nk, n->pr[0].Nl) && same_supports(n) && 2 * L <= 16;
    for (const Pair& q : n->pr) pk = pk && (((q.dM * q.dD + 1) & ~1) <= CH_VMAX * CH_VMAX);      // (matrices are read from the record in place: only the row counts are bounded)
    if (pk) {
        PackArgs& pa = n->pack;
        int off = 0, ns = 0;
        // (with each tensor the gradient and momentum of the same taps: a fused update reads the taps through them, TapUpd)
        for (int l = 0; l < L; ++l) { const Pair& q = n->pr[l]; pa.seg[ns++] = PackSeg{q.c, q.dM * q.dD, l, off, q.grads(n->grad).dck, q.Dc}; off += (q.dM * q.dD + 1) & ~1; }
        for (int l = L - 1; l >= 0; --l) {
            const Pair& q = n->pr[l];
            pa.seg[ns++] = PackSeg{q.f, q.dM * q.dD, l, off, q.grads(n->grad).dfk, q.Df};
            off += (q.dM * q.dD + 1) & ~1;
        }
        pa.nseg = ns; pa.L = L; pa.E = off; pa.Nk = n->pr[0].Nk;
        for (int l = 0; l < L; ++l) { pa.Nx[l] = n->pr[l].Nx; pa.Ny[l] = n->pr[l].Ny; }
        pa.NxC = n->pr[L - 1].Nx; pa.NyC = n->pr[L - 1].Ny; pa.Pc = n->pr[L - 1].P; pa.tw = n->ctx->tw;
        if ((size_t)pa.Pc * pa.E * sizeof(float2) <= (size_t)1 << 30) {
            RET_IF(net_alloc_t(n, &n->Wp, (size_t)pa.Pc * pa.E));
            pa.Wp = n->Wp;
            if (2 * (L - 1) <= 8)
                for (int l = 0; l + 1 < L; ++l) RET_IF(net_alloc_t(n, &n->pr[l].Cc, (size_t)n->pr[l].dM * n->pr[l].dD * n->pr[l + 1].P));
            for (int l = 0; l < L; ++l)
                for (int k = 0; k < 2; ++k) {
                    if (l > 0) RET_IF(net_alloc_t(n, &n->pr[l].opA[k], (size_t)OPC * n->pr[l].dD * n->pr[l].P));
                    RET_IF(net_alloc_t(n, &n->pr[l].opO[k], (size_t)OPC * n->pr[l].dD * pa.Pc));
                }
        }
    }
    return AEFFT_OK;
}

extern "C" void aefft_net_destroy(aefft_net* net)
{
    if (!net) return;
    (void)hipStreamSynchronize(net->ctx->stream);
    for (int i = 0; i < aefft_ctx::NAUX; ++i) if (net->ctx->aux[i]) (void)hipStreamSynchronize(net->ctx->aux[i]);
    for (int i = 0; i < 2; ++i) if (net->ev_end[i]) (void)hipEventDestroy(net->ev_end[i]);
    if (net->ev_r2c) (void)hipEventDestroy(net->ev_r2c);
    if (net->ev_mid) (void)hipEventDestroy(net->ev_mid);
    for (void* p : net->allocs) (void)hipFree(p);
    delete net;
}

// opts = 0: aefft_net_create; AEFFT_NET_SMOOTH_SIZES: smooth Nx, Ny too (mixed-radix transforms), every pooled grid even and >= 8
static int net_create(aefft_ctx* ctx, const aefft_net_desc* d, unsigned opts, aefft_net** out)
{
    if (!ctx || !d || !out || d->npairs <= 0 || d->batch <= 0 || d->D <= 0 || !d->maps || !d->Nk || !d->Nl || !d->scale)
        return fail(ctx, AEFFT_EINVAL, "aefft_net_create: bad descriptor");
    *out = nullptr;
    const bool smooth = (opts & AEFFT_NET_SMOOTH_SIZES) != 0;
    if (smooth) {
        if (!net_size(d->Nx) || !net_size(d->Ny))
            return fail(ctx, AEFFT_EINVAL, "aefft_net_create_ex: Nx, Ny must be powers of two in 8..2048, or even sizes in 10..2048 with no prime factor above 5");
    } else RET_IF(chk_size(ctx, d->Nx, d->Ny));
    aefft_net* n = new aefft_net();
    n->ctx = ctx; n->D = d->D; n->Nx = d->Nx; n->Ny = d->Ny; n->L = d->npairs; n->B = d->batch;
    n->Bc = std::max(n->B, (int)OPC);
    n->smooth_opform = smooth && (opts & AEFFT_NET_SMOOTH_OPFORM) && (fft_size_smooth(d->Nx) || fft_size_smooth(d->Ny));
    n->pr.resize(n->L);
    int dD = d->D, nx = d->Nx, ny = d->Ny;
    size_t maxS = 0, maxBDP = 0, maxW = 0, maxReal = 0, goff = 0, maxMid = 0, maxDen = 0, maxSmall = 0, maxHid = 0, maxDM = 0, soff = 2 * (size_t)d->npairs;
    std::vector<size_t> esoff(d->npairs);
    int rc = AEFFT_OK;
    for (int l = 0; l < n->L && rc == AEFFT_OK; ++l) {
        Pair& q = n->pr[l];
        q.dD = dD; q.dM = d->maps[l]; q.Nk = d->Nk[l]; q.Nl = d->Nl[l]; q.s = d->scale[l];
        q.Nxin = nx; q.Nyin = ny;
        if (q.dM <= 0 || q.Nk <= 0 || q.Nl <= 0 || q.s < 1 || !pow2(q.s)) { rc = fail(ctx, AEFFT_EINVAL, "aefft_net_create: bad pair parameters"); break; }
        q.Nx = nx / q.s; q.Ny = ny / q.s;
        if (smooth && (nx % q.s || ny % q.s || (q.Nx & 1) || (q.Ny & 1) || q.Nx < 8 || q.Ny < 8)) {
            const std::string msg = "aefft_net_create_ex: every pair's pooled grid must be even and >= 8 (pair " + std::to_string(l) + ": " + std::to_string(nx) +
                                    " x " + std::to_string(ny) + " pooled by " + std::to_string(q.s) + ")";
            rc = fail(ctx, AEFFT_EINVAL, msg.c_str());
            break;
        }
        if (q.Nx < 8 || q.Ny < 8 || q.Nk > q.Nx || q.Nl > q.Ny) { rc = fail(ctx, AEFFT_EINVAL, "aefft_net_create: pooled size < 8 or kernel larger than plane"); break; }
        q.P = bins(q.Nx, q.Ny);
        const size_t nk = (size_t)q.dM * q.dD * q.Nk * q.Nl;
        if (nk < (size_t)q.dM || nk < (size_t)q.dD) { rc = fail(ctx, AEFFT_EINVAL, "aefft_net_create: degenerate kernel"); break; }
        q.goff = goff; goff += 2 * nk + q.dM + q.dD;
        // c|f, Dc|Df, C|F and dc|df are each ONE allocation so that both kernels of a pair go through one launch
        if ((rc = net_alloc_t(n, &q.c, 2 * nk)) || (rc = net_alloc_t(n, &q.Dc, 2 * nk))) break;
        q.f = q.c + nk; q.Df = q.Dc + nk;
        if ((rc = net_alloc_t(n, &q.b, q.dM)) || (rc = net_alloc_t(n, &q.Db, q.dM)) || (rc = net_alloc_t(n, &q.p, q.dD)) || (rc = net_alloc_t(n, &q.Dp, q.dD))) break;
        const size_t W = (size_t)q.dM * q.dD * q.P;
        if ((rc = net_alloc_t(n, &q.C, 2 * W))) break;
        q.F = q.C + W;
        q.spectra_valid = false;
        const size_t BDP = (size_t)n->Bc * q.dD * q.P, BMP = (size_t)n->Bc * q.dM * q.P;
        if (q.s == 1 && l > 0) q.X = n->pr[l - 1].H;
        else if ((rc = net_alloc_t(n, &q.X, BDP))) break;
        if ((rc = net_alloc_t(n, &q.H, BMP)) || (rc = net_alloc_t(n, &q.O, BDP))) break;
        q.Oc = nullptr;
        if ((rc = net_alloc_t(n, &q.S, (size_t)q.dD * q.dD * q.P)) || (rc = net_alloc_t(n, &q.G, (size_t)q.dD * q.dD * q.P)) || (rc = net_alloc_t(n, &q.dc, 2 * W))) break;
        q.df = q.dc + W;
        q.part = nullptr;
        // (sized by what the grid HAS, not by what AEFFT_F_NOPRUNESMOOTH selects at this moment: the switch may change on a live net, so a grid
        // with a smooth axis owns both the row chunks' partial sums and the full route's real planes)
        if (pruned_geometry(q.Nk, q.Nl, q.Nx, q.Ny)) { if ((rc = net_alloc_t(n, &q.part, kgrad_partial_floats(2L * q.dM * q.dD, q.Nx, q.Ny, q.Nk, q.Nl)))) break; }
        if (!pruned_geometry(q.Nk, q.Nl, q.Nx, q.Ny) || !pruned_pow2(q.Nx, q.Ny)) n->pruned = false;
        maxS = std::max(maxS, (size_t)q.dD * q.dD * q.P); maxBDP = std::max(maxBDP, BDP); maxW = std::max(maxW, W);
        esoff[l] = soff; soff += 2 * (size_t)q.dD;
        maxReal = std::max(maxReal, (size_t)q.dM * q.dD * q.Nx * q.Ny);
        maxMid = std::max(maxMid, (size_t)q.dM * q.dD * q.Nx * (q.Ny / 2));
        maxMid = std::max(maxMid, (size_t)n->B * q.dM * q.Nx * (q.Ny / 2));      // (a hidden layer of the whole batch: aefft_net_infer)
        maxHid = std::max(maxHid, (size_t)OPC * q.dM * q.P);
        maxDM = std::max(maxDM, (size_t)q.dM);
        maxDen = std::max(maxDen, gradient_diff_ws_floats(q.dM, q.dD, q.Nk, q.Nl));
        maxSmall = std::max(maxSmall, 2 * nk + q.dM + q.dD + 64);
        dD = q.dM; nx = q.Nx; ny = q.Ny;
    }
    if (rc == AEFFT_OK) {
        maxMid = std::max(maxMid, (size_t)n->B * n->D * n->Nx * (n->Ny / 2));
        void* dummy;
        // size the context workspaces once so nothing reallocates inside a step
        if ((rc = ws_get(ctx, WS_MID, sizeof(float2) * maxMid, &dummy)) == AEFFT_OK &&
            (rc = ws_get(ctx, WS_MID3, sizeof(float2) * (size_t)n->B * n->D * n->Nx * (n->Ny / 2), &dummy)) == AEFFT_OK &&
            // (smooth sizes: the input transform's side-stream workspace of aefft_net_set_input_ready as well)
            (!smooth || (rc = ws_get(ctx, WS_MID2, sizeof(float2) * (size_t)n->B * n->D * n->Nx * (n->Ny / 2), &dummy)) == AEFFT_OK) &&
            (rc = ws_get(ctx, WS_DEN, sizeof(float) * maxDen, &dummy)) == AEFFT_OK &&
            (rc = ws_get(ctx, WS_SMALL, sizeof(float) * maxSmall, &dummy)) == AEFFT_OK &&
            (rc = net_alloc_t(n, &n->real, n->pruned ? 64 : maxReal)) == AEFFT_OK &&
            (rc = net_alloc_t(n, &n->mse_slots, n->L * MSE_PAIR_FLOATS)) == AEFFT_OK &&
            (rc = net_alloc_t(n, &n->score_part, (size_t)n->B * score_pairs_per_frame(n))) == AEFFT_OK &&
            (rc = net_alloc_t(n, &n->map_part, score_map_strips(n))) == AEFFT_OK &&
            (rc = net_alloc_t(n, &n->grad, goff + 2 * (size_t)n->L)) == AEFFT_OK && (rc = net_alloc_t(n, &n->scratch, soff)) == AEFFT_OK) {
            n->scratch_n = soff; n->mse_pre = n->scratch; n->mse_post = n->scratch + n->L;
            for (int l = 0; l < n->L; ++l) n->pr[l].es = n->scratch + esoff[l];
            n->grad_n = goff;
            n->Xf = n->pr[0].X;
            if (n->D <= OPC - 1) {
                const Pair& q0 = n->pr[0];
                if (rc == AEFFT_OK) rc = net_alloc_t(n, &n->A0hat, (size_t)OPC * q0.dD * q0.P);
                if (rc == AEFFT_OK) rc = net_alloc_t(n, &n->Mhat, (size_t)OPC * OPC * q0.P);
                if (rc == AEFFT_OK && launch_basis_fill(n->A0hat, q0.dD, q0.P, ctx->stream) != hipSuccess) rc = fail(ctx, AEFFT_EHIP, "basis_fill");
                if (rc == AEFFT_OK) rc = build_chain_items(n);
                // frozen-weight inference sizes what it needs here: the hidden-layer operator, and the reconstruction's per-frame spectra where
                // launch_recon writes them out (AEFFT_X_RECON_EXPAND_BYTES)
                if (rc == AEFFT_OK) rc = net_alloc_t(n, &n->Hhat, maxHid);
                // ... and decode (aefft_net_decode) its operator T^_l on the coarsest grid's bins, for the widest pair, with the rows in flight
                // while it is formed -- on nets whose shapes can take an operator form at all (op_shapes).  A row
                // is a stage's OUTPUT with its affine element, at most max dM + 1 long (stage 0 reads row d of F_0 directly: D is no row
                // length); the bins in flight are cut down so that the workspace stays within DEC_WS_BYTES.
                if (op_shapes(n)) {
                    const long PcD = n->pr[n->L - 1].P;
                    n->dec_w = (int)maxDM + 1;
                    const long fit = (long)(DEC_WS_BYTES / (2.0 * n->D * n->dec_w * sizeof(float2))) / 64 * 64;
                    n->dec_nt = (int)std::max<long>(64, std::min<long>({(PcD + 63) / 64 * 64, (long)DEC_MAX_THREADS, fit}));
                    if (rc == AEFFT_OK) rc = net_alloc_t(n, &n->That, (size_t)n->D * n->dec_w * PcD);
                    if (rc == AEFFT_OK) rc = net_alloc_t(n, &n->dec_ws, 2 * (size_t)n->D * n->dec_w * n->dec_nt);
                }
                // (launch_recon's own test: O^_0 lives on the coarsest pair's grid -- of a one-pair net, pair 0's)
                const Pair& qc0 = n->pr[n->L - 1];
                if (rc == AEFFT_OK && (double)n->B * q0.dD * qc0.P * 8.0 > AEFFT_X_RECON_EXPAND_BYTES) {
                    n->recon_exp_n = (size_t)n->B * q0.dD * qc0.P;
                    rc = net_alloc_t(n, &n->recon_exp, n->recon_exp_n);
                }
            }
            // compact decoder outputs (training step): the coarsest pair's grid
            const Pair& qc = n->pr[n->L - 1];
            n->NxC = qc.Nx; n->NyC = qc.Ny; n->Pc = qc.P;
            for (int l = 0; l < n->L && rc == AEFFT_OK; ++l) {
                Pair& q = n->pr[l];
                if (rc == AEFFT_OK) rc = net_alloc_t(n, &q.beta, (size_t)q.dD);
                if (q.P == n->Pc) q.Oc = q.O;            // already on the coarsest grid: nothing to compact
                else rc = net_alloc_t(n, &q.Oc, (size_t)n->Bc * q.dD * n->Pc);
                if (rc == AEFFT_OK && qpath_support(q.Nk, q.Nl)) {
                    const size_t tt = (size_t)(2 * q.Nk - 1) * (2 * q.Nk - 1);
                    q.Qn = kgrad_group_chunks((long)q.dD * q.dD, q.Nx, q.Ny);       // room for the row chunks' partial sums
                    rc = net_alloc_t(n, &q.Q, (size_t)q.dD * q.dD * tt * q.Qn);
                }
            }
        }
    }
    if (rc != AEFFT_OK) { aefft_net_destroy(n); return rc; }
    hipError_t e = hipMemsetAsync(n->mse_slots, 0, sizeof(float) * n->L * MSE_PAIR_FLOATS, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(n->grad + n->grad_n, 0, sizeof(float) * 2 * n->L, ctx->stream);      // (the MSE tail of the packed buffer: zero before the first step)
    if (e != hipSuccess) { aefft_net_destroy(n); return fail(ctx, AEFFT_EHIP, "memset(mse slots)", e); }
    for (auto& q : n->pr) {
        const size_t nk = (size_t)q.dM * q.dD * q.Nk * q.Nl;
        e = hipMemsetAsync(q.c, 0, nk * 4, ctx->stream); if (e) break;
        e = hipMemsetAsync(q.f, 0, nk * 4, ctx->stream); if (e) break;
        e = hipMemsetAsync(q.b, 0, q.dM * 4, ctx->stream); if (e) break;
        e = hipMemsetAsync(q.p, 0, q.dD * 4, ctx->stream); if (e) break;
    }
    if (e != hipSuccess) { aefft_net_destroy(n); return fail(ctx, AEFFT_EHIP, "memset weights", e); }
    if (smooth && (fft_size_smooth(n->Nx) || fft_size_smooth(n->Ny))) {
        // the mixed-radix twiddle tables of every size the net transforms: built here, not inside a step
        std::vector<int> sizes{n->Nx, n->Ny};
        for (const Pair& q : n->pr) { sizes.push_back(q.Nx); sizes.push_back(q.Ny); }
        for (int m : sizes) if (fft_size_mixed(m) && (e = fft_mixed_prepare(m)) != hipSuccess) break;
        if (e != hipSuccess) { aefft_net_destroy(n); return fail(ctx, AEFFT_EHIP, "mixed-radix twiddle tables", e); }
        // ... and the phase tables of the pruned kernel transforms on those grids
        for (const Pair& q : n->pr) if (pruned_geometry(q.Nk, q.Nl, q.Nx, q.Ny) && (e = pruned_prepare(q.Nx, q.Ny)) != hipSuccess) break;
        if (e != hipSuccess) { aefft_net_destroy(n); return fail(ctx, AEFFT_EHIP, "pruned transforms' phase tables", e); }
    }
    if (ensure_aux(ctx) != AEFFT_OK) { aefft_net_destroy(n); return AEFFT_EHIP; }
    *out = n;
    return aefft_net_reset_momentum(n);
}

extern "C" int aefft_net_create(aefft_ctx* ctx, const aefft_net_desc* d, aefft_net** out) { return net_create(ctx, d, 0, out); }
extern "C" int aefft_net_create_ex(aefft_ctx* ctx, const aefft_net_desc* d, unsigned opts, aefft_net** out)
{
    if (opts & ~(unsigned)(AEFFT_NET_SMOOTH_SIZES | AEFFT_NET_SPATIAL | AEFFT_NET_SMOOTH_OPFORM)) return fail(ctx, AEFFT_EINVAL, "aefft_net_create_ex: unknown option bits");
    if (opts & AEFFT_NET_SPATIAL) {       // (AEFFT_NET_SMOOTH_SIZES and AEFFT_NET_SMOOTH_OPFORM have no effect: the spatial mode takes any frame size)
        if (!ctx || !d || !out || d->npairs <= 0 || d->batch <= 0 || d->D <= 0 || !d->maps || !d->Nk || !d->Nl || !d->scale)
            return fail(ctx, AEFFT_EINVAL, "aefft_net_create_ex: bad descriptor");
        *out = nullptr;
        return sp_create(ctx, d, out);
    }
    return net_create(ctx, d, opts, out);
}

extern "C" int aefft_net_npairs(aefft_net* n) { return n ? n->L : -1; }
extern "C" int aefft_net_pair_shape(aefft_net* n, int l, int* dD, int* dM, int* Nk, int* Nl)
{
    if (!n || l < 0 || l >= n->L) return fail(n ? n->ctx : nullptr, AEFFT_EINVAL, "aefft_net_pair_shape: bad pair index");
    const Pair& q = n->pr[l];
    if (dD) *dD = q.dD;
    if (dM) *dM = q.dM;
    if (Nk) *Nk = q.Nk;
    if (Nl) *Nl = q.Nl;
    return AEFFT_OK;
}

extern "C" int aefft_net_reset_momentum(aefft_net* n)
{
    if (!n) return AEFFT_EINVAL;
    n->upd_after_fwd = false;          // (w + D no longer is the previous weight)
    aefft_ctx* ctx = n->ctx;
    for (auto& q : n->pr) {
        const size_t nk = (size_t)q.dM * q.dD * q.Nk * q.Nl;
        HIPCHK(ctx, hipMemsetAsync(q.Dc, 0, nk * 4, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(q.Df, 0, nk * 4, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(q.Db, 0, q.dM * 4, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(q.Dp, 0, q.dD * 4, ctx->stream));
    }
    return AEFFT_OK;
}

extern "C" int aefft_net_set_pair(aefft_net* n, int l, const float* c_h, const float* b_h, const float* f_h, const float* p_h)
{
    if (!n || l < 0 || l >= n->L || !c_h || !b_h || !f_h || !p_h) return fail(n ? n->ctx : nullptr, AEFFT_EINVAL, "aefft_net_set_pair: bad argument");
    n->upd_after_fwd = false;
    aefft_ctx* ctx = n->ctx;
    Pair& q = n->pr[l];
    const size_t nk = (size_t)q.dM * q.dD * q.Nk * q.Nl;
    HIPCHK(ctx, hipMemcpyAsync(q.c, c_h, nk * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(q.f, f_h, nk * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(q.b, b_h, q.dM * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(q.p, p_h, q.dD * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // host buffers may be pageable / reused by the caller
    q.spectra_valid = false; weights_changed(n, &q);
    return AEFFT_OK;
}

extern "C" int aefft_net_get_pair(aefft_net* n, int l, float* c_h, float* b_h, float* f_h, float* p_h)
{
    if (!n || l < 0 || l >= n->L) return fail(n ? n->ctx : nullptr, AEFFT_EINVAL, "aefft_net_get_pair: bad argument");
    aefft_ctx* ctx = n->ctx;
    Pair& q = n->pr[l];
    const size_t nk = (size_t)q.dM * q.dD * q.Nk * q.Nl;
    if (c_h) HIPCHK(ctx, hipMemcpyAsync(c_h, q.c, nk * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (f_h) HIPCHK(ctx, hipMemcpyAsync(f_h, q.f, nk * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (b_h) HIPCHK(ctx, hipMemcpyAsync(b_h, q.b, q.dM * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (p_h) HIPCHK(ctx, hipMemcpyAsync(p_h, q.p, q.dD * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return AEFFT_OK;
}

// kernels -> spectra for both tensors of a pair (StoreLoad_cfreq first pass, fft_backproplib.cu:1150-1152; :1274-1282)
int aefft::pair_spectra(aefft_net* n, Pair& q)
{
    const long planes = (long)q.dM * q.dD;
    if (pruned_supported(q.Nk, q.Nl, q.Nx, q.Ny)) return do_pad_r2c(n->ctx, q.c, q.C, nullptr, 2 * planes, q.Nx, q.Ny, q.Nk, q.Nl);
    RET_IF(do_pad_r2c(n->ctx, q.c, q.C, n->real, planes, q.Nx, q.Ny, q.Nk, q.Nl));
    return do_pad_r2c(n->ctx, q.f, q.F, n->real, planes, q.Nx, q.Ny, q.Nk, q.Nl);
}

int aefft::ensure_spectra(aefft_net* n, Pair& q)
{
    if (q.spectra_valid) return AEFFT_OK;
    RET_IF(pair_spectra(n, q));
    q.spectra_valid = true;
    return AEFFT_OK;
}

extern "C" int aefft_net_pair_spectra(aefft_net* n, int l, float** C_d, float** F_d)
{
    if (!n || l < 0 || l >= n->L) return fail(n ? n->ctx : nullptr, AEFFT_EINVAL, "aefft_net_pair_spectra: bad argument");
    if (n->spatial) return sp_refuse(n, "aefft_net_pair_spectra");
    RET_IF(ensure_spectra(n, n->pr[l]));
    if (C_d) *C_d = reinterpret_cast<float*>(n->pr[l].C);
    if (F_d) *F_d = reinterpret_cast<float*>(n->pr[l].F);
    return AEFFT_OK;
}

extern "C" int aefft_net_store_spectra(aefft_net* n, int l, float* C_h, float* F_h)
{
    if (!n || l < 0 || l >= n->L) return fail(n ? n->ctx : nullptr, AEFFT_EINVAL, "aefft_net_store_spectra: bad argument");
    if (n->spatial) return sp_refuse(n, "aefft_net_store_spectra");
    aefft_ctx* ctx = n->ctx;
    Pair& q = n->pr[l];
    RET_IF(ensure_spectra(n, q));
    const size_t W = (size_t)q.dM * q.dD * q.P * sizeof(float2);
    if (C_h) HIPCHK(ctx, hipMemcpyAsync(C_h, q.C, W, hipMemcpyDeviceToHost, ctx->stream));
    if (F_h) HIPCHK(ctx, hipMemcpyAsync(F_h, q.F, W, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return AEFFT_OK;
}

// load_cfreq semantics (fft_backproplib.cu:1131-1141): the cached SPECTRA are the source of truth;
// the coordinate-space kernels are re-derived from them (export_cfreq, :1166) to stay consistent.
extern "C" int aefft_net_load_spectra(aefft_net* n, int l, const float* C_h, const float* b_h, const float* F_h, const float* p_h)
{
    if (!n || l < 0 || l >= n->L || !C_h || !b_h || !F_h || !p_h) return fail(n ? n->ctx : nullptr, AEFFT_EINVAL, "aefft_net_load_spectra: bad argument");
    if (n->spatial) return sp_refuse(n, "aefft_net_load_spectra");
    n->upd_after_fwd = false;
    aefft_ctx* ctx = n->ctx;
    Pair& q = n->pr[l];
    const size_t W = (size_t)q.dM * q.dD * q.P * sizeof(float2);
    HIPCHK(ctx, hipMemcpyAsync(q.C, C_h, W, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(q.F, F_h, W, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(q.b, b_h, q.dM * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(q.p, p_h, q.dD * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    q.spectra_valid = true; weights_changed(n, &q);
    RET_IF(aefft_kernel_export(ctx, reinterpret_cast<const float*>(q.C), q.c, q.dM, q.dD, q.Nk, q.Nl, q.Nx, q.Ny));
    RET_IF(aefft_kernel_export(ctx, reinterpret_cast<const float*>(q.F), q.f, q.dD, q.dM, q.Nk, q.Nl, q.Nx, q.Ny));
    return AEFFT_OK;
}

// layer exports ------------------------------------------------------------------------------
extern "C" int aefft_net_get_layer(aefft_net* n, int layer, float* out_d, int* ch, int* nx, int* ny)
{
    if (!n || layer < 0 || layer > 4 * n->L) return fail(n ? n->ctx : nullptr, AEFFT_EINVAL, "aefft_net_get_layer: bad layer index");
    if (n->spatial) return sp_get_layer(n, layer, out_d, ch, nx, ny);
    aefft_ctx* ctx = n->ctx;
    RET_IF(join_recon(ctx));
    if (out_d && n->have_forward) RET_IF(ensure_frames(n));
    const int L = n->L, B = n->B;
    int c, x, y, xi, yi;            // channels, output size, stored spectrum size
    const float2* S = nullptr;
    if (layer == 0) { c = n->D; x = xi = n->Nx; y = yi = n->Ny; }
    else if (layer <= 2 * L) {
        const Pair& q = n->pr[(layer - 1) / 2];
        x = xi = q.Nx; y = yi = q.Ny;
        if (layer & 1) { c = q.dD; S = q.X; }
        else {
            c = q.dM; S = q.H;
            if (out_d && q.H_stale) {          // hidden layer skipped by the training step's forward: form it now (fft_backproplib.cu:1347)
                Pair& qm = n->pr[(layer - 1) / 2];
                if (n->upd_after_fwd && n->op_chain) {
                    // chain form after aefft_net_step_apply: X_l is the step's own (expanded from its operators), so the hidden layer must
                    // come from the step's encoder too, not from the updated one.  The update was w <- w - D with D left in the momentum
                    // buffer: c_old = c + Dc, b_old = b + Db (to one rounding of the subtraction), its spectrum into the pair's planar C
                    // buffer -- which this form keeps stale anyway (spectra_valid stays false: rebuilt from the current weights on demand).
                    const size_t nk = (size_t)qm.dM * qm.dD * qm.Nk * qm.Nl;
                    void *tmp, *real = nullptr;
                    RET_IF(ws_get(ctx, WS_TMP, sizeof(float) * (nk + qm.dM), &tmp));
                    float* c_old = (float*)tmp; float* b_old = c_old + nk;
                    hipError_t e = launch_vec_add(c_old, qm.c, qm.Dc, (long)nk, ctx->cur);
                    if (e == hipSuccess) e = launch_vec_add(b_old, qm.b, qm.Db, qm.dM, ctx->cur);
                    if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "get_layer: previous encoder", e);
                    if (!pruned_supported(qm.Nk, qm.Nl, qm.Nx, qm.Ny)) real = n->real;
                    qm.spectra_valid = false;
                    RET_IF(do_pad_r2c(ctx, c_old, qm.C, (float*)real, (long)qm.dM * qm.dD, qm.Nx, qm.Ny, qm.Nk, qm.Nl));
                    RET_IF(do_conv(n->ctx, qm.X, qm.C, b_old, qm.H, n->B, qm.dM, qm.dD, qm.Nx, qm.Ny));
                } else {
                    RET_IF(ensure_spectra(n, qm));
                    RET_IF(do_conv(n->ctx, qm.X, qm.C, qm.b, qm.H, n->B, qm.dM, qm.dD, qm.Nx, qm.Ny));
                }
                qm.H_stale = false;
            }
        }
    } else {
        const int nn = (layer - 1) / 2;           // decoder conv index L..2L-1
        const Pair& q = n->pr[2 * L - 1 - nn];
        const OutView v = out_view(n, q);                            // (training-step forward: the layer is stored on its support only)
        c = q.dD; S = v.O; xi = v.nx; yi = v.ny;
        if (layer & 1) { x = q.Nx; y = q.Ny; } else { x = q.Nxin; y = q.Nyin; }   // odd: conv output; even: up-sampled
    }
    if (ch) *ch = c;
    if (nx) *nx = x;
    if (ny) *ny = y;
    if (!out_d) return AEFFT_OK;
    if (!n->have_forward) return fail(ctx, AEFFT_ESTATE, "aefft_net_get_layer: no forward pass yet");
    if (layer == 0) {
        if (n->last_frames_u8) {
            hipError_t e = launch_u8_to_f32(out_d, reinterpret_cast<const unsigned char*>(n->last_frames), (long)B * c * x * y, ctx->stream);
            if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "get_layer: 8-bit frames", e);
            return AEFFT_OK;
        }
        HIPCHK(ctx, hipMemcpyAsync(out_d, n->last_frames, sizeof(float) * B * c * x * y, hipMemcpyDeviceToDevice, ctx->stream));
        return AEFFT_OK;
    }
    RET_IF(do_c2r(ctx, S, out_d, (long)B * c, xi, yi, x, y, 1.0f / ((float)x * (float)y)));
    return mark_step_point(n);
}

extern "C" int aefft_magnitude(aefft_ctx* ctx, const float* X_d, float* mag_d, long planes, int ch, int Nx, int Ny, int shift)
{
    if (!ctx || !X_d || !mag_d || planes <= 0 || ch <= 0 || Nx <= 0 || Ny <= 1) return fail(ctx, AEFFT_EINVAL, "aefft_magnitude: bad argument");
    Bracket br(ctx, KID_RESIZE, (double)planes * ((double)Nx * (Ny / 2 + 1) * 8.0 + (double)Nx * Ny * 4.0));
    hipError_t e = launch_magnitude(CF2(X_d), mag_d, planes, ch, Nx, Ny, shift, ctx->stream);
    if (e != hipSuccess) return fail(ctx, AEFFT_EHIP, "magnitude", e);
    return AEFFT_OK;
}

extern "C" int aefft_net_layers_layout(aefft_net* n, size_t* offsets_h)
{
    if (!n || !offsets_h) return fail(n ? n->ctx : nullptr, AEFFT_EINVAL, "aefft_net_layers_layout: bad argument");
    size_t off = 0;
    for (int l = 0; l <= 4 * n->L; ++l) {
        int c, x, y;
        RET_IF(aefft_net_get_layer(n, l, nullptr, &c, &x, &y));
        offsets_h[l] = off;
        off += (size_t)n->B * c * x * y;
    }
    offsets_h[4 * n->L + 1] = off;
    return AEFFT_OK;
}

// All layers of the last forward in coordinate space (fft_l = 1, fft_backproplib.cu:1347,1357,1361).  A decoder conv output and
// the up-sampled layer after it are inverse transforms of the SAME spectrum onto two grids; an encoder's pooled input and the
// previous hidden layer likewise -- each stored spectrum is read where it lies, the crop / zero-pad is fused into the transform.
extern "C" int aefft_net_get_layers(aefft_net* n, float* out_d)
{
    if (!n || !out_d) return fail(n ? n->ctx : nullptr, AEFFT_EINVAL, "aefft_net_get_layers: bad argument");
    if (!n->have_forward) return fail(n->ctx, AEFFT_ESTATE, "aefft_net_get_layers: no forward pass yet");
    std::vector<size_t> off(4 * n->L + 2);
    RET_IF(aefft_net_layers_layout(n, off.data()));
    for (int l = 0; l <= 4 * n->L; ++l) RET_IF(aefft_net_get_layer(n, l, out_d + off[l], nullptr, nullptr, nullptr));
    return AEFFT_OK;
}
