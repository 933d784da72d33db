// The resident network (aefft_net) and its pairs, shared by net.hip (lifetime, weights and spectra, chain set-up, layer exports),
// net_forward.hip (forward, inference, decode), net_score.hip (read-outs of the reconstruction) and net_step.hip (bursts, training step): the rules more than one of them applies, each
// stated once, and the helpers one unit defines for another.  Nothing here is exported.
#pragma once
#include "host.h"

// one pair's segment of the packed gradient buffer: dck [dM][dD][Nk][Nl] | dfk [dD][dM][Nk][Nl] | db [dM] | dp [dD]
struct GradSeg { float *dck, *dfk, *db, *dp; };

struct Pair {
    int dD, dM, Nk, Nl, s;
    int Nxin, Nyin;          // resolution before this pair's pooling
    int Nx, Ny;              // working resolution (after pooling)
    long P;
    float *c, *f, *b, *p;
    float *Dc, *Df, *Db, *Dp;
    float2 *C, *F;
    bool spectra_valid;
    bool H_stale = false;    // the last (lazy) forward produced only the pooled part of H: recompute before reading H
    float2* G = nullptr;     // [dD][dD][P] collapsed pair operator F.C/(dM dD) (post-update MSE; innermost pair's forward)
    bool G_valid = false;    // G and beta (its DC bias) belong to the CURRENT weights (left by aefft_net_step_apply; dropped by weights_changed)
    float* beta = nullptr;   // [dD]
    float* Q = nullptr;      // [dD][dD][Qn][T*T], T = 2Nk-1: pruned inverse transform of S (weight_kernels.hip), Qn row-chunk partial sums
    int Qn = 1;
    float2* Oc = nullptr;    // [B][dD][Pc] decoder output on the support of the up-sampled spectra (the coarsest pair's grid); last pair: == O
    float2* opA[2] = {nullptr, nullptr};   // [OPC][dD][P]  operator chain: the pair's input on the basis frames, two sets (the step in progress / the next step's)
    float2* opO[2] = {nullptr, nullptr};   // [OPC][dD][Pc] ... its decoder output on the coarsest grid's support
    float2* Cc = nullptr;    // [dM][dD][P of the next pair] C sampled where the next pair's grid lands (operator chain: its planar tiles read nothing else of C)
    bool O_stale = false;    // the last (lazy) forward produced Oc only: expand before reading O
    float2 *X, *H, *O;       // [B][dD][P], [B][dM][P], [B][dD][P] (X aliases the previous pair's H when s == 1)
    size_t goff;             // offset (floats) of this pair's segment in the packed gradient buffer
    float* es;               // [2*dD] DC bins of the error summed over the batch (inside the net scratch)
    float2 *S, *dc, *df;     // per-pair gradient workspaces (pairs run concurrently on side streams); df == dc + W
    float* part;             // kgrad partial sums
    float *Lin = nullptr, *Lhid = nullptr, *Lout = nullptr;   // spatial net: layers 2l+1, 2l+2 and 4L-1-2l, [B][dD|dM|dD][Nx][Ny]
    size_t nk() const { return (size_t)dM * dD * Nk * Nl; }     // taps of each of the two kernels
    GradSeg grads(float* buf) const { float* g = buf + goff; return GradSeg{g, g + nk(), g + 2 * nk(), g + 2 * nk() + dM}; }   // its segment of buf (aefft_net::grad)
};

struct aefft_net {
    aefft_ctx* ctx;
    int D, Nx, Ny, L, B;
    std::vector<Pair> pr;
    std::vector<void*> allocs;
    // operator form of the training step (opform_kernels.hip)
    int Bc = 0;                // columns every activation buffer is allocated for: max(B, OPC)
    float2* Xf = nullptr;      // [B][D][P0] input spectra of the frames (pair 0's X in the per-frame form)
    float2* A0hat = nullptr;   // [OPC][D][P0] basis frames (pair 0's X in the operator form); null: D > OPC-1
    float2* Mhat = nullptr;    // [OPC][OPC][P0] second moments of the batch
    bool smooth_opform = false; // created with AEFFT_NET_SMOOTH_OPFORM on a grid with a smooth axis: the operator form also where a pair's grid is not a power of two
    bool op_state = false;     // the activation buffers hold OPERATORS (basis-frame responses) of the last step_grad, not frames
    // chain mode (the step's forward is chain_kernel): the operators live in their OWN buffers (Pair::opA / opO), two sets, because the
    // tail launch of a step already runs the NEXT step's chain on the updated weights (it depends on the weights only) while the
    // post-update MSE still reads this step's operators
    bool op_chain = false;     // the last step_grad ran in chain mode: operators in set op_fwd, activation buffers NOT refreshed (act_stale)
    bool act_stale = false;    // the activation buffers do not hold the last forward's frames (ensure_frames expands them from the operators)
    bool upd_after_fwd = false; // aefft_net_step_apply has changed the weights since the step's forward: a layer export forms a skipped hidden layer with
                               // the encoder of THAT forward, recovered as w + D (the momentum buffer holds the step that was applied)
    bool chain_valid = false;  // set op_set holds the operators of the CURRENT weights (weights_changed)
    int op_set = 0, op_fwd = 0;
    // frozen-weight inference (aefft_net_infer): what it caches beside the operator sets
    bool ops_valid = false;    // operator form without the chain launch: the activation buffers hold the operators of the CURRENT weights (weights_changed)
    float2* Hhat = nullptr;    // [OPC][dM][P] of the largest pair: one pair's hidden layer as an operator, H^_l = C_l A_l / dM + bias
    int hid_pair = -1;         // ... of this pair
    bool hid_valid = false;    // ... and of the CURRENT weights (weights_changed)
    // decode (aefft_net_decode): the remainder of the network from one pair's hidden layer as an operator on the coarsest grid's bins
    float2* That = nullptr;    // [D][dM_l + 1][Pc], sized for the widest pair: T^_l (decode_kernels.hip); null: D > OPC-1
    float2* dec_ws = nullptr;  // [2][D][dec_w][dec_nt] rows in flight while decode_op_kernel forms it
    int dec_nt = 0, dec_w = 0; // threads (bins in flight) and column stride (max dM + 1: the longest row with its affine element) it was allocated for
    int dec_pair = -1;         // ... of this pair
    bool dec_valid = false;    // ... and of the CURRENT weights (weights_changed)
    // per-frame reconstruction error (aefft_net_score)
    float* score_part = nullptr; // [B][(D*Nx + 1)/2] one partial sum of squared differences per ROW PAIR of a frame (the row passes' scoring epilogue, score_diff_kernel)
    float* map_part = nullptr;   // [B*D*Nx/2][Ny/tile] one float per STRIP (two rows x tile columns of a channel; aefft_net_score_map), sized for tile 8
    float* ssim_part = nullptr;  // [5][B*D*Nx/2][Ny/tile] five floats per strip (aefft_net_ssim_map), sized for tile 8: allocated by the net's first SSIM call
    float2* Wp = nullptr;      // [Pc][packE] bin-major copy of the kernel spectra the coarsest-grid chain items read (kspec_packed_kernel)
    aefft::PackArgs pack{};    // its description (static per net)
    bool packed_valid = false; // Wp belongs to the CURRENT weights (weights_changed)
    float* grad = nullptr; size_t grad_n = 0;
    float* scratch = nullptr;  // [mse_pre[L] | mse_post[L] | es of pair 0 (2*dD) | es of pair 1 | ...], zeroed once per step
    size_t scratch_n = 0;
    float* mse_pre = nullptr;  // = scratch
    float* mse_post = nullptr; // = scratch + L
    float* gtaps = nullptr;      // G' from the stored taps on HBM-sized grids: the (2Nk-1)^2 taps of every plane of every pair (gprime_from_taps)
    // training toward a target (aefft_net_step_grad_target, target_kernels.hip): allocated by the net's first target call
    float2* Tf = nullptr;        // [B][D][P0] the targets' spectra on pair 0's grid
    float2* tgtK = nullptr;      // [D][D+1][P0] K = sum_b N_b [X_0,b; 1]^H, N_b = X_0,b - T_b (the post-update MSE's cross term)
    float* tgtN2 = nullptr;      // [P0] sum_b |N_b|^2
    bool target_step = false;    // the pending step (have_grad) has a target: from aefft_net_step_grad_target to its aefft_net_step_apply
    float *gd_out = nullptr, *gd_part = nullptr;   // multiobjective mode: [cd | fd | bd | pd] per pair, and the chunk partial sums (gradient_diff_ws_floats)
    bool mse_pending = false;   // the slots hold the unsummed post-update MSE of the last aefft_net_step_apply (mse_d == NULL): summed by the next step's wgrad launch or mse_flush
    float mse_pending_scale = 1.f;
    float* mse_slots = nullptr; // [L][MSE_PAIR_FLOATS] accumulators of the fused re-forward MSE (zero between uses)
    float* mse_dev = nullptr;  // scratch for bursts
    size_t mse_cap = 0;
    const float* last_frames = nullptr;
    bool last_frames_u8 = false;     // ... and they were 8-bit pixels
    bool have_forward = false, have_grad = false;
    int tail_route = 0;        // AEFFT_TAIL_*: the step code of the last tail launch (launch_opmse_group; aefft_net_tail_route)
    int NxC = 0, NyC = 0; long Pc = 0;   // grid of the coarsest pair = support of every decoder output
    bool compact = true;                 // the training step may keep decoder outputs on that support only
    // input prefetch (aefft_net_set_input_ready): second buffer for pair 0's input spectra, end-of-step events, step counter
    bool input_ready = false;
    float2* X0alt = nullptr;
    hipEvent_t ev_end[2] = {nullptr, nullptr}, ev_r2c = nullptr, ev_mid = nullptr;
    bool ev_mid_valid = false;
    bool ev_end_valid[2] = {false, false};
    unsigned long step_no = 0;
    size_t recon_exp_n = 0;       // complex elements recon_exp holds
    float2* recon_exp = nullptr;  // [B][D][PO] per-frame output spectra of the reconstruction when they are written out (large supports, launch_recon)
    unsigned ox_done = 0;         // bit l: the forward already launched pair l's support term S += sum_b Oc X^H
    bool xx_done = false;         // the forward already launched S = -sum_b X X^H (grouped with the innermost decoder conv)
    bool recon_pending = false;   // the reconstruction's inverse FFT is still running on aux[0]
    float* recon_deferred = nullptr;   // pipelined mode: the reconstruction is launched at the end of the gradient half
    bool burst = false;        // inside aefft_net_train_pair (its MSE slots are zeroed up front, not by the update kernel)
    // shared scratch sized for the largest pair
    bool fuse_crop = true;     // encoder convs also write the next pair's cropped input (no resize launches)
    bool pruned = true;        // every pair's kernel support has a pruned transform -> no shared FFT workspace in the backward
    float* real;
    // spatial net (AEFFT_NET_SPATIAL, spatial_net.hip): coordinate-space layers per pair, no spectra
    bool spatial = false;
    float alpha = 0.9f;        // inertia weight of backprop_gpu (autoencoder.cpp:89), aefft_net_set_inertia
    float* sp_ws = nullptr;    // back-convolved error of the largest pair (launch_spatial_grad's fallback routes)
    float* sp_part = nullptr;  // tiled weight-gradient partial sums (spatial_partial_floats of the largest pair)
    float* sp_rq = nullptr;    // error-input region sums (spatial_rq_floats)
    float* sp_up = nullptr;    // an up-sampled decoder input, for kernel shapes the tiled convolutions do not serve
    float* sp_sqd = nullptr;   // MSE partial sums (SQD_MAX * SQD_BLOCKS)
};

namespace aefft {

// pair l's accumulators of the fused re-forward MSE (aefft_net::mse_slots)
constexpr size_t MSE_PAIR_FLOATS = (size_t)MSE_SLOTS * MSE_SLOT_STRIDE;
inline float* mse_slot(const aefft_net* n, int l) { return n->mse_slots + (size_t)l * MSE_PAIR_FLOATS; }

// ---- net.hip ---------------------------------------------------------------------------
int net_alloc(aefft_net* n, void** p, size_t bytes);
template <typename T> int net_alloc_t(aefft_net* n, T** p, size_t count) { return net_alloc(n, reinterpret_cast<void**>(p), count * sizeof(T)); }
int pair_spectra(aefft_net* n, Pair& q);
int ensure_spectra(aefft_net* n, Pair& q);

// ---- spatial_net.hip (a net created with AEFFT_NET_SPATIAL: the entry points hand over to these) ------------------------
int sp_create(aefft_ctx* ctx, const aefft_net_desc* d, aefft_net** out);
int sp_forward(aefft_net* n, const float* frames_d, float* recon_d);
int sp_decode(aefft_net* n, int l, const float* code_d, float* recon_d);
int sp_step_grad(aefft_net* n, const float* frames_d, float* recon_d);
int sp_step_apply(aefft_net* n, float del0, int maxdiff, int sym, float grad_scale, float* mse_d);
int sp_get_layer(aefft_net* n, int layer, float* out_d, int* ch, int* nx, int* ny);
int sp_last_mse(aefft_net* n, float* mse_d);
int sp_refuse(aefft_net* n, const char* entry);     // AEFFT_EINVAL: `entry` does not apply to a spatial net

// ---- net_step.hip ----------------------------------------------------------------------
int mark_step_point(aefft_net* n);

// ---- net_forward.hip -------------------------------------------------------------------
int ensure_frames(aefft_net* n);

// What follows was local to one file while that held the forward and the step: it stays out of the library's symbol table (an inline function
// the compiler does not inline would be a weak symbol of it)
#pragma GCC visibility push(hidden)
// ---- rules that more than one unit applies, each stated once ---------------------------
// The weights of pair `only` (nullptr: of every pair) change: A NEW CACHE OF THE WEIGHTS IS CLEARED HERE, and nowhere else.  Not in the list:
// Pair::spectra_valid (the caller knows whether it wrote taps or spectra) and upd_after_fwd (which is about the last forward).
inline void weights_changed(aefft_net* n, Pair* only)
{
    for (Pair& q : n->pr) if (!only || only == &q) q.G_valid = false;
    n->packed_valid = n->chain_valid = n->ops_valid = n->hid_valid = n->dec_valid = false;
}
// kernel supports of the Q-path gradient and the operator form: square 3x3 or 5x5; every pair has pair 0's support
inline bool qpath_support(int Nk, int Nl) { return Nk == Nl && (Nk == 3 || Nk == 5); }
inline bool same_supports(const aefft_net* n) { for (const Pair& q : n->pr) if (q.Nk != n->pr[0].Nk || q.Nl != n->pr[0].Nl) return false; return true; }
// shapes that can take an operator form at all (the part of op_eligible no switch moves; net_create sizes the decode buffers by it): the
// channel counts the operator-form kernels' LDS tiles take (msgrad_kernel: 2*OPC*dD*8 complex; opmse: OPC*(dD+dM)*4), 8 pairs, one Q-path support
inline bool op_shapes(const aefft_net* n)
{
    for (const Pair& q : n->pr) if (q.dD > 256 || q.dM > 512 || q.dD + q.dM > 1024) return false;
    return n->L <= 8 && qpath_support(n->pr[0].Nk, n->pr[0].Nl) && same_supports(n);
}
// an operator-form reconstruction above this size writes its per-frame spectra out (launch_recon; net_create sizes their buffer by it)
#ifndef AEFFT_X_RECON_EXPAND_BYTES
#define AEFFT_X_RECON_EXPAND_BYTES 16e6      // (experiment builds, tools/mkx.sh: 0 sends every reconstruction through the stored planes)
#endif
// where pair q's decoder output of the last forward lies: O on its own grid, or Oc on the coarsest grid's support (O_stale); its support term
struct OutView { const float2* O; int nx, ny; long P; };
inline OutView out_view(const aefft_net* n, const Pair& q) { return q.O_stale ? OutView{q.Oc, n->NxC, n->NyC, n->Pc} : OutView{q.O, q.Nx, q.Ny, q.P}; }
inline Contract mk_OX(const aefft_net* n, const Pair& q, int B) { const OutView v = out_view(n, q); return mk_OX(v.O, q.X, q.S, B, q.dD, q.P, v.P, q.Nx, q.Ny, v.nx, v.ny); }
// operator form: where pair l's operators of the step in progress are (A_l [OPC][dD][P], O^_l [OPC][dD][PO] on the grid nxo x nyo): op_view
struct OpView { const float2 *A, *O; int nxo, nyo; long PO; };
inline bool op_mode(const aefft_net* n) { return n->op_state || n->op_chain; }

// ---- net_forward.hip, for net_step.hip and net_score.hip -------------------------------
bool chain_form(const aefft_net* n);       // the step's forward is one chain launch: Wp && (compact || L == 1) && the switches allow it
bool op_eligible(const aefft_net* n);      // the step runs in operator form
OpView op_view(const aefft_net* n, int l);
int cc_problems(aefft_net* n, PrunedGroup& pg, int first, double* bytes);
int ensure_packed(aefft_net* n);
void fill_chain(aefft_net* n, ChainArgs& ca, int set, double* bytes);
// score (nullable, aefft_net_score): handed to the inverse transform's row pass (do_c2r); recon_d may then be null where c2r_scores_in_rows
int launch_recon(aefft_net* n, void* recon_d, int wsid, bool out_u8 = false, const ScoreArg* score = nullptr);
inline bool aligned16p(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }      // (null passes: optional pointers)
inline long score_pairs_per_frame(const aefft_net* n) { return ((long)n->D * n->Nx + 1) / 2; }
inline size_t score_map_strips(const aefft_net* n) { return ((size_t)n->B * n->D * n->Nx * n->Ny + 15) / 16; }     // the most strips: tile 8
int net_forward(aefft_net* n, const float* frames_d, bool u8, float* recon_d, bool lazy, bool op = false, bool infer = false);
#pragma GCC visibility pop

}  // namespace aefft
