// Host-side interface of the C-ABI layer (include/aefft.h), shared by its units: aefft_capi.hip (context, workspaces, flags,
// side streams, profiling), ops.hip (op helpers, op-level and spatial entry points), image_ops.hip (image-boundary entry points), register_ops.hip (registration), net.hip, net_forward.hip, net_score.hip and net_step.hip (resident network).
// The context and the profiling brackets, and the helpers one unit defines for another.  Nothing here is exported.
#pragma once
#include "../../include/aefft.h"
#include "internal.h"

#include <string>
#include <vector>

enum { WS_MID = 0, WS_REAL = 1, WS_S = 2, WS_ES = 3, WS_E = 4, WS_DC = 5, WS_DF = 6, WS_SMALL = 7, WS_DEN = 8, WS_TMP = 9, WS_PART = 10, WS_MID2 = 11, WS_MID3 = 12, WS_COUNT = 13 };

// fine-grained kernel ids for profiling; the public classes (aefft.h) aggregate them
enum {
    KID_R2C_ROWS = 0, KID_R2C_COLS, KID_C2R_COLS, KID_C2R_ROWS, KID_CONTRACT, KID_RESIZE, KID_DIFFMSE, KID_BIASGRAD,
    KID_PAD, KID_SHRINK, KID_UPDATE, KID_GDIFF, KID_SPATIAL, KID_KSPEC, KID_KGRAD, KID_WGRAD, KID_OPFORM, KID_CHAIN, KID_SGRAD, KID_OPMSE, KID_SCORE, KID_SCORE_MAP, KID_IMAGE, KID_TARGET, KID_SSIM, KID_COUNT
};

struct ProfEvent { hipEvent_t a, b; int kid; double bytes; };

// Flags of the events that order the library's OWN queues against each other: the fork and the join of the reconstruction's side stream
// (ev_fork, ev_join[]) and the three of the pipelined mode (ev_r2c, ev_mid, ev_end[]).  Device scope is enough for them: whoever waits for one
// is a kernel of this library on the same device in another queue (hipStreamWaitEvent), and the kernel packets' own agent-scope release and
// acquire order such kernels; no host thread waits for these events (aefft_sync synchronises the context stream itself) and no other device
// sees them.  Without the flag the record behind fwd_cols -- its dispatch's own completion signal -- is a system-scope release: a cache
// write-back and invalidation right behind the 25 MB of Xf that msgrad reads next.
// NEVER with this flag: the profiling pool's events (the host reads their times), the events of dp_rccl.cpp (another device's queue, or the
// host, waits for them), and any event a caller of include/aefft.h is given.
#ifndef AEFFT_X_QUEUE_EVENT_FLAGS
#define AEFFT_X_QUEUE_EVENT_FLAGS (hipEventDisableTiming | hipEventDisableSystemFence)
#endif

struct aefft_ctx {
    int device = 0;
    hipStream_t stream = nullptr;    // the caller-visible stream: every public call is ordered on it
    hipStream_t cur = nullptr;       // stream the helpers enqueue on (== stream except inside a forked section)
    bool own_stream = false;
    int biasColP1 = 0;               // operator form: conv_k biases go to the affine column of the basis frames only (Contract::biasColP1)
    bool recon_join = false;         // a deferred reconstruction (pipelined mode) still has to be joined from aux[0] (ev_join[0])
    static const int NAUX = 2;
    hipStream_t aux[NAUX] = {};      // side streams: 0 = reconstruction inverse FFT, 1 = input prefetch (created with the first net)
    hipEvent_t ev_fork = nullptr, ev_join[NAUX] = {};
    int side_cus = 0;                // aefft_ctx_partition: CUs of the side streams (0: no partition)
    std::string err;
    const float2* tw = nullptr;      // device twiddle table
    void* ws[WS_COUNT] = {};
    size_t ws_bytes[WS_COUNT] = {};
    bool prof = false;
    std::vector<ProfEvent> pool;     // pre-created events
    size_t used = 0;
    long launches[KID_COUNT] = {};
    double ms[KID_COUNT] = {};
    double bytes[KID_COUNT] = {};
};

#define HIPCHK(ctx, call)                                                     \
    do {                                                                      \
        hipError_t e_ = (call);                                               \
        if (e_ != hipSuccess) return fail(ctx, AEFFT_EHIP, #call, e_);        \
    } while (0)
#define RET_IF(x)                    \
    do {                             \
        int r_ = (x);                \
        if (r_ != AEFFT_OK) return r_; \
    } while (0)

// profiling brackets --------------------------------------------------------------------------
struct Bracket {
    aefft_ctx* ctx; int idx = -1;
    Bracket(aefft_ctx* c, int kid, double bytes) : ctx(c)
    {
        if (!c->prof) return;
        if (c->used >= c->pool.size()) return;   // pool exhausted: stop recording (read() reports what it has)
        idx = (int)c->used++;
        c->pool[idx].kid = kid; c->pool[idx].bytes = bytes;
        (void)hipEventRecord(c->pool[idx].a, c->cur);
    }
    ~Bracket() { if (idx >= 0) (void)hipEventRecord(ctx->pool[idx].b, ctx->cur); }
};

// helpers enqueue on a side stream for one scope: ctx->cur is the context stream again on every return path
struct OnStream {
    aefft_ctx* ctx;
    OnStream(aefft_ctx* c, hipStream_t s) : ctx(c) { c->cur = s; }
    ~OnStream() { ctx->cur = ctx->stream; }
};

// operator form: conv_k biases go to the affine column of the basis frames only, for one scope
struct BiasColGuard {
    aefft_ctx* ctx;
    BiasColGuard(aefft_ctx* c, int col) : ctx(c) { c->biasColP1 = col; }
    ~BiasColGuard() { ctx->biasColP1 = 0; }
};

#define CF2(p) reinterpret_cast<const float2*>(p)
#define F2(p) reinterpret_cast<float2*>(p)

struct Momentum { float *Dc, *Df, *Db, *Dp; };

namespace aefft {

// ---- aefft_capi.hip --------------------------------------------------------------------
int fail(aefft_ctx* ctx, int code, const char* what, hipError_t e = hipSuccess);
int ws_get(aefft_ctx* ctx, int slot, size_t bytes, void** out);
int ensure_aux(aefft_ctx* ctx);
int join_recon(aefft_ctx* ctx);

// ---- ops.hip (all enqueue on ctx->cur); image_ops.hip defines nothing for another unit ----
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }   // (ops.hip and image_ops.hip: required pointers)
long bins(int Nx, int Ny);
int chk_size(aefft_ctx* ctx, int Nx, int Ny);
bool net_size(int n);
int do_r2c(aefft_ctx* ctx, const float* x, float2* X, long planes, int Nx, int Ny, int Nxs, int Nys, int ws_id = WS_MID, hipEvent_t done = nullptr,
           bool u8 = false);
// out_u8: x is unsigned char [planes][Nx][Ny] (8-bit pixels, SpinToImage_C's rule; the power-of-two and mixed-radix routes only)
// score (nullable, aefft_net_score): the row-pair partial sums of the squared difference between score->frames and the rows this transform
// produces, into score->part -- by the row pass's scoring epilogue (x may then be null: nothing is stored), or, on the any-size route, by
// score_diff_kernel from the stored x (which it needs: c2r_scores_in_rows says which)
int do_c2r(aefft_ctx* ctx, const float2* X, void* x, long planes, int Nxi, int Nyi, int Nx, int Ny, float scale, int ws_id = WS_MID,
           const OpIn* opin = nullptr, bool out_u8 = false, const ScoreArg* score = nullptr);
bool c2r_scores_in_rows(int Nx, int Ny);     // a net's reconstruction on this frame grid comes out of one of the two row kernels (under the current switches)
double contract_bytes(const Contract& q);
Contract bc(const aefft_ctx* ctx, Contract q);
int do_contract(aefft_ctx* ctx, const Contract& q0);
float grad_norm(int dM, int dD, int Nx, int Ny);
Contract mk_S(const float2* Xin, const float2* T, const float2* O, float2* S, int B, int dD, long P);
Contract mk_XXneg(const float2* X, float2* S, int B, int dD, long P);
Contract mk_OX(const float2* Oc, const float2* X, float2* S, int B, int dD, long P, long Pc, int Nx, int Ny, int NxC, int NyC);
Contract mk_dc(const float2* F, const float2* S, float2* dc, int B, int dM, int dD, long P, float Norm);
Contract mk_df(const float2* C, const float2* S, float2* df, int B, int dM, int dD, long P, float Norm);
Contract mk_G(const float2* F, const float2* C, float2* G, int dM, int dD, long P);
Contract mk_gmse(const float2* G, const float2* X, const float2* F, const float* b, const float* p, float* mse_slot,
                 int B, int dM, int dD, int Nx, int Ny);
int do_contract_group(aefft_ctx* ctx, const Contract* qs, int n, int nA, int cls);
int do_conv_pooled(aefft_ctx* ctx, const float2* X, const float2* W, const float* bias, float2* Xs, int B, int R, int K,
                   int Nx, int Ny, int Nxs, int Nys, bool* done);
int do_conv(aefft_ctx* ctx, const float2* X, const float2* W, const float* bias, float2* O, int B, int R, int K, int Nx, int Ny,
            float2* Ocrop = nullptr, int Nxs = 0, int Nys = 0);
int do_conv_up(aefft_ctx* ctx, const float2* Xs, const float2* W, const float* bias, float2* O, int B, int R, int K,
               int Nx, int Ny, int sNx, int sNy);
int do_resize(aefft_ctx* ctx, const float2* in, float2* out, long planes, int Nx, int Ny, int Nxs, int Nys);
int do_diff_mse(aefft_ctx* ctx, const float2* T, const float2* O, float2* E, float* mse, float* es, int B, int dM, int dD, int Nx, int Ny);
int do_gradient(aefft_ctx* ctx, const float2* Xin, const float2* T, const float2* O, const float2* C, const float2* F,
                const float* b, float2* S, float2* dc, float2* df, float* db, float* dp, int B, int dM, int dD, int Nx, int Ny);
int do_c2r_shrink(aefft_ctx* ctx, const float2* dspec, float* gk, float* realws, float* part, long planes, int Nx, int Ny, int Nk, int Nl, float scale = 1.0f);
int do_pad_r2c(aefft_ctx* ctx, const float* k, float2* K, float* realws, long planes, int Nx, int Ny, int Nk, int Nl);
int do_update(aefft_ctx* ctx, float* c, float* f, float* b, float* p, const float* dck, const float* dfk, const float* db,
              const float* dp, Momentum mo, int dM, int dD, int Nk, int Nl, float del, int maxdiff, int sym, float gscale,
              float* zero = nullptr);
UpdateArgs mk_update(float* c, float* f, float* b, float* p, const float* dck, const float* dfk, const float* db, const float* dp,
                     Momentum mo, int dM, int dD, int Nk, int Nl, float del, int sym, float gscale, float* zero);

}  // namespace aefft

// launch() (one or more launches returning hipError_t) inside one profiling bracket: AEFFT_OK or the fail() code of its error
template <typename Launch> int launch_or_fail(aefft_ctx* ctx, int kid, double bytes, const char* what, Launch launch)
{
    hipError_t e;
    {
        Bracket br(ctx, kid, bytes);
        e = launch();
    }
    return e == hipSuccess ? AEFFT_OK : aefft::fail(ctx, AEFFT_EHIP, what, e);
}

// ... for launches that may decline shapes they do not serve (hipErrorInvalidValue): AEFFT_OK (launched), DECLINED (the error is
// cleared; the caller falls back) or the fail() code of any other error
enum { DECLINED = -1 };
template <typename Launch> int launch_or_decline(aefft_ctx* ctx, int kid, double bytes, const char* what, Launch launch)
{
    hipError_t e;
    {
        Bracket br(ctx, kid, bytes);
        e = launch();
    }
    if (e != hipErrorInvalidValue) return e == hipSuccess ? AEFFT_OK : aefft::fail(ctx, AEFFT_EHIP, what, e);
    (void)hipGetLastError();
    return DECLINED;
}
