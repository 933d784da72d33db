// C-ABI layer (include/aefft.h), context part: aefft_ctx create / destroy, the development switches (AEFFT_FLAGS, aefft_ctx_set_flags),
// workspaces, side streams and their CU partition, and the profiling API.  The op-level entry points are in ops.hip, the image-boundary ones in image_ops.hip, the resident
// network in net.hip, net_forward.hip, net_score.hip and net_step.hip; host.h is what they share.  Host-side orchestration only -- all arithmetic lives in the
// *_kernels.hip files.
#include "host.h"

#include <hip/hip_ext.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace aefft;

// ------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------
int aefft::fail(aefft_ctx* ctx, int code, const char* what, hipError_t e)
{
    if (ctx) {
        char buf[512];
        if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
        else snprintf(buf, sizeof buf, "%s", what);
        ctx->err = buf;
    }
    return code;
}

int aefft::ws_get(aefft_ctx* ctx, int slot, size_t bytes, void** out)
{
    if (ctx->ws_bytes[slot] < bytes) {
        if (ctx->ws[slot]) {
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            HIPCHK(ctx, hipFree(ctx->ws[slot]));
            ctx->ws[slot] = nullptr; ctx->ws_bytes[slot] = 0;
        }
        size_t want = (bytes + 255) & ~size_t(255);
        hipError_t e = hipMalloc(&ctx->ws[slot], want);
        if (e != hipSuccess) return fail(ctx, AEFFT_ENOMEM, "hipMalloc(workspace)", e);
        if (flag(AEFFT_F_POISON)) { HIPCHK(ctx, hipMemset(ctx->ws[slot], 0xFF, want)); HIPCHK(ctx, hipDeviceSynchronize()); }   // NaN-fill: uninitialised reads show up in the tests
        ctx->ws_bytes[slot] = want;
    }
    *out = ctx->ws[slot];
    return AEFFT_OK;
}

namespace aefft { unsigned dev_flags = 0; }
static const struct { const char* name; unsigned bit; } flag_names[] = {
    {"NOLAZY", AEFFT_F_NOLAZY}, {"NOCOMPACT", AEFFT_F_NOCOMPACT}, {"NOQPATH", AEFFT_F_NOQPATH}, {"NOFUSEMSE", AEFFT_F_NOFUSEMSE},
    {"NOGROUP", AEFFT_F_NOGROUP}, {"NOMFMA", AEFFT_F_NOMFMA}, {"NOGFWD", AEFFT_F_NOGFWD}, {"NOOVERLAP", AEFFT_F_NOOVERLAP},
    {"NOFUSECROP", AEFFT_F_NOFUSECROP}, {"GTAPS", AEFFT_F_GTAPS}, {"NOPREFETCH", AEFFT_F_NOPREFETCH}, {"NODEFER", AEFFT_F_NODEFER},
    {"NOTILEDSPATIAL", AEFFT_F_NOTILEDSPATIAL}, {"NOFAST", AEFFT_F_NOFAST}, {"NOSPLITK", AEFFT_F_NOSPLITK}, {"POISON", AEFFT_F_POISON},
    {"NOOPFORM", AEFFT_F_NOOPFORM}, {"NOCHAIN", AEFFT_F_NOCHAIN}, {"NOFUSEUPD", AEFFT_F_NOFUSEUPD}, {"NOAHEAD", AEFFT_F_NOAHEAD}, {"NORCORR", AEFFT_F_NORCORR}, {"NOLAZYMSE", AEFFT_F_NOLAZYMSE},
    {"SMALLOVERLAP", AEFFT_F_SMALLOVERLAP}, {"CHAINMSE", AEFFT_F_CHAINMSE}, {"CHIRPZ", AEFFT_F_CHIRPZ}, {"NOPRUNESMOOTH", AEFFT_F_NOPRUNESMOOTH},
    {"NOSTATICCHAIN", AEFFT_F_NOSTATICCHAIN}};
// The switches named by AEFFT_FLAGS stay on for the life of the process: aefft_ctx_set_flags ORs its argument onto them (a test fixture
// that restores "no flags" does not clear an AEFFT_FLAGS=POISON run).  A name the library does not know is an error, not a silent
// default run: the first aefft_ctx_create fails with AEFFT_EINVAL and says which.
static unsigned env_flags = 0;
static std::string env_flags_error;
static void flags_from_env_once()
{
    static bool done = false;
    if (done) return;
    done = true;
    const char* e = getenv("AEFFT_FLAGS");           // the ONLY environment lookup of the library
    if (!e) return;
    std::string s(e);
    size_t i = 0;
    while (i <= s.size()) {
        size_t j = s.find(',', i);
        if (j == std::string::npos) j = s.size();
        const std::string w = s.substr(i, j - i);
        bool known = w.empty();
        for (const auto& f : flag_names) if (w == f.name) { env_flags |= f.bit; known = true; }
        if (!known) env_flags_error += (env_flags_error.empty() ? "" : ",") + w;
        i = j + 1;
    }
    dev_flags = env_flags;
}
extern "C" int aefft_ctx_set_flags(aefft_ctx* ctx, unsigned flags) { if (!ctx) return AEFFT_EINVAL; dev_flags = env_flags | flags; return AEFFT_OK; }
extern "C" unsigned aefft_ctx_get_flags(const aefft_ctx*) { return dev_flags; }

extern "C" const char* aefft_version(void) { return "aefft 0.2 (gfx950)"; }

extern "C" int aefft_ctx_create(aefft_ctx** out, int device, void* hip_stream, int create_stream)
{
    if (!out) return AEFFT_EINVAL;
    *out = nullptr;
    flags_from_env_once();
    if (!env_flags_error.empty()) { fprintf(stderr, "aefft: unknown name(s) in AEFFT_FLAGS: %s\n", env_flags_error.c_str()); return AEFFT_EINVAL; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return AEFFT_EHIP;
    aefft_ctx* ctx = new aefft_ctx();
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess) { delete ctx; return AEFFT_EHIP; }
    if (!create_stream) ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);   // NULL = the legacy default stream
    else {
        // the library's own stream carries the latency-bound chain of the step: highest priority, so that the bandwidth-bound
        // side-stream work (reconstruction, input prefetch) takes the slots it leaves free instead of crowding it out
        int pr_least = 0, pr_greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&pr_least, &pr_greatest);
        if (hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, pr_greatest) != hipSuccess) { delete ctx; return AEFFT_EHIP; }
        ctx->own_stream = true;
    }
    if (upload_twiddles(ctx->stream) != hipSuccess) { if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream); delete ctx; return AEFFT_EHIP; }
    ctx->cur = ctx->stream;
    ctx->tw = twiddle_table();
    *out = ctx;
    return AEFFT_OK;
}

extern "C" void aefft_ctx_destroy(aefft_ctx* ctx)
{
    if (!ctx) return;
    (void)hipStreamSynchronize(ctx->stream);
    for (int i = 0; i < WS_COUNT; ++i) if (ctx->ws[i]) (void)hipFree(ctx->ws[i]);
    for (auto& e : ctx->pool) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    for (int i = 0; i < aefft_ctx::NAUX; ++i) { if (ctx->aux[i]) { (void)hipStreamSynchronize(ctx->aux[i]); (void)hipStreamDestroy(ctx->aux[i]); } if (ctx->ev_join[i]) (void)hipEventDestroy(ctx->ev_join[i]); }
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

// CU mask of one side of the partition: the side streams take mask bits [0, side_cus), the context stream the rest.  (Mask bits are dealt
// to the XCDs round-robin by the driver -- tools/cumask_probe.hip -- so a run of consecutive bits is the same share of every XCD.)
static hipError_t masked_stream(hipStream_t* st, int ncu, int lo, int hi)
{
    std::vector<uint32_t> m((size_t)(ncu + 31) / 32, 0u);
    for (int i = lo; i < hi; ++i) m[(size_t)i / 32] |= 1u << (i % 32);
    return hipExtStreamCreateWithCUMask(st, (uint32_t)m.size(), m.data());
}
static int device_cus(int device)
{
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) return 0;
    return n;
}

// side streams (0: reconstruction inverse FFT, 1: input prefetch) and their events (device scope: host.h AEFFT_X_QUEUE_EVENT_FLAGS); all-or-nothing
int aefft::ensure_aux(aefft_ctx* ctx)
{
    if (ctx->aux[0]) return AEFFT_OK;
    hipError_t e = hipSuccess;
    for (int i = 0; i < aefft_ctx::NAUX && e == hipSuccess; ++i) {
        int pr_least = 0, pr_greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&pr_least, &pr_greatest);
        if (ctx->side_cus > 0) e = masked_stream(&ctx->aux[i], device_cus(ctx->device), 0, ctx->side_cus);
        else
        e = hipStreamCreateWithPriority(&ctx->aux[i], hipStreamNonBlocking, pr_least);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_join[i], AEFFT_X_QUEUE_EVENT_FLAGS);
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_fork, AEFFT_X_QUEUE_EVENT_FLAGS);
    if (e == hipSuccess) return AEFFT_OK;
    for (int i = 0; i < aefft_ctx::NAUX; ++i) {
        if (ctx->aux[i]) (void)hipStreamDestroy(ctx->aux[i]);
        if (ctx->ev_join[i]) (void)hipEventDestroy(ctx->ev_join[i]);
        ctx->aux[i] = nullptr; ctx->ev_join[i] = nullptr;
    }
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    ctx->ev_fork = nullptr;
    return fail(ctx, AEFFT_EHIP, "side streams", e);
}

extern "C" int aefft_ctx_partition(aefft_ctx* ctx, int side_cus)
{
    if (!ctx) return AEFFT_EINVAL;
    if (!ctx->own_stream || ctx->aux[0]) return fail(ctx, AEFFT_ESTATE, "aefft_ctx_partition: needs a context that owns its stream, before its first net");
    const int ncu = device_cus(ctx->device);
    if (side_cus < 0 || (side_cus > 0 && (ncu < 16 || side_cus < 8 || side_cus > ncu - 8))) return fail(ctx, AEFFT_EINVAL, "aefft_ctx_partition: side_cus out of range");
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    hipStream_t st = nullptr;
    if (side_cus > 0) HIPCHK(ctx, masked_stream(&st, ncu, side_cus, ncu));
    else {
        int pr_least = 0, pr_greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&pr_least, &pr_greatest);
        HIPCHK(ctx, hipStreamCreateWithPriority(&st, hipStreamNonBlocking, pr_greatest));
    }
    (void)hipStreamDestroy(ctx->stream);
    ctx->stream = ctx->cur = st;
    ctx->side_cus = side_cus;
    return AEFFT_OK;
}

extern "C" const char* aefft_last_error(const aefft_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }
int aefft::join_recon(aefft_ctx* ctx)
{
    if (!ctx->recon_join) return AEFFT_OK;
    HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join[0], 0));
    ctx->recon_join = false;
    return AEFFT_OK;
}
extern "C" int aefft_sync(aefft_ctx* ctx) { if (!ctx) return AEFFT_EINVAL; RET_IF(join_recon(ctx)); HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); return AEFFT_OK; }
extern "C" void* aefft_stream(aefft_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

extern "C" int aefft_prof_enable(aefft_ctx* ctx, int enable)
{
    if (!ctx) return AEFFT_EINVAL;
    if (enable && ctx->pool.empty()) {
        ctx->pool.resize(8192);
        for (auto& e : ctx->pool) { HIPCHK(ctx, hipEventCreate(&e.a)); HIPCHK(ctx, hipEventCreate(&e.b)); }
    }
    ctx->prof = enable != 0;
    return AEFFT_OK;
}

static int prof_collect(aefft_ctx* ctx)
{
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < aefft_ctx::NAUX; ++i) if (ctx->aux[i]) HIPCHK(ctx, hipStreamSynchronize(ctx->aux[i]));
    for (size_t i = 0; i < ctx->used; ++i) {
        float ms = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->pool[i].a, ctx->pool[i].b));
        const int k = ctx->pool[i].kid;
        ctx->launches[k]++; ctx->ms[k] += ms; ctx->bytes[k] += ctx->pool[i].bytes;
    }
    ctx->used = 0;
    return AEFFT_OK;
}

extern "C" int aefft_prof_reset(aefft_ctx* ctx)
{
    if (!ctx) return AEFFT_EINVAL;
    RET_IF(prof_collect(ctx));
    memset(ctx->launches, 0, sizeof ctx->launches); memset(ctx->ms, 0, sizeof ctx->ms); memset(ctx->bytes, 0, sizeof ctx->bytes);
    return AEFFT_OK;
}

static const char* kid_names[KID_COUNT] = {"r2c_rows", "r2c_cols", "c2r_cols", "c2r_rows", "contract", "resize", "diff_mse",
                                           "bias_grad", "pad", "shrink", "update", "gradient_diff", "spatial", "kspec", "kgrad", "weight_taps", "moment", "chain", "sgrad", "opmse", "score", "score_map", "image", "target", "ssim"};

extern "C" int aefft_prof_read(aefft_ctx* ctx, int kid, long* launches, double* total_ms, double* algo_bytes)
{
    if (!ctx || kid < 0 || kid >= KID_COUNT) return AEFFT_EINVAL;
    RET_IF(prof_collect(ctx));
    if (launches) *launches = ctx->launches[kid];
    if (total_ms) *total_ms = ctx->ms[kid];
    if (algo_bytes) *algo_bytes = ctx->bytes[kid];
    return AEFFT_OK;
}
extern "C" const char* aefft_prof_name(int kid) { return (kid >= 0 && kid < KID_COUNT) ? kid_names[kid] : nullptr; }
extern "C" int aefft_prof_count(void) { return KID_COUNT; }
