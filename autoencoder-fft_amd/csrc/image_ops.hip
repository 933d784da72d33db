// C-ABI layer (include/aefft.h), image boundary: the entry points between camera images as delivered and the library's planar frames.  Host code only:
// every call checks its arguments, joins a deferred reconstruction and hands over to the launcher of its kernel file.
#include "host.h"
#include <climits>
#include <cmath>

using namespace aefft;

// image boundary ------------------------------------------------------------------------------
// the rules of include/aefft.h "image boundary", each once; where two calls word one rule differently, the words are an argument; nothing is enqueued
// when one fails.  A rejection is AEFFT_EINVAL with "<call>: <rule>" as the context's last error
struct Bad {
    aefft_ctx* ctx; const char* fn;
    int operator()(const std::string& rule) const { return fail(ctx, AEFFT_EINVAL, (std::string(fn) + ": " + rule).c_str()); }
};
static const size_t HALF = ~size_t(0) >> 1;          // what "fits the address space" means
static bool dim_ok(int v) { return v >= 1 && v <= 8192; }
static bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + nb && b0 < a0 + na;
}
// the sizes of a batch of images or frames: D, B and the two sizes; `names` is how the call's sentence lists them, `others` the verdict on further sizes it lists
static int chk_dims(const Bad& bad, int B, int D, int W, int H, const char* names = "W, H", bool others = true)
{
    if (D < 1 || D > 4) return bad("D must be 1..4 (grey, BGR, BGRA)");
    if (B < 1 || !dim_ok(W) || !dim_ok(H) || !others) return bad(std::string("B must be >= 1 and ") + names + " in 1..8192");
    return AEFFT_OK;
}
static int chk_frame_size(const Bad& bad, int Nx, int Ny) { return dim_ok(Nx) && dim_ok(Ny) ? AEFFT_OK : bad("Nx, Ny must be in 1..8192"); }
// the image buffer rule: B buffers of `rows` rows, `live` bytes of each row used, a pitch between rows and a stride between buffers (read for
// B > 1 only).  `extent` receives the bytes from the first buffer's first byte to the last one's last live byte
struct RowWords { const char *pitch, *rows, *stride, *batch; };
static const RowWords IMAGE_WORDS = {"pitch must be at least W * D bytes", "H * pitch does not fit the address space",
                                     "image_stride must be at least (H - 1) * pitch + W * D bytes for B > 1", "B * image_stride does not fit the address space"};
// (aefft_image_to_frames / aefft_frames_to_image have no stride argument: image b + 1 starts Ny * pitch behind image b, and one bound covers the batch)
static const RowWords PACKED_WORDS = {"pitch must be at least Nx * D bytes", "B * Ny * pitch does not fit the address space", nullptr, nullptr};
static const RowWords PLANE_WORDS = {"pitch too small: pitch[0] >= W (YUYV 2 W), NV12 pitch[1] >= 2 ceil(W / 2), I420 pitch[1], pitch[2] >= ceil(W / 2)",
                                     "rows * pitch does not fit the address space", "stride too small: each used stride[k] must be at least (rows - 1) * "
                                     "pitch[k] + the live bytes of a row for B > 1", "B * stride does not fit the address space"};
static int chk_rows(const Bad& bad, const RowWords& w, size_t pitch, size_t stride, size_t live, size_t rows, int B, size_t* extent)
{
    if (pitch < live) return bad(w.pitch);
    if (!w.stride) { rows *= (size_t)B; B = 1; }
    if (pitch > HALF / rows) return bad(w.rows);
    const size_t one = (rows - 1) * pitch + live;                              // the bytes of one buffer, up to its last row's live bytes
    if (B > 1 && stride < one) return bad(w.stride);
    if (B > 1 && stride > (HALF - one) / (size_t)(B - 1)) return bad(w.batch);
    *extent = (B > 1 ? (size_t)(B - 1) * stride : 0) + one;
    return AEFFT_OK;
}
static int chk_present_image(const Bad& bad, size_t pitch, size_t image_stride, int W, int H, int B, int D, size_t* extent)
{
    RET_IF(chk_dims(bad, B, D, W, H));
    return chk_rows(bad, IMAGE_WORDS, pitch, image_stride, (size_t)W * D, (size_t)H, B, extent);
}
// the frames buffer rule: `count` (B, or the tile calls' T) frames of D * Nx * Ny elements, 8-bit or float, behind a 16-byte aligned pointer; `bytes`
// receives their size.  `names`: the pointer(s) the alignment sentence speaks of; `int_rule`, where set: the sentence for a count beyond an int
static int chk_frames_aligned16(const Bad& bad, const void* p, const char* names, const char* count_name, size_t count, int D, int Nx, int Ny, int u8, size_t* bytes, const char* int_rule = nullptr)
{
    if (!aligned16(p)) return bad(std::string(names) + " must be 16-byte aligned");
    if (int_rule && count > (size_t)INT_MAX) return bad(int_rule);
    const size_t per = (size_t)D * Nx * Ny * (u8 ? 1 : 4);                     // (at most 2^30 bytes of one frame set)
    if (count > HALF / per) return bad(std::string(count_name) + " * D * Nx * Ny does not fit the address space");
    *bytes = count * per;
    return AEFFT_OK;
}
// the mode rule: LINEAR or AREA, and AREA from (sw, sh) to (dw, dh) does not enlarge; `needs` words that for the call's direction
static int chk_mode(const Bad& bad, int mode, int sw, int sh, int dw, int dh, const char* needs)
{
    if (mode != AEFFT_RESIZE_LINEAR && mode != AEFFT_RESIZE_AREA) return bad("mode must be AEFFT_RESIZE_LINEAR or AEFFT_RESIZE_AREA");
    if (mode == AEFFT_RESIZE_AREA && (dw > sw || dh > sh)) return bad(std::string("AEFFT_RESIZE_AREA does not enlarge: it needs ") + needs);
    return AEFFT_OK;
}

// pack and unpack -----------------------------------------------------------------------------
static int chk_image(const Bad& bad, const void* image_d, size_t pitch, const void* frames_d, int frames_u8, int B, int D, int Nx, int Ny)
{
    if (!bad.ctx || !image_d || !frames_d) return bad("null context, image or frames");
    RET_IF(chk_dims(bad, B, D, Nx, Ny, "Nx, Ny"));
    size_t extent = 0, fb = 0;                        // the bytes either side touches: the image up to the last row's Nx * D, the frames whole
    RET_IF(chk_rows(bad, PACKED_WORDS, pitch, 0, (size_t)Nx * D, (size_t)Ny, B, &extent));
    RET_IF(chk_frames_aligned16(bad, frames_d, "frames_d", "B", (size_t)B, D, Nx, Ny, frames_u8, &fb));
    if (ranges_overlap(frames_d, fb, image_d, extent)) return bad("the frame and image ranges overlap (the op is out-of-place)");
    return AEFFT_OK;
}

extern "C" int aefft_image_to_frames(aefft_ctx* ctx, const unsigned char* image_d, size_t pitch, void* frames_d, int frames_u8, int B, int D, int Nx, int Ny)
{
    RET_IF(chk_image(Bad{ctx, "aefft_image_to_frames"}, image_d, pitch, frames_d, frames_u8, B, D, Nx, Ny));
    RET_IF(join_recon(ctx));                          // (frames_d may be a buffer a deferred reconstruction is still writing)
    return launch_or_fail(ctx, KID_IMAGE, (double)B * D * Nx * Ny * (frames_u8 ? 2.0 : 5.0), "image_unpack",
                          [&] { return launch_image_unpack(image_d, pitch, frames_d, !frames_u8, B, D, Nx, Ny, ctx->cur); });
}

extern "C" int aefft_frames_to_image(aefft_ctx* ctx, const void* frames_d, int frames_u8, unsigned char* image_d, size_t pitch, int B, int D, int Nx, int Ny)
{
    RET_IF(chk_image(Bad{ctx, "aefft_frames_to_image"}, image_d, pitch, frames_d, frames_u8, B, D, Nx, Ny));
    RET_IF(join_recon(ctx));                          // (frames_d may be the reconstruction of a step whose inverse transform is still on the side stream)
    return launch_or_fail(ctx, KID_IMAGE, (double)B * D * Nx * Ny * (frames_u8 ? 2.0 : 5.0), "image_pack",
                          [&] { return launch_image_pack(frames_d, !frames_u8, image_d, pitch, B, D, Nx, Ny, ctx->cur); });
}

// resize in and out, overlay, degrade ---------------------------------------------------------
extern "C" int aefft_image_resize_to_frames(aefft_ctx* ctx, const unsigned char* image_d, size_t pitch, size_t image_stride, int W, int H, int mode,
                                            void* frames_d, int frames_u8, int B, int D, int Nx, int Ny)
{
    const Bad bad{ctx, "aefft_image_resize_to_frames"};
    if (!ctx || !image_d || !frames_d) return bad("null context, image or frames");
    RET_IF(chk_dims(bad, B, D, W, H, "W, H, Nx, Ny", dim_ok(Nx) && dim_ok(Ny)));
    RET_IF(chk_mode(bad, mode, W, H, Nx, Ny, "Nx <= W and Ny <= H"));
    size_t extent = 0, fb = 0;
    RET_IF(chk_rows(bad, IMAGE_WORDS, pitch, image_stride, (size_t)W * D, (size_t)H, B, &extent));
    RET_IF(chk_frames_aligned16(bad, frames_d, "frames_d", "B", (size_t)B, D, Nx, Ny, frames_u8, &fb));
    if (ranges_overlap(frames_d, fb, image_d, extent)) return bad("the frame and image ranges overlap (the op is out-of-place)");
    RET_IF(join_recon(ctx));                          // (frames_d may be a buffer a deferred reconstruction is still writing)
    return launch_or_fail(ctx, KID_IMAGE, (double)B * D * ((double)W * H + (double)Nx * Ny * (frames_u8 ? 1.0 : 4.0)), "image_resize",
                          [&] { return launch_image_resize(image_d, pitch, image_stride, W, H, mode, frames_d, !frames_u8, B, D, Nx, Ny, ctx->cur); });
}

extern "C" int aefft_frames_resize_to_image(aefft_ctx* ctx, const void* frames_d, int frames_u8, int Nx, int Ny, int mode,
                                            unsigned char* image_d, size_t pitch, size_t image_stride, int W, int H, int B, int D)
{
    const Bad bad{ctx, "aefft_frames_resize_to_image"};
    if (!ctx || !image_d || !frames_d) return bad("null context, image or frames");
    RET_IF(chk_frame_size(bad, Nx, Ny));
    size_t extent = 0, fb = 0;
    RET_IF(chk_present_image(bad, pitch, image_stride, W, H, B, D, &extent));
    RET_IF(chk_mode(bad, mode, Nx, Ny, W, H, "W <= Nx and H <= Ny"));
    RET_IF(chk_frames_aligned16(bad, frames_d, "frames_d", "B", (size_t)B, D, Nx, Ny, frames_u8, &fb));
    if (ranges_overlap(frames_d, fb, image_d, extent)) return bad("the frame and image ranges overlap (the op is out-of-place)");
    RET_IF(join_recon(ctx));                          // (frames_d may be the reconstruction of a step whose inverse transform is still on the side stream)
    return launch_or_fail(ctx, KID_IMAGE, (double)B * D * ((double)Nx * Ny * (frames_u8 ? 1.0 : 4.0) + (double)W * H), "frames_resize",
                          [&] { return launch_frames_resize(frames_d, !frames_u8, Nx, Ny, mode, image_d, pitch, image_stride, W, H, B, D, ctx->cur); });
}

extern "C" int aefft_map_overlay_image(aefft_ctx* ctx, const float* map_d, int Mx, int My, float lo, float hi, int smooth, const unsigned char* lut_d, int alpha,
                                       unsigned char* image_d, size_t pitch, size_t image_stride, int W, int H, int B, int D)
{
    const Bad bad{ctx, "aefft_map_overlay_image"};
    if (!ctx || !map_d || !lut_d || !image_d) return bad("null context, map, lut or image");
    if (Mx < 1 || My < 1 || Mx > 1024 || My > 1024) return bad("Mx, My must be in 1..1024");
    size_t extent = 0;
    RET_IF(chk_present_image(bad, pitch, image_stride, W, H, B, D, &extent));
    if (alpha < 0 || alpha > 256) return bad("alpha must be 0..256");
    const float inv = 255.0f / (hi - lo);
    if (!std::isfinite(lo) || !std::isfinite(hi) || lo == hi || !std::isfinite(inv)) return bad("lo and hi must be finite and different (255 / (hi - lo) finite)");
    if (!aligned16(map_d)) return bad("map_d must be 16-byte aligned");
    if ((size_t)B > HALF / ((size_t)4 * Mx * My)) return bad("B * Mx * My does not fit the address space");
    if (ranges_overlap(map_d, (size_t)B * Mx * My * 4, image_d, extent)) return bad("the map and image ranges overlap");
    if (ranges_overlap(lut_d, (size_t)256 * D, image_d, extent)) return bad("the lut and image ranges overlap");
    RET_IF(join_recon(ctx));                          // (image_d may hold a reconstruction that is still on the side stream)
    return launch_or_fail(ctx, KID_IMAGE, (double)B * (4.0 * Mx * My + 2.0 * D * W * H) + 256.0 * D, "map_overlay",
                          [&] { return launch_map_overlay(map_d, Mx, My, lo, inv, smooth, lut_d, alpha, image_d, pitch, image_stride, W, H, B, D, ctx->cur); });
}

extern "C" int aefft_frames_degrade(aefft_ctx* ctx, const void* src_d, int src_u8, void* dst_d, int dst_u8, int B, int D, int Nx, int Ny,
                                    int blur, float sigma, float impulse, unsigned long long seed, unsigned long long first_frame)
{
    const Bad bad{ctx, "aefft_frames_degrade"};
    if (!ctx || !src_d || !dst_d) return bad("null context, source or destination");
    RET_IF(chk_dims(bad, B, D, Nx, Ny, "Nx, Ny"));
    if (blur < 0 || blur > 4) return bad("blur must be 0..4");
    if (!std::isfinite(sigma) || sigma < 0.f || sigma > 255.f) return bad("sigma must be finite and in 0..255");
    if (!std::isfinite(impulse) || impulse < 0.f || impulse > 1.f) return bad("impulse must be finite and in 0..1");
    size_t sb = 0, db = 0;
    RET_IF(chk_frames_aligned16(bad, src_d, "src_d and dst_d", "B", (size_t)B, D, Nx, Ny, src_u8, &sb));
    RET_IF(chk_frames_aligned16(bad, dst_d, "src_d and dst_d", "B", (size_t)B, D, Nx, Ny, dst_u8, &db));
    const bool in_place = dst_d == src_d && blur == 0 && !src_u8 == !dst_u8;
    if (!in_place && ranges_overlap(src_d, sb, dst_d, db)) return bad("the source and destination ranges overlap (in place needs dst_d == src_d, blur == 0 and src_u8 == dst_u8)");
    RET_IF(join_recon(ctx));                          // (src_d may be a reconstruction that is still on the side stream)
    return launch_or_fail(ctx, KID_IMAGE, (double)(sb + db), "frames_degrade",
                          [&] { return launch_degrade(src_d, !src_u8, dst_d, !dst_u8, B, D, Nx, Ny, blur, sigma, impulse, seed, first_frame, ctx->cur); });
}

// YUV video -----------------------------------------------------------------------------------
// the source bytes one image's conversion reads: the luma samples and, unless the order is GRAY, the chroma samples (YUYV: the rows whole)
static double yuv_bytes(const aefft_yuv_desc& s, int order)
{
    const double W = s.W, H = s.H, Wc = (s.W + 1) / 2, Hc = (s.H + 1) / 2;
    if (s.format == AEFFT_YUV_YUYV) return 2.0 * W * H;
    return W * H + (order == AEFFT_YUV_GRAY ? 0.0 : 2.0 * Wc * Hc);
}
// the source rules aefft_yuv_to_image and aefft_yuv_resize_to_frames share: `D` receives the channels the order asks for, `used` the planes the call
// reads and `extent[k]` the bytes of plane k over the B images, first byte to last
// (Desc: aefft_yuv_desc, or the aefft_yuv_dst of the calls that write the planes -- the same fields; `gray_luma_only`: GRAY uses plane[0] alone, which
// holds for a source; `null_rule` words the planes the side needs; `one[k]`, where asked for, receives the bytes of ONE image's plane k)
template <class Desc>
static int chk_yuv_planes(const Bad& bad, const Desc* src, int order, int B, bool gray_luma_only, const char* null_rule, int* D, int* used, size_t* extent, size_t* one = nullptr)
{
    if (src->format != AEFFT_YUV_NV12 && src->format != AEFFT_YUV_I420 && src->format != AEFFT_YUV_YUYV) return bad("format must be AEFFT_YUV_NV12, AEFFT_YUV_I420 or AEFFT_YUV_YUYV");
    if (src->matrix != AEFFT_YUV_BT601 && src->matrix != AEFFT_YUV_BT709 && src->matrix != AEFFT_YUV_JPEG) return bad("matrix must be AEFFT_YUV_BT601, AEFFT_YUV_BT709 or AEFFT_YUV_JPEG");
    if (order != AEFFT_YUV_BGR && order != AEFFT_YUV_RGB && order != AEFFT_YUV_GRAY) return bad("order must be AEFFT_YUV_BGR, AEFFT_YUV_RGB or AEFFT_YUV_GRAY");
    *D = order == AEFFT_YUV_GRAY ? 1 : 3;
    RET_IF(chk_dims(bad, B, *D, src->W, src->H));
    const bool yuyv = src->format == AEFFT_YUV_YUYV;
    if (yuyv && (src->W & 1)) return bad("YUYV needs an even W");
    const size_t W = (size_t)src->W, H = (size_t)src->H, Wc = (W + 1) / 2, Hc = (H + 1) / 2;
    // live bytes of a row and rows of each plane
    const size_t live[3] = {yuyv ? 2 * W : W, src->format == AEFFT_YUV_NV12 ? 2 * Wc : Wc, Wc}, rows[3] = {H, Hc, Hc};
    *used = (gray_luma_only && order == AEFFT_YUV_GRAY) || yuyv ? 1 : (src->format == AEFFT_YUV_NV12 ? 2 : 3);
    for (int k = 0; k < *used; ++k) {
        if (!src->plane[k]) return bad(null_rule);
        RET_IF(chk_rows(bad, PLANE_WORDS, src->pitch[k], src->stride[k], live[k], rows[k], B, &extent[k]));
        if (one) one[k] = (rows[k] - 1) * src->pitch[k] + live[k];
    }
    return AEFFT_OK;
}
static int chk_yuv_source(const Bad& bad, const aefft_yuv_desc* src, int order, int B, int* D, int* used, size_t* extent)
{
    return chk_yuv_planes(bad, src, order, B, true, "null plane (NV12 needs plane[0..1], I420 plane[0..2], YUYV and AEFFT_YUV_GRAY plane[0])", D, used, extent);
}

extern "C" int aefft_yuv_to_image(aefft_ctx* ctx, const aefft_yuv_desc* src, int order, unsigned char* image_d, size_t pitch, size_t image_stride, int B)
{
    const Bad bad{ctx, "aefft_yuv_to_image"};
    if (!ctx || !src || !image_d) return bad("null context, descriptor or image");
    int D = 0, used = 0;
    size_t sext[3] = {0, 0, 0}, extent = 0;
    RET_IF(chk_yuv_source(bad, src, order, B, &D, &used, sext));
    RET_IF(chk_rows(bad, IMAGE_WORDS, pitch, image_stride, (size_t)src->W * D, (size_t)src->H, B, &extent));
    for (int k = 0; k < used; ++k)
        if (ranges_overlap(src->plane[k], sext[k], image_d, extent)) return bad("a source plane and the image range overlap (the op is out-of-place)");
    RET_IF(join_recon(ctx));                          // (a plane may be a buffer the side stream is still writing)
    return launch_or_fail(ctx, KID_IMAGE, (double)B * (yuv_bytes(*src, order) + (double)D * src->W * src->H), "yuv_to_image", [&] {
        return launch_yuv_image(src->format, src->plane, src->pitch, src->stride, src->W, src->H, src->matrix, order, image_d, pitch, image_stride, B, ctx->cur);
    });
}

extern "C" int aefft_yuv_resize_to_frames(aefft_ctx* ctx, const aefft_yuv_desc* src, int order, int mode, void* frames_d, int frames_u8, int B, int Nx, int Ny)
{
    const Bad bad{ctx, "aefft_yuv_resize_to_frames"};
    if (!ctx || !src || !frames_d) return bad("null context, descriptor or frames");
    int D = 0, used = 0;
    size_t sext[3] = {0, 0, 0}, fb = 0;
    RET_IF(chk_yuv_source(bad, src, order, B, &D, &used, sext));
    RET_IF(chk_frame_size(bad, Nx, Ny));
    RET_IF(chk_mode(bad, mode, src->W, src->H, Nx, Ny, "Nx <= W and Ny <= H"));
    RET_IF(chk_frames_aligned16(bad, frames_d, "frames_d", "B", (size_t)B, D, Nx, Ny, frames_u8, &fb));
    for (int k = 0; k < used; ++k)
        if (ranges_overlap(src->plane[k], sext[k], frames_d, fb)) return bad("a source plane and the frame range overlap (the op is out-of-place)");
    RET_IF(join_recon(ctx));                          // (frames_d may be a buffer a deferred reconstruction is still writing)
    return launch_or_fail(ctx, KID_IMAGE, (double)B * (yuv_bytes(*src, order) + (double)(fb / (size_t)B)), "yuv_resize", [&] {
        return launch_yuv_resize(src->format, src->plane, src->pitch, src->stride, src->W, src->H, src->matrix, order, mode, frames_d, !frames_u8, B, Nx, Ny, ctx->cur);
    });
}

// YUV video out (include/aefft.h "aefft_image_to_yuv, aefft_frames_resize_to_yuv") ---------------
// two batches of B buffers each, buffer i at base + i * stride (ascending, not meeting one another: chk_rows), n bytes long: does any buffer of one
// meet any of the other?  NV12 surfaces in a batch interleave -- surface b's chroma lies between the lumas of b and b + 1 --, so the batches' whole
// extents say nothing; one sweep over both in address order does
static bool batches_overlap(const void* a, size_t sa, size_t na, const void* b, size_t sb, size_t nb, int B)
{
    if (B == 1) sa = sb = 0;
    if (!ranges_overlap(a, (size_t)(B - 1) * sa + na, b, (size_t)(B - 1) * sb + nb)) return false;
    for (int i = 0, j = 0; i < B && j < B;) {
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(a) + (size_t)i * sa, b0 = reinterpret_cast<uintptr_t>(b) + (size_t)j * sb;
        if (a0 < b0 + nb && b0 < a0 + na) return true;
        if (a0 + na <= b0 + nb) ++i; else ++j;       // (the one that ends first cannot meet a later buffer of the other)
    }
    return false;
}
// the destination rules aefft_image_to_yuv and aefft_frames_resize_to_yuv share: chk_yuv_planes with every plane of the format needed (GRAY writes
// 128 into the chroma) and the planes not meeting one another; `D` receives the channels the order names, `used` the planes the call writes and
// `one[k]` the bytes of one image's plane k
static int chk_yuv_dest(const Bad& bad, const aefft_yuv_dst* dst, int order, int B, int* D, int* used, size_t* one)
{
    size_t extent[3] = {0, 0, 0};
    RET_IF(chk_yuv_planes(bad, dst, order, B, false, "null plane (NV12 needs plane[0..1], I420 plane[0..2], YUYV plane[0])", D, used, extent, one));
    for (int k = 0; k < *used; ++k)
        for (int l = k + 1; l < *used; ++l)
            if (batches_overlap(dst->plane[k], dst->stride[k], one[k], dst->plane[l], dst->stride[l], one[l], B)) return bad("two destination planes' byte ranges overlap");
    return AEFFT_OK;
}
// no destination plane meets the source: B buffers of src_one bytes, src_stride apart
static int chk_yuv_dest_source(const Bad& bad, const aefft_yuv_dst* dst, int used, const size_t* one, int B, const void* src, size_t src_stride, size_t src_one)
{
    for (int k = 0; k < used; ++k)
        if (batches_overlap(dst->plane[k], dst->stride[k], one[k], src, src_stride, src_one, B)) return bad("a destination plane and the source range overlap (the op is out-of-place)");
    return AEFFT_OK;
}
// the bytes one image's conversion writes: every plane of the format
static double yuv_dst_bytes(const aefft_yuv_dst& d)
{
    const double W = d.W, H = d.H, Wc = (d.W + 1) / 2, Hc = (d.H + 1) / 2;
    return d.format == AEFFT_YUV_YUYV ? 2.0 * W * H : W * H + 2.0 * Wc * Hc;
}

extern "C" int aefft_image_to_yuv(aefft_ctx* ctx, const unsigned char* image_d, size_t pitch, size_t image_stride, int order, const aefft_yuv_dst* dst, int B)
{
    const Bad bad{ctx, "aefft_image_to_yuv"};
    if (!ctx || !dst || !image_d) return bad("null context, descriptor or image");
    int D = 0, used = 0;
    size_t one[3] = {0, 0, 0}, extent = 0;
    RET_IF(chk_yuv_dest(bad, dst, order, B, &D, &used, one));
    RET_IF(chk_present_image(bad, pitch, image_stride, dst->W, dst->H, B, D, &extent));
    RET_IF(chk_yuv_dest_source(bad, dst, used, one, B, image_d, image_stride, (size_t)(dst->H - 1) * pitch + (size_t)dst->W * D));
    RET_IF(join_recon(ctx));                          // (image_d may hold a reconstruction that is still on the side stream)
    return launch_or_fail(ctx, KID_IMAGE, (double)B * ((double)D * dst->W * dst->H + yuv_dst_bytes(*dst)), "image_to_yuv", [&] {
        return launch_image_yuv(image_d, pitch, image_stride, order, dst->format, dst->plane, dst->pitch, dst->stride, dst->W, dst->H, dst->matrix, B, ctx->cur);
    });
}

extern "C" int aefft_frames_resize_to_yuv(aefft_ctx* ctx, const void* frames_d, int frames_u8, int Nx, int Ny, int mode, int order, const aefft_yuv_dst* dst, int B)
{
    const Bad bad{ctx, "aefft_frames_resize_to_yuv"};
    if (!ctx || !dst || !frames_d) return bad("null context, descriptor or frames");
    int D = 0, used = 0;
    size_t one[3] = {0, 0, 0}, fb = 0;
    RET_IF(chk_yuv_dest(bad, dst, order, B, &D, &used, one));
    RET_IF(chk_frame_size(bad, Nx, Ny));
    RET_IF(chk_mode(bad, mode, Nx, Ny, dst->W, dst->H, "W <= Nx and H <= Ny"));
    RET_IF(chk_frames_aligned16(bad, frames_d, "frames_d", "B", (size_t)B, D, Nx, Ny, frames_u8, &fb));
    RET_IF(chk_yuv_dest_source(bad, dst, used, one, B, frames_d, fb / (size_t)B, fb / (size_t)B));
    RET_IF(join_recon(ctx));                          // (frames_d may be the reconstruction of a step whose inverse transform is still on the side stream)
    return launch_or_fail(ctx, KID_IMAGE, (double)fb + (double)B * yuv_dst_bytes(*dst), "frames_to_yuv", [&] {
        return launch_frames_yuv(frames_d, !frames_u8, Nx, Ny, mode, order, dst->format, dst->plane, dst->pitch, dst->stride, dst->W, dst->H, dst->matrix, B, ctx->cur);
    });
}

// regions (include/aefft.h "aefft_map_regions") ------------------------------------------------
extern "C" size_t aefft_map_regions_workspace(int Mx, int My, int B) { return map_regions_workspace(Mx, My, B); }

extern "C" int aefft_map_regions(aefft_ctx* ctx, const float* map_d, const float* ref_d, int Mx, int My, int B, int sense, float lo, float hi, int connectivity,
                                 int min_area, int* labels_d, aefft_region* regions_d, int max_regions, int* count_d, void* work_d, size_t work_bytes)
{
    const Bad bad{ctx, "aefft_map_regions"};
    if (!ctx || !map_d || !labels_d || !count_d || !work_d) return bad("null context, map, labels, count or workspace");
    if (Mx < 1 || My < 1 || Mx > 1024 || My > 1024) return bad("Mx, My must be in 1..1024");
    if (B < 1) return bad("B must be >= 1");
    if ((long long)B * Mx * My > (long long)INT_MAX) return bad("B * Mx * My does not fit an int");
    if (sense != AEFFT_REGIONS_ABOVE && sense != AEFFT_REGIONS_BELOW) return bad("sense must be AEFFT_REGIONS_ABOVE or AEFFT_REGIONS_BELOW");
    if (connectivity != 4 && connectivity != 8) return bad("connectivity must be 4 or 8");
    if (!std::isfinite(lo) || !std::isfinite(hi)) return bad("lo and hi must be finite");
    if (sense == AEFFT_REGIONS_ABOVE ? lo > hi : hi > lo) return bad("lo and hi in the wrong order: AEFFT_REGIONS_ABOVE needs lo <= hi, AEFFT_REGIONS_BELOW hi <= lo");
    if (min_area < 1) return bad("min_area must be >= 1");
    if (max_regions < 0 || max_regions > 65536) return bad("max_regions must be in 0..65536");
    if ((regions_d == nullptr) != (max_regions == 0)) return bad("regions_d must be NULL exactly when max_regions == 0");
    if (!aligned16(map_d) || !aligned16(ref_d) || !aligned16(labels_d) || !aligned16(regions_d) || !aligned16(count_d) || !aligned16(work_d))
        return bad("map_d, ref_d, labels_d, regions_d, count_d and work_d must be 16-byte aligned");
    const size_t need = map_regions_workspace(Mx, My, B);
    if (work_bytes < need) return bad("work_bytes is below aefft_map_regions_workspace(Mx, My, B)");
    const size_t cells = (size_t)Mx * My, mb = (size_t)B * cells * 4;
    // the outputs and the workspace against the inputs and one another (a null pointer has no range)
    struct Range { const void* p; size_t n; bool out; };
    const Range r[6] = {{map_d, mb, false}, {ref_d, ref_d ? cells * 4 : 0, false}, {labels_d, mb, true},
                        {regions_d, (size_t)B * max_regions * sizeof(aefft_region), true}, {count_d, (size_t)B * 4, true}, {work_d, need, true}};
    for (int i = 0; i < 6; ++i)
        for (int j = i + 1; j < 6; ++j)
            if ((r[i].out || r[j].out) && r[i].n && r[j].n && ranges_overlap(r[i].p, r[i].n, r[j].p, r[j].n))
                return bad("the labels, regions, count and workspace ranges overlap an input or each other");
    RET_IF(join_recon(ctx));                          // (the map may come out of a reconstruction that is still on the side stream)
    return launch_or_fail(ctx, KID_IMAGE, (double)B * cells * 24.0 + 32.0 * B * max_regions, "map_regions", [&] {
        return launch_map_regions(map_d, ref_d, Mx, My, B, sense, lo, hi, connectivity, min_area, labels_d, regions_d, max_regions, count_d, work_d, ctx->cur);
    });
}

extern "C" int aefft_region_to_pixels(const aefft_region* r, int Mx, int My, int W, int H, int* x0, int* y0, int* x1, int* y1)
{
    if (!r || !x0 || !y0 || !x1 || !y1 || !dim_ok(W) || !dim_ok(H) || Mx < 1 || My < 1 || Mx > 1024 || My > 1024 || Mx > W || My > H) return AEFFT_EINVAL;
    if (r->i0 < 0 || r->i0 > r->i1 || r->i1 >= Mx || r->j0 < 0 || r->j0 > r->j1 || r->j1 >= My) return AEFFT_EINVAL;
    *x0 = (r->i0 * W + Mx - 1) / Mx; *x1 = ((r->i1 + 1) * W + Mx - 1) / Mx;      // ((i1 + 1) W <= 2^23)
    *y0 = (r->j0 * H + My - 1) / My; *y1 = ((r->j1 + 1) * H + My - 1) / My;
    return AEFFT_OK;
}

// align and rectify (include/aefft.h "aefft_image_warp_affine, aefft_image_remap") ---------------
extern "C" int aefft_affine_make(const double m[6], aefft_affine* out)
{
    if (!m || !out) return AEFFT_EINVAL;
    aefft_affine q;
    for (int k = 0; k < 6; ++k) {
        const double limit = k % 3 == 2 ? 549755813888.0 : 536870912.0;           // 2^39 for the offsets, 2^29 for the others
        if (!std::isfinite(m[k])) return AEFFT_EINVAL;
        const double a = std::nearbyint(m[k] * 16777216.0);                        // (the product is exact; to nearest, ties to even)
        if (std::fabs(a) > limit) return AEFFT_EINVAL;
        q.a[k] = (long long)a;
    }
    *out = q;
    return AEFFT_OK;
}

// the rules the two calls share: both images by the image buffer rule, each sentence led by the image's name, and the destination clear of the
// source; `de` receives the destination's extent
static int chk_warp(const Bad& bad, const void* src_d, size_t src_pitch, size_t src_stride, int Ws, int Hs, int interp, int border, const void* dst_d,
                    size_t dst_pitch, size_t dst_stride, int Wd, int Hd, int B, int D, size_t* de)
{
    RET_IF(chk_dims(bad, B, D, Ws, Hs, "Ws, Hs, Wd, Hd", dim_ok(Wd) && dim_ok(Hd)));
    if (interp != AEFFT_WARP_NEAREST && interp != AEFFT_WARP_LINEAR) return bad("interp must be AEFFT_WARP_NEAREST or AEFFT_WARP_LINEAR");
    if (border != AEFFT_BORDER_CONSTANT && border != AEFFT_BORDER_REPLICATE && border != AEFFT_BORDER_REFLECT)
        return bad("border must be AEFFT_BORDER_CONSTANT, AEFFT_BORDER_REPLICATE or AEFFT_BORDER_REFLECT");
    size_t se = 0;
    const std::string src_name = std::string(bad.fn) + ": src_d", dst_name = std::string(bad.fn) + ": dst_d";
    RET_IF(chk_rows(Bad{bad.ctx, src_name.c_str()}, IMAGE_WORDS, src_pitch, src_stride, (size_t)Ws * D, (size_t)Hs, B, &se));
    RET_IF(chk_rows(Bad{bad.ctx, dst_name.c_str()}, IMAGE_WORDS, dst_pitch, dst_stride, (size_t)Wd * D, (size_t)Hd, B, de));
    if (ranges_overlap(src_d, se, dst_d, *de)) return bad("the source and destination ranges overlap (the op is out-of-place)");
    return AEFFT_OK;
}

extern "C" int aefft_image_warp_affine(aefft_ctx* ctx, const unsigned char* src_d, size_t src_pitch, size_t src_stride, int Ws, int Hs, const aefft_affine* m_d, int nm,
                                       int interp, int border, unsigned border_value, unsigned char* dst_d, size_t dst_pitch, size_t dst_stride, int Wd, int Hd,
                                       int B, int D)
{
    const Bad bad{ctx, "aefft_image_warp_affine"};
    if (!ctx || !src_d || !m_d || !dst_d) return bad("null context, source, affines or destination");
    size_t de = 0;
    RET_IF(chk_warp(bad, src_d, src_pitch, src_stride, Ws, Hs, interp, border, dst_d, dst_pitch, dst_stride, Wd, Hd, B, D, &de));
    if (nm != 1 && nm != B) return bad("nm must be 1 (one affine for the batch) or B (one per image)");
    if (!aligned16(m_d)) return bad("m_d must be 16-byte aligned");
    if (ranges_overlap(m_d, (size_t)nm * sizeof(aefft_affine), dst_d, de)) return bad("the affines and the destination range overlap");
    RET_IF(join_recon(ctx));                          // (the source may hold a reconstruction that is still on the side stream)
    return launch_or_fail(ctx, KID_IMAGE, (double)B * D * ((double)Ws * Hs + (double)Wd * Hd) + 48.0 * nm, "image_warp_affine", [&] {
        return launch_image_warp_affine(src_d, src_pitch, src_stride, Ws, Hs, m_d, nm, interp, border, border_value, dst_d, dst_pitch, dst_stride, Wd, Hd, B, D, ctx->cur);
    });
}

extern "C" int aefft_image_remap(aefft_ctx* ctx, const unsigned char* src_d, size_t src_pitch, size_t src_stride, int Ws, int Hs, const int* map_d, int interp,
                                 int border, unsigned border_value, unsigned char* dst_d, size_t dst_pitch, size_t dst_stride, int Wd, int Hd, int B, int D)
{
    const Bad bad{ctx, "aefft_image_remap"};
    if (!ctx || !src_d || !map_d || !dst_d) return bad("null context, source, table or destination");
    size_t de = 0;
    RET_IF(chk_warp(bad, src_d, src_pitch, src_stride, Ws, Hs, interp, border, dst_d, dst_pitch, dst_stride, Wd, Hd, B, D, &de));
    if (!aligned16(map_d)) return bad("map_d must be 16-byte aligned");
    if (ranges_overlap(map_d, (size_t)8 * Wd * Hd, dst_d, de)) return bad("the table and the destination range overlap");
    RET_IF(join_recon(ctx));                          // (the source may hold a reconstruction that is still on the side stream)
    return launch_or_fail(ctx, KID_IMAGE, (double)B * D * ((double)Ws * Hs + (double)Wd * Hd) + 8.0 * Wd * Hd, "image_remap", [&] {
        return launch_image_remap(src_d, src_pitch, src_stride, Ws, Hs, map_d, interp, border, border_value, dst_d, dst_pitch, dst_stride, Wd, Hd, B, D, ctx->cur);
    });
}

// calibration (include/aefft.h "aefft_map_stats_update") ----------------------------------------
extern "C" size_t aefft_map_stats_bytes(int Mx, int My) { return map_stats_bytes(Mx, My); }

// the rules the calibration calls share: the grid, the batch and a state of at least the query's bytes (stats_d null: the call has no state)
static int chk_calib(const Bad& bad, int Mx, int My, int B, const void* stats_d, size_t stats_bytes, const char* stats_names)
{
    if (Mx < 1 || My < 1 || Mx > 1024 || My > 1024) return bad("Mx, My must be in 1..1024");
    if (B < 1) return bad("B must be >= 1");
    if ((long long)B * Mx * My > (long long)INT_MAX) return bad("B * Mx * My does not fit an int");
    if (stats_d && stats_bytes < map_stats_bytes(Mx, My)) return bad(std::string(stats_names) + " is below aefft_map_stats_bytes(Mx, My)");
    return AEFFT_OK;
}
static bool sense_ok(int sense) { return sense == AEFFT_REGIONS_ABOVE || sense == AEFFT_REGIONS_BELOW; }

extern "C" int aefft_map_stats_update(aefft_ctx* ctx, const float* map_d, int Mx, int My, int B, void* stats_d, size_t stats_bytes)
{
    const Bad bad{ctx, "aefft_map_stats_update"};
    if (!ctx || !map_d || !stats_d) return bad("null context, map or state");
    RET_IF(chk_calib(bad, Mx, My, B, stats_d, stats_bytes, "stats_bytes"));
    if (!aligned16(map_d) || !aligned16(stats_d)) return bad("map_d and stats_d must be 16-byte aligned");
    const size_t n = (size_t)Mx * My, need = map_stats_bytes(Mx, My);
    if (ranges_overlap(map_d, (size_t)B * n * 4, stats_d, need)) return bad("the map and state ranges overlap");
    RET_IF(join_recon(ctx));                          // (the map may come out of a reconstruction that is still on the side stream)
    return launch_or_fail(ctx, KID_IMAGE, 4.0 * B * n + 104.0 * n, "map_stats_update", [&] { return launch_map_stats_update(map_d, Mx, My, B, stats_d, ctx->cur); });
}

extern "C" int aefft_map_stats_merge(aefft_ctx* ctx, void* dst_d, const void* src_d, int Mx, int My, size_t stats_bytes)
{
    const Bad bad{ctx, "aefft_map_stats_merge"};
    if (!ctx || !dst_d || !src_d) return bad("null context, dst or src state");
    RET_IF(chk_calib(bad, Mx, My, 1, dst_d, stats_bytes, "stats_bytes"));
    if (!aligned16(dst_d) || !aligned16(src_d)) return bad("dst_d and src_d must be 16-byte aligned");
    const size_t n = (size_t)Mx * My, need = map_stats_bytes(Mx, My);
    if (ranges_overlap(dst_d, need, src_d, need)) return bad("the dst and src state ranges overlap");
    RET_IF(join_recon(ctx));
    return launch_or_fail(ctx, KID_IMAGE, 156.0 * n, "map_stats_merge", [&] { return launch_map_stats_merge(dst_d, src_d, Mx, My, ctx->cur); });
}

extern "C" int aefft_map_stats_finish(aefft_ctx* ctx, const void* stats_d, size_t stats_bytes, int Mx, int My, int mode, int sense, float k, int rank, float empty,
                                      float* ref_d)
{
    const Bad bad{ctx, "aefft_map_stats_finish"};
    if (!ctx || !stats_d || !ref_d) return bad("null context, state or ref");
    RET_IF(chk_calib(bad, Mx, My, 1, stats_d, stats_bytes, "stats_bytes"));
    if (mode != AEFFT_CALIB_SIGMA && mode != AEFFT_CALIB_RANK) return bad("mode must be AEFFT_CALIB_SIGMA or AEFFT_CALIB_RANK");
    if (!sense_ok(sense)) return bad("sense must be AEFFT_REGIONS_ABOVE or AEFFT_REGIONS_BELOW");
    if (rank < 1 || rank > 4) return bad("rank must be in 1..4");
    if (!std::isfinite(k)) return bad("k must be finite");
    if (!aligned16(stats_d) || !aligned16(ref_d)) return bad("stats_d and ref_d must be 16-byte aligned");
    const size_t n = (size_t)Mx * My;
    if (ranges_overlap(stats_d, map_stats_bytes(Mx, My), ref_d, n * 4)) return bad("the state and ref ranges overlap");
    RET_IF(join_recon(ctx));
    return launch_or_fail(ctx, KID_IMAGE, 56.0 * n, "map_stats_finish",
                          [&] { return launch_map_stats_finish(stats_d, Mx, My, mode, sense, k, rank, empty, ref_d, ctx->cur); });
}

extern "C" int aefft_map_peak(aefft_ctx* ctx, const float* map_d, const float* ref_d, int Mx, int My, int B, int sense, float* peak_d, int* cell_d)
{
    const Bad bad{ctx, "aefft_map_peak"};
    if (!ctx || !map_d || !peak_d || !cell_d) return bad("null context, map, peak or cell");
    RET_IF(chk_calib(bad, Mx, My, B, nullptr, 0, ""));
    if (!sense_ok(sense)) return bad("sense must be AEFFT_REGIONS_ABOVE or AEFFT_REGIONS_BELOW");
    if (!aligned16(map_d) || !aligned16(ref_d) || !aligned16(peak_d) || !aligned16(cell_d)) return bad("map_d, ref_d, peak_d and cell_d must be 16-byte aligned");
    const size_t n = (size_t)Mx * My, mb = (size_t)B * n * 4, ob = (size_t)B * 4;
    if (ranges_overlap(peak_d, ob, cell_d, ob) || ranges_overlap(peak_d, ob, map_d, mb) || ranges_overlap(cell_d, ob, map_d, mb) ||
        (ref_d && (ranges_overlap(peak_d, ob, ref_d, n * 4) || ranges_overlap(cell_d, ob, ref_d, n * 4))))
        return bad("the peak and cell ranges overlap an input or each other");
    RET_IF(join_recon(ctx));
    return launch_or_fail(ctx, KID_IMAGE, 4.0 * B * n + (ref_d ? 4.0 * n : 0.0) + 8.0 * B, "map_peak",
                          [&] { return launch_map_peak(map_d, ref_d, Mx, My, B, sense, peak_d, cell_d, ctx->cur); });
}

// raw sensor data (include/aefft.h "aefft_raw_to_image") ----------------------------------------
static const RowWords RAW_WORDS = {"pitch too small: U8 pitch >= W, U16 pitch >= 2 W, PACKED pitch >= ceil(W * bits / 8)", "H * pitch does not fit the address space",
                                   "stride must be at least (H - 1) * pitch + the live bytes of a row for B > 1", "B * stride does not fit the address space"};

extern "C" int aefft_raw_to_image(aefft_ctx* ctx, const aefft_raw_desc* src, int order, unsigned char* image_d, size_t pitch, size_t image_stride, int B)
{
    const Bad bad{ctx, "aefft_raw_to_image"};
    if (!ctx || !src || !src->data || !image_d) return bad("null context, descriptor, data or image");
    if (src->pattern < AEFFT_RAW_RGGB || src->pattern > AEFFT_RAW_MONO) return bad("pattern must be AEFFT_RAW_RGGB, _GRBG, _GBRG, _BGGR or _MONO");
    if (src->container != AEFFT_RAW_U8 && src->container != AEFFT_RAW_U16 && src->container != AEFFT_RAW_PACKED) return bad("container must be AEFFT_RAW_U8, AEFFT_RAW_U16 or AEFFT_RAW_PACKED");
    if (src->method != AEFFT_DEMOSAIC_BILINEAR && src->method != AEFFT_DEMOSAIC_MHC) return bad("method must be AEFFT_DEMOSAIC_BILINEAR or AEFFT_DEMOSAIC_MHC");
    const bool mono = src->pattern == AEFFT_RAW_MONO;
    if (!mono && order != AEFFT_YUV_BGR && order != AEFFT_YUV_RGB) return bad("order must be AEFFT_YUV_BGR or AEFFT_YUV_RGB");
    const int bits = src->bits, D = mono ? 1 : 3;
    if (src->container == AEFFT_RAW_U8 ? bits != 8 : src->container == AEFFT_RAW_U16 ? (bits < 9 || bits > 16) : (bits != 10 && bits != 12))
        return bad("bits must be 8 for AEFFT_RAW_U8, 9..16 for AEFFT_RAW_U16 and 10 or 12 for AEFFT_RAW_PACKED");
    if (B < 1 || src->W < 4 || src->W > 8192 || src->H < 4 || src->H > 8192) return bad("B must be >= 1 and W, H in 4..8192");
    if (src->container == AEFFT_RAW_U16 && ((reinterpret_cast<uintptr_t>(src->data) | src->pitch | (B > 1 ? src->stride : 0)) & 1u))
        return bad("AEFFT_RAW_U16 needs data, pitch and stride to be multiples of 2");
    const size_t W = (size_t)src->W, H = (size_t)src->H;
    const size_t live = src->container == AEFFT_RAW_U8 ? W : src->container == AEFFT_RAW_U16 ? 2 * W : (W * bits + 7) / 8;
    size_t sext = 0, extent = 0;
    RET_IF(chk_rows(bad, RAW_WORDS, src->pitch, src->stride, live, H, B, &sext));
    RET_IF(chk_rows(bad, IMAGE_WORDS, pitch, image_stride, W * D, H, B, &extent));
    if (src->black < 0 || src->black >= src->white || src->white > (1 << bits) - 1) return bad("black and white must satisfy 0 <= black < white <= 2^bits - 1");
    for (int c = 0; c < D; ++c) {
        if (!std::isfinite(src->gain[c]) || src->gain[c] < 0.f || src->gain[c] > 64.f) return bad("every gain must be finite and in 0..64");
        if (raw_multiplier(src->gain[c], src->black, src->white) > 1073741824.0) return bad("gain * 255 * 65536 / (white - black) exceeds 2^30");
    }
    for (int k = 0; k < 9 && !mono && src->ccm; ++k)
        if (!std::isfinite(src->ccm[k]) || std::fabs(src->ccm[k]) >= 4.f) return bad("every ccm entry must be finite and below 4 in magnitude");
    if (ranges_overlap(src->data, sext, image_d, extent)) return bad("the source and image ranges overlap (the op is out-of-place)");
    if (src->lut_d && ranges_overlap(src->lut_d, 4096, image_d, extent)) return bad("the table and image ranges overlap");
    RET_IF(join_recon(ctx));                          // (the source may be a buffer the side stream is still writing)
    return launch_or_fail(ctx, KID_IMAGE, (double)B * (double)H * ((double)live + (double)(W * D)) + (src->lut_d ? 4096.0 : 0.0), "raw_to_image",
                          [&] { return launch_raw_image(*src, order, image_d, pitch, image_stride, B, ctx->cur); });
}

// compare (include/aefft.h "aefft_image_compare_map") -----------------------------------------
extern "C" int aefft_image_compare_map(aefft_ctx* ctx, const unsigned char* a_d, size_t a_pitch, size_t a_stride, const unsigned char* b_d, size_t b_pitch,
                                       size_t b_stride, int W, int H, int B, int D, int metric, int Mx, int My, float* map_d, float* score_d)
{
    const Bad bad{ctx, "aefft_image_compare_map"};
    if (!ctx || !a_d || !b_d || !map_d) return bad("null context, image or map");
    RET_IF(chk_dims(bad, B, D, W, H));
    if (Mx < 1 || My < 1 || Mx > 1024 || My > 1024 || Mx > W || My > H) return bad("Mx must be in 1..min(W, 1024) and My in 1..min(H, 1024)");
    if ((W + Mx - 1) / Mx > 64 || (H + My - 1) / My > 64) return bad("a cell side above 64: ceil(W / Mx) and ceil(H / My) must be at most 64");
    if (metric != AEFFT_COMPARE_MSE && metric != AEFFT_COMPARE_SSIM) return bad("metric must be AEFFT_COMPARE_MSE or AEFFT_COMPARE_SSIM");
    size_t ea = 0, eb = 0;                            // each image by the image buffer rule, the sentence led by the image's name
    RET_IF(chk_rows(Bad{ctx, "aefft_image_compare_map: a_d"}, IMAGE_WORDS, a_pitch, a_stride, (size_t)W * D, (size_t)H, B, &ea));
    RET_IF(chk_rows(Bad{ctx, "aefft_image_compare_map: b_d"}, IMAGE_WORDS, b_pitch, b_stride, (size_t)W * D, (size_t)H, B, &eb));
    if (!aligned16(map_d) || !aligned16(score_d)) return bad("map_d and score_d must be 16-byte aligned");
    if ((size_t)B > HALF / ((size_t)4 * Mx * My) || (size_t)B * My > (size_t)INT_MAX) return bad("B * Mx * My does not fit the address space or B * My an int");
    const size_t mb = (size_t)B * Mx * My * 4, sb = (size_t)B * 4;
    if (ranges_overlap(map_d, mb, a_d, ea) || ranges_overlap(map_d, mb, b_d, eb)) return bad("the map and image ranges overlap");
    if (score_d && (ranges_overlap(score_d, sb, a_d, ea) || ranges_overlap(score_d, sb, b_d, eb))) return bad("the score and image ranges overlap");
    if (score_d && ranges_overlap(score_d, sb, map_d, mb)) return bad("the score and map ranges overlap");
    RET_IF(join_recon(ctx));                          // (either image may hold a reconstruction that is still on the side stream)
    RET_IF(launch_or_fail(ctx, KID_IMAGE, (double)B * (2.0 * W * H * D + 4.0 * Mx * My), "compare_map",
                          [&] { return launch_compare_map(a_d, a_pitch, a_stride, b_d, b_pitch, b_stride, W, H, B, D, metric, Mx, My, map_d, ctx->cur); }));
    if (!score_d) return AEFFT_OK;                    // (the finish reads the map the launch before it wrote: its bytes are accounted there)
    return launch_or_fail(ctx, KID_IMAGE, 0.0, "compare_score", [&] { return launch_compare_score(map_d, score_d, W, H, B, Mx, My, ctx->cur); });
}

// tiled inference (include/aefft.h "tiled inference"): the plan is host arithmetic only --------
extern "C" int aefft_tile_plan_make(const aefft_tile_desc* desc, aefft_tile_plan* plan) { return tile_plan(desc, plan) ? AEFFT_OK : AEFFT_EINVAL; }

// the rules aefft_image_tiles_to_frames and aefft_frames_tiles_to_image share; `frame_bytes` receives the bytes of the T tile frames
static int chk_tiles(const Bad& bad, const void* image_d, size_t pitch, size_t image_stride, const aefft_tile_desc* desc, const void* frames_d, int frames_u8, int B, int D, size_t* frame_bytes)
{
    if (!bad.ctx || !image_d || !frames_d || !desc) return bad("null context, image, frames or description");
    aefft_tile_plan plan;
    if (!tile_plan(desc, &plan)) return bad("the description is not one aefft_tile_plan_make takes (W, H in 1..8192; Nx, Ny in 2..2048; 0 <= 2 overlap <= N; 0 <= 2 rim <= overlap)");
    size_t extent = 0;
    RET_IF(chk_present_image(bad, pitch, image_stride, desc->W, desc->H, B, D, &extent));
    const size_t T = (size_t)B * plan.ntx * plan.nty;                            // (at most 2^26 tiles of an image, at most 2^26 bytes of a tile)
    RET_IF(chk_frames_aligned16(bad, frames_d, "frames_d", "T", T, D, desc->Nx, desc->Ny, frames_u8, frame_bytes, "B * ntx * nty tiles do not fit an int"));
    if (ranges_overlap(frames_d, *frame_bytes, image_d, extent)) return bad("the frame and image ranges overlap (the op is out-of-place)");
    return AEFFT_OK;
}

extern "C" int aefft_image_tiles_to_frames(aefft_ctx* ctx, const unsigned char* image_d, size_t pitch, size_t image_stride, const aefft_tile_desc* desc,
                                           void* frames_d, int frames_u8, int B, int D)
{
    size_t fb = 0;
    RET_IF(chk_tiles(Bad{ctx, "aefft_image_tiles_to_frames"}, image_d, pitch, image_stride, desc, frames_d, frames_u8, B, D, &fb));
    RET_IF(join_recon(ctx));                          // (frames_d may be a buffer a deferred reconstruction is still writing)
    return launch_or_fail(ctx, KID_IMAGE, (double)B * D * desc->W * desc->H + (double)fb, "tile_gather",
                          [&] { return launch_tile_gather(image_d, pitch, image_stride, desc, frames_d, !frames_u8, B, D, ctx->cur); });
}

extern "C" int aefft_frames_tiles_to_image(aefft_ctx* ctx, const void* frames_d, int frames_u8, const aefft_tile_desc* desc, unsigned char* image_d,
                                           size_t pitch, size_t image_stride, int B, int D)
{
    size_t fb = 0;
    RET_IF(chk_tiles(Bad{ctx, "aefft_frames_tiles_to_image"}, image_d, pitch, image_stride, desc, frames_d, frames_u8, B, D, &fb));
    RET_IF(join_recon(ctx));                          // (frames_d may be the reconstruction of a step whose inverse transform is still on the side stream)
    return launch_or_fail(ctx, KID_IMAGE, (double)B * D * desc->W * desc->H + (double)fb, "tile_blend",
                          [&] { return launch_tile_blend(frames_d, !frames_u8, desc, image_d, pitch, image_stride, B, D, ctx->cur); });
}
