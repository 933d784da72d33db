// Internal launch interface between the HIP kernel files and the C-ABI layer (aefft_capi.hip, ops.hip, image_ops.hip, net.hip, net_forward.hip, net_score.hip, net_step.hip).
// Nothing here is exported; the public boundary is include/aefft.h and the three C++ headers.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/aefft.h"

namespace aefft {

// Development switches (include/aefft.h AEFFT_F_*, aefft_ctx_set_flags): one process-wide word, written by the setter (and once
// from the AEFFT_FLAGS environment variable when the first context is created), read by the launchers.  No getenv afterwards.
extern unsigned dev_flags;
inline bool flag(unsigned f) { return (dev_flags & f) != 0; }

// ---- fft_kernels.hip -------------------------------------------------------------------
// Twiddle table W[k] = exp(-2*pi*i*k/TW_N), uploaded once per device.
constexpr int TW_N = 4096;
hipError_t upload_twiddles(hipStream_t st);
bool fft_size_supported(int n);

// Batched 2-D R2C with optional fused spectral crop (== fft.cu:764 `fft` followed by
// fft.cu:87 `resize` down-sampling to Nxs x Nys).  in [planes][Nx][Ny] real ->
// out [planes][Nxs][Nys/2+1] complex.  `mid` is a workspace of planes*Nx*(Nys/2) complex.
// in_u8: `in` holds 8-bit pixels instead of floats (the row pass converts on load).
hipError_t launch_r2c(const void* in, float2* out, float2* mid, long planes, int Nx, int Ny,
                      int Nxs, int Nys, hipStream_t st, hipEvent_t done = nullptr /* recorded by the column pass's own completion signal */, bool in_u8 = false);
// Batched 2-D C2R with optional fused spectral zero-pad (== `resize` up-sampling from
// Nxi x Nyi, then cufftExecC2R, then * scale).  in [planes][Nxi][Nyi/2+1] -> out [planes][Nx][Ny].
// opin (nullable): the input spectra are not stored but evaluated from an operator (inv_cols_kernel, mix_inv_cols_kernel): plane (b, d) at bin t is
// A[OPIN_COLS-1][d][t] + sum_{j<D0} A[j][d][t] * Xf[b][j][u(t)], A [OPIN_COLS][D0][Nxi*(Nyi/2+1)], Xf [B][D0][Nx0*(Ny0/2+1)]
constexpr int OPIN_COLS = 4;
constexpr int OPMSE_PACKED_STEPS = 16;  // steps of the innermost pair's two stages in the post-update MSE (opmse_packed)
constexpr int CH_MAXSTEPS = 40;       // most steps of a per-bin chain item (chain_geometry's table; cfg5: 26)
constexpr int CH_VMAX = 128;          // most rows of a matrix the packed-record kernels (chain, innermost-pair MSE) take
struct OpIn { const float2* A; const float2* Xf; int D0, Nx0, Ny0; };
// out_u8: `out` is unsigned char [planes][Nx][Ny]: the row pass writes 8-bit pixels by SpinToImage_C's rule (netlib.cpp:66-68)
// score (nullable; aefft_net_score): the row pass compares the rows it holds with the frames instead of only storing them -- frames [planes][Nx][Ny]
// float, or unsigned char when u8; part [planes*Nx/2] receives one float per ROW PAIR, the sum of (x - r)^2 over the pair's 2 Ny pixels with r the
// rounded product the float row pass stores.  `out` (float, not out_u8) is then optional: non-null, it receives r as without `score`.
// tile (0: none; 8, 16, 32 or 64, dividing Nx and Ny; aefft_net_score_map): the row pass stops its reduction at a STRIP -- two rows x tile
// columns of one channel -- and strips [planes*Nx/2][Ny/tile] receives one float per strip; `part` is then not written.
// ssim (with a tile; aefft_net_ssim_map): FIVE floats per strip instead of one -- the sums of x', r', x'^2, r'^2, x'r' over the strip, x' = x - pivot,
// r' = r - pivot -- and strips is [SSIM_MOMENTS][planes*Nx/2][Ny/tile], one plane per moment.
// `frames` is whatever the reconstruction is compared with: the frames the net read, or a target of the same shape (the _target calls).
struct ScoreArg { const void* frames; bool u8; float* part; int tile = 0; float* strips = nullptr; bool ssim = false; float pivot = 0.f; };
constexpr int SSIM_MOMENTS = 5;
inline int score_tile_log2(int tile) { return tile == 8 ? 3 : tile == 16 ? 4 : tile == 32 ? 5 : tile == 64 ? 6 : -1; }
hipError_t launch_c2r(const float2* in, void* out, float2* mid, long planes, int Nxi, int Nyi,
                      int Nx, int Ny, float scale, hipStream_t st, const OpIn* opin = nullptr, bool out_u8 = false, const ScoreArg* score = nullptr);
// The same partials from a STORED float reconstruction (routes whose reconstruction does not come out of one of the two row kernels): a frame's
// `rows` rows of n floats are taken two at a time (an odd last row alone), part [B][(rows+1)/2]
hipError_t launch_score_diff(const void* frames, bool u8, const float* recon, float* part, int B, long rows, int n, hipStream_t st);
// score[b] = scale * (part[b][0] + part[b][1] + ...), npf partials per frame, summed in double in a fixed order
hipError_t launch_score_finish(const float* part, float* score, int B, long npf, double scale, hipStream_t st);
// ---- score_map_kernels.hip (aefft_net_score_map) ----
// The strips of launch_c2r's ScoreArg from a STORED float reconstruction: npairs row pairs of 2 x n floats, strips [npairs][n/tile]
hipError_t launch_score_map_diff(const void* frames, bool u8, const float* recon, float* strips, long npairs, int n, int tile, hipStream_t st);
// map[b][I][J] = sum over d < D and the tile/2 row pairs of tile row I of strips[((b D + d) Nx/2 + I tile/2 + p)][J], in double, / (D tile tile)
hipError_t launch_score_map_finish(const float* strips, float* map, int B, int D, int Nx, int Ny, int tile, hipStream_t st);
// ---- ssim_kernels.hip (aefft_net_ssim_map) ----
// The five strip sums of launch_c2r's ScoreArg (ssim) from a STORED float reconstruction: strips [SSIM_MOMENTS][npairs][n/tile]
hipError_t launch_ssim_diff(const void* ref, bool u8, const float* recon, float* strips, long npairs, int n, int tile, float pivot, hipStream_t st);
// map[b][I][J] = mean over d < D of the window's SSIM, from its tile/2 strips of each moment added in double (ssim_kernels.hip ssim_finish_kernel)
hipError_t launch_ssim_finish(const float* strips, float* map, int B, int D, int Nx, int Ny, int tile, float data_range, float pivot, hipStream_t st);
// ---- image_kernels.hip (aefft_image_to_frames / aefft_frames_to_image) ----
// ImageToSpin_C / SpinToImage_C for a batch: image = B images of Ny rows of `pitch` bytes, pixel (row j, column i) channel d at j pitch + i D + d;
// frames [B][D][Nx][Ny], float when f32, unsigned char otherwise: frames[b][d][i][j] = image[b][j][i][d] (float frames -> pixels by px_u8).
// D in 1..4, Nx, Ny in 1..8192, pitch >= Nx D (hipErrorInvalidValue otherwise); any alignment of image and pitch, frames 16-byte aligned.
hipError_t launch_image_unpack(const unsigned char* image, size_t pitch, void* frames, bool f32, int B, int D, int Nx, int Ny, hipStream_t st);
hipError_t launch_image_pack(const void* frames, bool f32, unsigned char* image, size_t pitch, int B, int D, int Nx, int Ny, hipStream_t st);
// ---- resize_kernels.hip (aefft_image_resize_to_frames) ----
// B images of H rows of `pitch` bytes, image b at b * stride, W x H interleaved pixels of D channels -> frames [B][D][Nx][Ny] (float when f32): the bilinear
// (mode 0) or box-average (mode 1, Nx <= W and Ny <= H) resize and ImageToSpin_C's transposition in one launch, all-integer (include/aefft.h).
// D in 1..4, W, H, Nx, Ny in 1..8192, pitch >= W D (hipErrorInvalidValue otherwise); any alignment of image, pitch and stride, frames 16-byte aligned.
hipError_t launch_image_resize(const unsigned char* image, size_t pitch, size_t stride, int W, int H, int mode, void* frames, bool f32,
                               int B, int D, int Nx, int Ny, hipStream_t st);
// ---- present_kernels.hip (aefft_frames_resize_to_image, aefft_map_overlay_image) ----
// frames [B][D][Nx][Ny] (float when f32, through px_u8) -> B images of H rows of `pitch` bytes, image b at b * stride, W x H interleaved pixels: the same
// two resizes with the roles swapped (mode 1: W <= Nx and H <= Ny) and SpinToImage_C's transposition in one launch.  Shape rules as above.
hipError_t launch_frames_resize(const void* frames, bool f32, int Nx, int Ny, int mode, unsigned char* image, size_t pitch, size_t stride,
                                int W, int H, int B, int D, hipStream_t st);
// map [B][Mx][My] (Mx, My in 1..1024) -> k0 = px_u8((m - lo) * inv) -> bilinear (smooth) or per-tile index k -> lut[k][d] blended IN PLACE onto the
// images with weight alpha / 256 (alpha in 0..256); lut: 256 * D bytes of any alignment.
hipError_t launch_map_overlay(const float* map, int Mx, int My, float lo, float inv, int smooth, const unsigned char* lut, int alpha,
                              unsigned char* image, size_t pitch, size_t stride, int W, int H, int B, int D, hipStream_t st);
// ---- degrade_kernels.hip (aefft_frames_degrade) ----
// frames [B][D][Nx][Ny] -> frames of the same shape (float when the side's f32 is set; a float source through px_u8): the binomial blur of radius
// `blur` in 0..4, the Irwin-Hall noise of standard deviation sigma and the impulses of probability `impulse`, keyed by (seed, first_frame + b),
// all-integer behind the two quantisations of dg_quantise (include/aefft.h).  D in 1..4, Nx, Ny in 1..8192, sigma in 0..255, impulse in 0..1
// (hipErrorInvalidValue otherwise); both sides 16-byte aligned; dst == src only with blur == 0 and the same element type.
hipError_t launch_degrade(const void* src, bool src_f32, void* dst, bool dst_f32, int B, int D, int Nx, int Ny, int blur, float sigma, float impulse,
                          unsigned long long seed, unsigned long long first_frame, hipStream_t st);
// ---- yuv_kernels.hip (aefft_yuv_to_image, aefft_yuv_resize_to_frames) ----
// B video images of W x H luma samples, format 0 NV12 / 1 I420 / 2 YUYV in up to three planes (plane k of image b at plane[k] + b * stride[k]) -> the
// integer colour conversion of include/aefft.h (matrix 0 BT601 / 1 BT709 / 2 JPEG; order 0 BGR / 1 RGB / 2 GRAY, D = 3, 3, 1) -> B interleaved images
// (launch_yuv_image: layout as launch_frames_resize's destination), or the resize of launch_image_resize applied to those pixels -> frames
// [B][D][Nx][Ny] (launch_yuv_resize), one launch each, no intermediate image.  W, H, Nx, Ny in 1..8192, YUYV: W even; any alignment of planes,
// pitches and strides, frames 16-byte aligned (hipErrorInvalidValue for what the kernels cannot serve; the C entry points check the rest).
hipError_t launch_yuv_image(int fmt, const unsigned char* const* plane, const size_t* pitch, const size_t* stride, int W, int H, int matrix, int order,
                            unsigned char* image, size_t ipitch, size_t istride, int B, hipStream_t st);
hipError_t launch_yuv_resize(int fmt, const unsigned char* const* plane, const size_t* pitch, const size_t* stride, int W, int H, int matrix, int order,
                             int mode, void* frames, bool f32, int B, int Nx, int Ny, hipStream_t st);
// ---- yuv_out_kernels.hip (aefft_image_to_yuv, aefft_frames_resize_to_yuv) ----
// the way back: B interleaved images of W x H pixels (layout as launch_image_resize's source; order 0 BGR / 1 RGB / 2 GRAY, D = 3, 3, 1), or frames
// [B][D][Nx][Ny] resized to W x H as launch_frames_resize does it, -> the integer conversion of include/aefft.h (matrix 0 BT601 / 1 BT709 / 2 JPEG,
// chroma the rounded box average of its live pixels) -> every plane of format 0 NV12 / 1 I420 / 2 YUYV (plane k of image b at plane[k] + b * stride[k]),
// one launch each, no intermediate image.  W, H, Nx, Ny in 1..8192, YUYV: W even; any alignment of image, planes, pitches and strides, frames
// 16-byte aligned (hipErrorInvalidValue for what the kernels cannot serve; the C entry points check the rest).
hipError_t launch_image_yuv(const unsigned char* image, size_t ipitch, size_t istride, int order, int fmt, unsigned char* const* plane, const size_t* pitch,
                            const size_t* stride, int W, int H, int matrix, int B, hipStream_t st);
hipError_t launch_frames_yuv(const void* frames, bool f32, int Nx, int Ny, int mode, int order, int fmt, unsigned char* const* plane, const size_t* pitch,
                             const size_t* stride, int W, int H, int matrix, int B, hipStream_t st);
// ---- tile_kernels.hip (aefft_tile_plan_make, aefft_image_tiles_to_frames, aefft_frames_tiles_to_image) ----
// the plan of include/aefft.h from a description: false, and nothing written, for a null pointer or a value out of range
bool tile_plan(const aefft_tile_desc* desc, aefft_tile_plan* plan);
// B images of H rows of `pitch` bytes, image b at b * stride, W x H interleaved pixels of D channels <-> the T = B ntx nty overlapping tiles of the plan as
// frames [T][D][Nx][Ny] (float when f32): the gather reflects beyond the image's edge, the blend weighs the one, two or four tiles of a pixel with the
// integer ramps (float frames through px_u8 first).  One launch each.  D in 1..4, pitch >= W D, a description tile_plan takes (hipErrorInvalidValue
// otherwise); any alignment of image, pitch and stride, frames 16-byte aligned.
hipError_t launch_tile_gather(const unsigned char* image, size_t pitch, size_t stride, const aefft_tile_desc* desc, void* frames, bool f32, int B, int D,
                              hipStream_t st);
hipError_t launch_tile_blend(const void* frames, bool f32, const aefft_tile_desc* desc, unsigned char* image, size_t pitch, size_t stride, int B, int D,
                             hipStream_t st);
// ---- compare_kernels.hip (aefft_image_compare_map) ----
// two batches of B interleaved images of W x H pixels of D channels, each with its own pitch and stride and of any alignment -> map [B][Mx][My]: per
// cell (cell I: columns [ceil(I W / Mx), ceil((I+1) W / Mx)), rows alike) the mean squared error (metric 0) or the mean SSIM of the channels
// (metric 1), from integer sums (include/aefft.h).  W, H in 1..8192, D in 1..4, Mx <= min(W, 1024), My <= min(H, 1024), cells of at most 64 x 64
// pixels, pitches >= W D (hipErrorInvalidValue otherwise).  One launch.
hipError_t launch_compare_map(const unsigned char* a, size_t a_pitch, size_t a_stride, const unsigned char* b, size_t b_pitch, size_t b_stride, int W, int H,
                              int B, int D, int metric, int Mx, int My, float* map, hipStream_t st);
// score[b] = the pixel-weighted mean of map[b] as stored, added along J, then along I, in double.  One launch.
hipError_t launch_compare_score(const float* map, float* score, int W, int H, int B, int Mx, int My, hipStream_t st);
// ---- regions_kernels.hip (aefft_map_regions) ----
// map [B][Mx][My] (minus ref [Mx][My] where given) -> labels [B][Mx][My], regions [B][max_regions] (null exactly when max_regions == 0), count [B]:
// hysteresis threshold, connected components, the kept ones numbered in index order (include/aefft.h).  work: map_regions_workspace bytes, 16 a cell.
// Mx, My in 1..1024, B Mx My < 2^31, sense 0 / 1, connectivity 4 / 8, min_area >= 1, max_regions in 0..65536 (hipErrorInvalidValue otherwise).  Six
// launches, integer atomics only, no workgroup waits for another.
size_t map_regions_workspace(int Mx, int My, int B);      // 0 for sizes the launcher does not take
hipError_t launch_map_regions(const float* map, const float* ref, int Mx, int My, int B, int sense, float lo, float hi, int connectivity, int min_area,
                              int* labels, aefft_region* regions, int max_regions, int* count, void* work, hipStream_t st);
// ---- bayer_kernels.hip (aefft_raw_to_image) ----
// B raw images of W x H samples (the descriptor of include/aefft.h: Bayer pattern or MONO, U8 / U16 / PACKED container, black, white, gains, demosaic
// method, colour matrix, table) -> B interleaved 8-bit images of D = 3 channels (order 0 BGR / 1 RGB) or, MONO, D = 1: layout as launch_yuv_image's
// destination.  W, H in 4..8192; any alignment of either side (U16: even); hipErrorInvalidValue for what the kernels cannot serve, the C entry
// point checks the rest.  One launch.  raw_multiplier: the Q16 multiplier m_c of a gain as the launcher quantises it (an integer in a double).
double raw_multiplier(float gain, int black, int white);
hipError_t launch_raw_image(const aefft_raw_desc& d, int order, unsigned char* image, size_t ipitch, size_t istride, int B, hipStream_t st);
// ---- calib_kernels.hip (aefft_map_stats_update / _merge / _finish, aefft_map_peak) ----
// The calibration state of Mx x My cells: map_stats_bytes bytes (52 a cell rounded up to 16; 0 for sizes outside 1..1024), planar -- double S1, S2,
// float hi[4], lo[4], int c --, all-zero bytes when empty (include/aefft.h).  update: the B maps [B][Mx][My] enter the state in ascending b, in place.
// merge: src (only read) enters dst.  finish: ref [Mx][My] from a state, mode 0 SIGMA (mean + k sd in double) / 1 RANK (hi[rank-1], lo[rank-1] under
// sense 1), `empty` for a cell that counted nothing.  peak: the maximal (sense 0) or minimal (sense 1) map - ref (ref nullable) of each image over
// its non-NaN cells and the smallest index that attains it; NaN and -1 for an image of NaN only.  One launch each, no atomics, no workspace.
// Mx, My in 1..1024, B >= 1, B Mx My < 2^31, rank in 1..4 (hipErrorInvalidValue otherwise); the C entry points check the rest.
size_t map_stats_bytes(int Mx, int My);
hipError_t launch_map_stats_update(const float* map, int Mx, int My, int B, void* stats, hipStream_t st);
hipError_t launch_map_stats_merge(void* dst, const void* src, int Mx, int My, hipStream_t st);
hipError_t launch_map_stats_finish(const void* stats, int Mx, int My, int mode, int sense, float k, int rank, float empty, float* ref, hipStream_t st);
hipError_t launch_map_peak(const float* map, const float* ref, int Mx, int My, int B, int sense, float* peak, int* cell, hipStream_t st);
// ---- warp_kernels.hip (aefft_image_warp_affine, aefft_image_remap) ----
// B interleaved 8-bit source images (pitch, stride, Ws x Hs) sampled into B destination images (their own pitch, stride, Wd x Hd) at the source
// position (tx, ty) / 2048 of every destination pixel (include/aefft.h): from nm (1 or B) Q24 affines on the device, or from the table
// int [Hd][Wd][2] the batch shares.  interp 0 NEAREST / 1 LINEAR, border 0 CONSTANT (bval: channel d's byte at bits 8 d) / 1 REPLICATE / 2 REFLECT.
// One launch each, no atomics, no workspace.  D in 1..4, sizes in 1..8192, B >= 1, the pitches at least a row (hipErrorInvalidValue otherwise);
// the C entry points check the rest.
hipError_t launch_image_warp_affine(const unsigned char* src, size_t spitch, size_t sstride, int Ws, int Hs, const aefft_affine* m, int nm, int interp, int border,
                                    unsigned bval, unsigned char* dst, size_t dpitch, size_t dstride, int Wd, int Hd, int B, int D, hipStream_t st);
hipError_t launch_image_remap(const unsigned char* src, size_t spitch, size_t sstride, int Ws, int Hs, const int* map, int interp, int border, unsigned bval,
                              unsigned char* dst, size_t dpitch, size_t dstride, int Wd, int Hd, int B, int D, hipStream_t st);
// ---- register_kernels.hip (aefft_frames_register, aefft_frames_register_ref) ----
// The kernels around the two transforms of the phase correlation (include/aefft.h).  prepare: planes [B][Nx][Ny] = window times the channel sum of
// the frames [B][D][Nx][Ny] (8-bit or float), window 0 HANN / 1 NOWINDOW.  cross: spec [B][Nx][Ny/2+1] becomes the normalised cross-power with ref
// (nref 1 or B spectra) over the bins with |u| <= umax, |v| <= vmax and not (|u| <= low and |v| <= low), 0 elsewhere, in place.  peak: two launches,
// register_parts partials an image into `part`, then the shift of each surface [B][Nx][Ny] and, with `affine` non-null, its affine.
// register_workspace: the bytes of planes | spectra | partials, each rounded up to 16, with the offsets of the last two; 0 for sizes that are no
// power of two in 8..2048 or even smooth size in 10..2048, B < 1 or B Nx Ny >= 2^29.  register_kept: the kept bins K of the full spectrum and the
// three index limits; -1 for a cutoff outside (0, 1].  No atomics; D in 1..4 (hipErrorInvalidValue otherwise); the C entry points check the rest.
size_t register_workspace(int Nx, int Ny, int B, size_t* spec_at = nullptr, size_t* part_at = nullptr);
long long register_kept(int Nx, int Ny, int window, float cutoff, int* umax, int* vmax, int* low);
hipError_t launch_register_prepare(const void* frames, int frames_u8, float* planes, int B, int D, int Nx, int Ny, int window, hipStream_t st);
hipError_t launch_register_cross(float2* spec, const float2* ref, int nref, int B, int Nx, int Ny, int window, int umax, int vmax, int low, hipStream_t st);
hipError_t launch_register_peak(const float* surf, void* part, int B, int Nx, int Ny, float min_response, double scale_x, double scale_y, aefft_shift* shift,
                                aefft_affine* affine, hipStream_t st);
size_t fft_mid_elems(long planes, int Nx, int Wc);   // complex elements needed in `mid`
// sizes that are not powers of two (cufftPlanMany takes any size, fft.cu:773-779): even n in 8..1024 through Bluestein's chirp-z form on the
// power-of-two LDS passes; rows -> transpose -> rows -> transpose.  w1, w2: workspaces of fft_any_ws_elems complex each.
bool fft_size_supported_any(int n);
size_t fft_any_ws_elems(long planes, int Nx, int Ny);
hipError_t launch_r2c_any(const float* in, float2* out, float2* w1, float2* w2, long planes, int Nx, int Ny, hipStream_t st);
hipError_t launch_c2r_any(const float2* in, float* out, float2* w1, float2* w2, long planes, int Nx, int Ny, float scale, hipStream_t st);
// ---- fft_mixed_kernels.hip -------------------------------------------------------------
// Mixed-radix (2, 3, 4, 5, 8) passes for sizes with no prime factor above 5.  launch_r2c / launch_c2r pick them per axis: an axis whose
// size is not a power of two (or whose packed width Wc the power-of-two pass cannot tile) takes the mixed-radix pass, the other axis keeps
// its power-of-two pass; `mid` and the crop / zero-pad contract are the same.
bool fft_size_mixed(int n);    // even n in 8..2048 whose prime factors are 2, 3, 5 (powers of two included)
bool fft_size_smooth(int n);   // ... in 10..2048 and not a power of two: the sizes only the mixed-radix passes serve
hipError_t fft_mixed_prepare(int n);     // builds the n-point twiddle table of the current device (done on first use otherwise)
hipError_t launch_mix_r2c_rows(const void* in, float2* mid, long npairs, int Ny, int Wc, hipStream_t st, bool in_u8);
hipError_t launch_mix_fwd_cols(const float2* mid, float2* out, long planes, int Nx, int Wc, int Nxs, hipStream_t st, hipEvent_t done);
hipError_t launch_mix_inv_cols(const float2* in, float2* mid, long planes, int Nx, int Wc, int Nxi, hipStream_t st,
                               const OpIn* opin = nullptr /* the spectra evaluated on load from an operator (launch_c2r); then in == null */);
hipError_t launch_mix_c2r_rows(const float2* mid, void* out, long npairs, int Ny, int Wc, float scale, hipStream_t st, bool out_u8 = false,
                               const ScoreArg* score = nullptr);

// ---- spectral_kernels.hip --------------------------------------------------------------
// Per-bin complex contraction  Out[r][c][bin] = alpha * sum_k opA(A[r][k][bin]) * opB(B[k][c][bin])
// (+ bias[r]*biasScale added to Re at bin 0), the one primitive behind conv_k (fft.cu:162) and
// both halves of gradient_k_io (fft.cu:395).  Strides are in complex elements.
struct Contract {
    const float2* A; long a_r, a_k;     // A[r][k] plane base = A + r*a_r + k*a_k
    const float2* A2;                   // optional: the A operand is (A - A2), same strides (E = O - T fused, fft.cu:417-424)
    const float2* B; long b_k, b_c;     // B[k][c] plane base = B + k*b_k + c*b_c
    float2* Out;     long o_r, o_c;     // Out[r][c] plane base
    int R, C, K;                        // rows, cols, contraction length
    long P;                             // bins per (A / Out) plane
    bool conjA, conjB;
    float preDivB;                      // !=0: B elements are divided by this BEFORE the product (conv_k: in/dM, fft.cu:176-177)
    float postDiv;                      // !=0: the sum is divided by this (gradient_k_io: /Norm, fft.cu:440-441)
    const float* bias; float biasScale; // Re(Out[r][c][0]) += bias[r]*biasScale; null = none
    bool biasAfterFirst;                // true: added right after the k==0 term (fft.cu:183-184); false: after the sum (fft.cu:454)
    int biasColP1;                      // 0: the bias goes to every column c; k+1: to column k only (operator form: the affine column)
    // Virtual spectral up-sampling of the B operand (fft.cu:117-152 fused into the consumer): B planes
    // are [upNxs][upNys/2+1] spectra that are zero-padded on the fly to the [upNx][upNy/2+1] grid of A/Out.
    // Destination bins outside the padded support only receive the bias term (everything else is 0).
    int upNx, upNy, upNxs, upNys;       // upNx == 0: no remap
    // Fused spectral down-sampling of the OUTPUT (fft.cu:98-113): besides Out, every output bin that survives the
    // crop from [dnNx][dnNy/2+1] to [dnNxs][dnNys/2+1] is also written to Out2 (same [r][c] plane order, small planes).
    float2* Out2; int dnNx, dnNy, dnNxs, dnNys;   // Out2 == null: off
    // Small-grid iteration (matrix-core kernel only): P counts the bins of the SMALL grid [gdNxs][gdNys/2+1]; bin s of it
    // corresponds to bin map(s) of the [gdNx][gdNy/2+1] grid (the index map of pool_fft, fft.cu:102-111 / 117-152).
    // gdMask selects which tensors live on the BIG grid and are addressed at map(s): 1 = A (and A2), 2 = B, 4 = Out.
    // Uses: conv_k + down-sampling without the discarded bins (A|B big, Out small); the decoder on the support of the
    // up-sampled spectra (A big); gradient terms of an up-sampled operand (B, Out big).  gdNx == 0: off.
    int gdNx, gdNy, gdNxs, gdNys, gdMask;
    bool accumulate;                    // Out += result (the element is owned by one lane: no race)
    // MSE epilogue instead of a store (mse.acc != null; needs R == K): with A = G[d'][d] = (F.C)/(dM*dD) of one pair and
    // B = X (the pair's input spectra) the tile holds the pair-local reconstruction O_b[d'] = sum_d G[d'][d] X_b[d] + beta[d']
    // at the DC bin (beta = Nx*Ny*(p[d'] + sum_m F[d'][m](0,0) b[m] / dD): the two bias terms of conv_k o conv_k,
    // fft.cu:183-184), and *mse.acc += scale * sum |X_b[d'] - O_b[d']|^2 / n_bin   (mse_fft, fft.cu:480-498,1188-1190).
    // mse.acc -> MSE_SLOTS accumulators, MSE_SLOT_STRIDE floats apart (zero before the first use; launch_mse_finish sums and clears them).
    struct Mse { float* acc; const float2* F; const float* b; const float* p; int dM, Nyr; float nfull, scale, norm; } mse;
};
enum { MSE_SLOTS = 256, MSE_SLOT_STRIDE = 16 };
struct BetaArgs { float* beta; const float2* F; const float *b, *p; int dM, dD; long P; };     // beta == null: off
hipError_t launch_mse_finish(float* slots /*[L][MSE_SLOTS*MSE_SLOT_STRIDE]*/, float* out /*[L], accumulated*/, float* copy /*[L] nullable*/, int L, hipStream_t st,
                             const BetaArgs* beta = nullptr, float* copy2 = nullptr /*[2L] nullable: the tail of the packed gradient buffer -- [l] <- out[l] after [L + l] <- [l] * prev_scale*/,
                             float prev_scale = 1.0f);
struct Contract2 { Contract q[2]; int n; };   // up to two independent contractions in one launch (grid.z is split)
hipError_t launch_contract2(const Contract2& qq, hipStream_t st);
// Up to 8 independent contractions of one class in ONE launch (the four pairs' S / dc,df / re-forward convs):
// cls 0 = plain conv_k, 1 = S (a*conj(b), fused subtraction), 2 = first nA problems conj(a)*b (dc), the rest a*conj(b) (df).
struct ContractN { Contract q[8]; int n, nA; int gx[8], gy[8], gz[8], start[9], ks[8], xmin; };
// matrix-core (MFMA 4x4x1, block = bin) kernel for any mix of classes; hipErrorInvalidValue = not served, use the scalar kernels
hipError_t launch_contract_mfma(ContractN& g, hipStream_t st);
hipError_t launch_contract_group(ContractN& g, int cls, hipStream_t st);
hipError_t launch_contract(const Contract& q, hipStream_t st);

hipError_t launch_resize(const float2* in, float2* out, long planes, int Nx, int Ny, int Nxs, int Nys, hipStream_t st);
hipError_t launch_magnitude(const float2* X, float* mag, long planes, int ch, int Nx, int Ny, int shift, hipStream_t st);   // fft.cu:27-63
// E = O - T and MSE (fft.cu:480-498): *mse_acc += scale * sum_bins |T-O|^2/n_bin.
hipError_t launch_diff_mse(const float2* T, const float2* O, float2* E /*nullable*/, float* mse_acc /*1 float, pre-zeroed, nullable*/,
                           float* es /*[2*ch] floats, pre-zeroed, nullable: sum_b E_b[d](0,0)*/, int B, int ch, int Nx, int Ny, float scale, hipStream_t st);
// db, dp and the DC-bin bias term of df from es[d] = sum_b (O_b[d] - T_b[d])(0,0)  (fft.cu:448-455,463-473)
hipError_t launch_bias_grad(const float2* O, const float2* T, const float2* F, const float* b, float2* df, float* db, float* dp,
                            int B, int dM, int dD, long P, float norm, float Norm, hipStream_t st);

struct BiasGradArgs { const float2 *O, *T, *F; const float* b; float2* df; float *db, *dp; int B, dM, dD; long P; float norm, Norm; long PO; /* plane stride of O (== P unless O is stored on its support only) */
                      float* es_out; /* nullable: [2*dD] floats, es[d] = sum_b (O_b[d] - T_b[d])(0,0) */
                      const float* es_in; /* nullable: es already known (operator form, sgrad_kernel): O and T are not read */ };
struct BiasGradGroup { BiasGradArgs a[8]; int n; int start[9], fix[8]; };
hipError_t launch_bias_grad_group(BiasGradGroup& g, hipStream_t st);

// ---- pruned_kernels.hip ----------------------------------------------------------------
// Kernel-support-pruned transforms: only Nk x Nl taps are non-zero going forward / needed coming back,
// so pad+R2C and C2R+shrink become direct DFT evaluations (fft.cu:1219-1226 and :1274-1282 fused).
// Grids: both axes powers of two (the TW_N-point twiddle table) or smooth (even, 10..2048, no prime factor above 5: an N-point phase table
// per (device, axis size), built on first use or by pruned_prepare), Ny/2+1 <= 320.  pruned_supported: the route is taken (false on a grid
// with a smooth axis under AEFFT_F_NOPRUNESMOOTH); pruned_geometry: the grid has the route at all -- what buffers are sized by, the switch
// may change on a live net; pruned_pow2: neither axis needs a table of its own.
bool pruned_supported(int Nk, int Nl, int Nx, int Ny);
bool pruned_geometry(int Nk, int Nl, int Nx, int Ny);
bool pruned_pow2(int Nx, int Ny);
hipError_t pruned_prepare(int Nx, int Ny);     // the phase tables of the current device for this grid: built here instead of inside a step
hipError_t launch_kspec(const float* k, float2* K, const float2* tw, long planes, int Nx, int Ny, int Nk, int Nl, hipStream_t st);
hipError_t launch_kgrad(const float2* D, float* g, float* part /*workspace: kgrad_partial_floats()*/, const float2* tw, long planes, int Nx, int Ny, int Nk, int Nl, float scale, hipStream_t st);
size_t kgrad_partial_floats(long planes, int Nx, int Ny, int Nk, int Nl);
// The same transforms for up to 8 problems with equal (Nk, Nl) in ONE launch (kgrad: no row chunks, so no ksum pass).
struct PrunedProb { const void* src; void* dst; long planes; int Nx, Ny; float scale;
                    int NxB, NyB; /* forward transform only: the grid the phases are taken on (0: the plane's own); rows / columns of the
                                     [Nx][Ny/2+1] output are then the images of pool_fft's crop in it (map_up_row / map_up_col) */ };
// forward transform only: the problem's planes are G' = F'.C'/(dM dD) [dD][dD] of a pair, their (2Nk-1)^2 taps formed inside the launch from
// c | f (read through the problem's TapUpd); f == null: an ordinary problem (taps at PrunedProb::src)
struct GtapSrc { const float* c; const float* f; int dM, dD; float scale; };
// the taps of G' = F.C / (dM dD) of up to 8 pairs, [dD*dD][(2Nk-1)^2] each, in one launch (HBM-sized grids: every plane is transformed by several
// row-chunk workgroups, which would each form the same taps again -- 238 of the 538 us of the G' launch at cfg3-P1); their spectra are then an
// ordinary pruned transform of (2Nk-1)^2-tap kernels: launch_kspec_group_taps
struct GtapsGroup { GtapSrc gs[8]; float* out[8]; int n; int start[9]; };
hipError_t launch_gtaps_group(GtapsGroup& g, int Nk, hipStream_t st);
struct PrunedGroup;
hipError_t launch_kspec_group_taps(PrunedGroup& g, const float2* tw, int T, hipStream_t st);      // spectra of stored T x T-tap kernels, T = 5 or 9
// forward pruned transform only: the taps are read THROUGH the pending clipped-momentum update (w - clip_step(g*gscale, D)), which
// another launch stores afterwards (update_device.h) -- g == null: taps as stored
struct TapUpd { const float* g; const float* D; float del, alpha, gscale; };
struct BiasUpd { float *b, *p, *Db, *Dp; const float *db, *dp; float* zero; int dM, dD; };
struct BiasUpdGroup { BiasUpd a[8]; int n; float del, alpha, gscale; };      // n == 0: none
struct PrunedGroup {
    PrunedProb q[8]; int n; int start[9], ppb[8], rows[8], pblocks[8];
    TapUpd upd[8];
    GtapSrc gsrc[8];
    // grouped inverse transform only: rows per slice; chunks[p] in: row chunks dst has room for ([planes][chunks][taps], 0/1 = none),
    // out: the chunks the launch used (the consumer adds them in order)
    int rb[8], chunks[8];
};
int kgrad_group_chunks(long planes, int Nx, int Ny);
struct PackArgs;
hipError_t launch_kspec_group(PrunedGroup& g, const float2* tw, int Nk, int Nl, hipStream_t st, PackArgs* packed = nullptr /* the bin-major copy rides along as extra workgroups */,
                              const BiasUpdGroup* bias_upd = nullptr /* the bias half of a fused update as trailing workgroups */);
hipError_t launch_kgrad_group(PrunedGroup& g, const float2* tw, int Nk, int Nl, hipStream_t st);
// the inverse transform on a T x T support with T = 5 or 9 (the offsets kl + k'l' of 3x3 / 5x5 kernels, weight_kernels.hip)
hipError_t launch_kgrad_group_taps(PrunedGroup& g, const float2* tw, int T, hipStream_t st, BiasGradGroup* bias = nullptr /* fused: the DC-bin terms as extra workgroups */);

// ---- weight_kernels.hip ----------------------------------------------------------------
struct WgradProb { const float *c, *f, *Q, *es, *b; float *gc, *gf; int dM, dD; float inv_den, norm; int nq; };   // Q [dD][dD][nq][T*T] (nq row-chunk partial sums, added here), es [2*dD]
struct WgradGroup { WgradProb q[8]; int n; int start[9];
                    // nullable: the slot sums of the PREVIOUS step's post-update MSE (launch_mse_finish deferred by aefft_net_step_apply(mse_d = NULL)) as one trailing workgroup
                    float *fin_slots, *fin_out, *fin_tail; int fin_L; float fin_scale; };
hipError_t launch_wgrad_taps_group(WgradGroup& g, int Nk, hipStream_t st);

const float2* twiddle_table();   // device address of the table uploaded by upload_twiddles()

// ---- opform_kernels.hip ----------------------------------------------------------------
// Operator form of the training step.  The FFT-mode network is linear (identity activation,
// backproplib.cu:38-51; conv_k and pool_fft are linear maps), so every per-frame spectrum of a step is an affine function of
// the frame's own input spectrum x_b (D0 <= 3 channels on pair 0's grid):  X_l,b = A_l [x_b; 1],  O_l,b = O^_l [x_b; 1],
// with per-bin operators A_l [dD_l x OPC] (column j < D0: response to the unit input on channel j, column OPC-1: response
// to the zero input = the bias terms).  The operators come out of the ordinary forward run on OPC "basis frames"; the batch
// enters only through the input transform, the second moments M^[u] = sum_b [x_b;1][x_b;1]^H (OPC x OPC per bin of grid 0)
// and the reconstruction.  Same sums as gradient_k_io / mse_fft (fft_backproplib.cu:395-498), batch contracted first.
constexpr int OPC = 4;
hipError_t launch_basis_fill(float2* A0 /*[OPC][D0][P0]*/, int D0, long P0, hipStream_t st);
struct OpPair {
    const float2* A;        // A_l    [OPC][dD][P]      (the pair's input on the basis frames)
    const float2* O;        // O^_l   [OPC][dD][PO]     (its decoder output on the basis frames, stored on the grid [NxO][NyO/2+1])
    float2* S;              // out:   [dD][dD][P]       S = sum_b (O_b - X_b) X_b^H  (mk_S layout)
    float* es;              // out:   [2*dD]            es[d] = sum_b (O_b - X_b)[d](0,0)
    int dD, Nx, Ny, NxO, NyO; long P, PO;
};
// (msgrad_kernel: the batch moments are formed from the input spectra Xf [B][D0][P0] inside the launch and stored to Mout [OPC*OPC][P0] in their
// CENTRED form -- layout in opform_kernels.hip)
struct SgradGroup { OpPair q[8]; int n; int start[9], bt[8]; const float2* Xf; float2* Mout; int B, D0, Nx0, Ny0; long P0; };
hipError_t launch_msgrad_group(SgradGroup& g, hipStream_t st);
// O_0,b = O^_0 [x_b; 1] on the grid O^_0 is stored on: Of [B][D0][PO]
hipError_t launch_recon_expand(const float2* O0, const float2* Xf, float2* Of, int B, int D0, int Nx0, int Ny0, int NxO, int NyO, hipStream_t st);
// X_l,b = A_l [x_b; 1] for get_layer-style exports: out [B][dD][P] on the grid [Nx][Ny/2+1] of A
hipError_t launch_op_expand(const float2* A, const float2* Xf, float2* out, int B, int D0, int dD, int Nx0, int Ny0, int Nx, int Ny, hipStream_t st);
// H^_l = C_l A_l / dM (+ b_l Nx Ny on the affine column's DC bin): pair l's hidden layer as an operator [OPC][dM][P], from its input
// operator A [OPC][dD][P] and the encoder spectrum C [dM][dD][P] (what conv_k gives on the basis frames); launch_op_expand then gives the frames' planes
hipError_t launch_hidden_op(const float2* C, const float2* A, const float* b, float2* H, int dM, int dD, int Nx, int Ny, hipStream_t st);
// Decode (decode_kernels.hip, aefft_net_decode): the remainder of the network from pair l's hidden layer as one affine operator per bin of
// the coarsest grid, T [D][dM_l + 1][Pc] (last column: every bias below).  One stage per conv_k on the way, in the order the ROW vector
// e_d^T F_0 F_1 .. F_{L-1} C_{L-1} .. C_{l+1} meets them: W [K][M][P] row-major over (in, out) -- F_j [dD][dM], C_j [dM][dD] as stored --
// on the grid Nx x Ny, inv = 1 / (the conv's output channels), bias [K] of the conv, nn = Nx * Ny.
constexpr int DEC_MAX_STAGES = 16;       // 2 L - 1 stages of a net of L <= 8 pairs (the operator forms' limit)
constexpr int DEC_MAX_THREADS = 16384;   // bins in flight: sizes the row workspace ws [2][D][maxW][NT]
constexpr double DEC_WS_BYTES = 16e6;     // ... which stays within this: wide rows take fewer bins in flight (the kernel's threads stride over the bins)
struct DecodeStage { const float2* W; const float* bias; int K, M, Nx, Ny; long P; float inv, nn; };
// maxW, NT: the column stride and thread count ws was ALLOCATED for; Tw: the rows T was allocated for (T [D][Tw][Pc] at least)
struct DecodeOpArgs { DecodeStage st[DEC_MAX_STAGES]; int nst; float2* T; float2* ws; int D, NxC, NyC; long Pc; int NT, maxW, Tw; };
hipError_t launch_decode_op(const DecodeOpArgs& g, hipStream_t st);
// out[b][d][t] = sum_m T[d][m][t] h[b][m][t] + T[d][K][t]: h [B][K][Pc], out [B][D][Pc], D <= 3
hipError_t launch_decode_apply(const float2* T, const float2* h, float2* out, int B, int D, int K, long Pc, hipStream_t st);
struct OpMsePair {
    const float2 *A, *C, *F;   // A_l [OPC][dD][P]; the UPDATED kernel spectra C [dM][dD][P], F [dD][dM][P]
    const float2* G;           // nullable: G' = F.C/(dM dD) [dD][dD][P] of the updated weights -- then C and F are not read (opmse_gbody) ...
    const float2* Fdc; long fdc_stride;   // ... except F at the DC bin: element (a, m) at Fdc[(a*dM + m) * fdc_stride]
    const float *b, *p;        // updated biases
    float* slots;              // MSE_SLOTS accumulators (launch_mse_finish sums them)
    int dD, dM, Nx, Ny; long P;
    float scale;               // 1 / (2 dM Nx Ny B) / (dD Nx Ny)
};
struct OpMseGroup { OpMsePair q[8]; int n; int start[9], bt[8], base; const float2* Mhat; int Nx0, Ny0; long P0;
                    const float2* Wp; int E, offC, offF; /* nullable: bin-major record of the UPDATED spectra; offsets of the innermost pair's C, F in it */
                    unsigned pst_off[OPMSE_PACKED_STEPS], pst_desc[OPMSE_PACKED_STEPS]; int pst_n; /* (filled by the launcher) that pair's two stages as a step list */ };
struct ChainArgs;
struct UpdateGroup;
// the MSE of every pair; optionally in the same launch: the operator chain of the NEXT step (chain, reading the just-written Wp / Cc, writing its own
// operator buffers) and the tap half of a fused update (weights_upd) -- tail_kernel
// route (nullable, out): which step code the launch's chain items and packed MSE run -- AEFFT_TAIL_STATIC when the net's step lists equal one of the
// compile-time tables (opform_kernels.hip ChainTable), AEFFT_TAIL_GENERIC otherwise and under AEFFT_F_NOSTATICCHAIN
hipError_t launch_opmse_group(OpMseGroup& g, hipStream_t st, ChainArgs* chain = nullptr, const UpdateGroup* weights_upd = nullptr, int* route = nullptr);
// the network on the basis frames in one launch (chain_kernel): per pair the spectra, biases and the operator outputs
struct ChainLevel { const float2 *C, *F; const float *b, *p; float2 *A /*[OPC][dD][P]*/, *O /*[OPC][dD][Pc]*/; int dD, dM, Nx, Ny; long P;
                    const float2* Cc; /* nullable: C sampled at the bins the NEXT level's grid lands on, [dM][dD][P of the next level] (then C is not read) */ };
struct ChainArgs {
    ChainLevel lv[8]; int L, D0;
    long Pc;
    const float2* Wp; int E;   // bin-major copy of every matrix a coarsest-grid bin needs (kspec_packed_kernel)
    int tile_start[9];         // (filled by launch_chain) first workgroup of the planar tiles of grid j
    int vt_elems;              // (filled by launch_chain) elements of one V tile of the planar part
    int tile_bt[8];            // (filled by launch_chain) bins per planar tile of grid j (8, 16 or 32)
    // (filled by launch_chain) the per-bin item's step list (chain_item_pipelined, opform_kernels.hip)
    unsigned st_off[CH_MAXSTEPS], st_desc[CH_MAXSTEPS]; int st_n;
};
hipError_t launch_chain(ChainArgs& g, hipStream_t st, hipEvent_t done = nullptr /* recorded by the dispatch itself */);
// Wp[t][E]: per bin t of the coarsest grid the elements of C_0 .. C_{L-1}, F_{L-1} .. F_0 at the bins t maps to, from the taps
struct PackSeg { const float* k; int n, lev, off; const float *g, *D; };   // taps [n][Nk*Nk] of one tensor, its pair, its element offset in a record; gradient / momentum of the same taps (TapUpd)
struct PackArgs { PackSeg seg[16]; int nseg, L, E, Nk; int Nx[8], Ny[8]; int NxC, NyC; long Pc; float2* Wp; const float2* tw;
                  unsigned char blk_seg[128]; int blk_start[128]; int nblk; /* (pack_blocks) element blocks: tensor, first element */
                  int upd; float upd_del, upd_alpha, upd_gscale; /* upd != 0: taps read through the pending update (TapUpd) */ };
void pack_blocks(PackArgs& g);
hipError_t launch_kspec_packed(PackArgs& g, hipStream_t st);
// (pruned_kernels.hip) some level of the record's net has a smooth axis: its phases then come from N-point tables per level and axis
// (PackTabs, opform_device.h: the cached tables of pruned_prepare), by value in the kernel arguments
struct PackTabs;
bool pack_mod(const PackArgs& g);
hipError_t pack_tabs(const PackArgs& g, PackTabs& t);

// ---- target_kernels.hip (aefft_net_step_grad_target) -----------------------------------
// With N_b = Xf_b - Tf_b (both [B][D][P0], D <= 4):  S [D][D][P0] += sum_b N_b Xf_b^H (mk_S layout),  es[2 a + {0, 1}] += sum_b N_b[a](0,0) (nullable),
// K [D][D+1][P0] = sum_b N_b [Xf_b; 1]^H,  n2 [P0] = sum_b |N_b|^2.  The batch is summed in a fixed order, no atomics.
hipError_t launch_target_terms(const float2* Xf, const float2* Tf, float2* S, float* es, float2* K, float* n2, int B, int D, long P0, hipStream_t st);
// slots += scale * sum over the bins, with calc_mse's weights, of -2 Re tr(R K^H) + n2, R = [I - G' | -beta^] of pair 0's UPDATED weights:
// G [D][D][P] = F'.C'/(dM D), or null and the planar C [dM][D][P], F [D][dM][P]; F' at the DC bin: element (a, m) at Fdc[(a*dM + m) * fdc_stride]
struct TargetMseArgs { const float2 *G, *C, *F, *Fdc; long fdc_stride; const float *b, *p; const float2* K; const float* n2; float* slots;
                       int dM, Nx, Ny; long P; float scale; };
hipError_t launch_target_mse(const TargetMseArgs& q, int D, hipStream_t st);

// ---- update_kernels.hip ----------------------------------------------------------------
hipError_t launch_pad(const float* ck, float* cpad, long planes, int Nx, int Ny, int Nk, int Nl, hipStream_t st);   // fft.cu:570 (zero-fills)
hipError_t launch_shrink(const float* cpad, float* ck, long planes, int Nx, int Ny, int Nk, int Nl, float scale, hipStream_t st); // fft.cu:535
struct UpdateArgs {
    float *c, *f, *b, *p;                 // weights, updated in place
    const float *dck, *dfk, *db, *dp;     // gradients (coordinate space)
    float *Dc, *Df, *Db, *Dp;             // momentum
    const float *cd, *fd, *bd, *pd;       // multiobjective gradients (null when maxdiff=0)
    int dM, dD, Nk, Nl;
    float del, alpha, w0, w1;
    float gscale;                         // gradients are multiplied by this first (1/world_size for data-parallel means)
    int sym;                              // tied weights: g = g_c[m][d] + g_f[d][m], f[d][m] <- c[m][d]
    float *ddc, *ddf, *ddb, *ddp;         // optional: record the gradients used (adapt_rate, backproplib.cu:33); may be null
    float* zero;                          // optional: one float set to 0 (the pair's MSE accumulator, saves a memset launch)
};
hipError_t launch_update(const UpdateArgs& a, hipStream_t st);
hipError_t launch_vec_add(float* out, const float* a, const float* b, long n, hipStream_t st);      // out = a + b
hipError_t launch_u8_to_f32(float* out, const unsigned char* in, long n, hipStream_t st);             // out = (float)in
struct UpdateGroup { UpdateArgs a[8]; int n; int start[9]; };
hipError_t launch_update_group(UpdateGroup& g, hipStream_t st);                                       // up to 8 pairs, one launch                                      // fft.cu:605 / 657
size_t gradient_diff_ws_floats(int dM, int dD, int Nk, int Nl);      // floats of launch_gradient_diff's workspace (chunk partial sums)
hipError_t launch_gradient_diff(const float* c, const float* f, const float* b, const float* p, float* cd, float* fd,
                                float* bd, float* pd, float* den_ws, int dM, int dD, int Nk, int Nl, hipStream_t st);   // fft.cu:709

struct GdiffProb { const float *c, *f, *b, *p; float *cd, *fd, *bd, *pd, *part; int dM, dD; int chunk, nchunks; /* (filled by the launcher) */ };
struct GdiffGroup { GdiffProb q[8]; int n; int start[9], fstart[9]; };
hipError_t launch_gradient_diff_group(GdiffGroup& g, int Nk, int Nl, hipStream_t st);                 // every pair's fft.cu:709 terms, two launches

// ---- spatial_kernels.hip ---------------------------------------------------------------
hipError_t launch_conv_spatial(const float* in, float* out, const float* c, const float* b, int B, int dD, int dM,
                               int Nx, int Ny, int Nk, int Nl, int ak, int al, float in_scale_div, int lo, hipStream_t st,
                               int pool = 0 /* fused Pool(scale) in front: `in` is [B][dD][Nx*pool][Ny*pool] */, float* pooled_out = nullptr,
                               int up = 0 /* fused Pool(-up) in front: `in` is [B][dD][Nx/up][Ny/up] */,
                               float* out_up = nullptr, int out_up_s = 0 /* also the output up-sampled by out_up_s: [B][dM][Nx*s][Ny*s] */);
struct SpatialGradArgs {
    const float *in, *out, *hin, *f;      // [dD][Nx][Ny], [dD][Nx][Ny], [dM][Nx][Ny], [dD][dM][Nk][Nl]
    float *gc, *gf, *gb, *gp;             // [dM][dD][Nk][Nl], [dD][dM][Nk][Nl], [dM], [dD]
    float *ws;                            // workspace: dM*Nx*Ny (back-conv) floats
    float *part;                          // workspace: spatial_partial_floats() floats (tiled weight-gradient partial sums); null: naive kernels
    float *rq;                            // workspace: spatial_rq_floats() floats (the error-input correlation R and its row sums); null: dC through the back-convolved error
    int B, dD, dM, Nx, Ny, Nk, Nl, ak, al;
    float Norm;
    int lo;                               // 0: GPU boundary test '>=0' (backproplib.cu:95), 1: CPU test '>0' (netlib.cpp:344)
    int tied;                             // backprop_gpu_cc: add the f-gradient into the c-gradient (backproplib.cu:466)
    // fused step (aefft_step_spatial): hin IS Conv_gpu(in; c1, b1) -- then dF, dP follow from the same error-input region sums as dC
    // (dF[d][m][t] = sum_{d2,t2} c1[m][d2][t2]/div1 R_t[d][d2][t+t2] + b1[m] S_t[d]) and the hidden layer is not read by the gradient
    const float *c1 = nullptr, *b1 = nullptr;
    float div1 = 1.f;
    // nullable: on the region route (spatial_regions_ok) also sum (out - in)^2 / Norm / B into *mse, from the error tile the route stages anyway
    float* mse = nullptr;
};
hipError_t launch_spatial_grad(const SpatialGradArgs& a, hipStream_t st);
bool spatial_regions_ok(const SpatialGradArgs& a);   // the gradient goes through the error-input region sums (what the fused step needs)
hipError_t launch_spatial_compat(const SpatialGradArgs& a, hipStream_t st);   // B-11: gf and gb as the CUDA source computes them (after launch_spatial_grad)
size_t spatial_partial_floats(int B, int dD, int dM, int Nx, int Ny, int Nk, int Nl);
size_t spatial_rq_floats(int dD, int Nk, int Nl);
hipError_t launch_pool_spatial(const float* in, float* out, long planes, int Nxi, int Nyi, int Nxo, int Nyo, int scale, hipStream_t st);   // netlib.cpp:114   // 0: shape not served by the tiled kernels
// the spatial net's per-pair MSE: dst[k] = scale[k] * sum (a[k] - b[k])^2 over n[k] floats, for up to SQD_MAX pairs in two launches (fixed-order
// partial sums: the same inputs give the same bits); part: SQD_MAX * SQD_BLOCKS floats
constexpr int SQD_MAX = 8, SQD_BLOCKS = 128;
struct SqdiffGroup { const float* a[SQD_MAX]; const float* b[SQD_MAX]; long n[SQD_MAX]; float scale[SQD_MAX]; float* dst[SQD_MAX]; int count; };
hipError_t launch_sqdiff_group(const SqdiffGroup& g, float* part, hipStream_t st);
// the spatial net's MSE tail at aefft_net_step_apply: tail[l] <- tail[l] * scale, the same into save[l] and mse[l] (nullable).  The tail then
// holds the global mean on every rank, so a further all-reduce of it times 1/world (dp.py flush_mse) gives the mean back
hipError_t launch_scale_tail(float* tail, float* save, float* mse, int L, float scale, hipStream_t st);

}  // namespace aefft
