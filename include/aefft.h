/* aefft.h -- flat C ABI of the MI355X-native FFT-convolution autoencoder training path.
 *
 * This is the drop-in boundary UNDER the reference's C++ operator headers.  The reference
 * (fabrii4/AutoEncoder-FFT) exposes its hot path as C++ free functions over nested std::vector
 * (source/fft_backproplib.h:5-11, source/backproplib.h:5-16, source/netlib.h:4-24); those same
 * functions are re-exported, mangled identically, by include/fft_backproplib.h, backproplib.h and
 * netlib.h of this repo, and are thin marshalling shims over the entry points below.  Every entry
 * point here names the reference function (file:line) whose arithmetic it reproduces.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++ / torch types.
 *   - "_d" pointers are DEVICE pointers (16-byte aligned), "_h" are host pointers.
 *   - real tensors  : float32, [ch][Nx][Ny]   (x = first index, y contiguous; reference layout)
 *   - spectra       : interleaved complex64 (float pairs), [ch][Nx][Nyr], Nyr = Ny/2+1
 *   - encoder kernel: c[dM][dD][Nk][Nl], bias b[dM]; decoder kernel f[dD][dM][Nk][Nl], bias p[dD]
 *   - batches add an outermost [B] dimension.  B = 1 reproduces the reference call exactly.
 *   - Nx, Ny: powers of two in 8..2048; pooling scales: powers of two -- for the resident network and the per-bin ops.
 *     "Smooth" sizes -- even, 10..2048, no prime factor other than 2, 3, 5 (640, 480, 720, 1920, ...: camera frames) -- go through
 *     mixed-radix transforms and are taken by the per-bin ops (aefft_kernel_spectrum, aefft_kernel_export, aefft_conv, aefft_gradient,
 *     aefft_update) and, opted in with AEFFT_NET_SMOOTH_SIZES, by the resident network (aefft_net_create_ex), mixed freely with
 *     power-of-two axes.  The transforms and the spectral resize at op level (aefft_r2c, aefft_c2r, aefft_pool, aefft_r2c_pool,
 *     aefft_unpool_c2r) take smooth sizes up to 2048 and, through Bluestein's chirp-z form, every other EVEN size in 8..1024 (cufftPlanMany
 *     takes any size, fft_backproplib.cu:773-779), with any integer scale, sized as the reference sizes it (:980-984: int(Nx / l) in float
 *     arithmetic; the resized grid must be even).
 *   - every function returns AEFFT_OK (0) or an error code; aefft_last_error() gives the text.
 *     Work is enqueued on the context's stream; nothing blocks unless stated.
 *   - there is NO CPU fallback: every call fails with AEFFT_EHIP when no MI355X is present.
 */
#ifndef AEFFT_H
#define AEFFT_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct aefft_ctx aefft_ctx;   /* device + stream + twiddle tables + workspace pool */
typedef struct aefft_net aefft_net;   /* a stacked autoencoder resident on the device       */

enum {
    AEFFT_OK = 0,
    AEFFT_EINVAL = 1,       /* bad argument (size not a power of two, misaligned pointer, ...) */
    AEFFT_EHIP = 2,         /* HIP runtime error / no device */
    AEFFT_ENOMEM = 3,
    AEFFT_ESTATE = 4        /* call order violated (e.g. train before forward) */
};

/* ---- context ------------------------------------------------------------------------------- */
/* create_stream = 0: enqueue on `hip_stream`, a hipStream_t owned by the caller (e.g. torch's
 * current stream; NULL is the legacy default stream).  create_stream = 1: the context creates
 * and owns a non-blocking stream (`hip_stream` ignored). */
int aefft_ctx_create(aefft_ctx** out, int device, void* hip_stream, int create_stream);
void aefft_ctx_destroy(aefft_ctx* ctx);
const char* aefft_last_error(const aefft_ctx* ctx);
/* Optional spatial partition of the chip for pipelined training loops (aefft_net_set_input_ready): side_cus > 0 gives the library's side
 * streams (reconstruction inverse FFT, input prefetch: bandwidth-bound) `side_cus` of the device's compute units and the context's own
 * stream (the latency-bound weight side of the step) the rest, through CU-masked HIP streams; 0 removes the partition.  Only for a context
 * that owns its stream (create_stream = 1) and before its first net is created (AEFFT_ESTATE otherwise): aefft_stream() changes. */
int aefft_ctx_partition(aefft_ctx* ctx, int side_cus);
int aefft_sync(aefft_ctx* ctx);                 /* hipStreamSynchronize on the context stream */
void* aefft_stream(aefft_ctx* ctx);             /* the hipStream_t in use */
/* Development switches: each bit turns ONE optimisation of the training step off (or forces one the shapes would not choose), so
 * that the parity tests can run every fallback against the oracle.  Process-wide (one word for every context); the default is 0.  The
 * environment variable AEFFT_FLAGS (comma-separated names without the AEFFT_F_ prefix, e.g. "NOMFMA,NOGROUP") is read ONCE, when the
 * first context is created; the library never calls getenv after that.  Its switches stay on for the life of the process:
 * aefft_ctx_set_flags sets the word to (AEFFT_FLAGS | flags).  A name in AEFFT_FLAGS that the library does not know makes
 * aefft_ctx_create fail with AEFFT_EINVAL (message on stderr) instead of silently running the default path. */
enum {
    AEFFT_F_NOLAZY = 1 << 0,      /* encoder layers on the full grid even when only their pooled part is consumed */
    AEFFT_F_NOCOMPACT = 1 << 1,   /* decoder outputs on the full grid instead of the support of the up-sampled spectra */
    AEFFT_F_NOQPATH = 1 << 2,     /* weight gradients through the dc|df spectra instead of the pruned transform Q of S */
    AEFFT_F_NOFUSEMSE = 1 << 3,   /* post-update MSE by conv, conv, diff instead of the collapsed operator + epilogue */
    AEFFT_F_NOGROUP = 1 << 4,     /* one launch per pair instead of grouped launches */
    AEFFT_F_NOMFMA = 1 << 5,      /* scalar-FMA contraction kernels instead of the matrix-core kernel */
    AEFFT_F_NOGFWD = 1 << 6,      /* innermost pair by conv, conv instead of the collapsed operator left by the previous step */
    AEFFT_F_NOOVERLAP = 1 << 7,   /* reconstruction inverse FFT on the context stream instead of a side stream (reconstructions below 8 MB or above 256 MB
                                   * stay there anyway) */
    AEFFT_F_NOFUSECROP = 1 << 8,  /* separate resize launches instead of the crop fused into the encoder contraction */
    AEFFT_F_GTAPS = 1 << 9,       /* force G = spectrum of f (*) c (chosen by itself for HBM-sized spectra) */
    AEFFT_F_NOPREFETCH = 1 << 10, /* pipelined mode: input R2C on the context stream */
    AEFFT_F_NODEFER = 1 << 11,    /* pipelined mode: reconstruction not deferred to the end of the gradient half */
    AEFFT_F_NOTILEDSPATIAL = 1 << 12, /* spatial mode: naive kernels instead of the LDS-tiled / matrix-core ones */
    AEFFT_F_NOFAST = 1 << 13,     /* generic scalar contraction kernel instead of the lean one */
    AEFFT_F_NOSPLITK = 1 << 14,   /* no split-K in the scalar contraction */
    AEFFT_F_POISON = 1 << 15,     /* NaN-fill every allocation (uninitialised reads show up in the tests) */
    AEFFT_F_NOOPFORM = 1 << 16,   /* training step per frame (batch contractions) instead of the operator form */
    AEFFT_F_NOCHAIN = 1 << 17,    /* operator form: the network on the basis frames layer by layer instead of one fused launch */
    AEFFT_F_NOFUSEUPD = 1 << 18,  /* operator form: the clipped-momentum update as its own launch instead of riding with the spectra / MSE launches */
    AEFFT_F_NOAHEAD = 1 << 19,    /* operator form: the next step's operator chain as the first launch of that step instead of riding in this step's last launch */
    AEFFT_F_NORCORR = 1 << 20,    /* spatial mode: dC through the back-convolved error (a dM-plane tensor) instead of the error-input correlation R */
    AEFFT_F_NOLAZYMSE = 1 << 21,   /* aefft_net_step_apply(mse_d = NULL) still sums the MSE slots in a launch of its own instead of leaving them to the next step's gradient launch */
    AEFFT_F_SMALLOVERLAP = 1 << 22, /* reconstructions below 8 MB take the side stream as well (the test suite's small nets then run the two-stream path of the large ones) */
    AEFFT_F_CHAINMSE = 1 << 23,    /* operator form with the chain: the innermost pair's post-update MSE inside the chain's per-bin items whatever the launch's size
                                   * (by default only in launches of more than ~6 000 workgroups, which are bound by their resident slots -- and, for the
                                   * net 3 -> 8,16,32,64 with its fused kernel compiled from a static table, in launches of more than one round of 1 536) */
    AEFFT_F_CHIRPZ = 1 << 24,      /* grids with a smooth axis, both axes up to 1024, through Bluestein's chirp-z transforms instead of the mixed-radix ones (the two
                                   * paths compared; power-of-two grids never take the mixed-radix passes) */
    AEFFT_F_NOPRUNESMOOTH = 1 << 25, /* grids with a smooth axis: kernel spectra and weight gradients by pad + full R2C / full C2R + shrink instead of the
                                   * support-pruned transforms (the two routes compared; power-of-two grids are not affected) */
    AEFFT_F_NOSTATICCHAIN = 1 << 26 /* operator form with the chain: the tail launch's per-bin steps from the step list in the kernel's arguments
                                   * (the generic step code, which serves any net) even where the net's channel counts have a compile-time
                                   * step table; the two routes give the same bits (aefft_net_tail_route says which one ran) */
};
int aefft_ctx_set_flags(aefft_ctx* ctx, unsigned flags);
unsigned aefft_ctx_get_flags(const aefft_ctx* ctx);
const char* aefft_version(void);

/* ---- op level: one entry point per reference device routine --------------------------------- */

/* fft_backproplib.cu:764-801 `fft`: batched unnormalised 2-D R2C.  x_d [planes][Nx][Ny] -> X_d [planes][Nx][Nyr]. */
int aefft_r2c(aefft_ctx* ctx, const float* x_d, float* X_d, long planes, int Nx, int Ny);
/* fft_backproplib.cu:806-864 `fft_inv` (scale = 1/(Nx*Ny)) and the bare cufftExecC2R of
 * :1219-1220 (scale = 1).  Imaginary parts of self-conjugate bins are ignored. */
int aefft_c2r(aefft_ctx* ctx, const float* X_d, float* x_d, long planes, int Nx, int Ny, float scale);
/* fft_backproplib.cu:975-1002 `pool_fft` + :87-157 `resize`: scale > 1 crops to Nx/scale,
 * scale < -1 zero-pads to Nx*|scale|, no amplitude rescale.  Out-of-place; *Nxs,*Nys receive
 * the new size (may be NULL). */
int aefft_pool(aefft_ctx* ctx, const float* X_d, float* Xs_d, long planes, int Nx, int Ny, int scale, int* Nxs, int* Nys);
/* Fused forms used by the resident network (same arithmetic, fewer bytes):
 * r2c followed by pool(scale>=1), and pool(scale<=-1) followed by c2r. */
int aefft_r2c_pool(aefft_ctx* ctx, const float* x_d, float* Xs_d, long planes, int Nx, int Ny, int scale);
int aefft_unpool_c2r(aefft_ctx* ctx, const float* Xs_d, float* x_d, long planes, int Nxs, int Nys, int scale, float out_scale);

/* fft_backproplib.cu:1018-1064 `kernel_pad` + :869-916 `kfft` (first pass of StoreLoad_cfreq,
 * :1146-1158): k_d [nA][nB][Nk][Nl] -> K_d [nA][nB][Nx][Nyr].
 * 3x3 / 5x5 / 7x7 supports are evaluated directly (the DFT of the support, no padded plane) on grids whose axes are powers of two or
 * smooth sizes (even, no prime factor above 5) with Ny/2+1 <= 320; other shapes, and grids with a smooth axis under
 * AEFFT_F_NOPRUNESMOOTH, take pad + R2C.
 * The first pruned call of a process on a smooth axis size builds that size's phase table on the device in use (one allocation and a
 * blocking upload per (device, axis size), kept for the life of the process): a one-time synchronisation inside the call, which must
 * therefore not be the first one made while the stream is being captured.  A net builds its tables in aefft_net_create_ex. */
int aefft_kernel_spectrum(aefft_ctx* ctx, const float* k_d, float* K_d, int nA, int nB, int Nk, int Nl, int Nx, int Ny);
/* fft_backproplib.cu:1166-1172 `export_cfreq` (= `kfft_inv` :921-970 + `kernel_invpad` :1069-1112).  The same shapes as
 * aefft_kernel_spectrum take the pruned adjoint (the inverse transform sampled on the support) instead of C2R + shrink, smooth grids included. */
int aefft_kernel_export(aefft_ctx* ctx, const float* K_d, float* k_d, int nA, int nB, int Nk, int Nl, int Nx, int Ny);

/* fft_backproplib.cu:1007-1013 `conv_fft` / :162-189 `conv_k`:
 *   O[b][m] = sum_d (X[b][d]/dM) * C[m][d];  Re O[b][m](0,0) += bias[m]*Nx*Ny.
 * X_d [B][dD][P], C_d [dM][dD][P], bias_d [dM], O_d [B][dM][P]. */
int aefft_conv(aefft_ctx* ctx, const float* X_d, const float* C_d, const float* bias_d, float* O_d,
               int B, int dM, int dD, int Nx, int Ny);

/* fft_backproplib.cu:395-475 `gradient_k_io`.  Xin/Xout/O [B][dD][P]; C [dM][dD][P]; F [dD][dM][P];
 * outputs dc [dM][dD][P], df [dD][dM][P], db [dM], dp [dD]; for B > 1 the mean over frames. */
int aefft_gradient(aefft_ctx* ctx, const float* Xin_d, const float* Xout_d, const float* O_d, const float* C_d,
                   const float* F_d, const float* b_d, float* dc_d, float* df_d, float* db_d, float* dp_d,
                   int B, int dM, int dD, int Nx, int Ny);

/* fft_backproplib.cu:1178-1192 `mse_fft` (+ :480-498 `calc_mse`); mean over the B frames.
 * mse_d: one float on the device. */
int aefft_mse(aefft_ctx* ctx, const float* T_d, const float* O_d, float* mse_d, int B, int dM, int dD, int Nx, int Ny);

/* fft_backproplib.cu:1197-1291 host `backprop`: unnormalised C2R of dc/df, shrink_k (:535),
 * backprop_d (:605) or gradient_diff + backprop_double (:709,:657) when maxdiff, pad_k (:570),
 * R2C -> new C, F.  c,f,b,p and the momentum buffers Dc,Df,Db,Dp are updated in place.
 * `del` is the step actually applied (the reference passes 0.1*del0, :1445).
 * Both transforms take the pruned routes of aefft_kernel_export / aefft_kernel_spectrum where those do, on power-of-two and smooth grids. */
int aefft_update(aefft_ctx* ctx, float* c_d, float* f_d, float* b_d, float* p_d, float* C_d, float* F_d,
                 const float* dc_d, const float* df_d, const float* db_d, const float* dp_d,
                 float* Dc_d, float* Df_d, float* Db_d, float* Dp_d,
                 int dM, int dD, int Nx, int Ny, int Nk, int Nl, float del, int maxdiff);

/* ---- spatial mode (coordinate space) --------------------------------------------------------- */
/* backproplib.cu:114-182 `Conv_gpu` (+ :70-111 `conv_parallel`): zero-padded direct convolution,
 * tap offset -2*ak-1+k with ak=((Nk-1)/2-1)/2, input divided by dM first (:134), + b[m].
 * in_d [B][dD][Nx][Ny] -> out_d [B][dM][Nx][Ny].  cpu_semantics=1 gives netlib.cpp:318-358 `Conv`
 * instead (ak=(Nk-1)/2-1, boundary test '>0', no division). */
int aefft_conv_spatial(aefft_ctx* ctx, const float* in_d, float* out_d, const float* c_d, const float* b_d,
                       int B, int dD, int dM, int Nx, int Ny, int Nk, int Nl, int cpu_semantics);
/* netlib.cpp:114-164 `Pool` on the device: scale > 0 pools scale x scale windows through the reference's
 * integer accumulator (`int smax = 0`: result = max(0, trunc(window maximum)), also at scale 1); scale < 0 up-samples by
 * nearest neighbour.  in_d [planes][Nxi][Nyi] -> out_d [planes][Nxo][Nyo]; outputs the reference loop never writes stay untouched. */
int aefft_pool_spatial(aefft_ctx* ctx, const float* in_d, float* out_d, long planes, int Nxi, int Nyi, int Nxo, int Nyo, int scale);
/* Pool(scale >= 1) followed by Conv_gpu in ONE launch (autoencoder.cpp:135-150 calls them back to back and
 * bounces the pooled layer through host vectors).  in_d [B][dD][Nx*scale][Ny*scale]; pooled_d (nullable) also receives the pooled
 * layer [B][dD][Nx][Ny] -- the training step needs it as the pair's input; out_d [B][dM][Nx][Ny].  Served for square 3x3 / 5x5 /
 * 7x7 kernels (AEFFT_EINVAL otherwise: pool and convolve separately). */
int aefft_pool_conv_spatial(aefft_ctx* ctx, const float* in_d, float* pooled_d, float* out_d, const float* c_d, const float* b_d,
                            int B, int dD, int dM, int Nx, int Ny, int scale, int Nk, int Nl, int cpu_semantics);
/* backproplib.cu:291-418 `backprop_gpu` (tied=0) / :521-644 `backprop_gpu_cc` (tied=1): back-conv
 * through f + weight-gradient correlation, then the inertia update
 *   d <- (1-alpha)*delmax*g/max(10,|g|) + alpha*d ; w <- w - d     (:392-396)
 * dc..dp are the caller's persistent previous-update buffers, ddc..ddp receive the gradients
 * (adapt_rate, :28-35, is otherwise inert -- Appendix B-12).  All device pointers; for B > 1 the
 * gradient is the mean over frames.  cpu_semantics: 0 = GPU geometry with the index / stale-buffer bugs of gradient_CF and the
 * `dDdB2 =` of gradient_CFBP (Appendix B-11) following the CPU reference (netlib.cpp:425-430) -- the default; 1 = the CPU
 * reference's geometry (ak = (Nk-1)/2-1, range test '>0'); 2 = GPU geometry WITH the B-11 bugs exactly as the CUDA source
 * computes them (backproplib.cu:220,225-227,283; hidden-layer reads outside the buffer, undefined there, read 0): the
 * "identical to the reference CUDA run" switch, slow. */
int aefft_backprop_spatial(aefft_ctx* ctx, const float* in_d, const float* out_d, const float* hin_d,
                           float* c_d, float* b_d, float* f_d, float* p_d,
                           float* dc_d, float* db_d, float* df_d, float* dp_d,
                           float* ddc_d, float* ddb_d, float* ddf_d, float* ddp_d,
                           int B, int dD, int dM, int Nx, int Ny, int Nk, int Nl,
                           float delmax, float alpha, int tied, int cpu_semantics);

/* One spatial-mode training step in ONE call: Conv_gpu (in -> hin), Conv_gpu (hin -> out), backprop_gpu[_cc] -- the sequence
 * autoencoder.cpp:140-148,200 runs per pair (backproplib.cu:114-182, 291-418, 521-644).  Because the hidden layer is then known to be
 * this call's own convolution of `in`, the decoder gradients dF, dP are formed from the same error-input region sums as dC, dB
 *  and the dM-plane hidden layer is read once (by the second convolution) instead of twice; shapes the region
 * route does not serve (kernels other than 3x3, more than 3 input channels, ...) run the plain sequence.  hin_d [B][dM][Nx][Ny] and
 * out_d [B][dD][Nx][Ny] receive the two layers; everything else as aefft_backprop_spatial.  cpu_semantics: 0 or 1. */
int aefft_step_spatial(aefft_ctx* ctx, const float* in_d, float* hin_d, float* out_d,
                       float* c_d, float* b_d, float* f_d, float* p_d,
                       float* dc_d, float* db_d, float* df_d, float* dp_d,
                       float* ddc_d, float* ddb_d, float* ddf_d, float* ddp_d,
                       int B, int dD, int dM, int Nx, int Ny, int Nk, int Nl,
                       float delmax, float alpha, int tied, int cpu_semantics);

/* ---- image boundary: camera images as delivered <-> the library's planar frames --------------- */
/* netlib.cpp:37-51 `ImageToSpin_C` and :54-77 `SpinToImage_C` on the device, for a batch, one launch each.  Every 8-bit entry point of the
 * network level takes PLANAR pixels; a camera, a cv::Mat, a V4L2 buffer or an image file delivers rows of interleaved pixels.  These two
 * calls convert between the two on the device, so that no host loop touches the pixels.
 * Image layout: B images, each Ny rows of `pitch` bytes; image b starts at b * Ny * pitch; pixel (row j, column i), channel d, is the byte at
 *   j * pitch + i * D + d,     pitch >= Nx * D   (cv::Mat::step, a V4L2 bytesperline, the pitch of a 2-D copy).
 * Bytes of a row beyond Nx * D are never read by aefft_image_to_frames and never written by aefft_frames_to_image.  The channel order is the
 * image's own (d is d: BGR stays BGR, as in the reference).
 * Frame layout: the library's [B][D][Nx][Ny], unsigned char when frames_u8 != 0, float otherwise:
 *   frames[b][d][i][j] = image[b][j][i][d]        i < Nx = image columns,  j < Ny = image rows.
 * The transposition is the reference's: ImageToSpin_C fills spin[c][i][j] = img.at<Vec3b>(j, i)[c] with Nx = img.cols, Ny = img.rows.
 * Values: to frames (float)pixel, exact; from float frames SpinToImage_C's rule exactly as the inverse row pass applies it for
 * aefft_net_infer(recon_u8 = 1) -- clamp((int)round(v), 0, 255), halves away from zero, NaN -> 0, -inf -> 0, +inf -> 255; from 8-bit frames
 * the bytes themselves.
 * Shapes: D in 1..4 (grey, BGR, BGRA); Nx, Ny in 1..8192, odd sizes included -- the calls are not tied to what a net accepts; B >= 1.
 * Alignment: frames_d is 16-byte aligned (the library's rule); image_d and pitch may have ANY alignment.  With image_d and pitch multiples of 4
 * the image side moves dwords, with Ny a multiple of 4 the frame side does; otherwise that side moves single bytes.  Every accepted argument
 * gives the same bytes.
 * One launch on the context's stream; no host synchronisation, no allocation, no workspace; safe under stream capture.  Out-of-place.
 * AEFFT_EINVAL, with aefft_last_error naming the rule and nothing enqueued: a null context or pointer, D outside 1..4, a size outside its
 * range, pitch < Nx * D, frames_d not 16-byte aligned, frame and image ranges that overlap. */
int aefft_image_to_frames(aefft_ctx* ctx, const unsigned char* image_d, size_t pitch, void* frames_d, int frames_u8, int B, int D, int Nx, int Ny);
int aefft_frames_to_image(aefft_ctx* ctx, const void* frames_d, int frames_u8, unsigned char* image_d, size_t pitch, int B, int D, int Nx, int Ny);

/* aefft_image_resize_to_frames: camera images of ANY size to frames -- the reference loop's `resize(rgb, imgC, Size(Nx, Ny))` followed by
 * ImageToSpin_C (autoencoder.cpp:124-125) in one launch, so that a 640 x 480 or 1920 x 1080 stream feeds a 256^2 / 512^2 / 1024^2 net without a
 * host resize and without a float, planar copy of the camera image.
 * Source: B images; image b starts at b * image_stride (ignored when B == 1); each image is H rows of `pitch` bytes; pixel (row y, column x),
 * channel d, is the byte at  y * pitch + x * D + d.  pitch >= W * D; for B > 1, image_stride >= (H - 1) * pitch + W * D.  image_d, pitch and
 * image_stride may have ANY alignment (all three multiples of 4: the image side loads dwords, bytes otherwise; the same bytes come out).  A region
 * of interest of a larger image is image_d + y0 * pitch + x0 * D with the parent's pitch and stride.  Bytes beyond W * D of a row are never read.
 * Destination: the library's [B][D][Nx][Ny] frames, unsigned char when frames_u8 != 0, float otherwise, 16-byte aligned; frames[b][d][i][j] is
 * destination column i, destination row j: the transposition of aefft_image_to_frames.
 * Shapes: D in 1..4; W, H, Nx, Ny in 1..8192, odd sizes included; B >= 1.
 * Arithmetic: all-integer, so every route and a numpy restatement give the same bits.  Per axis, source size S, destination size N:
 *   AEFFT_RESIZE_LINEAR  cv::resize's default geometry -- half-pixel centres, edges replicated, weights quantised to 1/2048.  For destination
 *     index i:  n = (2i+1) S - N, den = 2N, s = floor(n / den), r = n - s den,  w = floor((4096 r + den) / (2 den))  = round(2048 r / den),
 *     halves up;  s < 0: s = 0, w = 0;  s >= S-1: s = S-1, w = 0;  the second tap is min(s+1, S-1).  With column taps (x0, x1, wx) and row taps
 *     (y0, y1, wy):  v = (2048-wy) ((2048-wx) p[y0][x0] + wx p[y0][x1]) + wy ((2048-wx) p[y1][x0] + wx p[y1][x1])  < 2^30.
 *     8-bit frame: (v + 2^21) >> 22.  Float frame: q * 2^-16 with q = (v + 32) >> 6  (q < 2^24: the float is exact).  Any size to any size.
 *   AEFFT_RESIZE_AREA    the exact box average, the anti-aliased choice for decimation (1080p -> 256^2); requires Nx <= W and Ny <= H.
 *     Overlap of destination cell i with source pixel k:  o(i,k) = max(0, min((i+1) S, (k+1) N) - max(i S, k N))  (sum over k: S).
 *     num = sum_y oy(j,y) sum_x ox(i,x) p[y][x]  (64 bits).  8-bit frame: floor((2 num + W H) / (2 W H)).  Float frame: q * 2^-16 with
 *     q = floor((65536 num + floor(W H / 2)) / (W H)), exact in float.
 * Consequences: with W == Nx and H == Ny both modes give exactly aefft_image_to_frames' output; with integer ratios AREA is the rounded block mean.
 * Relation to OpenCV: LINEAR has cv::resize's geometry and 11-bit weights but is NOT promised byte-identical to it -- OpenCV derives its weights
 * in float and truncates in its vertical pass, and it silently switches to INTER_AREA at exact 2x reduction, which this call never does (it never
 * switches modes).  Differences of one grey level are to be expected; the difference is unmeasured (OpenCV was not available to the build).
 * One launch on the context's stream; no host synchronisation, no allocation, no workspace; safe under stream capture.  Out-of-place.
 * AEFFT_EINVAL, with aefft_last_error naming the rule, nothing enqueued and the outputs untouched: a null context or pointer, D or a size out of
 * range, an unknown mode, AREA with an enlarging axis, pitch < W * D, image_stride too small for B > 1, frames_d not 16-byte aligned, source and
 * destination byte ranges that overlap. */
enum { AEFFT_RESIZE_LINEAR = 0, AEFFT_RESIZE_AREA = 1 };
int aefft_image_resize_to_frames(aefft_ctx* ctx, const unsigned char* image_d, size_t pitch, size_t image_stride,
                                 int W, int H, int mode, void* frames_d, int frames_u8, int B, int D, int Nx, int Ny);

/* aefft_frames_resize_to_image: the mirror of aefft_image_resize_to_frames -- frames of ANY size back to camera-sized images, SpinToImage_C
 * (autoencoder.cpp:217-223) and the resize in one launch, so that a 512^2 reconstruction is written into the 640 x 480 video it came from.
 * Source: the library's [B][D][Nx][Ny] frames, 16-byte aligned, unsigned char when frames_u8 != 0, float otherwise.  The source sample at column
 * x, row y, channel d is  p[y][x] = frames[b][d][x][y]  for 8-bit frames and  px_u8(frames[b][d][x][y])  for float frames -- px_u8 is SpinToImage_C's
 * rule exactly as aefft_frames_to_image applies it: clamp((int)round(v), 0, 255), halves away from zero, NaN -> 0, -inf -> 0, +inf -> 255.  So
 * float frames are first turned into pixels, then resized.
 * Destination: B images of H rows of `pitch` bytes; image b starts at b * image_stride (ignored when B == 1); pixel (row y, column x), channel d,
 * is the byte at  y * pitch + x * D + d.  pitch >= W * D; for B > 1, image_stride >= (H - 1) * pitch + W * D.  image_d, pitch and image_stride may
 * have ANY alignment (all three multiples of 4: the image side stores dwords, bytes otherwise; the same bytes come out).  Bytes of a row beyond
 * W * D are never written.  A region of interest of a larger image is image_d + y0 * pitch + x0 * D with the parent's pitch and stride.
 * Shapes: D in 1..4; Nx, Ny, W, H in 1..8192, odd sizes included; B >= 1.
 * Arithmetic: all-integer, the per-axis formulas of AEFFT_RESIZE_LINEAR and AEFFT_RESIZE_AREA above with the roles swapped -- source sizes
 * (Nx, Ny), destination sizes (W, H).  The output is always 8-bit: LINEAR (v + 2^21) >> 22; AREA floor((2 num + Nx Ny) / (2 Nx Ny)), which requires
 * W <= Nx and H <= Ny.
 * Consequences: with W == Nx and H == Ny both modes give exactly aefft_frames_to_image's bytes.  For every accepted argument the result equals the
 * composition of three existing calls, bit for bit: aefft_frames_to_image(F) -> aefft_image_resize_to_frames(.., (W, H), mode, 8-bit) ->
 * aefft_frames_to_image; this call does it in one launch, with no intermediate image.  The relation to OpenCV's own resize is that of
 * aefft_image_resize_to_frames, and as unmeasured.
 * One launch on the context's stream; no host synchronisation, no allocation, no workspace; safe under stream capture.  Out-of-place.
 * AEFFT_EINVAL, with aefft_last_error starting "aefft_frames_resize_to_image: " and naming the rule, nothing enqueued and the outputs untouched: a
 * null context or pointer, D or a size out of range, an unknown mode, AREA with an enlarging axis, pitch < W * D, image_stride too small for
 * B > 1, frames_d not 16-byte aligned, source and destination byte ranges that overlap, sizes that overflow the address space. */
int aefft_frames_resize_to_image(aefft_ctx* ctx, const void* frames_d, int frames_u8, int Nx, int Ny, int mode,
                                 unsigned char* image_d, size_t pitch, size_t image_stride, int W, int H, int B, int D);

/* aefft_map_overlay_image: a heat map onto an image, in place -- the [B][Nx/t][Ny/t] maps of aefft_net_score_map / aefft_net_ssim_map coloured
 * and blended onto the camera-sized images on the device.
 * map_d: float [B][Mx][My], 16-byte aligned, the layout those calls write: Mx along image columns, My along image rows, My contiguous; Mx, My in
 * 1..1024.  lut_d: a colour table of 256 * D bytes on the device, entry k, channel d, at k * D + d; any alignment; supplied by the caller (the
 * library ships no colour map).  The image layout and shape rules are those of aefft_frames_resize_to_image.  alpha in 0..256.  lo, hi finite and
 * lo != hi (255 / (hi - lo) must be finite in float); hi < lo inverts the scale, which is what an SSIM map wants.
 * Definition (every step can be restated exactly in numpy):
 *   1. inv = 255.0f / (hi - lo), computed once on the host in float.
 *   2. k0[I][J] = px_u8((map[b][I][J] - lo) * inv): the subtraction and the product each rounded to float32; px_u8 as above (NaN -> 0, clamped
 *      to 0..255, halves away from zero).
 *   3. smooth == 0:  k(x, y) = k0[floor(x Mx / W)][floor(y My / H)], the tile the pixel lies in.
 *   4. smooth != 0:  the AEFFT_RESIZE_LINEAR taps on the axes (Mx -> W) and (My -> H) applied to k0, k = (v + 2^21) >> 22.
 *   5. image[y][x][d] = (alpha * lut[k][d] + (256 - alpha) * image[y][x][d] + 128) >> 8.
 * alpha = 0 leaves every byte as it was; alpha = 256 writes the table's colour exactly.  Bytes beyond W * D of a row are neither read nor written.
 * One launch on the context's stream; no host synchronisation, no allocation, no workspace; safe under stream capture.  Accounted under the
 * profile id `image` with B (4 Mx My + 2 W H D) + 256 D bytes.
 * AEFFT_EINVAL, with aefft_last_error starting "aefft_map_overlay_image: " and naming the rule, nothing enqueued and the image untouched: a null
 * context or pointer, a size, D or alpha out of range, non-finite or equal lo / hi, map_d not 16-byte aligned, pitch or image_stride too small,
 * map_d or lut_d overlapping the image range. */
int aefft_map_overlay_image(aefft_ctx* ctx, const float* map_d, int Mx, int My, float lo, float hi, int smooth,
                            const unsigned char* lut_d, int alpha,
                            unsigned char* image_d, size_t pitch, size_t image_stride, int W, int H, int B, int D);

/* aefft_frames_degrade: the degraded input of target training from the clean frame -- blur, additive noise and impulses in one launch, so that
 * aefft_net_step_grad_target(frames = degraded, targets = clean) needs no float copies of the frames and no generator outside the library.
 * src_d, dst_d: the library's [B][D][Nx][Ny] frames, 16-byte aligned, each unsigned char when its _u8 flag != 0, float otherwise.
 * Shapes: D in 1..4; Nx, Ny in 1..8192, odd sizes included; B >= 1.
 * Definition: everything behind the host's two quantisations (m and t below) is integer arithmetic, so a numpy restatement gives the same bits.
 *   1. Pixels.  p[b][d][i][j] is the source byte; for a float source px_u8(src[b][d][i][j]), SpinToImage_C's rule exactly as
 *      aefft_frames_to_image applies it: NaN -> 0, clamp to 0..255, halves away from zero.  So float frames are first turned into pixels, as in
 *      aefft_frames_resize_to_image.
 *   2. Blur, blur = r in 0..4: the separable binomial filter of 2r+1 taps per axis, w_k = C(2r, k) (sum 4^r), indices clamped to the plane
 *      (edges replicated):  h[i][j] = sum_k w_k p[clamp(i+k-r)][j],  v[i][j] = sum_l w_l h[i][clamp(j+l-r)]  <= 255 * 16^r < 2^24.  The working
 *      value in Q16 is  u = v << (16 - 4r), exact: no rounding anywhere; r = 0 gives u = p << 16.
 *   3. Random words.  Philox4x32-10 with the standard constants (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85);
 *      key = (seed low word, seed high word).  For the element of linear index n = (d Nx + i) Ny + j of frame g = first_frame + b (64-bit,
 *      wrapping) the counter is (n >> 1, 0, g low word, g high word): one call serves two elements.  An even n takes the output words
 *      (a, c) = (x0, x1), an odd n (x2, x3).  T = (sum of the four bytes of a) + (sum of the two low bytes of c) - 765;  hsel = c >> 16.
 *   4. Noise.  m = floor(((double)sigma * 65536.0) / sqrt(32767.5) + 0.5), once on the host;  u += T * m.  T is an Irwin-Hall sum of six
 *      bytes: zero mean, standard deviation sqrt(32767.5) exactly, excess kurtosis -0.2, bounded at +-4.23 sigma.  The noise is APPROXIMATELY
 *      normal, not normal: lighter tails and a hard bound.  The effective sigma is m sqrt(32767.5) / 65536: sigma quantised to about 1/362 of a
 *      grey level.  With sigma <= 255, |u| < 2^27: everything fits 32 bits.
 *   5. Impulses.  t = floor((double)impulse * 65536.0 + 0.5), once on the host.  If hsel < t the element is replaced:  u = 255 << 16 when
 *      a & 1, else u = 0.  Resolution 1/65536; impulse = 1 replaces every element.  Each element (channel) is hit on its own.
 *   6. Output.  8-bit: clamp((u + 32768) >> 16, 0, 255), arithmetic shift -- it clips as a sensor does.  Float: (float)u * 2^-16, the
 *      int32 -> float conversion rounding to nearest even; not clamped: it models additive noise.
 * Consequences: blur = 0, sigma = 0, impulse = 0 is a copy for 8-bit -> 8-bit, px_u8 for float -> 8-bit and the exact conversion for
 * 8-bit -> float.  A frame's result depends only on (seed, first_frame + b) and its own pixels, so
 *   degrade(B = 2, first_frame = f)[1] == degrade(B = 1, first_frame = f + 1)[0]:
 * a data-parallel rank passes first_frame = step * global_batch + rank * B, and the union over the ranks is the single-process batch.  A constant
 * frame stays constant under any blur.  The same arguments always give the same bytes, on every route (Ny % 4 == 0: the frame side moves dwords /
 * float4; single elements otherwise).
 * In place: dst_d == src_d is allowed exactly when blur == 0 and src_u8 == dst_u8 (the operation is then element-wise); any other overlap of the
 * two byte ranges is an error.
 * One launch on the context's stream; no host synchronisation, no allocation, no workspace; safe under stream capture.  Accounted under the
 * profile id `image` with the bytes read plus the bytes written, B D Nx Ny (source element size + destination element size).
 * AEFFT_EINVAL, with aefft_last_error starting "aefft_frames_degrade: " and naming the rule, nothing enqueued and the outputs untouched: a null
 * context or pointer; D, a size or B out of range; blur outside 0..4; sigma not finite, negative or above 255; impulse not finite or outside
 * 0..1; a pointer not 16-byte aligned; overlapping ranges other than the in-place case above; sizes that overflow the address space. */
int aefft_frames_degrade(aefft_ctx* ctx, const void* src_d, int src_u8, void* dst_d, int dst_u8,
                         int B, int D, int Nx, int Ny,
                         int blur, float sigma, float impulse,
                         unsigned long long seed, unsigned long long first_frame);

/* aefft_yuv_to_image, aefft_yuv_resize_to_frames: video as delivered -- the NV12 surface of a hardware decoder, the I420 planes of a software
 * decoder, the YUYV buffer of a V4L2 webcam -- to interleaved 8-bit images, or straight to the planar frames every 8-bit net call takes.  The
 * reference gets BGR because `cam >> rgb` (autoencoder.cpp:123) runs OpenCV's colour conversion on the host; these two calls are that conversion on
 * the device, defined bit for bit, alone or fused with the resize + ImageToSpin_C of aefft_image_resize_to_frames in one launch.
 * Source: the descriptor below, read on the host during the call (it need not outlive it).  W x H is the luma size, each in 1..8192; write
 * Wc = ceil(W / 2), Hc = ceil(H / 2).  plane[k] are device pointers of ANY alignment, pitch[k] the bytes per row of plane k; for B > 1 image b's
 * plane k starts at plane[k] + b * stride[k] (stride is ignored when B == 1).
 *   AEFFT_YUV_NV12  plane[0] is Y: H rows, Y(x, y) at y * pitch[0] + x, pitch[0] >= W.  plane[1] is interleaved chroma: Hc rows, U at
 *                   y' * pitch[1] + 2 x', V one byte behind, pitch[1] >= 2 Wc.  plane[2] is ignored.  A decoder surface that keeps both planes in
 *                   one allocation is plane[1] = plane[0] + pitch * surface_height.
 *   AEFFT_YUV_I420  plane[0] as NV12; plane[1] is U and plane[2] is V, each Hc rows of Wc bytes, pitch[k] >= Wc.  YV12 is the same call with the
 *                   two pointers swapped.
 *   AEFFT_YUV_YUYV  (YUY2) plane[0] only; W must be even.  Y(x, y) at y * pitch[0] + 2 x, U at y * pitch[0] + 4 (x >> 1) + 1, V two bytes further;
 *                   pitch[0] >= 2 W.
 * Chroma rule: NEAREST, i.e. replication -- the chroma of pixel (x, y) is the sample at (x >> 1, y >> 1) for NV12 and I420 and at (x >> 1, y) for
 * YUYV; no interpolation and no siting offset.  Odd W and H are served for NV12 and I420 (the chroma planes have the ceil sizes: the last chroma
 * column and row then serve one pixel).  For B > 1 each used stride[k] must be at least the plane's extent, (rows - 1) * pitch[k] + the live bytes
 * of a row.  Bytes of a row beyond its live bytes are never read.  With order == AEFFT_YUV_GRAY no chroma plane is read, and plane[1] and plane[2]
 * may be NULL.  A region of interest with even x0, y0 is pointer arithmetic on the caller's side, as for aefft_image_resize_to_frames.
 * Arithmetic: all-integer, 32 bits suffice.  With c = Y - yoff, u = U - 128, v = V - 128:
 *   p[y][x][ch] = clamp((ky c + a_ch u + b_ch v + 2^19) >> 20, 0, 255)          (>> 20: an arithmetic shift, i.e. the floor)
 *   matrix            yoff  ky        R: (a, b)       G: (a, b)             B: (a, b)
 *   AEFFT_YUV_BT601   16    1220945   (0, 1673555)    (-410793, -852458)    (2115221, 0)       BT.601, limited range
 *   AEFFT_YUV_BT709   16    1220945   (0, 1879825)    (-223607, -558796)    (2215014, 0)       BT.709, limited range
 *   AEFFT_YUV_JPEG    0     1048576   (0, 1470104)    (-360853, -748826)    (1858077, 0)       BT.601, full range (MJPEG)
 * Each entry is round(k * 2^20) of the standards' constants in double: Kr = 0.299, Kb = 0.114 (601) or Kr = 0.2126, Kb = 0.0722 (709),
 * Kg = 1 - Kr - Kb;  ky = s_y,  b_R = 2 (1 - Kr) s_c,  a_G = -2 (1 - Kb) (Kb / Kg) s_c,  b_G = -2 (1 - Kr) (Kr / Kg) s_c,  a_B = 2 (1 - Kb) s_c;
 * s_y = 255 / 219 and s_c = 255 / 224 for the limited ranges, both 1 for JPEG.  c is NOT clamped below zero (Y < 16): the final clamp does that
 * work.  The largest magnitude is below 2^30.  order AEFFT_YUV_BGR stores the rows (B, G, R) at d = 0, 1, 2 and AEFFT_YUV_RGB the reverse: D = 3.
 * AEFFT_YUV_GRAY is clamp((ky c + 2^19) >> 20, 0, 255), D = 1; for AEFFT_YUV_JPEG that is Y itself.
 * Relation to OpenCV: cv::cvtColor's YUV conversions have the same form (fixed-point, nearest chroma) but OpenCV's OWN constants and its own
 * handling of Y < 16; they are not the ones above.  Differences of a grey level are to be expected; the difference is unmeasured (OpenCV was not
 * available to the build).
 * aefft_yuv_to_image writes p into B interleaved images of D channels with the destination layout and rules of aefft_frames_resize_to_image:
 * pixel (row y, column x), channel d, at y * pitch + x * D + d; pitch >= W * D; image b at b * image_stride, image_stride >= (H - 1) * pitch + W * D for
 * B > 1 (ignored when B == 1); any alignment; bytes beyond W * D of a row are never written.
 * aefft_yuv_resize_to_frames is, for every accepted argument and bit for bit, aefft_yuv_to_image into a tight image followed by
 * aefft_image_resize_to_frames(.., W, H, mode, frames_d, frames_u8, B, D, Nx, Ny): the AEFFT_RESIZE_LINEAR / AEFFT_RESIZE_AREA formulas above with p
 * as the source pixels, to 8-bit or float frames [B][D][Nx][Ny], 16-byte aligned -- in one launch with no intermediate image.  With Nx == W and
 * Ny == H both modes give aefft_yuv_to_image -> aefft_image_to_frames.  Nx, Ny in 1..8192; AEFFT_RESIZE_AREA requires Nx <= W and Ny <= H.
 * Both calls: one launch on the context's stream; no host synchronisation, no allocation, no workspace; safe under stream capture.  Out-of-place.
 * Accounted under the profile id `image` with the bytes read plus the bytes written: B times the source samples (W H luma and, unless the order is
 * GRAY, 2 Wc Hc chroma; YUYV 2 W H) plus B W H D image bytes or the B D Nx Ny frame elements.
 * AEFFT_EINVAL, with aefft_last_error starting with the call's name ("aefft_yuv_to_image: ", "aefft_yuv_resize_to_frames: ") and naming the rule,
 * nothing enqueued and the outputs untouched: a null context, descriptor, output or needed plane; an unknown format, matrix, order or mode; a size
 * or B out of range; YUYV with odd W; a pitch or stride too small; AREA with an enlarging axis; frames_d not 16-byte aligned; any source plane's
 * byte range overlapping the destination's; sizes that overflow the address space. */
enum { AEFFT_YUV_NV12 = 0, AEFFT_YUV_I420 = 1, AEFFT_YUV_YUYV = 2 };      /* format */
enum { AEFFT_YUV_BT601 = 0, AEFFT_YUV_BT709 = 1, AEFFT_YUV_JPEG = 2 };    /* matrix: 601 limited, 709 limited, 601 full range (MJPEG) */
enum { AEFFT_YUV_BGR = 0, AEFFT_YUV_RGB = 1, AEFFT_YUV_GRAY = 2 };        /* order of the produced channels: D = 3, 3, 1 */
typedef struct {
    int format, matrix;
    int W, H;                          /* luma size; 1..8192 */
    const unsigned char* plane[3];     /* device pointers, ANY alignment */
    size_t pitch[3];                   /* bytes per row of each plane */
    size_t stride[3];                  /* image b's plane k starts at plane[k] + b * stride[k]; ignored when B == 1 */
} aefft_yuv_desc;
int aefft_yuv_to_image(aefft_ctx* ctx, const aefft_yuv_desc* src, int order,
                       unsigned char* image_d, size_t pitch, size_t image_stride, int B);
int aefft_yuv_resize_to_frames(aefft_ctx* ctx, const aefft_yuv_desc* src, int order, int mode,
                               void* frames_d, int frames_u8, int B, int Nx, int Ny);

/* aefft_tile_plan_make, aefft_image_tiles_to_frames, aefft_frames_tiles_to_image: tiled inference.  A net takes frames of its own size; an image
 * of the sensor's size is cut into overlapping tiles of that size (the gather), the net runs over the tiles, and the reconstructed tiles are
 * blended back into an image of the sensor's size (the blend).  The FFT net's convolution is circular, so the rim of every tile is contaminated
 * by wrap-around from the opposite edge: tiles overlap, the rim is never used, and across the rest of the overlap the two tiles are blended
 * with integer ramp weights that sum to a constant, so that an unchanged image is restored exactly.
 * The plan (host only: no device, no context).  Per axis, with image size W, tile N, overlap V and rim M, in integer arithmetic only:
 *   S = N - V  (the step)   and   R = V - 2M  (the ramp);
 *   n = max(1, ceil((W - N + 2M) / S) + 1), the smallest count whose kept areas [o_t + M, o_t + N - M) cover [0, W);
 *   E = (n-1) S + N - 2M - W >= 0;   o_0 = -M - floor(E / 2), so the grid is centred;   o_t = o_0 + t S.
 * Ranges: W, H in 1..8192; Nx, Ny in 2..2048 (Nx along image columns, Ny along rows); 0 <= 2 V <= N; 0 <= 2 M <= V.  The last two guarantee that
 * at most two tiles per axis cover any pixel.  Examples (W, N, V, M): (1920, 512, 64, 8) gives n = 5, S = 448, R = 48, o_0 = -192;
 * (13, 8, 4, 1) gives n = 3, S = 4, R = 2, o_0 = -1; (5, 8, 4, 1) gives n = 1, o_0 = -1; (9, 8, 4, 2) gives n = 3, R = 0, o_0 = -3.
 * aefft_tile_plan_make returns AEFFT_EINVAL for a null pointer or any value outside the ranges above and writes nothing in that case.
 * Tile order in the frame buffer is image-major, then tile row, then tile column: frame f = (b * nty + ty) * ntx + tx, and T = B * ntx * nty.
 * aefft_image_tiles_to_frames (the gather).  Source: B interleaved images with the layout and rules of aefft_image_resize_to_frames -- pixel
 * (row y, column x), channel d, at y * pitch + x * D + d; any alignment; pitch >= W * D; image b at image_d + b * image_stride,
 * image_stride >= (H - 1) * pitch + W * D for B > 1 (ignored when B == 1); bytes beyond W * D of a row are never read.  Destination: frames
 * [T][D][Nx][Ny], unsigned char when frames_u8 != 0, float with (float)pixel otherwise, 16-byte aligned:
 *   frames[f][d][i][j] = image[b][ry(oy_ty + j)][rx(ox_tx + i)][d]
 * r is reflection without repeating the edge pixel (OpenCV's BORDER_REFLECT_101), iterated so that it is defined for any reach: for W = 1 the
 * result is 0; otherwise P = 2(W-1), m = x mod P taken non-negative, r = m when m < W, else P - m.  Every element of every tile is written.
 * aefft_frames_tiles_to_image (the blend).  Source samples p are the bytes of 8-bit frames, or px_u8(v) for float frames: float frames are first
 * turned into pixels, as in aefft_frames_resize_to_image and aefft_frames_degrade.  Destination: B images, layout as above.  The per-axis weight
 * of tile t at image coordinate x, with k = x - o_t, is
 *   0                      when k < M or k >= N - M;
 *   2(k - M) + 1           when t > 0 and k < M + R                (left ramp);
 *   2(N - M - 1 - k) + 1   when t < n-1 and k >= N - M - R        (right ramp);
 *   den                    otherwise, with den = 2R for R > 0 and den = 1 for R = 0.
 * In a seam the two weights add up to 2R, so the weights over all tiles sum to den at every x.  With R = 0 the kept areas abut and there is no
 * blend.  The outermost tiles have no ramp on their outer side.  The output is
 *   acc = sum over the (at most four) tiles of wx * wy * p;    image[y][x][d] = floor((2 acc + denx deny) / (2 denx deny)).
 * With N <= 2048, acc < 255 * 2^22, so 32 bits are enough.  Every pixel of [0,W) x [0,H) is written once; bytes beyond W * D of a row are never
 * written and the image is never read.
 * Consequences: blend(gather(image)) returns the image's bytes for every valid description.  With W == Nx, H == Ny, V = 0 the two calls are
 * aefft_image_to_frames / aefft_frames_to_image.  Constant tiles give a constant image.  The same arguments always give the same bytes, on every
 * route (image pointer, pitch and stride multiples of 4: the image side moves dwords; Ny % 4 == 0: the frame side moves dwords / float4; single
 * elements otherwise).
 * Both calls: one launch on the context's stream; no host synchronisation, no allocation, no workspace; safe under stream capture.  Out-of-place.
 * Accounted under the profile id `image` with the bytes read plus the bytes written: the B W H D image bytes plus the T D Nx Ny frame elements
 * (1 or 4 bytes each).
 * AEFFT_EINVAL, with aefft_last_error starting with the call's name ("aefft_image_tiles_to_frames: ", "aefft_frames_tiles_to_image: ") and naming
 * the rule, nothing enqueued and the outputs untouched: a null context, pointer or description; anything aefft_tile_plan_make refuses; D outside
 * 1..4; B < 1; a pitch or stride that is too small; frames_d not 16-byte aligned; overlapping source and destination ranges; sizes that overflow the
 * address space or an int tile count. */
typedef struct { int W, H;            /* image size, 1..8192 */
                 int Nx, Ny;          /* tile = frame size, 2..2048 (Nx along image columns, Ny along rows) */
                 int overlap_x, overlap_y;   /* V: pixels two neighbouring tiles share, 0 <= 2 V <= N */
                 int rim_x, rim_y;           /* M: pixels at each tile edge that are never used, 0 <= 2 M <= V */
} aefft_tile_desc;
typedef struct { int ntx, nty;        /* tiles per image along columns / rows */
                 int ox0, oy0;        /* origin of tile 0 in image coordinates (<= 0) */
                 int step_x, step_y;  /* S = N - V */
                 int ramp_x, ramp_y;  /* R = V - 2 M */
} aefft_tile_plan;
int aefft_tile_plan_make(const aefft_tile_desc* desc, aefft_tile_plan* plan);
int aefft_image_tiles_to_frames(aefft_ctx* ctx, const unsigned char* image_d, size_t pitch, size_t image_stride,
                                const aefft_tile_desc* desc, void* frames_d, int frames_u8, int B, int D);
int aefft_frames_tiles_to_image(aefft_ctx* ctx, const void* frames_d, int frames_u8, const aefft_tile_desc* desc,
                                unsigned char* image_d, size_t pitch, size_t image_stride, int B, int D);

/* aefft_image_to_yuv, aefft_frames_resize_to_yuv: video OUT, the mirror of aefft_yuv_to_image / aefft_yuv_resize_to_frames -- interleaved 8-bit
 * images, or the planar frames a net writes, to the NV12 surface a hardware encoder takes, the I420 planes of a software encoder or the YUYV
 * buffer of a V4L2 loopback or capture-card sink.  The reference's display path ends in SpinToImage_C + imshow (autoencoder.cpp:217-223); a
 * deployed restorer ends in an encoder, and these two calls close decoder -> frames -> net -> frames -> encoder on the device.
 * Destination: the descriptor below, read on the host during the call (it need not outlive it), with EXACTLY the plane layouts, pitches,
 * ceil-sized chroma planes and odd sizes of aefft_yuv_desc above.  W x H is the luma size, each in 1..8192; Wc = ceil(W / 2), Hc = ceil(H / 2).
 * plane[k] are device pointers of ANY alignment, pitch[k] the bytes per row; for B > 1 image b's plane k starts at plane[k] + b * stride[k]
 * (ignored when B == 1), each stride at least (rows - 1) * pitch[k] + the live bytes of a row.
 *   AEFFT_YUV_NV12  plane[0] Y: H rows, Y(x, y) at y * pitch[0] + x, pitch[0] >= W.  plane[1]: Hc rows, U at y' * pitch[1] + 2 x', V one byte
 *                   behind, pitch[1] >= 2 Wc.  One surface, plane[1] = plane[0] + pitch * surface_height, is the normal case.
 *   AEFFT_YUV_I420  plane[0] as NV12; plane[1] is U and plane[2] is V, each Hc rows of Wc bytes, pitch[k] >= Wc.  YV12: swap the two pointers.
 *   AEFFT_YUV_YUYV  plane[0] only; W must be even.  Y(x, y) at y * pitch[0] + 2 x, U at y * pitch[0] + 4 (x >> 1) + 1, V two bytes further;
 *                   pitch[0] >= 2 W.
 * order names the channels of the image or frames: AEFFT_YUV_BGR, AEFFT_YUV_RGB (D = 3) or AEFFT_YUV_GRAY (D = 1).
 * aefft_image_to_yuv reads B images with the source layout of aefft_image_resize_to_frames: pixel (row y, column x), channel d, at
 * y * pitch + x * D + d; any alignment; pitch >= W * D; image b at b * image_stride, image_stride >= (H - 1) * pitch + W * D for B > 1.
 * aefft_frames_resize_to_yuv reads frames [B][D][Nx][Ny], 16-byte aligned, 8-bit when frames_u8 != 0, float through px_u8 otherwise, and resizes
 * them to W x H by `mode` with every rule of aefft_frames_resize_to_image (AEFFT_RESIZE_AREA requires W <= Nx and H <= Ny).
 * Arithmetic: all-integer, 32 bits, defined bit for bit.  With R, G, B the pixel's channels, one luma sample per pixel:
 *   Y = yoff + ((yr R + yg G + yb B + 2^19) >> 20)                      in 16..235 (0..255 for JPEG) without a clamp
 * For a chroma sample let S_R, S_G, S_B be the channel sums over the n LIVE pixels it covers -- NV12 and I420: the block (2x'..2x'+1, 2y'..2y'+1)
 * cut to the image, n = 4, 2 at an odd edge, 1 at the odd corner; YUYV: the pair (2x', 2x'+1) of one row, n = 2:
 *   U = clamp(128 + ((ur S_R + ug S_G + ub S_B + (n << 19)) >> (20 + log2 n)), 0, 255)          V likewise with (vr, vg, vb)
 * The shifts are arithmetic shifts, i.e. the floor.  This is the rounded box average of the block: the counterpart of the nearest (replicated)
 * chroma that aefft_yuv_to_image reads; no interpolation and no siting offset.  Every magnitude stays below 2^30.
 *   matrix            yoff  ky        Y: (r, g, b)                U: (r, g, b)                   V: (r, g, b)
 *   AEFFT_YUV_BT601   16    900542    (269262, 528618, 102662)    (-155423, -305128, 460551)     (460551, -385654, -74897)
 *   AEFFT_YUV_BT709   16    900542    (191455, 644068, 65019)     (-105533, -355018, 460551)     (460551, -418321, -42230)
 *   AEFFT_YUV_JPEG    0     1048576   (313524, 615514, 119538)    (-176932, -347356, 524288)     (524288, -439026, -85262)
 * Derivation, in double with q(k) = round(k 2^20), Kr, Kb, Kg as for the table above, s_y = 219 / 255 and s_c = 224 / 255 for the limited
 * ranges, both 1 for JPEG:  ky = q(s_y), yr = q(Kr s_y), yb = q(Kb s_y), yg = ky - yr - yb;  ub = vr = q(s_c / 2),
 * ur = q(-Kr s_c / (2 (1 - Kb))), vb = q(-Kb s_c / (2 (1 - Kr)));  ug = -(ur + ub), vg = -(vr + vb).  The G entries are the remainders, so the U
 * and V rows sum to exactly 0 and the Y row to ky; each G entry is within 0.55 of its own rounding.
 * AEFFT_YUV_GRAY: Y = yoff + ((ky g + 2^19) >> 20), which is g itself for JPEG, and every chroma sample is written as 128.  All planes of the
 * format are always written.
 * Consequences: an image with R = G = B gives U = V = 128 everywhere and the planes of the GRAY order; RGB is BGR with the channel rows swapped; a
 * chroma block of four equal pixels gives what one pixel would; a constant image gives constant planes.  aefft_frames_resize_to_yuv is, for every
 * accepted argument and bit for bit, aefft_frames_resize_to_image into a tight image followed by aefft_image_to_yuv -- in one launch with no
 * intermediate image; with W == Nx and H == Ny both modes give aefft_frames_to_image -> aefft_image_to_yuv.
 * Writes: bytes of a plane row beyond its live bytes are never written -- W for Y, 2 ceil(W / 2) for NV12 chroma, ceil(W / 2) for I420 chroma,
 * 2 W for YUYV -- and nothing is read from the destination.  Stores are whole dwords when every used plane pointer, pitch and stride is a
 * multiple of 4, bytes otherwise; both routes give the same bytes.
 * Relation to OpenCV: cv::cvtColor's RGB -> YUV conversions have the same form (fixed-point, averaged chroma for the planar formats) with OpenCV's
 * OWN constants; they are not the ones above.  Differences of a grey level are to be expected; the difference is unmeasured (OpenCV was not
 * available to the build).
 * Both calls: one launch on the context's stream; no host synchronisation, no allocation, no workspace; safe under stream capture.  Out-of-place.
 * Accounted under the profile id `image` with the bytes read plus the bytes written: the B W H D image bytes or the B D Nx Ny frame elements,
 * plus B times the plane samples (W H luma and 2 Wc Hc chroma; YUYV 2 W H).
 * AEFFT_EINVAL, with aefft_last_error starting with the call's name ("aefft_image_to_yuv: ", "aefft_frames_resize_to_yuv: ") and naming the rule,
 * nothing enqueued and every output untouched: a null context, descriptor, source or needed plane; an unknown format, matrix, order or mode; a
 * size or B out of range; YUYV with an odd W; a pitch or stride below the plane's live extent; an image pitch or stride that is too small; AREA
 * with an enlarging axis; frames_d not 16-byte aligned; any two destination planes' byte ranges overlapping each other (image by image: the
 * surfaces of a batch may interleave); any destination plane overlapping the source; sizes that overflow the address space. */
typedef struct {
    int format, matrix;                /* AEFFT_YUV_NV12 / I420 / YUYV; AEFFT_YUV_BT601 / BT709 / JPEG -- the enums above */
    int W, H;                          /* luma size; 1..8192 */
    unsigned char* plane[3];           /* device pointers, ANY alignment */
    size_t pitch[3];                   /* bytes per row of each plane */
    size_t stride[3];                  /* image b's plane k starts at plane[k] + b * stride[k]; ignored when B == 1 */
} aefft_yuv_dst;
int aefft_image_to_yuv(aefft_ctx* ctx, const unsigned char* image_d, size_t pitch, size_t image_stride, int order,
                       const aefft_yuv_dst* dst, int B);
int aefft_frames_resize_to_yuv(aefft_ctx* ctx, const void* frames_d, int frames_u8, int Nx, int Ny, int mode, int order,
                               const aefft_yuv_dst* dst, int B);

/* aefft_image_compare_map: where two images differ, at the images' own resolution -- a per-cell mean squared error or SSIM map of two interleaved
 * 8-bit images (the camera image and the blended reconstruction of tiled inference, or a clean target and a restored image) and, optionally, the
 * per-image score; the map is what aefft_map_overlay_image paints.
 * a_d, b_d: B images each of W x H pixels of D channels in the layout of aefft_image_resize_to_frames -- pixel (row y, column x), channel d, at
 * y * pitch + x * D + d; pointer, pitch and stride of any alignment; pitch >= W * D; for B > 1 stride >= (H - 1) * pitch + W * D (ignored when
 * B == 1); bytes of a row beyond W * D are never read.  Each image has its own pitch and stride (a region of interest of a padded buffer against a
 * tight one).  Both are only read: a_d == b_d and any overlap of the two are allowed.  map_d: float [B][Mx][My], My contiguous, 16-byte aligned
 * -- the layout aefft_net_score_map writes and aefft_map_overlay_image reads.  score_d: float [B], 16-byte aligned, or NULL.
 * Cells: pixel column x belongs to cell I = floor(x Mx / W), row y to J = floor(y My / H) -- step 3 of aefft_map_overlay_image read backwards, so
 * smooth = 0 colours exactly the pixels an entry was computed from, whatever W and H are.  Cell I covers the columns [ceil(I W / Mx),
 * ceil((I+1) W / Mx)), nx_I = floor(W / Mx) or ceil(W / Mx) of them; rows alike; with W = t Mx the cells are the t x t tiles.  W, H in 1..8192,
 * D in 1..4, B >= 1, 1 <= Mx <= min(W, 1024), 1 <= My <= min(H, 1024), ceil(W / Mx) <= 64 and ceil(H / My) <= 64: a cell has
 * n = nx_I ny_J <= 4096 pixels.  B * My <= 2^31 - 1 (the cell rows of a batch are counted in an int).
 * Definition -- integers up to a stated handful of IEEE double operations, so that numpy gives the same bits.  x, r: the bytes of a and b.
 *   AEFFT_COMPARE_MSE:   e = sum over d < D and the cell's pixels of (x - r)^2 (< 2^31);  map = (float)((double)e / (double)(D n)).
 *   AEFFT_COMPARE_SSIM:  data range 255, C1 = 6.5025, C2 = 58.5225, uniform weights, population statistics: the formula of aefft_net_ssim_map
 *     cleared of its denominators.  Per channel d, with the integer moments Sx, Sr, Sxx, Srr, Sxr of the cell, K1 = 65025 and K2 = 585225:
 *       A1 = 20000 Sx Sr + K1 n^2              A2 = 20000 (n Sxr - Sx Sr) + K2 n^2   (may be negative)
 *       B1 = 10000 (Sx^2 + Sr^2) + K1 n^2      B2 = 10000 (n Sxx - Sx^2 + n Srr - Sr^2) + K2 n^2
 *     exact in signed 64 bits (magnitudes below 2.3e16), B1, B2 > 0;  ssim_d = ((double)A1 * (double)A2) / ((double)B1 * (double)B2): four
 *     conversions (round to nearest even), two products, one division -- nothing that can contract into an FMA;
 *     map = (float)((ssim_0 + ... + ssim_{D-1}) / (double)D), added in ascending d.
 * Identical images give exactly 0.0f (MSE) and exactly 1.0f (SSIM); swapping a and b gives the same bits.
 * Score (score_d != NULL), a function of the map AS STORED, its pixel-weighted mean: r_I = ((m[I][0] n_I0 + m[I][1] n_I1) + ...) in double,
 * ascending J; S = ((r_0 + r_1) + ...), ascending I; score[b] = (float)(S / (double)(W H)).  Each product of a float with an integer <= 4096 is
 * exact in double.  For MSE the score is the image's mean squared error up to the float rounding of the entries -- PSNR = 10 log10(255^2 / score)
 * --, for SSIM the pixel-weighted mean SSIM.
 * One launch on the context's stream, two with score_d (a small finish kernel that reads the map back); no host synchronisation, no allocation,
 * no workspace, no global atomics (every cell is owned by one workgroup); safe under stream capture.  Accounted under the profile id `image` with
 * 2 B W H D + 4 B Mx My bytes.
 * AEFFT_EINVAL, with aefft_last_error starting "aefft_image_compare_map: " and naming the rule, nothing enqueued and both outputs untouched: a
 * null context, source or map; a size, D, B, Mx or My out of range; a cell side above 64; an unknown metric; a pitch or stride that is too small;
 * map_d or score_d not 16-byte aligned; map_d or score_d overlapping either image or each other; sizes that overflow the address space or B * My beyond an int. */
enum { AEFFT_COMPARE_MSE = 0, AEFFT_COMPARE_SSIM = 1 };
int aefft_image_compare_map(aefft_ctx* ctx,
                            const unsigned char* a_d, size_t a_pitch, size_t a_stride,
                            const unsigned char* b_d, size_t b_pitch, size_t b_stride,
                            int W, int H, int B, int D, int metric, int Mx, int My,
                            float* map_d, float* score_d /* nullable */);

/* aefft_map_regions: detections from a map -- hysteresis threshold, connected components, a label map, per-region boxes with area and peak, and a
 * per-image count, on the device: the step a caller of aefft_net_score_map, aefft_net_ssim_map or aefft_image_compare_map otherwise takes on the
 * host, behind a copy and a synchronisation.
 * map_d: float [B][Mx][My], My contiguous -- the layout the map calls write and the overlay reads.  ref_d: an optional per-cell baseline
 * [Mx][My] shared by the batch (a calibration map from nominal footage), or NULL.  labels_d: int [B][Mx][My].  regions_d: aefft_region
 * [B][max_regions], NULL exactly when max_regions == 0.  count_d: int [B].  work_d: work_bytes >= aefft_map_regions_workspace(Mx, My, B) bytes
 * (16 a cell; 0 from the query means sizes the call does not take).  Mx, My in 1..1024; B >= 1 and B * Mx * My <= 2^31 - 1; min_area >= 1;
 * max_regions in 0..65536; every pointer 16-byte aligned; the output buffers and the workspace disjoint from the inputs and from each other;
 * lo and hi finite.  A cell is (I, J), I along Mx (the image's columns) and J along My (its rows); its linear index is I * My + J.
 * Definition, exact -- nothing is rounded but the one subtraction:
 *   1. Value: v = map[b][I][J] when ref_d is NULL, otherwise v = map[b][I][J] - ref[I][J], rounded once to float32.  A -0 result counts as +0.
 *   2. Foreground: AEFFT_REGIONS_ABOVE requires lo <= hi; a cell is foreground when v >= lo and strong when v >= hi.  AEFFT_REGIONS_BELOW (an
 *      SSIM map, where low is bad) requires hi <= lo; a cell is foreground when v <= lo and strong when v <= hi.  NaN is background, because
 *      every comparison with it is false; +inf and -inf are ordinary values.
 *   3. Components: the maximal connected sets of foreground cells of one image under 4- or 8-connectivity on the (I, J) grid; there is no
 *      wrap-around and nothing connects across images.
 *   4. Kept: a component is kept when it holds at least one strong cell and area >= min_area.  hi == lo means a plain threshold.
 *   5. Numbering: the kept components of image b are numbered 1..n in ascending order of their smallest linear index I * My + J.
 *      labels[b][I][J] is that number; background cells and cells of dropped components get 0.  count[b] = n, also when n > max_regions.
 *   6. Regions: regions[b * max_regions + r - 1] is written for r <= min(n, max_regions): the inclusive bounds, the area in cells, and the peak
 *      -- the maximal v under ABOVE, the minimal v under BELOW, at the smallest linear index that attains it.  Entries from index
 *      min(n, max_regions) on are left untouched.
 *   7. aefft_region_to_pixels: aefft_image_compare_map's cell rule, host arithmetic -- the half-open pixel ranges x0 = ceil(i0 W / Mx),
 *      x1 = ceil((i1+1) W / Mx), y0 = ceil(j0 H / My), y1 = ceil((j1+1) H / My); the full grid gives (0, 0, W, H).  AEFFT_EINVAL for a null
 *      pointer, bounds outside the grid (0 <= i0 <= i1 < Mx, 0 <= j0 <= j1 < My) or sizes outside that call's ranges (W, H in 1..8192,
 *      1 <= Mx <= min(W, 1024), 1 <= My <= min(H, 1024)).
 * Six launches on the context's stream (a tiled union-find: tiles in LDS, the tile edges by atomicMin, the sums by integer add / min / max and
 * one 64-bit max); no host synchronisation, no allocation (the caller supplies the workspace); safe under stream capture; no workgroup waits for
 * another; the result is a function of the inputs alone, on every run.  Accounted under the profile id `image` with
 * B Mx My (4 + 4 + 16) + 32 B max_regions bytes.
 * AEFFT_EINVAL, with aefft_last_error starting "aefft_map_regions: " and naming the rule, nothing enqueued and every output untouched: a null
 * pointer; a size out of range; an unknown sense or connectivity; lo / hi that are non-finite or in the wrong order for the sense; misalignment;
 * overlap; work_bytes below the query; regions_d and max_regions disagreeing; B * Mx * My beyond an int. */
typedef struct {
    int i0, j0, i1, j1;   /* inclusive cell bounds: I (image columns) in i0..i1, J (image rows) in j0..j1 */
    int area;             /* cells */
    int peak_i, peak_j;   /* the peak's cell */
    float peak;           /* the peak's value v */
} aefft_region;           /* 32 bytes, no padding */
enum { AEFFT_REGIONS_ABOVE = 0, AEFFT_REGIONS_BELOW = 1 };   /* BELOW: an SSIM map, where low is bad */
size_t aefft_map_regions_workspace(int Mx, int My, int B);   /* bytes; 0 on invalid sizes; at most 16 B per cell */
int aefft_map_regions(aefft_ctx* ctx, const float* map_d, const float* ref_d /* nullable, [Mx][My] */,
                      int Mx, int My, int B, int sense, float lo, float hi, int connectivity /* 4 or 8 */, int min_area,
                      int* labels_d /* [B][Mx][My] */, aefft_region* regions_d /* nullable */, int max_regions,
                      int* count_d /* [B] */, void* work_d, size_t work_bytes);
int aefft_region_to_pixels(const aefft_region* r, int Mx, int My, int W, int H, int* x0, int* y0, int* x1, int* y1);  /* host arithmetic */

/* aefft_raw_to_image: sensor data as delivered -- what a GigE / USB3 Vision or MIPI industrial camera sends: the raw colour-filter mosaic
 * (BayerRG8, BayerRG12, BayerRG12p, ...) or Mono8 / Mono12 / Mono16, one linear sample per pixel with a black level and often more than 8 bits --
 * to the interleaved 8-bit image the image calls take (aefft_image_resize_to_frames, aefft_image_tiles_to_frames, aefft_image_compare_map, the
 * tiled net calls).  Black level, white balance, demosaic, colour matrix and the gamma table are applied on the device, in one launch, before the
 * value is cut to 8 bits; everything behind the host's quantisations is integer arithmetic, so the result is defined bit for bit.
 * Source: the descriptor below, read on the host during the call (it need not outlive it; neither need ccm).  W x H samples, each in 4..8192,
 * odd sizes included.  Row y of image b starts at data + b * stride + y * pitch (stride is ignored when B == 1); data is a device pointer of ANY
 * alignment.  Sample x of a row, r:
 *   AEFFT_RAW_U8      the byte at x; bits == 8; pitch >= W.
 *   AEFFT_RAW_U16     the little-endian 16-bit word at 2 x, the value in its low `bits` bits, bits in 9..16 (bits of the word above `bits` are
 *                     ignored); pitch >= 2 W; data, pitch and stride must be multiples of 2.
 *   AEFFT_RAW_PACKED  GenICam's 10p / 12p (bits == 10 or 12): bits [x * bits, (x + 1) * bits) of the row's bytes read as a little-endian bit
 *                     stream (bit k of the stream is bit k mod 8 of byte k / 8); pitch >= ceil(W * bits / 8).  The MIPI RAW10 / RAW12 byte
 *                     order (the high bytes of a group first, the low bits gathered in a trailing byte) is a different layout and is out of scope.
 * Source bytes beyond a row's live bytes (W, 2 W, ceil(W * bits / 8)) are never read.  For B > 1 stride must be at least (H - 1) * pitch + the live
 * bytes of a row.
 * Pattern: the name gives the colours of pixels (0,0), (1,0) of row 0 and (0,1), (1,1) of row 1 -- AEFFT_RAW_RGGB: R G / G B, GRBG: G R / B G,
 * GBRG: G B / R G, BGGR: B G / G R.  This is GenICam's naming (BayerRG = RGGB).  OpenCV's COLOR_Bayer* names are shifted by one pixel: they name
 * pixels (1,1), (2,1) of the mosaic, so COLOR_BayerBG2BGR is the conversion for a GenICam BayerRG sensor.  A region of interest is pointer
 * arithmetic on the caller's side (U8, U16; PACKED when x0 * bits is a multiple of 8); an odd x0 or y0 offset selects the other pattern.
 *   1. Linearise.  Once on the host, in double, per colour c: m_c = floor(gain_c * 255 * 65536 / (white - black) + 0.5); AEFFT_EINVAL if
 *      m_c > 2^30.  Per sample of colour c: s = max(r - black, 0), u = min(s * m_c, 255 << 16), the product as in 64 bits.  u is the sample in Q16
 *      grey levels, below 2^24.  (Clamping s at ceil((255 << 16) / m_c) first and multiplying in 32 bits gives the same bits.)  Samples are
 *      white-balanced and clipped BEFORE the demosaic.  0 <= black < white <= 2^bits - 1; gain[] is R, G, B, each finite and in 0..64.
 *   2. Borders.  An index outside the image is reflected without repeating the edge: -1 -> 1, -2 -> 2, W -> W - 2, W + 1 -> W - 3 (rows alike).
 *      This keeps the mosaic's parity.
 *   3. Demosaic.  At each pixel the native colour is u itself; the two missing colours v come from the filters below over the samples u around
 *      it, c the sample at the pixel, N, S, E, W its neighbours, NE .. SW the diagonal ones, N2, S2, E2, W2 those two pixels away.  "R" stands for
 *      the colour being produced and swaps with B by symmetry.
 *      AEFFT_DEMOSAIC_BILINEAR (rounded means):
 *        G at an R/B site    (N + S + E + W + 2) >> 2
 *        R at a G site       (a + b + 1) >> 1 of its two R neighbours (E, W in an R row; N, S in a B row)
 *        R at a B site       (NE + NW + SE + SW + 2) >> 2
 *      AEFFT_DEMOSAIC_MHC (Malvar-He-Cutler's gradient-corrected 5 x 5 filters, scaled to sixteenths): v = clamp((sum + 8) >> 4, 0, 255 << 16),
 *      >> an arithmetic shift; 32 bits suffice (|sum| < 2^29):
 *        G at an R/B site                   8 c + 4 (N + S + E + W) - 2 (N2 + S2 + E2 + W2)
 *        R at a G site, R in the same row   10 c + 8 (E + W) - 2 (E2 + W2) + (N2 + S2) - 2 (NE + NW + SE + SW)
 *        R at a G site, R in the same column  the transpose: 10 c + 8 (N + S) - 2 (N2 + S2) + (E2 + W2) - 2 (NE + NW + SE + SW)
 *        R at a B site                      12 c + 4 (NE + NW + SE + SW) - 3 (N2 + S2 + E2 + W2)
 *      Every filter's coefficients sum to 16: a constant mosaic gives a constant image under both methods.
 *   4. Colour matrix.  ccm is a HOST pointer to 9 floats, row-major, out = ccm * (R, G, B); NULL is the identity and gives the identity's bits.
 *      c_ij = floor(ccm_ij * 1024 + 0.5) once on the host (floor, so negatives round to nearest too); each entry finite and |entry| < 4.
 *      q_j = (v_j + 128) >> 8 (the native colour's v is u);  o_i = sum_j c_ij q_j, which is Q18 with |o| < 2^30.
 *   5. Output byte.  Without a table (lut_d == NULL): clamp((o + 2^17) >> 18, 0, 255).  With lut_d, a DEVICE pointer to 4096 bytes of any
 *      alignment: lut[clamp((o + 2^13) >> 14, 0, 4080)] -- the table is indexed in sixteenths of a grey level of the LINEAR value, so gamma is
 *      applied before the value is cut to 8 bits; entries above 4080 are never read.  The identity table (lut[k] = (k + 8) >> 4) is NOT promised to
 *      equal the no-table route: it rounds twice.  Channels are stored B, G, R (order AEFFT_YUV_BGR) or R, G, B (AEFFT_YUV_RGB): D = 3.
 *   6. AEFFT_RAW_MONO.  Step 1 with gain[0], no demosaic: q = (u + 128) >> 8, o = 1024 q, then step 5.  D = 1; order, ccm and method's filters
 *      are ignored (method must still be a known value).
 * Consequences: with 8-bit samples, black 0, white 255, gains 1, no ccm and no table every pixel's native channel is its raw byte; a constant
 * mosaic gives a constant image; a PACKED source gives the bytes of the U16 source that holds the same samples.
 * Destination: the layout and rules of aefft_yuv_to_image -- pixel (row y, column x), channel d, at y * pitch + x * D + d; pitch >= W * D; image b
 * at b * image_stride, image_stride >= (H - 1) * pitch + W * D for B > 1 (ignored when B == 1); any alignment: dword stores when image_d, pitch and
 * image_stride are all multiples of 4, byte stores otherwise, the same bytes on both routes; bytes beyond W * D of a row are never written.
 * One launch on the context's stream; no host synchronisation, no allocation, no workspace; safe under stream capture.  Out-of-place.  Accounted
 * under the profile id `image` with the bytes read plus the bytes written: B H times the live bytes of a source row, plus B W H D image bytes,
 * plus 4096 with a table.
 * AEFFT_EINVAL, with aefft_last_error starting "aefft_raw_to_image: " and naming the rule, nothing enqueued and the outputs untouched: a null
 * context, descriptor, data or image; an unknown pattern, container, method or order; a `bits` value the container does not take; a size or B out
 * of range; a U16 pointer, pitch or stride that is odd; a pitch or stride too small; black / white out of order or out of range; a gain or ccm
 * entry that is not finite or out of range; m_c > 2^30; source, table and destination ranges that overlap; sizes that overflow the address
 * space. */
enum { AEFFT_RAW_RGGB = 0, AEFFT_RAW_GRBG = 1, AEFFT_RAW_GBRG = 2, AEFFT_RAW_BGGR = 3, AEFFT_RAW_MONO = 4 };  /* pattern */
enum { AEFFT_RAW_U8 = 0, AEFFT_RAW_U16 = 1, AEFFT_RAW_PACKED = 2 };                                         /* container */
enum { AEFFT_DEMOSAIC_BILINEAR = 0, AEFFT_DEMOSAIC_MHC = 1 };
typedef struct {
    int pattern, container, bits;      /* bits: 8 (U8); 9..16 (U16, little endian, value in the low bits); 10 or 12 (PACKED) */
    int W, H;                          /* 4..8192 each, odd sizes included */
    const void* data;                  /* device pointer, ANY alignment (U16: a multiple of 2) */
    size_t pitch, stride;              /* bytes per row; image b at data + b * stride, ignored when B == 1 */
    int black, white;                  /* 0 <= black < white <= 2^bits - 1 */
    float gain[3];                     /* R, G, B (MONO: gain[0]); finite, 0..64 */
    int method;
    const float* ccm;                  /* HOST float[9], row-major, out = ccm * (R,G,B); nullable = identity; |entry| < 4; ignored for MONO */
    const unsigned char* lut_d;        /* DEVICE, 4096 bytes, nullable; any alignment */
} aefft_raw_desc;
int aefft_raw_to_image(aefft_ctx* ctx, const aefft_raw_desc* src, int order /* AEFFT_YUV_BGR | _RGB; MONO: ignored, D = 1 */,
                       unsigned char* image_d, size_t pitch, size_t image_stride, int B);

/* aefft_map_stats_update, aefft_map_stats_merge, aefft_map_stats_finish, aefft_map_peak: the baseline aefft_map_regions subtracts (its ref_d, "a
 * calibration map from nominal footage") learned on the device -- streaming per-cell statistics of the maps of nominal footage, the merge of two
 * such states, the baseline map out of a state, and the per-image peak of map - ref, which is both the image-level anomaly score and the number a
 * threshold is chosen from.  Without them a caller pulls every nominal map to the host, behind a copy and a synchronisation.
 * Maps are float [B][Mx][My], My contiguous -- the layout the map calls write; a cell is (I, J) with the linear index I * My + J; n = Mx * My.
 * Mx, My in 1..1024; B >= 1 and B * Mx * My <= 2^31 - 1; every pointer 16-byte aligned.
 * The state is caller-owned device memory of aefft_map_stats_bytes(Mx, My) bytes: 52 * Mx * My rounded up to a multiple of 16 (0 from the query
 * means sizes the calls do not take).  Its layout is planar and part of the interface:
 *   [0, 8n)     double S1[n]      the sum of the counted values
 *   [8n, 16n)   double S2[n]      the sum of their squares
 *   [16n, 32n)  float hi[4][n]    the largest values seen, hi[0] the largest
 *   [32n, 48n)  float lo[4][n]    the smallest values seen, lo[0] the smallest
 *   [48n, 52n)  int c[n]          the number of values counted
 * All-zero bytes are the empty state: there is no reset call, hipMemsetAsync starts a calibration.  Only the first min(c, 4) slots of hi and lo
 * are live; the others hold +0.0f, so that the hi, lo and c bytes of a state are a function of the multiset of values alone, whatever order the
 * footage arrived in.  The total number of frames per cell is the caller's bound: c <= 2^31 - 1.
 *   1. aefft_map_stats_update.  Per cell, for b = 0 .. B-1 in ascending order: x = map[b][I][J].  A non-finite x (NaN, +inf, -inf) is skipped
 *      and not counted; -0 counts as +0; otherwise S1 = S1 + (double)x, S2 = S2 + (double)x * (double)x, c = c + 1, each sum rounded once, and x
 *      enters hi if it is among the four largest seen so far and lo if it is among the four smallest.  Multiplicity is kept: equal values occupy
 *      several slots.  The product of two floats is exact in double, so S2's bits do not depend on whether the product is fused into the addition.
 *      The state is updated in place.
 *   2. aefft_map_stats_merge.  Per cell: S1 = S1_dst + S1_src and S2 alike, one addition each; c = c_dst + c_src; hi is the four largest of the
 *      up to eight live values, lo the four smallest; dead slots end up +0.0f.  src is only read; dst and src must not overlap.  hi, lo and c of
 *      a merged state equal those of one run over all the footage; S1 and S2 are the sums in the order the merge defines.
 *   3. aefft_map_stats_finish writes ref_d, float [Mx][My], exactly what aefft_map_regions takes.  In both modes a cell with c == 0 gets `empty`,
 *      which is any float: +inf under ABOVE switches the cell off, as map - inf is never foreground.
 *      AEFFT_CALIB_RANK: rank in 1..4, r = min(rank, c); ref = hi[r-1] under AEFFT_REGIONS_ABOVE, lo[r-1] under AEFFT_REGIONS_BELOW -- the
 *      per-cell maximum (minimum) of the nominal footage with rank - 1 outliers tolerated.  No arithmetic: exact, and independent of the order
 *      the footage arrived in.  k is ignored but must be finite.
 *      AEFFT_CALIB_SIGMA: k is a finite float, negative for BELOW; sense and rank are ignored but must be valid values.  In double, each
 *      operation rounded once, in this order: mean = S1 / (double)c.  If c == 1, sd = 0; otherwise p = S1 * mean, d = S2 - p, d = d < 0 ? 0 : d,
 *      var = d / (double)(c - 1), sd = sqrt(var), correctly rounded.  t = (double)k * sd.  ref = (float)(mean + t).  p and t are rounded products:
 *      neither is fused into the subtraction or addition it feeds.
 *      The accepted limit of the S2 - S1^2 / c form: the variance loses about log2(mean^2 / var) of double's 53 bits to cancellation.  That is
 *      fine for error and SSIM maps (values up to 65025 that vary by more than a millionth of their mean keep a dozen bits or more); it is not a
 *      general-purpose variance.
 *   4. aefft_map_peak.  v is exactly aefft_map_regions' step 1: map[b][I][J] when ref_d is NULL, otherwise map[b][I][J] - ref[I][J], rounded once
 *      to float32; a -0 result counts as +0.  peak[b] is the maximal v under AEFFT_REGIONS_ABOVE and the minimal v under AEFFT_REGIONS_BELOW over
 *      the cells whose v is not NaN (+inf and -inf are ordinary values); cell[b] is the smallest linear index I * My + J that attains it.  An
 *      image of NaN only gives peak = NaN (the quiet NaN 0x7FC00000) and cell = -1.  peak_d: float [B]; cell_d: int [B].
 * One launch each on the context's stream: a lane owns a cell and walks b (update: the order of the sums is the definition, nothing reduces over
 * b in parallel), or a workgroup owns an image and reduces an order-preserving 64-bit key by integer max (peak).  No atomics, no float
 * reduction, no workspace, no host synchronisation, no allocation; safe under stream capture; the result is a function of the inputs alone, on
 * every run.  The peak is sized for the common maps, up to 240 x 135 cells an image; larger maps are served, one workgroup an image.  Accounted
 * under the profile id `image` with 4 B n + 104 n bytes (update), 156 n (merge), 56 n (finish) and 4 B n (+ 4 n with ref_d) + 8 B (peak).
 * AEFFT_EINVAL, with aefft_last_error starting with the call's name ("aefft_map_stats_update: ", "aefft_map_stats_merge: ",
 * "aefft_map_stats_finish: ", "aefft_map_peak: ") and naming the rule, nothing enqueued and every output and the state untouched: a null context
 * or pointer (ref_d of aefft_map_peak may be NULL); Mx, My outside 1..1024; B < 1 or B * Mx * My beyond an int; a pointer that is not 16-byte
 * aligned; stats_bytes below the query; an unknown mode or sense; rank outside 1..4; a non-finite k; outputs that overlap inputs or each other
 * (the state and the map, dst and src, the state and ref_d, peak_d and cell_d and the peak's inputs). */
enum { AEFFT_CALIB_SIGMA = 0, AEFFT_CALIB_RANK = 1 };   /* mode of aefft_map_stats_finish */
size_t aefft_map_stats_bytes(int Mx, int My);           /* 52 * Mx * My rounded up to 16; 0 on invalid sizes */
int aefft_map_stats_update(aefft_ctx* ctx, const float* map_d, int Mx, int My, int B, void* stats_d, size_t stats_bytes);
int aefft_map_stats_merge(aefft_ctx* ctx, void* dst_d, const void* src_d, int Mx, int My, size_t stats_bytes);
int aefft_map_stats_finish(aefft_ctx* ctx, const void* stats_d, size_t stats_bytes, int Mx, int My, int mode, int sense /* AEFFT_REGIONS_* */,
                           float k, int rank, float empty, float* ref_d /* [Mx][My] */);
int aefft_map_peak(aefft_ctx* ctx, const float* map_d, const float* ref_d /* nullable, [Mx][My] */, int Mx, int My, int B, int sense,
                   float* peak_d /* [B] */, int* cell_d /* [B] */);

/* aefft_image_warp_affine, aefft_image_remap: align and rectify -- the geometric stage in front of the per-cell chain (aefft_image_compare_map,
 * the calibrated baseline, aefft_map_peak, aefft_map_regions), which assumes that the scene sits on the same pixels in every image.  The lens and
 * the camera's view of the plane are fixed calibrations, one per-pixel table for every frame (aefft_image_remap); the part arrives shifted and
 * rotated, one affine per image from a fiducial, an encoder or a matcher (aefft_image_warp_affine).
 * Images: source and destination are interleaved 8-bit images with the layout and rules of aefft_image_resize_to_frames -- pixel (row y, column
 * x), channel d, is the byte at  y * pitch + x * D + d; pointer, pitch and stride may have ANY alignment; pitch >= W * D; for B > 1,
 * stride >= (H - 1) * pitch + W * D (ignored when B == 1); bytes of a row beyond W * D are never read or written.  Source and destination each
 * have their own size (Ws, Hs / Wd, Hd), pitch and stride.  D in 1..4; Ws, Hs, Wd, Hd in 1..8192; B >= 1.  Out of place: source and destination
 * byte ranges must not overlap.
 * Direction: the transform maps a DESTINATION pixel to the source position it samples -- cv::warpAffine with WARP_INVERSE_MAP, and cv::remap.
 * Integer coordinates are pixel centres.  NOT byte-identical to OpenCV, which keeps 5 fraction bits of the position where this keeps 11; the
 * difference is unmeasured (OpenCV was not available to the build).
 * Source position in Q11: both calls reduce to a pair (tx, ty) of signed 32-bit integers per destination pixel, the source position times 2048.
 *   aefft_image_remap reads the pair from the table  int map[Hd][Wd][2], x first, 16-byte aligned, shared by all B images.  Any int32 value is
 *     legal.
 *   aefft_image_warp_affine computes it from aefft_affine: six coefficients in Q24 (48 bytes), on the device, 16-byte aligned; nm of them, nm == 1
 *     (shared by the batch) or nm == B (one per image).  For destination column x and row y:  U = a[0] x + a[1] y + a[2]  and
 *     V = a[3] x + a[4] y + a[5]  in wrapping 64-bit arithmetic;  tx = clamp((U + 2^12) >> 13, -2^31, 2^31 - 1)  with an arithmetic shift, ty the
 *     same from V.  The host cannot see the coefficients: the wrap and the clamp make the call defined for every bit pattern, and whatever the
 *     coefficients are, no byte outside the source images is read, because every index passes the border rule.  Within the ranges that
 *     aefft_affine_make accepts neither the wrap nor the clamp is ever active (|tx| stays below 2^30 + 2^27 at x, y = 8191).
 *   aefft_affine_make (host arithmetic only, like aefft_tile_plan_make): a[k] = m[k] * 2^24 rounded to nearest, ties to even, for the row-major
 *     2 x 3 matrix m.  AEFFT_EINVAL, with nothing written, for a null pointer, a non-finite entry, |a[0]|, |a[1]|, |a[3]|, |a[4]| > 2^29 (a scale
 *     of 32) or |a[2]|, |a[5]| > 2^39 (an offset of 32768 pixels).  Q24 keeps a rotation's error over 8192 pixels below 2^-11 pixel; Q16 would not.
 * Sampling, per axis with S = Ws or Hs:
 *   AEFFT_WARP_NEAREST  sx = (tx + 1024) >> 11 (halves up), rows alike.  One tap.
 *   AEFFT_WARP_LINEAR   sx = tx >> 11 and wx = tx & 2047, rows alike.  The taps are (sy, sx), (sy, sx+1), (sy+1, sx), (sy+1, sx+1):
 *     v = (2048-wy) ((2048-wx) p00 + wx p01) + wy ((2048-wx) p10 + wx p11)  < 2^30;  the byte is (v + 2^21) >> 22 -- the resize's weights and
 *     rounding.
 * Border: the rule is applied to each tap on its own, per axis.
 *   AEFFT_BORDER_CONSTANT   a tap with sx outside 0..Ws-1 or sy outside 0..Hs-1 has the value (border_value >> 8 d) & 255 for channel d.
 *   AEFFT_BORDER_REPLICATE  clamp(s, 0, S-1).
 *   AEFFT_BORDER_REFLECT    reflection without repeating the edge pixel (OpenCV's BORDER_REFLECT_101), iterated so that it is defined for any
 *     reach: for S = 1 the result is 0; otherwise P = 2(S-1), m = s mod P taken non-negative, r = m when m < S, else P - m.
 *   border_value is ignored under the other two rules.
 * Consequences, for both interpolations and all three borders: the identity gives the source's bytes; an integer translation gives the shifted
 * bytes, with the border rule in the uncovered strip; the quarter turns are exact -- {0, 1, 0, -1, 0, Hs-1} gives the source turned clockwise
 * (numpy's rot90(src, -1): dst[y][x] = src[Hs-1-x][y]) and {0, -1, Ws-1, 1, 0, 0} the source turned counter-clockwise (rot90(src, 1)), both
 * into a destination of Hs x Ws --; a half-pixel offset between bytes 10 and 20 gives 15; a transform that lands entirely outside the
 * source gives the constant everywhere; aefft_image_remap with the table (tx, ty) of an affine equals aefft_image_warp_affine with that affine,
 * byte for byte.
 * Both device calls: one launch each on the context's stream; no host synchronisation, no allocation, no workspace, no atomics; safe under
 * stream capture.  Every accepted alignment gives the same bytes (destination pointer, pitch and stride multiples of 4: dword stores; bytes
 * otherwise).  Accounted under the profile id `image` with B D (Ws Hs + Wd Hd) bytes plus 48 nm for the affines or 8 Wd Hd for the table.
 * AEFFT_EINVAL, with aefft_last_error starting with the call's name ("aefft_image_warp_affine: ", "aefft_image_remap: ") and naming the rule,
 * nothing enqueued and the destination untouched: a null context or pointer; D, B or a size out of range; nm not 1 or B; an unknown interp or
 * border; a pitch or stride that is too small; m_d or map_d not 16-byte aligned; the destination overlapping the source, the affines or the
 * table; sizes that overflow the address space. */
enum { AEFFT_WARP_NEAREST = 0, AEFFT_WARP_LINEAR = 1 };
enum { AEFFT_BORDER_CONSTANT = 0, AEFFT_BORDER_REPLICATE = 1, AEFFT_BORDER_REFLECT = 2 };
typedef struct { long long a[6]; } aefft_affine;   /* Q24: a[k] = m[k] * 2^24 of the row-major 2 x 3 matrix (destination -> source) */
int aefft_affine_make(const double m[6], aefft_affine* out);   /* host arithmetic */
int aefft_image_warp_affine(aefft_ctx* ctx, const unsigned char* src_d, size_t src_pitch, size_t src_stride, int Ws, int Hs,
                            const aefft_affine* m_d, int nm, int interp, int border, unsigned border_value,
                            unsigned char* dst_d, size_t dst_pitch, size_t dst_stride, int Wd, int Hd, int B, int D);
int aefft_image_remap(aefft_ctx* ctx, const unsigned char* src_d, size_t src_pitch, size_t src_stride, int Ws, int Hs,
                      const int* map_d, int interp, int border, unsigned border_value,
                      unsigned char* dst_d, size_t dst_pitch, size_t dst_stride, int Wd, int Hd, int B, int D);

/* aefft_frames_register_ref, aefft_frames_register: estimate the shift by phase correlation -- the pose that aefft_image_warp_affine consumes,
 * computed on the device with the library's own transforms against a stored reference spectrum.  Translation only; rotation and scale are not
 * estimated.
 * Inputs: frames [B][D][Nx][Ny], 8-bit (frames_u8) or float, 16-byte aligned; axis i is the image column and axis j the image row, as
 * aefft_image_to_frames defines them.  D in 1..4, B >= 1, B Nx Ny < 2^29; Nx and Ny are sizes the per-bin ops accept: powers of two in 8..2048 or
 * even smooth sizes in 10..2048.
 * Steps:
 *   1. prepare      g[b][i][j] = wx[i] wy[j] sum_d p[b][d][i][j] in float.  AEFFT_REGISTER_HANN: the periodic Hann window
 *                   w[n] = 0.5 - 0.5 cos(2 pi n / N).  AEFFT_REGISTER_NOWINDOW: w = 1, for periodic content (and the exact case below).
 *   2. transform    G = r2c(g), unnormalised, [Nx][Ny/2+1] complex, by the route aefft_r2c takes on that grid.  aefft_frames_register_ref stops
 *                   here: spec_d receives G of each of the nref frames.
 *   3. cross-power  R = G_img conj(G_ref) per bin; Q = R / |R| where the bin is kept and |R| > 0, otherwise Q = 0.  A bin (u, v) (signed
 *                   frequencies) is kept when 2|u| <= cutoff Nx and 2|v| <= cutoff Ny and it is not in the dropped low set: the DC bin alone
 *                   under NOWINDOW, the nine bins with |u| <= 1 and |v| <= 1 under HANN (a Hann-windowed constant has its whole spectrum in
 *                   those nine, so dropping them removes the image mean's pull toward zero shift without a pass over the image).  cutoff is a
 *                   float in (0, 1].  K is the number of kept bins of the FULL Nx x Ny spectrum: host arithmetic, independent of the data.
 *   4. surface      s = c2r(Q) / K (scale = 1 / K in the transform).  A pure circular shift whose kept bins are all non-zero gives 1 at one
 *                   cell and (nearly) 0 elsewhere.
 *   5. peak         the largest s[b][i][j], the smallest index i Ny + j on ties (-0 counts as +0, a NaN is no candidate), at (pi, pj).  Over
 *                   its 5 x 5 circular neighbourhood with weights w = max(s, 0), accumulated in double in ascending (di, dj):
 *                   cx = sum w di / sum w, cy alike over dj (0 when sum w is 0).  dx = pi + cx, reduced by Nx when >= Nx / 2; dy alike with
 *                   Ny; response = s[pi][pj]; cell = pi Ny + pj.  One aefft_shift (16 bytes) per image.
 *   6. affine       (affine_d non-null) with the host doubles scale_x, scale_y -- image pixels per frame cell, each in (0, 32] --: when
 *                   response >= min_response (false for NaN)  a = {2^24, 0, rint((double)dx scale_x 2^24), 0, 2^24, rint((double)dy scale_y 2^24)},
 *                   otherwise the identity {2^24, 0, 0, 0, 2^24, 0}.  rint is to nearest, ties to even, in double, on the device; the offsets
 *                   stay within aefft_affine_make's 2^39.
 * Sign: if the image is the reference moved by +d, img(x) = ref(x - d), then (dx, dy) = +d; the affine maps destination to source,
 * src = dst + d, so aefft_image_warp_affine with it puts the image back on the reference's pixels.  Example: frames = np.roll(ref, 3, axis=-2)
 * gives dx = 3, dy = 0 and a[2] = 3 * 2^24.
 * Non-finite float frames give unspecified numbers; cell is always inside the grid and nothing is read or written out of range.
 * Reference: ref_spec_d holds nref spectra as aefft_frames_register_ref wrote them with the same Nx, Ny and window; nref == 1 (shared by the
 * batch) or nref == B (one per image).
 * Workspace: work_d is the caller's, 16-byte aligned, at least aefft_register_workspace(Nx, Ny, B) bytes (nref for B in
 * aefft_frames_register_ref): round16(4 B Nx Ny) for the windowed planes, which the surface reuses, + round16(8 B Nx (Ny/2+1)) for the image
 * spectra + round16(8 B ceil(Nx Ny / 4096)) for the peak partials.  The transforms take the context's transform workspace exactly as aefft_r2c
 * does: the first call at a new size may allocate (and, on a smooth axis size, build that size's table), so it must not be the first one made
 * under stream capture; later calls are safe under capture.
 * Both calls: launches on the context's stream only -- prepare, the transform, and for aefft_frames_register the cross-power, the inverse
 * transform and a two-stage peak (many workgroups an image write partials, one finishes); no host synchronisation, no atomics, no workgroup
 * waits for another; the same inputs give the same bytes from run to run.  The three kernels are accounted under the profile id `image`, the
 * transforms under their own ids.
 * AEFFT_EINVAL, with aefft_last_error starting with the call's name ("aefft_frames_register: ", "aefft_frames_register_ref: ") and naming the
 * rule, nothing enqueued and the outputs untouched: a null context or required pointer (affine_d may be NULL); D, B, nref or a size out of
 * range; an unknown window; cutoff outside (0, 1] or NaN; a cutoff that keeps no bin (K = 0); a scale outside (0, 32] or non-finite; a pointer
 * that is not 16-byte aligned; work_bytes too small; outputs that overlap inputs, the workspace or each other. */
enum { AEFFT_REGISTER_HANN = 0, AEFFT_REGISTER_NOWINDOW = 1 };
typedef struct { float dx, dy, response; int cell; } aefft_shift;
size_t aefft_register_spec_floats(int Nx, int Ny);          /* 2 Nx (Ny/2+1); 0 on invalid sizes */
size_t aefft_register_workspace(int Nx, int Ny, int B);     /* bytes; 0 on invalid sizes */
int aefft_frames_register_ref(aefft_ctx* ctx, const void* frames_d, int frames_u8, int nref, int D, int Nx, int Ny, int window,
                              float* spec_d /* [nref][Nx][Ny/2+1] complex */, void* work_d, size_t work_bytes);
int aefft_frames_register(aefft_ctx* ctx, const void* frames_d, int frames_u8, int B, int D, int Nx, int Ny, int window,
                          const float* ref_spec_d, int nref /* 1 or B */, float cutoff, float min_response,
                          double scale_x, double scale_y, aefft_shift* shift_d, aefft_affine* affine_d /* nullable */,
                          void* work_d, size_t work_bytes);

/* ---- network level: the resident, batched form of autoenc_fft / backprop_fft ------------------ */
typedef struct {
    int D, Nx, Ny;        /* input frames [B][D][Nx][Ny] */
    int npairs;           /* L encoder/decoder pairs (net_c holds 2L kernels, autoencoder.cpp:115-116,414-417) */
    const int* maps;      /* [L] feature maps dM of each pair */
    const int* Nk;        /* [L] kernel rows */
    const int* Nl;        /* [L] kernel cols */
    const int* scale;     /* [L] pooling scale s>=1 of each pair (decoder mirrors with -s, autoencoder.cpp:119-120) */
    int batch;            /* frames per call on this GPU */
} aefft_net_desc;

int aefft_net_create(aefft_ctx* ctx, const aefft_net_desc* desc, aefft_net** out);
/* aefft_net_create with options.  opts = 0 is exactly aefft_net_create.  AEFFT_NET_SMOOTH_SIZES: Nx, Ny may also be smooth sizes
 * (even, 10..2048, no prime factor above 5: 640 x 480, 1280 x 720, ...), mixed freely with power-of-two axes; every pair's pooled grid
 * must be even and >= 8 (pooling scales powers of two, kernels no larger than the grid as always) -- AEFFT_EINVAL names the rule otherwise
 * (480 over 5 pairs of scale 2: the 5th grid is 15).  A net with a smooth axis runs every step in the per-frame form unless it was also
 * created with AEFFT_NET_SMOOTH_OPFORM: aefft_net_step_form returns AEFFT_FORM_PER_FRAME; a power-of-two net
 * created with the option runs exactly as one from aefft_net_create.  Every aefft_net_* entry
 * point works on it, and the net sizes all its workspaces here.
 * AEFFT_NET_SMOOTH_OPFORM (with AEFFT_NET_SMOOTH_SIZES): a net with a smooth axis runs aefft_net_step_grad / _apply in the operator form
 * when it meets that form's other rules -- at most 3 input channels, every pair the same square 3x3 or 5x5 support, dD <= 256, dM <= 512,
 * dD + dM <= 1024, Ny/2+1 <= 320 on every pair's grid -- and in AEFFT_FORM_OPERATOR_CHAIN when in addition the coarsest grid has at most
 * 16384 bins and every dD, dM <= 128 (AEFFT_FORM_OPERATOR otherwise, and under AEFFT_F_NOCHAIN and its companions); aefft_net_step_form
 * reports the form the net runs in.  A net that does not meet the rules (7x7 or 5x3 kernels, 4 input channels) runs in the per-frame form
 * exactly as without the option.  AEFFT_F_NOOPFORM, AEFFT_F_NOQPATH and AEFFT_F_NOPRUNESMOOTH (the operator form needs the pruned kernel
 * transforms) force the per-frame form, also on a live net.  The option has no effect on a power-of-two net, on a spatial net, or
 * without AEFFT_NET_SMOOTH_SIZES (a smooth size then stays AEFFT_EINVAL). */
enum { AEFFT_NET_SMOOTH_SIZES = 1u << 0, AEFFT_NET_SPATIAL = 1u << 1, AEFFT_NET_SMOOTH_OPFORM = 1u << 2 };
/* AEFFT_NET_SPATIAL: the reference's coordinate-space training mode (autoencoder.cpp:135-150,171-201: Pool -> Conv_gpu per encoder,
 * Conv_gpu -> Pool(-s) per decoder, backprop_gpu / backprop_gpu_cc per pair) as a resident, batched net, with GPU semantics throughout
 * (cpu_semantics = 0 of the spatial ops above).  Same descriptor.  Any Nx, Ny; every pair's scale is an integer >= 1 that divides its
 * input grid EXACTLY (Pool(-s) with a remainder reads past its input in the reference, netlib.cpp:141-162) and every pooled grid is at
 * least the pair's kernel support -- AEFFT_EINVAL naming the rule and the pair otherwise (66 x 66 over two pairs of scale 2: pair 1 has
 * 33 x 33).  Kernel supports: whatever aefft_step_spatial takes.  AEFFT_NET_SMOOTH_SIZES together with it is accepted and has no effect.
 * Layers, pair l on the grid G_l = G_{l-1} / s_l: 2l+1 = Pool(2l, s_l), 2l+2 = Conv_gpu(2l+1; c_l, b_l), 4L-1-2l = Conv_gpu(4L-2-2l; f_l, p_l),
 * 4L-2l = Pool(4L-1-2l, -s_l); layer 4L is the reconstruction.  On such a net:
 *   aefft_net_forward       the forward (recon_d nullable).
 *   aefft_net_step_grad     the forward, then for EVERY pair backprop_gpu's gradients as the batch mean with in = layer 2l+1, out = layer
 *                           4L-1-2l (the whole network's decoder output at that grid, autoencoder.cpp:161-169,174 with q = 1), hin = layer
 *                           2l+2, normalised with the untied Norm = dD*dM*Nk*Nl*Nx*Ny, into the packed buffer in the FFT nets' layout;
 *                           its tail slot l holds sum (in - out)^2 / Norm, the mean over this rank's frames, BEFORE the update
 *                           (backproplib.cu:346-356).  The same inputs give the same buffer bit for bit.
 *   aefft_net_step_apply    backprop_gpu's update of every pair with its own momentum, d <- (1-alpha)*del0*g/max(10,|g|) + alpha*d,
 *                           w <- w - d, g = buffer * grad_scale: del0 IS delmax (autoencoder.cpp:87,178 pass `del` straight through, no
 *                           0.1 factor as in FFT mode); alpha: aefft_net_set_inertia.  sym = 1 is backprop_gpu_cc (backproplib.cu:521-644):
 *                           gradients and MSE halved (Norm x 2, :533), g = gc + gf^T, f = c^T exactly afterwards.  maxdiff != 0:
 *                           AEFFT_EINVAL (no multiobjective term).  The tail x grad_scale (x 1/2 with sym) replaces the tail and goes to
 *                           mse_d (nullable) and behind the buffer, and aefft_net_last_mse returns it: after the all-reduce it is the
 *                           global-batch PRE-update MSE of THIS step -- not one step behind as in FFT mode -- and, as on an FFT net, a
 *                           further all-reduce of the tail times 1/world gives that mean again.
 *   aefft_net_get_layer(s), aefft_net_layers_layout: every layer 0..4L of the last forward / step_grad (the pre-update weights); the
 *                           up-sampled decoder layers 4L-2l are not kept and are formed on request (Pool(-s)).
 *   npairs, pair_shape, set_pair, get_pair, reset_momentum, grad_buffer, last_mse, step_form (AEFFT_FORM_SPATIAL): as on any net.
 *   pair_spectra, store_spectra, load_spectra (no spectra), train_pair, step_grad_u8, forward_u8, set_input_ready(1): AEFFT_EINVAL.
 * The development switches AEFFT_F_NOTILEDSPATIAL and AEFFT_F_NORCORR select the fallback routes, as at op level. */
int aefft_net_create_ex(aefft_ctx* ctx, const aefft_net_desc* desc, unsigned opts, aefft_net** out);
void aefft_net_destroy(aefft_net* net);
/* the descriptor back: number of pairs (negative for a null net); channels / maps / kernel support of pair l (any pointer nullable) */
int aefft_net_npairs(aefft_net* net);
int aefft_net_pair_shape(aefft_net* net, int l, int* dD, int* dM, int* Nk, int* Nl);
/* weights of pair l (host pointers, reference layouts).  set = the caller's net_cfreq.clear():
 * spectra are rebuilt from c,f (fft_backproplib.cu:1148-1158). */
int aefft_net_set_pair(aefft_net* net, int l, const float* c_h, const float* b_h, const float* f_h, const float* p_h);
int aefft_net_get_pair(aefft_net* net, int l, float* c_h, float* b_h, float* f_h, float* p_h);
/* device views of the cached kernel spectra (C [dM][dD][P], F [dD][dM][P]) of pair l */
int aefft_net_pair_spectra(aefft_net* net, int l, float** C_d, float** F_d);
/* the caller-side `net_cfreq` cache (fft_backproplib.cu:1117-1141 store_cfreq / load_cfreq): host
 * copies of the spectra, interleaved floats in the reference layout.  load makes the spectra the
 * source of truth and re-derives c, f from them (export_cfreq, :1166). */
int aefft_net_store_spectra(aefft_net* net, int l, float* C_h, float* F_h);
int aefft_net_load_spectra(aefft_net* net, int l, const float* C_h, const float* b_h, const float* F_h, const float* p_h);

/* fft_backproplib.cu:1331-1376 `autoenc_fft` over a batch.  frames_d [B][D][Nx][Ny];
 * recon_d (nullable) receives layers.back().  All intermediate spectra stay resident. */
int aefft_net_forward(aefft_net* net, const float* frames_d, float* recon_d);
/* fft_l=1 semantics (:1347,1357,1361): coordinate-space copy of reference layer index `layer`
 * (autoencoder.cpp:110-114 ordering, 0..4L) from the last forward.  out_d [B][ch][nx][ny];
 * ch/nx/ny (nullable) receive its shape.  Pass out_d=NULL to query the shape only.
 * After aefft_net_step_grad (with or without the following aefft_net_step_apply) the layers are those of THAT step's forward, i.e. of the
 * weights before the update.  What they are formed from depends on the step form (aefft_net_step_form):
 *   OPERATOR_CHAIN  the resident input spectra and the step's stored operators -- neither the caller's frame buffer nor the current
 *                   weights enter (layer 0, the input itself, is copied from the frame buffer of the last step_grad / forward);
 *   OPERATOR        the per-frame forward of the frames of the last step_grad is re-run with the CURRENT weights: the caller's frame buffer
 *                   must still hold them, and after aefft_net_step_apply the layers are those of the updated weights;
 *   PER_FRAME       the spectra of the step's forward as stored.
 * A HIDDEN layer (even index <= 2L) that the training step did not materialise is formed on request from the pair's input of the step and
 * the encoder of THAT step: in the OPERATOR_CHAIN form after aefft_net_step_apply the pre-update encoder is recovered as w + D (the update was
 * w <- w - D and D stays in the momentum buffer: exact to one rounding), so every layer of one export belongs to the same weight set; in
 * the other two forms from the pair's CURRENT encoder (PER_FRAME before step_apply, OPERATOR as described above). */
int aefft_net_get_layer(aefft_net* net, int layer, float* out_d, int* ch, int* nx, int* ny);

/* fft_l = 1 in one call: EVERY layer 0..4L of the last forward, coordinate space, packed into out_d at the
 * offsets aefft_net_layers_layout reports (floats; offsets_h[4L+1] = total).  Each layer is one inverse transform of the spectrum
 * where it is stored (spectral crop / zero-pad fused); hidden layers the training step skipped are formed first. */
int aefft_net_layers_layout(aefft_net* net, size_t* offsets_h /* [4L+2] */);
int aefft_net_get_layers(aefft_net* net, float* out_d);
/* fft_backproplib.cu:27-63 `magnitude` + `shift_magnitude` (the reference's spectrum display path, dead in its main()):
 * mag[d][i][j] = sqrt(|X[d][i][j]| / (ch*Nx*Ny)) on the half-plane j < Nyr, the mirrored element
 * X[d][Nx-1-i][2*Nyr-1-j] beyond it (the reference's index arithmetic, :53), shift != 0: quadrants swapped so that the zero
 * frequency sits in the centre (:33-36).  X_d [planes][Nx][Nyr] -> mag_d [planes][Nx][Ny]; ch = channels per frame. */
int aefft_magnitude(aefft_ctx* ctx, const float* X_d, float* mag_d, long planes, int ch, int Nx, int Ny, int shift);

/* fft_backproplib.cu:1381-1511 `backprop_fft` burst on pair l, using the spectra of the last
 * forward as in / expout(=in) / out (autoencoder.cpp:169,194): zeroes the momentum (:1420-1423),
 * del = 0.1*del0 (:1445), n_iter iterations (reference: 100, :1446) of gradient -> update ->
 * re-forward -> mse.  mse_h (nullable) receives n_iter+1 values (initial, then one per
 * iteration, :1440,1463); blocks until done when mse_h != NULL. */
int aefft_net_train_pair(aefft_net* net, int l, int n_iter, float del0, int maxdiff, int sym, float* mse_h);

/* One data-parallel training step = forward + ONE loop-body iteration for every pair
 * (SURVEY 8d "one frame fwd+bwd"), split so the caller can all-reduce in between:
 *   step_grad : forward (recon_d nullable: layers.back()), then per pair the batch-mean gradient of the
 *               first loop-body iteration (fft_backproplib.cu:1454-1456: gradient_k_io on the forward's
 *               in / out spectra, C2R, shrink_k) -> packed buffer [dck | dfk | db | dp] per pair, pairs
 *               concatenated.
 *   (caller: all-reduce SUM of aefft_net_grad_buffer over ranks)
 *   step_apply: gradients * grad_scale (1/world_size), update (:1229-1272), new kernel spectra
 *               (:1274-1282), post-update MSE of each pair's own re-forward (:1460-1463).
 *               mse_d (nullable): [L] floats on the device.
 * Same sums as the reference, re-associated; intermediate layers that the
 * reference itself never exports (fft_l = 0) are formed on demand by aefft_net_get_layer.
 * Momentum persists across steps (reset with aefft_net_reset_momentum). */
int aefft_net_step_grad(aefft_net* net, const float* frames_d, float* recon_d);
/* The same calls on 8-BIT frames (frames_d [B][D][Nx][Ny] unsigned char, planar: what a camera delivers -- the reference's application turns each
 * 8-bit pixel into a float on the host, `(float)col[c]`, netlib.cpp:37-51 ImageToSpin_C, called at autoencoder.cpp:125): the input transform
 * converts on load, a quarter of its reads; results are those of the float call on the same pixel values, bit for bit.  Every frame size the net
 * itself takes: powers of two, and with AEFFT_NET_SMOOTH_SIZES the smooth sizes (the mixed-radix row pass converts on load as well);
 * 16-byte aligned.  aefft_net_get_layer(0) returns the pixels as floats. */
int aefft_net_step_grad_u8(aefft_net* net, const unsigned char* frames_d, float* recon_d);
int aefft_net_forward_u8(aefft_net* net, const unsigned char* frames_d, float* recon_d);
/* Training toward a TARGET frame -- supervised image-to-image training: denoising, deblurring, restoration.  The reference's entry point takes
 * three tensors, backprop_fft(in, expout, out, ..) (fft_backproplib.cu:1381-1463), and gradient_k_io (:395-475) reads the expected output only in
 * the error `ofreq - freqout`; the application passes expout = in, and its commented-out lines (autoencoder.cpp:126-127,192-193) show the
 * intended use: a second image as expout for the first pair, `if(n_l!=0) expout1=in_s` for the deeper ones.
 * The call is aefft_net_step_grad with one change: for PAIR 0 the expected output is T_b = pool_fft(fft(target_b), s_0), the target's spectrum
 * on pair 0's grid, instead of the pair's input X_0,b; the input role (freqin) stays X_0,b.  Pairs l >= 1 keep expout = in.  frames_d and
 * targets_d are [B][D][Nx][Ny], each float, or unsigned char when its _u8 flag is set (8-bit pixels convert on load as everywhere else; the
 * two may differ in type).  All pointers 16-byte aligned.  The forward pass, recon_d (nullable), the layers exported afterwards and the packed
 * buffer's layout are those of aefft_net_step_grad; a data-parallel caller all-reduces the same buffer.
 * The following aefft_net_step_apply is the existing call.  After a target step pair 0's post-update MSE is mse_fft(T, O') (:1463 with
 * freqo_d = the target) wherever it is reported: mse_d, the packed buffer's tail, aefft_net_last_mse, the deferred sums under mse_d = NULL.
 * The net remembers that the pending step has a target from this call until that step's aefft_net_step_apply, or any call that ends a pending
 * step; a plain aefft_net_step_grad clears it.
 * Every term of gradient_k_io is linear in the error, so with N_b = X_0,b - T_b (exactly zero when the target is the frame) the target enters
 * as S_0 += sum_b N_b X_b^H and es_0 += sum_b N_b(0,0) behind the launch that forms them, and as -2 Re(E^H N) + |N|^2 in pair 0's MSE sums
 * (DESIGN.md section 18): the target's input transform (never prefetched) and two short launches on top of the plain step, batch sums in a
 * fixed order with no atomics -- replicas of a data-parallel run keep bit-identical gradients.  With target == frames the gradients and the
 * updated weights are those of the plain step by value.
 * The call runs in whatever form aefft_net_step_form reports and under every development switch; everything it adds is ordered on the
 * context stream, also under aefft_net_set_input_ready(1).  The FIRST target call of a net allocates the target's workspaces (as
 * aefft_net_set_input_ready and the multiobjective buffers are allocated on first use): it must not be made under stream capture.  Later
 * calls allocate nothing and do not synchronise.
 * AEFFT_EINVAL, with nothing enqueued: a null net, null frames or null targets; a pointer not 16-byte aligned; a spatial net; D > 4 (frames
 * are images: grey, BGR, BGRA).  Not offered: targets for aefft_net_train_pair bursts (backprop_fft of the vector API takes expout) and for
 * pairs l >= 1.  (Judging such a net: aefft_net_score_target, aefft_net_score_map_target, aefft_net_ssim_map.) */
int aefft_net_step_grad_target(aefft_net* net, const void* frames_d, int frames_u8, const void* targets_d, int targets_u8, float* recon_d /* nullable */);
/* Frozen-weight inference over a batch -- the application's display loop (ImageToSpin_C, autoenc_fft, SpinToImage_C on every camera frame,
 * netlib.cpp:37-77, autoencoder.cpp:218-227): the reconstruction (layers.back() of autoenc_fft) and optionally ONE hidden layer, from the
 * CURRENT weights.  frames_d [B][D][Nx][Ny] float, or unsigned char when frames_u8; recon_d (nullable) [B][D][Nx][Ny] float, or
 * unsigned char when recon_u8 with SpinToImage_C's rule (netlib.cpp:66-68): clamp((int)round(v), 0, 255), halves away from zero,
 * NaN -> 0 (written by the inverse transform's row pass, four pixels per store); hidden_d (nullable) receives layer 2*hidden_pair+2,
 * float [B][dM][Nx_l][Ny_l].  All pointers 16-byte aligned.
 * The call runs in the form aefft_net_step_form reports.  OPERATOR / OPERATOR_CHAIN: the layers are evaluated as operators only when the
 * operators of the current weights are not at hand -- the first call, and after aefft_net_set_pair, aefft_net_load_spectra,
 * aefft_net_step_apply (whose last launch already carries the next chain in the chain form) or aefft_net_train_pair; any other call is
 * the input transform and the inverse transform with the operator applied on load (or written out first above 16 MB of output spectra),
 * nothing else.  The hidden layer is the operator H^_l = C_l A_l / dM + bias, cached with them and formed again when the weights or
 * hidden_pair change; the frames' spectra H^_l [x_b; 1] are written out by one launch and go through one inverse transform.  PER_FRAME: the per-frame forward in its lazy
 * form (bins a crop discards are not formed), the hidden layer formed on request as by aefft_net_get_layer.
 * State: as aefft_net_forward -- the call ends a pending aefft_net_step_grad (aefft_net_step_apply then fails with AEFFT_ESTATE), and
 * aefft_net_get_layer(s) afterwards export the layers of this call.  Training is not disturbed: operator sets, the chain carried ahead,
 * the double-buffered input spectra and the deferred MSE sums are left so that the next aefft_net_step_grad / _apply give bit for bit
 * what they would have given without the call.  Everything is ordered on the context stream, also under aefft_net_set_input_ready(1)
 * and the development switches that move the step's reconstruction to a side stream: the outputs are complete when the call's work is.
 * No host synchronisation, no allocation (sized by aefft_net_create*).
 * Spatial net: float frames and float outputs only (sp_forward; hidden_d from the stored layer); any 8-bit argument is AEFFT_EINVAL.
 * AEFFT_EINVAL: null net or frames, both outputs null, hidden_d with hidden_pair outside 0..L-1, a pointer not 16-byte aligned. */
int aefft_net_infer(aefft_net* net, const void* frames_d, int frames_u8, void* recon_d, int recon_u8, int hidden_pair, float* hidden_d);
/* Per-frame reconstruction error under the CURRENT (frozen) weights -- a validation curve on held-out frames, an anomaly score:
 *     score_d[b] = sum over d, i, j of (x_b[d][i][j] - r_b[d][i][j])^2 / (D Nx Ny)
 * x the frame as floats (8-bit pixels converted as everywhere else), r the float32 reconstruction aefft_net_infer would write for the same
 * frames and weights (layer 4L of autoenc_fft, fft_backproplib.cu:1331-1376).  frames_d [B][D][Nx][Ny] float, or unsigned char when
 * frames_u8; score_d [B] float; recon_d (nullable) float [B][D][Nx][Ny].  All pointers 16-byte aligned.
 * By Parseval this is mse_fft's sum (fft_backproplib.cu:480-498, :1178-1192) between layer 0 and layer 4L, times 2*dM -- for the whole
 * network instead of one pair, per frame instead of a batch mean, and with no weight update behind it.
 * The inverse transform's row pass holds every reconstructed pixel in registers just before it would store it: it loads the frame's pixels
 * for the same elements and forms the squared difference there, so the reconstruction need not reach memory.  The difference is formed from
 * the ROUNDED product z*scale, the value the row pass stores (the compiler is kept from contracting the product into the subtraction):
 * score_d is exactly a function of the float reconstruction, whether or not recon_d is given, and a trained net's small residual does not
 * depend on which variant ran.  recon_d, when given, receives the float reconstruction, bit for bit what aefft_net_infer writes, from the
 * same launch.  There is no 8-bit reconstruction here: callers that want pixels use aefft_net_infer.
 * Every frame's score is reduced in a fixed order, with no atomics: one float per pair of rows (the lane's terms in order, a butterfly
 * over the wave, the pair's waves in order), then the frame's D*Nx/2 row-pair sums in double.  The same inputs give the same bits, and a
 * frame's score does not depend on the other frames of the batch.
 * Form, caches, state and ordering are exactly those of aefft_net_infer (DESIGN.md sections 13 and 15): the call runs in the form
 * aefft_net_step_form reports and reuses the operators of the current weights where they are at hand (in the chain form five launches:
 * the input transform's two, the inverse column pass with the operator on load, the scoring row pass, the finish; one more above 16 MB of
 * output spectra); it ends a pending aefft_net_step_grad (aefft_net_step_apply then fails with AEFFT_ESTATE) and aefft_net_get_layer(s)
 * afterwards export the layers of this call; it leaves training bit for bit undisturbed; it runs on the context stream only, with no host
 * synchronisation and no allocation (sized by aefft_net_create*).
 * Routes whose reconstruction does not come out of one of the two row kernels -- the spatial net (float frames only), and smooth grids up to
 * 1024 x 1024 under AEFFT_F_CHIRPZ -- form the same row-pair sums from the STORED reconstruction in a launch of their own: they need recon_d.
 * AEFFT_EINVAL: null net, frames or score_d; a pointer not 16-byte aligned; frames_u8 on a spatial net; recon_d == NULL on one of the routes
 * just named (the message says why).  The outputs are then untouched. */
int aefft_net_score(aefft_net* net, const void* frames_d, int frames_u8, float* score_d, float* recon_d /* nullable */);
/* Per-tile reconstruction error under the CURRENT (frozen) weights -- WHERE in the frame the error is: one heat map over the image plane
 * per frame, channels summed.  With t = tile and map_d float [B][Nx/t][Ny/t]:
 *     map_d[b][I][J] = sum over d < D, i in [I t, I t + t), j in [J t, J t + t) of (x_b[d][i][j] - r_b[d][i][j])^2 / (D t t)
 * x and r are exactly those of aefft_net_score: 8-bit pixels converted exactly, r the ROUNDED product z*scale the float row pass stores, so
 * the map is a function of the float reconstruction whether or not recon_d is given.  tile is one of 8, 16, 32, 64 and must divide both Nx
 * and Ny (640 x 480 takes 8, 16, 32; 1280 x 720 takes 8, 16; a power-of-two grid every tile up to its shorter side).
 * score_d (nullable) [B] float: the mean of the frame's Nx/t * Ny/t map entries, taken from the float entries as stored, added in double
 * and rounded once -- a function of the map.  It agrees with aefft_net_score to rounding, NOT bit for bit: the two add the same terms in
 * different orders and round at different places.
 * recon_d (nullable) float [B][D][Nx][Ny] receives the float reconstruction, bit for bit what aefft_net_infer writes, from the same launch.
 * All pointers 16-byte aligned.
 * The inverse row pass's scoring epilogue with its reduction stopped early: one float per STRIP (two rows x t columns of one channel; the
 * lane's terms in order, then a butterfly over the strip's lanes of the wave), then score_map_finish_kernel adds an entry's D * t/2 strips
 * in double, channel outer, row pair inner, and rounds once.  There are no atomics: the same inputs give the same bits, and a frame's map
 * does not depend on the other frames of the batch.
 * Form, operator caches, state and ordering are exactly those of aefft_net_score: the form aefft_net_step_form reports; in the chain form
 * with the operators at hand five launches (the input transform's two, the inverse column pass with the operator on load, the mapping row
 * pass, the map finish), six with score_d; a pending aefft_net_step_grad is ended (aefft_net_step_apply then fails with AEFFT_ESTATE);
 * aefft_net_get_layer(s) afterwards export the layers of this call; training is left bit for bit undisturbed; the context stream only, no
 * host synchronisation and no allocation (the strip buffer, B*D*Nx*Ny/16 floats, is sized by aefft_net_create*).
 * The spatial net (float frames only) and smooth grids under AEFFT_F_CHIRPZ form the same strips from the STORED reconstruction in a
 * launch of their own: they need recon_d.
 * AEFFT_EINVAL: null net, frames or map_d; a pointer not 16-byte aligned; a tile that is not 8, 16, 32 or 64 or does not divide Nx and Ny;
 * frames_u8 on a spatial net; recon_d == NULL on one of the routes just named (the message says why).  The outputs are then untouched. */
int aefft_net_score_map(aefft_net* net, const void* frames_d, int frames_u8, int tile, float* map_d, float* score_d /* nullable */,
                        float* recon_d /* nullable */);
/* aefft_net_score and aefft_net_score_map against a TARGET -- the validation numbers of a net trained by aefft_net_step_grad_target (a
 * denoiser is judged against the clean frame, not against its noisy input).  They are exactly the two calls above with x replaced by the
 * target's pixels t_b[d][i][j] in (x - r)^2: the net still reads frames_d, the inverse row pass loads targets_d for the comparison.  frames_d
 * and targets_d are [B][D][Nx][Ny], each float, or unsigned char when its _u8 flag is set -- each on its own, as in
 * aefft_net_step_grad_target.  With targets_d == frames_d (and equal flags) they give the bits of the plain calls.
 * Everything else is that of the plain calls: form, operator caches, state, launch counts (no new kernel, no further launch), ordering,
 * determinism, training left bit for bit undisturbed, no allocation, and the routes that need recon_d.  A spatial net takes float frames and
 * float targets only.  The PSNR follows from score_d: 10 log10(L^2 / score_d[b]) with L the data range (255 for 8-bit images).
 * AEFFT_EINVAL, with the outputs untouched: what the plain calls refuse, and a null or misaligned targets_d. */
int aefft_net_score_target(aefft_net* net, const void* frames_d, int frames_u8, const void* targets_d, int targets_u8, float* score_d,
                           float* recon_d /* nullable */);
int aefft_net_score_map_target(aefft_net* net, const void* frames_d, int frames_u8, const void* targets_d, int targets_u8, int tile, float* map_d,
                               float* score_d /* nullable */, float* recon_d /* nullable */);
/* Block SSIM of the reconstruction under the CURRENT (frozen) weights -- the structural similarity index over non-overlapping windows, the
 * second number restoration quality is quoted in.  With
 *   x the reference pixels: the target, or the frame when targets_d == NULL (8-bit pixels converted exactly);
 *   r the ROUNDED float reconstruction, exactly the r of aefft_net_score;
 *   t = tile, one of 8, 16, 32, 64, which must divide both Nx and Ny, and n = t*t;
 *   L = data_range > 0 (255 for 8-bit images);
 * for every channel d and window (I, J) -- rows [I t, I t + t), columns [J t, J t + t) -- with uniform weights and population statistics:
 *     mx = sum x / n,  mr = sum r / n,  vx = max(sum x^2 / n - mx^2, 0),  vr = max(sum r^2 / n - mr^2, 0),  c = sum x r / n - mx mr
 *     C1 = (0.01 L)^2,  C2 = (0.03 L)^2
 *     ssim = (2 mx mr + C1)(2 c + C2) / ((mx^2 + mr^2 + C1)(vx + vr + C2))
 * map_d[b][I][J], float [B][Nx/t][Ny/t], is the mean over d < D of ssim.  score_d (nullable) [B] float is the mean of the frame's map entries,
 * taken from the floats as stored, added in double and rounded once -- a function of the map.  recon_d (nullable) float [B][D][Nx][Ny]
 * receives the float reconstruction, bit for bit what aefft_net_infer writes, from the same launch.  frames_d and targets_d are
 * [B][D][Nx][Ny], each float, or unsigned char when its _u8 flag is set (targets_u8 is ignored with targets_d == NULL).  All pointers 16-byte
 * aligned.
 * The mapping epilogue of the inverse row pass with five sums per STRIP (two rows x t columns of one channel) where the error map keeps one:
 * sum x', r', x'^2, r'^2, x'r' with x' = x - L/2, r' = r - L/2 -- the pivot keeps the float sums of squares small where a window is flat;
 * variances and the covariance do not depend on it, the finish adds it back to the means.  Each sum: the lane's terms in order, then a
 * butterfly over the strip's lanes of the wave.  ssim_finish_kernel then adds, per channel, the window's t/2 strips of each moment in double,
 * evaluates the formula in double, adds the channels in order, scales by 1/D and rounds once.  There are no atomics: the same inputs give
 * the same bits, and a frame's map does not depend on the other frames of the batch.
 * Form, operator caches, state and ordering are exactly those of aefft_net_score_map: the form aefft_net_step_form reports; in the chain form
 * with the operators at hand five launches (the input transform's two, the inverse column pass with the operator on load, the SSIM row
 * pass, the finish), six with score_d; a pending aefft_net_step_grad is ended (aefft_net_step_apply then fails with AEFFT_ESTATE);
 * aefft_net_get_layer(s) afterwards export the layers of this call; training is left bit for bit undisturbed; the context stream only, no
 * host synchronisation.  The FIRST SSIM call of a net allocates its strip buffer (5 B*D*Nx*Ny/16 floats, as the first target step allocates
 * its workspaces): it must not be made under stream capture.  Later calls allocate nothing and do not synchronise.
 * The spatial net (float frames and float targets only) and smooth grids under AEFFT_F_CHIRPZ form the same strips from the STORED
 * reconstruction in a launch of their own: they need recon_d.
 * AEFFT_EINVAL: null net, frames or map_d; a pointer not 16-byte aligned; a tile that is not 8, 16, 32 or 64 or does not divide Nx and Ny;
 * a data_range that is not finite or not greater than 0; an 8-bit argument on a spatial net; recon_d == NULL on one of the routes just named
 * (the message says why).  The outputs are then untouched. */
int aefft_net_ssim_map(aefft_net* net, const void* frames_d, int frames_u8, const void* targets_d /* nullable: the frames */, int targets_u8,
                       int tile, float data_range, float* map_d, float* score_d /* nullable */, float* recon_d /* nullable */);
/* Decode: the reconstruction from a STORED hidden layer -- the other half of aefft_net_infer(hidden_pair = l, hidden_d).  code_d
 * [B][dM_l][Nx_l][Ny_l] float, l = hidden_pair: layer 2l+2 in coordinate space, shape and layout as aefft_net_infer writes hidden_d (stored,
 * transmitted or edited since: it need not be an encoder output).  recon_d [B][D][Nx][Ny] float, or unsigned char when recon_u8 under
 * SpinToImage_C's rule as in aefft_net_infer.  Both pointers 16-byte aligned; B is the net's batch.
 * The result is layer 4L of autoenc_fft (fft_backproplib.cu:1331-1376) run from its loop index n = l+1 with freq = fft(code), on the
 * CURRENT weights: pool then conv_k with c_n for the pairs below l, conv_k with f_n then pool(-s) for every decoder down to pair 0.
 * The call runs in the form aefft_net_step_form reports.  OPERATOR / OPERATOR_CHAIN: every pooling crop below the code discards the bins
 * outside the coarsest grid, so the remainder of the network is one affine operator T^_l [D][dM_l + 1] per bin of that grid (the last
 * column carries every bias below).  It is formed by one launch from the kernel spectra and cached until aefft_net_set_pair,
 * aefft_net_load_spectra, aefft_net_step_apply or aefft_net_train_pair change the weights, or hidden_pair changes; any other call is
 * five launches: the code's transform with the crop to the coarsest grid fused (2), the per-bin product (1), the reconstruction's
 * sparse inverse transform (2).  PER_FRAME: the code's transform, then the lazy per-frame forward from pair l+1's pooling onward and the
 * reconstruction, with the contraction kernels of the step.
 * State: the call ends a pending aefft_net_step_grad (aefft_net_step_apply then fails with AEFFT_ESTATE).  No frame stands behind a
 * decode: aefft_net_get_layer(s) return AEFFT_ESTATE until the next aefft_net_forward, aefft_net_infer or aefft_net_step_grad.  Training
 * is not disturbed: operator sets, the chain carried ahead, the double-buffered input spectra, the cached hidden-layer operator of
 * aefft_net_infer and the deferred MSE sums are left so that the next aefft_net_step_grad / _apply give bit for bit what they would have
 * given without the call.  Everything is ordered on the context stream, whatever the pipelining switches and aefft_net_set_input_ready
 * say.  No host synchronisation, no allocation (sized by aefft_net_create*).
 * Spatial net: the coordinate-space sequence from layer 2l+2 (float only; recon_u8 is AEFFT_EINVAL).
 * AEFFT_EINVAL: null net, code or reconstruction, hidden_pair outside 0..L-1, a pointer not 16-byte aligned. */
int aefft_net_decode(aefft_net* net, int hidden_pair, const float* code_d, void* recon_d, int recon_u8);
/* Opt-in input prefetch for pipelined training loops.  enable = 1 asserts that the frames handed to
 * aefft_net_step_grad are COMPLETE in device memory when the call is made (not merely ordered on the
 * context stream, e.g. a loader that synchronises its own copy stream): their R2C then runs on an
 * internal side stream and may overlap the tail of the previous step still queued on the context
 * stream (the input spectra are double-buffered); and the reconstruction written by aefft_net_step_grad is
 * launched at the END of the gradient half (where a data-parallel rank waits for its all-reduce) and is complete
 * on the context stream only after the following aefft_net_step_apply, aefft_sync or any later call on the net.
 * Default 0: everything is ordered on the context stream and recon_d is complete when aefft_net_step_grad's work is. */
int aefft_net_set_input_ready(aefft_net* net, int enable);
/* The packed buffer (device), nfloats = [dck | dfk | db | dp of pair 0] ... [of pair L-1] | mse[L]: the batch-mean gradients of the last
 * aefft_net_step_grad, then ONE float per pair: the post-update MSE of this rank's frames as the PREVIOUS aefft_net_step_apply left it
 * (zero before the first).  A data-parallel caller all-reduces (SUM) the whole buffer: the gradients are then applied with grad_scale =
 * 1/world, and the tail times 1/world is the global-batch MSE of the previous step (the MSE rides in the gradients' message;
 * the post-update MSE of a step needs that step's reduced gradients, so it travels one step behind).  aefft_net_step_apply reads the
 * gradient part only and overwrites the tail; what it finds there it first saves, times its grad_scale, in the L floats BEHIND the
 * buffer (buf_d[nfloats .. nfloats + L), not part of the message): after step_apply of step t+1 they hold the global-batch MSE of step t
 * (with mse_d = NULL, see aefft_net_last_mse: once the sums of step t+1 have been formed, i.e. after the next aefft_net_step_grad).
 * A spatial net (AEFFT_NET_SPATIAL) puts the PRE-update MSE of THIS step in the tail: see aefft_net_create_ex. */
int aefft_net_grad_buffer(aefft_net* net, float** buf_d, size_t* nfloats);
/* Which form the NEXT aefft_net_step_grad / _apply of this net runs in (decided by the net's shapes and the development switches; the
 * arithmetic is the reference's in every form, re-associated -- DESIGN.md section 4):
 *   AEFFT_FORM_PER_FRAME       every layer evaluated for every frame (batch contractions on the matrix cores).  Taken for inputs of more
 *                              than 3 channels, kernel supports other than equal square 3x3 / 5x5, channel counts beyond the operator
 *                              kernels' tiles, and under AEFFT_F_NOOPFORM / AEFFT_F_NOQPATH.
 *   AEFFT_FORM_OPERATOR        the network is linear: layers evaluated once per step as per-bin operators on 4 basis frames, the batch
 *                              enters through the input transform, its centred second moments and the reconstruction; layer by layer.
 *   AEFFT_FORM_OPERATOR_CHAIN  ... with the whole operator chain in one launch out of a bin-major copy of the kernel spectra (coarsest grid
 *                              of at most 16384 bins); the next step's chain rides in the last launch of this step.
 * aefft_net_infer runs in the same form (its operators are then evaluated once per weight set).  Returns -1 for a null net. */
enum { AEFFT_FORM_PER_FRAME = 0, AEFFT_FORM_OPERATOR = 1, AEFFT_FORM_OPERATOR_CHAIN = 2, AEFFT_FORM_SPATIAL = 3 /* AEFFT_NET_SPATIAL */ };
int aefft_net_step_form(aefft_net* net);
/* Which step code the LAST tail launch of this net ran (the launch that ends aefft_net_step_apply in the operator forms: the next step's operator
 * chain, the post-update MSE and the tap stores): AEFFT_TAIL_STATIC when the per-bin steps came from a compile-time table for the net's channel
 * counts (input 3; maps 8,16,32 / 8,16,32,64 / 8,16,32,64,128), AEFFT_TAIL_GENERIC when they were decoded from the step list in the kernel's
 * arguments (every other net, launches without the chain, AEFFT_F_NOSTATICCHAIN), AEFFT_TAIL_NONE before the first such launch and on nets that
 * have none.  The results do not depend on the route.  Returns -1 for a null net. */
enum { AEFFT_TAIL_NONE = 0, AEFFT_TAIL_GENERIC = 1, AEFFT_TAIL_STATIC = 2 };
int aefft_net_tail_route(aefft_net* net);
int aefft_net_step_apply(aefft_net* net, float del0, int maxdiff, int sym, float grad_scale, float* mse_d);
/* The per-pair post-update MSEs of the LAST aefft_net_step_apply (fft_backproplib.cu:1463), to mse_d[L] (device), in stream order.
 * aefft_net_step_apply(mse_d = NULL) does not form them in a launch of its own: the per-workgroup partial sums wait in the net and are
 * added up by one extra workgroup of the next aefft_net_step_grad's gradient launch -- in time for the packed buffer's MSE tail and that
 * step's all-reduce -- or by this call, whichever comes first.  A loop that logs the MSE every K steps calls this every K steps. */
int aefft_net_last_mse(aefft_net* net, float* mse_d);
int aefft_net_reset_momentum(aefft_net* net);
/* The inertia weight alpha of backprop_gpu's update (backproplib.cu:392-396) on a spatial net; default 0.9 (autoencoder.cpp:89; the
 * application changes it with keys 6 / 7).  AEFFT_EINVAL for alpha outside [0, 1] or for an FFT net (its update has no alpha). */
int aefft_net_set_inertia(aefft_net* net, float alpha);

/* ---- measurement ----------------------------------------------------------------------------- */
/* Per-kernel HIP event timing on the context stream (bench.py's roofline figure).  With
 * enable=1 every kernel launch is bracketed by hipEvents recorded on the stream it runs on.
 * aefft_prof_read synchronises and returns, for kernel id `kid` (0..aefft_prof_count()-1,
 * named by aefft_prof_name), launches, total milliseconds and total ALGORITHMIC bytes
 * (unique tensors entering + leaving each launch) since the last reset. */
int aefft_prof_enable(aefft_ctx* ctx, int enable);
int aefft_prof_count(void);
const char* aefft_prof_name(int kid);
int aefft_prof_read(aefft_ctx* ctx, int kid, long* launches, double* total_ms, double* algo_bytes);
int aefft_prof_reset(aefft_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* AEFFT_H */
