// The image boundary (aefft_image_to_frames / aefft_frames_to_image, gfx950): netlib.cpp:37-51 ImageToSpin_C and :54-77 SpinToImage_C on the
// device, for a batch.  An image is Ny rows of interleaved pixels, pixel (row j, column i) channel d at byte j * pitch + i * D + d; a frame is the
// library's planar [D][Nx][Ny] with y contiguous: frames[b][d][i][j] = image[b][j][i][d] -- a de-interleave AND a transposition (Nx = img.cols).
//   image_unpack_kernel<D, F32>   image rows -> frames (unsigned char, or float when F32: (float)pixel)
//   image_pack_kernel<D, F32>     frames -> image rows (float frames through px_u8, fft_common.h: SpinToImage_C's rule as the inverse row pass applies it)
// Both are one LDS-tiled transposing copy.  A workgroup owns a tile of 64 image columns x 64 image rows, all D channels, of
// one image: 64 runs of 64 D bytes on the image side, 64 D runs of 64 elements on the frame side.  The tile is staged in LDS in IMAGE order, a row
// of 16 D dwords per image row; each side moves it with the accesses that are contiguous on that side:
//   image side   lane -> one dword of a row, consecutive lanes consecutive dwords (a wave: 256 contiguous bytes of the tile's rows, in pieces of
//                at least 64 bytes).  A dword that crosses the row's end Nx D is split into bytes: nothing beyond Nx D is read or written.
//   frame side   lane -> a block of 4 columns c = i D + d (one LDS dword) x 4 rows j: four LDS dwords, transposed as 4 x 4 bytes IN REGISTERS, four
//                global accesses of 4 pixels (one dword of 8-bit frames, one float4 of float frames), 16 consecutive lanes on one run of 64 pixels.
// So no access, global or LDS, is narrower than a dword on these paths.  They need: image_d and pitch multiples of 4 (image side); Ny a
// multiple of 4 (frame side; frames_d is 16-byte aligned by the library's rule).  Either side falls back ON ITS OWN to one element per lane --
// byte accesses, coalesced along the side's contiguous axis, the same LDS image -- when its condition fails: every accepted argument gives the
// same bytes.
// LDS: four image rows form a super-row of 64 D + 2 dwords (16 super-rows, 4 K D + 128 bytes: 16.1 KiB at D = 4).  The frame side's lanes q = 0..15
// of a run read dword g of rows 4 q + k: addresses q (64 D + 2) + 16 D k + g, banks 2 q + g + const (mod 32) -- the 32 lanes of a ds_read_b32 /
// ds_write_b32 lane group (q = 0..15 x two neighbouring g) on 32 different banks.  With a plain row pitch the lane stride would be 4 rows, a
// multiple of 4 dwords whatever the padding: 8 banks at best.  No scratch, no atomics.
#include "internal.h"
#include "fft_common.h"

namespace aefft {

constexpr int IMG_TILE = 64;                                                     // image columns and image rows of a tile
template <int D> struct ImgLds {
    static constexpr int RW = IMG_TILE * D / 4;                                  // dwords of a tile row
    static constexpr int SR = 4 * RW + 2;                                        // dwords of a super-row (four tile rows + the pad)
    static constexpr int WORDS = IMG_TILE / 4 * SR;
    static __device__ __forceinline__ int word(int j, int w) { return (j >> 2) * SR + (j & 3) * RW + w; }
    static __device__ __forceinline__ int byte(int j, int c) { return 4 * word(j, c >> 2) + (c & 3); }
};

struct ImgTileAt { long b; int i0, j0, ncols, nrows; };                          // a tile's image, origin, and live columns / rows (<= 64)
__device__ __forceinline__ ImgTileAt img_tile_at(long t, int tx, int ty, int Nx, int Ny)
{
    ImgTileAt a;
    const long r = t / tx;
    a.i0 = (int)(t - r * tx) * IMG_TILE;
    a.b = r / ty;
    a.j0 = (int)(r - a.b * ty) * IMG_TILE;
    a.ncols = min(Nx - a.i0, IMG_TILE);
    a.nrows = min(Ny - a.j0, IMG_TILE);
    return a;
}

// image side: rows [0, nrows) x bytes [0, nb) of the tile at img (the tile's first byte), row pitch `pitch`
template <int D> __device__ __forceinline__ void img_rows_to_lds(const unsigned char* __restrict__ img, size_t pitch, int nb, int nrows, unsigned* lds, bool words)
{
    typedef ImgLds<D> L;
    if (words) {
        for (int idx = threadIdx.x; idx < nrows * L::RW; idx += 256) {
            const int j = idx / L::RW, w = idx - j * L::RW, n = nb - 4 * w;
            const unsigned char* p = img + (size_t)j * pitch + 4 * w;
            unsigned v = 0;
            if (n >= 4) v = *reinterpret_cast<const unsigned*>(p);
            else
                for (int k = 0; k < n; ++k) v |= (unsigned)p[k] << (8 * k);      // (the dword that crosses the row's end: its live bytes only)
            lds[L::word(j, w)] = v;
        }
    } else {
        unsigned char* lb = reinterpret_cast<unsigned char*>(lds);
        for (int idx = threadIdx.x; idx < nrows * (IMG_TILE * D); idx += 256) {
            const int j = idx / (IMG_TILE * D), c = idx - j * (IMG_TILE * D);
            if (c < nb) lb[L::byte(j, c)] = img[(size_t)j * pitch + c];
        }
    }
}
template <int D> __device__ __forceinline__ void lds_to_img_rows(const unsigned* lds, unsigned char* __restrict__ img, size_t pitch, int nb, int nrows, bool words)
{
    typedef ImgLds<D> L;
    if (words) {
        for (int idx = threadIdx.x; idx < nrows * L::RW; idx += 256) {
            const int j = idx / L::RW, w = idx - j * L::RW, n = nb - 4 * w;
            unsigned char* p = img + (size_t)j * pitch + 4 * w;
            const unsigned v = lds[L::word(j, w)];
            if (n >= 4) *reinterpret_cast<unsigned*>(p) = v;
            else
                for (int k = 0; k < n; ++k) p[k] = (unsigned char)(v >> (8 * k));
        }
    } else {
        const unsigned char* lb = reinterpret_cast<const unsigned char*>(lds);
        for (int idx = threadIdx.x; idx < nrows * (IMG_TILE * D); idx += 256) {
            const int j = idx / (IMG_TILE * D), c = idx - j * (IMG_TILE * D);
            if (c < nb) img[(size_t)j * pitch + c] = lb[L::byte(j, c)];
        }
    }
}

// first element of frame row (d, i) of image b at row j: ((b D + d) Nx + i) Ny + j
__device__ __forceinline__ size_t frame_at(long b, int D, int d, int i, int j, int Nx, int Ny) { return (((size_t)b * D + d) * Nx + i) * (size_t)Ny + j; }

template <int D, bool F32>
__global__ __launch_bounds__(256) void image_unpack_kernel(const unsigned char* __restrict__ image, size_t pitch, void* __restrict__ frames, int Nx, int Ny,
                                                           int tx, int ty, long ntiles, bool img_words, bool frm_words)
{
    typedef ImgLds<D> L;
    __shared__ unsigned lds[L::WORDS];
    for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {                      // (uniform: a grid folded onto fewer workgroups loops)
        const ImgTileAt a = img_tile_at(t, tx, ty, Nx, Ny);
        img_rows_to_lds<D>(image + ((size_t)a.b * Ny + a.j0) * pitch + (size_t)a.i0 * D, pitch, a.ncols * D, a.nrows, lds, img_words);
        __syncthreads();
        if (frm_words) {
            for (int blk = threadIdx.x; blk < 16 * L::RW; blk += 256) {
                const int q = blk & 15, g = blk >> 4;
                if (4 * q >= a.nrows) continue;                                   // (Ny is a multiple of 4: a block of four rows is live or not)
                unsigned r[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) r[k] = lds[q * L::SR + k * L::RW + g];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int c = 4 * g + s, i = c / D, d = c - i * D;
                    if (i >= a.ncols) continue;
                    const unsigned p0 = (r[0] >> (8 * s)) & 255u, p1 = (r[1] >> (8 * s)) & 255u, p2 = (r[2] >> (8 * s)) & 255u, p3 = (r[3] >> (8 * s)) & 255u;
                    const size_t o = frame_at(a.b, D, d, a.i0 + i, a.j0 + 4 * q, Nx, Ny);
                    if constexpr (F32) *reinterpret_cast<float4*>(static_cast<float*>(frames) + o) = make_float4((float)p0, (float)p1, (float)p2, (float)p3);
                    else *reinterpret_cast<unsigned*>(static_cast<unsigned char*>(frames) + o) = p0 | p1 << 8 | p2 << 16 | p3 << 24;
                }
            }
        } else {
            const unsigned char* lb = reinterpret_cast<const unsigned char*>(lds);
            for (int idx = threadIdx.x; idx < IMG_TILE * D * IMG_TILE; idx += 256) {
                const int j = idx & 63, c = idx >> 6, i = c / D, d = c - i * D;
                if (j >= a.nrows || i >= a.ncols) continue;
                const unsigned char v = lb[L::byte(j, c)];
                const size_t o = frame_at(a.b, D, d, a.i0 + i, a.j0 + j, Nx, Ny);
                if constexpr (F32) static_cast<float*>(frames)[o] = (float)v;
                else static_cast<unsigned char*>(frames)[o] = v;
            }
        }
        __syncthreads();
    }
}

template <int D, bool F32>
__global__ __launch_bounds__(256) void image_pack_kernel(const void* __restrict__ frames, unsigned char* __restrict__ image, size_t pitch, int Nx, int Ny,
                                                         int tx, int ty, long ntiles, bool img_words, bool frm_words)
{
    typedef ImgLds<D> L;
    __shared__ unsigned lds[L::WORDS];
    for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const ImgTileAt a = img_tile_at(t, tx, ty, Nx, Ny);
        if (frm_words) {
            for (int blk = threadIdx.x; blk < 16 * L::RW; blk += 256) {
                const int q = blk & 15, g = blk >> 4;
                if (4 * q >= a.nrows) continue;
                unsigned r[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int c = 4 * g + s, i = c / D, d = c - i * D;
                    if (i >= a.ncols) continue;                                   // (columns beyond the image: bytes the image side never stores)
                    const size_t o = frame_at(a.b, D, d, a.i0 + i, a.j0 + 4 * q, Nx, Ny);
                    unsigned p0, p1, p2, p3;
                    if constexpr (F32) {
                        const float4 v = *reinterpret_cast<const float4*>(static_cast<const float*>(frames) + o);
                        p0 = px_u8(v.x); p1 = px_u8(v.y); p2 = px_u8(v.z); p3 = px_u8(v.w);
                    } else {
                        const unsigned v = *reinterpret_cast<const unsigned*>(static_cast<const unsigned char*>(frames) + o);
                        p0 = v & 255u; p1 = (v >> 8) & 255u; p2 = (v >> 16) & 255u; p3 = v >> 24;
                    }
                    r[0] |= p0 << (8 * s); r[1] |= p1 << (8 * s); r[2] |= p2 << (8 * s); r[3] |= p3 << (8 * s);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) lds[q * L::SR + k * L::RW + g] = r[k];
            }
        } else {
            unsigned char* lb = reinterpret_cast<unsigned char*>(lds);
            for (int idx = threadIdx.x; idx < IMG_TILE * D * IMG_TILE; idx += 256) {
                const int j = idx & 63, c = idx >> 6, i = c / D, d = c - i * D;
                if (j >= a.nrows || i >= a.ncols) continue;
                const size_t o = frame_at(a.b, D, d, a.i0 + i, a.j0 + j, Nx, Ny);
                if constexpr (F32) lb[L::byte(j, c)] = (unsigned char)px_u8(static_cast<const float*>(frames)[o]);
                else lb[L::byte(j, c)] = static_cast<const unsigned char*>(frames)[o];
            }
        }
        __syncthreads();
        lds_to_img_rows<D>(lds, image + ((size_t)a.b * Ny + a.j0) * pitch + (size_t)a.i0 * D, pitch, a.ncols * D, a.nrows, img_words);
        __syncthreads();
    }
}

// the launch geometry both directions share: one workgroup per tile, folded onto at most 2^20 workgroups (the kernels loop)
struct ImgGrid { int tx, ty; long ntiles; unsigned blocks; bool img_words, frm_words; };
static ImgGrid img_grid(const void* image, size_t pitch, int B, int Nx, int Ny)
{
    ImgGrid g;
    g.tx = (Nx + IMG_TILE - 1) / IMG_TILE; g.ty = (Ny + IMG_TILE - 1) / IMG_TILE;
    g.ntiles = (long)B * g.tx * g.ty;
    g.blocks = (unsigned)(g.ntiles < (1L << 20) ? g.ntiles : (1L << 20));
    g.img_words = ((reinterpret_cast<uintptr_t>(image) | pitch) & 3u) == 0;
    g.frm_words = (Ny & 3) == 0;
    return g;
}
static bool img_shape_ok(int B, int D, int Nx, int Ny, size_t pitch)
{
    return B >= 1 && D >= 1 && D <= 4 && Nx >= 1 && Nx <= 8192 && Ny >= 1 && Ny <= 8192 && pitch >= (size_t)Nx * D;
}

#define IMG_LAUNCH(KERNEL, ...)                                                                           \
    do {                                                                                                  \
        const dim3 gr(g.blocks), bl(256);                                                                 \
        switch (D * 2 + (f32 ? 1 : 0)) {                                                                  \
            case 2: KERNEL<1, false><<<gr, bl, 0, st>>>(__VA_ARGS__); break;                             \
            case 3: KERNEL<1, true><<<gr, bl, 0, st>>>(__VA_ARGS__); break;                              \
            case 4: KERNEL<2, false><<<gr, bl, 0, st>>>(__VA_ARGS__); break;                             \
            case 5: KERNEL<2, true><<<gr, bl, 0, st>>>(__VA_ARGS__); break;                              \
            case 6: KERNEL<3, false><<<gr, bl, 0, st>>>(__VA_ARGS__); break;                             \
            case 7: KERNEL<3, true><<<gr, bl, 0, st>>>(__VA_ARGS__); break;                              \
            case 8: KERNEL<4, false><<<gr, bl, 0, st>>>(__VA_ARGS__); break;                             \
            default: KERNEL<4, true><<<gr, bl, 0, st>>>(__VA_ARGS__); break;                             \
        }                                                                                                 \
    } while (0)

hipError_t launch_image_unpack(const unsigned char* image, size_t pitch, void* frames, bool f32, int B, int D, int Nx, int Ny, hipStream_t st)
{
    if (!image || !frames || !img_shape_ok(B, D, Nx, Ny, pitch)) return hipErrorInvalidValue;
    const ImgGrid g = img_grid(image, pitch, B, Nx, Ny);
    IMG_LAUNCH(image_unpack_kernel, image, pitch, frames, Nx, Ny, g.tx, g.ty, g.ntiles, g.img_words, g.frm_words);
    return hipGetLastError();
}

hipError_t launch_image_pack(const void* frames, bool f32, unsigned char* image, size_t pitch, int B, int D, int Nx, int Ny, hipStream_t st)
{
    if (!image || !frames || !img_shape_ok(B, D, Nx, Ny, pitch)) return hipErrorInvalidValue;
    const ImgGrid g = img_grid(image, pitch, B, Nx, Ny);
    IMG_LAUNCH(image_pack_kernel, frames, image, pitch, Nx, Ny, g.tx, g.ty, g.ntiles, g.img_words, g.frm_words);
    return hipGetLastError();
}

}  // namespace aefft
