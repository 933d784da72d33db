// The lane harness of the host-check programs (tools/*_hostcheck.cpp): what a kernel file of the image boundary needs to compile for the HOST and run
// with 256 threads as the lanes of a workgroup -- the index variables, a barrier for __syncthreads, float4, the pixel rule, the host forms of the kernel
// files' qualifier macros -- and what every program does around its cases: the launch, the random bytes, the counters and the closing report.
// Plain C++ with nothing from HIP.  A program includes this header first and then the kernel file by path; AEFFT_HOSTCHECK makes the kernel file leave
// out its own includes, its device-side qualifier macros and its launchers.
#pragma once
#include <math.h>
#include <pthread.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <thread>
#include <vector>

#define AEFFT_HOSTCHECK

struct Dim3 { unsigned x, y, z; };
static thread_local Dim3 threadIdx, blockIdx;
static Dim3 gridDim;
static pthread_barrier_t wg_barrier;
static void __syncthreads() { pthread_barrier_wait(&wg_barrier); }
struct float4 { float x, y, z, w; } __attribute__((aligned(16)));
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
// SpinToImage_C's pixel rule as fft_common.h states it for the device
static inline unsigned px_u8(float v) { return v > 0.f ? (unsigned)fminf(roundf(v), 255.f) : 0u; }
#define __device__
#define __forceinline__ inline
#define RZ_HD static inline
#define RZ_UNIFORM(x) (x)
#define TL_HD static inline
#define TL_MHD static inline
#define DG_HD static inline
#define CM_HD static inline
#define BA_HD static inline
#define WP_HD static inline
#define RG_HD static inline

// the launch: every workgroup of the grid, one after the other, its 256 lanes as threads; body(lds) is one lane's run of the kernel body
template <class F> static void launch(unsigned gx, unsigned gy, unsigned gz, size_t lds_words, F body)
{
    void* lds = nullptr;
    if (lds_words && posix_memalign(&lds, 16, 4 * lds_words)) abort();           // exactly what the launcher asks for: LDS overruns show
    gridDim = Dim3{gx, gy, gz};
    pthread_barrier_init(&wg_barrier, nullptr, 256);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < 256; ++t)
        th.emplace_back([&, t] {
            for (unsigned bz = 0; bz < gridDim.z; ++bz)
                for (unsigned by = 0; by < gridDim.y; ++by)
                    for (unsigned bx = 0; bx < gridDim.x; ++bx) {
                        threadIdx = Dim3{t, 0, 0};
                        blockIdx = Dim3{bx, by, bz};
                        body((unsigned*)lds);
                        __syncthreads();                                         // (the next workgroup reuses this one's LDS)
                    }
        });
    for (auto& x : th) x.join();
    pthread_barrier_destroy(&wg_barrier);
    free(lds);
}

static unsigned rnd_state = 12345;
static unsigned rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 24; }

// a program counts every run and every failed one, and ends with `return report();`
static int runs = 0, failures = 0;
static int report()
{
    if (failures) printf("%d of %d runs FAILED\n", failures, runs);
    else printf("all %d runs exact\n", runs);
    return failures ? 1 : 0;
}
