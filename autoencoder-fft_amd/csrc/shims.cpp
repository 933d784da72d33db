// C++ operator-API shims: the reference's netlib.h / backproplib.h / fft_backproplib.h entry points
// (same mangled symbols, nested std::vector arguments) implemented over the flat C ABI (aefft.h).
// They marshal host vectors to the device, call the HIP path and marshal back -- this is the
// link-compatibility layer for an unchanged autoencoder.cpp; throughput work drives aefft.h directly.
//
// The host-only functions of netlib.h (the reference's own CPU path: Conv, backprop, Pool, Portion,
// Init_conv, SaveLoad_conv, LoadParam, act, act1) are implemented here in plain C++ with the
// reference's semantics (cited per function).  They are NOT a fallback for the GPU entry points:
// autoenc_fft / backprop_fft / Conv_gpu / backprop_gpu / backprop_gpu_cc abort loudly without a device.
#include "../../include/aefft.h"
#include "../../include/netlib.h"
#include "../../include/backproplib.h"
#include "../../include/fft_backproplib.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>

#if __has_include(<opencv2/core.hpp>)
#include <opencv2/core.hpp>
#define AEFFT_HAVE_OPENCV 1
#else
#define AEFFT_HAVE_OPENCV 0
#endif

using namespace aefft_vec;

namespace {

[[noreturn]] void die(const char* where, const char* what)
{
    fprintf(stderr, "aefft shim: %s: %s\n", where, what);
    abort();
}

aefft_ctx* context()
{
    static aefft_ctx* ctx = nullptr;
    if (!ctx) {
        if (aefft_ctx_create(&ctx, 0, nullptr, 1) != AEFFT_OK || !ctx)
            die("context", "no MI355X available -- the GPU entry points have no CPU fallback");
    }
    return ctx;
}
void chk(int rc, const char* where) { if (rc != AEFFT_OK) die(where, aefft_last_error(context())); }
void hchk(hipError_t e, const char* where) { if (e != hipSuccess) die(where, hipGetErrorString(e)); }

// device buffer with host marshalling
struct DevBuf {
    float* d = nullptr; size_t n = 0;
    explicit DevBuf(size_t count) : n(count)
    {
        hchk(hipMalloc(&d, std::max<size_t>(count, 4) * sizeof(float)), "hipMalloc");
        if (aefft_ctx_get_flags(nullptr) & AEFFT_F_POISON) { hchk(hipMemset(d, 0xFF, std::max<size_t>(count, 4) * sizeof(float)), "poison"); hchk(hipDeviceSynchronize(), "poison"); }
    }
    ~DevBuf() { if (d) (void)hipFree(d); }
    DevBuf(const DevBuf&) = delete;
    // All traffic goes through the context's own (non-blocking) stream: a hipMemcpy / hipMemset on the NULL stream is NOT ordered
    // against kernels on a non-blocking stream, and a pageable H2D copy may return before its DMA has landed -- the kernels
    // of the same call could otherwise read the buffer before the data is there (seen as rare run-to-run differences).
    static hipStream_t stream() { return static_cast<hipStream_t>(aefft_stream(context())); }
    void up(const std::vector<float>& h)
    {
        hchk(hipMemcpyAsync(d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, stream()), "H2D");
        hchk(hipStreamSynchronize(stream()), "H2D sync");                // the host vector may be a temporary
    }
    void down(std::vector<float>& h)
    {
        hchk(hipMemcpyAsync(h.data(), d, h.size() * sizeof(float), hipMemcpyDeviceToHost, stream()), "D2H");
        hchk(hipStreamSynchronize(stream()), "D2H sync");
    }
    void zero() { hchk(hipMemsetAsync(d, 0, n * sizeof(float), stream()), "memset"); }
};

std::vector<float> flat3(const Maps& t)
{
    std::vector<float> v;
    for (auto& p : t) for (auto& r : p) v.insert(v.end(), r.begin(), r.end());
    return v;
}
void unflat3(const std::vector<float>& v, Maps& t)
{
    size_t q = 0;
    for (auto& p : t) for (auto& r : p) for (float& x : r) x = v[q++];
}
std::vector<float> flat4(const Kernels& t)
{
    std::vector<float> v;
    for (auto& a : t) for (auto& p : a) for (auto& r : p) v.insert(v.end(), r.begin(), r.end());
    return v;
}
void unflat4(const std::vector<float>& v, Kernels& t)
{
    size_t q = 0;
    for (auto& a : t) for (auto& p : a) for (auto& r : p) for (float& x : r) x = v[q++];
}

// cached resident network for autoenc_fft (rebuilt when the caller changes the structure, e.g. keys n/d)
struct NetCache {
    aefft_net* net = nullptr;
    std::vector<int> sig;
    ~NetCache() { if (net) aefft_net_destroy(net); }
} g_net;

}  // namespace

// ------------------------------------------------------------------------------------------------
// fft_backproplib.h
// ------------------------------------------------------------------------------------------------
void autoenc_fft(Kernels& layers, KernelStack& net_c, BiasStack& net_cfreq, BiasStack& net_b, std::vector<int>& scale, int fft_l)
{
    aefft_ctx* ctx = context();
    const int N = (int)net_c.size(), L = N / 2;
    if (L < 1 || (int)layers.size() != 4 * L + 1 || (int)scale.size() < N) die("autoenc_fft", "inconsistent layers / net_c / scale sizes");
    const int D = (int)layers[0].size(), Nx = (int)layers[0][0].size(), Ny = (int)layers[0][0][0].size();
    std::vector<int> maps(L), Nk(L), Nl(L), sc(L), sig = {D, Nx, Ny, L};
    for (int l = 0; l < L; ++l) {
        maps[l] = (int)net_c[l].size(); Nk[l] = (int)net_c[l][0][0].size(); Nl[l] = (int)net_c[l][0][0][0].size(); sc[l] = scale[l];
        sig.insert(sig.end(), {maps[l], Nk[l], Nl[l], sc[l]});
    }
    bool rebuilt = false;
    if (!g_net.net || g_net.sig != sig) {
        if (g_net.net) aefft_net_destroy(g_net.net);
        aefft_net_desc d = {D, Nx, Ny, L, maps.data(), Nk.data(), Nl.data(), sc.data(), 1};
        // (smooth sizes -- the reference's users feed it camera frames, 640 x 480 -- take the mixed-radix transforms)
        chk(aefft_net_create_ex(ctx, &d, AEFFT_NET_SMOOTH_SIZES, &g_net.net), "aefft_net_create_ex");
        g_net.sig = sig; rebuilt = true;
    }
    aefft_net* net = g_net.net;
    int dD = D, nx = Nx, ny = Ny;
    std::vector<size_t> W(L);
    for (int l = 0; l < L; ++l) { nx /= sc[l]; ny /= sc[l]; W[l] = (size_t)maps[l] * dD * nx * (ny / 2 + 1) * 2; dD = maps[l]; }
    if ((int)net_cfreq.size() < N) {
        // fft_backproplib.cu:1148-1158: spectra recomputed from net_c for every conv of this call; pushed for n >= size()
        for (int l = 0; l < L; ++l) {
            std::vector<float> c = flat4(net_c[l]), f = flat4(net_c[N - 1 - l]);
            chk(aefft_net_set_pair(net, l, c.data(), net_b[l].data(), f.data(), net_b[N - 1 - l].data()), "aefft_net_set_pair");
        }
        for (int n = (int)net_cfreq.size(); n < N; ++n) {
            const int l = n < L ? n : N - 1 - n;
            std::vector<float> S(W[l]);
            chk(n < L ? aefft_net_store_spectra(net, l, S.data(), nullptr) : aefft_net_store_spectra(net, l, nullptr, S.data()), "aefft_net_store_spectra");
            net_cfreq.push_back(S);
        }
    } else {
        (void)rebuilt;
        // :1160 load_cfreq: the cached spectra (and net_b) are authoritative
        for (int l = 0; l < L; ++l) {
            if (net_cfreq[l].size() != W[l] || net_cfreq[N - 1 - l].size() != W[l]) die("autoenc_fft", "net_cfreq entry has the wrong size (stale cache: clear it)");
            chk(aefft_net_load_spectra(net, l, net_cfreq[l].data(), net_b[l].data(), net_cfreq[N - 1 - l].data(), net_b[N - 1 - l].data()), "aefft_net_load_spectra");
        }
    }
    std::vector<float> x = flat3(layers[0]);
    DevBuf frames(x.size()), recon(x.size());
    frames.up(x);
    chk(aefft_net_forward(net, frames.d, recon.d), "aefft_net_forward");
    if (fft_l) {
        // fft_l = 1 (fft_backproplib.cu:1347,1357,1361): every layer in ONE call and one download
        std::vector<size_t> off(4 * L + 2);
        chk(aefft_net_layers_layout(net, off.data()), "aefft_net_layers_layout");
        std::vector<float> all(off[4 * L + 1]);
        DevBuf d(all.size());
        chk(aefft_net_get_layers(net, d.d), "aefft_net_get_layers");
        d.down(all);
        for (int l = 1; l <= 4 * L; ++l) {
            const size_t sz = off[l + 1] - off[l];
            if (layers[l].empty() || layers[l][0].empty() || (size_t)layers[l].size() * layers[l][0].size() * layers[l][0][0].size() != sz)
                die("autoenc_fft", "layers[l] is not pre-sized to the network's shape");
            std::vector<float> h(all.begin() + off[l], all.begin() + off[l + 1]);
            unflat3(h, layers[l]);
        }
    } else {
        recon.down(x);
        unflat3(x, layers.back());
    }
}

void kernel_pad(Kernels& c, Kernels& c_pad, int Nx, int Ny)
{
    // fft_backproplib.cu:1018-1064: tap (k,l) -> ((k - Nk/2) mod Nx, (l - Nl/2) mod Ny), everything else 0
    const int dM = (int)c.size(), dD = (int)c[0].size(), Nk = (int)c[0][0].size(), Nl = (int)c[0][0][0].size();
    Kernels out(dM, Maps(dD, Plane(Nx, Bias(Ny, 0.f))));
    for (int m = 0; m < dM; ++m) for (int d = 0; d < dD; ++d) for (int k = 0; k < Nk; ++k) for (int l = 0; l < Nl; ++l)
        out[m][d][((k - Nk / 2) % Nx + Nx) % Nx][((l - Nl / 2) % Ny + Ny) % Ny] = c[m][d][k][l];
    c_pad = out;
}

void backprop_fft(Maps& in, Maps& expout, Maps& out, Bias& cfreq, Kernels& c, Bias& ffreq, Kernels& f, Bias& b, Bias& p,
                  int dM, float del0, int maxdiff)
{
    aefft_ctx* ctx = context();
    const int dD = (int)in.size(), Nx = (int)in[0].size(), Ny = (int)in[0][0].size();
    const int Nk = (int)c[0][0].size(), Nl = (int)c[0][0][0].size();
    const size_t P2 = (size_t)Nx * (Ny / 2 + 1) * 2, W = (size_t)dM * dD * P2, nk = (size_t)dM * dD * Nk * Nl;
    if (cfreq.size() != W || ffreq.size() != W) die("backprop_fft", "cfreq/ffreq size does not match dM*dD*Nx*Nyr*2");
    std::vector<float> hin = flat3(in), hex = flat3(expout), hout = flat3(out), hc = flat4(c), hf = flat4(f);
    DevBuf x(hin.size()), t(hex.size()), o(hout.size());
    DevBuf X(dD * P2), T(dD * P2), O(dD * P2), H(dM * P2), C(W), F(W), dc(W), df(W);
    DevBuf cd(nk), fd(nk), bd(dM), pd(dD), db(dM), dp(dD), Dc(nk), Df(nk), Db(dM), Dp(dD), mse(101);
    x.up(hin); t.up(hex); o.up(hout); C.up(cfreq); F.up(ffreq); cd.up(hc); fd.up(hf); bd.up(b); pd.up(p);
    Dc.zero(); Df.zero(); Db.zero(); Dp.zero();                                   // fft_backproplib.cu:1420-1423
    chk(aefft_r2c(ctx, x.d, X.d, dD, Nx, Ny), "r2c(in)");                          // :1430-1432
    chk(aefft_r2c(ctx, t.d, T.d, dD, Nx, Ny), "r2c(expout)");
    chk(aefft_r2c(ctx, o.d, O.d, dD, Nx, Ny), "r2c(out)");
    chk(aefft_mse(ctx, T.d, O.d, mse.d, 1, dM, dD, Nx, Ny), "mse");               // :1440
    const float del = 0.1f * del0;                                                 // :1445
    const int n_iter = 100;                                                        // :1446
    for (int n = 0; n < n_iter; ++n) {
        chk(aefft_gradient(ctx, X.d, T.d, O.d, C.d, F.d, bd.d, dc.d, df.d, db.d, dp.d, 1, dM, dD, Nx, Ny), "gradient");
        chk(aefft_update(ctx, cd.d, fd.d, bd.d, pd.d, C.d, F.d, dc.d, df.d, db.d, dp.d, Dc.d, Df.d, Db.d, Dp.d, dM, dD, Nx, Ny, Nk, Nl, del, maxdiff), "update");
        chk(aefft_conv(ctx, X.d, C.d, bd.d, H.d, 1, dM, dD, Nx, Ny), "conv");       // :1460
        chk(aefft_conv(ctx, H.d, F.d, pd.d, O.d, 1, dD, dM, Nx, Ny), "conv");       // :1461
        chk(aefft_mse(ctx, T.d, O.d, mse.d + n + 1, 1, dM, dD, Nx, Ny), "mse");     // :1463
    }
    std::vector<float> hm(101);
    mse.down(hm);
    std::cout << "mse fft: " << hm[0] << std::endl;                                // :1441
    for (int n = 0; n < n_iter; ++n) std::cout << "n: " << n << " mse: " << hm[n + 1] << std::endl;   // :1464
    C.down(cfreq); F.down(ffreq);                                                  // :1484-1485
    // :1487-1488 export_cfreq: kernels are recovered FROM THE SPECTRA (C2R/(Nx*Ny) + un-pad), biases copied back
    chk(aefft_kernel_export(ctx, C.d, cd.d, dM, dD, Nk, Nl, Nx, Ny), "kernel_export");
    chk(aefft_kernel_export(ctx, F.d, fd.d, dD, dM, Nk, Nl, Nx, Ny), "kernel_export");
    cd.down(hc); fd.down(hf); bd.down(b); pd.down(p);
    unflat4(hc, c); unflat4(hf, f);
}

// ------------------------------------------------------------------------------------------------
// backproplib.h
// ------------------------------------------------------------------------------------------------
float act(float x) { return x; }                   // backproplib.cu:38-44
float act1(float) { return 1; }                    // backproplib.cu:45-51

void Conv_gpu(Maps& in, Maps& out, Kernels& c, Bias& b)
{
    aefft_ctx* ctx = context();
    const int dD = (int)c[0].size(), dM = (int)c.size(), Nx = (int)in[0].size(), Ny = (int)in[0][0].size();
    const int Nk = (int)c[0][0].size(), Nl = (int)c[0][0][0].size();
    std::vector<float> hi = flat3(in), hc = flat4(c), ho((size_t)dM * Nx * Ny);
    DevBuf di(hi.size()), dc(hc.size()), db(dM), dout(ho.size());
    di.up(hi); dc.up(hc); db.up(b);
    chk(aefft_conv_spatial(ctx, di.d, dout.d, dc.d, db.d, 1, dD, dM, Nx, Ny, Nk, Nl, 0), "aefft_conv_spatial");
    dout.down(ho);
    unflat3(ho, out);
}

static void backprop_spatial_shim(Maps& in, Maps& out, Maps& hin, Kernels& c, Bias& b, Kernels& f, Bias& p, Kernels& dc, Bias& db,
                                  Kernels& df, Bias& dp, Kernels& ddc, Bias& ddb, Kernels& ddf, Bias& ddp, float delmax, float alpha, int tied)
{
    aefft_ctx* ctx = context();
    const int dM = (int)c.size(), dD = (int)c[0].size(), Nk = (int)c[0][0].size(), Nl = (int)c[0][0][0].size();
    const int Nx = (int)in[0].size(), Ny = (int)in[0][0].size();
    // printed distance (backproplib.cu:346-357 / :577-588): sum (in-out)^2 / Norm
    float Norm = (float)(dD * dM * Nk * Nl * Nx * Ny);
    if (tied) Norm = (float)(2 * dD * dM * Nk * Nl * Nx * Ny);
    float dist = 0;
    for (int d = 0; d < dD; ++d) for (int i = 0; i < Nx; ++i) for (int j = 0; j < Ny; ++j) dist += (float)std::pow(in[d][i][j] - out[d][i][j], 2);
    std::cout << "mse: " << dist / Norm << std::endl;
    std::vector<float> hi = flat3(in), ho = flat3(out), hh = flat3(hin), hc = flat4(c), hf = flat4(f);
    std::vector<float> hdc = flat4(dc), hdf = flat4(df), hddc = flat4(ddc), hddf = flat4(ddf);
    DevBuf di(hi.size()), dout(ho.size()), dh(hh.size()), Dc(hc.size()), Df(hf.size()), Db(dM), Dp(dD);
    DevBuf mc(hdc.size()), mf(hdf.size()), mb(dM), mp(dD), gc(hddc.size()), gf(hddf.size()), gb(dM), gp(dD);
    di.up(hi); dout.up(ho); dh.up(hh); Dc.up(hc); Df.up(hf); Db.up(b); Dp.up(p);
    mc.up(hdc); mf.up(hdf); mb.up(db); mp.up(dp); gc.up(hddc); gf.up(hddf); gb.up(ddb); gp.up(ddp);
    chk(aefft_backprop_spatial(ctx, di.d, dout.d, dh.d, Dc.d, Db.d, Df.d, Dp.d, mc.d, mb.d, mf.d, mp.d, gc.d, gb.d, gf.d, gp.d,
                               1, dD, dM, Nx, Ny, Nk, Nl, delmax, alpha, tied, 0), "aefft_backprop_spatial");
    Dc.down(hc); Df.down(hf); Db.down(b); Dp.down(p); mc.down(hdc); mb.down(db); mp.down(dp); gc.down(hddc); gb.down(ddb); gp.down(ddp);
    unflat4(hc, c); unflat4(hf, f); unflat4(hdc, dc); unflat4(hddc, ddc);
    if (!tied) { mf.down(hdf); gf.down(hddf); unflat4(hdf, df); unflat4(hddf, ddf); }
}

void backprop_gpu(Maps& in, Maps& out, Maps& hin, Kernels& c, Bias& b, Kernels& f, Bias& p, Kernels& dc, Bias& db, Kernels& df, Bias& dp,
                  Kernels& ddc, Bias& ddb, Kernels& ddf, Bias& ddp, float delmax, float alpha, int /*active: inert, backproplib.cu:34*/)
{
    backprop_spatial_shim(in, out, hin, c, b, f, p, dc, db, df, dp, ddc, ddb, ddf, ddp, delmax, alpha, 0);
}

void backprop_gpu_cc(Maps& in, Maps& out, Maps& hin, Kernels& c, Bias& b, Kernels& f, Bias& p, Kernels& dc, Bias& db, Kernels& df, Bias& dp,
                     Kernels& ddc, Bias& ddb, Kernels& ddf, Bias& ddp, float delmax, float alpha, int /*active*/)
{
    backprop_spatial_shim(in, out, hin, c, b, f, p, dc, db, df, dp, ddc, ddb, ddf, ddp, delmax, alpha, 1);
}

// ------------------------------------------------------------------------------------------------
// netlib.h -- host-side functions (the reference's CPU path and plumbing)
// ------------------------------------------------------------------------------------------------
void Pool(Maps& in, Maps& out, int scale)
{
    const int D = (int)in.size();
    if (scale > 0) {                                   // netlib.cpp:117-140
        const int Nx = (int)in[0].size(), Ny = (int)in[0][0].size();
        for (int d = 0; d < D; ++d)
            for (int i = 0; i < Nx; i += scale)
                for (int j = 0; j < Ny; j += scale) {
                    int smax = 0;                      // integer accumulator: truncation + clamp at 0 (:127)
                    for (int k = 0; k < scale; ++k)
                        for (int l = 0; l < scale; ++l)
                            if (i + k < Nx && j + l < Ny && in[d][i + k][j + l] > smax) smax = (int)in[d][i + k][j + l];
                    out[d][i / scale][j / scale] = (float)smax;
                }
    } else {                                           // :141-163 nearest-neighbour up-sampling
        const int Nx = (int)out[0].size(), Ny = (int)out[0][0].size(), s = -scale;
        for (int d = 0; d < D; ++d)
            for (int i = 0; i < Nx; i += s)
                for (int j = 0; j < Ny; j += s)
                    for (int k = 0; k < s; ++k)
                        for (int l = 0; l < s; ++l)
                            if (i + k < Nx && j + l < Ny) out[d][i + k][j + l] = in[d][i / s][j / s];
    }
}

void Init_conv(Kernels& c, Bias& b, int mS, int dS, int kS, int lS, float max)
{
    // netlib.cpp:167-197: one rand() per tap in (m,d,k,l) order, then one per map for the bias
    c.assign(mS, Maps(dS, Plane(kS, Bias(lS))));
    b.assign(mS, 0.f);
    for (int m = 0; m < mS; ++m) {
        for (int d = 0; d < dS; ++d) for (int k = 0; k < kS; ++k) for (int l = 0; l < lS; ++l)
            c[m][d][k][l] = -max + 2 * max * (float)rand() / (float)RAND_MAX;
        b[m] = -max + 2 * max * (float)rand() / (float)RAND_MAX;
    }
}

void SaveLoad_conv(Kernels& c, Bias& b, int scale, int L, int io, int write)
{
    // netlib.cpp:220-272: raw float32 [m][d][k][l] weights then [m] biases; file name encodes L, in/out, D, M, Lk, Ll, S
    const int dM = (int)c.size(), dD = (int)c[0].size(), Nk = (int)c[0][0].size(), Nl = (int)c[0][0][0].size();
    std::vector<float> vec((size_t)dM * dD * Nk * Nl + dM);
    const std::string path = "./weights/C_weights_" + std::to_string(L) + (io == 0 ? "_in" : "_out") + "_D=" + std::to_string(dD) +
                             "_M=" + std::to_string(dM) + "_Lk=" + std::to_string((Nk - 1) / 2 - 1) + "_Ll=" + std::to_string((Nl - 1) / 2 - 1) +
                             "_S=" + std::to_string(scale) + ".conv";
    std::cout << "path " << L << (io == 0 ? "_in" : "_out") << " " << path << std::endl;
    if (write == 1) {
        std::vector<float> w = flat4(c);
        std::copy(w.begin(), w.end(), vec.begin());
        std::copy(b.begin(), b.begin() + dM, vec.begin() + w.size());
        std::ofstream file(path, std::ios::out | std::ios::binary);
        file.write(reinterpret_cast<const char*>(vec.data()), vec.size() * sizeof(float));
    } else {
        std::ifstream file(path, std::ios::in | std::ios::binary);
        file.read(reinterpret_cast<char*>(vec.data()), vec.size() * sizeof(float));
        unflat4(vec, c);
        for (int m = 0; m < dM; ++m) b[m] = vec[(size_t)dM * dD * Nk * Nl + m];
    }
}

void LoadParam(int& dM, int& Lk, int& Ll, int& scal, float& rmax)
{
    // netlib.cpp:274-289: values are read positionally; names are ignored
    std::vector<float> values;
    std::string name; float value;
    std::ifstream file("New_Layer_Param.txt");
    while (file >> name >> value) values.push_back(value);
    if (values.size() < 5) die("LoadParam", "New_Layer_Param.txt must hold five 'name value' lines");
    dM = (int)values[0]; Lk = (int)values[1]; Ll = (int)values[2]; scal = (int)values[3]; rmax = values[4];
}

void Portion(Maps& in, Maps& hin, Maps& out, Maps& in_s, Maps& hin_s, Maps& out_s, int q)
{
    // netlib.cpp:292-315: centred crop of size (Nx/q, Ny/q)
    const int Nx = (int)in[0].size(), Ny = (int)in[0][0].size(), D = (int)in.size(), M = (int)hin.size();
    const int dx = (Nx - Nx / q) / 2, dy = (Ny - Ny / q) / 2;
    for (int i = 0; i < Nx / q; ++i)
        for (int j = 0; j < Ny / q; ++j) {
            for (int d = 0; d < D; ++d) { in_s[d][i][j] = in[d][i + dx][j + dy]; out_s[d][i][j] = out[d][i + dx][j + dy]; }
            for (int m = 0; m < M; ++m) hin_s[m][i][j] = hin[m][i + dx][j + dy];
        }
}

void Conv(Maps& in, Maps& out, Kernels& c, Bias& b)
{
    // netlib.cpp:318-358
    const int Nx = (int)in[0].size(), Ny = (int)in[0][0].size(), Nk = (int)c[0][0].size(), Nl = (int)c[0][0][0].size();
    const int ak = (Nk - 1) / 2 - 1, al = (Nl - 1) / 2 - 1, dM = (int)c.size(), dD = (int)c[0].size();
    for (int m = 0; m < dM; ++m)
        for (int i = 0; i < Nx; ++i)
            for (int j = 0; j < Ny; ++j) {
                float h = 0;
                for (int d = 0; d < dD; ++d)
                    for (int k = 0; k < Nk; ++k) {
                        const int ii = i - (-2 * ak - 1 + k);
                        for (int l = 0; l < Nl; ++l) {
                            const int jj = j - (-2 * al - 1 + l);
                            if (ii > 0 && ii < Nx && jj > 0 && jj < Ny) h += c[m][d][k][l] * in[d][ii][jj];   // '>0', :344
                        }
                    }
                out[m][i][j] = act(h + b[m]);
            }
}

static inline float clip10(float g) { return (10 < std::fabs(g)) ? std::fabs(g) : 10; }

void backprop(Maps& in, Maps& out, Maps& hin, Kernels& c, Bias& b, Kernels& f, Bias& p, float del)
{
    // netlib.cpp:361-451: per weight element, full sums over (d1,i,j,k1,l1); weights updated inside the loops
    const int Nx = (int)in[0].size(), Ny = (int)in[0][0].size(), dM = (int)c.size(), dD = (int)c[0].size();
    const int Nk = (int)c[0][0].size(), Nl = (int)c[0][0][0].size(), ak = (Nk - 1) / 2 - 1, al = (Nl - 1) / 2 - 1;
    const float Norm = (float)(dD * dM * Nk * Nl * Nx * Ny);
    float dist = 0;
    for (int d = 0; d < dD; ++d) for (int i = 0; i < Nx; ++i) for (int j = 0; j < Ny; ++j) dist += (float)std::pow(in[d][i][j] - out[d][i][j], 2);
    std::cout << "mse: " << dist << std::endl;                                      // :385 (un-normalised)
    for (int m = 0; m < dM; ++m)
        for (int d = 0; d < dD; ++d)
            for (int k = 0; k < Nk; ++k) {
                const int ik = -2 * ak - 1 + k;
                for (int l = 0; l < Nl; ++l) {
                    const int il = -2 * al - 1 + l;
                    float dDdC = 0, dDdF = 0, dDdB = 0, dDdP = 0;
                    for (int d1 = 0; d1 < dD; ++d1)
                        for (int i = 0; i < Nx; ++i)
                            for (int j = 0; j < Ny; ++j) {
                                float dDdB1 = 0, dDdC1 = 0;
                                for (int k1 = 0; k1 < Nk; ++k1) {
                                    const int i1 = i - (-2 * ak - 1 + k1);
                                    for (int l1 = 0; l1 < Nl; ++l1) {
                                        const int j1 = j - (-2 * al - 1 + l1);
                                        if (i1 > 0 && i1 < Nx && j1 > 0 && j1 < Ny) {
                                            const float prod = f[d1][m][k1][l1] * act1(hin[m][i1][j1]);
                                            dDdB1 += prod;
                                            if (i1 - ik > 0 && i1 - ik < Nx && j1 - il > 0 && j1 - il < Ny) dDdC1 += prod * in[d][i1 - ik][j1 - il];
                                        }
                                    }
                                }
                                const float sum0 = (out[d1][i][j] - in[d1][i][j]) * act1(out[d1][i][j]);
                                dDdC += sum0 * dDdC1 / Norm;
                                dDdB += sum0 * dDdB1 / Norm;
                                if (d1 == d) {
                                    if (i - ik > 0 && i - ik < Nx && j - il > 0 && j - il < Ny) dDdF += sum0 * act(hin[m][i - ik][j - il]) / Norm;
                                    dDdP += sum0 / Norm;
                                }
                            }
                    c[m][d][k][l] += -del * dDdC / clip10(dDdC);
                    f[d][m][k][l] += -del * dDdF / clip10(dDdF);
                    if (k == 0 && l == 0) {
                        if (d == 0) b[m] += -del * dDdB / clip10(dDdB);
                        if (m == 0) p[d] += -del * dDdP / clip10(dDdP);
                    }
                }
            }
}

// ---- image converters (UI only) ----------------------------------------------------------------
#if AEFFT_HAVE_OPENCV
void ImageToSpin_C(cv::Mat& img, Maps& spin)
{   // netlib.cpp:37-51: spin[ch][x][y] = pixel (row y, column x), raw 0..255
    for (int i = 0; i < img.cols; ++i) for (int j = 0; j < img.rows; ++j) {
        const cv::Vec3b col = img.at<cv::Vec3b>(j, i);
        for (int ch = 0; ch < 3; ++ch) spin[ch][i][j] = (float)col[ch];
    }
}
void SpinToImage_C(cv::Mat& img, Maps& spin)
{   // netlib.cpp:54-77: round, clamp to [0,255]
    const int Nx = (int)spin[0].size(), Ny = (int)spin[0][0].size();
    for (int i = 0; i < Nx; ++i) for (int j = 0; j < Ny; ++j) {
        cv::Vec3b col;
        for (int m = 0; m < 3; ++m) { int v = (int)std::round(spin[m][i][j]); col[m] = (unsigned char)(v > 255 ? 255 : (v < 0 ? 0 : v)); }
        img.at<cv::Vec3b>(j, i) = col;
    }
}
void SpinToImage_V(cv::Mat& img, Plane& spin)
{   // netlib.cpp:80-94
    for (int i = 0; i < (int)spin.size(); ++i) for (int j = 0; j < (int)spin[0].size(); ++j) img.at<unsigned char>(j, i) = (unsigned char)(int)spin[i][j];
}
void SpinToImage_K(cv::Mat& img, Plane& spin)
{   // netlib.cpp:97-111
    for (int i = 0; i < (int)spin.size(); ++i) for (int j = 0; j < (int)spin[0].size(); ++j) {
        int v = (int)(100 * spin[i][j]);
        v = v > 0 ? v + 128 : 128 - v;
        img.at<unsigned char>(j, i) = (unsigned char)v;
    }
}
#else
// Built without OpenCV headers: the symbols exist so autoencoder.cpp links, but a cv::Mat cannot be
// touched without its definition -- fail loudly rather than guess its layout.
void ImageToSpin_C(cv::Mat&, Maps&) { die("ImageToSpin_C", "libaefft.so was built without OpenCV headers; rebuild where <opencv2/core.hpp> exists"); }
void SpinToImage_C(cv::Mat&, Maps&) { die("SpinToImage_C", "libaefft.so was built without OpenCV headers; rebuild where <opencv2/core.hpp> exists"); }
void SpinToImage_V(cv::Mat&, Plane&) { die("SpinToImage_V", "libaefft.so was built without OpenCV headers; rebuild where <opencv2/core.hpp> exists"); }
void SpinToImage_K(cv::Mat&, Plane&) { die("SpinToImage_K", "libaefft.so was built without OpenCV headers; rebuild where <opencv2/core.hpp> exists"); }
#endif
