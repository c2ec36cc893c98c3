// The element-wise passes that are not BatchNorm (that family is norm_act.hip), NHWC, gfx950: the flat optimizer steps (SGD,
// RMSprop, Adam), segnb_add, the general MaxPool2d(k, stride, pad) forward and its two backward forms, bilinear and nearest x2
// upsampling and the NHWC -> NCHW fp32 move.  One thread per 8-channel chunk, grid-stride loops; the launch geometry helpers are ew.h,
// and every launch is written once, generically in the element type (segnb_dispatch_dtype, common.h).
#include "ew.h"
#include "../../include/segnb_upsample.h"

namespace {

__global__ void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, long long n, float lr) {
    const long long n4 = n >> 2;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 pv = reinterpret_cast<float4*>(p)[i];
        const float4 gv = reinterpret_cast<const float4*>(g)[i];
        pv.x -= lr * gv.x; pv.y -= lr * gv.y; pv.z -= lr * gv.z; pv.w -= lr * gv.w;
        reinterpret_cast<float4*>(p)[i] = pv;
    }
    for (long long i = (n4 << 2) + blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += stride)
        p[i] -= lr * g[i];
}

// ------------------------------------------------------------------------------------------------
// small generic NHWC ops for the other model families (LinkNet34 / FCDenseNet / UNet16)
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(NTHR) void add_kernel(const T* __restrict__ a, int ld_a, const T* __restrict__ b, int ld_b,
                                                   T* __restrict__ out, int ld_out, long long npix, int CPP) {
    const long long total = npix * CPP;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const long long pix = i / CPP;
        const int c0 = (int)(i - pix * CPP) * 8;
        float x[8], yv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = yv[e] = 0.f;
        if (a != nullptr) load8(a + pix * ld_a + c0, x);          // (a missing operand counts as zeros: copy / clear)
        if (b != nullptr) load8(b + pix * ld_b + c0, yv);
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] += yv[e];
        store8(out + pix * ld_out + c0, x);
    }
}

// MaxPool2d(k, stride, pad) forward (floor mode) and its gather-form backward: every input pixel checks the
// (up to ceil(k/stride)^2) windows that contain it and takes the window's gradient if it is that window's
// FIRST maximum in scan order (torch's tie rule).
template <typename T>
__global__ __launch_bounds__(NTHR) void maxpool_fwd_kernel(const T* __restrict__ x, int ld_x, int N, int H, int W, int CPP,
                                                           int k, int st, int pd, int Ho, int Wo, T* __restrict__ out,
                                                           int ld_out, unsigned char* __restrict__ idx) {
    const long long total = (long long)N * Ho * Wo * CPP;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % CPP) * 8;
        long long q = i / CPP;
        const int wo = (int)(q % Wo);
        q /= Wo;
        const int ho = (int)(q % Ho);
        const int n = (int)(q / Ho);
        float m[8];
        unsigned am[8];                    // window position a * k + b of the FIRST maximum in scan order (torch's tie rule)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            m[e] = -INFINITY;
            am[e] = 255u;
        }
        for (int a = 0; a < k; ++a)
            for (int b = 0; b < k; ++b) {
                const int hi = ho * st - pd + a, wi = wo * st - pd + b;
                if ((unsigned)hi < (unsigned)H && (unsigned)wi < (unsigned)W) {
                    float v[8];
                    load8(x + (((long long)n * H + hi) * W + wi) * ld_x + c0, v);
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (v[e] > m[e] || am[e] == 255u) {
                            m[e] = v[e];
                            am[e] = (unsigned)(a * k + b);
                        }
                }
            }
        store8(out + (((long long)n * Ho + ho) * Wo + wo) * ld_out + c0, m);
        if (idx != nullptr) {
            uint2 pk;
            pk.x = am[0] | (am[1] << 8) | (am[2] << 16) | (am[3] << 24);
            pk.y = am[4] | (am[5] << 8) | (am[6] << 16) | (am[7] << 24);
            *reinterpret_cast<uint2*>(idx + (i / CPP) * (long long)(CPP * 8) + c0) = pk;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(NTHR) void maxpool_bwd_kernel(const T* __restrict__ x, int ld_x, const T* __restrict__ go,
                                                           int ld_go, int N, int H, int W, int CPP, int k, int st,
                                                           int pd, int Ho, int Wo, T* __restrict__ dx, int ld_dx) {
    const long long total = (long long)N * H * W * CPP;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int c0 = (int)(i % CPP) * 8;
        long long q = i / CPP;
        const int w = (int)(q % W);
        q /= W;
        const int h = (int)(q % H);
        const int n = (int)(q / H);
        float me[8], g[8];
        load8(x + (((long long)n * H + h) * W + w) * ld_x + c0, me);
#pragma unroll
        for (int e = 0; e < 8; ++e) g[e] = 0.f;
        // windows (ho, wo) with ho*st - pd <= h <= ho*st - pd + k - 1
        int ho_lo = (h + pd - k + st) / st;
        if (h + pd - k + 1 < 0) ho_lo = 0;
        int wo_lo = (w + pd - k + st) / st;
        if (w + pd - k + 1 < 0) wo_lo = 0;
        const int ho_hi = min((h + pd) / st, Ho - 1), wo_hi = min((w + pd) / st, Wo - 1);
        for (int ho = ho_lo; ho <= ho_hi; ++ho)
            for (int wo = wo_lo; wo <= wo_hi; ++wo) {
                // is (h, w) the first maximum of window (ho, wo)?
                bool win[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) win[e] = true;
                for (int a = 0; a < k; ++a)
                    for (int b = 0; b < k; ++b) {
                        const int hi = ho * st - pd + a, wi = wo * st - pd + b;
                        if ((unsigned)hi >= (unsigned)H || (unsigned)wi >= (unsigned)W) continue;
                        if (hi == h && wi == w) continue;
                        const bool before = hi < h || (hi == h && wi < w);
                        float v[8];
                        load8(x + (((long long)n * H + hi) * W + wi) * ld_x + c0, v);
#pragma unroll
                        for (int e = 0; e < 8; ++e)
                            if (before ? v[e] >= me[e] : v[e] > me[e]) win[e] = false;
                    }
                float gv[8];
                load8(go + (((long long)n * Ho + ho) * Wo + wo) * ld_go + c0, gv);
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (win[e]) g[e] += gv[e];
            }
        store8(dx + (((long long)n * H + h) * W + w) * ld_dx + c0, g);
    }
}

// The same from the argmax positions the forward pass recorded (segnb_maxpool_fwd idx): a pixel reads one index vector and
// one gradient vector per covering window (<= ceil(k / stride)^2 of them) instead of re-scanning every window --
// 3x3 stride 2 at 256x256x64 (the ResNet stem of LinkNet34 at 512x512): 2.4 ms -> the price of a streaming pass.
// I32: N * H * W * CPP < 2^31 -- the index decomposition on 32-bit integers with reciprocal divisions (three 64-bit divisions per
// item were half of the kernel's issue slots: 89 -> 6x us on LinkNet34's stem, 16 x 256 x 256 x 64)
template <typename T, bool I32>
__global__ __launch_bounds__(NTHR) void maxpool_bwd_idx_kernel(const unsigned char* __restrict__ idx, const T* __restrict__ go,
                                                               int ld_go, int N, int H, int W, int CPP, int k, int st,
                                                               int pd, int Ho, int Wo, T* __restrict__ dx, int ld_dx,
                                                               const T* __restrict__ go2, int ld_go2) {
    // go2 (segnb_maxpool_bwd_add): a second gradient of the pooled tensor (two consumers: linknet.py:41-62's first BasicBlock and
    // its identity branch); the routed value is round(go + go2), what segnb_add would have stored
    const long long total = (long long)N * H * W * CPP;
    const FastDiv d_cpp(CPP), d_w(W), d_h(H);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        int c0, w, h, n;
        if constexpr (I32) {
            const int ii = (int)i;
            const int q0 = d_cpp.div(ii);
            c0 = (ii - q0 * CPP) * 8;
            const int q1 = d_w.div(q0);
            w = q0 - q1 * W;
            n = d_h.div(q1);
            h = q1 - n * H;
        } else {
            c0 = (int)(i % CPP) * 8;
            long long q = i / CPP;
            w = (int)(q % W);
            q /= W;
            h = (int)(q % H);
            n = (int)(q / H);
        }
        float g[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) g[e] = 0.f;
        int ho_lo = (h + pd - k + st) / st;
        if (h + pd - k + 1 < 0) ho_lo = 0;
        int wo_lo = (w + pd - k + st) / st;
        if (w + pd - k + 1 < 0) wo_lo = 0;
        const int ho_hi = min((h + pd) / st, Ho - 1), wo_hi = min((w + pd) / st, Wo - 1);
        for (int ho = ho_lo; ho <= ho_hi; ++ho)
            for (int wo = wo_lo; wo <= wo_hi; ++wo) {
                const unsigned mine = (unsigned)((h - (ho * st - pd)) * k + (w - (wo * st - pd)));
                const long long wpix = ((long long)n * Ho + ho) * Wo + wo;
                const uint2 pk = *reinterpret_cast<const uint2*>(idx + wpix * (long long)(CPP * 8) + c0);
                float gv[8];
                load8(go + wpix * ld_go + c0, gv);
                if (go2 != nullptr) {
                    float g2[8];
                    load8(go2 + wpix * ld_go2 + c0, g2);
#pragma unroll
                    for (int e = 0; e < 8; ++e) gv[e] = round_as(gv[e] + g2[e], (const T*)nullptr);
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const unsigned a = ((e < 4 ? pk.x : pk.y) >> (8 * (e & 3))) & 0xffu;
                    if (a == mine) g[e] += gv[e];
                }
            }
        store8(dx + (((long long)n * H + h) * W + w) * ld_dx + c0, g);
    }
}

template <typename T>
__global__ void nhwc_to_nchw_f32_kernel(const T* __restrict__ a, int ld, int N, int H, int W, int C,
                                        float* __restrict__ out) {
    const long long total = (long long)N * C * H * W;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const long long hw = i % ((long long)H * W);
        const long long q = i / ((long long)H * W);
        const int c = (int)(q % C);
        const long long n = q / C;
        out[i] = Elem<T>::to_f32(a[(n * H * W + hw) * ld + c]);
    }
}

}  // namespace

// torch.optim.RMSprop (alpha, eps; no momentum / centering / weight decay) and torch.optim.Adam (betas, eps; no
// amsgrad / weight decay) over the flat buffers: get_optimizer('rms' | 'adam') of torch_train.py:73-77
__global__ void rmsprop_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ sq, long long n,
                               float lr, float alpha, float eps) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += stride) {
        const float gi = g[i];
        const float v = alpha * sq[i] + (1.f - alpha) * gi * gi;
        sq[i] = v;
        p[i] -= lr * gi / (sqrtf(v) + eps);
    }
}

__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, long long n, float step_size, float beta1, float beta2,
                            float inv_sqrt_bc2, float eps) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += stride) {
        const float gi = g[i];
        const float mi = beta1 * m[i] + (1.f - beta1) * gi;         // exp_avg.lerp_(grad, 1 - beta1)
        const float vi = beta2 * v[i] + (1.f - beta2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        p[i] -= step_size * mi / (sqrtf(vi) * inv_sqrt_bc2 + eps);
    }
}

extern "C" int segnb_rmsprop_step(float* p, const float* g, float* square_avg, long long n, float lr, float alpha,
                                  float eps, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_rmsprop_step, p, g, square_avg, n, lr, alpha, eps, stream);
    SEGNB_CHECK_ARG(p && g && square_avg && n > 0, "bad arguments");
    int grid = ceil_div(n, 256);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(rmsprop_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, g, square_avg, n, lr, alpha, eps);
    SEGNB_LAUNCH_CHECK();
    return 0;
}

extern "C" int segnb_adam_step(float* p, const float* g, float* exp_avg, float* exp_avg_sq, long long n, float lr,
                               float beta1, float beta2, float eps, int step, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_adam_step, p, g, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step, stream);
    SEGNB_CHECK_ARG(p && g && exp_avg && exp_avg_sq && n > 0 && step >= 1, "bad arguments");
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    int grid = ceil_div(n, 256);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(adam_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, g, exp_avg, exp_avg_sq, n,
                       (float)((double)lr / bc1), beta1, beta2, (float)(1.0 / sqrt(bc2)), eps);
    SEGNB_LAUNCH_CHECK();
    return 0;
}

extern "C" int segnb_sgd_step(float* p, const float* g, long long n, float lr, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_sgd_step, p, g, n, lr, stream);
    SEGNB_CHECK_ARG(p && g && n > 0, "bad arguments");
    SEGNB_CHECK_ARG((((uintptr_t)p | (uintptr_t)g) & 15) == 0, "buffers must be 16-byte aligned");
    int grid = ceil_div(n / 4 + 1, 256);
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(sgd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, g, n, lr);
    SEGNB_LAUNCH_CHECK();
    return 0;
}

extern "C" int segnb_add(int dtype, const void* a, int ld_a, const void* b, int ld_b, void* out, int ld_out, int N,
                         int H, int W, int Cp, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_add, dtype, a, ld_a, b, ld_b, out, ld_out, N, H, W, Cp, stream);
    if (int rc = check_ew(N, H, W, Cp)) return rc;
    SEGNB_CHECK_ARG(out, "NULL tensor");
    const long long npix = (long long)N * H * W;
    int grid = ceil_div(npix * (Cp / 8), NTHR);
    if (grid > 4096) grid = 4096;
    if (int rc = segnb_dispatch_dtype(dtype, "segnb_add", [&](auto tag) SEGNB_INLINE_LAMBDA {
            using T = SEGNB_TAG_T(tag);
            hipLaunchKernelGGL(add_kernel<T>, dim3(grid), dim3(NTHR), 0, (hipStream_t)stream, (const T*)a, ld_a, (const T*)b, ld_b,
                               (T*)out, ld_out, npix, Cp / 8);
        }))
        return rc;
    SEGNB_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// nn.Upsample(scale_factor=2, mode='bilinear') of the DecoderBlock's non-deconvolution branch (lib/models/unet16.py:42-46;
// align_corners=False, torch's default): output row 2i = 0.25 in[i-1] + 0.75 in[i], row 2i+1 = 0.75 in[i] + 0.25 in[i+1] with the
// neighbour index clamped to the image (columns alike).  fp32 arithmetic in torch's order -- rows of column-interpolated values
// -- rounded once.  The backward is the exact transpose in gather form: an input pixel collects from the <= 4 x 4 outputs that
// read it, so no atomics and a fixed summation order.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void bilin_src(int o, int n, int& i0, int& i1, float& w0, float& w1) {
    const int i = o >> 1;
    if (o & 1) { i0 = i; i1 = i + 1 < n ? i + 1 : n - 1; w0 = 0.75f; w1 = 0.25f; }
    else       { i0 = i > 0 ? i - 1 : 0; i1 = i; w0 = 0.25f; w1 = 0.75f; }
}
template <typename T>
__global__ __launch_bounds__(NTHR) void upsample_bilinear2x_fwd_kernel(const T* __restrict__ x, int ld_x, int N, int H, int W, int CPP,
                                                                       T* __restrict__ out, int ld_out) {
    const int Ho = 2 * H, Wo = 2 * W;
    const long long total = (long long)N * Ho * Wo * CPP;
    for (long long i = blockIdx.x * (long long)NTHR + threadIdx.x; i < total; i += (long long)gridDim.x * NTHR) {
        const int cc = (int)(i % CPP);
        long long q = i / CPP;
        const int ox = (int)(q % Wo);
        q /= Wo;
        const int oy = (int)(q % Ho);
        const int n = (int)(q / Ho);
        int y0, y1, x0, x1;
        float wy0, wy1, wx0, wx1;
        bilin_src(oy, H, y0, y1, wy0, wy1);
        bilin_src(ox, W, x0, x1, wx0, wx1);
        float a[8], b[8], c[8], d[8], v[8];
        const T* base = x + (long long)n * H * W * ld_x + cc * 8;
        load8(base + ((long long)y0 * W + x0) * ld_x, a);
        load8(base + ((long long)y0 * W + x1) * ld_x, b);
        load8(base + ((long long)y1 * W + x0) * ld_x, c);
        load8(base + ((long long)y1 * W + x1) * ld_x, d);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = wy0 * (wx0 * a[e] + wx1 * b[e]) + wy1 * (wx0 * c[e] + wx1 * d[e]);
        store8(out + (((long long)n * Ho + oy) * Wo + ox) * ld_out + cc * 8, v);
    }
}
template <typename T>
__global__ __launch_bounds__(NTHR) void upsample_bilinear2x_bwd_kernel(const T* __restrict__ go, int ld_go, int N, int H, int W, int CPP,
                                                                       T* __restrict__ dx, int ld_dx) {
    const int Ho = 2 * H, Wo = 2 * W;
    const long long total = (long long)N * H * W * CPP;
    for (long long i = blockIdx.x * (long long)NTHR + threadIdx.x; i < total; i += (long long)gridDim.x * NTHR) {
        const int cc = (int)(i % CPP);
        long long q = i / CPP;
        const int ix = (int)(q % W);
        q /= W;
        const int iy = (int)(q % H);
        const int n = (int)(q / H);
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        for (int oy = 2 * iy - 2; oy <= 2 * iy + 3; ++oy) {
            if (oy < 0 || oy >= Ho) continue;
            int y0, y1;
            float wy0, wy1;
            bilin_src(oy, H, y0, y1, wy0, wy1);
            const float wy = (y0 == iy ? wy0 : 0.f) + (y1 == iy ? wy1 : 0.f);
            if (wy == 0.f) continue;
            for (int ox = 2 * ix - 2; ox <= 2 * ix + 3; ++ox) {
                if (ox < 0 || ox >= Wo) continue;
                int x0, x1;
                float wx0, wx1;
                bilin_src(ox, W, x0, x1, wx0, wx1);
                const float wx = (x0 == ix ? wx0 : 0.f) + (x1 == ix ? wx1 : 0.f);
                if (wx == 0.f) continue;
                float g[8];
                load8(go + (((long long)n * Ho + oy) * Wo + ox) * ld_go + cc * 8, g);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += (wy * wx) * g[e];
            }
        }
        store8(dx + (((long long)n * H + iy) * W + ix) * ld_dx + cc * 8, acc);
    }
}

extern "C" int segnb_upsample_bilinear2x_fwd(int dtype, const void* x, int ld_x, int N, int H, int W, int Cp, void* out, int ld_out,
                                             segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_upsample_bilinear2x_fwd, dtype, x, ld_x, N, H, W, Cp, out, ld_out, stream);
    if (int rc = check_ew(N, 2 * H, 2 * W, Cp)) return rc;
    SEGNB_CHECK_ARG(x && out && ld_x >= Cp && ld_out >= Cp, "bad arguments");
    int grid = ceil_div((long long)N * 4 * H * W * (Cp / 8), NTHR);
    if (grid > 16384) grid = 16384;
    if (int rc = segnb_dispatch_dtype(dtype, "segnb_upsample_bilinear2x_fwd", [&](auto tag) SEGNB_INLINE_LAMBDA {
            using T = SEGNB_TAG_T(tag);
            hipLaunchKernelGGL(upsample_bilinear2x_fwd_kernel<T>, dim3(grid), dim3(NTHR), 0, (hipStream_t)stream, (const T*)x, ld_x,
                               N, H, W, Cp / 8, (T*)out, ld_out);
        }))
        return rc;
    SEGNB_LAUNCH_CHECK();
    return 0;
}

extern "C" int segnb_upsample_bilinear2x_bwd(int dtype, const void* g_out, int ld_go, int N, int H, int W, int Cp, void* dx,
                                             int ld_dx, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_upsample_bilinear2x_bwd, dtype, g_out, ld_go, N, H, W, Cp, dx, ld_dx, stream);
    if (int rc = check_ew(N, 2 * H, 2 * W, Cp)) return rc;
    SEGNB_CHECK_ARG(g_out && dx && ld_go >= Cp && ld_dx >= Cp, "bad arguments");
    int grid = ceil_div((long long)N * H * W * (Cp / 8), NTHR);
    if (grid > 16384) grid = 16384;
    if (int rc = segnb_dispatch_dtype(dtype, "segnb_upsample_bilinear2x_bwd", [&](auto tag) SEGNB_INLINE_LAMBDA {
            using T = SEGNB_TAG_T(tag);
            hipLaunchKernelGGL(upsample_bilinear2x_bwd_kernel<T>, dim3(grid), dim3(NTHR), 0, (hipStream_t)stream, (const T*)g_out,
                               ld_go, N, H, W, Cp / 8, (T*)dx, ld_dx);
        }))
        return rc;
    SEGNB_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// nn.Upsample(scale_factor=2, mode='nearest') of lib/models/unet.py:53 (include/segnb_upsample.h): the bilinear pair above with
// the weights removed.  One lane per 16 bytes (8 bf16 / 4 fp32 channels) of one LOW-resolution pixel, the lanes of a wave over
// consecutive channels and then consecutive pixels of a row: the forward reads 1 and writes 4 vectors (the two of an output row
// are neighbours in memory), the backward reads 4 and writes 1.  Pixel row r = n * H + h of the source is rows 2r, 2r + 1 of
// the upsampled tensor, so the index takes two divisions (vectors per pixel, W); I32: the item count fits 32 bits and they
// are reciprocal multiplications (FastDiv, as maxpool_bwd_idx_kernel).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void load16(const float* p, float (&v)[4]) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
}
__device__ __forceinline__ void load16(const bf16_t* p, float (&v)[8]) { load8(p, v); }
__device__ __forceinline__ void store16(float* p, const float (&v)[4]) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void store16(bf16_t* p, const float (&v)[8]) { store8(p, v); }

// item -> (element offset of its vector in the low-resolution view of stride ld_lo, in the upsampled view of stride ld_hi)
template <typename T, bool I32>
__device__ __forceinline__ void nearest_item(long long i, int W, int VPP, const FastDiv& d_vpp, const FastDiv& d_w, int ld_lo,
                                             int ld_hi, long long& lo, long long& hi) {
    constexpr int E = 16 / (int)sizeof(T);
    long long pix, row;
    int c;
    if constexpr (I32) {
        const int p = d_vpp.div((int)i);
        c = (int)i - p * VPP;
        pix = p;
        row = d_w.div(p);
    } else {
        pix = i / VPP;
        c = (int)(i - pix * VPP);
        row = pix / W;
    }
    const long long w = pix - row * W;
    lo = pix * ld_lo + c * E;
    hi = (4 * row * W + 2 * w) * ld_hi + c * E;           // pixel (2 * row, 2 * w) of [N * 2H][2W]
}

template <typename T, bool I32>
__global__ __launch_bounds__(NTHR) void upsample_nearest2x_fwd_kernel(const T* __restrict__ x, int ld_x, long long total, int W, int VPP,
                                                                      T* __restrict__ out, int ld_out) {
    const FastDiv d_vpp(VPP), d_w(W);
    const long long below = 2ll * W * ld_out;               // the same column, one output row down
    for (long long i = blockIdx.x * (long long)NTHR + threadIdx.x; i < total; i += (long long)gridDim.x * NTHR) {
        long long lo, hi;
        nearest_item<T, I32>(i, W, VPP, d_vpp, d_w, ld_x, ld_out, lo, hi);
        const uint4 v = *reinterpret_cast<const uint4*>(x + lo);
        *reinterpret_cast<uint4*>(out + hi) = v;
        *reinterpret_cast<uint4*>(out + hi + ld_out) = v;
        *reinterpret_cast<uint4*>(out + hi + below) = v;
        *reinterpret_cast<uint4*>(out + hi + below + ld_out) = v;
    }
}

template <typename T, bool I32>
__global__ __launch_bounds__(NTHR) void upsample_nearest2x_bwd_kernel(const T* __restrict__ go, int ld_go, long long total, int W, int VPP,
                                                                      T* __restrict__ dx, int ld_dx) {
    constexpr int E = 16 / (int)sizeof(T);
    const FastDiv d_vpp(VPP), d_w(W);
    const long long below = 2ll * W * ld_go;
    for (long long i = blockIdx.x * (long long)NTHR + threadIdx.x; i < total; i += (long long)gridDim.x * NTHR) {
        long long lo, hi;
        nearest_item<T, I32>(i, W, VPP, d_vpp, d_w, ld_dx, ld_go, lo, hi);
        float a[E], b[E], c[E], d[E];
        load16(go + hi, a);
        load16(go + hi + ld_go, b);
        load16(go + hi + below, c);
        load16(go + hi + below + ld_go, d);
#pragma unroll
        for (int e = 0; e < E; ++e) a[e] = ((a[e] + b[e]) + c[e]) + d[e];      // scan order, as the g_up of the BatchNorm and ELU passes
        store16(dx + lo, a);
    }
}

// the checks of both directions, under the caller's name; lo / hi: the low-resolution and the upsampled view
static int check_nearest2x(const char* who, const void* lo, int ld_lo, const void* hi, int ld_hi, int N, int H, int W, int Cp) {
    SEGNB_CHECK_ARG_AS(who, N > 0 && H > 0 && W > 0 && Cp > 0 && Cp % 8 == 0, "bad NHWC shape (Cp % 8 != 0?)");
    SEGNB_CHECK_ARG_AS(who, (long long)N * H * W * 16 < (1ll << 31), "upsampled pixel count exceeds int32");
    SEGNB_CHECK_ARG_AS(who, lo != nullptr && hi != nullptr, "NULL tensor");
    SEGNB_CHECK_ARG_AS(who, ld_lo >= Cp && ld_hi >= Cp && ld_lo % 8 == 0 && ld_hi % 8 == 0, "pixel stride below Cp or not a multiple of 8");
    SEGNB_CHECK_ARG_AS(who, (((uintptr_t)lo | (uintptr_t)hi) & 15) == 0, "tensors must be 16-byte aligned");
    SEGNB_CHECK_ARG_AS(who, lo != hi, "the two tensors may not alias");
    return 0;
}

// 8 blocks per CU of 256 CUs, the rest by the grid-stride loop: 32 KiB of loads per CU and trip in the forward, 128 KiB in the backward
constexpr int NEAREST_MAX_BLOCKS = 2048;

extern "C" int segnb_upsample_nearest2x_fwd(int dtype, const void* x, int ld_x, int N, int H, int W, int Cp, void* out, int ld_out,
                                            segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_upsample_nearest2x_fwd, dtype, x, ld_x, N, H, W, Cp, out, ld_out, stream);
    if (int rc = check_nearest2x(__func__, x, ld_x, out, ld_out, N, H, W, Cp)) return rc;
    if (int rc = segnb_dispatch_dtype(dtype, "segnb_upsample_nearest2x_fwd", [&](auto tag) SEGNB_INLINE_LAMBDA {
            using T = SEGNB_TAG_T(tag);
            const int vpp = Cp / (16 / (int)sizeof(T));
            const long long total = (long long)N * H * W * vpp;
            int grid = ceil_div(total, NTHR);
            if (grid > NEAREST_MAX_BLOCKS) grid = NEAREST_MAX_BLOCKS;
            segnb_dispatch_bool(total < (1ll << 30), [&](auto I32) SEGNB_INLINE_LAMBDA {
                hipLaunchKernelGGL((upsample_nearest2x_fwd_kernel<T, decltype(I32)::value>), dim3(grid), dim3(NTHR), 0, (hipStream_t)stream,
                                   (const T*)x, ld_x, total, W, vpp, (T*)out, ld_out);
            });
        }))
        return rc;
    SEGNB_LAUNCH_CHECK();
    return 0;
}

extern "C" int segnb_upsample_nearest2x_bwd(int dtype, const void* g_out, int ld_go, int N, int H, int W, int Cp, void* dx, int ld_dx,
                                            segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_upsample_nearest2x_bwd, dtype, g_out, ld_go, N, H, W, Cp, dx, ld_dx, stream);
    if (int rc = check_nearest2x(__func__, dx, ld_dx, g_out, ld_go, N, H, W, Cp)) return rc;
    if (int rc = segnb_dispatch_dtype(dtype, "segnb_upsample_nearest2x_bwd", [&](auto tag) SEGNB_INLINE_LAMBDA {
            using T = SEGNB_TAG_T(tag);
            const int vpp = Cp / (16 / (int)sizeof(T));
            const long long total = (long long)N * H * W * vpp;
            int grid = ceil_div(total, NTHR);
            if (grid > NEAREST_MAX_BLOCKS) grid = NEAREST_MAX_BLOCKS;
            segnb_dispatch_bool(total < (1ll << 30), [&](auto I32) SEGNB_INLINE_LAMBDA {
                hipLaunchKernelGGL((upsample_nearest2x_bwd_kernel<T, decltype(I32)::value>), dim3(grid), dim3(NTHR), 0, (hipStream_t)stream,
                                   (const T*)g_out, ld_go, total, W, vpp, (T*)dx, ld_dx);
            });
        }))
        return rc;
    SEGNB_LAUNCH_CHECK();
    return 0;
}

extern "C" int segnb_maxpool_fwd(int dtype, const void* x, int ld_x, int N, int H, int W, int Cp, int k, int stride,
                                 int pad, void* out, int ld_out, unsigned char* idx, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_maxpool_fwd, dtype, x, ld_x, N, H, W, Cp, k, stride, pad, out, ld_out, idx, stream);
    if (int rc = check_ew(N, H, W, Cp)) return rc;
    SEGNB_CHECK_ARG(x && out && k >= 1 && stride >= 1 && pad >= 0 && pad < k, "bad pooling arguments");
    const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
    SEGNB_CHECK_ARG(Ho > 0 && Wo > 0, "empty pooled output");
    int grid = ceil_div((long long)N * Ho * Wo * (Cp / 8), NTHR);
    if (grid > 8192) grid = 8192;
    if (int rc = segnb_dispatch_dtype(dtype, "segnb_maxpool_fwd", [&](auto tag) SEGNB_INLINE_LAMBDA {
            using T = SEGNB_TAG_T(tag);
            hipLaunchKernelGGL(maxpool_fwd_kernel<T>, dim3(grid), dim3(NTHR), 0, (hipStream_t)stream, (const T*)x, ld_x, N, H, W,
                               Cp / 8, k, stride, pad, Ho, Wo, (T*)out, ld_out, idx);
        }))
        return rc;
    SEGNB_LAUNCH_CHECK();
    return 0;
}

static int maxpool_bwd_impl(int dtype, const void* x, int ld_x, const void* g_out, int ld_go, int N, int H, int W, int Cp, int k,
                            int stride, int pad, void* dx, int ld_dx, const unsigned char* idx, const void* g_out2, int ld_go2,
                            segnb_stream_t stream);

extern "C" int segnb_maxpool_bwd(int dtype, const void* x, int ld_x, const void* g_out, int ld_go, int N, int H, int W,
                                 int Cp, int k, int stride, int pad, void* dx, int ld_dx, const unsigned char* idx,
                                 segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_maxpool_bwd, dtype, x, ld_x, g_out, ld_go, N, H, W, Cp, k, stride, pad, dx, ld_dx, idx, stream);
    return maxpool_bwd_impl(dtype, x, ld_x, g_out, ld_go, N, H, W, Cp, k, stride, pad, dx, ld_dx, idx, nullptr, 0, stream);
}

extern "C" int segnb_maxpool_bwd_add(int dtype, const void* x, int ld_x, const void* g_out, int ld_go, const void* g_out2,
                                     int ld_go2, int N, int H, int W, int Cp, int k, int stride, int pad, void* dx, int ld_dx,
                                     const unsigned char* idx, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_maxpool_bwd_add, dtype, x, ld_x, g_out, ld_go, g_out2, ld_go2, N, H, W, Cp, k, stride, pad, dx, ld_dx, idx, stream);
    SEGNB_CHECK_ARG(g_out2 != nullptr && idx != nullptr, "the two-source form takes the recorded argmax positions");
    return maxpool_bwd_impl(dtype, x, ld_x, g_out, ld_go, N, H, W, Cp, k, stride, pad, dx, ld_dx, idx, g_out2, ld_go2, stream);
}

static int maxpool_bwd_impl(int dtype, const void* x, int ld_x, const void* g_out, int ld_go, int N, int H, int W, int Cp, int k,
                            int stride, int pad, void* dx, int ld_dx, const unsigned char* idx, const void* g_out2, int ld_go2,
                            segnb_stream_t stream) {
    if (int rc = check_ew(N, H, W, Cp)) return rc;
    SEGNB_CHECK_ARG(x && g_out && dx && k >= 1 && stride >= 1 && pad >= 0 && pad < k && k * k < 255, "bad pooling arguments");
    const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
    int grid = ceil_div((long long)N * H * W * (Cp / 8), NTHR);
    if (grid > 8192) grid = 8192;
    // (segnb_maxpool_bwd_add's dtype refusal has always carried segnb_maxpool_bwd's name)
    if (int rc = segnb_dispatch_dtype(dtype, "segnb_maxpool_bwd", [&](auto tag) SEGNB_INLINE_LAMBDA {
            using T = SEGNB_TAG_T(tag);
            if (idx == nullptr) {
                hipLaunchKernelGGL(maxpool_bwd_kernel<T>, dim3(grid), dim3(NTHR), 0, (hipStream_t)stream, (const T*)x, ld_x,
                                   (const T*)g_out, ld_go, N, H, W, Cp / 8, k, stride, pad, Ho, Wo, (T*)dx, ld_dx);
                return;
            }
            // the recorded argmax positions; the item index fits 32 bits or not
            segnb_dispatch_bool((long long)N * H * W * (Cp / 8) < (1ll << 31), [&](auto I32) SEGNB_INLINE_LAMBDA {
                hipLaunchKernelGGL((maxpool_bwd_idx_kernel<T, decltype(I32)::value>), dim3(grid), dim3(NTHR), 0, (hipStream_t)stream,
                                   idx, (const T*)g_out, ld_go, N, H, W, Cp / 8, k, stride, pad, Ho, Wo, (T*)dx, ld_dx,
                                   (const T*)g_out2, ld_go2);
            });
        }))
        return rc;
    SEGNB_LAUNCH_CHECK();
    return 0;
}

extern "C" int segnb_nhwc_to_nchw_f32(int dtype, const void* a, int ld, int N, int H, int W, int C, float* out,
                                      segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_nhwc_to_nchw_f32, dtype, a, ld, N, H, W, C, out, stream);
    SEGNB_CHECK_ARG(a && out && N > 0 && H > 0 && W > 0 && C > 0 && ld >= C, "bad arguments");
    int grid = ceil_div((long long)N * C * H * W, 256);
    if (grid > 8192) grid = 8192;
    if (int rc = segnb_dispatch_dtype(dtype, "segnb_nhwc_to_nchw_f32", [&](auto tag) SEGNB_INLINE_LAMBDA {
            using T = SEGNB_TAG_T(tag);
            hipLaunchKernelGGL(nhwc_to_nchw_f32_kernel<T>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const T*)a, ld, N, H, W,
                               C, out);
        }))
        return rc;
    SEGNB_LAUNCH_CHECK();
    return 0;
}
