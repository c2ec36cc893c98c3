// GCN decoder kernels, gfx950: Global Convolution Module, Boundary Refine Module and the align_corners=True bilinear resize of
// the reference's lib/models/gcn152.py:9-48, 98-115 (ABI: include/segnb_gcn.h).
//
// The decoder maps are K <= 32 channels wide (K = num_classes): every kernel here is a bandwidth-bound stencil on fp32 planar
// [N][K][H][W] maps or a thin convolution that reads a C-wide NHWC encoder feature.  Vector fp32 FMA throughout (GCM at K = 32
// on the 128 x 128 feature is ~15 GFLOP per step); consecutive lanes take consecutive pixels, so a wave reads 256 contiguous
// bytes of a plane, and the weights -- read in their own nn.Conv2d layout -- are wave-uniform loads.
//
// Determinism: parameter gradients reduce over N*H*W pixels.  Each workgroup sums its lanes with a fixed butterfly per wave,
// the four waves in wave order, and writes ONE row of partial sums; a finish launch adds the rows in block order into the
// gradient.  The resize backward is a gather (each input pixel sums the output pixels that read it, in output order).  No
// floating-point atomics anywhere.
#include "common.h"
#include "../../include/segnb_gcn.h"

namespace {

constexpr int BS = 256;          // threads per workgroup everywhere
constexpr int GT = 7;            // GCM window (gcn152.py:72-75: kernel_size (7, 7))
constexpr int MAXT = 9;          // taps of the planar convolutions: 1x7, 7x1, 3x3
constexpr int JB = 4;            // input channels per workgroup of the planar weight gradient
constexpr int PV = JB * MAXT + 1;               // values per partial row of the planar weight gradient (+ bias)
constexpr int GV = 2 * GT * 8 + 2;              // values per partial row of the GCM first-stage weight gradient
constexpr int MAX_WG_BLOCKS = 16384;            // workgroups of one weight-gradient launch (bounds the partial rows)

// ---------------------------------------------------------------------------------------------------------------------------
// planar stride-1 "same" convolutions on [N][J][H][W] fp32 maps, weight [K][J][kh][kw]
// ---------------------------------------------------------------------------------------------------------------------------
// out[k][p] = act(bias[k] + sum_j sum_t w[k][j][t] in[j][p + d(t)]) + res[k][p]; d(t) = (t / kw - (kh-1)/2, t % kw - (kw-1)/2).
// res may alias out (each lane reads its own pixels before it writes them).
template <int KM>
__global__ __launch_bounds__(BS) void pconv_fwd_kernel(const float* __restrict__ in, int J, const float* __restrict__ wt, int kh,
                                                       int kw, const float* __restrict__ bias, const float* res, int relu,
                                                       float* out, int N, int H, int W, int K) {
    const int HW = H * W;
    const int pix = blockIdx.x * BS + threadIdx.x;
    if (pix >= N * HW) return;
    const int n = pix / HW, r = pix - n * HW, h = r / W, x = r - h * W;
    const int T = kh * kw, ph = (kh - 1) / 2, pw = (kw - 1) / 2;
    float acc[KM];
#pragma unroll
    for (int k = 0; k < KM; ++k) acc[k] = (k < K && bias != nullptr) ? bias[k] : 0.f;
    const float* inn = in + (long long)n * J * HW;
    for (int j = 0; j < J; ++j) {
        for (int t = 0; t < T; ++t) {
            const int hh = h + t / kw - ph, xx = x + t % kw - pw;
            const bool ok = hh >= 0 && hh < H && xx >= 0 && xx < W;
            const float v = ok ? inn[(long long)j * HW + hh * W + xx] : 0.f;
#pragma unroll
            for (int k = 0; k < KM; ++k)
                if (k < K) acc[k] += wt[((long long)k * J + j) * T + t] * v;
        }
    }
    const long long o = (long long)n * K * HW + r;
#pragma unroll
    for (int k = 0; k < KM; ++k)
        if (k < K) {
            float v = acc[k];
            if (relu) v = fmaxf(v, 0.f);
            if (res != nullptr) v += res[o + (long long)k * HW];
            out[o + (long long)k * HW] = v;
        }
}

// din[j][p] = mask(r[j][p] > 0) * sum_k sum_t w[k][j][t] dy[k][p - d(t)] + res[j][p]  (the transposed stencil, J <= KM)
template <int KM>
__global__ __launch_bounds__(BS) void pconv_dgrad_kernel(const float* __restrict__ dy, int K, const float* __restrict__ wt, int kh,
                                                         int kw, const float* __restrict__ mask, const float* __restrict__ res,
                                                         float* __restrict__ din, int N, int H, int W, int J) {
    const int HW = H * W;
    const int pix = blockIdx.x * BS + threadIdx.x;
    if (pix >= N * HW) return;
    const int n = pix / HW, r = pix - n * HW, h = r / W, x = r - h * W;
    const int T = kh * kw, ph = (kh - 1) / 2, pw = (kw - 1) / 2;
    float acc[KM];
#pragma unroll
    for (int j = 0; j < KM; ++j) acc[j] = 0.f;
    const float* dyn = dy + (long long)n * K * HW;
    for (int k = 0; k < K; ++k) {
        for (int t = 0; t < T; ++t) {
            const int hh = h - (t / kw - ph), xx = x - (t % kw - pw);
            const bool ok = hh >= 0 && hh < H && xx >= 0 && xx < W;
            const float g = ok ? dyn[(long long)k * HW + hh * W + xx] : 0.f;
#pragma unroll
            for (int j = 0; j < KM; ++j)
                if (j < J) acc[j] += wt[((long long)k * J + j) * T + t] * g;
        }
    }
    const long long o = (long long)n * J * HW + r;
#pragma unroll
    for (int j = 0; j < KM; ++j)
        if (j < J) {
            float v = acc[j];
            if (mask != nullptr && !(mask[o + (long long)j * HW] > 0.f)) v = 0.f;
            if (res != nullptr) v += res[o + (long long)j * HW];
            din[o + (long long)j * HW] = v;
        }
}

// the workgroup's sum of v (fixed order: butterfly per wave, waves 0..3) -> lane 0 of wave 0; red: LDS [4]
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[wv] = v;
    __syncthreads();
    const float s = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return s;
}

// partial rows of dw[k][j][t] = sum_p dy[k][p] in[j][p + d(t)] and db[k] = sum_p dy[k][p]: grid (GX, K * JG), JG = ceil(J / JB);
// row (k * JG + jg) * GX + bx, slot jj * MAXT + t, bias at slot JB * MAXT (rows of jg = 0)
__global__ __launch_bounds__(BS) void pconv_wgrad_kernel(const float* __restrict__ dy, int K, const float* __restrict__ in, int J,
                                                         int kh, int kw, int N, int H, int W, float* __restrict__ part) {
    __shared__ float red[4];
    const int HW = H * W, npix = N * HW;
    const int JG = (J + JB - 1) / JB;
    const int k = blockIdx.y / JG, jg = blockIdx.y - k * JG, j0 = jg * JB;
    const int T = kh * kw, ph = (kh - 1) / 2, pw = (kw - 1) / 2;
    float acc[JB][MAXT], accb = 0.f;
#pragma unroll
    for (int jj = 0; jj < JB; ++jj)
#pragma unroll
        for (int t = 0; t < MAXT; ++t) acc[jj][t] = 0.f;
    for (int pix = blockIdx.x * BS + threadIdx.x; pix < npix; pix += gridDim.x * BS) {
        const int n = pix / HW, r = pix - n * HW, h = r / W, x = r - h * W;
        const float g = dy[((long long)n * K + k) * HW + r];
        accb += g;
#pragma unroll
        for (int jj = 0; jj < JB; ++jj) {
            const int j = j0 + jj;
            if (j >= J) break;
            const float* inj = in + ((long long)n * J + j) * HW;
#pragma unroll
            for (int t = 0; t < MAXT; ++t)
                if (t < T) {
                    const int hh = h + t / kw - ph, xx = x + t % kw - pw;
                    if (hh >= 0 && hh < H && xx >= 0 && xx < W) acc[jj][t] += g * inj[hh * W + xx];
                }
        }
    }
    float* prow = part + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * PV;
#pragma unroll
    for (int jj = 0; jj < JB; ++jj)
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            const float s = block_sum(acc[jj][t], red);
            if (threadIdx.x == 0) prow[jj * MAXT + t] = s;
        }
    const float sb = block_sum(accb, red);
    if (threadIdx.x == 0) prow[JB * MAXT] = sb;
}

// dw[k][j][t] += the sum of its GX partial rows; db[k] likewise.  One workgroup per output: lanes stride the rows, then the
// fixed-order block sum (the same rows, the same order, every launch).
__global__ __launch_bounds__(BS) void pconv_wgrad_finish_kernel(const float* __restrict__ part, int GX, int K, int J, int T,
                                                                float* __restrict__ dw, float* __restrict__ db) {
    __shared__ float red[4];
    const int o = blockIdx.x;
    const int JG = (J + JB - 1) / JB;
    const int nw = K * J * T;
    int row, slot;
    if (o < nw) {
        const int k = o / (J * T), j = (o / T) % J, t = o % T;
        row = k * JG + j / JB;
        slot = (j % JB) * MAXT + t;
    } else {
        row = (o - nw) * JG;
        slot = JB * MAXT;
    }
    float s = 0.f;
    for (int bx = threadIdx.x; bx < GX; bx += BS) s += part[((long long)row * GX + bx) * PV + slot];
    s = block_sum(s, red);
    if (threadIdx.x == 0) {
        if (o < nw) {
            if (dw != nullptr) dw[o] += s;
        } else if (db != nullptr) {
            db[o - nw] += s;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// GCM first stage: conv_l1 (7x1, pad (3,0)) and conv_r1 (1x7, pad (0,3)), C -> K, on the NHWC feature times the Dropout2d table
// ---------------------------------------------------------------------------------------------------------------------------
// 64 pixels per workgroup, the four waves split the 8-channel chunks (wave w: chunks w, w + 4, ...) and add their K-wide partial
// sums through LDS in wave order.  Each lane loads its pixel's 13 distinct window positions once per chunk.
template <typename T, int KM>
__global__ __launch_bounds__(BS) void gcm1_fwd_kernel(const T* __restrict__ x, int ld, int N, int H, int W, int C, int K,
                                                      const float* __restrict__ drop, const float* __restrict__ wl,
                                                      const float* __restrict__ bl, const float* __restrict__ wr,
                                                      const float* __restrict__ br, float* __restrict__ yl,
                                                      float* __restrict__ yr) {
    __shared__ float red[3][8][64];
    const int HW = H * W;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int pix = blockIdx.x * 64 + lane;
    const bool valid = pix < N * HW;
    const int pc = valid ? pix : 0;
    const int n = pc / HW, r = pc - n * HW, h = r / W, w = r - h * W;
    constexpr int NV = 2 * KM;
    float acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.f;
    const int NC = C / 8;
    if (valid) {
        for (int cc = wv; cc < NC; cc += 4) {
            const int c0 = cc * 8;
            float dm[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) dm[e] = drop != nullptr ? drop[(long long)n * C + c0 + e] : 1.f;
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                const float* wt = side == 0 ? wl : wr;
                for (int t = 0; t < GT; ++t) {
                    const int hh = side == 0 ? h + t - 3 : h, ww = side == 0 ? w : w + t - 3;
                    if (hh < 0 || hh >= H || ww < 0 || ww >= W) continue;
                    float v[8];
                    load8(x + ((long long)(n * H + hh) * W + ww) * ld + c0, v);
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] *= dm[e];
#pragma unroll
                    for (int k = 0; k < KM; ++k)
                        if (k < K) {
                            const float* wk = wt + ((long long)k * C + c0) * GT + t;
                            float s = acc[side * KM + k];
#pragma unroll
                            for (int e = 0; e < 8; ++e) s += wk[e * GT] * v[e];
                            acc[side * KM + k] = s;
                        }
                }
            }
        }
    }
    // waves 1..3 hand their partial sums to wave 0, eight values at a time, added in wave order
#pragma unroll
    for (int g0 = 0; g0 < NV; g0 += 8) {
        if (wv > 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (g0 + i < NV) red[wv - 1][i][lane] = acc[g0 + i];
        }
        __syncthreads();
        if (wv == 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (g0 + i < NV) acc[g0 + i] = ((acc[g0 + i] + red[0][i][lane]) + red[1][i][lane]) + red[2][i][lane];
        }
        __syncthreads();
    }
    if (wv == 0 && valid) {
        const long long o = (long long)n * K * HW + r;
#pragma unroll
        for (int k = 0; k < KM; ++k)
            if (k < K) {
                yl[o + (long long)k * HW] = acc[k] + (bl != nullptr ? bl[k] : 0.f);
                yr[o + (long long)k * HW] = acc[KM + k] + (br != nullptr ? br[k] : 0.f);
            }
    }
}

// partial rows of the first-stage weight / bias gradients: grid (GX, C / 8, K).  Lane q loads its 8 channels of (drop * x)[q]
// ONCE and pairs them with the 7 + 7 output gradients that read them: dw_l[k][c][t] += dyl[k][q - (t-3, 0)] xd[q][c],
// dw_r[k][c][t] += dyr[k][q - (0, t-3)] xd[q][c].  Row ((k * NC + cc) * GX + bx): slots t * 8 + e (l), 56 + t * 8 + e (r),
// 112 / 113 the biases (rows of chunk 0)
template <typename T>
__global__ __launch_bounds__(BS) void gcm1_wgrad_kernel(const T* __restrict__ x, int ld, int N, int H, int W, int C, int K,
                                                        const float* __restrict__ drop, const float* __restrict__ dyl,
                                                        const float* __restrict__ dyr, float* __restrict__ part) {
    __shared__ float red[4];
    const int HW = H * W, npix = N * HW;
    const int cc = blockIdx.y, k = blockIdx.z, c0 = cc * 8;
    float al[GT][8], ar[GT][8], bl = 0.f, brs = 0.f;
#pragma unroll
    for (int t = 0; t < GT; ++t)
#pragma unroll
        for (int e = 0; e < 8; ++e) al[t][e] = ar[t][e] = 0.f;
    for (int q = blockIdx.x * BS + threadIdx.x; q < npix; q += gridDim.x * BS) {
        const int n = q / HW, r = q - n * HW, h = r / W, w = r - h * W;
        float v[8];
        load8(x + (long long)q * ld + c0, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] *= drop != nullptr ? drop[(long long)n * C + c0 + e] : 1.f;
        const float* gl = dyl + ((long long)n * K + k) * HW;
        const float* gr = dyr + ((long long)n * K + k) * HW;
        if (cc == 0) {
            bl += gl[r];
            brs += gr[r];
        }
#pragma unroll
        for (int t = 0; t < GT; ++t) {
            const int hp = h - (t - 3), wp = w - (t - 3);
            const float a = (hp >= 0 && hp < H) ? gl[hp * W + w] : 0.f;
            const float b = (wp >= 0 && wp < W) ? gr[h * W + wp] : 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                al[t][e] += a * v[e];
                ar[t][e] += b * v[e];
            }
        }
    }
    float* prow = part + (((long long)k * gridDim.y + cc) * gridDim.x + blockIdx.x) * GV;
#pragma unroll
    for (int t = 0; t < GT; ++t)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float s = block_sum(al[t][e], red);
            if (threadIdx.x == 0) prow[t * 8 + e] = s;
            const float s2 = block_sum(ar[t][e], red);
            if (threadIdx.x == 0) prow[GT * 8 + t * 8 + e] = s2;
        }
    const float s3 = block_sum(bl, red);
    const float s4 = block_sum(brs, red);
    if (threadIdx.x == 0) {
        prow[2 * GT * 8] = s3;
        prow[2 * GT * 8 + 1] = s4;
    }
}

// g_wl1 / g_wr1 [K][C][7] and g_bl1 / g_br1 [K] += the partial rows, in block order
__global__ __launch_bounds__(BS) void gcm1_wgrad_finish_kernel(const float* __restrict__ part, int GX, int K, int C,
                                                               float* __restrict__ gwl, float* __restrict__ gbl,
                                                               float* __restrict__ gwr, float* __restrict__ gbr) {
    const int o = blockIdx.x * BS + threadIdx.x;
    const int nw = K * C * GT, NC = C / 8;
    if (o >= 2 * nw + 2 * K) return;
    int k, slot, cc = 0;
    if (o < 2 * nw) {
        const int side = o / nw, i = o - side * nw;
        k = i / (C * GT);
        const int c = (i / GT) % C, t = i % GT;
        cc = c / 8;
        slot = side * GT * 8 + t * 8 + (c & 7);
    } else {
        const int i = o - 2 * nw;
        k = i % K;
        slot = 2 * GT * 8 + i / K;
    }
    float s = 0.f;
    const long long row = (long long)k * NC + cc;
    for (int bx = 0; bx < GX; ++bx) s += part[(row * GX + bx) * GV + slot];
    if (o < nw) {
        if (gwl != nullptr) gwl[o] += s;
    } else if (o < 2 * nw) {
        if (gwr != nullptr) gwr[o - nw] += s;
    } else if (o < 2 * nw + K) {
        if (gbl != nullptr) gbl[k] += s;
    } else if (gbr != nullptr) {
        gbr[k] += s;
    }
}

// dx[q][c] = drop[n][c] (sum_k sum_t wl[k][c][t] dyl[k][q - (t-3, 0)] + wr[k][c][t] dyr[k][q - (0, t-3)]): grid (pixel blocks,
// C / 8); the chunk is the workgroup's, so the weights are wave-uniform loads
template <typename T>
__global__ __launch_bounds__(BS) void gcm1_dx_kernel(const float* __restrict__ dyl, const float* __restrict__ dyr, int N, int H,
                                                     int W, int C, int K, const float* __restrict__ wl,
                                                     const float* __restrict__ wr, const float* __restrict__ drop,
                                                     T* __restrict__ dx, int ld_dx) {
    const int HW = H * W;
    const int q = blockIdx.x * BS + threadIdx.x;
    if (q >= N * HW) return;
    const int n = q / HW, r = q - n * HW, h = r / W, w = r - h * W;
    const int c0 = blockIdx.y * 8;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    for (int k = 0; k < K; ++k) {
        const float* gl = dyl + ((long long)n * K + k) * HW;
        const float* gr = dyr + ((long long)n * K + k) * HW;
        const float* wlk = wl + ((long long)k * C + c0) * GT;
        const float* wrk = wr + ((long long)k * C + c0) * GT;
#pragma unroll
        for (int t = 0; t < GT; ++t) {
            const int hp = h - (t - 3), wp = w - (t - 3);
            const float a = (hp >= 0 && hp < H) ? gl[hp * W + w] : 0.f;
            const float b = (wp >= 0 && wp < W) ? gr[h * W + wp] : 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += wlk[e * GT + t] * a + wrk[e * GT + t] * b;
        }
    }
    if (drop != nullptr) {
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] *= drop[(long long)n * C + c0 + e];
    }
    store8(dx + (long long)q * ld_dx + c0, acc);
}

// ---------------------------------------------------------------------------------------------------------------------------
// bilinear resize, align_corners=True (F.interpolate: source = dst * (in - 1) / (out - 1), fp32)
// ---------------------------------------------------------------------------------------------------------------------------
float ac_scale_host(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

// the weight with which output row Y reads input row y (0 when it does not)
__device__ __forceinline__ float ac_weight(int Y, int y, float sc, int in) {
    const float s = sc * (float)Y;
    const int y0 = (int)s;
    const float l1 = s - (float)y0, l0 = 1.f - l1;
    const int y1 = y0 + (y0 < in - 1 ? 1 : 0);
    float w = 0.f;
    if (y0 == y) w += l0;
    if (y1 == y) w += l1;
    return w;
}

__global__ __launch_bounds__(BS) void resize_ac_fwd_kernel(const float* __restrict__ in, int NK, int h, int w, int H, int W,
                                                           float sh, float sw, const float* __restrict__ skip,
                                                           float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * BS + threadIdx.x;
    if (i >= (long long)NK * H * W) return;
    const int X = (int)(i % W), Y = (int)((i / W) % H);
    const long long nk = i / ((long long)H * W);
    const float fy = sh * (float)Y, fx = sw * (float)X;
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float ly = fy - (float)y0, lx = fx - (float)x0;
    const float* p = in + nk * h * w;
    float v = (1.f - ly) * ((1.f - lx) * p[y0 * w + x0] + lx * p[y0 * w + x1]) +
              ly * ((1.f - lx) * p[y1 * w + x0] + lx * p[y1 * w + x1]);
    if (skip != nullptr) v += skip[i];
    out[i] = v;
}

// first output index whose source coordinate can reach input index y - 1 (a safe lower bound), and the last one reaching y + 1
__device__ __forceinline__ void ac_range(int y, float sc, int in, int out, int& lo, int& hi) {
    if (sc <= 0.f) {
        lo = 0;
        hi = out - 1;
        return;
    }
    lo = (int)floorf((float)(y - 1) / sc) - 1;
    hi = (int)ceilf((float)(y + 1) / sc) + 1;
    lo = lo < 0 ? 0 : lo;
    hi = hi > out - 1 ? out - 1 : hi;
}

__global__ __launch_bounds__(BS) void resize_ac_bwd_kernel(const float* __restrict__ dout, int NK, int h, int w, int H, int W,
                                                           float sh, float sw, float* __restrict__ din) {
    const long long i = (long long)blockIdx.x * BS + threadIdx.x;
    if (i >= (long long)NK * h * w) return;
    const int x = (int)(i % w), y = (int)((i / w) % h);
    const long long nk = i / ((long long)h * w);
    int ylo, yhi, xlo, xhi;
    ac_range(y, sh, h, H, ylo, yhi);
    ac_range(x, sw, w, W, xlo, xhi);
    const float* g = dout + nk * H * W;
    float acc = 0.f;
    for (int Y = ylo; Y <= yhi; ++Y) {
        const float wy = ac_weight(Y, y, sh, h);
        if (wy == 0.f) continue;
        float row = 0.f;
        for (int X = xlo; X <= xhi; ++X) {
            const float wx = ac_weight(X, x, sw, w);
            if (wx != 0.f) row += wx * g[(long long)Y * W + X];
        }
        acc += wy * row;
    }
    din[i] = acc;
}

// ---------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------
int kbucket(int K) { return K <= 1 ? 1 : K <= 4 ? 4 : K <= 8 ? 8 : K <= 16 ? 16 : 32; }

#define GCN_KM_SWITCH(K_, MACRO) \
    switch (kbucket(K_)) {       \
        case 1: MACRO(1); break; \
        case 4: MACRO(4); break; \
        case 8: MACRO(8); break; \
        case 16: MACRO(16); break; \
        default: MACRO(32); break; \
    }

void pconv_fwd(const float* in, int J, const float* wt, int kh, int kw, const float* bias, const float* res, int relu, float* out,
               int N, int H, int W, int K, hipStream_t st) {
    const int grid = ceil_div((long long)N * H * W, BS);
#define GCN_PF(KM_) pconv_fwd_kernel<KM_><<<grid, BS, 0, st>>>(in, J, wt, kh, kw, bias, res, relu, out, N, H, W, K)
    GCN_KM_SWITCH(K, GCN_PF)
#undef GCN_PF
}

void pconv_dgrad(const float* dy, int K, const float* wt, int kh, int kw, const float* mask, const float* res, float* din, int N,
                 int H, int W, int J, hipStream_t st) {
    const int grid = ceil_div((long long)N * H * W, BS);
#define GCN_PD(KM_) pconv_dgrad_kernel<KM_><<<grid, BS, 0, st>>>(dy, K, wt, kh, kw, mask, res, din, N, H, W, J)
    GCN_KM_SWITCH(J, GCN_PD)
#undef GCN_PD
}

// workgroups along the pixels of the planar weight gradient
int pconv_wgrad_gx(int N, int H, int W, int K, int J) {
    const int rows = K * ((J + JB - 1) / JB);
    int gx = ceil_div((long long)N * H * W, BS * 8);
    const int cap = MAX_WG_BLOCKS / rows > 2048 ? 2048 : MAX_WG_BLOCKS / rows;
    if (gx > cap) gx = cap;
    return gx < 1 ? 1 : gx;
}

size_t pconv_wgrad_floats(int N, int H, int W, int K, int J) {
    return (size_t)pconv_wgrad_gx(N, H, W, K, J) * K * ((J + JB - 1) / JB) * PV;
}

void pconv_wgrad(const float* dy, int K, const float* in, int J, int kh, int kw, int N, int H, int W, float* part, float* dw,
                 float* db, hipStream_t st) {
    const int gx = pconv_wgrad_gx(N, H, W, K, J);
    pconv_wgrad_kernel<<<dim3(gx, K * ((J + JB - 1) / JB)), BS, 0, st>>>(dy, K, in, J, kh, kw, N, H, W, part);
    pconv_wgrad_finish_kernel<<<K * J * kh * kw + K, BS, 0, st>>>(part, gx, K, J, kh * kw, dw, db);
}

int gcm1_wgrad_gx(int N, int H, int W, int C, int K) {
    const int rows = (C / 8) * K;
    int gx = ceil_div((long long)N * H * W, BS * 16);
    const int cap = MAX_WG_BLOCKS / rows > 128 ? 128 : MAX_WG_BLOCKS / rows;
    if (gx > cap) gx = cap;
    return gx < 1 ? 1 : gx;
}

bool gcn_ok(int C, int K, int N, int H, int W) {
    if (K < 1 || K > SEGNB_GCN_MAX_K || N < 1 || H < 1 || W < 1) return false;
    if (C != 0 && (C < 8 || C % 8 != 0 || C > SEGNB_GCN_MAX_C)) return false;
    // pixel indices are 32-bit; the planar maps' element offsets too
    return (long long)N * H * W * K < (1ll << 31);
}

}  // namespace

extern "C" int segnb_gcn_ok(int C, int K, int N, int H, int W) { return gcn_ok(C, K, N, H, W) ? 1 : 0; }

extern "C" int segnb_gcm_fwd(int dtype, const void* x, int ld, int N, int H, int W, int C, int K, const float* drop,
                             const float* w_l1, const float* b_l1, const float* w_l2, const float* b_l2, const float* w_r1,
                             const float* b_r1, const float* w_r2, const float* b_r2, float* yl, float* yr, float* out,
                             segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_gcm_fwd, dtype, x, ld, N, H, W, C, K, drop, w_l1, b_l1, w_l2, b_l2, w_r1, b_r1, w_r2, b_r2, yl, yr,
                      out, stream);
    SEGNB_CHECK_ARG(x && w_l1 && w_l2 && w_r1 && w_r2 && yl && yr && out, "NULL tensor");
    SEGNB_CHECK_ARG(C > 0 && gcn_ok(C, K, N, H, W), "1 <= K <= 32, C a multiple of 8 up to 2048 (segnb_gcn_ok)");
    SEGNB_CHECK_ARG(ld % 8 == 0 && ld >= C, "feature pixel stride");
    SEGNB_CHECK_ARG(dtype == SEGNB_F32 || dtype == SEGNB_BF16, "dtype");
    hipStream_t st = (hipStream_t)stream;
    const int grid = ceil_div((long long)N * H * W, 64);
#define GCN_G1(TT, KM_)                                                                                                   \
    gcm1_fwd_kernel<TT, KM_><<<grid, BS, 0, st>>>((const TT*)x, ld, N, H, W, C, K, drop, w_l1, b_l1, w_r1, b_r1, yl, yr)
#define GCN_G1F(KM_) GCN_G1(float, KM_)
#define GCN_G1B(KM_) GCN_G1(bf16_t, KM_)
    if (dtype == SEGNB_BF16) {
        GCN_KM_SWITCH(K, GCN_G1B)
    } else {
        GCN_KM_SWITCH(K, GCN_G1F)
    }
#undef GCN_G1B
#undef GCN_G1F
#undef GCN_G1
    SEGNB_LAUNCH_CHECK();
    // out = conv_l2(yl) + b_l2, then out += conv_r2(yr) + b_r2 (gcn152.py:29-33: x_l + x_r)
    pconv_fwd(yl, K, w_l2, 1, GT, b_l2, nullptr, 0, out, N, H, W, K, st);
    pconv_fwd(yr, K, w_r2, GT, 1, b_r2, out, 0, out, N, H, W, K, st);
    SEGNB_LAUNCH_CHECK();
    return 0;
}

extern "C" int segnb_gcm_bwd(int dtype, const void* x, int ld, int N, int H, int W, int C, int K, const float* drop,
                             const float* w_l1, const float* w_l2, const float* w_r1, const float* w_r2, const float* yl,
                             const float* yr, const float* dout, float* dyl, float* dyr, void* dx, int ld_dx, float* g_wl1,
                             float* g_bl1, float* g_wl2, float* g_bl2, float* g_wr1, float* g_br1, float* g_wr2, float* g_br2,
                             segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_gcm_bwd, dtype, x, ld, N, H, W, C, K, drop, w_l1, w_l2, w_r1, w_r2, yl, yr, dout, dyl, dyr, dx, ld_dx,
                      g_wl1, g_bl1, g_wl2, g_bl2, g_wr1, g_br1, g_wr2, g_br2, stream);
    SEGNB_CHECK_ARG(x && w_l1 && w_l2 && w_r1 && w_r2 && yl && yr && dout && dyl && dyr, "NULL tensor");
    SEGNB_CHECK_ARG(C > 0 && gcn_ok(C, K, N, H, W), "1 <= K <= 32, C a multiple of 8 up to 2048 (segnb_gcn_ok)");
    SEGNB_CHECK_ARG(ld % 8 == 0 && ld >= C, "feature pixel stride");
    SEGNB_CHECK_ARG(dx == nullptr || (ld_dx % 8 == 0 && ld_dx >= C), "gradient pixel stride");
    SEGNB_CHECK_ARG(dtype == SEGNB_F32 || dtype == SEGNB_BF16, "dtype");
    hipStream_t st = (hipStream_t)stream;
    const int gx1 = gcm1_wgrad_gx(N, H, W, C, K);
    size_t need = (size_t)gx1 * (C / 8) * K * GV;
    const size_t need2 = pconv_wgrad_floats(N, H, W, K, K);
    if (need2 > need) need = need2;
    float* part = segnb_head_scratch(need * sizeof(float), st);
    if (part == nullptr) return SEGNB_E_BADARG;
    // second stage: dyl = conv_l2^T(dout), dyr = conv_r2^T(dout), their weight / bias gradients
    pconv_dgrad(dout, K, w_l2, 1, GT, nullptr, nullptr, dyl, N, H, W, K, st);
    pconv_dgrad(dout, K, w_r2, GT, 1, nullptr, nullptr, dyr, N, H, W, K, st);
    if (g_wl2 != nullptr || g_bl2 != nullptr) pconv_wgrad(dout, K, yl, K, 1, GT, N, H, W, part, g_wl2, g_bl2, st);
    if (g_wr2 != nullptr || g_br2 != nullptr) pconv_wgrad(dout, K, yr, K, GT, 1, N, H, W, part, g_wr2, g_br2, st);
    SEGNB_LAUNCH_CHECK();
    // first stage: weight / bias gradients (the feature read once per class), then the feature's gradient
    if (g_wl1 != nullptr || g_bl1 != nullptr || g_wr1 != nullptr || g_br1 != nullptr) {
        const dim3 grid(gx1, C / 8, K);
        if (dtype == SEGNB_BF16)
            gcm1_wgrad_kernel<bf16_t><<<grid, BS, 0, st>>>((const bf16_t*)x, ld, N, H, W, C, K, drop, dyl, dyr, part);
        else
            gcm1_wgrad_kernel<float><<<grid, BS, 0, st>>>((const float*)x, ld, N, H, W, C, K, drop, dyl, dyr, part);
        gcm1_wgrad_finish_kernel<<<ceil_div(2ll * K * C * GT + 2 * K, BS), BS, 0, st>>>(part, gx1, K, C, g_wl1, g_bl1, g_wr1,
                                                                                        g_br1);
        SEGNB_LAUNCH_CHECK();
    }
    if (dx != nullptr) {
        const dim3 grid(ceil_div((long long)N * H * W, BS), C / 8);
        if (dtype == SEGNB_BF16)
            gcm1_dx_kernel<bf16_t><<<grid, BS, 0, st>>>(dyl, dyr, N, H, W, C, K, w_l1, w_r1, drop, (bf16_t*)dx, ld_dx);
        else
            gcm1_dx_kernel<float><<<grid, BS, 0, st>>>(dyl, dyr, N, H, W, C, K, w_l1, w_r1, drop, (float*)dx, ld_dx);
        SEGNB_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int segnb_brm_fwd(int N, int H, int W, int K, const float* x, const float* w1, const float* b1, const float* w2,
                             const float* b2, float* r, float* out, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_brm_fwd, N, H, W, K, x, w1, b1, w2, b2, r, out, stream);
    SEGNB_CHECK_ARG(x && w1 && w2 && r && out, "NULL tensor");
    SEGNB_CHECK_ARG(gcn_ok(0, K, N, H, W), "1 <= K <= 32 (segnb_gcn_ok)");
    SEGNB_CHECK_ARG(out != x && r != x && r != out, "outputs must not alias");
    hipStream_t st = (hipStream_t)stream;
    pconv_fwd(x, K, w1, 3, 3, b1, nullptr, 1, r, N, H, W, K, st);
    pconv_fwd(r, K, w2, 3, 3, b2, x, 0, out, N, H, W, K, st);
    SEGNB_LAUNCH_CHECK();
    return 0;
}

extern "C" int segnb_brm_bwd(int N, int H, int W, int K, const float* x, const float* w1, const float* w2, const float* r,
                             const float* dout, float* dr, float* dx, float* g_w1, float* g_b1, float* g_w2, float* g_b2,
                             segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_brm_bwd, N, H, W, K, x, w1, w2, r, dout, dr, dx, g_w1, g_b1, g_w2, g_b2, stream);
    SEGNB_CHECK_ARG(x && w1 && w2 && r && dout && dr && dx, "NULL tensor");
    SEGNB_CHECK_ARG(gcn_ok(0, K, N, H, W), "1 <= K <= 32 (segnb_gcn_ok)");
    SEGNB_CHECK_ARG(dx != dout && dr != dout && dr != dx, "dx / dr must not alias dout");
    hipStream_t st = (hipStream_t)stream;
    float* part = segnb_head_scratch(pconv_wgrad_floats(N, H, W, K, K) * sizeof(float), st);
    if (part == nullptr) return SEGNB_E_BADARG;
    pconv_dgrad(dout, K, w2, 3, 3, r, nullptr, dr, N, H, W, K, st);               // dr = relu'(r) conv2^T(dout)
    if (g_w2 != nullptr || g_b2 != nullptr) pconv_wgrad(dout, K, r, K, 3, 3, N, H, W, part, g_w2, g_b2, st);
    pconv_dgrad(dr, K, w1, 3, 3, nullptr, dout, dx, N, H, W, K, st);               // dx = dout + conv1^T(dr)
    if (g_w1 != nullptr || g_b1 != nullptr) pconv_wgrad(dr, K, x, K, 3, 3, N, H, W, part, g_w1, g_b1, st);
    SEGNB_LAUNCH_CHECK();
    return 0;
}

extern "C" int segnb_resize_bilinear_ac_fwd(int N, int K, int h, int w, const float* in, int H, int W, const float* skip,
                                            float* out, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_resize_bilinear_ac_fwd, N, K, h, w, in, H, W, skip, out, stream);
    SEGNB_CHECK_ARG(in && out && in != out, "NULL or aliased tensor");
    SEGNB_CHECK_ARG(gcn_ok(0, K, N, h, w) && gcn_ok(0, K, N, H, W), "1 <= K <= 32 (segnb_gcn_ok)");
    const long long n = (long long)N * K * H * W;
    resize_ac_fwd_kernel<<<ceil_div(n, BS), BS, 0, (hipStream_t)stream>>>(in, N * K, h, w, H, W, ac_scale_host(h, H),
                                                                          ac_scale_host(w, W), skip, out);
    SEGNB_LAUNCH_CHECK();
    return 0;
}

extern "C" int segnb_resize_bilinear_ac_bwd(int N, int K, int h, int w, int H, int W, const float* dout, float* din,
                                            segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_resize_bilinear_ac_bwd, N, K, h, w, H, W, dout, din, stream);
    SEGNB_CHECK_ARG(dout && din && dout != din, "NULL or aliased tensor");
    SEGNB_CHECK_ARG(gcn_ok(0, K, N, h, w) && gcn_ok(0, K, N, H, W), "1 <= K <= 32 (segnb_gcn_ok)");
    const long long n = (long long)N * K * h * w;
    resize_ac_bwd_kernel<<<ceil_div(n, BS), BS, 0, (hipStream_t)stream>>>(dout, N * K, h, w, H, W, ac_scale_host(h, H),
                                                                          ac_scale_host(w, W), din);
    SEGNB_LAUNCH_CHECK();
    return 0;
}
