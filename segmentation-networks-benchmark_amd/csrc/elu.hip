// ELU passes (include/segnb_elu.h): nn.ELU over an executor tensor -- optionally with the nearest x2 upsample + skip add of
// squeezenet.py:137-149 in the same launch -- and the backward that writes the producing convolution's dz and sums it.
//
// HBM-bound passes in the element-wise geometry of ew.h: one thread column per 8-channel chunk (16-byte accesses in bf16, two in
// fp32), a grid sized from the CU count with a grid-stride loop over the pixels, every load of a trip requested before the
// first use.  Nothing here is shared with the convolution kernels: their epilogues know an activation as ONE multiplier for
// negative values (common.h users: neg = act == RELU ? 0 : ...), which ELU is not.
#include "ew.h"

#include "../../include/segnb_elu.h"

namespace {

constexpr int REPL = SEGNB_STAT_REPLICAS;

__device__ __forceinline__ float elu_f(float v) { return v > 0.f ? v : expm1f(v); }

static bool elu_ok(int dtype, int N, int H, int W, int Cp) {
    if (dtype != SEGNB_F32 && dtype != SEGNB_BF16) return false;
    if (N < 1 || H < 1 || W < 1) return false;
    if (Cp < 8 || Cp > SEGNB_ELU_MAX_C || Cp % 8 != 0) return false;
    return (long long)N * H * W * 16 < (1ll << 31);
}

// blocks: one column per chunk tile, rows from the CU count (8 blocks of 256 threads per CU at most), never more than the trips
static dim3 elu_grid(const EwShape& s, long long npix, int per_trip) {
    const int gy = ceil_div(s.CPP, s.CT);
    long long cap = (long long)segnb_num_cus() * 8 / gy;
    if (cap < 1) cap = 1;
    long long gx = (npix + (long long)s.PY * per_trip - 1) / ((long long)s.PY * per_trip);
    if (gx > cap) gx = cap;
    if (gx < 1) gx = 1;
    return dim3((unsigned)gx, (unsigned)gy);
}

// offset (in pixels) of the top-left pixel of low-resolution pixel pix's 2x2 window in the [N][2H][2W] tensor
__device__ __forceinline__ long long up_origin(int pix, const EwShape& s, const FastDiv& d_hw, const FastDiv& d_w) {
    const int n = d_hw.div(pix);
    const int rem = pix - n * (s.H * s.W);
    const int h = d_w.div(rem);
    const int w = rem - h * s.W;
    return ((long long)n * 2 * s.H + 2 * h) * (2ll * s.W) + 2 * w;
}

template <typename T, bool UP>
__global__ __launch_bounds__(NTHR) void elu_fwd_kernel(const T* z, int ld_z, EwShape s, T* a, int ld_a, const T* up_skip,
                                                       int ld_skip, T* up_out, int ld_up) {
    constexpr int U = UP ? 2 : 4;                     // pixels per trip
    const int tx = threadIdx.x % s.CT, ty = threadIdx.x / s.CT;
    const int cc = blockIdx.y * s.CT + tx;
    if (cc >= s.CPP) return;
    const int c0 = cc * 8;
    const int npix = s.N * s.H * s.W;                 // 32-bit: elu_ok bounds 16 * N * H * W < 2^31
    const int stride = gridDim.x * s.PY;
    const FastDiv d_hw(s.H * s.W), d_w(s.W);
    const long long up_row = 2ll * s.W;
    for (int p0 = blockIdx.x * s.PY + ty; p0 < npix; p0 += U * stride) {
        float v[U][8], sk[UP ? U : 1][UP ? 4 : 1][8];
        long long o00[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int pix = p0 + u * stride;
            if (pix >= npix) break;
            load8(z + (long long)pix * ld_z + c0, v[u]);
            if constexpr (UP) {
                o00[u] = up_origin(pix, s, d_hw, d_w);
                load8(up_skip + o00[u] * ld_skip + c0, sk[u][0]);
                load8(up_skip + (o00[u] + 1) * ld_skip + c0, sk[u][1]);
                load8(up_skip + (o00[u] + up_row) * ld_skip + c0, sk[u][2]);
                load8(up_skip + (o00[u] + up_row + 1) * ld_skip + c0, sk[u][3]);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int pix = p0 + u * stride;
            if (pix >= npix) break;
            float r[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) r[e] = round_as(elu_f(v[u][e]), (const T*)nullptr);
            store8(a + (long long)pix * ld_a + c0, r);
            if constexpr (UP) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float o[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[e] = r[e] + sk[u][q][e];
                    const long long op = o00[u] + (q >> 1) * up_row + (q & 1);
                    store8(up_out + op * ld_up + c0, o);
                }
            }
        }
    }
}

// Per-channel sums of the stored dz: fp64 partials per thread (the table is fp64 and is compared against an fp64 sum), butterfly
// over the lanes of a wave that share a chunk column, one LDS row per wave, the four rows added in wave order, then ONE fp64
// atomic per channel per block into replica blockIdx.x % REPL.
template <typename T, bool HAS_D, bool HAS_A, bool HAS_U>
__global__ __launch_bounds__(NTHR) void elu_bwd_kernel(const T* a, int ld_a, EwShape s, const T* g_direct, int ld_gd,
                                                       const T* g_add, int ld_ga, const T* g_up, int ld_gu, T* dz, int ld_dz,
                                                       double* sums0, int C0p, double* sums1) {
    __shared__ double sred[(NTHR / 64) * 32 * 8];
    constexpr int U = HAS_U ? 1 : 2;
    const int tx = threadIdx.x % s.CT, ty = threadIdx.x / s.CT;
    const int cc = blockIdx.y * s.CT + tx;
    const bool active = cc < s.CPP;
    const int c0 = active ? cc * 8 : 0;
    const int npix = s.N * s.H * s.W;
    const int stride = gridDim.x * s.PY;
    const FastDiv d_hw(s.H * s.W), d_w(s.W);
    const long long up_row = 2ll * s.W;
    const bool do_sums = sums0 != nullptr;
    double acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.0;
    if (active) {
        for (int p0 = blockIdx.x * s.PY + ty; p0 < npix; p0 += U * stride) {
            float av[U][8], gd[HAS_D ? U : 1][8], ga[HAS_A ? U : 1][8], gu[HAS_U ? U : 1][HAS_U ? 4 : 1][8];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int pix = p0 + u * stride;
                if (pix >= npix) break;
                load8(a + (long long)pix * ld_a + c0, av[u]);
                if constexpr (HAS_D) load8(g_direct + (long long)pix * ld_gd + c0, gd[u]);
                if constexpr (HAS_A) load8(g_add + (long long)pix * ld_ga + c0, ga[u]);
                if constexpr (HAS_U) {
                    const long long o00 = up_origin(pix, s, d_hw, d_w);
                    load8(g_up + o00 * ld_gu + c0, gu[u][0]);
                    load8(g_up + (o00 + 1) * ld_gu + c0, gu[u][1]);
                    load8(g_up + (o00 + up_row) * ld_gu + c0, gu[u][2]);
                    load8(g_up + (o00 + up_row + 1) * ld_gu + c0, gu[u][3]);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int pix = p0 + u * stride;
                if (pix >= npix) break;
                float d[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    // g_direct + g_add + (the window's four, in scan order): a missing source is left out
                    float g = 0.f;
                    if constexpr (HAS_D) g = gd[u][e];
                    if constexpr (HAS_A) g = HAS_D ? g + ga[u][e] : ga[u][e];
                    if constexpr (HAS_U) {
                        const float w4 = ((gu[u][0][e] + gu[u][1][e]) + gu[u][2][e]) + gu[u][3][e];
                        g = (HAS_D || HAS_A) ? g + w4 : w4;
                    }
                    const float av1 = av[u][e];
                    d[e] = round_as(g * (av1 > 0.f ? 1.f : av1 + 1.f), (const T*)nullptr);
                    acc[e] += (double)d[e];
                }
                store8(dz + (long long)pix * ld_dz + c0, d);
            }
        }
    }
    if (!do_sums) return;                              // (uniform: a kernel argument)
    for (int off = s.CT; off < 64; off <<= 1) {
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += __shfl_xor(acc[e], off);
    }
    const int nch = s.CT * 8;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < s.CT) {
#pragma unroll
        for (int e = 0; e < 8; ++e) sred[wave * nch + tx * 8 + e] = acc[e];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nch; i += NTHR) {
        const int ch = blockIdx.y * nch + i;
        if (ch >= s.Cp) continue;
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < NTHR / 64; ++w) t += sred[w * nch + i];
        const int rep = blockIdx.x % REPL;
        if (ch < C0p)
            atomicAdd(sums0 + (long long)rep * 2 * C0p + ch, t);
        else
            atomicAdd(sums1 + (long long)rep * 2 * (s.Cp - C0p) + (ch - C0p), t);
    }
}

static bool ld_ok(const void* p, int ld, int Cp) { return p == nullptr || (ld % 8 == 0 && ld >= Cp); }

}  // namespace

extern "C" int segnb_elu_ok(int dtype, int N, int H, int W, int Cp) { return elu_ok(dtype, N, H, W, Cp) ? 1 : 0; }

extern "C" int segnb_elu_fwd(int dtype, const void* z, int ld_z, int N, int H, int W, int Cp, void* a, int ld_a,
                             const void* up_skip, int ld_skip, void* up_out, int ld_up, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_elu_fwd, dtype, z, ld_z, N, H, W, Cp, a, ld_a, up_skip, ld_skip, up_out, ld_up, stream);
    SEGNB_CHECK_ARG(elu_ok(dtype, N, H, W, Cp), "dtype / shape out of range (segnb_elu_ok)");
    SEGNB_CHECK_ARG(z != nullptr && a != nullptr, "NULL tensor");
    SEGNB_CHECK_ARG(ld_ok(z, ld_z, Cp) && ld_ok(a, ld_a, Cp), "pixel stride");
    SEGNB_CHECK_ARG((up_out == nullptr) == (up_skip == nullptr), "up_skip and up_out go together");
    SEGNB_CHECK_ARG(ld_ok(up_skip, ld_skip, Cp) && ld_ok(up_out, ld_up, Cp), "upsampled pixel stride");
    SEGNB_CHECK_ARG(up_out == nullptr || (up_out != a && up_out != z), "up_out must not alias a");
    const EwShape s = make_shape(N, H, W, Cp);
    const long long npix = (long long)N * H * W;
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = segnb_dispatch_dtype(dtype, "segnb_elu_fwd", [&](auto tag) SEGNB_INLINE_LAMBDA {
            using T = SEGNB_TAG_T(tag);
            segnb_dispatch_bool(up_out != nullptr, [&](auto UP) SEGNB_INLINE_LAMBDA {
                const dim3 grid = elu_grid(s, npix, decltype(UP)::value ? 2 : 4);
                hipLaunchKernelGGL((elu_fwd_kernel<T, decltype(UP)::value>), grid, dim3(NTHR), 0, st, (const T*)z, ld_z, s, (T*)a,
                                   ld_a, (const T*)up_skip, ld_skip, (T*)up_out, ld_up);
            });
        }))
        return rc;
    SEGNB_LAUNCH_CHECK();
    return 0;
}

extern "C" int segnb_elu_bwd(int dtype, const void* a, int ld_a, int N, int H, int W, int Cp, const void* g_direct, int ld_gd,
                             const void* g_add, int ld_ga, const void* g_up, int ld_gu, void* dz, int ld_dz, double* sums0,
                             int C0p, double* sums1, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_elu_bwd, dtype, a, ld_a, N, H, W, Cp, g_direct, ld_gd, g_add, ld_ga, g_up, ld_gu, dz, ld_dz, sums0, C0p,
                      sums1, stream);
    SEGNB_CHECK_ARG(elu_ok(dtype, N, H, W, Cp), "dtype / shape out of range (segnb_elu_ok)");
    SEGNB_CHECK_ARG(a != nullptr && dz != nullptr, "NULL tensor");
    SEGNB_CHECK_ARG(g_direct || g_add || g_up, "no gradient source");
    SEGNB_CHECK_ARG(ld_ok(a, ld_a, Cp) && ld_ok(dz, ld_dz, Cp) && ld_ok(g_direct, ld_gd, Cp) && ld_ok(g_add, ld_ga, Cp)
                    && ld_ok(g_up, ld_gu, Cp), "pixel stride");
    SEGNB_CHECK_ARG(dz != a && dz != g_add && dz != g_up, "dz may alias g_direct only");
    if (sums0 != nullptr) {
        SEGNB_CHECK_ARG(C0p >= 8 && C0p % 8 == 0 && C0p <= Cp && (sums1 != nullptr) == (C0p < Cp),
                        "sums: C0p a multiple of 8 in [8, Cp]; sums1 exactly when C0p < Cp");
    } else {
        SEGNB_CHECK_ARG(sums1 == nullptr, "sums1 without sums0");
    }
    const EwShape s = make_shape(N, H, W, Cp);
    const long long npix = (long long)N * H * W;
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = segnb_dispatch_dtype(dtype, "segnb_elu_bwd", [&](auto tag) SEGNB_INLINE_LAMBDA {
            using T = SEGNB_TAG_T(tag);
            segnb_dispatch_bool(g_direct != nullptr, [&](auto D) SEGNB_INLINE_LAMBDA {
                segnb_dispatch_bool(g_add != nullptr, [&](auto A) SEGNB_INLINE_LAMBDA {
                    segnb_dispatch_bool(g_up != nullptr, [&](auto U) SEGNB_INLINE_LAMBDA {
                        if constexpr (decltype(D)::value || decltype(A)::value || decltype(U)::value) {
                            const dim3 grid = elu_grid(s, npix, decltype(U)::value ? 1 : 2);
                            SEGNB_LAUNCH_FORKABLE((elu_bwd_kernel<T, decltype(D)::value, decltype(A)::value, decltype(U)::value>),
                                                  grid, dim3(NTHR), 0, st, (const T*)a, ld_a, s, (const T*)g_direct, ld_gd,
                                                  (const T*)g_add, ld_ga, (const T*)g_up, ld_gu, (T*)dz, ld_dz, sums0, C0p, sums1);
                        }
                    });
                });
            });
        }))
        return rc;
    SEGNB_LAUNCH_CHECK();
    return 0;
}
