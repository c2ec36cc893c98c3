// Weight pack, weight-gradient unpack and the fused SGD + pack for the gather-convolution kernels (conv_igemm.hip and the
// fprop_* / wgrad_* files): the packed matrices [rows][taps x columns] of segnb.engine.ConvOp, one parameter per launch or a job
// table per launch, and the NCHW fp32 -> NHWC input pack.
#include "common.h"

namespace {

// ================================================================================================
// weight pack / gradient unpack
// ================================================================================================
struct PackArgs {
    int Mp, Cp, ntaps;
    long long s_m, s_c;
    const int* mmap;
    const int* cmap;
    int tap_off[SEGNB_MAX_TAPS];
};

template <typename T>
__global__ void pack_weight_kernel(const float* __restrict__ w, T* __restrict__ wp, const PackArgs p) {
    const long long total = (long long)p.Mp * p.ntaps * p.Cp;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int cp = (int)(i % p.Cp);
        const long long q = i / p.Cp;
        const int t = (int)(q % p.ntaps);
        const int mp = (int)(q / p.ntaps);
        const int m = p.mmap[mp], c = p.cmap[cp];
        float v = 0.f;
        if (m >= 0 && c >= 0) v = w[m * p.s_m + c * p.s_c + p.tap_off[t]];
        wp[i] = Elem<T>::from_f32(v);
    }
}

__global__ void unpack_wgrad_kernel(float* __restrict__ dwp, float* __restrict__ gw, const PackArgs p,
                                    int accumulate) {
    const long long total = (long long)p.Mp * p.ntaps * p.Cp;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int cp = (int)(i % p.Cp);
        const long long q = i / p.Cp;
        const int t = (int)(q % p.ntaps);
        const int mp = (int)(q / p.ntaps);
        const int m = p.mmap[mp], c = p.cmap[cp];
        if (m >= 0 && c >= 0) {
            float* dst = gw + m * p.s_m + c * p.s_c + p.tap_off[t];
            *dst = accumulate ? (*dst + dwp[i]) : dwp[i];
        }
        dwp[i] = 0.f;   // workspace is consumed: ready for the next step's atomics without a memset
    }
}

// ---- batched forms: ONE launch packs every weight matrix of a model (or unpacks every gradient) --------
// job table in device memory (built once by the host, pointers are stable); block -> job by binary search
struct __attribute__((aligned(8))) PackJob {
    const float* w;          // pack: fp32 parameter (source);  unpack: fp32 gradient (destination)
    void* packed;            // pack: destination (dtype);      unpack: fp32 workspace (source, re-zeroed)
    const int* mmap;
    const int* cmap;
    long long s_m, s_c;
    int Mp, Cp, ntaps, dtype;
    int block_start;         // first block of this job; jobs sorted by it
    int nslab;               // unpack jobs: partial slabs to sum ([nslab][Mp][ntaps][Cp]); 0/1 = one
    // masked != 0: tap_off[t] is a BIT MASK over the (<= 9) kernel positions of the parameter tensor instead of one offset --
    //   pack  : packed(m, t, c) = sum over the set positions k of w(m, c, k)      (rounded once, after the fp32 sum)
    //   unpack: gw(m, c, k)    += sum over the taps t whose mask holds k of dwp(m, t, c)          (taps in order)
    // = the convolution of a nearest-x2 upsampled tensor as the 4x4 / stride-2 transposed convolution it is, on the
    // reference's own 3x3 parameter (lib/models/zf_unet.py:42,78-90: Upsample(scale_factor=2) -> cat -> conv3x3)
    int masked;
    int pad_;
    int tap_off[SEGNB_MAX_TAPS];
};

// the job that owns block b (block_start ascending, job 0 starts at 0): every wave counts the starts <= b, 64 jobs per round trip
// (a binary search was log2(njobs) DEPENDENT loads -- 6 for ZF_UNET's 46 jobs, most of a small tile's life)
template <typename Job>
__device__ __forceinline__ int find_job(const Job* jobs, int njobs, int b) {
    const int lane = threadIdx.x & 63;
    int cnt = 0;
    for (int k = 0; k < njobs; k += 64) {
        const bool le = k + lane < njobs && jobs[k + lane].block_start <= b;
        cnt += __popcll(__ballot(le));
    }
    return __builtin_amdgcn_readfirstlane(cnt - 1);
}

// Tiled through LDS so that BOTH sides are coalesced.  The parameter tensor has the tap index fastest
// (stride 1) and one of the two channel indices at stride T_src = min(s_m, s_c) ("fast" channel), the other at
// a large stride ("slow" channel).  A tile = SLOW x FAST channels x all taps:
//   parameter side : for each slow index a run of FAST*T_src contiguous floats
//   packed side    : [mp][t][cp], contiguous along cp
// fwd pack  (rows = co slow, cols = ci fast): tile 1 x 256   -> packed runs of 256 elements
// dgrad pack (rows = ci fast, cols = co slow): tile 8 x 64   -> packed runs of 64 elements
struct TileGeom {
    int fast_is_c;      // 1: cp indexes the fast channel (fwd layout), 0: mp does (dgrad layout)
    int F, S;           // tile extents along fast / slow packed index
    int nF, nS;         // tiles along each
    int Tsrc;           // taps in the parameter tensor (KH*KW)
};

__device__ __forceinline__ TileGeom tile_geom(const PackJob& j) {
    TileGeom g;
    g.fast_is_c = j.s_c < j.s_m;
    g.Tsrc = (int)(g.fast_is_c ? j.s_c : j.s_m);
    if (g.fast_is_c) {
        g.F = 256; g.S = 1;
        g.nF = (j.Cp + g.F - 1) / g.F; g.nS = j.Mp;
    } else {
        g.F = 8; g.S = 64;
        g.nF = (j.Mp + g.F - 1) / g.F; g.nS = (j.Cp + g.S - 1) / g.S;
    }
    return g;
}

constexpr int PACK_LDS_FLOATS = 256 * 9 > 64 * 8 * 9 ? 256 * 9 : 64 * 8 * 9;   // 4608

// is_pack: parameter -> packed (round to dtype); else packed fp32 workspace -> += gradient, workspace zeroed.
// The channel maps of the tile are staged in LDS once (a map lookup per element made every parameter access the
// tail of a dependent-load chain) and the packed side moves 16 bytes per lane (8 bf16 / 4 fp32 along the
// contiguous channel index; channel counts are padded to multiples of 8).
template <bool IS_PACK>
__device__ __forceinline__ void pack_tile(const PackJob* __restrict__ jobs, int njobs, int bid, float* tile, long long* sFast,
                                          long long* sSlow, int& sCnt) {
    const PackJob& j = jobs[find_job(jobs, njobs, bid)];
    const TileGeom g = tile_geom(j);
    const int tb = bid - j.block_start;
    const int tf = tb % g.nF, ts = tb / g.nF;
    const int f0 = tf * g.F, s0 = ts * g.S;
    const int run = g.F * g.Tsrc;                    // contiguous floats per slow index on the parameter side
    const int Mp = j.Mp, Cp = j.Cp, nt = j.ntaps;
    float* param = const_cast<float*>(j.w);
    const int n_param = g.S * run;
    {
        const int* fmap = g.fast_is_c ? j.cmap : j.mmap;
        const int* smap = g.fast_is_c ? j.mmap : j.cmap;
        const int nfast = g.fast_is_c ? Cp : Mp, nslow = g.fast_is_c ? Mp : Cp;
        const long long fstride = g.fast_is_c ? j.s_c : j.s_m, sstride = g.fast_is_c ? j.s_m : j.s_c;
        for (int i = threadIdx.x; i < g.F; i += 256) {
            const int v = f0 + i < nfast ? fmap[f0 + i] : -1;
            sFast[i] = v >= 0 ? v * fstride : -1;
        }
        for (int i = threadIdx.x; i < g.S; i += 256) {
            const int v = s0 + i < nslow ? smap[s0 + i] : -1;
            sSlow[i] = v >= 0 ? v * sstride : -1;
        }
    }
    __syncthreads();
    // Parameter side in 16-byte accesses when the tile's fast channels are a contiguous run of the tensor (consecutive real
    // channels: everything but a tile that crosses a padding gap) and every row starts 16-byte aligned: dword accesses moved
    // the 0.38 GB of a ZF_UNET pack at 2.5 TB/s
    int nvalid = 0;
    bool vec;
    {
        const int nfast = g.fast_is_c ? Cp : Mp;
        const int lim = min(g.F, nfast - f0);
        bool ok = true;
        for (int i = threadIdx.x; i < g.F; i += 256) {
            const long long v = sFast[i];
            if (i < lim && v >= 0) ok = ok && v == sFast[0] + (long long)i * g.Tsrc;
            if (v >= 0 && i > 0 && sFast[i - 1] < 0) ok = false;               // a gap inside the run
        }
        for (int i = threadIdx.x; i < g.S; i += 256) {
            const long long v = sSlow[i];
            if (v >= 0) ok = ok && ((v + (sFast[0] < 0 ? 0 : sFast[0])) & 3) == 0;
        }
        // count of valid fast channels (they form a prefix when ok)
        int cnt = 0;
        for (int i = threadIdx.x; i < g.F; i += 256) cnt += sFast[i] >= 0 ? 1 : 0;
        if (threadIdx.x == 0) sCnt = 0;
        __syncthreads();
        if (cnt) atomicAdd(&sCnt, cnt);
        vec = __syncthreads_and(ok ? 1 : 0) != 0;
        nvalid = sCnt;
        vec = vec && sFast[0] >= 0 && ((nvalid * g.Tsrc) & 3) == 0 && ((const uintptr_t)param & 15) == 0;
    }
    const int row4 = nvalid * g.Tsrc / 4;               // float4 per slow row on the vector path
    auto param_off = [&](int sl, int fa) -> long long {      // element offset of (slow, fast, tap 0) or -1
        const long long a = sSlow[sl], b = sFast[fa];
        return (a < 0 || b < 0) ? -1 : a + b;
    };
    // packed side: [mp][t][cp]; groups of 8 consecutive cp (one 16-byte bf16 vector / two fp32 vectors)
    const int ncp = g.fast_is_c ? g.F : g.S;             // cp extent of the tile (multiple of 8)
    const int nmp = g.fast_is_c ? g.S : g.F;
    const int groups = nmp * nt * (ncp / 8);
    auto group = [&](int gi, int& mpl, int& t, int& cpl) {       // tile-local (mp, tap, first cp) of group gi
        cpl = (gi % (ncp / 8)) * 8;
        t = (gi / (ncp / 8)) % nt;
        mpl = gi / ((ncp / 8) * nt);
    };
    auto tile_idx = [&](int mpl, int t, int cpl) {               // LDS index of packed element (mp, t, cp)
        const int sl = g.fast_is_c ? mpl : cpl, fa = g.fast_is_c ? cpl : mpl;
        return sl * run + fa * g.Tsrc + j.tap_off[t];
    };
    const int cp_step = g.fast_is_c ? g.Tsrc : run;              // LDS stride between consecutive cp
    auto tile_base = [&](int mpl, int cpl) {                     // LDS index of kernel position 0 of packed (mp, cp)
        const int sl = g.fast_is_c ? mpl : cpl, fa = g.fast_is_c ? cpl : mpl;
        return sl * run + fa * g.Tsrc;
    };

    if (IS_PACK) {
        // parameter -> LDS, in parameter order (coalesced along the fast channel and the taps).  All of a lane's loads
        // are issued before the first LDS store (a rolled loop kept ONE 4-byte load per lane in flight: 2.5 TB/s)
        constexpr int MAXU = PACK_LDS_FLOATS / 256;
        if (vec) {
            constexpr int MAXU4 = (PACK_LDS_FLOATS / 4 + 255) / 256;
            if (nvalid < g.F)                                    // padding channels of the tile read as zero
                for (int i = threadIdx.x; i < n_param; i += 256) tile[i] = 0.f;
            if (nvalid < g.F) __syncthreads();
            float4 pv4[MAXU4];
            const int n4 = g.S * row4;
#pragma unroll
            for (int u = 0; u < MAXU4; ++u) {
                const int i = threadIdx.x + u * 256;
                pv4[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (i < n4) {
                    const int sl = i / row4, r = i - sl * row4;
                    if (sSlow[sl] >= 0) pv4[u] = *reinterpret_cast<const float4*>(param + sSlow[sl] + sFast[0] + 4 * r);
                }
            }
#pragma unroll
            for (int u = 0; u < MAXU4; ++u) {
                const int i = threadIdx.x + u * 256;
                if (i < n4) {
                    const int sl = i / row4, r = i - sl * row4;
                    *reinterpret_cast<float4*>(tile + sl * run + 4 * r) = pv4[u];
                }
            }
        } else {
        float pv[MAXU];
#pragma unroll
        for (int u = 0; u < MAXU; ++u) {
            const int i = threadIdx.x + u * 256;
            pv[u] = 0.f;
            if (i < n_param) {
                const int sl = i / run, r = i - sl * run;
                const int fa = r / g.Tsrc, tp = r - fa * g.Tsrc;
                const long long off = param_off(sl, fa);
                if (off >= 0) pv[u] = param[off + tp];
            }
        }
#pragma unroll
        for (int u = 0; u < MAXU; ++u) {
            const int i = threadIdx.x + u * 256;
            if (i < n_param) tile[i] = pv[u];
        }
        }
        __syncthreads();
        // LDS -> packed, 8 consecutive cp per lane
        for (int gi = threadIdx.x; gi < groups; gi += 256) {
            int mpl, t, cpl;
            group(gi, mpl, t, cpl);
            const int mp = (g.fast_is_c ? s0 : f0) + mpl, cp = (g.fast_is_c ? f0 : s0) + cpl;
            if (mp < Mp && cp < Cp) {
                float v[8];
                if (j.masked) {
                    const int base0 = tile_base(mpl, cpl);
                    const unsigned mask = (unsigned)j.tap_off[t];
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] = 0.f;
                    for (int pos = 0; pos < g.Tsrc; ++pos)
                        if (mask >> pos & 1u) {
#pragma unroll
                            for (int k = 0; k < 8; ++k) v[k] += tile[base0 + pos + k * cp_step];
                        }
                } else {
                    const int base = tile_idx(mpl, t, cpl);
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] = tile[base + k * cp_step];
                }
                const long long di = ((long long)mp * nt + t) * Cp + cp;
                if (j.dtype == SEGNB_BF16)
                    store8(reinterpret_cast<bf16_t*>(j.packed) + di, v);
                else
                    store8(reinterpret_cast<float*>(j.packed) + di, v);
            }
        }
    } else {
        float* dwp = reinterpret_cast<float*>(j.packed);
        for (int i = threadIdx.x; i < n_param; i += 256) tile[i] = 0.f;
        __syncthreads();
        if (j.masked) {
            // one thread owns every tap of its (mp, 8 x cp) group: the taps that share a kernel position are summed in
            // registers, in tap order (no collisions in the tile, bitwise reproducible)
            const int pairs = nmp * (ncp / 8);
            const long long sstride = (long long)Mp * nt * Cp;
            for (int gi = threadIdx.x; gi < pairs; gi += 256) {
                const int cpl = (gi % (ncp / 8)) * 8, mpl = gi / (ncp / 8);
                const int mp = (g.fast_is_c ? s0 : f0) + mpl, cp = (g.fast_is_c ? f0 : s0) + cpl;
                if (mp >= Mp || cp >= Cp) continue;
                float acc[9][8];
#pragma unroll
                for (int pos = 0; pos < 9; ++pos)
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc[pos][k] = 0.f;
                for (int t = 0; t < nt; ++t) {
                    const long long di = ((long long)mp * nt + t) * Cp + cp;
                    float v[8];
                    load8(dwp + di, v);
                    for (int sl = 1; sl < j.nslab; ++sl) {
                        float u[8];
                        load8(dwp + sl * sstride + di, u);
#pragma unroll
                        for (int k = 0; k < 8; ++k) v[k] += u[k];
                    }
                    const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    store8(dwp + di, z);
                    const unsigned mask = (unsigned)j.tap_off[t];
#pragma unroll
                    for (int pos = 0; pos < 9; ++pos)
                        if (mask >> pos & 1u) {
#pragma unroll
                            for (int k = 0; k < 8; ++k) acc[pos][k] += v[k];
                        }
                }
                const int base0 = tile_base(mpl, cpl);
#pragma unroll
                for (int pos = 0; pos < 9; ++pos)
                    if (pos < g.Tsrc) {
#pragma unroll
                        for (int k = 0; k < 8; ++k) tile[base0 + pos + k * cp_step] = acc[pos][k];
                    }
            }
        } else
        for (int gi = threadIdx.x; gi < groups; gi += 256) {
            int mpl, t, cpl;
            group(gi, mpl, t, cpl);
            const int mp = (g.fast_is_c ? s0 : f0) + mpl, cp = (g.fast_is_c ? f0 : s0) + cpl;
            if (mp < Mp && cp < Cp) {
                const long long di = ((long long)mp * nt + t) * Cp + cp;
                float v[8];
                load8(dwp + di, v);
                // partial slabs of pixel splits (a job's nslab > 1): summed here, in slab order, instead of by
                // a reduction launch per layer that wrote the sum back for this kernel to read again
                const long long sstride = (long long)Mp * nt * Cp;
                for (int sl = 1; sl < j.nslab; ++sl) {
                    float u[8];
                    load8(dwp + sl * sstride + di, u);
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] += u[k];
                }
                const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                store8(dwp + di, z);                                  // workspace consumed
                const int base = tile_idx(mpl, t, cpl);
#pragma unroll
                for (int k = 0; k < 8; ++k) tile[base + k * cp_step] = v[k];      // taps are distinct: no collisions
            }
        }
        __syncthreads();
        constexpr int MAXU = PACK_LDS_FLOATS / 256;
        if (vec) {
            constexpr int MAXU4 = (PACK_LDS_FLOATS / 4 + 255) / 256;
            float4 pv4[MAXU4];
            const int n4 = g.S * row4;
#pragma unroll
            for (int u = 0; u < MAXU4; ++u) {
                const int i = threadIdx.x + u * 256;
                if (i < n4) {
                    const int sl = i / row4, r = i - sl * row4;
                    if (sSlow[sl] >= 0) pv4[u] = *reinterpret_cast<const float4*>(param + sSlow[sl] + sFast[0] + 4 * r);
                }
            }
#pragma unroll
            for (int u = 0; u < MAXU4; ++u) {
                const int i = threadIdx.x + u * 256;
                if (i < n4) {
                    const int sl = i / row4, r = i - sl * row4;
                    if (sSlow[sl] >= 0) {
                        const float4 t4 = *reinterpret_cast<const float4*>(tile + sl * run + 4 * r);
                        float4 o = pv4[u];
                        o.x += t4.x; o.y += t4.y; o.z += t4.z; o.w += t4.w;
                        *reinterpret_cast<float4*>(param + sSlow[sl] + sFast[0] + 4 * r) = o;
                    }
                }
            }
            return;
        }
        float pv[MAXU];
        long long po[MAXU];
#pragma unroll
        for (int u = 0; u < MAXU; ++u) {                       // all gradient loads of the lane first (see the pack side)
            const int i = threadIdx.x + u * 256;
            po[u] = -1;
            if (i < n_param) {
                const int sl = i / run, r = i - sl * run;
                const int fa = r / g.Tsrc, tp = r - fa * g.Tsrc;
                const long long off = param_off(sl, fa);
                if (off >= 0) {
                    po[u] = off + tp;
                    pv[u] = param[off + tp];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < MAXU; ++u)
            if (po[u] >= 0) param[po[u]] = pv[u] + tile[threadIdx.x + u * 256];
    }
}

// One block per tile, or (grid < total: segnb_tune "pack_blocks" / SEGNB_PACK_BLOCKS) persistent blocks that walk the tiles: a
// pack launched BESIDE the forward's first levels on few CUs takes its time without taking their HBM bandwidth
template <bool IS_PACK>
__global__ __launch_bounds__(256) void pack_tiled_kernel(const PackJob* __restrict__ jobs, int njobs, int total) {
    __shared__ __attribute__((aligned(16))) float tile[PACK_LDS_FLOATS];
    __shared__ long long sFast[256], sSlow[64];         // element offset of each fast / slow channel of the tile, -1 = pad
    __shared__ int sCnt;
    for (int b = blockIdx.x; b < total; b += gridDim.x) {
        pack_tile<IS_PACK>(jobs, njobs, b, tile, sFast, sSlow, sCnt);
        if (b + (int)gridDim.x < total) __syncthreads();
    }
}

// BOTH matrices of a plain 3 x 3 convolution from ONE read of its parameter (bf16): the forward matrix [Cop][9][Cip] and the
// data-gradient matrix [Cip][9][Cop] (kernel positions in each form's own tap order).  At every step's start the two tiled
// packs above read each fp32 parameter twice and their 9-KB tiles are a chain of dependent round trips (ZF_UNET: 88 us for
// 252 MB read + 123 MB written, tools/pack_bench.py); here a block owns 32 output x 64 input channels (72 KB of the
// parameter, 18 float4 loads per lane issued together), rounds once into an LDS tile and writes both forms from it in
// 128-byte / 64-byte runs.  Channels are in place (no maps: real channel c = packed channel c, padding behind them).
struct PackPairJob {
    const float* w;        // [Co][Ci][3][3]
    void* pf;              // bf16 [Cop][9][Cip]
    void* pd;              // bf16 [Cip][9][Cop], or NULL: forward matrix only
    int Ci, Co, Cip, Cop;
    int block_start, pad_;
    int tapf[9], tapd[9];  // kernel position kh * 3 + kw of packed tap t of either form
};
constexpr int PP_CO = 32, PP_CI = 64;
constexpr int PP_RS = PP_CI * 9 + 4;          // LDS row in bf16 elements (rows 8-byte aligned; 8 rows apart = 16 banks apart)
constexpr int PP_LOADS = PP_CO * PP_CI * 9 / 4 / 256;

// SGD (segnb_sgd_pack_pair_multi): the optimizer's update w -= lr * g is applied to the tile on its way through the registers --
// sgd_kernel's expression, so the parameters are bit-identical to segnb_sgd_step's -- and written back; the packed matrices are
// then those of the UPDATED parameters: the next forward's weight pack (a second read of every parameter) is already done.
// g_delta: the gradient of element e of the flat parameter buffer sits g_delta floats behind it (flat_g - flat_p).
template <bool SGD>
__global__ __launch_bounds__(256) void pack_pair_kernel(const PackPairJob* __restrict__ jobs, int njobs, long long g_delta, float lr) {
    __shared__ __attribute__((aligned(16))) unsigned short tile[PP_CO * PP_RS];
    const PackPairJob& j = jobs[find_job(jobs, njobs, (int)blockIdx.x)];
    const int tb = blockIdx.x - j.block_start;
    const int nci = (j.Cip + PP_CI - 1) / PP_CI;
    const int ci0 = (tb % nci) * PP_CI, co0 = (tb / nci) * PP_CO;
    const int Ci = j.Ci, Co = j.Co, Cip = j.Cip, Cop = j.Cop;
    const int nv = min(PP_CI, Ci - ci0);                    // real input channels of the tile (a multiple of 4, maybe <= 0)
    const int run4 = nv > 0 ? nv * 9 / 4 : 0;               // float4 per parameter row
    constexpr int ROW4 = PP_CI * 9 / 4;
    float4 v[PP_LOADS];
    if ((Ci & 3) == 0) {
#pragma unroll
        for (int u = 0; u < PP_LOADS; ++u) {
            const int i = threadIdx.x + 256 * u;
            const int co_l = i / ROW4, r = i - co_l * ROW4;
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < run4 && co0 + co_l < Co)
                v[u] = *reinterpret_cast<const float4*>(j.w + ((long long)(co0 + co_l) * Ci + ci0) * 9 + 4 * r);
        }
        if constexpr (SGD) {
            float4 gv[PP_LOADS];
#pragma unroll
            for (int u = 0; u < PP_LOADS; ++u) {
                const int i = threadIdx.x + 256 * u;
                const int co_l = i / ROW4, r = i - co_l * ROW4;
                gv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (r < run4 && co0 + co_l < Co)
                    gv[u] = *reinterpret_cast<const float4*>(j.w + g_delta + ((long long)(co0 + co_l) * Ci + ci0) * 9 + 4 * r);
            }
#pragma unroll
            for (int u = 0; u < PP_LOADS; ++u) {
                const int i = threadIdx.x + 256 * u;
                const int co_l = i / ROW4, r = i - co_l * ROW4;
                float4 pv = v[u];
                pv.x -= lr * gv[u].x; pv.y -= lr * gv[u].y; pv.z -= lr * gv[u].z; pv.w -= lr * gv[u].w;
                v[u] = pv;
                if (r < run4 && co0 + co_l < Co)
                    *reinterpret_cast<float4*>(const_cast<float*>(j.w) + ((long long)(co0 + co_l) * Ci + ci0) * 9 + 4 * r) = pv;
            }
        }
    } else {
        // rows that are not 16-byte aligned (the first layer: 3 input channels): element loads, same tile image
        const int runf = nv > 0 ? nv * 9 : 0;
#pragma unroll
        for (int u = 0; u < PP_LOADS; ++u) {
            const int i = threadIdx.x + 256 * u;
            const int co_l = i / ROW4, r = i - co_l * ROW4;
            const float* row = j.w + ((long long)(co0 + co_l) * Ci + ci0) * 9 + 4 * r;
            const bool in = co0 + co_l < Co;
            v[u].x = (in && 4 * r < runf) ? row[0] : 0.f;
            v[u].y = (in && 4 * r + 1 < runf) ? row[1] : 0.f;
            v[u].z = (in && 4 * r + 2 < runf) ? row[2] : 0.f;
            v[u].w = (in && 4 * r + 3 < runf) ? row[3] : 0.f;
            if constexpr (SGD) {
                float* wrow = const_cast<float*>(row);
                const float* grow = row + g_delta;
                if (in && 4 * r < runf) { v[u].x -= lr * grow[0]; wrow[0] = v[u].x; }
                if (in && 4 * r + 1 < runf) { v[u].y -= lr * grow[1]; wrow[1] = v[u].y; }
                if (in && 4 * r + 2 < runf) { v[u].z -= lr * grow[2]; wrow[2] = v[u].z; }
                if (in && 4 * r + 3 < runf) { v[u].w -= lr * grow[3]; wrow[3] = v[u].w; }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < PP_LOADS; ++u) {
        const int i = threadIdx.x + 256 * u;
        const int co_l = i / ROW4, r = i - co_l * ROW4;
        uint2 pk;
        pk.x = pack2bf(v[u].x, v[u].y);
        pk.y = pack2bf(v[u].z, v[u].w);
        *reinterpret_cast<uint2*>(tile + co_l * PP_RS + 4 * r) = pk;
    }
    __syncthreads();
    unsigned short* const pf = reinterpret_cast<unsigned short*>(j.pf);
    unsigned short* const pd = reinterpret_cast<unsigned short*>(j.pd);
    // forward form: (co, t) rows of 64 input channels, 8 per lane
    for (int gi = threadIdx.x; gi < PP_CO * 9 * (PP_CI / 8); gi += 256) {
        const int c8 = gi % (PP_CI / 8), t = (gi / (PP_CI / 8)) % 9, co_l = gi / (9 * (PP_CI / 8));
        const int co = co0 + co_l, ci = ci0 + c8 * 8;
        if (co >= Cop || ci >= Cip) continue;
        const unsigned short* src = tile + co_l * PP_RS + c8 * 72 + j.tapf[t];
        uint4 o;
        o.x = (unsigned)src[0] | ((unsigned)src[9] << 16);
        o.y = (unsigned)src[18] | ((unsigned)src[27] << 16);
        o.z = (unsigned)src[36] | ((unsigned)src[45] << 16);
        o.w = (unsigned)src[54] | ((unsigned)src[63] << 16);
        *reinterpret_cast<uint4*>(pf + ((long long)co * 9 + t) * Cip + ci) = o;
    }
    // data-gradient form: (ci, t) rows of 32 output channels, 8 per lane (pd == NULL: a layer without a data gradient)
    if (pd == nullptr) return;
    for (int gi = threadIdx.x; gi < PP_CI * 9 * (PP_CO / 8); gi += 256) {
        const int o8 = gi % (PP_CO / 8), t = (gi / (PP_CO / 8)) % 9, ci_l = gi / (9 * (PP_CO / 8));
        const int ci = ci0 + ci_l, co = co0 + o8 * 8;
        if (ci >= Cip || co >= Cop) continue;
        const unsigned short* src = tile + (o8 * 8) * PP_RS + ci_l * 9 + j.tapd[t];
        uint4 o;
        o.x = (unsigned)src[0] | ((unsigned)src[PP_RS] << 16);
        o.y = (unsigned)src[2 * PP_RS] | ((unsigned)src[3 * PP_RS] << 16);
        o.z = (unsigned)src[4 * PP_RS] | ((unsigned)src[5 * PP_RS] << 16);
        o.w = (unsigned)src[6 * PP_RS] | ((unsigned)src[7 * PP_RS] << 16);
        *reinterpret_cast<uint4*>(pd + ((long long)ci * 9 + t) * Cop + co) = o;
    }
}

// Element-wise batched forms for the jobs the tiled kernel does not take (parameter tensors with more than 3 x 3 positions: the
// 7 x 7 stem, the 4 x 4 transposed convolutions): the same job table, PACKW_ITEMS packed elements per thread, block -> job by
// binary search.  One launch instead of one ctypes call + launch per job (LinkNet34: 21 of them at every step's start).
constexpr int PACKW_ITEMS = 4;
template <bool IS_PACK>
__global__ __launch_bounds__(256) void pack_elem_multi_kernel(const PackJob* __restrict__ jobs, int njobs) {
    const PackJob& j = jobs[find_job(jobs, njobs, blockIdx.x)];
    const long long total = (long long)j.Mp * j.ntaps * j.Cp;
    const long long base = (long long)(blockIdx.x - j.block_start) * (256 * PACKW_ITEMS);
    float* param = const_cast<float*>(j.w);
#pragma unroll
    for (int u = 0; u < PACKW_ITEMS; ++u) {
        const long long i = base + u * 256 + threadIdx.x;
        if (i >= total) continue;
        const int cp = (int)(i % j.Cp);
        const long long q = i / j.Cp;
        const int t = (int)(q % j.ntaps);
        const int mp = (int)(q / j.ntaps);
        const int m = j.mmap[mp], c = j.cmap[cp];
        if (IS_PACK) {
            float v = 0.f;
            if (m >= 0 && c >= 0) v = param[m * j.s_m + c * j.s_c + j.tap_off[t]];
            if (j.dtype == SEGNB_BF16) reinterpret_cast<bf16_t*>(j.packed)[i] = Elem<bf16_t>::from_f32(v);
            else reinterpret_cast<float*>(j.packed)[i] = v;
        } else {
            float* dwp = reinterpret_cast<float*>(j.packed);
            if (m >= 0 && c >= 0) param[m * j.s_m + c * j.s_c + j.tap_off[t]] += dwp[i];
            dwp[i] = 0.f;   // workspace is consumed: ready for the next step's atomics without a memset
        }
    }
}

template <typename T>
__global__ void pack_input_kernel(const float* __restrict__ x, T* __restrict__ out, int N, int C, int H, int W,
                                  int Cp, int ld) {
    // one thread per (pixel, 8-channel chunk); reads are W-contiguous per channel plane
    const long long npix = (long long)N * H * W;
    const int CPP = Cp / 8;
    const long long total = npix * CPP;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const long long pix = i / CPP;
        const int cc = (int)(i - pix * CPP);
        const long long n = pix / ((long long)H * W);
        const long long hw = pix - n * (long long)H * W;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int ch = cc * 8 + e;
            v[e] = ch < C ? x[(n * C + ch) * (long long)H * W + hw] : 0.f;
        }
        store8(out + pix * ld + cc * 8, v);
    }
}

}  // namespace

static int fill_pack_args(PackArgs& p, int Mp, int Cp, int ntaps, long long s_m, long long s_c,
                          const int* tap_off_host, const int* mmap, const int* cmap) {
    SEGNB_CHECK_ARG(Mp > 0 && Cp > 0 && ntaps >= 1 && ntaps <= SEGNB_MAX_TAPS, "bad packed shape");
    SEGNB_CHECK_ARG(tap_off_host && mmap && cmap, "NULL map");
    p.Mp = Mp;
    p.Cp = Cp;
    p.ntaps = ntaps;
    p.s_m = s_m;
    p.s_c = s_c;
    p.mmap = mmap;
    p.cmap = cmap;
    for (int t = 0; t < ntaps; ++t) p.tap_off[t] = tap_off_host[t];
    return 0;
}

extern "C" int segnb_pack_weight(const float* w, void* wpacked, int dtype, int Mp, int Cp, int ntaps,
                                 long long s_m, long long s_c, const int* tap_off_host, const int* mmap,
                                 const int* cmap, segnb_stream_t stream) {
    SEGNB_PLAN_REFUSE("segnb_pack_weight takes a host tap table");
    SEGNB_CHECK_ARG(w && wpacked, "NULL tensor");
    PackArgs p;
    if (int rc = fill_pack_args(p, Mp, Cp, ntaps, s_m, s_c, tap_off_host, mmap, cmap)) return rc;
    const long long total = (long long)Mp * ntaps * Cp;
    int grid = ceil_div(total, 256);
    if (grid > 4096) grid = 4096;
    if (int rc = segnb_dispatch_dtype(dtype, "segnb_pack_weight", [&](auto tag) SEGNB_INLINE_LAMBDA {
            using T = SEGNB_TAG_T(tag);
            hipLaunchKernelGGL(pack_weight_kernel<T>, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, (T*)wpacked, p);
        }))
        return rc;
    SEGNB_LAUNCH_CHECK();
    return 0;
}

extern "C" int segnb_unpack_wgrad(float* dwp, float* gw, int Mp, int Cp, int ntaps, long long s_m,
                                  long long s_c, const int* tap_off_host, const int* mmap, const int* cmap,
                                  int accumulate, segnb_stream_t stream) {
    SEGNB_PLAN_REFUSE("segnb_unpack_wgrad takes a host tap table");
    SEGNB_CHECK_ARG(dwp && gw, "NULL tensor");
    PackArgs p;
    if (int rc = fill_pack_args(p, Mp, Cp, ntaps, s_m, s_c, tap_off_host, mmap, cmap)) return rc;
    const long long total = (long long)Mp * ntaps * Cp;
    int grid = ceil_div(total, 256);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(unpack_wgrad_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, dwp, gw, p, accumulate);
    SEGNB_LAUNCH_CHECK();
    return 0;
}

extern "C" int segnb_pack_job_bytes(void) { return (int)sizeof(PackJob); }

// number of blocks (tiles) a job occupies -- the host needs it to fill PackJob.block_start
extern "C" int segnb_pack_job_blocks(int Mp, int Cp, int ntaps, long long s_m, long long s_c) {
    PackJob j;
    j.Mp = Mp; j.Cp = Cp; j.ntaps = ntaps; j.s_m = s_m; j.s_c = s_c;
    const bool fast_is_c = s_c < s_m;
    const long long tsrc = fast_is_c ? s_c : s_m;
    // tiled kernel sized for parameter tensors of <= 3x3 positions.  An unmasked job has at most one packed tap per kernel
    // position (ntaps <= tsrc <= 9); more packed taps than positions means a MASKED job (several packed taps per position,
    // PackJob.masked: the 4 x 4 sub-pixel kernels, 16 taps) -- anything beyond that is refused
    if (tsrc > 9 || ntaps > 16) return -1;
    if (fast_is_c) return ((Cp + 255) / 256) * Mp;
    return ((Mp + 7) / 8) * ((Cp + 63) / 64);
}

extern "C" int segnb_pack_weight_multi(const void* jobs, int njobs, int total_blocks, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_pack_weight_multi, jobs, njobs, total_blocks, stream);
    SEGNB_CHECK_ARG(jobs && njobs > 0 && total_blocks > 0, "bad job table");
    int grid = total_blocks;
    const int cap = segnb_knob_pack_blocks();
    if (cap > 0 && grid > cap) grid = cap;
    hipLaunchKernelGGL(pack_tiled_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream,
                       (const PackJob*)jobs, njobs, total_blocks);
    SEGNB_LAUNCH_CHECK();
    return 0;
}

extern "C" int segnb_unpack_wgrad_multi(const void* jobs, int njobs, int total_blocks, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_unpack_wgrad_multi, jobs, njobs, total_blocks, stream);
    SEGNB_CHECK_ARG(jobs && njobs > 0 && total_blocks > 0, "bad job table");
    hipLaunchKernelGGL(pack_tiled_kernel<false>, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream,
                       (const PackJob*)jobs, njobs, total_blocks);
    SEGNB_LAUNCH_CHECK();
    return 0;
}

extern "C" int segnb_pack_pair_job_bytes(void) { return (int)sizeof(PackPairJob); }

// blocks of one pair job, or -1 when the shape is not served (the two single-form jobs of segnb_pack_weight_multi then)
extern "C" int segnb_pack_pair_job_blocks(int Co, int Ci, int Cop, int Cip) {
    if (Co <= 0 || Ci <= 0 || Cop < Co || Cip < Ci || Cop % 8 != 0 || Cip % 8 != 0) return -1;
    return ((Cop + PP_CO - 1) / PP_CO) * ((Cip + PP_CI - 1) / PP_CI);
}

extern "C" int segnb_pack_weight_pair_multi(const void* jobs, int njobs, int total_blocks, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_pack_weight_pair_multi, jobs, njobs, total_blocks, stream);
    SEGNB_CHECK_ARG(jobs && njobs > 0 && total_blocks > 0, "bad job table");
    hipLaunchKernelGGL(pack_pair_kernel<false>, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, (const PackPairJob*)jobs, njobs,
                       0ll, 0.f);
    SEGNB_LAUNCH_CHECK();
    return 0;
}

// torch.optim.SGD.step() (torch_train.py:71,190: plain SGD) on the parameters of the job table AND their weight pack in one pass:
// flat_p / flat_g are the flat parameter / gradient buffers every job's `w` points into (segnb.engine.FlatParams); the parameters the
// table does not cover take segnb_sgd_ranges
extern "C" int segnb_sgd_pack_pair_multi(const void* jobs, int njobs, int total_blocks, float* flat_p, const float* flat_g, float lr,
                                         segnb_stream_t stream) {
    SEGNB_PLAN_REFUSE("segnb_sgd_pack_pair_multi belongs to optimizer.step(), outside the recorded lists");
    SEGNB_CHECK_ARG(jobs && njobs > 0 && total_blocks > 0 && flat_p && flat_g, "bad job table / buffers");
    SEGNB_CHECK_ARG((((uintptr_t)flat_p | (uintptr_t)flat_g) & 15) == 0, "buffers must be 16-byte aligned");
    hipLaunchKernelGGL(pack_pair_kernel<true>, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, (const PackPairJob*)jobs, njobs,
                       (long long)(flat_g - flat_p), lr);
    SEGNB_LAUNCH_CHECK();
    return 0;
}

// p[i] -= lr * g[i] over nranges element ranges of two parallel fp32 buffers: ranges = device int64 [nranges][3] (start, length,
// first index of the range in the concatenation of all ranges), total = sum of the lengths.  What segnb_sgd_pack_pair_multi leaves
// of a model's flat parameter buffer: convolution biases, BatchNorm parameters, the classifier (a few thousand elements)
__global__ __launch_bounds__(256) void sgd_ranges_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                         const long long* __restrict__ ranges, int nranges, long long total, float lr) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    int lo = 0, hi = nranges - 1;                    // last range whose first index is <= i
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (ranges[3 * mid + 2] <= i) lo = mid; else hi = mid - 1;
    }
    const long long e = ranges[3 * lo] + (i - ranges[3 * lo + 2]);
    p[e] -= lr * g[e];
}

extern "C" int segnb_sgd_ranges(float* p, const float* g, const long long* ranges, int nranges, long long total, float lr,
                                segnb_stream_t stream) {
    SEGNB_PLAN_REFUSE("segnb_sgd_ranges belongs to optimizer.step(), outside the recorded lists");
    SEGNB_CHECK_ARG(p && g && ranges && nranges > 0 && total > 0, "bad arguments");
    hipLaunchKernelGGL(sgd_ranges_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, g, ranges,
                       nranges, total, lr);
    SEGNB_LAUNCH_CHECK();
    return 0;
}

extern "C" int segnb_pack_elem_job_blocks(int Mp, int Cp, int ntaps) {
    if (Mp <= 0 || Cp <= 0 || ntaps < 1 || ntaps > SEGNB_MAX_TAPS) return -1;
    return (int)(((long long)Mp * ntaps * Cp + 256 * PACKW_ITEMS - 1) / (256 * PACKW_ITEMS));
}

extern "C" int segnb_pack_weight_elem_multi(const void* jobs, int njobs, int total_blocks, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_pack_weight_elem_multi, jobs, njobs, total_blocks, stream);
    SEGNB_CHECK_ARG(jobs && njobs > 0 && total_blocks > 0, "bad job table");
    hipLaunchKernelGGL(pack_elem_multi_kernel<true>, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream,
                       (const PackJob*)jobs, njobs);
    SEGNB_LAUNCH_CHECK();
    return 0;
}

extern "C" int segnb_unpack_wgrad_elem_multi(const void* jobs, int njobs, int total_blocks, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_unpack_wgrad_elem_multi, jobs, njobs, total_blocks, stream);
    SEGNB_CHECK_ARG(jobs && njobs > 0 && total_blocks > 0, "bad job table");
    hipLaunchKernelGGL(pack_elem_multi_kernel<false>, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream,
                       (const PackJob*)jobs, njobs);
    SEGNB_LAUNCH_CHECK();
    return 0;
}

extern "C" int segnb_pack_input_nchw(const float* x, int N, int C, int H, int W, void* out, int dtype, int Cp,
                                     int ld_out, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_pack_input_nchw, x, N, C, H, W, out, dtype, Cp, ld_out, stream);
    SEGNB_CHECK_ARG(x && out, "NULL tensor");
    SEGNB_CHECK_ARG(N > 0 && C > 0 && H > 0 && W > 0 && Cp % 8 == 0 && Cp >= C && ld_out >= Cp && ld_out % 8 == 0,
                    "bad shape");
    const long long total = (long long)N * H * W * (Cp / 8);
    int grid = ceil_div(total, 256);
    if (grid > 8192) grid = 8192;
    if (int rc = segnb_dispatch_dtype(dtype, "segnb_pack_input_nchw", [&](auto tag) SEGNB_INLINE_LAMBDA {
            using T = SEGNB_TAG_T(tag);
            hipLaunchKernelGGL(pack_input_kernel<T>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, (T*)out, N, C, H, W, Cp,
                               ld_out);
        }))
        return rc;
    SEGNB_LAUNCH_CHECK();
    return 0;
}
