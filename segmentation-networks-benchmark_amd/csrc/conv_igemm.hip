// Implicit-GEMM gather-convolution on MFMA for gfx950: forward / data-gradient (conv_fprop) and
// weight-gradient (conv_wgrad), NHWC activations, no im2col buffer.
//
// Replaces aten::convolution / aten::convolution_backward as reached from nn.Conv2d /
// nn.ConvTranspose2d in lib/models/zf_unet.py:8, linknet.py:12-21,41, tiramisu.py:14,65,
// unet16.py:17,38 (cuDNN / oneDNN in the reference).
//
// GEMM view (fprop):  M = N*QH*QW pixels, N = Co, K = ntaps*Ci.
//   A[m][k]  gathered on the fly: k -> (tap, ci), row m -> (n, qh, qw) -> input pixel, zero outside
//   B[co][k] packed weights, K contiguous
// Block = 256 threads = 4 waves; tile BM x BN; K step = 128 bytes of K per row (64 bf16 / 32 f32),
// register-staged double-buffered LDS, rows padded to 144 B (conflict-free ds_read_b128).
// Wave tile WM x WN out of v_mfma_f32_32x32x16_bf16 (bf16) / v_mfma_f32_32x32x2_f32 (exact fp32).
// Epilogue: +bias, round to T, per-channel sum / sum^2 of the stored values (BatchNorm batch
// statistics), staged through LDS so global stores are 16-byte, pixel-contiguous.
#include <stdlib.h>

#include "device.h"

namespace {

constexpr int LDS_ROW = 144;  // 128 B of K + 16 B pad
constexpr int NT = 256;       // threads per block

// (every member has an initialiser: an entry point starts from make_fprop_args below and sets only what is its own)
struct FpropArgs {
    segnb_conv_geom g = {};
    const void* in = nullptr;
    const void* w = nullptr;
    const float* bias = nullptr;
    int bias_n = 0;
    const float* ep_coef = nullptr;      // affine + activation epilogue (segnb_conv_fprop_act); ep_act < 0: off
    int ep_act = -1;
    float ep_slope = 0.f;
    void* out = nullptr;
    double* stats = nullptr;
    int M = 0, Ktot = 0, ksteps = 0, MT = 0, NTL = 0, GM = 0;
    unsigned in_bytes = 0, w_bytes = 0;          // extents of the two buffers (buffer-load bounds checks)
    // fused BatchNorm-backward REDUCTION in the store pass of a data-gradient launch (segnb_conv_fprop_bnreduce; template BNR):
    // the output is the gradient g of an activation a = act(BatchNorm(y)); with y the store threads accumulate sum dz and
    // sum dz * yhat, dz = round(g * act'(z)) -- segnb_bn_act_bwd_reduce without its own pass over (g, y).  FCDenseNet's dense
    // layers (tiramisu.py:9-20: norm -> relu -> conv): the data gradient 16 -> C of every layer, C up to ~1100
    const void* bn_y = nullptr;
    int bn_ld = 0;
    const float* bn_coef = nullptr;      // [4][Co]: scale, shift, mean, invstd (segnb_bn_finalize)
    double* bn_sums = nullptr;           // [SEGNB_STAT_REPLICAS][2][Co]
    int bn_act = 0;
    float bn_slope = 0.f;
    // BNM 2 (segnb_conv_fprop_bnapply): the SECOND launch of a data gradient that is never stored -- the tile is recomputed (K is
    // 144 deep for a dense layer: the launch is its output's bytes), dz = round(g * act'(z)) again, and what leaves is the
    // BatchNorm-backward result dy = round(a * (dz - c1 - yhat * c2)) [+ the gradient already in bn_acc] with (a, c1, c2) from the
    // sums the first launch (BNM 1: sums only, nothing stored) completed -- segnb_bn_bwd_apply_fused_direct(_acc) without g in memory
    double bn_count = 0.0;
    const float* bn_gamma = nullptr;     // [bn_C] or NULL
    int bn_C = 0;                        // real BatchNorm channels (<= Co)
    float* bn_bcoef = nullptr;           // [3][Co] out (written by the blocks of pixel tile 0)
    float* bn_dgamma = nullptr;          // [bn_C] +=
    float* bn_dbeta = nullptr;
    void* bn_acc = nullptr;              // [N][Ho][Wo][bn_acc_ld] the BatchNorm input's gradient
    int bn_acc_ld = 0, bn_accumulate = 0;
    int bn_mode = 0;                     // the BNM instantiation a BNR launch takes
    // segnb_conv_fprop_drop (conv_fprop_deepk_kernel): out = round(round(acc + bias) * drop[n][co]); statistics rows stats_ld apart
    const float* drop = nullptr;
    int ld_drop = 0, stats_ld = 0;
};
static_assert(sizeof(FpropArgs) == 800, "FpropArgs is a kernel argument: its layout is that of the kernels compiled against it");

struct WgradArgs {
    segnb_conv_geom g;
    const void* in;
    const void* dout;
    float* dwp;
    int M, Ktot, MT, NTL, S, steps_per_split, total_steps;
};

// (make_rsrc, device.h: loads beyond the descriptor's `bytes` return zeros)
constexpr unsigned OOB_OFFSET = 0x80000000u;
__device__ __forceinline__ uint4 buf_load16(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0);
    return make_uint4(v.x, v.y, v.z, v.w);
}

// acc[TM][TN] += A_tile(rows am0.., K step) * B_tile(rows bn0..)^T ; tiles are [rows][LDS_ROW] images
template <typename T, int TM, int TN>
__device__ __forceinline__ void mma_step(const unsigned char* __restrict__ sA,
                                         const unsigned char* __restrict__ sB, int r, int h,
                                         f32x16_t (&acc)[TM][TN]) {
    if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            bf16x8_t af[TM], bfr[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i)
                af[i] = *reinterpret_cast<const bf16x8_t*>(sA + (32 * i + r) * LDS_ROW + kk * 32 + h * 16);
#pragma unroll
            for (int j = 0; j < TN; ++j)
                bfr[j] = *reinterpret_cast<const bf16x8_t*>(sB + (32 * j + r) * LDS_ROW + kk * 32 + h * 16);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        }
    } else {
        // fp32: lane (r,h) feeds k = 16h + 4q + e at sub-step (q,e) -- any K permutation is a valid
        // contraction order as long as A and B agree; this one keeps the LDS reads 16-byte.
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float4 af[TM], bfr[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i)
                af[i] = *reinterpret_cast<const float4*>(sA + (32 * i + r) * LDS_ROW + h * 64 + q * 16);
#pragma unroll
            for (int j = 0; j < TN; ++j)
                bfr[j] = *reinterpret_cast<const float4*>(sB + (32 * j + r) * LDS_ROW + h * 64 + q * 16);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].x, bfr[j].x, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].y, bfr[j].y, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].z, bfr[j].z, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].w, bfr[j].w, acc[i][j], 0, 0, 0);
                }
        }
    }
}

template <int BM, int BN, typename T>
constexpr int fprop_smem_bytes() {
    return 2 * (BM + BN) * LDS_ROW + BM * 16 + 4 * 2 * BN * 4 + SEGNB_MAX_TAPS * 8;
}

// ================================================================================================
// forward / data-gradient
// ================================================================================================
// BNM (with BNR): 0 the gradient is stored and reduced, 1 reduced only (nothing stored), 2 recomputed and APPLIED (FpropArgs::bn_acc)
template <typename T, int BM, int BN, int WM, int WN, bool EP = false, bool BNR = false, int BNM = 0>      // EP: affine + activation epilogue; BNR: FpropArgs::bn_y (separate instantiations)
__global__ __launch_bounds__(NT) void conv_fprop_kernel(const FpropArgs a) {
    static_assert(!BNR || (!EP && sizeof(T) == 2 && NT % (BN / 8) == 0 && NT >= 2 * BN), "BatchNorm-reduce store pass: bf16, one fixed channel chunk per thread");
    static_assert(BNM == 0 || BNR, "BNM selects the form of the BatchNorm store pass");
    __shared__ float sApp[BNM == 2 ? 4 * BN : 1];          // BNM 2: a, c1, c2, invstd of the block's channels
    constexpr int EPC = Elem<T>::EPC;
    constexpr int BK = 8 * EPC;
    constexpr int AI = BM / 32, BI = BN / 32;
    constexpr int WAVES_N = BN / WN;
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int TILE_BYTES = (BM + BN) * LDS_ROW;
    constexpr int OUT_ROW = BN * (int)sizeof(T) + 16;
    static_assert((BM / WM) * (BN / WN) == 4, "4 waves");
    static_assert(BM * OUT_ROW <= 2 * TILE_BYTES, "staging fits");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* sTiles = smem;
    int4* sRow = reinterpret_cast<int4*>(smem + 2 * TILE_BYTES);
    float* sStat = reinterpret_cast<float*>(sRow + BM);
    int2* sTap = reinterpret_cast<int2*>(sStat + 4 * 2 * BN);      // sStat: one [2*BN] row per wave row

    const segnb_conv_geom& g = a.g;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wr = wave / WAVES_N, wc = wave % WAVES_N;
    const int c = tid & 7, row0 = tid >> 3;

    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int nt = L % a.NTL;
    const int gq = L / a.NTL;
    const int n_base = nt * BN;

    T* __restrict__ outT = reinterpret_cast<T*>(a.out);

    if (tid < g.ntaps) sTap[tid] = make_int2(g.dh[tid], g.dw[tid]);

    const int QHW = g.QH * g.QW;
    double st = 0.0;
    const __amdgpu_buffer_rsrc_t rsrc_in = make_rsrc(a.in, a.in_bytes);
    const __amdgpu_buffer_rsrc_t rsrc_w = make_rsrc(a.w, a.w_bytes);
    unsigned b_off[BI];                 // weight rows of this thread: byte offset of (co, k = c*EPC), constant
#pragma unroll
    for (int j = 0; j < BI; ++j) {
        const int co = n_base + row0 + 32 * j;
        b_off[j] = co < g.Co ? (unsigned)(co * a.Ktot + c * EPC) * (unsigned)sizeof(T) : OOB_OFFSET;
    }

    // BNR: this thread stores channel chunk tid % OC of every row it stores: its two sums stay in registers, the per-channel
    // constants (mean, scale, shift) of the block's BN channels in LDS (sStat: a BNR launch takes no forward statistics) --
    // 24 registers that cost the 128 x 128 tile its second block per CU
    float bs1[BNR ? 8 : 1], bs2[BNR ? 8 : 1];
    float bneg = 0.f;
    if constexpr (BNR) {
        for (int c2 = tid; c2 < BN; c2 += NT) {
            const int ch = n_base + c2;
            const bool in = ch < g.Co;
            sStat[c2] = in ? a.bn_coef[2 * g.Co + ch] : 0.f;          // mean
            sStat[BN + c2] = in ? a.bn_coef[ch] : 0.f;                // scale
            sStat[2 * BN + c2] = in ? a.bn_coef[g.Co + ch] : 0.f;     // shift
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) bs1[e] = bs2[e] = 0.f;
        bneg = act_neg_scale(a.bn_act, a.bn_slope);
        if constexpr (BNM == 2) {
            // the fused finalize of bn_bwd_apply_kernel (norm_act.hip: bn_bwd_coef): every block derives (a, c1, c2) of its
            // channels from the completed sums; the blocks of pixel tile 0 publish them and add dgamma / dbeta
            for (int c2 = tid; c2 < BN; c2 += NT) {
                const int ch = n_base + c2;
                float av = 0.f, c1 = 0.f, c2v = 0.f, is = 0.f;
                if (ch < a.bn_C) {
                    double v1[SEGNB_STAT_REPLICAS], v2[SEGNB_STAT_REPLICAS];
#pragma unroll
                    for (int rp = 0; rp < SEGNB_STAT_REPLICAS; ++rp) {
                        v1[rp] = a.bn_sums[(long long)(rp * 2) * g.Co + ch];
                        v2[rp] = a.bn_sums[(long long)(rp * 2 + 1) * g.Co + ch];
                    }
                    double sdz = 0.0, sdzy = 0.0;
#pragma unroll
                    for (int rp = 0; rp < SEGNB_STAT_REPLICAS; ++rp) {
                        sdz += v1[rp];
                        sdzy += v2[rp];
                    }
                    is = a.bn_coef[3 * g.Co + ch];
                    av = (a.bn_gamma != nullptr ? a.bn_gamma[ch] : 1.f) * is;
                    c1 = (float)(sdz / a.bn_count);
                    c2v = (float)(sdzy / a.bn_count);
                    if (gq == 0) {
                        if (a.bn_dgamma != nullptr) a.bn_dgamma[ch] += (float)sdzy;
                        if (a.bn_dbeta != nullptr) a.bn_dbeta[ch] += (float)sdz;
                    }
                }
                if (gq == 0 && ch < g.Co && a.bn_bcoef != nullptr) {
                    a.bn_bcoef[ch] = av;
                    a.bn_bcoef[g.Co + ch] = c1;
                    a.bn_bcoef[2 * g.Co + ch] = c2v;
                }
                sApp[c2] = av;
                sApp[BN + c2] = c1;
                sApp[2 * BN + c2] = c2v;
                sApp[3 * BN + c2] = is;
            }
        }
    }

    for (int mt = gq; mt < a.MT; mt += a.GM) {
        const int m_base = mt * BM;
        __syncthreads();  // previous tile's staging / row table fully consumed
        for (int rr = tid; rr < BM; rr += NT) {
            const int m = m_base + rr;
            int4 ri;
            if (m < a.M) {
                const int n = m / QHW;
                const int rem = m - n * QHW;
                const int qh = rem / g.QW;
                const int qw = rem - qh * g.QW;
                ri.x = n * (g.Hi * g.Wi);
                ri.y = qh * g.in_step;
                ri.z = qw * g.in_step;
                ri.w = (n * g.Ho + qh * g.out_step + g.oh0) * g.Wo + qw * g.out_step + g.ow0;
            } else {
                ri.x = 0;
                ri.y = -(1 << 28);
                ri.z = -(1 << 28);
                ri.w = -1;
            }
            sRow[rr] = ri;
        }
        __syncthreads();

        int rn[AI], rh[AI], rw[AI];
#pragma unroll
        for (int i = 0; i < AI; ++i) {
            const int4 ri = sRow[row0 + 32 * i];
            rn[i] = ri.x;
            rh[i] = ri.y;
            rw[i] = ri.z;
        }

        f32x16_t acc[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

        // Loads go through buffer descriptors: a 32-bit byte offset per lane, a wave-uniform scalar offset per K
        // step, and the hardware bounds check -- a row outside the image (or a channel tile outside Co) gets an
        // offset beyond the buffer and reads back zeros, with no branch and no register clearing.  This thread's
        // 16-byte chunk walks K as (tap, channel): tracked incrementally, the gather offsets of the AI rows are
        // recomputed only when the tap changes.  (The previous form -- division of k by Ci, bounds tests, 64-bit
        // addresses and zero fills for every row of every K step -- issued 9 VALU instructions per MFMA.)
        uint4 ra[AI], rb[BI];
        int k_tap = 0, k_ci = c * EPC;                      // this thread's chunk of K step 0
        while (k_ci >= g.Ci) { k_ci -= g.Ci; ++k_tap; }
        unsigned a_off[AI];
        auto set_tap = [&]() {
            const int2 t = sTap[k_tap < g.ntaps ? k_tap : 0];
#pragma unroll
            for (int i = 0; i < AI; ++i) {
                const int hi = rh[i] + t.x, wi = rw[i] + t.y;
                const bool ok = k_tap < g.ntaps && (unsigned)hi < (unsigned)g.Hi && (unsigned)wi < (unsigned)g.Wi;
                a_off[i] = ok ? (unsigned)((rn[i] + hi * g.Wi + wi) * g.ld_in) * (unsigned)sizeof(T) : OOB_OFFSET;
            }
        };
        set_tap();
        auto gload = [&](int s) {
#pragma unroll
            for (int i = 0; i < AI; ++i) ra[i] = buf_load16(rsrc_in, a_off[i] + (unsigned)k_ci * (unsigned)sizeof(T), 0);
            const unsigned kb = (unsigned)(s * BK) * (unsigned)sizeof(T);          // wave-uniform
            const bool kok = s * BK + c * EPC < a.Ktot;                             // false only in a ragged last step
#pragma unroll
            for (int j = 0; j < BI; ++j) rb[j] = buf_load16(rsrc_w, kok ? b_off[j] : OOB_OFFSET, kb);
            // advance this thread's chunk by one K step
            k_ci += BK;
            if (k_ci >= g.Ci) {
                do { k_ci -= g.Ci; ++k_tap; } while (k_ci >= g.Ci);
                set_tap();
            }
        };
        auto lstore = [&](int buf) {
            unsigned char* base = sTiles + buf * TILE_BYTES;
#pragma unroll
            for (int i = 0; i < AI; ++i)
                *reinterpret_cast<uint4*>(base + (row0 + 32 * i) * LDS_ROW + c * 16) = ra[i];
#pragma unroll
            for (int j = 0; j < BI; ++j)
                *reinterpret_cast<uint4*>(base + (BM + row0 + 32 * j) * LDS_ROW + c * 16) = rb[j];
        };

        gload(0);
        lstore(0);
        __syncthreads();
        for (int s = 0; s < a.ksteps; ++s) {
            const int buf = s & 1;
            if (s + 1 < a.ksteps) gload(s + 1);
            const unsigned char* sA = sTiles + buf * TILE_BYTES + (wr * WM) * LDS_ROW;
            const unsigned char* sB = sTiles + buf * TILE_BYTES + (BM + wc * WN) * LDS_ROW;
            mma_step<T, TM, TN>(sA, sB, r, h, acc);
            if (s + 1 < a.ksteps) lstore(buf ^ 1);
            __syncthreads();
        }

        // BNR: the y rows of the pixels this thread stores are requested NOW -- their latency runs under the staging below
        // (requested inside the store loop they were RPT dependent round trips per tile: the launch took 2.4 x as long)
        constexpr int RPT = BNR ? BM * (BN / 8) / NT : 1;
        uint4 yq[RPT], xq[BNM == 2 ? RPT : 1];
        if constexpr (BNR) {
#pragma unroll
            for (int k = 0; k < RPT; ++k) {
                const int q = tid + k * NT;
                const int row = q / (BN / 8), cc = q - row * (BN / 8);
                const int opix = sRow[row].w;
                const int co = n_base + cc * 8;
                yq[k] = make_uint4(0u, 0u, 0u, 0u);
                if (opix >= 0 && co < g.Co)
                    yq[k] = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(a.bn_y) + (long long)opix * a.bn_ld + co);
                if constexpr (BNM == 2) {
                    xq[k] = make_uint4(0u, 0u, 0u, 0u);
                    if (opix >= 0 && co < g.Co && a.bn_accumulate)
                        xq[k] = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(a.bn_acc) + (long long)opix * a.bn_acc_ld + co);
                }
            }
        }
        // ---- epilogue: bias, round, stats, stage to LDS ------------------------------------------
        unsigned char* sOut = sTiles;
        float cs1[TN], cs2[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int col = wc * WN + 32 * j + r;
            const int co = n_base + col;
            float bv = (a.bias != nullptr && co < a.bias_n) ? a.bias[co] : 0.f;
            float sv = 1.f, ep_neg = 1.f;
            if constexpr (EP) {
                if (a.ep_coef != nullptr && co < a.g.Co) {       // (acc + bias - mean) * scale + shift
                    sv = a.ep_coef[co];
                    bv = (bv - a.ep_coef[2 * a.g.Co + co]) * sv + a.ep_coef[a.g.Co + co];
                }
                ep_neg = act_neg_scale(a.ep_act, a.ep_slope);
            }
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int row = wr * WM + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h;
                    float ev = acc[i][j][e] + bv;
                    if constexpr (EP) {
                        ev = act_fwd_neg(acc[i][j][e] * sv + bv, ep_neg);
                    }
                    const T tv = Elem<T>::from_f32(ev);
                    *reinterpret_cast<T*>(sOut + row * OUT_ROW + col * (int)sizeof(T)) = tv;
                    if (m_base + row < a.M) {
                        const float vr = Elem<T>::to_f32(tv);
                        s1 += vr;
                        s2 += vr * vr;
                    }
                }
            }
            cs1[j] = s1;
            cs2[j] = s2;
        }
        if (a.stats != nullptr) {
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const float t1 = cs1[j] + __shfl_xor(cs1[j], 32);
                const float t2 = cs2[j] + __shfl_xor(cs2[j], 32);
                if (h == 0) {
                    // one slot per (wave row, column), summed below in a fixed order: reproducible statistics
                    const int col = wc * WN + 32 * j + r;
                    sStat[wr * 2 * BN + col] = t1;
                    sStat[wr * 2 * BN + BN + col] = t2;
                }
            }
        }
        __syncthreads();
        if (a.stats != nullptr && tid < 2 * BN) {
#pragma unroll
            for (int q = 0; q < BM / WM; ++q) st += (double)sStat[q * 2 * BN + tid];
        }
        constexpr int OC = BN / EPC;
        static_assert(!BNR || (BM * OC) % NT == 0, "BatchNorm-reduce: whole store rounds");
#pragma unroll
        for (int k = 0; k < (BNR ? RPT : 1); ++k)
        for (int q = BNR ? tid + k * NT : tid; q < (BNR ? tid + k * NT + 1 : BM * OC); q += NT) {
            const int row = q / OC, cc = q - row * OC;
            const int opix = sRow[row].w;
            const int co = n_base + cc * EPC;
            if (opix >= 0 && co < g.Co) {
                const uint4 gv = *reinterpret_cast<const uint4*>(sOut + row * OUT_ROW + cc * 16);
                if constexpr (BNM == 0) *reinterpret_cast<uint4*>(outT + (long long)opix * g.ld_out + co) = gv;
                if constexpr (BNR) {
                    // dz = round(g * act'(z)), z = (y - mean) * scale + shift: bn_act_bwd_reduce_kernel's arithmetic on the
                    // ROUNDED gradient this launch stores
                    const uint4 yv = yq[k];
                    float gq8[8], yf[8];
                    gq8[0] = __uint_as_float(gv.x << 16); gq8[1] = __uint_as_float(gv.x & 0xffff0000u);
                    gq8[2] = __uint_as_float(gv.y << 16); gq8[3] = __uint_as_float(gv.y & 0xffff0000u);
                    gq8[4] = __uint_as_float(gv.z << 16); gq8[5] = __uint_as_float(gv.z & 0xffff0000u);
                    gq8[6] = __uint_as_float(gv.w << 16); gq8[7] = __uint_as_float(gv.w & 0xffff0000u);
                    yf[0] = __uint_as_float(yv.x << 16); yf[1] = __uint_as_float(yv.x & 0xffff0000u);
                    yf[2] = __uint_as_float(yv.y << 16); yf[3] = __uint_as_float(yv.y & 0xffff0000u);
                    yf[4] = __uint_as_float(yv.z << 16); yf[5] = __uint_as_float(yv.z & 0xffff0000u);
                    yf[6] = __uint_as_float(yv.w << 16); yf[7] = __uint_as_float(yv.w & 0xffff0000u);
                    float bmu[8], bsc[8], bsh[8];
                    load8(sStat + cc * 8, bmu);
                    load8(sStat + BN + cc * 8, bsc);
                    load8(sStat + 2 * BN + cc * 8, bsh);
                    if constexpr (BNM == 2) {
                        // bn_bwd_apply_kernel's arithmetic (bn_expr.h: bn_dz_elem, bn_apply_elem; the ACC form's rounded add)
                        float aa[8], ac1[8], ac2[8], ais[8], old[8], o8[8];
                        load8(sApp + cc * 8, aa);
                        load8(sApp + BN + cc * 8, ac1);
                        load8(sApp + 2 * BN + cc * 8, ac2);
                        load8(sApp + 3 * BN + cc * 8, ais);
                        const uint4 xv = xq[k];
                        old[0] = __uint_as_float(xv.x << 16); old[1] = __uint_as_float(xv.x & 0xffff0000u);
                        old[2] = __uint_as_float(xv.y << 16); old[3] = __uint_as_float(xv.y & 0xffff0000u);
                        old[4] = __uint_as_float(xv.z << 16); old[5] = __uint_as_float(xv.z & 0xffff0000u);
                        old[6] = __uint_as_float(xv.w << 16); old[7] = __uint_as_float(xv.w & 0xffff0000u);
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const float dv = round_bf16(bn_dz_elem(gq8[e], yf[e], bmu[e], bsc[e], bsh[e], bneg));
                            const float dy = round_bf16(bn_apply_elem(yf[e], dv, bmu[e], ais[e], aa[e], ac1[e], ac2[e]));
                            o8[e] = a.bn_accumulate ? __fadd_rn(old[e], dy) : dy;
                        }
                        uint4 ov;
                        ov.x = pack2bf(o8[0], o8[1]); ov.y = pack2bf(o8[2], o8[3]);
                        ov.z = pack2bf(o8[4], o8[5]); ov.w = pack2bf(o8[6], o8[7]);
                        *reinterpret_cast<uint4*>(reinterpret_cast<T*>(a.bn_acc) + (long long)opix * a.bn_acc_ld + co) = ov;
                    } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float yc = yf[e] - bmu[e];
                        const float z = yc * bsc[e] + bsh[e];
                        const float dv = round_bf16(gq8[e] * act_grad_neg(z, bneg));
                        bs1[e] += dv;
                        bs2[e] += dv * yc;
                    }
                    }
                }
            }
        }
    }
    if constexpr (BNR && BNM != 2) {
        // fixed-order block reduction (the threads of a channel chunk are tid = cc + k * OC), one fp64 atomic per channel
        constexpr int OC = BN / 8;
        __syncthreads();
        float* red = reinterpret_cast<float*>(smem);      // [NT][16]
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            red[tid * 16 + e] = bs1[e];
            red[tid * 16 + 8 + e] = bs2[e];
        }
        __syncthreads();
        if (tid < 2 * BN) {
            const int which = tid / BN, col = tid - which * BN;
            const int c8 = col >> 3, e = col & 7;
            double sum = 0.0;
            for (int k = 0; k < NT / OC; ++k) sum += (double)red[(k * OC + c8) * 16 + which * 8 + e];
            const int co = n_base + col;
            if (co < g.Co) {
                if (which == 1) sum *= (double)a.bn_coef[3 * g.Co + co];      // * invstd: sum dz * yhat
                atomicAdd(&a.bn_sums[((long long)(blockIdx.x % SEGNB_STAT_REPLICAS) * 2 + which) * g.Co + co], sum);
            }
        }
    }
    if (a.stats != nullptr && tid < 2 * BN) {
        const int which = tid / BN, col = tid - which * BN;
        const int co = n_base + col;
        if (co < g.Co) atomicAdd(&a.stats[((long long)(blockIdx.x % SEGNB_STAT_REPLICAS) * 2 + which) * g.Co + co], st);
    }
}

// ================================================================================================
// forward of FEW pixels x FEW output channels x VERY deep K (tiramisu.py:14 at the bottleneck: 8 x 16 x 16 pixels,
// Ci ~ 1000, Co = 16 -- the block tiles above leave 16 blocks walking 140 K steps each: 175 us for 0.6 GFLOP).
// Both MFMA operands are K-contiguous in HBM as they are (NHWC pixels, packed weights), and a 32 x 32 tile per wave
// shares nothing with its neighbours, so there is no LDS staging: each of the 16 waves of a block owns every 16th
// 16-element K unit of ONE 32-pixel x 32-channel tile, loads its fragments straight into registers (8 units in flight)
// and the 16 partial tiles are summed through LDS in a fixed order.  No statistics / epilogue forms (callers that need
// them take the general kernel).
// ================================================================================================
constexpr int DK_WAVES = 16, DK_DEPTH = 8;
__global__ __launch_bounds__(DK_WAVES * 64) void conv_fprop_deepk_kernel(const FpropArgs a) {
    __shared__ float sAcc[DK_WAVES][16][64];
    const segnb_conv_geom& g = a.g;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int m_base = blockIdx.x * 32, n_base = blockIdx.y * 32;
    const __amdgpu_buffer_rsrc_t rsrc_in = make_rsrc(a.in, a.in_bytes);
    const __amdgpu_buffer_rsrc_t rsrc_w = make_rsrc(a.w, a.w_bytes);
    const int QHW = g.QH * g.QW;
    // A row of this lane = pixel m_base + r; B row = output channel n_base + r
    const int m = m_base + r;
    const bool m_ok = m < a.M;
    const int n = m_ok ? m / QHW : 0;
    const int rem = m - n * QHW;
    const int qh = rem / g.QW, qw = rem - qh * g.QW;
    const int ph = qh * g.in_step, pw = qw * g.in_step;
    const int co = n_base + r;
    const unsigned b_row = co < g.Co ? (unsigned)(co * a.Ktot + h * 8) * 2u : OOB_OFFSET;
    const int cpt = g.Ci >> 4;                       // 16-element units per tap
    const int units = g.ntaps * cpt;
    int tap = 0, c16 = wave;                         // this wave's next unit
    while (c16 >= cpt) { c16 -= cpt; ++tap; }
    unsigned a_row = OOB_OFFSET;
    auto set_tap = [&]() {
        a_row = OOB_OFFSET;
        if (tap < g.ntaps && m_ok) {
            const int hi = ph + g.dh[tap], wi = pw + g.dw[tap];
            if ((unsigned)hi < (unsigned)g.Hi && (unsigned)wi < (unsigned)g.Wi)
                a_row = (unsigned)(((n * g.Hi + hi) * g.Wi + wi) * g.ld_in + h * 8) * 2u;
        }
    };
    set_tap();
    uint4 fa[DK_DEPTH], fb[DK_DEPTH];
    auto issue = [&](int slot) {
        const bool live = tap < g.ntaps;
        fa[slot] = buf_load16(rsrc_in, live && a_row != OOB_OFFSET ? a_row + (unsigned)(c16 * 32) : OOB_OFFSET, 0);
        fb[slot] = buf_load16(rsrc_w, live && b_row != OOB_OFFSET ? b_row + (unsigned)((tap * g.Ci + c16 * 16) * 2) : OOB_OFFSET, 0);
        c16 += DK_WAVES;
        if (c16 >= cpt) {
            do { c16 -= cpt; ++tap; } while (c16 >= cpt);
            set_tap();
        }
    };
    f32x16_t acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int i = 0; i < DK_DEPTH; ++i) issue(i);
    const int rounds = (units + DK_WAVES * DK_DEPTH - 1) / (DK_WAVES * DK_DEPTH);
    for (int it = 0; it < rounds; ++it) {
#pragma unroll
        for (int i = 0; i < DK_DEPTH; ++i) {
            const bf16x8_t af = *reinterpret_cast<const bf16x8_t*>(&fa[i]);
            const bf16x8_t bf = *reinterpret_cast<const bf16x8_t*>(&fb[i]);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc, 0, 0, 0);
            issue(i);                                 // (past the last unit: out-of-range offsets, zeros)
        }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) sAcc[wave][e][lane] = acc[e];
    __syncthreads();
    // thread -> accumulator element (e, lane) of the tile: 16 * 64 = the block's 1024 threads
    const int e = tid >> 6;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < DK_WAVES; ++w) v += sAcc[w][e][lane];
    const int row = (e & 3) + 8 * (e >> 2) + 4 * h;
    const int mo = m_base + row;
    float stored = 0.f;
    if (mo < a.M && co < g.Co) {
        if (a.bias != nullptr && co < a.bias_n) v += a.bias[co];
        const int no = mo / QHW;
        const int ro = mo - no * QHW;
        const int qho = ro / g.QW, qwo = ro - qho * g.QW;
        const long long opix = (long long)(no * g.Ho + qho * g.out_step + g.oh0) * g.Wo + qwo * g.out_step + g.ow0;
        bf16_t tv = Elem<bf16_t>::from_f32(v);
        if (a.drop != nullptr)       // Dropout2d multiplier of (image, channel): segnb_conv_fprop_drop
            tv = Elem<bf16_t>::from_f32(Elem<bf16_t>::to_f32(tv) * a.drop[(long long)no * a.ld_drop + co]);
        reinterpret_cast<bf16_t*>(a.out)[opix * g.ld_out + co] = tv;
        stored = Elem<bf16_t>::to_f32(tv);
    }
    if (a.stats != nullptr) {        // statistics of the stored tile: 32 rows per channel through LDS, fixed order, one atomic each
        __syncthreads();             // (every thread has read its partial sums)
        float* red = &sAcc[0][0][0];                     // [32 rows][32 channels]
        red[row * 32 + r] = stored;
        __syncthreads();
        if (tid < 64) {
            const int which = tid >> 5, col = tid & 31;
            double sum = 0.0;
            for (int k = 0; k < 32; ++k) {
                const float x = red[k * 32 + col];
                sum += which ? (double)(x * x) : (double)x;
            }
            const int cc = n_base + col;
            if (cc < g.Co)
                atomicAdd(&a.stats[((long long)(blockIdx.x % SEGNB_STAT_REPLICAS) * 2 + which) * a.stats_ld + cc], sum);
        }
    }
}

static bool fprop_deepk_shape(const segnb_conv_geom& g) {
    const int M = g.N * g.QH * g.QW, Ktot = g.ntaps * g.Ci;
    if (!segnb_knob_fprop_deepk() || (g.Ci & 15) != 0 || Ktot < 2048) return false;
    // the block tiles of the general kernel would leave more than half of the CUs without a block
    const long long general_blocks = (long long)ceil_div(M, 128) * ceil_div(g.Co, g.Co <= 32 ? 32 : 64);
    return general_blocks * 2 <= segnb_num_cus();
}
// (plain launches: no statistics -- the kernel has them for segnb_conv_fprop_drop, which calls it directly -- and no epilogue forms)
static bool fprop_deepk_applies(const FpropArgs& a) { return a.stats == nullptr && a.ep_act < 0 && fprop_deepk_shape(a.g); }
static void launch_deepk(const FpropArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(conv_fprop_deepk_kernel, dim3(ceil_div(a.M, 32), ceil_div(a.g.Co, 32)), dim3(DK_WAVES * 64), 0, stream, a);
}

// ================================================================================================
// weight gradient:  dW[co][k'] += sum_pixels dy[pix][co] * im2col(x)[pix][k']
// GEMM view: M = Co, N = K' = ntaps*Ci, reduction over pixels (split across blocks, fp32 atomics).
// Both operands are pixel-major in HBM but MFMA wants the reduction index contiguous per lane, so
// the loader transposes EPC x EPC (8x8 bf16 / 4x4 f32) blocks in registers on the way into LDS.
// ================================================================================================
__device__ __forceinline__ void transpose_block(const uint4 (&in)[8], uint4 (&out)[8], bf16_t*) {
    const unsigned* d = reinterpret_cast<const unsigned*>(in);  // d[p*4 + w]
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        unsigned o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned lo = d[(2 * j) * 4 + (c >> 1)];
            const unsigned hi = d[(2 * j + 1) * 4 + (c >> 1)];
            o[j] = (c & 1) ? ((lo >> 16) | (hi & 0xffff0000u)) : ((lo & 0xffffu) | (hi << 16));
        }
        out[c] = make_uint4(o[0], o[1], o[2], o[3]);
    }
}
__device__ __forceinline__ void transpose_block(const uint4 (&in)[4], uint4 (&out)[4], float*) {
    out[0] = make_uint4(in[0].x, in[1].x, in[2].x, in[3].x);
    out[1] = make_uint4(in[0].y, in[1].y, in[2].y, in[3].y);
    out[2] = make_uint4(in[0].z, in[1].z, in[2].z, in[3].z);
    out[3] = make_uint4(in[0].w, in[1].w, in[2].w, in[3].w);
}

template <typename T, int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(NT) void conv_wgrad_kernel(const WgradArgs a) {
    constexpr int EPC = Elem<T>::EPC;
    constexpr int BKP = 8 * EPC;               // pixels per K step
    constexpr int ITEMS_A = (BM / EPC) * 8;    // (chunk column, pixel group) blocks of the dy tile
    constexpr int ITEMS_B = (BN / EPC) * 8;
    constexpr int ITEMS = ITEMS_A + ITEMS_B;
    constexpr int IPT = (ITEMS + NT - 1) / NT;
    constexpr int WAVES_N = BN / WN;
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int TILE_BYTES = (BM + BN) * LDS_ROW;
    static_assert((BM / WM) * (BN / WN) == 4, "4 waves");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* sTiles = smem;

    const segnb_conv_geom& g = a.g;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wr = wave / WAVES_N, wc = wave % WAVES_N;

    const int ntiles = a.MT * a.NTL;
    const int split = blockIdx.x / ntiles;
    const int tile = blockIdx.x - split * ntiles;
    const int mtile = tile / a.NTL, ntile = tile - mtile * a.NTL;
    const int mb = mtile * BM;   // co base
    const int nb = ntile * BN;   // k' base

    const T* __restrict__ inT = reinterpret_cast<const T*>(a.in);
    const T* __restrict__ doT = reinterpret_cast<const T*>(a.dout);

    // per-item constants
    int it_rowbase[IPT];   // LDS row of channel 0 of this item (A rows first, then B rows)
    int it_o[IPT];         // pixel group within the K step
    int it_ch[IPT];        // channel / ci element offset in the source tensor, or -1 = nothing to load
    int it_dh[IPT], it_dw[IPT];
    bool it_isA[IPT];
#pragma unroll
    for (int u = 0; u < IPT; ++u) {
        const int it = tid + u * NT;
        it_rowbase[u] = -1;
        it_ch[u] = -1;
        it_o[u] = 0;
        it_dh[u] = it_dw[u] = 0;
        it_isA[u] = true;
        if (it < ITEMS) {
            const bool isA = it < ITEMS_A;
            const int idx = isA ? it : it - ITEMS_A;
            const int o = idx & 7, cc = idx >> 3;
            it_isA[u] = isA;
            it_o[u] = o;
            if (isA) {
                it_rowbase[u] = cc * EPC;
                const int co = mb + cc * EPC;
                it_ch[u] = (co < g.Co) ? co : -1;
            } else {
                it_rowbase[u] = BM + cc * EPC;
                const int kp = nb + cc * EPC;
                if (kp < a.Ktot) {
                    const int tap = kp / g.Ci;
                    it_ch[u] = kp - tap * g.Ci;
                    it_dh[u] = g.dh[tap];
                    it_dw[u] = g.dw[tap];
                }
            }
        }
    }

    const int QHW = g.QH * g.QW;
    const int step_begin = split * a.steps_per_split;
    int step_end = step_begin + a.steps_per_split;
    if (step_end > a.total_steps) step_end = a.total_steps;
    const int nsteps = step_end - step_begin;

    f32x16_t acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    uint4 regs[IPT][EPC];
    auto gload = [&](int s) {
        const int pix0 = (step_begin + s) * BKP;
#pragma unroll
        for (int u = 0; u < IPT; ++u) {
            int m = pix0 + it_o[u] * EPC;
            int n = m / QHW;
            int rem = m - n * QHW;
            int qh = rem / g.QW;
            int qw = rem - qh * g.QW;
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                // branch-free: an element outside the image / the pixel range loads the tensor's first chunk instead and
                // is zeroed afterwards, so that the EPC loads of an item are all in flight together (under the nested
                // conditions of the first version each load waited for the one before it)
                const T* p = it_isA[u] ? doT : inT;
                bool ok = it_ch[u] >= 0 && m < a.M;
                if (it_isA[u]) {
                    const long long pix = (long long)(n * g.Ho + qh * g.out_step + g.oh0) * g.Wo + qw * g.out_step + g.ow0;
                    if (ok) p = doT + pix * g.ld_out + it_ch[u];
                } else {
                    const int hi = qh * g.in_step + it_dh[u], wi = qw * g.in_step + it_dw[u];
                    ok = ok && (unsigned)hi < (unsigned)g.Hi && (unsigned)wi < (unsigned)g.Wi;
                    const long long pix = (long long)(n * g.Hi + hi) * g.Wi + wi;
                    if (ok) p = inT + pix * g.ld_in + it_ch[u];
                }
                const uint4 v = *reinterpret_cast<const uint4*>(p);
                regs[u][e] = ok ? v : make_uint4(0, 0, 0, 0);
                ++m;
                if (++qw == g.QW) {
                    qw = 0;
                    if (++qh == g.QH) {
                        qh = 0;
                        ++n;
                    }
                }
            }
        }
    };
    auto lstore = [&](int buf) {
        unsigned char* base = sTiles + buf * TILE_BYTES;
#pragma unroll
        for (int u = 0; u < IPT; ++u) {
            if (it_rowbase[u] >= 0) {
                uint4 t[EPC];
                transpose_block(regs[u], t, (T*)nullptr);
#pragma unroll
                for (int cidx = 0; cidx < EPC; ++cidx)
                    *reinterpret_cast<uint4*>(base + (it_rowbase[u] + cidx) * LDS_ROW + it_o[u] * 16) = t[cidx];
            }
        }
    };

    if (nsteps > 0) {
        // ONE LDS tile: a K step is a handful of MFMAs behind a gather of 8 scattered 16-byte loads per thread, so the loop
        // is bound by load latency (rocprofv3: 80-84 % of the wave cycles waiting, 0.1 % MFMA) and what hides it is the
        // number of blocks a CU holds, not a second tile (half the LDS per block: 5 blocks per CU instead of 2-3)
        gload(0);
        lstore(0);
        __syncthreads();
        const unsigned char* sA = sTiles + (wr * WM) * LDS_ROW;
        const unsigned char* sB = sTiles + (BM + wc * WN) * LDS_ROW;
        for (int s = 0; s < nsteps; ++s) {
            if (s + 1 < nsteps) gload(s + 1);
            mma_step<T, TM, TN>(sA, sB, r, h, acc);
            __syncthreads();                          // every wave has read the tile
            if (s + 1 < nsteps) {
                lstore(0);
                __syncthreads();
            }
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int kp = nb + wc * WN + 32 * j + r;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int co = mb + wr * WM + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h;
                    if (co < g.Co && kp < a.Ktot) atomicAdd(&a.dwp[(long long)co * a.Ktot + kp], acc[i][j][e]);
                }
            }
    }
}

// ================================================================================================
// weight gradient of a convolution with AT MOST 8 output channels (one 16-byte group of dy): the heads that are a general
// convolution (linknet.py:62: 2x2, 32 -> 1 at 512 x 512).  The MFMA tiles above are built for wide dW matrices; here dW is
// 8 x (taps * Ci) numbers and the work is one pass over x and dy -- HBM-bound.  Plain FMAs: thread = (tap, 8-channel group
// of x) x pixel lane, 8 x 8 accumulators; a block walks whole output rows (no per-pixel division), x is fetched as
// contiguous 64-byte pixel rows by neighbouring threads, dy as one broadcast 16-byte load.  Partial sums meet in LDS, then
// in the workspace, with fp32 atomics (as in the general kernel).
// ================================================================================================
__global__ __launch_bounds__(NT) void conv_wgrad_co8_kernel(const WgradArgs a, int nslot, int PL) {
    __shared__ float sAcc[NT * 64 / 4];      // [nslot][64] <= 64 slots x 64 when PL >= 4; larger slot counts loop below
    const segnb_conv_geom& g = a.g;
    const int tid = threadIdx.x;
    const int slot = tid % nslot, pl = tid / nslot;
    const bool live = pl < PL;
    const int cpt = g.Ci >> 3;
    const int tap = slot / cpt, chunk = slot - tap * cpt;
    const int dh = g.dh[tap], dw = g.dw[tap];
    const bf16_t* __restrict__ x = reinterpret_cast<const bf16_t*>(a.in);
    const bf16_t* __restrict__ dy = reinterpret_cast<const bf16_t*>(a.dout);
    float acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
    const int rows = g.N * g.QH;
    for (int row = blockIdx.x; row < rows && live; row += gridDim.x) {
        const int n = row / g.QH, qh = row - n * g.QH;
        const int hi = qh * g.in_step + dh;
        if ((unsigned)hi >= (unsigned)g.Hi) continue;
        const bf16_t* xr = x + (long long)(n * g.Hi + hi) * g.Wi * g.ld_in + chunk * 8;
        const bf16_t* dr = dy + ((long long)(n * g.Ho + qh * g.out_step + g.oh0) * g.Wo + g.ow0) * g.ld_out;
        // four pixels per trip, all eight loads issued before the first FMA
        for (int qw0 = pl; qw0 < g.QW; qw0 += 4 * PL) {
            float xv[4][8], dv[4][8];
            bool ok[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int qw = qw0 + u * PL;
                const int wi = qw * g.in_step + dw;
                ok[u] = qw < g.QW && (unsigned)wi < (unsigned)g.Wi;
                const int qs = ok[u] ? qw : 0, ws = ok[u] ? wi : 0;
                load8(xr + (long long)ws * g.ld_in, xv[u]);
                load8(dr + (long long)qs * g.out_step * g.ld_out, dv[u]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (!ok[u]) continue;
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[i][j] = fmaf(dv[u][i], xv[u][j], acc[i][j]);
            }
        }
    }
    // slots in groups that fit the LDS array
    const int per_pass = (NT * 64 / 4) / 64;          // 64 slots per pass
    for (int s0 = 0; s0 < nslot; s0 += per_pass) {
        for (int i = tid; i < per_pass * 64; i += NT) sAcc[i] = 0.f;
        __syncthreads();
        if (live && slot >= s0 && slot < s0 + per_pass) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) atomicAdd(&sAcc[(slot - s0) * 64 + i * 8 + j], acc[i][j]);
        }
        __syncthreads();
        const int n_here = nslot - s0 < per_pass ? nslot - s0 : per_pass;
        for (int i = tid; i < n_here * 64; i += NT) {
            const int sl = s0 + i / 64, co = (i >> 3) & 7, ci = i & 7;
            const int t = sl / cpt, ch = sl - t * cpt;
            const float v = sAcc[i];
            if (v != 0.f) atomicAdd(&a.dwp[(long long)co * a.Ktot + t * g.Ci + ch * 8 + ci], v);
        }
        __syncthreads();
    }
}

static bool wgrad_co8_applies(const segnb_conv_geom* g) {
    const int nslot = g->ntaps * (g->Ci / 8);
    return g->Co == 8 && nslot <= NT && (long long)g->N * g->QH * g->QW >= 1024;
}

template <typename T, int BM, int BN, int WM, int WN>
int launch_fprop(FpropArgs& a, hipStream_t stream) {
    constexpr int smem = fprop_smem_bytes<BM, BN, T>();
    static_assert(smem >= NT * 16 * 4, "BatchNorm-reduce scratch");
    static const int attr_rc = [] {
        int rc = segnb_opt_in_lds("fprop_general", smem, conv_fprop_kernel<T, BM, BN, WM, WN>, conv_fprop_kernel<T, BM, BN, WM, WN, true>);
        if constexpr (sizeof(T) == 2) {
            if (rc == 0) rc = segnb_opt_in_lds("fprop_general", smem, conv_fprop_kernel<T, BM, BN, WM, WN, false, true>);
            if constexpr (BN == 64) {         // (the two-launch form of a dense layer's data gradient: 64-channel tiles only)
                if (rc == 0)
                    rc = segnb_opt_in_lds("fprop_general", smem, conv_fprop_kernel<T, BM, BN, WM, WN, false, true, 1>,
                                          conv_fprop_kernel<T, BM, BN, WM, WN, false, true, 2>);
            }
        }
        return rc;
    }();
    if (attr_rc) return attr_rc;
    a.MT = ceil_div(a.M, BM);
    a.NTL = ceil_div(a.g.Co, BN);
    const int cus = segnb_num_cus();
    int per_cu = (160 * 1024) / smem;
    if (per_cu > 3) per_cu = 3;
    if (per_cu < 1) per_cu = 1;
    int gm = (cus * per_cu) / a.NTL;
    if (gm < 1) gm = 1;
    if (gm > a.MT) gm = a.MT;
    a.GM = gm;
    const int grid = a.GM * a.NTL;
    if (a.bn_y != nullptr) {
        if constexpr (sizeof(T) == 2) {
            if (a.bn_mode == 0) {
                hipLaunchKernelGGL((conv_fprop_kernel<T, BM, BN, WM, WN, false, true>), dim3(grid), dim3(NT), smem, stream, a);
            } else if constexpr (BN == 64) {
                if (a.bn_mode == 1)
                    hipLaunchKernelGGL((conv_fprop_kernel<T, BM, BN, WM, WN, false, true, 1>), dim3(grid), dim3(NT), smem, stream, a);
                else
                    hipLaunchKernelGGL((conv_fprop_kernel<T, BM, BN, WM, WN, false, true, 2>), dim3(grid), dim3(NT), smem, stream, a);
            } else {
                return SEGNB_E_UNSUPPORTED;
            }
        } else {
            return SEGNB_E_UNSUPPORTED;
        }
    } else if (a.ep_act >= 0)
        hipLaunchKernelGGL((conv_fprop_kernel<T, BM, BN, WM, WN, true>), dim3(grid), dim3(NT), smem, stream, a);
    else
        hipLaunchKernelGGL((conv_fprop_kernel<T, BM, BN, WM, WN>), dim3(grid), dim3(NT), smem, stream, a);
    return 0;
}

template <typename T>
int dispatch_fprop(FpropArgs& a, hipStream_t stream) {
    const int Co = a.g.Co;
    const long long M = a.M;
    const int cus = segnb_num_cus();
    const long long want = (long long)cus * 3 / 2;
    if (Co <= 32) return launch_fprop<T, 128, 32, 32, 32>(a, stream);
    if (Co <= 64) {
        if ((M + 127) / 128 >= want) return launch_fprop<T, 128, 64, 64, 32>(a, stream);
        return launch_fprop<T, 64, 64, 32, 32>(a, stream);
    }
    const long long t128 = ((M + 127) / 128) * ((Co + 127) / 128);
    // (BatchNorm-reduce store pass: eight y rows in flight + the sums would leave the 128 x 128 tile one block per CU -- its K
    // is 144 deep, the second read of the pixel rows by the narrower tile is cheap)
    if (t128 >= want && a.bn_y == nullptr) return launch_fprop<T, 128, 128, 64, 64>(a, stream);
    const long long t64 = ((M + 127) / 128) * ((Co + 63) / 64);
    if (t64 >= want) return launch_fprop<T, 128, 64, 64, 32>(a, stream);
    return launch_fprop<T, 64, 64, 32, 32>(a, stream);
}

template <typename T, int BM, int BN, int WM, int WN>
int launch_wgrad(WgradArgs& a, hipStream_t stream) {
    constexpr int smem = (BM + BN) * LDS_ROW;
    static const int attr_rc = segnb_opt_in_lds("wgrad_general", smem, conv_wgrad_kernel<T, BM, BN, WM, WN>);
    if (attr_rc) return attr_rc;
    constexpr int BKP = 8 * Elem<T>::EPC;
    a.MT = ceil_div(a.g.Co, BM);
    a.NTL = ceil_div(a.Ktot, BN);
    a.total_steps = ceil_div(a.M, BKP);
    const int tiles = a.MT * a.NTL;
    const int cus = segnb_num_cus();
    // blocks per CU the pixel range is split for (measured on LinkNet34's 7x7 / transposed / 2x2 layers: 2 -> 5.53 ms of
    // weight gradients per step, 4 -> 5.19 ms, 8 -> 5.10 ms; step 10.7 -> 10.3 ms at 4)
    constexpr int per_cu = 8;
    int S = (cus * per_cu + tiles - 1) / tiles;
    if (S < 1) S = 1;
    // keep at least 4 K steps per split so the pipeline prologue amortises
    const int maxS = a.total_steps / 4 > 0 ? a.total_steps / 4 : 1;
    if (S > maxS) S = maxS;
    a.steps_per_split = ceil_div(a.total_steps, S);
    a.S = ceil_div(a.total_steps, a.steps_per_split);
    hipLaunchKernelGGL((conv_wgrad_kernel<T, BM, BN, WM, WN>), dim3(tiles * a.S), dim3(NT), smem, stream, a);
    return 0;
}

template <typename T>
int dispatch_wgrad(WgradArgs& a, hipStream_t stream) {
    const int Co = a.g.Co;
    if (Co <= 32) return launch_wgrad<T, 32, 128, 32, 32>(a, stream);
    if (Co <= 64) return launch_wgrad<T, 64, 128, 32, 64>(a, stream);
    return launch_wgrad<T, 128, 128, 64, 64>(a, stream);
}

int check_geom(const segnb_conv_geom* g) {
    SEGNB_CHECK_ARG(g != nullptr, "geom is NULL");
    SEGNB_CHECK_ARG(g->ntaps >= 1 && g->ntaps <= SEGNB_MAX_TAPS, "ntaps out of range");
    SEGNB_CHECK_ARG(g->Ci > 0 && g->Ci % 8 == 0 && g->Co > 0 && g->Co % 8 == 0, "Ci/Co must be multiples of 8");
    SEGNB_CHECK_ARG(g->ld_in % 8 == 0 && g->ld_out % 8 == 0 && g->ld_in >= g->Ci && g->ld_out >= g->Co,
                    "ld must be a multiple of 8 and >= channels");
    SEGNB_CHECK_ARG(g->N > 0 && g->QH > 0 && g->QW > 0 && g->Hi > 0 && g->Wi > 0 && g->Ho > 0 && g->Wo > 0,
                    "empty tensor");
    SEGNB_CHECK_ARG(g->in_step >= 1 && g->out_step >= 1, "steps must be >= 1");
    SEGNB_CHECK_ARG((g->QH - 1) * g->out_step + g->oh0 < g->Ho && (g->QW - 1) * g->out_step + g->ow0 < g->Wo &&
                        g->oh0 >= 0 && g->ow0 >= 0,
                    "output positions exceed the output tensor");
    SEGNB_CHECK_ARG((long long)g->N * g->Hi * g->Wi < (1ll << 31) && (long long)g->N * g->Ho * g->Wo < (1ll << 31),
                    "pixel count exceeds int32");
    return 0;
}

}  // namespace

// ---- what the forward entry points share: the forced-general switch, operand extents, argument setup, the tail after a try -----------
bool segnb_fprop_general_forced() {
    static const bool v = getenv("SEGNB_FPROP_GENERAL") != nullptr;   // A/B testing only
    return v;
}
static bool wgrad_general_only() {
    static const bool v = getenv("SEGNB_WGRAD_GENERAL") != nullptr;   // A/B testing only
    return v;
}

static int oversize(const char* fn) {
    segnb_set_error("%s: bad argument: tensor larger than 2 GiB (32-bit buffer offsets)", fn);
    return SEGNB_E_BADARG;
}

// The 32-bit buffer extents of a launch's operands: the gathered tensor up to the ci_in channels of its last pixel (g->Ci; the
// skip tensor's Ci - Cu of a virtual concat) and the packed weights, esz bytes per element.  False when either passes 2 GiB.
static bool conv_extents_fit(const segnb_conv_geom* g, long long esz, int ci_in, unsigned* inb, unsigned* wb) {
    const long long w = (long long)g->Co * g->ntaps * g->Ci * esz;
    *wb = (unsigned)w;
    return segnb_fits_desc(segnb_nhwc_bytes((long long)g->N * g->Hi * g->Wi, g->ld_in, ci_in, (int)esz), inb) && w < (1ll << 31);
}
static int conv_extents(const char* fn, const segnb_conv_geom* g, long long esz, int ci_in, unsigned* inb, unsigned* wb) {
    return conv_extents_fit(g, esz, ci_in, inb, wb) ? 0 : oversize(fn);
}
// the same of segnb_upconv_fprop*: a bf16 N x H x W x Ci tensor and the four phase matrices [CoW][4 * Ci]
static int upconv_extents(const char* fn, int N, int H, int W, int Ci, int ld_in, int CoW, unsigned* inb, unsigned* wb) {
    const long long w = 4ll * CoW * 4 * Ci * 2;
    *wb = (unsigned)w;
    return segnb_fits_desc(segnb_nhwc_bytes((long long)N * H * W, ld_in, Ci, 2), inb) && w < (1ll << 31) ? 0 : oversize(fn);
}

// Arguments of a launch of conv_fprop_kernel / conv_fprop_deepk_kernel without any epilogue: geometry, operands and their extents,
// output, statistics (rows Co apart), M and Ktot.  An entry point adds its epilogue's fields and nothing else.
static int make_fprop_args(FpropArgs& a, const char* fn, const segnb_conv_geom* g, int dtype, const void* in, const void* w,
                           const float* bias, int bias_n, void* out, double* stats) {
    a.g = *g;
    a.in = in;
    a.w = w;
    a.bias = bias;
    a.bias_n = bias_n;
    a.out = out;
    a.stats = stats;
    a.stats_ld = g->Co;
    a.M = g->N * g->QH * g->QW;
    a.Ktot = g->ntaps * g->Ci;
    return conv_extents(fn, g, dtype == SEGNB_BF16 ? 2 : 4, g->Ci, &a.in_bytes, &a.w_bytes);
}

static int launch_status(const char* fn) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        segnb_set_error("%s: launch failed: %s", fn, hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

// The end of a fused forward entry point after its tries (rc: their status, did: what they did): the error, or declined_code with
// "fn: declined_text" when no kernel took the launch, or the launch check.  The forward counterpart of finish_wgrad below.
static int finish_fprop(const char* fn, int rc, segnb_try_outcome did, int declined_code, const char* declined_text) {
    if (rc) return rc;
    if (did == SEGNB_TRY_DECLINED) {
        segnb_set_error("%s: %s", fn, declined_text);
        return declined_code;
    }
    return launch_status(fn);
}

static int conv_fprop_impl(const segnb_conv_geom* g, int dtype, const void* in, const void* wpacked, const float* bias,
                           int bias_n, void* out, double* stats, segnb_stream_t stream, const segnb_act_epilogue* ep,
                           const segnb_bn_reduce_epilogue* bn = nullptr, const segnb_bn_apply_epilogue* ap = nullptr, int bn_mode = 0);

extern "C" int segnb_conv_fprop(const segnb_conv_geom* g, int dtype, const void* in, const void* wpacked,
                                const float* bias, int bias_n, void* out, double* stats,
                                segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_conv_fprop, g, dtype, in, wpacked, bias, bias_n, out, stats, stream);
    return conv_fprop_impl(g, dtype, in, wpacked, bias, bias_n, out, stats, stream, nullptr);
}

extern "C" int segnb_conv_fprop_act(const segnb_conv_geom* g, int dtype, const void* in, const void* wpacked,
                                    const float* bias, int bias_n, void* out, const segnb_act_epilogue* ep,
                                    segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_conv_fprop_act, g, dtype, in, wpacked, bias, bias_n, out, ep, stream);
    SEGNB_CHECK_ARG(ep != nullptr && ep->act >= SEGNB_ACT_NONE && ep->act <= SEGNB_ACT_LEAKY, "bad epilogue");
    return conv_fprop_impl(g, dtype, in, wpacked, bias, bias_n, out, nullptr, stream, ep);
}

static int conv_fprop_impl(const segnb_conv_geom* g, int dtype, const void* in, const void* wpacked, const float* bias,
                           int bias_n, void* out, double* stats, segnb_stream_t stream, const segnb_act_epilogue* ep,
                           const segnb_bn_reduce_epilogue* bn, const segnb_bn_apply_epilogue* ap, int bn_mode) {
    if (int rc = check_geom(g)) return rc;
    SEGNB_CHECK_ARG(in && wpacked && (out || bn_mode != 0), "NULL tensor");
    FpropArgs a;
    if (int rc = make_fprop_args(a, __func__, g, dtype, in, wpacked, bias, bias_n, out, stats)) return rc;
    a.bn_mode = bn_mode;
    if (bn != nullptr) {          // (the general kernel's BatchNorm-reduce store pass: segnb_conv_fprop_bnreduce)
        a.bn_y = bn->y;
        a.bn_ld = bn->ld_y;
        a.bn_coef = bn->coef;
        a.bn_sums = bn->sums;
        a.bn_act = bn->act;
        a.bn_slope = bn->slope;
    }
    if (ap != nullptr) {          // (segnb_conv_fprop_bnapply)
        a.bn_y = ap->y;
        a.bn_ld = ap->ld_y;
        a.bn_coef = ap->coef;
        a.bn_sums = const_cast<double*>(ap->sums);
        a.bn_act = ap->act;
        a.bn_slope = ap->slope;
        a.bn_count = ap->count;
        a.bn_gamma = ap->gamma;
        a.bn_C = ap->C;
        a.bn_bcoef = ap->bcoef;
        a.bn_dgamma = ap->dgamma;
        a.bn_dbeta = ap->dbeta;
        a.bn_acc = ap->dx;
        a.bn_acc_ld = ap->ld_dx;
        a.bn_accumulate = ap->accumulate;
    }
    if (ep != nullptr) {
        a.ep_act = ep->act;
        a.ep_coef = ep->coef;
        a.ep_slope = ep->slope;
    }
    int rc = 0;
    if (dtype == SEGNB_BF16) {
        const bool general_env = segnb_fprop_general_forced();
        const bool general_only = general_env || bn != nullptr || ap != nullptr;
        const hipStream_t st = (hipStream_t)stream;
        segnb_try_outcome did = SEGNB_TRY_DECLINED;       // (until a kernel below takes the launch)
        const char* served = nullptr;                     // the selector that took it, for the census (segnb_kernel_took)
        // one selector of the cascade: tried while nothing failed or launched and its gate holds (inlined: this runs once per launch
        // of every replayed list; as a call per selector it read 0.2 % in FCDenseNet103's step, profiles/convsel_ab.txt)
        const auto attempt = [&](const char* name, bool gate, auto&& thunk) __attribute__((always_inline)) {
            if (!rc && !did && gate) rc = thunk();
            segnb_kernel_took(did, &served, name);
        };
        // (the affine + activation epilogue lives in the c8, rw, ws and general kernels: s1 is skipped for it)
        attempt("kernel:fprop_c8", !general_only,
                [&] { return segnb_fprop_c8_try(&did, g, in, wpacked, bias, bias_n, out, stats, st, ep); });
        attempt("kernel:fprop_thin",      // (thin input, wide output; bn or plain)
                !general_env && ap == nullptr && bn_mode == 0 && out != nullptr && ep == nullptr && stats == nullptr && bias == nullptr,
                [&] { return segnb_fprop_thin_try(&did, g, in, wpacked, out, st, bn); });
        attempt("kernel:fprop_roll", !general_only && ep == nullptr, [&] {
            return segnb_fprop_roll_try(&did, g, in, a.in_bytes, wpacked, a.w_bytes, bias, bias_n, out, stats, st);
        });
        attempt("kernel:fprop_rw", !general_only, [&] {
            return segnb_fprop_rw_try(&did, g, in, a.in_bytes, wpacked, a.w_bytes, bias, bias_n, out, stats, st, nullptr, ep);
        });
        attempt("kernel:fprop_dma", !general_only, [&] {
            return segnb_fprop_dma_try(&did, g, in, a.in_bytes, wpacked, a.w_bytes, bias, bias_n, out, stats, st, ep);
        });
        // few pixels x few channels x deep K (before the halo-tile kernel below, whose blocks also walk K serially)
        attempt("kernel:fprop_deepk", !general_only, [&] {
            if (fprop_deepk_applies(a)) {
                launch_deepk(a, st);
                did = SEGNB_TRY_LAUNCHED;
            }
            return 0;
        });
        // stride-1 3x3: image halo tile staged once in LDS, all taps from shifted rows (fprop_s1.hip)
        attempt("kernel:fprop_s1", !general_only && ep == nullptr,
                [&] { return segnb_fprop_s1_try(&did, g, in, wpacked, bias, bias_n, out, stats, st); });
        attempt("kernel:fprop_sx", !general_only && ep == nullptr,
                [&] { return segnb_fprop_sx_try(&did, g, in, wpacked, bias, bias_n, out, stats, st); });
        if (rc) return rc;
        if (did) {
            if (g_segnb_census_on) segnb_census(served);
            SEGNB_LAUNCH_CHECK();
            return 0;
        }
        if (g_segnb_census_on) segnb_census("kernel:fprop_general");
        a.ksteps = ceil_div(a.Ktot, 64);
        rc = dispatch_fprop<bf16_t>(a, (hipStream_t)stream);
    } else if (dtype == SEGNB_F32) {
        if (g_segnb_census_on) segnb_census("kernel:fprop_general");
        a.ksteps = ceil_div(a.Ktot, 32);
        rc = dispatch_fprop<float>(a, (hipStream_t)stream);
    } else {
        segnb_set_error("segnb_conv_fprop: unknown dtype %d", dtype);
        return SEGNB_E_BADARG;
    }
    if (rc) return rc;
    SEGNB_LAUNCH_CHECK();
    return 0;
}

// ---- conv -> Dropout2d -> statistics in one launch (include/segnb_hip.h: segnb_conv_fprop_drop) -------------------------------------
// served where the plain cascade above ends in conv_fprop_deepk_kernel or conv_fprop_s1x9_kernel: <= 32 output channels behind more
// than 96 input channels (below that the rolling / LDS-DMA kernels take the launch), a stride-1 3 x 3 window
static bool drop_s1_shape(const segnb_conv_geom* g) { return whole_output_3x3_s1(g) && g->Wo > 8; }

// the refusals every bf16 fast-path query starts with (check_geom leaves its message behind)
static bool fast_path_refused(const segnb_conv_geom* g, int dtype) {
    return g == nullptr || dtype != SEGNB_BF16 || check_geom(g) || segnb_fprop_general_forced();
}

extern "C" int segnb_conv_fprop_drop_ok(const segnb_conv_geom* g, int dtype) {
    if (fast_path_refused(g, dtype) || !segnb_knob_fprop_drop()) return 0;
    if (g->Co > 32 || g->Co % 8 != 0 || g->Ci <= 96 || g->Ci % 8 != 0) return 0;
    if (g->ntaps == 9 && !segnb_taps_3x3(g)) return 0;      // (a dilated 3 x 3: the plain launch, whichever kernel it ends on)
    unsigned inb, wb;
    if (!conv_extents_fit(g, 2, g->Ci, &inb, &wb)) return 0;      // (an oversize tensor is not served: no error)
    return (fprop_deepk_shape(*g) || drop_s1_shape(g)) ? 1 : 0;
}

extern "C" int segnb_conv_fprop_drop(const segnb_conv_geom* g, int dtype, const void* in, const void* wpacked, const float* bias,
                                     int bias_n, void* out, const float* dropmul, int ld_drop, double* stats, int stats_ld,
                                     segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_conv_fprop_drop, g, dtype, in, wpacked, bias, bias_n, out, dropmul, ld_drop, stats, stats_ld, stream);
    if (int rc = check_geom(g)) return rc;
    SEGNB_CHECK_ARG(in && wpacked && out && dropmul, "NULL argument");
    SEGNB_CHECK_ARG(segnb_conv_fprop_drop_ok(g, dtype), "geometry not served (segnb_conv_fprop_drop_ok)");
    SEGNB_CHECK_ARG(ld_drop >= g->Co && (stats == nullptr || stats_ld >= g->Co), "bad strides");
    if (fprop_deepk_shape(*g)) {
        FpropArgs a;
        if (int rc = make_fprop_args(a, __func__, g, dtype, in, wpacked, bias, bias_n, out, stats)) return rc;
        a.drop = dropmul;
        a.ld_drop = ld_drop;
        if (stats_ld > 0) a.stats_ld = stats_ld;
        launch_deepk(a, (hipStream_t)stream);
        return launch_status(__func__);
    }
    segnb_try_outcome did;
    const int rc = segnb_fprop_s1_try(&did, g, in, wpacked, bias, bias_n, out, stats, (hipStream_t)stream, dropmul, ld_drop, stats_ld);
    return finish_fprop(__func__, rc, did, SEGNB_E_BADARG, "the kernel refused the launch");
}

// ---- forward of an Upsample(x2) -> conv3x3 segment on the low-resolution tensor, accumulating (fprop_dma.hip, WsCfg UP_ = 2)

// the shapes the four-phase kernel serves: more than co_floor output channels (32 where it accumulates, 0 where it stores)
static int upconv_shape_ok(int N, int H, int W, int Ci, int Co, int ld_out, int dtype, int co_floor) {
    if (dtype != SEGNB_BF16 || segnb_fprop_general_forced() || !segnb_knob_fprop_dma() || !segnb_knob_fprop_upd()) return 0;
    if (N <= 0 || H <= 0 || W <= 0 || Ci % 64 != 0 || Ci < 128 || Co <= co_floor || Co % 8 != 0 || W < 12) return 0;
    return segnb_fits_desc(segnb_nhwc_bytes((long long)N * 4 * H * W, ld_out, Co, 2)) ? 1 : 0;
}

// what the three entry points below do once their arguments are checked: extents, the launch, its tail
static int upconv_launch(const char* fn, int N, int H, int W, int Ci, int ld_in, const void* in, const void* wpacked, int Co, int CoW,
                         void* out, int ld_out, double* stats, segnb_stream_t stream, const float* bias = nullptr, int bias_n = 0,
                         int no_prev = 0, int ep_act = -1, float ep_slope = 0.f) {
    unsigned inb, wb;
    if (int rc = upconv_extents(fn, N, H, W, Ci, ld_in, CoW, &inb, &wb)) return rc;
    segnb_try_outcome did;
    const int rc = segnb_fprop_upf_try(&did, N, H, W, Ci, ld_in, in, inb, wpacked, wb, Co, CoW, out, ld_out, stats, (hipStream_t)stream,
                                       bias_n > 0 ? bias : nullptr, bias_n, no_prev, ep_act, ep_slope);
    return finish_fprop(fn, rc, did, SEGNB_E_UNSUPPORTED, "no kernel for this shape");
}

extern "C" int segnb_upconv_fprop_acc_ok(int N, int H, int W, int Ci, int Co, int ld_out, int dtype) {
    return upconv_shape_ok(N, H, W, Ci, Co, ld_out, dtype, 32);
}

extern "C" int segnb_upconv_fprop_acc(int dtype, int N, int H, int W, int Ci, int ld_in, const void* in, const void* wpacked,
                                      int Co, int CoW, void* out, int ld_out, double* stats, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_upconv_fprop_acc, dtype, N, H, W, Ci, ld_in, in, wpacked, Co, CoW, out, ld_out, stats, stream);
    SEGNB_CHECK_ARG(in && wpacked && out, "NULL tensor");
    SEGNB_CHECK_ARG(segnb_upconv_fprop_acc_ok(N, H, W, Ci, Co, ld_out, dtype), "shape not served (segnb_upconv_fprop_acc_ok)");
    SEGNB_CHECK_ARG(CoW >= Co && ld_in >= Ci && ld_out >= Co, "bad strides");
    return upconv_launch(__func__, N, H, W, Ci, ld_in, in, wpacked, Co, CoW, out, ld_out, stats, stream);
}

// ---- forward of a ConvTranspose2d(4, 2, 1) (unet16.py:30) on the same kernel: the four output phases in one launch, nothing to
// accumulate into, bias in the accumulator staging
extern "C" int segnb_upconv_fprop_ok(int N, int H, int W, int Ci, int Co, int ld_out, int dtype) {
    return upconv_shape_ok(N, H, W, Ci, Co, ld_out, dtype, 0);
}

extern "C" int segnb_upconv_fprop(int dtype, int N, int H, int W, int Ci, int ld_in, const void* in, const void* wpacked, int Co,
                                  int CoW, const float* bias, int bias_n, void* out, int ld_out, double* stats,
                                  segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_upconv_fprop, dtype, N, H, W, Ci, ld_in, in, wpacked, Co, CoW, bias, bias_n, out, ld_out, stats, stream);
    SEGNB_CHECK_ARG(in && wpacked && out, "NULL tensor");
    SEGNB_CHECK_ARG(segnb_upconv_fprop_ok(N, H, W, Ci, Co, ld_out, dtype), "shape not served (segnb_upconv_fprop_ok)");
    SEGNB_CHECK_ARG(CoW >= Co && ld_in >= Ci && ld_out >= Co && bias_n >= 0 && bias_n <= Co, "bad strides");
    return upconv_launch(__func__, N, H, W, Ci, ld_in, in, wpacked, Co, CoW, out, ld_out, stats, stream, bias, bias_n, 1);
}

// the same with the activation of unet16.py:38-40 (ConvTranspose2d -> ReLU) in the accumulator staging: no pass over the output
extern "C" int segnb_upconv_fprop_act(int dtype, int N, int H, int W, int Ci, int ld_in, const void* in, const void* wpacked, int Co,
                                      int CoW, const float* bias, int bias_n, void* out, int ld_out, const segnb_act_epilogue* ep,
                                      segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_upconv_fprop_act, dtype, N, H, W, Ci, ld_in, in, wpacked, Co, CoW, bias, bias_n, out, ld_out, ep, stream);
    SEGNB_CHECK_ARG(in && wpacked && out && ep, "NULL tensor");
    SEGNB_CHECK_ARG(ep->coef == nullptr && (ep->act == SEGNB_ACT_NONE || ep->act == SEGNB_ACT_RELU || ep->act == SEGNB_ACT_LEAKY),
                    "activation only (no folded BatchNorm on this kernel)");
    SEGNB_CHECK_ARG(ep->act != SEGNB_ACT_LEAKY || (ep->slope >= 0.f && ep->slope <= 1.f), "leaky slope outside [0, 1]");
    SEGNB_CHECK_ARG(segnb_upconv_fprop_ok(N, H, W, Ci, Co, ld_out, dtype), "shape not served (segnb_upconv_fprop_ok)");
    SEGNB_CHECK_ARG(CoW >= Co && ld_in >= Ci && ld_out >= Co && bias_n >= 0 && bias_n <= Co, "bad strides");
    return upconv_launch(__func__, N, H, W, Ci, ld_in, in, wpacked, Co, CoW, out, ld_out, nullptr, stream, bias, bias_n, 1, ep->act,
                         ep->slope);
}

// ---- virtual concat: cat([Upsample x2(u), skip]) read from the two tensors (include/segnb_hip.h)
static bool upcat_geom_ok(const segnb_conv_geom* g, int dtype, int Cu) {
    if (fast_path_refused(g, dtype) || wgrad_general_only() || !segnb_knob_fprop_dma()) return false;
    if (!whole_output_3x3_s1(g) || (g->Hi & 1) || (g->Wi & 1) || g->Hi != g->Ho || g->Wi != g->Wo || g->Wo < 12) return false;
    if (Cu <= 0 || Cu >= g->Ci) return false;
    const bool thin = g->Ci % 32 == 0 && g->Ci <= 96 && g->Co <= 64 && Cu % 32 == 0 && segnb_knob_fprop_rw();      // fprop_rw.hip
    const bool wide = g->Ci % 64 == 0 && Cu % 64 == 0 && g->Co > 32;                                                  // fprop_dma.hip
    if (!thin && !wide) return false;
    return segnb_wgrad_s1_slabs(g) > 0;
}

extern "C" int segnb_conv_upcat_ok(const segnb_conv_geom* g, int dtype, int Cu) { return upcat_geom_ok(g, dtype, Cu) ? 1 : 0; }

extern "C" int segnb_conv_fprop_upcat(const segnb_conv_geom* g, int dtype, const void* in, const segnb_upcat_src* src,
                                      const void* wpacked, const float* bias, int bias_n, void* out, double* stats,
                                      segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_conv_fprop_upcat, g, dtype, in, src, wpacked, bias, bias_n, out, stats, stream);
    SEGNB_CHECK_ARG(in && src && src->u && wpacked && out, "NULL tensor");
    SEGNB_CHECK_ARG(upcat_geom_ok(g, dtype, src->Cu), "geometry not served (segnb_conv_upcat_ok)");
    unsigned inb, wb;
    if (int rc = conv_extents(__func__, g, 2, g->Ci - src->Cu, &inb, &wb)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    segnb_try_outcome did;
    int rc = segnb_fprop_roll_try(&did, g, in, inb, wpacked, wb, bias, bias_n, out, stats, st, nullptr, nullptr, src);
    if (!rc && !did) rc = segnb_fprop_rw_try(&did, g, in, inb, wpacked, wb, bias, bias_n, out, stats, st, nullptr, nullptr, src);
    if (!rc && !did) rc = segnb_fprop_dma_try(&did, g, in, inb, wpacked, wb, bias, bias_n, out, stats, st, nullptr, src);
    return finish_fprop(__func__, rc, did, SEGNB_E_UNSUPPORTED, "no kernel for this geometry");
}

static bool upsum_geom_ok(const segnb_conv_geom* g, int dtype, int Cu) {
    if (fast_path_refused(g, dtype) || !segnb_knob_fprop_dma() || !segnb_knob_fprop_rw()) return false;
    if (!whole_output_3x3_s1(g) || (g->Ho & 1) || (g->Wo & 1) || g->Wo < 12) return false;
    return g->Ci % 32 == 0 && g->Ci <= 96 && g->Co <= 96 && g->Co % 8 == 0 && Cu % 8 == 0 && Cu > 0 && Cu < g->Co;
}

extern "C" int segnb_conv_fprop_upsum_ok(const segnb_conv_geom* g, int dtype, int Cu) { return upsum_geom_ok(g, dtype, Cu) ? 1 : 0; }

extern "C" int segnb_conv_fprop_upsum(const segnb_conv_geom* g, int dtype, const void* in, const void* wpacked, void* out,
                                      const segnb_upcat_src* dst, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_conv_fprop_upsum, g, dtype, in, wpacked, out, dst, stream);
    SEGNB_CHECK_ARG(in && wpacked && out && dst && dst->u, "NULL tensor");
    SEGNB_CHECK_ARG(upsum_geom_ok(g, dtype, dst->Cu), "geometry not served (segnb_conv_fprop_upsum_ok)");
    unsigned inb, wb;
    if (int rc = conv_extents(__func__, g, 2, g->Ci, &inb, &wb)) return rc;
    segnb_try_outcome did;
    const int rc = segnb_fprop_rw_try(&did, g, in, inb, wpacked, wb, nullptr, 0, out, nullptr, (hipStream_t)stream, nullptr, nullptr,
                                      nullptr, dst);
    return finish_fprop(__func__, rc, did, SEGNB_E_UNSUPPORTED, "no kernel for this geometry");
}

// ---- the shared ends of the four weight-gradient entry points (segnb_conv_wgrad, _upcat, _bnapply, _tf)
// The target armed for this call (segnb_wgrad_target_arm) or NULL, checked against g.  Each of them takes it right after
// SEGNB_PLAN_RECORD, before anything can return: the call consumes an armed target whatever happens next, an argument error
// included, so a target never leaks into the next call.
static int take_wgrad_target(const char* fn, const segnb_conv_geom* g, const segnb_wgrad_target** tgt) {
    const segnb_wgrad_target* t = *tgt = segnb_take_wgrad_target();
    if (t != nullptr && (g == nullptr || t->ntaps != g->ntaps || t->Co > g->Co || g->Co - t->Co >= 8 || t->Ci > g->Ci)) {
        segnb_set_error("%s: bad argument: the armed segnb_wgrad_target does not belong to this geometry (taps / channel counts)", fn);
        return SEGNB_E_BADARG;
    }
    return 0;
}

// After the kernel (did: what it did): the nslab slabs it left for a target are summed into the parameter's gradient
// (segnb_wgrad_to_param; rezero: slab 0 is cleared again for the general kernels' atomics), then the launch check.  A launch no
// kernel took is SEGNB_E_UNSUPPORTED.
static int finish_wgrad(const char* fn, segnb_try_outcome did, const segnb_conv_geom* g, float* dwp, int nslab,
                        const segnb_wgrad_target* tgt, bool rezero, hipStream_t stream) {
    if (did == SEGNB_TRY_DECLINED) {
        segnb_set_error("%s: no kernel for this geometry", fn);
        return SEGNB_E_UNSUPPORTED;
    }
    if (tgt != nullptr && did == SEGNB_TRY_LAUNCHED) segnb_wgrad_to_param(dwp, g->Co, g->ntaps, g->Ci, nslab, tgt, rezero, stream);
    return launch_status(fn);
}

extern "C" int segnb_conv_wgrad_upcat(const segnb_conv_geom* g, int dtype, const void* in, const segnb_upcat_src* src,
                                      const void* dout, float* dwp, int nslab, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_conv_wgrad_upcat, g, dtype, in, src, dout, dwp, nslab, stream);
    const segnb_wgrad_target* tgt;
    if (int rc = take_wgrad_target(__func__, g, &tgt)) return rc;
    SEGNB_CHECK_ARG(in && src && src->u && dout && dwp, "NULL tensor");
    SEGNB_CHECK_ARG(upcat_geom_ok(g, dtype, src->Cu), "geometry not served (segnb_conv_upcat_ok)");
    SEGNB_CHECK_ARG(nslab == segnb_conv_wgrad_slabs(g, dtype), "nslab differs from segnb_conv_wgrad_slabs()");
    segnb_try_outcome did;
    if (int rc = segnb_wgrad_s1_try(&did, g, in, dout, dwp, nslab, (hipStream_t)stream, false, nullptr, src, tgt)) return rc;
    return finish_wgrad(__func__, did, g, dwp, nslab, tgt, false, (hipStream_t)stream);
}

// a bf16 tensor of the output's pixels and channels, ld apart (the y / dx of an epilogue), within a buffer descriptor's 2 GiB
static bool out_slice_fits(const segnb_conv_geom* g, int ld) {
    return segnb_fits_desc(segnb_nhwc_bytes((long long)g->N * g->Ho * g->Wo, ld, g->Co, 2));
}

// few input channels -> many output channels: the data gradient of a dense layer (tiramisu.py:9-20, growth 16 -> the prefix);
// the general gather kernel serves it, with the reduction in its store pass (conv_fprop_kernel<..., BNR>)
static bool bnreduce_general(const segnb_conv_geom* g) { return g->Ci <= 24 && g->Co >= 32 && g->Co % 8 == 0; }

extern "C" int segnb_conv_fprop_bnreduce_ok(const segnb_conv_geom* g, int dtype) {
    if (g == nullptr || dtype != SEGNB_BF16 || check_geom(g) || !segnb_knob_bnreduce_fused()) return 0;
    if (!whole_output_3x3_s1(g) || g->Co % 8 != 0) return 0;
    if (bnreduce_general(g)) return 1;      // (the general gather kernel: any width)
    if (segnb_fprop_general_forced() || !segnb_knob_fprop_dma() || !segnb_knob_fprop_rw() || g->Wo < 12) return 0;
    for (int t = 0; t < 9; ++t)
        if (g->dh[t] < -1 || g->dh[t] > 1 || g->dw[t] < -1 || g->dw[t] > 1) return 0;
    if (g->Ci % 32 != 0 || g->Ci > 96 || g->Co > 64) return 0;
    if (g->Co > 32 && g->Ci > 32) return 0;      // (the 64-wide tile keeps one 32-channel chunk of weights resident)
    return 1;
}

extern "C" int segnb_conv_fprop_bnreduce(const segnb_conv_geom* g, int dtype, const void* in, const void* wpacked,
                                         void* out, const segnb_bn_reduce_epilogue* ep, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_conv_fprop_bnreduce, g, dtype, in, wpacked, out, ep, stream);
    if (int rc = check_geom(g)) return rc;
    SEGNB_CHECK_ARG(in && wpacked && out && ep && ep->y && ep->sums, "NULL argument");
    SEGNB_CHECK_ARG(ep->ld_y >= g->Co && ep->ld_y % 8 == 0, "bad y stride");
    unsigned inb, wb;
    if (int rc = conv_extents(__func__, g, 2, g->Ci, &inb, &wb)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    int rc = 0;
    segnb_try_outcome did;
    if (ep->coef == nullptr) {
        // activation mask of a producing layer without BatchNorm: out = dz (conv_roll_kernel, EPI = 3)
        SEGNB_CHECK_ARG(segnb_conv_fprop_actmask_ok(g, dtype), "geometry not served by a fused kernel (segnb_conv_fprop_actmask_ok)");
        if (segnb_fprop_roll_actmask_ok(g))
            rc = segnb_fprop_roll_try(&did, g, in, inb, wpacked, wb, nullptr, 0, out, nullptr, st, ep);
        else      // 64-channel-chunk inputs: the MASK instantiation of conv_fprop_ws_kernel
            rc = segnb_fprop_dma_try(&did, g, in, inb, wpacked, wb, nullptr, 0, out, nullptr, st, nullptr, nullptr, ep);
    } else {
        SEGNB_CHECK_ARG(segnb_conv_fprop_bnreduce_ok(g, dtype), "geometry not served by a fused kernel (segnb_conv_fprop_bnreduce_ok)");
        if (bnreduce_general(g)) {
            SEGNB_CHECK_ARG(ep->ld_y % 8 == 0 && out_slice_fits(g, ep->ld_y), "bad y");
            return conv_fprop_impl(g, dtype, in, wpacked, nullptr, 0, out, nullptr, stream, nullptr, ep);
        }
        if (g->Ci <= 96) {
            rc = segnb_fprop_roll_try(&did, g, in, inb, wpacked, wb, nullptr, 0, out, nullptr, st, ep);
            if (!rc && !did) rc = segnb_fprop_rw_try(&did, g, in, inb, wpacked, wb, nullptr, 0, out, nullptr, st, ep);
        } else {
            rc = segnb_fprop_dma_try(&did, g, in, inb, wpacked, wb, nullptr, 0, out, nullptr, st, nullptr, nullptr, ep);
        }
    }
    return finish_fprop(__func__, rc, did, SEGNB_E_BADARG, "the fused kernel refused the launch");
}

// ---- a dense layer's data gradient that is never stored (include/segnb_hip.h): two launches of the general kernel
extern "C" int segnb_conv_fprop_bnapply_ok(const segnb_conv_geom* g, int dtype) {
    if (g == nullptr || dtype != SEGNB_BF16 || check_geom(g) || !segnb_knob_bnreduce_fused()) return 0;
    if (!whole_output_3x3_s1(g) || g->Co % 8 != 0 || g->Co <= 32) return 0;      // (64-channel tiles)
    return bnreduce_general(g) ? 1 : 0;
}

extern "C" int segnb_conv_fprop_bnsums(const segnb_conv_geom* g, int dtype, const void* in, const void* wpacked,
                                       const segnb_bn_reduce_epilogue* ep, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_conv_fprop_bnsums, g, dtype, in, wpacked, ep, stream);
    if (int rc = check_geom(g)) return rc;
    SEGNB_CHECK_ARG(in && wpacked && ep && ep->y && ep->coef && ep->sums, "NULL argument");
    SEGNB_CHECK_ARG(segnb_conv_fprop_bnapply_ok(g, dtype), "geometry not served (segnb_conv_fprop_bnapply_ok)");
    SEGNB_CHECK_ARG(ep->ld_y >= g->Co && ep->ld_y % 8 == 0 && out_slice_fits(g, ep->ld_y), "bad y");
    return conv_fprop_impl(g, dtype, in, wpacked, nullptr, 0, nullptr, nullptr, stream, nullptr, ep, nullptr, 1);
}

extern "C" int segnb_conv_fprop_bnapply(const segnb_conv_geom* g, int dtype, const void* in, const void* wpacked,
                                        const segnb_bn_apply_epilogue* ep, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_conv_fprop_bnapply, g, dtype, in, wpacked, ep, stream);
    if (int rc = check_geom(g)) return rc;
    SEGNB_CHECK_ARG(in && wpacked && ep && ep->y && ep->coef && ep->sums && ep->dx, "NULL argument");
    SEGNB_CHECK_ARG(segnb_conv_fprop_bnapply_ok(g, dtype), "geometry not served (segnb_conv_fprop_bnapply_ok)");
    SEGNB_CHECK_ARG(ep->C > 0 && ep->C <= g->Co && ep->count > 0.0, "bad channel count / pixel count");
    SEGNB_CHECK_ARG(ep->ld_y >= g->Co && ep->ld_y % 8 == 0 && out_slice_fits(g, ep->ld_y), "bad y");
    SEGNB_CHECK_ARG(ep->ld_dx >= g->Co && ep->ld_dx % 8 == 0 && out_slice_fits(g, ep->ld_dx), "bad dx");
    return conv_fprop_impl(g, dtype, in, wpacked, nullptr, 0, nullptr, nullptr, stream, nullptr, nullptr, ep, 2);
}

extern "C" int segnb_conv_wgrad_slabs(const segnb_conv_geom* g, int dtype) {
    if (check_geom(g)) return -1;
    if (dtype == SEGNB_BF16 && !wgrad_general_only()) {
        const int s = segnb_wgrad_s1_slabs(g);
        if (s > 0) return s;
        const int sx = segnb_wgrad_sx_slabs(g);
        if (sx > 0) return sx;
    }
    return 1;
}

extern "C" int segnb_conv_wgrad(const segnb_conv_geom* g, int dtype, const void* in, const void* dout,
                                float* dwp, int nslab, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_conv_wgrad, g, dtype, in, dout, dwp, nslab, stream);
    const segnb_wgrad_target* tgt;
    if (int rc = take_wgrad_target(__func__, g, &tgt)) return rc;
    if (int rc = check_geom(g)) return rc;
    SEGNB_CHECK_ARG(in && dout && dwp, "NULL tensor");
    SEGNB_CHECK_ARG(nslab == segnb_conv_wgrad_slabs(g, dtype), "nslab differs from segnb_conv_wgrad_slabs()");
    WgradArgs a;
    a.g = *g;
    a.in = in;
    a.dout = dout;
    a.dwp = dwp;
    a.M = g->N * g->QH * g->QW;
    a.Ktot = g->ntaps * g->Ci;
    const hipStream_t st = (hipStream_t)stream;
    int rc = 0;
    if (dtype == SEGNB_BF16) {
        // stride-1 3x3: pixel-major LDS tiles + transposing LDS reads, all taps per block (wgrad_s1.hip)
        // (with a target the fast kernels leave their slabs unreduced: segnb_wgrad_to_param sums them into the parameter's gradient)
        const bool part = tgt != nullptr, general = wgrad_general_only();
        segnb_try_outcome did = SEGNB_TRY_DECLINED;       // (until a kernel below takes the launch)
        const char* served = nullptr;                     // the selector that took it, for the census (segnb_kernel_took)
        // (one selector of the cascade, as in conv_fprop_impl)
        const auto attempt = [&](const char* name, bool gate, auto&& thunk) __attribute__((always_inline)) {
            if (!rc && !did && gate) rc = thunk();
            segnb_kernel_took(did, &served, name);
        };
        attempt("kernel:wgrad_roll", !general && segnb_knob_wgrad_roll(),
                [&] { return segnb_wgrad_roll_try(&did, g, in, dout, dwp, nslab, st, part); });
        attempt("kernel:wgrad_c8roll", !general && segnb_knob_wgrad_c8roll() && segnb_wgrad_s1_slabs(g) > 0,
                [&] { return segnb_wgrad_c8roll_try(&did, g, in, dout, dwp, nslab, st, part); });
        attempt("kernel:wgrad_s1", !general,
                [&] { return segnb_wgrad_s1_try(&did, g, in, dout, dwp, nslab, st, false, nullptr, nullptr, tgt); });
        attempt("kernel:wgrad_sx", !general, [&] { return segnb_wgrad_sx_try(&did, g, in, dout, dwp, nslab, st, part); });
        if (rc) return rc;
        if (did) {
            if (g_segnb_census_on) segnb_census(served);
            return finish_wgrad(__func__, did, g, dwp, nslab, tgt, false, st);
        }
        if (g_segnb_census_on) segnb_census("kernel:wgrad_general");
        if (wgrad_co8_applies(g)) {
            const int nslot = g->ntaps * (g->Ci / 8), PL = NT / nslot;
            int grid = segnb_num_cus() * 8;
            if (grid > g->N * g->QH) grid = g->N * g->QH;
            hipLaunchKernelGGL(conv_wgrad_co8_kernel, dim3(grid), dim3(NT), 0, (hipStream_t)stream, a, nslot, PL);
        } else
            rc = dispatch_wgrad<bf16_t>(a, (hipStream_t)stream);
    } else if (dtype == SEGNB_F32) {
        if (g_segnb_census_on) segnb_census("kernel:wgrad_general");
        rc = dispatch_wgrad<float>(a, (hipStream_t)stream);
    } else {
        segnb_set_error("segnb_conv_wgrad: unknown dtype %d", dtype);
        return SEGNB_E_BADARG;
    }
    if (rc) return rc;
    // general kernels: one slab, accumulated with atomics into the zeroed workspace -- delivered and re-zeroed in one pass
    return finish_wgrad(__func__, SEGNB_TRY_LAUNCHED, g, dwp, 1, tgt, true, st);
}

// weight gradient whose dy operand is the BatchNorm-backward apply of (g, y), recomputed in the kernel (first layer of a
// network: nothing else reads that dy -- no data gradient -- so the apply pass and its tensor disappear)
extern "C" int segnb_conv_wgrad_bnapply_ok(const segnb_conv_geom* g, int dtype) {
    if (g == nullptr || dtype != SEGNB_BF16 || check_geom(g) || wgrad_general_only()) return 0;
    // SEGNB_WGRAD_BNAPPLY: unset = only where the rolling first-layer kernel serves (conv_wgrad_c8roll_kernel: -0.85 % of the
    // timed step), 1 = the thin tile kernel's variant too (measured neutral: profiles/r04_ab.txt), 0 = never
    const char* e = getenv("SEGNB_WGRAD_BNAPPLY");
    if ((e != nullptr && e[0] == '0') || g->Co > 32 || g->Co % 8 != 0 || segnb_wgrad_s1_slabs(g) <= 0) return 0;
    if (segnb_knob_wgrad_c8roll() && segnb_wgrad_c8roll_applies(g)) return 1;
    return e != nullptr ? 1 : 0;
}

extern "C" int segnb_conv_wgrad_bnapply(const segnb_conv_geom* g, int dtype, const void* in, const void* gsrc, int ld_g,
                                        const void* y, int ld_y, const float* coef, const float* bcoef, int Cp, int act,
                                        float slope, float* dwp, int nslab, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_conv_wgrad_bnapply, g, dtype, in, gsrc, ld_g, y, ld_y, coef, bcoef, Cp, act, slope, dwp, nslab, stream);
    const segnb_wgrad_target* tgt;
    if (int rc = take_wgrad_target(__func__, g, &tgt)) return rc;
    if (int rc = check_geom(g)) return rc;
    SEGNB_CHECK_ARG(in && gsrc && y && coef && bcoef && dwp, "NULL tensor");
    SEGNB_CHECK_ARG(segnb_conv_wgrad_bnapply_ok(g, dtype), "geometry not served (segnb_conv_wgrad_bnapply_ok)");
    SEGNB_CHECK_ARG(nslab == segnb_conv_wgrad_slabs(g, dtype), "nslab differs from segnb_conv_wgrad_slabs()");
    SEGNB_CHECK_ARG(Cp >= g->Co && ld_g >= g->Co && ld_y >= g->Co, "bad strides");
    const segnb_wgrad_bnapply bna = {gsrc, ld_g, y, ld_y, coef, bcoef, Cp, act, slope};
    segnb_try_outcome did = SEGNB_TRY_DECLINED;
    int rc = 0;
    if (segnb_knob_wgrad_c8roll()) rc = segnb_wgrad_c8roll_try(&did, g, in, nullptr, dwp, nslab, (hipStream_t)stream, tgt != nullptr, &bna);
    if (!rc && !did) rc = segnb_wgrad_s1_try(&did, g, in, nullptr, dwp, nslab, (hipStream_t)stream, false, &bna, nullptr, tgt);
    if (rc) return rc;
    return finish_wgrad(__func__, did, g, dwp, nslab, tgt, false, (hipStream_t)stream);
}

// weight gradient whose operands are recomputed on load (include/segnb_hip.h: segnb_operand_tf)
extern "C" int segnb_conv_wgrad_tf_ok(const segnb_conv_geom* g, int dtype) {
    if (g == nullptr || dtype != SEGNB_BF16 || check_geom(g) || wgrad_general_only()) return 0;
    return (segnb_wgrad_roll_applies(g) && segnb_wgrad_s1_slabs(g) > 0) ? 1 : 0;
}

extern "C" int segnb_conv_wgrad_tf(const segnb_conv_geom* g, int dtype, const void* in, const segnb_operand_tf* tf_in,
                                   const void* dout, const segnb_operand_tf* tf_dout, float* dwp, int nslab,
                                   segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_conv_wgrad_tf, g, dtype, in, tf_in, dout, tf_dout, dwp, nslab, stream);
    const segnb_wgrad_target* tgt;
    if (int rc = take_wgrad_target(__func__, g, &tgt)) return rc;
    if (int rc = check_geom(g)) return rc;
    SEGNB_CHECK_ARG(in && dout && dwp, "NULL tensor");
    SEGNB_CHECK_ARG(segnb_conv_wgrad_tf_ok(g, dtype), "geometry not served (segnb_conv_wgrad_tf_ok)");
    SEGNB_CHECK_ARG(nslab == segnb_conv_wgrad_slabs(g, dtype), "nslab differs from segnb_conv_wgrad_slabs()");
    SEGNB_CHECK_ARG(tf_in == nullptr || (tf_in->kind == SEGNB_TF_ACT && tf_in->coef != nullptr && tf_in->Cp >= g->Ci), "bad input transform");
    SEGNB_CHECK_ARG(tf_dout == nullptr || (tf_dout->kind == SEGNB_TF_BNBWD && tf_dout->coef && tf_dout->bcoef && tf_dout->y &&
                                           tf_dout->drop == nullptr && tf_dout->Cp >= g->Co), "bad dout transform");
    segnb_try_outcome did;
    if (int rc = segnb_wgrad_roll_try(&did, g, in, dout, dwp, nslab, (hipStream_t)stream, tgt != nullptr, tf_in, tf_dout)) return rc;
    return finish_wgrad(__func__, did, g, dwp, nslab, tgt, false, (hipStream_t)stream);
}
