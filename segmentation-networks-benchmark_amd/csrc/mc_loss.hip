// Multi-class segmentation losses, gfx950: FocalLossMulti / JaccardLossMulti / FocalAndJaccardLossMulti /
// NLLLAndJaccardLossMulti of the reference's lib/losses.py:105-232 and nn.NLLLoss(weight, ignore_index).
//
// One streaming pass over (logits fp32 NCHW, target int64) produces every global sum (include/segnb_mc_loss.h), a finalize
// turns them into the loss and the per-class derivatives on the device (no host sync), a second pass writes d(loss)/d(logits).
//
// Layout: consecutive lanes take consecutive pixels.  HW % 4 == 0 with 16-byte aligned tensors: a lane takes four pixels and
// reads one float4 per class (a wave reads 1 KB contiguous per class plane); otherwise one pixel per lane, scalar loads.
// Class-count buckets CB = 4 / 8 / 16 / 32 keep a pixel's logits in registers for the max / exp-sum / probability passes;
// above 32 classes (CB = 0) the passes re-read them (online max + exp-sum, then the class pass).
//
// Determinism (run to run, bit for bit): per-class sums of a tile are wave sums (a fixed butterfly) added in tile order into
// the wave's own LDS row; the four waves' rows are added in wave order; every workgroup writes ONE row of partial sums with
// plain (agent-scope) stores -- no floating-point atomics anywhere.  The rows are added in a fixed order by a two-level
// hand-over: the last workgroup of each group of MC_GROUP adds its group's rows in block order, the last group adds the
// group rows in group order.  The hand-over is the recipe of loss_reduce_kernel<true> (head_loss.hip) / ks_publish
// (fprop_dma.hip): contribution performed at the device's coherence point, drain (s_waitcnt vmcnt(0)), workgroup barrier,
// one relaxed agent-scope ticket add; the last block takes an agent-scope acquire fence and reads through coherent loads.
#include "common.h"
#include "../../include/segnb_mc_loss.h"

// (the plan recorder copies host structs passed by pointer: common.h, segnb_plan_keep)
inline const segnb_mc_loss_spec* segnb_plan_keep(const segnb_mc_loss_spec* g) {
    return g ? (const segnb_mc_loss_spec*)segnb_plan_dup(g, sizeof(*g)) : g;
}

namespace {

constexpr int MC_GRID_MAX = 1024;                        // workgroups of a reduce launch
constexpr int MC_GROUP = 16;                             // rows added by a group's last workgroup
constexpr int MC_NGROUP_MAX = MC_GRID_MAX / MC_GROUP;
constexpr int MC_TICKET_DOUBLES = 40;                    // MC_NGROUP_MAX + 1 unsigned tickets
constexpr double MC_SMOOTH = 100.0;                      // losses.py:163

static_assert(MC_NGROUP_MAX + 1 <= MC_TICKET_DOUBLES * 2, "ticket space");

__host__ __device__ inline int mc_row_len(int C) { return 3 * C + 8; }

struct McArgs {
    const float* x;
    const long long* tg;
    long long npix;
    int hw;
    int C;
    int mode;
    long long ignore;
    float gamma;
    const float* nll_w;
};

// (1 - pt)^gamma as torch's pow: exact products for the small integer exponents, pow(x, 0) = 1
__device__ __forceinline__ float mc_pow(float om, float g) {
    if (g == 0.f) return 1.f;
    if (g == 1.f) return om;
    if (g == 2.f) return om * om;
    if (g == 3.f) return om * om * om;
    return powf(om, g);
}

// focal element -(1-pt)^gamma logpt and its derivative w.r.t. logpt:  -(1-pt)^gamma + gamma (1-pt)^(gamma-1) pt logpt
// (gamma == 0: torch's pow backward masks the exponent-0 term to exactly 0)
// pt == 1 in fp32 (the winning logit leads by ~17 or more): the derivative is its limit, 0 for gamma > 0, as pix_terms of
// head_loss.hip returns it -- for gamma < 1, (1-pt)^(gamma-1) * logpt would be inf * 0, or inf * -6e-8
__device__ __forceinline__ float mc_focal(float logpt, float g) {
    const float pt = expf(logpt);
    return -mc_pow(1.f - pt, g) * logpt;
}
__device__ __forceinline__ float mc_dfocal(float logpt, float g) {
    const float pt = expf(logpt);
    const float om = 1.f - pt;
    if (g == 0.f) return -1.f;
    if (!(om > 0.f)) return 0.f;
    return -mc_pow(om, g) + g * mc_pow(om, g - 1.f) * pt * logpt;
}

template <int PPT>
struct Px {
    float v[PPT];
};
template <int PPT>
__device__ __forceinline__ Px<PPT> mc_load(const float* p) {
    Px<PPT> o;
    if constexpr (PPT == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        o.v[0] = q.x; o.v[1] = q.y; o.v[2] = q.z; o.v[3] = q.w;
    } else {
        o.v[0] = *p;
    }
    return o;
}
template <int PPT>
__device__ __forceinline__ void mc_store(float* p, const float (&v)[PPT]) {
    if constexpr (PPT == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
}
template <int PPT>
__device__ __forceinline__ void mc_load_targets(const long long* tg, long long p0, long long (&t)[PPT]) {
    if constexpr (PPT == 4) {
        const longlong2 t01 = *reinterpret_cast<const longlong2*>(tg + p0);
        const longlong2 t23 = *reinterpret_cast<const longlong2*>(tg + p0 + 2);
        t[0] = t01.x; t[1] = t01.y; t[2] = t23.x; t[3] = t23.y;
    } else {
        t[0] = tg[p0];
    }
}

// tot[col] = sum over rows 0 .. R-1 of src[row * RL + col], read through coherent loads.  When few columns leave threads idle
// the rows are split into S consecutive segments (S from R and RL only: the same association on every call of a shape), each
// summed in row order, the segments then added in segment order.  Every thread of the block calls this.
__device__ void mc_sum_rows(const double* src, int R, int RL, double* tot, double* seg) {
    int S = 1;
    while (S * 2 * RL <= 256 && S * 2 <= R) S *= 2;
    const int RS = (R + S - 1) / S;
    for (int j = threadIdx.x; j < S * RL; j += blockDim.x) {
        const int sg = j / RL, col = j - sg * RL;
        const int r1 = min(R, (sg + 1) * RS);
        double s = 0.0;
#pragma unroll 8
        for (int r = sg * RS; r < r1; ++r)
            s += __hip_atomic_load(src + (long long)r * RL + col, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (S == 1) tot[col] = s;
        else seg[j] = s;
    }
    __syncthreads();
    if (S > 1) {
        for (int col = threadIdx.x; col < RL; col += blockDim.x) {
            double s = seg[col];
            for (int sg = 1; sg < S; ++sg) s += seg[sg * RL + col];
            tot[col] = s;
        }
    }
    __syncthreads();
}

// publish row[0 .. RL) (LDS) to dst with agent-scope stores, drain, then draw a ticket; -> true in the block that drew the
// last one of `count` (it has taken the acquire fence).  Every thread of the block calls this.
__device__ bool mc_publish(const double* row, double* dst, int RL, unsigned* ticket, unsigned count) {
    for (int i = threadIdx.x; i < RL; i += blockDim.x)
        __hip_atomic_store(dst + i, row[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    __shared__ int last;
    if (threadIdx.x == 0) {
        const unsigned tk = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = tk == count - 1 ? 1 : 0;
        if (last) {
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next launch
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    return last != 0;
}

// the global sums S[3C + 8] -> fin[8 + 3C]; lw: LDS scratch of C doubles.  Every thread of the block calls this.
__device__ void mc_finalize(const double* S, const segnb_mc_loss_spec& sp, float* __restrict__ fin, double* lw) {
    const int C = sp.C;
    const double jscale = sp.reduce ? (double)sp.w_jaccard / (double)sp.norm : 1.0;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const double I = S[c], P = S[C + c], T = S[2 * C + c];
        const double w = sp.jac_weight != nullptr ? (double)sp.jac_weight[c] : 1.0;
        double L = 0.0, gI = 0.0, gP = 0.0;
        if (T > 0.0) {        // a class absent from the masked targets: loss 0, no gradient (losses.py:176-177)
            const double D = P + T - I + MC_SMOOTH;
            L = 1.0 - (I + MC_SMOOTH) / D;
            gI = -(P + T + 2.0 * MC_SMOOTH) / (D * D);
            gP = (I + MC_SMOOTH) / (D * D);
        }
        lw[c] = w * L;
        fin[8 + c] = (float)(w * L);
        fin[8 + C + c] = (float)(jscale * w * gI);
        fin[8 + 2 * C + c] = (float)(jscale * w * gP);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double jac = 0.0;
        for (int c = 0; c < C; ++c) jac += lw[c];
        const double nall = S[3 * C + 4], W = S[3 * C + 2];
        const double focal = sp.focal_mean ? S[3 * C] / nall : S[3 * C];
        const double nll = S[3 * C + 1] / W;
        double loss = (double)sp.w_jaccard * jac;
        if (sp.w_focal != 0.f) loss += (double)sp.w_focal * focal;
        if (sp.w_nll != 0.f) loss += (double)sp.w_nll * nll;
        fin[0] = (float)(loss / (double)sp.norm);
        fin[1] = (float)((double)sp.w_focal / (double)sp.norm / (sp.focal_mean ? nall : 1.0));
        fin[2] = sp.w_nll != 0.f ? (float)((double)sp.w_nll / (double)sp.norm / W) : 0.f;
        fin[3] = (float)S[3 * C + 3];
        fin[4] = (float)nall;
        fin[5] = (float)S[3 * C + 5];
        fin[6] = (float)focal;
        fin[7] = (float)nll;
    }
    __syncthreads();
}

// reduce pass.  FIN: the last workgroup finalizes into fin; otherwise it writes the sums to sums_out.
template <int CB, int PPT, bool FIN>
__global__ __launch_bounds__(256) void mc_reduce_kernel(McArgs a, double* __restrict__ work, double* __restrict__ sums_out,
                                                        segnb_mc_loss_spec sp, float* __restrict__ fin) {
    extern __shared__ double sacc[];            // [4 waves][I | P | T][C], then the block's row [3C + 8]; later the totals
    __shared__ double sseg[256];
    __shared__ double ssc[4][6];
    const int C = a.C, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 12 * C; i += 256) sacc[i] = 0.0;
    __syncthreads();
    double* const my = sacc + wave * 3 * C;
    float focal = 0.f, nll = 0.f, wsum = 0.f;
    int nvalid = 0, nbad = 0;
    const long long units = a.npix / PPT;
    // (the trip count is uniform over the block: the wave sums below need every lane)
    for (long long base = (long long)blockIdx.x * 256; base < units; base += (long long)gridDim.x * 256) {
        const long long u = base + tid;
        const bool act = u < units;
        const long long p0 = (act ? u : 0) * PPT;
        const long long n = p0 / a.hw;
        const int r = (int)(p0 - n * a.hw);
        const float* xp = a.x + n * C * (long long)a.hw + r;
        long long tv[PPT];
        mc_load_targets<PPT>(a.tg, p0, tv);
        int ti[PPT];
        bool valid[PPT];
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            valid[k] = act && tv[k] != a.ignore;
            const bool inr = valid[k] && tv[k] >= 0 && tv[k] < C;
            ti[k] = inr ? (int)tv[k] : -1;            // a bad label is never an index
            nvalid += valid[k] ? 1 : 0;
            nbad += (valid[k] && !inr) ? 1 : 0;
        }
        float mx[PPT], sh[PPT], logpt[PPT];      // the pixel's max logit and log(sum exp(x - max)): logp = (x - max) - log sum
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            mx[k] = 0.f;
            sh[k] = 0.f;
            logpt[k] = 0.f;
        }
        // one class: its p for the lane's pixels, the tile's I / P / T sums of it into the wave's LDS row
        auto klass = [&](int c, const Px<PPT>& xv) {
            float Pv = 0.f, Iv = 0.f, Tv = 0.f;
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                const float lp = (xv.v[k] - mx[k]) - sh[k];
                const float p = expf(lp);
                if (valid[k]) Pv += p;
                if (c == ti[k]) {
                    Iv += p;
                    Tv += 1.f;
                    logpt[k] = lp;
                }
            }
            Pv = wave_sum(Pv);
            Iv = wave_sum(Iv);
            Tv = wave_sum(Tv);
            if (lane == 0) {
                my[c] += (double)Iv;
                my[C + c] += (double)Pv;
                my[2 * C + c] += (double)Tv;
            }
        };
        if constexpr (CB > 0) {
            Px<PPT> xr[CB];
#pragma unroll
            for (int c = 0; c < CB; ++c)
                if (c < C) xr[c] = mc_load<PPT>(xp + (long long)c * a.hw);
            if (a.mode == 0) {
#pragma unroll
                for (int k = 0; k < PPT; ++k) {
                    float m = xr[0].v[k];
#pragma unroll
                    for (int c = 1; c < CB; ++c)
                        if (c < C) m = fmaxf(m, xr[c].v[k]);
                    float s = 0.f;
#pragma unroll
                    for (int c = 0; c < CB; ++c)
                        if (c < C) s += expf(xr[c].v[k] - m);
                    mx[k] = m;
                    sh[k] = logf(s);
                }
            }
#pragma unroll
            for (int c = 0; c < CB; ++c)
                if (c < C) klass(c, xr[c]);
        } else {
            if (a.mode == 0) {
                float m[PPT], s[PPT];
                const Px<PPT> x0 = mc_load<PPT>(xp);
#pragma unroll
                for (int k = 0; k < PPT; ++k) {
                    m[k] = x0.v[k];
                    s[k] = 1.f;
                }
                for (int c = 1; c < C; ++c) {
                    const Px<PPT> xv = mc_load<PPT>(xp + (long long)c * a.hw);
#pragma unroll
                    for (int k = 0; k < PPT; ++k) {
                        const float nm = fmaxf(m[k], xv.v[k]);
                        s[k] = s[k] * expf(m[k] - nm) + expf(xv.v[k] - nm);
                        m[k] = nm;
                    }
                }
#pragma unroll
                for (int k = 0; k < PPT; ++k) {
                    mx[k] = m[k];
                    sh[k] = logf(s[k]);
                }
            }
            for (int c = 0; c < C; ++c) klass(c, mc_load<PPT>(xp + (long long)c * a.hw));
        }
#pragma unroll
        for (int k = 0; k < PPT; ++k)
            if (ti[k] >= 0) {
                focal += mc_focal(logpt[k], a.gamma);
                const float w = a.nll_w != nullptr ? a.nll_w[ti[k]] : 1.f;
                nll -= w * logpt[k];
                wsum += w;
            }
    }
    {
        const double v[6] = {(double)focal, (double)nll, (double)wsum, (double)nvalid, 0.0, (double)nbad};
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const double s = wave_sum(v[q]);
            if (lane == 0) ssc[wave][q] = s;
        }
    }
    __syncthreads();
    // this block's row, in LDS behind the wave slices
    const int RL = mc_row_len(C);
    double* const row = sacc + 12 * C;
    for (int i = tid; i < RL; i += 256) {
        double val;
        if (i < 3 * C) {
            val = ((sacc[i] + sacc[3 * C + i]) + sacc[6 * C + i]) + sacc[9 * C + i];
        } else {
            const int q = i - 3 * C;
            val = q < 6 ? ((ssc[0][q] + ssc[1][q]) + ssc[2][q]) + ssc[3][q] : 0.0;
            if (q == 4) val = blockIdx.x == 0 ? (double)a.npix : 0.0;
        }
        row[i] = val;
    }
    __syncthreads();
    double* const rows = work;
    double* const grows = work + (long long)MC_GRID_MAX * RL;
    unsigned* const tickets = reinterpret_cast<unsigned*>(work + (long long)(MC_GRID_MAX + MC_NGROUP_MAX) * RL);
    const int g = blockIdx.x / MC_GROUP;
    const int ng = (gridDim.x + MC_GROUP - 1) / MC_GROUP;
    const int gsz = min(MC_GROUP, (int)gridDim.x - g * MC_GROUP);
    if (!mc_publish(row, rows + (long long)blockIdx.x * RL, RL, tickets + g, (unsigned)gsz)) return;
    // the last block of its group: the group's rows in block order
    mc_sum_rows(rows + (long long)g * MC_GROUP * RL, gsz, RL, sacc, sseg);
    if (!mc_publish(sacc, grows + (long long)g * RL, RL, tickets + MC_NGROUP_MAX, (unsigned)ng)) return;
    // the last group: the group rows in group order
    mc_sum_rows(grows, ng, RL, sacc, sseg);
    if constexpr (FIN) {
        mc_finalize(sacc, sp, fin, sacc + RL);
    } else {
        for (int i = tid; i < RL; i += 256) sums_out[i] = sacc[i];
    }
}

__global__ __launch_bounds__(256) void mc_finalize_kernel(const double* __restrict__ sums, segnb_mc_loss_spec sp,
                                                          float* __restrict__ fin) {
    extern __shared__ double sfin[];              // [RL] sums, [C] scratch
    const int RL = mc_row_len(sp.C);
    for (int i = threadIdx.x; i < RL; i += blockDim.x) sfin[i] = sums[i];
    __syncthreads();
    mc_finalize(sfin, sp, fin, sfin + RL);
}

// backward pass: dz_j = a (d_jt - p_j) + p_j (g_j - sum_c p_c g_c)   (mode 0; mode 1: a d_jt + p_j g_j)
//   a   = d(loss)/d(logp_t): focal and NLL terms (0 for ignored pixels and bad labels)
//   g_c = d(loss)/d(p_c): the Jaccard term, dP_c + dI_c [t == c] inside the mask, 0 outside
template <int CB, int PPT>
__global__ __launch_bounds__(256) void mc_bwd_kernel(McArgs a, const float* __restrict__ fin, const float* __restrict__ gout,
                                                     int gvec, float* __restrict__ dx) {
    extern __shared__ float scoef[];              // [C] dI coefficients, [C] dP coefficients (upstream gradient folded in)
    const int C = a.C;
    const float g0 = gout != nullptr ? gout[0] : 1.f;
    for (int c = threadIdx.x; c < C; c += 256) {
        const float gc = gvec ? gout[c] : g0;
        scoef[c] = gc * fin[8 + C + c];
        scoef[C + c] = gc * fin[8 + 2 * C + c];
    }
    __syncthreads();
    const float cf = g0 * fin[1], cn = g0 * fin[2];
    const float* const cI = scoef;
    const float* const cP = scoef + C;
    const long long units = a.npix / PPT;
    for (long long u = (long long)blockIdx.x * 256 + threadIdx.x; u < units; u += (long long)gridDim.x * 256) {
        const long long p0 = u * PPT;
        const long long n = p0 / a.hw;
        const int r = (int)(p0 - n * a.hw);
        const long long off = n * C * (long long)a.hw + r;
        const float* xp = a.x + off;
        float* dp = dx + off;
        long long tv[PPT];
        mc_load_targets<PPT>(a.tg, p0, tv);
        int ti[PPT];
        bool valid[PPT];
        float mx[PPT], sh[PPT], logpt[PPT], S[PPT], av[PPT];
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            valid[k] = tv[k] != a.ignore;
            ti[k] = (valid[k] && tv[k] >= 0 && tv[k] < C) ? (int)tv[k] : -1;
            mx[k] = 0.f;
            sh[k] = 0.f;
            logpt[k] = 0.f;
            S[k] = 0.f;
        }
        // p_c of the lane's pixels (overwrites xv), the running sum_c p_c g_c and logp_t
        auto probs = [&](int c, Px<PPT>& xv) {
            const float cp = cP[c], ci = cI[c];
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                const float lp = (xv.v[k] - mx[k]) - sh[k];
                const float p = expf(lp);
                xv.v[k] = p;
                if (valid[k]) S[k] += p * (c == ti[k] ? cp + ci : cp);
                if (c == ti[k]) logpt[k] = lp;
            }
        };
        auto coef = [&]() {
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                float ak = 0.f;
                if (ti[k] >= 0) {
                    ak = cf * mc_dfocal(logpt[k], a.gamma);
                    if (cn != 0.f) ak -= cn * (a.nll_w != nullptr ? a.nll_w[ti[k]] : 1.f);
                }
                av[k] = ak;
            }
        };
        auto write = [&](int c, const Px<PPT>& pv) {
            const float cp = cP[c], ci = cI[c];
            float o[PPT];
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                const float p = pv.v[k];
                const float gc = valid[k] ? (c == ti[k] ? cp + ci : cp) : 0.f;
                const float d = c == ti[k] ? av[k] : 0.f;
                o[k] = a.mode == 0 ? (d - av[k] * p) + p * (gc - S[k]) : d + p * gc;
            }
            mc_store<PPT>(dp + (long long)c * a.hw, o);
        };
        if constexpr (CB > 0) {
            Px<PPT> xr[CB];
#pragma unroll
            for (int c = 0; c < CB; ++c)
                if (c < C) xr[c] = mc_load<PPT>(xp + (long long)c * a.hw);
            if (a.mode == 0) {
#pragma unroll
                for (int k = 0; k < PPT; ++k) {
                    float m = xr[0].v[k];
#pragma unroll
                    for (int c = 1; c < CB; ++c)
                        if (c < C) m = fmaxf(m, xr[c].v[k]);
                    float s = 0.f;
#pragma unroll
                    for (int c = 0; c < CB; ++c)
                        if (c < C) s += expf(xr[c].v[k] - m);
                    mx[k] = m;
                    sh[k] = logf(s);
                }
            }
#pragma unroll
            for (int c = 0; c < CB; ++c)
                if (c < C) probs(c, xr[c]);
            coef();
#pragma unroll
            for (int c = 0; c < CB; ++c)
                if (c < C) write(c, xr[c]);
        } else {
            if (a.mode == 0) {
                float m[PPT], s[PPT];
                const Px<PPT> x0 = mc_load<PPT>(xp);
#pragma unroll
                for (int k = 0; k < PPT; ++k) {
                    m[k] = x0.v[k];
                    s[k] = 1.f;
                }
                for (int c = 1; c < C; ++c) {
                    const Px<PPT> xv = mc_load<PPT>(xp + (long long)c * a.hw);
#pragma unroll
                    for (int k = 0; k < PPT; ++k) {
                        const float nm = fmaxf(m[k], xv.v[k]);
                        s[k] = s[k] * expf(m[k] - nm) + expf(xv.v[k] - nm);
                        m[k] = nm;
                    }
                }
#pragma unroll
                for (int k = 0; k < PPT; ++k) {
                    mx[k] = m[k];
                    sh[k] = logf(s[k]);
                }
            }
            for (int c = 0; c < C; ++c) {
                Px<PPT> xv = mc_load<PPT>(xp + (long long)c * a.hw);
                probs(c, xv);
            }
            coef();
            for (int c = 0; c < C; ++c) {
                Px<PPT> xv = mc_load<PPT>(xp + (long long)c * a.hw);
#pragma unroll
                for (int k = 0; k < PPT; ++k) xv.v[k] = expf((xv.v[k] - mx[k]) - sh[k]);
                write(c, xv);
            }
        }
    }
}

int mc_check(const float* logits, const long long* target, int N, int HW, const segnb_mc_loss_spec* spec) {
    SEGNB_CHECK_ARG(logits && target && spec, "NULL tensor");
    SEGNB_CHECK_ARG(spec->C >= 1 && spec->C <= SEGNB_MC_MAX_CLASSES, "1 <= C <= 256");
    SEGNB_CHECK_ARG(N > 0 && HW > 0, "bad shape");
    SEGNB_CHECK_ARG(spec->mode == 0 || spec->mode == 1, "mode 0 (logits) or 1 (log-probabilities)");
    SEGNB_CHECK_ARG(spec->norm != 0.f, "loss norm must be non-zero");
    SEGNB_CHECK_ARG(spec->reduce || (spec->w_focal == 0.f && spec->w_nll == 0.f), "reduce=0 is the Jaccard vector alone");
    return 0;
}

McArgs mc_args(const float* logits, const long long* target, int N, int HW, const segnb_mc_loss_spec* spec) {
    return McArgs{logits, target, (long long)N * HW, HW, spec->C, spec->mode, spec->ignore_index, spec->gamma,
                  spec->nll_weight};
}

// the class-count bucket x the pixels-per-lane form
#define SEGNB_MC_DISPATCH(LAUNCH)                   \
    do {                                            \
        if (vec) {                                  \
            if (C <= 4) LAUNCH(4, 4);               \
            else if (C <= 8) LAUNCH(8, 4);          \
            else if (C <= 16) LAUNCH(16, 4);        \
            else if (C <= 32) LAUNCH(32, 4);        \
            else LAUNCH(0, 4);                      \
        } else {                                    \
            if (C <= 4) LAUNCH(4, 1);               \
            else if (C <= 8) LAUNCH(8, 1);          \
            else if (C <= 16) LAUNCH(16, 1);        \
            else if (C <= 32) LAUNCH(32, 1);        \
            else LAUNCH(0, 1);                      \
        }                                           \
    } while (0)

template <bool FIN>
int mc_reduce_launch(const float* logits, const long long* target, int N, int HW, const segnb_mc_loss_spec* spec,
                     double* work, double* sums, float* fin, hipStream_t stream) {
    const McArgs a = mc_args(logits, target, N, HW, spec);
    const int C = spec->C;
    const int vec = HW % 4 == 0 && (((uintptr_t)logits | (uintptr_t)target) & 15) == 0;
    const long long units = a.npix / (vec ? 4 : 1);
    int grid = ceil_div(units, 256);
    if (grid > MC_GRID_MAX) grid = MC_GRID_MAX;
    const size_t smem = (size_t)(12 * C + mc_row_len(C)) * sizeof(double);
#define SEGNB_MC_REDUCE(CB_, PPT_)                                                                                      \
    hipLaunchKernelGGL((mc_reduce_kernel<CB_, PPT_, FIN>), dim3(grid), dim3(256), smem, stream, a, work, sums, *spec, fin)
    SEGNB_MC_DISPATCH(SEGNB_MC_REDUCE);
#undef SEGNB_MC_REDUCE
    return 0;
}

}  // namespace

extern "C" int segnb_mc_loss_work_doubles(int C) {
    if (C < 1 || C > SEGNB_MC_MAX_CLASSES) return 0;
    return (MC_GRID_MAX + MC_NGROUP_MAX) * mc_row_len(C) + MC_TICKET_DOUBLES;
}

extern "C" int segnb_mc_loss_reduce(const float* logits, const long long* target, int N, int HW, const segnb_mc_loss_spec* spec,
                                    double* work, double* sums, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_mc_loss_reduce, logits, target, N, HW, spec, work, sums, stream);
    if (int rc = mc_check(logits, target, N, HW, spec)) return rc;
    SEGNB_CHECK_ARG(work && sums, "NULL work / sums");
    mc_reduce_launch<false>(logits, target, N, HW, spec, work, sums, nullptr, (hipStream_t)stream);
    SEGNB_LAUNCH_CHECK();
    return 0;
}

extern "C" int segnb_mc_loss_finalize(const double* sums, const segnb_mc_loss_spec* spec, float* fin, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_mc_loss_finalize, sums, spec, fin, stream);
    SEGNB_CHECK_ARG(sums && spec && fin, "NULL argument");
    SEGNB_CHECK_ARG(spec->C >= 1 && spec->C <= SEGNB_MC_MAX_CLASSES, "1 <= C <= 256");
    SEGNB_CHECK_ARG(spec->norm != 0.f, "loss norm must be non-zero");
    const size_t smem = (size_t)(mc_row_len(spec->C) + spec->C) * sizeof(double);
    hipLaunchKernelGGL(mc_finalize_kernel, dim3(1), dim3(256), smem, (hipStream_t)stream, sums, *spec, fin);
    SEGNB_LAUNCH_CHECK();
    return 0;
}

extern "C" int segnb_mc_loss_reduce_finalize(const float* logits, const long long* target, int N, int HW,
                                             const segnb_mc_loss_spec* spec, double* work, float* fin, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_mc_loss_reduce_finalize, logits, target, N, HW, spec, work, fin, stream);
    if (int rc = mc_check(logits, target, N, HW, spec)) return rc;
    SEGNB_CHECK_ARG(work && fin, "NULL work / fin");
    mc_reduce_launch<true>(logits, target, N, HW, spec, work, nullptr, fin, (hipStream_t)stream);
    SEGNB_LAUNCH_CHECK();
    return 0;
}

extern "C" int segnb_mc_loss_bwd(const float* logits, const long long* target, int N, int HW, const segnb_mc_loss_spec* spec,
                                 const float* fin, const float* grad_out, float* dlogits, segnb_stream_t stream) {
    SEGNB_PLAN_RECORD(segnb_mc_loss_bwd, logits, target, N, HW, spec, fin, grad_out, dlogits, stream);
    if (int rc = mc_check(logits, target, N, HW, spec)) return rc;
    SEGNB_CHECK_ARG(fin && dlogits, "NULL fin / dlogits");
    SEGNB_CHECK_ARG(spec->reduce || grad_out, "reduce=0 needs the [C] upstream gradient");
    const McArgs a = mc_args(logits, target, N, HW, spec);
    const int C = spec->C;
    const int vec = HW % 4 == 0 && (((uintptr_t)logits | (uintptr_t)target | (uintptr_t)dlogits) & 15) == 0;
    const long long units = a.npix / (vec ? 4 : 1);
    int grid = ceil_div(units, 256);
    if (grid > 4096) grid = 4096;
    const size_t smem = (size_t)2 * C * sizeof(float);
    const int gvec = spec->reduce ? 0 : 1;
    hipStream_t st = (hipStream_t)stream;
#define SEGNB_MC_BWD(CB_, PPT_) \
    hipLaunchKernelGGL((mc_bwd_kernel<CB_, PPT_>), dim3(grid), dim3(256), smem, st, a, fin, grad_out, gvec, dlogits)
    SEGNB_MC_DISPATCH(SEGNB_MC_BWD);
#undef SEGNB_MC_BWD
    SEGNB_LAUNCH_CHECK();
    return 0;
}
