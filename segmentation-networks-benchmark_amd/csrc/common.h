// Shared device/host helpers for libsegnb_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/segnb_hip.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;

struct bf16_t {
    unsigned short bits;
};

// ------------------------------------------------------------------------------------------------
// error plumbing (never throw across the ABI)
// ------------------------------------------------------------------------------------------------
void segnb_set_error(const char* fmt, ...);

// (the _AS forms: a helper shared by several entry points reports under the name the caller gives it)
#define SEGNB_CHECK_ARG_AS(who, cond, msg)                           \
    do {                                                             \
        if (!(cond)) {                                               \
            segnb_set_error("%s: bad argument: %s", who, msg);       \
            return SEGNB_E_BADARG;                                   \
        }                                                            \
    } while (0)
#define SEGNB_CHECK_ARG(cond, msg) SEGNB_CHECK_ARG_AS(__func__, cond, msg)

// A launch that can carry the completion event of an armed cross-stream fork (segnb_stream_fork_arm / _commit, runtime.hip): the
// event rides on the kernel's own dispatch packet (hipExtLaunchKernelGGL stopEvent) instead of a marker packet of its own between
// two dependent kernels of the queue -- tools/fork_cost.hip: +1.7 us instead of +5.5 us per fork on MI355X.
hipEvent_t segnb_take_armed_event(hipStream_t stream);
#define SEGNB_LAUNCH_FORKABLE(kernel, grid, block, shmem, stream, ...)                                          \
    do {                                                                                                        \
        hipEvent_t seg_ev_ = segnb_take_armed_event(stream);                                                    \
        if (seg_ev_ != nullptr)                                                                                 \
            hipExtLaunchKernelGGL(kernel, grid, block, shmem, stream, nullptr, seg_ev_, 0, __VA_ARGS__);        \
        else                                                                                                    \
            hipLaunchKernelGGL(kernel, grid, block, shmem, stream, __VA_ARGS__);                                \
    } while (0)

#define SEGNB_LAUNCH_CHECK_AS(who)                                                            \
    do {                                                                                      \
        hipError_t e__ = hipGetLastError();                                                   \
        if (e__ != hipSuccess) {                                                              \
            segnb_set_error("%s: launch failed: %s", who, hipGetErrorString(e__));            \
            return (int)e__;                                                                  \
        }                                                                                     \
    } while (0)
#define SEGNB_LAUNCH_CHECK() SEGNB_LAUNCH_CHECK_AS(__func__)

// ------------------------------------------------------------------------------------------------
// launch plans (runtime.hip: segnb_plan_begin / _end / _run): while a plan is being recorded on this thread every
// top-level C-ABI call appends itself -- function pointer + its arguments, host structs copied into the plan -- and then
// executes as usual; segnb_plan_run replays the list from C (the Python launcher needs 10-14 us per launch).
// ------------------------------------------------------------------------------------------------
#include <functional>
#include <type_traits>
#include <tuple>
bool segnb_plan_recording();
void segnb_plan_push(std::function<int()> op, const char* name);
const void* segnb_plan_dup(const void* p, size_t bytes);
struct SegnbPlanScope {          // nested entry points (conv_wgrad_partial -> conv_wgrad) record once, at the top
    bool top;
    SegnbPlanScope();
    ~SegnbPlanScope();
};
template <class T>
inline T segnb_plan_keep(T v) {
    // (a HOST struct passed by pointer is copied into the plan by an overload below: without one the recorded call would replay
    // with a dangling pointer -- the compiler refuses the entry point instead)
    static_assert(!(std::is_pointer<T>::value && std::is_class<typename std::remove_pointer<T>::type>::value),
                  "segnb_plan_keep: add an overload that copies this struct into the plan");
    return v;
}
inline const segnb_conv_geom* segnb_plan_keep(const segnb_conv_geom* g) {
    return g ? (const segnb_conv_geom*)segnb_plan_dup(g, sizeof(*g)) : g;
}
inline const segnb_loss_spec* segnb_plan_keep(const segnb_loss_spec* g) {
    return g ? (const segnb_loss_spec*)segnb_plan_dup(g, sizeof(*g)) : g;
}
inline const segnb_bn_reduce_epilogue* segnb_plan_keep(const segnb_bn_reduce_epilogue* g) {
    return g ? (const segnb_bn_reduce_epilogue*)segnb_plan_dup(g, sizeof(*g)) : g;
}
inline const segnb_bn_apply_epilogue* segnb_plan_keep(const segnb_bn_apply_epilogue* g) {
    return g ? (const segnb_bn_apply_epilogue*)segnb_plan_dup(g, sizeof(*g)) : g;
}
inline const segnb_upcat_src* segnb_plan_keep(const segnb_upcat_src* g) {
    return g ? (const segnb_upcat_src*)segnb_plan_dup(g, sizeof(*g)) : g;
}
inline const segnb_operand_tf* segnb_plan_keep(const segnb_operand_tf* g) {
    return g ? (const segnb_operand_tf*)segnb_plan_dup(g, sizeof(*g)) : g;
}
inline const segnb_wgrad_target* segnb_plan_keep(const segnb_wgrad_target* g) {
    return g ? (const segnb_wgrad_target*)segnb_plan_dup(g, sizeof(*g)) : g;
}
inline const segnb_act_epilogue* segnb_plan_keep(const segnb_act_epilogue* g) {
    return g ? (const segnb_act_epilogue*)segnb_plan_dup(g, sizeof(*g)) : g;
}
template <class... P, class... A>
inline void segnb_plan_record_call(const char* name, int (*fn)(P...), A... args) {
    static_assert(sizeof...(P) == sizeof...(A), "argument count");
    std::tuple<P...> kept(segnb_plan_keep((P)args)...);
    segnb_plan_push([fn, kept]() { return std::apply(fn, kept); }, name);
}
// first statement of a recordable extern "C" entry point (entry points that take HOST arrays -- tap offsets, mean / std --
// are not recordable: SEGNB_PLAN_REFUSE marks the plan being recorded as unusable)
extern int g_segnb_census_on;          // segnb_tune("call_census"): count the top-level entry points by name (segnb_debug_census)
void segnb_census(const char* name);
#define SEGNB_PLAN_RECORD(fn, ...)                                                           \
    SegnbPlanScope plan_scope__;                                                             \
    if (plan_scope__.top && g_segnb_census_on) segnb_census(#fn);                            \
    if (plan_scope__.top && segnb_plan_recording()) segnb_plan_record_call(#fn, fn, __VA_ARGS__)
void segnb_plan_refuse(const char* why);
#define SEGNB_PLAN_REFUSE(why)                                         \
    SegnbPlanScope plan_scope__;                                       \
    if (plan_scope__.top && g_segnb_census_on) segnb_census(__func__); \
    if (plan_scope__.top && segnb_plan_recording()) segnb_plan_refuse(why)

int segnb_num_cus();
bool segnb_fprop_general_forced();      // conv_igemm.hip: SEGNB_FPROP_GENERAL is set (A/B testing; read once per process)
int segnb_knob_fprop_dma();       // runtime.hip: segnb_tune() knobs
int segnb_knob_fprop_dma_cfg();
int segnb_knob_fprop_dma_dbg();
int segnb_knob_fprop_dma_epi();   // -1 default, 0 / 1: store rows of conv_fprop_ws_kernel on taps chosen at run time / on peeled taps
int segnb_knob_fprop_nostats();   // 1: launches without statistics run the statistics-free instantiation of conv_fprop_ws_kernel
int segnb_knob_bnreduce_fused();  // 1: segnb_conv_fprop_bnreduce_ok may say yes
int segnb_knob_fprop_deepk();     // 1: conv_fprop_deepk_kernel serves the shapes it applies to
int segnb_knob_fprop_thin();      // 1: conv_thin_kernel (fprop_thin.hip) serves <= 16 -> >= 48 channel stride-1 3x3 launches
// The segnb_*_try kernel selectors below report two things that never share a value: their int return is the error status
// alone -- 0, or exactly what the calling entry point returns (hipError_t > 0, SEGNB_E_* < 0) -- and *did says what they did.
enum segnb_try_outcome {
    SEGNB_TRY_DECLINED = 0,     // not this kernel's geometry / operands: nothing launched, the caller tries the next one
    SEGNB_TRY_LAUNCHED,         // launched
    SEGNB_TRY_DELIVERED,        // launched, and the kernel wrote the armed segnb_wgrad_target itself (nothing left to deliver)
};
// What a launch_* / dispatch_* helper inside a try returns when its kernel does not serve the arguments after all (no hipError_t,
// no SEGNB_E_*).  It never leaves a try: segnb_try_launched below is its only reader, and every such result goes through it.
constexpr int SEGNB_LAUNCH_DECLINED = INT_MIN;
// the tail of a try whose launch helper returned rc (0, SEGNB_LAUNCH_DECLINED or an error): launched unless it declined or failed
inline int segnb_try_launched(segnb_try_outcome* did, int rc) {
    if (rc == SEGNB_LAUNCH_DECLINED) {
        *did = SEGNB_TRY_DECLINED;
        return 0;
    }
    if (rc == 0) *did = SEGNB_TRY_LAUNCHED;
    return rc;
}
#define SEGNB_HOST_INLINE static inline __attribute__((always_inline))
// More than 64 KB of dynamic LDS has to be asked for once per kernel: every kernel a launcher may start, in one call that stops at
// the first failure, reports it once and returns the status.  A launcher keeps the result:
//     static const int attr_rc = segnb_opt_in_lds("fprop_rw", C::SMEM, k0, k1, k2);
template <class... K>
int segnb_opt_in_lds(const char* who, int bytes, K... kernels) {
    hipError_t e = hipSuccess;
    (void)(... && ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernels), hipFuncAttributeMaxDynamicSharedMemorySize,
                                            bytes)) == hipSuccess));
    if (e != hipSuccess) segnb_set_error("%s hipFuncSetAttribute(%d bytes): %s", who, bytes, hipGetErrorString(e));
    return (int)e;
}
// The extent in bytes of an NHWC tensor of npix pixels, ld elements apart, up to the C channels of its last pixel, and the one
// comparison with what a buffer descriptor (32-bit offsets, 2 GiB) addresses; *out (may be NULL) receives the extent.
SEGNB_HOST_INLINE long long segnb_nhwc_bytes(long long npix, int ld, int C, int esz) { return ((npix - 1) * ld + C) * esz; }
SEGNB_HOST_INLINE bool segnb_fits_desc(long long bytes, unsigned* out = nullptr) {
    if (out != nullptr) *out = (unsigned)bytes;
    return bytes < (1ll << 31);
}
// after a try of the plain forward / weight-gradient cascades (segnb_conv_fprop, _act, segnb_conv_wgrad): remember the first
// selector that launched.  With the call census on, the cascade counts it -- or "kernel:fprop_general" / "kernel:wgrad_general"
// when every selector declined -- beside the entry points, so a test can tell which kernel served a geometry (tests/test_dilation_gpu.py)
inline void segnb_kernel_took(segnb_try_outcome did, const char** served, const char* name) {
    if (did != SEGNB_TRY_DECLINED && *served == nullptr) *served = name;
}
// The fused epilogues of a try into its kernel's argument struct (FdArgs, RollArgs, ThinArgs, C8Args: the same field names).
// take_bn_reduce: false -- the try declines -- when y's extent [N][Ho][Wo][ld_y] passes the 2 GiB of a buffer descriptor.
// (forced inline: left to the inliner the tries of fprop_dma.hip, fprop_rw.hip and fprop_roll.hip called it)
template <class Args>
__attribute__((always_inline)) inline bool take_bn_reduce(Args& a, const segnb_conv_geom* g, const segnb_bn_reduce_epilogue* bn) {
    const long long yb = segnb_nhwc_bytes((long long)g->N * g->Ho * g->Wo, bn->ld_y, g->Co, 2);
    if (!segnb_fits_desc(yb)) return false;
    a.bn_y = (const bf16_t*)bn->y;
    a.bn_y_bytes = (unsigned)yb;
    a.bn_ld = bn->ld_y;
    a.bn_coef = bn->coef;
    a.bn_sums = bn->sums;
    a.bn_act = bn->act;
    a.bn_slope = bn->slope;
    return true;
}
// ep NULL: no affine + activation epilogue on this launch (ep_act < 0)
template <class Args>
__attribute__((always_inline)) inline void take_act_epilogue(Args& a, const segnb_act_epilogue* ep) {
    a.ep_act = ep != nullptr ? ep->act : -1;
    a.ep_coef = ep != nullptr ? ep->coef : nullptr;
    a.ep_slope = ep != nullptr ? ep->slope : 0.f;
}
// fprop_thin.hip; bn: the BatchNorm-backward reduction epilogue of segnb_conv_fprop_bnreduce or NULL
int segnb_fprop_thin_try(segnb_try_outcome* did, const segnb_conv_geom* g, const void* in, const void* wpacked, void* out,
                         hipStream_t stream, const segnb_bn_reduce_epilogue* bn);
int segnb_fprop_thin_ok(const segnb_conv_geom* g);
int segnb_knob_fprop_upd();       // 1: 4x4 / stride-2 gathers (ntaps 16, in_step 2) on the plane-gather form of conv_fprop_ws_kernel
int segnb_knob_fprop_drop();      // 1: segnb_conv_fprop_drop_ok may say yes
int segnb_knob_fprop_mask();      // 1: conv_fprop_ws_kernel serves activation-mask data gradients (segnb_conv_fprop_bnreduce, coef NULL)
int segnb_fprop_dma_actmask_ok(const segnb_conv_geom* g);
int segnb_fprop_roll_actmask_ok(const segnb_conv_geom* g);     // fprop_roll.hip: conv_roll_kernel (EPI = 3) serves g      // fprop_dma.hip: the MASK instantiation serves g
int segnb_knob_fprop_rw();
int segnb_knob_fprop_ksplit();   // conv_fprop_ws_kernel split K: 0 off, 1 automatic (default), 2 / 4 forced where it applies
// head backward's per-(device, stream) partial-sum scratch and its fixed-order finish launch (head_loss.hip)
float* segnb_head_scratch(size_t bytes, hipStream_t stream);
void segnb_head_bwd_finish(const float* part, int gx, int gy, int K, int C, int CT, float* dw, float* db, hipStream_t stream);
int segnb_knob_pack_blocks();    // persistent blocks of segnb_pack_weight_multi (0: one block per tile)
int segnb_knob_fprop_roll();     // 0: off, 1: conv_roll_kernel with 16-column strips, 2: 32-column strips (segnb_tune "fprop_roll")
int segnb_knob_wg_cu_pct();      // segnb_tune "wg_cu_pct": 0 = default share of the CUs for the 64x64-tile weight gradients
int segnb_knob_conv_cus();        // CUs the persistent fprop / dgrad kernels size their grids for (segnb_tune "conv_cu_pct")
int segnb_fprop_dma_read_stamps(unsigned long long* host_dst);
// fast path of segnb_conv_fprop (fprop_s1.hip)
// (drop / ld_drop / stats_ld: the Dropout2d multipliers and the statistics row stride of segnb_conv_fprop_drop; NULL / 0 / 0: off)
int segnb_fprop_s1_try(segnb_try_outcome* did, const segnb_conv_geom* g, const void* in, const void* wpacked, const float* bias, int bias_n,
                       void* out, double* stats, hipStream_t stream, const float* drop = nullptr, int ld_drop = 0, int stats_ld = 0);
// direct-to-LDS pipeline for Ci % 64 == 0 (fprop_dma.hip)
int segnb_fprop_dma_try(segnb_try_outcome* did, const segnb_conv_geom* g, const void* in, unsigned in_bytes, const void* wpacked,
                        unsigned w_bytes, const float* bias, int bias_n, void* out, double* stats,
                        hipStream_t stream, const segnb_act_epilogue* ep = nullptr, const segnb_upcat_src* uc = nullptr,
                        const segnb_bn_reduce_epilogue* bn = nullptr);
// resident-weights pipeline for the thin layers, Ci <= 96 and Co <= 96 (fprop_rw.hip)
int segnb_fprop_rw_try(segnb_try_outcome* did, const segnb_conv_geom* g, const void* in, unsigned in_bytes, const void* wpacked,
                       unsigned w_bytes, const float* bias, int bias_n, void* out, double* stats,
                       hipStream_t stream, const segnb_bn_reduce_epilogue* bn = nullptr,
                       const segnb_act_epilogue* ep = nullptr, const segnb_upcat_src* uc = nullptr,
                       const segnb_upcat_src* upsum = nullptr);
// rolling-window kernel for the thin layers, weights in registers, no block-level synchronisation (fprop_roll.hip)
int segnb_fprop_roll_try(segnb_try_outcome* did, const segnb_conv_geom* g, const void* in, unsigned in_bytes, const void* wpacked,
                         unsigned w_bytes, const float* bias, int bias_n, void* out, double* stats, hipStream_t stream,
                         const segnb_bn_reduce_epilogue* bn = nullptr, const segnb_operand_tf* tf = nullptr,
                         const segnb_upcat_src* uc = nullptr);
// first layer: 8-channel (3 padded) input, <= 32 output channels (fprop_c8.hip)
int segnb_fprop_c8_try(segnb_try_outcome* did, const segnb_conv_geom* g, const void* in, const void* wpacked, const float* bias, int bias_n,
                       void* out, double* stats, hipStream_t stream, const segnb_act_epilogue* ep = nullptr);
// bna (optional): the dy operand is not in memory -- it is the BatchNorm-backward apply of the layer, recomputed while
// the tile is staged: dy = round(a (round(g act'(z)) - c1 - yhat c2)) from the incoming gradient g and the pre-BatchNorm
// output y (segnb_conv_wgrad_bnapply; the arithmetic and roundings of bn_bwd_apply_kernel's direct form)
struct segnb_wgrad_bnapply {
    const void* g;
    int ld_g;
    const void* y;
    int ld_y;
    const float* coef;      // [4][Cp]: scale, shift, mean, invstd (segnb_bn_finalize)
    const float* bcoef;     // [3][Cp]: a, c1, c2 (segnb_bn_bwd_finalize)
    int Cp;
    int act;
    float slope;
};
// tgt: the armed segnb_wgrad_target or NULL.  With a target a single-slab launch writes the parameter's gradient from its
// accumulators (*did = SEGNB_TRY_DELIVERED: nothing left to do); launches with several slabs leave them unreduced for
// segnb_wgrad_to_param
int segnb_wgrad_s1_try(segnb_try_outcome* did, const segnb_conv_geom* g, const void* in, const void* dout, float* dwp, int nslab,
                       hipStream_t stream, bool partial, const segnb_wgrad_bnapply* bna = nullptr,
                       const segnb_upcat_src* uc = nullptr, const segnb_wgrad_target* tgt = nullptr);      // partial: leave the nslab slabs unreduced
// runtime.hip: the target armed by segnb_wgrad_target_arm on this thread (disarmed by the call), or NULL
const segnb_wgrad_target* segnb_take_wgrad_target();
// wgrad_s1.hip: sum the nslab slabs [Cop][ntaps][Cip] of dwp (fixed order) into the parameter-layout gradient of tgt; rezero: slab 0
// is cleared afterwards (the atomics of the general kernel need a zeroed workspace)
void segnb_wgrad_to_param(float* dwp, int Cop, int ntaps, int Cip, int nslab, const segnb_wgrad_target* tgt, bool rezero,
                          hipStream_t stream);
int segnb_wgrad_s1_slabs(const segnb_conv_geom* g);
void segnb_slab_reduce(float* dwp, long long total, int nslab, hipStream_t stream);
// rolling-window weight gradient of the thin layers (wgrad_roll.hip); tfx / tfd: operands recomputed on load (or NULL)
bool segnb_wgrad_roll_applies(const segnb_conv_geom* g);
int segnb_wgrad_roll_try(segnb_try_outcome* did, const segnb_conv_geom* g, const void* in, const void* dout, float* dwp, int nslab,
                         hipStream_t stream, bool partial, const segnb_operand_tf* tfx = nullptr, const segnb_operand_tf* tfd = nullptr);
int segnb_knob_wgrad_roll();
// the first layer (8 padded input channels): conv_wgrad_c8roll_kernel; bna: dy recomputed from (g, y), dout ignored
bool segnb_wgrad_c8roll_applies(const segnb_conv_geom* g);
int segnb_wgrad_c8roll_try(segnb_try_outcome* did, const segnb_conv_geom* g, const void* in, const void* dout, float* dwp, int nslab,
                           hipStream_t stream, bool partial, const segnb_wgrad_bnapply* bna = nullptr);
int segnb_knob_wgrad_c8roll();
// strided / wide-window tile kernel (wgrad_s1.hip: conv_wgrad_sx_kernel): same protocol
int segnb_wgrad_sx_try(segnb_try_outcome* did, const segnb_conv_geom* g, const void* in, const void* dout, float* dwp, int nslab,
                       hipStream_t stream, bool partial);
int segnb_wgrad_sx_slabs(const segnb_conv_geom* g);
// the four output phases of an Upsample(x2) -> conv3x3 / ConvTranspose2d(4, 2, 1) on the low-resolution tensor (fprop_dma.hip)
int segnb_fprop_upf_try(segnb_try_outcome* did, int N, int H, int W, int Ci, int ld_in, const void* in, unsigned in_bytes,
                        const void* wpacked, unsigned w_bytes, int Co, int CoW, void* out, int ld_out, double* stats,
                        hipStream_t stream, const float* bias = nullptr, int bias_n = 0, int no_prev = 0, int ep_act = -1,
                        float ep_slope = 0.f);
// forward / data gradient of strided, transposed-phase, 2x2, 1x1 and 16-channel-multiple convolutions on halo tiles (fprop_sx.hip)
int segnb_fprop_sx_try(segnb_try_outcome* did, const segnb_conv_geom* g, const void* in, const void* wpacked, const float* bias,
                       int bias_n, void* out, double* stats, hipStream_t stream);

// ------------------------------------------------------------------------------------------------
// element helpers: 8 channels per thread ("chunk8"), fp32 math
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float bf16_bits_to_f32(unsigned short b) {
    return __uint_as_float(((unsigned)b) << 16);
}
__device__ __forceinline__ unsigned short f32_to_bf16_bits(float f) {
    __bf16 h = (__bf16)f;  // v_cvt_pk_bf16_f32: RNE, NaN stays NaN
    return __builtin_bit_cast(unsigned short, h);
}
// value as it reads back from a bf16 store
__device__ __forceinline__ float round_bf16(float v) { return bf16_bits_to_f32(f32_to_bf16_bits(v)); }

template <typename T>
struct Elem;
template <>
struct Elem<float> {
    static constexpr int EPC = 4;  // elements per 16-byte chunk
    __device__ static __forceinline__ float to_f32(float v) { return v; }
    __device__ static __forceinline__ float from_f32(float v) { return v; }
    __device__ static __forceinline__ float round(float v) { return v; }
};
template <>
struct Elem<bf16_t> {
    static constexpr int EPC = 8;
    __device__ static __forceinline__ float to_f32(bf16_t v) { return bf16_bits_to_f32(v.bits); }
    __device__ static __forceinline__ bf16_t from_f32(float v) {
        bf16_t r;
        r.bits = f32_to_bf16_bits(v);
        return r;
    }
    __device__ static __forceinline__ float round(float v) { return round_bf16(v); }
};

// ------------------------------------------------------------------------------------------------
// run-time dtype / flag / small count -> compile-time argument: a launch is written once, generically, in a lambda
//     if (int rc = segnb_dispatch_dtype(dtype, "segnb_x", [&](auto tag) SEGNB_INLINE_LAMBDA {
//             using T = SEGNB_TAG_T(tag);
//             hipLaunchKernelGGL(x_kernel<T>, grid, block, 0, stream, (const T*)in, (T*)out);
//         })) return rc;
//     SEGNB_LAUNCH_CHECK();
// Argument checks and SEGNB_LAUNCH_CHECK stay OUTSIDE the lambda: they print __func__, which inside it is "operator()".
// SEGNB_INLINE_LAMBDA on every such lambda: left to the inliner a helper lambda became a call per use (conv_igemm.hip).
// ------------------------------------------------------------------------------------------------
template <typename T>
struct segnb_type_tag {
    using type = T;
};
#define SEGNB_TAG_T(tag) typename decltype(tag)::type
#define SEGNB_INLINE_LAMBDA __attribute__((always_inline))
// f(segnb_type_tag<bf16_t>) or f(segnb_type_tag<float>); any other dtype is refused here, once, under the caller's name
template <class F>
__attribute__((always_inline)) inline int segnb_dispatch_dtype(int dtype, const char* who, F&& f) {
    if (dtype != SEGNB_BF16 && dtype != SEGNB_F32) {
        segnb_set_error("%s: unknown dtype %d", who, dtype);
        return SEGNB_E_BADARG;
    }
    dtype == SEGNB_BF16 ? f(segnb_type_tag<bf16_t>{}) : f(segnb_type_tag<float>{});
    return 0;
}
// the refusal alone: for an entry point that has to refuse before it prepares its launch (scratch buffers, later checks)
inline int segnb_check_dtype(int dtype, const char* who) {
    return segnb_dispatch_dtype(dtype, who, [](auto) {});
}
// f(std::true_type) or f(std::false_type)
template <class F>
__attribute__((always_inline)) inline void segnb_dispatch_bool(bool v, F&& f) {
    v ? f(std::true_type{}) : f(std::false_type{});
}
// f(std::integral_constant<int, K>) for the first of the ascending bounds K0, Ks... with v <= K (the last one if none holds)
template <int K0, int... Ks, class F>
__attribute__((always_inline)) inline void segnb_dispatch_le(int v, F&& f) {
    if constexpr (sizeof...(Ks) > 0) {
        if (v > K0) return segnb_dispatch_le<Ks...>(v, f);
    }
    f(std::integral_constant<int, K0>{});
}

// load / store 8 consecutive channels as fp32
__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    const float4 b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void load8(const bf16_t* p, float (&v)[8]) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    v[0] = __uint_as_float(u.x << 16); v[1] = __uint_as_float(u.x & 0xffff0000u);
    v[2] = __uint_as_float(u.y << 16); v[3] = __uint_as_float(u.y & 0xffff0000u);
    v[4] = __uint_as_float(u.z << 16); v[5] = __uint_as_float(u.z & 0xffff0000u);
    v[6] = __uint_as_float(u.w << 16); v[7] = __uint_as_float(u.w & 0xffff0000u);
}
__device__ __forceinline__ void store8(float* p, const float (&v)[8]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}
// two fp32 -> one dword of two bf16 (lo in bits 0..15): ONE v_cvt_pk_bf16_f32 through the vector conversion (two scalar
// conversions + shift + or compile to four instructions; same RNE result)
typedef float segnb_f32x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 segnb_bf16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pack2bf(float lo, float hi) {
    const segnb_f32x2_t v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, segnb_bf16x2_t));
}
__device__ __forceinline__ void store8(bf16_t* p, const float (&v)[8]) {
    uint4 u;
    u.x = pack2bf(v[0], v[1]); u.y = pack2bf(v[2], v[3]);
    u.z = pack2bf(v[4], v[5]); u.w = pack2bf(v[6], v[7]);
    *reinterpret_cast<uint4*>(p) = u;
}
// value as it will read back from a T-typed store
__device__ __forceinline__ float round_as(float v, const float*) { return v; }
__device__ __forceinline__ float round_as(float v, const bf16_t*) { return round_bf16(v); }

#include "bn_expr.h"

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

static inline int ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

// ------------------------------------------------------------------------------------------------
// what the kernel tries (segnb_*_try, the *_ok / *_applies predicates beside them) say about a geometry, once.  Forced inline:
// they run per launch, and left to the inliner some of them became calls (as take_bn_reduce above, as the lambdas of 13.20)
// ------------------------------------------------------------------------------------------------
// The window of g's taps: its origin (the smallest row and column offset -- every fast path addresses its input from there) and
// its extent in rows and columns.
struct segnb_tap_win {
    int dhmin, dwmin, kh, kw;
};
SEGNB_HOST_INLINE segnb_tap_win segnb_tap_window(const segnb_conv_geom* g) {
    int dhmin = g->dh[0], dhmax = g->dh[0], dwmin = g->dw[0], dwmax = g->dw[0];
    for (int t = 1; t < g->ntaps; ++t) {
        dhmin = g->dh[t] < dhmin ? g->dh[t] : dhmin;
        dhmax = g->dh[t] > dhmax ? g->dh[t] : dhmax;
        dwmin = g->dw[t] < dwmin ? g->dw[t] : dwmin;
        dwmax = g->dw[t] > dwmax ? g->dw[t] : dwmax;
    }
    return {dhmin, dwmin, dhmax - dhmin + 1, dwmax - dwmin + 1};
}
// a dense 3 x 3 window: 9 taps whose row and column offsets both span exactly 2 (pad 0 or 1, forward or flipped).  Every kernel
// that assumes +-1 neighbours gates on this; a dilated 3 x 3 (segnb.convplan, dilation > 1) has 9 taps over a wider span and goes
// to the general gather kernel
SEGNB_HOST_INLINE bool segnb_taps_3x3(const segnb_conv_geom* g) {
    if (g->ntaps != 9) return false;
    const segnb_tap_win win = segnb_tap_window(g);
    return win.kh == 3 && win.kw == 3;
}
// the tap tables of a kernel's argument struct, relative to the window's origin: 0 .. kh - 1 and 0 .. kw - 1 (after segnb_taps_3x3:
// 0 .. 2); E: int, or signed char in the structs that hold SEGNB_MAX_TAPS of them
template <class E>
SEGNB_HOST_INLINE void segnb_rel_taps(const segnb_conv_geom* g, const segnb_tap_win& win, E* dh_out, E* dw_out) {
    for (int t = 0; t < g->ntaps; ++t) {
        dh_out[t] = (E)(g->dh[t] - win.dhmin);
        dw_out[t] = (E)(g->dw[t] - win.dwmin);
    }
}
// after segnb_taps_3x3 (the spans are 2): each of the nine positions of the window is one tap's, none twice; k_of_tap (may be
// NULL) receives the position row * 3 + column of every tap
SEGNB_HOST_INLINE bool segnb_window_once_3x3(const segnb_conv_geom* g, const segnb_tap_win& win, int* k_of_tap = nullptr) {
    bool seen[9] = {false, false, false, false, false, false, false, false, false};
    for (int t = 0; t < 9; ++t) {
        const int k = (g->dh[t] - win.dhmin) * 3 + (g->dw[t] - win.dwmin);
        if (seen[k]) return false;
        seen[k] = true;
        if (k_of_tap != nullptr) k_of_tap[t] = k;
    }
    return true;
}
// one launch that writes every output pixel of its tensor ...
SEGNB_HOST_INLINE bool whole_output(const segnb_conv_geom* g) {
    return g->out_step == 1 && g->oh0 == 0 && g->ow0 == 0 && g->QH == g->Ho && g->QW == g->Wo;
}
// ... of a dense stride-1 3 x 3: what the fused forward entry points and most of the tries serve
SEGNB_HOST_INLINE bool whole_output_3x3_s1(const segnb_conv_geom* g) { return segnb_taps_3x3(g) && g->in_step == 1 && whole_output(g); }
