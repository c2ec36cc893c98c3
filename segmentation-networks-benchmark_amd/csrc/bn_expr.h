// The per-element expressions of the activation and BatchNorm passes, defined ONCE (included by common.h).
//
// A training step is bit-reproducible, and several fusions rest on different kernels computing the same bits for the same
// expression: a kernel that recomputes a BatchNorm pass on the way in or out (wgrad_s1.hip BNA, wgrad_roll.hip TFD = 3, the
// store passes of the data-gradient kernels) calls these helpers and never restates them.  One expression tree = one
// contraction decision of the compiler; the "* 1.f" and "+ 0.f" below are part of the tree.
#pragma once

// Branch-free activations: none / ReLU / LeakyReLU are all "negative side scaled by s" with s = 1 / 0 / slope (a
// switch on `act` per element compiled to two scalar branches per element -- 153 branches in the pooled backward
// kernel -- with the loads fenced between them).  "+ 0.f" turns ReLU's -0.0 into torch's +0.0.
__device__ __forceinline__ float act_neg_scale(int act, float slope) {
    return act == SEGNB_ACT_RELU ? 0.f : (act == SEGNB_ACT_LEAKY ? slope : 1.f);
}
__device__ __forceinline__ float act_fwd(float z, int act, float slope) {
    return (z > 0.f ? z : z * act_neg_scale(act, slope)) + 0.f;
}
__device__ __forceinline__ float act_grad(float z, int act, float slope) {
    return z > 0.f ? 1.f : act_neg_scale(act, slope);
}
// ... with neg = act_neg_scale() taken once, outside the pixel loop.  The activation epilogues of the convolutions:
__device__ __forceinline__ float act_fwd_neg(float v, float neg) { return v < 0.f ? v * neg + 0.f : v; }
__device__ __forceinline__ float act_grad_neg(float z, float neg) { return z > 0.f ? 1.f : neg; }
// g * act'(z) as a select between g and g * neg
__device__ __forceinline__ float act_bwd_neg(float g, float z, float neg) { return z > 0.f ? g : g * neg; }

// The two per-element expressions of the BatchNorm-backward apply pass (bn_bwd_apply_kernel, both forms) and of every kernel
// that recomputes its result: dz = d * act'(z), dy = a * (dz - c1 - yhat * c2)
__device__ __forceinline__ float bn_dz_elem(float d, float yv, float mu, float sc, float sh, int act, float slope) {
    return d * 1.f * act_grad((yv - mu) * sc + sh + 0.f, act, slope);
}
__device__ __forceinline__ float bn_dz_elem(float d, float yv, float mu, float sc, float sh, float neg) {
    const float z = (yv - mu) * sc + sh + 0.f;
    return d * 1.f * act_grad_neg(z, neg);
}
__device__ __forceinline__ float bn_apply_elem(float yv, float d, float mu, float is, float a, float c1, float c2) {
    const float yh = (yv - mu) * is;
    return a * (d - c1 - yh * c2);
}

// The seven per-channel constants of that pass: coef [4][Cp] (scale, shift, mean, invstd: segnb_bn_finalize) and bcoef [3][Cp]
// (a, c1, c2: segnb_bn_bwd_finalize)
struct BnBwdConsts {
    float sc, sh, mu, is, a, c1, c2;
};
__device__ __forceinline__ BnBwdConsts bn_bwd_consts(const float* coef, const float* bcoef, int Cp, int c) {
    return {coef[c], coef[Cp + c], coef[2 * Cp + c], coef[3 * Cp + c], bcoef[c], bcoef[Cp + c], bcoef[2 * Cp + c]};
}

// The folded row of the on-load transforms of the rolling kernels (fprop_roll.hip TF = 2, wgrad_roll.hip TFD = 2): five
// constants per channel instead of seven, the registers being the budget there.  With z = y * sc + shh, sel = act'(z):
//   dy = a * (g * sel) + (B * y + C),   shh = shift - mean * scale,  B = -a * c2 * invstd,  C = a * (c2 * invstd * mean - c1)
// row[k * stride + c], k = 0..4, receives (sc, shh, a, B, C) of channel c
__device__ __forceinline__ void bn_fold5_row(float* row, int stride, int c, const BnBwdConsts& k) {
    row[c] = k.sc;
    row[stride + c] = k.sh - k.mu * k.sc;
    row[2 * stride + c] = k.a;
    row[3 * stride + c] = -k.a * k.c2 * k.is;
    row[4 * stride + c] = k.a * (k.c2 * k.is * k.mu - k.c1);
}
