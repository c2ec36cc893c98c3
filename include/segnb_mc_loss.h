/* segnb_mc_loss.h -- C ABI of the multi-class segmentation losses in libsegnb_hip.so (csrc/mc_loss.hip):
 * FocalLossMulti, JaccardLossMulti, FocalAndJaccardLossMulti and NLLLAndJaccardLossMulti of the reference's
 * lib/losses.py:105-232, and torch.nn.NLLLoss(weight, ignore_index).
 *
 * Same conventions as segnb_hip.h (status codes, explicit stream, device pointers, graph-capturable).
 * Inputs: logits fp32 NCHW [N][C][HW], target int64 [N][HW] class indices, 1 <= C <= 256.
 *
 * Per pixel, mode 0 takes raw logits (logp = log_softmax, p = softmax over the C channels), mode 1 takes
 * log-probabilities (the reference's from_logits=True: logp = x, p = exp(x)).  A pixel whose label equals
 * ignore_index is ignored.  A label outside [0, C) that is not ignore_index ("bad label"; the reference
 * raises on it) is never used as an index: it adds nothing to the focal and NLL terms, is inside the Jaccard
 * mask without belonging to any class, and is counted.
 *
 * Global sums, 3C + 8 doubles (what a data-parallel job all-reduces):
 *   [0, C) I_c = sum_mask p_c [t == c]   [C, 2C) P_c = sum_mask p_c   [2C, 3C) T_c = #(t == c)
 *   3C focal sum  3C+1 weighted NLL sum  3C+2 weight sum  3C+3 valid pixels  3C+4 all pixels  3C+5 bad labels
 *   3C+6, 3C+7 zero
 * Result vector `fin`, 8 + 3C floats:
 *   0 loss   1 focal coefficient  2 NLL coefficient  3 valid pixels  4 all pixels  5 bad labels
 *   6 focal term  7 NLL term   [8, 8+C) weighted per-class Jaccard losses w_c L_c (the reduce=0 output)
 *   [8+C, 8+2C) dloss/dI_c   [8+2C, 8+3C) dloss/dP_c
 * log_softmax is shift invariant: logp = (x - max) - log(sum exp(x - max)), so a common offset of the logits changes nothing.
 * pt == 1 (logp_t rounds to 0: the target's logit leads by ~17 or more): the focal derivative is its limit, 0 for gamma > 0,
 * also for gamma < 1 where (1 - pt)^(gamma - 1) is unbounded.
 * All pixels ignored: every sum but the pixel count is 0, the focal term, the Jaccard terms and dlogits are exactly 0; the NLL
 * term is 0 / 0: fin[7], and the loss when w_nll != 0, are NaN -- what torch.nn.NLLLoss returns when every target is ignored.
 * Reductions are bitwise reproducible: every workgroup writes one row of partial sums, the last one to finish
 * adds the rows in a fixed order (no floating-point atomics).
 */
#ifndef SEGNB_MC_LOSS_H
#define SEGNB_MC_LOSS_H

#include "segnb_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SEGNB_MC_MAX_CLASSES 256

typedef struct segnb_mc_loss_spec {
    int C;                        /* classes, 1 .. SEGNB_MC_MAX_CLASSES */
    int mode;                     /* 0: logits, 1: log-probabilities */
    long long ignore_index;
    float gamma;                  /* focal exponent */
    float w_focal, w_nll, w_jaccard;  /* term weights */
    float norm;                   /* loss = (w_focal focal + w_nll nll + w_jaccard jaccard) / norm */
    int focal_mean;               /* 1: focal sum / ALL pixels (size_average, ignored ones included); 0: sum */
    int reduce;                   /* 1: Jaccard = sum_c w_c L_c; 0: the per-class vector (w_focal = w_nll = 0) */
    int reserved;
    const float* nll_weight;      /* device [C] or NULL: weights of the NLL term */
    const float* jac_weight;      /* device [C] or NULL: class weights of the Jaccard term, already normalised */
} segnb_mc_loss_spec;

/* doubles of the work buffer the reduce calls need for C classes: per-workgroup rows + a ticket.  Allocate once,
 * ZERO on first use; every call leaves it ready for the next one. */
int segnb_mc_loss_work_doubles(int C);
/* sums [3C + 8] := the global sums of this device's pixels (overwritten, not accumulated) */
int segnb_mc_loss_reduce(const float* logits, const long long* target, int N, int HW, const segnb_mc_loss_spec* spec,
                         double* work, double* sums, segnb_stream_t stream);
/* fin [8 + 3C] from the (all-reduced) sums */
int segnb_mc_loss_finalize(const double* sums, const segnb_mc_loss_spec* spec, float* fin, segnb_stream_t stream);
/* segnb_mc_loss_reduce + segnb_mc_loss_finalize as ONE launch on one device (the last workgroup finalizes);
 * bitwise equal to the two-launch form */
int segnb_mc_loss_reduce_finalize(const float* logits, const long long* target, int N, int HW,
                                  const segnb_mc_loss_spec* spec, double* work, float* fin, segnb_stream_t stream);
/* dlogits [N][C][HW] = d(loss)/d(logits) times the upstream gradient: grad_out is a device fp32 scalar, or a [C]
 * vector when spec->reduce == 0.  Ignored pixels get exactly 0 from the focal and NLL terms. */
int segnb_mc_loss_bwd(const float* logits, const long long* target, int N, int HW, const segnb_mc_loss_spec* spec,
                      const float* fin, const float* grad_out, float* dlogits, segnb_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
