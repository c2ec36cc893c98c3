/* segnb_elu.h -- C ABI of the ELU passes in libsegnb_hip.so (csrc/elu.hip): nn.ELU (alpha = 1) over an executor tensor, with
 * the nearest x2 upsample + skip add of the reference's lib/models/squeezenet.py:137-149 folded into the same launch, and the
 * matching backward.
 *
 * Same conventions as segnb_hip.h (status codes, explicit stream, device pointers, graph-capturable, recordable into launch
 * plans).  Tensors are the executor's NHWC views: dtype SEGNB_F32 / SEGNB_BF16, Cp channels per pixel (Cp % 8 == 0), pixel
 * stride ld (ld % 8 == 0, ld >= Cp: a slice of a concat buffer is wider than its channels; channels [Cp, ld) are never
 * touched).  All arithmetic is fp32; rnd() is the rounding to the storage type.
 *
 * ELU is not one of the SEGNB_ACT_* codes: the convolution epilogues encode an activation as one multiplier for negative
 * values, which ELU is not.  A convolution in front of an ELU runs with SEGNB_ACT_NONE and these passes do the rest.
 */
#ifndef SEGNB_ELU_H
#define SEGNB_ELU_H

#include "segnb_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SEGNB_ELU_MAX_C 1024

/* 1 when the two launches serve the shape: dtype SEGNB_F32 / SEGNB_BF16, N, H, W >= 1, Cp a multiple of 8 in
 * [8, SEGNB_ELU_MAX_C], 16 * N * H * W < 2^31 (the upsampled tensor is indexed in 32 bits); else 0 */
int segnb_elu_ok(int dtype, int N, int H, int W, int Cp);

/* a = rnd(elu(z)), elu(v) = v > 0 ? v : expm1f(v).  a may be z (in place).
 * up_out != NULL: up_skip and up_out are [N][2H][2W] views and
 *   up_out[n][2h+i][2w+j][c] = rnd(float(a[n][h][w][c]) + float(up_skip[n][2h+i][2w+j][c])),  i, j in {0, 1}
 * with a the ROUNDED value just stored: the launch is bit-equal to the ELU pass, a materialised nearest copy and segnb_add.
 * up_out may alias up_skip; it may not alias a. */
int segnb_elu_fwd(int dtype, const void* z, int ld_z, int N, int H, int W, int Cp, void* a, int ld_a,
                  const void* up_skip, int ld_skip, void* up_out, int ld_up, segnb_stream_t stream);

/* From the STORED activated tensor a (the raw z need not survive):
 *   g  = g_direct + g_add + (g_up[2h][2w] + g_up[2h][2w+1] + g_up[2h+1][2w] + g_up[2h+1][2w+1])      (fp32, in this order)
 *   dz = rnd(g * (a > 0 ? 1 : float(a) + 1))
 * g_direct, g_add: [N][H][W] views; g_up: [N][2H][2W], the gradient of up_out.  Any source may be NULL, at least one is given.
 * dz may alias g_direct.
 * sums: the per-channel sum of the stored dz is added to row 0 of the producing convolution's table, fp64
 * [SEGNB_STAT_REPLICAS][2][row] (the table segnb_head_conv_bwd fills for a layer without BatchNorm; a block adds into replica
 * blockIdx.x % SEGNB_STAT_REPLICAS).  Channels [0, C0p) go to sums0 (row = C0p), channels [C0p, Cp) to sums1 (row = Cp - C0p):
 * one pass over a concat buffer whose halves belong to two convolutions.  sums1 NULL with C0p == Cp: one table.  Both NULL:
 * no sums (C0p ignored). */
int segnb_elu_bwd(int dtype, const void* a, int ld_a, int N, int H, int W, int Cp, const void* g_direct, int ld_gd,
                  const void* g_add, int ld_ga, const void* g_up, int ld_gu, void* dz, int ld_dz, double* sums0, int C0p,
                  double* sums1, segnb_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
