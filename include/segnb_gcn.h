/* segnb_gcn.h -- C ABI of the GCN decoder kernels in libsegnb_hip.so (csrc/gcn.hip): the Global Convolution Module (GCM),
 * the Boundary Refine Module (BRM) and the align_corners=True bilinear resize of the reference's lib/models/gcn152.py:9-48,
 * 98-115.
 *
 * Same conventions as segnb_hip.h (status codes, explicit stream, device pointers, graph-capturable, recordable into launch
 * plans).  Decoder maps are fp32 planar [N][K][H][W], 1 <= K <= SEGNB_GCN_MAX_K.  The encoder feature x of a GCM is an NHWC
 * view (dtype SEGNB_F32 / SEGNB_BF16, pixel stride ld, ld % 8 == 0, ld >= C), C % 8 == 0, C <= SEGNB_GCN_MAX_C.
 * Parameters are read in their nn.Conv2d layout: conv weight [K_out][K_in][kh][kw], bias [K_out].  Every convolution is
 * stride 1 with "same" zero padding ((kh - 1) / 2, (kw - 1) / 2).
 *
 * Parameter gradients are ADDED into the g* pointers (NULL: not computed).  Their reductions over the N*H*W pixels are bitwise
 * reproducible: each workgroup writes one row of partial sums, a second launch adds the rows in a fixed order (no
 * floating-point atomics).  No entry point allocates, except the partial-sum scratch it shares with the head kernels.
 */
#ifndef SEGNB_GCN_H
#define SEGNB_GCN_H

#include "segnb_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SEGNB_GCN_MAX_K 32
#define SEGNB_GCN_MAX_C 2048

/* 1 when the kernels serve C feature channels (0: no feature, BRM / resize only), K classes and an N x H x W map, else 0 */
int segnb_gcn_ok(int C, int K, int N, int H, int W);

/* GCM forward (gcn152.py:26-34): xd = x * drop[n][c] (drop fp32 [N][C] Dropout2d multipliers, or NULL);
 *   yl = conv_l1(xd) (7x1, pad (3,0), C -> K), yr = conv_r1(xd) (1x7, pad (0,3), C -> K)   -- kept for the backward
 *   out = conv_l2(yl) (1x7, K -> K) + conv_r2(yr) (7x1, K -> K)
 * x is read once. */
int segnb_gcm_fwd(int dtype, const void* x, int ld, int N, int H, int W, int C, int K, const float* drop,
                  const float* w_l1, const float* b_l1, const float* w_l2, const float* b_l2,
                  const float* w_r1, const float* b_r1, const float* w_r2, const float* b_r2,
                  float* yl, float* yr, float* out, segnb_stream_t stream);
/* GCM backward from dout [N][K][H][W]: dyl, dyr are fp32 [N][K][H][W] work maps; dx (NHWC view of dtype, stride ld_dx, or
 * NULL) := drop * (conv_l1^T(dyl) + conv_r1^T(dyr)) -- written, not accumulated; the eight parameter gradients are added. */
int segnb_gcm_bwd(int dtype, const void* x, int ld, int N, int H, int W, int C, int K, const float* drop,
                  const float* w_l1, const float* w_l2, const float* w_r1, const float* w_r2,
                  const float* yl, const float* yr, const float* dout, float* dyl, float* dyr, void* dx, int ld_dx,
                  float* g_wl1, float* g_bl1, float* g_wl2, float* g_bl2, float* g_wr1, float* g_br1, float* g_wr2,
                  float* g_br2, segnb_stream_t stream);

/* BRM forward (gcn152.py:37-48): r = relu(conv1(x)) (kept for the backward), out = x + conv2(r); 3x3 convs, K -> K */
int segnb_brm_fwd(int N, int H, int W, int K, const float* x, const float* w1, const float* b1, const float* w2,
                  const float* b2, float* r, float* out, segnb_stream_t stream);
/* BRM backward: dr is an fp32 [N][K][H][W] work map; dx := dout + conv1^T(relu'(r) * conv2^T(dout)) (dx must not alias dout) */
int segnb_brm_bwd(int N, int H, int W, int K, const float* x, const float* w1, const float* w2, const float* r,
                  const float* dout, float* dr, float* dx, float* g_w1, float* g_b1, float* g_w2, float* g_b2,
                  segnb_stream_t stream);

/* out [N][K][H][W] = bilinear resize of in [N][K][h][w] with align_corners=True (F.interpolate) + skip (same shape as out,
 * or NULL) */
int segnb_resize_bilinear_ac_fwd(int N, int K, int h, int w, const float* in, int H, int W, const float* skip, float* out,
                                 segnb_stream_t stream);
/* din [N][K][h][w] := the adjoint of the resize applied to dout [N][K][H][W], as a gather: each input pixel sums the output
 * pixels that read it, in a fixed order (written, not accumulated) */
int segnb_resize_bilinear_ac_bwd(int N, int K, int h, int w, int H, int W, const float* dout, float* din,
                                 segnb_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
