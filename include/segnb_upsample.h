/* segnb_upsample.h -- C ABI of the nearest-neighbour x2 upsample passes in libsegnb_hip.so (csrc/elementwise.hip):
 * nn.Upsample(scale_factor=2, mode='nearest') of the reference's lib/models/unet.py:53 (UNet, UNetABN, Afterburner) over an
 * executor tensor, and its backward.
 *
 * Same conventions as segnb_hip.h (status codes, explicit stream, device pointers, graph-capturable, recordable into launch
 * plans) and the same argument order as segnb_upsample_bilinear2x_fwd / _bwd.  Tensors are the executor's NHWC views: dtype
 * SEGNB_F32 / SEGNB_BF16, Cp channels per pixel (Cp % 8 == 0), pixel stride ld (ld % 8 == 0, ld >= Cp: the output is normally a
 * slice of a concat buffer and the gradient a slice of a concat gradient; channels [Cp, ld) are never read or written), base
 * pointers 16-byte aligned.  H, W: the LOW-resolution size; 16 * N * H * W < 2^31 (the upsampled tensor is indexed as the
 * bilinear pair indexes it).  Anything else is refused with SEGNB_E_BADARG and a message.
 *
 * A header of its own: segnb_hip.h's set of names is the one its CPU restatement (oracle/abi_emulator.py) and the recorded
 * element-wise table (tests/ew_table_parent.json) cover; these two are restated in tests/unet_ref.py.
 */
#ifndef SEGNB_UPSAMPLE_H
#define SEGNB_UPSAMPLE_H

#include "segnb_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[n][2h+i][2w+j][c] = x[n][h][w][c], i, j in {0, 1}: a copy -- no arithmetic, no rounding.  x is not written; out may not
 * alias x. */
int segnb_upsample_nearest2x_fwd(int dtype, const void* x, int ld_x, int N, int H, int W, int Cp, void* out, int ld_out,
                                 segnb_stream_t stream);

/* dx[n][h][w][c] = rnd(((g[2h][2w] + g[2h][2w+1]) + g[2h+1][2w]) + g[2h+1][2w+1]), g = g_out[n]: summed in fp32 in exactly this
 * scan order and rounded once to the storage type -- the order of segnb_bn_act_bwd_reduce's g_up and of segnb_elu_bwd's g_up, so
 * the three agree bit for bit.  dx is written, not accumulated; it may not alias g_out. */
int segnb_upsample_nearest2x_bwd(int dtype, const void* g_out, int ld_go, int N, int H, int W, int Cp, void* dx, int ld_dx,
                                 segnb_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
