"""Tape helpers of the GCN decoder (lib.models.gcn; the reference's lib/models/gcn152.py:9-48, 98-115) over the kernels of
csrc/gcn.hip (include/segnb_gcn.h).

The decoder works on K = num_classes channels, so its maps are fp32 planar [N, K, H, W] tensors (``Map``) in both compute
dtypes -- the last one IS the fp32 NCHW logits.  Only the Global Convolution Modules touch the executor's NHWC encoder
views: they read one (Dropout2d multipliers applied on load) and hand its data gradient to ``Tape.contribute``.  Every other
decoder map has exactly one consumer, whose backward sets the map's gradient (``Map.g``).

Every helper launches its forward at once and records its backward on the tape, like segnb.net's helpers; every buffer is
cached per call site, so steady-state steps allocate nothing and replay from the recorded launch lists.  Parameter
gradients are added into the flat gradient buffer (``FlatParams.grad_of``), as the head kernels do.
"""
import torch

from . import _native as nv
from .engine import vld, vptr


class Map(object):
    """A decoder map: fp32 [N, K, H, W] tensor ``t`` and, during backward, its gradient ``g`` (same shape) or None."""
    __slots__ = ('t', 'g')

    def __init__(self, t):
        self.t, self.g = t, None


def _buf(tape, key, shape):
    return tape.cached((key, tuple(shape)), lambda: torch.zeros(shape, dtype=torch.float32, device=tape.rt.device))


def _p(t):
    return nv.ptr(t.detach())


def _check(C, K, N, H, W):
    if not nv.query('segnb_gcn_ok', C, K, N, H, W):
        raise ValueError('GCN decoder kernels: %d classes, %d feature channels, %dx%dx%d maps are out of range '
                         '(segnb_gcn_ok: 1 <= K <= 32, C a multiple of 8 up to 2048)' % (K, C, N, H, W))


def global_conv(tape, x, gcm, tag='gcm'):
    """gcm(x) (gcn152.py:26-34): Dropout2d, then conv_l2(conv_l1(x)) + conv_r2(conv_r1(x)) -> Map.  x: the encoder's Act."""
    rt, xv = tape.rt, x.v
    site = tape.site(tag)
    tape.consume(x)
    l1, l2, r1, r2 = gcm.conv_l1, gcm.conv_l2, gcm.conv_r1, gcm.conv_r2
    N, H, W, C, K = xv.N, xv.H, xv.W, l1.in_channels, l1.out_channels
    if xv.Cp != C:
        raise ValueError('GCM over %d channels reads a view of %d' % (C, xv.Cp))
    _check(C, K, N, H, W)
    shape = (N, K, H, W)
    yl, yr, out = _buf(tape, site + '/yl', shape), _buf(tape, site + '/yr', shape), _buf(tape, site + '/o', shape)
    drop = tape.dropout_table(site, N, C, gcm.pre_drop.p)
    nv.call('segnb_gcm_fwd', rt.code, xv.ptr, xv.ld, N, H, W, C, K, nv.ptr(drop), _p(l1.weight), _p(l1.bias), _p(l2.weight),
            _p(l2.bias), _p(r1.weight), _p(r1.bias), _p(r2.weight), _p(r2.bias), nv.ptr(yl), nv.ptr(yr), nv.ptr(out), rt.stream)
    m = Map(out)

    def backward():
        if m.g is None:
            return
        g = tape.flat.grad_of
        dyl, dyr = _buf(tape, site + '/dyl', shape), _buf(tape, site + '/dyr', shape)
        dx = tape.view(site + '/dx', N, H, W, xv.Cp) if x.needs_grad else None
        nv.call('segnb_gcm_bwd', rt.code, xv.ptr, xv.ld, N, H, W, C, K, nv.ptr(drop), _p(l1.weight), _p(l2.weight),
                _p(r1.weight), _p(r2.weight), nv.ptr(yl), nv.ptr(yr), nv.ptr(m.g), nv.ptr(dyl), nv.ptr(dyr), vptr(dx), vld(dx),
                nv.ptr(g(l1.weight)), nv.ptr(g(l1.bias)), nv.ptr(g(l2.weight)), nv.ptr(g(l2.bias)), nv.ptr(g(r1.weight)),
                nv.ptr(g(r1.bias)), nv.ptr(g(r2.weight)), nv.ptr(g(r2.bias)), rt.stream)
        if dx is not None:
            tape.contribute(x, dx)

    tape.record(backward)
    return m


def boundary_refine(tape, m, brm, dlogits_ref=None, tag='brm'):
    """brm(m) = m + conv2(relu(conv1(m))) (gcn152.py:37-48) -> Map; with dlogits_ref (the model's last module) -> the fp32
    NCHW logits tensor, whose gradient the backward reads from dlogits_ref[0]."""
    rt = tape.rt
    site = tape.site(tag)
    N, K, H, W = m.t.shape
    _check(0, K, N, H, W)
    shape = (N, K, H, W)
    r, out = _buf(tape, site + '/r', shape), _buf(tape, site + '/o', shape)
    c1, c2 = brm.conv1, brm.conv2
    nv.call('segnb_brm_fwd', N, H, W, K, nv.ptr(m.t), _p(c1.weight), _p(c1.bias), _p(c2.weight), _p(c2.bias), nv.ptr(r),
            nv.ptr(out), rt.stream)
    o = Map(out)

    def backward():
        dout = dlogits_ref[0] if dlogits_ref is not None else o.g
        if dout is None:
            return
        g = tape.flat.grad_of
        dr, dx = _buf(tape, site + '/dr', shape), _buf(tape, site + '/dx', shape)
        nv.call('segnb_brm_bwd', N, H, W, K, nv.ptr(m.t), _p(c1.weight), _p(c2.weight), nv.ptr(r), nv.ptr(dout), nv.ptr(dr),
                nv.ptr(dx), nv.ptr(g(c1.weight)), nv.ptr(g(c1.bias)), nv.ptr(g(c2.weight)), nv.ptr(g(c2.bias)), rt.stream)
        m.g = dx

    tape.record(backward)
    return out if dlogits_ref is not None else o


def resize_add(tape, a, size, skip=None, tag='resize'):
    """F.interpolate(a, size, mode='bilinear', align_corners=True) (+ skip) (gcn152.py:107-111) -> Map."""
    rt = tape.rt
    site = tape.site(tag)
    N, K, h, w = a.t.shape
    H, W = size
    _check(0, K, N, H, W)
    if skip is not None and tuple(skip.t.shape) != (N, K, H, W):
        raise ValueError('resize_add: skip %s does not match the output %s' % (tuple(skip.t.shape), (N, K, H, W)))
    out = _buf(tape, site + '/o', (N, K, H, W))
    nv.call('segnb_resize_bilinear_ac_fwd', N, K, h, w, nv.ptr(a.t), H, W, nv.ptr(skip.t) if skip is not None else None,
            nv.ptr(out), rt.stream)
    o = Map(out)

    def backward():
        if o.g is None:
            return
        din = _buf(tape, site + '/d', (N, K, h, w))
        nv.call('segnb_resize_bilinear_ac_bwd', N, K, h, w, H, W, nv.ptr(o.g), nv.ptr(din), rt.stream)
        a.g = din
        if skip is not None:
            skip.g = o.g              # (the skip's only consumer: nothing writes o.g again in this backward)

    tape.record(backward)
    return o
