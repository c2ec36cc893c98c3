"""Float64 CPU restatement of GCN34 and of the GCN decoder ABI (include/segnb_gcn.h) -- TEST INFRASTRUCTURE ONLY.

``gcm`` / ``brm`` / ``resize`` restate the reference's _GlobalConvModule, _BoundaryRefineModule and
F.upsample(..., mode='bilinear', align_corners=True) (lib/models/gcn152.py:9-48, 98-115) with torch functional ops;
``forward(sd, x, input_size, train)`` chains them behind the ResNet34 encoder on GCN34's state_dict keys.
``GcnAbiEmulator`` exposes the entry points of segnb_gcn.h on raw host memory the way oracle.abi_emulator.AbiEmulator does for
segnb_hip.h, so the product's host code (segnb.gcn, lib.models.gcn) runs on CPU against the fixture.
"""
import torch
import torch.nn.functional as F

from oracle.abi_emulator import AbiEmulator, _mem, _nhwc, _tdt

F64 = torch.float64
LAYERS = [3, 4, 6, 3]


def gcm(x, drop, wl1, bl1, wl2, bl2, wr1, br1, wr2, br2):
    """-> (out, yl, yr); x [N, C, H, W], drop [N, C] or None"""
    if drop is not None:
        x = x * drop[:, :, None, None]
    yl = F.conv2d(x, wl1, bl1, padding=(wl1.shape[2] // 2, 0))
    yr = F.conv2d(x, wr1, br1, padding=(0, wr1.shape[3] // 2))
    out = F.conv2d(yl, wl2, bl2, padding=(0, wl2.shape[3] // 2)) + F.conv2d(yr, wr2, br2, padding=(wr2.shape[2] // 2, 0))
    return out, yl, yr


def brm(x, w1, b1, w2, b2):
    """-> (out, r)"""
    r = torch.relu(F.conv2d(x, w1, b1, padding=1))
    return x + F.conv2d(r, w2, b2, padding=1), r


def resize(a, size, skip=None):
    out = F.interpolate(a, size=tuple(size), mode='bilinear', align_corners=True)
    return out if skip is None else out + skip


def _bn(sd, p, x, train):
    return F.batch_norm(x, sd[p + 'running_mean'], sd[p + 'running_var'], sd[p + 'weight'], sd[p + 'bias'], training=train,
                        momentum=0.1, eps=1e-5)


def forward(sd, x, input_size, train=True):
    """GCN34 (gcn152.py:63-115) on its state_dict; the GCMs' Dropout2d off"""
    fm0 = torch.relu(_bn(sd, 'layer0.1.', F.conv2d(x, sd['layer0.0.weight'], None, stride=2, padding=3), train))
    h = F.max_pool2d(fm0, 3, 2, 1)
    feats = []
    for li, n in enumerate(LAYERS):
        for bi in range(n):
            p = ('layer1.1.%d.' % bi) if li == 0 else ('layer%d.%d.' % (li + 1, bi))
            stride = 2 if (li > 0 and bi == 0) else 1
            a = torch.relu(_bn(sd, p + 'bn1.', F.conv2d(h, sd[p + 'conv1.weight'], None, stride=stride, padding=1), train))
            b = _bn(sd, p + 'bn2.', F.conv2d(a, sd[p + 'conv2.weight'], None, padding=1), train)
            ident = h
            if (p + 'downsample.0.weight') in sd:
                ident = _bn(sd, p + 'downsample.1.', F.conv2d(h, sd[p + 'downsample.0.weight'], None, stride=stride), train)
            h = torch.relu(b + ident)
        feats.append(h)
    fm1, fm2, fm3, fm4 = feats

    def G(i, t):
        p = 'gcm%d.' % i
        return gcm(t, None, *[sd[p + c + '.' + k] for c in ('conv_l1', 'conv_l2', 'conv_r1', 'conv_r2')
                              for k in ('weight', 'bias')])[0]

    def B(i, t):
        p = 'brm%d.' % i
        return brm(t, sd[p + 'conv1.weight'], sd[p + 'conv1.bias'], sd[p + 'conv2.weight'], sd[p + 'conv2.bias'])[0]

    size = (input_size, input_size) if isinstance(input_size, int) else tuple(input_size)
    gcfm1, gcfm2, gcfm3, gcfm4 = B(1, G(1, fm4)), B(2, G(2, fm3)), B(3, G(3, fm2)), B(4, G(4, fm1))
    fs1 = B(5, resize(gcfm1, fm3.shape[2:], gcfm2))
    fs2 = B(6, resize(fs1, fm2.shape[2:], gcfm3))
    fs3 = B(7, resize(fs2, fm1.shape[2:], gcfm4))
    fs4 = B(8, resize(fs3, fm0.shape[2:]))
    return B(9, resize(fs4, size))


def _f32(p, n):
    return _mem(p, n, torch.float32)


def _leaf(p, shape):
    return _f32(p, int(torch.tensor(shape).prod())).view(*shape).to(F64).requires_grad_(True)


def _add_grad(p, g):
    if p:
        t = _f32(p, g.numel())
        t.copy_((t.double() + g.reshape(-1)).float())


class GcnAbiEmulator(AbiEmulator):
    """AbiEmulator + the entry points of include/segnb_gcn.h, on raw host memory (CPU tensors)."""

    def segnb_gcn_ok(self, C, K, N, H, W):
        if not (1 <= K <= 32 and N >= 1 and H >= 1 and W >= 1):
            return 0
        if C != 0 and (C < 8 or C % 8 or C > 2048):
            return 0
        return 1 if N * H * W * K < 2 ** 31 else 0

    @staticmethod
    def _x(dtype, x, ld, N, H, W, C):
        return _nhwc(x, N, H, W, C, ld, _tdt(dtype)).permute(0, 3, 1, 2).to(F64)

    @staticmethod
    def _gcm_w(C, K, wl1, wl2, wr1, wr2):
        return (_leaf(wl1, (K, C, 7, 1)), _leaf(wl2, (K, K, 1, 7)), _leaf(wr1, (K, C, 1, 7)), _leaf(wr2, (K, K, 7, 1)))

    def segnb_gcm_fwd(self, dtype, x, ld, N, H, W, C, K, drop, wl1, bl1, wl2, bl2, wr1, br1, wr2, br2, yl, yr, out, stream):
        if not self.segnb_gcn_ok(C, K, N, H, W) or not C:
            return -1
        X = self._x(dtype, x, ld, N, H, W, C)
        D = _f32(drop, N * C).view(N, C).to(F64) if drop else None
        Wl1, Wl2, Wr1, Wr2 = self._gcm_w(C, K, wl1, wl2, wr1, wr2)
        b = [_leaf(p, (K,)) for p in (bl1, bl2, br1, br2)]
        with torch.no_grad():
            o, l, r = gcm(X, D, Wl1, b[0], Wl2, b[1], Wr1, b[2], Wr2, b[3])
        for p, t in ((yl, l), (yr, r), (out, o)):
            _f32(p, t.numel()).copy_(t.reshape(-1).float())
        return 0

    @torch.enable_grad()           # (called from inside an autograd backward)
    def segnb_gcm_bwd(self, dtype, x, ld, N, H, W, C, K, drop, wl1, wl2, wr1, wr2, yl, yr, dout, dyl, dyr, dx, ld_dx,
                      g_wl1, g_bl1, g_wl2, g_bl2, g_wr1, g_br1, g_wr2, g_br2, stream):
        if not self.segnb_gcn_ok(C, K, N, H, W) or not C:
            return -1
        shape = (N, K, H, W)
        Xd = self._x(dtype, x, ld, N, H, W, C)
        D = _f32(drop, N * C).view(N, C).to(F64) if drop else None
        if D is not None:
            Xd = Xd * D[:, :, None, None]
        Xd.requires_grad_(True)
        Wl1, Wl2, Wr1, Wr2 = self._gcm_w(C, K, wl1, wl2, wr1, wr2)
        bz = [torch.zeros(K, dtype=F64, requires_grad=True) for _ in range(4)]
        Yl, Yr = _leaf(yl, shape), _leaf(yr, shape)
        G = _f32(dout, N * K * H * W).view(shape).to(F64)
        o = F.conv2d(Yl, Wl2, bz[1], padding=(0, 3)) + F.conv2d(Yr, Wr2, bz[3], padding=(3, 0))
        o.backward(G)
        _f32(dyl, Yl.grad.numel()).copy_(Yl.grad.reshape(-1).float())
        _f32(dyr, Yr.grad.numel()).copy_(Yr.grad.reshape(-1).float())
        dYl, dYr = Yl.grad.float().double(), Yr.grad.float().double()      # (the kernel reads its fp32 work maps back)
        l = F.conv2d(Xd, Wl1, bz[0], padding=(3, 0))
        r = F.conv2d(Xd, Wr1, bz[2], padding=(0, 3))
        torch.autograd.backward([l, r], [dYl, dYr])
        for p, t in ((g_wl1, Wl1.grad), (g_bl1, bz[0].grad), (g_wl2, Wl2.grad), (g_bl2, bz[1].grad), (g_wr1, Wr1.grad),
                     (g_br1, bz[2].grad), (g_wr2, Wr2.grad), (g_br2, bz[3].grad)):
            _add_grad(p, t)
        if dx:
            d = Xd.grad if D is None else Xd.grad * D[:, :, None, None]
            _nhwc(dx, N, H, W, C, ld_dx, _tdt(dtype)).copy_(d.permute(0, 2, 3, 1))
        return 0

    def segnb_brm_fwd(self, N, H, W, K, x, w1, b1, w2, b2, r, out, stream):
        if not self.segnb_gcn_ok(0, K, N, H, W):
            return -1
        shape = (N, K, H, W)
        with torch.no_grad():
            o, rr = brm(_leaf(x, shape), _leaf(w1, (K, K, 3, 3)), _leaf(b1, (K,)), _leaf(w2, (K, K, 3, 3)), _leaf(b2, (K,)))
        _f32(r, rr.numel()).copy_(rr.reshape(-1).float())
        _f32(out, o.numel()).copy_(o.reshape(-1).float())
        return 0

    @torch.enable_grad()           # (called from inside an autograd backward)
    def segnb_brm_bwd(self, N, H, W, K, x, w1, w2, r, dout, dr, dx, g_w1, g_b1, g_w2, g_b2, stream):
        if not self.segnb_gcn_ok(0, K, N, H, W):
            return -1
        shape = (N, K, H, W)
        X, W1, W2, R = _leaf(x, shape), _leaf(w1, (K, K, 3, 3)), _leaf(w2, (K, K, 3, 3)), _leaf(r, shape)
        b1, b2 = torch.zeros(K, dtype=F64, requires_grad=True), torch.zeros(K, dtype=F64, requires_grad=True)
        G = _f32(dout, N * K * H * W).view(shape).to(F64)
        o = X + F.conv2d(R, W2, b2, padding=1)
        o.backward(G)
        dR = (R.grad * (R.detach() > 0)).float().double()
        _f32(dr, dR.numel()).copy_(dR.reshape(-1).float())
        X2 = X.detach().clone().requires_grad_(True)
        F.conv2d(X2, W1, b1, padding=1).backward(dR)
        _f32(dx, X.numel()).copy_((X.grad + X2.grad).reshape(-1).float())
        for p, t in ((g_w1, W1.grad), (g_b1, b1.grad), (g_w2, W2.grad), (g_b2, b2.grad)):
            _add_grad(p, t)
        return 0

    def segnb_resize_bilinear_ac_fwd(self, N, K, h, w, a, H, W, skip, out, stream):
        if not (self.segnb_gcn_ok(0, K, N, h, w) and self.segnb_gcn_ok(0, K, N, H, W)):
            return -1
        A = _f32(a, N * K * h * w).view(N, K, h, w).to(F64)
        S = _f32(skip, N * K * H * W).view(N, K, H, W).to(F64) if skip else None
        _f32(out, N * K * H * W).copy_(resize(A, (H, W), S).reshape(-1).float())
        return 0

    @torch.enable_grad()           # (called from inside an autograd backward)
    def segnb_resize_bilinear_ac_bwd(self, N, K, h, w, H, W, dout, din, stream):
        if not (self.segnb_gcn_ok(0, K, N, h, w) and self.segnb_gcn_ok(0, K, N, H, W)):
            return -1
        A = torch.zeros((N, K, h, w), dtype=F64, requires_grad=True)
        resize(A, (H, W)).backward(_f32(dout, N * K * H * W).view(N, K, H, W).to(F64))
        _f32(din, A.numel()).copy_(A.grad.reshape(-1).float())
        return 0
