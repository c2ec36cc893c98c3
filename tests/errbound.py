"""Derived per-element error bounds and exact impulse probes for the convolution kernels (helper module: no fixtures, no
pytest settings).

Every reference here is computed on the CPU in float64 with F.conv2d / F.conv_transpose2d and autograd, on the very operands the
kernel under test receives (bf16-rounded on the bf16 path).

The bound.  A kernel accumulates K exact products a_i * b_i in fp32, in an order of its own, and stores the sum in the output
type.  With acc the fp32 sum and ref the exact one,

    |store(acc) - ref| <= r_out * |acc| + |acc - ref|,      |acc - ref| <= gamma_K * sum |a_i b_i|      (any order)

so, with mag = sum |a_i b_i| (the same operation on the operands' magnitudes) and gamma_K ~ K * u,

    bound = r_out * |ref| * (1 + 2^-8) + K * u * mag * (1 + r_out) + 2^-126

r_out = 2^-8 for a bf16 store (round to nearest even: f32_to_bf16_bits of csrc/common.h; half an ulp is at most 2^-8 relative),
0 for an fp32 store; the factor (1 + 2^-8) covers r_out * |acc| where |acc| exceeds |ref| by the store's own rounding step, and
2^-126 is the smallest normal fp32 (results below it may be flushed).

The impulse probes.  Operands with so few non-zero entries that every output element is one product (plus the bias): then the
result is the same in every summation order and the comparison is `==`, with no tolerance.
"""
import zlib

import torch
import torch.nn.functional as F

# Unit roundoff of one fp32 addition inside the kernels: 2^-23, not 2^-24.  Whether the additions inside an MFMA instruction
# round to nearest has not been measured in this project; 2^-23 covers truncation, the worst a binary adder does.
U_ACC = 2.0 ** -23
R_BF16 = 2.0 ** -8
TINY = 2.0 ** -126


# ------------------------------------------------------------------------------------------------------
# operands and references
# ------------------------------------------------------------------------------------------------------
def full_case(case):
    """the 6-field rows of the DMA / RW tables (3 x 3, stride 1, pad 1) in the 10-field form of CONV_CASES"""
    return tuple(case) if len(case) == 10 else tuple(case) + (3, 1, 1, False)


def out_size(case):
    name, N, H, W, segs, Co, k, s, p, transposed = case
    if transposed:
        return (H - 1) * s - 2 * p + k, (W - 1) * s - 2 * p + k
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def seed_of(name):
    return zlib.crc32(name.encode()) % 1000


def operands(case, dtype):
    """the data recipe of test_conv_fprop_dgrad_wgrad: -> w, b, x [N,Ci,H,W], dy [N,Co,Ho,Wo] (fp32 tensors; w, x, dy bf16-rounded
    on the bf16 path)"""
    name, N, H, W, segs, Co, k, s, p, transposed = case
    Ci = sum(r for r, _ in segs)
    gen = torch.Generator().manual_seed(seed_of(name))
    w = torch.randn((Ci, Co, k, k) if transposed else (Co, Ci, k, k), generator=gen) * (2.0 / (Ci * k * k)) ** 0.5
    b = torch.randn(Co, generator=gen) * 0.1
    x = torch.randn(N, Ci, H, W, generator=gen)
    Ho, Wo = out_size(case)
    dy = torch.randn(N, Co, Ho, Wo, generator=gen)
    if dtype == 'bf16':
        w, x, dy = (t.bfloat16().float() for t in (w, x, dy))
    return w, b, x, dy


def _conv64(x, w, b, stride, pad, transposed):
    if transposed:
        return F.conv_transpose2d(x, w, b, stride=stride, padding=pad)
    return F.conv2d(x, w, b, stride=stride, padding=pad)


def _three(x, w, b, dy, stride, pad, transposed):
    x = x.detach().double().clone().requires_grad_(True)
    w = w.detach().double().clone().requires_grad_(True)
    y = _conv64(x, w, None if b is None else b.detach().double(), stride, pad, transposed)
    y.backward(dy.detach().double())
    return y.detach(), x.grad, w.grad


def conv_refs(x, w, b, dy, stride, pad, transposed):
    """float64 y, dx, dW of the convolution; mag_y, mag_dx (and mag_dW): the same operations on |x|, |w|, |b|, |dy|, i.e. the sum
    of the magnitudes of the products behind each element; K_y, K_dx: the number of terms of an element of y / dx."""
    y, dx, dW = _three(x, w, b, dy, stride, pad, transposed)
    mag_y, mag_dx, mag_dW = _three(x.abs(), w.abs(), None if b is None else b.abs(), dy.abs(), stride, pad, transposed)
    k = w.shape[-1] * w.shape[-2]
    Ci, Co = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
    return dict(y=y, dx=dx, dW=dW, mag_y=mag_y, mag_dx=mag_dx, mag_dW=mag_dW, K_y=Ci * k + 1, K_dx=Co * k)


def round_out(t, out_dtype):
    """the rounding of the stored output type applied to an fp32 tensor (bf16: round to nearest even; f32: none)"""
    t = t.float()
    return t.bfloat16().float() if out_dtype == 'bf16' else t


def real_channels(t_nhwc, segs):
    """[N,H,W,Cip] with padded segments -> NCHW tensor of the real channels, and the largest magnitude among the pad channels"""
    parts, pads, off = [], 0.0, 0
    for real, padded in segs:
        parts.append(t_nhwc[..., off:off + real])
        if padded > real:
            pads = max(pads, float(t_nhwc[..., off + real:off + padded].abs().max()))
        off += padded
    return torch.cat(parts, -1).permute(0, 3, 1, 2), pads


# ------------------------------------------------------------------------------------------------------
# the bound
# ------------------------------------------------------------------------------------------------------
def bound_of(ref64, mag, K, out_dtype):
    r_out = R_BF16 if out_dtype == 'bf16' else 0.0
    return r_out * ref64.abs() * (1 + R_BF16) + K * U_ACC * mag * (1 + r_out) + TINY


def bound_ratio(got, ref64, mag, K, out_dtype):
    """err / bound per element (float64)"""
    ref64, mag = ref64.detach().double().cpu(), mag.detach().double().cpu()
    err = (got.detach().double().cpu() - ref64).abs()
    return err / bound_of(ref64, mag, K, out_dtype)


def within_bound(name, got, ref64, mag, K, out_dtype):
    """-> (worst err / bound, failure message or None)"""
    assert tuple(got.shape) == tuple(ref64.shape), '%s: shape %s vs reference %s' % (name, tuple(got.shape), tuple(ref64.shape))
    ratio = bound_ratio(got, ref64, mag, K, out_dtype)
    bad = ~(ratio <= 1.0)            # (a NaN is a failure)
    worst = float(torch.nan_to_num(ratio, nan=float('inf')).max()) if ratio.numel() else 0.0
    if not bool(bad.any()):
        return worst, None
    return worst, '%s [%s]: %d/%d elements over the bound, worst err/bound %.3g, first bad idx %s' % (
        name, out_dtype, int(bad.sum()), bad.numel(), worst, bad.nonzero()[:4].tolist())


def assert_within_bound(name, got, ref64, mag, K, out_dtype):
    """assert |got - ref64| <= bound element by element; -> the worst err / bound (always, for the record)"""
    worst, msg = within_bound(name, got, ref64, mag, K, out_dtype)
    assert msg is None, msg
    return worst


# ------------------------------------------------------------------------------------------------------
# impulse probes
# ------------------------------------------------------------------------------------------------------
def _axis(n, k):
    """positions on an axis of n pixels, at least k apart, that include 0 and n - 1 (0 alone when n - 1 < k)"""
    if n - 1 < k:
        return [0]
    return list(range(0, n - k, k)) + [n - 1]


def impulse_passes(N, C, H, W, k):
    """number of launches until every one of C channels has carried an impulse"""
    P = N * len(_axis(H, k)) * len(_axis(W, k))
    return (C + P - 1) // P


def impulse_tensor(N, C, H, W, k, pas):
    """[N,C,H,W], zero but for impulses 2^j, j cycling over -2..2, on a grid of Chebyshev spacing >= k that includes rows and
    columns 0 and H-1 / W-1 of every image; the i-th grid position (over the whole batch) carries its impulse in channel
    (i + pas * P) mod C, P the number of positions: any k x k window holds at most one impulse."""
    rows, cols = _axis(H, k), _axis(W, k)
    t = torch.zeros(N, C, H, W)
    P = N * len(rows) * len(cols)
    i = 0
    for n in range(N):
        for r in rows:
            for c in cols:
                t[n, (i + pas * P) % C, r, c] = 2.0 ** ((i + pas) % 5 - 2)
                i += 1
    return t


def seam_pixels(N, H, W):
    """pixels (n, r, c) where a weight-gradient kernel's pixel loop can go wrong: the corners and borders of the first and last
    image, the last (ragged) row's segments, both sides of every 16 / 32 / 64-column strip seam and 8 / 16-row seam, and both
    sides of the 64- and 256-pixel seams of the flattened batch"""
    out, seen = [], set()

    def add(n, r, c):
        if 0 <= n < N and 0 <= r < H and 0 <= c < W and (n, r, c) not in seen:
            seen.add((n, r, c))
            out.append((n, r, c))

    cs = [0, 1, W - 2, W - 1] + [c + d for c in range(16, W, 16) for d in (-1, 0)]
    rs = [0, 1, H - 2, H - 1] + [r + d for r in range(8, H, 8) for d in (-1, 0)]
    for n in (0, N - 1):
        for r in (0, H - 1):
            for c in cs:
                add(n, r, c)
        for r in rs:
            for c in (0, W - 1):
                add(n, r, c)
    for j, r in enumerate(rs):
        for i, c in enumerate(cs):
            add((i + j) % N, r, c)
    for step in (64, 256):
        for lin in range(step, N * H * W, step):
            for d in (-1, 0):
                n, rem = divmod(lin + d, H * W)
                add(n, rem // W, rem % W)
    return out


def essential_pixels(N, H, W):
    """one representative (both sides, where it is a seam) of every class of seam_pixels, spread over the first, a middle and the
    last image: what even a 3-channel probe must reach.  Corners; the seam between two images; the start and the end of the
    last row's ragged 16-column segment in the last image; both sides of the 16 / 32 / 64-column seams; both sides of the 8 /
    16-row seams; both sides of the first and the last 64- and 256-pixel seam of the flattened batch."""
    out = []

    def add(n, r, c):
        if 0 <= n < N and 0 <= r < H and 0 <= c < W and (n, r, c) not in out:
            out.append((n, r, c))

    last, mid = N - 1, N // 2
    for n, r, c in ((0, 0, 0), (last, H - 1, W - 1), (0, H - 1, 0), (last, 0, W - 1), (0, H - 1, W - 1), (1, 0, 0)):
        add(n, r, c)
    c0 = 16 * ((W - 1) // 16)
    if c0 > 0:
        add(last, H - 1, c0 - 1)
        add(last, H - 1, c0)
    for j, seam in enumerate((16, 32, 64)):
        if W > seam:
            add((mid, last, 0)[j], (H // 2, H - 1, 0)[j], seam - 1)
            add((mid, last, 0)[j], (H // 2, H - 1, 0)[j], seam)
    for j, seam in enumerate((8, 16)):
        if H > seam:
            add((last, mid)[j], seam - 1, (W // 2, W - 1)[j])
            add((last, mid)[j], seam, (W // 2, W - 1)[j])
    for step in (64, 256):
        seams = list(range(step, N * H * W, step))
        for lin in seams[:1] + seams[-1:]:
            for d in (-1, 0):
                n, rem = divmod(lin + d, H * W)
                add(n, rem // W, rem % W)
    return out


def wgrad_probe_pixels(N, C, H, W):
    """the pixels the weight-gradient probe places, C per pass: essential_pixels first -- as many passes as they need, however few
    the channels -- then an even sample of the rest of seam_pixels up to 4 passes"""
    ess = essential_pixels(N, H, W)
    rest = [q for q in seam_pixels(N, H, W) if q not in ess]
    npass = max((len(ess) + C - 1) // C, min(4, (len(ess) + len(rest) + C - 1) // C))
    want = npass * C - len(ess)
    if want >= len(rest):
        return ess + rest
    return ess + [rest[i * len(rest) // want] for i in range(want)]


def wgrad_probe_passes(N, C, H, W):
    return (len(wgrad_probe_pixels(N, C, H, W)) + C - 1) // C


def wgrad_probe_tensor(N, C, H, W, pas):
    """[N,C,H,W] with exactly one non-zero pixel per channel, 2^j (j cycling over -2..2), at wgrad_probe_pixels()[c + pas * C]
    (wrapping round at the end): every element of the weight gradient is then one product, or zero where the tap falls outside"""
    px = wgrad_probe_pixels(N, C, H, W)
    t = torch.zeros(N, C, H, W)
    for c in range(C):
        n, r, q = px[(c + pas * C) % len(px)]
        t[n, c, r, q] = 2.0 ** ((c + pas) % 5 - 2)
    return t


def products_per_element(x, dy, w_shape, stride, pad, transposed):
    """how many non-zero products reach each element of y, dx and dW when x and dy are non-zero where given (weights all
    non-zero): the convolution of the 0/1 indicators with all-ones weights -> (max over y, max over dx, max over dW)"""
    ix, idy = (x != 0).double(), (dy != 0).double()
    y, _, dW = _three(ix, torch.ones(w_shape), None, torch.ones_like(idy), stride, pad, transposed)
    _, dx, _ = _three(torch.ones_like(ix), torch.ones(w_shape), None, idy, stride, pad, transposed)
    return float(y.max()), float(dx.max()), float(dW.max())


def impulse_expect_y(x, w, b, stride, pad, transposed, out_dtype):
    """y of a forward whose every output is at most one product: round_out(fp32(w * 2^j) + b), one fp32 addition"""
    prod = _conv64(x.double(), w.double(), None, stride, pad, transposed)
    assert torch.equal(prod.float().double(), prod), 'the single products must be exact in fp32'
    return round_out(prod.float() + b.float()[None, :, None, None], out_dtype)


def impulse_expect_dx(x_like, w, dy, stride, pad, transposed, out_dtype):
    _, dx, _ = _three(torch.zeros_like(x_like), w, None, dy, stride, pad, transposed)
    assert torch.equal(dx.float().double(), dx)
    return round_out(dx.float(), out_dtype)


def wgrad_expect(x, w_like, dy, stride, pad, transposed):
    _, _, dW = _three(x, torch.zeros_like(w_like), None, dy, stride, pad, transposed)
    assert torch.equal(dW.float().double(), dW)
    return dW.float()


def mismatches(name, got, want):
    """value equality (-0.0 == 0.0) -> failure message or None"""
    assert tuple(got.shape) == tuple(want.shape), '%s: shape %s vs %s' % (name, tuple(got.shape), tuple(want.shape))
    bad = ~(got.float().cpu() == want.float().cpu())
    if not bool(bad.any()):
        return None
    idx = bad.nonzero()[:4].tolist()
    return '%s: %d/%d elements differ, first idx %s got %s want %s' % (
        name, int(bad.sum()), bad.numel(), idx, [float(got[tuple(i)]) for i in idx], [float(want[tuple(i)]) for i in idx])
