"""Dense operands for the BatchNorm passes (helper module: no fixtures, no pytest settings): the cases of
tests/test_ew_errbound_cpu.py and tests/test_ew_errbound_gpu.py.

Multiples of 1/4 (tests/ew_table.py) cannot show a loss of precision, so the statistics pass, finalize + activation, the
backward reduction and finalize + apply also run on normally distributed operands, on the five ew_table.SHAPES, in both dtypes:
operands are round(randn * 2 + 0.5) in the storage type; on f32 every shape has one ill-conditioned variant, y = 100 + 0.1 *
randn, which a cancelling formulation of z fails.  The statistics handed to a finalize are the float64 sums of the operands as
stored; the coefficients handed to a pass are the oracle's own (tests/ew_oracle.py), so no stage is charged with the rounding
of the one before it.  A case is a function of (Run, operands) that makes the calls and returns its output buffers, as the rows
of ew_table do; the same function runs under the oracle, the emulator and the library.
"""
import functools

import torch

import ew_oracle as eo
import ew_table as ew
from ew_table import EPS, MOM, SENTINEL, SLOPE, L, P, pad8

# name, source set, residual, dz stored, second same-size source (reduce_add): every combination ew_table.ROWS uses
REDUCE_FORMS = ([('src%d' % k, k, False, True, False) for k in range(1, 8)] +
                [('src%d_res' % k, k, True, True, False) for k in (1, 4, 5)] +
                [('src%d_nodz' % k, k, False, False, False) for k in (1, 3)] +
                [('add', 1, False, True, True), ('add_res', 1, True, True, True)])
ROWS = ['stats', 'fwd', 'fused'] + ['reduce_' + f[0] for f in REDUCE_FORMS] + ['apply', 'apply_fused', 'apply_fused_src']
VARIANTS = [('bf16', False), ('f32', False), ('f32', True)]
CASES = ['%s/s%d:%s%s' % (row, i, dt, '_ill' if ill else '') for row in ROWS for i in range(len(ew.SHAPES)) for dt, ill in VARIANTS]


class Ops(object):
    pass


def vb(r, npix, Cp, t=None):
    """a [pixels][Cp] view with row stride Cp + 8 of a sentinel-filled buffer holding t"""
    buf = torch.full((npix, Cp + 8), SENTINEL, dtype=r.td)
    if t is not None:
        buf[:, :Cp] = t.to(r.td)
    return ew.V(buf.to(r.dev), Cp + 8)


def dev(r, t):
    return None if t is None else t.clone().to(r.dev)


@functools.lru_cache(maxsize=None)
def operands(i, dt, ill):
    s = ew.SHAPES[i]
    N, H, W, C, act, pool, up, drop = s
    Cp, npix = pad8(C), N * H * W
    gen = torch.Generator().manual_seed(7000 + 10 * i + int(ill))
    td = torch.bfloat16 if dt == 'bf16' else torch.float32
    o = Ops()
    o.s, o.dt, o.Cp, o.npix = s, dt, Cp, npix

    def dense(n, ill_=False):
        t = torch.randn(n, Cp, generator=gen)
        t = (100 + 0.1 * t) if ill_ else (t * 2 + 0.5)
        t[:, C:] = 0
        return t.to(td)

    o.y, o.res = dense(npix, ill), dense(npix)
    o.gd, o.ga = dense(npix), dense(npix)
    o.gp, o.gu = dense(N * (H // 2) * (W // 2)), dense(4 * npix)
    o.dm = (torch.randint(0, 2, (N, Cp), generator=gen).float() * 2) if drop else None
    o.gamma, o.beta = 0.5 + torch.rand(C, generator=gen), torch.randn(C, generator=gen)
    o.rm, o.rv = torch.randn(C, generator=gen), 0.5 + torch.rand(C, generator=gen)
    o.dgamma, o.dbeta = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    y64 = o.y.double()
    o.stats = torch.zeros(16, 2, Cp, dtype=torch.float64)               # the float64 sums of the operand as stored
    o.stats[3, 0], o.stats[11, 1] = y64.sum(0), (y64 * y64).sum(0)
    # the oracle's own coefficients
    orc = eo.Oracle()
    st, o.coef = o.stats.clone(), torch.zeros(4, Cp)
    orc.segnb_bn_finalize(st.data_ptr(), C, Cp, float(npix), o.gamma.data_ptr(), o.beta.data_ptr(), EPS, MOM, None, None, None, 1,
                          o.coef.data_ptr(), None)
    # the oracle's dz of the direct source, its float64 sums, the oracle's bcoef
    r = ew.Run(dt, 'cpu')
    yb, gb, dzb = vb(r, npix, Cp, o.y), vb(r, npix, Cp, o.gd), vb(r, npix, Cp)
    orc.segnb_bn_act_bwd_reduce(r.code, yb.ptr, yb.ld, N, H, W, Cp, o.coef.data_ptr(), act, SLOPE, P(o.dm), gb.ptr, gb.ld, None, 0,
                                None, 0, dzb.ptr, dzb.ld, None, None, 0, None)
    o.dz = dzb.buf[:, :Cp].clone()
    dz64, co = o.dz.double(), o.coef.double()
    o.sums = torch.zeros(16, 2, Cp, dtype=torch.float64)
    o.sums[3, 0], o.sums[11, 1] = dz64.sum(0), (dz64 * ((y64 - co[2]) * co[3])).sum(0)
    sm, o.bcoef = o.sums.clone(), torch.zeros(3, Cp)
    orc.segnb_bn_bwd_finalize(sm.data_ptr(), C, Cp, float(npix), o.gamma.data_ptr(), o.coef.data_ptr(), o.bcoef.data_ptr(), None,
                              None, 0, None)
    return o


def _geo(o):
    N, H, W, C, act, pool, up, drop = o.s
    return N, H, W, C, o.Cp, act


def d_stats(r, o):
    N, H, W, C, Cp, _ = _geo(o)
    x, st = vb(r, o.npix, Cp, o.y), r.full((16, 2, Cp), 0.0, torch.float64)
    r.call('segnb_bn_stats', r.code, x.ptr, x.ld, N, H, W, Cp, P(st), None)
    return ew._outs(stats=st)


def _fwd_outputs(r, o):
    N, H, W, C, Cp, _ = _geo(o)
    po = vb(r, N * (H // 2) * (W // 2), Cp) if o.s[5] else None
    uo = vb(r, 4 * o.npix, Cp) if o.s[6] else None
    return vb(r, o.npix, Cp), po, uo


def d_fwd(r, o, coef=None):
    """segnb_bn_finalize on the float64 statistics, then segnb_bn_act_fwd under the coefficients given (the oracle's own)"""
    N, H, W, C, Cp, act = _geo(o)
    outs = {}
    if coef is None:
        st, co, gamma, beta, rm, rv = dev(r, o.stats), r.full((4, Cp), SENTINEL), dev(r, o.gamma), dev(r, o.beta), dev(r, o.rm), dev(r, o.rv)
        nbt = torch.full((1,), 3, dtype=torch.int64, device=r.dev)
        r.call('segnb_bn_finalize', P(st), C, Cp, float(o.npix), P(gamma), P(beta), EPS, MOM, P(rm), P(rv), P(nbt), 1, P(co), None)
        outs = dict(coef=co, running_mean=rm, running_var=rv, nbt=nbt, stats_in=st)
    y, cf, dm = vb(r, o.npix, Cp, o.y), dev(r, o.coef if coef is None else coef), dev(r, o.dm)
    out, po, uo = _fwd_outputs(r, o)
    r.call('segnb_bn_act_fwd', r.code, y.ptr, y.ld, N, H, W, Cp, P(cf), act, SLOPE, P(dm), out.ptr, out.ld, P(po), L(po), P(uo), L(uo),
           None, 0, None)
    return ew._outs(out=out, pool_out=po, up_out=uo, **outs)


def d_fused(r, o):
    N, H, W, C, Cp, act = _geo(o)
    st, co, gamma, beta, rm, rv = dev(r, o.stats), r.full((4, Cp), SENTINEL), dev(r, o.gamma), dev(r, o.beta), dev(r, o.rm), dev(r, o.rv)
    nbt, clear = torch.full((1,), 3, dtype=torch.int64, device=r.dev), r.full((16, 2, Cp), SENTINEL, torch.float64)
    y, dm = vb(r, o.npix, Cp, o.y), dev(r, o.dm)
    out, po, uo = _fwd_outputs(r, o)
    r.call('segnb_bn_fwd_fused', r.code, y.ptr, y.ld, N, H, W, C, Cp, P(st), P(gamma), P(beta), EPS, MOM, P(rm), P(rv), P(nbt), P(co),
           P(clear), act, SLOPE, P(dm), out.ptr, out.ld, P(po), L(po), P(uo), L(uo), None, 0, None)
    return ew._outs(out=out, pool_out=po, up_out=uo, coef=co, running_mean=rm, running_var=rv, nbt=nbt, cleared=clear, stats_in=st)


def _sources(r, o, src):
    N, H, W, C, Cp, _ = _geo(o)
    gd = vb(r, o.npix, Cp, o.gd) if src & 1 else None
    gp = vb(r, N * (H // 2) * (W // 2), Cp, o.gp) if src & 2 else None
    gu = vb(r, 4 * o.npix, Cp, o.gu) if src & 4 else None
    return gd, gp, gu


def d_reduce(r, o, form):
    _, src, res, store, second = form
    N, H, W, C, Cp, act = _geo(o)
    y, cf, dm = vb(r, o.npix, Cp, o.y), dev(r, o.coef), dev(r, o.dm)
    dz = vb(r, o.npix, Cp) if store else None
    rs = vb(r, o.npix, Cp, o.res) if res else None
    sums = r.full((16, 2, Cp), 0.0, torch.float64)
    if second:
        gd, ga = vb(r, o.npix, Cp, o.gd), vb(r, o.npix, Cp, o.ga)
        r.call('segnb_bn_act_bwd_reduce_add', r.code, y.ptr, y.ld, N, H, W, Cp, P(cf), act, SLOPE, P(dm), gd.ptr, gd.ld, ga.ptr, ga.ld,
               dz.ptr, dz.ld, P(sums), P(rs), L(rs), None)
    else:
        gd, gp, gu = _sources(r, o, src)
        r.call('segnb_bn_act_bwd_reduce', r.code, y.ptr, y.ld, N, H, W, Cp, P(cf), act, SLOPE, P(dm), P(gd), L(gd), P(gp), L(gp),
               P(gu), L(gu), P(dz), L(dz), P(sums), P(rs), L(rs), None)
    return ew._outs(dz=dz, sums=sums)


def _fused_args(r, o):
    N, H, W, C, Cp, _ = _geo(o)
    y, cf, sums, gamma = vb(r, o.npix, Cp, o.y), dev(r, o.coef), dev(r, o.sums), dev(r, o.gamma)
    bc, dg, db = r.full((3, Cp), SENTINEL), dev(r, o.dgamma), dev(r, o.dbeta)
    clear = r.full((16, 2, Cp), SENTINEL, torch.float64)
    args = (r.code, y.ptr, y.ld, N, H, W, C, Cp, P(cf), P(sums), P(gamma), P(bc), P(dg), P(db), 1, P(clear))
    return args, dict(bcoef=bc, dgamma=dg, dbeta=db, cleared=clear, y_in=y, coef_in=cf, sums_in=sums, gamma_in=gamma)


def d_apply(r, o):
    """segnb_bn_bwd_finalize on the float64 sums of the stored dz, then segnb_bn_bwd_apply under the oracle's bcoef"""
    N, H, W, C, Cp, _ = _geo(o)
    sums, cf, gamma = dev(r, o.sums), dev(r, o.coef), dev(r, o.gamma)
    bc, dg, db = r.full((3, Cp), SENTINEL), dev(r, o.dgamma), dev(r, o.dbeta)
    r.call('segnb_bn_bwd_finalize', P(sums), C, Cp, float(o.npix), P(gamma), P(cf), P(bc), P(dg), P(db), 1, None)
    y, dz, dy, bco, dbias = vb(r, o.npix, Cp, o.y), vb(r, o.npix, Cp, o.dz), vb(r, o.npix, Cp), dev(r, o.bcoef), r.full((C,), 0.0)
    r.call('segnb_bn_bwd_apply', r.code, y.ptr, y.ld, N, H, W, Cp, P(cf), P(bco), dz.ptr, dz.ld, dy.ptr, dy.ld, P(dbias), C, None)
    return ew._outs(dy=dy, dbias=dbias, bcoef=bc, dgamma=dg, dbeta=db, sums_in=sums)


def d_apply_fused(r, o):
    args, tables = _fused_args(r, o)
    dz, dy = vb(r, o.npix, o.Cp, o.dz), vb(r, o.npix, o.Cp)
    r.call('segnb_bn_bwd_apply_fused', *args, dz.ptr, dz.ld, dy.ptr, dy.ld, None)
    return ew._outs(dy=dy, **tables)


def d_apply_fused_src(r, o):
    """dz recomputed from the direct source (the one the sums were taken over)"""
    args, tables = _fused_args(r, o)
    act = o.s[4]
    gd, dy, dm = vb(r, o.npix, o.Cp, o.gd), vb(r, o.npix, o.Cp), dev(r, o.dm)
    r.call('segnb_bn_bwd_apply_fused_src', *args, act, SLOPE, P(dm), gd.ptr, gd.ld, None, 0, None, 0, dy.ptr, dy.ld, None)
    return ew._outs(dy=dy, **tables)


def parse(case):
    """-> (row name, function, arguments after the Run)"""
    head, var = case.rsplit(':', 1)
    row, sh = head.rsplit('/s', 1)
    o = operands(int(sh), var.split('_')[0], var.endswith('_ill'))
    if row.startswith('reduce_'):
        return row, d_reduce, (o, [f for f in REDUCE_FORMS if f[0] == row[len('reduce_'):]][0])
    return row, {'stats': d_stats, 'fwd': d_fwd, 'fused': d_fused, 'apply': d_apply, 'apply_fused': d_apply_fused,
                 'apply_fused_src': d_apply_fused_src}[row], (o,)


def run(case, device):
    _, fn, args = parse(case)
    outs = fn(ew.Run(case.rsplit(':', 1)[1].split('_')[0], device), *args)
    if torch.device(device).type == 'cuda':
        torch.cuda.synchronize()
    return outs


def stored_sums_failures(case, outs):
    """the sums of a reduction against the float64 sums of the dz THE RUN ITSELF stored (so the rounding of dz is not charged
    to the sums): |sum - sum64 dz| <= P U sum |dz|, and (P + 2) U invstd sum |dz (y - mean)| for the second -> messages"""
    row, _, args = parse(case)
    if not row.startswith('reduce_') or 'dz' not in outs:
        return []
    o = args[0]
    dz = outs['dz'].detach().cpu()[:, :o.Cp].double()
    got = outs['sums'].detach().cpu().sum(0)
    co, y = o.coef.double(), o.y.double()
    t = dz * (y - co[2])
    want = torch.stack([dz.sum(0), t.sum(0) * co[3]])
    lim = torch.stack([o.npix * eo.U * dz.abs().sum(0), (o.npix + 2) * eo.U * co[3].abs() * t.abs().sum(0)]) + eo.TINY
    bad = ~((got - want).abs() <= lim)
    return [] if not bool(bad.any()) else ['%s: sums of the stored dz: %d over the bound, worst %.3g' % (
        case, int(bad.sum()), float(((got - want).abs() / lim).max()))]
