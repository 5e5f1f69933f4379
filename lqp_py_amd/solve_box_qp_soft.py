"""The box-QP layer with a soft band in the objective:

    x* = argmin_x 0.5 x^T Q x + p^T x + sum_i [ wl_i (lo_i - x_i)_+ + wu_i (x_i - hi_i)_+ ]   s.t.  A x = b,  lb <= x <= ub,
    wl, wu >= 0 and finite,  lo <= hi (lo may be -inf, hi may be +inf)

-- soft position limits inside the hard box, a no-cost band around yesterday's holdings, a one-sided hinge (a borrow fee),
asymmetric costs; ``lo = hi = c``, ``wl = wu = w`` is the L1 layer.  In ADMM the term is one more separable piece of the z-update
(the band's prox, two thresholds and two kinks, then the clamp); x-update, factorisations, stopping rule and rho adaptation are
``torch_solve_box_qp``'s.  Everything numeric runs in the HIP library (``lqp_boxqp_forward_soft``, the two element-wise kernels
``lqp_boxqp_soft_effective_box`` / ``lqp_boxqp_soft_finish_grads`` around ``lqp_boxqp_backward_fp``; include/lqp_amd.h).

The solve always takes the loop schedule: bounds that are all infinite are an ordinary case, ``control['rho']`` is never written
to, the rho = 0 one-shot is never chosen.  ``alpha``, ``sync=False``, ``linsolve``, ``launch_mode`` and per-problem ``rho`` /
``beta`` work as in the plain layer; what does not is refused by ``check_soft``.
"""
import torch
import torch.nn as nn

from . import _lib
from . import _terms as _T
from . import solve_box_qp_admm_torch as _S


def check_soft(control, Q=None, p=None, wl=None, wu=None, lo=None, hi=None):
    """What the soft-band layer cannot be combined with, and the shapes and dtypes of wl, wu, lo and hi (``_terms.check_term``)."""
    _T.check_term(_T.SOFT, control, p, (wl, wu, lo, hi))


def torch_solve_box_qp_soft(Q, p, A, b, lb, ub, wl, wu, lo, hi, control):
    """Forward solve; returns torch_solve_box_qp's dict {"x","z","u","lams","nus","rho","iter"} and
      "zone"   (B,n,1): +2 / -2 where x_i rests above hi_i / below lo_i (or is pushed there by a bound), +1 / -1 exactly on the kink
                        x_i = hi_i / x_i = lo_i (only where that side's weight is positive), 0 inside the band
      "u_box"  (B,n,1): the box's share of the dual u -- zero unless the element is clamped at a bound;
    "lams" is built from u_box (the rest of u is the band's multiplier, -wl <= rho (u - u_box) <= wu)."""
    return _T.solve(_T.SOFT, (Q, p, A, b, lb, ub), (wl, wu, lo, hi), control)


class SolveBoxQPSoft(nn.Module):
    """nn.Module holding the control dict: SolveBoxQPSoft(control)(Q, p, A, b, lb, ub, wl, wu, lo, hi) -> x, differentiable in all ten."""

    def __init__(self, control):
        super().__init__()
        self.control = control

    def forward(self, Q, p, A, b, lb, ub, wl, wu, lo, hi):
        return SolveBoxQPSoftLayer.apply(Q, p, A, b, lb, ub, wl, wu, lo, hi, self.control)


class SolveBoxQPSoftLayer(torch.autograd.Function):
    """ADMM forward with the soft band's step / fixed-point implicit backward on the effective box.

    An element on a kink (zone = +-1, and not held by a hard bound: u_box == 0) behaves exactly like one whose two bounds are both
    that kink; a free element on a sloped piece
    (zone = +-2) like p_i shifted by wu_i / -wl_i.  So the backward is ``lqp_boxqp_backward_fp``, unchanged, on
    (lb_e, ub_e) = K ? (kink, kink) : (lb, ub) with the dual u_e = K ? u : u_box, and then dlb, dub = 0 on K, dhi / dlo = dlb_e + dub_e on
    their kink sets, dwu = dp on zone == +2, dwl = -dp on zone == -2.  A plain call at `backward` time."""

    @staticmethod
    def forward(ctx, Q, p, A, b, lb, ub, wl, wu, lo, hi, control):
        return _T.layer_forward(ctx, _T.SOFT, (Q, p, A, b, lb, ub), (wl, wu, lo, hi), control, ('x', 'u', 'u_box', 'zone', 'nus'),
                                (Q, A, lb, ub, lo, hi))

    @staticmethod
    def backward(ctx, dl_dz):
        x, u, u_box, zone, nus, Q, A, lb, ub, lo, hi = ctx.saved_tensors
        h = _T.backward_prelude(ctx, x, Q, A, box_grads=True)
        need, lib, B, n = h.need, h.lib, h.B, h.n
        lbc, ubc, loc, hic = (_lib.norm(t, h.dty) for t in (lb, ub, lo, hi))
        lb_e, ub_e, u_e = (torch.empty((B, n, 1), dtype=h.dty, device=h.dev) for _ in range(3))
        lams_e = torch.empty((B, 2 * n, 1), dtype=h.dty, device=h.dev)
        with _lib.on_device(h.dev):
            _lib.check(lib.lqp_boxqp_soft_effective_box(h.stream, h.dt, B, n, _lib.ptr(zone), _lib.ptr(u), _lib.ptr(u_box), _lib.ptr(lbc),
                                                        _lib.ptr(ubc), _lib.ptr(loc), _lib.ptr(hic), h.rho_mode, h.rho_value,
                                                        _lib.ptr(h.rho_tensor), _lib.ptr(lb_e), _lib.ptr(ub_e), _lib.ptr(u_e),
                                                        _lib.ptr(lams_e)), "soft_effective_box")
        dQ, dp, dA, db, dlb, dub, _ = _S._fp_backward(dl_dz, x, u_e, lams_e, nus, Q, A, lb_e, ub_e, ctx.rho, h.want, sync=ctx.sync,
                                                      linsolve=ctx.linsolve)
        dwl, dwu, dlo, dhi = (torch.empty_like(dp) if need[k] else None for k in (6, 7, 8, 9))
        with _lib.on_device(h.dev):
            _lib.check(lib.lqp_boxqp_soft_finish_grads(h.stream, h.dt, B, n, _lib.ptr(zone), _lib.ptr(u_box), _lib.ptr(dp), _lib.ptr(dlb), _lib.ptr(dub),
                                                       _lib.ptr(dlb), _lib.ptr(dub), _lib.ptr(dwl), _lib.ptr(dwu), _lib.ptr(dlo),
                                                       _lib.ptr(dhi)), "soft_finish_grads")
        return (dQ, dp if need[1] else None, dA, db, dlb if need[4] else None, dub if need[5] else None, dwl, dwu, dlo, dhi, None)
