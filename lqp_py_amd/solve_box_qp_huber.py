"""The box-QP layer with a Huber term in the objective:

    x* = argmin_x 0.5 x^T Q x + p^T x + sum_i w_i H_{delta_i}(x_i - c_i)   s.t.  A x = b,  lb <= x <= ub
    H_delta(d) = 0.5 d^2 for |d| <= delta,   delta |d| - 0.5 delta^2 beyond;      w >= 0 finite, delta >= 0 (+inf allowed), c finite

-- a robust tracking / regression penalty (``Q = X'X`` with bounded coefficients, outliers taken linearly), a trade cost that is
quadratic for small trades and linear for large ones.  A pure quadratic ``0.5 w (x - c)^2`` can be folded into Q and p by the
caller; Huber cannot, because where the curvature acts depends on the solution.  In ADMM the term is one more separable piece of the
z-update (shrink towards c by t / (1 + t) inside the quadratic zone, shift by t delta beyond, then the clamp); x-update,
factorisations, stopping rule and rho adaptation are ``torch_solve_box_qp``'s.  Everything numeric runs in the HIP library
(``lqp_boxqp_forward_huber``, ``lqp_boxqp_backward_fp_curv`` between the two element-wise kernels
``lqp_boxqp_huber_effective_duals`` / ``lqp_boxqp_huber_finish_grads``; include/lqp_amd.h).

The solve always takes the loop schedule: bounds that are all infinite are an ordinary case, ``control['rho']`` is never written
to, the rho = 0 one-shot is never chosen.  ``alpha``, ``sync=False``, ``linsolve``, ``launch_mode`` and per-problem ``rho`` /
``beta`` work as in the plain layer; what does not is refused by ``check_huber``.
"""
import torch
import torch.nn as nn

from . import _lib
from . import _terms as _T
from . import solve_box_qp_admm_torch as _S


def check_huber(control, Q=None, p=None, w=None, c=None, delta=None):
    """What the Huber layer cannot be combined with, and the shapes and dtypes of w, c, delta (``_terms.check_term``)."""
    _T.check_term(_T.HUBER, control, p, (w, c, delta))


def torch_solve_box_qp_huber(Q, p, A, b, lb, ub, w, c, delta, control):
    """Forward solve; returns torch_solve_box_qp's dict {"x","z","u","lams","nus","rho","iter"} and
      "zone"   (B,n,1): +1 / -1 on the upper / lower linear piece, 0 on the quadratic zone and wherever w = 0;
      "u_box"  (B,n,1): the box's share of the dual u, u - w clip(z - c, -delta, delta) / rho on an element a bound holds, zero
               elsewhere;
    "lams" is built from u_box."""
    return _T.solve(_T.HUBER, (Q, p, A, b, lb, ub), (w, c, delta), control)


class SolveBoxQPHuber(nn.Module):
    """nn.Module holding the control dict: SolveBoxQPHuber(control)(Q, p, A, b, lb, ub, w, c, delta) -> x, differentiable in all nine."""

    def __init__(self, control):
        super().__init__()
        self.control = control

    def forward(self, Q, p, A, b, lb, ub, w, c, delta):
        return SolveBoxQPHuberLayer.apply(Q, p, A, b, lb, ub, w, c, delta, self.control)


class SolveBoxQPHuberLayer(torch.autograd.Function):
    """ADMM forward with the Huber step / fixed-point implicit backward with the term's curvature on the quadratic zone.

    The term is C1: it has no kink sets, so the backward runs on the true box -- ``lqp_boxqp_backward_fp_curv`` with the dual
    u_e = u_box (the clamped set is where the BOX pushes) and curv = w on the free elements of the quadratic zone; on a linear
    piece the term is a constant force, p shifted by +-w delta.  Then dw = dp clip(z - c, -delta, delta), dc = -w dp on zone 0 and
    ddelta = w zone dp.  A plain call at `backward` time."""

    @staticmethod
    def forward(ctx, Q, p, A, b, lb, ub, w, c, delta, control):
        return _T.layer_forward(ctx, _T.HUBER, (Q, p, A, b, lb, ub), (w, c, delta), control, ('x', 'z', 'u_box', 'zone', 'nus'),
                                (Q, A, lb, ub, w, c, delta))

    @staticmethod
    def backward(ctx, dl_dz):
        x, z, u_box, zone, nus, Q, A, lb, ub, w, c, delta = ctx.saved_tensors
        h = _T.backward_prelude(ctx, x, Q, A)
        need, lib, B, n = h.need, h.lib, h.B, h.n
        u_e = torch.empty((B, n, 1), dtype=h.dty, device=h.dev)
        curv = torch.empty((B, n, 1), dtype=h.dty, device=h.dev)
        lams_e = torch.empty((B, 2 * n, 1), dtype=h.dty, device=h.dev)
        wc = _lib.norm(w, h.dty)
        with _lib.on_device(h.dev):
            _lib.check(lib.lqp_boxqp_huber_effective_duals(h.stream, h.dt, B, n, _lib.ptr(u_box), _lib.ptr(zone), _lib.ptr(wc), h.rho_mode,
                                                           h.rho_value, _lib.ptr(h.rho_tensor), _lib.ptr(u_e), _lib.ptr(lams_e), _lib.ptr(curv)),
                       "huber_effective_duals")
        dQ, dp, dA, db, dlb, dub, _ = _S._fp_backward(dl_dz, x, u_e, lams_e, nus, Q, A, lb, ub, ctx.rho, h.want, sync=ctx.sync,
                                                      linsolve=ctx.linsolve, curv=curv)
        dw, dc, dd = (torch.empty_like(dp) if need[k] else None for k in (6, 7, 8))
        if dw is not None or dc is not None or dd is not None:
            cc, dlc = _lib.norm(c, h.dty), _lib.norm(delta, h.dty)
            with _lib.on_device(h.dev):
                _lib.check(lib.lqp_boxqp_huber_finish_grads(h.stream, h.dt, B, n, _lib.ptr(dp), _lib.ptr(z), _lib.ptr(zone), _lib.ptr(wc),
                                                            _lib.ptr(cc), _lib.ptr(dlc), _lib.ptr(dw), _lib.ptr(dc), _lib.ptr(dd)),
                           "huber_finish_grads")
        return (dQ, dp if need[1] else None, dA, db, dlb, dub, dw, dc, dd, None)
