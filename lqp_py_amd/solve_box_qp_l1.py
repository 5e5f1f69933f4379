"""The box-QP layer with an L1 term in the objective:

    x* = argmin_x 0.5 x^T Q x + p^T x + sum_i w_i |x_i - c_i|   s.t.  A x = b,  lb <= x <= ub,     w >= 0, c finite

-- turnover or transaction cost around yesterday's holdings c, without doubling the variables.  In ADMM the term is one more
separable piece of the z-update (soft-threshold around c, then clamp); x-update, factorisations, stopping rule and rho adaptation
are ``torch_solve_box_qp``'s.  Everything numeric runs in the HIP library (``lqp_boxqp_forward_l1``, the two element-wise kernels
``lqp_boxqp_l1_effective_box`` / ``lqp_boxqp_l1_finish_grads`` around ``lqp_boxqp_backward_fp``; include/lqp_amd.h).

The solve always takes the loop schedule: bounds that are all infinite are an ordinary case, ``control['rho']`` is never written
to, the rho = 0 one-shot is never chosen.  ``alpha``, ``sync=False``, ``linsolve``, ``launch_mode`` and per-problem ``rho`` /
``beta`` work as in the plain layer; what does not is refused by ``check_l1``.
"""
import torch
import torch.nn as nn

from . import _lib
from . import _terms as _T
from . import solve_box_qp_admm_torch as _S


def check_l1(control, Q=None, p=None, w=None, c=None):
    """What the L1 layer cannot be combined with, and the shapes and dtypes of w and c (``_terms.check_term``)."""
    _T.check_term(_T.L1, control, p, (w, c))


def torch_solve_box_qp_l1(Q, p, A, b, lb, ub, w, c, control):
    """Forward solve; returns torch_solve_box_qp's dict {"x","z","u","lams","nus","rho","iter"} and
      "side"   (B,n,1): +1 / -1 where x_i rests above / below c_i or is pushed there by a bound, 0 exactly on the kink x_i = c_i
      "u_box"  (B,n,1): the box's share of the dual u -- zero unless the element is clamped at a bound;
    "lams" is built from u_box (the rest of u is the L1 term's multiplier, |rho (u - u_box)| <= w)."""
    return _T.solve(_T.L1, (Q, p, A, b, lb, ub), (w, c), control)


class SolveBoxQPL1(nn.Module):
    """nn.Module holding the control dict: SolveBoxQPL1(control)(Q, p, A, b, lb, ub, w, c) -> x, differentiable in all eight."""

    def __init__(self, control):
        super().__init__()
        self.control = control

    def forward(self, Q, p, A, b, lb, ub, w, c):
        return SolveBoxQPL1Layer.apply(Q, p, A, b, lb, ub, w, c, self.control)


class SolveBoxQPL1Layer(torch.autograd.Function):
    """ADMM forward with the L1 step / fixed-point implicit backward on the effective box.

    An element on the kink behaves exactly like one whose two bounds are both c_i; a thresholded free element like p_i shifted by
    side_i w_i.  So the backward is ``lqp_boxqp_backward_fp``, unchanged, on (lb_e, ub_e) = K ? (c, c) : (lb, ub) with the dual
    u_e = K ? u : u_box, and then dlb, dub = 0 on K, dc = dlb_e + dub_e on K (0 elsewhere), dw = side * dp.  A plain call at
    `backward` time: nothing of it runs ahead of the cotangent."""

    @staticmethod
    def forward(ctx, Q, p, A, b, lb, ub, w, c, control):
        return _T.layer_forward(ctx, _T.L1, (Q, p, A, b, lb, ub), (w, c), control, ('x', 'u', 'u_box', 'side', 'nus'), (Q, A, lb, ub, c))

    @staticmethod
    def backward(ctx, dl_dz):
        x, u, u_box, side, nus, Q, A, lb, ub, c = ctx.saved_tensors
        h = _T.backward_prelude(ctx, x, Q, A, box_grads=True)
        need, lib, B, n = h.need, h.lib, h.B, h.n
        lbc, ubc, cc = (_lib.norm(t, h.dty) for t in (lb, ub, c))
        lb_e, ub_e, u_e = (torch.empty((B, n, 1), dtype=h.dty, device=h.dev) for _ in range(3))
        lams_e = torch.empty((B, 2 * n, 1), dtype=h.dty, device=h.dev)
        with _lib.on_device(h.dev):
            _lib.check(lib.lqp_boxqp_l1_effective_box(h.stream, h.dt, B, n, _lib.ptr(side), _lib.ptr(u), _lib.ptr(u_box), _lib.ptr(lbc),
                                                      _lib.ptr(ubc), _lib.ptr(cc), h.rho_mode, h.rho_value, _lib.ptr(h.rho_tensor),
                                                      _lib.ptr(lb_e), _lib.ptr(ub_e), _lib.ptr(u_e), _lib.ptr(lams_e)), "l1_effective_box")
        dQ, dp, dA, db, dlb, dub, _ = _S._fp_backward(dl_dz, x, u_e, lams_e, nus, Q, A, lb_e, ub_e, ctx.rho, h.want, sync=ctx.sync,
                                                      linsolve=ctx.linsolve)
        dc = torch.empty_like(dp) if need[7] else None
        dw = torch.empty_like(dp) if need[6] else None
        with _lib.on_device(h.dev):
            _lib.check(lib.lqp_boxqp_l1_finish_grads(h.stream, h.dt, B, n, _lib.ptr(side), _lib.ptr(dp), _lib.ptr(dlb), _lib.ptr(dub),
                                                     _lib.ptr(dlb), _lib.ptr(dub), _lib.ptr(dc), _lib.ptr(dw)), "l1_finish_grads")
        return (dQ, dp if need[1] else None, dA, db, dlb if need[4] else None, dub if need[5] else None, dw, dc, None)
