"""The box-QP layer with a logarithmic barrier in the objective:

    x* = argmin_x 0.5 x^T Q x + p^T x - sum_i w_i log(x_i)   s.t.  A x = b,  lb <= x <= ub,    w >= 0 and finite

-- risk budgeting (risk parity with ``Q = Sigma``, ``w`` the budgets), a long-only barrier that keeps holdings off zero, Kelly /
log-utility terms.  In ADMM the term is one more separable piece of the z-update (the positive root of S^2 - v S - w / rho = 0,
then the clamp); x-update, factorisations, stopping rule and rho adaptation are ``torch_solve_box_qp``'s.  Everything numeric
runs in the HIP library (``lqp_boxqp_forward_log``, ``lqp_boxqp_backward_fp_curv`` between the two element-wise kernels
``lqp_boxqp_log_effective_duals`` / ``lqp_boxqp_log_finish_grads``; include/lqp_amd.h).

The solve always takes the loop schedule: bounds that are all infinite are an ordinary case, ``control['rho']`` is never written
to, the rho = 0 one-shot is never chosen.  ``alpha``, ``sync=False``, ``linsolve``, ``launch_mode`` and per-problem ``rho`` /
``beta`` work as in the plain layer; what does not is refused by ``check_log``.
"""
import torch
import torch.nn as nn

from . import _lib
from . import _terms as _T
from . import solve_box_qp_admm_torch as _S


def check_log(control, Q=None, p=None, w=None):
    """What the log-barrier layer cannot be combined with, and the shape and dtype of w (``_terms.check_term``)."""
    _T.check_term(_T.LOG, control, p, (w,))


def torch_solve_box_qp_log(Q, p, A, b, lb, ub, w, control):
    """Forward solve; returns torch_solve_box_qp's dict {"x","z","u","lams","nus","rho","iter"} and
      "u_box"  (B,n,1): the box's share of the dual u, rho u + w / z over rho on an element a bound holds, zero elsewhere;
      "curv"   (B,n,1): w_i / z_i^2 on the free barrier elements (w_i > 0, u_box_i == 0), zero elsewhere -- the barrier's Hessian;
    "lams" is built from u_box."""
    return _T.solve(_T.LOG, (Q, p, A, b, lb, ub), (w,), control)


class SolveBoxQPLog(nn.Module):
    """nn.Module holding the control dict: SolveBoxQPLog(control)(Q, p, A, b, lb, ub, w) -> x, differentiable in all seven."""

    def __init__(self, control):
        super().__init__()
        self.control = control

    def forward(self, Q, p, A, b, lb, ub, w):
        return SolveBoxQPLogLayer.apply(Q, p, A, b, lb, ub, w, self.control)


class SolveBoxQPLogLayer(torch.autograd.Function):
    """ADMM forward with the barrier's step / fixed-point implicit backward with the barrier's curvature.

    The barrier is smooth: on the free set the stationarity condition carries its Hessian diag(w_i / x_i^2), so the backward is
    ``lqp_boxqp_backward_fp_curv`` on the true box with the dual u_e = u_box (the clamped set is where the BOX pushes) and
    ``curv`` on the diagonal of the free-set block; then dw_i = -dp_i / z_i where w_i > 0, else 0.  A plain call at `backward`
    time."""

    @staticmethod
    def forward(ctx, Q, p, A, b, lb, ub, w, control):
        return _T.layer_forward(ctx, _T.LOG, (Q, p, A, b, lb, ub), (w,), control, ('x', 'z', 'u_box', 'curv', 'nus'), (Q, A, lb, ub, w))

    @staticmethod
    def backward(ctx, dl_dz):
        x, z, u_box, curv, nus, Q, A, lb, ub, w = ctx.saved_tensors
        h = _T.backward_prelude(ctx, x, Q, A)
        need, lib, B, n = h.need, h.lib, h.B, h.n
        u_e = torch.empty((B, n, 1), dtype=h.dty, device=h.dev)
        lams_e = torch.empty((B, 2 * n, 1), dtype=h.dty, device=h.dev)
        with _lib.on_device(h.dev):
            _lib.check(lib.lqp_boxqp_log_effective_duals(h.stream, h.dt, B, n, _lib.ptr(u_box), h.rho_mode, h.rho_value, _lib.ptr(h.rho_tensor),
                                                         _lib.ptr(u_e), _lib.ptr(lams_e)), "log_effective_duals")
        dQ, dp, dA, db, dlb, dub, _ = _S._fp_backward(dl_dz, x, u_e, lams_e, nus, Q, A, lb, ub, ctx.rho, h.want, sync=ctx.sync,
                                                      linsolve=ctx.linsolve, curv=curv)
        dw = torch.empty_like(dp) if need[6] else None
        if dw is not None:
            wc = _lib.norm(w, h.dty)
            with _lib.on_device(h.dev):
                _lib.check(lib.lqp_boxqp_log_finish_grads(h.stream, h.dt, B, n, _lib.ptr(dp), _lib.ptr(z), _lib.ptr(wc), _lib.ptr(dw)),
                           "log_finish_grads")
        return (dQ, dp if need[1] else None, dA, db, dlb, dub, dw, None)
