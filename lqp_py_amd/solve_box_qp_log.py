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
import ctypes

import torch
import torch.nn as nn

from . import _lib
from . import solve_box_qp_admm_torch as _S
from .utils import get_ncon


def check_log(control, Q=None, p=None, w=None):
    """What the log-barrier layer cannot be combined with, and the shape and dtype of w.  Raises the package's ValueError at the
    call, before any launch; the one place that holds these rules."""
    if control.get('stop', 'all') != 'all':
        _S._bad("the log-barrier layer has no per-problem stop: control['stop'] = 'each' cannot be combined with it")
    for key in ('infeasible', 'unbounded'):
        if control.get(key) is not None:
            _S._bad(f"control['{key}'] cannot be combined with the log-barrier layer: the certificates belong to the per-problem stop")
    if control.get('unroll', False):
        _S._bad("unroll=True cannot be combined with the log-barrier layer: the tape replays the plain step")
    if control.get('backward', 'fixed_point') == 'kkt':
        _S._bad("control['backward'] = 'kkt' cannot be combined with the log-barrier layer: its backward is the fixed-point form with the barrier's curvature")
    if any(control.get(k) is not None for k in ('_global_bounds', '_bound_flags_dev', '_check_hook', '_owner')) or \
            control.get('dist_strict_stop', False):
        _S._bad("the sharded wrapper (lqp_py_amd.dist) does not carry the log-barrier layer")
    rho = control.get('rho')
    if rho is not None and not torch.is_tensor(rho) and not float(rho) > 0.0:
        _S._bad("control['rho'] must be positive (or None) for the log-barrier layer: it always iterates")
    if p is None:
        return
    if not torch.is_tensor(w) or tuple(w.shape) != tuple(p.shape):
        _S._bad(f"w must be a tensor of p's shape {tuple(p.shape)}")
    if w.dtype != p.dtype:
        _S._bad(f"w must have p's dtype {p.dtype}, got {w.dtype}")


def _solve(Q, p, A, b, lb, ub, w, control, sync=True):
    check_log(control, Q, p, w)
    _lib.require_gpu(w)
    # (bounds known = "some bound is finite": the loop schedule whatever the data hold; nothing is assumed, compared or remembered)
    return _S._forward_solve(Q, p, A, b, lb, ub, control, bounds=(True, True), sync=sync, log=(w,))


def torch_solve_box_qp_log(Q, p, A, b, lb, ub, w, control):
    """Forward solve; returns torch_solve_box_qp's dict {"x","z","u","lams","nus","rho","iter"} and
      "u_box"  (B,n,1): the box's share of the dual u, rho u + w / z over rho on an element a bound holds, zero elsewhere;
      "curv"   (B,n,1): w_i / z_i^2 on the free barrier elements (w_i > 0, u_box_i == 0), zero elsewhere -- the barrier's Hessian;
    "lams" is built from u_box."""
    return _solve(Q, p, A, b, lb, ub, w, control)


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
        sync = bool(control.get('sync', True))
        sol = _solve(Q, p, A, b, lb, ub, w, control, sync=sync)
        ctx.rho, ctx.sync = sol['rho'], sync
        ctx.linsolve = int(sol['_stats']['linsolve_used'])
        ctx.save_for_backward(sol['x'], sol['z'], sol['u_box'], sol['curv'], sol['nus'], Q, A, lb, ub, w)
        return sol['x']

    @staticmethod
    def backward(ctx, dl_dz):
        x, z, u_box, curv, nus, Q, A, lb, ub, w = ctx.saved_tensors
        need = ctx.needs_input_grad
        lib, B, n = _lib.load(), Q.shape[0], Q.shape[1]
        dt, dev, dty = _lib.dtype_code(x), x.device, x.dtype
        stream = ctypes.c_void_p(_lib.current_stream_handle(dev))
        rho_mode, rho_value, rho_tensor = _S._per_problem_argument('rho', '(B,1,1)', ctx.rho, B, x)
        u_e = torch.empty((B, n, 1), dtype=dty, device=dev)
        lams_e = torch.empty((B, 2 * n, 1), dtype=dty, device=dev)
        with _lib.on_device(dev):
            _lib.check(lib.lqp_boxqp_log_effective_duals(stream, dt, B, n, _lib.ptr(u_box), rho_mode, rho_value, _lib.ptr(rho_tensor),
                                                         _lib.ptr(u_e), _lib.ptr(lams_e)), "log_effective_duals")
        has_eq = get_ncon(A, dim=1) > 0
        want = dict(dQ=need[0], dp=True, dA=need[2] and has_eq, db=need[3] and has_eq, dlb=need[4], dub=need[5])
        dQ, dp, dA, db, dlb, dub, _ = _S._fp_backward(dl_dz, x, u_e, lams_e, nus, Q, A, lb, ub, ctx.rho, want, sync=ctx.sync,
                                                      linsolve=ctx.linsolve, curv=curv)
        dw = torch.empty_like(dp) if need[6] else None
        if dw is not None:
            wc = _lib.norm(w, dty)
            with _lib.on_device(dev):
                _lib.check(lib.lqp_boxqp_log_finish_grads(stream, dt, B, n, _lib.ptr(dp), _lib.ptr(z), _lib.ptr(wc), _lib.ptr(dw)),
                           "log_finish_grads")
        return (dQ, dp if need[1] else None, dA, db, dlb, dub, dw, None)
