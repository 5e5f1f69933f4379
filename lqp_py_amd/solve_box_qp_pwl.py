"""The box-QP layer with a convex piecewise-linear term per element in the objective:

    x* = argmin_x 0.5 x^T Q x + p^T x + sum_i f_i(x_i)   s.t.  A x = b,  lb <= x <= ub,
    f_i(x) = s_i0 x + sum_{k=1..K} (s_ik - s_i,k-1) (x - c_ik)_+ ,   1 <= K <= 3,
    s (B, n, K+1) finite and non-decreasing in k,  c (B, n, K) non-decreasing in k (-inf at the low end, +inf at the high end allowed)

-- several separable terms in ONE solve: turnover cost around yesterday's holdings and soft position limits at once, costs that rise
with the trade's size (kinks c - delta, c, c + delta), asymmetric buy and sell tiers.  ``K = 1`` with slopes ``(-w, w)`` is the L1
layer and ``K = 2`` with slopes ``(-wl, 0, wu)`` the soft band, bit for bit.  In ADMM the term is one more separable piece of the
z-update (a compare scan over the kinks from the top, then the clamp); x-update, factorisations, stopping rule and rho adaptation
are ``torch_solve_box_qp``'s.  Everything numeric runs in the HIP library (``lqp_boxqp_forward_pwl``, the two element-wise kernels
``lqp_boxqp_pwl_effective_box`` / ``lqp_boxqp_pwl_finish_grads`` around ``lqp_boxqp_backward_fp``; include/lqp_amd.h), whose kernels
are written for three kinks: fewer are padded at the top here (a kink at +inf, the last slope once more), which changes no piece
number, and the gradients returned are those of the slots the caller gave.

The solve always takes the loop schedule: bounds that are all infinite are an ordinary case, ``control['rho']`` is never written
to, the rho = 0 one-shot is never chosen.  ``alpha``, ``sync=False``, ``linsolve``, ``launch_mode`` and per-problem ``rho`` /
``beta`` work as in the plain layer; what does not is refused by ``check_pwl``.
"""
import torch
import torch.nn as nn

from . import _lib
from . import _terms as _T
from . import solve_box_qp_admm_torch as _S

PWL_K = 3       # the kinks the kernels are written for (csrc/lqp_boxqp.hpp)


def check_pwl(control, Q=None, p=None, s=None, c=None):
    """What the piecewise-linear layer cannot be combined with, and the shapes and dtypes of s and c (``_terms.check_term``)."""
    _T.check_term(_T.PWL, control, p, (s, c))


def _pad(s, c):
    """(B, n, K+1), (B, n, K) -> the same with PWL_K kinks: kinks at +inf and the last slope repeated, at the top"""
    K = c.shape[2]
    if K == PWL_K:
        return s, c
    return (torch.cat([s, s[:, :, -1:].expand(-1, -1, PWL_K - K)], dim=2),
            torch.cat([c, c.new_full(c.shape[:2] + (PWL_K - K,), float('inf'))], dim=2))


def _slots(t):
    """(B, n, K) -> [K][B][n], the library's layout: slot k of every element as one vector of p's shape"""
    return t.detach().permute(2, 0, 1).contiguous()


def _lower(tensors):
    s, c = _pad(*tensors)
    return _slots(s), _slots(c), PWL_K


def torch_solve_box_qp_pwl(Q, p, A, b, lb, ub, s, c, control):
    """Forward solve; returns torch_solve_box_qp's dict {"x","z","u","lams","nus","rho","iter"} and
      "piece"  (B,n,1): where x_i rests -- 2k on the slope s_k (0 below every kink), 2k - 1 exactly on kink k (only where the kink's jump
                        s_k - s_{k-1} is positive; with none the element belongs to the piece below, 2k - 2)
      "u_box"  (B,n,1): the box's share of the dual u -- zero unless the element is clamped at a bound;
    "lams" is built from u_box (the rest of u is the term's multiplier, s_0 <= rho (u - u_box) <= s_K)."""
    return _T.solve(_T.PWL, (Q, p, A, b, lb, ub), (s, c), control, lower=_lower)


class SolveBoxQPPwl(nn.Module):
    """nn.Module holding the control dict: SolveBoxQPPwl(control)(Q, p, A, b, lb, ub, s, c) -> x, differentiable in all eight."""

    def __init__(self, control):
        super().__init__()
        self.control = control

    def forward(self, Q, p, A, b, lb, ub, s, c):
        return SolveBoxQPPwlLayer.apply(Q, p, A, b, lb, ub, s, c, self.control)


class SolveBoxQPPwlLayer(torch.autograd.Function):
    """ADMM forward with the piecewise-linear step / fixed-point implicit backward on the effective box.

    An element on kink k (piece = 2k - 1, and not held by a hard bound: u_box == 0) behaves exactly like one whose two bounds are both
    c_k; a free element on a slope (piece = 2k) like p_i shifted by s_ik.  So the backward is ``lqp_boxqp_backward_fp``, unchanged, on
    (lb_e, ub_e) = on ? (c_k, c_k) : (lb, ub) with the dual u_e = on ? u : u_box, and then dlb, dub = 0 on the kink sets, dc_k =
    dlb_e + dub_e on kink set k, ds_k = dp on piece == 2k.  A plain call at `backward` time."""

    @staticmethod
    def forward(ctx, Q, p, A, b, lb, ub, s, c, control):
        return _T.layer_forward(ctx, _T.PWL, (Q, p, A, b, lb, ub), (s, c), control, ('x', 'u', 'u_box', 'piece', 'nus'),
                                (Q, A, lb, ub, c), lower=_lower)

    @staticmethod
    def backward(ctx, dl_dz):
        x, u, u_box, piece, nus, Q, A, lb, ub, c = ctx.saved_tensors
        h = _T.backward_prelude(ctx, x, Q, A, box_grads=True)
        need, lib, B, n, K = h.need, h.lib, h.B, h.n, c.shape[2]
        lbc, ubc = (_lib.norm(t, h.dty) for t in (lb, ub))
        ck = _lib.norm(_slots(c), h.dty)
        lb_e, ub_e, u_e = (torch.empty((B, n, 1), dtype=h.dty, device=h.dev) for _ in range(3))
        lams_e = torch.empty((B, 2 * n, 1), dtype=h.dty, device=h.dev)
        with _lib.on_device(h.dev):
            _lib.check(lib.lqp_boxqp_pwl_effective_box(h.stream, h.dt, B, n, _lib.ptr(piece), _lib.ptr(u), _lib.ptr(u_box), _lib.ptr(lbc),
                                                       _lib.ptr(ubc), _lib.ptr(ck), K, h.rho_mode, h.rho_value, _lib.ptr(h.rho_tensor),
                                                       _lib.ptr(lb_e), _lib.ptr(ub_e), _lib.ptr(u_e), _lib.ptr(lams_e)), "pwl_effective_box")
        dQ, dp, dA, db, dlb, dub, _ = _S._fp_backward(dl_dz, x, u_e, lams_e, nus, Q, A, lb_e, ub_e, ctx.rho, h.want, sync=ctx.sync,
                                                      linsolve=ctx.linsolve)
        # (the library's layout, [K + 1][B][n] and [K][B][n]; returned as views in the caller's)
        ds = torch.empty((K + 1, B, n), dtype=h.dty, device=h.dev) if need[6] else None
        dc = torch.empty((K, B, n), dtype=h.dty, device=h.dev) if need[7] else None
        with _lib.on_device(h.dev):
            _lib.check(lib.lqp_boxqp_pwl_finish_grads(h.stream, h.dt, B, n, _lib.ptr(piece), _lib.ptr(u_box), _lib.ptr(dp), _lib.ptr(dlb),
                                                      _lib.ptr(dub), K, _lib.ptr(dlb), _lib.ptr(dub), _lib.ptr(ds), _lib.ptr(dc)),
                       "pwl_finish_grads")
        return (dQ, dp if need[1] else None, dA, db, dlb if need[4] else None, dub if need[5] else None,
                None if ds is None else ds.permute(1, 2, 0), None if dc is None else dc.permute(1, 2, 0), None)
