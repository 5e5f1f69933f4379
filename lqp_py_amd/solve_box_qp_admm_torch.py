"""Batched box-constrained QP layer on MI355X: ADMM forward + fixed-point
implicit backward, behind the reference's Python surface.

    x* = argmin_x 0.5 x^T Q x + p^T x   s.t.  A x = b,  lb <= x <= ub

Drop-in for ``lqp_py/solve_box_qp_admm_torch.py`` of ipo-lab/lqp_py:
``SolveBoxQP`` (:7-18), ``SolveBoxQPLayer`` (:21-67), ``BoxQPTH`` (:70-105),
``torch_solve_box_qp`` (:108-333), ``torch_solve_box_qp_grad`` (:349-432).
Everything numeric runs in the HIP library (``lqp_boxqp_forward`` /
``lqp_boxqp_backward_fp``, include/lqp_amd.h); this module only resolves the
control dict -- including its key-name traps and the caller-dict side effect --
and moves pointers.  Tensors must be on the GPU; there is no CPU fallback.
"""
import collections
import ctypes
import numbers
import os
import re
import threading
import types
import weakref

import torch
import torch.nn as nn

from . import _lib
from .utils import get_ncon

_INF = float("inf")
_SYNC_SPLIT = os.environ.get("LQP_SYNC_SPLIT", "1") != "0"      # (A/B knob: 0 = one-call synchronous forward)
_KKT_NATIVE = os.environ.get("LQP_KKT_NATIVE", "1") != "0"      # (A/B knob: 0 = the KKT backward composed from torch ops + lqp_kkt_solve)
_PREPARE_BWD = os.environ.get("LQP_PREPARE_BWD", "1") != "0"    # (A/B knob: 0 = the backward prepares itself when it is called)
_PREFACTOR_BWD = os.environ.get("LQP_PREFACTOR_BWD", "1") != "0"   # (A/B knob: 0 = nothing of the backward runs ahead of the cotangent)
_BWD_PREFACTORED = 0x100                                         # include/lqp_amd.h: LQP_BWD_PREFACTORED
_BWD_REPORTED = 0x200                                            # include/lqp_amd.h: LQP_BWD_REPORTED


class SolveBoxQP(nn.Module):
    """nn.Module holding the control dict (reference :7-18).  The extension keys (``stop``, ``alpha``, ``sync``, ``launch_mode``,
    ``linsolve``) are read from it at every call, see ``torch_solve_box_qp``; both backward forms only read the solution, so an
    over-relaxed forward (``alpha``) needs nothing of them."""

    def __init__(self, control):
        super().__init__()
        self.control = control

    def forward(self, Q, p, A, b, lb, ub):
        if self.control.get('unroll', False):
            return torch_solve_box_qp(Q=Q, p=p, A=A, b=b, lb=lb, ub=ub, control=self.control)
        # what the layer remembers between calls (did the last batch hold a finite bound?) it remembers per MODULE, in a
        # weak-keyed side table -- never in the caller's dict
        prev = getattr(_tls, 'holder', None)
        _tls.holder = self
        try:
            return SolveBoxQPLayer.apply(Q, p, A, b, lb, ub, self.control)
        finally:
            _tls.holder = prev


class SolveBoxQPLayer(torch.autograd.Function):
    """ADMM forward solve / fixed-point implicit backward (reference :21-67)."""

    @staticmethod
    def forward(ctx, Q, p, A, b, lb, ub, control):
        # Default (control['sync'] absent or True): the reference's semantics -- the call waits for the solve, a
        # singular KKT matrix raises HERE (:215), a Q outside the symmetric x-update falls back to LU by itself.
        # control['sync'] = False (extension, for training loops): the whole schedule is enqueued and the call
        # returns at once; an error is raised by a later call / lqp_py_amd.synchronize(), and the outputs of a
        # failed solve are NaN, never plausible numbers.
        # Whether any bound is finite (:33-38) is found on the device; when none is, control['rho'] = 0 is written into
        # the CALLER's dict as the reference does (_forward_solve, mutate=True).
        # (lqp_py_amd.dist passes the flags of the WHOLE batch when this call holds one shard of it.)
        sync = bool(control.get('sync', True))
        ctx.backward_method = control.get('backward', 'fixed_point')
        ctx.prepared = None
        while_running = None
        need = ctx.needs_input_grad
        if sync and ctx.backward_method != 'kkt' and any(need[:6]) and _PREPARE_BWD:
            # a synchronous call only waits while its schedule runs: the backward's outputs, workspace and argument list are
            # made in that window (the cotangent is all that is missing), see _fp_backward_prepare
            def while_running(parts, linsolve_used):
                if parts is None:          # (the solve is being repeated on another schedule: what was prepared is void)
                    ctx.prepared = None
                    return
                # ... and the part of the backward that does not need the cotangent (free set, Q_FF, its Cholesky
                # factorisation) is enqueued right behind the forward: it runs while this call returns, the caller forms its
                # loss and autograd finds its way to `backward`, which then only solves
                ctx.prepared = _fp_backward_prepare(parts['x'], parts['u'], parts['lams'], parts['nus'], Q, A, lb, ub,
                                                    parts['rho_out'], _wanted(need, A), sync=True, linsolve=linsolve_used,
                                                    prefactor=_PREFACTOR_BWD)
        sol = _forward_solve(Q, p, A, b, lb, ub, control, bounds=control.get('_global_bounds'), sync=sync,
                             check_hook=control.get('_check_hook'), mutate=True,
                             holder=control.get('_holder') or getattr(_tls, 'holder', None), while_running=while_running,
                             raise_infeasible=control.get('infeasible') == 'raise', raise_unbounded=control.get('unbounded') == 'raise')
        # control['infeasible'] / control['unbounded'] = 'flag': the rows of a flagged problem (status 2 / 3) are zero in every gradient
        # (one mask, made on the device, no host sync)
        ctx.flagged = None
        if sol.get('status') is not None:
            for key, code in (('infeasible', 2), ('unbounded', 3)):
                if control.get(key) == 'flag':
                    hit = sol['status'] == code
                    ctx.flagged = hit if ctx.flagged is None else ctx.flagged | hit
        ctx.rho = sol['rho']
        st_ = sol['_stats']
        ctx.bound_flags = (bool(st_['any_lb']), bool(st_['any_ub'])) if st_['any_lb'] >= 0 else None     # (pipelined: not known)
        ctx.linsolve = int(sol['_stats']['linsolve_used'])     # 2: Q was checked symmetric by the forward
        ctx.sync = sync
        ctx.save_for_backward(sol['x'], sol['u'], sol['lams'], sol['nus'], Q, A, lb, ub)
        return sol['x']

    @staticmethod
    def backward(ctx, dl_dz):
        x, u, lams, nus, Q, A, lb, ub = ctx.saved_tensors
        if ctx.flagged is None:
            return SolveBoxQPLayer._backward(ctx, dl_dz, x, u, lams, nus, Q, A, lb, ub)
        # The iterate of a flagged problem is no solution: whatever the backward makes of it -- a singular reduced system among it -- is
        # not a gradient and not an error.  Its rows are exactly zero; a "singular" report is raised only if a problem that was NOT
        # flagged is behind it (cold path: the one host read of the mask).
        _tls.flagged = ctx.flagged           # (a backward that does not wait reports late: _backward_call hands the mask to that report)
        try:
            grads = SolveBoxQPLayer._backward(ctx, dl_dz, x, u, lams, nus, Q, A, lb, ub)
        except RuntimeError as exc:
            at = re.search(r"batch index (-?\d+)", str(exc))
            if "singular" not in str(exc) or at is None or int(at.group(1)) < 0 or not bool(ctx.flagged[int(at.group(1))]):
                raise
            keep = (~ctx.flagged).nonzero().flatten()
            part = lambda t: None if t is None else t[keep]
            sub = SolveBoxQPLayer._backward_plain(ctx, part(dl_dz), part(x), part(u), part(lams), part(nus), part(Q), part(A), part(lb),
                                                  part(ub), None if not torch.is_tensor(ctx.rho) or ctx.rho.numel() == 1 else ctx.rho[keep])
            grads = tuple(None if g is None else torch.zeros((Q.shape[0],) + tuple(g.shape[1:]), dtype=g.dtype, device=g.device)
                          .index_copy_(0, keep, g) for g in sub)
        finally:
            _tls.flagged = None
        gone = ctx.flagged.view(-1, 1, 1)
        return tuple(None if g is None else torch.where(gone, torch.zeros((), dtype=g.dtype, device=g.device), g) for g in grads)

    @staticmethod
    def _backward_plain(ctx, dl_dz, x, u, lams, nus, Q, A, lb, ub, rho):
        rho = ctx.rho if rho is None else rho
        if ctx.backward_method == 'kkt':
            return _kkt_backward(dl_dz, x, lams, nus, Q, A, lb, ub, flags=ctx.bound_flags, linsolve=ctx.linsolve,
                                 want=_wanted(ctx.needs_input_grad, A), sync=ctx.sync)
        return _fp_backward(dl_dz, x, u, lams, nus, Q, A, lb, ub, rho, _wanted(ctx.needs_input_grad, A), sync=ctx.sync,
                            linsolve=ctx.linsolve)

    @staticmethod
    def _backward(ctx, dl_dz, x, u, lams, nus, Q, A, lb, ub):
        if ctx.backward_method == 'kkt':
            return _kkt_backward(dl_dz, x, lams, nus, Q, A, lb, ub, flags=ctx.bound_flags, linsolve=ctx.linsolve,
                                 want=_wanted(ctx.needs_input_grad, A), sync=ctx.sync)
        prep, ctx.prepared = ctx.prepared, None
        if prep is not None:
            return _fp_backward_run(prep, dl_dz)
        return _fp_backward(dl_dz, x, u, lams, nus, Q, A, lb, ub, ctx.rho, _wanted(ctx.needs_input_grad, A), sync=ctx.sync,
                            linsolve=ctx.linsolve)


def _wanted(need, A):
    return dict(dQ=need[0], dp=need[1], dA=need[2] and A is not None, db=need[3] and A is not None, dlb=need[4], dub=need[5])


class BoxQPTH:
    """Stateful holder (reference :70-105), including its quirk that passing
    ``lb``/``ub`` to ``update`` clears them (:99-102).  ``control['stop']`` and
    ``control['alpha']`` act as in ``torch_solve_box_qp``."""

    def __init__(self, Q, p, A, b, lb, ub, control):
        self.Q, self.p, self.A, self.b, self.lb, self.ub = Q, p, A, b, lb, ub
        self.control = control
        self.sol = {}

    def solve(self):
        self.sol = torch_solve_box_qp(Q=self.Q, p=self.p, A=self.A, b=self.b, lb=self.lb, ub=self.ub,
                                      control=self.control)
        return self.sol.get('x')

    def update(self, Q=None, p=None, A=None, b=None, lb=None, ub=None, control=None):
        if Q is not None:
            self.Q = Q
        if p is not None:
            self.p = p
        if A is not None:
            self.A = A
        if b is not None:
            self.b = b
        if lb is not None:
            self.lb = None
        if ub is not None:
            self.ub = None
        if control is not None:
            self.control = control
        return None


def torch_solve_box_qp(Q, p, A, b, lb, ub, control):
    """Forward solve; returns {"x","z","u","lams","nus","rho","iter"} (reference :108-333).

    control['stop'] = 'each' (extension; default 'all', the reference's torch.all at :312): every problem is solved as the reference
    would solve it in a batch of one -- it stops at the first check at which IT is optimal, and at an adaptive-rho event it adapts
    iff its own residuals ask for it -- so its result does not depend on what else is in the batch or on how the batch was sharded.
    "iter" is then the largest per-problem count and "iters" a (B,) int32 device tensor of all of them.  With verbose=True the
    trace printed is the maximum over the problems still running at each check.  Not with unroll=True, dist_strict_stop or a
    check hook (ValueError).

    control['alpha'] (extension; default 1.0, the reference's plain step): over-relaxation, as OSQP's alpha.  The z- and the dual
    update of an iteration see xh = alpha x + (1 - alpha) z_prev in place of x; the residuals of the check (r = x - z with the
    unrelaxed x), the next right-hand side, the rho events and the returned x are as before, and so is the fixed point (x = z
    there), hence both backward forms.  A number or a one-element tensor inside (0, 2), anything else is a ValueError at the call;
    1.6 takes about a third of the iterations off the reference's count.  Every loop kernel takes it: with
    stop='each', sync=False, any launch_mode and linsolve, under lqp_py_amd.dist with and without dist_strict_stop.  Not with
    unroll=True (ValueError: the tape replays the unrelaxed step).  A batch without any finite bound does not iterate and ignores it.

    control['infeasible'] (extension; absent or None: off | 'raise' | 'flag') with control['eps_prim_inf'] (default 1e-4, inside
    (0, 1)): primal infeasibility detection, only with stop='each' (ValueError otherwise, and with unroll=True).  At every check of
    a problem the differences of y = rho u, g = Qs x + s and nu against the check before (same rho) are tested as a Farkas
    certificate of {A x = b} and [lb, ub] not meeting -- OSQP's test; the rule is in DESIGN.md section 7.  A flagged problem stops
    like an optimal one, x, z, u hold its iterate of that check.  This function never raises for it: with stop='each', detection on
    or off, the dict holds "status", a (B,) int32 device tensor -- 0 optimal, 1 ended at max_iters without being optimal, 2 primal
    infeasible, 3 dual infeasible.  The layer raises lqp_py_amd.InfeasibleQPError ('raise') or zeroes the gradient rows of flagged
    problems ('flag').

    control['unbounded'] (extension; absent or None: off | 'raise' | 'flag') with control['eps_dual_inf'] (default 1e-4, inside
    (0, 1)): dual infeasibility detection -- the objective is unbounded below on the feasible set (a Q that is only positive
    semi-definite, a bound that is infinite on one side, p pointing down a null direction of Q that the box and A leave open) --
    under the same conditions and independent of control['infeasible']: either key alone or both.  At every check of a problem the
    differences dx, d(Qs x) against the check before (same rho) are tested as OSQP's certificate: Qs dx = 0, ps^T dx < 0, dx inside
    the recession cone of the box (As dx is not tested: the x-update keeps As x = bs).  Optimal is tested
    first, then primal, then dual infeasible.  A flagged problem stops like an optimal one with its iterate of that check, "status"
    says 3; the layer raises lqp_py_amd.UnboundedQPError ('raise') or zeroes its gradient rows ('flag')."""
    check_stop(control)
    if control.get('unroll', False):
        # autograd through the loop (:328-329 returns the bare x); see lqp_py_amd/unrolled.py
        from .unrolled import unrolled_solve_box_qp
        _lib.require_gpu(Q, p, A, b, lb, ub)
        has_lb, has_ub = _finite_bounds(lb, ub)
        return unrolled_solve_box_qp(Q, p, A, b, lb, ub, resolve_control(control, p.shape[1]), has_lb, has_ub, control=control)
    return _forward_solve(Q, p, A, b, lb, ub, control, bounds=None)


def torch_solve_box_qp_grad(dl_dz, x, u, lams, nus, Q, A, lb, ub, rho):
    """Fixed-point implicit gradients -> (dQ, dp, dA, db, dlb, dub, None) (reference :349-432)."""
    has_eq = A is not None
    want = dict(dQ=True, dp=True, dA=has_eq, db=has_eq, dlb=True, dub=True)
    return _fp_backward(dl_dz, x, u, lams, nus, Q, A, lb, ub, rho, want)


def torch_solve_box_qp_grad_kkt(dl_dz, x, lams, nus, Q, A, lb, ub):
    """KKT-system backward (reference :435-469).  The reference solves the (3n+m) system
        [[Q, G^T diag(lam), A^T], [G, -diag(slack), 0], [A, 0, 0]] [dx; dlam; dnu] = [-dl_dz; 0; 0]
    with G = [-I; I].  Eliminating dlam = diag(1/slack) G dx exactly turns it into one (n+m) KKT
    solve with Q + diag(lam_lo/slack_lo + lam_hi/slack_hi) -- the same solution, on the HIP KKT
    solve (lqp_kkt_solve).  Clamps (1e-8) and the lb/ub bookkeeping of :565-584 are kept."""
    return _kkt_backward(dl_dz, x, lams, nus, Q, A, lb, ub)


def _kkt_backward(dl_dz, x, lams, nus, Q, A, lb, ub, flags=None, linsolve=1, want=None, sync=True):
    """flags: (any_lb, any_ub) when the caller knows them (the layer's forward saw them in the device's report).  With both
    true the whole backward is the library's (lqp_boxqp_backward_kkt: the reduced system on the fixed-point backward's
    kernels, gradients formed in its epilogue); since round 5 the one-sided and unbounded cases too, with the reference's
    bookkeeping of which half of dl_dh goes where (:565-584) applied to the kernel's outputs.  _KKT_NATIVE = False keeps
    the composition below.  Pinned by tests/kkt_table.py: every form and entry against the oracle's float64 solve_box_qp_grad_kkt."""
    from .solve_qp_eqcon_torch import _kkt_solve
    _lib.require_gpu(dl_dz, x, lams, nus, Q, A, lb, ub)
    n = Q.shape[1]
    any_lb, any_ub = flags if flags is not None else _finite_bounds(lb, ub)
    if _KKT_NATIVE:
        lib, B, m = _lib.load(), Q.shape[0], get_ncon(A, dim=1)
        dt, dev, dty = _lib.dtype_code(x), x.device, x.dtype
        want = want or dict(dQ=True, dp=True, dA=m > 0, db=m > 0, dlb=True, dub=True)
        gc, xc, lc, nc, Qc, Ac, lbc, ubc = (_lib.norm(t, dty) for t in (dl_dz, x, lams, nus, Q, A, lb, ub))
        # One-sided and unbounded batches run the same kernels (round 5): the reference keeps BOTH halves of G = [-I; I] whenever any
        # bound is finite (:446-452), an infinite bound has an infinite slack, and lam / inf = 0 takes its rows out of the reduced
        # system exactly.  Only the reference's bookkeeping of dl_dh differs (:573-584): lower bounds only -> dlb; upper bounds only
        # -> dub = dl_dh[:n], the LOWER half (all zeros: its quirk, kept); no bounds -> neither.
        only_lb, only_ub = any_lb and not any_ub, any_ub and not any_lb
        dQ, dp, dA, db, dlb, dub = _grad_outputs(
            (want['dQ'], want['dp'], want['dA'], want['db'], (want['dlb'] and any_lb) or (want['dub'] and only_ub),
             want['dub'] and any_lb and any_ub), B, n, m, dty, dev)
        stream = _lib.current_stream_handle(dev)
        ws = _lib.workspace(dev, lib.lqp_boxqp_backward_fp_workspace_bytes(dt, B, n, m), "bwd", stream)
        fail, report = ctypes.c_int32(-1), _lib.host_report(B)
        args = (ctypes.c_void_p(stream), dt, B, n, m, _lib.ptr(gc), _lib.ptr(xc), _lib.ptr(lc), _lib.ptr(nc), _lib.ptr(Qc), _lib.ptr(Ac),
                _lib.ptr(lbc), _lib.ptr(ubc), _lib.ptr(dQ), _lib.ptr(dp), _lib.ptr(dA), _lib.ptr(db), _lib.ptr(dlb), _lib.ptr(dub),
                ctypes.byref(fail) if sync else None, _lib.ptr(ws), ws.numel(), int(linsolve), ctypes.c_void_p(report.data_ptr()))
        _backward_call(lib.lqp_boxqp_backward_kkt, args, "torch_solve_box_qp_grad_kkt", fail, report, dev, B, sync)
        if only_ub:
            dlb, dub = None, (-dlb if want['dub'] else None)
        elif only_lb:
            dub = None
            if not want['dlb']:
                dlb = None
        elif not any_lb:
            dlb = dub = None
        return (dQ, dp, dA, db, dlb, dub, None)
    dlam = None
    Qw = Q
    if any_lb or any_ub:
        slack = torch.clamp(torch.cat((x - lb, ub - x), dim=1), 10 ** -8)          # h - G x
        lams = torch.clamp(lams, 10 ** -8)
        w = lams[:, :n, :] / slack[:, :n, :] + lams[:, n:, :] / slack[:, n:, :]
        Qw = Q.detach().clone()
        Qw.diagonal(dim1=1, dim2=2).add_(w.squeeze(2))
    zeros = None if A is None else torch.zeros((Q.shape[0], A.shape[1], 1), dtype=Q.dtype, device=Q.device)
    dx, dnu = _kkt_solve(Qw, dl_dz, A, zeros)
    if any_lb or any_ub:
        dlam = torch.cat((-dx / slack[:, :n, :], dx / slack[:, n:, :]), dim=1)
    return torch_qp_int_grads_admm(x=x, lams=lams, nus=nus, dx=dx, dlam=dlam, dnu=dnu, any_lb=any_lb, any_ub=any_ub)


def torch_qp_int_grads(x, lams, nus, dx, dlam, dnu):
    """(dQ, dp, dA, db, dG, dh) from the differentials (reference :527-562)."""
    from .solve_qp_eqcon_torch import _outer_grads
    dl_dQ, dl_dA = _outer_grads(dx, x, dnu, nus if dnu is not None else None)
    dl_db = -dnu if dnu is not None else None
    dl_dG = dl_dh = None
    if dlam is not None:
        dl_dG = lams * (dlam * x.transpose(1, 2)) + torch.matmul(lams, dx.transpose(1, 2))
        dl_dh = -lams * dlam
    return (dl_dQ, dx, dl_dA, dl_db, dl_dG, dl_dh)


def torch_qp_int_grads_admm(x, lams, nus, dx, dlam, dnu, any_lb, any_ub):
    """7-tuple (dQ, dp, dA, db, dlb, dub, None) (reference :565-584, including its choice of the
    first n rows of dl_dh in the ub-only case)."""
    n = x.shape[1]
    dl_dQ, dl_dp, dl_dA, dl_db, _, dl_dh = torch_qp_int_grads(x=x, lams=lams, nus=nus, dx=dx, dlam=dlam, dnu=dnu)
    dl_dlb = dl_dub = None
    if any_lb and any_ub:
        dl_dlb, dl_dub = -dl_dh[:, :n, :], dl_dh[:, n:(2 * n), :]
    elif any_lb:
        dl_dlb = -dl_dh[:, :n, :]
    elif any_ub:
        dl_dub = dl_dh[:, :n, :]
    return (dl_dQ, dl_dp, dl_dA, dl_db, dl_dlb, dl_dub, None)


# ---------------------------------------------------------------------------
# internals
# ---------------------------------------------------------------------------
def _finite_bounds(lb, ub):
    """(any_lb, any_ub): global over the whole batch, as in the reference (:33-34, :129-130) -- two reductions and a
    host round trip.  Only the cold paths use it (``unroll``, ``backward='kkt'``, the FIRST un-synchronised call with a
    given control -- a module, or a plain dict with settings not seen before); the layer itself learns the answer from the
    device (see _forward_solve)."""
    flags = torch.stack((torch.max(lb) > -_INF, torch.min(ub) < _INF)).tolist()
    return bool(flags[0]), bool(flags[1])


# "Does the batch hold any finite bound?" selects the schedule (rho = 0: one KKT solve, :157-158) and is a host decision
# in the reference.  Here the setup kernel answers it from the data of EVERY call (status words 12/13); the host only
# assumes an answer when it enqueues -- what the last solve of the same LAYER saw -- and compares afterwards: a call
# that waits for the GPU repeats itself on the other schedule, an un-synchronised one reports the mismatch late (its
# outputs are then not the reference's and must not be used).  The remembered answer lives in a side table, never in
# the caller's control dict (box_qp_control(**control), dict comparisons and serialisation see the dict unchanged):
# keyed weakly by the nn.Module that made the call (SolveBoxQP, ShardedBoxQP), or -- SolveBoxQPLayer.apply /
# torch_solve_box_qp called directly: plain dicts cannot be weakly referenced -- by the dict's id in a bounded table
# (a stale entry after an id is re-used costs one repeated solve, nothing else).
_tls = threading.local()
_seen_by_module = weakref.WeakKeyDictionary()
_seen_by_dict_id = {}


def _same_settings(snap, control):
    """Does `control` hold what `snap` (a shallow copy taken when the answer was remembered) held?  Tensor values count
    only by identity."""
    if len(snap) != len(control):
        return False
    for k, v in snap.items():
        if k not in control:
            return False
        w = control[k]
        if v is w:
            continue
        if torch.is_tensor(v) or torch.is_tensor(w):
            return False
        try:
            if not (v == w):
                return False
        except Exception:
            return False
    return True


def _assume_any_bound(holder, control, sync=True):
    if holder is not None:
        return _seen_by_module.get(holder)
    # CPython hands the address of a short-lived dict (box_qp_control(...) built per call) to the next one: an entry of the
    # id table may belong to another dict.  The entry therefore carries a copy of the settings it was remembered for and
    # only answers for a dict that holds the same (a pipelined call without a module used to look at the bounds
    # on every call instead -- two reductions and a host read that drain the stream).  A dict with EQUAL settings at a
    # recycled address is, for this purpose, the same control: "what the last solve with these settings saw"; a wrong
    # assumption is caught by the device-side flags as before (repeat / late report).
    ent = _seen_by_dict_id.get(id(control))
    if ent is None:
        return None
    snap, any_bound = ent
    return any_bound if _same_settings(snap, control) else None


def _remember_any_bound(holder, control, any_bound):
    if holder is not None:
        _seen_by_module[holder] = bool(any_bound)
        return
    if len(_seen_by_dict_id) > 256:
        _seen_by_dict_id.clear()
    _seen_by_dict_id[id(control)] = (dict(control), bool(any_bound))


def resolve_control(control, n_x):
    """Numbers the loop uses, with the reference's defaults and key names (:133-154)."""
    g = control.get
    check = g('check_solved', max(round((n_x ** 0.5) / 10) * 10, 1))
    ar_iter = max(round(g('adaptive_rho_iter', 100) / check) * check, 1)
    infeasible, eps_prim_inf = check_infeasible(control)
    unbounded, eps_dual_inf = check_infeasible(control, 'unbounded', 'eps_dual_inf')
    return dict(
        infeasible=infeasible,                   # extension: None | 'raise' | 'flag' -- primal infeasibility detection (stop='each' only)
        eps_prim_inf=eps_prim_inf,               # ... and its threshold, inside (0, 1)
        unbounded=unbounded,                     # extension: None | 'raise' | 'flag' -- dual infeasibility detection (stop='each' only)
        eps_dual_inf=eps_dual_inf,               # ... and its threshold, inside (0, 1)
        max_iters=g('max_iters', 10_000),
        eps_abs=max(g('eps_abs', 1e-3), 1e-12),
        eps_rel=max(g('eps_rel', 1e-3), 1e-12),
        check_solved=check,
        rho=g('rho', None), rho_min=g('rho_min', 1e-6), rho_max=g('rho_max', 1e6),
        adaptive_rho=bool(g('adaptive_rho', False)),
        adaptive_rho_tol=g('adaptive_rho_tol', 5),
        adaptive_rho_iter=ar_iter,
        adaptive_rho_max_iter=g('adaptive_max_iter', 1000),
        adaptive_rho_threshold=g('adaptive_rho_threshold', 1e-5),
        scale=bool(g('scale', False)),
        beta=g('beta'),
        verbose=g('verbose', False),
        launch_mode=g('launch_mode', 0),         # extension: 0 auto, 1 segmented, 2 persistent
        linsolve=g('linsolve', 'auto'),          # extension: 'auto' | 'lu' (the reference's cached LU) | 'spd'
        stop=g('stop', 'all'),                   # extension: 'all' (the reference's torch.all, :312) | 'each' (every problem as a batch of one)
        alpha=check_alpha(control),              # extension: over-relaxation factor in (0, 2); 1.0 = the reference's plain step
    )


def check_alpha(control):
    """control['alpha'] as a float (default 1.0): a number, or a one-element tensor taken with float(), inside (0, 2); not 1 with
    unroll=True.  Raises at the call, before any launch; the one place that holds this rule (check_stop comes here)."""
    a = control.get('alpha', 1.0)
    if a.__class__ is float and a == 1.0:         # (the default, and every call without the key)
        return 1.0
    if isinstance(a, bool) or not (isinstance(a, numbers.Real) or (torch.is_tensor(a) and a.numel() == 1)):
        _bad("control['alpha'] must be a number (or a one-element tensor) inside (0, 2)")
    a = float(a)
    if not 0.0 < a < 2.0:                         # (NaN fails both comparisons)
        _bad("control['alpha'] must be inside (0, 2)")
    if a != 1.0 and control.get('unroll', False):
        _bad("control['alpha'] != 1 cannot be combined with unroll=True: the tape replays the unrelaxed step")
    return a


def check_infeasible(control, key='infeasible', eps_key='eps_prim_inf'):
    """control['infeasible'] and control['eps_prim_inf'] -- or, the same rule, control['unbounded'] and control['eps_dual_inf'] --
    -> (None | 'raise' | 'flag', eps as a float).  Raises at the call, before any launch; the one place that holds this rule
    (check_stop comes here for both pairs).  Detection lives in the per-problem stop: the key needs stop='each' and cannot be combined
    with unroll=True."""
    mode = control.get(key)
    if mode is not None and not (isinstance(mode, str) and mode in ('raise', 'flag')):
        _bad(f"control['{key}'] must be None, 'raise' or 'flag'")
    eps = control.get(eps_key, 1e-4)
    if eps.__class__ is not float:
        if isinstance(eps, bool) or not (isinstance(eps, numbers.Real) or (torch.is_tensor(eps) and eps.numel() == 1)):
            _bad(f"control['{eps_key}'] must be a number (or a one-element tensor) inside (0, 1)")
        eps = float(eps)
    if not 0.0 < eps < 1.0:                       # (NaN fails both comparisons)
        _bad(f"control['{eps_key}'] must be inside (0, 1)")
    if mode is not None:
        if control.get('stop', 'all') != 'each':
            _bad(f"control['{key}'] needs control['stop'] = 'each': the certificate is part of a problem's own stopping check")
        if control.get('unroll', False):
            _bad(f"control['{key}'] cannot be combined with unroll=True: the tape has one length")
    return mode, eps


def check_stop(control, check_hook=None):
    """control['stop'] and what it cannot be combined with; -> True for 'each'.  Raises at the call, before any launch.  The one place
    that holds these rules: torch_solve_box_qp, _forward_solve, lqp_py_amd.dist and lqp_py_amd.unrolled all come here (and, through
    it, to check_alpha and check_infeasible: control['alpha'], control['infeasible'] and control['unbounded'] are refused at the same
    places)."""
    check_alpha(control)
    check_infeasible(control)
    check_infeasible(control, 'unbounded', 'eps_dual_inf')
    stop = control.get('stop', 'all')
    if not isinstance(stop, str) or stop not in ('all', 'each'):
        _bad("control['stop'] must be 'all' or 'each'")
    if stop == 'all':
        return False
    if control.get('unroll', False):
        _bad("control['stop'] = 'each' cannot be combined with unroll=True: the tape has one length")
    if control.get('dist_strict_stop', False) or check_hook is not None or control.get('_check_hook') is not None:
        _bad("control['stop'] = 'each' cannot be combined with dist_strict_stop or a check hook: a global stop is its opposite")
    return True


def _per_problem_argument(name, example, value, B, like):
    """-> (mode, scalar value, device tensor or None): 0 the default rule (rho: auto, beta: the quantile rule), 1 scalar,
    2 one value per problem (the reference broadcasts a (B,1) beta against D (B,n), :171-175)"""
    if value is None:
        return 0, 0.0, None
    if not torch.is_tensor(value) or value.numel() == 1:
        return 1, float(value), None
    if value.numel() != B:
        _bad(f"a {name} tensor must hold one value per problem, e.g. shape {example}")
    return 2, 0.0, value.detach().to(device=like.device, dtype=like.dtype).reshape(B).contiguous()


_LINSOLVE = {'auto': 0, 'lu': 1, 'spd': 2, 0: 0, 1: 1, 2: 2}
_ws_bytes = {}                      # (dtype, B, n, m) -> lqp_boxqp_forward_workspace_bytes (a library call per solve otherwise)
_ctl_cache = threading.local()      # .d: (control items, n, any_bound, sync, dtype) -> (resolved dict, rho, lqp_boxqp_ctrl)


def _bad(msg):
    raise ValueError("lqp_py_amd: " + msg)


def _control_struct(control, B, n, like, any_bound, sync, cacheable):
    """-> (resolved dict, rho, lqp_boxqp_ctrl, rho tensor, beta tensor).  The struct of the last call with the same settings
    is reused (resolving ~25 keys and filling it costs ~15 us, in front of the first kernel launch); anything that holds a
    tensor (per-problem rho / beta) is resolved afresh.  The fields of one CALL (reserved, reserved2, bound_flags_in,
    host_report, check_hook) are not set here: _forward_attempt writes them, into a cached struct too."""
    ckey, cached = None, None
    cache = _ctl_cache.__dict__.setdefault('d', {})   # (per thread: every call writes to the struct)
    if cacheable:
        # (the dict of the last call, unchanged -- one C-level comparison of two dicts -- skips building and hashing the key)
        last = _ctl_cache.__dict__.get('last')
        try:
            same = last is not None and last[0] is control and last[2] == (n, any_bound, sync, like.dtype) and last[1] == control
        except Exception:                             # (a value that does not compare to a truth value: a tensor)
            same = False
        if same:
            return last[4] + (None, None)
        try:
            ckey = (tuple(kv for kv in control.items() if kv[0][0] != '_'), n, bool(any_bound), bool(sync), like.dtype)
            cached = cache.get(ckey)
        except Exception:                             # an unhashable value, a key that is not a string: no caching
            ckey = None
        if cached is not None:
            _ctl_cache.last = (control, dict(control), (n, any_bound, sync, like.dtype), ckey, cached)
            return cached + (None, None)
    r = resolve_control(control, n)
    rho = r['rho'] if any_bound else 0                # (no finite bound: one iteration solves it, :157-158)
    rho_mode, rho_value, rho_tensor = _per_problem_argument('rho', '(B,1,1)', rho, B, like)
    beta_mode, beta_value, beta_tensor = _per_problem_argument('beta', '(B,1)', r['beta'], B, like)
    if r['linsolve'] not in _LINSOLVE:
        _bad("control['linsolve'] must be 'auto', 'lu' or 'spd'")
    ctl = _lib.BoxQPCtrl(
        linsolve=_LINSOLVE[r['linsolve']], max_iters=int(r['max_iters']), check_solved=int(r['check_solved']),
        adaptive_rho=int(r['adaptive_rho']), adaptive_rho_iter=int(r['adaptive_rho_iter']),
        adaptive_rho_max_iter=int(r['adaptive_rho_max_iter']), scale=int(r['scale']),
        any_lb=int(any_bound), any_ub=int(any_bound), rho_mode=rho_mode, beta_mode=beta_mode, launch_mode=int(r['launch_mode']),
        eps_abs=float(r['eps_abs']), eps_rel=float(r['eps_rel']), rho_value=rho_value,
        rho_min=float(r['rho_min']), rho_max=float(r['rho_max']), adaptive_rho_tol=float(r['adaptive_rho_tol']),
        adaptive_rho_threshold=float(r['adaptive_rho_threshold']), beta_value=beta_value,
        beta_in=None if beta_tensor is None else beta_tensor.data_ptr(),
        alpha=0.0 if r['alpha'] == 1.0 else r['alpha'])   # (0: not set -- an absent key and alpha=1.0 give the same bytes)
    if ckey is not None and rho_tensor is None and beta_tensor is None and not any(torch.is_tensor(v) for v in control.values()):
        if len(cache) > 64:
            cache.clear()
        cache[ckey] = (r, rho, ctl)
    return r, rho, ctl, rho_tensor, beta_tensor


def _output_block(B, n, m, dtype, dev):
    """-> (x, the six output addresses lqp_boxqp_forward takes, views).  x is its own allocation (a caller that collects
    solutions across batches keeps n floats per problem, not the iterates and duals); z, u, lams, nus, rho share one, each
    16-byte aligned.  Only ADDRESSES are needed in front of the launches: views() -> (z, u, lams, nus, rho) is for afterwards
    (everything in front is host time the GPU idles through in experiment_1's protocol)."""
    n4, m4 = (n + 3) // 4 * 4, (m + 3) // 4 * 4
    sizes = (B * n4, B * n4, 2 * B * n4, B * m4, 4 * B)
    x = torch.empty((B, n, 1), dtype=dtype, device=dev)
    buf = torch.empty((B * (4 * n4 + m4 + 4),), dtype=dtype, device=dev)
    es, o_z = buf.element_size(), buf.data_ptr()
    o_u, o_l, o_nu, o_rho = (o_z + sum(sizes[:k]) * es for k in (1, 2, 3, 4))

    def views():
        parts = buf.split_with_sizes(sizes)
        if n4 == n:
            z, u, lams = parts[0].view(B, n, 1), parts[1].view(B, n, 1), parts[2].view(B, 2 * n, 1)
        else:
            z, u, lams = (parts[k][:B * n * w].view(B, n * w, 1) for k, w in ((0, 1), (1, 1), (2, 2)))
        return z, u, lams, (parts[3][:B * m].view(B, m, 1) if m > 0 else None), parts[4][:B]
    return x, (x.data_ptr(), o_z, o_u, o_l, o_nu if m > 0 else None, o_rho), views


def _strict_stop_hook(check_hook, ws):
    """-> (the C callback, the list its exceptions land in).  check_hook(counters) all-reduces (SUM) the four uint32 words of
    a check -- {not optimal, arrivals, wants rho, ratio trigger} -- in place; it gets a tensor VIEW of the workspace at the
    device address the library names.  check_index -1: the same reduction over a factorisation's failure vote (include/lqp_amd.h)"""
    errors = []

    def _c_hook(_user, _stream, counters_ptr, check_index):
        try:
            off = int(counters_ptr) - ws.data_ptr()
            check_hook(ws[off:off + 16].view(torch.int32), int(check_index))
            return 0
        except Exception as exc:                      # never let an exception cross the C frame
            errors.append(exc)
            return 1
    return _lib.CHECK_HOOK(_c_hook), errors


# What one attempt of a forward solve runs on, and all that a retry rule changes.  bounds: (any_lb, any_ub) when KNOWN; None: assumed
# from the layer's last solve, compared with the device's flags.  one_call: the library waits itself, nothing shared between workgroups.
_Try = collections.namedtuple("_Try", "control bounds one_call")
# What _forward_decide makes of an attempt.  next: the _Try to repeat with; error: what to raise; neither: done.  release, how the report
# buffer goes back: 'now' (the split wait read every word), 'wait' (kernels of a failed call may still write it: wait for the stream
# first), 'tail' (a good call: poll the earlier calls' errors, then defer the report or pool it).
_Verdict = collections.namedtuple("_Verdict", "next error release void_prepared remember", defaults=(None, None, 'wait', False, None))


class _Outcome(types.SimpleNamespace):
    """One trip through the library, not interpreted.  status: of lqp_boxqp_forward, or of lqp_boxqp_forward_finish when the call was
    split (split_wait); any_bound: what it was enqueued for, known: whether that was given or assumed; dims = (dt, B, n, m)."""


def _forward_decide(out, att, owner, look):
    """Every retry rule of the forward solve, in order of precedence; -> _Verdict.  A pure function (no torch, no library): `look`
    () -> (any_lb, any_ub) is called only where a rule needs the bounds themselves.  No rule fires twice in one call, by
    construction: one_call disables the first, linsolve='lu' the second, known bounds the last two, and one_call does not
    outlive the attempt it was set for.  The first two are the retries the library makes by itself inside a one-call solve
    (forward_impl, csrc/lqp_amd.hip): status 5 <-> reserved2 bit 1, status 7 <-> linsolve 'lu'."""
    st, stats = out.status, out.stats
    if out.split_wait and st == 5 and not att.one_call:
        # a kernel that shares its problem with a partner workgroup gave up waiting for it (bounded spins; something else
        # held the CUs): one workgroup per matrix, the loop that needs nobody, instead of failing.  That repeat
        # has no window (while_running) of its own: what this attempt's window prepared is void
        return _Verdict(next=att._replace(one_call=True), release='now', void_prepared=True)
    if out.split_wait and st == 7:
        # the matrix left the symmetric x-update (not symmetric, or Qs + rho I not positive definite in f32): the
        # reference's algorithm -- the pivoted LU -- takes the solve, as a one-call synchronous forward does by itself
        return _Verdict(next=_Try(dict(att.control, linsolve='lu', _owner=owner), att.bounds, False), release='now')
    if out.hook_error:
        return _Verdict(error=out.hook_error[0])
    if st == 3:
        if not out.known and not out.any_bound:
            # the rho = 0 one-shot was enqueued on the ASSUMPTION that this batch, like the layer's last one, holds no
            # finite bound.  If it does, the reference would have run its ADMM loop with rho > 0 (:157-158 do not apply),
            # whose KKT matrix can be regular where [[Q, A^T], [A, 0]] is not (Q = 0: an LP, zero rows): look (cold path)
            has = look()
            if has[0] or has[1]:
                return _Verdict(next=att._replace(bounds=has, one_call=False), remember=True)
        # the reference's torch.linalg.lu_factor raises on an exactly singular KKT matrix (:215)
        return _Verdict(error=RuntimeError(f"lqp_py_amd.torch_solve_box_qp: LU factorisation hit an exactly zero pivot "
                                           f"(batch index {stats.fail_index}); the KKT matrix is singular"))
    if st == 1 and getattr(out, 'term', None) is not None:
        # a layer with a separable term alone: the input checks made on the device (every other cause of this status is refused in Python first)
        return _Verdict(error=ValueError(f"lqp_py_amd: {out.term.device_check} (batch index {stats.fail_index})"))
    try:
        _lib.check(st, "torch_solve_box_qp")
    except RuntimeError as exc:
        return _Verdict(error=exc)
    if stats.mode_used == 3 or out.known or stats.any_lb < 0:
        return _Verdict(release='tail')
    # the device looked at the bounds: did the schedule we enqueued fit them?
    seen = bool(stats.any_lb or stats.any_ub)
    if seen == out.any_bound:
        return _Verdict(release='tail', remember=seen)
    return _Verdict(next=att._replace(bounds=(bool(stats.any_lb), bool(stats.any_ub)), one_call=False), release='tail', remember=seen)


def _forward_attempt(qp, att, owner, sync, check_hook, holder, private_ws, keep_factor, while_running, term=None):
    """One trip through the library on `att` (a _Try): settle the assumption, fetch the control struct, allocate, launch, make
    the views and run the caller's window while the GPU works, wait.  -> _Outcome, for _forward_decide to read.  What stands
    between entry and the first kernel launch is the forward time of a step that starts from an idle queue (experiment_1's
    protocol): errors of EARLIER calls are polled after this one is enqueued, the outputs are one allocation.
    term = (record, tensors): a layer with a separable term (lqp_py_amd/_terms.py, whose check_term has refused what those entry points
    cannot run) -- the record's entry point, with the term's inputs behind ub and its two outputs behind rho_out."""
    Q, p, A, b, lb, ub = qp
    control, bounds, one_call = att
    lib, dev = _lib.load(), p.device
    dt, B, n, m = _lib.dtype_code(p), Q.shape[0], p.shape[1], get_ncon(A, dim=1)
    flags_dev = control.get('_bound_flags_dev')       # (lqp_py_amd.dist: device-side flags of the whole batch)
    known = bounds is not None
    any_bound = bool(bounds[0] or bounds[1]) if known else _assume_any_bound(holder, owner, sync)
    if any_bound is None:                             # first solve of this layer: a call that waits can repeat itself
        # (a shard: the flags of the WHOLE batch decide -- one host read, the same answer on every rank: a shard without any
        #  finite bound inside a batch that has some must enqueue the schedule its peers enqueue)
        any_bound = True if sync else bool(flags_dev.max().item()) if flags_dev is not None else any(_finite_bounds(lb, ub))
    r, rho, ctl, rho_tensor, beta_tensor = _control_struct(control, B, n, p, any_bound, sync, check_hook is None)
    # 1: pipelined (nothing waits); 2: split synchronous call -- enqueue, build the output views while the GPU runs, then
    # lqp_boxqp_forward_finish polls the report (include/lqp_amd.h); 0: the library waits itself (and repeats by itself on the
    # schedule that needs no partner when a shared kernel timed out: one_call).  reserved2 -- bit 0: keep the factor in the
    # workspace (unroll: private_ws); bit 1: nothing shared between workgroups (one_call); bit 2: keep the check trace;
    # bit 3: the problems are independent (control['stop'] = 'each')
    each = r['stop'] == 'each'
    ctl.reserved = (2 if (check_hook is None and _SYNC_SPLIT and not one_call) else 0) if sync else 1
    ctl.reserved2 = (1 if keep_factor else 0) | (2 if one_call else 0) | (4 if r['verbose'] else 0) | (8 if each else 0)
    ctl.bound_flags_in = None if flags_dev is None else flags_dev.data_ptr()
    Qc, pc, Ac, bc, lbc, ubc = (_lib.norm(t, p.dtype) for t in qp)
    # status / info words arrive in pinned host memory, stored there by the forward's last kernel (include/lqp_amd.h:
    # host_report): an un-synchronised call reads them later, a synchronous one right after its wait -- no copies either way
    report, stats = _lib.host_report(_lib.ST_WORDS + 2 * B), _lib.BoxQPStats()
    ctl.host_report = report.data_ptr()
    x, addresses, views = _output_block(B, n, m, p.dtype, dev)
    # control['infeasible'] (with stop='each' alone, check_stop): the entry point with the certificate, and its larger workspace -- the
    # forward's layout with the snapshots behind it.  Key absent: the entry point and the size there always were
    # control['unbounded'], alone or with it: the certifying entry point (either threshold 0 = off) and the workspace whose snapshots
    # hold x and Qs x too
    detect = each and r['infeasible'] is not None
    certify = each and r['unbounded'] is not None
    rec, term_in = term if term is not None else (None, ())
    ws_key = (dt, B, n, m, detect, certify) if rec is None else (dt, B, n, m, rec.entry)
    nbytes = _ws_bytes.get(ws_key)
    if nbytes is None:
        size_of = (getattr(lib, rec.size_of) if rec is not None else
                   lib.lqp_boxqp_forward_certify_workspace_bytes if certify else
                   lib.lqp_boxqp_forward_detect_workspace_bytes if detect else lib.lqp_boxqp_forward_workspace_bytes)
        nbytes = _ws_bytes[ws_key] = size_of(dt, B, n, m)
    stream = _lib.current_stream_handle(dev)
    ws = private_ws if private_ws is not None else _lib.workspace(dev, nbytes, "fwd", stream)
    hook_c = hook_error = None
    if check_hook is not None:
        hook_c, hook_error = _strict_stop_hook(check_hook, ws)      # (hook_c: alive until the library has returned)
        ctl.check_hook = hook_c
    args = (ctypes.c_void_p(stream), dt, B, n, m,
            _lib.ptr(Qc), _lib.ptr(pc), _lib.ptr(Ac), _lib.ptr(bc), _lib.ptr(lbc), _lib.ptr(ubc),
            ctypes.byref(ctl), _lib.ptr(rho_tensor), *addresses,
            ctypes.byref(stats), _lib.ptr(ws), ws.numel())
    aux = u_box = None
    if rec is not None:
        tc = tuple(_lib.norm(t, p.dtype) if torch.is_tensor(t) else t for t in term_in)      # (a plain int of the entry point as it is)
        aux, u_box = torch.empty((B, n, 1), dtype=p.dtype, device=dev), torch.empty((B, n, 1), dtype=p.dtype, device=dev)
        extra = dict(aux=_lib.ptr(aux), u_box=_lib.ptr(u_box))
        term_args = args[:11] + tuple(_lib.ptr(t) if torch.is_tensor(t) else t for t in tc) + args[11:19] + tuple(extra[k] for k in rec.outputs) + args[19:]
    with _lib.on_device(dev):
        if rec is not None:
            st = getattr(lib, rec.entry)(*term_args)
        elif certify:
            st = lib.lqp_boxqp_forward_certify(*args, float(r['eps_prim_inf']) if detect else 0.0, float(r['eps_dual_inf']))
        else:
            st = lib.lqp_boxqp_forward_detect(*args, float(r['eps_prim_inf'])) if detect else lib.lqp_boxqp_forward(*args)
    split_wait = st == 0 and stats.mode_used == 4
    z, u, lams, nus, rho_out = views()
    iters = pstatus = None
    if each and st == 0:
        # the per-problem iteration counts, and how every problem ended (0 optimal, 1 out of iterations, 2 primal, 3 dual infeasible): two copy
        # kernels behind the solve on its stream, into device tensors -- no host wait
        iters = torch.empty((B,), dtype=torch.int32, device=dev)
        pstatus = torch.empty((B,), dtype=torch.int32, device=dev)
        with _lib.on_device(dev):
            _lib.check(lib.lqp_boxqp_problem_iters(ctypes.c_void_p(stream), dt, B, n, m, _lib.ptr(ws), ws.numel(), _lib.ptr(iters)),
                       "problem_iters")
            _lib.check(lib.lqp_boxqp_problem_status(ctypes.c_void_p(stream), dt, B, n, m, _lib.ptr(ws), ws.numel(), _lib.ptr(pstatus)),
                       "problem_status")
    if split_wait:
        if while_running is not None:
            while_running(dict(x=x, u=u, lams=lams, nus=nus, rho_out=rho_out.view(B, 1, 1)), int(stats.linsolve_used))
        # (the views above were made while the GPU ran; now the report: polled in pinned memory, no stream wait)
        st = lib.lqp_boxqp_forward_finish(ctypes.c_void_p(stream), B, ctl.max_iters, ctl.check_solved,
                                          ctypes.c_void_p(report.data_ptr()), ctypes.byref(stats))
    return _Outcome(status=st, split_wait=split_wait, stats=stats, hook_error=hook_error, any_bound=any_bound, known=known,
                    report=report, ws=ws, stream=stream, dims=(dt, B, n, m), r=r, rho=rho, rho_mode=ctl.rho_mode,
                    x=x, z=z, u=u, lams=lams, nus=nus, rho_out=rho_out, iters=iters, pstatus=pstatus, term=rec, aux=aux, u_box=u_box)


def _print_check_trace(out, dev):
    """The reference prints three lines at every check (:289-294); here the loop runs on the device without the host, so the
    trace it kept -- the largest primal and dual error of the batch per check -- is printed once the solve is over."""
    stats, r, ws = out.stats, out.r, out.ws
    n_chk = int(stats.n_check) if stats.n_check >= 0 else int(r['max_iters'] - 1) // int(r['check_solved']) + 1
    tr = torch.empty((2 * max(min(n_chk, 2048), 1),), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().lqp_boxqp_check_trace(_lib.stream_ptr(dev), *out.dims, _lib.ptr(ws), ws.numel(), min(n_chk, 2048),
                                                     _lib.ptr(tr)), "check_trace")
    trh = tr.cpu()
    it_last = int(stats.iters) if stats.iters >= 0 else None
    for c in range(min(n_chk, 2048)):
        it_c = c * int(r['check_solved'])
        if it_last is not None and it_c > it_last:
            break
        if stats.iters < 0 and float(trh[2 * c]) == 0.0 and float(trh[2 * c + 1]) == 0.0 and c > 0:
            break                                      # (a pipelined call: the checks that never ran left no mark)
        print(f'iteration = {it_c}')
        print(f'|| primal_error|| = {float(trh[2 * c]):.10f}')
        print(f'|| dual_error|| = {float(trh[2 * c + 1]):.10f}')


def _solution(out, like, residuals):
    """The dict a forward solve returns, and the record last_forward_status reads."""
    stats, r, ws, dev = out.stats, out.r, out.ws, like.device
    dt, B, n, m = out.dims
    # type of the returned rho follows the reference: a python number stays one unless
    # adaptive rho rewrote it (:248-250); None becomes a (B,1,1) tensor (:200-203)
    as_given = out.rho_mode == 1 and not stats.rho_updated and not (stats.mode_used == 3 and r['adaptive_rho'])
    rho_ret = out.rho if as_given else out.rho_out.view(B, 1, 1)     # (un-synchronised calls cannot know whether rho was adapted: tensor)
    sol = {"x": out.x, "z": out.z, "u": out.u, "lams": out.lams, "nus": out.nus, "rho": rho_ret, "iter": int(stats.iters)}
    if getattr(out, 'term', None) is not None:      # a separable term: where every element rests (side / zone / curv), the box's share of u
        sol[out.term.aux], sol["u_box"] = out.aux, out.u_box
    if out.iters is not None:            # control['stop'] = 'each': every problem's own count; "iter" is the largest
        sol["iters"] = out.iters
        sol["status"] = out.pstatus      # (B,) int32: 0 optimal, 1 ended at max_iters, 2 primal infeasible (control['infeasible']), 3 dual infeasible (control['unbounded'])
    _last_problem_status[(dev.index, out.stream)] = out.pstatus
    if residuals:                        # errors of the last check (the NumPy twin's extra outputs)
        pri, dua = (torch.empty((B,), dtype=like.dtype, device=dev) for _ in range(2))
        with torch.cuda.device(dev):
            _lib.check(_lib.load().lqp_boxqp_last_residuals(_lib.stream_ptr(dev), dt, B, n, m, _lib.ptr(ws), ws.numel(),
                                                            _lib.ptr(pri), _lib.ptr(dua)), "last_residuals")
        sol["primal_error"], sol["dual_error"] = pri, dua
    sol["_stats"] = {k: getattr(stats, k) for k, _ in stats._fields_}
    _last_forward[(dev.index, out.stream)] = (ws, dt, B, n, m, dict(sol["_stats"]), int(r['check_solved']), int(r['max_iters']))
    return sol


def _forward_solve(Q, p, A, b, lb, ub, control, bounds=None, sync=True, residuals=False, check_hook=None, mutate=False,
                   holder=None, private_ws=None, keep_factor=False, while_running=None, one_call=False, raise_infeasible=False,
                   raise_unbounded=False, term=None):
    """bounds: (any_lb, any_ub) when the caller KNOWS them (a shard of a larger batch with host-side flags); None: found
    on the device.  mutate: apply the reference layer's dict side effect control['rho'] = 0 (:37-38).  holder: the
    nn.Module on whose behalf the call is made (keys what is remembered between calls, see _assume_any_bound).
    Attempt, decide, act on the verdict, in a loop: _forward_attempt runs the library once, _forward_decide holds the rules.
    raise_infeasible (the layer with control['infeasible'] = 'raise'): a problem flagged primal infeasible raises InfeasibleQPError
    once the whole batch is done -- here when the call waited, where the other late errors surface when it did not.
    raise_unbounded (control['unbounded'] = 'raise'): the same for a problem flagged dual infeasible, UnboundedQPError, behind the
    primal one."""
    check_stop(control, check_hook)
    _lib.require_gpu(Q, p, A, b, lb, ub)
    sync = sync or check_hook is not None             # (the strict global stop is host-driven: one launch per check)
    owner = control.get('_owner') or control          # (lqp_py_amd.dist hands the layer a copy of the caller's dict)
    att, dev = _Try(control, bounds, one_call), p.device
    while True:
        out = _forward_attempt((Q, p, A, b, lb, ub), att, owner, sync, check_hook, holder, private_ws, keep_factor, while_running, term=term)
        v = _forward_decide(out, att, owner, lambda: _finite_bounds(lb, ub))
        if v.release == 'tail':
            try:
                _lib.poll_errors()        # (an error of an EARLIER un-synchronised call surfaces here: this call is enqueued,
            finally:                      #  its own report is queued behind the poll -- it is never raised at its own call)
                if out.stats.mode_used == 3:  # nothing was waited for: the report is read once the stream has passed the call
                    _lib.defer_check("SolveBoxQP.forward", dev, out.report, Q.shape[0], True,
                                     bounds_check=None if out.known else (
                                         out.any_bound, owner, mutate, lambda _c, seen: _remember_any_bound(holder, owner, seen)),
                                     raise_infeasible=raise_infeasible and out.pstatus is not None,
                                     raise_unbounded=raise_unbounded and out.pstatus is not None)
                else:                     # (the library waited after all: nothing left to report late)
                    _lib.report_done(out.report)
        else:
            if v.release == 'wait':       # (cold path)
                torch.cuda.current_stream(dev).synchronize()
            _lib.report_done(out.report)
        if v.void_prepared and while_running is not None:
            while_running(None, 0)
        if v.remember is not None:
            _remember_any_bound(holder, owner, v.remember)
        if v.error is not None:
            raise v.error
        if v.next is None:
            break
        att = v.next
    if mutate and not out.any_bound:
        att.control['rho'] = owner['rho'] = 0      # written into the CALLER's dict, as the reference does (:37-38)
    if out.r['verbose']:
        _print_check_trace(out, dev)
    sol = _solution(out, p, residuals)
    if (raise_infeasible or raise_unbounded) and out.pstatus is not None and out.stats.mode_used != 3:
        ended = out.pstatus.tolist()          # (the call waited for the solve: this read waits for a copy kernel)
        for wanted, code, error in ((raise_infeasible, 2, _lib.InfeasibleQPError), (raise_unbounded, 3, _lib.UnboundedQPError)):
            flagged = [i for i, e in enumerate(ended) if e == code]
            if wanted and flagged:
                raise error("SolveBoxQP.forward", flagged)
    return sol


_last_forward = {}
_last_problem_status = {}


def last_problem_status(device):
    """How every problem of the most recent forward solve on `device`, on the CURRENT stream, ended: a (B,) int32 device tensor --
    0 optimal, 1 it ended at max_iters without being optimal, 2 flagged primal infeasible (control['infeasible']), 3 flagged dual
    infeasible (control['unbounded']) -- or None when that
    solve did not run with control['stop'] = 'each'.  Stream-ordered like the solution itself: reading it on the host waits for the
    solve.  Valid until the next forward on the same stream, like last_forward_status."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return _last_problem_status[(device.index, _lib.current_stream_handle(device))]


def last_forward_status(device):
    """Bookkeeping of the most recent forward solve on `device`, on the CURRENT stream (workspaces are per stream): {"iters", "n_check", "n_factor", "mode_used",
    "linsolve_used", "factor_launches", "loop_workgroups_per_qp", "loop_kind"}.  A call that did not wait for the GPU
    (control['sync'] = False) could not report its iteration count; it is read here from the device-side status
    block of that call's workspace (this waits for the device).  Valid until the next forward on the same stream."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    ws, dt, B, n, m, st, check, max_iters = _last_forward[(device.index, _lib.current_stream_handle(device))]
    if st["mode_used"] == 3:
        lib = _lib.load()
        so, sb, io, ib = (ctypes.c_size_t() for _ in range(4))
        _lib.check(lib.lqp_boxqp_forward_layout(dt, B, n, m, ctypes.byref(so), ctypes.byref(sb), ctypes.byref(io),
                                                ctypes.byref(ib)), "forward_layout")
        torch.cuda.synchronize(device)
        status = ws[so.value:so.value + sb.value].view(torch.int32).cpu().tolist()
        iters = status[1] if status[0] else max_iters - 1          # [0] done, [1] final iteration, [3] refactorisations
        st = dict(st, iters=iters, n_check=iters // check + 1, n_factor=1 + status[3], n_solve=iters + 1,
                  any_lb=status[12], any_ub=status[13])
    st["loop_workgroups_per_qp"] = st.pop("loop_workgroups")
    return st


def _grad_outputs(on, B, n, m, dty, dev):
    """(dQ, dp, dA, db, dlb, dub) of a backward call: an uninitialised tensor where `on` (six flags, same order) says so"""
    mk = lambda flag, *shape: torch.empty(shape, dtype=dty, device=dev) if flag else None
    return (mk(on[0], B, n, n), mk(on[1], B, n, 1), mk(on[2] and m > 0, B, m, n), mk(on[3] and m > 0, B, m, 1),
            mk(on[4], B, n, 1), mk(on[5], B, n, 1))


def _backward_call(fn, args, what, fail, report, dev, B, sync):
    """fn(*args), one lqp_boxqp_backward_* call, and what follows every one of them: status 3 is the reference's "singular"
    error, the rest goes through _lib.check; then the errors of earlier calls (this call's own report is queued behind the
    poll), and the report buffer is deferred (nothing waited) or goes back to the pool."""
    try:
        with _lib.on_device(dev):
            st = fn(*args)
        if st == 3:
            raise RuntimeError(f"lqp_py_amd.{what}: the input matrix is singular (batch index {fail.value})")
        _lib.check(st, what)
    except Exception:
        _lib.pinned_release(report)     # (a failed call: its pinned report goes back -- quarantined while a queued kernel may still write it)
        raise
    try:
        _lib.poll_errors()
    finally:
        if not sync:
            _lib.defer_check("SolveBoxQP.backward", dev, report, B, False, ignore=getattr(_tls, 'flagged', None))
        else:
            _lib.report_done(report)


class _Prepared(dict):
    """What _fp_backward_prepare hands to _fp_backward_run.  A forward that is never followed by its backward (validation with
    grad enabled, an exception, a retry on the other schedule) drops it: the pinned report buffer then goes back to the pool
    instead of leaking one buffer per call.  The prefactor phase reports into that buffer (include/lqp_amd.h,
    lqp_boxqp_backward_fp_prefactor): it is re-used only once every word of it has arrived (_lib.pinned_release)."""

    def __del__(self):
        try:
            rep = self.get('report')
            if rep is not None and not self.get('ran'):
                if self.get('pref_reported'):
                    _lib.pinned_release(rep)
                else:
                    _lib.report_done(rep)
        except Exception:
            pass


# dQ of a prepared backward is allocated up front (in the window where the host only waits for the forward) up to this many
# bytes; above, at `backward` itself: a forward without a backward would hold it for nothing -- 1 GB at B = 1024, n = 500
_PREPARE_DQ_MAX_BYTES = 256 << 20
_TAIL_DQ = 8 + 3          # (the slot of dQ in _fp_backward_prepare's `tail`, lqp_boxqp_backward_fp's argument list: behind 8 inputs and 3 rho words)


def _fp_backward_prepare(x, u, lams, nus, Q, A, lb, ub, rho, want, sync=True, linsolve=1, prefactor=False):
    """Everything of the fixed-point backward that does not need the cotangent: output tensors, workspace, report buffer,
    the argument list of lqp_boxqp_backward_fp.  A synchronous layer call runs this WHILE its forward is on the GPU (the host
    would only wait), so that `backward` is one library call behind the autograd engine's thread hop."""
    _lib.require_gpu(x, u, lams, nus, Q, A, lb, ub)
    lib, B, n, m = _lib.load(), Q.shape[0], Q.shape[1], get_ncon(A, dim=1)
    dt, dev, dty = _lib.dtype_code(x), x.device, x.dtype
    rho_mode, rho_value, rho_tensor = _per_problem_argument('rho', '(B,1,1)', 1.0 if rho is None else rho, B, x)     # (:356-357)
    xc, uc, lc, nc, Qc, Ac, lbc, ubc = (_lib.norm(t, dty) for t in (x, u, lams, nus, Q, A, lb, ub))
    late_dQ = bool(want['dQ']) and prefactor and B * n * n * x.element_size() > _PREPARE_DQ_MAX_BYTES
    dQ, dp, dA, db, dlb, dub = _grad_outputs((want['dQ'] and not late_dQ, want['dp'], want['dA'], want['db'], want['dlb'],
                                              want['dub']), B, n, m, dty, dev)
    stream = _lib.current_stream_handle(dev)
    ws = _lib.workspace(dev, lib.lqp_boxqp_backward_fp_workspace_bytes(dt, B, n, m), "bwd", stream)
    fail, report = ctypes.c_int32(-1), _lib.host_report(B)      # (the info words go straight into pinned host memory)
    head = (ctypes.c_void_p(stream), dt, B, n, m)
    tail = (_lib.ptr(xc), _lib.ptr(uc), _lib.ptr(lc), _lib.ptr(nc), _lib.ptr(Qc), _lib.ptr(Ac), _lib.ptr(lbc), _lib.ptr(ubc),
            rho_mode, rho_value, _lib.ptr(rho_tensor),
            _lib.ptr(dQ), _lib.ptr(dp), _lib.ptr(dA), _lib.ptr(db), _lib.ptr(dlb), _lib.ptr(dub),
            ctypes.byref(fail) if sync else None, _lib.ptr(ws), ws.numel())
    rep = None if report is None else ctypes.c_void_p(report.data_ptr())
    keep = (xc, uc, lc, nc, Qc, Ac, lbc, ubc, rho_tensor, ws)          # (the pointers above point into these)
    pref, pref_reported = None, False
    if prefactor:
        # (reads x, u behind the forward's kernels in stream order -- the Cholesky form with linsolve 2, else the reduced system's
        #  pivoted LU and its packed factor; LQP_ERR_UNSUPPORTED = this form has no phases: nothing was enqueued.  The
        #  factorisation's info words go into the report buffer of the backward call: that call then waits for them only -- it
        #  returns while its solves and the gradient epilogue run)
        with _lib.on_device(dev):
            st = lib.lqp_boxqp_backward_fp_prefactor(*head, _lib.ptr(xc), _lib.ptr(uc), _lib.ptr(Qc), _lib.ptr(Ac), _lib.ptr(lbc),
                                                     _lib.ptr(ubc), _lib.ptr(ws), ws.numel(), int(linsolve), rep if sync else None)
        if st == 0:
            pref = _lib.workspace_uses(dev, "bwd", stream)      # (still ours at `backward` if nobody asked for the buffer since)
            pref_reported = bool(sync and rep is not None)
        elif st != 6:
            _lib.check(st, "torch_solve_box_qp_grad (prefactor)")
    return _Prepared(lib=lib, head=head, tail=tail, keep=keep, grads=(dQ, dp, dA, db, dlb, dub, None), fail=fail, report=report,
                     dev=dev, dty=dty, B=B, sync=sync, linsolve=int(linsolve), rep=rep, pref=pref, stream=stream,
                     late_dQ=(B, n) if late_dQ else None, pref_reported=pref_reported)


def _fp_backward_run(prep, dl_dz, curv=None):
    """curv: a (B,n,1) non-negative diagonal for the free-set block (lqp_boxqp_backward_fp_curv; never on a prefactored `prep`)"""
    _lib.require_gpu(dl_dz, curv)
    gc = _lib.norm(dl_dz, prep['dty'])
    dev, report, B, sync, linsolve = prep['dev'], prep['report'], prep['B'], prep['sync'], prep['linsolve']
    if prep['pref'] is not None and prep['pref'] == _lib.workspace_uses(dev, "bwd", prep['stream']):
        linsolve |= _BWD_PREFACTORED                       # the factorisation made behind the forward is still in the workspace
        if prep.get('pref_reported'):
            linsolve |= _BWD_REPORTED                      # ... and its info words are in (or on their way into) the report buffer
    # Every run writes the (shared, cached) backward workspace: a full run rebuilds free set, factor and info words in it, the
    # solve phase its right-hand sides.  Whoever prefactored into the same buffer earlier (forward A, forward B, backward A,
    # backward B: B's factor is overwritten by A's full run) must see the count move and run in full too.
    _lib.workspace_touch(dev, "bwd", prep['stream'])
    tail = prep['tail']
    if prep.get('late_dQ'):
        Bq, nq = prep['late_dQ']
        dQ = torch.empty((Bq, nq, nq), dtype=prep['dty'], device=dev)
        prep['grads'] = (dQ,) + tuple(prep['grads'][1:])
        tail = tail[:_TAIL_DQ] + (_lib.ptr(dQ),) + tail[_TAIL_DQ + 1:]
    prep['ran'] = True                                                 # (the report buffer is this run's to hand back from here on)
    entry = prep['lib'].lqp_boxqp_backward_fp
    if curv is not None:
        cc = _lib.norm(curv, prep['dty'])
        entry, tail = prep['lib'].lqp_boxqp_backward_fp_curv, tail[:8] + (_lib.ptr(cc),) + tail[8:]      # (behind ub)
    _backward_call(entry, (*prep['head'], _lib.ptr(gc), *tail, linsolve, prep['rep']),
                   "torch_solve_box_qp_grad", prep['fail'], report, dev, B, sync)
    return prep['grads']


def _fp_backward(dl_dz, x, u, lams, nus, Q, A, lb, ub, rho, want, sync=True, linsolve=1, curv=None):
    return _fp_backward_run(_fp_backward_prepare(x, u, lams, nus, Q, A, lb, ub, rho, want, sync=sync, linsolve=linsolve), dl_dz, curv=curv)
