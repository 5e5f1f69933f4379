"""``unroll=True``: differentiate THROUGH the ADMM loop (reference: lqp_py/solve_box_qp_admm_torch.py:14-15 routes the
module here, :216-219/:255-256/:264-265 swap the plain LU solve for the ``TorchLU`` layer so that autograd tapes every
iteration).

Native path (one factor for the whole solve, i.e. no adaptive-rho refactorisation): the forward is the ordinary persistent HIP
solve; the backward is ONE reverse sweep over the recorded iterations in the HIP library (csrc/lqp_unroll.hpp): float32 on the
symmetric x-update (the benchmark case) ``lqp_boxqp_unroll_backward`` -- per iteration one product with the cached inverse --,
the pivoted-LU x-update (float64, m > 16, non-symmetric Q, ``linsolve='lu'``) ``lqp_boxqp_unroll_backward_lu`` -- per iteration the
two cached triangular solves of ``TorchLULayer`` --: no taped node, no per-iteration torch op, no host sync.  The kernel differentiates the loop, i.e. it returns the
gradients w.r.t. the SCALED problem (Qs, ps, As, bs, lbs, ubs, rho, D); the scaling itself (:160-203: ~25 element-wise /
reduction ops, once per call) is differentiated by autograd on a small eager graph rebuilt in ``backward``.

A solve in which rho was ADAPTED (the reference's tape then runs through the adaptation itself, :237-256): the tape is walked
epoch by epoch in the library on the pivoted LU of each epoch's KKT matrix (``lqp_boxqp_unroll_tape_segment``) and the adaptation --
a few norms of the iterates of ONE check per event -- is differentiated by autograd on its own small graph
(``_backward_with_rho_events``): no torch op per iteration there either.  What is left (no finite bound: rho = 0, one solve)
takes the eager path below: the loop as torch ops with ``TorchLU`` (HIP LU factor / cached solves) as the taped solve.

Two conventions where the tape is not differentiable, the same on every path (tests/unroll_table.py):
  * an exact tie x_k + u_k == bound is treated as free by the kernels (torch.maximum would split the gradient in two).  At an entry
    with lb == ub every path returns the same dlb + dub; the kernels give the whole of it to the side the iterate came from, the
    taped loop (``torch.minimum`` on the tie max(., lb) == ub) half to each.
  * an infinite bound never binds and carries no gradient: with ``scale=True`` the chain through lbs = lb / D must not hand D the
    0 * inf = NaN of autograd's division rule (``_scale_bound``; k_unroll_scale_vectors takes 0 * inf as 0 too).
"""
import ctypes
import os

import torch

from . import _lib
from .lu_layer import TorchLU, lu_factor
from .utils import get_ncon

_INF = float("inf")
_TINY = 1e-16


def _floor_nonpositive(norms):
    """entries <= 0 -> max(row mean, 1e-6)   (reference :164-168, :182-186)"""
    bad = norms <= 0.0
    if torch.any(bad):
        floor = torch.clamp(norms.mean(dim=1), min=1e-6).unsqueeze(1)
        repl = torch.clamp(norms, min=floor)
        norms = torch.where(bad, repl, norms)
    return norms


def _inf_norm(v):
    return torch.linalg.norm(v, ord=_INF, dim=1, keepdim=True)


def _scale_bound(v, D):
    """v / D (:189) with no gradient through an infinite entry: plain ``v / D`` hands D the gradient 0 * inf = NaN there, and so
    does the untaken branch of a single ``where`` -- the numerator is masked first.  Values unchanged."""
    fin = torch.isfinite(v)
    return torch.where(fin, torch.where(fin, v, torch.zeros_like(v)) / D, v.detach())


def _scaled_problem(Q, p, A, b, lb, ub, r, has_box, colmax=None, fro=None):
    """The reference's pre-conditioning (:160-203) as differentiable torch ops -> (Qs, ps, As, bs, lbs, ubs, D, E, rho);
    D / E are 1.0 without scaling, rho may be a python number.
    colmax (B,n) / fro (B,1,1) given: the column maxima of |Q| (:163) and ||Qs||_F (:201) come from the caller (leaves of its own
    graph, formed by the library's one-pass kernels) and Qs is NOT formed: the first return value is then the scaling vector d
    (B,n) (None without scaling) -- the n-sized part of the chain only, see _UnrolledLoop.backward."""
    dev = p.device
    n = p.shape[1]
    m = get_ncon(A, dim=1)
    rho = r['rho']
    if not has_box:
        rho = 0
    D = E = 1.0
    d = None
    if r['scale']:
        d = torch.sqrt(1 / _floor_nonpositive(torch.linalg.norm(Q, ord=_INF, dim=1) if colmax is None else colmax))
        beta = r['beta']
        if beta is None:
            q = torch.quantile(d, q=torch.tensor([0.10, 0.90], dtype=d.dtype, device=dev), dim=1)
            beta = (1 - q[[0]] / q[[1]]).T
        d = (1 - beta) * d + beta * d.mean(dim=1, keepdim=True)
        if colmax is None:
            Q = d.unsqueeze(2) * Q * d.unsqueeze(1)
        p = d.unsqueeze(2) * p
        if m > 0:
            A = A * d.unsqueeze(1)
            E = (1 / _floor_nonpositive(torch.linalg.norm(A, ord=_INF, dim=2))).unsqueeze(2)
            A = E * A
            b = E * b
        D = d.unsqueeze(2)
        if has_box:
            lb, ub = _scale_bound(lb, D), _scale_bound(ub, D)
    if rho is None:
        rho = torch.clamp((torch.linalg.matrix_norm(Q, keepdim=True) if fro is None else fro) / n ** 0.5, min=r['rho_min'], max=r['rho_max'])
    return (Q if colmax is None and fro is None else d), p, A, b, lb, ub, D, E, rho


def _kkt_matrix(Qs, As, rho):
    """[[Qs + rho I, As^T], [As, 0]] (:205-213); Qs + rho I without equality rows."""
    B, n = Qs.shape[0], Qs.shape[1]
    m = get_ncon(As, dim=1)
    M = Qs + rho * torch.eye(n, dtype=Qs.dtype, device=Qs.device).unsqueeze(0)
    if m > 0:
        corner = torch.zeros(B, m, m, dtype=Qs.dtype, device=Qs.device)
        M = torch.cat((torch.cat((M, As.transpose(1, 2)), 2), torch.cat((As, corner), 2)), 1)
    return M


def _graph_leaves(inputs, need):
    """The inputs as leaves of a graph of their own (None stays None)"""
    return [None if t is None else t.detach().requires_grad_(bool(nd)) for t, nd in zip(inputs, need)]


def _chain_by_autograd(pairs, leaves):
    """The scaling chain (:160-203) by autograd.  pairs: (output of the chain, its cotangent); one that is no tensor of the graph (D = 1.0,
    a given rho) or has no cotangent drops out.  -> one gradient per entry of `leaves`, None for a leaf that is None or needs none."""
    outs = [(o, go) for o, go in pairs if torch.is_tensor(o) and o.requires_grad and go is not None]
    wanted = [t for t in leaves if t is not None and t.requires_grad]
    grads = iter(torch.autograd.grad([o for o, _ in outs], wanted, [go.reshape(o.shape) for o, go in outs], allow_unused=True)
                 if outs and wanted else [None] * len(wanted))
    return [next(grads) if (t is not None and t.requires_grad) else None for t in leaves]


def _output_block(B, n, m, dt, dev, with_dQs, alloc=None):
    """What the library's sweep returns, the gradients w.r.t. the scaled problem (dQs is written whole: never cleared).
    alloc: torch.zeros for outputs that are added to; None: torch.empty, looked up at the call (tests/memharness.py replaces it)"""
    mk = lambda *shape: (torch.empty if alloc is None else alloc)(shape, dtype=dt, device=dev)
    return dict(dQs=torch.empty((B, n, n), dtype=dt, device=dev) if with_dQs else None, dps=mk(B, n, 1), dlbs=mk(B, n, 1), dubs=mk(B, n, 1),
                dD=mk(B, n, 1), dAs=mk(B, m, n) if m > 0 else None, dbs=mk(B, m, 1) if m > 0 else None)


class _UnrolledLoop(torch.autograd.Function):
    """forward: the persistent HIP solve on a workspace of its own (kept for the backward).  backward: one reverse sweep in the library
    where one factor served the whole solve (lqp_boxqp_unroll_backward on the symmetric x-update, lqp_boxqp_unroll_backward_lu on the
    pivoted LU), the walk epoch by epoch where rho was adapted (_backward_with_rho_events); the scaling chain behind either on the
    library's kernels or by autograd.  Raises _NotNative when the solve took neither x-update (no finite bound: rho = 0, one solve) or
    LQP_UNROLL_EVENTS=0 asks for the taped loop on an adapted solve."""

    @staticmethod
    def forward(ctx, Q, p, A, b, lb, ub, control, r, bounds):
        from .solve_box_qp_admm_torch import _forward_solve
        lib = _lib.load()
        B, n = Q.shape[0], p.shape[1]
        m = get_ncon(A, dim=1)
        ws = torch.empty(int(lib.lqp_boxqp_forward_workspace_bytes(_lib.dtype_code(p), B, n, m)), dtype=torch.uint8, device=p.device)
        sol = _forward_solve(Q, p, A, b, lb, ub, control, bounds=bounds, sync=True, private_ws=ws, keep_factor=True)
        st = sol['_stats']
        # the symmetric x-update (float32: the packed inverse) or the pivoted LU (any dtype: the packed factor)
        if st['linsolve_used'] not in (1, 2) or (st['linsolve_used'] == 2 and p.dtype != torch.float32):
            raise _NotNative()
        # rho was adapted along the solve: the tape is walked epoch by epoch on the pivoted LU of each epoch's KKT matrix
        # (_backward_with_rho_events); LQP_UNROLL_EVENTS=0 keeps the taped loop of torch ops for it
        ctx.events = st['n_factor'] != 1
        if ctx.events and os.environ.get("LQP_UNROLL_EVENTS", "1") == "0":
            raise _NotNative()
        ctx.lu = st['linsolve_used'] == 1
        ctx.ws, ctx.iters, ctx.r, ctx.has_box = ws, int(st['iters']), r, bool(bounds[0] or bounds[1])
        ctx.rho_fwd = sol['rho'] if torch.is_tensor(sol['rho']) else None      # (B,1,1): clamp(||Qs||_F / sqrt(n)) when rho was not given
        ctx.save_for_backward(Q, p, A, b, lb, ub)
        return sol['x']

    @staticmethod
    def backward(ctx, g):
        if ctx.events:
            return _backward_with_rho_events(ctx, g)
        Q, p, A, b, lb, ub = ctx.saved_tensors
        lib = _lib.load()
        B, n = Q.shape[0], p.shape[1]
        m = get_ncon(A, dim=1)
        dev, dt = p.device, p.dtype
        need = ctx.needs_input_grad
        up = _output_block(B, n, m, dt, dev, need[0])
        up['drho'] = torch.empty((B, 1, 1), dtype=dt, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        gc = _lib.norm(g, dt)
        # one call: the sweep on the pivoted LU takes the dtype in front, the symmetric one is float32
        entry, query, lead, what = ((lib.lqp_boxqp_unroll_backward_lu, lib.lqp_boxqp_unroll_backward_lu_workspace_bytes, (_lib.dtype_code(p),),
                                     "unroll_backward_lu") if ctx.lu else
                                    (lib.lqp_boxqp_unroll_backward, lib.lqp_boxqp_unroll_backward_workspace_bytes, (), "unroll_backward"))
        scratch = _lib.workspace(dev, query(*lead, B, n, m, ctx.iters), "unroll", stream)
        with _lib.on_device(dev):
            _lib.check(entry(ctypes.c_void_p(stream), *lead, B, n, m, _lib.ptr(ctx.ws), ctx.ws.numel(), ctx.iters, _lib.ptr(gc),
                             *(_lib.ptr(up[k]) for k in ("dQs", "dps", "dAs", "dbs", "dlbs", "dubs", "drho", "dD")),
                             _lib.ptr(scratch), scratch.numel()), what)
        ctx.ws = None
        if need[0] and dt == torch.float32 and os.environ.get("LQP_UNROLL_SCALE_NATIVE", "1") != "0":
            return _scaling_backward_native(ctx, lib, stream, (Q, p, A, b, lb, ub), need, up)
        # ---- the scaling (:160-203) by autograd: leaves -> (Qs, ps, As, bs, lbs, ubs, D, rho) ----
        leaves = _graph_leaves((Q, p, A, b, lb, ub), need)
        with torch.enable_grad():
            Qs, ps, As, bs, lbs, ubs, D, _E, rho = _scaled_problem(*leaves, ctx.r, ctx.has_box)
        pairs = [(Qs, up['dQs']), (ps, up['dps']), (As, up['dAs']), (bs, up['dbs']), (lbs, up['dlbs']), (ubs, up['dubs']), (D, up['dD']),
                 (rho, up['drho'])]
        return tuple(_chain_by_autograd(pairs, leaves)) + (None, None, None)


def _check_quantities(r, rho, x, z, z_old, u, D, Qs, p_inf):
    """What a check of the loop computes (lqp_py/solve_box_qp_admm_torch.py:285-305) and the adaptive step reads (:239-251), as
    differentiable torch ops on (B,n,1) vectors: -> (ratio, wants)."""
    dt = x.dtype
    tiny = torch.full((1,), _TINY, dtype=dt, device=x.device)
    thr = torch.full((1,), float(r['adaptive_rho_threshold']), dtype=dt, device=x.device)
    res = x - z
    s = rho * (z - z_old)
    r_inf, s_inf = _inf_norm(D * res), _inf_norm(D * s)
    pri = torch.maximum(torch.maximum(_inf_norm(D * x), _inf_norm(D * z)), tiny)
    dua = torch.maximum(torch.maximum(torch.maximum(_inf_norm(rho * D * u), _inf_norm(torch.matmul(Qs, x) / D)), p_inf), tiny)
    tol_p = r['eps_abs'] + r['eps_rel'] * pri
    tol_d = r['eps_abs'] + r['eps_rel'] * dua
    wants = torch.logical_or(r_inf > torch.maximum(tol_p, thr), s_inf > torch.maximum(tol_d, thr))
    ratio = (torch.clamp(r_inf / pri, min=_TINY) / torch.clamp(s_inf / dua, min=_TINY)) ** 0.5
    return ratio, wants


def _adapted_rho(r, rho, ratio, wants):
    """:246-251"""
    rho = rho * torch.logical_not(wants) + (rho * ratio) * wants
    return torch.clamp(rho, min=r['rho_min'], max=r['rho_max'])


def _tape_segments(T, ar, ar_iter, ar_max):
    """The cuts [(k0, k1)] of a tape of T x-updates at the iterations where rho may be adapted (:237: the multiples of adaptive_rho_iter
    below adaptive_rho_max_iter): an event can only sit at the head of a segment, never inside one."""
    segs, k = [], 0
    while k < T:
        k1 = T
        if ar:
            nxt = (k // ar_iter + 1) * ar_iter
            if nxt < ar_max and nxt < T:
                k1 = nxt
        segs.append((k, k1))
        k = k1
    return segs


class _AdaptedTape:
    """What the replay and the walk back of an adapted tape share: the sizes, the solve's workspace, the tape's scratch with its rows of
    iterates, the outputs every reverse segment adds to, and the library's calls on them."""

    def __init__(self, ctx, g, p, B, n, m):
        self.lib = _lib.load()
        self.B, self.n, self.m, self.iters, self.ws = B, n, m, ctx.iters, ctx.ws
        self.dt, self.dev, self.dtc = p.dtype, p.device, _lib.dtype_code(p)
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        nbytes = self.lib.lqp_boxqp_unroll_tape_workspace_bytes(self.dtc, B, n, m, ctx.iters)
        self.scratch = torch.empty(int(nbytes), dtype=torch.uint8, device=self.dev)
        self.g = _lib.norm(g, self.dt)
        self.out = _output_block(B, n, m, self.dt, self.dev, False, torch.zeros)      # (dQs: when the walk is done, tape_sums)
        # where the scratch keeps z_{k+1}, u_{k+1}, x_k of every replayed x-update: (B, T, n) each
        rows = B * (ctx.iters + 1) * n * p.element_size()
        self.Zr, self.Ur, self.Xr = (self.scratch[v - self.scratch.data_ptr():][:rows].view(self.dt).view(B, ctx.iters + 1, n)
                                     for v in self.segment(0, 0, 0, None, None, None, rows=True))

    def zeros(self, *shape):
        return torch.zeros(shape, dtype=self.dt, device=self.dev)

    def segment(self, k0, k1, mode, packed, rho_now, state, inj_k=-1, inj=None, drho=None, rows=False):
        """x-updates [k0, k1): replayed (mode 1) or walked back (mode 2) on the epoch's factor; rows: -> where the rows live"""
        o, ptr = self.out, _lib.ptr
        zp, up, xp = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        with _lib.on_device(self.dev):
            _lib.check(self.lib.lqp_boxqp_unroll_tape_segment(
                self.stream, self.dtc, self.B, self.n, self.m, ptr(self.ws), self.ws.numel(), self.iters, k0, k1, mode, ptr(packed),
                ptr(rho_now), ptr(state), inj_k, ptr(inj), ptr(self.g), ptr(o['dps']), ptr(o['dlbs']), ptr(o['dubs']),
                ptr(drho), ptr(o['dD']), ptr(self.scratch), self.scratch.numel(),
                ctypes.byref(zp) if rows else None, ctypes.byref(up) if rows else None, ctypes.byref(xp) if rows else None),
                "unroll_tape_segment")
        return zp.value, up.value, xp.value

    def packed_factor(self, M):
        """The pivoted LU of an epoch's KKT matrix in the layout the sweep streams"""
        LU, piv = lu_factor(M)
        N = self.n + self.m
        buf = torch.empty(self.lib.lqp_lu_packed_bytes(self.dtc, self.B, N), dtype=torch.uint8, device=self.dev)
        with _lib.on_device(self.dev):
            _lib.check(self.lib.lqp_lu_pack(self.stream, self.dtc, self.B, N, _lib.ptr(LU), _lib.ptr(piv), _lib.ptr(buf)), "lu_pack")
        return buf

    def tape_sums(self, with_dQs):
        """What is summed over the whole tape once every segment is walked -> dQs (or None); dAs, dbs into the outputs"""
        o = self.out
        dQs = torch.empty(self.B, self.n, self.n, dtype=self.dt, device=self.dev) if with_dQs else None
        with _lib.on_device(self.dev):
            _lib.check(self.lib.lqp_boxqp_unroll_tape_finish(self.stream, self.dtc, self.B, self.n, self.m, self.iters, _lib.ptr(dQs),
                                                            _lib.ptr(o['dAs']), _lib.ptr(o['dbs']), _lib.ptr(self.scratch),
                                                            self.scratch.numel()), "unroll_tape_finish")
        return dQs


def _replay_epochs(tape, r, rho_e, Qsd, Asd, Dd, p_inf):
    """Replay the loop segment by segment with the reference's own decision rule (:237-251) on the replayed iterates -- the only place
    that decides events.  -> (segs, epochs): segs = [(k0, k1, index of the epoch)]; epochs = [dict(rho (B,), packed: its factor, event)],
    event = None or dict(check: the iterates of the check the adaptation read, wants, c: that check's iteration) of what ENDED it."""
    B, n, T = tape.B, tape.n, tape.iters + 1
    chk = int(r['check_solved'])
    epoch = lambda rho: dict(rho=rho.reshape(B).contiguous(), packed=tape.packed_factor(_kkt_matrix(Qsd, Asd, rho)), event=None)
    state = tape.zeros(B, 2, n)
    segs, epochs = [], [epoch(rho_e)]
    wants = last = last_c = None
    for k, k1 in _tape_segments(T, bool(r['adaptive_rho']), int(r['adaptive_rho_iter']), int(r['adaptive_rho_max_iter'])):
        if k > 0 and bool(torch.any(wants)):           # (the head of a later segment: where _tape_segments says rho may change)
            ratio, _ = _check_quantities(r, rho_e, *last)
            if bool((ratio > r['adaptive_rho_tol']).any()) or bool((ratio < 1 / r['adaptive_rho_tol']).any()):
                epochs[-1]['event'] = dict(check=last, wants=wants, c=last_c)
                rho_e = _adapted_rho(r, rho_e, ratio, wants)
                epochs.append(epoch(rho_e))
        e = epochs[-1]
        tape.segment(k, k1, 1, e['packed'], e['rho'], state)
        segs.append((k, k1, len(epochs) - 1))
        if k1 < T:
            last_c = ((k1 - 1) // chk) * chk
            col = lambda R, kk: R[:, kk, :].unsqueeze(2).clone()
            z_old = col(tape.Zr, last_c - 1) if last_c > 0 else tape.zeros(B, n, 1)
            last = (col(tape.Xr, last_c), col(tape.Zr, last_c), z_old, col(tape.Ur, last_c), Dd, Qsd, p_inf)
            _, wants = _check_quantities(r, rho_e, *last)
    return segs, epochs


def _walk_back(tape, r, segs, epochs):
    """The segments in reverse, the adaptation of every event by autograd on its own small graph: its gradient w.r.t. the iterates goes
    back into the sweep as injected cotangents, w.r.t. the previous rho into that epoch's rho.  -> (rho_bar: one (B,) per epoch, and what
    the adaptations add to the cotangents of D, Qs (None: no event) and ||p||_inf)."""
    B, n = tape.B, tape.n
    rho_bar = [tape.zeros(B) for _ in epochs]
    dD_extra, dQs_extra, dpinf = tape.zeros(B, n, 1), None, tape.zeros(B, 1, 1)
    sbar = tape.zeros(B, 2, n)
    for (k0, k1, ei) in reversed(segs):
        e = epochs[ei]
        inj, inj_k = None, -1
        ev = e['event']
        if ev is not None and ei + 1 < len(epochs) and k1 == min(kk for (kk, _, ej) in segs if ej == ei + 1):
            # rho_{e+1} = adapt(rho_e, the iterates of check c): its cotangent is complete now (every later segment is walked)
            with torch.enable_grad():
                small = [t.detach().clone().requires_grad_(True) for t in ev['check']]
                rl = e['rho'].reshape(B, 1, 1).detach().clone().requires_grad_(True)
                ratio, _ = _check_quantities(r, rl, *small)
                rho_new = _adapted_rho(r, rl, ratio, ev['wants'])
                gr = torch.autograd.grad(rho_new, small + [rl], rho_bar[ei + 1].reshape(B, 1, 1), allow_unused=True)
            zero = lambda t, like: torch.zeros_like(like) if t is None else t
            gx, gz1, gz0, gu1, gDl, gQl, gpl, grl = [zero(t, like) for t, like in zip(gr, small + [rl])]
            inj = torch.stack((gx, gz1, gu1, gz0), 1).reshape(B, 4, n).contiguous()
            inj_k = ev['c']
            rho_bar[ei] += grl.reshape(B)
            dD_extra += gDl
            dQs_extra = gQl if dQs_extra is None else dQs_extra + gQl
            dpinf += gpl
        drho_seg = tape.zeros(B)
        tape.segment(k0, k1, 2, e['packed'], e['rho'], sbar, inj_k=inj_k, inj=inj, drho=drho_seg)
        rho_bar[ei] += drho_seg
    return rho_bar, dD_extra, dQs_extra, dpinf


def _backward_with_rho_events(ctx, g):
    """The tape of a solve in which rho was ADAPTED (solve_box_qp_admm_torch.py:237-256 inside the unrolled loop): the factor
    changes along it, so it is walked epoch by epoch in the library (lqp_boxqp_unroll_tape_segment: every x-update a pair of cached
    triangular solves with the pivoted LU of THAT epoch's KKT matrix, TorchLULayer's node), and the adaptation itself -- a few
    norms of the iterates of one check, once per event -- is differentiated by autograd on its own small graph.  No torch op per
    iteration.  Three steps on one _AdaptedTape: _replay_epochs re-derives the epochs (segments between the possible events,
    _tape_segments), _walk_back takes them in reverse, the scaling chain by autograd closes."""
    Q, p, A, b, lb, ub = ctx.saved_tensors
    r = ctx.r
    B, n = Q.shape[0], p.shape[1]
    m = get_ncon(A, dim=1)
    dev, dt = p.device, p.dtype
    need = ctx.needs_input_grad
    # ---- the scaling (:160-203) as a graph: leaves -> (Qs, ps, As, bs, lbs, ubs, D, rho0), and ||p||_inf of the unscaled p (:127) ----
    leaves = _graph_leaves((Q, p, A, b, lb, ub), need)
    with torch.enable_grad():
        Qs, ps, As, bs, lbs, ubs, D, _E, rho0 = _scaled_problem(*leaves, r, ctx.has_box)
        p_inf = _inf_norm(leaves[1])
    Dd = D.detach() if torch.is_tensor(D) else torch.ones(B, n, 1, dtype=dt, device=dev)
    rho_e = (rho0.detach().reshape(B, 1, 1).to(dt) if torch.is_tensor(rho0) else torch.full((B, 1, 1), float(rho0), dtype=dt, device=dev)).clone()
    tape = _AdaptedTape(ctx, g, p, B, n, m)
    segs, epochs = _replay_epochs(tape, r, rho_e, Qs.detach(), As.detach() if m > 0 else None, Dd, p_inf.detach())
    rho_bar, dD_extra, dQs_extra, dpinf = _walk_back(tape, r, segs, epochs)
    dQs = tape.tape_sums(need[0])
    if dQs is not None and dQs_extra is not None:
        dQs = dQs + dQs_extra
    ctx.ws = None
    o = tape.out
    pairs = [(Qs, dQs), (ps, o['dps']), (As, o['dAs']), (bs, o['dbs']), (lbs, o['dlbs']), (ubs, o['dubs']), (D, o['dD'] + dD_extra),
             (rho0, rho_bar[0].reshape(B, 1, 1)), (p_inf, dpinf)]
    return tuple(_chain_by_autograd(pairs, leaves)) + (None, None, None)


def _rho_norm_seed(ctx, drho, n):
    """rho = clamp(||Qs||_F / sqrt(n)) (:201-203) when it was not given: inside the clamp ||Qs||_F = rho sqrt(n) with the FORWARD's rho
    and dL/dQs += drho / sqrt(n) * Qs / ||Qs||_F = (drho / (n rho)) Qs; on the clamp nothing passes (no pass over Q for the norm).
    -> the factor (B,) in front of Qs, or None."""
    if ctx.r['rho'] is not None or not ctx.has_box or ctx.rho_fwd is None:
        return None
    B = drho.shape[0]
    rho_f = ctx.rho_fwd.reshape(B).to(drho.dtype)
    inside = (rho_f > ctx.r['rho_min']) & (rho_f < ctx.r['rho_max'])
    return torch.where(inside, drho.reshape(B) / (n * rho_f), torch.zeros_like(rho_f)).contiguous()


def _column_maxima(lib, sp, Qc, B, n):
    """The column maxima of |Q| (:163) on the library's one-pass kernel -> (maxima (B,n), a row that attains each, how many do)"""
    cn = torch.empty((B, n), dtype=Qc.dtype, device=Qc.device)
    arg = torch.empty((B, n), dtype=torch.int32, device=Qc.device)
    cnt = torch.empty((B, n), dtype=torch.int32, device=Qc.device)
    _lib.check(lib.lqp_unroll_scale_colmax(sp, B, n, _lib.ptr(Qc), _lib.ptr(cn), _lib.ptr(arg), _lib.ptr(cnt)), "unroll_scale_colmax")
    return cn, arg, cnt


def _scaling_backward_native(ctx, lib, stream, inputs, need, up):
    """The scaling chain (:160-203) behind the unrolled loop on the library's kernels (include/lqp_amd.h, lqp_unroll_scale_*): column
    maxima of |Q|, the n-sized chain forward (-> the scaling vector), the backward of Qs = D Q D in place over dQs with the
    reductions dL/dd needs, the n-sized chain backward, the scatter of the maxima's gradient: five launches.  As eager torch ops the
    chain was ~150 launches per backward, ~25 of them passes over 128 MB at the headline size -- 2.0 of the 4.2 ms of kernels in an
    unroll step, and host-bound behind that.  LQP_UNROLL_SCALE_NATIVE=2 (and a per-problem beta tensor) keeps autograd for the
    n-sized part; =0 for everything."""
    Q, p, A, b, lb, ub = inputs
    B, n = Q.shape[0], p.shape[1]
    dev, dt = p.device, p.dtype
    r = ctx.r
    Qc = _lib.norm(Q, dt)
    sp = ctypes.c_void_p(stream)
    G = up['dQs']                                          # dL/dQs in, dL/dQ out (in place)
    scale = bool(r['scale'])
    m = get_ncon(A, dim=1)
    beta = r['beta']
    all_native = os.environ.get("LQP_UNROLL_SCALE_NATIVE", "1") != "2" and (not scale or beta is None or not torch.is_tensor(beta))
    s = _rho_norm_seed(ctx, up['drho'], n)
    if all_native:
        # ---- everything on the library's kernels: five launches, no autograd graph (a per-problem beta tensor keeps the hybrid below) ----
        with _lib.on_device(dev):
            slabs = int(lib.lqp_unroll_scale_grad_slabs(B, n))
            parts = torch.empty((B, 1 + slabs, n), dtype=dt, device=dev)
            if not scale:
                _lib.check(lib.lqp_unroll_scale_grad(sp, B, n, _lib.ptr(Qc), None, _lib.ptr(s), _lib.ptr(G), _lib.ptr(parts), slabs), "unroll_scale_grad")
                res = [up['dps'], up['dAs'], up['dbs'], up['dlbs'], up['dubs']]
                return (G,) + tuple(g if (t is not None and nd) else None for g, t, nd in zip(res, (p, A, b, lb, ub), need[1:6])) + (None, None, None)
            cn, arg, cnt = _column_maxima(lib, sp, Qc, B, n)
            dvec = torch.empty((B, n), dtype=dt, device=dev)
            gcn = torch.empty((B, n), dtype=dt, device=dev)
            pc, Ac, bc, lbc, ubc = (_lib.norm(t, dt) for t in (p, A, b, lb, ub))
            mk = lambda t, nd: torch.empty_like(t) if (t is not None and nd) else None
            dp, dA, db, dlb, dub = (mk(t, nd) for t, nd in zip((pc, Ac, bc, lbc, ubc), need[1:6]))
            bg, bv = (0, 0.0) if beta is None else (1, float(beta))
            vec = lambda phase, *tail: lib.lqp_unroll_scale_vectors(sp, B, n, m, phase, int(ctx.has_box), bg, bv, _lib.ptr(cn), _lib.ptr(pc),
                                                                    _lib.ptr(Ac), _lib.ptr(bc), _lib.ptr(lbc), _lib.ptr(ubc), *tail)
            _lib.check(vec(0, None, None, None, None, None, None, None, 0, _lib.ptr(dvec), None, None, None, None, None, None), "unroll_scale_vectors")
            _lib.check(lib.lqp_unroll_scale_grad(sp, B, n, _lib.ptr(Qc), _lib.ptr(dvec), _lib.ptr(s), _lib.ptr(G), _lib.ptr(parts), slabs), "unroll_scale_grad")
            _lib.check(vec(1, _lib.ptr(up['dps']), _lib.ptr(up['dAs']), _lib.ptr(up['dbs']), _lib.ptr(up['dlbs']), _lib.ptr(up['dubs']),
                           _lib.ptr(up['dD']), _lib.ptr(parts), 1 + slabs, None, _lib.ptr(dp), _lib.ptr(dA), _lib.ptr(db), _lib.ptr(dlb),
                           _lib.ptr(dub), _lib.ptr(gcn)), "unroll_scale_vectors")
            _lib.check(lib.lqp_unroll_scale_scatter(sp, B, n, _lib.ptr(Qc), _lib.ptr(cn), _lib.ptr(arg), _lib.ptr(cnt), _lib.ptr(gcn), _lib.ptr(G)),
                       "unroll_scale_scatter")
        shaped = [None if g is None else g.reshape(t.shape) for g, t in zip((dp, dA, db, dlb, dub), (p, A, b, lb, ub))]
        return (G,) + tuple(shaped) + (None, None, None)
    # ---- the hybrid: the passes over Q on the library's kernels, the n-sized rest by autograd ----
    leaves = _graph_leaves((p, A, b, lb, ub), need[1:6])
    cn = arg = cnt = None
    with _lib.on_device(dev):
        if scale:
            cn, arg, cnt = _column_maxima(lib, sp, Qc, B, n)
            cn.requires_grad_(True)
        with torch.enable_grad():
            d, ps, As, bs, lbs, ubs, D, _E, rho = _scaled_problem(None, *leaves, r, ctx.has_box,
                                                                  colmax=cn if scale else torch.empty(0),
                                                                  fro=torch.empty(0) if (r['rho'] is None and ctx.has_box) else None)
        dvec = _lib.norm(d.detach(), dt) if scale else None
        slabs = int(lib.lqp_unroll_scale_grad_slabs(B, n))
        parts = torch.empty((B, 1 + slabs, n), dtype=dt, device=dev)
        _lib.check(lib.lqp_unroll_scale_grad(sp, B, n, _lib.ptr(Qc), _lib.ptr(dvec), _lib.ptr(s), _lib.ptr(G), _lib.ptr(parts), slabs),
                   "unroll_scale_grad")
        # ---- (cn, p, A, b, lb, ub) -> (d, ps, As, bs, lbs, ubs, D) ----
        pairs = [(ps, up['dps']), (As, up['dAs']), (bs, up['dbs']), (lbs, up['dlbs']), (ubs, up['dubs']), (D, up['dD'])]
        if scale:
            pairs.append((d, parts.sum(dim=1)))
        gcn, *res = _chain_by_autograd(pairs, [cn] + leaves)
        if gcn is not None:
            _lib.check(lib.lqp_unroll_scale_scatter(sp, B, n, _lib.ptr(Qc), _lib.ptr(cn.detach()), _lib.ptr(arg), _lib.ptr(cnt),
                                                    _lib.ptr(gcn.contiguous()), _lib.ptr(G)), "unroll_scale_scatter")
    return (G,) + tuple(res) + (None, None, None)


class _NotNative(Exception):
    pass


def unrolled_solve_box_qp(Q, p, A, b, lb, ub, r, has_lb, has_ub, control=None):
    """``r`` is the resolved control (solve_box_qp_admm_torch.resolve_control). Returns x only,
    as the reference does in unroll mode (:328-329)."""
    from .solve_box_qp_admm_torch import check_stop
    check_stop(dict(control or {}, stop=r.get('stop', 'all'), unroll=True))
    if (control is not None and p.dtype in (torch.float32, torch.float64) and (has_lb or has_ub)
            and os.environ.get("LQP_UNROLL_NATIVE", "1") != "0"):
        try:
            ctl = {k: v for k, v in control.items() if k != 'unroll'}
            return _UnrolledLoop.apply(Q, p, A, b, lb, ub, ctl, r, (has_lb, has_ub))
        except _NotNative:
            pass                   # (LU path / adapted rho: the taped loop below)
    return _eager_unrolled(Q, p, A, b, lb, ub, r, has_lb, has_ub)


def _eager_unrolled(Q, p, A, b, lb, ub, r, has_lb, has_ub, solver_cls=TorchLU):
    """The loop as ordinary differentiable torch ops; every x-update is ``TorchLU`` (lqp_py_amd/lu_layer.py): HIP batched
    LU factor + cached solves with the analytic backward of lu_layer.py:41-58.  (solver_cls: tests substitute a CPU
    float64 stand-in for the HIP layer to obtain a higher-precision truth of the same taped computation.)"""
    dev, dt = p.device, p.dtype
    B, n = Q.shape[0], p.shape[1]
    m = get_ncon(A, dim=1)
    has_box = has_lb or has_ub
    p_inf = _inf_norm(p)
    Q, p, A, b, lb, ub, D, E, rho = _scaled_problem(Q, p, A, b, lb, ub, r, has_box)

    M = _kkt_matrix(Q, A, rho)
    solver = solver_cls(A=M)                      # HIP factorisation, no_grad inside

    x = z = u = torch.zeros(B, n, 1, dtype=dt, device=dev)
    tiny = torch.full((1,), _TINY, dtype=dt, device=dev)
    thr = torch.full((1,), float(r['adaptive_rho_threshold']), dtype=dt, device=dev)
    r_inf = s_inf = pri = dua = None
    wants = r['adaptive_rho']
    for it in range(r['max_iters']):
        if (r['adaptive_rho'] and it % r['adaptive_rho_iter'] == 0 and 0 < it < r['adaptive_rho_max_iter']
                and bool(torch.any(wants))):
            ratio = (torch.clamp(r_inf / pri, min=_TINY) / torch.clamp(s_inf / dua, min=_TINY)) ** 0.5
            if bool((ratio > r['adaptive_rho_tol']).any()) or bool((ratio < 1 / r['adaptive_rho_tol']).any()):
                rho = rho * torch.logical_not(wants) + (rho * ratio) * wants
                rho = torch.clamp(rho, min=r['rho_min'], max=r['rho_max'])
                M = _kkt_matrix(Q, A, rho)
                solver = solver_cls(A=M)
        rhs = -p + rho * (z - u)
        if m > 0:
            rhs = torch.cat((rhs, b), 1)
        xv = solver(A=M, b=rhs)
        x = xv[:, :n, :]
        z_old = z
        z = x + u
        if has_lb:
            z = torch.maximum(z, lb)
        if has_ub:
            z = torch.minimum(z, ub)
        res = x - z
        s = rho * (z - z_old)
        u = u + res
        if it % r['check_solved'] == 0:
            r_inf, s_inf = _inf_norm(D * res), _inf_norm(D * s)
            pri = torch.maximum(torch.maximum(_inf_norm(D * x), _inf_norm(D * z)), tiny)
            dua = torch.maximum(torch.maximum(torch.maximum(_inf_norm(rho * D * u), _inf_norm(torch.matmul(Q, x) / D)),
                                              p_inf), tiny)
            tol_p = r['eps_abs'] + r['eps_rel'] * pri
            tol_d = r['eps_abs'] + r['eps_rel'] * dua
            wants = torch.logical_or(r_inf > torch.maximum(tol_p, thr), s_inf > torch.maximum(tol_d, thr))
            if bool(torch.all(torch.logical_and(r_inf < tol_p, s_inf < tol_d))):
                break
    return D * x
