"""The separable terms a box-QP layer can carry in its objective (solve_box_qp_l1 / _soft / _log / _pwl / _huber): one record per term, and what the
layers share -- the rules of what a term cannot be combined with, the forward solve, the body of ``Function.forward`` and the
prelude of ``Function.backward``.  What is a term's own stays in its module: the docstrings, the two element-wise kernels around the
fixed-point backward, and the gradients it returns.  The device-side twin is the Term trait of csrc/lqp_boxqp.hpp.
"""
import collections
import ctypes
import types

import torch

from . import _lib
from . import solve_box_qp_admm_torch as _S
from .utils import get_ncon

# label: the layer's name in messages | inputs: the names of its input tensors, each of p's shape (or of `shapes`) | aux: the key of the output that
# tells the backward where every element rests | entry, size_of: the library's forward and workspace-size function | outputs: the
# order of the two extra outputs in the C argument list (behind rho_out) | device_check: what the input check made on the device
# says (status 1) | kkt_reason: why control['backward'] = 'kkt' is refused | shapes: None = every input has p's shape, else
# shapes(p, tensors) -> the shape each input must have (it raises where they cannot be told)
Term = collections.namedtuple("Term", "label inputs aux entry size_of outputs device_check kkt_reason shapes", defaults=(None,))

L1 = Term("L1", ("w", "c"), "side", "lqp_boxqp_forward_l1", "lqp_boxqp_forward_l1_workspace_bytes", ("aux", "u_box"),
          "w must be finite and >= 0, and rho positive and finite",
          "its backward is the fixed-point form on the effective box")
SOFT = Term("soft-band", ("wl", "wu", "lo", "hi"), "zone", "lqp_boxqp_forward_soft", "lqp_boxqp_forward_soft_workspace_bytes", ("aux", "u_box"),
            "wl and wu must be finite and >= 0, lo <= hi without NaN, and rho positive and finite",
            "its backward is the fixed-point form on the effective box")
LOG = Term("log-barrier", ("w",), "curv", "lqp_boxqp_forward_log", "lqp_boxqp_forward_log_workspace_bytes", ("u_box", "aux"),
           "w must be finite and >= 0, ub > 0 wherever w > 0, and rho positive and finite",
           "its backward is the fixed-point form with the barrier's curvature")


def _pwl_shapes(p, tensors):
    """s (B, n, K + 1) and c (B, n, K) with 1 <= K <= 3: K is read from c"""
    c = tensors[1]
    if not torch.is_tensor(c) or c.dim() != 3 or not 1 <= c.shape[2] <= 3:
        _S._bad(f"c must be a tensor of shape {tuple(p.shape[:2])} + (K,) with 1 <= K <= 3 kinks per element")
    K = int(c.shape[2])
    return (tuple(p.shape[:2]) + (K + 1,), tuple(p.shape[:2]) + (K,))


PWL = Term("piecewise-linear", ("s", "c"), "piece", "lqp_boxqp_forward_pwl", "lqp_boxqp_forward_pwl_workspace_bytes", ("aux", "u_box"),
           "s must be finite and non-decreasing, c non-decreasing without NaN, and rho positive and finite",
           "its backward is the fixed-point form on the effective box", _pwl_shapes)
HUBER = Term("Huber", ("w", "c", "delta"), "zone", "lqp_boxqp_forward_huber", "lqp_boxqp_forward_huber_workspace_bytes", ("aux", "u_box"),
             "w must be finite and >= 0, delta >= 0 without NaN, c finite, and rho positive and finite",
             "its backward is the fixed-point form with the term's curvature on the quadratic zone")


def check_term(term, control, p=None, tensors=()):
    """What a layer with a term cannot be combined with, and the shapes and dtypes of the term's inputs.  Raises the package's
    ValueError at the call, before any launch; the one place that holds these rules."""
    if control.get('stop', 'all') != 'all':
        _S._bad(f"the {term.label} layer has no per-problem stop: control['stop'] = 'each' cannot be combined with it")
    for key in ('infeasible', 'unbounded'):
        if control.get(key) is not None:
            _S._bad(f"control['{key}'] cannot be combined with the {term.label} layer: the certificates belong to the per-problem stop")
    if control.get('unroll', False):
        _S._bad(f"unroll=True cannot be combined with the {term.label} layer: the tape replays the plain step")
    if control.get('backward', 'fixed_point') == 'kkt':
        _S._bad(f"control['backward'] = 'kkt' cannot be combined with the {term.label} layer: {term.kkt_reason}")
    if any(control.get(k) is not None for k in ('_global_bounds', '_bound_flags_dev', '_check_hook', '_owner')) or \
            control.get('dist_strict_stop', False):
        _S._bad(f"the sharded wrapper (lqp_py_amd.dist) does not carry the {term.label} layer")
    rho = control.get('rho')
    if rho is not None and not torch.is_tensor(rho) and not float(rho) > 0.0:
        _S._bad(f"control['rho'] must be positive (or None) for the {term.label} layer: it always iterates")
    if p is None:
        return
    shapes = (tuple(p.shape),) * len(term.inputs) if term.shapes is None else term.shapes(p, tensors)
    for name, t, shape in zip(term.inputs, tensors, shapes):
        if not torch.is_tensor(t) or tuple(t.shape) != shape:
            _S._bad(f"{name} must be a tensor of " + ("p's " if term.shapes is None else "") + f"shape {shape}")
        if t.dtype != p.dtype:
            _S._bad(f"{name} must have p's dtype {p.dtype}, got {t.dtype}")


def solve(term, qp, tensors, control, sync=True, lower=None):
    """The forward solve of a layer with `term`: qp = (Q, p, A, b, lb, ub), tensors = the term's inputs in the record's order.
    lower: tensors -> the arguments the record's entry point takes in their place (tensors, and plain ints as they are), for a term
    whose inputs reach the library in another layout."""
    check_term(term, control, qp[1], tensors)
    _lib.require_gpu(*tensors)
    # (bounds known = "some bound is finite": the loop schedule whatever the data hold; nothing is assumed, compared or remembered)
    return _S._forward_solve(*qp, control, bounds=(True, True), sync=sync, term=(term, tuple(tensors) if lower is None else tuple(lower(tensors))))


def layer_forward(ctx, term, qp, tensors, control, keep, inputs, lower=None):
    """The body of a layer's Function.forward: solve, and save for the backward the solution's tensors named in `keep`, then `inputs`."""
    sync = bool(control.get('sync', True))
    sol = solve(term, qp, tensors, control, sync=sync, lower=lower)
    ctx.rho, ctx.sync = sol['rho'], sync
    ctx.linsolve = int(sol['_stats']['linsolve_used'])
    ctx.save_for_backward(*(sol[k] for k in keep), *inputs)
    return sol['x']


def backward_prelude(ctx, x, Q, A, box_grads=None):
    """The head of a layer's Function.backward: library, dims, stream, the rho argument of the element-wise kernels, and the `want`
    dict of the fixed-point backward (box_grads: whether it returns dlb and dub; None: as the caller needs them)."""
    need = ctx.needs_input_grad
    B, n = Q.shape[0], Q.shape[1]
    rho_mode, rho_value, rho_tensor = _S._per_problem_argument('rho', '(B,1,1)', ctx.rho, B, x)
    has_eq = get_ncon(A, dim=1) > 0
    want = dict(dQ=need[0], dp=True, dA=need[2] and has_eq, db=need[3] and has_eq,
                dlb=need[4] if box_grads is None else box_grads, dub=need[5] if box_grads is None else box_grads)
    return types.SimpleNamespace(need=need, lib=_lib.load(), B=B, n=n, dt=_lib.dtype_code(x), dev=x.device, dty=x.dtype,
                                 stream=ctypes.c_void_p(_lib.current_stream_handle(x.device)),
                                 rho_mode=rho_mode, rho_value=rho_value, rho_tensor=rho_tensor, want=want)
