"""The Huber layer on the GPU: every row of tests/huber_table.py against its truth at a pinned iteration count, zero weights against
the plain forward bit for bit, all nine gradients through the module, a solve that stops by itself, a memory row, the refusals made
on the device; and the curvature path of this layer -- `k_huber_effective_duals`' curv into lqp_boxqp_backward_fp_curv -- on the
synthetic fixed points of tests/fp_table.py.  GPU only.

The bars are tests/tier_table.py's (`compare`): float32 |hip - t64| <= R |t32 - t64| + F scale, float64 1e-9 scale, t32 / t64 the
truth (huber_table.solve_huber) in float32 / float64.  `zone` is compared exactly; an element may differ only where the float64 truth
says it sits within the bar for z of changing its set (huber_table.excused), and at most 1 % of a problem's elements may.
tests/test_huber_table.py shows, without a GPU, that the iterates of the plain step, of the pure quadratic step and of the L1 step at
weight w delta miss every row's bar for z by at least 100 x.  The gradients' bars are the ones tests/test_gpu_fp.py uses,
fp_table.compare: tier_table.compare over every gradient.
"""
import ctypes

import pytest
import torch

import lqp_py_amd as L
from lqp_py_amd import _lib
import lqp_py_amd.solve_box_qp_admm_torch as SB
from oracle import boxqp_oracle as O
import fp_table as FT
import huber_table as G
import term_checks as C
from term_checks import _control, _report, dev, cus          # (the fixtures, by name)
import tier_table as T

pytestmark = pytest.mark.gpu
LAYER = (G.TERM, L.torch_solve_box_qp_huber, L.SolveBoxQPHuber)


@pytest.mark.parametrize("key", list(G.ROWS))
def test_row_against_the_truth(dev, cus, monkeypatch, key):
    C.row_against_the_truth(LAYER, dev, cus, monkeypatch, key)


@pytest.mark.parametrize("name", G.SAME_BITS)
def test_zero_weights_are_the_plain_forward_bit_for_bit(dev, cus, monkeypatch, name):
    zero = C.zero_term_is_the_plain_forward(LAYER, dev, cus, monkeypatch, name)
    assert not bool(zero["zone"].any()) and bool(torch.isfinite(zero["u_box"]).all())          # (no weight, no zone)


@pytest.mark.parametrize("name", list(G.GRAD_ROWS))
def test_all_nine_gradients_through_the_module(dev, cus, monkeypatch, name):
    res, _, g64, t64, sub, cot = C.gradients_through_the_module(LAYER, dev, cus, monkeypatch, name)
    for k in ("dw", "dc", "ddelta"):
        assert float(g64[k].abs().max()) > 0, k          # (the new gradients are not trivially zero)
    # ... and the curvature matters: the recipe without it (w = 0 in curv_of alone) is far outside the bar for dp
    d = [None if t is None else t.double() for t in sub]
    u_e = t64["u_box"]
    y = t64["rho"] * u_e
    flat = O.solve_box_qp_grad(cot.double(), t64["x"], u_e, torch.cat((torch.relu(-y), torch.relu(y)), 1), t64["nus"], d[0], d[2], d[4], d[5],
                                 t64["rho"])[1]
    assert float(G.curv_of(t64, d[6]).max()) > 0
    assert float((flat - g64["dp"]).abs().max()) > 100 * res["dp"]["bar"]


def test_a_solve_that_stops_by_itself_takes_the_truths_iterations(dev):
    C.stopped_solve_takes_the_truths_iterations(LAYER, dev)


def test_no_result_depends_on_what_the_new_memory_held(dev, cus, monkeypatch):
    """In the manner of tests/mem_table.py, on tests/memharness.py: every workspace (the six new regions behind the forward's layout
    among them), output and temporary of a forward and a backward through the module is a guarded buffer filled with 0x00, then with
    0xFF -- the same bits come back, no guard is touched."""
    C.no_result_depends_on_what_the_new_memory_held(LAYER, dev, cus, monkeypatch, "lqp_boxqp_forward_l1_workspace_bytes")


MESSAGE = r"w must be finite and >= 0, delta >= 0 without NaN, c finite, and rho positive and finite \(batch index %d\)"
# (what is planted, the input it goes into, the problem that holds it)
BAD = {"negative_w": (6, -1e-3, 1), "infinite_w": (6, float("inf"), 2), "negative_delta": (8, -1e-3, 0), "nan_delta": (8, float("nan"), 2),
       "infinite_c": (7, float("inf"), 1)}


def _small_batch(dev):
    """n = 8, B = 3, m = 1"""
    g = torch.Generator().manual_seed(5)
    n, B = 8, 3
    Gm = torch.randn(B, 12, n, generator=g)
    Q = Gm.transpose(1, 2) @ Gm / 12 + 0.2 * torch.eye(n)
    p, A = torch.randn(B, n, 1, generator=g), torch.randn(B, 1, n, generator=g)
    lb, ub = -(0.3 + torch.rand(B, n, 1, generator=g)), 0.3 + torch.rand(B, n, 1, generator=g)
    b = A @ (0.1 * torch.rand(B, n, 1, generator=g))
    w, c = 0.5 + torch.rand(B, n, 1, generator=g), 0.3 * torch.randn(B, n, 1, generator=g)
    delta = 0.05 + 0.3 * torch.rand(B, n, 1, generator=g)
    return [t.to(dev) for t in (Q, p, A, b, lb, ub, w, c, delta)]


@pytest.mark.parametrize("case", list(BAD))
def test_bad_data_are_refused_on_the_device(dev, case):
    """One bad element in one problem of a small batch, checked where the data are: the call that waits raises the package's
    ValueError and names the problem (LQP_ERR_INVALID with fail_index underneath); un-synchronised through the module the problem's
    outputs are NaN, the others' are not, and bit 22 of its flag word is set -- the late report names it; the next call works"""
    which, value, b = BAD[case]
    args = _small_batch(dev)
    ctl = dict(max_iters=21, eps_abs=1e-12, eps_rel=1e-12)
    bad = list(args)
    bad[which] = args[which].clone()
    bad[which][b, 5, 0] = value
    with pytest.raises(ValueError, match=MESSAGE % b):
        L.torch_solve_box_qp_huber(*bad, L.box_qp_control(**ctl))
    x = L.SolveBoxQPHuber(control=L.box_qp_control(sync=False, **ctl))(*bad)
    torch.cuda.synchronize()
    others = [i for i in range(3) if i != b]
    assert bool(torch.isnan(x[b]).all()) and bool(torch.isfinite(x[others]).all())
    with pytest.raises(RuntimeError, match=r"w must be finite and >= 0, delta >= 0.*batch index %d" % b):          # (raised on RP_HUBER_INPUT alone)
        _lib.poll_errors(block=True)
    assert _lib.RP_HUBER_INPUT == 1 << 22
    # ... while an infinite delta and a zero delta are data, not errors; the workspace and the layer are as good as before
    good = list(args)
    good[8] = args[8].clone()
    good[8][b, 5, 0] = float("inf")
    good[8][b, 6, 0] = 0.0
    sol = L.torch_solve_box_qp_huber(*good, L.box_qp_control(**ctl))
    assert sol["iter"] > 0 and all(bool(torch.isfinite(sol[k]).all()) for k in ("x", "z", "u", "zone", "u_box"))


# ---------------------------------------------------------------------------
# the curvature path of this layer on the synthetic fixed points of tests/fp_table.py: k_huber_effective_duals' outputs into
# lqp_boxqp_backward_fp_curv, against the float64 oracle on Q + diag(curv)
# ---------------------------------------------------------------------------
CURV_ROWS = ("chol_nf65_n150", "lu_nf100_n200")


def _zones_and_weights(r, pt):
    """zone in {-1, 0, 1} and w >= 0 with zeros, drawn for every element of the point -- clamped ones too: curv must be 0 there"""
    g = torch.Generator().manual_seed(T.seed_of(r) + 91)
    shape = pt[1].shape
    zone = torch.randint(-1, 2, shape, generator=g).to(FT.dtype_of(r))
    w = (0.2 + 2.0 * torch.rand(shape, generator=g, dtype=torch.float64)) * (torch.rand(shape, generator=g) > 0.25)
    return zone, w.to(FT.dtype_of(r))


@pytest.mark.parametrize("name", CURV_ROWS)
def test_curvature_path_against_the_oracle(dev, cus, monkeypatch, name):
    """truth: the float64 oracle's backward on Q + diag(curv) with u_e, lams_e as the layer builds them; the budget: the float32
    oracle's on the same (the bars of test_gpu_log.py's curvature rows, fp_table.compare)"""
    r = FT.ROW_BY_NAME[name]
    B, n = T.batch(r, cus), r["n"]
    pt = FT.point(r, B)
    rho = float(pt[9])
    zone, w = _zones_and_weights(r, pt)
    u_box = pt[2]
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    d_ubox, d_zone, d_w = u_box.to(dev), zone.to(dev), w.to(dev)
    u_e, curv, lams_e = torch.empty_like(d_ubox), torch.empty_like(d_ubox), torch.empty((B, 2 * n, 1), dtype=d_ubox.dtype, device=dev)
    lib = _lib.load()
    with _lib.on_device(dev):
        _lib.check(lib.lqp_boxqp_huber_effective_duals(ctypes.c_void_p(_lib.current_stream_handle(dev)), _lib.dtype_code(d_ubox), B, n,
                                                       _lib.ptr(d_ubox), _lib.ptr(d_zone), _lib.ptr(d_w), 1, rho, None, _lib.ptr(u_e),
                                                       _lib.ptr(lams_e), _lib.ptr(curv)), "huber_effective_duals")
    torch.cuda.synchronize()
    # the kernel's three outputs, exactly
    want_curv = torch.where((zone == 0) & (w > 0) & (u_box == 0), w, torch.zeros_like(w))
    y = torch.tensor(rho, dtype=u_box.dtype) * u_box
    assert torch.equal(u_e.cpu(), u_box) and torch.equal(curv.cpu(), want_curv)
    assert torch.equal(lams_e.cpu(), torch.cat((torch.relu(-y), torch.relu(y)), 1))
    free = FT.free_set(pt, torch.float64).unsqueeze(2)
    assert float(want_curv.max()) > 0 and not bool(want_curv[~free].any()) and int(((want_curv == 0) & free).sum()) > 0
    # the backward with them
    gpu_pt = tuple(t.to(dev) if torch.is_tensor(t) else t for t in pt)
    want = dict(dQ=True, dp=True, dA=r["m"] > 0, db=r["m"] > 0, dlb=True, dub=True)
    _lib.profile(enable=True, reset=True)
    try:
        prep = SB._fp_backward_prepare(gpu_pt[1], u_e, lams_e, *gpu_pt[4:], want, linsolve=2 if r["entry"] == "chol" else 1)
        out = SB._fp_backward_run(prep, gpu_pt[0], curv=curv)
        torch.cuda.synchronize()
        used = _lib.profile()
    finally:
        _lib.profile(enable=False)
    ran = tuple(used[c][1] for c in FT.PROF_CLASSES)
    assert ran == FT.FORMS[r["form"]], (name, dict(zip(FT.PROF_CLASSES, ran)))
    idx = torch.tensor(T.sample(B))
    sub = tuple(t[idx] if torch.is_tensor(t) else t for t in pt)
    csub = want_curv[idx]

    def as_the_layer(args):
        args = list(args)
        yy = args[9] * args[2]
        args[3] = torch.cat((torch.relu(-yy), torch.relu(yy)), 1)
        args[5] = args[5] + torch.diag_embed(csub.to(args[5].dtype)[:, :, 0])
        return args
    t64 = FT.oracle(sub, torch.float64, hook=as_the_layer)
    t32 = FT.oracle(sub, torch.float32, hook=as_the_layer) if r["dtype"] == "f32" else None
    hip = {k: (None if v is None else v[idx.to(dev)].cpu()) for k, v in zip(FT.GRADS, out[:6])}
    res = FT.compare(r, hip, t32, t64)
    _report(name, res)
    assert set(res) == {k for k in FT.GRADS if t64[k] is not None}

    def without_curv(args):
        args = as_the_layer(args)
        args[5] = args[5] - torch.diag_embed(csub.to(args[5].dtype)[:, :, 0])
        return args
    far = float((FT.oracle(sub, torch.float64, hook=without_curv)["dp"] - t64["dp"]).abs().max())
    print(name, "without curv: dp off by %.3e" % far)
    assert far > 100 * res["dp"]["bar"], (far, res["dp"])
    bad = [(k, rec) for k, rec in res.items() if not rec["ok"]]
    assert not bad, (name, bad)
