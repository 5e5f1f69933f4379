"""The log-barrier layer on the GPU: every row of tests/log_table.py against its truth at a pinned iteration count, zero weights
against the plain forward bit for bit, all seven gradients through the module, a solve that stops by itself, a memory row, the
refusals made on the device, sync=False; and the curvature hook of the fixed-point backward (lqp_boxqp_backward_fp_curv) called
directly on the synthetic fixed points of tests/fp_table.py.  GPU only.

The bars are tests/tier_table.py's (`compare`): float32 |hip - t64| <= R |t32 - t64| + F scale, float64 1e-9 scale, t32 / t64 the
truth (log_table.solve_log) in float32 / float64.  The clamped set (u_box != 0) is compared exactly; an element may differ only where
the float64 truth says its S sits within the bar for z of a bound (log_table.excused), and at most 1 % of a problem's elements may.
`curv` jumps between w / z^2 and 0 where an element changes sets (u_box does not: u + t / z tends to 0 at the bound), so the
elements inside that margin are left out of its comparison, in the GPU's values and in the float32 truth's alike.
tests/test_log_table.py shows, without a GPU, that the iterate of the plain step misses every row's bar for z by at least 100 x.
The gradients' bars are the ones tests/test_gpu_fp.py uses, fp_table.compare: tier_table.compare over every gradient.
"""
import pytest
import torch

import lqp_py_amd as L
from lqp_py_amd import _lib
import lqp_py_amd.solve_box_qp_admm_torch as SB
import fp_table as FT
import log_table as G
import term_checks as C
from term_checks import _control, _pick, _report, dev, cus          # (the fixtures, by name)
import tier_table as T

pytestmark = pytest.mark.gpu
LAYER = (G.TERM, L.torch_solve_box_qp_log, L.SolveBoxQPLog)


@pytest.mark.parametrize("key", list(G.ROWS))
def test_row_against_the_truth(dev, cus, monkeypatch, key):
    args, got, idx, t32, t64, res = C.row_against_the_truth(LAYER, dev, cus, monkeypatch, key)
    # curv: the elements inside the margin take the float64 truth's value on both sides (see the module's docstring)
    ex = G.excused(t64, res["z"]["bar"])
    c64 = t64["curv"]
    chip = torch.where(ex, c64, got["curv"].double())
    c32 = None if t32 is None else dict(t32, curv=torch.where(ex, c64, t32["curv"].double()))
    rec = T.compare(G.ROWS[key], {"curv": chip}, c32, t64, keys=("curv",))
    _report(key, rec)
    assert rec["curv"]["ok"], (key, rec)
    assert bool((got["z"][_pick(args[6], idx) > 0] > 0).all()), (key, "z > 0 on the barrier elements")


@pytest.mark.parametrize("name", G.SAME_BITS)
def test_zero_weights_are_the_plain_forward_bit_for_bit(dev, cus, monkeypatch, name):
    zero = C.zero_term_is_the_plain_forward(LAYER, dev, cus, monkeypatch, name)
    assert not bool(zero["curv"].any()) and bool(torch.isfinite(zero["u_box"]).all())


@pytest.mark.parametrize("name", list(G.GRAD_ROWS))
def test_all_seven_gradients_through_the_module(dev, cus, monkeypatch, name):
    res, _, g64, t64, sub, cot = C.gradients_through_the_module(LAYER, dev, cus, monkeypatch, name)
    assert float(g64["dw"].abs().max()) > 0 and float(t64["curv"].max()) > 0          # (the new gradient and the curvature are not trivially zero)
    # ... and the curvature matters: the recipe without it is far outside the bar for dp
    flat = G.grad_recipe(cot.double(), dict(t64, curv=torch.zeros_like(t64["curv"])), *[None if sub[k] is None else sub[k].double() for k in (0, 2, 4, 5, 6)])
    assert float((flat["dp"] - g64["dp"]).abs().max()) > 100 * res["dp"]["bar"]


def test_a_solve_that_stops_by_itself_takes_the_truths_iterations(dev):
    C.stopped_solve_takes_the_truths_iterations(LAYER, dev)


def test_no_result_depends_on_what_the_new_memory_held(dev, cus, monkeypatch):
    """In the manner of tests/mem_table.py, on tests/memharness.py: every workspace (the two new regions behind the forward's layout
    among them), output and temporary of a forward and a backward through the module is a guarded buffer filled with 0x00, then with
    0xFF -- the same bits come back, no guard is touched."""
    C.no_result_depends_on_what_the_new_memory_held(LAYER, dev, cus, monkeypatch, "lqp_boxqp_forward_workspace_bytes")


MESSAGE = r"w must be finite and >= 0, ub > 0 wherever w > 0, and rho positive and finite \(batch index %d\)"


def test_bad_barrier_data_are_refused_on_the_device(dev):
    """checked where the data are: the call that waits raises the package's ValueError and names the problem (LQP_ERR_INVALID with
    fail_index underneath), the problem's outputs are NaN and bit 20 of its flag word is set; the next call works"""
    r = G.ROWS["small_n31_m1-K10"]
    args = [None if t is None else t.to(dev) for t in G.log_inputs(r, 4)]
    e = int(torch.nonzero(args[6][2, :, 0] > 0)[0])          # a barrier element of problem 2

    def solve(**over):
        a = list(args)
        for k, v in over.items():
            a[dict(ub=5, w=6)[k]] = v
        return L.torch_solve_box_qp_log(*a, _control(r))

    def planted(k, b, i, value):
        t = args[dict(ub=5, w=6)[k]].clone()
        t[b, i, 0] = value
        return {k: t}
    for value in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=MESSAGE % 2):
            solve(**planted("w", 2, 5, value))
    # w_i > 0 with ub_i <= 0: the domain is empty
    for value in (0.0, -0.5):
        with pytest.raises(ValueError, match=MESSAGE % 2):
            solve(**planted("ub", 2, e, value))
    # ... while ub_i <= 0 under w_i = 0 is data, not an error
    z0 = int(torch.nonzero(args[6][1, :, 0] == 0)[0])
    ok = solve(**planted("ub", 1, z0, max(-0.5, float(args[4][1, z0, 0]))))
    assert ok["iter"] == r["K"] and bool(torch.isfinite(ok["x"]).all())
    # a per-problem rho: t is a threshold only for a positive, finite one
    for value in (0.0, -1.0, float("inf")):
        rho = torch.ones(4, 1, 1, device=dev)
        rho[1] = value
        with pytest.raises(ValueError, match=MESSAGE % 1):
            L.torch_solve_box_qp_log(*args, _control(r, rho=rho))
    # the C entry itself, un-synchronised through the module: NaN outputs for the bad problem alone, bit 20 in its flag word
    bad_w = planted("w", 3, 5, -1.0)["w"]
    x = L.SolveBoxQPLog(control=_control(r, sync=False))(*args[:6], bad_w)
    torch.cuda.synchronize()
    assert bool(torch.isnan(x[3]).all()) and bool(torch.isfinite(x[:3]).all())
    with pytest.raises(RuntimeError, match=r"w must be finite and >= 0.*batch index 3"):
        _lib.poll_errors(block=True)
    sol = solve()          # (the workspace and the layer are as good as before)
    assert sol["iter"] == r["K"] and bool(torch.isfinite(sol["x"]).all())


# ---------------------------------------------------------------------------
# the curvature hook, called directly on the synthetic fixed points of tests/fp_table.py
# ---------------------------------------------------------------------------
CURV_ROWS = ("chol_nf1_n130", "chol_nf64_n150", "chol_nf65_n150", "chol_mixed_m2_n576", "chol_nf0_among_n200", "chol_equil0_nf200_n330",
             "lu_nf65_n150_f64", "lu_nf100_n200", "lu_full_nf100_n200", "lu_nonsym_nf150_n300")


def _curv_of(r, pt):
    """a random non-negative diagonal on the free set of the point (float32 and float64 agree on it: fp_table._point), spread over
    1e-3 .. 10, zero on the clamped set (the all-zero diagonal has a test of its own below)"""
    free = FT.free_set(pt, torch.float64).unsqueeze(2)
    g = torch.Generator().manual_seed(T.seed_of(r) + 77)
    c = 10.0 ** (-3 + 4 * torch.rand(free.shape, generator=g, dtype=torch.float64)) * free
    return c.to(FT.dtype_of(r))


def _full_want(r):
    return dict(dQ=True, dp=True, dA=r["m"] > 0, db=r["m"] > 0, dlb=True, dub=True)


def _bwd(r, gpu_pt, curv, use_curv_entry=True):
    cot, rest = gpu_pt[0], gpu_pt[1:]
    linsolve = 2 if r["entry"] == "chol" else 1
    _lib.profile(enable=True, reset=True)
    try:
        if use_curv_entry:
            prep = SB._fp_backward_prepare(*rest, _full_want(r), linsolve=linsolve)
            out = _run_curv(prep, cot, curv)
        else:
            out = SB._fp_backward(cot, *rest, _full_want(r), linsolve=linsolve)
        torch.cuda.synchronize()
        used = _lib.profile()
    finally:
        _lib.profile(enable=False)
    return dict(zip(FT.GRADS, out[:6])), tuple(used[c][1] for c in FT.PROF_CLASSES)


def _run_curv(prep, cot, curv):
    """lqp_boxqp_backward_fp_curv itself, with a null pointer when `curv` is None (SB._fp_backward_run takes the plain entry then)"""
    if curv is not None:
        return SB._fp_backward_run(prep, cot, curv=curv)
    gc = _lib.norm(cot, prep['dty'])
    tail = prep['tail'][:8] + (None,) + prep['tail'][8:]
    _lib.workspace_touch(prep['dev'], "bwd", prep['stream'])
    prep['ran'] = True
    SB._backward_call(prep['lib'].lqp_boxqp_backward_fp_curv, (*prep['head'], _lib.ptr(gc), *tail, prep['linsolve'], prep['rep']),
                      "torch_solve_box_qp_grad", prep['fail'], prep['report'], prep['dev'], prep['B'], prep['sync'])
    return prep['grads']


@pytest.mark.parametrize("name", CURV_ROWS)
def test_curvature_backward_against_the_oracle(dev, cus, monkeypatch, name):
    """truth: the float64 oracle's backward on Q + diag(curv); the budget: the float32 oracle's on the same"""
    r = FT.ROW_BY_NAME[name]
    B = T.batch(r, cus)
    pt = FT.point(r, B)
    curv = _curv_of(r, pt)
    idx = torch.tensor(T.sample(B))
    sub = tuple(t[idx] if torch.is_tensor(t) else t for t in pt)
    csub = curv[idx]
    assert bool((csub >= 0).all()) and float(csub.max()) > 0 and not bool(csub[~FT.free_set(sub, torch.float64).unsqueeze(2)].any())
    gpu_pt = tuple(t.to(dev) if torch.is_tensor(t) else t for t in pt)
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    grads, ran = _bwd(r, gpu_pt, curv.to(dev))
    assert ran == FT.FORMS[r["form"]], (name, dict(zip(FT.PROF_CLASSES, ran)))

    def with_curv(args):
        args = list(args)
        args[5] = args[5] + torch.diag_embed(csub.to(args[5].dtype)[:, :, 0])
        return args
    t64 = FT.oracle(sub, torch.float64, hook=with_curv)
    t32 = FT.oracle(sub, torch.float32, hook=with_curv) if r["dtype"] == "f32" else None
    hip = {k: (None if v is None else v[idx.to(dev)].cpu()) for k, v in grads.items()}
    res = FT.compare(r, hip, t32, t64)
    _report(name, res)
    assert set(res) == {k for k in FT.GRADS if t64[k] is not None}
    # the diagonal matters at this point: the backward without it is far outside the bar for dp (not where every free set is tiny)
    flat = FT.oracle(sub, torch.float64)
    far = float((flat["dp"] - t64["dp"]).abs().max())
    print(name, "without curv: dp off by %.3e" % far)
    assert far > 100 * res["dp"]["bar"], (far, res["dp"])
    bad = [(k, rec) for k, rec in res.items() if not rec["ok"]]
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", ("chol_nf65_n150", "lu_nf100_n200"))
def test_null_and_zero_curvature_are_the_plain_backward_bit_for_bit(dev, cus, monkeypatch, name):
    r = FT.ROW_BY_NAME[name]
    B = T.batch(r, cus)
    gpu_pt = tuple(t.to(dev) if torch.is_tensor(t) else t for t in FT.point(r, B))
    plain, ran0 = _bwd(r, gpu_pt, None, use_curv_entry=False)
    null, ran1 = _bwd(r, gpu_pt, None)
    zero, ran2 = _bwd(r, gpu_pt, torch.zeros_like(gpu_pt[1]))
    assert ran0 == ran1 == ran2 == FT.FORMS[r["form"]]
    for k in FT.GRADS:
        if plain[k] is None:
            assert null[k] is None and zero[k] is None
        else:
            assert torch.equal(plain[k], null[k]) and torch.equal(plain[k], zero[k]), k
