"""tests/pwl_table.py on the CPU: the truth of the piecewise-linear layer is solve_l1 at K = 1 with slopes (-w, w), solve_soft at K = 2
with slopes (-wl, 0, wu) and the oracle's loop at zero slopes, bit for bit, padded to three kinks too; it satisfies the optimality
conditions of the problem it claims to solve, piece by piece; its gradient recipe matches central differences in all eight arguments;
every row populates the seven pieces and the clamped set; a kernel that ignores the term or its middle kink cannot pass; the Python
and C entry points refuse what they cannot run.  No GPU.
"""
import ctypes
import os
import re

import pytest
import torch

import lqp_py_amd as L
import lqp_py
from lqp_py_amd import _lib
from lqp_py_amd import solve_box_qp_pwl as SP
from oracle import boxqp_oracle as O
import l1_table as LT
import pwl_table as PT
import soft_table as ST
import term_checks as C
import tier_table as T

CUS = C.CUS
HERE = os.path.dirname(os.path.abspath(__file__))


def _same(a, b):
    return (torch.equal(a, b) if torch.is_tensor(a) else a == b)


@pytest.mark.parametrize("name", ["small_n31_m1", "sweep2_n129_m1", "lu_nonsym_n300"])
def test_zero_slopes_are_the_oracle_bit_for_bit(name):
    r = dict(T.ROW_BY_NAME[name], pwl="plain", soft="plain", l1="plain", alpha=1.0, K=30)
    for dt in (torch.float32, torch.float64):
        inp = [None if t is None else t.to(dt) for t in PT.pwl_inputs(r, 3)]
        ctl = O.make_control(**T.control(r))
        ref = O.solve_box_qp(*inp[:6], ctl)
        got = PT.solve_pwl(*inp[:6], torch.zeros_like(inp[6]), inp[7], ctl)
        for k in ("x", "z", "u", "rho", "iter"):
            assert _same(ref[k], got[k]), (name, dt, k)
        assert not bool((got["piece"] % 2 == 1).any())          # (no jump, no kink set)


@pytest.mark.parametrize("name,alpha", [("small_n31_m1", 1.0), ("sweep2_n129_m1", LT.ALPHA), ("lu1_n300_f64", 1.0)])
def test_l1eq_is_solve_l1_bit_for_bit(name, alpha):
    """K = 1, slopes (-w, w): x, z, u, u_box and the iteration count of l1_table.solve_l1, over-relaxed too, and padded to three kinks;
    side = piece - 1"""
    r = dict(T.ROW_BY_NAME[name], pwl="l1eq", soft="plain", l1="plain", alpha=alpha, K=60)
    for dt in (torch.float32, torch.float64):
        inp = [None if t is None else t.to(dt) for t in PT.pwl_inputs(r, 3)]
        l1 = [None if t is None else t.to(dt) for t in LT.l1_inputs(r, 3)]
        assert inp[6].shape[2] == 2 and torch.equal(inp[6][:, :, 1:], l1[6]) and torch.equal(inp[7], l1[7])
        ctl = O.make_control(**T.control(r))
        ref = LT.solve_l1(*l1, ctl, alpha=alpha)
        for s, c in ((inp[6], inp[7]), PT.pad(inp[6], inp[7])):
            got = PT.solve_pwl(*inp[:6], s, c, ctl, alpha=alpha)
            for k in ("x", "z", "u", "u_box", "rho", "iter", "lams"):
                assert _same(ref[k], got[k]), (name, dt, k, c.shape)
            assert torch.equal(got["piece"] - 1, ref["side"])
        assert int((ref["side"] == 0).sum()) > 0


@pytest.mark.parametrize("name,alpha", [("small_n31_m1", 1.0), ("sweep2_n129_m1", LT.ALPHA), ("lu1_n300_f64", 1.0)])
def test_bandeq_is_solve_soft_bit_for_bit(name, alpha):
    """K = 2, slopes (-wl, 0, wu): solve_soft's, padded to three kinks too; zone = piece - 2"""
    r = dict(T.ROW_BY_NAME[name], pwl="bandeq", soft="plain", l1="plain", alpha=alpha, K=60)
    for dt in (torch.float32, torch.float64):
        inp = [None if t is None else t.to(dt) for t in PT.pwl_inputs(r, 3)]
        soft = [None if t is None else t.to(dt) for t in ST.soft_inputs(r, 3)]
        assert torch.equal(inp[7], torch.cat((soft[8], soft[9]), 2)) and torch.equal(inp[6], torch.cat((-soft[6], 0 * soft[6], soft[7]), 2))
        ctl = O.make_control(**T.control(r))
        ref = ST.solve_soft(*soft, ctl, alpha=alpha)
        for s, c in ((inp[6], inp[7]), PT.pad(inp[6], inp[7])):
            got = PT.solve_pwl(*inp[:6], s, c, ctl, alpha=alpha)
            for k in ("x", "z", "u", "u_box", "rho", "iter", "lams"):
                assert _same(ref[k], got[k]), (name, dt, k, c.shape)
            assert torch.equal(got["piece"] - 2, ref["zone"])
        assert all(int((ref["zone"] == k).sum()) > 0 for k in ST.ZONES)


def test_the_scan_is_the_two_older_proxes_bit_for_bit_at_their_boundaries():
    """the step alone on random values with the exact comparison boundaries planted, float32 and float64, as given and padded"""
    g = torch.Generator().manual_seed(5)
    for dt in (torch.float32, torch.float64):
        N = 200000
        v = (2 * torch.randn(N, generator=g, dtype=torch.float64)).to(dt)
        tl, tu = (torch.rand(N, generator=g, dtype=torch.float64).to(dt) for _ in range(2))
        tl[::7], tu[::11] = 0, 0
        lo = torch.randn(N, generator=g, dtype=torch.float64).to(dt)
        hi = lo + torch.rand(N, generator=g, dtype=torch.float64).to(dt)
        hi[::5] = lo[::5]
        lo[3::13], hi[4::13] = -float("inf"), float("inf")
        q = N // 8          # planted: d == t, d == -t, v == kink, on both kinks
        v[0:q] = (hi + tu)[0:q]
        v[q:2 * q] = (lo - tl)[q:2 * q]
        v[2 * q:3 * q] = hi[2 * q:3 * q]
        v[3 * q:4 * q] = lo[3 * q:4 * q]
        v = torch.where(torch.isnan(v), torch.zeros_like(v), v)
        inf = torch.full_like(v, float("inf"))
        ref = ST.prox(v, tl, tu, lo, hi)
        assert torch.equal(ref, PT.prox(v, [-tl, 0 * tl, tu], [lo, hi]))
        assert torch.equal(ref, PT.prox(v, [-tl, 0 * tl, tu, tu], [lo, hi, inf]))
        c = torch.where(torch.isinf(lo), torch.zeros_like(lo), lo)
        v[4 * q:5 * q] = (c + tl)[4 * q:5 * q]
        v[5 * q:6 * q] = (c - tl)[5 * q:6 * q]
        ref = LT.shrink(v, tl, c)
        assert torch.equal(ref, PT.prox(v, [-tl, tl], [c]))
        assert torch.equal(ref, PT.prox(v, [-tl, tl, tl, tl], [c, inf, inf]))
        zero = torch.zeros_like(v)
        assert torch.equal(v, PT.prox(v, [zero] * 4, [lo, hi, inf]))


def test_equal_slopes_are_the_plain_solve_of_p_plus_s():
    """every slope of an element equal to s_i: the term is s'x, whatever the kinks.  Both solves run until they stop (the two loops
    start from different duals, so their iterates meet at the solution only), and meet within tier_table's float64 bar"""
    r = dict(T.ROW_BY_NAME["small_n31_m1"], pwl="plain", soft="plain", l1="plain", alpha=1.0, K=60)
    inp = list(PT.pwl_inputs(dict(r, dtype="f64"), 3))
    s = inp[6][:, :, 2:3]
    ctl = O.make_control(eps_abs=1e-13, eps_rel=1e-13, max_iters=200000)
    ref = O.solve_box_qp(inp[0], inp[1] + s, *inp[2:6], ctl)
    got = PT.solve_pwl(*inp[:6], s.expand(-1, -1, 4).contiguous(), inp[7], ctl)
    assert got["iter"] < 199999 and ref["iter"] < 199999
    for k in ("x", "z"):
        rec = T.compare(dict(r, dtype="f64"), {k: got[k]}, None, {k: ref[k]}, keys=(k,))[k]
        print(k, rec)
        assert rec["ok"], (k, rec)
    assert not bool((got["piece"] % 2 == 1).any())


def test_the_truth_satisfies_the_optimality_conditions():
    """float64 to eps = 1e-10, piece by piece: with g = Qx + p + A'nu, the term's multiplier -g is the slope s_k on piece 2k and lies in
    [s_{k-1}, s_k] on kink k, where x = c_k; on the hard bounds the residual has the bound's sign and is lams"""
    r = dict(PT.ROWS["hibound_n31-K60"])
    Q, p, A, b, lb, ub, s, c = PT.pwl_inputs(dict(r, dtype="f64"), 4)
    sol = PT.solve_pwl(Q, p, A, b, lb, ub, s, c, O.make_control(eps_abs=1e-10, eps_rel=1e-10, max_iters=40000))
    assert sol["iter"] < 39999
    x, piece, n = sol["x"], sol["piece"], 31
    g = Q @ x + p + A.transpose(1, 2) @ sol["nus"]
    sets = PT.sets(sol)
    tol = 1e-7
    assert float((A @ x - b).abs().max()) < tol and float((x - sol["z"]).abs().max()) < tol
    assert all(int(v.sum()) for v in sets.values()), {k: int(v.sum()) for k, v in sets.items()}
    sk, ck = PT._cols(s), PT._cols(c)
    for k in range(4):
        on = sets[f"p{2 * k}"]
        assert float((g + sk[k])[on].abs().max()) < tol, k
        if k > 0:
            assert float((x - ck[k - 1])[on].min()) > -tol, k
        if k < 3:
            assert float((ck[k] - x)[on].min()) > -tol, k
    for k in range(1, 4):
        on = sets[f"p{2 * k - 1}"]
        assert float((x - ck[k - 1])[on].abs().max()) < tol, k
        assert float((-g - sk[k - 1])[on].min()) > -tol and float((-g - sk[k])[on].max()) < tol, k
        assert bool((sk[k] > sk[k - 1])[on].all())
    # clamped: x on the bound; the term's multiplier is the rest of u, inside [s_0, s_K]; the bound's has the right sign and is lams
    cl = sets["clamped"]
    at_lb, at_ub = cl & (sol["u_box"] < 0), cl & (sol["u_box"] > 0)
    assert float((x - lb)[at_lb].abs().max()) < tol and float((x - ub)[at_ub].abs().max()) < tol
    mult = sol["rho"] * (sol["u"] - sol["u_box"])
    assert float((mult - sk[3]).max()) < tol and float((mult - sk[0]).min()) > -tol
    res = g + mult
    assert float(res[at_lb].min()) > -tol and float(res[at_ub].max()) < tol
    assert float((res - sol["lams"][:, :n] + sol["lams"][:, n:])[cl].abs().max()) < 1e-6
    # ... and everywhere: the term's multiplier is the slope the piece says
    for k in range(4):
        assert float((mult - sk[k])[piece == 2 * k].abs().max()) < tol, k


def _fd_case(seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    ru = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    n, B = 16, 1
    G = rn(B, 20, n)
    Q = G.transpose(1, 2) @ G / 20 + 0.3 * torch.eye(n, dtype=torch.float64)
    p = rn(B, n, 1)
    A = rn(B, 1, n)
    lb, ub = -(0.5 + 0.6 * ru(B, n, 1)), 0.5 + 0.6 * ru(B, n, 1)
    b = A @ (0.2 * rn(B, n, 1))
    wl, wu, w0, w1 = (0.05 + 0.5 * ru(B, n, 1) for _ in range(4))
    c = 0.3 * rn(B, n, 1)
    lo, hi = c - 0.05 - 0.3 * ru(B, n, 1), c + 0.05 + 0.3 * ru(B, n, 1)
    return [Q, p, A, b, lb, ub, torch.cat((-(w0 + wl), -w0, w1, w1 + wu), 2), torch.cat((lo, c, hi), 2)], rn(B, n, 1)


FD_SEED = 0          # (a seed at which most sets are populated and no element is within 1e-3 of changing sets)


def test_the_gradient_recipe_matches_central_differences():
    """n = 16, m = 1: d(cot' x*) / d(every entry of the eight arguments) by central differences of the truth run to 1e-13; the kinks
    of this case are distinct, so every dc is checked"""
    args, cot = _fd_case(FD_SEED)
    ctl = O.make_control(eps_abs=1e-13, eps_rel=1e-13, max_iters=100000, scale=False, adaptive_rho=False, rho=1.0)
    sol = PT.solve_pwl(*args, ctl)
    sizes = {k: int(v.sum()) for k, v in PT.sets(sol).items()}
    print(sizes)
    assert sizes["clamped"] >= 1 and sum(sizes[f"p{k}"] > 0 for k in (1, 3, 5)) >= 2 and sum(sizes[f"p{k}"] > 0 for k in (0, 2, 4, 6)) >= 3, sizes
    assert float(sol["margin"].min()) > 1e-3          # (no element near a change of set: the differences below stay on one piece)
    assert float((args[7][:, :, 1:] - args[7][:, :, :-1]).min()) > 0.04
    got = C.central_differences(PT.TERM, args, cot, ctl, sol)
    for name in ("ds", "dc"):
        assert float(got[name].abs().max()) > 1e-3, name          # (the new gradients are not trivially zero here)


@pytest.mark.parametrize("key", list(PT.ROWS))
def test_every_row_holds_the_eight_sets_and_needs_the_step(key):
    # the plain iterate and the band's iterate on (lo, hi) alone are at least 100 bars away in z: a kernel without the step, or one
    # that ignores the middle kink, cannot pass (l1eq has no outer kinks and bandeq IS the band: the plain iterate alone there); the
    # seven pieces (unclamped) and the clamped set
    r, idx, t32, t64, sub = C.row_needs_the_step(PT.TERM, key)
    C.row_holds_its_sets(PT.TERM, key, r, PT.sets(t64), len(idx))
    n, kind = r["n"], r["pwl"]
    sl, cn = sub[6], sub[7]
    assert bool((sl[:, :, 1:] >= sl[:, :, :-1]).all()) and bool((cn[:, :, 1:] >= cn[:, :, :-1]).all())
    assert cn.shape[2] == {"l1eq": 1, "bandeq": 2}.get(kind, 3) and sl.shape[2] == cn.shape[2] + 1
    if kind == "bandeq":
        assert float(sl[:, :, 1].abs().max()) == 0.0
    if kind == "flat":
        assert bool((sl[:, 0::2, 1] == sl[:, 0::2, 2]).all()) and bool((sl[:, 1::2, 1] < sl[:, 1::2, 2]).all())
        assert not bool((t64["piece"][:, 0::2] == 3).any())          # (no jump, no kink set)
    if kind == "hibound":
        assert int(((cn[:, :, 2:3] == sub[5]) | (cn[:, :, 0:1] == sub[4])).sum()) >= len(idx) * n // 5
    if kind == "allinf":
        assert bool(torch.isinf(sub[4]).all()) and bool(torch.isinf(sub[5]).all())


@pytest.mark.parametrize("name", list(PT.GRAD_ROWS))
def test_gradient_rows_have_the_same_pieces_in_both_precisions(name):
    r, idx, t32, t64, sub = C.gradient_row_in_both_precisions(PT.TERM, name)
    g64 = PT.truth_grads(r, sub, t64, PT.cot_of(r, T.batch(r, CUS), torch.float64)[idx], torch.float64)
    for k in range(4):
        assert float(g64["ds"][:, :, k].abs().max()) > 0, k          # (not trivially zero, in every slot)
    for k in range(3):
        assert float(g64["dc"][:, :, k].abs().max()) > 0, k


def test_the_stopped_solve_stops_at_one_count():
    C.stopped_solve_stops_at_one_count(PT.TERM)


def test_refusals():
    n, B = 6, 2
    Q = torch.eye(n).repeat(B, 1, 1)
    p, lb, ub = torch.zeros(B, n, 1), -torch.ones(B, n, 1), torch.ones(B, n, 1)
    s = torch.tensor([-1.0, -0.5, 0.5, 1.0]).repeat(B, n, 1)
    c = torch.tensor([-0.1, 0.0, 0.1]).repeat(B, n, 1)
    ok = L.box_qp_control()
    SP.check_pwl(ok, Q, p, s, c)
    SP.check_pwl(ok, Q, p, s[:, :, :3], c[:, :, :2])
    SP.check_pwl(ok, Q, p, s[:, :, :2], c[:, :, :1])
    for extra in (dict(stop='each'), dict(stop='each', infeasible='flag'), dict(stop='each', unbounded='raise'), dict(unroll=True),
                  dict(backward='kkt'), dict(dist_strict_stop=True), dict(_global_bounds=(True, True)), dict(_bound_flags_dev=torch.ones(2)),
                  dict(_check_hook=lambda *a: None), dict(rho=0), dict(rho=0.0), dict(rho=-1.0)):
        for call in (lambda ctl: L.torch_solve_box_qp_pwl(Q, p, None, None, lb, ub, s, c, ctl),
                     lambda ctl: L.SolveBoxQPPwl(ctl)(Q, p, None, None, lb, ub, s, c)):
            with pytest.raises(ValueError, match="lqp_py_amd"):
                call(dict(ok, **extra))
    for bad_s, bad_c in ((s[:, :3], c), (s, c[:, :3]), (s[:, :, :3], c), (s, c[:, :, :2]), (s.double(), c), (s, c.double()), (None, c), (s, None),
                         (1.0, c), (s, c[:, :, 0]), (torch.cat((s, s), 2)[:, :, :5], torch.cat((c, c), 2)[:, :, :4]), (s[:, :, :1], c[:, :, :0])):
        with pytest.raises(ValueError, match="lqp_py_amd"):
            L.torch_solve_box_qp_pwl(Q, p, None, None, lb, ub, bad_s, bad_c, ok)
    # the shape rule says for the older terms what it said
    with pytest.raises(ValueError, match=r"w must be a tensor of p's shape \(2, 6, 1\)"):
        L.torch_solve_box_qp_l1(Q, p, None, None, lb, ub, p[:, :3], p, ok)
    with pytest.raises(ValueError, match=r"hi must be a tensor of p's shape \(2, 6, 1\)"):
        L.torch_solve_box_qp_soft(Q, p, None, None, lb, ub, p, p, p, None, ok)
    with pytest.raises(ValueError, match=r"w must have p's dtype torch.float32, got torch.float64"):
        L.torch_solve_box_qp_log(Q, p, None, None, lb, ub, p.double(), ok)
    with pytest.raises(ValueError, match=r"s must be a tensor of shape \(2, 6, 4\)"):
        L.torch_solve_box_qp_pwl(Q, p, None, None, lb, ub, s[:, :, :3], c, ok)
    # valid arguments on the CPU get as far as the device check: there is no CPU path
    with pytest.raises(RuntimeError, match="GPU"):
        L.torch_solve_box_qp_pwl(Q, p, None, None, lb, ub, s, c, ok)
    assert lqp_py.solve_box_qp_pwl.SolveBoxQPPwl is L.SolveBoxQPPwl
    assert lqp_py.solve_box_qp_pwl.torch_solve_box_qp_pwl is L.torch_solve_box_qp_pwl


def test_the_module_pads_at_the_top():
    s = torch.tensor([-1.0, 0.25]).repeat(2, 5, 1)
    c = torch.tensor([0.5]).repeat(2, 5, 1)
    ps, pc = SP._pad(s, c)
    ts, tc = PT.pad(s, c)
    assert torch.equal(ps, ts) and torch.equal(pc, tc) and ps.shape == (2, 5, 4) and pc.shape == (2, 5, 3)
    ls, lc, K = SP._lower((s, c))
    assert K == 3 and ls.shape == (4, 2, 5) and lc.shape == (3, 2, 5) and ls.is_contiguous() and lc.is_contiguous()
    assert torch.equal(ls[3], s[:, :, 1]) and bool(torch.isinf(lc[1:]).all())


NEW_SYMBOLS = {"lqp_boxqp_forward_pwl", "lqp_boxqp_forward_pwl_workspace_bytes", "lqp_boxqp_pwl_effective_box",
               "lqp_boxqp_pwl_finish_grads"}


def test_abi_facts():
    """The new symbols are declared, exported and bound; the version is still 17; the flag bit is 1 << 21 on both sides; the workspace
    query grows by the eleven regions; the C entries refuse null pointers, a K outside 1 .. 3, the per-problem stop, the unroll factor
    bit, a check hook, a non-positive scalar rho and a short workspace before any launch -- without a GPU."""
    lib = _lib.load()
    assert _lib.ABI_VERSION == 17 and lib.lqp_abi_version() == 17
    assert _lib.RP_PWL_INPUT == 1 << 21
    csrc = open(os.path.join(os.path.dirname(HERE), "lqp_py_amd", "csrc", "lqp_boxqp.hpp")).read()
    assert re.search(r"RP_PWL_INPUT = 1 << 21\b", csrc) and re.search(r"constexpr int PWL_K = 3;", csrc)
    header = open(os.path.join(os.path.dirname(HERE), "include", "lqp_amd.h")).read()
    declared = set(re.findall(r"\b(lqp_\w+)\s*\(", header))
    assert NEW_SYMBOLS <= declared and NEW_SYMBOLS <= set(_lib.SYMBOLS)
    for s in NEW_SYMBOLS:
        assert getattr(lib, s) is not None
    assert ctypes.sizeof(_lib.BoxQPCtrl) == lib.lqp_boxqp_ctrl_bytes() and _lib.BoxQPCtrl._fields_[-1][0] == "alpha"
    for dt, B, n, m in ((0, 4, 100, 1), (1, 3, 257, 2), (0, 2, 1025, 0)):
        fwd, soft = lib.lqp_boxqp_forward_workspace_bytes(dt, B, n, m), lib.lqp_boxqp_forward_soft_workspace_bytes(dt, B, n, m)
        pwl = lib.lqp_boxqp_forward_pwl_workspace_bytes(dt, B, n, m)
        assert fwd + 11 * B * n * (4, 8)[dt] <= pwl <= fwd + 11 * B * (n + 8) * (4, 8)[dt] + 512, (fwd, pwl)
        assert pwl > soft
    assert lib.lqp_boxqp_forward_pwl_workspace_bytes(7, 1, 1, 0) == 0
    # refusals of the C entry (nothing is dereferenced before them: 4096 stands for any non-null pointer)
    P = ctypes.c_void_p(4096)
    ctl, stats = _lib.BoxQPCtrl(max_iters=10, check_solved=1), _lib.BoxQPStats()
    nbytes = lib.lqp_boxqp_forward_pwl_workspace_bytes(0, 2, 8, 0)
    some_hook = _lib.CHECK_HOOK(lambda user, stream, counters, index: 0)

    def call(s=P, c=P, K=3, piece=P, u_box=P, ws_bytes=nbytes, hook=None, **ctl_over):
        for k, v in dict(dict(reserved2=0, rho_mode=0, rho_value=0.0), **ctl_over).items():
            setattr(ctl, k, v)
        ctl.check_hook = hook if hook is not None else _lib.CHECK_HOOK()
        return lib.lqp_boxqp_forward_pwl(None, 0, 2, 8, 0, P, P, None, None, P, P, s, c, K, ctypes.byref(ctl), None, P, P, P, P, None, P,
                                         piece, u_box, ctypes.byref(stats), P, ws_bytes)
    for kw in (dict(s=None), dict(c=None), dict(K=0), dict(K=4), dict(piece=None), dict(u_box=None), dict(reserved2=8),
               dict(reserved2=1), dict(hook=some_hook), dict(rho_mode=1, rho_value=0.0), dict(rho_mode=1, rho_value=-1.0)):
        assert call(**kw) == 1, kw
    for K in (1, 2, 3):
        assert call(K=K, ws_bytes=lib.lqp_boxqp_forward_workspace_bytes(0, 2, 8, 0)) == 2
    assert call(ws_bytes=lib.lqp_boxqp_forward_soft_workspace_bytes(0, 2, 8, 0)) == 2
    assert lib.lqp_boxqp_pwl_effective_box(None, 0, 2, 8, None, P, P, P, P, P, 3, 1, 1.0, None, P, P, P, P) == 1
    assert lib.lqp_boxqp_pwl_effective_box(None, 0, 2, 8, P, P, P, P, P, None, 3, 1, 1.0, None, P, P, P, P) == 1
    assert lib.lqp_boxqp_pwl_effective_box(None, 0, 2, 8, P, P, P, P, P, P, 3, 2, 1.0, None, P, P, P, P) == 1
    assert lib.lqp_boxqp_pwl_effective_box(None, 0, 2, 8, P, P, P, P, P, P, 4, 1, 1.0, None, P, P, P, P) == 1
    assert lib.lqp_boxqp_pwl_finish_grads(None, 0, 2, 8, P, P, None, P, P, 3, P, P, P, P) == 1
    assert lib.lqp_boxqp_pwl_finish_grads(None, 0, 2, 8, P, None, P, P, P, 3, P, P, P, P) == 1
    assert lib.lqp_boxqp_pwl_finish_grads(None, 0, 2, 8, P, P, P, P, P, 0, P, P, P, P) == 1
    assert lib.lqp_boxqp_pwl_finish_grads(None, 3, 2, 8, P, P, P, P, P, 3, P, P, P, P) == 1
