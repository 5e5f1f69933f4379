"""CPU-only checks: the C-ABI library loads and exports every symbol that
include/lqp_amd.h declares, the control-dict resolution mirrors the reference's
traps, and the product path refuses CPU tensors (no fallback)."""
import ctypes
import os
import re

import pytest
import torch

import lqp_py_amd as L
from lqp_py_amd import _lib
from lqp_py_amd.solve_box_qp_admm_torch import resolve_control

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    text = open(os.path.join(REPO, "include", "lqp_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lqp_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    _lib.build_library()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = header_functions()
    assert len(names) >= 20
    for name in names:
        assert hasattr(lib, name), f"{name} declared in include/lqp_amd.h but not exported"
    assert set(names) == set(_lib.SYMBOLS), set(names) ^ set(_lib.SYMBOLS)
    assert _lib.load().lqp_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define LQP_ABI_VERSION (\d+)", open(os.path.join(REPO, "include", "lqp_amd.h")).read()).group(1))


def test_workspace_queries_and_argument_checks_without_gpu():
    lib = _lib.load()
    assert lib.lqp_boxqp_forward_workspace_bytes(0, 128, 500, 1) > 128 * 512 * 512 * 4 * 2
    assert lib.lqp_boxqp_forward_workspace_bytes(7, 1, 1, 0) == 0          # unknown dtype
    assert lib.lqp_lu_packed_bytes(1, 2, 100) > 2 * 128 * 128 * 8
    # the KKT solve's and the backward's workspaces share one carve: (dtype, B, n, m) -> bytes of each, as every build so far gave them
    for (dt, B, n, m), (kkt, bwd) in {(0, 3, 40, 3): (150272, 152576), (0, 1, 1, 0): (50432, 51456), (0, 2, 513, 17): (5617664, 5631488),
                                      (1, 3, 40, 3): (298496, 302336), (1, 1, 1, 0): (99840, 101376),
                                      (1, 2, 513, 17): (11225600, 11248640)}.items():
        assert lib.lqp_kkt_solve_workspace_bytes(dt, B, n, m) == kkt, (dt, B, n, m)
        assert lib.lqp_boxqp_backward_fp_workspace_bytes(dt, B, n, m) == bwd, (dt, B, n, m)
    # null pointers are rejected before anything touches the device
    ctl = _lib.BoxQPCtrl(max_iters=10, check_solved=1)
    assert lib.lqp_boxqp_forward(None, 0, 1, 4, 0, None, None, None, None, None, None, ctypes.byref(ctl), None,
                                 None, None, None, None, None, None, None, None, 0) == 1
    assert lib.lqp_status_string(3).decode().startswith("singular")


@pytest.mark.parametrize("dt", [0, 1])
def test_backward_refuses_before_it_touches_anything(monkeypatch, dt):
    """A workspace one byte short, and a prefactor call for a form without phases (LQP_BWD_FULL=1): the status comes back
    before any launch -- no GPU is needed to see it -- and before the report words or fail_index are written."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.c_void_p(ctypes.addressof(buf))            # (never dereferenced on these paths)
    B, n, m = 3, 40, 3
    need = lib.lqp_boxqp_backward_fp_workspace_bytes(dt, B, n, m)
    fail, rep = ctypes.c_int32(-5), (ctypes.c_int32 * B)(7, 7, 7)
    rp = ctypes.cast(rep, ctypes.c_void_p)
    assert lib.lqp_boxqp_backward_fp(None, dt, B, n, m, p, p, p, p, p, p, p, p, p, 1, 1.0, None, p, p, p, p, p, p,
                                     ctypes.byref(fail), p, need - 1, 2, rp) == 2
    assert lib.lqp_boxqp_backward_fp_prefactor(None, dt, B, n, m, p, p, p, p, p, p, p, need - 1, 2, rp) == 2
    assert lib.lqp_boxqp_backward_kkt(None, dt, B, n, m, p, p, p, p, p, p, p, p, p, p, p, p, p, p, ctypes.byref(fail), p,
                                      need - 1, 1, rp) == 2
    monkeypatch.setenv("LQP_BWD_FULL", "1")
    assert lib.lqp_boxqp_backward_fp_prefactor(None, dt, B, n, m, p, p, p, p, p, p, p, need, 2, rp) == 6
    assert list(rep) == [7, 7, 7] and fail.value == -5


# (B, n, m, iters) -> scratch bytes of lqp_boxqp_unroll_backward (float32 only) | of _backward_lu | of the tape in segments, (f32, f64) each
_UNROLL_BYTES = {(1, 1, 0, 0): (1281, (1537, 1537), (2052, 2056)),
                 (3, 40, 3, 7): (13248, (13760, 25792), (21504, 41216)),
                 (2, 513, 17, 20): (283690, (286762, 551210), (459432, 896336))}
_UNROLL_ROWS = {0: (13568, 17408, 0), 1: (25600, 33280, 0)}      # (3, 40, 3, 7): offsets of the z, u, x rows in the tape's scratch


def _never_read():
    buf = ctypes.create_string_buffer(64)
    return buf, ctypes.c_void_p(ctypes.addressof(buf))


@pytest.mark.parametrize("dt", [0, 1])
def test_unroll_workspace_queries_and_row_offsets_are_pinned(dt):
    """The three workspace queries of the unroll entries and where the query form of lqp_boxqp_unroll_tape_segment (k1 <= k0) says the
    rows of iterates live, as every build so far gave them: callers size their scratch by the first and unrolled.py views the rows
    in it by the second.  The query launches nothing and dereferences nothing."""
    lib = _lib.load()
    for (B, n, m, iters), (sym, lu, tape) in _UNROLL_BYTES.items():
        assert lib.lqp_boxqp_unroll_backward_workspace_bytes(B, n, m, iters) == sym, (B, n, m, iters)
        assert lib.lqp_boxqp_unroll_backward_lu_workspace_bytes(dt, B, n, m, iters) == lu[dt], (dt, B, n, m, iters)
        assert lib.lqp_boxqp_unroll_tape_workspace_bytes(dt, B, n, m, iters) == tape[dt], (dt, B, n, m, iters)
    B, n, m, iters = 3, 40, 3, 7
    keep, p = _never_read()
    z, u, x = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.lqp_boxqp_unroll_tape_segment(None, dt, B, n, m, p, lib.lqp_boxqp_forward_workspace_bytes(dt, B, n, m), iters, 0, 0, 0, None,
                                             None, None, -1, None, None, None, None, None, None, None, p, _UNROLL_BYTES[(B, n, m, iters)][2][dt],
                                             ctypes.byref(z), ctypes.byref(u), ctypes.byref(x)) == 0
    assert (z.value - p.value, u.value - p.value, x.value - p.value) == _UNROLL_ROWS[dt]


@pytest.mark.parametrize("dt", [0, 1])
def test_unroll_entries_refuse_before_they_touch_anything(dt):
    """The four unroll entries answer a null pointer (1), a forward workspace one byte short (2), a scratch one byte short (2) and a size
    they do not take (6) before any launch -- no GPU is needed to see it, no buffer is read -- and in that order: the symmetric entry
    says "unsupported" for n = 1025, m = 17 although its scratch is too short as well."""
    lib = _lib.load()
    keep, p = _never_read()
    B, n, m, iters = 3, 40, 3, 7
    fwd = lib.lqp_boxqp_forward_workspace_bytes(dt, B, n, m)
    fwd32 = lib.lqp_boxqp_forward_workspace_bytes(0, B, n, m)
    sym, lu, tape = (v if isinstance(v, int) else v[dt] for v in _UNROLL_BYTES[(B, n, m, iters)])
    outs = (p,) * 8                                          # dQs, dps, dAs, dbs, dlbs, dubs, drho, dD

    def backward_sym(fw=p, fw_bytes=fwd32, scratch=p, scratch_bytes=sym, n=n, m=m):
        return lib.lqp_boxqp_unroll_backward(None, B, n, m, fw, fw_bytes, iters, p, *outs, scratch, scratch_bytes)

    def backward_lu(fw=p, fw_bytes=fwd, scratch=p, scratch_bytes=lu, n=n, m=m):
        return lib.lqp_boxqp_unroll_backward_lu(None, dt, B, n, m, fw, fw_bytes, iters, p, *outs, scratch, scratch_bytes)

    def segment(fw=p, fw_bytes=fwd, scratch=p, scratch_bytes=tape, n=n, m=m, dps=p):
        return lib.lqp_boxqp_unroll_tape_segment(None, dt, B, n, m, fw, fw_bytes, iters, 0, iters + 1, 3, p, p, p, -1, None, p, dps, p, p, p, p,
                                                 scratch, scratch_bytes, None, None, None)

    def finish(scratch=p, scratch_bytes=tape, dAs=p):
        return lib.lqp_boxqp_unroll_tape_finish(None, dt, B, n, m, iters, p, dAs, p, scratch, scratch_bytes)

    for entry, fw_bytes, scratch_bytes in ((backward_sym, fwd32, sym), (backward_lu, fwd, lu), (segment, fwd, tape)):
        assert entry(fw=None) == 1 and entry(scratch=None) == 1, entry.__name__
        assert entry(fw_bytes=fw_bytes - 1) == 2 and entry(scratch_bytes=scratch_bytes - 1) == 2, entry.__name__
    assert segment(dps=None) == 1
    assert finish(scratch=None) == 1 and finish(dAs=None) == 1 and finish(scratch_bytes=tape - 1) == 2      # (it reads no forward workspace)
    rows = (4096, 2048)[dt]                                  # n + m above the pivoted LU's limit: before either workspace is looked at
    assert backward_lu(n=rows, m=1, fw_bytes=0, scratch_bytes=0) == 6 and segment(n=rows, m=1, fw_bytes=0, scratch_bytes=0) == 6
    big = lib.lqp_boxqp_forward_workspace_bytes(0, B, 1025, 17)
    assert backward_sym(n=1025, m=17, fw_bytes=big, scratch_bytes=0) == 6
    assert backward_sym(n=1025, m=17, fw_bytes=big - 1, scratch_bytes=0) == 2      # (the forward workspace still comes first)


def test_tape_segments_cut_where_rho_may_change():
    from lqp_py_amd.unrolled import _tape_segments
    assert _tape_segments(31, True, 10, 1000) == [(0, 10), (10, 20), (20, 30), (30, 31)]
    assert _tape_segments(31, True, 10, 20) == [(0, 10), (10, 31)]             # (no event at or past adaptive_rho_max_iter)
    assert _tape_segments(10, True, 10, 1000) == [(0, 10)]
    assert _tape_segments(1, True, 1, 1000) == [(0, 1)]
    assert _tape_segments(31, False, 10, 1000) == [(0, 31)] and _tape_segments(1, False, 1, 1000) == [(0, 1)]
    import unroll_table
    assert [unroll_table._segments(K, it, mx) for K, it, mx in ((30, 10, 1000), (30, 10, 20), (9, 10, 1000), (0, 1, 1000))] == [4, 2, 1, 1]


def test_chain_by_autograd_against_autograd_called_directly():
    """Three tensor leaves (one of them needs no gradient) and a None among them; pairs whose output is a number or whose cotangent is
    None drop out, a cotangent comes in another shape than its output: exactly what torch.autograd.grad gives when called directly."""
    from lqp_py_amd.unrolled import _chain_by_autograd
    g = torch.Generator().manual_seed(11)
    rnd = lambda *shape: torch.randn(*shape, dtype=torch.float64, generator=g)
    a0, c0, d0, g1, g2, g3 = rnd(2, 3, 1), rnd(2, 3, 1), rnd(2, 1, 1), rnd(2, 3, 1), rnd(2), rnd(2, 3, 1)

    def graph():
        a, c, d = a0.clone().requires_grad_(True), c0.clone(), d0.clone().requires_grad_(True)
        return (a, c, d), (a * d + c, (a * a * c).sum(dim=1) / d.reshape(2, 1), torch.sin(a) * c)
    (a, c, d), (o1, o2, o3) = graph()
    got = _chain_by_autograd([(o1, g1), (1.0, g3), (o2, g2), (o3, None)], [a, None, c, d])
    (a, c, d), (o1, o2, o3) = graph()
    want = torch.autograd.grad([o1, o2], [a, d], [g1, g2.reshape(2, 1)])
    assert got[1] is None and got[2] is None and torch.equal(got[0], want[0]) and torch.equal(got[3], want[1])
    (a, c, d), (o1, o2, o3) = graph()
    assert _chain_by_autograd([(1.0, g3), (o3, None)], [a, None, c, d]) == [None, None, None, None]       # (nothing to differentiate)
    assert _chain_by_autograd([(o1.detach(), g1)], [None, c]) == [None, None]


@pytest.mark.parametrize("m", [0, 2])
def test_kkt_matrix_is_the_literal_expression(m):
    from lqp_py_amd.unrolled import _kkt_matrix
    g = torch.Generator().manual_seed(5)
    B, n = 3, 4
    Qs, rho = torch.randn(B, n, n, generator=g), torch.rand(B, 1, 1, generator=g) + 0.5
    As = torch.randn(B, m, n, generator=g) if m > 0 else None
    M = Qs + rho * torch.eye(n).unsqueeze(0)
    if m > 0:
        M = torch.cat((torch.cat((M, As.transpose(1, 2)), 2), torch.cat((As, torch.zeros(B, m, m)), 2)), 1)
    got = _kkt_matrix(Qs, As, rho)
    assert got.shape == (B, n + m, n + m) and torch.equal(got, M)
    assert torch.equal(_kkt_matrix(Qs, As, 0.25), _kkt_matrix(Qs, As, torch.full((B, 1, 1), 0.25)))       # (rho as a number)


def test_control_factory_and_resolution_traps():
    c = L.box_qp_control(check_solved=3, adaptive_rho_max_iter=7, reduce='max')
    assert c["check_terimnation"] == 3 and "check_solved" not in c and c["reduce"] == 'max'
    r = resolve_control(c, 500)
    assert r["check_solved"] == 20 and r["adaptive_rho_max_iter"] == 1000 and r["adaptive_rho_iter"] == 100
    assert [resolve_control({}, n)["check_solved"] for n in (10, 50, 100, 250, 500, 1000)] == [1, 10, 10, 20, 20, 30]
    assert resolve_control({}, 1000)["adaptive_rho_iter"] == 90
    e = resolve_control({}, 10)
    assert (e["adaptive_rho"], e["adaptive_rho_tol"], e["scale"]) == (False, 5, False)
    assert resolve_control({"eps_abs": 0.0}, 10)["eps_abs"] == 1e-12


def test_no_cpu_fallback():
    Q = torch.eye(4).unsqueeze(0)
    p = torch.ones(1, 4, 1)
    lb, ub = -torch.ones(1, 4, 1), torch.ones(1, 4, 1)
    with pytest.raises(RuntimeError, match="GPU"):
        L.torch_solve_box_qp(Q, p, None, None, lb, ub, L.box_qp_control())
    with pytest.raises(RuntimeError, match="GPU"):
        L.torch_solve_qp_eqcon(Q, p, None, None)


def test_utils_match_reference_shapes():
    assert L.get_ncon(None, 1) == 0 and L.get_ncon(torch.zeros(3, 2, 5), 1) == 2
    Q, A = torch.randn(2, 3, 3), torch.randn(2, 1, 3)
    M = L.torch_qp_eqcon_mat(Q, A)
    assert M.shape == (2, 4, 4) and torch.equal(M[:, 3:, :3], A) and float(M[:, 3, 3].abs().max()) == 0


def test_product_never_imports_the_oracle():
    pkg = os.path.join(REPO, "lqp_py_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                src = open(os.path.join(root, f)).read()
                assert "oracle" not in src.replace("the oracle", ""), f"{f} mentions the oracle"


def test_oracle_is_only_used_as_a_checker():
    """tools/ and examples/ never import it; bench.py does so only inside its cpu_baseline leg."""
    for sub in ("tools", "examples"):
        for f in os.listdir(os.path.join(REPO, sub)):
            if f.endswith((".py", ".sh")):
                assert "oracle" not in open(os.path.join(REPO, sub, f)).read(), f"{sub}/{f}"
    src = open(os.path.join(REPO, "bench.py")).read()
    start = src.index("def cpu_baseline_worker")
    end = src.index("\ndef ", start + 1)
    outside = src[:start] + src[end:]
    assert "import oracle" not in outside and "from oracle" not in outside


def test_synthetic_generator_matches_the_oracle_and_the_golden_inputs():
    from conftest import load_golden
    from lqp_py_amd.synthetic import create_qp_data
    from oracle import boxqp_oracle as O
    for kw in (dict(n_x=12, n_batch=5, seed=3), dict(n_x=9, n_batch=4, seed=1, with_eq=False),
               dict(n_x=10, n_batch=32, seed=0, with_eq=False, unit_box=True),
               dict(n_x=7, n_batch=3, seed=2, dtype=torch.float64)):
        for a, b in zip(create_qp_data(**kw), O.create_qp_data(**kw)):
            assert (a is None and b is None) or (a.dtype == b.dtype and torch.equal(a, b))
    from lqp_py_amd.synthetic import create_hard_qp_data
    for a, b in zip(create_hard_qp_data(30, 0.15, [0, 1, 7]), O.create_hard_qp_data(30, 0.15, [0, 1, 7])):
        assert a.dtype == b.dtype == torch.float64 and torch.equal(a, b)
    # (tests/golden/make_golden.py holds the oracle's generator equal to the reference's generate_hard_qp_torch)
    g = load_golden("g1_b32_n10_box")
    Q, p, _, _, lb, ub = create_qp_data(10, 32, seed=0, with_eq=False, unit_box=True)
    assert torch.equal(Q, g["Q"]) and torch.equal(p, g["p"]) and torch.equal(lb, g["lb"]) and torch.equal(ub, g["ub"])


def test_lqp_py_import_path_is_an_alias_of_the_hip_package():
    """callers import lqp_py.<module>; every such module IS the lqp_py_amd module of that name."""
    import lqp_py_amd
    from lqp_py.solve_box_qp_admm_torch import SolveBoxQP, SolveBoxQPLayer, torch_solve_box_qp, torch_solve_box_qp_grad
    from lqp_py.control import box_qp_control
    from lqp_py.lu_layer import TorchLU
    from lqp_py.solve_qp_eqcon_torch import torch_solve_qp_eqcon
    from lqp_py.utils import get_ncon
    import lqp_py.solve_box_qp_admm_torch as mod
    assert mod is lqp_py_amd.solve_box_qp_admm_torch and mod.__name__ == "lqp_py_amd.solve_box_qp_admm_torch"
    assert SolveBoxQP is lqp_py_amd.SolveBoxQP and SolveBoxQPLayer is lqp_py_amd.SolveBoxQPLayer
    assert torch_solve_box_qp is lqp_py_amd.torch_solve_box_qp and torch_solve_box_qp_grad is lqp_py_amd.torch_solve_box_qp_grad
    assert box_qp_control is lqp_py_amd.box_qp_control and TorchLU is lqp_py_amd.TorchLU
    assert torch_solve_qp_eqcon is lqp_py_amd.torch_solve_qp_eqcon and get_ncon is lqp_py_amd.get_ncon
    import os
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert sorted(os.listdir(os.path.join(here, "lqp_py"))) in (["__init__.py"], ["__init__.py", "__pycache__"])


def test_bench_spawns_its_own_ranks_without_touching_the_gpu(tmp_path, monkeypatch):
    """`python bench.py --gpus N` with no torchrun environment: the parent only builds the torchrun command line
    (one rank per GPU, 127.0.0.1 rendezvous) and relays the child's exit code."""
    import importlib.util
    import subprocess
    import sys as _sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(repo, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    seen = {}

    def fake_run(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = cmd, env
        return subprocess.CompletedProcess(cmd, 7)
    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(_sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3"])
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("GPU touched by the parent")))
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 7
    cmd = seen["cmd"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[-4:] == ["--gpus", "4", "--steps", "3"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_bench_dump_outputs_writes_a_fixed_sample(tmp_path):
    """bench.py --dump-outputs: x (x_local / x_all with N ranks), dp and dQ of the last step as .npy in the computed dtype;
    an array above SAMPLE_MAX elements as the seeded, sorted sample_index of its flat entries, the same in every run."""
    import importlib.util
    import numpy as np
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(repo, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    B, n = 128, 500
    idx = bench.sample_index(B * n * n)
    assert idx.numel() == bench.SAMPLE_MAX and torch.equal(idx, bench.sample_index(B * n * n))
    assert bool((idx[1:] >= idx[:-1]).all()) and 0 <= int(idx[0]) and int(idx[-1]) < B * n * n
    assert torch.equal(bench.sample_index(1000), torch.arange(1000))
    assert 4 * bench.SAMPLE_MAX * 4 <= 64 * 10 ** 6
    g = torch.Generator().manual_seed(5)
    x, Q, p = torch.randn(B, n, 1, generator=g), torch.randn(B, n, n), torch.randn(B, n, 1)
    Q.grad, p.grad = torch.randn(B, n, n, generator=g), torch.randn(B, n, 1, generator=g)
    bench.dump_outputs(str(tmp_path / "one"), (x, Q, p), 1)
    got = {f[:-4]: np.load(tmp_path / "one" / f) for f in os.listdir(tmp_path / "one")}
    assert sorted(got) == ["dQ", "dp", "x"] and all(a.dtype == np.float32 for a in got.values())
    assert np.array_equal(got["x"], x.numpy()) and np.array_equal(got["dp"], p.grad.numpy())
    assert np.array_equal(got["dQ"], Q.grad.reshape(-1)[idx].numpy())
    bench.dump_outputs(str(tmp_path / "two"), ((x[:64], x.double()), Q, p), 2)
    got = {f[:-4]: np.load(tmp_path / "two" / f) for f in os.listdir(tmp_path / "two")}
    assert sorted(got) == ["dQ", "dp", "x_all", "x_local"] and got["x_all"].dtype == np.float64
    assert np.array_equal(got["x_local"], x[:64].numpy()) and np.array_equal(got["x_all"], x.double().numpy())


def _kernel_resources(path=None):
    """{demangled kernel name: (vgprs, spilled vgprs, scratch bytes)} from the code-object metadata of the built library
    (every translation unit of the split build carries its own code object), or of one object file of its build."""
    import shutil
    import subprocess
    import tempfile
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf) and shutil.which("c++filt")):
        pytest.skip("llvm-objdump / llvm-readelf / c++filt not available")
    _lib.build_library()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(path or _lib.LIB_PATH, os.path.join(tmp, "lib.so"))
        subprocess.run([objdump, "--offloading", "lib.so"], cwd=tmp, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        for f in sorted(os.listdir(tmp)):
            if "gfx950" not in f:
                continue
            notes = subprocess.run([readelf, "--notes", os.path.join(tmp, f)], capture_output=True, text=True, check=True).stdout
            for blk in notes.split("- .agpr_count")[1:]:
                g = lambda k: re.search(r"\." + k + r":\s*(\S+)", blk).group(1)
                name = subprocess.run(["c++filt", g("name")], capture_output=True, text=True).stdout.strip()
                out[name.split("(")[0].replace("void ", "")] = (int(g("vgpr_count")), int(g("vgpr_spill_count")),
                                                                int(g("private_segment_fixed_size")))
    return out


def test_register_budgets_of_the_hot_kernels():
    """What the shipped code object says about the kernels of the benched step (VERDICT r3 asked for this check after
    DESIGN.md claimed 0 spilled registers for a kernel that had 20).  Exact zeros where they hold; elsewhere the measured
    numbers as CEILINGS, so that a change that makes the compiler spill more is caught here and not on the GPU:
      * k_spd_resident<8,2>: ONE spilled VGPR / 8 B of scratch (round 3: 20 / 44 with ~40 scratch instructions in the step
        body: lane addresses derived from a slot's tile indices, formed once in front of the step loop; the indices are opaque
        per step now and nothing is reloaded inside the loop -- same speed; the look-ahead form,
        round 4, held its tiles with 7 and was no faster: DESIGN.md section 8; its code left the sources in round 5);
      * the other k_spd_resident instances: no spilled VGPR, at most 72 B of scratch (the by-value parameter block of the sweep);
      * k_admm_loop_split<8,512,false,2,FormAll>: 132 spilled VGPRs, all in the once-per-launch equality prologue."""
    res = _kernel_resources()
    assert len(res) >= 80, len(res)
    exact_zero = ["lqp::k_admm_loop_split<5, 512, false, 2, lqp::FormAll>",
                  "lqp::k_admm_loop_split<6, 512, false, 2, lqp::FormAll>",
                  "lqp::k_admm_loop_split<7, 512, false, 2, lqp::FormAll>", "lqp::k_admm_loop_split<7, 512, false, 4, lqp::FormAll>",
                  "lqp::k_admm_loop_split<8, 512, false, 4, lqp::FormAll>", "lqp::k_admm_loop_small<lqp::FormAll>", "lqp::k_spd_prep<0>",
                  "lqp::k_bwd_build_chol<0>", "lqp::k_unroll_outer<0>", "lqp::k_pack<float>", "lqp::k_pack<double>",
                  "lqp::k_fwd_setup<double>"]
    for k in exact_zero:
        assert res[k][1] == 0 and res[k][2] == 0, (k, res[k])
    ceilings = {"lqp::k_spd_resident<8, 2, false>": (1, 8), "lqp::k_spd_resident<7, 2, false>": (0, 72), "lqp::k_spd_resident<6, 2, false>": (0, 72), "lqp::k_spd_resident<8, 4, false>": (0, 72),
                "lqp::k_spd_resident<5, 2, false>": (0, 72), "lqp::k_spd_resident<7, 4, false>": (0, 72), "lqp::k_spd_resident<3, 2, false>": (0, 72), "lqp::k_spd_resident<4, 2, false>": (0, 72),
                # round 6, the same sweep with two-half operands on the float16 matrix pipe (the instances that run by default)
                "lqp::k_spd_resident<8, 2, true>": (94, 208), "lqp::k_spd_resident<7, 2, true>": (23, 100), "lqp::k_spd_resident<6, 2, true>": (0, 72), "lqp::k_spd_resident<8, 4, true>": (0, 72),
                "lqp::k_spd_resident<5, 2, true>": (0, 72), "lqp::k_spd_resident<7, 4, true>": (0, 72), "lqp::k_spd_resident<3, 2, true>": (0, 72), "lqp::k_spd_resident<4, 2, true>": (0, 72),
                "lqp::k_admm_loop_split<8, 512, false, 2, lqp::FormAll>": (132, 260),
                "lqp::k_bwd_chol_solve<0, false>": (36, 124), "lqp::k_bwd_chol_solve<0, true>": (38, 128), "lqp::k_bwd_chol_solve<4, true>": (38, 132),
                # round 5, the two-workgroup pivoted LU: nothing spilled in the panel's column steps (the chain); 24 registers around
                # the hand-off loads of the f32 build
                "lqp::k_lu_factor2<float, 32>": (24, 100), "lqp::k_lu_factor2<double, 16>": (0, 0),
                # round 5, second half: the wide LU (nothing spilled in float64; 12 registers around the float32 panel), the dense loop on W
                # workgroups (192 float32 columns per thread: 9 registers outside the product; 64 float64 columns: none), the two-workgroup
                # unroll sweep and the scaling-chain kernels (none)
                "lqp::k_lu_factor_wide<float>": (12, 48), "lqp::k_lu_factor_wide<double>": (0, 320),
                "lqp::k_lu_factor_wide_tall<float>": (17, 336),      # (round 6: 2048 < N <= 4096, sixteen panel rows per thread)
                "lqp::k_admm_loop_dense_w<float>": (9, 40), "lqp::k_admm_loop_dense_w<double>": (0, 0),
                "lqp::k_unroll_sweep_split<8, 1>": (0, 0), "lqp::k_unroll_sweep_split<8, 16>": (0, 0), "lqp::k_unroll_sweep_split<7, 16>": (0, 0),
                "lqp::k_unroll_scale_grad<0>": (0, 0), "lqp::k_unroll_scale_vectors<0>": (0, 0), "lqp::k_lu_inverse<float, true>": (0, 0)}
    # the one-workgroup pivoted LU, every instance (wg_lu_factor with one panel row per thread; with two and four: k_lu_factor_big),
    # at the numbers of the build before the families came to share one panel routine and one interchange step: nothing spilled
    # but in float64 with 16-column panels on 1024 threads (row and pivot row are 64 of its 128 registers), and the 96 B of the
    # float32 k_lu_factor_big that holds both of its forms
    for inst in ("float, 16, true, 1024", "float, 16, true, 512", "float, 32, true, 512", "float, 16, false, 1024", "float, 16, false, 512",
                 "float, 32, false, 512", "float, 8, false, 1024", "float, 8, false, 512", "double, 8, true, 1024", "double, 8, true, 512",
                 "double, 16, true, 512"):
        ceilings[f"lqp::k_lu_factor<{inst}>"] = (0, 0)
    ceilings["lqp::k_lu_factor<double, 16, true, 1024>"] = (24, 68)
    ceilings["lqp::k_lu_factor_big<float>"] = (0, 96)
    ceilings["lqp::k_lu_factor_big<double>"] = (0, 0)
    assert sum(k.startswith("lqp::k_lu_factor<") for k in res) == sum(k.startswith("lqp::k_lu_factor<") for k in ceilings) == 12
    for k, (spill, scratch) in ceilings.items():
        assert res[k][1] <= spill and res[k][2] <= scratch, (k, res[k])
    for k, (vg, _, _) in res.items():
        assert vg <= 256, (k, vg)


HOST_UNIT_KERNELS = {"k_debug_spin", "k_debug_xcd"}       # the two kernels written in csrc/lqp_amd.hip itself


def _manifest():
    """tools/gen_split_build.py as a module: its manifest says which kernel instances the library contains"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_split_build", os.path.join(REPO, "tools", "gen_split_build.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_split_build_lists_are_what_the_generator_writes():
    """csrc/split/ is generated from the manifest in tools/gen_split_build.py and never edited: --check writes nothing and
    fails when a committed file differs from what the generator would write."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "gen_split_build.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_host_unit_holds_only_the_debug_kernels():
    """The host translation unit of the split build sees every kernel instance as an `extern template`; one that the host
    code names and the manifest lacks would be compiled here instead, silently and on one thread.  Its device code object
    defines exactly the two kernels written in csrc/lqp_amd.hip itself."""
    _lib.build_library()
    obj = os.path.join(_lib.CSRC, "build", "lqp_amd.o")
    if not os.path.exists(obj):
        pytest.skip("no csrc/build/lqp_amd.o: the library was built from a single source (LQP_UNITY_BUILD)")
    assert set(_kernel_resources(obj)) == HOST_UNIT_KERNELS


def test_library_holds_the_instances_of_the_manifest():
    """The kernels of the built library are the manifest's instances and the host unit's two: none missing, none besides."""
    built, want = set(_kernel_resources()), set(_manifest().instances()) | HOST_UNIT_KERNELS
    assert built == want, (sorted(built - want), sorted(want - built))


def test_report_buffer_quarantine():
    """A report buffer that a queued kernel may still write (a prefactored backward that was dropped) is handed out again only
    once every word of it has arrived: -1 is the library's "missing", everything else -- 0, a pivot index, -7 -- has arrived."""
    import torch
    words = 5
    saved_free, saved_q = dict(_lib._pinned_free), list(_lib._pinned_quarantine)
    try:
        _lib._pinned_free.clear(); del _lib._pinned_quarantine[:]
        spare = torch.zeros(words, dtype=torch.int32)
        _lib._pinned_free[words] = [spare]                      # (so that the pool is never refilled from pinned memory here)
        done = torch.tensor([0, 0, 3, 0, -7], dtype=torch.int32)
        _lib.pinned_release(done)
        assert _lib._pinned_free[words][-1] is done and not _lib._pinned_quarantine
        busy = torch.tensor([0, -1, 0, -1, 0], dtype=torch.int32)
        _lib.pinned_release(busy)
        assert _lib._pinned_quarantine == [busy] or (len(_lib._pinned_quarantine) == 1 and _lib._pinned_quarantine[0] is busy)
        got = _lib.host_report(words)
        assert got is done and _lib._pinned_quarantine[0] is busy          # (still being written: stays out of the pool)
        busy[1] = 0; busy[3] = 2
        got2 = _lib.host_report(words)
        assert not _lib._pinned_quarantine and got2 is busy                # (swept into the pool, handed out last-in first-out)
    finally:
        _lib._pinned_free.clear(); _lib._pinned_free.update(saved_free)
        del _lib._pinned_quarantine[:]; _lib._pinned_quarantine.extend(saved_q)


def test_bound_assumption_remembered_for_plain_dicts():
    """a pipelined call made with a plain control dict (no nn.Module to key on) used to look at the bounds on EVERY call
    (two reductions and a host read: the stream drained).  The id-keyed table now carries a copy of the settings it answered for and
    only answers for a dict that holds the same: a recycled address with other settings is a miss, equal settings are a hit,
    tensor values count by identity, and nothing is written into the caller's dict."""
    import torch
    from lqp_py_amd import solve_box_qp_admm_torch as S
    S._seen_by_dict_id.clear()
    c = dict(eps_abs=1e-5, eps_rel=1e-5, sync=False)
    assert S._assume_any_bound(None, c, sync=False) is None
    S._remember_any_bound(None, c, True)
    assert S._assume_any_bound(None, c, sync=False) is True and S._assume_any_bound(None, c, sync=True) is True
    assert set(c) == {"eps_abs", "eps_rel", "sync"}                      # the caller's dict stays clean
    c["eps_abs"] = 1e-3                                                   # the same object, other settings: not the remembered control
    assert S._assume_any_bound(None, c, sync=False) is None
    c["eps_abs"] = 1e-5
    assert S._assume_any_bound(None, c, sync=False) is True
    # an entry left under a recycled address by ANOTHER dict
    other = dict(rho=1.0)
    S._seen_by_dict_id[id(other)] = S._seen_by_dict_id.pop(id(c))
    assert S._assume_any_bound(None, other, sync=False) is None
    # tensor-valued settings: by identity only
    t = torch.ones(3, 1, 1)
    d = dict(rho=t)
    S._remember_any_bound(None, d, False)
    assert S._assume_any_bound(None, d, sync=False) is False
    d["rho"] = torch.ones(3, 1, 1)
    assert S._assume_any_bound(None, d, sync=False) is None
    S._seen_by_dict_id.clear()


# ---------------------------------------------------------------- the retry rules of the forward solve (_forward_decide)
def _outcome(status, split_wait=True, known=False, any_bound=True, mode_used=4, any_lb=1, any_ub=1, hook_error=None):
    from lqp_py_amd import solve_box_qp_admm_torch as S
    stats = _lib.BoxQPStats(mode_used=mode_used, any_lb=any_lb, any_ub=any_ub, fail_index=2)
    return S._Outcome(status=status, split_wait=split_wait, stats=stats, hook_error=hook_error, known=known, any_bound=any_bound)


_HOOK_EXC = ValueError("raised inside the strict-stop hook")
_SINGULAR = "lqp_py_amd.torch_solve_box_qp: LU factorisation hit an exactly zero pivot (batch index 2); the KKT matrix is singular"
# name -> (outcome, one_call and bounds of the attempt, what `look` answers (None: must not be asked),
#          expected: what changes in the next attempt (None: no repeat), release, remember, error type and text)
_DECIDE_ROWS = {
    "1 time-out of a split call": (dict(status=5), False, None, None, dict(one_call=True), 'now', None, None),
    "1 ... not twice: one_call set": (dict(status=5, split_wait=False, mode_used=0), True, None, None, None, 'wait', None,
                                      (RuntimeError, "lqp_py_amd.torch_solve_box_qp: grid barrier timeout")),
    "1 ... not twice, even if split": (dict(status=5), True, None, None, None, 'wait', None,
                                       (RuntimeError, "lqp_py_amd.torch_solve_box_qp: grid barrier timeout")),
    "2 outside the symmetric x-update": (dict(status=7), False, (True, False), None, dict(linsolve='lu'), 'now', None, None),
    "2 ... drops one_call": (dict(status=7), True, None, None, dict(linsolve='lu', one_call=False), 'now', None, None),
    "2 ... only after a split wait": (dict(status=7, split_wait=False, mode_used=0), False, None, None, None, 'wait', None,
                                      (RuntimeError, "lqp_py_amd.torch_solve_box_qp: matrix outside the symmetric x-update")),
    "3 hook error, status 0": (dict(status=0, split_wait=False, mode_used=0, hook_error=[_HOOK_EXC]), False, None, None, None, 'wait',
                               None, (ValueError, str(_HOOK_EXC))),
    "3 hook error first": (dict(status=3, split_wait=False, mode_used=0, any_bound=False, hook_error=[_HOOK_EXC]), False, None, None,
                           None, 'wait', None, (ValueError, str(_HOOK_EXC))),
    "4 singular, 'no bound' assumed, some seen": (dict(status=3, any_bound=False), False, None, (False, True),
                                                  dict(bounds=(False, True)), 'wait', True, None),
    "4 ... drops one_call": (dict(status=3, split_wait=False, mode_used=0, any_bound=False), True, None, (True, True),
                             dict(bounds=(True, True), one_call=False), 'wait', True, None),
    "4 ... none seen": (dict(status=3, any_bound=False), False, None, (False, False), None, 'wait', None, (RuntimeError, _SINGULAR)),
    "4 ... not twice: bounds known": (dict(status=3, known=True, any_bound=False), False, (False, False), None, None, 'wait', None,
                                      (RuntimeError, _SINGULAR)),
    "4 ... bounds were assumed": (dict(status=3, any_bound=True), False, None, None, None, 'wait', None, (RuntimeError, _SINGULAR)),
    "5 any other status": (dict(status=6, split_wait=False, mode_used=0), False, None, None, None, 'wait', None,
                           (RuntimeError, "lqp_py_amd.torch_solve_box_qp: unsupported size (n + m <= 4096 in float32, 2048 in float64)")),
    "6 pipelined: nothing to compare": (dict(status=0, split_wait=False, mode_used=3, any_lb=-1, any_ub=-1), False, None, None, None,
                                        'tail', None, None),
    "6 waited, assumption held": (dict(status=0), False, None, None, None, 'tail', True, None),
    "6 waited, 'no bound' held": (dict(status=0, any_bound=False, any_lb=0, any_ub=0), False, None, None, None, 'tail', False, None),
    "6 waited, bounds known": (dict(status=0, known=True, any_lb=0, any_ub=0), False, (True, True), None, None, 'tail', None, None),
    "6 waited, flags not reported": (dict(status=0, any_lb=-1, any_ub=-1), False, None, None, None, 'tail', None, None),
    "7 bounds assumed, none there": (dict(status=0, any_lb=0, any_ub=0), False, None, None, dict(bounds=(False, False)), 'tail', False,
                                     None),
    "7 none assumed, one side there": (dict(status=0, split_wait=False, mode_used=0, any_bound=False, any_lb=0, any_ub=1), True, None,
                                       None, dict(bounds=(False, True), one_call=False), 'tail', True, None),
}


@pytest.mark.parametrize("row", sorted(_DECIDE_ROWS))
def test_forward_retry_rules(row):
    """One row per rule of _forward_decide (numbered as in its order of precedence) and per way a rule must NOT fire: which of
    control['linsolve'], '_owner', bounds and one_call the next attempt changes and which it keeps, how the report buffer goes
    back, what is remembered, what is raised.  The prepared backward is voided by the time-out rule alone."""
    from lqp_py_amd import solve_box_qp_admm_torch as S
    out_kw, one_call, bounds, look_says, change, release, remember, error = _DECIDE_ROWS[row]
    owner = dict(eps_abs=1e-5, linsolve='auto')
    control = dict(owner)                                    # (what lqp_py_amd.dist hands the layer: a copy, owner apart)
    before = dict(control)
    att = S._Try(control, bounds, one_call)
    asked = []

    def look():
        asked.append(1)
        assert look_says is not None, "the bounds were looked at"
        return look_says
    v = S._forward_decide(_outcome(**out_kw), att, owner, look)
    assert control == before and owner == before             # nothing is written into either dict
    assert len(asked) == (0 if look_says is None else 1)
    assert v.release == release and v.remember is remember
    assert v.void_prepared is (row == "1 time-out of a split call")
    if error is not None:
        assert v.next is None and type(v.error) is error[0] and str(v.error) == error[1]
        return
    assert v.error is None
    if change is None:
        assert v.next is None
        return
    want_control = dict(control, linsolve='lu', _owner=owner) if change.get('linsolve') else control
    assert v.next.control == want_control
    if change.get('linsolve'):
        assert v.next.control['_owner'] is owner and v.next.control is not control
    else:
        assert v.next.control is control
    assert v.next.bounds == change.get('bounds', bounds)
    assert v.next.one_call is change.get('one_call', False)      # (set by the time-out rule, dropped by every other repeat)


def test_per_problem_argument_of_rho_and_beta():
    """rho and beta share one resolver: None -> the default rule, a number or a one-element tensor -> a scalar, B values -> a
    tensor of (B,) on the device and in the dtype of the problem; any other size is refused with each one's own text."""
    from lqp_py_amd.solve_box_qp_admm_torch import _per_problem_argument as arg
    like = torch.zeros(3, 4, 1, dtype=torch.float64)
    for name, example in (("rho", "(B,1,1)"), ("beta", "(B,1)")):
        assert arg(name, example, None, 3, like) == (0, 0.0, None)
        assert arg(name, example, 0.25, 3, like) == (1, 0.25, None)
        assert arg(name, example, torch.tensor([[0.5]]), 3, like) == (1, 0.5, None)
        mode, value, t = arg(name, example, torch.tensor([1.0, 2.0, 3.0]).reshape(3, 1, 1), 3, like)
        assert (mode, value) == (2, 0.0) and t.shape == (3,) and t.dtype == torch.float64 and t.is_contiguous()
        assert t.tolist() == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError) as e:
        arg("rho", "(B,1,1)", torch.ones(2, 1, 1), 3, like)
    assert str(e.value) == "lqp_py_amd: a rho tensor must hold one value per problem, e.g. shape (B,1,1)"
    with pytest.raises(ValueError) as e:
        arg("beta", "(B,1)", torch.ones(2, 1), 3, like)
    assert str(e.value) == "lqp_py_amd: a beta tensor must hold one value per problem, e.g. shape (B,1)"
