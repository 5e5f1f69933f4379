"""Over-relaxation (control['alpha']) on the headline step: B = 128, n = 500, m = 1, eps 1e-5, forward + backward w.r.t. Q and p.

For every alpha given (`none` = the key absent): the iteration count of the forward, the time of its loop kernel (the library's
per-class device events, synchronous calls) and the step time, pipelined (control['sync'] = False) and synchronous, between two
device events around K steps, `--rounds` times after a warm-up.  One JSON line per alpha.

    python tools/gpu_relax.py --alphas none 1.6
    python tools/gpu_relax.py --alphas none --tree /path/to/another/checkout     # the same measurement on another build: A/B

--tree imports the package from another checkout (its own built library); run the two alternately, each in a fresh process,
and compare the difference with the spread one tree shows against itself.
"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--alphas", nargs="+", default=["none", "1.6"])
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--n", type=int, default=500)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--warmup", type=int, default=30)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--tag", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import torch
import lqp_py_amd as L
from lqp_py_amd import _lib
from lqp_py_amd.solve_box_qp_admm_torch import last_forward_status
from lqp_py_amd.synthetic import create_qp_data

dev = torch.device("cuda:0")
B, n = args.batch, args.n
data = [[t.to(dev) for t in create_qp_data(n, B, seed=s)] for s in range(3)]
ones = torch.ones(B, n, 1, device=dev)


def step(layer, i):
    Q, p, A, b, lb, ub = data[i % len(data)]
    Q = Q.detach().requires_grad_(True)
    p = p.detach().requires_grad_(True)
    layer(Q, p, A, b, lb, ub).backward(ones)


def rounds_ms(layer):
    """ms per step of `--rounds` rounds of `--steps` steps, each between two device events"""
    for i in range(args.warmup):
        step(layer, i)
    torch.cuda.synchronize(dev)
    out = []
    for _ in range(args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(args.steps):
            step(layer, i)
        e1.record()
        torch.cuda.synchronize(dev)
        out.append(e0.elapsed_time(e1) / args.steps)
    L.synchronize()
    return sorted(out)


for a in args.alphas:
    extra = {} if a == "none" else dict(alpha=float(a))
    ctl = L.box_qp_control(eps_abs=1e-5, eps_rel=1e-5, verbose=False, **extra)
    rec = dict(tag=args.tag, alpha=a, B=B, n=n)
    for name, sync in (("pipelined", False), ("sync", True)):
        ms = rounds_ms(L.SolveBoxQP(control=dict(ctl, sync=sync)))
        rec[f"step_{name}_ms"] = dict(median=round(ms[len(ms) // 2], 4), min=round(ms[0], 4), max=round(ms[-1], 4))
    # iteration count and the loop's own time: synchronous forwards under the library's per-class events
    for _ in range(3):
        sol = L.torch_solve_box_qp(*data[0], dict(ctl))
    torch.cuda.synchronize(dev)
    _lib.profile(enable=True, reset=True)
    reps = 10
    for i in range(reps):
        sol = L.torch_solve_box_qp(*data[i % len(data)], dict(ctl))
    torch.cuda.synchronize(dev)
    pr = _lib.profile()
    _lib.profile(enable=False)
    st = last_forward_status(dev)
    rec.update(iters=sol["iter"], x_updates=st["n_solve"], loop_us=round(pr["admm_loop"][0] / reps * 1e3, 2),
               loop_us_per_iteration=round(pr["admm_loop"][0] / reps * 1e3 / st["n_solve"], 3))
    print(json.dumps(rec), flush=True)
