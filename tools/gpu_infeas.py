"""What infeasibility detection costs on problems that are feasible: the split row's shape (n = 130, m = 1) at B = 128 with
control['stop'] = 'each', eps 1e-5, the keys set against the keys absent.  `--keys`: none | flag (control['infeasible'], the primal
certificate) | unbounded (control['unbounded'], the dual one) | both.

For each of the two: the iteration count, the time of the loop kernels (the library's per-class device events, synchronous
forwards) and the forward's time between two device events, `--rounds` times after a warm-up.  One JSON line each; run the script
several times and compare the difference with the spread one setting shows against itself.

    python tools/gpu_infeas.py
    python tools/gpu_infeas.py --keys none --tree /path/to/another/checkout     # key absent on another build: A/B
    python tools/gpu_infeas.py --keys none unbounded both --n 600               # the dual certificate, alone and with the primal one
"""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--keys", nargs="+", default=["none", "flag", "none", "flag", "none", "flag"])
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--n", type=int, default=130)
ap.add_argument("--reps", type=int, default=20)
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

for key in args.keys:
    extra = {"none": {}, "unbounded": dict(unbounded='flag'), "both": dict(infeasible='flag', unbounded='flag')}.get(key, dict(infeasible=key))
    ctl = L.box_qp_control(eps_abs=1e-5, eps_rel=1e-5, verbose=False, stop='each', **extra)
    for i in range(5):
        sol = L.torch_solve_box_qp(*data[i % len(data)], dict(ctl))
    torch.cuda.synchronize(dev)
    fwd = []
    for _ in range(args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(args.reps):
            L.torch_solve_box_qp(*data[i % len(data)], dict(ctl))
        e1.record()
        torch.cuda.synchronize(dev)
        fwd.append(e0.elapsed_time(e1) / args.reps * 1e3)
    fwd.sort()
    _lib.profile(enable=True, reset=True)
    for i in range(args.reps):
        sol = L.torch_solve_box_qp(*data[i % len(data)], dict(ctl))
    torch.cuda.synchronize(dev)
    pr = _lib.profile()
    _lib.profile(enable=False)
    st = last_forward_status(dev)
    status = sol.get("status")
    print(json.dumps(dict(tag=args.tag, infeasible=key, B=B, n=n, iters=sol["iter"], loop_kind=st["loop_kind"],
                          loop_workgroups_per_qp=st["loop_workgroups_per_qp"],
                          checks=sol["iter"] // int(ctl.get("check_solved") or max(round((n ** 0.5) / 10) * 10, 1)) + 1,
                          flagged=None if status is None else int((status >= 2).sum()),
                          loop_us=round(pr["admm_loop"][0] / args.reps * 1e3, 2),
                          forward_us=dict(median=round(fwd[len(fwd) // 2], 1), min=round(fwd[0], 1), max=round(fwd[-1], 1)))), flush=True)
