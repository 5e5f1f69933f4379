#!/usr/bin/env python3
"""What control['stop'] = 'each' costs and buys: forward + backward steps timed with device events.

    python tools/gpu_each.py --stop each          # this tree
    python tools/gpu_each.py --stop all           # run from a checkout of the parent commit for the comparison

Three shapes, n = 500, m = 1, benchmark data (lqp_py_amd.synthetic.create_qp_data, eps 1e-5): the headline batch (B = 128, all
problems alike: the mode's overhead or saving on a homogeneous batch) and a heterogeneous batch at B = 128 and B = 1024, in which every
second problem has p and b scaled by 1e-6 so that x = 0 is optimal to the tolerance and it stops at its first or second check.  One
untimed first-use pass, then three rounds of K steps; the median round is reported, with the spread, and the per-problem iteration
histogram where the solve returns it.  One JSON line per shape."""
import argparse
import collections
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lqp_py_amd as L
from lqp_py_amd.synthetic import create_qp_data


def batch(B, n, seed, hetero, dev):
    Q, p, A, b, lb, ub = create_qp_data(n, B, seed=seed)
    if hetero:
        s = torch.ones(B, 1, 1)
        s[1::2] = 1e-6
        p, b = p * s, b * s
    return [t.to(dev) for t in (Q, p, A, b, lb, ub)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stop", choices=["all", "each"], required=True)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--n", type=int, default=500)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctl = L.box_qp_control(eps_abs=1e-5, eps_rel=1e-5)
    if args.stop == "each":
        ctl["stop"] = "each"
    layer = L.SolveBoxQP(control=ctl)
    for name, B, hetero in (("headline_b128", 128, False), ("hetero_b128", 128, True), ("hetero_b1024", 1024, True)):
        data = [batch(B, args.n, s, hetero, dev) for s in range(3)]
        ones = torch.ones(B, args.n, 1, device=dev)

        def step(i):
            Q, p, A, b, lb, ub = data[i % len(data)]
            Q = Q.detach().requires_grad_(True)
            p = p.detach().requires_grad_(True)
            layer(Q, p, A, b, lb, ub).backward(ones)

        for i in range(2 * len(data)):      # first use of every batch, untimed
            step(i)
        torch.cuda.synchronize()
        rounds = []
        for _ in range(3):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for i in range(args.steps):
                step(i)
            t1.record()
            torch.cuda.synchronize()
            rounds.append(t0.elapsed_time(t1) / args.steps)
        rounds.sort()
        sol = L.torch_solve_box_qp(*data[0], ctl)
        hist = None
        if "iters" in sol:
            hist = dict(sorted(collections.Counter(sol["iters"].cpu().tolist()).items()))
        st = L.solve_box_qp_admm_torch.last_forward_status(dev)
        print(json.dumps(dict(shape=name, stop=args.stop, B=B, n=args.n, ms_per_step=round(rounds[1], 4), min=round(rounds[0], 4),
                              max=round(rounds[2], 4), iter=sol["iter"], iters_histogram=hist,
                              loop_workgroups_per_qp=st["loop_workgroups_per_qp"], mode_used=st["mode_used"])), flush=True)


if __name__ == "__main__":
    main()
