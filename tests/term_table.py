"""What the tables of the separable-term layers share (tests/l1_table.py, soft_table.py, log_table.py, pwl_table.py): one record per
term, `Table`, and on it the truth, the inputs, the shared truth of a row, the gradients and the stopped solve -- each written once.
No GPU needed to import this module.

The truth of every term is the oracle's own loop, ``oracle.solve_box_qp(term=...)``: the loop the reference-made goldens pin, with the
term's prox in front of the clamp.  A term object (``Table.term(*data)``, one class per table module) has three parts: ``scale(D)`` keeps
the term's data in the scaled space of the loop (x = D xs), ``step(v, rho)`` is S of the z-update in exactly its branch form, and
``finish(z, u, rho, lbs, ubs, D)`` takes the step once more at the returned iterate (v = z + u) and returns the classification (the
table's `aux` key), "u_box" -- the box's share of the dual -- and "margin": how far every element is from changing its set, unscaled.
The solve always takes the loop schedule (``bounds=(True, True)``): bounds that are all infinite are an ordinary case.

A table module keeps what is its own: the term's mathematics, the prox, the classification, the gradient recipe, the data kinds, and
the rows with their seed offsets.
"""
import dataclasses
import functools
import math

import torch

from oracle import boxqp_oracle as O
import tier_table as T

# a solve that stops by itself (eps 1e-5, the oracle's generator): (n, B, seed)
STOP = (100, 4, 0)
STOP_CONTROL = dict(eps_abs=1e-5, eps_rel=1e-5)
STOP_ROW = dict(dtype="f32", R=T.R_DEFAULT, F=T.F_DEFAULT)


@dataclasses.dataclass(eq=False)
class Table:
    name: str                   # "l1", "soft", ...: the key of a row that holds its kind, and the infix of the entry points
    weights: int                # how many of the term's inputs (behind Q, p, A, b, lb, ub), the first ones, are weights: all zero is no term
    aux: str                    # the output the bars for values do not take
    grads: tuple                # the gradients, in the order of the inputs
    term: type                  # term(*data): the term object of oracle.solve_box_qp
    others: dict                # step name -> (term class, the kinds it is not asked of): the steps the rows must be far from
    far_keys: tuple             # ... in these outputs
    data: object                # (r, i, lb, ub) -> the term's data of problem i of row r, float64 (n, .) each
    stop_inputs: object         # dtype -> the inputs of the solve that stops by itself
    label: object               # sol -> what is compared exactly between precisions and with the device
    what: str                   # ... and its name in a message
    grad_recipe: object         # (cot, sol, Q, A, lb, ub, *recipe data) -> {gradient name: tensor}
    recipe_data: tuple          # which of the term's data the recipe takes
    tables: dict                # {"ROWS": ..., "GRAD_ROWS": ...}
    share: float = 0.0          # every set of every sampled problem holds at least this share of the elements ...
    empty: dict = dataclasses.field(default_factory=dict)         # ... but the sets a kind empties by construction,
    pooled_below: int = 0       # and below this n the share is asked of the row's sampled problems together

    def inputs(self, r, B, idx=None):
        """(Q, p, A, b, lb, ub, *data) of the batch -- or of the problems `idx` of it -- in the row's dtype (rounding to float32 is
        monotone: what is sorted stays sorted, what is equal stays equal)"""
        dt = torch.float32 if r["dtype"] == "f32" else torch.float64
        idx = list(range(B)) if idx is None else list(idx)
        base = [None if t is None else t.double() for t in T.inputs(dict(r, dtype="f64"), B, idx)]
        if r.get(self.name) == "allinf":
            base[4] = torch.full_like(base[4], -math.inf)
            base[5] = torch.full_like(base[5], math.inf)
        per = [self.data(r, i, base[4][k], base[5][k]) for k, i in enumerate(idx)]
        base += [torch.stack([x[j] for x in per]) for j in range(len(per[0]))]
        return tuple(None if t is None else t.to(dt) for t in base)

    def solve(self, *args, alpha=1.0, trace=None, step=None):
        """The oracle's forward with the term's step on (Q, p, A, b, lb, ub, *data, control); returns its dict -- "lams" built from
        u_box -- plus the term's own outputs and "n_factor".  step: a name of `others`, or a term class of the caller's own (a test
        that watches the step wraps it): the iterate of a kernel that takes another step -- what the rows must be far from."""
        *inp, control = args
        make = self.term if step is None else self.others[step][0] if step in self.others else step
        tr = {}
        sol = O.solve_box_qp(*inp[:6], control, trace=tr, bounds=(True, True), alpha=alpha, term=make(*inp[6:]))
        if trace is not None:
            trace.update(n_factor=tr["n_factor"])
        return dict(sol, n_factor=tr["n_factor"])

    def truth(self, r, inp, dtype, step=None):
        """The truth of row r on `inp` in `dtype`, pinned to the row's K"""
        d = [None if t is None else t.to(dtype) for t in inp]
        return self.solve(*d, O.make_control(**T.control(r)), alpha=r["alpha"], step=step)

    @functools.lru_cache(maxsize=None)
    def row_truth(self, key, cus, table="ROWS"):
        """-> (idx, t32 or None, t64) of a row at `cus` compute units: the problems `tier_table.sample` picks, computed once and shared"""
        r = self.tables[table][key]
        B = T.batch(r, cus)
        idx = T.sample(B)
        sub = self.inputs(r, B, idx)
        t64 = self.truth(r, sub, torch.float64)
        t32 = self.truth(r, sub, torch.float32) if r["dtype"] == "f32" else None
        return idx, t32, t64

    def truth_grads(self, r, inp, sol, cot, dtype):
        d = [None if t is None else t.to(dtype) for t in inp]
        return self.grad_recipe(cot.to(dtype), sol, d[0], d[2], d[4], d[5], *[d[6 + k] for k in self.recipe_data])

    @functools.lru_cache(maxsize=None)
    def stop_truth(self, dtype):
        """The truth of a solve that stops by itself"""
        return self.solve(*self.stop_inputs(dtype), O.make_control(**STOP_CONTROL))

    def steps_of(self, kind):
        """the other steps a row of this kind must be far from"""
        return [s for s, (_, left_out) in self.others.items() if kind not in left_out]


def cot_of(r, B, dtype):
    g = torch.Generator().manual_seed(T.seed_of(r) + 1)
    return torch.randn(B, r["n"], 1, generator=g, dtype=torch.float64).to(dtype)


def excused(t64, bar_z):
    """bool (B, n, 1): elements whose label may differ from the float64 truth's -- in that truth they sit within the bar for z of a
    comparison of the step or of a bound (its "margin")"""
    return t64["margin"] < bar_z

