"""Exact inputs for the pivoted-LU kernels, as data (no GPU needed to import this module): matrices with a PLANTED factorisation
whose every intermediate is exactly representable in float32, so that any correct partial-pivoting LU -- LAPACK's, and each of
the five kernel families of csrc/lqp_lu.hpp (one panel row per thread, and several: k_lu_factor_big), lqp_lu2.hpp,
lqp_lu_wide.hpp (and its tall form) -- returns the
planted factor and pivots BIT FOR BIT, in float32 and in float64, whatever the order of its sums.  tests/test_gpu_lu_exact.py runs
every row on the GPU under torch.equal; tests/test_lu_table.py proves the table on the CPU first (LAPACK returns the plant, the
plain getf2 below agrees, P A' = L U in integers, the rows cover every panel kind and tie class per kernel family, and a wrong
tie rule changes the pivots of every row that claims a tie).

The construction.  L unit lower triangular, U upper triangular with diagonal +-2^k (k = 0, 1, 2) and small integers above it,
A' = Pi0 (L U) with Pi0 a product of DISJOINT transpositions (k, s_k), k < s_k, one per *swap column* k.
  swap column k   : every multiplier is 0 or +-1/2 at the positions above s_k, so the planted row (position s_k) is the strict
                    winner -- or, in a *tied swap column*, some rows at positions BELOW s_k carry +-1: they tie with the planted
                    row and lose to it by the first-index rule;
  other columns   : multipliers 0, +-1/2 or +-1; a row with +-1 ties with the diagonal row and loses to it.
All multipliers lie in {0, +-1/2, +-1}, every Schur complement is a small multiple of 1/2: exact in any summation order.

What the ties are aimed at.  Between panels the kernels move rows physically; inside a panel thread t keeps the row it loaded
(relative row t, or t + q * NTP in register slot q) and only its `curpos` moves.  So the live rows whose position differs from
their holder are the rows displaced from a diagonal position by a swap EARLIER IN THE SAME PANEL: they sit in threads < pb with a
position far below.  A tie later in that panel between such a row and a row at a smaller position held by a higher lane, 16-lane
row, wave or register slot is decided rightly only by the positions -- "lowest lane wins" picks the displaced row.

Row fields:
  name, N, B, dtype ("f32" | "f64"), env (LQP_* overrides)
  kernel         the family the row targets: "one" | "two" | "big" | "wide" | "tall"
  expect_kernel  what select() -- launch_lu's selection (csrc/lqp_amd.hip) restated -- gives for (N, B, dtype, env) on 256 CUs
  zero           None, or the columns j with U[j,j] = 0 (the factorisation must report the first of them)
  why            what the row is there for / what "the kernel ran" rests on
Batch element 1 of a B = 2 row is -A' (the same L and pivots, -U).
"""
import functools

import numpy as np
import torch

DTYPES = {"f32": torch.float32, "f64": torch.float64}
# panel kinds: no swap at all | swaps inside the panel only (ne = 0, src[j] != j) | 1, 8, 9, pb displaced rows (ne) | a swap, then a
# tie whose winner is not the lowest holder | the last, partial panel with a swap and a tie (the scalar load path)
KINDS = ("none", "inside", "d1", "d8", "d9", "dpb", "swaptie", "last")
# tie classes: the winner against a tied row in the same 16-lane row | another 16-lane row of its wave | another wave | another
# register slot of its own thread
CLASSES = ("row16", "wave16", "waves", "slot")
FAMILIES = ("one", "two", "big", "wide", "tall")
CUS = (256, 304)


# ---------------------------------------------------------------------------------------------------------------------------------
# launch_lu's selection (csrc/lqp_amd.hip: launch_lu, launch_lu_wide, launch_lu_big, launch_lu2; csrc/lqp_lu.hpp: lu_threads,
# lu_panel_width), restated.  One 1024-thread workgroup of the wide kernels per CU, at least one 512-thread one of lqp_lu2.hpp.
def select(N, B, dtype, env=None, cus=256):
    env = env or {}
    e = lambda k, d: int(env.get(k, d))
    f32 = dtype == "f32"
    sz = 4 if f32 else 8
    nmax = 4096 if f32 else 2048
    if N > nmax:
        raise ValueError("unsupported size")
    if N > 512:
        ntile = -(-N // (128 // sz))
        W = min(cus // B, ntile, 62)
        if N > e("LQP_LU_WIDE_MIN", 1024) and e("LQP_LU_WIDE", 1) != 0 and W >= 2:
            if N > 2048:
                return dict(kernel="tall", pb=4, ntp=256, slots=16, name="tall/pb4")
            return dict(kernel="wide", pb=8 if f32 else 4, ntp=256, slots=8, name=f"wide/pb{8 if f32 else 4}")
    if N > 1024:
        if N > 2048:
            return dict(kernel="big", pb=4, ntp=1024, slots=4, name="big/pb4/r4")
        return dict(kernel="big", pb=8 if f32 else 4, ntp=1024, slots=2, name=f"big/pb{8 if f32 else 4}/r2")
    pb2 = 32 if f32 else 16
    if N <= 512 and N >= 3 * pb2 and e("LQP_LU2", 1) != 0 and 2 * 8 * ((B + 7) // 8) <= cus:
        return dict(kernel="two", pb=pb2, ntp=256, slots=2, name=f"two/pb{pb2}")
    nt = 512 if N <= 512 else 1024
    mpad = -(-N // 64) * 64
    widest = (16 if f32 else 8) * (2 if nt == 512 else 1)
    pb = 32 if (widest >= 32 and 2 * 32 * mpad * sz <= 128 * 1024) else 16 if (widest >= 16 and 2 * 16 * mpad * sz <= 128 * 1024) else 8
    mfma = True
    if f32:
        if e("LQP_LU_NT", 0) == 1024:
            nt, pb = 1024, min(pb, 16)
        want = e("LQP_LU_PB", 0)
        if (want in (8, 16) or (want == 32 and nt == 512)) and 2 * want * mpad * 4 <= 128 * 1024:
            pb = want
        mfma = e("LQP_LU_MFMA", 1) != 0 and pb != 8
    return dict(kernel="one", pb=pb, ntp=nt, slots=1, name=f"one/pb{pb}/{'mfma' if mfma else 'valu'}/{nt}")


def holder(rel, ntp):
    """Who holds relative panel row `rel` (numpy arrays welcome): thread, register slot, lane, 16-lane row, wave -- one row per
    thread in k_lu_factor (ntp = the workgroup), rows t + q * 256 in the panel waves of lqp_lu2.hpp and lqp_lu_wide.hpp, rows
    t + q * 1024 in k_lu_factor_big."""
    t = rel % ntp
    return dict(thread=t, slot=rel // ntp, lane=t % 64, row16=(t % 64) // 16, wave=t // 64)


# ---------------------------------------------------------------------------------------------------------------------------------
# the plant
class _Plant:
    def __init__(self, N, pb, ntp, seed, reserved=()):
        self.N, self.pb, self.ntp = N, pb, ntp
        self.rng = np.random.RandomState(seed)
        self.L = {}                                   # (final row, column) -> multiplier
        self.swap = {}                                # swap column -> partner
        self.free = np.ones(N, dtype=bool)            # positions in no transposition yet
        self.reserved = set(reserved)                 # columns that never swap and carry no multiplier (the zero pivots)

    def sign(self):
        return 1.0 if self.rng.rand() < 0.5 else -1.0

    def add_swap(self, k, s):
        assert k < s and self.free[k] and self.free[s] and k not in self.reserved
        self.free[k] = self.free[s] = False
        self.swap[k] = s
        self.L[(s, k)] = 0.5 * self.sign()            # the row that sat on the diagonal goes down with +-1/2

    def partners(self, lo, count, far, ok=None):
        """`count` free positions >= lo (that satisfy ok): the nearest ones, or (far) the last ones."""
        idx = np.nonzero(self.free[lo:])[0] + lo
        if ok is not None:
            idx = np.array([p for p in idx if ok(int(p))], dtype=int)
        if len(idx) < count:
            return None
        return list(idx[-count:]) if far else list(idx[:count])

    def find(self, k0, lo, hi, pred):
        """The smallest free position p in [lo, hi) whose holder in the panel at k0 satisfies pred."""
        for p in np.nonzero(self.free[lo:hi])[0] + lo:
            if pred(int(p), holder(int(p) - k0, self.ntp)):
                return int(p)
        return None


def _plan(N, pb, ntp, slots, seed, first_kind, reserved=()):
    P = _Plant(N, pb, ntp, seed, reserved)
    # Panels take roles in fours (shifted by the row's first_kind): two panels of the kinds below in turn, one swap-then-tie
    # panel, one POOL panel whose rows serve as the near partners of the others -- a position can be in one transposition only,
    # so partners taken from anywhere would leave no later panel with all its columns free (the "pb displaced rows" kind).
    seq = ("none", "inside", "d1", "d8", "d9", "dpb")
    ki = first_kind
    pool = lambda p: ((p // pb) + first_kind) % 4 == 3
    npanel = -(-N // pb)
    if N % pb:
        # the last, partial panel (first, while its rows are free): a swap inside it, then a tie between the displaced row and
        # the diagonal
        cols = [c for c in range((npanel - 1) * pb, N) if c not in P.reserved]
        if len(cols) >= 3 and cols[-1] == N - 1:
            P.add_swap(cols[0], N - 1)
            P.L[(N - 1, cols[1])] = P.sign()
        elif len(cols) >= 2:
            P.add_swap(cols[0], cols[-1])
    for k in range(npanel):
        k0 = k * pb
        pbk = min(pb, N - k0)
        below = k0 + pbk
        cols = [c for c in range(k0, below) if c not in P.reserved and P.free[c]]
        nfree_below = int(P.free[below:].sum())
        if pbk < pb:
            continue
        role = (k + first_kind) % 4
        done = None
        if role == 2 and len(cols) >= 4 and nfree_below >= 8:
            # column 0 swaps with a far row s; later columns tie that displaced row (thread of column 0, slot 0) with a row
            # at a smaller position in a higher lane / 16-lane row / wave / slot
            s = P.partners(below, 1, far=True)[0]
            c0 = cols[0]
            P.add_swap(c0, int(s))
            h0 = holder(c0 - k0, ntp)
            rest = cols[1:]
            P.L[(s, rest[0])] = P.sign()                                  # against the diagonal: same 16-lane row
            rest = rest[1:]
            preds = [("wave16", lambda h: h["slot"] == 0 and h["wave"] == h0["wave"] and h["row16"] > h0["row16"]),
                     ("waves", lambda h: h["slot"] == 0 and h["wave"] > h0["wave"]),
                     ("slot", lambda h: h["thread"] == h0["thread"] and h["slot"] > 0),
                     ("row16", lambda h: h["slot"] == 0 and h["wave"] == h0["wave"] and h["row16"] == h0["row16"] and h["lane"] > h0["lane"])]
            if slots > 1 and (k // 4) % 2 == 1:       # (panels of 4 columns have room for two of them)
                preds = preds[2:] + preds[:2]
            for cls, pred in preds:
                if not rest:
                    break
                p = P.find(k0, below, int(s), lambda q, h: pool(q) and pred(h))
                if p is None:
                    p = P.find(k0, below, int(s), lambda q, h: pred(h))
                if p is None:
                    continue
                j = rest[0]
                rest = rest[1:]
                P.add_swap(j, p)                                          # a tied swap column: the planted row at p ...
                P.L[(s, j)] = P.sign()                                    # ... and the displaced row below it, as large
            if pb >= 32 and len(rest) > 1 and rest[-1] - k0 >= 16:
                P.L[(s, rest[-1])] = P.sign()                             # against a diagonal in the second 16-lane row
            done = "swaptie"
        elif role != 3:
            for t in range(len(seq)):
                kind = seq[(ki + t) % len(seq)]
                if kind == "none":
                    done = kind
                elif kind == "inside" and len(cols) >= 4:
                    P.add_swap(cols[0], cols[2])
                    P.add_swap(cols[1], cols[3])
                    done = kind
                elif kind in ("d1", "d8", "d9", "dpb"):
                    c = {"d1": 1, "d8": 8, "d9": 9, "dpb": pb}[kind]
                    if c > len(cols) or nfree_below - c < 6:
                        continue
                    near = P.partners(below, (c + 1) // 2, far=False, ok=pool) or P.partners(below, (c + 1) // 2, far=False)
                    for s in near:
                        P.free[s] = False
                    farp = P.partners(below, c // 2, far=True) if c // 2 else []
                    for s in near:
                        P.free[s] = True
                    for col, s in zip(cols[:c], near + farp):
                        P.add_swap(col, int(s))
                    done = kind
                if done:
                    ki += t + 1
                    break
    # filler: two multipliers per row, +-1/2 in swap columns, +-1/2 or +-1 (a tie with the diagonal) elsewhere
    for i in range(1, N):
        for j in P.rng.randint(0, i, size=2):
            j = int(j)
            if (i, j) in P.L or j in P.reserved:
                continue
            P.L[(i, j)] = P.sign() * (0.5 if (j in P.swap or P.rng.rand() < 0.5) else 1.0)
    # U: diagonal +-2^k, two small integers above it per row
    U = {}
    for i in range(N):
        U[(i, i)] = 0.0 if i in P.reserved else P.sign() * float(2 ** P.rng.randint(0, 3))
        if i + 1 < N:
            for j in P.rng.randint(i + 1, N, size=2):
                U[(i, int(j))] = P.sign() * float(P.rng.randint(1, 3))
    for j in P.reserved:                              # a zero pivot by cancellation, not a zero input column
        if j > 0 and not any((i, j) in U for i in range(j)):
            U[(j - 1, j)] = P.sign()
    return P, U


@functools.lru_cache(maxsize=4)
def _planted_cached(N, pb, ntp, slots, seed, first_kind, reserved):
    P, U = _plan(N, pb, ntp, slots, seed, first_kind, reserved)
    LU = np.zeros((N, N))
    A = np.zeros((N, N))
    urows = {}
    for (i, j), v in U.items():
        LU[i, j] = v
        urows.setdefault(i, []).append((j, v))
    lrows = {i: [(i, 1.0)] for i in range(N)}
    for (i, j), v in P.L.items():
        LU[i, j] = v
        lrows[i].append((j, v))
    for i in range(N):
        for k, l in lrows[i]:
            for j, u in urows[k]:
                A[i, j] += l * u
    ipiv = np.arange(1, N + 1, dtype=np.int32)
    for k, s in P.swap.items():
        A[[k, s]] = A[[s, k]]
        ipiv[k] = s + 1
    return A, LU, ipiv


def geometry(r):
    s = select(r["N"], r["B"], r["dtype"], r["env"])
    return s["pb"], s["ntp"], s["slots"]


def _key(r):
    pb, ntp, slots = geometry(r)
    return (r["N"], pb, ntp, slots, 1000 + r["N"], r["first_kind"], tuple(r["zero"] or ()))


def planted(r):
    """(A', LU_want, ipiv_want) of the row as float64 / int32 CPU tensors of shape (B, N, N) / (B, N); A' and LU_want are exact in
    float32 too (cast with .to(DTYPES[r["dtype"]]))."""
    A, LU, ipiv = _planted_cached(*_key(r))
    A, LU, ipiv = torch.from_numpy(A), torch.from_numpy(LU), torch.from_numpy(ipiv)
    if r["B"] == 1:
        return A[None].clone(), LU[None].clone(), ipiv[None].clone()
    assert r["B"] == 2
    return torch.stack([A, -A]), torch.stack([LU, torch.tril(LU, -1) - torch.triu(LU)]), torch.stack([ipiv, ipiv])


# ---------------------------------------------------------------------------------------------------------------------------------
# plain getf2 with the holders of the row's kernel
def getf2(A, pb, ntp, rule="first", stop_at=None):
    """Unblocked LU with partial pivoting of the float64 matrix A (numpy), LAPACK layout, explicit interchanges, l = 0 on a zero
    pivot column.  Ties: rule "first" = the smallest position (isamax); the wrong rules "lowthread" (the tied row in the lowest
    thread, then slot, of the panel of width pb -- what an arg-max by lane gives) and "highpos".  Tracks who holds every live row
    in the kernel whose panel threads keep relative rows t + q * ntp.  stop_at: pivots to compare with, stop at the first that
    differs (the wrong rules fill the matrix in).  Returns dict(LU, ipiv, info, ties, panels, diff)."""
    S = np.array(A, dtype=np.float64)
    N = S.shape[0]
    ipiv = np.zeros(N, dtype=np.int32)
    info = 0
    ties, panels = [], []
    phys = np.arange(N)                    # position -> relative row its holder loaded (this panel)
    diff = None
    for j in range(N):
        k0 = (j // pb) * pb
        if j == k0:
            phys[k0:] = np.arange(N - k0)
            pan = dict(k0=k0, pb=min(pb, N - k0), swaps=0, ties=0, tie_after_swap=False, nonlowest_after_swap=False)
            panels.append(pan)
        a = np.abs(S[j:, j])
        m = a.max()
        tied = np.nonzero(a == m)[0] + j
        if len(tied) > 1:
            h = holder(phys[tied], ntp)
            if rule == "first":
                w = 0
            elif rule == "highpos":
                w = len(tied) - 1
            else:
                w = int(np.lexsort((h["slot"], h["thread"]))[0])
            # the classes of this step: the true winner (smallest position, index 0) against every other tied row
            same_t = h["thread"][1:] == h["thread"][0]
            same_w = h["wave"][1:] == h["wave"][0]
            same_r = same_w & (h["row16"][1:] == h["row16"][0])
            cls = {"slot": same_t, "row16": same_r & ~same_t, "wave16": same_w & ~same_r, "waves": ~same_w}
            low = {"slot": h["slot"][1:] < h["slot"][0], "row16": h["lane"][1:] < h["lane"][0],
                   "wave16": h["row16"][1:] < h["row16"][0], "waves": h["wave"][1:] < h["wave"][0]}
            rec = dict(step=j, panel=len(panels) - 1, zero=bool(m == 0), n=len(tied),
                       classes={c for c in CLASSES if cls[c].any()},
                       nonlowest={c for c in CLASSES if (cls[c] & low[c]).any()},
                       tied=[(int(p), int(h["thread"][i]), int(h["slot"][i])) for i, p in enumerate(tied[:6])])
            ties.append(rec)
            if m > 0:
                pan["ties"] += 1
                if pan["swaps"]:
                    pan["tie_after_swap"] = True
                    pan["nonlowest_after_swap"] = pan["nonlowest_after_swap"] or bool(rec["nonlowest"])
        else:
            w = 0
        p = int(tied[w])
        ipiv[j] = p + 1
        if stop_at is not None and ipiv[j] != stop_at[j]:
            diff = j
            break
        if m == 0 and info == 0:
            info = j + 1
        if p != j:
            S[[j, p]] = S[[p, j]]
            phys[[j, p]] = phys[[p, j]]
            pan["swaps"] += 1
        if m > 0 and j + 1 < N:
            l = S[j + 1:, j] / S[j, j]
            S[j + 1:, j] = l
            rows = np.nonzero(l)[0]
            cols = np.nonzero(S[j, j + 1:])[0]
            if len(rows) and len(cols):
                S[np.ix_(rows + j + 1, cols + j + 1)] -= np.outer(l[rows], S[j, cols + j + 1])
        if j == k0 + pan["pb"] - 1:
            # the panel's bookkeeping as the kernels keep it: src[j] != j, displaced rows ne
            rel = np.arange(N - k0)
            moved = phys[k0:] != rel
            pan["ne"] = int(moved[pan["pb"]:].sum())
            pan["anyswap"] = bool(moved.any())
            pan["full"] = pan["pb"] == pb
    return dict(LU=S, ipiv=ipiv, info=info, ties=ties, panels=panels, diff=diff)


@functools.lru_cache(maxsize=4)
def _holders_cached(key, pb, ntp):
    A = _planted_cached(*key)[0]
    return getf2(A, pb, ntp)


def holders(r):
    pb, ntp, _ = geometry(r)
    return _holders_cached(_key(r), pb, ntp)


def panel_kinds(h, pb):
    """The kinds of panel the plain getf2 saw (a panel may count for several)."""
    out = set()
    for p in h["panels"]:
        if not p["full"]:
            if p["swaps"] and p["ties"]:
                out.add("last")
            continue
        if not p["anyswap"]:
            out.add("none")
        elif p["ne"] == 0:
            out.add("inside")
        for kind, c in (("d1", 1), ("d8", 8), ("d9", 9), ("dpb", pb)):
            if p["ne"] == c:
                out.add(kind)
        if p["nonlowest_after_swap"]:
            out.add("swaptie")
    return out


def kinds_possible(pb):
    return {"none", "inside", "d1", "dpb", "swaptie", "last"} | ({"d8"} if pb >= 8 else set()) | ({"d9"} if pb >= 9 else set())


def tie_classes(h, nonlowest=False):
    out = set()
    for t in h["ties"]:
        if not t["zero"]:
            out |= t["nonlowest"] if nonlowest else t["classes"]
    return out


def classes_possible(kernel):
    return {"row16", "wave16", "waves"} | (set() if kernel == "one" else {"slot"})


def explain(r, LU, piv):
    """Why a GPU result is wrong: the first wrong pivot column with its panel, tie and holders, or the first wrong tile."""
    _, LU_want, ipiv_want = planted(r)
    pb, ntp, _ = geometry(r)
    h = holders(r)
    lines = []
    for b in range(r["B"]):
        bad = torch.nonzero(piv[b].cpu().int() != ipiv_want[b].int())
        if bad.numel():
            j = int(bad[0])
            tie = next((t for t in h["ties"] if t["step"] == j), None)
            lines.append(f"matrix {b}: first wrong pivot at column {j} (panel {j // pb}, column {j % pb} of it): got "
                         f"{int(piv[b, j])}, want {int(ipiv_want[b, j])}; tie: {tie}  [tied rows as (position, thread, slot)]")
            continue
        d = torch.nonzero(LU[b].cpu().double() != LU_want[b])
        if d.numel():
            i, j = int(d[0, 0]), int(d[0, 1])
            lines.append(f"matrix {b}: pivots right; first wrong entry ({i}, {j}) in the 32 x 32 tile ({i // 32}, {j // 32}), panel "
                         f"{min(i, j) // pb}: got {float(LU[b, i, j])!r}, want {float(LU_want[b, i, j])!r}; {d.shape[0]} wrong entries")
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------------------------
# the rows
EXPECT_ONLY = "the instantiations of the one-workgroup kernel write the same four counters: that THIS one ran rests on expect_kernel"
COUNTERS = "the cycle counters of lqp_debug_set_lu_counters tell this family's launch from the others"
BIG_NONE = "k_lu_factor_big writes no counters: none written, and a size only it takes"


def row(name, N, kernel, dtype="f32", B=1, env=None, zero=None, first_kind=0, why=None):
    env = dict(env or {})
    if N <= 130:
        first_kind = 4 * first_kind + 2            # few panels: the first one a swap-then-tie panel
    r = dict(name=f"{name}_{dtype}", N=N, B=B, dtype=dtype, env=env, kernel=kernel, zero=zero, first_kind=first_kind)
    r["expect_kernel"] = select(N, B, dtype, env)["name"]
    r["why"] = why or (EXPECT_ONLY if kernel == "one" else BIG_NONE if kernel == "big" else COUNTERS)
    return r


def _rows():
    rows = []
    one = {"LQP_LU2": "0"}
    fk = 0
    # one workgroup, 512 threads, float32: every panel width and both trailing updates; and the same sizes on 1024 threads
    for N in (70, 130, 512):
        for pb in (8, 16, 32):
            for mf in ((0,) if pb == 8 else (0, 1)):
                rows.append(row(f"one{N}_pb{pb}_mf{mf}", N, "one", env=dict(one, LQP_LU_PB=str(pb), LQP_LU_MFMA=str(mf)), first_kind=fk))
                fk += 1
        for pb in (8, 16):
            rows.append(row(f"one{N}_nt1024_pb{pb}", N, "one", env=dict(one, LQP_LU_NT="1024", LQP_LU_PB=str(pb)), first_kind=fk))
            fk += 1
        rows.append(row(f"one{N}", N, "one", dtype="f64", env=one, first_kind=fk))
    # one workgroup, 1024 threads (517: a partial last panel of 5 columns)
    for N in (513, 517, 1024):
        rows.append(row(f"one{N}", N, "one", first_kind=fk))
        rows.append(row(f"one{N}", N, "one", dtype="f64", first_kind=fk + 1))
        fk += 2
    # N = 1 and N = PB exactly
    rows += [row("one1", 1, "one"), row("one1", 1, "one", dtype="f64"), row("one32", 32, "one"), row("one16", 16, "one", dtype="f64"),
             row("one8_pb8", 8, "one", env={"LQP_LU_PB": "8"})]
    # two workgroups at B = 2, both sides of N >= 3 PB (below it the one-workgroup kernel takes the row); 101: a partial panel of 5
    for N in (47, 48, 95, 96, 101, 130, 512):
        for dt in ("f32", "f64"):
            k = select(N, 2, dt)["kernel"]
            rows.append(row(f"two{N}", N, k, dtype=dt, B=2, first_kind=fk))
            fk += 1
    # two and four rows per thread (1031 / 2055: partial last panels of 7 | 3 columns)
    nowide = {"LQP_LU_WIDE": "0"}
    for N in (1025, 1031, 2048):
        for dt in ("f32", "f64"):
            rows.append(row(f"big{N}", N, "big", dtype=dt, env=nowide, first_kind=fk))
            rows.append(row(f"wide{N}", N, "wide", dtype=dt, B=2, first_kind=fk + 1))
            fk += 2
    for N in (2049, 2055, 4096):
        rows.append(row(f"big{N}", N, "big", env=nowide, first_kind=fk))
        rows.append(row(f"tall{N}", N, "tall", first_kind=fk + 1))
        fk += 2
    # zero pivots by exact cancellation (U[j,j] = 0): first / last column, first / last column of a panel, the edge of a column
    # tile of the wide kernels, two of them (the first is reported)
    def zeros(name, N, kernel, dt, B=1, env=None, tile=None, few=False):
        pb = select(N, B, dt, env)["pb"]
        js = [(pb + 1, N - 2)] if few else [(0,), (N - 1,), (pb,), (2 * pb - 1,), (pb + 1, N - 2)]
        if tile:
            js += [(tile - 1,), (tile,)]
        return [row(f"{name}_z{'_'.join(map(str, z))}", N, kernel, dtype=dt, B=B, env=env, zero=z, first_kind=6) for z in js]
    rows += zeros("one70", 70, "one", "f32", env=one) + zeros("one70", 70, "one", "f64", env=one)
    rows += zeros("one70_pb8", 70, "one", "f32", env=dict(one, LQP_LU_PB="8"), few=True)
    rows += zeros("one517", 517, "one", "f32", few=True) + zeros("one517", 517, "one", "f64", few=True)
    rows += zeros("two130", 130, "two", "f32", B=2) + zeros("two130", 130, "two", "f64", B=2)
    rows += zeros("big1031", 1031, "big", "f32", env=nowide, few=True) + zeros("big1031", 1031, "big", "f64", env=nowide, few=True)
    rows += zeros("wide1031", 1031, "wide", "f32", B=2, tile=32) + zeros("wide1031", 1031, "wide", "f64", B=2, tile=16, few=True)
    rows += zeros("big2055", 2055, "big", "f32", env=nowide, few=True) + zeros("tall2055", 2055, "tall", "f32", tile=32, few=True)
    return rows


ROWS = _rows()
ROW_BY_NAME = {r["name"]: r for r in ROWS}
assert len(ROW_BY_NAME) == len(ROWS)
REGULAR = [r for r in ROWS if r["zero"] is None]
SINGULAR = [r for r in ROWS if r["zero"] is not None]
