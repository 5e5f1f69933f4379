"""The deterministic seed search of tests/unroll_table.py: for each row (or the rows named on the command line) the smallest seed
offset j < 16 at which the clamp decisions of the sampled problems are settled (unroll_table.settled), with the oracle's n_factor.
Prints one line per row; the chosen j is written into the table by hand, so that no test searches.
    python tests/tools/unroll_seed_search.py [row ...]"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import unroll_table as U  # noqa: E402


def search(r):
    for j in range(16):
        t0 = time.time()
        _, _, t64, t32, tr64, tr32 = U.row_tapes(r, j=j)
        v = U.settled(r, tr64, tr32)
        nf = (t64["n_factor"], None if t32 is None else t32["n_factor"])
        finite = all(bool(t.isfinite().all()) for t in t64.values() if hasattr(t, "isfinite"))
        print(f"  {r['name']} j={j} settled={v:.3g} n_factor={nf} finite={finite} {time.time() - t0:.1f}s", flush=True)
        if U.settled_ok(r, v) and len(set(x for x in nf if x is not None)) == 1 and nf[0] == r["n_factor"]:
            return j, v
    return None, None


if __name__ == "__main__":
    names = sys.argv[1:] or [r["name"] for r in U.ROWS]
    for name in names:
        j, v = search(U.ROW_BY_NAME[name])
        print(f"{name}: j = {j} (settled {v})", flush=True)
