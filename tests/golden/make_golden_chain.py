"""Generate the narrow-shape chain goldens (chain_solve_n8_*.npz) by running the REFERENCE.

make_golden_wide.py's recipe (the same chain, problem data, settings and 1e-3 argmin-gap
filter, imported from it) at n = 8, m = 2, where the select and the Riccati pass both run
the narrow kernels.  Run it the same way, from outside both trees:

    PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_chain.py [REFERENCE_DIR]

Seeds 4008, 4009 and 4010 are kept (T_hist [13, 13, 13], [9, 9, 9], [16, 16, 16]; minimum
gaps 1.0e-2, 4.1e-2, 2.4e-2).  Each file holds data only.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import make_golden_wide as wide  # noqa: E402  (imports the reference's solver)

N_STATES, M_INPUTS = 8, 2


def main():
    kept, seed = 0, 4000 + N_STATES
    while kept < wide.KEEP:
        d = wide.run(N_STATES, M_INPUTS, seed)
        ok = len(d["gaps"]) > 0 and d["gaps"].min() >= wide.MIN_GAP and len(d["T_hist"]) >= 2
        print(f"n={N_STATES} seed={seed} selects={len(d['gaps'])} min gap={d['gaps'].min():.2e} "
              f"T_hist={d['T_hist'].tolist()} {'kept' if ok else 'dropped'}")
        if ok:
            np.savez(os.path.join(HERE, f"chain_solve_n{N_STATES}_{kept}.npz"), **d)
            kept += 1
        seed += 1
        if seed > 4000 + N_STATES + 40:
            raise RuntimeError("too few trials pass the gap filter")


if __name__ == "__main__":
    main()
