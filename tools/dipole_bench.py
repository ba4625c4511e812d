"""Timing aid: the point-dipole Ewald term beside the charge routines it accompanies, in the same process on the same inputs.

Real space: `ewald_dipole_real_space` beside `ewald_real_space` and `gaussian_charge_correction` on the list of BASELINE config 4 (100 000-atom
periodic FCC box, 9 A full list, padded M = 256, fp64).  Reciprocal space: `ewald_dipole_reciprocal_space` beside `ewald_reciprocal_space` on the
same atoms and the same K k-vectors (Miller indices up to --k-index per axis, half space).  Warm-up, then the median of event-bracketed
repeats of the whole public call.

    python tools/dipole_bench.py [--atoms 100000] [--k-index 6] [--repeats 30] [--dtype f64]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nvalchemi-toolkit-ops_amd")]
from tests import systems as S  # noqa: E402

from nvalchemiops.interactions.electrostatics import (ewald_dipole_real_space, ewald_dipole_reciprocal_space, ewald_real_space,  # noqa: E402
                                                      ewald_reciprocal_space, gaussian_charge_correction, generate_k_vectors_ewald_summation)
from nvalchemiops.neighborlist import cell_list  # noqa: E402
from tools.gaussian_bench import median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--cutoff", type=float, default=9.0)
    ap.add_argument("--max-neighbors", type=int, default=256)
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--alpha", type=float, default=0.35)
    ap.add_argument("--k-index", type=int, default=6, help="largest Miller index per axis of the k set")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f64")
    args = ap.parse_args()
    dev, dt = "cuda:0", (torch.float64 if args.dtype == "f64" else torch.float32)
    pos, cell, q, _ = S.fcc_box(args.atoms, dtype=np.float64)
    n = pos.shape[0]
    P, C, Q = (torch.as_tensor(a, device=dev, dtype=dt) for a in (pos, cell, q))
    C = C.reshape(1, 3, 3)
    M = torch.as_tensor(0.3 * np.random.default_rng(0).normal(size=(n, 3)), device=dev, dtype=dt)
    pbc = torch.ones(3, dtype=torch.bool, device=dev)
    nm, num, sh = cell_list(P, args.cutoff, C[0], pbc, max_neighbors=args.max_neighbors)
    assert int(num.max()) <= args.max_neighbors, "rows overflow: raise --max-neighbors"
    sig = torch.full((n,), args.sigma, dtype=dt, device=dev)
    alpha = torch.tensor([args.alpha], dtype=dt, device=dev)
    kv = generate_k_vectors_ewald_summation(C, 2.0 * math.pi * (args.k_index - 0.01) / float(torch.linalg.norm(C[0], dim=-1).max()))
    lists = dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=n)
    every = dict(compute_forces=True, compute_charge_gradients=True, compute_dipole_gradients=True, compute_virial=True)
    cases = {
        "ewald_real_space E+F": lambda: ewald_real_space(P, Q, C, alpha, compute_forces=True, **lists),
        "gaussian_charge_correction E+F": lambda: gaussian_charge_correction(P, Q, sig, C, compute_forces=True, **lists),
        "ewald_dipole_real_space E": lambda: ewald_dipole_real_space(P, Q, M, C, alpha, **lists),
        "ewald_dipole_real_space E+F": lambda: ewald_dipole_real_space(P, Q, M, C, alpha, compute_forces=True, **lists),
        "ewald_dipole_real_space E+F+dq+dmu+virial": lambda: ewald_dipole_real_space(P, Q, M, C, alpha, **every, **lists),
        "ewald_reciprocal_space E+F": lambda: ewald_reciprocal_space(P, Q, C, kv, alpha, compute_forces=True),
        "ewald_dipole_reciprocal_space E": lambda: ewald_dipole_reciprocal_space(P, Q, M, C, kv, alpha),
        "ewald_dipole_reciprocal_space E+F": lambda: ewald_dipole_reciprocal_space(P, Q, M, C, kv, alpha, compute_forces=True),
        "ewald_dipole_reciprocal_space E+F+dq+dmu+virial": lambda: ewald_dipole_reciprocal_space(P, Q, M, C, kv, alpha, **every),
    }
    result = {"atoms": n, "cutoff": args.cutoff, "max_neighbors": args.max_neighbors, "dtype": args.dtype, "k_vectors": int(kv.shape[0]),
              "stored_entries": int(num.sum()), "slots": int(nm.numel()), "repeats": args.repeats, "ms": {}}
    for name, fn in cases.items():
        med, best = median_ms(fn, args.warmup, args.repeats)
        result["ms"][name] = {"median": round(med, 4), "min": round(best, 4)}
        print(f"{name:50s} median {med:.3f} ms   min {best:.3f} ms", flush=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
