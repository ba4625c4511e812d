"""Timing aid: the point-quadrupole Ewald term beside the point-dipole term it accompanies, in the same process on the same inputs.

Real space: `ewald_quadrupole_real_space` beside `ewald_dipole_real_space` on the list of BASELINE config 4 (100 000-atom periodic FCC box, 9 A
full list, padded M = 256, fp64).  Reciprocal space: `ewald_quadrupole_reciprocal_space` beside `ewald_dipole_reciprocal_space` on the same
atoms and the same K k-vectors (Miller indices up to --k-index per axis, half space).  The adjoints are the backward passes of the energies
under a random upstream gradient.  Warm-up, then the median of event-bracketed repeats of the whole public call.  The real-space rows also
state the algorithmic traffic -- 16 B of list (index + shift code words) plus one record gather per slot -- and the fraction of --peak-tbs
(8 TB/s) the pass reaches with it.

    python tools/quadrupole_bench.py [--atoms 100000] [--k-index 6] [--repeats 30] [--dtype f64]
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

from nvalchemiops.interactions.electrostatics import (ewald_dipole_real_space, ewald_dipole_reciprocal_space,  # noqa: E402
                                                      ewald_quadrupole_real_space, ewald_quadrupole_reciprocal_space,
                                                      generate_k_vectors_ewald_summation)
from nvalchemiops.neighborlist import cell_list  # noqa: E402
from tools.gaussian_bench import median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--cutoff", type=float, default=9.0)
    ap.add_argument("--max-neighbors", type=int, default=256)
    ap.add_argument("--alpha", type=float, default=0.35)
    ap.add_argument("--k-index", type=int, default=6, help="largest Miller index per axis of the k set")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f64")
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="memory bandwidth the real-space fraction is stated against, TB/s")
    args = ap.parse_args()
    dev, dt = "cuda:0", (torch.float64 if args.dtype == "f64" else torch.float32)
    pos, cell, q, _ = S.fcc_box(args.atoms, dtype=np.float64)
    n = pos.shape[0]
    P, C, Q = (torch.as_tensor(a, device=dev, dtype=dt) for a in (pos, cell, q))
    C = C.reshape(1, 3, 3)
    g = np.random.default_rng(0)
    M = torch.as_tensor(0.3 * g.normal(size=(n, 3)), device=dev, dtype=dt)
    T = torch.as_tensor(0.2 * g.normal(size=(n, 3, 3)), device=dev, dtype=dt)
    T = 0.5 * (T + T.transpose(-1, -2))
    W = torch.as_tensor(g.uniform(0.5, 1.5, n), device=dev, dtype=dt)
    pbc = torch.ones(3, dtype=torch.bool, device=dev)
    nm, num, sh = cell_list(P, args.cutoff, C[0], pbc, max_neighbors=args.max_neighbors)
    assert int(num.max()) <= args.max_neighbors, "rows overflow: raise --max-neighbors"
    alpha = torch.tensor([args.alpha], dtype=dt, device=dev)
    kv = generate_k_vectors_ewald_summation(C, 2.0 * math.pi * (args.k_index - 0.01) / float(torch.linalg.norm(C[0], dim=-1).max()))
    lists = dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=n)
    dp_every = dict(compute_forces=True, compute_charge_gradients=True, compute_dipole_gradients=True, compute_virial=True)
    qd_every = dict(compute_quadrupole_gradients=True, **dp_every)

    def adjoint(fn, leaves):
        def run():
            ls = [t.detach().requires_grad_(True) for t in leaves]
            return torch.autograd.grad((fn(*ls) * W).sum(), ls)
        return run

    cases = {
        "ewald_dipole_real_space E": lambda: ewald_dipole_real_space(P, Q, M, C, alpha, **lists),
        "ewald_dipole_real_space E+F": lambda: ewald_dipole_real_space(P, Q, M, C, alpha, compute_forces=True, **lists),
        "ewald_dipole_real_space all outputs": lambda: ewald_dipole_real_space(P, Q, M, C, alpha, **dp_every, **lists),
        "ewald_dipole_real_space E + adjoint": adjoint(lambda p, q_, m: ewald_dipole_real_space(p, q_, m, C, alpha, **lists), (P, Q, M)),
        "ewald_quadrupole_real_space E": lambda: ewald_quadrupole_real_space(P, Q, M, T, C, alpha, **lists),
        "ewald_quadrupole_real_space E+F": lambda: ewald_quadrupole_real_space(P, Q, M, T, C, alpha, compute_forces=True, **lists),
        "ewald_quadrupole_real_space all outputs": lambda: ewald_quadrupole_real_space(P, Q, M, T, C, alpha, **qd_every, **lists),
        "ewald_quadrupole_real_space E + adjoint": adjoint(lambda p, q_, m, t: ewald_quadrupole_real_space(p, q_, m, t, C, alpha, **lists),
                                                           (P, Q, M, T)),
        "ewald_dipole_reciprocal_space E": lambda: ewald_dipole_reciprocal_space(P, Q, M, C, kv, alpha),
        "ewald_dipole_reciprocal_space E+F": lambda: ewald_dipole_reciprocal_space(P, Q, M, C, kv, alpha, compute_forces=True),
        "ewald_dipole_reciprocal_space all outputs": lambda: ewald_dipole_reciprocal_space(P, Q, M, C, kv, alpha, **dp_every),
        "ewald_dipole_reciprocal_space E + adjoint": adjoint(lambda p, q_, m: ewald_dipole_reciprocal_space(p, q_, m, C, kv, alpha), (P, Q, M)),
        "ewald_quadrupole_reciprocal_space E": lambda: ewald_quadrupole_reciprocal_space(P, Q, M, T, C, kv, alpha),
        "ewald_quadrupole_reciprocal_space E+F": lambda: ewald_quadrupole_reciprocal_space(P, Q, M, T, C, kv, alpha, compute_forces=True),
        "ewald_quadrupole_reciprocal_space all outputs": lambda: ewald_quadrupole_reciprocal_space(P, Q, M, T, C, kv, alpha, **qd_every),
        "ewald_quadrupole_reciprocal_space E + adjoint": adjoint(lambda p, q_, m, t: ewald_quadrupole_reciprocal_space(p, q_, m, t, C, kv, alpha),
                                                                 (P, Q, M, T)),
    }
    word = 8 if args.dtype == "f64" else 4
    slots = int(nm.numel())
    traffic = {"dipole": slots * 16 + int(num.sum()) * 8 * word, "quadrupole": slots * 16 + int(num.sum()) * 16 * word}
    result = {"atoms": n, "cutoff": args.cutoff, "max_neighbors": args.max_neighbors, "dtype": args.dtype, "k_vectors": int(kv.shape[0]),
              "stored_entries": int(num.sum()), "slots": slots, "repeats": args.repeats, "algorithmic_bytes": traffic, "ms": {}}
    for name, fn in cases.items():
        med, best = median_ms(fn, args.warmup, args.repeats)
        result["ms"][name] = {"median": round(med, 4), "min": round(best, 4)}
        line = f"{name:50s} median {med:.3f} ms   min {best:.3f} ms"
        if "real_space" in name and "adjoint" not in name:
            nbytes = traffic["quadrupole" if "quadrupole" in name else "dipole"]
            frac = nbytes / (med * 1e-3) / (args.peak_tbs * 1e12)
            result["ms"][name]["fraction_of_peak"] = round(frac, 4)
            line += f"   {nbytes / 1e6:.0f} MB algorithmic, {100 * frac:.1f} % of {args.peak_tbs:g} TB/s"
        print(line, flush=True)
    for half in ("real_space", "reciprocal_space"):
        for what in ("E", "E+F", "all outputs", "E + adjoint"):
            ratio = result["ms"][f"ewald_quadrupole_{half} {what}"]["median"] / result["ms"][f"ewald_dipole_{half} {what}"]["median"]
            result.setdefault("ratio_to_dipole", {})[f"{half} {what}"] = round(ratio, 3)
            print(f"quadrupole / dipole, {half} {what}: {ratio:.2f}", flush=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
