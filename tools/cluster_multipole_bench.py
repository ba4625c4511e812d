"""Timing aid: the bare (1/r) dipole and quadrupole launches beside their Ewald siblings on the same list, and one cluster solve beside
`induced_dipoles(reciprocal="ewald")`, in one process.

(a), (b)  100 000-atom periodic FCC box, 9 A full list (padded M = 256), fp64, random charges (neutral), dipoles and quadrupoles: the list of
          BASELINE config 4 and of tools/thole_bench.py.  `mi_coulomb_dipole` against `mi_ewald_dipole_real` and `mi_coulomb_quadrupole`
          against `mi_ewald_quadrupole_real` through their public functions (same pack kernel, same row walk, same outputs: the radial part
          is the only difference), energies only and with forces + dipole gradients.  The pairs are timed alternately in `--rounds` rounds of
          warm-up + event-bracketed repeats; the table gives the median of the round medians and their range, which is the run-to-run spread
          of this session that a difference has to exceed.
(c)       `--solve-atoms` atoms of that lattice: `cluster_induced_dipoles` on the list WITHOUT images (a free cluster), undamped and with
          thole = 0.39, beside `induced_dipoles(reciprocal="ewald")` on the periodic list of the same atoms; polarisabilities uniform in
          [0.02, 0.08] d_min^3 (the set of tools/induced_bench.py).  Iterations and ms.

The tables of DESIGN.md section 3.29 are the `--markdown` output of this tool.

    python tools/cluster_multipole_bench.py [--atoms 100000] [--solve-atoms 8788] [--repeats 20] [--rounds 3] [--markdown]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nvalchemi-toolkit-ops_amd")]
from tests import systems as S  # noqa: E402

from nvalchemiops.interactions.electrostatics import (cluster_induced_dipoles, coulomb_dipole_correction,  # noqa: E402
                                                      coulomb_quadrupole_correction, ewald_dipole_real_space, ewald_quadrupole_real_space,
                                                      generate_k_vectors_ewald_summation, induced_dipoles)
from nvalchemiops.neighborlist import cell_list  # noqa: E402
from tools.induced_bench import median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--solve-atoms", type=int, default=8788)
    ap.add_argument("--cutoff", type=float, default=9.0)
    ap.add_argument("--max-neighbors", type=int, default=256)
    ap.add_argument("--alpha", type=float, default=0.35)
    ap.add_argument("--k-cutoff", type=float, default=2.4)
    ap.add_argument("--thole", type=float, default=0.39)
    ap.add_argument("--tolerance", type=float, default=1e-8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--solve-repeats", type=int, default=3)
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    dev, dt = "cuda:0", torch.float64
    g = np.random.default_rng(0)
    t = lambda a: torch.as_tensor(a, device=dev, dtype=dt)  # noqa: E731
    yes, no = torch.ones(3, dtype=torch.bool, device=dev), torch.zeros(3, dtype=torch.bool, device=dev)
    result = {"atoms": args.atoms, "cutoff": args.cutoff, "max_neighbors": args.max_neighbors, "repeats": args.repeats, "rounds": args.rounds,
              "ms": {}, "solves": {}}

    # ---- (a), (b): the pair launches on one list -------------------------------------------------------------------------------------
    pos, cell, _, _ = S.fcc_box(args.atoms, dtype=np.float64)
    n = pos.shape[0]
    P, Cl = t(pos), t(cell).reshape(1, 3, 3)
    q = g.normal(size=n)
    q, mu, Q = t(q - q.mean()), t(0.3 * g.normal(size=(n, 3))), t(0.2 * g.normal(size=(n, 3, 3)))
    nm, num, sh = cell_list(P, args.cutoff, Cl[0], yes, max_neighbors=args.max_neighbors)
    assert int(num.max()) <= args.max_neighbors, "rows overflow: raise --max-neighbors"
    result.update(slots=int(nm.numel()), stored=int(num.sum()))
    alpha = torch.tensor([args.alpha], dtype=dt, device=dev)
    lists = dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=n)
    grads = dict(compute_forces=True, compute_dipole_gradients=True)
    pairs = []
    for label, extra in (("energies", {}), ("forces + dipole gradients", grads)):
        pairs.append((f"a ewald_dipole_real_space, {label}", lambda extra=extra: ewald_dipole_real_space(P, q, mu, Cl, alpha, **extra, **lists)))
        pairs.append((f"a coulomb_dipole_correction, {label}", lambda extra=extra: coulomb_dipole_correction(P, q, mu, Cl, **extra, **lists)))
    for label, extra in (("energies", {}), ("forces + dipole gradients", grads)):
        pairs.append((f"b ewald_quadrupole_real_space, {label}",
                      lambda extra=extra: ewald_quadrupole_real_space(P, q, mu, Q, Cl, alpha, **extra, **lists)))
        pairs.append((f"b coulomb_quadrupole_correction, {label}", lambda extra=extra: coulomb_quadrupole_correction(P, q, mu, Q, Cl, **extra, **lists)))
    rounds = {name: [] for name, _ in pairs}
    for _ in range(args.rounds):  # siblings alternate inside a round, rounds repeat: the spread of the round medians is this session's noise
        for name, fn in pairs:
            rounds[name].append(median_ms(fn, args.warmup, args.repeats)[0])
    for name, v in rounds.items():
        result["ms"][name] = {"median": round(float(np.median(v)), 4), "low": min(v), "high": max(v)}
        print(f"{name:64s} median of {args.rounds} round medians {np.median(v):.3f} ms   range {min(v):.3f} - {max(v):.3f} ms", flush=True)
    del nm, num, sh, P, q, mu, Q

    # ---- (c): one solve --------------------------------------------------------------------------------------------------------------
    pos, cell, _, _ = S.fcc_box(args.solve_atoms, dtype=np.float64)
    n = pos.shape[0]
    P, Cl = t(pos), t(cell).reshape(1, 3, 3)
    q = g.normal(size=n)
    q = t(q - q.mean())
    per = cell_list(P, args.cutoff, Cl[0], yes, max_neighbors=args.max_neighbors)
    free = cell_list(P, args.cutoff, Cl[0], no, max_neighbors=args.max_neighbors)
    assert int(per[1].max()) <= args.max_neighbors
    row = per[0][0, : int(per[1][0])].long()
    d_min = float(torch.linalg.norm(P[row] - P[0] + per[2][0, : int(per[1][0])].to(dt) @ Cl[0], dim=-1).min())
    polar = t(g.uniform(0.02, 0.08, n) * d_min**3)
    kv = generate_k_vectors_ewald_summation(Cl, args.k_cutoff)
    result.update(solve_atoms=n, d_min=d_min, k_vectors=int(kv.shape[-2]), stored_periodic=int(per[1].sum()), stored_free=int(free[1].sum()))
    solves = {
        "induced_dipoles(reciprocal='ewald'), periodic list": lambda: induced_dipoles(
            P, q, polar, Cl, reciprocal="ewald", alpha=alpha, k_vectors=kv, tolerance=args.tolerance, return_info=True, neighbor_matrix=per[0],
            neighbor_matrix_shifts=per[2], mask_value=n),
        "cluster_induced_dipoles, free list": lambda: cluster_induced_dipoles(P, q, polar, tolerance=args.tolerance, return_info=True,
                                                                              neighbor_matrix=free[0], mask_value=n),
        f"cluster_induced_dipoles(thole={args.thole:g}), free list": lambda: cluster_induced_dipoles(
            P, q, polar, thole=args.thole, tolerance=args.tolerance, return_info=True, neighbor_matrix=free[0], mask_value=n),
    }
    for name, solve in solves.items():
        out = solve()
        med, best = median_ms(solve, 1, args.solve_repeats)
        result["solves"][name] = {"iterations": int(out.iterations[0]), "residual": float(out.residual[0]), "median_ms": med, "min_ms": best}
        print(f"c {name} to {args.tolerance:g}: {int(out.iterations[0])} iterations, median {med:.2f} ms, min {best:.2f} ms", flush=True)
    print(json.dumps(result))
    if args.markdown:
        print(f"\n| pass | median of {args.rounds} round medians, ms | range of the round medians, ms |\n|---|---|---|")
        for name, v in result["ms"].items():
            print(f"| {name[2:]} | {v['median']:.3f} | {v['low']:.3f} - {v['high']:.3f} |")
        print("\n| solve to %g | iterations | median ms |\n|---|---|---|" % args.tolerance)
        for name, v in result["solves"].items():
            print(f"| {name} | {v['iterations']} | {v['median_ms']} |")


if __name__ == "__main__":
    main()
