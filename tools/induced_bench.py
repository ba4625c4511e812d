"""Timing aid: `induced_dipoles` and its pieces on the list of BASELINE config 4, in one process.

100 000-atom periodic FCC box, 9 A full list (padded M = 256), fp64, random charges (neutral), polarisabilities uniform in
[0.02, 0.08] d_min^3 (d_min the nearest-neighbour distance: H stays positive definite on the close-packed lattice); PME as the headline benchmark runs it (alpha 0.35 / A, mesh 128^3, order 5).  Warm-up, then event-bracketed repeats:

  (a) `mi_induced_pair_tensors`             once per geometry
  (b) `mi_induced_apply`                    per matrix-vector product (with and without the per-system partials)
  (c) the recompute path it replaces        `ewald_dipole_real_space(compute_dipole_gradients=True)` on the same list
  (d) the reciprocal-space call             per iteration
  (e) the whole solve to `--tolerance`      iterations and ms

    python tools/induced_bench.py [--atoms 100000] [--repeats 30] [--tolerance 1e-8]
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

from nvalchemiops.interactions.electrostatics import ewald_dipole_real_space, induced_dipoles  # noqa: E402
from nvalchemiops.interactions.electrostatics import induced as I  # noqa: E402
from nvalchemiops.neighborlist import cell_list  # noqa: E402


def median_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return round(float(np.median(times)), 4), round(float(np.min(times)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--cutoff", type=float, default=9.0)
    ap.add_argument("--max-neighbors", type=int, default=256)
    ap.add_argument("--alpha", type=float, default=0.35)
    ap.add_argument("--mesh", type=int, default=128)
    ap.add_argument("--order", type=int, default=5)
    ap.add_argument("--tolerance", type=float, default=1e-8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--solve-repeats", type=int, default=5)
    args = ap.parse_args()
    dev, dt = "cuda:0", torch.float64
    pos, cell, _, _ = S.fcc_box(args.atoms, dtype=np.float64)
    n = pos.shape[0]
    g = np.random.default_rng(0)
    P, Cl = torch.as_tensor(pos, device=dev, dtype=dt), torch.as_tensor(cell, device=dev, dtype=dt).reshape(1, 3, 3)
    q = g.normal(size=n)
    q = torch.as_tensor(q - q.mean(), device=dev, dtype=dt)
    nm, num, sh = cell_list(P, args.cutoff, Cl[0], torch.ones(3, dtype=torch.bool, device=dev), max_neighbors=args.max_neighbors)
    assert int(num.max()) <= args.max_neighbors, "rows overflow: raise --max-neighbors"
    row = nm[0, : int(num[0])].long()
    d_min = float(torch.linalg.norm(P[row] - P[0] + sh[0, : int(num[0])].to(dt) @ Cl[0], dim=-1).min())  # every site of the lattice is alike
    polar = torch.as_tensor(g.uniform(0.02, 0.08, n) * d_min**3, device=dev, dtype=dt)
    x3 = torch.as_tensor(g.normal(size=(n, 3)), device=dev, dtype=dt)
    alpha = torch.tensor([args.alpha], dtype=dt, device=dev)
    mesh = (args.mesh,) * 3
    lists = dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=n)
    op = I._Operator(P, polar, Cl, None, 1, (None, None, None, nm, sh), n, "pme", alpha, mesh, None, args.order, None, None, 1e-6)
    zero_q = torch.zeros(n, dtype=dt, device=dev)

    def product(with_partial):
        part = torch.empty((1, op.blocks), dtype=dt, device=dev) if with_partial else None
        return lambda: op.apply(x3, None, part)

    result = {"atoms": n, "cutoff": args.cutoff, "max_neighbors": args.max_neighbors, "slots": int(nm.numel()), "stored": int(num.sum()),
              "bytes_per_slot": 44, "d_min": d_min, "mesh": args.mesh, "order": args.order, "repeats": args.repeats, "ms": {}}

    def record(name, fn):
        med, best = median_ms(fn, args.warmup, args.repeats)
        result["ms"][name] = {"median": med, "min": best}
        print(f"{name:50s} median {med:.3f} ms   min {best:.3f} ms", flush=True)

    record("a mi_induced_pair_tensors", op.pair_tensors)
    record("b mi_induced_apply", product(False))
    record("b mi_induced_apply + per-system partials", product(True))
    record("c ewald_dipole_real_space dE/dmu", lambda: ewald_dipole_real_space(P, zero_q, x3, Cl, alpha, compute_dipole_gradients=True, **lists))
    record("d reciprocal call of one iteration", lambda: op.reciprocal_gradient(x3))
    solve = lambda: induced_dipoles(P, q, polar, Cl, alpha=alpha, mesh_dimensions=mesh, spline_order=args.order,  # noqa: E731
                                    tolerance=args.tolerance, return_info=True, **lists)
    out = solve()
    med, best = median_ms(solve, 1, args.solve_repeats)
    its = int(out.iterations[0])
    result["solve"] = {"tolerance": args.tolerance, "iterations": its, "residual": float(out.residual[0]), "median_ms": med, "min_ms": best,
                       "ms_per_iteration": round(med / max(its, 1), 4)}
    print(f"e solve to {args.tolerance:g}: {its} iterations, median {med:.2f} ms, min {best:.2f} ms ({med / max(its, 1):.3f} ms per iteration, "
          f"set-up included)", flush=True)
    print(f"operator streams {result['slots'] * 44 / 1e6:.1f} MB per product; x gathers: 24 bytes per slot out of a {n * 24 / 1e6:.1f} MB vector")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
