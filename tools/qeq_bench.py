"""Timing aid: `charge_equilibration` and its pieces on the list of BASELINE config 4, in one process.

100 000-atom periodic FCC box, 9 A full list (padded M = 256), fp64, sigma = 0.5 A for every atom, random electronegativities and
hardnesses; PME as the headline benchmark runs it (alpha 0.35 / A, mesh 128^3, order 5).  Warm-up, then event-bracketed repeats:

  (a) `mi_qeq_pair_coefficients`            once per geometry
  (b) `mi_qeq_apply`                        per matrix-vector product (with and without the per-system partials)
  (c) the recompute path it replaces        the three public charge-gradient calls per product
  (d) the reciprocal-space call             per iteration
  (e) the whole solve to `--tolerance`      iterations and ms

    python tools/qeq_bench.py [--atoms 100000] [--repeats 30] [--tolerance 1e-8]
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

from nvalchemiops import _capi as C  # noqa: E402
from nvalchemiops.interactions.electrostatics import (charge_equilibration, ewald_real_space, gaussian_charge_correction,  # noqa: E402
                                                      pme_reciprocal_space)
from nvalchemiops.interactions.electrostatics import qeq as Q  # noqa: E402
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
    ap.add_argument("--sigma", type=float, default=0.5)
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
    chi = torch.as_tensor(g.normal(size=n), device=dev, dtype=dt)
    hard = torch.as_tensor(g.uniform(1.0, 2.0, n), device=dev, dtype=dt)
    x = torch.as_tensor(g.normal(size=n), device=dev, dtype=dt)
    x -= x.mean()
    nm, num, sh = cell_list(P, args.cutoff, Cl[0], torch.ones(3, dtype=torch.bool, device=dev), max_neighbors=args.max_neighbors)
    assert int(num.max()) <= args.max_neighbors, "rows overflow: raise --max-neighbors"
    sig = torch.full((n,), args.sigma, dtype=dt, device=dev)
    alpha = torch.tensor([args.alpha], dtype=dt, device=dev)
    mesh = (args.mesh,) * 3
    lists = dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=n)
    op = Q._Operator(P, hard, sig, Cl, None, 1, (None, None, None, nm, sh), n, "pme", alpha, mesh, None, args.order, None, None, 1e-6)
    L = C.lib()
    part = torch.empty((1, op.blocks, 2), dtype=dt, device=dev)
    y = torch.empty(n, dtype=dt, device=dev)
    shi = C.i32(sh)

    def coefficients():
        C.check(L.mi_qeq_pair_coefficients(C.ptr(op.pos), C.ptr(op.sigma), C.ptr(hard), C.ptr(op.cells), C.ptr(op.alpha), None, n, 1, C.MI_F64,
                                           C.ptr(op.idx), C.ptr(shi), None, op.m, n, C.ptr(op.coef), C.ptr(op.nbr), C.ptr(op.diag), C.stream_of(P)),
                "mi_qeq_pair_coefficients")

    def product(with_partial):
        C.check(L.mi_qeq_apply(C.ptr(op.coef), C.ptr(op.nbr), C.ptr(op.diag), C.ptr(x), None, None, n, 1, None, op.m, C.ptr(y),
                               C.ptr(part) if with_partial else None, C.stream_of(x)), "mi_qeq_apply")

    cases = {
        "a mi_qeq_pair_coefficients": coefficients,
        "b mi_qeq_apply": lambda: product(False),
        "b mi_qeq_apply + per-system partials": lambda: product(True),
        "c ewald_real_space dE/dq": lambda: ewald_real_space(P, x, Cl, alpha, compute_charge_gradients=True, **lists),
        "c gaussian_charge_correction dE/dq": lambda: gaussian_charge_correction(P, x, sig, Cl, compute_charge_gradients=True, **lists),
        "c pme_reciprocal_space dE/dq": lambda: pme_reciprocal_space(P, x, Cl, alpha, mesh_dimensions=mesh, spline_order=args.order,
                                                                    compute_charge_gradients=True),
        "d reciprocal call of one iteration": lambda: op.reciprocal_gradient(x),
    }
    result = {"atoms": n, "cutoff": args.cutoff, "max_neighbors": args.max_neighbors, "slots": int(nm.numel()), "stored": int(num.sum()),
              "bytes_per_slot": 12, "mesh": args.mesh, "order": args.order, "repeats": args.repeats, "ms": {}}
    for name, fn in cases.items():
        med, best = median_ms(fn, args.warmup, args.repeats)
        result["ms"][name] = {"median": med, "min": best}
        print(f"{name:45s} median {med:.3f} ms   min {best:.3f} ms", flush=True)
    solve = lambda: charge_equilibration(P, chi, hard, sig, Cl, alpha=alpha, mesh_dimensions=mesh, spline_order=args.order,  # noqa: E731
                                         tolerance=args.tolerance, return_info=True, **lists)
    out = solve()
    med, best = median_ms(solve, 1, args.solve_repeats)
    its = int(out.iterations[0])
    result["solve"] = {"tolerance": args.tolerance, "iterations": its, "residual": float(out.residual[0]), "median_ms": med, "min_ms": best,
                       "ms_per_iteration": round(med / max(its, 1), 4)}
    print(f"e solve to {args.tolerance:g}: {its} iterations, median {med:.2f} ms, min {best:.2f} ms ({med / max(its, 1):.3f} ms per iteration, "
          f"set-up and final product included)")
    stream = result["slots"] * 12 / 1e6
    print(f"coefficient + index stream {stream:.1f} MB per product; x gathers: one 8-byte word per slot out of a {n * 8 / 1e6:.1f} MB vector")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
