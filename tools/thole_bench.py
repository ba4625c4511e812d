"""Timing aid: the Thole correction and the damped induced-dipole set-up on the list of BASELINE config 4, in one process.

100 000-atom periodic FCC box, 9 A full list (padded M = 256), fp64, random charges (neutral), random dipoles, polarisabilities uniform in
[0.02, 0.08] d_min^3 (the set of tools/induced_bench.py) and, as a second set, those times `--large` (default 8: beyond the polarisation
catastrophe of undamped dipoles on this lattice).  Warm-up, then event-bracketed repeats:

  (a) `thole_dipole_correction` against `ewald_dipole_real_space` on the same list      energies only, and with forces + dipole gradients
  (b) `mi_thole_induced_pair_tensors` against `mi_induced_pair_tensors`                 once per geometry
  (c) `thole_induced_dipoles` against `induced_dipoles`                                 iterations and ms, both polarisability sets

The tables of DESIGN.md section 3.23 are the `--markdown` output of this tool.

    python tools/thole_bench.py [--atoms 100000] [--repeats 30] [--tolerance 1e-8] [--markdown]
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

from nvalchemiops.interactions.electrostatics import (InducedDipoleError, ewald_dipole_real_space, induced_dipoles,  # noqa: E402
                                                      thole_dipole_correction, thole_induced_dipoles)
from nvalchemiops.interactions.electrostatics import induced as I  # noqa: E402
from nvalchemiops.neighborlist import cell_list  # noqa: E402
from tools.induced_bench import median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--cutoff", type=float, default=9.0)
    ap.add_argument("--max-neighbors", type=int, default=256)
    ap.add_argument("--alpha", type=float, default=0.35)
    ap.add_argument("--mesh", type=int, default=128)
    ap.add_argument("--order", type=int, default=5)
    ap.add_argument("--thole", type=float, default=0.39)
    ap.add_argument("--large", type=float, default=8.0)
    ap.add_argument("--tolerance", type=float, default=1e-8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--solve-repeats", type=int, default=3)
    ap.add_argument("--markdown", action="store_true")
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
    mu = torch.as_tensor(0.3 * g.normal(size=(n, 3)), device=dev, dtype=dt)
    alpha = torch.tensor([args.alpha], dtype=dt, device=dev)
    mesh = (args.mesh,) * 3
    lists = dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=n)
    result = {"atoms": n, "cutoff": args.cutoff, "max_neighbors": args.max_neighbors, "slots": int(nm.numel()), "stored": int(num.sum()),
              "d_min": d_min, "thole": args.thole, "large": args.large, "repeats": args.repeats, "ms": {}, "solves": {}}
    # the share of the stored entries that pass the E < 50 exit, per polarisability set
    valid = nm < n
    j = torch.where(valid, nm, torch.zeros_like(nm)).long()
    r = torch.linalg.norm(P[j] - P.unsqueeze(1) + torch.einsum("nma,ab->nmb", sh.to(dt), Cl[0]), dim=-1)
    sets = {"standard": polar, f"x{args.large:g}": polar * args.large}
    for name, a in sets.items():
        big = args.thole * r**3 / torch.sqrt(a.unsqueeze(1) * a[j])
        result[f"active_share_{name}"] = round(float(((big < 50.0) & valid).sum()) / float(valid.sum()), 4)
    del j, r, valid

    def record(name, fn):
        med, best = median_ms(fn, args.warmup, args.repeats)
        result["ms"][name] = {"median": med, "min": best}
        print(f"{name:64s} median {med:.3f} ms   min {best:.3f} ms", flush=True)

    grads = dict(compute_forces=True, compute_dipole_gradients=True)
    record("a ewald_dipole_real_space, energies", lambda: ewald_dipole_real_space(P, q, mu, Cl, alpha, **lists))
    record("a ewald_dipole_real_space, forces + dipole gradients", lambda: ewald_dipole_real_space(P, q, mu, Cl, alpha, **grads, **lists))
    for name, a in sets.items():
        record(f"a thole_dipole_correction ({name}), energies", lambda a=a: thole_dipole_correction(P, q, mu, a, Cl, thole=args.thole, **lists))
        record(f"a thole_dipole_correction ({name}), forces + dipole gradients",
               lambda a=a: thole_dipole_correction(P, q, mu, a, Cl, thole=args.thole, **grads, **lists))
    for name, a in sets.items():
        for thole in (None, args.thole):
            op = I._Operator(P, a, Cl, None, 1, (None, None, None, nm, sh), n, "pme", alpha, mesh, None, args.order, None, None, 1e-6, thole)
            record(f"b {'mi_thole_induced_pair_tensors' if thole else 'mi_induced_pair_tensors'} ({name})", op.pair_tensors)
            del op
    for name, a in sets.items():
        for thole in (None, args.thole):
            common = dict(alpha=alpha, mesh_dimensions=mesh, spline_order=args.order, tolerance=args.tolerance, return_info=True, **lists)
            solve = ((lambda a=a: induced_dipoles(P, q, a, Cl, **common)) if thole is None
                     else (lambda a=a, thole=thole: thole_induced_dipoles(P, q, a, Cl, thole=thole, **common)))
            key = f"{name}, {'thole ' + format(args.thole, 'g') if thole else 'undamped'}"
            try:
                out = solve()
            except InducedDipoleError as err:
                result["solves"][key] = {"error": "not positive definite" if "not positive definite" in str(err) else "no convergence"}
                print(f"c solve ({key}): {result['solves'][key]['error']}", flush=True)
                continue
            med, best = median_ms(solve, 1, args.solve_repeats)
            its = int(out.iterations[0])
            result["solves"][key] = {"iterations": its, "residual": float(out.residual[0]), "median_ms": med, "min_ms": best}
            print(f"c solve ({key}) to {args.tolerance:g}: {its} iterations, median {med:.2f} ms, min {best:.2f} ms", flush=True)
    print(json.dumps(result))
    if args.markdown:
        print("\n| pass | median ms | min ms |\n|---|---|---|")
        for name, v in result["ms"].items():
            print(f"| {name[2:]} | {v['median']:.3f} | {v['min']:.3f} |")
        print("\n| solve to %g | iterations | median ms |\n|---|---|---|" % args.tolerance)
        for name, v in result["solves"].items():
            print(f"| {name} | {v.get('iterations', v.get('error'))} | {v.get('median_ms', '-')} |")


if __name__ == "__main__":
    main()
