"""Timing aid: the mesh half of the dispersion lattice sum (`pme_dispersion_reciprocal_space`) against the explicit reciprocal sum
(`ewald_dispersion_reciprocal_space`) at matched accuracy, in the same process.

Periodic FCC box (100 000 atoms by default), energies + forces.  The forces of an explicit sum to `--k-ref` are the reference; every
`--k-cutoffs` value and every `--meshes` value (cubic meshes, `--order`) is given its relative force error against it (largest |difference|
over largest |force|) and the median of event-bracketed repeats after a warm-up.  "Matched" is the cheapest setting of either kind whose
error is within `--target`.  Run it in three fresh processes and take the median of the medians; run it at several `--atoms` for the
crossover.

    python tools/dispersion_pme_bench.py [--atoms 100000] [--alpha 0.35] [--k-ref 2.2] [--k-cutoffs 0.8,1.0,1.2,1.4] [--meshes 72,96,120,144]
                                         [--order 5] [--target 1e-3] [--repeats 20] [--dtype f64]
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
from tools.dispersion_ewald_bench import median_ms  # noqa: E402

from nvalchemiops.interactions import ewald_dispersion_reciprocal_space, pme_dispersion_reciprocal_space  # noqa: E402
from nvalchemiops.interactions.electrostatics.k_vectors import generate_k_vectors_ewald_summation  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--alpha", type=float, default=0.35)
    ap.add_argument("--k-ref", type=float, default=2.2)
    ap.add_argument("--k-cutoffs", default="0.8,1.0,1.2,1.4")
    ap.add_argument("--meshes", default="72,96,120,144")
    ap.add_argument("--order", type=int, default=5)
    ap.add_argument("--target", type=float, default=1e-3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f64")
    args = ap.parse_args()
    dev, dt = "cuda:0", (torch.float64 if args.dtype == "f64" else torch.float32)
    pos, cell, _, _ = S.fcc_box(args.atoms, dtype=np.float64)
    n = pos.shape[0]
    P, C = (torch.as_tensor(a, device=dev, dtype=dt) for a in (pos, cell))
    C = C.reshape(1, 3, 3)
    c = 2.0 + 3.0 * torch.rand(n, generator=torch.Generator(device=dev).manual_seed(1), device=dev, dtype=dt)
    k_of = lambda kc: generate_k_vectors_ewald_summation(C[0], kc).reshape(-1, 3)  # noqa: E731
    ref = ewald_dispersion_reciprocal_space(P, c, C, k_of(args.k_ref), args.alpha, compute_forces=True)[1].double()
    scale = float(ref.abs().max())
    result = {"atoms": n, "box": float(cell[0, 0]), "alpha": args.alpha, "dtype": args.dtype, "order": args.order, "k_ref": args.k_ref,
              "target": args.target, "repeats": args.repeats, "explicit": [], "mesh": []}
    for kc in (float(v) for v in args.k_cutoffs.split(",")):
        kv = k_of(kc)
        call = lambda: ewald_dispersion_reciprocal_space(P, c, C, kv, args.alpha, compute_forces=True)  # noqa: E731
        err = float((call()[1].double() - ref).abs().max()) / scale
        med, best = median_ms(call, args.warmup, args.repeats)
        result["explicit"].append({"k_cutoff": kc, "k_vectors": int(kv.shape[0]), "force_error": err, "median_ms": round(med, 4), "min_ms": round(best, 4)})
        print(f"explicit k_cutoff {kc:5.2f} ({kv.shape[0]:7d} k)  force error {err:.2e}  median {med:.3f} ms  min {best:.3f} ms", flush=True)
    for m in (int(v) for v in args.meshes.split(",")):
        call = lambda: pme_dispersion_reciprocal_space(P, c, C, args.alpha, mesh_dimensions=(m, m, m), spline_order=args.order,  # noqa: E731
                                                       compute_forces=True)
        err = float((call()[1].double() - ref).abs().max()) / scale
        med, best = median_ms(call, args.warmup, args.repeats)
        result["mesh"].append({"mesh": m, "force_error": err, "median_ms": round(med, 4), "min_ms": round(best, 4)})
        print(f"mesh {m:4d}^3 order {args.order}            force error {err:.2e}  median {med:.3f} ms  min {best:.3f} ms", flush=True)
    for kind in ("explicit", "mesh"):
        ok = [r for r in result[kind] if r["force_error"] <= args.target]
        result[f"matched {kind}"] = min(ok, key=lambda r: r["median_ms"]) if ok else None
    print(json.dumps(result))


if __name__ == "__main__":
    main()
