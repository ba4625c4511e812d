"""Cost of the electrostatic virial on the config-4 box (100 000 atoms, fp64, rc 9 A, M = 256, alpha 0.35, mesh 128^3, order 5):
`particle_mesh_ewald(compute_forces=True)` against `particle_mesh_ewald_with_virial(compute_forces=True)` and against the autograd strain route
(forward under grad with an explicit strain variable + backward).  Event-bracketed medians, the variants alternated inside one process.
Usage: python tools/virial_bench.py [--reps 30] [--warmup 5]   -> one JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "nvalchemi-toolkit-ops_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from nvalchemiops.interactions.electrostatics import particle_mesh_ewald, particle_mesh_ewald_with_virial
    from nvalchemiops.neighborlist import neighbor_list
    from tests import systems as S

    dev = "cuda:0"
    pos, cell, q, _ = S.fcc_box(100000, seed=1234, dtype=np.float64)
    P, Cc, Q = (torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in (pos, cell, q))
    nm, num, sh = neighbor_list(P, 9.0, cell=Cc, pbc=torch.tensor([True] * 3, device=dev), method="cell_list", max_neighbors=256)
    kw = dict(alpha=0.35, mesh_dimensions=(128, 128, 128), spline_order=5, neighbor_matrix=nm, neighbor_matrix_shifts=sh, compute_forces=True)

    def plain():
        return particle_mesh_ewald(P, Q, Cc, **kw)

    def with_virial():
        return particle_mesh_ewald_with_virial(P, Q, Cc, **kw)

    def strain_autograd():
        eps = torch.zeros((3, 3), dtype=P.dtype, device=dev, requires_grad=True)
        f = torch.eye(3, dtype=P.dtype, device=dev) + eps
        e, frc = particle_mesh_ewald(P @ f.T, Q, Cc @ f.T, **kw)
        return frc, -torch.autograd.grad(e.sum(), eps)[0]

    variants = {"pme": plain, "pme_with_virial": with_virial, "strain_autograd": strain_autograd}
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.reps):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b))
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"box": "config4", "reps": args.reps, "median_ms": {k: round(v, 4) for k, v in med.items()},
           "with_virial_over_pme": round(med["pme_with_virial"] / med["pme"], 4),
           "strain_autograd_over_with_virial": round(med["strain_autograd"] / med["pme_with_virial"], 3),
           "spread_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
