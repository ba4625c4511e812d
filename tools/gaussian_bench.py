"""Timing aid: `gaussian_charge_correction` (energies + forces) beside `ewald_real_space` on the same list, in the same process.

The list is the one of BASELINE config 4: 100 000-atom periodic FCC box, 9 A full list (padded M = 256), fp64; sigma = 0.5 A for every atom.
Warm-up, then the median of event-bracketed repeats; also the share of stored entries that pass the kernel's x = r / g_ij < 6 test.

    python tools/gaussian_bench.py [--atoms 100000] [--sigma 0.5] [--repeats 30] [--dtype f64]
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

from nvalchemiops.interactions.electrostatics import ewald_real_space, gaussian_charge_correction  # noqa: E402
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
    return float(np.median(times)), float(np.min(times))


def passing_share(pos, cell, nm, sh, sigma, n, rows=10000):
    """Share of the stored entries with r / sqrt(4 sigma^2) < 6 (uniform sigma), in row blocks."""
    stored = passing = 0
    for a in range(0, n, rows):
        j, s = nm[a:a + rows].long(), sh[a:a + rows].to(pos.dtype)
        ok = j < n
        r = pos[j.clamp(max=n - 1)] - pos[a:a + rows, None, :] + s @ cell.reshape(3, 3)
        x = torch.linalg.norm(r, dim=-1) / (2.0 * sigma)
        stored += int(ok.sum())
        passing += int((ok & (x < 6.0)).sum())
    return stored, passing


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--cutoff", type=float, default=9.0)
    ap.add_argument("--max-neighbors", type=int, default=256)
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--alpha", type=float, default=0.35)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f64")
    args = ap.parse_args()
    dev, dt = "cuda:0", (torch.float64 if args.dtype == "f64" else torch.float32)
    pos, cell, q, _ = S.fcc_box(args.atoms, dtype=np.float64)
    n = pos.shape[0]
    P, C, Q = (torch.as_tensor(a, device=dev, dtype=dt) for a in (pos, cell, q))
    C = C.reshape(1, 3, 3)
    pbc = torch.ones(3, dtype=torch.bool, device=dev)
    nm, num, sh = cell_list(P, args.cutoff, C[0], pbc, max_neighbors=args.max_neighbors)
    assert int(num.max()) <= args.max_neighbors, "rows overflow: raise --max-neighbors"
    sig = torch.full((n,), args.sigma, dtype=dt, device=dev)
    alpha = torch.tensor([args.alpha], dtype=dt, device=dev)
    lists = dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=n)
    cases = {
        "ewald_real_space E+F": lambda: ewald_real_space(P, Q, C, alpha, compute_forces=True, **lists),
        "gaussian_charge_correction E+F": lambda: gaussian_charge_correction(P, Q, sig, C, compute_forces=True, **lists),
        "gaussian_charge_correction E": lambda: gaussian_charge_correction(P, Q, sig, C, **lists),
        "gaussian_charge_correction E+F+dq+dsigma+virial": lambda: gaussian_charge_correction(
            P, Q, sig, C, compute_forces=True, compute_charge_gradients=True, compute_sigma_gradients=True, compute_virial=True, **lists),
    }
    result = {"atoms": n, "cutoff": args.cutoff, "max_neighbors": args.max_neighbors, "dtype": args.dtype, "sigma": args.sigma,
              "repeats": args.repeats, "ms": {}}
    for name, fn in cases.items():
        med, best = median_ms(fn, args.warmup, args.repeats)
        result["ms"][name] = {"median": round(med, 4), "min": round(best, 4)}
        print(f"{name:50s} median {med:.3f} ms   min {best:.3f} ms", flush=True)
    stored, passing = passing_share(P, C, nm, sh, args.sigma, n)
    result["entries"] = {"stored": stored, "slots": int(nm.numel()), "passing_x_lt_6": passing, "share": round(passing / max(stored, 1), 4)}
    print(f"stored entries {stored} of {nm.numel()} slots; passing x < 6: {passing} ({100.0 * passing / max(stored, 1):.1f} %)")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
