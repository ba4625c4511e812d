"""Timing aid: `buffered_14_7` and `lennard_jones` beside the plain-torch expression over the same neighbour matrix, in the same process.

100 000-atom periodic FCC box, 12 A full list (padded M = 640), with and without reduced sites (two of three atoms take a listed neighbour as
parent, kappa = 0.9).  Warm-up, then the median of event-bracketed repeats.  The torch expression is evaluated in row blocks (energies only:
its [N, M, 3] temporaries do not fit otherwise).

    python tools/vdw_bench.py [--atoms 100000] [--cutoff 12] [--repeats 20] [--dtype f64]
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
from tests import vdw_reference as R  # noqa: E402

from nvalchemiops.interactions import ReducedSites, buffered_14_7, lennard_jones  # noqa: E402
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


def torch_energies(kind, pos, radii, eps, cell, nm, sh, cutoff, taper, sites, rules, rows=4000):
    """The definition in plain torch over the matrix, row block by row block: per-atom energies."""
    n = pos.shape[0]
    site = R.site_positions(pos, cell, torch.zeros(n, dtype=torch.long, device=pos.device), sites)
    out = torch.empty(n, dtype=pos.dtype, device=pos.device)
    for a in range(0, n, rows):
        j = nm[a:a + rows].long()
        ok = j < n
        j = j.clamp(max=n - 1)
        d = site[j] - site[a:a + rows, None, :] + sh[a:a + rows].to(pos.dtype) @ cell[0]
        r = torch.linalg.norm(d, dim=-1)
        i = torch.arange(a, min(a + rows, n), device=pos.device)[:, None].expand_as(j)
        Rij, eij = R.combine(radii, eps, i, j, *rules)
        keep = ok & (r < cutoff) & (r > 1e-8)
        rs = torch.where(keep, r, torch.ones_like(r))
        out[a:a + rows] = 0.5 * torch.where(keep, eij * R.switch(rs, cutoff, taper) * R.potential(kind, rs / Rij), torch.zeros_like(r)).sum(-1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--cutoff", type=float, default=12.0)
    ap.add_argument("--max-neighbors", type=int, default=640)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f64")
    args = ap.parse_args()
    dev, dt = "cuda:0", (torch.float64 if args.dtype == "f64" else torch.float32)
    pos, cell, _, _ = S.fcc_box(args.atoms, dtype=np.float64)
    n = pos.shape[0]
    P, C = (torch.as_tensor(a, device=dev, dtype=dt) for a in (pos, cell))
    C = C.reshape(1, 3, 3)
    nm, num, sh = cell_list(P, args.cutoff, C[0], torch.ones(3, dtype=torch.bool, device=dev), max_neighbors=args.max_neighbors)
    assert int(num.max()) <= args.max_neighbors, "rows overflow: raise --max-neighbors"
    g = torch.Generator(device=dev).manual_seed(1)
    radii = 3.2 + 0.6 * torch.rand(n, generator=g, device=dev, dtype=dt)
    eps = 0.05 + 0.2 * torch.rand(n, generator=g, device=dev, dtype=dt)
    # two of three atoms are reduced onto their first listed neighbour whose index is a multiple of 3 (those atoms stay their own sites)
    own = torch.arange(n, device=dev)
    heavy = (nm < n) & (nm % 3 == 0)
    first = nm.gather(1, heavy.int().argmax(1, keepdim=True))[:, 0].long()
    parent = torch.where((own % 3 != 0) & heavy.any(1), first, torch.full_like(own, -1))
    sites = ReducedSites(parent, torch.full((n,), 0.9, dtype=dt, device=dev))
    taper = 0.9 * args.cutoff
    lists = dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=n, cutoff=args.cutoff, taper=taper)
    result = {"atoms": n, "cutoff": args.cutoff, "max_neighbors": args.max_neighbors, "dtype": args.dtype, "stored_entries": int(num.sum()),
              "repeats": args.repeats, "ms": {}}
    for kind, fn, rules in (("buffered_14_7", buffered_14_7, ("cubic-mean", "hhg")), ("lennard_jones", lennard_jones, ("arithmetic", "geometric"))):
        for label, st in (("atoms", None), ("sites", sites)):
            table = None if st is None else (st.parent, st.reduction)
            cases = {
                f"{kind} {label} E": lambda: fn(P, radii, eps, C, sites=st, **lists),
                f"{kind} {label} E+F": lambda: fn(P, radii, eps, C, sites=st, compute_forces=True, **lists),
                f"{kind} {label} E+F+dR+deps+virial": lambda: fn(P, radii, eps, C, sites=st, compute_forces=True, compute_radius_gradients=True,
                                                                  compute_epsilon_gradients=True, compute_virial=True, **lists),
                f"{kind} {label} torch E": lambda: torch_energies(kind, P, radii, eps, C, nm, sh, args.cutoff, taper, table, rules),
            }
            for name, call in cases.items():
                med, best = median_ms(call, args.warmup, 3 if "torch" in name else args.repeats)
                result["ms"][name] = {"median": round(med, 4), "min": round(best, 4)}
                print(f"{name:50s} median {med:.3f} ms   min {best:.3f} ms", flush=True)
            want = torch_energies(kind, P, radii, eps, C, nm, sh, args.cutoff, taper, table, rules)
            err = float((fn(P, radii, eps, C, sites=st, **lists) - want).abs().max() / want.abs().max())
            print(f"{kind} {label}: max |E_i - torch| / max |E_i| = {err:.2e}", flush=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
