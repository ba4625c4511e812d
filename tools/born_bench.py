"""Timing aid: `generalized_born` beside the plain-torch expression of the same sum over the same padded neighbour matrix, in one process.

100 000 atoms of the jittered FCC box taken as a cluster (no cell, no shifts), 16 A full list, fp64; radii 1.5 A, screening 0.8.  Warm-up,
then the median of event-bracketed repeats, with and without forces (the torch forces come from autograd).  The torch expression holds
tens of [N, M] float64 temporaries: lower --atoms if the device runs out of memory.

    python tools/born_bench.py [--atoms 100000] [--cutoff 16] [--repeats 20] [--dtype f64] [--skip-torch]
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

from nvalchemiops.interactions.electrostatics import generalized_born  # noqa: E402
from nvalchemiops.neighborlist import neighbor_list  # noqa: E402

OFFSET, OBC, TAU = 0.09, (1.0, 0.8, 4.85), 1.0 - 1.0 / 78.5


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


def torch_born(pos, q, rad, scr, nm, forces):
    """The definition with torch ops over the padded matrix: per-atom energies, and forces by autograd."""
    n = pos.shape[0]
    pos = pos.detach().requires_grad_(forces)
    ok = nm < n
    j = nm.clamp(max=n - 1).long()
    d = pos[j] - pos[:, None, :]
    r = torch.where(ok, d.norm(dim=-1), torch.ones_like(d[..., 0]))
    rho = rad - OFFSET
    ri, sj = rho[:, None], (scr * rho)[j]
    U, L = r + sj, torch.maximum(ri, (r - sj).abs())
    val = 0.5 * (1 / L - 1 / U + 0.25 * r * (1 / U**2 - 1 / L**2) + torch.log(L / U) / (2 * r) + sj * sj / (4 * r) * (1 / L**2 - 1 / U**2))
    val = val + torch.where(ri < sj - r, 1 / ri - 1 / L, torch.zeros_like(val))
    psi = rho * torch.where(ok & (U > ri), val, torch.zeros_like(val)).sum(1)
    born = 1 / (1 / rho - torch.tanh(OBC[0] * psi - OBC[1] * psi**2 + OBC[2] * psi**3) / rad)
    bb = born[:, None] * born[j]
    pair = torch.where(ok, q[:, None] * q[j] / torch.sqrt(r * r + bb * torch.exp(-r * r / (4 * bb))), torch.zeros_like(r))
    e = -0.5 * TAU * (q * q / born + pair.sum(1))
    return (e, -torch.autograd.grad(e.sum(), pos)[0]) if forces else e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--cutoff", type=float, default=16.0)
    ap.add_argument("--max-neighbors", type=int, default=1280)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f64")
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    dev, dt = "cuda:0", (torch.float64 if args.dtype == "f64" else torch.float32)
    pos, cell, q, _ = S.fcc_box(args.atoms, dtype=np.float64)
    n = pos.shape[0]
    P, C, Q = (torch.as_tensor(a, device=dev, dtype=dt) for a in (pos, cell, q))
    nm, num, _ = neighbor_list(P, args.cutoff, cell=C.reshape(1, 3, 3), pbc=torch.zeros((1, 3), dtype=torch.bool, device=dev), method="cell_list",
                               max_neighbors=args.max_neighbors)
    assert int(num.max()) <= args.max_neighbors, "rows overflow: raise --max-neighbors"
    rad, scr = torch.full((n,), 1.5, dtype=dt, device=dev), torch.full((n,), 0.8, dtype=dt, device=dev)
    kw = dict(neighbor_matrix=nm, mask_value=n, offset=OFFSET, obc=OBC)
    cases = {"generalized_born E": lambda: generalized_born(P, Q, rad, scr, **kw),
             "generalized_born E+F": lambda: generalized_born(P, Q, rad, scr, compute_forces=True, **kw)}
    if not args.skip_torch:
        cases.update({"torch E": lambda: torch_born(P, Q, rad, scr, nm, False), "torch E+F": lambda: torch_born(P, Q, rad, scr, nm, True)})
        e, f = cases["generalized_born E+F"]()
        te, tf = (t.detach() for t in cases["torch E+F"]())
        print(f"max |E - E_torch| / max |E| = {float((e - te).abs().max() / te.abs().max()):.2e}, forces {float((f - tf).abs().max() / tf.abs().max()):.2e}")
    result = {"atoms": n, "cutoff": args.cutoff, "row_width": int(nm.shape[1]), "mean_neighbors": round(float(num.double().mean()), 1),
              "dtype": args.dtype, "repeats": args.repeats, "ms": {}}
    for name, fn in cases.items():
        med, best = median_ms(fn, args.warmup, args.repeats)
        result["ms"][name] = {"median": round(med, 4), "min": round(best, 4)}
        print(f"{name:24s} median {med:.3f} ms   min {best:.3f} ms", flush=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
