"""Timing aid: both halves of `ewald_dispersion_correction` beside the point-dipole Ewald halves and beside the plain-torch expression over
the same list and k-vectors, in the same process.

100 000-atom periodic FCC box, 9 A full list, half-space k set to `--k-cutoff`.  Warm-up, then the median of event-bracketed repeats.  The
torch expressions are evaluated in blocks (energies only: their [N, M, 3] and [N, K] temporaries do not fit otherwise).  Run it in three
fresh processes and take the median of the medians.

    python tools/dispersion_ewald_bench.py [--atoms 100000] [--cutoff 9] [--k-cutoff 0.6] [--repeats 20] [--dtype f64]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nvalchemi-toolkit-ops_amd")]
from tests import dispersion_ewald_reference as R  # noqa: E402
from tests import systems as S  # noqa: E402

from nvalchemiops.interactions import ewald_dispersion_real_space, ewald_dispersion_reciprocal_space  # noqa: E402
from nvalchemiops.interactions.electrostatics import ewald_dipole_real_space, ewald_dipole_reciprocal_space  # noqa: E402
from nvalchemiops.interactions.electrostatics.k_vectors import generate_k_vectors_ewald_summation  # noqa: E402
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


def torch_real(pos, c, cell, alpha, nm, sh, rows=4000):
    """The real-space definition in plain torch over the matrix, row block by row block: per-atom energies."""
    n = pos.shape[0]
    out = torch.empty(n, dtype=pos.dtype, device=pos.device)
    for a in range(0, n, rows):
        j = nm[a:a + rows].long()
        ok = j < n
        j = j.clamp(max=n - 1)
        d = pos[j] - pos[a:a + rows, None, :] + sh[a:a + rows].to(pos.dtype) @ cell[0]
        r2 = (d * d).sum(-1)
        keep = ok & (r2 > 1e-16)
        r2 = torch.where(keep, r2, torch.ones_like(r2))
        a2 = alpha * alpha * r2
        g = torch.exp(-a2) * (1.0 + a2 + 0.5 * a2 * a2)
        out[a:a + rows] = -0.5 * c[a:a + rows] * torch.where(keep, c[j] * g / r2 ** 3, torch.zeros_like(r2)).sum(-1)
    return out


def torch_recip(pos, c, cell, kv, alpha, block=64):
    """The reciprocal-space definition in plain torch, k block by k block: per-atom energies."""
    vol = torch.linalg.det(cell[0]).abs()
    pref = np.pi ** 1.5 * alpha ** 3 / (3.0 * vol)
    e = -0.5 * pref * c * c.sum() + alpha ** 6 / 12.0 * c * c
    for a in range(0, kv.shape[0], block):
        k = kv[a:a + block]
        w = R.f_of_b(k.norm(dim=-1) / (2.0 * alpha))
        phase = pos @ k.T
        cs, sn = c[:, None] * torch.cos(phase), c[:, None] * torch.sin(phase)
        e = e - pref * ((cs * cs.sum(0) + sn * sn.sum(0)) * w).sum(-1)
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--cutoff", type=float, default=9.0)
    ap.add_argument("--k-cutoff", type=float, default=0.6)
    ap.add_argument("--alpha", type=float, default=0.35)
    ap.add_argument("--max-neighbors", type=int, default=288)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f64")
    args = ap.parse_args()
    dev, dt = "cuda:0", (torch.float64 if args.dtype == "f64" else torch.float32)
    pos, cell, q, _ = S.fcc_box(args.atoms, dtype=np.float64)
    n = pos.shape[0]
    P, C, Q = (torch.as_tensor(a, device=dev, dtype=dt) for a in (pos, cell, q))
    C = C.reshape(1, 3, 3)
    nm, num, sh = cell_list(P, args.cutoff, C[0], torch.ones(3, dtype=torch.bool, device=dev), max_neighbors=args.max_neighbors)
    assert int(num.max()) <= args.max_neighbors, "rows overflow: raise --max-neighbors"
    g = torch.Generator(device=dev).manual_seed(1)
    c = 2.0 + 3.0 * torch.rand(n, generator=g, device=dev, dtype=dt)
    mu = 0.1 * torch.randn(n, 3, generator=g, device=dev, dtype=dt)
    kv = generate_k_vectors_ewald_summation(C[0], args.k_cutoff).reshape(-1, 3)
    lists = dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=n)
    every = dict(compute_forces=True, compute_coefficient_gradients=True, compute_virial=True)
    dp_every = dict(compute_forces=True, compute_charge_gradients=True, compute_dipole_gradients=True, compute_virial=True)
    taper = dict(counted_cutoff=args.cutoff, counted_taper=0.9 * args.cutoff)
    result = {"atoms": n, "cutoff": args.cutoff, "k_cutoff": args.k_cutoff, "k_vectors": int(kv.shape[0]), "alpha": args.alpha, "dtype": args.dtype,
              "stored_entries": int(num.sum()), "repeats": args.repeats, "ms": {}}
    cases = {
        "dispersion real E": lambda: ewald_dispersion_real_space(P, c, C, args.alpha, **lists),
        "dispersion real E+F": lambda: ewald_dispersion_real_space(P, c, C, args.alpha, compute_forces=True, **lists),
        "dispersion real E+F+dc+virial": lambda: ewald_dispersion_real_space(P, c, C, args.alpha, **every, **lists),
        "dispersion real counted E+F+dc+virial": lambda: ewald_dispersion_real_space(P, c, C, args.alpha, **every, **taper, **lists),
        "dipole real E+F+dq+dmu+virial": lambda: ewald_dipole_real_space(P, Q, mu, C, args.alpha, **dp_every, **lists),
        "torch real E": lambda: torch_real(P, c, C, args.alpha, nm, sh),
        "dispersion reciprocal E": lambda: ewald_dispersion_reciprocal_space(P, c, C, kv, args.alpha),
        "dispersion reciprocal E+F": lambda: ewald_dispersion_reciprocal_space(P, c, C, kv, args.alpha, compute_forces=True),
        "dispersion reciprocal E+F+dc+virial": lambda: ewald_dispersion_reciprocal_space(P, c, C, kv, args.alpha, **every),
        "dipole reciprocal E+F+dq+dmu+virial": lambda: ewald_dipole_reciprocal_space(P, Q, mu, C, kv, args.alpha, **dp_every),
        "torch reciprocal E": lambda: torch_recip(P, c, C, kv, args.alpha),
    }
    for name, call in cases.items():
        med, best = median_ms(call, args.warmup, 3 if "torch" in name else args.repeats)
        result["ms"][name] = {"median": round(med, 4), "min": round(best, 4)}
        print(f"{name:45s} median {med:.3f} ms   min {best:.3f} ms", flush=True)
    for half, got, want in (("real", cases["dispersion real E"](), cases["torch real E"]()),
                            ("reciprocal", cases["dispersion reciprocal E"](), cases["torch reciprocal E"]())):
        err = float((got - want).abs().max() / want.abs().max())
        result[f"{half} max |E_i - torch| / max |E_i|"] = err
        print(f"{half}: max |E_i - torch| / max |E_i| = {err:.2e}", flush=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
