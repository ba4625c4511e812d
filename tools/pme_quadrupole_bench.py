"""Timing aid: the quadrupole mesh sum beside the dipole mesh sum, whose two-mesh solve it shares, and the explicit reciprocal sum it replaces
at size, in one process on the same inputs.  After tools/pme_dipole_bench.py.

The box of BASELINE config 4 (100 000-atom periodic FCC box), spline order 5, alpha and mesh as `particle_mesh_ewald` estimates them at its
default accuracy.  Timed: `pme_dipole_reciprocal_space` (energies + forces), `pme_quadrupole_reciprocal_space` (energies; energies + forces;
everything) and `ewald_quadrupole_reciprocal_space` at the K = 1 098 of tools/dipole_bench.py and at the k-cutoff
`estimate_ewald_parameters` gives for the same accuracy.  Warm-up, then median and minimum of event-bracketed repeats of the whole public
call.  An explicit sum whose single call does not fit --limit seconds is reported as such and retried with the k-cutoff scaled down by 0.8
until one fits; its repeats are cut to fit the limit as well (the count used is in the output).

    python tools/pme_quadrupole_bench.py [--atoms 100000] [--order 5] [--repeats 30] [--dtype f64] [--limit 60]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nvalchemi-toolkit-ops_amd")]
from tests import systems as S  # noqa: E402

from nvalchemiops.interactions.electrostatics import (ewald_quadrupole_reciprocal_space, generate_k_vectors_ewald_summation,  # noqa: E402
                                                      pme_dipole_reciprocal_space, pme_quadrupole_reciprocal_space)
from nvalchemiops.interactions.electrostatics.parameters import estimate_ewald_parameters, estimate_pme_parameters  # noqa: E402
from tools.gaussian_bench import median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--order", type=int, default=5)
    ap.add_argument("--k-index", type=int, default=6, help="largest Miller index per axis of the small explicit k set")
    ap.add_argument("--accuracy", type=float, default=1e-6)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--limit", type=float, default=60.0, help="seconds one explicit-sum case may take in all")
    ap.add_argument("--dtype", choices=["f32", "f64"], default="f64")
    args = ap.parse_args()
    dev, dt = "cuda:0", (torch.float64 if args.dtype == "f64" else torch.float32)
    pos, cell, q, _ = S.fcc_box(args.atoms, dtype=np.float64)
    n = pos.shape[0]
    P, C, Q = (torch.as_tensor(a, device=dev, dtype=dt) for a in (pos, cell, q))
    C = C.reshape(1, 3, 3)
    g = np.random.default_rng(0)
    M = torch.as_tensor(0.3 * g.normal(size=(n, 3)), device=dev, dtype=dt)
    T = 0.3 * g.normal(size=(n, 3, 3))
    T = torch.as_tensor(0.5 * (T + T.transpose(0, 2, 1)), device=dev, dtype=dt)
    est = estimate_pme_parameters(P, C, None, args.accuracy)
    alpha, dims = est.alpha.to(dt), tuple(int(v) for v in est.mesh_dimensions)
    every = dict(compute_forces=True, compute_charge_gradients=True, compute_dipole_gradients=True, compute_quadrupole_gradients=True,
                 compute_virial=True)
    mesh = dict(mesh_dimensions=dims, spline_order=args.order)
    result = {"atoms": n, "dtype": args.dtype, "order": args.order, "mesh": dims, "alpha": float(alpha[0]), "repeats": args.repeats, "ms": {}}

    def record(name, fn, warmup=args.warmup, repeats=args.repeats, **extra):
        med, best = median_ms(fn, warmup, repeats)
        result["ms"][name] = {"median": round(med, 4), "min": round(best, 4), **extra}
        print(f"{name:62s} median {med:.3f} ms   min {best:.3f} ms   {extra if extra else ''}", flush=True)

    record("pme_dipole_reciprocal_space E+F", lambda: pme_dipole_reciprocal_space(P, Q, M, C, alpha, compute_forces=True, **mesh))
    record("pme_quadrupole_reciprocal_space E", lambda: pme_quadrupole_reciprocal_space(P, Q, M, T, C, alpha, **mesh))
    record("pme_quadrupole_reciprocal_space E+F", lambda: pme_quadrupole_reciprocal_space(P, Q, M, T, C, alpha, compute_forces=True, **mesh))
    record("pme_quadrupole_reciprocal_space E+F+dq+dmu+dQ+virial", lambda: pme_quadrupole_reciprocal_space(P, Q, M, T, C, alpha, **every, **mesh))

    edge = float(torch.linalg.norm(C[0], dim=-1).max())
    kv = generate_k_vectors_ewald_summation(C, 2.0 * math.pi * (args.k_index - 0.01) / edge)
    record(f"ewald_quadrupole_reciprocal_space E+F, K = {kv.shape[0]}",
           lambda: ewald_quadrupole_reciprocal_space(P, Q, M, T, C, kv, alpha, compute_forces=True), k_vectors=int(kv.shape[0]))
    ew = estimate_ewald_parameters(P, C, None, args.accuracy)
    k_cut, al = float(ew.reciprocal_space_cutoff.max()), ew.alpha.to(dt)
    result["explicit_k_cutoff_wanted"] = k_cut
    while True:
        kv = generate_k_vectors_ewald_summation(C, k_cut)
        fn = lambda: ewald_quadrupole_reciprocal_space(P, Q, M, T, C, kv, al, compute_forces=True)  # noqa: E731
        fn()  # first call: allocations
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        once = time.perf_counter() - t0
        if once <= args.limit:
            break
        print(f"ewald_quadrupole_reciprocal_space at k_cutoff {k_cut:.3f} (K = {kv.shape[0]}): one call takes {once:.1f} s, over the limit", flush=True)
        result.setdefault("explicit_over_limit", []).append({"k_cutoff": k_cut, "k_vectors": int(kv.shape[0]), "seconds": round(once, 2)})
        k_cut *= 0.8
    fit = max(1, min(args.repeats, int(args.limit / max(once, 1e-9)) - 2))
    record(f"ewald_quadrupole_reciprocal_space E+F, k_cutoff {k_cut:.3f}, K = {kv.shape[0]}", fn, warmup=min(args.warmup, 1), repeats=fit,
           k_vectors=int(kv.shape[0]), k_cutoff=round(k_cut, 4), repeats_used=fit)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
