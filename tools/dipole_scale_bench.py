"""Timing aid for the scaled bonded dipole pairs (csrc/dipole_scale.hip), on the water and hexane boxes of tools/pair_scale_bench.py
(100 000 atoms each), every pair of variants alternated in one process:

    energy   `dipole_pair_scale_correction(compute_forces=True, minimum_image=True)` beside the composed path it replaces, two
             `pair_scale_correction` calls (q, mu) - (q alone): that path exists only for the undamped, equal-scale case, which is what is timed
    product  `mi_scaled_dipole_apply` over the bonded matrix beside `mi_induced_apply` over the real-space list of the same box (cut-off 8:
             about 215 of 256 slots per row), and the byte counts both stream
    solve    `scaled_induced_dipoles(reciprocal="pme")` (1-2 and 1-3 pairs: direct and mutual scale 0) beside `induced_dipoles` on the same box

`--rounds` rounds of warm-up + event-bracketed repeats; the table gives the median of the round medians and their range.  There is no pass /
fail threshold.  The table of DESIGN.md section 3.34 is the `--markdown` output of this tool.

    python tools/dipole_scale_bench.py [--repeats 20] [--rounds 3] [--markdown]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nvalchemi-toolkit-ops_amd")]

from nvalchemiops.interactions.electrostatics import (PolarizationPairScales, bonded_pair_scales, dipole_pair_scale_correction,  # noqa: E402
                                                      induced_dipoles, pair_scale_correction, scaled_induced_dipoles)
from nvalchemiops.interactions.electrostatics import induced as I  # noqa: E402
from nvalchemiops.neighborlist import cell_list  # noqa: E402
from tools.induced_bench import median_ms  # noqa: E402
from tools.pair_scale_bench import build, hexane, water  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--waters", type=int, default=33334)
    ap.add_argument("--chains", type=int, default=5000)
    ap.add_argument("--cutoff", type=float, default=8.0)
    ap.add_argument("--max-neighbors", type=int, default=256)
    ap.add_argument("--mesh", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--solve-repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    dev, dt = "cuda:0", torch.float64
    g = np.random.default_rng(0)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev, dtype=dt)  # noqa: E731
    result = {"repeats": args.repeats, "rounds": args.rounds, "cases": {}}
    for name, molecule, count in (("water", water(), args.waters), ("hexane", hexane(), args.chains)):
        pos, bonds, cell = build(molecule, count, g)
        n = pos.shape[0]
        P, Cl = t(pos), t(cell).reshape(1, 3, 3)
        q, mu, x3 = t(g.normal(size=n)), t(0.3 * g.normal(size=(n, 3))), t(g.normal(size=(n, 3)))
        q = q - q.mean()
        polar = t(g.uniform(0.02, 0.08, n) * 0.95**3)  # below a tenth of the cube of the shortest bond: the unscaled solve converges too
        nm, s = bonded_pair_scales(bonds, n, (0.0, 0.0), device=dev)[:2]
        sp = PolarizationPairScales(nm, s, s)
        bonded = dict(neighbor_matrix=nm, mask_value=n, minimum_image=True, compute_forces=True)

        def fused():
            return dipole_pair_scale_correction(P, q, mu, s, s, Cl, **bonded)

        def composed():
            e1, f1 = pair_scale_correction(P, q, mu, None, s, Cl, **bonded)
            e0, f0 = pair_scale_correction(P, q, None, None, s, Cl, **bonded)
            return e1 - e0, f1 - f0

        (ef, ff), (ec, fc) = fused(), composed()
        parity = (float((ec - ef).abs().max() / ec.abs().max()), float((fc - ff).abs().max() / fc.abs().max()))
        rnm, num, sh = cell_list(P, args.cutoff, Cl[0], torch.ones(3, dtype=torch.bool, device=dev), max_neighbors=args.max_neighbors)
        assert int(num.max()) <= args.max_neighbors, "rows overflow: raise --max-neighbors"
        lists = (None, None, None, rnm, sh)
        alpha, mesh = torch.tensor([0.35], dtype=dt, device=dev), (args.mesh,) * 3
        op = I._Operator(P, polar, Cl, None, 1, lists, n, "pme", alpha, mesh, None, 5, None, None, 1e-6, None, sp)
        scaled, op.scaled = op.scaled, None  # `op.apply` is then the main product alone
        kw = dict(alpha=alpha, mesh_dimensions=mesh, tolerance=1e-8, return_info=True, neighbor_matrix=rnm, neighbor_matrix_shifts=sh, mask_value=n)
        solve = lambda pairs: (induced_dipoles(P, q, polar, Cl, **kw) if pairs is None  # noqa: E731
                               else scaled_induced_dipoles(P, q, polar, Cl, scaled_pairs=pairs, **kw))
        variants = {"energy fused": (fused, args.repeats), "energy composed": (composed, args.repeats),
                    "product bonded": (lambda: scaled.apply(x3), args.repeats), "product main": (lambda: op.apply(x3), args.repeats),
                    "solve scaled": (lambda: solve(sp), args.solve_repeats), "solve unscaled": (lambda: solve(None), args.solve_repeats)}
        rounds = {k: [] for k in variants}
        for _ in range(args.rounds):
            for label, (fn, reps) in variants.items():
                rounds[label].append(median_ms(fn, min(args.warmup, reps), reps)[0])
        case = dict(atoms=n, bonded_width=int(nm.shape[1]), bonded_slots=int(nm.numel()), main_slots=int(rnm.numel()), main_stored=int(num.sum()),
                    bonded_mb=round(nm.numel() * 44 / 1e6, 2), main_mb=round(rnm.numel() * 44 / 1e6, 2), parity_energies=parity[0],
                    parity_forces=parity[1], iterations={k: int(solve(p).iterations[0]) for k, p in (("scaled", sp), ("unscaled", None))})
        for label, v in rounds.items():
            case[label] = {"median": round(float(np.median(v)), 4), "low": min(v), "high": max(v)}
            print(f"{name:8s} {label:16s} median of {args.rounds} round medians {np.median(v):.3f} ms   range {min(v):.3f} - {max(v):.3f} ms", flush=True)
        print(f"{name:8s} {n} atoms, bonded rows of {case['bonded_width']} slots ({case['bonded_mb']} MB) against {args.max_neighbors} "
              f"({case['main_mb']} MB), fused against composed: energies {parity[0]:.1e}, forces {parity[1]:.1e}, iterations {case['iterations']}",
              flush=True)
        result["cases"][name] = case
    print(json.dumps(result))
    if args.markdown:
        print("\n| topology | variant | median, ms | range, ms |\n|---|---|---|---|")
        for name, c in result["cases"].items():
            for label in variants:
                print(f"| {name} | {label} | {c[label]['median']:.3f} | {c[label]['low']:.3f} - {c[label]['high']:.3f} |")


if __name__ == "__main__":
    main()
