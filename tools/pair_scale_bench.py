"""Timing aid: the fused `pair_scale_correction` beside the composed path it replaces, on the same bonded lists, in one process.

Composed path: one list per distinct scale value s and, per list, `coulomb_energy_forces` + `coulomb_dipole_correction` +
`coulomb_quadrupole_correction` with forces, each multiplied by (s - 1) on the host and added up -- nine launch sequences for AMOEBA's
three values 0 / 0.4 / 0.8, each with its own record pack and a wave64 per row.  Fused path: ONE `pair_scale_correction(compute_forces=True,
minimum_image=True)` over the whole list of `bonded_pair_scales` (8 lanes per row).  fp64, random charges, dipoles and quadrupoles.

Two topologies in an orthorhombic cell, molecules whole (the composed operators have no minimum image, so they run without shifts):
    water    33 334 molecules, 100 002 atoms: rows of 2 entries, one scale value (1-2 and 1-3 are both 0)
    hexane   5 000 alkane-like C6H14 chains of 20 atoms, 100 000 atoms: rows of 10 to 19 entries, three scale values

The two are timed alternately in `--rounds` rounds of warm-up + event-bracketed repeats; the table gives the median of the round medians
and their range, which is the run-to-run spread of the session.  There is no pass / fail threshold.  The table of DESIGN.md section 3.32
is the `--markdown` output of this tool.

    python tools/pair_scale_bench.py [--repeats 20] [--rounds 3] [--markdown]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nvalchemi-toolkit-ops_amd")]

from nvalchemiops.interactions.electrostatics import (bonded_pair_scales, coulomb_dipole_correction,  # noqa: E402
                                                      coulomb_quadrupole_correction, pair_scale_correction)
from nvalchemiops.interactions.electrostatics.coulomb import coulomb_energy_forces  # noqa: E402
from tools.induced_bench import median_ms  # noqa: E402


def water():
    h = np.deg2rad(104.5 / 2.0)
    pos = np.array([[0.0, 0.0, 0.0], [0.9572 * np.sin(h), 0.9572 * np.cos(h), 0.0], [-0.9572 * np.sin(h), 0.9572 * np.cos(h), 0.0]])
    return pos, [(0, 1), (0, 2)], (3.1, 3.1, 3.1)


def hexane():
    """C6H14: carbons 0 ... 5 in a zig-zag along x, hydrogens 6 ... 19 (three on each end carbon, two on each inner one)."""
    k = np.arange(6, dtype=np.float64)
    carbon = np.stack([1.27 * k, 0.43 * (-1.0) ** k, 0.0 * k], -1)
    pos, bonds = [c for c in carbon], [(a, a + 1) for a in range(5)]
    for a in range(6):
        out = -np.sign(carbon[a, 1])
        dirs = [(0.0, 0.55 * out, 0.83), (0.0, 0.55 * out, -0.83)]
        if a in (0, 5):
            dirs.append((-0.9 if a == 0 else 0.9, -0.43 * out, 0.0))
        for d in dirs:
            bonds.append((a, len(pos)))
            pos.append(carbon[a] + 1.09 * np.asarray(d) / np.linalg.norm(d))
    return np.array(pos), bonds, (9.5, 4.6, 4.6)


def build(molecule, count, g):
    """`count` copies of a molecule on an orthorhombic grid: positions [N, 3], bonds [B, 2], cell [3, 3]."""
    pos, bonds, pitch = molecule
    m = pos.shape[0]
    side = int(np.ceil(count ** (1.0 / 3.0)))
    grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:count]
    origins = grid * np.asarray(pitch) + g.uniform(-0.05, 0.05, (count, 3))
    allpos = (origins[:, None, :] + pos[None, :, :]).reshape(-1, 3)
    allbonds = (np.asarray(bonds)[None, :, :] + m * np.arange(count)[:, None, None]).reshape(-1, 2)
    return allpos, allbonds, np.diag(side * np.asarray(pitch))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--waters", type=int, default=33334)
    ap.add_argument("--chains", type=int, default=5000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
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
        q, mu, Q = t(g.normal(size=n)), t(0.3 * g.normal(size=(n, 3))), t(0.2 * g.normal(size=(n, 3, 3)))
        topo = bonded_pair_scales(bonds, n, device=dev)
        nm, sc, num = topo
        values = sorted(set(sc[nm != n].tolist()))
        rows = torch.arange(n, device=dev).unsqueeze(1).expand_as(nm)
        classes = []
        for s in values:  # one CSR list per distinct scale value, built once
            sel = (nm != n) & (sc == s)
            i, j = rows[sel], nm[sel].long()
            ptr = torch.zeros(n + 1, dtype=torch.int32, device=dev)
            ptr[1:] = torch.cumsum(torch.bincount(i, minlength=n), 0)
            classes.append((s, dict(neighbor_list=torch.stack([i, j]).to(torch.int32).contiguous(), neighbor_ptr=ptr),
                            torch.zeros((i.shape[0], 3), dtype=torch.int32, device=dev)))

        def composed():
            e = f = None
            for s, lists, zero_shifts in classes:
                e0, f0 = coulomb_energy_forces(P, q, Cl, 1e6, 0.0, neighbor_shifts=zero_shifts, **lists)
                e1, f1 = coulomb_dipole_correction(P, q, mu, compute_forces=True, **lists)
                e2, f2 = coulomb_quadrupole_correction(P, q, mu, Q, compute_forces=True, **lists)
                de, df = (s - 1.0) * (e0 + e1 + e2), (s - 1.0) * (f0 + f1 + f2)
                e, f = (de, df) if e is None else (e + de, f + df)
            return e, f

        def fused():
            return pair_scale_correction(P, q, mu, Q, sc, Cl, neighbor_matrix=nm, mask_value=n, minimum_image=True, compute_forces=True)

        (ec, fc), (ef, ff) = composed(), fused()
        parity = (float((ec - ef).abs().max() / ec.abs().max()), float((fc - ff).abs().max() / fc.abs().max()))
        rounds = {"composed": [], "fused": []}
        for _ in range(args.rounds):
            for label, fn in (("composed", composed), ("fused", fused)):
                rounds[label].append(median_ms(fn, args.warmup, args.repeats)[0])
        case = dict(atoms=n, row_width=int(nm.shape[1]), rows_min=int(num.min()), rows_max=int(num.max()), entries=int(num.sum()),
                    scale_values=values, parity_energies=parity[0], parity_forces=parity[1])
        for label, v in rounds.items():
            case[label] = {"median": round(float(np.median(v)), 4), "low": min(v), "high": max(v)}
            print(f"{name:8s} {label:9s} median of {args.rounds} round medians {np.median(v):.3f} ms   range {min(v):.3f} - {max(v):.3f} ms", flush=True)
        print(f"{name:8s} {n} atoms, rows of {case['rows_min']} - {case['rows_max']} entries, scale values {values}, fused against composed: "
              f"energies {parity[0]:.1e}, forces {parity[1]:.1e}", flush=True)
        result["cases"][name] = case
    print(json.dumps(result))
    if args.markdown:
        print(f"\n| topology | atoms | rows | scale values | composed, ms | fused, ms | ratio |\n|---|---|---|---|---|---|---|")
        for name, c in result["cases"].items():
            print(f"| {name} | {c['atoms']} | {c['rows_min']} - {c['rows_max']} | {len(c['scale_values'])} | {c['composed']['median']:.3f} "
                  f"({c['composed']['low']:.3f} - {c['composed']['high']:.3f}) | {c['fused']['median']:.3f} ({c['fused']['low']:.3f} - "
                  f"{c['fused']['high']:.3f}) | {c['composed']['median'] / c['fused']['median']:.1f} |")


if __name__ == "__main__":
    main()
