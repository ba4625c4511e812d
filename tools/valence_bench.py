"""Timing aid: the five valence functions (energies and forces) beside the plain-torch expression a user writes today -- the float64-capable
restatement tests/valence_reference.py with autograd and `index_add` -- on the same device, in the same process.

A periodic box of hexane-like molecules (20 atoms: a zigzag carbon backbone with its hydrogens; 19 bonds, 36 angles, 45 torsions and, as
stand-ins for trigonal centres, 24 out-of-plane terms per molecule): 100 000 atoms give 95 000 bonds, 180 000 angles and 225 000 torsions.
Warm-up, then the median of event-bracketed repeats.  The public call is timed once; its launch is timed twice each with the gradient record in planes
[A][3][T] (the shipped layout) and term-major [T][A][3], alternating.  `bytes_per_term` is what the two passes have to move for energies and forces (term
pass: A positions and indices, P parameters, E_t and the record out; gather pass: per slot its index, E_t and a record vector, per atom the
outputs), so bytes_per_term * T / time is the achieved bandwidth.

The four coupled torsion terms (`--kinds coupled`, or `all`) run on the same box: stretch- and angle-torsion over its torsions, pi-torsion
over stand-ins (a C-C bond with two more neighbours of either end), torsion-torsion over every five-atom path, reading eight 24 x 24 maps;
and as a peptide-like mix, one torsion-torsion, two pi-torsions and eight stretch- and angle-torsions per 20-atom molecule (a protein has
about one torsion-torsion per 16 atoms), the terms in molecule order.  The torsion-torsion launch is timed for terms grouped by map and for
the map drawn at random per term, twice each, alternating: the corner records are read through the cache and the order does not matter.  The
plain-torch expression is tests/coupled_torsion_reference.py with autograd and `index_add`; all times are whole calls.

    python tools/valence_bench.py [--atoms 100000] [--repeats 200] [--kinds simple|coupled|all]
"""
import argparse
import itertools
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nvalchemi-toolkit-ops_amd")]
from tests import coupled_torsion_reference as CR  # noqa: E402
from tests import valence_reference as R  # noqa: E402

from nvalchemiops.interactions import valence as V  # noqa: E402
from nvalchemiops.interactions.valence import functions as F  # noqa: E402
from nvalchemiops.interactions.valence import tortor as TT  # noqa: E402


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


def hexane():
    """(positions [20, 3], bonds) of one molecule: carbons 0..5 on a zigzag, two hydrogens each, a third on both ends."""
    pos = [[1.27 * i, 0.43 * (-1) ** i, 0.0] for i in range(6)]
    bonds = [(i, i + 1) for i in range(5)]
    for i in range(6):
        for s in (-1.0, 1.0):
            bonds.append((i, len(pos)))
            pos.append([1.27 * i, (0.43 + 0.63) * (-1) ** i, 0.89 * s])
    for i, dx in ((0, -1.03), (5, 1.03)):
        bonds.append((i, len(pos)))
        pos.append([1.27 * i + dx, 0.43 * (-1) ** i - 0.36 * (-1) ** i, 0.0])
    return np.array(pos), bonds


def topology(bonds, n):
    nb = [[] for _ in range(n)]
    for a, b in bonds:
        nb[a].append(b)
        nb[b].append(a)
    angles = [(a, b, c) for b in range(n) for a, c in itertools.combinations(nb[b], 2)]
    torsions = [(a, b, c, d) for b, c in bonds for a in nb[b] if a != c for d in nb[c] if d != b]
    oop = [(x[0], b, x[1], d) for b in range(n) if len(nb[b]) == 4 for d in nb[b] for x in [[y for y in nb[b] if y != d]]]
    pi = [(x[0], x[1], b, c, y[0], y[1]) for b, c in bonds for x in [[a for a in nb[b] if a != c]] for y in [[d for d in nb[c] if d != b]]
          if len(x) >= 2 and len(y) >= 2]
    paths = [(a, b, c, d, e) for a, b, c, d in torsions + [t[::-1] for t in torsions] for e in nb[d] if e not in (a, b, c) and a < e]
    return dict(bond_stretch=bonds, angle_bend=angles, stretch_bend=angles, out_of_plane_bend=oop, torsion=torsions, stretch_torsion=torsions,
                angle_torsion=torsions, pi_torsion=pi, torsion_torsion=paths)


def coupled(result, one, m, n, pos, cell, args, dev):
    """The four coupled torsion terms on the box (`one`: the terms of one molecule) and as a peptide-like mix."""
    width = dict(stretch_torsion=15, angle_torsion=11, pi_torsion=1)
    grid = -np.pi + 2 * np.pi * torch.arange(24, dtype=torch.float64) / 24
    x, y = torch.meshgrid(grid, grid, indexing="ij")
    values = torch.stack([torch.sin(x + 0.3 * k) * torch.cos(2 * y) + 0.5 * torch.cos(x - y + 0.7 * k) for k in range(8)])
    maps, records = V.TorsionTorsionMaps(values.to(dev)), CR.node_records(values.to(dev))  # both prepared once

    def timed(label, cases):
        for name, call in cases.items():
            med, best = median_ms(call, args.warmup, args.repeats)
            result["ms"][f"{label} {name}"] = {"median": round(med, 4), "min": round(best, 4)}
            print(f"{label:34s} {name:34s} median {med:.4f} ms   min {best:.4f} ms", flush=True)

    for dtype, label in ((torch.float64, "f64"), (torch.float32, "f32")):
        P, C = torch.as_tensor(pos, device=dev, dtype=dtype), cell.to(dev, dtype)
        for mix in ("box", "peptide"):
            for kind in CR.KINDS:
                A = CR.ARITY[kind]
                keep = {"stretch_torsion": 8, "angle_torsion": 8, "pi_torsion": 2, "torsion_torsion": 1}[kind] if mix == "peptide" else None
                tuples = torch.tensor(one[kind])[:keep]
                atoms = (tuples[None] + 20 * torch.arange(m)[:, None, None]).reshape(-1, A).to(dev)
                T = atoms.shape[0]
                result["terms"][f"{kind} {mix}"] = T
                sz = P.element_size()  # as in main(); torsion-torsion reads a map index, a sign and four 32-byte corner records for parameters
                own = width[kind] * sz if kind in width else 4 + 8 + 4 * 32
                result["bytes_per_term"][f"{kind} {mix} {label}"] = round(A * (3 * sz + 4) + own + 8 + 24 * A + A * (4 + 8 + 24) + n / T * (4 * sz + 8), 1)
                tag = f"{kind} {mix} {label} E+F"
                if kind != "torsion_torsion":
                    par = (0.5 + torch.rand((T, width[kind]), generator=torch.Generator().manual_seed(T))).to(dev, dtype)
                    terms = (V.WideValenceTerms if A > 4 else V.ValenceTerms)(atoms, n)
                    fn = getattr(V, kind)

                    def plain():
                        xs = P.detach().requires_grad_(True)
                        et = CR.term_energies(kind, xs, atoms, par, C)
                        e = torch.zeros(n, dtype=dtype, device=dev).index_add(0, atoms.reshape(-1), (et / A).repeat_interleave(A))
                        return e, -torch.autograd.grad(e.sum(), xs)[0]

                    timed(tag, {"public call": lambda: fn(P, terms, par, C, compute_forces=True), "torch autograd + index_add": plain})
                    (e, f), (we, wf) = fn(P, terms, par, C, compute_forces=True), (t.detach() for t in plain())
                else:
                    gen = torch.Generator().manual_seed(T)
                    signs = (1.0 - 2.0 * torch.randint(0, 2, (T,), generator=gen)).to(dev)
                    index = {"grouped by map": (torch.arange(T) * 8 // T), "random map": torch.randint(0, 8, (T,), generator=gen)}
                    tables = {k: V.TorsionTorsionTerms(atoms, v.to(dev), n, signs=signs) for k, v in index.items()}

                    def hip(t):  # one launch: the public call without its argument checks
                        return TT._launch(P, C, None, t.atoms, t.slot_ptr, t.slot_idx, maps.nodes, t.map_index, t.signs, F.VALENCE_FORCES)[:2]

                    def plain():
                        t = tables["grouped by map"]
                        xs = P.detach().requires_grad_(True)
                        et = CR.term_energies(kind, xs, atoms, None, C, maps=records, map_index=t.map_index, signs=t.signs.to(dtype))
                        e = torch.zeros(n, dtype=et.dtype, device=dev).index_add(0, atoms.reshape(-1), (et / A).repeat_interleave(A))
                        return e.to(dtype), -torch.autograd.grad(e.sum(), xs)[0]

                    cases = {"public call": lambda: V.torsion_torsion(P, tables["grouped by map"], maps, C, compute_forces=True)}
                    for again in ("", " again"):
                        for k, t in tables.items():
                            cases[f"launch, {k}{again}"] = lambda t=t: hip(t)
                    cases["torch autograd + index_add"] = plain
                    timed(tag, cases)
                    (e, f), (we, wf) = hip(tables["grouped by map"]), (t.detach() for t in plain())
                print(f"{tag}: max |E_i - torch| / max |E_i| = {float((e - we).abs().max() / we.abs().max()):.2e}, "
                      f"forces {float((f - wf).abs().max() / wf.abs().max()):.2e}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--kinds", choices=("simple", "coupled", "all"), default="all")
    args = ap.parse_args()
    dev = "cuda:0"
    mol, bonds = hexane()
    m = args.atoms // 20
    side = int(np.ceil(m ** (1 / 3)))
    grid = np.array([(i, j, k) for i in range(side) for j in range(side) for k in range(side)][:m], dtype=np.float64)
    rng = np.random.default_rng(1)
    pos = (grid[:, None, :] * 9.0 + mol[None] + 1.5 + 0.05 * rng.standard_normal((m, 20, 3))).reshape(-1, 3)
    n = pos.shape[0]
    cell = torch.eye(3, dtype=torch.float64) * (9.0 * side)
    one = topology(bonds, 20)
    width = dict(bond_stretch=2, angle_bend=2, stretch_bend=5, out_of_plane_bend=1, torsion=6)
    result = {"atoms": n, "repeats": args.repeats, "terms": {}, "bytes_per_term": {}, "ms": {}}
    for dtype, label in ((torch.float64, "f64"), (torch.float32, "f32")):
        P, C = torch.as_tensor(pos, device=dev, dtype=dtype), cell.to(dev, dtype)
        for kind in R.KINDS if args.kinds != "coupled" else ():
            A = R.ARITY[kind]
            atoms = (torch.tensor(one[kind])[None] + 20 * torch.arange(m)[:, None, None]).reshape(-1, A).to(dev)
            T, W = atoms.shape[0], width[kind]
            par = (0.5 + torch.rand((T, W), generator=torch.Generator().manual_seed(T))).to(dev, dtype)
            terms = V.ValenceTerms(atoms, n)
            fn = getattr(V, kind)
            sz = P.element_size()
            result["terms"][kind] = T
            result["bytes_per_term"][f"{kind} {label}"] = round(A * (3 * sz + 4) + W * sz + 8 + 24 * A + A * (4 + 8 + 24) + n / T * (4 * sz + 8), 1)

            def hip(layout):  # one launch with the layout flag: the public call without its argument checks
                return F._launch(R.KINDS.index(kind), P, par, C, None, terms.atoms, terms.slot_ptr, terms.slot_idx, (0.0,) * 4, 0,
                                 F.VALENCE_FORCES | layout)[:2]

            def plain():
                x = P.detach().requires_grad_(True)
                et = R.term_energies(kind, x, atoms, par, C)
                e = torch.zeros(n, dtype=dtype, device=dev).index_add(0, atoms.reshape(-1), (et / A).repeat_interleave(A))
                return e, -torch.autograd.grad(e.sum(), x)[0]

            cases = {"public call": lambda: fn(P, terms, par, C, compute_forces=True), "planes": lambda: hip(0),
                     "term-major": lambda: hip(F.VALENCE_TERM_MAJOR), "planes again": lambda: hip(0),
                     "term-major again": lambda: hip(F.VALENCE_TERM_MAJOR), "torch autograd + index_add": plain}
            for name, call in cases.items():
                med, best = median_ms(call, args.warmup, args.repeats)
                result["ms"][f"{kind} {label} E+F {name}"] = {"median": round(med, 4), "min": round(best, 4)}
                print(f"{kind:18s} {label} E+F {name:28s} median {med:.4f} ms   min {best:.4f} ms", flush=True)
            (e, f), (we, wf) = hip(0), (t.detach() for t in plain())
            print(f"{kind} {label}: max |E_i - torch| / max |E_i| = {float((e - we).abs().max() / we.abs().max()):.2e}, "
                  f"forces {float((f - wf).abs().max() / wf.abs().max()):.2e}", flush=True)
    if args.kinds != "simple":
        coupled(result, one, m, n, pos, cell, args, dev)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
