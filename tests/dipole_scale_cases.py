"""Problems of the `dipole_pair_scale_correction` and `scaled_induced_dipoles` tests (CPU, float64), shared by tests/test_dipole_scale_reference_cpu.py
and tests/test_dipole_scale_gpu.py.

Energy cases are the hand-made lists of tests/pair_scale_cases.py -- the 70-atom ladder whose rows hold 0, 1, 7, 8, 9, 16, 17 and 25 entries,
the 7-atom all-pairs cluster, the triclinic box with explicit shifts, the batch of three wrapped molecules -- with each scale class of those
lists mapped to a pair (s^d, s^m) out of {(0, 0), (0.4, 1), (1, 0.3), (1, 1)}, polarisabilities uniform in [0.3, 1.5], atom 3 not polarisable
(a = 0) and atom 4 with a = NaN.  Ladder pairs are not neighbours in space, so their distances run from 1.3 to about 15: at a_T = 0.39 both
E < 50 and E >= 50 occur (asserted on the CPU).

Solve cases: "bent", three bent three-atom molecules 5 apart as one cluster over its all-pairs list, 1-2 and 1-3 pairs with direct and mutual
scale 0, the last atom not polarisable; "chains", the 27-atom lattice of tests/induced_cases.py with nine three-atom chains (atoms 3k, 3k + 1,
3k + 2), 1-2 scales (0, 0) and 1-3 scales (0.4, 0.3), atom 5 not polarisable, real-space list within 7.0."""
import functools

import numpy as np
import torch

from tests import cluster_multipole_reference as CR
from tests import dipole_reference as DR
from tests import dipole_scale_reference as SR
from tests import induced_cases as IC
from tests import induced_reference as IR
from tests import pair_scale_cases as PC
from tests import thole_reference as TR

F64 = torch.float64
A_T = 0.39
CLASS = {0.0: (0.0, 0.0), 0.4: (0.4, 1.0), 0.8: (1.0, 0.3), 1.0: (1.0, 1.0)}  # scale class of pair_scale_cases -> (s^d, s^m)
KINDS = ("ladder70", "ladder7", "periodic", "molecules")


@functools.lru_cache(maxsize=None)
def problem(kind):
    """A problem of tests/pair_scale_cases.py plus polar [n], sd / sm [entries]."""
    p = dict(PC.ladder(int(kind[6:])) if kind.startswith("ladder") else PC.periodic() if kind == "periodic" else PC.molecules())
    g = np.random.default_rng(300 + p["n"])
    polar = g.uniform(0.3, 1.5, p["n"])
    polar[3], polar[4] = 0.0, np.nan
    sd, sm = np.array([CLASS[float(s)] for s in p["scales"]]).reshape(-1, 2).T
    p.update(polar=polar, sd=sd, sm=sm)
    return p


def matrix(i, j, n, width, cols=(), fill=1.0):
    """Padded [n, width] int64 matrix of the entries (sorted by row; padding n) and the per-entry arrays `cols` scattered alike (padding:
    `fill` for floating-point arrays, 0 for integer ones)."""
    counts = torch.bincount(i, minlength=n)
    col = torch.arange(i.shape[0]) - (torch.cumsum(counts, 0) - counts)[i]
    nm = torch.full((n, width), n, dtype=torch.long)
    nm[i, col] = j
    out = []
    for c in cols:
        m = torch.full((n, width) + tuple(c.shape[1:]), fill if c.is_floating_point() else 0, dtype=c.dtype)
        m[i, col] = c
        out.append(m)
    return (nm, *out)


def _bonded(chains, scales12, scales13):
    """Entries (i, j, 0) sorted by row, sd, sm of three-atom chains (a, b, c) bonded a-b, b-c."""
    pairs = {}
    for a, b, c in chains:
        for x, y, s in ((a, b, scales12), (b, c, scales12), (a, c, scales13)):
            pairs[(x, y)] = pairs[(y, x)] = s
    keys = sorted(pairs)
    i, j = torch.as_tensor([k[0] for k in keys]), torch.as_tensor([k[1] for k in keys])
    s = torch.as_tensor([pairs[k] for k in keys], dtype=F64)
    return (i, j, torch.zeros((len(keys), 3), dtype=torch.long)), s[:, 0].contiguous(), s[:, 1].contiguous()


@functools.lru_cache(maxsize=None)
def solve_case(kind):
    """dict of CPU float64 tensors: pos, q, polar, field, cell | None, ent (the solver's list), bent (the bonded list), sd, sm, and for
    "chains" alpha and kv."""
    g = np.random.default_rng(41)
    if kind == "bent":
        mol = PC._water()  # O at the apex, bonds of 1.4, H-H 2.21
        pos = np.concatenate([mol + o for o in ([0.0, 0.0, 0.0], [5.0, 0.5, 0.3], [0.4, 5.2, -0.6])]) + g.uniform(-0.05, 0.05, (9, 3))
        polar = g.uniform(0.8, 1.2, 9)
        polar[8] = 0.0
        bent, sd, sm = _bonded([(3 * k + 1, 3 * k, 3 * k + 2) for k in range(3)], (0.0, 0.0), (0.0, 0.0))
        c = dict(n=9, pos=pos, q=0.5 * g.normal(size=9), polar=polar, cell=None, ent=CR.all_pairs([9]))
    else:
        lat = IC.lattice("l27")
        polar = lat["polar"].copy()
        polar[5] = 0.0
        bent, sd, sm = _bonded([(3 * k, 3 * k + 1, 3 * k + 2) for k in range(9)], (0.0, 0.0), (0.4, 0.3))
        c = dict(n=27, pos=lat["pos"], q=lat["q"], polar=polar, cell=lat["cell"].reshape(1, 3, 3), ent=IC.entries("l27", 7.0, 1),
                 alpha=IC.EWALD["alpha"], kv=IC.k_vectors(lat["cell"], IC.EWALD["k_cutoff"]))
    c.update(field=0.1 * g.normal(size=(c["n"], 3)), w=g.normal(size=(c["n"], 3)))
    c = {k: torch.as_tensor(v, dtype=F64) if isinstance(v, np.ndarray) else v for k, v in c.items()}
    c.update(bent=bent, sd=sd, sm=sm)
    return c


def dense(c, thole, dev="cpu", leaves=None):
    """(H_ref [3n, 3n], b [3n]) of a solve case on `dev`: the exact Hessian in mu of the existing reference total (+ E_thole) plus the
    scaled-pair term, + diag(1 / a).  `leaves`: dict(pos, q, polar, field) to differentiate with respect to."""
    t = lambda v: v.to(dev) if isinstance(v, torch.Tensor) else v  # noqa: E731
    r = leaves or {k: t(c[k]) for k in ("pos", "q", "polar", "field")}
    ent, bent = tuple(t(e) for e in c["ent"]), tuple(t(e) for e in c["bent"])
    cell = None if c["cell"] is None else t(c["cell"])

    def base(mu):
        if cell is None:
            e = CR.dipole_energies(r["pos"], r["q"], mu, ent).sum()
        else:
            e = DR.energies(r["pos"], r["q"], mu, cell, c["alpha"], ent, t(c["kv"])).sum()
        return e if thole is None else e + TR.energies(r["pos"], r["q"], mu, r["polar"], cell, thole, *ent).sum()

    T, lin = SR.scaled_operator(base, r["pos"], r["q"], r["polar"], t(c["sd"]), t(c["sm"]), bent, cell=cell, thole=thole,
                                minimum_image=cell is not None, differentiable=leaves is not None)
    return IR.system_matrix(T, r["polar"]), IR.right_hand_side(lin, r["polar"], r["field"])
