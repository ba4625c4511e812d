"""Yardstick of the cluster (bare, 1/r) multipole sums and of the induced-dipole solve on them: the float64 operator-definition references of
the periodic routines, evaluated at alpha = 0.

`erfc(0 * r) / r` is `1 / r` in torch, so tests/dipole_reference.py, tests/quadrupole_reference.py and tests/induced_reference.py already ARE
the bare kernel at alpha = 0, and tests/thole_reference.py does not depend on alpha at all.  Nothing is restated here: a cluster is handed to
them with an identity cell and zero shifts (the shifts then contribute S . cell = 0 exactly), a periodic cut-off sum with its own cell and
shifts.  tests/test_cluster_multipole_reference_cpu.py checks this yardstick against closed forms and the point-charge limit.

Also here: the hand-made all-pairs lists and the problems of the GPU tests (numpy / torch on the CPU, independent of the neighbour search).
"""
import numpy as np
import torch

from tests import dipole_reference as DR
from tests import induced_reference as IR
from tests import quadrupole_reference as QR
from tests import thole_reference as TR

F64 = torch.float64
ALPHA = 0.0  # the bare kernel


def _cell(cell, device):
    return torch.eye(3, dtype=F64, device=device).reshape(1, 3, 3) if cell is None else cell.detach().to(F64).reshape(-1, 3, 3)


def _batch(cell, batch_idx):
    return None if cell is None else batch_idx  # a cluster has one (identity) cell: the list confines pairs to systems


def _drop_virial(out, cell):
    if cell is None:
        out.pop("virial")
    return out


def dipole_energies(pos, q, mu, entries, cell=None, batch_idx=None, distance_dtype=F64):
    """Per-atom float64 energies of `coulomb_dipole_correction` (differentiable)."""
    return DR.real_energies(pos, q, mu, _cell(cell, pos.device), ALPHA, *entries, batch_idx=_batch(cell, batch_idx), distance_dtype=distance_dtype)


def dipole_evaluate(pos, q, mu, entries, cell=None, batch_idx=None, distance_dtype=F64, weights=None):
    """`dipole_reference.evaluate` at alpha = 0: energies, forces, charge_grads, dipole_grads and, with a cell, the nine-word virial."""
    out = DR.evaluate(pos, q, mu, _cell(cell, pos.device), ALPHA, entries=entries, batch_idx=_batch(cell, batch_idx), distance_dtype=distance_dtype,
                      weights=weights)
    return _drop_virial(out, cell)


def quadrupole_energies(pos, q, mu, Q, entries, cell=None, batch_idx=None, distance_dtype=F64):
    """Per-atom float64 energies of `coulomb_quadrupole_correction` (differentiable)."""
    return QR.real_energies(pos, q, mu, Q, _cell(cell, pos.device), ALPHA, *entries, batch_idx=_batch(cell, batch_idx), distance_dtype=distance_dtype)


def quadrupole_evaluate(pos, q, mu, Q, entries, cell=None, batch_idx=None, distance_dtype=F64, weights=None):
    """`quadrupole_reference.evaluate` at alpha = 0."""
    out = QR.evaluate(pos, q, mu, Q, _cell(cell, pos.device), ALPHA, entries=entries, batch_idx=_batch(cell, batch_idx),
                      distance_dtype=distance_dtype, weights=weights)
    return _drop_virial(out, cell)


def operator(pos, q, polar, thole, entries, differentiable=False):
    """(T [3N, 3N], c [N, 3]) of the cluster energy E(q, mu) = c . mu + 1/2 mu^T T mu: `induced_reference.dipole_operator` at alpha = 0, or
    `thole_reference.damped_operator` (E + E_thole) when `thole` is given."""
    cell = _cell(None, pos.device)
    if thole is None:
        return IR.dipole_operator(pos, q, cell, ALPHA, entries, differentiable=differentiable)
    return TR.damped_operator(pos, q, polar, cell, ALPHA, thole, entries, differentiable=differentiable)


def pair_tensors(pos, entries, distance_dtype=F64):
    """T_e [E, 3, 3] = -Hess_R (1 / r) of every stored entry: `induced_reference.pair_tensors` at alpha = 0."""
    return IR.pair_tensors(pos, _cell(None, pos.device), ALPHA, *entries, distance_dtype=distance_dtype)


# ---- hand-made lists and problems -------------------------------------------------------------------------------------------------------
def all_pairs(sizes):
    """(i, j, S) int64 of the all-pairs list of clusters with `sizes` atoms each, atoms of a cluster contiguous, rows sorted: row a of a cluster
    of m atoms has m - 1 entries."""
    ii, jj, off = [], [], 0
    for m in sizes:
        a = np.arange(m)
        i, j = np.nonzero(a[:, None] != a[None, :])
        ii.append(i + off); jj.append(j + off)
        off += m
    i, j = torch.as_tensor(np.concatenate(ii)), torch.as_tensor(np.concatenate(jj))
    return i, j, torch.zeros((i.shape[0], 3), dtype=torch.long)


def jittered_grid(shape, spacing, jitter, g, origin=(0.0, 0.0, 0.0)):
    """prod(shape) positions on a grid of `spacing`, each moved by up to `jitter` per axis: the shortest distance is >= spacing - 2 jitter."""
    pts = np.stack(np.meshgrid(*[np.arange(k) for k in shape], indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    return pts * spacing + g.uniform(-jitter, jitter, pts.shape) + np.asarray(origin)


SPACING, JITTER = 2.0, 0.35
D_MIN = SPACING - 2.0 * JITTER  # a lower bound of every distance of the problems below
PLAIN = (2, 5, 9)               # atoms that carry a charge only: no dipole, no quadrupole
FROZEN = (4, 11)                # atoms that are not polarisable (a = 0 and a < 0) in the solver problems


def problem(kind, seed=7):
    """dict of float64 numpy arrays of one problem.  "c150": one cluster of 150 atoms (rows of 149 entries: two full wave trips and a tail of
    21).  "batch": three clusters of 70, 2 and 1 atoms (a row longer than 64, one-entry rows, an empty row), far apart only in the sense that
    the list never joins them.  Atoms `PLAIN` have no dipole and no quadrupole; quadrupoles are neither symmetric nor traceless.
    Polarisabilities are uniform in [0.02, 0.08] D_MIN^3 (`polar`; the dense H of the undamped problem is positive definite, which the tests
    assert) with atoms `FROZEN` not polarisable."""
    g = np.random.default_rng(seed)
    if kind == "c150":
        sizes, pos = (150,), jittered_grid((6, 5, 5), SPACING, JITTER, g)
    elif kind == "batch":
        sizes = (70, 2, 1)
        pos = np.concatenate([jittered_grid((7, 5, 2), SPACING, JITTER, g), jittered_grid((2, 1, 1), SPACING, JITTER, g, (1.0, 0.5, 0.25)),
                              jittered_grid((1, 1, 1), SPACING, JITTER, g, (3.0, 3.0, 3.0))])
    else:
        raise ValueError(kind)
    n = sum(sizes)
    q, mu, Q = g.normal(size=n) + 0.05, 0.4 * g.normal(size=(n, 3)), 0.3 * g.normal(size=(n, 3, 3))
    mu[list(PLAIN)], Q[list(PLAIN)] = 0.0, 0.0
    polar = g.uniform(0.02, 0.08, n) * D_MIN**3
    polar[FROZEN[0]], polar[FROZEN[1]] = 0.0, -0.3
    return dict(kind=kind, n=n, sizes=sizes, nsys=len(sizes), pos=pos, q=q, mu=mu, Q=Q, polar=polar, w=g.normal(size=n),
                field=0.1 * g.normal(size=(n, 3)), batch_idx=np.repeat(np.arange(len(sizes)), sizes).astype(np.int32), entries=all_pairs(sizes))


def periodic_problem(seed=11):
    """About 100 atoms (96) in a triclinic box and every image within 9.0: rows of more than 64 entries and self-image entries (i, i, S != 0)
    present (both asserted by the test).  The cut-off sum over a periodic list, with the nine-word virial."""
    g = np.random.default_rng(seed)
    pos = jittered_grid((6, 4, 4), 2.2, 0.4, g)
    cell = np.array([[13.2, 0.0, 0.0], [1.1, 8.8, 0.0], [-0.7, 0.9, 8.8]])
    n = pos.shape[0]
    shifts = np.stack(np.meshgrid(*[np.arange(-2, 3)] * 3, indexing="ij"), -1).reshape(-1, 3)
    d = pos[None, :, None, :] + (shifts @ cell)[None, None, :, :] - pos[:, None, None, :]  # [i, j, S, 3]
    r = np.linalg.norm(d, axis=-1)
    i, j, s = np.nonzero((r < 9.0) & (r > 1e-6))
    order = np.argsort(i, kind="stable")
    i, j, s = i[order], j[order], s[order]
    q, mu, Q = g.normal(size=n), 0.4 * g.normal(size=(n, 3)), 0.3 * g.normal(size=(n, 3, 3))
    return dict(n=n, pos=pos, cell=cell, q=q - q.mean(), mu=mu, Q=Q, w=g.normal(size=n),
                entries=(torch.as_tensor(i), torch.as_tensor(j), torch.as_tensor(shifts[s])))


def dense_problem(p, thole, device, scale=1.0):
    """(H [3N, 3N], b [3N], c [N, 3], polar [N]) of the solver problem `p` on `device`: polarisabilities `scale` times those of the problem,
    the problem's external field."""
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=device, dtype=F64)  # noqa: E731
    polar = t(p["polar"]) * scale
    entries = tuple(e.to(device) for e in p["entries"])
    T, c = operator(t(p["pos"]), t(p["q"]), polar, thole, entries)
    return IR.system_matrix(T, polar), IR.right_hand_side(c, polar, t(p["field"])), c, polar
