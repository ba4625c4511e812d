"""Float64 torch restatement of stretch-torsion, angle-torsion, pi-torsion and torsion-torsion from their definitions, every derivative by
autograd, the virial as the strain derivative.  No kernel code is consulted.  The bicubic interpolant has its own construction: a dense cyclic
solve for the spline derivatives, Hermite basis products, torch.floor and a modulo for the cell.  Pinned in test_coupled_torsion_reference_cpu.py."""
import math

import torch

from tests.valence_reference import _angle

KINDS = ("stretch_torsion", "angle_torsion", "pi_torsion", "torsion_torsion")
ARITY = dict(zip(KINDS, (4, 4, 6, 5)))
F64 = torch.float64


def _dihedral(b1, b2, b3):
    m, n = torch.linalg.cross(b1, b2), torch.linalg.cross(b2, b3)
    return torch.atan2(b2.norm(dim=-1) * (b1 * n).sum(-1), (m * n).sum(-1))


def spline_derivative(f, dim):  # of the periodic cubic spline through f along `dim`: d_{i-1} + 4 d_i + d_{i+1} = 3 (f_{i+1} - f_{i-1}) / h, h = 2 pi / n
    n = f.shape[dim]
    rhs = torch.movedim(3 * (torch.roll(f, -1, dim) - torch.roll(f, 1, dim)) / (2 * math.pi / n), dim, 0)
    return torch.movedim(torch.linalg.solve(sum(torch.roll(w * torch.eye(n, dtype=F64, device=f.device), k, 0) for w, k in ((4, 0), (1, 1), (1, -1))), rhs.reshape(n, -1)).reshape(rhs.shape), 0, dim)


def node_records(values):
    f = values.to(F64)  # [M, n1, n2] -> (f, f_1, f_2, f_12)
    f1 = spline_derivative(f, 1)
    return f, f1, spline_derivative(f, 2), spline_derivative(f1, 2)


def bicubic(values, m, x, y):  # F_m(x, y) [T] of the maps `values` [M, n1, n2] (or their `node_records`): the cubic Hermite patch of the cell
    records = values if isinstance(values, tuple) else node_records(values)

    def cell(x, n):  # the two node indices and the basis (H00, H01), h (H10, H11) at x
        u = (x + math.pi) * n / (2 * math.pi)
        i = torch.floor(u.detach()).long()
        t = u - i
        return (i % n, (i + 1) % n), ((2 * t ** 3 - 3 * t ** 2 + 1, 3 * t ** 2 - 2 * t ** 3), ((t ** 3 - 2 * t ** 2 + t) * 2 * math.pi / n, (t ** 3 - t ** 2) * 2 * math.pi / n))

    (i, a), (j, b), m = cell(x, records[0].shape[1]), cell(y, records[0].shape[2]), m.long()
    return sum(a[da][p] * b[db][q] * records[da + 2 * db][m, i[p], j[q]] for p in range(2) for q in range(2) for da in range(2) for db in range(2))


def term_energies(kind, pos, atoms, par, cell=None, batch_idx=None, maps=None, map_index=None, signs=None):
    """E_t [T] (float64).  `cell` [S, 3, 3]: every difference vector is the minimum image in the cell of the term's first atom."""
    atoms = atoms.long()
    r = pos[atoms]

    def diff(x, y):  # r_x - r_y
        d = r[:, x] - r[:, y]
        if cell is None:
            return d
        sys = batch_idx.long()[atoms[:, 0]] if batch_idx is not None else torch.zeros_like(atoms[:, 0])
        c = cell.reshape(-1, 3, 3)
        return d - torch.einsum("tk,tkc->tc", torch.round(torch.einsum("tk,tkc->tc", d, torch.linalg.inv(c)[sys])).detach(), c[sys])

    if kind == "pi_torsion":
        p, q = torch.linalg.cross(diff(0, 3), diff(1, 3)), torch.linalg.cross(diff(4, 2), diff(5, 2))
        return par[:, 0] * (1 - torch.cos(2 * _dihedral(-p, diff(3, 2), q)))
    b = [diff(k + 1, k) for k in range(atoms.shape[1] - 1)]
    phi = _dihedral(b[0], b[1], b[2])
    if kind == "torsion_torsion":
        return bicubic(maps, map_index, signs * phi, signs * _dihedral(b[1], b[2], b[3]))
    rows = 3 if kind == "stretch_torsion" else 2
    D = [b[m].norm(dim=-1) if rows == 3 else _angle(-b[m], b[m + 1]) for m in range(rows)]
    k, ref, gamma = par[:, :3 * rows].reshape(-1, rows, 3), par[:, 3 * rows:4 * rows], par[:, 4 * rows:]
    return sum((D[m] - ref[:, m]) * k[:, m, n] * (1 + torch.cos((n + 1) * phi - gamma[:, n])) for m in range(rows) for n in range(3))


def evaluate(kind, pos, atoms, par=None, cell=None, batch_idx=None, weights=None, **tt):
    """tests/valence_reference.py's `evaluate` for these kinds: energies, forces, parameter_grads, virial | None, positions_grad, parameters_grad."""
    n, A = pos.shape[0], ARITY[kind]
    pos = pos.to(F64).clone().requires_grad_(True)
    par = torch.zeros((atoms.shape[0], 1), dtype=F64, requires_grad=True) if par is None else par.to(F64).clone().requires_grad_(True)
    cells = None if cell is None else cell.to(F64).reshape(-1, 3, 3)
    nsys = 1 if cells is None or batch_idx is None else cells.shape[0]
    sys = torch.zeros(n, dtype=torch.long) if nsys == 1 else batch_idx.long()
    eps = torch.zeros((nsys, 3, 3), dtype=F64, requires_grad=True)
    strain = torch.eye(3, dtype=F64) + eps  # x -> (I + eps) x, cell and positions together
    spos = torch.einsum("npq,nq->np", strain[sys], pos)
    scell = None if cells is None else torch.einsum("spq,skq->skp", strain[:cells.shape[0]] if nsys > 1 else strain.expand(cells.shape[0], 3, 3), cells)
    et = term_energies(kind, spos, atoms, par, scell, batch_idx if cells is not None else None, **tt)
    energies = torch.zeros(n, dtype=F64).index_add(0, atoms.long().reshape(-1), (et / A).repeat_interleave(A))
    gp, gq, ge = torch.autograd.grad(energies.sum(), (pos, par, eps), retain_graph=True, allow_unused=True)
    out = dict(energies=energies.detach(), forces=-gp, parameter_grads=gq, virial=None if cells is None else -ge)
    if weights is not None:
        out["positions_grad"], out["parameters_grad"] = torch.autograd.grad((weights.to(F64) * energies).sum(), (pos, par), allow_unused=True)
    return out
