"""Float64 torch restatement of the five valence terms of nvalchemiops.interactions.valence, from their definitions (Tinker's, angles in
radians, no 1/2): the term energies below, every derivative by autograd, the virial as the strain derivative.  theta and phi come from
atan2, so the restatement stays well conditioned.  No kernel code is consulted.  Pinned by closed forms in tests/test_valence_reference_cpu.py."""
import torch

KINDS = ("bond_stretch", "angle_bend", "stretch_bend", "out_of_plane_bend", "torsion")
ARITY = dict(zip(KINDS, (2, 3, 3, 4, 4)))
F64 = torch.float64


def _poly(D, k, c):
    return k * D ** 2 * (1 + c[0] * D + c[1] * D ** 2 + c[2] * D ** 3 + c[3] * D ** 4)


def _angle(u, v):
    return torch.atan2(torch.linalg.cross(u, v).norm(dim=-1), (u * v).sum(-1))


def term_energies(kind, pos, atoms, par, cell=None, batch_idx=None, consts=(0.0, 0.0, 0.0, 0.0), plane="wdc"):
    """E_t [T] (float64).  `cell` [S, 3, 3]: every difference vector is the minimum image in the cell of the term's first atom."""
    atoms = atoms.long()
    r = pos[atoms]  # [T, A, 3]

    def diff(x, y):  # r_x - r_y
        d = r[:, x] - r[:, y]
        if cell is None:
            return d
        sys = batch_idx.long()[atoms[:, 0]] if batch_idx is not None else torch.zeros_like(atoms[:, 0])
        c = cell.reshape(-1, 3, 3)
        return d - torch.einsum("tk,tkc->tc", torch.round(torch.einsum("tk,tkc->tc", d, torch.linalg.inv(c)[sys])).detach(), c[sys])

    p = par.unbind(-1)
    if kind == "bond_stretch":
        return _poly(diff(0, 1).norm(dim=-1) - p[1], p[0], (consts[0], consts[1], 0.0, 0.0))
    if kind == "angle_bend":
        return _poly(_angle(diff(0, 1), diff(2, 1)) - p[1], p[0], consts)
    if kind == "stretch_bend":
        u, v = diff(0, 1), diff(2, 1)
        return (p[0] * (u.norm(dim=-1) - p[2]) + p[1] * (v.norm(dim=-1) - p[3])) * (_angle(u, v) - p[4])
    if kind == "out_of_plane_bend":
        u, v, w = diff(0, 1), diff(2, 1), diff(3, 1)
        V = (w * torch.linalg.cross(u, v)).sum(-1)
        x, y = (u, v) if plane == "wdc" else (diff(0, 3), diff(2, 3))
        cc = (x * x).sum(-1) * (y * y).sum(-1) - (x * y).sum(-1) ** 2
        return _poly(torch.asin(V.abs() / torch.sqrt(cc * (w * w).sum(-1))), p[0], consts)
    b1, b2, b3 = diff(1, 0), diff(2, 1), diff(3, 2)
    m, n = torch.linalg.cross(b1, b2), torch.linalg.cross(b2, b3)
    phi = torch.atan2(b2.norm(dim=-1) * (b1 * n).sum(-1), (m * n).sum(-1))
    F = par.shape[1] // 2
    return sum(p[f] * (1 + torch.cos((f + 1) * phi - p[F + f])) for f in range(F))


def evaluate(kind, pos, atoms, par, cell=None, batch_idx=None, weights=None, **model):
    """dict of float64 tensors: energies [N] (atom shares), forces, parameter_grads, virial [S, 3, 3] (None without a cell) of the total
    energy, and with `weights` g the gradients positions_grad, parameters_grad of L = sum_i g_i E_i."""
    n, A = pos.shape[0], ARITY[kind]
    pos, par = pos.to(F64).clone().requires_grad_(True), par.to(F64).clone().requires_grad_(True)
    cells = None if cell is None else cell.to(F64).reshape(-1, 3, 3)
    nsys = 1 if cells is None or batch_idx is None else cells.shape[0]
    sys = torch.zeros(n, dtype=torch.long) if nsys == 1 else batch_idx.long()
    eps = torch.zeros((nsys, 3, 3), dtype=F64, requires_grad=True)
    strain = torch.eye(3, dtype=F64) + eps  # x -> (I + eps) x, cell and positions together
    spos = torch.einsum("npq,nq->np", strain[sys], pos)
    scell = None if cells is None else torch.einsum("spq,skq->skp", strain[:cells.shape[0]] if nsys > 1 else strain.expand(cells.shape[0], 3, 3), cells)
    et = term_energies(kind, spos, atoms, par, scell, batch_idx if cells is not None else None, **model)
    energies = torch.zeros(n, dtype=F64).index_add(0, atoms.long().reshape(-1), (et / A).repeat_interleave(A))
    gp, gq, ge = torch.autograd.grad(energies.sum(), (pos, par, eps), retain_graph=True, allow_unused=True)
    out = dict(energies=energies.detach(), forces=-gp, parameter_grads=gq, virial=None if cells is None else -ge)
    if weights is not None:
        out["positions_grad"], out["parameters_grad"] = torch.autograd.grad((weights.to(F64) * energies).sum(), (pos, par))
    return out
