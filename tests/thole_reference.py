"""Float64 torch restatement of the exponential Thole damping of point dipoles (the AMOEBA form), written from the damping factors and not from
the expanded formulas of the kernel.  Works on the stored entries (i, j, S) of a full neighbour list; runs on any device.

Every dipole is smeared over the density rho(u) = (3 a_T / 4 pi) exp(-a_T u^3), u = r / (a_i a_j)^(1/6).  With E = a_T u^3 = a_T r^3 / sqrt(a_i a_j)

    l3 = 1 - e^-E                         the charge of rho enclosed within u: damps 1/r^3
    l5 = 1 - (1 + E) e^-E                 l_{2n+3} = l_{2n+1} - (r / (2n + 1)) d l_{2n+1} / dr: damps 3/r^5
    l7 = 1 - (1 + E + 3/5 E^2) e^-E       damps 15/r^7 (forces only: here it is used by tests/test_thole_reference_cpu.py alone)

The undamped pair energy of point charges plus point dipoles, without its charge-charge part, is  (1/r^3) A - (3/r^5) c_i c_j  with
A = q_j c_i - q_i c_j + d, c_i = mu_i . R, c_j = mu_j . R, d = mu_i . mu_j; the damped one has l3 / r^3 and 3 l5 / r^5.  The correction that is
ADDED to the undamped energy is therefore

    dU = ((l3 - 1) / r^3) A - (3 (l5 - 1) / r^5) c_i c_j,        E_i = 1/2 sum_{entries of row i} dU

for entries with a_i > 0, a_j > 0 and r > 1e-8; every other entry contributes 0.  There is NO cut at large E here.  Forces, every gradient
and the virial come from autograd (the virial with respect to an explicit strain, dipoles fixed in the laboratory frame).
`distance_dtype=torch.float32` forms the pair vector and the distance in float32 and everything after that in float64: the kernel's arithmetic
model for float32 inputs.  The damped dense operator and solve are those of tests/induced_reference.py with E_dip + E_thole.
"""
import torch

from tests import dipole_reference as DR
from tests import induced_reference as IR

F64 = torch.float64


def lambdas(E):
    """(l3, l5, l7) at E = a_T u^3."""
    ex = torch.exp(-E)
    return 1.0 - ex, 1.0 - (1.0 + E) * ex, 1.0 - (1.0 + E + 0.6 * E * E) * ex


def energies(pos, q, mu, polar, cell, thole, i, j, S, batch_idx=None, distance_dtype=F64):
    """Per-atom float64 energies of the correction (differentiable in pos, q, mu, polar, cell).  cell: [3, 3] / [B, 3, 3] or None (a cluster)."""
    n, dev = pos.shape[0], pos.device
    sys_of = DR._systems(n, batch_idx, dev)
    cells = None if cell is None else cell.reshape(-1, 3, 3)

    def pair_vectors(dtype, p, c):
        v = p.to(dtype)[j] - p.to(dtype)[i]
        return v if c is None else v + torch.einsum("ea,eab->eb", S.to(dtype), c.to(dtype)[sys_of[i]])

    rvec = pair_vectors(F64, pos, cells)
    low = None
    if distance_dtype != F64:
        # the VALUES of the pair vector and of the distance are those of the low-precision arithmetic; derivatives keep flowing through the
        # float64 expressions (value + detached difference)
        low = pair_vectors(distance_dtype, pos.detach(), None if cells is None else cells.detach())
        rvec = rvec + (low.to(F64) - rvec).detach()
    r_val = torch.sqrt((rvec.detach() ** 2).sum(-1)) if low is None else torch.sqrt((low * low).sum(-1)).to(F64)
    a = polar.to(F64)
    ok = a > 0  # (NaN: not polarisable)
    keep = (r_val > 1e-8) & ok[i] & ok[j]
    unit = torch.zeros_like(rvec)
    unit[:, 0] = 1.0
    rv = torch.where(keep.unsqueeze(1), rvec, unit)  # skipped entries: a harmless vector, no gradient to the positions
    r = torch.sqrt((rv * rv).sum(-1))
    if low is not None:
        r = r + (torch.where(keep, r_val, torch.ones_like(r_val)) - r).detach()
    safe = torch.where(ok, a, torch.ones_like(a))
    E = float(thole) * r**3 / torch.sqrt(safe[i] * safe[j])
    l3, l5, _ = lambdas(E)
    q, mu = q.to(F64), mu.to(F64)
    ci, cj = (mu[i] * rv).sum(-1), (mu[j] * rv).sum(-1)
    A = q[j] * ci - q[i] * cj + (mu[i] * mu[j]).sum(-1)
    pair = (l3 - 1.0) / r**3 * A - 3.0 * (l5 - 1.0) / r**5 * ci * cj
    pair = torch.where(keep, pair, torch.zeros_like(pair))
    return torch.zeros(n, dtype=F64, device=dev).index_add(0, i, 0.5 * pair)


def evaluate(pos, q, mu, polar, cell, thole, entries, batch_idx=None, distance_dtype=F64, weights=None):
    """dict of float64 numpy arrays: energies, forces (-dL/dr), charge_grads, dipole_grads, polar_grads of L = sum_i w_i E_i (w = 1 by default)
    and, with a cell, the virial [B, 3, 3] = -dE/d(strain) of the unweighted total (nine independent components)."""
    pos = pos.detach().to(F64).clone().requires_grad_(True)
    q = q.detach().to(F64).clone().requires_grad_(True)
    mu = mu.detach().to(F64).clone().requires_grad_(True)
    polar = polar.detach().to(F64).clone().requires_grad_(True)
    cells = None if cell is None else cell.detach().to(F64).reshape(-1, 3, 3)
    kw = dict(batch_idx=batch_idx, distance_dtype=distance_dtype)
    e = energies(pos, q, mu, polar, cells, thole, *entries, **kw)
    loss = e.sum() if weights is None else (e * weights.to(F64)).sum()
    grads = torch.autograd.grad(loss, [pos, q, mu, polar])
    out = dict(energies=e.detach(), forces=-grads[0], charge_grads=grads[1], dipole_grads=grads[2], polar_grads=torch.nan_to_num(grads[3]))
    if cells is not None:
        nsys = cells.shape[0]
        sys_of = DR._systems(pos.shape[0], batch_idx, pos.device)
        eps = torch.zeros((nsys, 3, 3), dtype=F64, device=pos.device, requires_grad=True)
        defo = torch.eye(3, dtype=F64, device=pos.device) + eps  # x -> (I + eps) x: a row vector becomes x (I + eps)^T
        pos_e = torch.einsum("nb,nab->na", pos.detach(), defo[sys_of])
        cell_e = torch.einsum("srb,sab->sra", cells, defo)
        es = energies(pos_e, q.detach(), mu.detach(), polar.detach(), cell_e, thole, *entries, **kw).sum()
        out["virial"] = -torch.autograd.grad(es, eps)[0]
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def pair_tensor(R, a_i, a_j, thole):
    """The damped bare dipole-dipole tensor of one pair, (l3 / r^3) I - (3 l5 / r^5) R R^T [3, 3] (float64; -expm1 keeps l3 exact at small E)."""
    R = R.to(F64)
    r = torch.sqrt((R * R).sum())
    E = float(thole) * r**3 / (float(a_i) * float(a_j)) ** 0.5
    l3 = -torch.expm1(-E)
    l5 = l3 - E * torch.exp(-E)
    return l3 / r**3 * torch.eye(3, dtype=F64, device=R.device) - 3.0 * l5 / r**5 * torch.outer(R, R)


def damped_operator(pos, q, polar, cell, alpha, thole, entries, k_vectors=None, batch_idx=None, distance_dtype=F64, differentiable=False):
    """(T, c) of E_dip + E_thole (tests/induced_reference.quadratic_form): the parts of E_dip that are given (`entries` for the real-space
    sum, `k_vectors` for the explicit reciprocal sum) plus the Thole correction over the same entries.  `differentiable`: with respect to
    pos, q and polar."""
    if not differentiable:
        pos, q, polar = pos.detach(), q.detach(), polar.detach()
    pos, q = pos.to(F64), q.to(F64)
    cells = cell.detach().to(F64)

    def energy(mu):
        e = DR.energies(pos, q, mu, cells, alpha, entries, k_vectors, batch_idx=batch_idx, distance_dtype=distance_dtype).sum()
        return e + energies(pos, q, mu, polar, cells, thole, *entries, batch_idx=batch_idx, distance_dtype=distance_dtype).sum()

    return IR.quadratic_form(energy, pos.shape[0], pos.device, differentiable)
