"""Float64 torch yardstick of `dipole_pair_scale_correction` and of the scaled induced-dipole solves, written from the definition.  Works on
the stored entries (i, j, S) of a full list with two scales per entry; runs on any device.

    E_i = 1/2 sum_{entries of row i} [ (s^d - 1) l3 / r^3 (q_j c_i - q_i c_j) + (s^m - 1) (l3 / r^3 mu_i . mu_j - 3 l5 / r^5 c_i c_j) ]

R = r_j - r_i + S . cell (or its minimum image), c = mu . R, l3 / l5 the `lambdas` of tests/thole_reference.py at E = a_T r^3 / sqrt(a_i a_j)
where a width is given and both ends are polarisable (a > 0), 1 otherwise.  There is NO cut at large E here.  Pair vectors, the
float32-distance mode and the skipped entries (r <= 1e-8, both scales 1) are those of tests/pair_scale_reference.py; every derivative comes
from autograd, the virial from an explicit strain.  `scaled_operator` is the dense (T, c) of an existing reference energy plus this term.
"""
import torch

from tests import induced_reference as IR
from tests import thole_reference as TR
from tests.dipole_reference import F64, _systems
from tests.pair_scale_reference import _pair_vectors_of


def pair_energies(pos, q, mu, polar, sd, sm, i, j, S, cell=None, thole=None, batch_idx=None, distance_dtype=F64, minimum_image=False):
    """Per-atom float64 energies (differentiable in pos, q, mu, polar, cell).  sd / sm: one scale per entry."""
    n, dev = pos.shape[0], pos.device
    cells = torch.eye(3, dtype=F64, device=dev).reshape(1, 3, 3) if cell is None else cell.reshape(-1, 3, 3)
    sys_of = _systems(n, batch_idx if cell is not None else None, dev)
    rvec = _pair_vectors_of(pos.to(F64), cells.to(F64), i, j, S, sys_of, minimum_image)
    low = None
    if distance_dtype != F64:
        if minimum_image:  # the float64 reduction of the low-precision positions and cell, rounded once
            low = _pair_vectors_of(pos.detach().to(distance_dtype).to(F64), cells.detach().to(distance_dtype).to(F64), i, j, S, sys_of,
                                   True).to(distance_dtype)
        else:
            low = _pair_vectors_of(pos.detach().to(distance_dtype), cells.detach().to(distance_dtype), i, j, S, sys_of, False)
        rvec = rvec + (low.to(F64) - rvec).detach()
    r_val = torch.sqrt((rvec.detach() ** 2).sum(-1)) if low is None else torch.sqrt((low * low).sum(-1)).to(F64)
    sd, sm = sd.detach().to(F64), sm.detach().to(F64)
    keep = (r_val > 1e-8) & ((sd != 1.0) | (sm != 1.0))
    unit = torch.zeros_like(rvec)
    unit[:, 0] = 1.0
    rv = torch.where(keep.unsqueeze(1), rvec, unit)  # skipped entries: a harmless vector, no gradient to the positions
    r = torch.sqrt((rv * rv).sum(-1))
    if low is not None:
        r = r + (torch.where(keep, r_val, torch.ones_like(r_val)) - r).detach()
    l3 = l5 = torch.ones_like(r)
    if thole is not None:
        a = polar.to(F64)
        ok = a > 0  # (NaN: not polarisable)
        safe = torch.where(ok, a, torch.ones_like(a))
        d3, d5, _ = TR.lambdas(float(thole) * r**3 / torch.sqrt(safe[i] * safe[j]))
        damped = ok[i] & ok[j]
        l3, l5 = torch.where(damped, d3, l3), torch.where(damped, d5, l5)
    q, mu = q.to(F64), mu.to(F64)
    ci, cj = (mu[i] * rv).sum(-1), (mu[j] * rv).sum(-1)
    pair = (sd - 1.0) * l3 / r**3 * (q[j] * ci - q[i] * cj) + (sm - 1.0) * (l3 / r**3 * (mu[i] * mu[j]).sum(-1) - 3.0 * l5 / r**5 * ci * cj)
    pair = torch.where(keep, pair, torch.zeros_like(pair))
    return torch.zeros(n, dtype=F64, device=dev).index_add(0, i, 0.5 * pair)


def evaluate(pos, q, mu, polar, sd, sm, entries, cell=None, thole=None, batch_idx=None, distance_dtype=F64, weights=None, minimum_image=False):
    """dict of float64 numpy arrays: energies, forces (-dL/dr), charge_grads, dipole_grads, polar_grads of L = sum_i w_i E_i (w = 1 by
    default) and, with a cell, the virial [B, 3, 3] = -dE/d(strain) of the unweighted total."""
    n, dev = pos.shape[0], pos.device
    leaves = [t.detach().to(F64).clone().requires_grad_(True) for t in (pos, q, mu, polar)]
    cells = None if cell is None else cell.detach().to(F64).reshape(-1, 3, 3)
    kw = dict(thole=thole, batch_idx=batch_idx, distance_dtype=distance_dtype, minimum_image=minimum_image)
    e = pair_energies(*leaves, sd, sm, *entries, cell=cells, **kw)
    loss = e.sum() if weights is None else (e * weights.to(F64)).sum()
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else torch.nan_to_num(g) for g, t in zip(grads, leaves)]
    out = dict(energies=e.detach(), forces=-grads[0], charge_grads=grads[1], dipole_grads=grads[2], polar_grads=grads[3])
    if cells is not None:
        sys_of = _systems(n, batch_idx, dev)
        eps = torch.zeros((cells.shape[0], 3, 3), dtype=F64, device=dev, requires_grad=True)
        defo = torch.eye(3, dtype=F64, device=dev) + eps  # x -> (I + eps) x: a row vector becomes x (I + eps)^T
        pos_e = torch.einsum("nb,nab->na", leaves[0].detach(), defo[sys_of])
        cell_e = torch.einsum("srb,sab->sra", cells, defo)
        es = pair_energies(pos_e, *[t.detach() for t in leaves[1:]], sd, sm, *entries, cell=cell_e, **kw).sum()
        out["virial"] = -torch.autograd.grad(es, eps)[0]
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def scaled_operator(base_energy, pos, q, polar, sd, sm, entries, cell=None, thole=None, batch_idx=None, minimum_image=False,
                    differentiable=False):
    """(T [3n, 3n], c [n, 3]): the exact Hessian in mu, and the gradient at mu = 0, of `base_energy(mu)` (an existing reference total) plus
    the scaled-pair term.  H_ref = `induced_reference.system_matrix(T, polar)`."""
    def energy(mu):
        return base_energy(mu) + pair_energies(pos, q, mu, polar, sd, sm, *entries, cell=cell, thole=thole, batch_idx=batch_idx,
                                               minimum_image=minimum_image).sum()

    return IR.quadratic_form(energy, pos.shape[0], pos.device, differentiable)
