"""Float64 torch restatement of the definition of `generalized_born` over explicit entries (i, j, S) of a full list, with autograd for every
derivative; checked on its own in tests/test_born_reference_cpu.py.  `descreen_quadrature` integrates the volume integral that defines I."""
import math

import numpy as np
import torch

OBC1, OBC2 = (0.8, 0.0, 2.909125), (1.0, 0.8, 4.85)


def descreen(r, rho, S):
    """I(r; rho, S), the closed form."""
    U, L = r + S, torch.maximum(rho, (r - S).abs())
    val = 0.5 * (1 / L - 1 / U + 0.25 * r * (1 / U**2 - 1 / L**2) + torch.log(L / U) / (2 * r) + S * S / (4 * r) * (1 / L**2 - 1 / U**2))
    val = val + torch.where(rho < S - r, 1 / rho - 1 / L, torch.zeros_like(val))
    return torch.where(U <= rho, torch.zeros_like(val), val)


def descreen_quadrature(r, rho, S, order=96):
    """(1/4pi) int |x|^-4 d^3x over the part of the sphere S at distance r outside the sphere rho: the shell of radius x about the origin
    lies inside the sphere where cos(theta) >= (x^2 + r^2 - S^2) / (2 x r), a fraction (1 - c) / 2 of it; Gauss-Legendre on each smooth piece."""
    frac = lambda x: 0.5 * (1 - np.clip((x * x + r * r - S * S) / (2 * x * r), -1, 1))  # noqa: E731
    t, w = np.polynomial.legendre.leggauss(order)
    cuts = sorted({min(max(c, rho), max(r + S, rho)) for c in (rho, abs(r - S), r + S)})
    total = 0.0
    for a, b in zip(cuts[:-1], cuts[1:]):
        x = 0.5 * (b - a) * t + 0.5 * (a + b)
        total += 0.5 * (b - a) * np.sum(w * frac(x) / x**2)
    return total


def entries(neighbor_matrix=None, shifts=None, mask_value=-1, neighbor_list=None):
    """(i, j, S) int64 CPU tensors of a matrix (padding removed) or of a [2, P] list."""
    if neighbor_list is not None:
        i, j = neighbor_list.cpu().long()
        S = torch.zeros((len(i), 3), dtype=torch.long) if shifts is None else shifts.cpu().long()
        return i, j, S
    nm = neighbor_matrix.cpu().long()
    keep = (nm != mask_value) & (nm >= 0) & (nm < nm.shape[0])
    i = torch.arange(nm.shape[0])[:, None].expand_as(nm)[keep]
    S = torch.zeros((len(i), 3), dtype=torch.long) if shifts is None else shifts.cpu().long()[keep]
    return i, nm[keep], S


def evaluate(pos, q, radii, screening, i, j, S=None, cell=None, batch_idx=None, weights=None, *, solute_dielectric=1.0, solvent_dielectric=78.5,
             coulomb_constant=1.0, offset=0.09, obc=OBC2, surface_tension=None, probe_radius=1.4):
    """dict of float64 CPU energies, forces, charge_grads, born_radii, virial [nsys, 3, 3] (and `loss` = sum_i w_i E_i, whose derivatives the
    forces, charge_grads and virial are; w = 1 without weights)."""
    f64 = lambda t: torch.as_tensor(t).detach().cpu().to(torch.float64)  # noqa: E731
    pos, q, R, scr = f64(pos).requires_grad_(True), f64(q).requires_grad_(True), f64(radii), f64(screening)
    n = pos.shape[0]
    cells = None if cell is None else f64(cell).reshape(-1, 3, 3)
    sys_i = torch.zeros(len(i), dtype=torch.long) if (batch_idx is None or cells is None) else batch_idx.cpu().long()[i]
    nsys = cells.shape[0] if (cells is not None and batch_idx is not None) else 1
    eps = torch.zeros((nsys, 3, 3), dtype=torch.float64, requires_grad=True)
    d = pos[j] - pos[i]
    if cells is not None and S is not None:
        d = d + torch.einsum("ea,eab->eb", S.to(torch.float64), cells[sys_i])
    d = d + torch.einsum("eab,eb->ea", eps[sys_i], d)
    r = d.norm(dim=1)
    rho = R - offset
    psi = rho * torch.zeros(n, dtype=torch.float64).index_add(0, i, descreen(r, rho[i], (scr * rho)[j]))
    a, b, c = obc
    born = 1 / (1 / rho - torch.tanh(a * psi - b * psi**2 + c * psi**3) / R)
    bb = born[i] * born[j]
    pair = q[i] * q[j] / torch.sqrt(r * r + bb * torch.exp(-r * r / (4 * bb)))
    pref = -0.5 * coulomb_constant * (1 / solute_dielectric - 1 / solvent_dielectric)
    e = pref * (q * q / born + torch.zeros(n, dtype=torch.float64).index_add(0, i, pair))
    if surface_tension is not None:
        e = e + 4 * math.pi * surface_tension * (R + probe_radius) ** 2 * (R / born) ** 6
    loss = e.sum() if weights is None else (f64(weights) * e).sum()
    gpos, gq, geps = torch.autograd.grad(loss, (pos, q, eps))
    return dict(energies=e.detach(), forces=-gpos, charge_grads=gq, born_radii=born.detach(), virial=-geps, loss=loss.detach())
