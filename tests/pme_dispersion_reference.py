"""Torch restatement of the dispersion lattice sum on a mesh (LJ-PME), from its definition; tests/test_pme_dispersion_reference_cpu.py pins it.
Runs on the CPU in float64, or with `dtype=torch.float32` the same arithmetic in float32.

    W_i(g) = prod_d M_p(p/2 + m_d - g_d), the dense B-spline weights of tests/pme_dipole_reference.py (recursion, periodic wrap)
    rho = sum_i c_i W_i,   phi = IFFT_unscaled[D FFT(rho)]   (the rfft half grid with Miller indices m_z >= 0)
    D(m) = -(pi^1.5 beta^3 / (6 V)) f(b_m) / sf^2(m),  b = |k| / (2 beta),  f(b) = (1 - 2 b^2) exp(-b^2) + 2 sqrt(pi) b^3 erfc(b),  f(0) = 1
    k = 2 pi cell^-1 m,   sf^2 = max(prod_d sinc(m_d / n_d)^p, 1e-10)^2
    E_i = c_i W_i . phi + (beta^6 / 12) c_i^2

Forces and dE/dc are autograd of the (weighted) summed energy; the virial is autograd with respect to an explicit strain eps applied to
positions and cell rows, x -> (I + eps) x: fractional coordinates, mesh and beta stay, k and V follow the cell."""
import math

import torch

from tests.dispersion_ewald_reference import f_of_b
from tests.pme_dipole_reference import _mesh, _solve, axis_weights

F64 = torch.float64


def influence(cell, alpha, dims, order):
    """D on the rfft half grid [nx, ny, nz/2 + 1]; differentiable in the cell."""
    dt = cell.dtype
    nx, ny, nz = dims
    miller = lambda n: torch.tensor([i if i < (n + 1) // 2 else i - n for i in range(n)], dtype=dt)  # noqa: E731
    m = torch.stack(torch.meshgrid(miller(nx), miller(ny), torch.arange(nz // 2 + 1, dtype=dt), indexing="ij"), dim=-1)
    k = torch.einsum("cd,xyzd->xyzc", 2.0 * math.pi * torch.linalg.inv(cell), m)
    k2 = (k * k).sum(-1)
    origin = (m == 0).all(-1)
    b = torch.sqrt(torch.where(origin, torch.ones_like(k2), k2)) / (2.0 * alpha)  # (no square root at 0: its derivative is not finite)
    f = torch.where(origin, torch.ones_like(k2), f_of_b(b))
    sf = torch.clamp((torch.sinc(m[..., 0] / nx) * torch.sinc(m[..., 1] / ny) * torch.sinc(m[..., 2] / nz)) ** order, min=1e-10)
    return -(math.pi ** 1.5) * alpha ** 3 / (6.0 * torch.abs(torch.linalg.det(cell))) * f / (sf * sf)


def system_energies(pos, c, cell, alpha, dims, order):
    """Per-atom mesh energies [n] of ONE system, self term included; differentiable in pos, c, cell."""
    dims = tuple(int(v) for v in dims)
    w = axis_weights(pos, cell, dims, order)
    phi = _solve(_mesh(c, w), influence(cell, alpha, dims, order), dims)
    return c * torch.einsum("ix,iy,iz,xyz->i", *w, phi) + alpha ** 6 / 12.0 * c * c


def evaluate(pos, c, cell, alpha, dims, order, weights=None, dtype=F64, virial=True):
    """dict of float64 numpy arrays of ONE system: energies, forces (-dL/dr), coefficient_grads of L = sum_i w_i E_i (w = 1 by default) and
    the virial [1, 3, 3] = -dE/d(strain) of the unweighted total, all evaluated in `dtype` on the CPU."""
    cpu = lambda t: t.detach().cpu().to(dtype)  # noqa: E731
    pos, c = (cpu(t).clone().requires_grad_(True) for t in (pos, c))
    cell, alpha = cpu(cell).reshape(3, 3), float(alpha)
    e = system_energies(pos, c, cell, alpha, dims, order)
    grads = torch.autograd.grad(e.sum() if weights is None else (e * cpu(weights)).sum(), [pos, c])
    out = dict(energies=e.detach(), forces=-grads[0], coefficient_grads=grads[1])
    if virial:
        eps = torch.zeros((1, 3, 3), dtype=dtype, requires_grad=True)
        defo = torch.eye(3, dtype=dtype) + eps[0]  # x -> (I + eps) x: a row vector becomes x (I + eps)^T
        out["virial"] = -torch.autograd.grad(system_energies(pos.detach() @ defo.T, c.detach(), cell @ defo.T, alpha, dims, order).sum(), eps)[0]
    return {k: v.detach().to(F64).numpy() for k, v in out.items()}
