"""Torch restatement of the particle-mesh Ewald term for point quadrupoles, written from its definition (not from the kernels' expanded sums).
Runs on the CPU in float64, or with `dtype=torch.float32` the same arithmetic in float32.

    W_i(g) = prod_d M_p(p/2 + m_d - g_d), the B-spline weights of tests/pme_dipole_reference.py (`bspline`, `axis_weights`), and the mesh
    solve S[rho] = IFFT[G FFT(rho) / sf^2] of that file (`_influence`, `_solve`)
    l_i = q_i + mu_i . grad_i,   Theta_i = Q_i : grad_i grad_i   (Q_i = 1/2 (Q + Q^T) of what is given)
    rho_l = sum_i l_i W_i,  rho_T = sum_i Theta_i W_i,  phi_T = S[rho_T],  phi_L = S[rho_l] + phi_T
    E_i = l_i W_i . phi_T + Theta_i W_i . phi_L + the self term of tests/quadrupole_reference.py (`self_energies`)

Neither operator is written out: the weights are evaluated at r_i + d_i and l_i, Theta_i are applied by nested
`torch.autograd.grad(create_graph=True)` with respect to the per-atom displacement d_i at d = 0.  The dense meshes come from the
test-function trick of `_spread_gradient` there: the operators act on f_i = W_i . v for a test mesh v, and rho is the derivative of
sum_i (operator_i f_i) with respect to v.  Every derivative output is autograd of the (weighted) summed energy; the virial is autograd with
respect to an explicit strain eps applied to positions and cell rows, x -> (I + eps) x, with the multipoles fixed in the laboratory frame."""
import math

import torch

from tests.pme_dipole_reference import F64, _influence, _solve, axis_weights, bspline  # noqa: F401
from tests.quadrupole_reference import self_energies


def _sym(Q):
    return 0.5 * (Q + Q.transpose(-1, -2))


def _lin(f, d, q, mu):
    """l f = (q + mu . d/dd) f, per atom (f_i depends on d_i only)."""
    (g,) = torch.autograd.grad(f.sum(), d, create_graph=True)
    return q * f + (mu * g).sum(-1)


def _quad(f, d, Q):
    """Theta f = Q : d/dd d/dd f, per atom."""
    (g,) = torch.autograd.grad(f.sum(), d, create_graph=True)
    out = torch.zeros_like(f)
    for a in range(3):
        out = out + (Q[:, a, :] * torch.autograd.grad(g[:, a].sum(), d, create_graph=True)[0]).sum(-1)  # row a of the Hessian
    return out


def _at(pos, cell, dims, order):
    """(d, probe): probe(phi) = W_i(r_i + d_i) . phi per atom, differentiable in the displacement d [N, 3] (zero)."""
    d = torch.zeros_like(pos, requires_grad=True)
    w = axis_weights(pos + d, cell, dims, order)
    return d, lambda phi: torch.einsum("ix,iy,iz,xyz->i", *w, phi)


def spread(pos, cell, dims, order, op):
    """rho(g) = sum_i op_i W_i(g): `op(f, d)` applies the per-atom operator to f_i = W_i . v; rho is the derivative with respect to v."""
    d, probe = _at(pos, cell, dims, order)
    v = torch.ones(tuple(dims), dtype=pos.dtype, requires_grad=True)
    (rho,) = torch.autograd.grad(op(probe(v), d).sum(), v, create_graph=True)
    return rho


def densities(pos, q, mu, Q, cell, dims, order):
    """(rho_l, rho_T) of ONE system."""
    Qs = _sym(Q)
    return (spread(pos, cell, dims, order, lambda f, d: _lin(f, d, q, mu)), spread(pos, cell, dims, order, lambda f, d: _quad(f, d, Qs)))


def system_energies(pos, q, mu, Q, cell, alpha, dims, order, self_term=True):
    """Per-atom mesh energies [n] of ONE system, self term included; differentiable in pos, q, mu, Q, cell."""
    dims = tuple(int(v) for v in dims)
    Qs = _sym(Q)
    infl = _influence(cell, alpha, dims, order)
    rho_l, rho_t = densities(pos, q, mu, Qs, cell, dims, order)
    phi_t = _solve(rho_t, infl, dims)
    phi_l = _solve(rho_l, infl, dims) + phi_t
    d, probe = _at(pos, cell, dims, order)
    e = _lin(probe(phi_t), d, q, mu) + _quad(probe(phi_l), d, Qs)
    if self_term:
        al = torch.as_tensor(alpha, dtype=F64).reshape(-1)[:1].expand(pos.shape[0])
        e = e + self_energies(q, mu, Qs, al).to(pos.dtype)
    return e


def energies(pos, q, mu, Q, cell, alpha, dims, order, batch_idx=None):
    """Per-atom energies [N]; cell [3, 3] or [B, 3, 3], alpha a number or [B] (atoms of one system need not be contiguous)."""
    cells = cell.reshape(-1, 3, 3)
    nsys = cells.shape[0]
    al = alpha.reshape(-1) if isinstance(alpha, torch.Tensor) else torch.tensor([float(alpha)], dtype=pos.dtype)
    al = al.to(pos.dtype).expand(nsys) if al.numel() == 1 else al.to(pos.dtype)
    if batch_idx is None:
        return system_energies(pos, q, mu, Q, cells[0], al[0], dims, order)
    e = torch.zeros(pos.shape[0], dtype=pos.dtype)
    for b in range(nsys):
        own = torch.nonzero(batch_idx.long() == b).reshape(-1)
        if own.numel():
            e = e.index_add(0, own, system_energies(pos[own], q[own], mu[own], Q[own], cells[b], al[b], dims, order))
    return e


def evaluate(pos, q, mu, Q, cell, alpha, dims, order, batch_idx=None, weights=None, dtype=F64, virial=True):
    """dict of float64 numpy arrays: energies, forces (-dL/dr), charge_grads, dipole_grads, quadrupole_grads of L = sum_i w_i E_i (w = 1 by
    default) and the virial [B, 3, 3] = -dE/d(strain) of the unweighted total, all evaluated in `dtype` on the CPU.  quadrupole_grads is the
    derivative with respect to the nine words of the input, which enters as 1/2 (Q + Q^T): it is symmetric."""
    cpu = lambda t: t.detach().cpu().to(dtype)  # noqa: E731
    pos, q, mu, Q = (cpu(t).clone().requires_grad_(True) for t in (pos, q, mu, Q))
    cells = cpu(cell).reshape(-1, 3, 3)
    alpha = cpu(alpha) if isinstance(alpha, torch.Tensor) else float(alpha)
    bi = None if batch_idx is None else batch_idx.detach().cpu().long()
    e = energies(pos, q, mu, Q, cells, alpha, dims, order, bi)
    loss = e.sum() if weights is None else (e * cpu(weights)).sum()
    grads = torch.autograd.grad(loss, [pos, q, mu, Q])
    out = dict(energies=e.detach(), forces=-grads[0], charge_grads=grads[1], dipole_grads=grads[2], quadrupole_grads=grads[3])
    if virial:
        nsys = cells.shape[0]
        sys_of = torch.zeros(pos.shape[0], dtype=torch.long) if bi is None else bi
        eps = torch.zeros((nsys, 3, 3), dtype=dtype, requires_grad=True)
        defo = torch.eye(3, dtype=dtype) + eps  # x -> (I + eps) x: a row vector becomes x (I + eps)^T
        pos_e = torch.einsum("nb,nab->na", pos.detach(), defo[sys_of])
        cell_e = torch.einsum("srb,sab->sra", cells, defo)
        es = energies(pos_e, q.detach(), mu.detach(), Q.detach(), cell_e, alpha, dims, order, bi).sum()
        out["virial"] = -torch.autograd.grad(es, eps)[0]
    return {k: v.detach().to(F64).numpy() for k, v in out.items()}


def closed_virial(pos, q, mu, Q, cell, alpha, dims, order):
    """[3, 3] numpy: the virial of ONE system by the closed formula the device code uses,
        W_ab = sum_m E_m (delta_ab - 2 (1/k^2 + 1/(4 alpha^2)) k_a k_b) + sum_i (dE/dmu_i)_a mu_i,b + 2 sum_i (G_i Q_i)_ab,
        E_m = h_m G_m (2 Re[conj(rho_l) rho_T] + |rho_T|^2) / sf2_m over the rfft half grid, h = 1 on the planes m_z = 0 and (even n_z) n_z / 2,
        2 elsewhere;  G_i = dE/dQ_i without its self terms (the derivative of the energy without the self term)."""
    dims = tuple(int(v) for v in dims)
    nx, ny, nz = dims
    Qs = _sym(Q)
    rho_l, rho_t = densities(pos, q, mu, Qs, cell, dims, order)
    sl, st = torch.fft.rfftn(rho_l.detach()), torch.fft.rfftn(rho_t.detach())
    h = torch.full((nz // 2 + 1,), 2.0, dtype=cell.dtype)
    h[0] = 1.0
    if nz % 2 == 0:
        h[-1] = 1.0
    e = _influence(cell, alpha, dims, order) * (2.0 * (sl.conj() * st).real + st.abs() ** 2) * h
    miller = lambda n: torch.tensor([i if i < (n + 1) // 2 else i - n for i in range(n)], dtype=cell.dtype)  # noqa: E731
    m = torch.stack(torch.meshgrid(miller(nx), miller(ny), torch.arange(nz // 2 + 1, dtype=cell.dtype), indexing="ij"), dim=-1)
    kv = torch.einsum("cd,xyzd->xyzc", 2.0 * math.pi * torch.linalg.inv(cell), m)
    k2 = (kv * kv).sum(-1)
    k2 = torch.where(k2 < 1e-10, torch.ones_like(k2), k2)  # E_m is 0 there
    out = torch.eye(3, dtype=cell.dtype) * e.sum() - 2.0 * torch.einsum("xyz,xyza,xyzb->ab", e * (1.0 / k2 + 0.25 / (alpha * alpha)), kv, kv)
    mu_, Q_ = mu.detach().clone().requires_grad_(True), Qs.detach().clone().requires_grad_(True)
    total = system_energies(pos.detach(), q.detach(), mu_, Q_, cell, alpha, dims, order, self_term=False).sum()
    gmu, gq = torch.autograd.grad(total, [mu_, Q_])
    gq = _sym(gq)
    out = out + torch.einsum("ia,ib->ab", gmu, mu.detach()) + 2.0 * torch.einsum("iac,icb->ab", gq, Qs.detach())
    return out.detach().numpy()


def half_spectrum_plane_virial(pos, q, mu, Q, cell, alpha, dims, order, k):
    """[3, 3] numpy: what plane k of the rfft half spectrum adds to the k-space virial of ONE system per unit of its Hermitian weight,
        sum over the plane of (G / sf^2)(2 Re[conj(rho_l) rho_T] + |rho_T|^2)(delta_ab - 2 (1/k^2 + 1/(4 alpha^2)) k_a k_b),
    the first sum of `closed_virial` restricted to one plane (the twin of `pme_dipole_reference.half_spectrum_plane_virial`).  On an odd axis
    the last plane k = (nz - 1) / 2 has weight 2; the test cases use this to make sure that plane is visible in the virial."""
    dims = tuple(int(v) for v in dims)
    nx, ny, _ = dims
    rho_l, rho_t = densities(pos, q, mu, _sym(Q), cell, dims, order)
    sl, st = torch.fft.rfftn(rho_l.detach())[:, :, k], torch.fft.rfftn(rho_t.detach())[:, :, k]
    e = _influence(cell, alpha, dims, order)[:, :, k] * (2.0 * (sl.conj() * st).real + st.abs() ** 2)
    miller = lambda n: torch.tensor([i if i < (n + 1) // 2 else i - n for i in range(n)], dtype=cell.dtype)  # noqa: E731
    m = torch.stack(torch.meshgrid(miller(nx), miller(ny), torch.tensor([float(k)], dtype=cell.dtype), indexing="ij"), dim=-1)[:, :, 0]
    kv = torch.einsum("cd,xyd->xyc", 2.0 * math.pi * torch.linalg.inv(cell), m)
    k2 = (kv * kv).sum(-1)
    k2 = torch.where(k2 < 1e-10, torch.ones_like(k2), k2)  # e is 0 there
    out = torch.eye(3, dtype=cell.dtype) * e.sum() - 2.0 * torch.einsum("xy,xya,xyb->ab", e * (1.0 / k2 + 0.25 / (alpha * alpha)), kv, kv)
    return out.detach().numpy()
