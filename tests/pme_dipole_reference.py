"""Torch restatement of the particle-mesh Ewald term for point dipoles, written from its definition (not from the kernels' expanded formulas).
Runs on the CPU in float64, or with `dtype=torch.float32` the same arithmetic in float32.

    frac = cell^-T r, m_d = frac_d n_d,  W_i(g) = prod_d M_p(p/2 + m_d - g_d) (periodic in g), M_p the cardinal B-spline of order p by its
    recursion  M_1 = 1 on [0, 1),  M_p(u) = [u M_{p-1}(u) + (p - u) M_{p-1}(u - 1)] / (p - 1)
    rho_q(g) = sum_i q_i W_i(g),   rho_mu(g) = sum_i mu_i . grad_{r_i} W_i(g)
    phi_X = IFFT[G FFT(rho_X) / sf^2]  (both transforms unscaled; the rfft half grid with Miller indices m_z >= 0),
        G = 2 pi exp(-k^2 / 4 alpha^2) / (k^2 V), 0 at k = 0,  k = 2 pi cell^-1 m,  sf^2 = max(prod_d sinc(m_d / n_d)^p, 1e-10)^2
    E_i = q_i W_i . phi_mu + mu_i . grad W_i . (phi_q + phi_mu) - 2 alpha^3 / (3 sqrt(pi)) |mu_i|^2

mu . grad W is not written out: the weights are evaluated at r_i + s_i mu_i and differentiated with respect to s_i at s = 0 by
`torch.autograd.grad(create_graph=True)` (for the spread, where a whole mesh is differentiated, by the double-backward form of a
Jacobian-vector product).  Every derivative output is autograd of the (weighted) summed energy; the virial is autograd with respect to an
explicit strain eps applied to positions and cell rows, x -> (I + eps) x, with the dipoles fixed in the laboratory frame."""
import math

import torch

F64 = torch.float64


def bspline(u, order):
    """Cardinal B-spline M_order(u), support [0, order), elementwise and differentiable in u."""
    m = [((u - k >= 0) & (u - k < 1)).to(u.dtype) for k in range(order)]  # M_1(u - k)
    for p in range(2, order + 1):
        m = [((u - k) * m[k] + (p - (u - k)) * m[k + 1]) / (p - 1) for k in range(order - p + 1)]
    return m[0]


def axis_weights(pos, cell, dims, order):
    """Three dense tensors [N, n_d]: M_p(p/2 + m_d - g) for every mesh index g of axis d, wrapped periodically (n_d >= p: one image)."""
    frac = pos @ torch.linalg.inv(cell)  # row vectors: cell^-T r
    out = []
    for d in range(3):
        g = torch.arange(dims[d], dtype=pos.dtype, device=pos.device)
        u = torch.remainder(order / 2.0 + frac[:, d:d + 1] * dims[d] - g[None, :], float(dims[d]))
        out.append(bspline(u, order))
    return out


def _mesh(values, w):
    return torch.einsum("i,ix,iy,iz->xyz", values, *w)


def _spread_gradient(pos, mu, cell, dims, order):
    """rho_mu(g) = sum_i d/ds_i W_i(g; r_i + s_i mu_i) at s = 0: the Jacobian-vector product by two backward passes."""
    s = torch.zeros(pos.shape[0], dtype=pos.dtype, requires_grad=True)
    w = axis_weights(pos + s[:, None] * mu, cell, dims, order)
    dense = _mesh(torch.ones_like(s), w)
    v = torch.ones_like(dense, requires_grad=True)
    (gs,) = torch.autograd.grad((dense * v).sum(), s, create_graph=True)
    (rho,) = torch.autograd.grad(gs.sum(), v, create_graph=True)
    return rho


def _influence(cell, alpha, dims, order):
    """G / sf^2 on the rfft half grid [nx, ny, nz/2 + 1]."""
    dt = cell.dtype
    nx, ny, nz = dims
    miller = lambda n: torch.tensor([i if i < (n + 1) // 2 else i - n for i in range(n)], dtype=dt)  # noqa: E731
    mx, my, mz = miller(nx), miller(ny), torch.arange(nz // 2 + 1, dtype=dt)
    m = torch.stack(torch.meshgrid(mx, my, mz, indexing="ij"), dim=-1)
    recip = 2.0 * math.pi * torch.linalg.inv(cell)  # k_c = sum_d recip[c][d] m_d
    k = torch.einsum("cd,xyzd->xyzc", recip, m)
    k2 = (k * k).sum(-1)
    origin = k2 < 1e-10
    k2s = torch.where(origin, torch.ones_like(k2), k2)
    vol = torch.abs(torch.linalg.det(cell))
    green = torch.where(origin, torch.zeros_like(k2), 2.0 * math.pi * torch.exp(-k2s / (4.0 * alpha * alpha)) / (k2s * vol))
    sinc = lambda x: torch.sinc(x)  # noqa: E731  (sin(pi x) / (pi x))
    sf = (sinc(m[..., 0] / nx) * sinc(m[..., 1] / ny) * sinc(m[..., 2] / nz)) ** order
    sf = torch.clamp(sf, min=1e-10)
    return green / (sf * sf)


def _solve(rho, infl, dims):
    return torch.fft.irfftn(torch.fft.rfftn(rho, norm="backward") * infl, s=tuple(dims), norm="forward")


def system_energies(pos, q, mu, cell, alpha, dims, order):
    """Per-atom mesh energies [n] of ONE system, self term included; differentiable in pos, q, mu, cell."""
    dims = tuple(int(v) for v in dims)
    infl = _influence(cell, alpha, dims, order)
    phi_q = _solve(_mesh(q, axis_weights(pos, cell, dims, order)), infl, dims)
    phi_mu = _solve(_spread_gradient(pos, mu, cell, dims, order), infl, dims)
    s = torch.zeros(pos.shape[0], dtype=pos.dtype, requires_grad=True)
    w = axis_weights(pos + s[:, None] * mu, cell, dims, order)
    at = lambda phi: torch.einsum("ix,iy,iz,xyz->i", *w, phi)  # noqa: E731  W_i . phi
    (dip,) = torch.autograd.grad(at(phi_q + phi_mu).sum(), s, create_graph=True)  # mu_i . grad W_i . phi_t
    c = 2.0 * alpha**3 / (3.0 * math.sqrt(math.pi))
    return q * at(phi_mu) + dip - c * (mu * mu).sum(-1)


def energies(pos, q, mu, cell, alpha, dims, order, batch_idx=None):
    """Per-atom energies [N]; cell [3, 3] or [B, 3, 3], alpha a number or [B] (atoms of one system need not be contiguous)."""
    cells = cell.reshape(-1, 3, 3)
    nsys = cells.shape[0]
    al = alpha.reshape(-1) if isinstance(alpha, torch.Tensor) else torch.tensor([float(alpha)], dtype=pos.dtype)
    al = al.to(pos.dtype).expand(nsys) if al.numel() == 1 else al.to(pos.dtype)
    if batch_idx is None:
        return system_energies(pos, q, mu, cells[0], al[0], dims, order)
    e = torch.zeros(pos.shape[0], dtype=pos.dtype)
    for b in range(nsys):
        own = torch.nonzero(batch_idx.long() == b).reshape(-1)
        if own.numel():
            e = e.index_add(0, own, system_energies(pos[own], q[own], mu[own], cells[b], al[b], dims, order))
    return e


def evaluate(pos, q, mu, cell, alpha, dims, order, batch_idx=None, weights=None, dtype=F64, virial=True):
    """dict of float64 numpy arrays: energies, forces (-dL/dr), charge_grads, dipole_grads of L = sum_i w_i E_i (w = 1 by default) and the
    virial [B, 3, 3] = -dE/d(strain) of the unweighted total, all evaluated in `dtype` on the CPU."""
    cpu = lambda t: t.detach().cpu().to(dtype)  # noqa: E731
    pos, q, mu = (cpu(t).clone().requires_grad_(True) for t in (pos, q, mu))
    cells = cpu(cell).reshape(-1, 3, 3)
    alpha = cpu(alpha) if isinstance(alpha, torch.Tensor) else float(alpha)
    bi = None if batch_idx is None else batch_idx.detach().cpu().long()
    e = energies(pos, q, mu, cells, alpha, dims, order, bi)
    loss = e.sum() if weights is None else (e * cpu(weights)).sum()
    grads = torch.autograd.grad(loss, [pos, q, mu])
    out = dict(energies=e.detach(), forces=-grads[0], charge_grads=grads[1], dipole_grads=grads[2])
    if virial:
        nsys = cells.shape[0]
        sys_of = torch.zeros(pos.shape[0], dtype=torch.long) if bi is None else bi
        eps = torch.zeros((nsys, 3, 3), dtype=dtype, requires_grad=True)
        defo = torch.eye(3, dtype=dtype) + eps  # x -> (I + eps) x: a row vector becomes x (I + eps)^T
        pos_e = torch.einsum("nb,nab->na", pos.detach(), defo[sys_of])
        cell_e = torch.einsum("srb,sab->sra", cells, defo)
        es = energies(pos_e, q.detach(), mu.detach(), cell_e, alpha, dims, order, bi).sum()
        out["virial"] = -torch.autograd.grad(es, eps)[0]
    return {k: v.detach().to(F64).numpy() for k, v in out.items()}


def half_spectrum_plane_virial(pos, q, mu, cell, alpha, dims, order, k):
    """[3, 3] numpy: what plane k of the rfft half spectrum adds to the k-space virial of ONE system per unit of its Hermitian weight,
        sum over the plane of (G / sf^2)(2 Re[conj(rho_q) rho_mu] + |rho_mu|^2)(delta_ab - 2 (1/k^2 + 1/(4 alpha^2)) k_a k_b).
    On an odd axis the last plane k = (nz - 1) / 2 has weight 2; the test cases use this to make sure that plane is visible in the virial."""
    dims = tuple(int(v) for v in dims)
    nx, ny, _ = dims
    rq = torch.fft.rfftn(_mesh(q, axis_weights(pos, cell, dims, order)))[:, :, k]
    rm = torch.fft.rfftn(_spread_gradient(pos, mu, cell, dims, order).detach())[:, :, k]
    e = _influence(cell, alpha, dims, order)[:, :, k] * (2.0 * (rq.conj() * rm).real + rm.abs() ** 2)
    miller = lambda n: torch.tensor([i if i < (n + 1) // 2 else i - n for i in range(n)], dtype=cell.dtype)  # noqa: E731
    m = torch.stack(torch.meshgrid(miller(nx), miller(ny), torch.tensor([float(k)], dtype=cell.dtype), indexing="ij"), dim=-1)[:, :, 0]
    kv = torch.einsum("cd,xyd->xyc", 2.0 * math.pi * torch.linalg.inv(cell), m)
    k2 = (kv * kv).sum(-1)
    out = torch.eye(3, dtype=cell.dtype) * e.sum() - 2.0 * torch.einsum("xy,xya,xyb->ab", e * (1.0 / k2 + 0.25 / (alpha * alpha)), kv, kv)
    return out.detach().numpy()
