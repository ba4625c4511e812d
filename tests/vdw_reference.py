"""Float64 torch restatement of `buffered_14_7` / `lennard_jones` from their definition: sites, entries, U, T, s and 1/2 per end.

    E_i = 1/2 sum_{entries (i, j, S) of row i} s_e T(r) U_ij(r),   d = site_j - site_i + S . cell,  r = |d|,  rho = r / R_ij

Derivatives come from autograd (the virial is the strain derivative, cell and positions strained together).  `distance_dtype=float32` rounds
site positions, pair vector and r^2 to float32 as the kernel does, derivatives still flowing through the float64 expressions; `nudge_r2`
moves every float32 r^2 by one ulp: what the float32 bar of tests/test_vdw_gpu.py is measured with."""
import torch

F64 = torch.float64
KINDS = ("buffered_14_7", "lennard_jones")


def entries_from_matrix(neighbor_matrix, shifts, mask_value, scales=None):
    """(i, j, S, s) of a padded matrix: entries equal to mask_value or outside [0, N) are padding."""
    nm = neighbor_matrix.long()
    n, m = nm.shape
    keep = (nm != int(mask_value)) & (nm >= 0) & (nm < n)
    i = torch.arange(n, device=nm.device).unsqueeze(1).expand(n, m)[keep]
    S = torch.zeros((n, m, 3), dtype=torch.long, device=nm.device) if shifts is None else shifts.long()
    return i, nm[keep], S[keep], None if scales is None else scales[keep].to(F64)


def site_positions(pos, cells, sys_of, sites):
    """site_i = r_i - (1 - kappa_i) (r_i - r_p) at the atom's own image, r_i - r_p the minimum image with a cell; sites = (parent, reduction) | None."""
    if sites is None:
        return pos
    own, par = torch.arange(pos.shape[0], device=pos.device), sites[0].long()
    reduced = (par >= 0) & (par < pos.shape[0]) & (par != own)
    p = torch.where(reduced, par, own)
    d = pos - pos[p]
    if cells is not None:
        c = cells[sys_of]
        images = torch.round(torch.einsum("na,nab->nb", d.detach(), torch.linalg.inv(c.detach())))
        d = d - torch.einsum("na,nab->nb", images, c)
    return pos - torch.where(reduced, 1.0 - sites[1].to(F64), torch.zeros_like(d[:, 0]))[:, None] * d


def combine(radii, eps, i, j, radius_rule, epsilon_rule):
    a, b, ea, eb = radii[i], radii[j], eps[i], eps[j]
    R = {"arithmetic": 0.5 * (a + b), "geometric": torch.sqrt(a * b), "cubic-mean": (a ** 3 + b ** 3) / (a ** 2 + b ** 2)}[radius_rule]
    return R, {"geometric": torch.sqrt(ea * eb), "hhg": 4.0 * ea * eb / (torch.sqrt(ea) + torch.sqrt(eb)) ** 2}[epsilon_rule]


def potential(kind, rho, delta=0.07, gamma=0.12):  # U / eps_ij
    if kind == "buffered_14_7":
        return ((1.0 + delta) / (rho + delta)) ** 7 * ((1.0 + gamma) / (rho ** 7 + gamma) - 2.0)
    return rho ** -12 - 2.0 * rho ** -6


def switch(r, cutoff, taper):
    t = torch.zeros_like(r) if taper is None else torch.clamp((r - taper) / (cutoff - taper), min=0.0)
    return 1.0 - 10.0 * t ** 3 + 15.0 * t ** 4 - 6.0 * t ** 5


def energies(kind, pos, radii, eps, cell, i, j, S, scales=None, *, cutoff, taper=None, sites=None, delta=0.07, gamma=0.12,
             radius_rule="cubic-mean", epsilon_rule="hhg", batch_idx=None, distance_dtype=F64, nudge_r2=False):
    """Per-atom float64 energies (differentiable in pos, radii, eps, cell).  cell: [3, 3] / [B, 3, 3] or None."""
    n = pos.shape[0]
    sys_of = torch.zeros(n, dtype=torch.long, device=pos.device) if batch_idx is None else batch_idx.long()
    cells = None if cell is None else cell.reshape(-1, 3, 3)
    site = site_positions(pos, cells, sys_of, sites)

    def pair_vectors(dtype, p, c):
        v = p.to(dtype)[j] - p.to(dtype)[i]
        return v if c is None else v + torch.einsum("ea,eab->eb", S.to(dtype), c.to(dtype)[sys_of[i]])

    rvec = pair_vectors(F64, site, cells)
    r2 = (rvec * rvec).sum(-1)
    if distance_dtype != F64:
        low = pair_vectors(distance_dtype, site.detach(), None if cells is None else cells.detach())
        low_r2 = (low * low).sum(-1)
        if nudge_r2:
            low_r2 = torch.nextafter(low_r2, torch.full_like(low_r2, float("inf")))
        rvec = rvec + (low.to(F64) - rvec).detach()
        r2 = (rvec * rvec).sum(-1)
        r2 = r2 + (low_r2.to(F64) - r2).detach()
    valid = (radii > 0) & (eps > 0)
    one = torch.ones_like(radii)
    R, e = combine(torch.where(valid, radii, one), torch.where(valid, eps, one), i, j, radius_rule, epsilon_rule)
    keep = valid[i] & valid[j] & (r2 < cutoff * cutoff) & (r2 > 1e-16)
    r = torch.sqrt(torch.where(keep, r2, torch.ones_like(r2)))
    pair = e * switch(r, cutoff, taper) * potential(kind, r / R, delta, gamma)
    if scales is not None:
        pair = pair * scales
    return torch.zeros(n, dtype=F64, device=pos.device).index_add(0, i, 0.5 * torch.where(keep, pair, torch.zeros_like(pair)))


def evaluate(kind, pos, radii, eps, cell, i, j, S, scales=None, batch_idx=None, **kw):
    """dict of float64 tensors: energies, forces (-dE/dr on atoms), radius_grads, epsilon_grads, virial [B, 3, 3] = -dE/d(strain) | None."""
    pos = pos.detach().to(F64).clone().requires_grad_(True)
    radii = radii.detach().to(F64).clone().requires_grad_(True)
    eps = eps.detach().to(F64).clone().requires_grad_(True)
    cell = None if cell is None else cell.detach().to(F64)
    e = energies(kind, pos, radii, eps, cell, i, j, S, scales, batch_idx=batch_idx, **kw)
    grads = torch.autograd.grad(e.sum(), [pos, radii, eps])
    out = dict(energies=e.detach(), forces=-grads[0], radius_grads=grads[1], epsilon_grads=grads[2], virial=None)
    if cell is not None:
        cells = cell.reshape(-1, 3, 3)
        sys_of = torch.zeros(pos.shape[0], dtype=torch.long, device=pos.device) if batch_idx is None else batch_idx.long()
        strain = torch.zeros((cells.shape[0], 3, 3), dtype=F64, device=pos.device, requires_grad=True)
        defo = torch.eye(3, dtype=F64, device=pos.device) + strain  # x -> (I + eps) x: a row vector becomes x (I + eps)^T
        pos_e = torch.einsum("nb,nab->na", pos.detach(), defo[sys_of])
        cell_e = torch.einsum("srb,sab->sra", cells, defo)
        es = energies(kind, pos_e, radii.detach(), eps.detach(), cell_e, i, j, S, scales, batch_idx=batch_idx, **kw).sum()
        out["virial"] = -torch.autograd.grad(es, strain)[0]
    return out
