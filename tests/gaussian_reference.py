"""Float64 torch restatement of the Gaussian-smeared charge correction, written from its definition (not from the kernel), plus the exact
sums it is checked against.  Works on stored entries (i, j, S) of a full neighbour list; runs on any device.

    s_i = max(sigma_i, 0)^2,  g_ij = sqrt(2 (s_i + s_j)),  r = r_j - r_i + S . cell,  x = r / g_ij
    E_i = -1/2 sum_{entries of row i} q_i q_j erfc(x) / r                         entries with r <= 1e-8, x >= 6 or g_ij = 0 skipped
          + q_i^2 / (2 sqrt(pi) sigma_i)             if self_energy and sigma_i > 0
          + (2 pi / V_s) Q_s q_i s_i                 if background and a cell is given

Gradients come from autograd, the virial from autograd with respect to a strain eps (x -> (I + eps) x applied to positions and cell rows).
`distance_dtype=torch.float32` forms the pair vector and the distance in float32 and everything after that in float64: the kernel's
arithmetic model for float32 inputs.
"""
import math

import numpy as np
import torch

F64 = torch.float64


def entries_from_matrix(neighbor_matrix, shifts, mask_value):
    """(i, j, S) of a padded matrix: entries equal to mask_value or outside [0, N) are padding."""
    nm = neighbor_matrix.long()
    n, m = nm.shape
    keep = (nm != int(mask_value)) & (nm >= 0) & (nm < n)
    i = torch.arange(n, device=nm.device).unsqueeze(1).expand(n, m)[keep]
    s = torch.zeros((n, m, 3), dtype=torch.long, device=nm.device) if shifts is None else shifts.long()
    return i, nm[keep], s[keep]


def entries_from_csr(neighbor_list, neighbor_ptr, shifts):
    j = neighbor_list[1].long()
    counts = (neighbor_ptr[1:] - neighbor_ptr[:-1]).long()
    i = torch.repeat_interleave(torch.arange(counts.shape[0], device=j.device), counts)
    s = torch.zeros((j.shape[0], 3), dtype=torch.long, device=j.device) if shifts is None else shifts.long()
    return i, j, s


def brute_force_entries(pos, cell, cutoff, images):
    """Every (i, j, S) with 1e-12 < |r_j - r_i + S . cell| < cutoff, S in [-images, images]^3 (numpy in, torch out): a full list."""
    rng = np.arange(-images, images + 1)
    S = np.array([(a, b, c) for a in rng for b in rng for c in rng])
    d = pos[None, :, None, :] - pos[:, None, None, :] + (S @ cell)[None, None, :, :]
    r = np.linalg.norm(d, axis=-1)
    i, j, k = np.nonzero((r < cutoff) & (r > 1e-12))
    return torch.as_tensor(i), torch.as_tensor(j), torch.as_tensor(S[k])


def energies(pos, q, sigma, cell, i, j, S, batch_idx=None, self_energy=True, background=True, distance_dtype=F64):
    """Per-atom float64 energies (differentiable in pos, q, sigma, cell).  cell: [3,3] / [B,3,3] or None."""
    n = pos.shape[0]
    sys_of = torch.zeros(n, dtype=torch.long, device=pos.device) if batch_idx is None else batch_idx.long()
    cells = None if cell is None else cell.reshape(-1, 3, 3)
    def pair_vectors(dtype, p, c):
        v = p.to(dtype)[j] - p.to(dtype)[i]
        return v if c is None else v + torch.einsum("ea,eab->eb", S.to(dtype), c.to(dtype)[sys_of[i]])

    rvec = pair_vectors(F64, pos, cells)
    low = None
    if distance_dtype != F64:
        # the VALUES of the pair vector and of the distance are those of the low-precision arithmetic; derivatives keep flowing through the
        # float64 expressions (value + detached difference), so gradients are accumulated in float64 as everything else is
        low = pair_vectors(distance_dtype, pos.detach(), None if cells is None else cells.detach())
        rvec = rvec + (low.to(F64) - rvec).detach()
    r2 = (rvec * rvec).sum(-1)
    ok_r = r2 > 0
    r = torch.sqrt(torch.where(ok_r, r2, torch.ones_like(r2)))
    if low is not None:
        r = r + (torch.sqrt((low * low).sum(-1)).to(F64) - r).detach()
    r = torch.where(ok_r, r, torch.zeros_like(r))
    q, sigma = q.to(F64), sigma.to(F64)
    s = torch.clamp(sigma, min=0.0) ** 2
    g2 = 2.0 * (s[i] + s[j])
    ok_g = g2 > 0
    gam = torch.sqrt(torch.where(ok_g, g2, torch.ones_like(g2)))
    x = r / gam
    keep = ok_g & (r > 1e-8) & (x < 6.0)
    r_safe = torch.where(keep, r, torch.ones_like(r))
    x_safe = torch.where(keep, x, torch.ones_like(x))
    pair = torch.where(keep, -0.5 * q[i] * q[j] * torch.erfc(x_safe) / r_safe, torch.zeros_like(r))
    e = torch.zeros(n, dtype=F64, device=pos.device).index_add(0, i, pair)
    if self_energy:
        smeared = sigma > 0
        e = e + torch.where(smeared, q * q / (2.0 * math.sqrt(math.pi) * torch.where(smeared, sigma, torch.ones_like(sigma))), torch.zeros_like(q))
    if background and cells is not None:
        e = e + background_energies(q, s, cells, sys_of)
    return e


def background_energies(q, s, cells, sys_of):
    nsys = cells.shape[0]
    vol = torch.abs(torch.linalg.det(cells.to(F64)))
    qsum = torch.zeros(nsys, dtype=F64, device=q.device).index_add(0, sys_of, q)
    return (2.0 * math.pi / vol * qsum)[sys_of] * q * s


def evaluate(pos, q, sigma, cell, i, j, S, batch_idx=None, self_energy=True, background=True, distance_dtype=F64, weights=None):
    """dict of float64 numpy arrays: energies, forces (-dL/dr), charge_grads, sigma_grads, cell_grads (None without a cell) of
    L = sum_i w_i E_i (w = 1 by default), and the virial [B,3,3] = -dE/d(strain) of the unweighted total (None without a cell)."""
    pos = pos.detach().to(F64).clone().requires_grad_(True)
    q = q.detach().to(F64).clone().requires_grad_(True)
    sigma = sigma.detach().to(F64).clone().requires_grad_(True)
    cell = None if cell is None else cell.detach().to(F64).clone().requires_grad_(True)
    kw = dict(batch_idx=batch_idx, self_energy=self_energy, background=background, distance_dtype=distance_dtype)
    e = energies(pos, q, sigma, cell, i, j, S, **kw)
    loss = e.sum() if weights is None else (e * weights.to(F64)).sum()
    grads = torch.autograd.grad(loss, [pos, q, sigma] + ([cell] if cell is not None else []))
    out = dict(energies=e.detach(), forces=-grads[0], charge_grads=grads[1], sigma_grads=grads[2], cell_grads=grads[3] if cell is not None else None,
               virial=None)
    if cell is not None:
        cells = cell.detach().reshape(-1, 3, 3)
        nsys = cells.shape[0]
        sys_of = torch.zeros(pos.shape[0], dtype=torch.long, device=pos.device) if batch_idx is None else batch_idx.long()
        eps = torch.zeros((nsys, 3, 3), dtype=F64, device=pos.device, requires_grad=True)
        defo = torch.eye(3, dtype=F64, device=pos.device) + eps  # x -> (I + eps) x: a row vector becomes x (I + eps)^T
        pos_e = torch.einsum("nb,nab->na", pos.detach(), defo[sys_of])
        cell_e = torch.einsum("srb,sab->sra", cells, defo)
        es = energies(pos_e, q.detach(), sigma.detach(), cell_e, i, j, S, **kw).sum()
        out["virial"] = -torch.autograd.grad(es, eps)[0]
    return {k: (None if v is None else v.detach().cpu().numpy()) for k, v in out.items()}


# ---- exact sums (numpy, float64, math.erfc) -------------------------------------------------------------------------------------------
_erfc = np.vectorize(math.erfc)


def _k_vectors(cell, kmax_index):
    rec = 2.0 * np.pi * np.linalg.inv(cell).T  # rows: reciprocal vectors
    rng = np.arange(-kmax_index, kmax_index + 1)
    m = np.stack(np.meshgrid(rng, rng, rng, indexing="ij"), axis=-1).reshape(-1, 3)
    return m[np.any(m != 0, axis=1)] @ rec


def _structure_factor_sum(k, pos, weight_of_k2, green_of_k2, chunk=20000):
    """sum_k green(k^2) |sum_i w_i(k^2) exp(i k.r_i)|^2, in chunks of k-vectors (bounded memory)."""
    total = 0.0
    for a in range(0, k.shape[0], chunk):
        kc = k[a:a + chunk]
        k2 = (kc * kc).sum(-1)
        w = weight_of_k2(k2)
        ph = kc @ pos.T
        sr, si = (np.cos(ph) * w).sum(-1), (np.sin(ph) * w).sum(-1)
        total += np.sum(green_of_k2(k2) * (sr * sr + si * si))
    return total


def point_charge_ewald_exact(pos, q, cell, alpha, images, kmax_index):
    """Total point-charge Ewald energy with exact erfc: real-space images in [-images, images]^3, k indices in [-kmax_index, kmax_index]^3,
    self term and the neutralising-background term -pi Q^2 / (2 alpha^2 V)."""
    vol = abs(np.linalg.det(cell))
    rng = np.arange(-images, images + 1)
    S = np.array([(a, b, c) for a in rng for b in rng for c in rng])
    d = pos[None, :, None, :] - pos[:, None, None, :] + (S @ cell)[None, None, :, :]
    r = np.linalg.norm(d, axis=-1)
    mask = r > 1e-12
    rs = np.where(mask, r, 1.0)
    real = 0.5 * np.sum(np.where(mask, (q[:, None, None] * q[None, :, None]) * _erfc(alpha * rs) / rs, 0.0))
    recip = 2.0 * np.pi / vol * _structure_factor_sum(_k_vectors(cell, kmax_index), pos, lambda k2: q[None, :],
                                                      lambda k2: np.exp(-k2 / (4.0 * alpha * alpha)) / k2)
    return real + recip - alpha / math.sqrt(math.pi) * np.sum(q * q) - math.pi * q.sum() ** 2 / (2.0 * alpha * alpha * vol)


def gaussian_kspace_exact(pos, q, sigma, cell, kmax_index):
    """(2 pi / V) sum_{k != 0} |sum_i q_i exp(-k^2 sigma_i^2 / 2) exp(i k.r_i)|^2 / k^2: the exact energy of periodic Gaussian charges
    (all sigma > 0) in a neutralising background, self-interaction of every cloud included.  No erfc anywhere."""
    vol = abs(np.linalg.det(cell))
    return 2.0 * np.pi / vol * _structure_factor_sum(_k_vectors(cell, kmax_index), pos,
                                                     lambda k2: q[None, :] * np.exp(-0.5 * k2[:, None] * (sigma * sigma)[None, :]), lambda k2: 1.0 / k2)
