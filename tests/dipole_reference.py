"""Float64 torch restatement of the point-dipole Ewald term, written from the operator definition (not from the expanded formulas of the
kernel).  Works on the stored entries (i, j, S) of a full neighbour list and on an explicit half-space k set; runs on any device.

    real space:        E_i = 1/2 sum_{entries of row i} [(q_i + mu_i . grad_i)(q_j + mu_j . grad_j) phi(|r_j - r_i + S . cell|) - q_i q_j phi]
                       phi(r) = erfc(alpha r) / r, the mu . grad applied by nested `torch.autograd.grad`; entries with r <= 1e-8 skipped
    reciprocal space:  E = 1/2 sum_k G_k (|S|^2 - |S_q|^2) - 2 alpha^3 / (3 sqrt(pi)) sum_i |mu_i|^2,  G_k = (8 pi / V) exp(-k^2 / 4 alpha^2) / k^2,
                       S = sum_j (q_j + i k.mu_j) e^{i k.r_j},  S_q = sum_j q_j e^{i k.r_j};  atom i owns Re[conj(s_i) S] - Re[conj(s_q,i) S_q]

Every derivative output comes from autograd of the (weighted) summed energy, the virial from autograd with respect to an explicit strain eps
(x -> (I + eps) x on positions and cell rows, k -> (I + eps)^-T k, dipoles fixed in the laboratory frame).  `distance_dtype=torch.float32`
forms the pair vector and the distance in float32 and everything after that in float64: the kernel's arithmetic model for float32 inputs.
"""
import math

import torch

from tests.gaussian_reference import brute_force_entries, entries_from_csr, entries_from_matrix  # noqa: F401  (the same entry helpers)

F64 = torch.float64


def _systems(n, batch_idx, device):
    return torch.zeros(n, dtype=torch.long, device=device) if batch_idx is None else batch_idx.long()


def _alpha(alpha, nsys, device):
    a = alpha if isinstance(alpha, torch.Tensor) else torch.tensor(float(alpha), dtype=F64)
    return a.detach().to(device=device, dtype=F64).reshape(-1).expand(nsys) if a.numel() == 1 else a.detach().to(device=device, dtype=F64).reshape(-1)


def real_energies(pos, q, mu, cell, alpha, i, j, S, batch_idx=None, distance_dtype=F64):
    """Per-atom float64 real-space energies (differentiable in pos, q, mu, cell).  cell: [3, 3] / [B, 3, 3]; alpha: number or [B]."""
    n, dev = pos.shape[0], pos.device
    sys_of = _systems(n, batch_idx, dev)
    cells = cell.reshape(-1, 3, 3)
    al = _alpha(alpha, cells.shape[0], dev)[sys_of[i]]

    def pair_vectors(dtype, p, c):
        return p.to(dtype)[j] - p.to(dtype)[i] + torch.einsum("ea,eab->eb", S.to(dtype), c.to(dtype)[sys_of[i]])

    rvec = pair_vectors(F64, pos, cells)
    low = None
    if distance_dtype != F64:
        # the VALUES of the pair vector and of the distance are those of the low-precision arithmetic; derivatives keep flowing through the
        # float64 expressions (value + detached difference)
        low = pair_vectors(distance_dtype, pos.detach(), cells.detach())
        rvec = rvec + (low.to(F64) - rvec).detach()
    if not rvec.requires_grad:
        rvec = rvec.detach().requires_grad_(True)
    r_val = torch.sqrt((rvec.detach() ** 2).sum(-1)) if low is None else torch.sqrt((low * low).sum(-1)).to(F64)
    keep = r_val > 1e-8
    unit = torch.zeros_like(rvec)
    unit[:, 0] = 1.0
    rv = torch.where(keep.unsqueeze(1), rvec, unit)  # skipped entries: a harmless vector, no gradient to the positions
    r = torch.sqrt((rv * rv).sum(-1))
    if low is not None:
        r = r + (torch.where(keep, r_val, torch.ones_like(r_val)) - r).detach()
    q, mu = q.to(F64), mu.to(F64)
    phi = torch.erfc(al * r) / r
    grad_j = torch.autograd.grad(phi.sum(), rv, create_graph=True)[0]          # grad_j phi = d phi / dR
    charge_part = q[j] * phi
    psi = charge_part + (mu[j] * grad_j).sum(-1)                               # (q_j + mu_j . grad_j) phi
    grad_i = -torch.autograd.grad(psi.sum(), rv, create_graph=True)[0]         # grad_i = -d / dR
    pair = (q[i] * psi + (mu[i] * grad_i).sum(-1)) - q[i] * charge_part        # ... minus the charge-charge part
    pair = torch.where(keep, pair, torch.zeros_like(pair))
    return torch.zeros(n, dtype=F64, device=dev).index_add(0, i, 0.5 * pair)


def green(k, cell, alpha):
    """G_k [K] of one system: (8 pi / V) exp(-k^2 / 4 alpha^2) / k^2, 0 for k^2 < 1e-10."""
    k2 = (k * k).sum(-1)
    ok = k2 >= 1e-10
    k2s = torch.where(ok, k2, torch.ones_like(k2))
    g = 8.0 * math.pi / torch.abs(torch.linalg.det(cell)) * torch.exp(-k2s / (4.0 * alpha * alpha)) / k2s
    return torch.where(ok, g, torch.zeros_like(g))


def _recip_system(pos, q, mu, cell, k, alpha):
    """(per-atom energies [n], sum_k |term| per atom [n]) of one system."""
    g = green(k, cell, alpha)
    ph = pos @ k.T                                                             # [n, K]
    c, s = torch.cos(ph), torch.sin(ph)
    p = mu @ k.T                                                               # k . mu_i
    sq_re, sq_im = q[:, None] * c, q[:, None] * s                              # s_q,i = q_i e^{i k.r_i}
    s_re, s_im = sq_re - p * s, sq_im + p * c                                  # s_i = (q_i + i k.mu_i) e^{i k.r_i}
    S_re, S_im, Sq_re, Sq_im = s_re.sum(0), s_im.sum(0), sq_re.sum(0), sq_im.sum(0)
    terms = 0.5 * g * ((s_re * S_re + s_im * S_im) - (sq_re * Sq_re + sq_im * Sq_im))
    self_term = 2.0 * alpha**3 / (3.0 * math.sqrt(math.pi)) * (mu * mu).sum(-1)
    return terms.sum(1) - self_term, terms.detach().abs().sum(1) + self_term.detach()


def recip_energies(pos, q, mu, cell, k_vectors, alpha, batch_idx=None, return_abs=False):
    """Per-atom float64 reciprocal energies, self term included (differentiable in pos, q, mu, cell, k_vectors).  k_vectors [K, 3] / [B, K, 3]."""
    n, dev = pos.shape[0], pos.device
    sys_of = _systems(n, batch_idx, dev)
    cells = cell.reshape(-1, 3, 3).to(F64)
    kv = (k_vectors if k_vectors.dim() == 3 else k_vectors.unsqueeze(0)).to(F64)
    if kv.shape[0] != cells.shape[0]:
        kv = kv.expand(cells.shape[0], -1, -1)
    al = _alpha(alpha, cells.shape[0], dev)
    pos, q, mu = pos.to(F64), q.to(F64), mu.to(F64)
    e, a = torch.zeros(n, dtype=F64, device=dev), torch.zeros(n, dtype=F64, device=dev)
    for b in range(cells.shape[0]):
        own = torch.nonzero(sys_of == b).reshape(-1)
        eb, ab = _recip_system(pos[own], q[own], mu[own], cells[b], kv[b], al[b])
        e, a = e.index_add(0, own, eb), a.index_add(0, own, ab)
    return (e, a) if return_abs else e


def recip_total(pos, q, mu, cell, k, alpha):
    """1/2 sum_k G_k (|S|^2 - |S_q|^2) - self term of ONE system, summed over whole structure factors (no per-atom split)."""
    pos, q, mu, cell, k = (t.to(F64) for t in (pos, q, mu, cell, k))
    ph = pos @ k.T
    e = torch.complex(torch.cos(ph), torch.sin(ph))
    S_q = (q[:, None] * e).sum(0)
    S = S_q + (torch.complex(torch.zeros_like(ph), mu @ k.T) * e).sum(0)
    return 0.5 * (green(k, cell, alpha) * (S.abs() ** 2 - S_q.abs() ** 2)).sum() - 2.0 * alpha**3 / (3.0 * math.sqrt(math.pi)) * (mu * mu).sum()


def charge_ewald_total(pos, q, cell, alpha, i, j, S, k):
    """Total point-charge Ewald energy of one system over the same entries and k set (exact erfc), with the neutralising-background term."""
    pos, q, cell, k = (t.to(F64) for t in (pos, q, cell, k))
    r = torch.linalg.norm(pos[j] - pos[i] + S.to(F64) @ cell, dim=-1)
    real = 0.5 * (q[i] * q[j] * torch.erfc(alpha * r) / r).sum()
    ph = pos @ k.T
    S_q = (q[:, None] * torch.complex(torch.cos(ph), torch.sin(ph))).sum(0)
    vol = torch.abs(torch.linalg.det(cell))
    return (real + 0.5 * (green(k, cell, alpha) * S_q.abs() ** 2).sum() - alpha / math.sqrt(math.pi) * (q * q).sum()
            - math.pi * q.sum() ** 2 / (2.0 * alpha * alpha * vol))


def energies(pos, q, mu, cell, alpha, entries=None, k_vectors=None, batch_idx=None, distance_dtype=F64):
    """Per-atom energies of the parts that are given: `entries` = (i, j, S) for the real-space sum, `k_vectors` for the reciprocal sum."""
    e = torch.zeros(pos.shape[0], dtype=F64, device=pos.device)
    if entries is not None:
        e = e + real_energies(pos, q, mu, cell, alpha, *entries, batch_idx=batch_idx, distance_dtype=distance_dtype)
    if k_vectors is not None:
        e = e + recip_energies(pos, q, mu, cell, k_vectors, alpha, batch_idx=batch_idx)
    return e


def evaluate(pos, q, mu, cell, alpha, entries=None, k_vectors=None, batch_idx=None, distance_dtype=F64, weights=None):
    """dict of float64 numpy arrays: energies, forces (-dL/dr), charge_grads, dipole_grads of L = sum_i w_i E_i (w = 1 by default), and the
    virial [B, 3, 3] = -dE/d(strain) of the unweighted total (nine independent components)."""
    pos = pos.detach().to(F64).clone().requires_grad_(True)
    q = q.detach().to(F64).clone().requires_grad_(True)
    mu = mu.detach().to(F64).clone().requires_grad_(True)
    cells = cell.detach().to(F64).reshape(-1, 3, 3)
    kv = None if k_vectors is None else k_vectors.detach().to(F64)
    kw = dict(batch_idx=batch_idx, distance_dtype=distance_dtype)
    e = energies(pos, q, mu, cells, alpha, entries, kv, **kw)
    loss = e.sum() if weights is None else (e * weights.to(F64)).sum()
    grads = torch.autograd.grad(loss, [pos, q, mu])
    out = dict(energies=e.detach(), forces=-grads[0], charge_grads=grads[1], dipole_grads=grads[2])
    nsys = cells.shape[0]
    sys_of = _systems(pos.shape[0], batch_idx, pos.device)
    eps = torch.zeros((nsys, 3, 3), dtype=F64, device=pos.device, requires_grad=True)
    defo = torch.eye(3, dtype=F64, device=pos.device) + eps  # x -> (I + eps) x: a row vector becomes x (I + eps)^T
    pos_e = torch.einsum("nb,nab->na", pos.detach(), defo[sys_of])
    cell_e = torch.einsum("srb,sab->sra", cells, defo)
    kv_e = None
    if kv is not None:
        k3 = kv if kv.dim() == 3 else kv.unsqueeze(0)
        if k3.shape[0] != nsys:
            k3 = k3.expand(nsys, -1, -1)
        kv_e = torch.einsum("skb,sba->ska", k3, torch.linalg.inv(defo))  # k -> (I + eps)^-T k: a row vector becomes k (I + eps)^-1
    es = energies(pos_e, q.detach(), mu.detach(), cell_e, alpha, entries, kv_e, **kw).sum()
    out["virial"] = -torch.autograd.grad(es, eps)[0]
    return {k: v.detach().cpu().numpy() for k, v in out.items()}
