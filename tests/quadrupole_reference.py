"""Float64 torch restatement of the point-quadrupole Ewald term, written from the operator definition (not from the expanded formulas of the
kernel).  Works on the stored entries (i, j, S) of a full neighbour list and on an explicit half-space k set; runs on any device.

    multipole operator: L_i = q_i + mu_i . grad_i + Q_i : grad_i grad_i,  l_i = q_i + mu_i . grad_i  (Q_i = 1/2 (Q + Q^T) of what is given)
    real space:        E_i = 1/2 sum_{entries of row i} [L_i L_j phi(R) - l_i l_j phi(R)],  R = r_j - r_i + S . cell, phi = erfc(alpha r) / r,
                       grad_j = d/dR, grad_i = -d/dR, gradient and Hessian contraction applied by nested `torch.autograd.grad`;
                       entries with r <= 1e-8 skipped
    reciprocal space:  per k, s_i = (q_i + i k.mu_i - k.Q_i.k) e^{i k.r_i}, s'_i = (q_i + i k.mu_i) e^{i k.r_i}, S = sum s_i, S' = sum s'_i:
                       atom i owns 1/2 G_k (Re[conj(s_i) S] - Re[conj(s'_i) S']),  G_k = (8 pi / V) exp(-k^2 / 4 alpha^2) / k^2
    self term:         -1/2 (L_i L_i - l_i l_i) on the Taylor polynomial of erf(alpha r) / r, c0 - c2 r^2 + c4 r^4, at R = 0 (the two operators
                       act on the two ends: one with d/dR, one with -d/dR), also by nested autograd

With L = l + Theta the differences above are the same operators as l_i Theta_j + Theta_i L_j (and, per k, -conj(tau_i e_i) S - conj(s'_i) T
with T = sum tau_j e^{i k.r_j}): that is how they are formed by default, so that zero quadrupoles give exact zeros in every output;
`subtract=True` forms the two products and subtracts them, and tests/test_quadrupole_reference_cpu.py holds the two forms together.

Every derivative output comes from autograd of the (weighted) summed energy, the virial from autograd with respect to an explicit strain eps
(x -> (I + eps) x on positions and cell rows, k -> (I + eps)^-T k, multipoles fixed in the laboratory frame), as in tests/dipole_reference.py,
whose entry helpers and `distance_dtype=torch.float32` mode are reused.
"""
import math

import torch

from tests.dipole_reference import (F64, _alpha, _systems, brute_force_entries, charge_ewald_total, entries_from_csr,  # noqa: F401
                                    entries_from_matrix, green)


def _sym(Q):
    return 0.5 * (Q + Q.transpose(-1, -2))


def _lin(f, rv, q, mu, sign):
    """l f = (q + sign mu . d/dR) f, per entry."""
    g = torch.autograd.grad(f.sum(), rv, create_graph=True)[0]
    return q * f + sign * (mu * g).sum(-1)


def _quad(f, rv, Q):
    """Theta f = Q : d/dR d/dR f, per entry (the sign of d/dR drops out)."""
    g = torch.autograd.grad(f.sum(), rv, create_graph=True)[0]
    out = torch.zeros_like(f)
    for a in range(3):
        out = out + (Q[:, a, :] * torch.autograd.grad(g[:, a].sum(), rv, create_graph=True)[0]).sum(-1)  # row a of the Hessian
    return out


def _quadrupole_part(f, rv, qi, mi, Qi, qj, mj, Qj, subtract=False):
    """(L_i L_j - l_i l_j) f with L = l + Theta, grad_j = d/dR, grad_i = -d/dR.  Default: as l_i Theta_j f + Theta_i L_j f, the same operator
    without a difference, so that zero quadrupoles give exact zeros in every derivative too; `subtract=True` forms both products and subtracts
    (tests/test_quadrupole_reference_cpu.py holds the two against each other)."""
    low_j = _lin(f, rv, qj, mj, 1.0)
    theta_j = _quad(f, rv, Qj)
    if subtract:
        full_j = low_j + theta_j
        return (_lin(full_j, rv, qi, mi, -1.0) + _quad(full_j, rv, Qi)) - _lin(low_j, rv, qi, mi, -1.0)
    return _lin(theta_j, rv, qi, mi, -1.0) + _quad(low_j + theta_j, rv, Qi)


def real_energies(pos, q, mu, Q, cell, alpha, i, j, S, batch_idx=None, distance_dtype=F64, subtract=False):
    """Per-atom float64 real-space energies (differentiable in pos, q, mu, Q, cell).  cell: [3, 3] / [B, 3, 3]; alpha: number or [B]."""
    n, dev = pos.shape[0], pos.device
    if i.numel() == 0:
        return (pos.to(F64).sum() + q.to(F64).sum() + mu.to(F64).sum() + Q.to(F64).sum()) * 0.0 + torch.zeros(n, dtype=F64, device=dev)
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
    q, mu, Qs = q.to(F64), mu.to(F64), _sym(Q.to(F64))
    phi = torch.erfc(al * r) / r
    pair = _quadrupole_part(phi, rv, q[i], mu[i], Qs[i], q[j], mu[j], Qs[j], subtract)
    pair = torch.where(keep, pair, torch.zeros_like(pair))
    return torch.zeros(n, dtype=F64, device=dev).index_add(0, i, 0.5 * pair)


def self_energies(q, mu, Q, alpha_per_atom, subtract=False):
    """-1/2 (L_i L_i - l_i l_i) on c0 - c2 r^2 + c4 r^4 (the Taylor polynomial of erf(alpha r) / r) at R = 0, per atom."""
    q, mu, Qs, al = q.to(F64), mu.to(F64), _sym(Q.to(F64)), alpha_per_atom
    R = torch.zeros((q.shape[0], 3), dtype=F64, device=q.device, requires_grad=True)
    r2 = (R * R).sum(-1)
    sp = math.sqrt(math.pi)
    poly = 2.0 * al / sp - 2.0 * al**3 / (3.0 * sp) * r2 + al**5 / (5.0 * sp) * r2 * r2
    return -0.5 * _quadrupole_part(poly, R, q, mu, Qs, q, mu, Qs, subtract)


def _recip_system(pos, q, mu, Qs, cell, k, alpha):
    g = green(k, cell, alpha)
    ph = pos @ k.T                                                             # [n, K]
    e = torch.complex(torch.cos(ph), torch.sin(ph))
    tau = torch.einsum("ka,nab,kb->nk", k, Qs, k)
    s_low = torch.complex(q[:, None].expand_as(ph), mu @ k.T) * e              # (q_i + i k.mu_i) e^{i k.r_i}
    s_tau = tau * e
    S_low, T = s_low.sum(0), s_tau.sum(0)
    S_all = S_low - T
    # Re[conj(s_i) S] - Re[conj(s'_i) S'] with s_i = s'_i - tau_i e_i and S = S' - T, multiplied out so that nothing is a difference of the
    # charge-and-dipole sums: zero quadrupoles give exact zeros
    terms = -0.5 * g * ((s_tau.conj() * S_all).real + (s_low.conj() * T).real)
    return terms.sum(1)


def recip_energies(pos, q, mu, Q, cell, k_vectors, alpha, batch_idx=None):
    """Per-atom float64 reciprocal energies, self term included (differentiable in pos, q, mu, Q, cell, k_vectors)."""
    n, dev = pos.shape[0], pos.device
    sys_of = _systems(n, batch_idx, dev)
    cells = cell.reshape(-1, 3, 3).to(F64)
    kv = (k_vectors if k_vectors.dim() == 3 else k_vectors.unsqueeze(0)).to(F64)
    if kv.shape[0] != cells.shape[0]:
        kv = kv.expand(cells.shape[0], -1, -1)
    al = _alpha(alpha, cells.shape[0], dev)
    pos, q, mu, Qs = pos.to(F64), q.to(F64), mu.to(F64), _sym(Q.to(F64))
    e = self_energies(q, mu, Qs, al[sys_of])
    for b in range(cells.shape[0]):
        own = torch.nonzero(sys_of == b).reshape(-1)
        e = e.index_add(0, own, _recip_system(pos[own], q[own], mu[own], Qs[own], cells[b], kv[b], al[b]))
    return e


def energies(pos, q, mu, Q, cell, alpha, entries=None, k_vectors=None, batch_idx=None, distance_dtype=F64):
    """Per-atom energies of the parts that are given: `entries` = (i, j, S) for the real-space sum, `k_vectors` for the reciprocal sum."""
    e = torch.zeros(pos.shape[0], dtype=F64, device=pos.device)
    if entries is not None:
        e = e + real_energies(pos, q, mu, Q, cell, alpha, *entries, batch_idx=batch_idx, distance_dtype=distance_dtype)
    if k_vectors is not None:
        e = e + recip_energies(pos, q, mu, Q, cell, k_vectors, alpha, batch_idx=batch_idx)
    return e


def evaluate(pos, q, mu, Q, cell, alpha, entries=None, k_vectors=None, batch_idx=None, distance_dtype=F64, weights=None):
    """dict of float64 numpy arrays: energies, forces (-dL/dr), charge_grads, dipole_grads, quadrupole_grads of L = sum_i w_i E_i (w = 1 by
    default), and the virial [B, 3, 3] = -dE/d(strain) of the unweighted total (nine independent components)."""
    pos = pos.detach().to(F64).clone().requires_grad_(True)
    q = q.detach().to(F64).clone().requires_grad_(True)
    mu = mu.detach().to(F64).clone().requires_grad_(True)
    Q = Q.detach().to(F64).clone().requires_grad_(True)
    cells = cell.detach().to(F64).reshape(-1, 3, 3)
    kv = None if k_vectors is None else k_vectors.detach().to(F64)
    kw = dict(batch_idx=batch_idx, distance_dtype=distance_dtype)
    e = energies(pos, q, mu, Q, cells, alpha, entries, kv, **kw)
    loss = e.sum() if weights is None else (e * weights.to(F64)).sum()
    grads = torch.autograd.grad(loss, [pos, q, mu, Q], allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, (pos, q, mu, Q))]
    out = dict(energies=e.detach(), forces=-grads[0], charge_grads=grads[1], dipole_grads=grads[2], quadrupole_grads=grads[3])
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
    es = energies(pos_e, q.detach(), mu.detach(), Q.detach(), cell_e, alpha, entries, kv_e, **kw).sum()
    vir = torch.autograd.grad(es, eps, allow_unused=True)[0]
    out["virial"] = torch.zeros_like(eps) if vir is None else -vir
    return {k: v.detach().cpu().numpy() for k, v in out.items()}
