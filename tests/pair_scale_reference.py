"""Float64 torch yardstick of `pair_scale_correction`, written from the definition (not from the expanded formulas of the kernel).  Works on
the stored entries (i, j, S) of a full list with one scale per entry; runs on any device.

    multipole operator: L_i = q_i + mu_i . grad_i + Q_i : grad_i grad_i  (Q_i = 1/2 (Q + Q^T) of what is given)
    E_i = 1/2 sum_{entries of row i} (s_e - 1) L_i L_j (1 / r),   R = r_j - r_i + S . cell,  r = |R|,  grad_j = d/dR, grad_i = -d/dR,
    gradient and Hessian contraction applied by nested `torch.autograd.grad`, as tests/quadrupole_reference.py forms its operator (whose
    `_lin` and `_quad` are reused); entries with r <= 1e-8 and entries with s_e == 1 skipped (the latter contribute an exact zero anyway)

Minimum-image mode: S is not read; R = d - rint(d . cell^-1) . cell with d = r_j - r_i, in float64 (rint is piecewise constant, so the
derivatives are those of the reduced vector, and a strained cell strains R homogeneously).  `distance_dtype=torch.float32` is the mode of the
siblings: the VALUES of the pair vector and the distance are those of the low-precision arithmetic -- float32 differences and products with
explicit shifts; under minimum image the float64 reduction of the float32 positions rounded once to float32 -- while derivatives flow
through the float64 expressions.

Every derivative output comes from autograd of the (weighted) summed energy, the virial from autograd with respect to an explicit strain
(x -> (I + eps) x on positions and cell rows, multipoles fixed in the laboratory frame), as in tests/quadrupole_reference.py.
"""
import torch

from tests.dipole_reference import F64, _systems
from tests.quadrupole_reference import _lin, _quad, _sym


def matrix_entries(neighbor_matrix, pair_scales, shifts=None, mask_value=None):
    """((i, j, S) int64, scales float64) of the entries of a padded matrix [N, M] that are not padding (the mask value or outside [0, N))."""
    n, m = neighbor_matrix.shape
    nm = neighbor_matrix.long()
    ok = (nm >= 0) & (nm < n)
    if mask_value is not None:
        ok &= nm != mask_value
    i = torch.arange(n, device=nm.device).unsqueeze(1).expand(n, m)[ok]
    S = torch.zeros((i.shape[0], 3), dtype=torch.long, device=nm.device) if shifts is None else shifts.long()[ok]
    return (i, nm[ok], S), pair_scales.to(F64)[ok]


def _pair_vectors_of(pos, cells, i, j, S, sys_of, minimum_image):
    d = pos[j] - pos[i]
    c = cells[sys_of[i]]
    if minimum_image:
        n = torch.round(torch.einsum("ea,eab->eb", d, torch.linalg.inv(c))).detach()  # torch.round is rint: half to even
        return d - torch.einsum("ea,eab->eb", n, c)
    return d + torch.einsum("ea,eab->eb", S.to(pos.dtype), c)


def pair_energies(pos, q, mu, Q, scales, i, j, S, cell=None, batch_idx=None, distance_dtype=F64, minimum_image=False, _pair_vectors=None):
    """Per-atom float64 energies (differentiable in pos, q, mu, Q, cell).  cell: None (a cluster), [3, 3] or [B, 3, 3].  `_pair_vectors`
    [E, 3]: the pair vectors to use in the place of the ones formed here (the virial test differentiates with respect to them)."""
    n, dev = pos.shape[0], pos.device
    if i.numel() == 0:
        return (pos.to(F64).sum() + q.to(F64).sum() + mu.to(F64).sum() + Q.to(F64).sum()) * 0.0 + torch.zeros(n, dtype=F64, device=dev)
    cells = torch.eye(3, dtype=F64, device=dev).reshape(1, 3, 3) if cell is None else cell.reshape(-1, 3, 3)
    sys_of = _systems(n, batch_idx if cell is not None else None, dev)
    rvec = _pair_vectors_of(pos.to(F64), cells.to(F64), i, j, S, sys_of, minimum_image) if _pair_vectors is None else _pair_vectors
    low = None
    if distance_dtype != F64:
        if minimum_image:  # the float64 reduction of the low-precision positions and cell, rounded once
            low = _pair_vectors_of(pos.detach().to(distance_dtype).to(F64), cells.detach().to(distance_dtype).to(F64), i, j, S, sys_of,
                                True).to(distance_dtype)
        else:
            low = _pair_vectors_of(pos.detach().to(distance_dtype), cells.detach().to(distance_dtype), i, j, S, sys_of, False)
        rvec = rvec + (low.to(F64) - rvec).detach()
    if not rvec.requires_grad:
        rvec = rvec.detach().requires_grad_(True)
    r_val = torch.sqrt((rvec.detach() ** 2).sum(-1)) if low is None else torch.sqrt((low * low).sum(-1)).to(F64)
    s = scales.detach().to(F64)
    keep = (r_val > 1e-8) & (s != 1.0)
    unit = torch.zeros_like(rvec)
    unit[:, 0] = 1.0
    rv = torch.where(keep.unsqueeze(1), rvec, unit)  # skipped entries: a harmless vector, no gradient to the positions
    r = torch.sqrt((rv * rv).sum(-1))
    if low is not None:
        r = r + (torch.where(keep, r_val, torch.ones_like(r_val)) - r).detach()
    q, mu, Qs = q.to(F64), mu.to(F64), _sym(Q.to(F64))
    phi = 1.0 / r
    full_j = _lin(phi, rv, q[j], mu[j], 1.0) + _quad(phi, rv, Qs[j])             # L_j (1 / r)
    pair = _lin(full_j, rv, q[i], mu[i], -1.0) + _quad(full_j, rv, Qs[i])        # L_i L_j (1 / r)
    pair = torch.where(keep, (s - 1.0) * pair, torch.zeros_like(pair))
    return torch.zeros(n, dtype=F64, device=dev).index_add(0, i, 0.5 * pair)


def evaluate(pos, q, mu, Q, scales, entries, cell=None, batch_idx=None, distance_dtype=F64, weights=None, minimum_image=False):
    """dict of float64 numpy arrays: energies, forces (-dL/dr), charge_grads, dipole_grads, quadrupole_grads of L = sum_i w_i E_i (w = 1 by
    default) and, with a cell, the virial [B, 3, 3] = -dE/d(strain) of the unweighted total (nine independent components).  `mu=None` /
    `Q=None`: no dipoles / no quadrupoles."""
    n, dev = pos.shape[0], pos.device
    mu = torch.zeros((n, 3), dtype=F64, device=dev) if mu is None else mu
    Q = torch.zeros((n, 3, 3), dtype=F64, device=dev) if Q is None else Q
    pos = pos.detach().to(F64).clone().requires_grad_(True)
    q = q.detach().to(F64).clone().requires_grad_(True)
    mu = mu.detach().to(F64).clone().requires_grad_(True)
    Q = Q.detach().to(F64).clone().requires_grad_(True)
    cells = None if cell is None else cell.detach().to(F64).reshape(-1, 3, 3)
    kw = dict(batch_idx=batch_idx, distance_dtype=distance_dtype, minimum_image=minimum_image)
    e = pair_energies(pos, q, mu, Q, scales, *entries, cell=cells, **kw)
    loss = e.sum() if weights is None else (e * weights.to(F64)).sum()
    grads = torch.autograd.grad(loss, [pos, q, mu, Q], allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, (pos, q, mu, Q))]
    out = dict(energies=e.detach(), forces=-grads[0], charge_grads=grads[1], dipole_grads=grads[2], quadrupole_grads=grads[3])
    if cells is not None:
        nsys = cells.shape[0]
        sys_of = _systems(n, batch_idx, dev)
        eps = torch.zeros((nsys, 3, 3), dtype=F64, device=dev, requires_grad=True)
        defo = torch.eye(3, dtype=F64, device=dev) + eps  # x -> (I + eps) x: a row vector becomes x (I + eps)^T
        pos_e = torch.einsum("nb,nab->na", pos.detach(), defo[sys_of])
        cell_e = torch.einsum("srb,sab->sra", cells, defo)
        es = pair_energies(pos_e, q.detach(), mu.detach(), Q.detach(), scales, *entries, cell=cell_e, **kw).sum()
        vir = torch.autograd.grad(es, eps, allow_unused=True)[0]
        out["virial"] = torch.zeros_like(eps) if vir is None else -vir
    return {k: v.detach().cpu().numpy() for k, v in out.items()}
