"""Float64 torch restatement of the dispersion Ewald sum from its definition (tests/test_dispersion_ewald_reference_cpu.py pins it).

    E = -1/2 sum'_{i, j, n} c_i c_j / |r_j - r_i + n|^6,   beta = alpha, a = beta r, g(a) = exp(-a^2) (1 + a^2 + a^4 / 2)
    real space        E_i = -1/2 sum_{entries of row i} c_i c_j (g(beta r) - T_c(r)) / r^6
    reciprocal space  E_i = -(pi^1.5 beta^3 / (3 V)) sum_{k in half space} f(b) c_i Re[e^{-i k.r_i} S(k)]      b = |k| / (2 beta)
                            - (pi^1.5 beta^3 / (6 V)) c_i sum_j c_j + (beta^6 / 12) c_i^2
                      f(b) = (1 - 2 b^2) exp(-b^2) + 2 sqrt(pi) b^3 erfc(b),   S(k) = sum_j c_j e^{i k.r_j}

T_c is Tinker's quintic switch of the part `lennard_jones(cutoff=, taper=)` has already summed (1 below the taper, 0 from the cutoff on; without
a taper 1 below the cutoff), 0 by default.  A caller's k-vector with |k|^2 < 1e-10 weighs nothing, as the k = 0 slot of a full set would.  Derivatives come from autograd; the virial is the strain derivative with positions, cell and k-vectors strained together.
`distance_dtype=float32` rounds pair vector and r^2 to float32 as the kernel does; `nudge_r2` moves every float32 r^2 by one ulp: what the
float32 real-space bars of tests/test_dispersion_ewald_gpu.py are measured with."""
import math

import torch

F64 = torch.float64
SERIES_BELOW = 1.0  # a^2 below which 1 - g is summed as a series; the kernel's threshold
SERIES_TERMS = 22


def one_minus_g_direct(a2):
    return 1.0 - torch.exp(-a2) * (1.0 + a2 + 0.5 * a2 * a2)


def one_minus_g_series(a2):
    """1 - g = exp(-a^2) sum_{n >= 3} a^(2n) / n!: positive terms only."""
    term = a2 * a2 * a2 / 6.0
    total = term.clone()
    for n in range(4, SERIES_TERMS + 1):
        term = term * a2 / n
        total = total + term
    return torch.exp(-a2) * total


def one_minus_g(a2):
    small = a2 < SERIES_BELOW
    return torch.where(small, one_minus_g_series(torch.where(small, a2, torch.zeros_like(a2))), one_minus_g_direct(a2))


def one_minus_switch(r, cutoff, taper):
    """1 - T: 0 below the taper, 1 from the cutoff on."""
    t = torch.clamp((r - taper) / (cutoff - taper), min=0.0, max=1.0)
    return t ** 3 * (10.0 - 15.0 * t + 6.0 * t * t)


def f_of_b(b):
    return (1.0 - 2.0 * b * b) * torch.exp(-b * b) + 2.0 * math.sqrt(math.pi) * b ** 3 * torch.erfc(b)


def entries_from_matrix(neighbor_matrix, shifts, mask_value):
    """(i, j, S) of a padded matrix: entries equal to mask_value or outside [0, N) are padding."""
    nm = neighbor_matrix.long()
    n, m = nm.shape
    keep = (nm != int(mask_value)) & (nm >= 0) & (nm < n)
    i = torch.arange(n, device=nm.device).unsqueeze(1).expand(n, m)[keep]
    S = torch.zeros((n, m, 3), dtype=torch.long, device=nm.device) if shifts is None else shifts.long()
    return i, nm[keep], S[keep]


def _systems(pos, cell, alpha, batch_idx):
    n = pos.shape[0]
    sys_of = torch.zeros(n, dtype=torch.long, device=pos.device) if batch_idx is None else batch_idx.long()
    cells = cell.reshape(-1, 3, 3)
    al = torch.as_tensor(alpha, dtype=F64, device=pos.device).reshape(-1)
    return sys_of, cells, al.expand(cells.shape[0]) if al.numel() == 1 else al


def entries_within(pos, cell, cutoff):
    """(i, j, S) of every pair image with 0 < r < cutoff of one system: a full list by brute force."""
    cell = cell.reshape(3, 3)
    heights = torch.linalg.det(cell).abs() / torch.stack([torch.linalg.cross(cell[(d + 1) % 3], cell[(d + 2) % 3]).norm() for d in range(3)])
    reach = [int(math.ceil(float(cutoff / h))) + 1 for h in heights]
    S = torch.cartesian_prod(*[torch.arange(-m, m + 1) for m in reach])
    n = pos.shape[0]
    d = pos[None, None, :, :] - pos[None, :, None, :] + (S.to(pos.dtype) @ cell)[:, None, None, :]  # [image, i, j]
    r2 = (d * d).sum(-1)
    s, i, j = torch.nonzero((r2 > 1e-16) & (r2 < cutoff * cutoff), as_tuple=True)
    return i, j, S[s]


def real_energies(pos, c, cell, alpha, i, j, S, batch_idx=None, counted=None, distance_dtype=F64, nudge_r2=False):
    """Per-atom float64 real-space energies over the entries (i, j, S); counted = (cutoff, taper) | None."""
    sys_of, cells, al = _systems(pos, cell, alpha, batch_idx)

    def pair_vectors(dtype, p, cm):
        return p.to(dtype)[j] - p.to(dtype)[i] + torch.einsum("ea,eab->eb", S.to(dtype), cm.to(dtype)[sys_of[i]])

    rvec = pair_vectors(F64, pos, cells)
    r2 = (rvec * rvec).sum(-1)
    if distance_dtype != F64:
        low = pair_vectors(distance_dtype, pos.detach(), cells.detach())
        low_r2 = (low * low).sum(-1)
        if nudge_r2:
            low_r2 = torch.nextafter(low_r2, torch.full_like(low_r2, float("inf")))
        rvec = rvec + (low.to(F64) - rvec).detach()
        r2 = (rvec * rvec).sum(-1)
        r2 = r2 + (low_r2.to(F64) - r2).detach()
    keep = r2 > 1e-16
    r2 = torch.where(keep, r2, torch.ones_like(r2))
    a2 = al[sys_of[i]] ** 2 * r2
    if counted is None:
        kernel = 1.0 - one_minus_g(a2)
    else:
        # g - T = (1 - T) - (1 - g); without a taper 1 - T is the step at the cutoff, taken on r^2 as the kernel takes it
        outside = (r2 >= counted[0] * counted[0]).to(F64) if counted[1] is None else one_minus_switch(torch.sqrt(r2), *counted)
        kernel = outside - one_minus_g(a2)
    pair = -0.5 * c[i] * c[j] * kernel / r2 ** 3
    return torch.zeros(pos.shape[0], dtype=F64, device=pos.device).index_add(0, i, torch.where(keep, pair, torch.zeros_like(pair)))


def recip_energies(pos, c, cell, k_vectors, alpha, batch_idx=None):
    """Per-atom float64 reciprocal-space energies, k = 0 and self terms included; k_vectors [K, 3] or [B, K, 3] (half space), K may be 0."""
    sys_of, cells, al = _systems(pos, cell, alpha, batch_idx)
    nsys = cells.shape[0]
    kv = k_vectors.to(F64)
    kv = (kv if kv.dim() == 3 else kv.unsqueeze(0)).expand(nsys, -1, 3)
    vol = torch.linalg.det(cells).abs()
    pref = math.pi ** 1.5 * al ** 3 / (3.0 * vol)  # [B]
    csum = torch.zeros(nsys, dtype=F64, device=pos.device).index_add(0, sys_of, c)
    e = -0.5 * pref[sys_of] * c * csum[sys_of] + al[sys_of] ** 6 / 12.0 * c * c
    if kv.shape[1]:
        knorm = kv.norm(dim=-1)
        w = torch.where(knorm > 1e-5, f_of_b(knorm / (2.0 * al[:, None])), torch.zeros_like(knorm))  # [B, K]
        phase = torch.einsum("nd,nkd->nk", pos, kv[sys_of])
        cs, sn = c[:, None] * torch.cos(phase), c[:, None] * torch.sin(phase)
        own = torch.nn.functional.one_hot(sys_of, nsys).to(F64)  # [N, B]
        sr, si = own.T @ cs, own.T @ sn  # [B, K]
        e = e - pref[sys_of] * (w[sys_of] * (cs * sr[sys_of] + sn * si[sys_of])).sum(-1)
    return e


def evaluate(pos, c, cell, alpha, entries=None, k_vectors=None, batch_idx=None, **kw):
    """dict of float64 tensors (energies, forces, coefficient_grads, virial [B, 3, 3]) of the real half (entries), the reciprocal half
    (k_vectors), or their sum (both)."""
    pos = pos.detach().to(F64).clone().requires_grad_(True)
    c = c.detach().to(F64).clone().requires_grad_(True)
    cell = cell.detach().to(F64).reshape(-1, 3, 3)
    alpha = alpha.detach().to(F64) if isinstance(alpha, torch.Tensor) else alpha
    kv = None if k_vectors is None else k_vectors.detach().to(F64)

    def total(p, cm, k):
        e = torch.zeros(p.shape[0], dtype=F64, device=p.device)
        if entries is not None:
            e = e + real_energies(p, c, cm, alpha, *entries, batch_idx=batch_idx, **kw)
        if k is not None:
            e = e + recip_energies(p, c, cm, k, alpha, batch_idx)
        return e

    e = total(pos, cell, kv)
    grads = torch.autograd.grad(e.sum(), [pos, c], allow_unused=True)  # (without k-vectors or entries the positions are not used)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, (pos, c))]
    sys_of = torch.zeros(pos.shape[0], dtype=torch.long, device=pos.device) if batch_idx is None else batch_idx.long()
    strain = torch.zeros((cell.shape[0], 3, 3), dtype=F64, device=pos.device, requires_grad=True)
    defo = torch.eye(3, dtype=F64, device=pos.device) + strain  # x -> (I + eps) x: a row vector becomes x (I + eps)^T
    pos_e = torch.einsum("nb,nab->na", pos.detach(), defo[sys_of])
    cell_e = torch.einsum("srb,sab->sra", cell, defo)
    kv_e = None
    if kv is not None:  # k -> (I + eps)^-T k: the row vector becomes k (I + eps)^-1
        kv_e = torch.einsum("skb,sba->ska", (kv if kv.dim() == 3 else kv.unsqueeze(0)).expand(cell.shape[0], -1, 3), torch.linalg.inv(defo))
    virial = -torch.autograd.grad(total(pos_e, cell_e, kv_e).sum(), strain)[0]
    return dict(energies=e.detach(), forces=-grads[0], coefficient_grads=grads[1], virial=virial)


def lattice_sum(pos, c, cell, radius):
    """Direct sum -1/2 sum' c_i c_j / r^6 over all images with r < radius, plus the continuum tail -1/2 (sum c)^2 4 pi / (3 V radius^3)."""
    pos, c, cell = pos.to(F64), c.to(F64), cell.to(F64).reshape(3, 3)
    heights = torch.linalg.det(cell).abs() / torch.stack([torch.linalg.cross(cell[(d + 1) % 3], cell[(d + 2) % 3]).norm() for d in range(3)])
    span = torch.norm(pos[:, None] - pos[None], dim=-1).max()
    reach = [int(math.ceil(float((radius + span) / h))) for h in heights]
    images = torch.cartesian_prod(*[torch.arange(-m, m + 1, dtype=F64) for m in reach]) @ cell
    total = 0.0
    cc = c[:, None] * c[None]
    for block in images.split(4096):
        d = pos[None, None, :, :] - pos[None, :, None, :] + block[:, None, None, :]
        r2 = (d * d).sum(-1)
        keep = (r2 > 1e-16) & (r2 < radius * radius)
        total = total + (torch.where(keep, cc / torch.where(keep, r2, torch.ones_like(r2)) ** 3, torch.zeros_like(r2))).sum()
    vol = torch.linalg.det(cell).abs()
    return float(-0.5 * total - 0.5 * c.sum() ** 2 * 4.0 * math.pi / (3.0 * vol * radius ** 3))
