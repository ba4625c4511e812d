"""Float64 torch restatement of charge equilibration, written from its definition (not from the kernels): a dense H built from the stored
entries (i, j, S) of a full neighbour list, solved per system through its KKT matrix with `torch.linalg.solve`, so autograd gives reference
gradients.  Runs on any device.

    minimise  sum chi_i q_i + 1/2 q^T H q   subject to  sum_{i in s} q_i = Q_s          =>   chi + H q = lambda_s,   H = diag(J) + A

    A with a cell (E_el = point-charge Ewald + Gaussian correction, as the package's public functions define them):
        pair      sum over entries (i, j, S) with r > 1e-8 of [erfc_lr(alpha_s r) - erfc(r / g_ij)] / r   (second term only for r / g_ij < 6, g_ij > 0)
        k-space   w (4 pi / V) sum_k exp(-k^2 / 4 alpha^2) cos(k . r_ij) / k^2  over a given k-vector set; w = 2 for a half-space set
                  (`generate_k_vectors_ewald_summation`), 1 for a full one
        self      -2 alpha / sqrt(pi) and 1 / (sqrt(pi) sigma_i) [sigma_i > 0] on the diagonal
        background -pi / (alpha^2 V) + (2 pi / V)(s_i + s_j) for every pair of one system
    A without a cell:   pair  [1 - erfc(r / g_ij)] / r,   self  1 / (sqrt(pi) sigma_i).
    s_i = max(sigma_i, 0)^2, g_ij = sqrt(2 (s_i + s_j)),  r = |r_j - r_i + S . cell|.

`erfc_lr` is a parameter: the exact erfc, the Abramowitz-Stegun 7.1.26 polynomial that `ewald_real_space` evaluates, or that polynomial with the
analytic derivative `ewald_real_space` differentiates it with (`erfc_as_analytic_derivative`: the model for gradient comparisons).
`distance_dtype=torch.float32` forms the pair vector and the distance in float32 and everything after that in float64: the kernel's
arithmetic model for float32 inputs (values only; derivatives flow through the float64 expressions, as in gaussian_reference).
"""
import math

import torch

F64 = torch.float64
_SQRT_PI = math.sqrt(math.pi)


def erfc_as(x):
    """Abramowitz-Stegun 7.1.26: erfc(x) ~ (a1 t + ... + a5 t^5) exp(-x^2), t = 1 / (1 + p x), x >= 0; |error| <= 1.5e-7."""
    p, a = 0.3275911, (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
    t = 1.0 / (1.0 + p * x)
    poly = a[0] * t + a[1] * t**2 + a[2] * t**3 + a[3] * t**4 + a[4] * t**5
    return poly * torch.exp(-x * x)


class _ErfcAsAnalyticDerivative(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return erfc_as(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * (-2.0 / _SQRT_PI) * torch.exp(-x * x)


def erfc_as_analytic_derivative(x):
    """The arithmetic model of `ewald_real_space` under autograd: the VALUE is the A-S polynomial, the DERIVATIVE is the analytic
    erfc'(x) = -2 / sqrt(pi) exp(-x^2) that its adjoint kernel uses (not the derivative of the polynomial, which differs by up to 1e-6)."""
    return _ErfcAsAnalyticDerivative.apply(x)


def _systems(n, batch_idx, device):
    return torch.zeros(n, dtype=torch.long, device=device) if batch_idx is None else batch_idx.long()


def pair_coefficients(pos, sigma, cell, alpha, i, j, S, batch_idx=None, erfc_lr=torch.erfc, distance_dtype=F64, parts=False):
    """Float64 c_e of every entry (differentiable in pos, sigma, cell).  `parts=True` returns (|lr / r|, |erfc / r|) instead: the two
    magnitudes whose rounding bounds the error of a row sum."""
    n = pos.shape[0]
    sys_of = _systems(n, batch_idx, pos.device)
    cells = None if cell is None else cell.reshape(-1, 3, 3)

    def pair_vectors(dtype, p, c):
        v = p.to(dtype)[j] - p.to(dtype)[i]
        return v if c is None else v + torch.einsum("ea,eab->eb", S.to(dtype), c.to(dtype)[sys_of[i]])

    rvec = pair_vectors(F64, pos, cells)
    low = None
    if distance_dtype != F64:
        low = pair_vectors(distance_dtype, pos.detach(), None if cells is None else cells.detach())
        rvec = rvec + (low.to(F64) - rvec).detach()
    r2 = (rvec * rvec).sum(-1)
    ok_r = r2 > 0
    r = torch.sqrt(torch.where(ok_r, r2, torch.ones_like(r2)))
    if low is not None:
        r = r + (torch.sqrt((low * low).sum(-1)).to(F64) - r).detach()
    r = torch.where(ok_r, r, torch.zeros_like(r))
    keep_r = r > 1e-8
    r_safe = torch.where(keep_r, r, torch.ones_like(r))
    s = torch.clamp(sigma.to(F64), min=0.0) ** 2
    g2 = 2.0 * (s[i] + s[j])
    ok_g = g2 > 0
    x = r_safe / torch.sqrt(torch.where(ok_g, g2, torch.ones_like(g2)))
    keep_g = ok_g & keep_r & (x < 6.0)
    short = torch.where(keep_g, torch.erfc(torch.where(keep_g, x, torch.ones_like(x))), torch.zeros_like(r))
    if cells is None:
        lr = torch.ones_like(r)
    else:
        lr = erfc_lr(alpha.to(F64).reshape(-1)[sys_of[i]] * r_safe)
    zero = torch.zeros_like(r)
    if parts:
        return torch.where(keep_r, (lr / r_safe).abs(), zero), torch.where(keep_r, (short / r_safe).abs(), zero)
    return torch.where(keep_r, (lr - short) / r_safe, zero)


def diagonal(hardness, sigma):
    sigma = sigma.to(F64)
    smeared = sigma > 0
    return hardness.to(F64) + torch.where(smeared, 1.0 / (_SQRT_PI * torch.where(smeared, sigma, torch.ones_like(sigma))), torch.zeros_like(sigma))


def real_space_operator(pos, sigma, hardness, cell, alpha, i, j, S, batch_idx=None, erfc_lr=torch.erfc, distance_dtype=F64):
    """Dense diag(d) + pair part [N, N] (what `mi_qeq_pair_coefficients` stores and `mi_qeq_apply` multiplies with)."""
    n = pos.shape[0]
    c = pair_coefficients(pos, sigma, cell, alpha, i, j, S, batch_idx, erfc_lr, distance_dtype)
    h = torch.zeros((n, n), dtype=F64, device=pos.device).index_put((i, j), c, accumulate=True)
    return h + torch.diag(diagonal(hardness, sigma))


def reciprocal_operator(pos, sigma, cell, alpha, k_vectors, batch_idx=None, half_space=True):
    """Dense k-space + self + background part of A [N, N] for a cell: zero between atoms of different systems.  k_vectors [K, 3] or [B, K, 3]."""
    n = pos.shape[0]
    sys_of = _systems(n, batch_idx, pos.device)
    cells = cell.reshape(-1, 3, 3).to(F64)
    kv = k_vectors.to(F64)
    kv = kv.unsqueeze(0).expand(cells.shape[0], -1, -1) if kv.dim() == 2 else kv
    al = alpha.to(F64).reshape(-1).expand(cells.shape[0]) if alpha.numel() == 1 else alpha.to(F64).reshape(-1)
    vol = torch.abs(torch.linalg.det(cells))
    s = torch.clamp(sigma.to(F64), min=0.0) ** 2
    p64 = pos.to(F64)
    a = torch.zeros((n, n), dtype=F64, device=pos.device)
    for b in range(cells.shape[0]):
        m = torch.nonzero(sys_of == b).flatten()
        if m.numel() == 0:
            continue
        k = kv[b]
        k2 = (k * k).sum(-1)
        ok = k2 > 1e-10
        k2s = torch.where(ok, k2, torch.ones_like(k2))
        green = torch.where(ok, torch.exp(-k2s / (4.0 * al[b] * al[b])) / k2s, torch.zeros_like(k2))
        ph = p64[m] @ k.T  # [n_b, K]
        cs, sn = torch.cos(ph), torch.sin(ph)
        blk = (2.0 if half_space else 1.0) * 4.0 * math.pi / vol[b] * ((cs * green) @ cs.T + (sn * green) @ sn.T)
        blk = blk - math.pi / (al[b] * al[b] * vol[b]) + 2.0 * math.pi / vol[b] * (s[m][:, None] + s[m][None, :])
        blk = blk - torch.diag(torch.full((m.numel(),), 1.0, dtype=F64, device=pos.device)) * (2.0 * al[b] / _SQRT_PI)
        a = a.index_put((m[:, None].expand(-1, m.numel()), m[None, :].expand(m.numel(), -1)), blk, accumulate=True)
    return a


def dense_operator(pos, sigma, hardness, cell, alpha, k_vectors, i, j, S, batch_idx=None, erfc_lr=torch.erfc, distance_dtype=F64, half_space=True):
    """H = diag(J) + A, every term: the Hessian of sum chi q + 1/2 sum J q^2 + E_el(q)."""
    h = real_space_operator(pos, sigma, hardness, cell, alpha, i, j, S, batch_idx, erfc_lr, distance_dtype)
    if cell is not None:
        h = h + reciprocal_operator(pos, sigma, cell, alpha, k_vectors, batch_idx, half_space)
    return h


def exact_gaussian_operator(pos, sigma, cell, kmax_index):
    """A_ij = (4 pi / V) sum_{k != 0} exp(-k^2 (sigma_i^2 + sigma_j^2) / 2) cos(k . r_ij) / k^2 over Miller indices in [-kmax, kmax]^3: the
    exact interaction of periodic Gaussian clouds (all sigma > 0) in a neutralising background.  No erfc, no Ewald split."""
    cell, pos, sigma = cell.reshape(3, 3).to(F64), pos.to(F64), sigma.to(F64)
    rec = 2.0 * math.pi * torch.linalg.inv(cell).T
    rng = torch.arange(-kmax_index, kmax_index + 1, dtype=F64)
    m = torch.stack(torch.meshgrid(rng, rng, rng, indexing="ij"), dim=-1).reshape(-1, 3)
    k = m[(m != 0).any(-1)] @ rec
    k2 = (k * k).sum(-1)
    n = pos.shape[0]
    a = torch.zeros((n, n), dtype=F64)
    for beg in range(0, k.shape[0], 20000):
        kc, k2c = k[beg:beg + 20000], k2[beg:beg + 20000]
        w = torch.exp(-0.5 * k2c[None, :] * (sigma * sigma)[:, None])  # [N, K]
        ph = pos @ kc.T
        cs, sn = torch.cos(ph) * w, torch.sin(ph) * w
        a = a + (cs / k2c) @ cs.T + (sn / k2c) @ sn.T
    return 4.0 * math.pi / torch.abs(torch.linalg.det(cell)) * a


def solve(h, chi, total_charge, batch_idx=None, num_systems=1):
    """(q [N], lambda [num_systems]) of chi + H q = lambda_s, sum_{i in s} q_i = Q_s: one (N_s + 1)-sized KKT solve per system."""
    n = chi.shape[0]
    sys_of = _systems(n, batch_idx, chi.device)
    total = torch.as_tensor(total_charge, dtype=F64, device=chi.device).reshape(-1)
    total = total.expand(num_systems) if total.numel() == 1 else total
    q = torch.zeros(n, dtype=F64, device=chi.device)
    lam = []
    for b in range(num_systems):
        m = torch.nonzero(sys_of == b).flatten()
        nb = m.numel()
        ones = torch.ones(nb, dtype=F64, device=chi.device)
        kkt = torch.cat([torch.cat([h[m][:, m], -ones[:, None]], dim=1),
                         torch.cat([ones, torch.zeros(1, dtype=F64, device=chi.device)])[None, :]], dim=0)  # [[H, -1], [1^T, 0]] (q; lambda) = (-chi; Q)
        rhs = torch.cat([-chi.to(F64)[m], total[b].reshape(1)])
        sol = torch.linalg.solve(kkt, rhs)
        q = q.index_put((m,), sol[:nb], accumulate=True)
        lam.append(sol[nb])
    return q, torch.stack(lam)


def projected_residual(h, chi, q, batch_idx=None, num_systems=1):
    """Per system ||P (chi + H q)||_2, P removing the per-system mean: zero exactly at the solution."""
    g = chi.to(F64) + h @ q.to(F64)
    sys_of = _systems(g.shape[0], batch_idx, g.device)
    out = []
    for b in range(num_systems):
        gb = g[sys_of == b]
        out.append(torch.linalg.norm(gb - gb.mean()) if gb.numel() else torch.zeros((), dtype=F64, device=g.device))
    return torch.stack(out)
