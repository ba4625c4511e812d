"""Dense float64 reference of the induced-dipole problem, built on the restatement of the point-dipole Ewald term (tests/dipole_reference.py).

    U(mu) = sum_i |mu_i|^2 / (2 a_i) + E_dip(q, mu) - sum_i mu_i . F_i,      E_dip(q, mu) = c(q) . mu + 1/2 mu^T T mu

T [3N, 3N] is the Hessian of `dipole_reference.energies(...).sum()` with respect to mu -- exact, because the energy is quadratic in mu -- and
c its gradient at mu = 0; b = -c + F.  H = diag(1 / a) + T on the polarisable atoms (a_i > 0); a non-polarisable atom has the identity row and
column, b = 0 and preconditioner entry 1.  Vectors are flattened atom-major: index 3 i + component.  Runs on any device."""
import torch

from tests import dipole_reference as DR

F64 = torch.float64


def quadratic_form(energy, n, device, differentiable=False):
    """(T [3n, 3n], c [n, 3]) of a scalar function `energy(mu)` that is quadratic in mu [n, 3]: its Hessian and its gradient at mu = 0.
    `differentiable` keeps the graph, so both can be differentiated with respect to whatever `energy` closes over."""
    mu = torch.zeros((n, 3), dtype=F64, device=device, requires_grad=True)
    (g,) = torch.autograd.grad(energy(mu), mu, create_graph=True)
    rows = [torch.autograd.grad(g.reshape(-1)[k], mu, retain_graph=True, create_graph=differentiable)[0].reshape(-1) for k in range(3 * n)]
    return torch.stack(rows), g if differentiable else g.detach()


def dipole_operator(pos, q, cell, alpha, entries=None, k_vectors=None, batch_idx=None, distance_dtype=F64, differentiable=False):
    """(T, c) of the parts of E_dip that are given: `entries` = (i, j, S) for the real-space sum, `k_vectors` for the explicit reciprocal sum.
    `differentiable`: with respect to pos and q."""
    if not differentiable:
        pos, q = pos.detach(), q.detach()
    pos, q = pos.to(F64), q.to(F64)

    def energy(mu):
        return DR.energies(pos, q, mu, cell.detach().to(F64), alpha, entries, k_vectors, batch_idx=batch_idx, distance_dtype=distance_dtype).sum()

    return quadratic_form(energy, pos.shape[0], pos.device, differentiable)


def expand(v):
    """[N] per-atom values -> [3N]."""
    return v.to(F64).repeat_interleave(3)


def system_matrix(T, polar):
    """H = diag(1 / a) + T on the polarisable atoms, identity rows and columns elsewhere."""
    ok = expand(polar) > 0
    a = torch.where(ok, expand(polar), torch.ones_like(expand(polar)))
    both = ok[:, None] & ok[None, :]
    return torch.where(both, T, torch.zeros_like(T)) + torch.diag(torch.where(ok, 1.0 / a, torch.ones_like(a)))


def right_hand_side(c, polar, field=None):
    """b [3N] = -c + F on the polarisable atoms, 0 elsewhere."""
    b = -c.to(F64) if field is None else field.to(F64) - c.to(F64)
    return torch.where(expand(polar) > 0, b.reshape(-1), torch.zeros_like(b.reshape(-1)))


def preconditioner(polar):
    return torch.where(expand(polar) > 0, expand(polar), torch.ones_like(expand(polar)))


def _members(n, batch_idx, nsys):
    sys_of = torch.zeros(n, dtype=torch.long) if batch_idx is None else batch_idx.long().cpu()
    return [torch.nonzero(sys_of.repeat_interleave(3) == s).flatten() for s in range(nsys)]


def solve(H, b, batch_idx=None, nsys=1):
    """mu [N, 3] = H^-1 b by `torch.linalg.solve`, block-diagonal per system (differentiable)."""
    mu = torch.zeros_like(b)
    for m in _members(b.shape[0] // 3, batch_idx, nsys):
        m = m.to(b.device)
        if m.numel():
            mu = mu.index_add(0, m, torch.linalg.solve(H[m][:, m], b[m]))
    return mu.reshape(-1, 3)


def pcg(H, b, d, tol, x0=None, max_iterations=500):
    """Plain Jacobi-preconditioned CG on ONE system: x += alpha p, r -= alpha H p, z = d r, p = z + beta p, started from x0 (default d b),
    stopped when |r| <= tol |b|.  Returns (x [N, 3], iterations)."""
    x = d * b if x0 is None else x0.reshape(-1).to(F64).clone()
    r = b - H @ x
    bb = float(b @ b)
    if bb == 0.0:
        return torch.zeros_like(b).reshape(-1, 3), 0
    z = d * r
    p, rz = z.clone(), r @ z
    it = 0
    while float(r @ r) > tol * tol * bb and it < max_iterations:
        hp = H @ p
        a = rz / (p @ hp)
        x, r = x + a * p, r - a * hp
        z = d * r
        rz_new = r @ z
        p, rz = z + (rz_new / rz) * p, rz_new
        it += 1
    return x.reshape(-1, 3), it


def energy(H, b, mu):
    """U(mu) = 1/2 mu^T H mu - b . mu (on the polarisable subspace this is the U of the module header)."""
    v = mu.reshape(-1).to(F64)
    return 0.5 * v @ (H @ v) - b @ v


def scaled_spectrum(H, polar):
    """Eigenvalues of D^1/2 H D^1/2, D = diag(a) (1 on non-polarisable atoms): what Jacobi-preconditioned CG sees."""
    s = torch.sqrt(preconditioner(polar))
    return torch.linalg.eigvalsh(s[:, None] * H * s[None, :])


def pair_tensors(pos, cell, alpha, i, j, S, batch_idx=None, distance_dtype=F64):
    """T_e [E, 3, 3] of every stored entry from the definition: the dipole-dipole energy of an entry is (mu_i . grad_i)(mu_j . grad_j) phi(R)
    = -mu_i . Hess_R[phi] . mu_j with phi = erfc(alpha r) / r, so T_e = -Hess_R phi, by two passes of autograd; zero for r <= 1e-8.
    `distance_dtype=torch.float32`: pair vector and distance take their float32 values (the kernel's arithmetic model for float32 inputs)."""
    n, dev = pos.shape[0], pos.device
    sys_of = DR._systems(n, batch_idx, dev)
    cells = cell.reshape(-1, 3, 3)
    al = DR._alpha(alpha, cells.shape[0], dev)[sys_of[i]]
    vec = lambda dt: pos.to(dt)[j] - pos.to(dt)[i] + torch.einsum("ea,eab->eb", S.to(dt), cells.to(dt)[sys_of[i]])  # noqa: E731
    low = vec(distance_dtype)
    r_val = torch.sqrt((low * low).sum(-1)).to(F64)
    keep = r_val > 1e-8
    unit = torch.zeros((i.shape[0], 3), dtype=F64, device=dev)
    unit[:, 0] = 1.0
    rv = torch.where(keep.unsqueeze(1), low.to(F64), unit).requires_grad_(True)
    r = torch.sqrt((rv * rv).sum(-1))
    r = r + (torch.where(keep, r_val, torch.ones_like(r_val)) - r).detach()
    phi = torch.erfc(al * r) / r
    (g,) = torch.autograd.grad(phi.sum(), rv, create_graph=True)
    hess = torch.stack([torch.autograd.grad(g[:, k].sum(), rv, retain_graph=True)[0] for k in range(3)], dim=1)
    return torch.where(keep[:, None, None], -hess, torch.zeros_like(hess))


def apply_rows(tensors, polar, i, j, x, y_in=None):
    """y_i = y_in,i + x_i / a_i + sum_{entries of row i} T_e x_j, row by row as stored (the list need not be full); entries with a
    non-polarisable atom at either end do not count and a non-polarisable atom has the identity row."""
    a = polar.to(F64)
    ok = a > 0
    t = torch.where((ok[i] & ok[j])[:, None, None], tensors, torch.zeros_like(tensors))
    y = (x / torch.where(ok, a, torch.ones_like(a)).unsqueeze(1)).index_add(0, i, torch.einsum("eab,eb->ea", t, x[j]))
    return y if y_in is None else y + y_in
