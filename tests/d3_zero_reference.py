"""Float64 torch restatement of DFT-D3 with zero damping, D3(0) / D3M(0): the checker of `dftd3_zero`.

Written from the definition of the damping, not from the kernel, on the pieces of tests/atm_reference.py (`enumerate_pairs`,
`c6_interpolate`, the strain construction of the virial, the `work_dtype` convention).  For every stored directed pair (i, j) at distance r
of the full list with cutoff `list_cutoff`:

    q      = 3 r4r2_i r4r2_j
    R0     = r0ab[Z_i, Z_j]                                  (a pair with R0 <= 0 contributes nothing)
    f_n(r) = 1 / (1 + 6 (r / (rs_n R0) + beta R0)^(-alpha_n))    n = 6, 8;  alpha_6 = alpha, alpha_8 = alpha + 2
    E_ij   = -C6_ij(CN_i, CN_j) (s6 f_6 / r^6 + s8 q f_8 / r^8) sw(r)      (nothing if C6 < 1e-12)
    E      = 1/2 sum_ij E_ij

with the coordination numbers summed over the same list and sw the S5 switch of `dftd3` (1 below `s5_on`, 0 above `s5_off`, the quintic
1 - 10 t^3 + 15 t^4 - 6 t^5 between; off unless `s5_off > s5_on`).  Energy is one differentiable scalar per system; forces are minus its
autograd gradient through the positions INCLUDING the coordination-number dependence of C6; the virial is minus the derivative with
respect to a symmetric strain applied to positions and cell.  Small systems only.

    reference(pos, numbers, tables, r0ab, rs6, s8, list_cutoff, ..., term="two_body", work_dtype=torch.float64 | torch.float32)

`work_dtype=torch.float32` evaluates every per-pair quantity (and its derivative) in float32 while every SUM stays float64 -- the
arithmetic model of the kernels; the distance between the two evaluations is what float32 pair arithmetic costs on a given system.  f_n is
evaluated as the logistic function of alpha_n ln x - ln 6 (the same number), so that a close contact, whose x^-alpha overflows float32,
gives f_n = 0 with a zero derivative in either mode.

`term="atm"` is the checker of `dftd3_zero_atm`: the three-body term of tests/atm_reference.py (same enumeration of triples, same weights,
same C9 and angular factor) with the radii R0_XY = rs9 r0ab[Z_X, Z_Y]; a triple with a pair whose r0ab entry is <= 0 contributes nothing.
    reference(pos, numbers, tables, r0ab, None, None, list_cutoff, three_body_cutoff=..., rs9=4/3, s9=1, alpha=16, term="atm")
"""
import numpy as np
import torch

from tests import atm_reference as A


def synthetic_r0ab(nz, seed=11, lo=3.5, hi=9.0):
    """A seeded symmetric table of pair cutoff radii in [lo, hi] Bohr with row / column 0 (padding) zero.  Not Grimme's table: the
    arithmetic does not care, and users supply their own (as they do for c6)."""
    g = np.random.default_rng(seed)
    a = g.uniform(lo, hi, (nz, nz))
    a = 0.5 * (a + a.T)
    a[0, :] = 0.0
    a[:, 0] = 0.0
    return a.astype(np.float32)


def _switch(r, on, off):
    if not off > on:
        return torch.ones_like(r)
    t = (r - on) / (off - on)
    poly = 1.0 - (10.0 * t ** 3 - 15.0 * t ** 4 + 6.0 * t ** 5)
    return torch.where(r <= on, torch.ones_like(r), torch.where(r >= off, torch.zeros_like(r), poly))


def _system(pos, numbers, tables, r0ab, cell, rs6, rs8, s6, s8, alpha, beta, list_cutoff, k1, k3, s5_on, s5_off, wd):
    """One system: (energy, forces[N,3], virial[3,3] or None, cn[N]) as float64 numpy."""
    f64 = torch.float64
    n = len(pos)
    z = torch.as_tensor(np.asarray(numbers), dtype=torch.long)
    rcov = torch.as_tensor(tables["rcov"], dtype=wd)
    r4r2 = torch.as_tensor(tables["r4r2"], dtype=wd)
    c6ab = torch.as_tensor(tables["c6ab"], dtype=wd)
    cn_ref = torch.as_tensor(tables["cn_ref"], dtype=wd)
    radii = torch.as_tensor(np.asarray(r0ab), dtype=wd)
    nz = len(rcov)
    real_np = (np.asarray(numbers) > 0) & (np.asarray(numbers) < nz)
    x0 = torch.tensor(np.asarray(pos, np.float64), dtype=f64, requires_grad=True)
    eps = torch.zeros(3, 3, dtype=f64, requires_grad=True)
    strain = torch.eye(3, dtype=f64) + 0.5 * (eps + eps.T)
    x = x0 @ strain
    h = None if cell is None else torch.as_tensor(np.asarray(cell, np.float64).reshape(3, 3)) @ strain

    li, lj, ls = A.enumerate_pairs(pos, cell, list_cutoff)
    m = real_np[li] & real_np[lj]
    li, lj, ls = li[m], lj[m], ls[m]
    tli, tlj = torch.as_tensor(li), torch.as_tensor(lj)
    d = x[tlj] - x[tli]  # float64 difference (+ shift), then the working dtype -- as the kernels cast
    if h is not None:
        d = d + torch.as_tensor(ls, dtype=f64) @ h
    r = d.to(wd).norm(dim=1)
    count = 1.0 / (1.0 + torch.exp(-k1 * ((rcov[z[tli]] + rcov[z[tlj]]) / r - 1.0)))
    cn64 = torch.zeros(n, dtype=f64).index_add(0, tli, count.to(f64))
    cn = cn64.to(wd)

    c6 = A.c6_interpolate(cn[tli], cn[tlj], z[tli], z[tlj], c6ab, cn_ref, k3)
    q = 3.0 * r4r2[z[tli]] * r4r2[z[tlj]]
    R0 = radii[z[tli], z[tlj]]
    live = (R0 > 0) & ~(c6 < 1e-12)
    R0s = torch.where(live, R0, torch.ones_like(R0))
    rs = torch.where(live, r, torch.ones_like(r))  # dead pairs: keep their (discarded) branch free of inf / nan gradients

    def term(n_pow, rs_n, alpha_n):
        xx = rs / (rs_n * R0s) + beta * R0s
        # 1 / (1 + 6 x^-alpha) written as the logistic function of alpha ln x - ln 6: the same number, and its autograd derivative is
        # alpha f (1 - f) / x -- finite and 0 where the power itself (and autograd's -6 f^2 alpha x^(-alpha - 1)) would overflow
        f = torch.sigmoid(alpha_n * torch.log(xx) - float(np.log(6.0)))
        return f / rs ** n_pow

    e = -c6 * (s6 * term(6, rs6, alpha) + s8 * q * term(8, rs8, alpha + 2.0)) * _switch(rs, s5_on, s5_off)
    e = torch.where(live, e, torch.zeros_like(e))
    total = 0.5 * e.to(f64).sum()
    if total.requires_grad:
        total.backward()
    forces = -x0.grad.numpy() if x0.grad is not None else np.zeros((n, 3))
    virial = None
    if cell is not None:
        virial = -eps.grad.numpy() if eps.grad is not None else np.zeros((3, 3))
        virial = 0.5 * (virial + virial.T)
    return float(total.detach()), forces, virial, cn64.detach().numpy()


def _system_atm(pos, numbers, tables, r0ab, cell, rs9, s9, alpha, list_cutoff, three_body_cutoff, k1, k3, wd, chunk=1_000_000):
    """One system, three-body term: the construction of tests/atm_reference.py::_system with table radii."""
    f64 = torch.float64
    n = len(pos)
    z = torch.as_tensor(np.asarray(numbers), dtype=torch.long)
    rcov = torch.as_tensor(tables["rcov"], dtype=wd)
    c6ab = torch.as_tensor(tables["c6ab"], dtype=wd)
    cn_ref = torch.as_tensor(tables["cn_ref"], dtype=wd)
    radii = torch.as_tensor(np.asarray(r0ab), dtype=wd)
    nz = len(rcov)
    real_np = (np.asarray(numbers) > 0) & (np.asarray(numbers) < nz)
    x0 = torch.tensor(np.asarray(pos, np.float64), dtype=f64, requires_grad=True)
    eps = torch.zeros(3, 3, dtype=f64, requires_grad=True)
    strain = torch.eye(3, dtype=f64) + 0.5 * (eps + eps.T)
    x = x0 @ strain
    h = None if cell is None else torch.as_tensor(np.asarray(cell, np.float64).reshape(3, 3)) @ strain

    def vectors(i, j, s):
        d = x[j] - x[i]
        if h is not None:
            d = d + torch.as_tensor(s, dtype=f64) @ h
        return d.to(wd)

    li, lj, ls = A.enumerate_pairs(pos, cell, list_cutoff)
    m = real_np[li] & real_np[lj]
    li, lj, ls = li[m], lj[m], ls[m]
    tli, tlj = torch.as_tensor(li), torch.as_tensor(lj)
    rl = vectors(li, lj, ls).norm(dim=1)
    count = 1.0 / (1.0 + torch.exp(-k1 * ((rcov[z[tli]] + rcov[z[tlj]]) / rl - 1.0)))
    cn64 = torch.zeros(n, dtype=f64).index_add(0, tli, count.to(f64))
    cn = cn64.to(wd)

    keep = np.linalg.norm(A._np_vectors(pos, cell, li, lj, ls), axis=1) < three_body_cutoff
    ti, tj, ts = li[keep], lj[keep], ls[keep]
    vec_np = A._np_vectors(pos, cell, ti, tj, ts)
    counts = np.bincount(ti, minlength=n)
    start = np.concatenate([[0], np.cumsum(counts)])
    vp, vq = [], []
    free = cell is None
    for c in range(n):
        k = counts[c]
        if k < 2:
            continue
        p, q = np.triu_indices(k, 1)
        p = p + start[c]; q = q + start[c]
        djk = vec_np[q] - vec_np[p]
        r2 = (djk * djk).sum(1)
        ok = (r2 < three_body_cutoff ** 2) & (r2 >= 1e-24)
        if free:  # each triple once: centre < j < k (rows are sorted by j)
            ok &= tj[p] > c
        vp.append(p[ok]); vq.append(q[ok])
    vp = np.concatenate(vp) if vp else np.zeros(0, np.int64)
    vq = np.concatenate(vq) if vq else np.zeros(0, np.int64)
    weight = 1.0 if free else 1.0 / 3.0  # periodic: every triple is met from its three vertices
    tti, ttj = torch.as_tensor(ti), torch.as_tensor(tj)
    total_val = 0.0
    for lo in range(0, max(len(vp), 1), chunk):
        p = torch.as_tensor(vp[lo:lo + chunk]); q = torch.as_tensor(vq[lo:lo + chunk])
        if len(p) == 0:
            break
        R = vectors(ti, tj, ts)
        c6_pair = A.c6_interpolate(cn[tti], cn[ttj], z[tti], z[ttj], c6ab, cn_ref, k3)
        r0_pair = rs9 * radii[z[tti], z[ttj]]
        cj, ck = ttj[p], ttj[q]
        rij, rik = R[p], R[q]
        rjk = rik - rij
        a = (rij * rij).sum(1); b = (rik * rik).sum(1); c = (rjk * rjk).sum(1)
        P = torch.sqrt(a) * torch.sqrt(b) * torch.sqrt(c)
        c6_ij, c6_ik = c6_pair[p], c6_pair[q]
        c6_jk = A.c6_interpolate(cn[cj], cn[ck], z[cj], z[ck], c6ab, cn_ref, k3)
        r0_jk = rs9 * radii[z[cj], z[ck]]
        live = (c6_ij >= 1e-12) & (c6_ik >= 1e-12) & (c6_jk >= 1e-12) & (r0_pair[p] > 0) & (r0_pair[q] > 0) & (r0_jk > 0)
        one = torch.ones_like(c6_ij)
        c9 = torch.sqrt(torch.where(live, c6_ij, one) * torch.where(live, c6_ik, one) * torch.where(live, c6_jk, one))
        ang = 0.375 * (a + b - c) * (a + c - b) * (b + c - a) / P ** 5 + 1.0 / P ** 3
        r0 = torch.where(live, r0_pair[p] * r0_pair[q] * r0_jk, one)
        fdamp = 1.0 / (1.0 + 6.0 * (r0 / P) ** (alpha / 3.0))
        e = torch.where(live, s9 * c9 * ang * fdamp, torch.zeros_like(ang))
        part = weight * e.to(f64).sum()
        if part.requires_grad:
            part.backward(retain_graph=True)
        total_val += float(part.detach())
    forces = -x0.grad.numpy() if x0.grad is not None else np.zeros((n, 3))
    virial = None
    if cell is not None:
        virial = -eps.grad.numpy() if eps.grad is not None else np.zeros((3, 3))
        virial = 0.5 * (virial + virial.T)
    triples = len(vp) if free else len(vp) // 3
    return total_val, forces, virial, cn64.detach().numpy(), triples


def reference(pos, numbers, tables, r0ab, rs6, s8, list_cutoff, rs8=1.0, alpha=None, beta=0.0, k1=16.0, k3=-4.0, s6=1.0, s5_on=1e10,
              s5_off=1e10, cell=None, batch_idx=None, term="two_body", work_dtype=torch.float64, three_body_cutoff=None, rs9=4.0 / 3.0, s9=1.0):
    """Returns dict(energy[B], forces[N,3], virial[B,3,3] (periodic only, else None), cn[N]) as float64 numpy arrays, and `triples`: the
    unordered triples the three-body term enumerated (0 for term "two_body").
    `cell`: None, [3,3] or [B,3,3]; `batch_idx`: None or [N] (systems are evaluated one by one).  `alpha` defaults to 14 for the two-body
    term and to 16 for the three-body term, as in the package; rs6 / s8 / rs8 / beta / s6 / the S5 window are not read for term="atm"."""
    if term not in ("two_body", "atm"):
        raise ValueError(term)
    if alpha is None:
        alpha = 14.0 if term == "two_body" else 16.0
    pos = np.asarray(pos, np.float64)
    numbers = np.asarray(numbers)
    n = len(pos)
    bi = np.zeros(n, np.int64) if batch_idx is None else np.asarray(batch_idx, np.int64)
    cells = None if cell is None else np.asarray(cell, np.float64).reshape(-1, 3, 3)
    nsys = (int(bi.max()) + 1 if n else 1) if cells is None else len(cells)
    energy = np.zeros(nsys)
    forces = np.zeros((n, 3))
    cn = np.zeros(n)
    virial = None if cells is None else np.zeros((nsys, 3, 3))
    triples = 0
    for s in range(nsys):
        sel = np.nonzero(bi == s)[0]
        if len(sel) == 0:
            continue
        cs = None if cells is None else cells[s]
        if term == "atm":
            e, f, v, c, k = _system_atm(pos[sel], numbers[sel], tables, r0ab, cs, rs9, s9, alpha, list_cutoff,
                                        three_body_cutoff if three_body_cutoff is not None else list_cutoff, k1, k3, work_dtype)
            triples += k
        else:
            e, f, v, c = _system(pos[sel], numbers[sel], tables, r0ab, cs, rs6, rs8, s6, s8, alpha, beta, list_cutoff, k1, k3, s5_on, s5_off,
                                 work_dtype)
        energy[s] = e
        forces[sel] = f
        cn[sel] = c
        if virial is not None:
            virial[s] = v
    return dict(energy=energy, forces=forces, virial=virial, cn=cn, triples=triples)
