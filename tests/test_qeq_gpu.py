"""`charge_equilibration` and the `mi_qeq_*` entry points on the device against the dense float64 restatement (tests/qeq_reference.py, itself
checked in tests/test_qeq_reference_cpu.py) built from the same stored entries.

Bounds.  eps = 2^-52.  A stored coefficient is c = (lr - ec) / r with lr = erfc_AS(alpha r) (1 without a cell) and ec = erfc(r / g).  The
kernel and the reference evaluate the same expressions in float64, so a term differs by the rounding of its argument (r^2 with or without
fused multiply-adds, the square root, the scaling: <= 3 eps) times the condition number of erfc, x erfc'(x) / erfc(x) <= 2 x^2 + 1 <= 73 for
x < 6 (larger arguments are dropped or below 2e-17), plus a handful of roundings of its own:  |dc| <= (3 * 73 + 8) eps (|lr / r| + |ec / r|),
plus the difference between the device library's erfc and torch's.  Both are documented to a few ulp; LIBM_ERFC = 4 eps is allowed and the
difference actually seen is printed by `test_device_erfc_against_torch` (DESIGN 3.13 records it).  A row sum of K terms adds its own
summation error:  |dy_i| <= 2 (K_i + 8) eps sum_row (|lr / r| + |ec / r|) |x_j| + LIBM_ERFC sum_row |ec / r| |x_j|, the diagonal term and
y_in counted among the terms.  float32 positions: the pair vector may differ from the reference's float32 model by one float32 rounding
(the shift is added in another order), 2 * 2^-23 on r, times the same condition number.
"""
import functools
import math

import numpy as np
import pytest
import torch

from tests import gaussian_reference as GR
from tests import qeq_reference as R
from tests import systems as SY

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
EPS = 2.0 ** -52
LIBM_ERFC = 4.0 * EPS
COND = 3.0 * 73.0 + 8.0
F32_PAIR = 2.0 * 2.0 ** -23 * 74.0


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


def _cell(box, triclinic=True):
    return np.array([[box, 0, 0], [0.2 * box, 0.9 * box, 0], [0.1 * box, -0.15 * box, 1.1 * box]]) if triclinic else np.eye(3) * box


def _lists(i, j, S, n, m, fill):
    """Padded matrix [n, m] (+ shifts) and CSR (+ shifts) of entries sorted by row."""
    i, j, S = i.to(DEV), j.to(DEV), S.to(DEV)
    counts = torch.bincount(i, minlength=n)
    assert int(counts.max()) <= m
    start = torch.cumsum(counts, 0) - counts
    col = torch.arange(i.shape[0], device=DEV) - start[i]
    nm = torch.full((n, m), fill, dtype=torch.int32, device=DEV)
    sh = torch.zeros((n, m, 3), dtype=torch.int32, device=DEV)
    nm[i, col] = j.to(torch.int32)
    sh[i, col] = S.to(torch.int32)
    return nm, sh


def _csr(nm, sh, mask):
    i, j, S = GR.entries_from_matrix(nm, sh, mask)
    n = nm.shape[0]
    ptr = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    ptr[1:] = torch.cumsum(torch.bincount(i, minlength=n), 0)
    return torch.stack([i, j]).to(torch.int32).contiguous(), ptr, S.to(torch.int32).contiguous()


def _kw(f, fmt, shifts=True):
    if fmt == "matrix":
        return dict(neighbor_matrix=f["nm"], mask_value=f["n"], **(dict(neighbor_matrix_shifts=f["sh"]) if shifts else {}))
    return dict(neighbor_list=f["nl"], neighbor_ptr=f["ptr"], **(dict(neighbor_shifts=f["lsh"]) if shifts else {}))


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def _coefficients(pos, sigma, hard, cells, alpha, bi, nsys, idx, sh, nptr, m, mask):
    from nvalchemiops import _capi as C

    n, slots = pos.shape[0], idx.numel()
    coef = torch.full((slots,), float("nan"), dtype=F64, device=DEV)
    nbr = torch.full((slots,), -12345, dtype=torch.int32, device=DEV)
    diag = torch.full((n,), float("nan"), dtype=F64, device=DEV)
    rc = C.lib().mi_qeq_pair_coefficients(C.ptr(pos), C.ptr(sigma), C.ptr(hard), C.ptr(cells), C.ptr(alpha), C.ptr(bi), n, nsys, C.dtype_code(pos.dtype),
                                          C.ptr(idx), C.ptr(sh), C.ptr(nptr), m, mask, C.ptr(coef), C.ptr(nbr), C.ptr(diag), C.stream_of(pos))
    C.check(rc, "mi_qeq_pair_coefficients")
    return coef, nbr, diag


def _apply(coef, nbr, diag, x, y_in, bi, nsys, nptr, m, want_partial=True):
    from nvalchemiops import _capi as C

    n = x.shape[0]
    y = torch.full((n,), float("nan"), dtype=F64, device=DEV)
    part = torch.full((nsys, C.lib().mi_qeq_blocks(), 2), float("nan"), dtype=F64, device=DEV) if want_partial else None
    rc = C.lib().mi_qeq_apply(C.ptr(coef), C.ptr(nbr), C.ptr(diag), C.ptr(x), C.ptr(y_in), C.ptr(bi), n, nsys, C.ptr(nptr), m, C.ptr(y), C.ptr(part),
                              C.stream_of(x))
    C.check(rc, "mi_qeq_apply")
    return y, part


@functools.lru_cache(maxsize=None)
def _abi_case(name):
    """'box150': 150 atoms (not a multiple of 4) in a triclinic box 12, cutoff 7 (rows of ~125 entries: more than 64, no multiple of 64), M = 200
    (no multiple of 64), row 17 emptied by hand, padding as mask value (150), as -1 and as 157, three point charges.
    'small9': 9 atoms in a triclinic box 5 with cutoff 6 > L, so self-image entries (i, i, S != 0) occur; one point charge."""
    g = np.random.default_rng(11 if name == "box150" else 12)
    n, box, cutoff, m, images = (150, 12.0, 7.0, 200, 1) if name == "box150" else (9, 5.0, 6.0, 0, 2)
    cell = _cell(box)
    pos = g.uniform(0, 1, (n, 3)) @ cell
    sigma = g.uniform(0.3, 0.8, n)
    sigma[g.choice(n, 3 if name == "box150" else 1, replace=False)] = 0.0
    i, j, S = GR.brute_force_entries(pos, cell, cutoff, images)
    counts = np.bincount(i.numpy(), minlength=n)
    if name == "box150":
        assert counts.max() < m - 2 and ((counts > 64) & (counts % 64 != 0)).any()
    else:
        m = int(counts.max()) + 3
        assert bool(((i == j) & (S != 0).any(-1)).any()), "no self-image entries"
    assert m % 64 != 0
    nm, sh = _lists(i, j, S, n, m, n)
    if name == "box150":
        nm[17] = n
        assert bool((nm[:, -2:] == n).all())
        nm[:, -1] = -1      # out-of-range padding below ...
        nm[::2, -2] = n + 7  # ... and above [0, N), next to mask-value padding
    nl, ptr, lsh = _csr(nm, sh, n)
    if name == "box150":
        assert int(ptr[18] - ptr[17]) == 0
    return dict(n=n, m=m, pos=pos, cell=cell, sigma=sigma, hard=g.uniform(0.5, 1.5, n), nm=nm.contiguous(), sh=sh.contiguous(), nl=nl, ptr=ptr, lsh=lsh,
                x=_t(g.normal(size=n)), y_in=_t(g.normal(size=n)), alpha=0.35)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("fmt", ["matrix", "csr"])
@pytest.mark.parametrize("name", ["box150", "small9"])
def test_coefficients_and_product_against_the_dense_reference(name, fmt, dtype):
    f = _abi_case(name)
    n, m = f["n"], f["m"]
    P, Sg, Cl = _t(f["pos"], dtype), _t(f["sigma"], dtype), _t(f["cell"], dtype).reshape(1, 3, 3)
    Jd, al = _t(f["hard"]), torch.tensor([f["alpha"]], dtype=dtype, device=DEV)
    if fmt == "matrix":
        idx, sh, nptr, mm = f["nm"], f["sh"], None, m
        keep = (f["nm"] != n) & (f["nm"] >= 0) & (f["nm"] < n)
        rows = torch.arange(n, device=DEV).unsqueeze(1).expand(n, m).reshape(-1)
        ent = GR.entries_from_matrix(f["nm"], f["sh"], n)
    else:
        idx, sh, nptr, mm = f["nl"][1].contiguous(), f["lsh"], f["ptr"], 0
        ent = GR.entries_from_csr(f["nl"], f["ptr"], f["lsh"])
        keep, rows = torch.ones(idx.numel(), dtype=torch.bool, device=DEV), ent[0]
    coef, nbr, diag = _coefficients(P, Sg, Jd, Cl, al, None, 1, idx.contiguous(), sh.contiguous(), nptr, mm, n)
    model = dict(erfc_lr=R.erfc_as, distance_dtype=dtype)
    c_ref = R.pair_coefficients(P, Sg, Cl, al, *ent, **model)
    lr_mag, ec_mag = R.pair_coefficients(P, Sg, Cl, al, *ent, parts=True, **model)
    keep = keep.reshape(-1)
    # padding and skipped slots: coefficient exactly zero on the row's own index; every index is safe to gather with
    assert bool((coef[~keep] == 0).all()) and bool((nbr[~keep] == rows[~keep].to(torch.int32)).all())
    assert int(nbr.min()) >= 0 and int(nbr.max()) < n
    stored = c_ref != 0
    assert bool((nbr[keep][stored] == ent[1][stored].to(torch.int32)).all())
    tol = COND * EPS * (lr_mag + ec_mag) + LIBM_ERFC * ec_mag + (F32_PAIR * (lr_mag + ec_mag) if dtype == torch.float32 else 0.0)
    err = (coef[keep] - c_ref).abs()
    print(f"{name} {fmt} {dtype}: max |dc| / bound {float((err / tol.clamp(min=1e-300)).max()):.3f}, max |dc| {float(err.max()):.2e}")
    assert bool((err <= tol).all())
    d_ref = R.diagonal(Jd, Sg)
    assert bool(((diag - d_ref).abs() <= 4 * EPS * d_ref.abs()).all())
    # the product against the dense one, row by row
    x, y_in = f["x"], f["y_in"]
    y, part = _apply(coef, nbr, diag, x, y_in, None, 1, nptr, mm)
    h = R.real_space_operator(P, Sg, Jd, Cl, al, *ent, **model)
    y_ref = y_in + h @ x
    zeros = torch.zeros(n, dtype=F64, device=DEV)
    k_row = zeros.index_add(0, ent[0], torch.ones_like(c_ref))
    mag = zeros.index_add(0, ent[0], (lr_mag + ec_mag) * x[ent[1]].abs()) + (d_ref * x).abs() + y_in.abs()
    bound = 2.0 * (k_row + 8.0) * EPS * mag + LIBM_ERFC * zeros.index_add(0, ent[0], ec_mag * x[ent[1]].abs())
    if dtype == torch.float32:
        bound = bound + F32_PAIR * mag
    err = (y - y_ref).abs()
    print(f"{name} {fmt} {dtype}: max |dy| / bound {float((err / bound).max()):.3f}, max |dy| {float(err.max()):.2e} on |y| {float(y_ref.abs().max()):.2f}")
    assert bool((err <= bound).all())
    if name == "box150":
        assert float(k_row[17]) == 0 and float(y[17]) == float(y_in[17] + diag[17] * x[17])
    sums = part.sum(1)[0]
    assert abs(float(sums[0] - y.sum())) <= n * EPS * float(y.abs().sum()) and abs(float(sums[1] - (x * y).sum())) <= n * EPS * float((x * y).abs().sum())
    y0, none = _apply(coef, nbr, diag, x, None, None, 1, nptr, mm, want_partial=False)
    assert none is None and bool(((y0 + y_in - y).abs() <= 4 * EPS * (y.abs() + y_in.abs() + y0.abs())).all())


def test_device_erfc_against_torch():
    """The device library's erfc as the coefficient kernel calls it, read back through coefficients: atoms on a line, sigma = 0.5 for all (so
    g_ij = 1 and x = r exactly), a cell with alpha so large that erfc_AS(alpha r) underflows: c r = -erfc(r).  Printed for DESIGN 3.13."""
    r = np.concatenate([[0.0], np.arange(1, 1501) / 256.0])  # exactly representable distances from atom 0, up to 5.86
    n = r.shape[0]
    pos = np.zeros((n, 3))
    pos[:, 0] = r
    nm = torch.full((n, n - 1), n, dtype=torch.int32, device=DEV)
    nm[0] = torch.arange(1, n, dtype=torch.int32, device=DEV)
    sig, hard = torch.full((n,), 0.5, dtype=F64, device=DEV), torch.ones(n, dtype=F64, device=DEV)
    cell, alpha = (torch.eye(3, dtype=F64, device=DEV) * 100.0).reshape(1, 3, 3), torch.tensor([4000.0], dtype=F64, device=DEV)
    coef, _, _ = _coefficients(_t(pos), sig, hard, cell, alpha, None, 1, nm, None, None, n - 1, n)
    x = _t(r[1:])
    got = -coef[: n - 1] * x
    worst = {}
    for where, ref in (("torch on the device", torch.erfc(x)), ("torch on the host", torch.erfc(x.cpu()).to(DEV))):
        worst[where] = float(((got - ref).abs() / ref).max()) / EPS
        print(f"device erfc (through c r, two extra roundings) vs {where}: max relative difference {worst[where]:.2f} eps over {n - 1} arguments in (0, 5.86]")
    # the reference of these tests evaluates torch.erfc on the device; the host figure is printed for the record only
    assert worst["torch on the device"] <= LIBM_ERFC / EPS + 2.0  # + the roundings of c = ec / r and of c r


@pytest.mark.parametrize("fmt", ["matrix", "csr"])
def test_product_is_the_sum_of_the_public_charge_gradients(fmt):
    """`mi_qeq_apply` on random x (J = 0) = dE/dq of `ewald_real_space` + `gaussian_charge_correction` (self term on, background off) at charges x,
    on the same full list, within the bound of the product."""
    from nvalchemiops.interactions.electrostatics import ewald_real_space, gaussian_charge_correction

    g = np.random.default_rng(21)
    n, cell = 150, _cell(12.0)
    pos, sigma = g.uniform(0, 1, (n, 3)) @ cell, g.uniform(0.3, 0.8, n)
    sigma[[3, 70, 149]] = 0.0
    i, j, S = GR.brute_force_entries(pos, cell, 7.0, 1)
    nm, sh = _lists(i, j, S, n, 200, n)
    nl, ptr, lsh = _csr(nm, sh, n)
    f = dict(n=n, nm=nm, sh=sh, nl=nl, ptr=ptr, lsh=lsh)
    P, Sg, Cl, x = _t(pos), _t(sigma), _t(cell).reshape(1, 3, 3), _t(g.normal(size=n))
    al = torch.tensor([0.35], dtype=F64, device=DEV)
    idx, shifts, nptr, mm = (nm, sh, None, 200) if fmt == "matrix" else (nl[1].contiguous(), lsh, ptr, 0)
    coef, nbr, diag = _coefficients(P, Sg, torch.zeros(n, dtype=F64, device=DEV), Cl, al, None, 1, idx, shifts, nptr, mm, n)
    y, _ = _apply(coef, nbr, diag, x, None, None, 1, nptr, mm)
    want = (ewald_real_space(P, x, Cl, al, compute_charge_gradients=True, **_kw(f, fmt))[1]
            + gaussian_charge_correction(P, x, Sg, Cl, neutralizing_background=False, compute_charge_gradients=True, **_kw(f, fmt))[1])
    ent = (i.to(DEV), j.to(DEV), S.to(DEV))
    lr_mag, ec_mag = R.pair_coefficients(P, Sg, Cl, al, *ent, erfc_lr=R.erfc_as, parts=True)
    zeros = torch.zeros(n, dtype=F64, device=DEV)
    k_row = zeros.index_add(0, ent[0], torch.ones_like(lr_mag))
    mag = zeros.index_add(0, ent[0], (lr_mag + ec_mag) * x[ent[1]].abs()) + (R.diagonal(zeros, Sg) * x).abs()
    bound = 2.0 * (k_row + 8.0) * EPS * mag + LIBM_ERFC * zeros.index_add(0, ent[0], ec_mag * x[ent[1]].abs())
    err = (y - want).abs()
    print(f"operator identity {fmt}: max |dy| / bound {float((err / bound).max()):.3f}, max |dy| {float(err.max()):.2e} on {float(want.abs().max()):.2f}")
    assert bool((err <= bound).all())


# ---- solves ----------------------------------------------------------------------------------------------------------------------------
def _cluster(sizes, seed):
    """Clusters side by side (far apart is not needed: the all-pairs lists do not connect them), all-pairs FULL list per cluster."""
    g, pos, bi, ii, jj, sigma = SY.clusters(sizes, seed)  # (the recipe, shared with tests/layout_cases.py)
    n = len(pos)
    i, j = torch.as_tensor(ii), torch.as_tensor(jj)
    S_ = torch.zeros((i.shape[0], 3), dtype=torch.long)
    m = max(max(sizes) - 1, 1) + 2
    nm, sh = _lists(i, j, S_, n, m, n)
    nl, ptr, lsh = _csr(nm, sh, n)
    return dict(n=n, nsys=len(sizes), pos=_t(pos), bi=_t(bi), sigma=_t(sigma), chi=_t(g.normal(size=n)),
                hard=_t(g.uniform(1.0, 2.0, n)), nm=nm, sh=sh, nl=nl, ptr=ptr, lsh=lsh, ent=(i.to(DEV), j.to(DEV), S_.to(DEV)))


def _check_solution(out, h, chi, total, bi, nsys, tol, max_iterations, what):
    """The checks every solve gets, with the dense reference H: true residual, constraint, chemical potential, charges, iteration count."""
    q = out.charges.to(F64)
    n = q.shape[0]
    sys_of = torch.zeros(n, dtype=torch.long, device=DEV) if bi is None else bi.long()
    counts = torch.bincount(sys_of, minlength=nsys).to(F64)
    total = torch.as_tensor(total, dtype=F64, device=DEV).reshape(-1).expand(nsys)
    q_ref, lam_ref = R.solve(h, chi, total, bi, nsys)
    b_norm = R.projected_residual(h, chi, (total / counts)[sys_of], bi, nsys)
    res = R.projected_residual(h, chi, q, bi, nsys)
    factor = torch.where(b_norm > 0, res / (tol * b_norm.clamp(min=1e-300)), torch.zeros_like(res))
    print(f"{what}: true residual / (tolerance ||b||) per system {[round(float(v), 3) for v in factor]}, reported {[float(v) for v in out.residual]}, "
          f"iterations {out.iterations.tolist()}")
    assert bool((factor <= 10.0).all()), "the true residual drifted more than a factor 10 above the tolerance"
    qsum = torch.zeros(nsys, dtype=F64, device=DEV).index_add(0, sys_of, q)
    assert bool(((qsum - total).abs() <= 1e-12 * counts).all())
    assert bool((out.iterations <= max_iterations).all()) and not bool(torch.isnan(q).any())
    # |dq| <= ||(P H P)^-1|| ||residual|| and |dlambda| <= ||H|| |dq|: both follow from the residual bar through the spectrum of the dense H
    for b in range(nsys):
        m = torch.nonzero(sys_of == b).flatten()
        ev = torch.linalg.eigvalsh(h[m][:, m])
        assert float(ev.min()) > 0, "the test problem must be positive definite"
        dq = 10.0 * tol * float(b_norm[b]) / float(ev.min()) + 1e-14
        assert float((q[m] - q_ref[m]).abs().max()) <= dq, (what, b)
        assert abs(float(out.chemical_potential[b] - lam_ref[b])) <= float(ev.abs().max()) * dq, (what, b)
    return q_ref, lam_ref


def test_solve_cluster_single_and_batched():
    from nvalchemiops.interactions.electrostatics import charge_equilibration as qeq

    tol = 1e-10
    f = _cluster((24,), 31)
    h = R.dense_operator(f["pos"], f["sigma"], f["hard"], None, None, None, *f["ent"])
    for fmt in ("matrix", "csr"):
        out = qeq(f["pos"], f["chi"], f["hard"], f["sigma"], total_charge=-0.7, tolerance=tol, return_info=True, **_kw(f, fmt, shifts=False))
        assert out.charges.dtype == F64 and out.charges.shape == (24,) and out.chemical_potential.shape == (1,)
        _check_solution(out, h, f["chi"], -0.7, None, 1, tol, 200, f"cluster 24 {fmt}")
    plain = qeq(f["pos"], f["chi"], f["hard"], f["sigma"], total_charge=-0.7, tolerance=tol, **_kw(f, "csr", shifts=False))
    assert isinstance(plain, torch.Tensor) and torch.equal(plain, out.charges)
    # three clusters of 37, 90 and 1 atoms with different total charges in one call; the number of systems comes from total_charge
    f = _cluster((37, 90, 1), 32)
    total = torch.tensor([1.5, 0.0, -0.4], dtype=F64, device=DEV)
    h = R.dense_operator(f["pos"], f["sigma"], f["hard"], None, None, None, *f["ent"], batch_idx=f["bi"])
    for fmt in ("matrix", "csr"):
        out = qeq(f["pos"], f["chi"], f["hard"], f["sigma"], total_charge=total, batch_idx=f["bi"], tolerance=tol, return_info=True,
                  **_kw(f, fmt, shifts=False))
        _check_solution(out, h, f["chi"], total, f["bi"], 3, tol, 200, f"clusters 37 + 90 + 1 {fmt}")
        assert float(out.charges[-1]) == -0.4 and int(out.iterations[2]) == 0, "the one-atom system carries its total charge"
    # fp32 positions: same solver arithmetic, charges in float32
    out32 = qeq(f["pos"].float(), f["chi"].float(), f["hard"].float(), f["sigma"].float(), total_charge=total, batch_idx=f["bi"], tolerance=tol,
                **_kw(f, "matrix", shifts=False))
    # a relative perturbation F32_PAIR of the coefficients moves the charges by at most cond(H) times that
    ev = torch.linalg.eigvalsh(h)
    assert out32.dtype == torch.float32
    assert float((out32.double() - out.charges).abs().max()) <= float(ev.max() / ev.min()) * F32_PAIR * float(out.charges.abs().max())


@functools.lru_cache(maxsize=None)
def _periodic_batch():
    """Two periodic systems in one batch: 40 atoms in a triclinic box 9 (charged), 55 atoms in a cubic box 10 (neutral); cutoff 6."""
    g = np.random.default_rng(41)
    parts, off, ii, jj, ss = [], 0, [], [], []
    for nb, cell in ((40, _cell(9.0)), (55, _cell(10.0, triclinic=False))):
        pos = g.uniform(0, 1, (nb, 3)) @ cell
        i, j, S = GR.brute_force_entries(pos, cell, 6.0, 1)
        ii.append(i + off); jj.append(j + off); ss.append(S)
        parts.append((pos, cell))
        off += nb
    n = off
    i, j, S = torch.cat(ii), torch.cat(jj), torch.cat(ss)
    nm, sh = _lists(i, j, S, n, int(torch.bincount(i).max()) + 5, n)
    nl, ptr, lsh = _csr(nm, sh, n)
    sigma = g.uniform(0.3, 0.8, n)
    sigma[[5, 60]] = 0.0
    return dict(n=n, pos=_t(np.concatenate([p for p, _ in parts])), cells=_t(np.stack([c for _, c in parts])), sigma=_t(sigma),
                bi=_t(np.array([0] * 40 + [1] * 55, dtype=np.int32)), chi=_t(g.normal(size=n)), hard=_t(g.uniform(1.0, 2.0, n)),
                nm=nm, sh=sh, nl=nl, ptr=ptr, lsh=lsh, ent=(i.to(DEV), j.to(DEV), S.to(DEV)))


def test_solve_periodic_ewald_batch():
    """reciprocal='ewald' with the same alpha, k-vectors and polynomial erfc in the reference: the operators agree to rounding."""
    from nvalchemiops.interactions.electrostatics import charge_equilibration as qeq, generate_k_vectors_ewald_summation

    f, tol = _periodic_batch(), 1e-10
    alpha = torch.tensor([0.45, 0.42], dtype=F64, device=DEV)
    kv = generate_k_vectors_ewald_summation(f["cells"], 3.2)
    total = torch.tensor([1.3, 0.0], dtype=F64, device=DEV)
    h = R.dense_operator(f["pos"], f["sigma"], f["hard"], f["cells"], alpha, kv, *f["ent"], batch_idx=f["bi"], erfc_lr=R.erfc_as)
    for fmt in ("matrix", "csr"):
        out = qeq(f["pos"], f["chi"], f["hard"], f["sigma"], f["cells"], total_charge=total, batch_idx=f["bi"], reciprocal="ewald", alpha=alpha,
                  k_vectors=kv, tolerance=tol, return_info=True, **_kw(f, fmt))
        _check_solution(out, h, f["chi"], total, f["bi"], 2, tol, 200, f"periodic ewald batch {fmt}")


# 3 x the 5.761e-8 measured on the MI355X (the CPU oracle's PME as the reciprocal operator of the dense reference gives the same 5.76e-8: it is
# the deviation of PME itself at this mesh)
PME_BAR = 1.73e-7


def test_solve_pme_against_ewald():
    """The same 60-atom box solved with reciprocal='pme' on a fine mesh (64^3, order 4, spacing 0.16 A) and with reciprocal='ewald' (k sum
    converged: k_cutoff 5.4 at alpha 0.45).  The deviation is that of PME itself (see PME_BAR)."""
    from nvalchemiops.interactions.electrostatics import charge_equilibration as qeq

    g = np.random.default_rng(51)
    n, cell = 60, _cell(10.0)
    pos = g.uniform(0, 1, (n, 3)) @ cell
    i, j, S = GR.brute_force_entries(pos, cell, 9.0, 1)
    nm, sh = _lists(i, j, S, n, int(torch.bincount(i).max()) + 1, n)
    f = dict(n=n, nm=nm, sh=sh)
    args = (_t(pos), _t(g.normal(size=n)), _t(g.uniform(1.0, 2.0, n)), _t(g.uniform(0.3, 0.8, n)), _t(cell).reshape(1, 3, 3))
    common = dict(total_charge=0.8, alpha=0.45, tolerance=1e-11, **_kw(f, "matrix"))
    q_ew = qeq(*args, reciprocal="ewald", k_cutoff=5.4, **common)
    q_pme = qeq(*args, reciprocal="pme", mesh_dimensions=(64, 64, 64), spline_order=4, **common)
    dev = float((q_pme - q_ew).abs().max()) / float(q_ew.abs().max())
    print(f"pme vs ewald charges: max deviation {dev:.3e} of max |q| {float(q_ew.abs().max()):.3f}")
    assert dev <= PME_BAR


def test_zero_right_hand_side_and_symmetric_lattice():
    """Equal chi, equal J, equal sigma on a 3 x 3 x 3 simple cubic lattice whose rows list the same offsets in the same order, neutral: the
    gradient at the uniform start is chi itself, b = 0 exactly, the system is done at iteration 0, the charges are the uniform solution
    (exactly zero) and nothing is NaN.  (With Q != 0 on such a lattice b is not zero but rounding noise of the reciprocal sum, which no solver
    can reduce by a factor 1e-8: that call raises ChargeEquilibrationError -- DESIGN 3.13.)"""
    from nvalchemiops.interactions.electrostatics import charge_equilibration as qeq

    grid = np.array([(a, b, c) for a in range(3) for b in range(3) for c in range(3)])
    offsets = np.array([(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)])
    target = grid[:, None, :] + offsets[None, :, :]
    S = np.floor_divide(target, 3)
    wrapped = target - 3 * S
    nm = _t((wrapped[..., 0] * 9 + wrapped[..., 1] * 3 + wrapped[..., 2]).astype(np.int32))
    sh = _t(S.astype(np.int32))
    n = 27
    pos, cell = _t(grid * 3.0, F64), (torch.eye(3, dtype=F64, device=DEV) * 9.0).reshape(1, 3, 3)
    chi, hard = torch.full((n,), 0.5, dtype=F64, device=DEV), torch.full((n,), 1.25, dtype=F64, device=DEV)
    kw = dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=n, alpha=0.4, mesh_dimensions=(18, 18, 18), return_info=True)
    out = qeq(pos, chi, hard, 0.5, cell, total_charge=0.0, **kw)
    assert bool((out.charges == 0).all()) and int(out.iterations[0]) == 0 and float(out.residual[0]) == 0.0
    assert not bool(torch.isnan(out.chemical_potential).any()) and abs(float(out.chemical_potential[0]) - 0.5) <= 1e-15
    assert not bool(torch.isnan(out.charges).any()) and not bool(torch.isnan(out.residual).any())
    # a warm start cannot talk such a system out of its solution: with b = 0 the uniform start is returned whatever `initial_charges` holds
    rough = torch.linspace(-1.0, 1.0, n, dtype=F64, device=DEV)
    out = qeq(pos, chi, hard, 0.5, cell, total_charge=0.0, initial_charges=rough, **kw)
    assert bool((out.charges == 0).all()) and int(out.iterations[0]) == 0 and float(out.residual[0]) == 0.0


def test_warm_start_and_non_convergence():
    from nvalchemiops.interactions.electrostatics import ChargeEquilibrationError, charge_equilibration as qeq

    f = _periodic_batch()
    total = torch.tensor([1.3, 0.0], dtype=F64, device=DEV)
    kw = dict(total_charge=total, batch_idx=f["bi"], alpha=0.45, mesh_dimensions=(24, 24, 24), return_info=True, **_kw(f, "matrix"))
    args = (f["pos"], f["chi"], f["hard"], f["sigma"], f["cells"])
    cold = qeq(*args, tolerance=1e-11, **kw)
    assert int(cold.iterations.min()) > 4
    # the solution (shifted off the constraint: the start is put back on it) is accepted at the first check, before any iteration counts
    warm = qeq(*args, tolerance=1e-8, initial_charges=cold.charges + 0.25, **kw)
    assert warm.iterations.tolist() == [0, 0] and float(warm.residual.max()) <= 1e-8
    assert float((warm.charges - cold.charges).abs().max()) <= 1e-13
    # a poor start still converges to the same charges
    rough = qeq(*args, tolerance=1e-11, initial_charges=torch.zeros_like(cold.charges), **kw)
    assert float((rough.charges - cold.charges).abs().max()) <= 1e-9 * float(cold.charges.abs().max())
    with pytest.raises(ChargeEquilibrationError, match=r"within 1 iterations for system 0 \(residual [0-9.e+-]+\), system 1 \(residual"):
        qeq(*args, tolerance=1e-11, max_iterations=1, **kw)


def test_bit_reproducible_between_calls_and_streams():
    """What is free of atomics is bit-reproducible: a solve without a cell (three clusters in one batch; two calls and one on a side stream)
    and the product with its per-system partials through the C ABI.  A periodic solve is not claimed to be: its reciprocal-space calls add
    with atomics in arrival order."""
    from nvalchemiops.interactions.electrostatics import charge_equilibration as qeq

    f = _cluster((37, 90, 1), 32)
    kw = dict(total_charge=torch.tensor([1.5, 0.0, -0.4], dtype=F64, device=DEV), batch_idx=f["bi"], tolerance=1e-10, **_kw(f, "csr", shifts=False))
    args = (f["pos"], f["chi"], f["hard"], f["sigma"])
    a, b = qeq(*args, **kw), qeq(*args, **kw)
    w = qeq(*args, initial_charges=torch.zeros_like(a), **kw), qeq(*args, initial_charges=torch.zeros_like(a), **kw)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = qeq(*args, **kw)
    side.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(w[0], w[1]) and float(a.abs().max()) > 0
    p = _abi_case("box150")
    P, Sg, Cl = _t(p["pos"]), _t(p["sigma"]), _t(p["cell"]).reshape(1, 3, 3)
    coef, nbr, diag = _coefficients(P, Sg, _t(p["hard"]), Cl, torch.tensor([0.35], dtype=F64, device=DEV), None, 1, p["nm"], p["sh"], None, p["m"], p["n"])
    coef2, nbr2, diag2 = _coefficients(P, Sg, _t(p["hard"]), Cl, torch.tensor([0.35], dtype=F64, device=DEV), None, 1, p["nm"], p["sh"], None, p["m"], p["n"])
    assert torch.equal(coef, coef2) and torch.equal(nbr, nbr2) and torch.equal(diag, diag2)
    (y1, p1), (y2, p2) = (_apply(coef, nbr, diag, p["x"], p["y_in"], None, 1, None, p["m"]) for _ in range(2))
    assert torch.equal(y1, y2) and torch.equal(p1, p2)


# ---- autograd --------------------------------------------------------------------------------------------------------------------------
# Relative to the largest |component| of each gradient; a decade above what was measured on the MI355X with both solves at tolerance 1e-12:
#   periodic  chi 8.86e-13, J 4.14e-13, Q 1.45e-13, sigma 2.28e-13; positions and cell: not measured with this reference yet -- their bar is
#             tolerance 1e-12 x the condition number of P H P (< 100 here), the reasoning behind the level of the measured ones; the test prints them
#   cluster   chi 6.35e-16, J 2.00e-15, Q 8.46e-14, sigma 2.33e-15, positions 2.76e-15
# The reference of the periodic case carries the arithmetic model of `ewald_real_space`: erfc evaluated by the A-S polynomial, differentiated
# analytically (`R.erfc_as_analytic_derivative`).  Differentiating the polynomial itself instead moves the position and cell gradients by
# 1.16e-6 and 2.10e-6 -- measured once that way -- which would hide an error of that size in the implicit backward.
GRAD_BARS = {"periodic": dict(chi=8.9e-12, hard=4.2e-12, total=1.5e-12, sigma=2.3e-12, pos=1e-10, cell=1e-10),
             "cluster": dict(chi=6.4e-15, hard=2.0e-14, total=8.5e-13, sigma=2.4e-14, pos=2.8e-14)}


def _grad_errors(got, ref):
    return {k: float((got[k] - ref[k]).abs().max()) / float(ref[k].abs().max()) for k in ref}


@pytest.mark.parametrize("case", ["periodic", "cluster"])
def test_gradients_against_the_reference_autograd(case):
    """L = sum_i w_i q_i with random w; gradients with respect to chi, J, Q, positions, sigma and (periodic) the cell against autograd through
    the dense reference's KKT solve.  Solves at tolerance 1e-12.  Each bar is relative to the largest |component| of that gradient
    (GRAD_BARS, with where each comes from); second order is refused."""
    from nvalchemiops.interactions.electrostatics import charge_equilibration as qeq, generate_k_vectors_ewald_summation

    g = np.random.default_rng(61 if case == "periodic" else 62)
    if case == "periodic":
        n, cell = 20, _cell(8.0)
        pos = g.uniform(0, 1, (n, 3)) @ cell
        i, j, S = GR.brute_force_entries(pos, cell, 7.0, 1)
    else:
        n, cell = 12, None
        pos = g.uniform(0, 4.5, (n, 3))
        a, c = np.nonzero(~np.eye(n, dtype=bool))
        i, j, S = torch.as_tensor(a), torch.as_tensor(c), torch.zeros((a.shape[0], 3), dtype=torch.long)
    nm, sh = _lists(i, j, S, n, int(torch.bincount(i).max()) + 2, n)
    ent = (i.to(DEV), j.to(DEV), S.to(DEV))
    sigma0 = g.uniform(0.4, 0.8, n)
    leaf = lambda a: _t(a, F64).requires_grad_(True)  # noqa: E731
    w = _t(g.normal(size=n))
    names = ["chi", "hard", "total", "pos", "sigma"] + (["cell"] if cell is not None else [])

    def inputs():
        d = dict(chi=leaf(g0["chi"]), hard=leaf(g0["hard"]), total=leaf(np.array([0.6])), pos=leaf(pos), sigma=leaf(sigma0))
        if cell is not None:
            d["cell"] = leaf(cell.reshape(1, 3, 3))
        return d

    g0 = dict(chi=g.normal(size=n), hard=g.uniform(1.0, 2.0, n))
    alpha = torch.tensor([0.5], dtype=F64, device=DEV)
    # the reference
    r = inputs()
    if cell is not None:
        kv = generate_k_vectors_ewald_summation(r["cell"], 4.0)
        h = R.dense_operator(r["pos"], r["sigma"], r["hard"], r["cell"], alpha, kv, *ent, erfc_lr=R.erfc_as_analytic_derivative)
    else:
        h = R.dense_operator(r["pos"], r["sigma"], r["hard"], None, None, None, *ent)
    q_ref, _ = R.solve(h, r["chi"], r["total"])
    ref = dict(zip(names, torch.autograd.grad((w * q_ref).sum(), [r[k] for k in names])))
    # the solver
    d = inputs()
    lists = dict(neighbor_matrix=nm, mask_value=n, tolerance=1e-12, total_charge=d["total"])
    if cell is not None:
        q = qeq(d["pos"], d["chi"], d["hard"], d["sigma"], d["cell"], neighbor_matrix_shifts=sh, reciprocal="ewald", alpha=alpha, k_cutoff=4.0, **lists)
    else:
        q = qeq(d["pos"], d["chi"], d["hard"], d["sigma"], **lists)
    assert float((q - q_ref).abs().max()) <= 1e-9 * float(q_ref.abs().max())
    got = dict(zip(names, torch.autograd.grad((w * q).sum(), [d[k] for k in names], retain_graph=True)))
    errs = _grad_errors(got, ref)
    print(f"gradients {case}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k in names:
        assert got[k].shape == d[k].shape and got[k].dtype == F64
    for k, v in errs.items():
        assert v <= GRAD_BARS[case][k], (k, v)
    with pytest.raises(NotImplementedError, match="second derivatives"):
        torch.autograd.grad((w * q).sum(), d["chi"], create_graph=True)
