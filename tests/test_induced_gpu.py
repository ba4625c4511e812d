"""`induced_dipoles` and the `mi_induced_*` entry points on the device against the dense float64 reference (tests/induced_reference.py, itself
checked in tests/test_induced_reference_cpu.py) built from the same stored entries and the same k-vectors.

Bars.  The stored operator follows the arithmetic model of `dp_pair_kernel`, so the product holds the bars tests/test_dipole_gpu.py holds for
that model: 1e-11 of the largest |value| for fp64 inputs, 1e-6 for float32 positions against the reference's float32-distance mode.  A solve
to tolerance tol leaves ||b - H mu|| <= tol ||b|| in exact arithmetic; the recurred residual drifts from the true one, so a factor 10 is
allowed (as tests/test_qeq_gpu.py allows it), and |mu - mu_ref| <= ||H^-1|| ||residual|| follows through the spectrum of the dense H.

Measured figures stand in the comments of the PME and gradient tests; DESIGN 3.22 has the iteration counts."""
import functools

import numpy as np
import pytest
import torch

from tests import gaussian_reference as GR
from tests import induced_cases as IC
from tests import induced_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
F32_PAIR = 2.0 * 2.0 ** -23 * 74.0  # the float32 pair bar of tests/test_qeq_gpu.py: one float32 rounding of r times the condition of erfc


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


def _matrix(i, j, S, n, m, fill):
    """Padded matrix [n, m] (+ shifts) of entries sorted by row."""
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


def _kw(f, fmt):
    if fmt == "matrix":
        return dict(neighbor_matrix=f["nm"], neighbor_matrix_shifts=f["sh"], mask_value=f["n"])
    return dict(neighbor_list=f["nl"], neighbor_ptr=f["ptr"], neighbor_shifts=f["lsh"])


def _api():
    from nvalchemiops.interactions.electrostatics import InducedDipoleError, induced_dipoles

    return induced_dipoles, InducedDipoleError


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def _tensors(pos, polar, cells, alpha, bi, nsys, idx, sh, nptr, m, mask):
    from nvalchemiops import _capi as C

    n, slots = pos.shape[0], idx.numel()
    ten = torch.full((C.lib().mi_induced_tensor_words(), slots), float("nan"), dtype=F64, device=DEV)
    nbr = torch.full((slots,), -12345, dtype=torch.int32, device=DEV)
    diag, pre = torch.full((n,), float("nan"), dtype=F64, device=DEV), torch.full((n,), float("nan"), dtype=F64, device=DEV)
    rc = C.lib().mi_induced_pair_tensors(C.ptr(pos), C.ptr(polar), C.ptr(cells), C.ptr(alpha), C.ptr(bi), n, nsys, C.dtype_code(pos.dtype), C.ptr(idx),
                                         C.ptr(sh), C.ptr(nptr), m, mask, slots, C.ptr(ten), C.ptr(nbr), C.ptr(diag), C.ptr(pre), C.stream_of(pos))
    C.check(rc, "mi_induced_pair_tensors")
    return ten, nbr, diag, pre


def _apply(ten, nbr, diag, x, y_in, bi, nsys, nptr, m, want_partial=True):
    from nvalchemiops import _capi as C

    n = x.shape[0]
    y = torch.full((n, 3), float("nan"), dtype=F64, device=DEV)
    part = torch.full((nsys, C.lib().mi_induced_blocks()), float("nan"), dtype=F64, device=DEV) if want_partial else None
    rc = C.lib().mi_induced_apply(C.ptr(ten), C.ptr(nbr), C.ptr(diag), C.ptr(x), C.ptr(y_in), C.ptr(bi), n, nsys, C.ptr(nptr), m, nbr.numel(),
                                  C.ptr(y), C.ptr(part), C.stream_of(x))
    C.check(rc, "mi_induced_apply")
    return y, part


@functools.lru_cache(maxsize=None)
def _operator_case(two_systems):
    """40 atoms in a triclinic box of edge 9, every image within 14 (two shells): about 600 entries per row, several trips of the unrolled
    loop and a tail.  Rows 10 .. 15 are cut to k * 64 * depth - 1, + 0, + 1 entries for k = 1, 2 (the list need not be full for the product),
    row 3 is empty (all padding in the matrix), the first entry of row 7 is the atom itself at zero distance, the matrix is three columns
    wider than the longest row and carries the mask value, -1 and N + 7 as padding.  With `two_systems` the 27-atom lattice case follows as a
    second system with its own cell and alpha."""
    from nvalchemiops import _capi as C

    depth = C.lib().mi_induced_unroll_depth()
    g = np.random.default_rng(71)
    cell = IC.triclinic(9.0)
    pos = g.uniform(0, 1, (40, 3)) @ cell
    i, j, S = GR.brute_force_entries(pos, cell, 14.0, 2)
    counts = np.bincount(i.numpy(), minlength=40)
    lengths = {10 + k: v for k, v in enumerate([64 * depth - 1, 64 * depth, 64 * depth + 1, 128 * depth - 1, 128 * depth, 128 * depth + 1])}
    assert counts[list(lengths)].min() >= 128 * depth + 1, counts
    start = np.cumsum(counts) - counts
    col = np.arange(i.shape[0]) - start[i.numpy()]
    keep = np.ones(i.shape[0], dtype=bool)
    for row, length in lengths.items():
        keep &= ~((i.numpy() == row) & (col >= length))
    keep &= i.numpy() != 3
    first7 = int(start[7])
    j[first7], S[first7] = 7, 0
    i, j, S = i[keep], j[keep], S[keep]
    assert bool(((i == j) & (S != 0).any(-1)).any()), "no self-image entries"
    cells, alpha, bi, polar = [cell], [0.45], None, g.uniform(0.05, 0.15, 40) * 8.0
    if two_systems:
        c = IC.lattice("l27")
        i2, j2, S2 = IC.entries("l27")
        pos, cells, alpha = np.concatenate([pos, c["pos"]]), cells + [c["cell"]], alpha + [0.4]
        i, j, S = torch.cat([i, i2 + 40]), torch.cat([j, j2 + 40]), torch.cat([S, S2])
        bi, polar = _t(np.array([0] * 40 + [1] * 27, dtype=np.int32)), np.concatenate([polar, c["polar"]])
    n = pos.shape[0]
    m = int(torch.bincount(i).max()) + 3
    nm, sh = _matrix(i, j, S, n, m, n)
    assert bool((nm[:, -3:] == n).all()) and bool((nm[3] == n).all())
    nm[:, -1] = -1
    nm[::2, -2] = n + 7
    nl, ptr, lsh = _csr(nm, sh, n)
    assert int(ptr[4] - ptr[3]) == 0 and [int(ptr[r + 1] - ptr[r]) for r in lengths] == list(lengths.values())
    return dict(n=n, m=m, nsys=len(cells), pos=pos, cells=np.stack(cells), alpha=np.array(alpha), bi=bi, polar=polar, nm=nm.contiguous(),
                sh=sh.contiguous(), nl=nl, ptr=ptr, lsh=lsh, ent=(i.to(DEV), j.to(DEV), S.to(DEV)), x=_t(g.normal(size=(n, 3))),
                y_in=_t(g.normal(size=(n, 3))))


def _layout(f, fmt):
    if fmt == "matrix":
        return f["nm"], f["sh"], None, f["m"]
    return f["nl"][1].contiguous(), f["lsh"], f["ptr"], 0


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("fmt", ["matrix", "csr"])
@pytest.mark.parametrize("two_systems", [False, True], ids=["one", "two"])
def test_product_against_the_dense_reference(two_systems, fmt, dtype):
    from nvalchemiops.interactions.electrostatics import ewald_dipole_real_space

    f = _operator_case(two_systems)
    n, nsys, bi = f["n"], f["nsys"], f["bi"]
    P, A, Cl, al = _t(f["pos"], dtype), _t(f["polar"], dtype), _t(f["cells"], dtype), _t(f["alpha"], dtype)
    idx, sh, nptr, mm = _layout(f, fmt)
    ten, nbr, diag, pre = _tensors(P, A, Cl, al, bi, nsys, idx, sh, nptr, mm, n)
    assert int(nbr.min()) >= 0 and int(nbr.max()) < n and not bool(torch.isnan(ten).any())
    if fmt == "matrix":  # padding slots: zero coefficients on the row's own index
        pad = ((f["nm"] == n) | (f["nm"] < 0) | (f["nm"] >= n)).reshape(-1)
        rows = torch.arange(n, device=DEV).unsqueeze(1).expand(n, mm).reshape(-1)
        assert bool((ten[:, pad] == 0).all()) and bool((nbr[pad] == rows[pad].to(torch.int32)).all())
    assert bool(((diag - 1.0 / A.to(F64)).abs() <= 4 * 2.0 ** -52 / A.to(F64)).all()) and torch.equal(pre, A.to(F64))
    rel = 1e-11 if dtype == torch.float64 else 1e-6
    t_ref = R.pair_tensors(P, Cl, al.to(F64), *f["ent"], batch_idx=bi, distance_dtype=dtype)
    x, y_in = f["x"], f["y_in"]
    y, part = _apply(ten, nbr, diag, x, y_in, bi, nsys, nptr, mm)
    y_ref = R.apply_rows(t_ref, A, f["ent"][0], f["ent"][1], x, y_in)
    err, scale = float((y - y_ref).abs().max()), float(y_ref.abs().max())
    print(f"product {fmt} {dtype} systems {nsys}: rel err {err / scale:.2e} (bar {rel:.0e})")
    assert err <= rel * scale + 1e-14
    assert torch.equal(y[3], y_in[3] + diag[3] * x[3]), "an empty row adds nothing"
    # without y_in and without the diagonal it is the dipole gradient of the public real-space function at zero charges
    y0, none = _apply(ten, nbr, diag, x, None, bi, nsys, nptr, mm, want_partial=False)
    assert none is None
    kw = _kw(f, "matrix" if fmt == "matrix" else "list")
    dg = ewald_dipole_real_space(P, torch.zeros(n, dtype=dtype, device=DEV), x.to(dtype), Cl, al, batch_idx=bi, compute_dipole_gradients=True, **kw)[1]
    if dtype == torch.float64:
        ident = float((y0 - diag.unsqueeze(1) * x - dg).abs().max())
        print(f"product - x / a against ewald_dipole_real_space dipole_grads: rel err {ident / float(dg.abs().max()):.2e}")
        assert ident <= 1e-11 * float(dg.abs().max()) + 1e-14
    # per-system partials of x . y
    sys_of = torch.zeros(n, dtype=torch.long, device=DEV) if bi is None else bi.long()
    for s in range(nsys):
        own = sys_of == s
        want = float((x[own] * y[own]).sum())
        assert abs(float(part[s].sum()) - want) <= 3 * n * 2.0 ** -52 * float((x[own] * y[own]).abs().sum())
    # bit-identical between two calls
    ten2, nbr2, diag2, pre2 = _tensors(P, A, Cl, al, bi, nsys, idx, sh, nptr, mm, n)
    y2, part2 = _apply(ten2, nbr2, diag2, x, y_in, bi, nsys, nptr, mm)
    assert torch.equal(ten, ten2) and torch.equal(nbr, nbr2) and torch.equal(diag, diag2) and torch.equal(pre, pre2)
    assert torch.equal(y, y2) and torch.equal(part, part2)


def test_non_polarisable_atoms_have_identity_rows_and_empty_columns():
    f = _operator_case(False)
    n = f["n"]
    polar = f["polar"].copy()
    polar[[1, 12]] = 0.0
    polar[20] = float("nan")
    polar[30] = -0.3
    frozen = [1, 12, 20, 30]
    P, A, Cl, al = _t(f["pos"]), _t(polar), _t(f["cells"]), _t(f["alpha"])
    idx, sh, nptr, mm = _layout(f, "csr")
    ten, nbr, diag, pre = _tensors(P, A, Cl, al, None, 1, idx, sh, nptr, mm, n)
    assert bool((diag[frozen] == 1).all()) and bool((pre[frozen] == 1).all())
    i, j = f["ent"][0], f["ent"][1]
    dead = torch.isin(i, _t(frozen)) | torch.isin(j, _t(frozen))
    assert bool((ten[:, dead] == 0).all()) and bool((nbr[dead] == i[dead].to(torch.int32)).all())
    y, _ = _apply(ten, nbr, diag, f["x"], None, None, 1, nptr, mm)
    assert torch.equal(y[frozen], f["x"][frozen])
    y_ref = R.apply_rows(R.pair_tensors(P, Cl, al, *f["ent"]), torch.nan_to_num(A, nan=0.0), i, j, f["x"])
    assert float((y - y_ref).abs().max()) <= 1e-11 * float(y_ref.abs().max())


# ---- solves ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch_case():
    """One batch: the 27-atom and the 64-atom lattice case and a one-atom system in a triclinic box of edge 6 whose list holds only its own
    images (cutoff 11, three shells).  Atoms 4, 40 and 70 are not polarisable; every atom sees an external field (the lone atom has no other
    source: the field of its own images vanishes by symmetry).  Explicit Ewald with one alpha and one k set per system; the dense reference
    is built once from the same entries and k-vectors."""
    from nvalchemiops.interactions.electrostatics import generate_k_vectors_ewald_summation

    g = np.random.default_rng(81)
    a27, a64 = IC.lattice("l27"), IC.lattice("l64")
    lone_cell = IC.triclinic(6.0)
    lone_pos = np.array([[1.0, 2.0, 3.0]])
    parts = [(a27["pos"], a27["cell"], IC.entries("l27")), (a64["pos"], a64["cell"], IC.entries("l64")),
             (lone_pos, lone_cell, GR.brute_force_entries(lone_pos, lone_cell, 11.0, 3))]
    off, ii, jj, ss = 0, [], [], []
    for pos, _, (i, j, S) in parts:
        ii.append(i + off); jj.append(j + off); ss.append(S)
        off += pos.shape[0]
    n = off
    i, j, S = torch.cat(ii), torch.cat(jj), torch.cat(ss)
    assert bool((i[-1] == n - 1) and (j[i == n - 1] == n - 1).all()), "the lone atom sees only its own images"
    nm, sh = _matrix(i, j, S, n, int(torch.bincount(i).max()) + 5, n)
    nl, ptr, lsh = _csr(nm, sh, n)
    polar = np.concatenate([a27["polar"], a64["polar"], [0.8]])
    polar[[4, 40, 70]] = 0.0
    f = dict(n=n, nsys=3, frozen=[4, 40, 70], pos=_t(np.concatenate([p for p, _, _ in parts])), cells=_t(np.stack([c for _, c, _ in parts])),
             q=_t(np.concatenate([a27["q"], a64["q"], [0.7]])), polar=_t(polar), field=_t(0.1 * g.normal(size=(n, 3))),
             bi=_t(np.array([0] * 27 + [1] * 64 + [2], dtype=np.int32)), alpha=_t(np.array([0.45, 0.45, 0.5])),
             nm=nm, sh=sh, nl=nl, ptr=ptr, lsh=lsh, ent=(i.to(DEV), j.to(DEV), S.to(DEV)))
    f["kv"] = generate_k_vectors_ewald_summation(f["cells"], 3.2)
    T, c = R.dipole_operator(f["pos"], f["q"], f["cells"], f["alpha"], f["ent"], f["kv"], batch_idx=f["bi"])
    f["T"], f["c"] = T, c
    f["H"], f["b"] = R.system_matrix(T, f["polar"]), R.right_hand_side(c, f["polar"], f["field"])
    return f


def _per_system(v, bi, nsys):
    """[nsys] Euclidean norms of a [N, 3] array per system."""
    return torch.sqrt(torch.zeros(nsys, dtype=F64, device=DEV).index_add(0, bi.long(), (v.to(F64) ** 2).sum(1)))


def _check_solution(out, H, b, polar, bi, nsys, tol, what, x0=None):
    """The checks every solve gets, with the dense reference H: true residual, dipoles, iteration count against the reference PCG."""
    mu = out.dipoles.to(F64)
    n = mu.shape[0]
    bi = torch.zeros(n, dtype=torch.int32, device=DEV) if bi is None else bi
    assert not bool(torch.isnan(mu).any())
    b_norm = _per_system(b.reshape(-1, 3), bi, nsys)
    res = _per_system((b - H @ mu.reshape(-1)).reshape(-1, 3), bi, nsys)
    factor = torch.where(b_norm > 0, res / (tol * b_norm.clamp(min=1e-300)), torch.zeros_like(res))
    mu_ref = R.solve(H, b, bi, nsys)
    d = R.preconditioner(polar)
    counts = []
    for s in range(nsys):
        m = torch.nonzero(bi.long().repeat_interleave(3) == s).flatten()
        ev = torch.linalg.eigvalsh(H[m][:, m])
        assert float(ev.min()) > 0, "the test problem must be positive definite"
        bound = 10.0 * tol * float(b_norm[s]) / float(ev.min()) + 1e-14
        assert float((mu.reshape(-1)[m] - mu_ref.reshape(-1)[m]).abs().max()) <= bound, (what, s)
        counts.append(R.pcg(H[m][:, m], b[m], d[m], tol, None if x0 is None else x0.reshape(-1)[m])[1])
    print(f"{what}: true residual / (tolerance ||b||) per system {[round(float(v), 3) for v in factor]}, reported {[float(v) for v in out.residual]}, "
          f"iterations {out.iterations.tolist()} (reference PCG {counts})")
    assert bool((factor <= 10.0).all()), "the true residual drifted more than a factor 10 above the tolerance"
    assert all(int(got) <= ref + 2 for got, ref in zip(out.iterations.tolist(), counts)), (out.iterations.tolist(), counts)
    return mu_ref


@pytest.mark.parametrize("fmt", ["matrix", "list"])
def test_solve_explicit_ewald_batch(fmt):
    from nvalchemiops.interactions.electrostatics import ewald_dipole_correction

    ind, _ = _api()
    f, tol = _batch_case(), 1e-10
    common = dict(batch_idx=f["bi"], **_kw(f, fmt))
    out = ind(f["pos"], f["q"], f["polar"], f["cells"], external_field=f["field"], reciprocal="ewald", alpha=f["alpha"], k_vectors=f["kv"],
              tolerance=tol, return_info=True, **common)
    assert out.dipoles.dtype == F64 and out.dipoles.shape == (f["n"], 3) and out.polarization_energy.shape == (3,)
    _check_solution(out, f["H"], f["b"], f["polar"], f["bi"], 3, tol, f"ewald batch {fmt}")
    mu = out.dipoles
    assert bool((mu[f["frozen"]] == 0).all()) and float(mu[-1].abs().max()) > 0
    plain = ind(f["pos"], f["q"], f["polar"], f["cells"], external_field=f["field"], reciprocal="ewald", alpha=f["alpha"], k_vectors=f["kv"],
                tolerance=tol, **common)
    assert isinstance(plain, torch.Tensor) and torch.equal(plain, mu)
    # stationarity with the public functions at the returned dipoles
    e, dg = ewald_dipole_correction(f["pos"], f["q"], mu, f["cells"], f["alpha"], f["kv"], compute_dipole_gradients=True, **common)
    ok = (f["polar"] > 0).unsqueeze(1)
    a = torch.where(ok, f["polar"].unsqueeze(1), torch.ones_like(mu))
    grad = torch.where(ok, mu / a + dg - f["field"], torch.zeros_like(mu))
    b_norm = _per_system(f["b"].reshape(-1, 3), f["bi"], 3)
    stat = _per_system(grad, f["bi"], 3) / (tol * b_norm)
    print(f"stationarity with the public functions / (tolerance ||b||): {[round(float(v), 3) for v in stat]}")
    assert bool((stat <= 10.0).all())
    # U at the solution
    per_atom = torch.where(ok[:, 0], (mu * mu).sum(1) / (2.0 * a[:, 0]), torch.zeros_like(e)) + e - (mu * f["field"]).sum(1)
    u = torch.zeros(3, dtype=F64, device=DEV).index_add(0, f["bi"].long(), per_atom)
    print(f"polarization energy {out.polarization_energy.tolist()} against U {u.tolist()}")
    assert bool(((out.polarization_energy - u).abs() <= 100.0 * tol * u.abs() + 1e-14).all())


@functools.lru_cache(maxsize=None)
def _single_case(name="l27"):
    """One lattice case as a single system, explicit Ewald (alpha 0.45, k_cutoff 3.2), the dense reference built once."""
    c = IC.lattice(name)
    i, j, S = IC.entries(name)
    n = c["n"]
    nm, sh = _matrix(i, j, S, n, int(torch.bincount(i).max()) + 1, n)
    nl, ptr, lsh = _csr(nm, sh, n)
    f = dict(n=n, pos=_t(c["pos"]), cell=_t(c["cell"]).reshape(1, 3, 3), q=_t(c["q"]), polar=_t(c["polar"]), nm=nm, sh=sh, nl=nl, ptr=ptr, lsh=lsh,
             ent=(i.to(DEV), j.to(DEV), S.to(DEV)), kv=IC.k_vectors(c["cell"], IC.EWALD["k_cutoff"]).to(DEV))
    f["T"], f["c"] = R.dipole_operator(f["pos"], f["q"], f["cell"], IC.EWALD["alpha"], f["ent"], f["kv"])
    f["H"], f["b"] = R.system_matrix(f["T"], f["polar"]), R.right_hand_side(f["c"], f["polar"])
    return f


def _ewald(f):
    return dict(reciprocal="ewald", alpha=IC.EWALD["alpha"], k_vectors=f["kv"], **_kw(f, "matrix"))


# The deviation of PME itself: the dense reference solved with tests/pme_dipole_reference.py as its reciprocal operator (float64, on the
# CPU, matrix-free PCG to 1e-12) against the dense reference with the explicit k sum, max |dmu| / max |mu| on the 64-atom case at alpha 0.45:
#     mesh 64^3:  order 4  2.260e-5,  order 5  4.001e-7        (mesh 48^3: 4.281e-5 and 1.140e-6)
# The bar is 3 x that figure, as PME_BAR of tests/test_qeq_gpu.py was set.  Measured on the MI355X: 2.260e-5 and 4.001e-7, the same figures.
PME_MESH = (64, 64, 64)
PME_REFERENCE = {4: 2.260e-5, 5: 4.001e-7}


@pytest.mark.parametrize("order", [4, 5])
def test_solve_pme_against_ewald(order):
    ind, _ = _api()
    f = _single_case("l64")
    args = (f["pos"], f["q"], f["polar"], f["cell"])
    mu_ew = ind(*args, tolerance=1e-11, **_ewald(f))
    mu_pme = ind(*args, tolerance=1e-11, reciprocal="pme", alpha=IC.EWALD["alpha"], mesh_dimensions=PME_MESH, spline_order=order, **_kw(f, "matrix"))
    dev = float((mu_pme - mu_ew).abs().max()) / float(mu_ew.abs().max())
    print(f"pme (mesh {PME_MESH}, order {order}) vs ewald dipoles: max deviation {dev:.3e} of max |mu| {float(mu_ew.abs().max()):.3f} "
          f"(reference {PME_REFERENCE[order]:.3e})")
    assert dev <= 3.0 * PME_REFERENCE[order]


def test_zero_right_hand_side():
    """q = 0 and no field: b = 0 exactly, the system is done at iteration 0 and the dipoles are exactly zero, with and without a warm start,
    for both reciprocal operators."""
    ind, _ = _api()
    f = _single_case()
    zero = torch.zeros_like(f["q"])
    for kw in (_ewald(f), dict(alpha=0.45, mesh_dimensions=(24, 24, 24), **_kw(f, "matrix"))):
        for extra in (dict(), dict(initial_dipoles=torch.ones_like(f["pos"]))):
            out = ind(f["pos"], zero, f["polar"], f["cell"], return_info=True, **kw, **extra)
            assert bool((out.dipoles == 0).all()) and int(out.iterations[0]) == 0 and float(out.residual[0]) == 0.0
            assert float(out.polarization_energy[0]) == 0.0
            assert not any(bool(torch.isnan(t.to(F64)).any()) for t in out)


def test_external_field_only_warm_start_and_non_convergence():
    ind, Err = _api()
    f, tol = _single_case(), 1e-10
    g = torch.Generator(device="cpu").manual_seed(5)
    field = (0.2 * torch.randn((f["n"], 3), dtype=F64, generator=g)).to(DEV)
    args = (f["pos"], torch.zeros_like(f["q"]), 0.9 * float(f["polar"].min()), f["cell"])  # a number as polarizability
    uniform = torch.full_like(f["polar"], 0.9 * float(f["polar"].min()))
    H, b = R.system_matrix(f["T"], uniform), R.right_hand_side(torch.zeros_like(f["c"]), uniform, field)
    out = ind(*args, external_field=field, tolerance=tol, return_info=True, **_ewald(f))
    _check_solution(out, H, b, uniform, None, 1, tol, "external field only")
    # charges and a field; the solution as warm start is accepted before any iteration counts
    args = (f["pos"], f["q"], f["polar"], f["cell"])
    H, b = f["H"], R.right_hand_side(f["c"], f["polar"], field)
    cold = ind(*args, external_field=field, tolerance=1e-11, return_info=True, **_ewald(f))
    mu_ref = _check_solution(cold, H, b, f["polar"], None, 1, 1e-11, "charges and field")
    assert int(cold.iterations[0]) > 4
    warm = ind(*args, external_field=field, tolerance=1e-8, initial_dipoles=cold.dipoles, return_info=True, **_ewald(f))
    assert warm.iterations.tolist() == [0] and float(warm.residual[0]) <= 1e-8 and torch.equal(warm.dipoles, cold.dipoles)
    # a poor start converges to the same dipoles
    poor = (0.5 * torch.randn((f["n"], 3), dtype=F64, generator=g)).to(DEV)
    rough = ind(*args, external_field=field, tolerance=tol, initial_dipoles=poor, return_info=True, **_ewald(f))
    lam = float(torch.linalg.eigvalsh(H).min())
    assert float((rough.dipoles - mu_ref).abs().max()) <= 10.0 * tol * float(b.norm()) / lam + 1e-14
    assert abs(float(rough.residual[0])) <= tol
    with pytest.raises(Err, match=r"no convergence to tolerance 1e-11 within 1 iterations for system 0 \(residual [0-9.e+-]+\)"):
        ind(*args, external_field=field, tolerance=1e-11, max_iterations=1, **_ewald(f))


def test_float32_positions():
    """float32 inputs: the stored operator is perturbed by one float32 rounding of the pair vector (F32_PAIR relative), which moves the dipoles by
    at most cond(H) times that.  The tolerance is 1e-6: the reciprocal-space gradients come back in float32."""
    ind, _ = _api()
    f = _single_case()
    mu64 = ind(f["pos"], f["q"], f["polar"], f["cell"], tolerance=1e-10, **_ewald(f))
    kw = dict(_ewald(f), k_vectors=f["kv"].float())
    out = ind(f["pos"].float(), f["q"].float(), f["polar"].float(), f["cell"].float(), tolerance=1e-6, return_info=True, **kw)
    assert out.dipoles.dtype == torch.float32 and out.polarization_energy.dtype == torch.float32
    ev = torch.linalg.eigvalsh(f["H"])
    dev = float((out.dipoles.double() - mu64).abs().max()) / float(mu64.abs().max())
    print(f"float32 dipoles against float64: {dev:.2e} of max |mu| (bar {float(ev.max() / ev.min()) * F32_PAIR:.2e}), iterations {out.iterations.tolist()}")
    assert dev <= float(ev.max() / ev.min()) * F32_PAIR


def test_breakdown_is_reported():
    """Two atoms at distance d with a = d^3 in a box of edge 8, no charges: head to tail along the axis the pair has curvature
    1 / a - 2 / d^3 < 0.  With that eigenvector as the external field the first search direction has p.Hp < 0."""
    ind, Err = _api()
    d = 1.5
    cell = np.eye(3) * 8.0
    pos = np.array([[3.0, 4.0, 4.0], [3.0 + d, 4.0, 4.0]])
    i, j, S = GR.brute_force_entries(pos, cell, 7.0, 1)
    nm, sh = _matrix(i, j, S, 2, int(torch.bincount(i).max()), 2)
    P, Cl, polar = _t(pos), _t(cell).reshape(1, 3, 3), torch.full((2,), d**3, dtype=F64, device=DEV)
    kv = IC.k_vectors(cell, 3.0).to(DEV)
    T, _ = R.dipole_operator(P, torch.zeros(2, dtype=F64, device=DEV), Cl, 0.45, (i.to(DEV), j.to(DEV), S.to(DEV)), kv)
    ev, vec = torch.linalg.eigh(R.system_matrix(T, polar))
    assert float(ev[0]) < 0, "the dense H must have a negative eigenvalue"
    field = vec[:, 0].reshape(2, 3).contiguous()
    with pytest.raises(Err, match="not positive definite for system 0") as err:
        ind(P, torch.zeros(2, dtype=F64, device=DEV), polar, Cl, external_field=field, reciprocal="ewald", alpha=0.45, k_vectors=kv,
            neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    assert "no convergence" not in str(err.value)


def test_bit_reproducible_between_calls_and_streams():
    """reciprocal='ewald': nothing in the loop uses atomics, so two calls and a call on a side stream give the same bits (not claimed for 'pme',
    whose mesh spread adds in arrival order)."""
    ind, _ = _api()
    f = _batch_case()
    kw = dict(external_field=f["field"], reciprocal="ewald", alpha=f["alpha"], k_vectors=f["kv"], tolerance=1e-10, batch_idx=f["bi"], **_kw(f, "list"))
    args = (f["pos"], f["q"], f["polar"], f["cells"])
    a, b = ind(*args, **kw), ind(*args, **kw)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = ind(*args, **kw)
    side.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c) and float(a.abs().max()) > 0


# ---- autograd --------------------------------------------------------------------------------------------------------------------------
# Relative to the largest |component| of each gradient.  Both solves run to tolerance 1e-12; an error of that size in mu or z is amplified
# by at most the condition number of D^1/2 H D^1/2 (taken from the reference inside the test, about 2), and a factor 100 covers the rounding
# of the public energy functions' adjoints (1e-11 of the largest value in tests/test_dipole_gpu.py): 100 * 1e-12 * cond.
# Measured on the MI355X (bar 2.06e-10): positions 1.82e-13, charges 1.62e-13, polarisability 2.54e-13, external field 1.54e-13.
def test_gradients_against_the_reference_autograd():
    ind, _ = _api()
    c = IC.lattice("l27")
    n, tol = c["n"], 1e-12
    i, j, S = IC.entries("l27", 7.0, 1)
    nm, sh = _matrix(i, j, S, n, int(torch.bincount(i).max()) + 2, n)
    ent = (i.to(DEV), j.to(DEV), S.to(DEV))
    cell, kv = _t(c["cell"]).reshape(1, 3, 3), IC.k_vectors(c["cell"], IC.EWALD["k_cutoff"]).to(DEV)
    g = np.random.default_rng(91)
    field0, w = 0.1 * g.normal(size=(n, 3)), _t(g.normal(size=(n, 3)))
    names = ["pos", "q", "polar", "field"]
    leaves = lambda: dict(pos=_t(c["pos"]).requires_grad_(True), q=_t(c["q"]).requires_grad_(True),  # noqa: E731
                          polar=_t(c["polar"]).requires_grad_(True), field=_t(field0).requires_grad_(True))
    r = leaves()
    T, lin = R.dipole_operator(r["pos"], r["q"], cell, IC.EWALD["alpha"], ent, kv, differentiable=True)
    H, b = R.system_matrix(T, r["polar"]), R.right_hand_side(lin, r["polar"], r["field"])
    mu_ref = R.solve(H, b)
    ref = dict(zip(names, torch.autograd.grad((w * mu_ref).sum(), [r[k] for k in names])))
    ev = R.scaled_spectrum(H.detach(), r["polar"].detach())
    bar = 100.0 * tol * float(ev.max() / ev.min())
    d = leaves()
    mu = ind(d["pos"], d["q"], d["polar"], cell, external_field=d["field"], reciprocal="ewald", alpha=IC.EWALD["alpha"], k_vectors=kv, tolerance=tol,
             neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=n)
    assert float((mu.detach() - mu_ref.detach()).abs().max()) <= 1e-9 * float(mu_ref.detach().abs().max())
    got = dict(zip(names, torch.autograd.grad((w * mu).sum(), [d[k] for k in names], retain_graph=True)))
    errs = {k: float((got[k] - ref[k]).abs().max()) / float(ref[k].abs().max()) for k in names}
    print(f"gradients (bar {bar:.2e}): " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k in names:
        assert got[k].shape == d[k].shape and got[k].dtype == F64
        assert errs[k] <= bar, (k, errs[k])
    with pytest.raises(NotImplementedError, match="second derivatives"):
        torch.autograd.grad((w * mu).sum(), d["field"], create_graph=True)
    fn = torch.compile(lambda p: ind(p, d["q"].detach(), d["polar"].detach(), cell, neighbor_matrix=nm, neighbor_matrix_shifts=sh, alpha=0.45,
                                     mesh_dimensions=(24, 24, 24)), backend="eager", fullgraph=True)
    with pytest.raises(Exception) as err:
        fn(d["pos"].detach())
    assert "cannot be traced by torch.compile" in str(err.value)
