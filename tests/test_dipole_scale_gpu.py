"""`mi_dipole_scale`, `mi_scaled_dipole_tensors` / `mi_scaled_dipole_apply` and their public face -- `dipole_pair_scale_correction` and
`scaled_induced_dipoles` with and without a cell -- on the device, against the float64 yardstick tests/dipole_scale_reference.py
(itself checked in tests/test_dipole_scale_reference_cpu.py) on the problems of tests/dipole_scale_cases.py.

Matrices are three columns wider than the longest row and padded with the mask value n, -1 in the last column and n + 7 in every other row of
the one before; the scales of all padding are NaN (they must not be looked at).

Bars: those of tests/test_dipole_gpu.py and tests/test_thole_gpu.py for the same arithmetic model -- 1e-11 of the largest |value| of each
output for float64 inputs (the adjoint too), 1e-6 for float32 positions against the yardstick's float32-distance mode; the solves hold the
bars of tests/test_induced_gpu.py: true residual <= 10 tol ||b||, |mu - mu_ref| <= 10 tol ||b|| / lambda_min(H), gradients 100 tol cond.

Measured on the MI355X.  fp64 outputs <= 2.7e-15, float32 positions <= 3.0e-7 (unwrapped molecules 8.9e-7); adjoint <= 6.8e-16; composed
`pair_scale_correction` calls <= 1.3e-15; stored product 7.0e-17 - 1.7e-16 (float32 1.4e-7); residual factors 0.05 - 0.79; implicit gradients
<= 1.2e-13 (bar 1.2e-10).  DESIGN 3.34 has the table."""
import functools

import numpy as np
import pytest
import torch

from tests import dipole_scale_cases as SC
from tests import dipole_scale_reference as SR
from tests import induced_reference as IR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
ALL = dict(compute_forces=True, compute_charge_gradients=True, compute_dipole_gradients=True, compute_polarizability_gradients=True)
NAMES = ("energies", "forces", "charge_grads", "dipole_grads", "polar_grads", "virial")


def _api():
    from nvalchemiops.interactions import electrostatics as E

    return E


def _close(got, ref, what, rel):
    got, ref = got.detach().cpu().numpy().astype(np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
    scale, err = max(np.abs(ref).max(), 1e-30), np.abs(got - ref).max()
    print(f"{what:64s} rel err {err / scale:.2e} (bar {rel:.0e})")
    assert err <= rel * scale + 1e-14, f"{what}: max err {err:.3e} > {rel * scale:.3e}"


@functools.lru_cache(maxsize=None)
def _case(kind):
    """The device tensors of an energy case: arrays, both list formats with the three kinds of padding, the yardstick's entries."""
    p = SC.problem(kind)
    n, (i, j, S) = p["n"], p["entries"]
    sd, sm = torch.as_tensor(p["sd"]), torch.as_tensor(p["sm"])
    width = (int(torch.bincount(i, minlength=n).max()) if i.numel() else 0) + 3
    nm, sh, dnm, mnm = SC.matrix(i, j, n, width, (S, sd, sm), fill=float("nan"))
    nm[:, -1] = -1
    nm[::2, -2] = n + 7
    ptr = torch.zeros(n + 1, dtype=torch.int32)
    ptr[1:] = torch.cumsum(torch.bincount(i, minlength=n), 0)
    d = lambda t: t.to(DEV).contiguous()  # noqa: E731
    periodic = p["cell"] is not None
    f = dict(n=n, periodic=periodic, nsys=p["nsys"], ent=(d(i), d(j), d(S)), sd=d(sd), sm=d(sm),
             cell=d(torch.as_tensor(p["cell"])) if periodic else None, bi=None if p["batch_idx"] is None else d(torch.as_tensor(p["batch_idx"])),
             w=d(torch.as_tensor(p["w"])),
             matrix=dict(neighbor_matrix=d(nm.int()), neighbor_matrix_shifts=d(sh.int()) if periodic else None, mask_value=n),
             csr=dict(neighbor_list=d(torch.stack([i, j]).int()), neighbor_ptr=d(ptr), neighbor_shifts=d(S.int()) if periodic else None),
             scales=dict(matrix=(d(dnm), d(mnm)), csr=(d(sd), d(sm))))
    src = dict(p, pos=p["pos_wrapped"]) if kind == "molecules" else p
    f["arrays"] = [d(torch.as_tensor(src[k], dtype=F64)) for k in ("pos", "q", "mu", "polar")]
    f["whole"] = d(torch.as_tensor(p["pos"], dtype=F64))
    return f


@functools.lru_cache(maxsize=None)
def _reference(kind, thole, dtype=F64, weighted=False, minimum_image=False):
    f = _case(kind)
    i, j, S = f["ent"]
    arrays = [a.to(dtype) for a in f["arrays"]]
    return SR.evaluate(*arrays, f["sd"], f["sm"], (i, j, torch.zeros_like(S) if minimum_image else S), thole=thole, batch_idx=f["bi"],
                       cell=None if f["cell"] is None else f["cell"].to(dtype), distance_dtype=dtype, weights=f["w"] if weighted else None,
                       minimum_image=minimum_image)


def _call(f, fmt, thole, dtype=F64, pos=None, shifts=True, **flags):
    pos_, q, mu, polar = (a.to(dtype) for a in f["arrays"])
    lists = dict(f[fmt])
    if not shifts:
        lists.update({k: None for k in lists if k.endswith("shifts")})
    sd, sm = f["scales"][fmt]
    return _api().dipole_pair_scale_correction(pos_ if pos is None else pos.to(dtype), q, mu, sd, sm, None if f["cell"] is None else f["cell"].to(dtype),
                                               polarizability=polar, thole=thole, batch_idx=f["bi"], **lists, **flags)


# ---- 1. the energy operator: all six outputs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("thole", [None, SC.A_T], ids=["bare", "thole"])
@pytest.mark.parametrize("fmt", ["matrix", "csr"])
@pytest.mark.parametrize("kind", ["ladder70", "periodic", "molecules"])
def test_every_output_against_the_yardstick(kind, fmt, thole, dtype):
    f, ref = _case(kind), _reference(kind, thole, dtype)
    out = _call(f, fmt, thole, dtype, compute_virial=f["periodic"], **ALL)
    assert len(out) == (6 if f["periodic"] else 5) and all(o.dtype == dtype for o in out)
    for name, o in zip(NAMES, out):
        _close(o, ref[name], f"{kind} {fmt} {name}", 1e-11 if dtype == F64 else 1e-6)
    if kind == "ladder70":  # row 0 is empty, rows 16 ... 23 are one whole wave of empty rows, atom 3 is not polarisable: exact zeros
        assert all(not bool(o[16:24].any()) and not bool(o[0].any()) for o in out)
        assert float(out[4][3]) == 0.0 and float(out[4][4]) == 0.0 and (thole is None) == (not bool(out[4].any()))


@pytest.mark.parametrize("thole", [None, SC.A_T], ids=["bare", "thole"])
def test_unit_scales_give_exact_zeros_and_one_sided_scales_select_their_term(thole):
    f = _case("ladder70")
    sd, sm = f["scales"]["matrix"]
    one = torch.where(torch.isnan(sd), sd, torch.ones_like(sd))
    call = lambda a, b: _api().dipole_pair_scale_correction(*f["arrays"][:3], a, b, polarizability=f["arrays"][3], thole=thole,  # noqa: E731
                                                            **f["matrix"], **ALL)
    assert all(not bool(o.any()) for o in call(one, one))
    both = call(sd, sm)
    for o, a, b in zip(both, call(sd, None), call(None, sm)):
        _close(a + b, o.cpu().numpy(), "direct alone + mutual alone", 1e-11)
    assert all(torch.equal(a, b) for a, b in zip(call(sd, None), call(sd, one))) and all(torch.equal(a, b) for a, b in zip(both, call(sd, sm)))


@pytest.mark.parametrize("dtype", [F64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("thole", [None, SC.A_T], ids=["bare", "thole"])
def test_minimum_image_of_wrapped_atoms_is_the_unwrapped_molecule(thole, dtype):
    f = _case("molecules")
    ref = _reference("molecules", thole, dtype, minimum_image=True)
    flags = dict(ALL, compute_virial=True, minimum_image=True, shifts=False)
    out = _call(f, "matrix", thole, dtype, **flags)
    whole = _call(f, "csr", thole, dtype, pos=f["whole"], **flags)
    for name, o, u in zip(NAMES, out, whole):
        _close(o, ref[name], f"minimum image {name}", 1e-11 if dtype == F64 else 1e-6)
        _close(u, ref[name], f"unwrapped {name}", 1e-11 if dtype == F64 else 1e-6)


# ---- 2. adjoint, 3. tie to pair_scale_correction -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thole", [None, SC.A_T], ids=["bare", "thole"])
def test_adjoint_and_compile(thole):
    f, ref = _case("ladder7"), _reference("ladder7", thole, weighted=True)
    leaves = [a.clone().requires_grad_(True) for a in f["arrays"]]
    sd, sm = f["scales"]["matrix"]
    fn = lambda *a: _api().dipole_pair_scale_correction(*a[:3], sd, sm, polarizability=a[3], thole=thole, **f["matrix"])  # noqa: E731
    e = fn(*leaves)
    grads = torch.autograd.grad((e * f["w"]).sum(), leaves)
    for name, g, sign in zip(NAMES[1:5], grads, (-1.0, 1.0, 1.0, 1.0)):
        _close(sign * torch.nan_to_num(g), ref[name], f"adjoint {name}", 1e-11)
    assert torch.equal(torch.compile(fn, fullgraph=True)(*f["arrays"]), e.detach())


@pytest.mark.parametrize("kind", ["ladder70", "molecules"])
def test_equal_scales_without_thole_are_two_pair_scale_calls(kind):
    E, f = _api(), _case(kind)
    pos, q, mu, _ = f["arrays"]
    s = torch.where(f["scales"]["matrix"][0] == 0.4, 0.4, 0.0).to(F64)  # any symmetric set; NaN padding becomes 0 and is not read
    kw = dict(cell=f["cell"], batch_idx=f["bi"], compute_forces=True, compute_charge_gradients=True, **f["matrix"])
    got = E.dipole_pair_scale_correction(pos, q, mu, s, s, compute_dipole_gradients=True, **kw)
    full = E.pair_scale_correction(pos, q, mu, None, s, compute_dipole_gradients=True, **kw)
    charges = E.pair_scale_correction(pos, q, None, None, s, **kw)
    for k, name in enumerate(NAMES[:3]):
        _close(got[k], (full[k] - charges[k]).cpu().numpy(), f"{kind} composed {name}", 1e-11)
    _close(got[3], full[3].cpu().numpy(), f"{kind} composed dipole_grads", 1e-11)


# ---- 4. the stored product -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind,thole", [("ladder70", None), ("ladder70", SC.A_T), ("molecules", SC.A_T)])
def test_stored_product_is_the_dipole_gradient_of_the_energy_operator(kind, thole, dtype):
    from nvalchemiops import _capi as C
    from nvalchemiops.interactions.electrostatics.dipole_scale import ScaledOperator

    E, f = _api(), _case(kind)
    pos, _, _, polar = (a.to(dtype) for a in f["arrays"])
    polar = torch.where(polar > 0, polar, torch.ones_like(polar))  # every atom polarisable: the operator zeroes the others by construction
    cell = None if f["cell"] is None else f["cell"].to(dtype)
    nm, (sd, sm) = f["matrix"]["neighbor_matrix"], f["scales"]["matrix"]
    op = ScaledOperator((nm, sd, sm), pos, polar, cell, f["bi"], f["nsys"], thole)
    assert int(C.lib().mi_scaled_dipole_tensor_words()) == 5 and bool((op.nbr >= 0).all()) and bool((op.nbr < f["n"]).all())
    assert not bool(torch.isnan(op.tensors).any())
    g = torch.Generator(device="cpu").manual_seed(5)
    x, y_in = (torch.randn((f["n"], 3), dtype=F64, generator=g).to(DEV) for _ in range(2))
    y = op.apply(x)
    ref = E.dipole_pair_scale_correction(pos, torch.zeros_like(polar), x.to(dtype), None, sm, cell, polarizability=polar, thole=thole, neighbor_matrix=nm,
                                         mask_value=f["n"], batch_idx=f["bi"], minimum_image=cell is not None, compute_dipole_gradients=True)[1]
    _close(y, ref.to(F64).cpu().numpy(), f"{kind} stored product", 1e-11 if dtype == F64 else 1e-6)
    assert torch.equal(op.apply(x), y) and torch.equal(op.apply(x, y_in), y_in + y)


# ---- 5. solves against the dense yardstick, 7. null behaviour -------------------------------------------------------------------------------
def _solve(kind, thole, scaled=True, tol=1e-10, leaves=None, **kw):
    E, c = _api(), SC.solve_case(kind)
    t = lambda v: v.to(DEV)  # noqa: E731
    r = leaves or {k: t(c[k]) for k in ("pos", "q", "polar", "field")}
    n, (i, j, S), (bi_, bj, _) = c["n"], c["ent"], c["bent"]
    nm, sh = SC.matrix(i, j, n, int(torch.bincount(i).max()) + 2, (S,))
    bm, sd, sm = SC.matrix(bi_, bj, n, 2, (c["sd"], c["sm"]))
    sp = E.PolarizationPairScales(t(bm.int()), t(sd), t(sm)) if scaled is True else scaled
    common = dict(external_field=r["field"], tolerance=tol, neighbor_matrix=t(nm.int()), mask_value=n, thole=thole, **kw)
    if c["cell"] is not None:
        common.update(cell=t(c["cell"]), reciprocal="ewald", alpha=c["alpha"], k_vectors=t(c["kv"]), neighbor_matrix_shifts=t(sh.int()))
    if sp is not None:
        return E.scaled_induced_dipoles(r["pos"], r["q"], r["polar"], scaled_pairs=sp, **common)
    return (E.cluster_induced_dipoles if c["cell"] is None else E.thole_induced_dipoles)(r["pos"], r["q"], r["polar"], **common)


@pytest.mark.parametrize("kind,thole", [("bent", None), ("bent", SC.A_T), ("chains", None), ("chains", SC.A_T)])
def test_scaled_solve_against_the_dense_yardstick(kind, thole):
    E, c, tol = _api(), SC.solve_case(kind), 1e-10
    H, b = SC.dense(c, thole, DEV)
    out = _solve(kind, thole, return_info=True)
    mu, mu_ref = out.dipoles.to(F64), IR.solve(H, b)
    b_norm, lam = float(b.norm()), float(torch.linalg.eigvalsh(H).min())
    res = float((b - H @ mu.reshape(-1)).norm())
    err = float((mu - mu_ref).abs().max())
    print(f"{kind} thole {thole}: residual / (tol ||b||) {res / (tol * b_norm):.3f}, |mu - mu_ref| {err:.2e} (bound {10 * tol * b_norm / lam:.2e}), "
          f"iterations {out.iterations.tolist()}")
    assert lam > 0 and res <= 10.0 * tol * b_norm and err <= 10.0 * tol * b_norm / lam + 1e-14
    frozen = torch.nonzero(~(c["polar"] > 0)).flatten()
    assert frozen.numel() and bool((out.dipoles[frozen.to(DEV)] == 0).all())
    u_ref = float(IR.energy(H, b, mu_ref))
    assert abs(float(out.polarization_energy[0]) - u_ref) <= 1e-8 * abs(u_ref)
    # stationarity with the new term: dipole_grads of every public energy + mu / a - F vanish on the polarisable atoms
    t = lambda v: v.to(DEV)  # noqa: E731
    pos, q, polar = t(c["pos"]), t(c["q"]), t(c["polar"])
    (i, j, S), (bi_, bj, _) = c["ent"], c["bent"]
    nm, sh = SC.matrix(i, j, c["n"], int(torch.bincount(i).max()), (S,))
    bm, sd, sm = SC.matrix(bi_, bj, c["n"], 2, (c["sd"], c["sm"]))
    lists = dict(neighbor_matrix=t(nm.int()), mask_value=c["n"], compute_dipole_gradients=True)
    cell = None if c["cell"] is None else t(c["cell"])
    if cell is None:
        g = E.coulomb_dipole_correction(pos, q, mu, **lists)[1]
    else:
        lists["neighbor_matrix_shifts"] = t(sh.int())
        g = E.ewald_dipole_correction(pos, q, mu, cell, alpha=c["alpha"], k_vectors=t(c["kv"]), **lists)[1]
    if thole is not None:
        g = g + E.thole_dipole_correction(pos, q, mu, polar, cell, thole=thole, **lists)[1]
    g = g + E.dipole_pair_scale_correction(pos, q, mu, t(sd), t(sm), cell, polarizability=polar, thole=thole, neighbor_matrix=t(bm.int()),
                                           mask_value=c["n"], minimum_image=cell is not None, compute_dipole_gradients=True)[1]
    ok = polar > 0
    grad = (g + mu / torch.where(ok, polar, torch.ones_like(polar)).unsqueeze(1) - t(c["field"]))[ok]
    assert float(grad.norm()) <= 10.0 * tol * b_norm


def test_unit_scales_give_the_bits_of_the_unscaled_function_which_launches_nothing_new(monkeypatch):
    from nvalchemiops.interactions.electrostatics import dipole_scale as DS

    E, c = _api(), SC.solve_case("chains")
    (bi_, bj, _) = c["bent"]
    bm = SC.matrix(bi_, bj, c["n"], 2)[0].int().to(DEV)
    ones = torch.ones(bm.shape, dtype=F64, device=DEV)
    unit = _solve("chains", SC.A_T, scaled=E.PolarizationPairScales(bm, ones, ones))
    calls = []
    for name in ("ScaledOperator", "dipole_pair_scale_correction", "_launch"):
        monkeypatch.setattr(DS, name, lambda *a, _n=name, **k: calls.append(_n))
    none = _solve("chains", SC.A_T, scaled=None)
    assert calls == [] and torch.equal(unit, none) and float(none.abs().max()) > 0


# ---- 6. the case the feature exists for -----------------------------------------------------------------------------------------------------
def test_two_bonded_atoms_beyond_the_catastrophe_solve_with_the_mutual_pair_excluded():
    E, d = _api(), 1.5
    pos = torch.tensor([[0.0, 0.0, 0.0], [d, 0.0, 0.0]], dtype=F64, device=DEV)
    field = torch.tensor([[0.3, -0.2, 0.1]] * 2, dtype=F64, device=DEV)
    nm = torch.tensor([[1], [0]], dtype=torch.int32, device=DEV)
    sp = E.PolarizationPairScales(nm, None, torch.zeros((2, 1), dtype=F64, device=DEV))
    out = E.scaled_induced_dipoles(pos, torch.zeros(2, dtype=F64, device=DEV), d**3, external_field=field, neighbor_matrix=nm, mask_value=2,
                                   scaled_pairs=sp, tolerance=1e-12, return_info=True)
    assert out.iterations.tolist() == [0] or out.iterations.tolist() == [1]
    _close(out.dipoles, (d**3 * field).cpu().numpy(), "mu = a F", 1e-12)


# ---- 8. implicit gradients -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thole", [None, SC.A_T], ids=["bare", "thole"])
def test_implicit_gradients_against_the_dense_yardstick(thole):
    c, tol, names = SC.solve_case("bent"), 1e-12, ("pos", "q", "polar", "field")
    leaves = lambda: {k: c[k].to(DEV).requires_grad_(True) for k in names}  # noqa: E731
    r, d, w = leaves(), leaves(), c["w"].to(DEV)
    H, b = SC.dense(c, thole, DEV, leaves=r)
    ref = torch.autograd.grad((w * IR.solve(H, b)).sum(), [r[k] for k in names])
    ev = IR.scaled_spectrum(H.detach(), r["polar"].detach())
    bar = 100.0 * tol * float(ev.max() / ev.min())
    got = torch.autograd.grad((w * _solve("bent", thole, tol=tol, leaves=d)).sum(), [d[k] for k in names])
    errs = {k: float((g - rg).abs().max()) / float(rg.abs().max()) for k, g, rg in zip(names, got, ref)}
    print(f"scaled gradients thole {thole} (bar {bar:.2e}): " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= bar for v in errs.values()), errs
