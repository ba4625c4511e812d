"""The point-dipole Ewald term on the device against the float64 restatement of its operator definition (tests/dipole_reference.py, itself
checked in tests/test_dipole_reference_cpu.py) on the same stored entries and the same k set.

fp64 inputs: kernels and reference follow the same arithmetic model (fp64 throughout), so they differ by summation order and the last bits of
erfc / exp / sincos only: 1e-11 of the largest |value| per output, the bar of tests/test_coulomb_gpu.py and tests/test_gaussian_charges_gpu.py
for the same model.  fp32 inputs: pair vector and distance in fp32, the rest fp64, against the reference's float32-distance mode at 1e-6 of the
largest |value|, the bar of the same tests.  The reciprocal sums hold the 1e-11 bar as well (no cancellation over k shows at these sizes: the
kernel never forms |S|^2 - |S_q|^2 as a difference), so the fallback bar the sums could have claimed is not used.

Zero dipoles: energies, forces, charge_grads and virial are exactly 0.0.  dipole_grads is dE/dmu = minus the electric field of the charges at
the atom, which the model defines as B1 q_j R summed over the row (plus the reciprocal part): it does not vanish and is checked against the
reference instead."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import dipole_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("energies", "forces", "charge_grads", "dipole_grads", "virial")
ALL = dict(compute_forces=True, compute_charge_gradients=True, compute_dipole_gradients=True, compute_virial=True)


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV) if dtype is None else torch.as_tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


def _np(x):
    return x.detach().cpu().numpy().astype(np.float64)


def _close(got, ref, what, rel=1e-11):
    got = _np(got) if isinstance(got, torch.Tensor) else got
    ref = _np(ref) if isinstance(ref, torch.Tensor) else ref
    assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
    scale = max(np.abs(ref).max(), 1e-30) if ref.size else 1.0
    err = np.abs(got - ref).max() if ref.size else 0.0
    print(f"{what:48s} rel err {err / scale:.2e} (bar {rel:.0e})")
    assert err <= rel * scale + 1e-14, f"{what}: max err {err:.3e} > {rel * scale:.3e}"
    return err / scale


def _system(n, seed, box, triclinic=True, no_dipole=3):
    g = np.random.default_rng(seed)
    cell = np.eye(3) * box
    if triclinic:
        cell = np.array([[box, 0, 0], [0.2 * box, 0.9 * box, 0], [0.1 * box, -0.15 * box, 1.1 * box]])
    pos = g.uniform(0, 1, (n, 3)) @ cell
    q = g.normal(size=n) + 0.05  # a charged box
    mu = 0.4 * g.normal(size=(n, 3))
    if no_dipole:
        mu[g.choice(n, min(no_dipole, n), replace=False)] = 0.0
    return pos, cell, q, mu


def _lists(pos, cell, cutoff, batch_idx=None, batch_ptr=None, max_neighbors=400):
    from nvalchemiops.neighborlist import neighbor_list

    cells = _t(cell).reshape(-1, 3, 3)
    pbc = torch.ones((cells.shape[0], 3), dtype=torch.bool, device=DEV)
    kw = dict(batch_idx=batch_idx, batch_ptr=batch_ptr, method="batch_cell_list") if batch_idx is not None else dict(method="cell_list")
    nm, num, sh = neighbor_list(_t(pos), cutoff, cell=cells, pbc=pbc, max_neighbors=max_neighbors, **kw)
    assert int(num.max()) <= max_neighbors
    nl, ptr, lsh = neighbor_list(_t(pos), cutoff, cell=cells, pbc=pbc, max_neighbors=max_neighbors, return_neighbor_list=True, **kw)
    return nm, num, sh, nl, ptr, lsh


def _k_vectors(cells, k_cutoff):
    from nvalchemiops.interactions.electrostatics import generate_k_vectors_ewald_summation

    return generate_k_vectors_ewald_summation(cells, k_cutoff)


def _fmt_kw(f, fmt):
    if fmt == "matrix":
        return dict(neighbor_matrix=f["nm"], neighbor_matrix_shifts=f["sh"], mask_value=f["n"])
    return dict(neighbor_list=f["nl"], neighbor_ptr=f["ptr"], neighbor_shifts=f["lsh"])


ALPHA = 0.45


@functools.lru_cache(maxsize=None)
def _single():
    """Case 1: 300 atoms, triclinic box of edge 12, charged, three atoms without a dipole, cutoff 7 (rows longer than 64 entries: several trips of
    the wave plus a tail), both list formats, K = 544 k-vectors (> 256, not a multiple of 64), the reference computed once."""
    pos, cell, q, mu = _system(300, seed=5, box=12.0)
    assert abs(q.sum()) > 1.0
    nm, num, sh, nl, ptr, lsh = _lists(pos, cell, 7.0)
    assert int(num.min()) > 64 and bool((num % 64 != 0).any())
    P, Q, M, C = _t(pos), _t(q), _t(mu), _t(cell).reshape(1, 3, 3)
    kv = _k_vectors(C, 2.2)
    assert kv.shape[0] > 256 and kv.shape[0] % 64 != 0, kv.shape
    n = pos.shape[0]
    A = torch.tensor([ALPHA], dtype=torch.float64, device=DEV)
    entries = R.entries_from_matrix(nm, sh, n)
    f = dict(P=P, Q=Q, M=M, C=C, A=A, kv=kv, nm=nm, sh=sh, nl=nl, ptr=ptr, lsh=lsh, n=n, entries=entries)
    f["ref"] = R.evaluate(P, Q, M, C, A, entries, kv)
    f["ref_real"] = R.evaluate(P, Q, M, C, A, entries, None)
    f["ref_recip"] = R.evaluate(P, Q, M, C, A, None, kv)
    return f


def _api():
    from nvalchemiops.interactions.electrostatics import ewald_dipole_correction, ewald_dipole_real_space, ewald_dipole_reciprocal_space

    return ewald_dipole_correction, ewald_dipole_real_space, ewald_dipole_reciprocal_space


# ---- 1. basic parity ----------------------------------------------------------------------------------------------------------------------
def test_parity_fp64_matrix_and_csr():
    both, real, recip = _api()
    f = _single()
    outs = {}
    for fmt in ("matrix", "list"):
        out = both(f["P"], f["Q"], f["M"], f["C"], f["A"], f["kv"], **_fmt_kw(f, fmt), **ALL)
        assert len(out) == 5 and all(o.dtype == torch.float64 for o in out)
        assert [tuple(o.shape) for o in out] == [(300,), (300, 3), (300,), (300, 3), (1, 3, 3)]
        for name, o in zip(NAMES, out):
            _close(o, f["ref"][name], f"fp64 {fmt} total {name}")
        part = real(f["P"], f["Q"], f["M"], f["C"], f["A"], **_fmt_kw(f, fmt), **ALL)
        for name, o in zip(NAMES, part):
            _close(o, f["ref_real"][name], f"fp64 {fmt} real space {name}")
        outs[fmt] = out
    rec = recip(f["P"], f["Q"], f["M"], f["C"], f["kv"], f["A"], **ALL)
    for name, o in zip(NAMES, rec):
        _close(o, f["ref_recip"][name], f"fp64 reciprocal space {name}")
    for name, a, b in zip(NAMES, outs["matrix"], outs["list"]):
        _close(a, b, f"matrix vs CSR {name}", 1e-10)
    frc = outs["matrix"][1]
    assert float(frc.sum(0).abs().max()) <= 1e-9 * float(frc.abs().max()), "net force"
    # a subset of the outputs is the same numbers; alpha as a Python number is the same as a tensor
    e, dg = both(f["P"], f["Q"], f["M"], f["C"], ALPHA, f["kv"], **_fmt_kw(f, "matrix"), compute_dipole_gradients=True)
    assert torch.equal(e, outs["matrix"][0]) and torch.equal(dg, outs["matrix"][3])
    e = both(f["P"], f["Q"], f["M"], f["C"], f["A"], f["kv"], **_fmt_kw(f, "list"))
    assert isinstance(e, torch.Tensor) and torch.equal(e, outs["list"][0])


def test_parity_fp32_inputs():
    both, real, recip = _api()
    f = _single()
    P, Q, M, C, A = (f[k].float() for k in ("P", "Q", "M", "C", "A"))
    kv = _k_vectors(C, 2.2)
    assert kv.dtype == torch.float32 and kv.shape == f["kv"].shape
    ref = R.evaluate(P, Q, M, C, A, f["entries"], kv, distance_dtype=torch.float32)
    for fmt in ("matrix", "list"):
        out = both(P, Q, M, C, A, kv, **_fmt_kw(f, fmt), **ALL)
        assert all(o.dtype == torch.float32 for o in out)
        for name, o in zip(NAMES, out):
            _close(o, ref[name], f"fp32 {fmt} total {name}", 1e-6)


# ---- 2. padding and self-images -----------------------------------------------------------------------------------------------------------
def test_self_images_padding_kinds_empty_row_and_wide_matrix():
    both, real, recip = _api()
    n, cutoff, empty_row = 9, 7.0, 4
    pos, cell, q, mu = _system(n, seed=9, box=5.0, no_dipole=1)
    i, j, S = R.brute_force_entries(pos, cell, cutoff, 3)
    assert int(((i == j) & (S != 0).any(-1)).sum()) > 0  # self-images: i = j entries with S != 0
    keep = (i != empty_row) & (j != empty_row)  # atom 4 leaves the list from both ends: its row is empty and the list stays full
    i, j, S = i[keep], j[keep], S[keep]
    counts = np.bincount(i.numpy(), minlength=n)
    width = int(counts.max()) + 7  # a caller matrix wider than needed
    mask = n
    fills = (mask, 1000, -5)  # the three kinds of padding: the mask value, an index >= N, a negative index
    nm = np.empty((n, width), dtype=np.int32)
    sh = np.zeros((n, width, 3), dtype=np.int32)
    g = np.random.default_rng(0)
    for a in range(n):
        nm[a] = [fills[(a + c) % 3] for c in range(width)]
        cols = np.sort(g.choice(width, counts[a], replace=False))  # padding sits between the entries, not only behind them
        nm[a, cols], sh[a, cols] = j[i == a].numpy(), S[i == a].numpy()
        sh[a, nm[a] < 0] = 7  # shifts of padding slots are never read
    assert counts[empty_row] == 0
    P, Q, M, C = _t(pos), _t(q), _t(mu), _t(cell).reshape(1, 3, 3)
    kv = _k_vectors(C, 3.0)
    NM, SH = _t(nm), _t(sh)
    ei, ej, eS = R.entries_from_matrix(NM, SH, mask)
    assert ei.shape[0] == int(counts.sum())
    ref = R.evaluate(P, Q, M, C, 0.5, (ei, ej, eS), kv)
    out = both(P, Q, M, C, 0.5, kv, neighbor_matrix=NM, neighbor_matrix_shifts=SH, mask_value=mask, **ALL)
    for name, o in zip(NAMES, out):
        _close(o, ref[name], f"9 atoms, matrix {name}")
    # the same entries as a CSR list
    order = torch.argsort(ei, stable=True)
    ptr = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    ptr[1:] = torch.cumsum(torch.bincount(ei, minlength=n), 0)
    csr = both(P, Q, M, C, 0.5, kv, neighbor_list=torch.stack([ei, ej])[:, order].int(), neighbor_ptr=ptr, neighbor_shifts=eS[order].int(), **ALL)
    for name, o in zip(NAMES, csr):
        _close(o, ref[name], f"9 atoms, CSR {name}")
    # the emptied row: only the reciprocal part is left for that atom
    rs = real(P, Q, M, C, 0.5, neighbor_matrix=NM, neighbor_matrix_shifts=SH, mask_value=mask, **ALL)
    assert all(float(o[empty_row].abs().max()) == 0.0 for o in rs[:4])


# ---- 3. batch -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch():
    """A ragged batch: 300 atoms triclinic, 420 atoms orthorhombic, and a one-atom system; per-system alpha."""
    p0, c0, q0, m0 = _system(300, seed=7, box=12.0)
    p1, c1, q1, m1 = _system(420, seed=8, box=15.0, triclinic=False)
    p2, c2, q2, m2 = _system(1, seed=10, box=15.0, triclinic=False, no_dipole=0)
    parts = ((p0, c0, q0, m0), (p1, c1, q1, m1), (p2, c2, q2, m2))
    pos, q, mu = (np.concatenate([p[k] for p in parts]) for k in (0, 2, 3))
    cells = np.stack([c0, c1, c2])
    bi = _t(np.concatenate([np.full(300, 0, np.int32), np.full(420, 1, np.int32), np.full(1, 2, np.int32)]))
    bptr = _t(np.array([0, 300, 720, 721], np.int32))
    nm, num, sh, nl, ptr, lsh = _lists(pos, cells, 7.0, batch_idx=bi, batch_ptr=bptr)
    assert int(num[720]) == 0
    C = _t(cells)
    A = torch.tensor([0.4, 0.5, 0.45], dtype=torch.float64, device=DEV)
    kv = _k_vectors(C, 2.0)
    assert kv.dim() == 3 and kv.shape[0] == 3
    return dict(P=_t(pos), Q=_t(q), M=_t(mu), C=C, A=A, kv=kv, bi=bi, nm=nm, sh=sh, nl=nl, ptr=ptr, lsh=lsh, n=721, parts=parts)


def test_batch_equals_single_calls_and_reference():
    both, real, recip = _api()
    b = _batch()
    ref = R.evaluate(b["P"], b["Q"], b["M"], b["C"], b["A"], R.entries_from_matrix(b["nm"], b["sh"], b["n"]), b["kv"], batch_idx=b["bi"])
    got = {}
    for fmt in ("matrix", "list"):
        got[fmt] = both(b["P"], b["Q"], b["M"], b["C"], b["A"], b["kv"], batch_idx=b["bi"], **_fmt_kw(b, fmt), **ALL)
        assert got[fmt][4].shape == (3, 3, 3)
        for name, o in zip(NAMES, got[fmt]):
            _close(o, ref[name], f"batch {fmt} {name}")
    bounds = (0, 300, 720, 721)
    for fmt in ("matrix", "list"):
        for s in range(3):
            p, c, q, m = b["parts"][s]
            sl = slice(bounds[s], bounds[s + 1])
            nm, num, sh, nl, ptr, lsh = _lists(p, c, 7.0)
            one = dict(nm=nm, sh=sh, nl=nl, ptr=ptr, lsh=lsh, n=p.shape[0])
            alone = both(_t(p), _t(q), _t(m), _t(c).reshape(1, 3, 3), b["A"][s:s + 1], b["kv"][s], **_fmt_kw(one, fmt), **ALL)
            for name, o, a in zip(NAMES[:4], got[fmt][:4], alone[:4]):
                _close(o[sl], a, f"{fmt} system {s} alone: {name}", 1e-12)
            _close(got[fmt][4][s], alone[4][0], f"{fmt} system {s} alone: virial", 1e-12)
    # the one-atom system: no neighbours, so its energy is its own reciprocal sum minus the self term -- two numbers 200 times the result, hence
    # a bar on the terms that were summed (64 eps sum_k |term|, both as the reference computes them) and not on the result
    e2 = float(got["matrix"][0][720])
    want, terms = R.recip_energies(b["P"][720:], b["Q"][720:], b["M"][720:], b["C"][2], b["kv"][2], 0.45, return_abs=True)
    print(f"one-atom system: {e2:.15e} vs {float(want[0]):.15e}, sum of |terms| {float(terms[0]):.3e}")
    assert abs(e2 - float(want[0])) <= 64 * np.finfo(np.float64).eps * float(terms[0]) and abs(float(want[0])) > 1e-6


# ---- 4. reciprocal edge cases -------------------------------------------------------------------------------------------------------------
def test_one_k_vector_and_empty_k_set():
    both, real, recip = _api()
    f = _single()
    one = recip(f["P"], f["Q"], f["M"], f["C"], f["kv"][:1], f["A"], **ALL)
    ref = R.evaluate(f["P"], f["Q"], f["M"], f["C"], f["A"], None, f["kv"][:1])
    for name, o in zip(NAMES, one):
        _close(o, ref[name], f"K = 1 {name}")
    none = recip(f["P"], f["Q"], f["M"], f["C"], f["kv"][:0], f["A"], **ALL)
    c = 2.0 * ALPHA**3 / (3.0 * math.sqrt(math.pi))
    _close(none[0], -c * (f["M"] * f["M"]).sum(-1), "K = 0 energies: the self term alone", 1e-15)
    _close(none[3], -2.0 * c * f["M"], "K = 0 dipole_grads", 1e-15)
    for k in (1, 2, 4):
        assert float(none[k].abs().max()) == 0.0, NAMES[k]
    total = both(f["P"], f["Q"], f["M"], f["C"], f["A"], f["kv"][:0], **_fmt_kw(f, "matrix"), **ALL)
    for name, o in zip(NAMES, total):
        _close(o, f["ref_real"][name] + (_np(none[NAMES.index(name)]) if name in ("energies", "dipole_grads") else 0.0), f"K = 0 total {name}")


# ---- 5. linearity and zero dipoles --------------------------------------------------------------------------------------------------------
def test_zero_dipoles_and_bilinearity():
    both, real, recip = _api()
    f = _single()
    zero = torch.zeros_like(f["M"])
    ref = R.evaluate(f["P"], f["Q"], zero, f["C"], f["A"], f["entries"], f["kv"])
    for fmt in ("matrix", "list"):
        for call in (lambda: both(f["P"], f["Q"], zero, f["C"], f["A"], f["kv"], **_fmt_kw(f, fmt), **ALL),
                     lambda: both(f["P"].float(), f["Q"].float(), zero.float(), f["C"].float(), ALPHA, f["kv"].float(), **_fmt_kw(f, fmt), **ALL)):
            out = call()
            for k in (0, 1, 2, 4):
                assert float(out[k].abs().max()) == 0.0 and not bool(torch.isnan(out[k]).any()), (fmt, NAMES[k])
        # minus the field of the charges: not zero, and the reference's
        out = both(f["P"], f["Q"], zero, f["C"], f["A"], f["kv"], **_fmt_kw(f, fmt), **ALL)
        _close(out[3], ref["dipole_grads"], f"{fmt} zero dipoles: dipole_grads")
    assert np.abs(ref["dipole_grads"]).max() > 1e-3
    # bilinear in (q, mu): everything times 2 gives energies, forces and virial times 4, charge and dipole gradients times 2
    base = both(f["P"], f["Q"], f["M"], f["C"], f["A"], f["kv"], **_fmt_kw(f, "matrix"), **ALL)
    twice = both(f["P"], 2.0 * f["Q"], 2.0 * f["M"], f["C"], f["A"], f["kv"], **_fmt_kw(f, "matrix"), **ALL)
    for name, a, b2, factor in zip(NAMES, base, twice, (4.0, 4.0, 2.0, 2.0, 4.0)):
        _close(b2, factor * a, f"(2 q, 2 mu): {name} times {factor:g}", 1e-14)


# ---- 6. consistency with the charge routines ----------------------------------------------------------------------------------------------
def test_charge_ewald_plus_dipole_term_at_two_alpha():
    """`ewald_summation` + `ewald_dipole_correction` at alpha = 0.45 and 0.5 over the same list (cutoff 7) and the same k set (k_cutoff 3.5) differ
    by the truncation of the sums only.  The reference's own difference over the same entries and k-vectors (exact erfc) is that truncation;
    twice it is allowed (the charge routine evaluates erfc by a polynomial)."""
    from nvalchemiops.interactions.electrostatics import ewald_summation

    both, real, recip = _api()
    f = _single()
    kv = _k_vectors(f["C"], 3.5)
    totals, refs = [], []
    for alpha in (0.45, 0.5):
        cc = ewald_summation(f["P"], f["Q"], f["C"], alpha=alpha, k_vectors=kv, **_fmt_kw(f, "matrix"))
        dd = both(f["P"], f["Q"], f["M"], f["C"], alpha, kv, **_fmt_kw(f, "matrix"))
        totals.append(float(cc.sum()) + float(dd.sum()))
        refs.append(float(R.charge_ewald_total(f["P"], f["Q"], f["C"][0], alpha, *f["entries"], kv))
                    + float(R.energies(f["P"], f["Q"], f["M"], f["C"], alpha, f["entries"], kv).sum().detach()))
    print(f"device  {totals[0]:.12e} {totals[1]:.12e} difference {abs(totals[0] - totals[1]):.3e}")
    print(f"reference {refs[0]:.12e} {refs[1]:.12e} difference {abs(refs[0] - refs[1]):.3e}")
    assert abs(totals[0] - totals[1]) <= 2.0 * abs(refs[0] - refs[1])


# ---- 7. autograd --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["list", "matrix"])
def test_autograd_matches_reference_and_explicit_outputs(fmt):
    both, real, recip = _api()
    f = _single()
    w = _t(np.random.default_rng(3).uniform(0.2, 1.8, f["n"]))
    ref = R.evaluate(f["P"], f["Q"], f["M"], f["C"], f["A"], f["entries"], f["kv"], weights=w)
    leaves = [f[k].clone().requires_grad_(True) for k in ("P", "Q", "M")]
    e = both(*leaves, f["C"], f["A"], f["kv"], **_fmt_kw(f, fmt))
    assert e.requires_grad
    gp, gq, gm = torch.autograd.grad((e * w).sum(), leaves)
    _close(-gp, ref["forces"], f"{fmt} dL/dr")
    _close(gq, ref["charge_grads"], f"{fmt} dL/dq")
    _close(gm, ref["dipole_grads"], f"{fmt} dL/dmu")
    # w = 1: the gradients of the total energy are the explicit outputs
    leaves = [f[k].clone().requires_grad_(True) for k in ("P", "Q", "M")]
    e, frc, cg, dg = both(*leaves, f["C"], f["A"], f["kv"], **_fmt_kw(f, fmt), compute_forces=True, compute_charge_gradients=True,
                          compute_dipole_gradients=True)
    gp, gq, gm = torch.autograd.grad(e.sum(), leaves)
    _close(-gp, frc, f"{fmt} -dE/dr vs forces", 1e-12)
    _close(gq, cg, f"{fmt} dE/dq vs charge_grads", 1e-12)
    _close(gm, dg, f"{fmt} dE/dmu vs dipole_grads", 1e-12)
    eager = both(f["P"], f["Q"], f["M"], f["C"], f["A"], f["kv"], **_fmt_kw(f, fmt), compute_forces=True)
    assert torch.equal(e.detach(), eager[0]) and torch.equal(frc.detach(), eager[1])


def test_autograd_fp32_only_dipoles_and_batch():
    both, real, recip = _api()
    b = _batch()
    w = _t(np.random.default_rng(4).uniform(0.2, 1.8, b["n"]))
    ref = R.evaluate(b["P"], b["Q"], b["M"], b["C"], b["A"], R.entries_from_matrix(b["nm"], b["sh"], b["n"]), b["kv"], batch_idx=b["bi"], weights=w)
    M = b["M"].clone().requires_grad_(True)  # the induced-dipole solver's use: only the dipoles require grad
    e = both(b["P"], b["Q"], M, b["C"], b["A"], b["kv"], batch_idx=b["bi"], **_fmt_kw(b, "list"))
    (gm,) = torch.autograd.grad((e * w).sum(), [M])
    _close(gm, ref["dipole_grads"], "batch dL/dmu")
    f = _single()
    P, Q, M, C, A, kv = (f[k].float() for k in ("P", "Q", "M", "C", "A", "kv"))
    w = _t(np.random.default_rng(3).uniform(0.2, 1.8, f["n"]))
    ref = R.evaluate(P, Q, M, C, A, f["entries"], kv, distance_dtype=torch.float32, weights=w)
    leaves = [t.clone().requires_grad_(True) for t in (P, Q, M)]
    e = both(*leaves, C, A, kv, **_fmt_kw(f, "matrix"))
    gp, gq, gm = torch.autograd.grad((e * w.float()).sum(), leaves)
    assert all(g.dtype == torch.float32 for g in (gp, gq, gm))
    _close(-gp, ref["forces"], "fp32 dL/dr", 1e-6)
    _close(gq, ref["charge_grads"], "fp32 dL/dq", 1e-6)
    _close(gm, ref["dipole_grads"], "fp32 dL/dmu", 1e-6)


def test_second_order_and_out_of_scope_gradients_are_refused():
    both, real, recip = _api()
    f = _single()
    # a loss on the explicit forces (or any explicit gradient, or the virial) is a second derivative: refused at backward, never a silent zero
    for flag in ALL:
        P = f["P"].clone().requires_grad_(True)
        _, explicit = both(P, f["Q"], f["M"], f["C"], f["A"], f["kv"], **_fmt_kw(f, "matrix"), **{flag: True})
        with pytest.raises(NotImplementedError, match="second derivatives of the pair kernels"):
            explicit.sum().backward()
    M = f["M"].clone().requires_grad_(True)
    e = both(f["P"], f["Q"], M, f["C"], f["A"], f["kv"], **_fmt_kw(f, "matrix"))
    (g,) = torch.autograd.grad(e.sum(), [M], create_graph=True)
    with pytest.raises(NotImplementedError, match="second derivatives of the pair kernels"):
        g.sum().backward()
    # cell and alpha gradients are out of scope: refused, with a pointer to the virial
    for name in ("C", "A"):
        leaf = f[name].clone().requires_grad_(True)
        args = dict(C=f["C"], A=f["A"])
        args[name] = leaf
        e = both(f["P"], f["Q"], f["M"], args["C"], args["A"], f["kv"], **_fmt_kw(f, "matrix"))
        with pytest.raises(NotImplementedError, match="use compute_virial"):
            e.sum().backward()


def test_virial_is_the_strain_derivative_and_not_symmetric():
    both, real, recip = _api()
    f = _single()
    for label, vir, ref in (("total", both(f["P"], f["Q"], f["M"], f["C"], f["A"], f["kv"], **_fmt_kw(f, "list"), compute_virial=True)[1], f["ref"]),
                            ("real space", real(f["P"], f["Q"], f["M"], f["C"], f["A"], **_fmt_kw(f, "list"), compute_virial=True)[1], f["ref_real"]),
                            ("reciprocal space", recip(f["P"], f["Q"], f["M"], f["C"], f["kv"], f["A"], compute_virial=True)[1], f["ref_recip"])):
        _close(vir, ref["virial"], f"{label} virial vs the reference's strain derivative")
        v = _np(vir)[0]
        anti = np.linalg.norm(0.5 * (v - v.T)) / np.linalg.norm(v)
        print(f"{label}: antisymmetric part / norm = {anti:.3e}")
        assert anti > 1e-6, label  # a six-word (symmetrised) virial fails here and above


# ---- 8. determinism -----------------------------------------------------------------------------------------------------------------------
def test_two_calls_and_a_side_stream_are_bit_identical():
    both, real, recip = _api()
    b = _batch()
    w = _t(np.random.default_rng(6).uniform(0.2, 1.8, b["n"]))

    def run(fmt):
        out = both(b["P"], b["Q"], b["M"], b["C"], b["A"], b["kv"], batch_idx=b["bi"], **_fmt_kw(b, fmt), **ALL)
        leaves = [b[k].clone().requires_grad_(True) for k in ("P", "Q", "M")]
        e = both(*leaves, b["C"], b["A"], b["kv"], batch_idx=b["bi"], **_fmt_kw(b, fmt))
        return tuple(out) + tuple(torch.autograd.grad((e * w).sum(), leaves))

    for fmt in ("list", "matrix"):
        first, second = run(fmt), run(fmt)
        torch.cuda.current_stream().synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            third = run(fmt)
        side.synchronize()
        for k, (a, b2, c) in enumerate(zip(first, second, third)):
            assert torch.equal(a, b2) and torch.equal(a, c), (fmt, k)


# ---- 9. compile ---------------------------------------------------------------------------------------------------------------------------
def test_compile_fullgraph_equals_eager_bitwise():
    both, real, recip = _api()
    f = _single()

    def fn(p, q, m):
        e, frc, dg, vir = both(p, q, m, f["C"], f["A"], f["kv"], neighbor_matrix=f["nm"], neighbor_matrix_shifts=f["sh"], mask_value=f["n"],
                               compute_forces=True, compute_dipole_gradients=True, compute_virial=True)
        return e * 2.0, frc, dg, vir

    torch._dynamo.reset()
    got = torch.compile(fn, mode="default", fullgraph=True)(f["P"], f["Q"], f["M"])
    want = fn(f["P"], f["Q"], f["M"])
    for a, b in zip(got, want):
        assert torch.equal(a, b)

    def parts(p, q, m):
        return (real(p, q, m, f["C"], f["A"], neighbor_list=f["nl"], neighbor_ptr=f["ptr"], neighbor_shifts=f["lsh"], compute_charge_gradients=True)
                + recip(p, q, m, f["C"], f["kv"], f["A"], compute_charge_gradients=True))

    got = torch.compile(parts, mode="default", fullgraph=True)(f["P"], f["Q"], f["M"])
    for a, b in zip(got, parts(f["P"], f["Q"], f["M"])):
        assert torch.equal(a, b)
