"""`gaussian_charge_correction` on the device against the float64 restatement of its definition (tests/gaussian_reference.py, itself checked
in tests/test_gaussian_reference_cpu.py) on the same stored entries.  fp64 inputs: the kernel and the reference follow the same arithmetic
model (fp64 throughout), so they differ by summation order and the last bits of erfc / exp only: 1e-11 of the largest |value| per output, the
bar of tests/test_coulomb_gpu.py for the same model.  fp32 inputs: pair vector and distance in fp32, the rest fp64, against the reference's
float32-distance mode at 1e-6 of the largest |value| (the model's own fp32-vs-fp64 distance on such a box is 3.4e-8 relative)."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import gaussian_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("energies", "forces", "charge_grads", "sigma_grads", "virial")
ALL = dict(compute_forces=True, compute_charge_gradients=True, compute_sigma_gradients=True, compute_virial=True)


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV) if dtype is None else torch.as_tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


def _np(x):
    return x.detach().cpu().numpy().astype(np.float64)


def _close(got, ref, what, rel=1e-11):
    got = _np(got) if isinstance(got, torch.Tensor) else got
    ref = _np(ref) if isinstance(ref, torch.Tensor) else ref
    assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
    tol = rel * max(np.abs(ref).max(), 1e-30) + 1e-14
    err = np.abs(got - ref).max() if ref.size else 0.0
    assert err <= tol, f"{what}: max err {err:.3e} > {tol:.3e}"
    return err / max(np.abs(ref).max(), 1e-30)


def _system(n, seed, box, triclinic=True, neutral=False, point_atoms=3):
    g = np.random.default_rng(seed)
    cell = np.eye(3) * box
    if triclinic:
        cell = np.array([[box, 0, 0], [0.2 * box, 0.9 * box, 0], [0.1 * box, -0.15 * box, 1.1 * box]])
    pos = g.uniform(0, 1, (n, 3)) @ cell
    q = g.normal(size=n)
    if neutral:
        q -= q.mean()
    sigma = g.uniform(0.3, 0.8, n)
    sigma[g.choice(n, point_atoms, replace=False)] = 0.0
    return pos, cell, q, sigma


def _lists(pos, cell, cutoff, batch_idx=None, batch_ptr=None, max_neighbors=400):
    from nvalchemiops.neighborlist import neighbor_list

    cells = _t(cell).reshape(-1, 3, 3)
    pbc = torch.ones((cells.shape[0], 3), dtype=torch.bool, device=DEV)
    kw = dict(batch_idx=batch_idx, batch_ptr=batch_ptr, method="batch_cell_list") if batch_idx is not None else dict(method="cell_list")
    nm, num, sh = neighbor_list(_t(pos), cutoff, cell=cells, pbc=pbc, max_neighbors=max_neighbors, **kw)
    assert int(num.max()) <= max_neighbors
    nl, ptr, lsh = neighbor_list(_t(pos), cutoff, cell=cells, pbc=pbc, max_neighbors=max_neighbors, return_neighbor_list=True, **kw)
    return nm, sh, nl, ptr, lsh


def _ref(P, Q, S, C, entries, batch_idx=None, **kw):
    out = R.evaluate(P, Q, S, C, *entries, batch_idx=batch_idx, **kw)
    return out


@functools.lru_cache(maxsize=None)
def _single():
    """300 atoms, triclinic box 12, charged cell, three point-charge atoms, cutoff 7: tensors, both list formats, the reference (computed once)."""
    pos, cell, q, sigma = _system(300, seed=5, box=12.0)
    assert abs(q.sum()) > 1.0
    nm, sh, nl, ptr, lsh = _lists(pos, cell, 7.0)
    P, Q, S, C = _t(pos), _t(q), _t(sigma), _t(cell).reshape(1, 3, 3)
    n = pos.shape[0]
    ref = _ref(P, Q, S, C, R.entries_from_matrix(nm, sh, n))
    return dict(P=P, Q=Q, S=S, C=C, nm=nm, sh=sh, nl=nl, ptr=ptr, lsh=lsh, n=n, ref=ref)


@functools.lru_cache(maxsize=None)
def _batch():
    """Two systems with batch_idx: 300 atoms triclinic and NEUTRAL, 420 atoms orthorhombic and charged."""
    p0, c0, q0, s0 = _system(300, seed=7, box=12.0, neutral=True)
    p1, c1, q1, s1 = _system(420, seed=8, box=15.0, triclinic=False)
    q1 += 0.02
    pos, q, sigma, cells = np.concatenate([p0, p1]), np.concatenate([q0, q1]), np.concatenate([s0, s1]), np.stack([c0, c1])
    bi = _t(np.concatenate([np.zeros(300, np.int32), np.ones(420, np.int32)]))
    bptr = _t(np.array([0, 300, 720], np.int32))
    nm, sh, nl, ptr, lsh = _lists(pos, cells, 7.0, batch_idx=bi, batch_ptr=bptr)
    return dict(P=_t(pos), Q=_t(q), S=_t(sigma), C=_t(cells), bi=bi, nm=nm, sh=sh, nl=nl, ptr=ptr, lsh=lsh, n=720,
                parts=((p0, c0, q0, s0), (p1, c1, q1, s1)))


def _fmt_kw(f, fmt):
    if fmt == "matrix":
        return dict(neighbor_matrix=f["nm"], neighbor_matrix_shifts=f["sh"], mask_value=f["n"])
    return dict(neighbor_list=f["nl"], neighbor_ptr=f["ptr"], neighbor_shifts=f["lsh"])


def test_parity_fp64_matrix_and_csr():
    from nvalchemiops.interactions.electrostatics import gaussian_charge_correction as gcc

    f = _single()
    outs = {}
    for fmt in ("matrix", "list"):
        out = gcc(f["P"], f["Q"], f["S"], f["C"], **_fmt_kw(f, fmt), **ALL)
        assert len(out) == 5 and all(o.dtype == torch.float64 for o in out)
        for name, o in zip(NAMES, out):
            err = _close(o, f["ref"][name], f"{fmt} {name}")
            print(f"fp64 {fmt:6s} {name:13s} rel err {err:.2e}")
        outs[fmt] = out
        frc, vir = out[1], out[4]
        assert vir.shape == (1, 3, 3)
        assert float(frc.sum(0).abs().max()) <= 1e-9 * float(frc.abs().max()), "net force"
        assert float((vir - vir.transpose(1, 2)).abs().max()) <= 1e-9 * float(vir.abs().max()), "virial symmetry"
    for name, a, b in zip(NAMES, outs["matrix"], outs["list"]):
        _close(a, b, f"matrix vs CSR {name}", 1e-10)
    # the three point-charge atoms: a width gradient of exactly zero, and the energies of a subset of outputs are those of the full call
    assert float(outs["matrix"][3][f["S"] <= 0].abs().max()) == 0.0
    e, sg = gcc(f["P"], f["Q"], f["S"], f["C"], **_fmt_kw(f, "matrix"), compute_sigma_gradients=True)
    assert torch.equal(e, outs["matrix"][0]) and torch.equal(sg, outs["matrix"][3])
    # the list reaches 7 < 6 g_max: widths enter through more than the self term, and the terms can be switched off one by one
    e_pair = gcc(f["P"], f["Q"], f["S"], f["C"], **_fmt_kw(f, "list"), self_energy=False, neutralizing_background=False)
    ref_pair = R.energies(f["P"], f["Q"], f["S"], f["C"], *R.entries_from_csr(f["nl"], f["ptr"], f["lsh"]), self_energy=False, background=False)
    _close(e_pair, ref_pair, "pair term alone")
    assert float(e_pair.abs().max()) > 1e-3


def test_scalar_sigma_is_expanded():
    from nvalchemiops.interactions.electrostatics import gaussian_charge_correction as gcc

    f = _single()
    want = gcc(f["P"], f["Q"], torch.full((f["n"],), 0.5, dtype=torch.float64, device=DEV), f["C"], **_fmt_kw(f, "matrix"), compute_forces=True)
    for sigma in (0.5, torch.tensor(0.5, device=DEV), torch.tensor(0.5)):
        got = gcc(f["P"], f["Q"], sigma, f["C"], **_fmt_kw(f, "matrix"), compute_forces=True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_padding_rules_empty_rows_and_point_charges():
    from nvalchemiops.interactions.electrostatics import gaussian_charge_correction as gcc

    f = _single()
    n, nm, sh = f["n"], f["nm"], f["sh"]
    base = gcc(f["P"], f["Q"], f["S"], f["C"], **_fmt_kw(f, "matrix"), **ALL)
    used = nm != n
    for fill, mask in ((n, n), (-1, -1), (-1, n), (n, -1)):  # the last two: padding by the "outside [0, N)" rule alone
        wide = torch.full((n, nm.shape[1] + 7), fill, dtype=torch.int32, device=DEV)
        wide[:, : nm.shape[1]] = torch.where(used, nm, torch.full_like(nm, fill))
        wsh = torch.zeros((n, wide.shape[1], 3), dtype=torch.int32, device=DEV)
        wsh[:, : nm.shape[1]] = sh
        out = gcc(f["P"], f["Q"], f["S"], f["C"], neighbor_matrix=wide, neighbor_matrix_shifts=wsh, mask_value=mask, **ALL)
        for name, o, b in zip(NAMES, out, base):
            _close(o, f["ref"][name], f"fill {fill} mask {mask} {name}")
            assert torch.equal(o, b), f"fill {fill} mask {mask} {name}: same entries in the same columns"
    # mask_value = a real atom's index k turns the entries that point to k into padding; with row k emptied too (a row without neighbours) the
    # list is full again: atom k has left the pair sum
    k = 17
    cut = nm.clone()
    cut[k] = n
    out = gcc(f["P"], f["Q"], f["S"], f["C"], neighbor_matrix=cut, neighbor_matrix_shifts=sh, mask_value=k, **ALL)
    ref = _ref(f["P"], f["Q"], f["S"], f["C"], R.entries_from_matrix(cut, sh, k))
    for name, o in zip(NAMES, out):
        _close(o, ref[name], f"mask_value = atom index: {name}")
    assert float(out[1][k].abs().max()) == 0.0 and float((out[0] - base[0]).abs().max()) > 1e-6
    sk, qk = float(f["S"][k]), float(f["Q"][k])
    assert sk > 0
    e_k = qk * qk / (2 * math.sqrt(math.pi) * sk) + 2 * math.pi / float(torch.linalg.det(f["C"][0]).abs()) * float(f["Q"].sum()) * qk * sk * sk
    assert abs(float(out[0][k]) - e_k) <= 1e-13 * abs(e_k)
    # no entries at all: self and background terms only; the same through a CSR list without entries
    none = torch.full((n, 4), n, dtype=torch.int32, device=DEV)
    e_none = gcc(f["P"], f["Q"], f["S"], f["C"], neighbor_matrix=none, neighbor_matrix_shifts=torch.zeros((n, 4, 3), dtype=torch.int32, device=DEV), mask_value=n)
    e_csr = gcc(f["P"], f["Q"], f["S"], f["C"], neighbor_list=torch.zeros((2, 0), dtype=torch.int32, device=DEV),
                neighbor_ptr=torch.zeros(n + 1, dtype=torch.int32, device=DEV), neighbor_shifts=torch.zeros((0, 3), dtype=torch.int32, device=DEV))
    empty = torch.zeros(0, dtype=torch.long, device=DEV)
    _close(e_none, R.energies(f["P"], f["Q"], f["S"], f["C"], empty, empty, torch.zeros((0, 3), dtype=torch.long, device=DEV)), "no entries")
    _close(e_csr, e_none, "no entries, CSR", 1e-15)
    # all sigma <= 0: point charges, exact zeros everywhere
    for sig in (torch.zeros_like(f["S"]), -f["S"] - 0.1, 0.0):
        for fmt in ("matrix", "list"):
            out = gcc(f["P"], f["Q"], sig, f["C"], **_fmt_kw(f, fmt), **ALL)
            for name, o in zip(NAMES, out):
                assert float(o.abs().max()) == 0.0 and not bool(torch.isnan(o).any()), name


def test_batch_parity_slices_and_per_system_background():
    from nvalchemiops.interactions.electrostatics import gaussian_charge_correction as gcc

    b = _batch()
    ref = _ref(b["P"], b["Q"], b["S"], b["C"], R.entries_from_matrix(b["nm"], b["sh"], b["n"]), batch_idx=b["bi"])
    got = {}
    for fmt in ("matrix", "list"):
        got[fmt] = gcc(b["P"], b["Q"], b["S"], b["C"], batch_idx=b["bi"], **_fmt_kw(b, fmt), **ALL)
        assert got[fmt][4].shape == (2, 3, 3)
        for name, o in zip(NAMES, got[fmt]):
            _close(o, ref[name], f"batch {fmt} {name}")
    out = got["matrix"]
    for s, sl in enumerate((slice(0, 300), slice(300, 720))):
        p, c, q, sg = b["parts"][s]
        nm, sh, *_ = _lists(p, c, 7.0)
        alone = gcc(_t(p), _t(q), _t(sg), _t(c).reshape(1, 3, 3), neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=p.shape[0], **ALL)
        for name, o, a in zip(NAMES[:4], out[:4], alone[:4]):
            _close(o[sl], a, f"system {s} alone: {name}", 1e-10)
        _close(out[4][s], alone[4][0], f"system {s} alone: virial", 1e-10)
        assert float(out[1][sl].sum(0).abs().max()) <= 1e-9 * float(out[1].abs().max()), f"net force of system {s}"
    # the background term belongs to each system's own charge and volume: nothing in the neutral system, the closed form in the charged one
    no_bg = gcc(b["P"], b["Q"], b["S"], b["C"], batch_idx=b["bi"], **_fmt_kw(b, "matrix"), neutralizing_background=False, compute_virial=True)
    diff = _np(out[0] - no_bg[0])
    (_, _, q0, _), (_, c1, q1, s1) = b["parts"]
    assert abs(q0.sum()) < 1e-12 and np.abs(diff[:300]).max() <= 1e-13
    want = 2 * math.pi / abs(np.linalg.det(c1)) * q1.sum() * q1 * s1**2
    assert np.abs(want).max() > 1e-4 and np.abs(diff[300:] - want).max() <= 1e-11 * np.abs(want).max()
    dv = _np(out[4] - no_bg[1])
    assert np.abs(dv[0]).max() <= 1e-12 and np.abs(dv[1] - want.sum() * np.eye(3)).max() <= 1e-10 * abs(want.sum())


def test_non_periodic():
    from nvalchemiops.interactions.electrostatics import gaussian_charge_correction as gcc
    from nvalchemiops.neighborlist import neighbor_list

    g = np.random.default_rng(11)
    pos, q, sigma = g.uniform(0, 14.0, (200, 3)), g.normal(size=200), g.uniform(0.3, 0.8, 200)
    sigma[[3, 50]] = 0.0
    P, Q, S = _t(pos), _t(q), _t(sigma)
    nm, num = neighbor_list(P, 7.0, method="naive", max_neighbors=200)
    nl, ptr = neighbor_list(P, 7.0, method="naive", max_neighbors=200, return_neighbor_list=True)
    assert int(num.max()) <= 200 and int(num.sum()) == nl.shape[1] > 1000
    ref = _ref(P, Q, S, None, R.entries_from_matrix(nm, None, 200))
    some = dict(compute_forces=True, compute_charge_gradients=True, compute_sigma_gradients=True)
    for kw in (dict(neighbor_matrix=nm, mask_value=200), dict(neighbor_list=nl, neighbor_ptr=ptr)):
        out = gcc(P, Q, S, **kw, **some)
        assert len(out) == 4
        for name, o in zip(NAMES[:4], out):
            _close(o, ref[name], f"non-periodic {name}")
    with pytest.raises(ValueError, match="compute_virial needs a cell"):
        gcc(P, Q, S, neighbor_matrix=nm, mask_value=200, compute_virial=True)


def test_fp32_inputs():
    from nvalchemiops.interactions.electrostatics import gaussian_charge_correction as gcc

    f = _single()
    P, Q, S, C = (f[k].float() for k in ("P", "Q", "S", "C"))
    ref = _ref(P, Q, S, C, R.entries_from_matrix(f["nm"], f["sh"], f["n"]), distance_dtype=torch.float32)
    for fmt in ("matrix", "list"):
        out = gcc(P, Q, S, C, **_fmt_kw(f, fmt), **ALL)
        assert all(o.dtype == torch.float32 for o in out)
        for name, o in zip(NAMES, out):
            err = _close(o, ref[name], f"fp32 {fmt} {name}", 1e-6)
            print(f"fp32 {fmt:6s} {name:13s} rel err {err:.2e} (bar 1e-6)")


@pytest.mark.parametrize("fmt", ["list", "matrix"])
def test_autograd_matches_reference_and_explicit_outputs(fmt):
    from nvalchemiops.interactions.electrostatics import gaussian_charge_correction as gcc

    b = _batch()
    w = _t(np.random.default_rng(3).uniform(0.2, 1.8, b["n"]))
    ref = _ref(b["P"], b["Q"], b["S"], b["C"], R.entries_from_matrix(b["nm"], b["sh"], b["n"]), batch_idx=b["bi"], weights=w)
    leaves = [b[k].clone().requires_grad_(True) for k in ("P", "Q", "S", "C")]
    e = gcc(*leaves, batch_idx=b["bi"], **_fmt_kw(b, fmt))
    assert e.requires_grad
    (e * w).sum().backward()
    _close(-leaves[0].grad, ref["forces"], "dL/dr", 1e-10)
    _close(leaves[1].grad, ref["charge_grads"], "dL/dq", 1e-10)
    _close(leaves[2].grad, ref["sigma_grads"], "dL/dsigma", 1e-10)
    _close(leaves[3].grad, ref["cell_grads"], "dL/dcell", 1e-10)
    # w = 1: the gradients of the total energy are the explicit outputs
    leaves = [b[k].clone().requires_grad_(True) for k in ("P", "Q", "S", "C")]
    e, frc, cg, sg = gcc(*leaves, batch_idx=b["bi"], **_fmt_kw(b, fmt), compute_forces=True, compute_charge_gradients=True, compute_sigma_gradients=True)
    e.sum().backward()
    _close(-leaves[0].grad, frc, "-dE/dr vs forces", 1e-10)
    _close(leaves[1].grad, cg, "dE/dq vs charge gradients", 1e-10)
    _close(leaves[2].grad, sg, "dE/dsigma vs sigma gradients", 1e-10)
    eager = gcc(b["P"], b["Q"], b["S"], b["C"], batch_idx=b["bi"], **_fmt_kw(b, fmt), compute_forces=True)
    assert torch.equal(e.detach(), eager[0]) and torch.equal(frc.detach(), eager[1])


def test_autograd_without_cell_and_second_order_is_refused():
    from nvalchemiops.interactions.electrostatics import gaussian_charge_correction as gcc

    f = _single()
    # a loss on the explicit forces (or any explicit gradient, or the virial) is a second derivative: refused at backward, never a silent zero
    for flag in ("compute_forces", "compute_charge_gradients", "compute_sigma_gradients", "compute_virial"):
        P = f["P"].clone().requires_grad_(True)
        _, explicit = gcc(P, f["Q"], f["S"], f["C"], **_fmt_kw(f, "matrix"), **{flag: True})
        with pytest.raises(NotImplementedError, match="second derivatives of the pair kernels"):
            explicit.sum().backward()
    # only the charges require grad, no cell: dE/dq through the op equals the explicit gradient
    g = np.random.default_rng(2)
    P, S = _t(g.uniform(0, 9.0, (90, 3))), _t(g.uniform(0.3, 0.8, 90))
    Q = _t(g.normal(size=90)).requires_grad_(True)
    from nvalchemiops.neighborlist import neighbor_list

    nm, _ = neighbor_list(P, 6.0, method="naive", max_neighbors=120)
    e, cg = gcc(P, Q, S, neighbor_matrix=nm, mask_value=90, compute_charge_gradients=True)
    e.sum().backward()
    _close(Q.grad, cg, "dE/dq, non-periodic", 1e-10)


def test_compile_fullgraph_equals_eager_bitwise():
    from nvalchemiops.interactions.electrostatics import gaussian_charge_correction as gcc

    f = _single()

    def fn(p, q, s):
        e, frc = gcc(p, q, s, f["C"], neighbor_matrix=f["nm"], neighbor_matrix_shifts=f["sh"], mask_value=f["n"], compute_forces=True)
        return e.sum() * 2.0, frc

    torch._dynamo.reset()
    got = torch.compile(fn, mode="default", fullgraph=True)(f["P"], f["Q"], f["S"])
    want = fn(f["P"], f["Q"], f["S"])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_side_stream_equals_default_stream_bitwise():
    from nvalchemiops.interactions.electrostatics import gaussian_charge_correction as gcc

    b = _batch()
    ref = gcc(b["P"], b["Q"], b["S"], b["C"], batch_idx=b["bi"], **_fmt_kw(b, "list"), **ALL)
    torch.cuda.current_stream().synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = gcc(b["P"], b["Q"], b["S"], b["C"], batch_idx=b["bi"], **_fmt_kw(b, "list"), **ALL)
    side.synchronize()
    for name, o, r in zip(NAMES, out, ref):
        assert torch.equal(o, r), name


def test_end_to_end_point_charge_ewald_plus_correction_against_the_exact_gaussian_sum():
    """A = ewald_summation total, B = A + correction total; A* = numpy point-charge Ewald with exact erfc, B* = the k-space Gaussian sum (no erfc).
    |B - B*| <= |A - A*| + 1e-10 |B*|: the composite is no further from exact than the point-charge routine (polynomial erfc) already is."""
    from nvalchemiops.interactions.electrostatics import ewald_summation, gaussian_charge_correction as gcc

    g = np.random.default_rng(21)
    cell = np.diag([15.0, 16.0, 17.0])
    pos, q, sigma = g.uniform(0, 1, (64, 3)) @ cell, g.normal(size=64), g.uniform(0.45, 0.6, 64)
    nm, sh, *_ = _lists(pos, cell, 7.4, max_neighbors=160)  # 6 g_max = 6 sqrt(4 * 0.36) = 7.2 < 7.4 < half the shortest edge
    P, Q, S, C = _t(pos), _t(q), _t(sigma), _t(cell).reshape(1, 3, 3)
    # alpha = 0.9: erfc(0.9 * 7.4) = 4e-21 beyond the list; k_cutoff = 12: exp(-144 / 3.24) = 5e-20
    a = float(ewald_summation(P, Q, C, alpha=0.9, k_cutoff=12.0, neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=64).sum())
    b = a + float(gcc(P, Q, S, C, neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=64).sum())
    a_star = R.point_charge_ewald_exact(pos, q, cell, 0.6, 1, 21)
    b_star = R.gaussian_kspace_exact(pos, q, sigma, cell, 33)
    print(f"|A - A*| = {abs(a - a_star):.3e} (A* = {a_star:.12e})   |B - B*| = {abs(b - b_star):.3e} (B* = {b_star:.12e})")
    assert abs(b - b_star) <= abs(a - a_star) + 1e-10 * abs(b_star)
