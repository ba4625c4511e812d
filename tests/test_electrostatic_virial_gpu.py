"""Electrostatic virial in the forward pass: `ewald_real_space_with_virial`, `pme_reciprocal_space_with_virial`, `particle_mesh_ewald_with_virial`,
`ewald_reciprocal_space_with_virial`, `ewald_summation_with_virial`.

Contract: W_s[a, b] = -dE_s/d eps[a, b] at eps = 0 under x -> (I + eps) x of every position and every lattice vector (rows of `cell`), with
alpha, the mesh, the spline order, the unit shifts and the Miller indices of the k set held fixed.  "The strain derivative" below is that
derivative taken by autograd through the EXISTING functions (positions pos (I + eps)^T, cell cell (I + eps)^T)."""
import math

import numpy as np
import pytest
import torch

from tests import systems as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _system(n, seed=0, box=12.0, dtype=np.float64, charged=False):
    rng = np.random.default_rng(seed)
    cell = (np.eye(3) * box + 0.8 * rng.standard_normal((3, 3))).astype(dtype)
    pos = (rng.random((n, 3)) @ cell).astype(dtype)
    q = rng.standard_normal(n)
    if not charged:
        q -= q.mean()
    return pos, cell, q.astype(dtype)


def _strained(pos, cell, eps, batch_idx=None):
    """positions and cells of the strained systems: x -> (I + eps_s) x, rows of cell likewise."""
    f = torch.eye(3, dtype=eps.dtype, device=eps.device) + eps               # [B, 3, 3]
    fa = f[batch_idx.long()] if batch_idx is not None else f[0].expand(pos.shape[0], 3, 3)
    return (fa @ pos.unsqueeze(-1)).squeeze(-1), cell.reshape(-1, 3, 3) @ f.transpose(-1, -2)


def _per_system(e, batch_idx, nsys):
    if batch_idx is None:
        return e.sum().reshape(1)
    return torch.zeros(nsys, dtype=e.dtype, device=e.device).index_add(0, batch_idx.long(), e)


def _strain_derivative(energy_fn, pos, cell, batch_idx=None):
    """-dE_s/d eps_s by autograd through `energy_fn(positions, cells) -> per-atom energies` (the existing, differentiable functions)."""
    nsys = cell.reshape(-1, 3, 3).shape[0] if batch_idx is not None else 1
    eps = torch.zeros((nsys, 3, 3), dtype=pos.dtype, device=pos.device, requires_grad=True)
    p, c = _strained(pos, cell, eps, batch_idx)
    e = energy_fn(p, c)
    (g,) = torch.autograd.grad(_per_system(e, batch_idx, nsys).sum(), eps)
    return -g


def _strain_fd(energy_fn, pos, cell, h=1e-5):
    """central finite differences of the summed energy of one system under the strain (no autograd)."""
    w = torch.zeros((3, 3), dtype=F64)
    with torch.no_grad():
        for a in range(3):
            for b in range(3):
                e = []
                for s in (h, -h):
                    eps = torch.zeros((1, 3, 3), dtype=pos.dtype, device=pos.device)
                    eps[0, a, b] = s
                    p, c = _strained(pos, cell, eps)
                    e.append(float(energy_fn(p, c).to(F64).sum()))
                w[a, b] = -(e[0] - e[1]) / (2 * h)
    return w


def _same(a, b):
    """The sibling's outputs.  The PME spread adds with float atomics, so the sibling is not bitwise reproducible between two of its own calls
    (last-bit differences, measured); 'same outputs' is therefore checked at 1e-12 of the largest value, far below any path difference."""
    torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12 * float(b.abs().max()))
    return True


def _close(a, b, rtol, what=""):
    a, b = a.detach().to(F64).cpu(), b.detach().to(F64).cpu()
    scale = float(b.abs().max())
    err = float((a - b).abs().max())
    assert err <= rtol * scale, f"{what}: max |dW| = {err:.3e} > {rtol:.0e} x {scale:.3e}"


# ------------------------------------------------------------------------------------------------------------------------------ real space
def _real_inputs(kind, n=160, seed=3):
    from nvalchemiops.neighborlist import neighbor_list

    pos, cell, q = _system(n, seed=seed)
    P, Cc, Q = _t(pos), _t(cell), _t(q)
    pbc = torch.tensor([True] * 3, device=DEV)
    if kind == "csr":
        lst, nptr, lsh = neighbor_list(P, 6.0, cell=Cc, pbc=pbc, method="cell_list", return_neighbor_list=True)
        return P, Cc, Q, dict(neighbor_list=lst, neighbor_ptr=nptr, neighbor_shifts=lsh)
    nm, num, sh = neighbor_list(P, 6.0, cell=Cc, pbc=pbc, method="cell_list", max_neighbors=128, half_fill=(kind == "half"))
    if kind == "asym":
        nm, sh = nm.clone(), sh.clone()
        nm[::3, 0] = n        # drop the first entry of every third row (padding = mask_value n): the list is no longer symmetric
        sh[5, 1] = sh[5, 1] + 1
    return P, Cc, Q, dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=n)


@pytest.mark.parametrize("kind", ["csr", "matrix", "half", "asym"])
def test_real_space_matches_strain_derivative(kind):
    from nvalchemiops.interactions.electrostatics import ewald_real_space, ewald_real_space_with_virial

    P, Cc, Q, nl = _real_inputs(kind)
    alpha = torch.tensor([0.35], dtype=F64, device=DEV)
    e, f, w = ewald_real_space_with_virial(P, Q, Cc[None], alpha, compute_forces=True, **nl)
    e0, f0 = ewald_real_space(P, Q, Cc[None], alpha, compute_forces=True, **nl)
    assert torch.equal(e, e0)
    if kind in ("half", "asym"):  # forces of a non-symmetric list take the atomic scatter: run-to-run order of the adds
        torch.testing.assert_close(f, f0, rtol=1e-12, atol=1e-14)
    else:
        assert torch.equal(f, f0)
    assert w.shape == (1, 3, 3) and w.dtype == F64
    ref = _strain_derivative(lambda p, c: ewald_real_space(p, Q, c, alpha, **nl), P, Cc)
    _close(w, ref, 1e-10, kind)


def test_real_space_batch_triclinic_own_alpha():
    from nvalchemiops.interactions.electrostatics import ewald_real_space, ewald_real_space_with_virial
    from nvalchemiops.neighborlist import neighbor_list

    parts = [_system(90 + 20 * b, seed=10 + b, box=11.0 + b) for b in range(3)]
    P = _t(np.concatenate([p[0] for p in parts]))
    Q = _t(np.concatenate([p[2] for p in parts]))
    Cc = _t(np.stack([p[1] for p in parts]))
    bi = _t(np.concatenate([np.full(len(p[0]), b) for b, p in enumerate(parts)]).astype(np.int32))
    nm, num, sh = neighbor_list(P, 6.0, cell=Cc, pbc=torch.tensor([[True] * 3] * 3, device=DEV), batch_idx=bi, method="batch_cell_list",
                                max_neighbors=128)
    alpha = torch.tensor([0.3, 0.35, 0.4], dtype=F64, device=DEV)
    nl = dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=P.shape[0], batch_idx=bi)
    e, w = ewald_real_space_with_virial(P, Q, Cc, alpha, **nl)
    assert torch.equal(e, ewald_real_space(P, Q, Cc, alpha, **nl)) and w.shape == (3, 3, 3)
    ref = _strain_derivative(lambda p, c: ewald_real_space(p, Q, c, alpha, **nl), P, Cc, batch_idx=bi)
    for b in range(3):
        _close(w[b], ref[b], 1e-10, f"system {b}")


def test_real_space_fp32_and_trusted_form():
    from nvalchemiops.interactions.electrostatics import ewald_real_space_with_virial
    from nvalchemiops.neighborlist import invalidate, neighbor_list

    pos, cell, q = _system(400, seed=5, box=16.0)
    w = {}
    for dt in (np.float64, np.float32):
        P, Cc, Q = _t(pos.astype(dt)), _t(cell.astype(dt)), _t(q.astype(dt))
        nm, num, sh = neighbor_list(P, 7.0, cell=Cc, pbc=torch.tensor([True] * 3, device=DEV), method="cell_list", max_neighbors=160)
        alpha = torch.tensor([0.35], dtype=P.dtype, device=DEV)
        w[dt] = ewald_real_space_with_virial(P, Q, Cc[None], alpha, neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=400)[-1]
        if dt == np.float64:
            trusted = w[dt]
            invalidate(nm, sh)
            general = ewald_real_space_with_virial(P, Q, Cc[None], alpha, neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=400)[-1]
            _close(trusted, general, 1e-12, "trusted vs general")
    assert w[np.float32].dtype == torch.float32
    _close(w[np.float32], w[np.float64], 1e-4, "fp32 vs fp64")


# -------------------------------------------------------------------------------------------------------------------------- PME reciprocal
def _pme_case(batched, triclinic=True, n=120):
    if not batched:
        pos, cell, q = _system(n, seed=21, box=10.0 if triclinic else 10.0)
        if not triclinic:
            cell = np.eye(3) * 10.0
            pos = np.mod(pos, 10.0)
        return _t(pos), _t(cell), _t(q), None
    parts = [_system(n - 30 * b, seed=30 + b, box=9.0 + b) for b in range(2)]
    P = _t(np.concatenate([p[0] for p in parts]))
    Q = _t(np.concatenate([p[2] for p in parts]))
    Cc = _t(np.stack([p[1] for p in parts]))
    bi = _t(np.concatenate([np.full(len(p[0]), b) for b, p in enumerate(parts)]).astype(np.int32))
    return P, Cc, Q, bi


@pytest.mark.parametrize("order", [4, 5])
@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("mesh", [(30, 30, 30), (28, 28, 28)])
def test_pme_reciprocal_matches_strain_derivative(order, batched, mesh):
    from nvalchemiops.interactions.electrostatics import pme_reciprocal_space, pme_reciprocal_space_with_virial

    P, Cc, Q, bi = _pme_case(batched)
    cells = Cc if batched else Cc[None]
    nsys = cells.shape[0] if batched else 1
    alpha = torch.full((cells.shape[0],), 0.4, dtype=F64, device=DEV)
    kw = dict(mesh_dimensions=mesh, spline_order=order, batch_idx=bi)
    e, f, w = pme_reciprocal_space_with_virial(P, Q, cells, alpha, compute_forces=True, **kw)
    e0, f0 = pme_reciprocal_space(P, Q, cells, alpha, compute_forces=True, **kw)
    assert _same(e, e0) and _same(f, f0) and w.shape == (nsys, 3, 3)
    ref = _strain_derivative(lambda p, c: pme_reciprocal_space(p, Q, c, alpha, **kw), P, cells, batch_idx=bi)
    _close(w, ref, 1e-9, f"order {order} mesh {mesh}")


def test_pme_reciprocal_dense_dft_and_caller_k(monkeypatch):
    from nvalchemiops.interactions.electrostatics import generate_k_vectors_pme, pme_reciprocal_space, pme_reciprocal_space_with_virial
    from nvalchemiops.interactions.electrostatics import pme as PM

    P, Cc, Q, _ = _pme_case(False)
    alpha = torch.tensor([0.4], dtype=F64, device=DEV)
    mesh = (20, 18, 22)
    kw = dict(mesh_dimensions=mesh, spline_order=4)
    ref = _strain_derivative(lambda p, c: pme_reciprocal_space(p, Q, c, alpha, **kw), P, Cc[None])
    # caller-supplied k arrays: the derivative through the existing function with k generated from the strained cell
    kv, k2 = generate_k_vectors_pme(Cc, mesh)
    w_k = pme_reciprocal_space_with_virial(P, Q, Cc[None], alpha, k_vectors=kv, k_squared=k2, **kw)[-1]
    ref_k = _strain_derivative(lambda p, c: pme_reciprocal_space(p, Q, c, alpha, k_vectors=generate_k_vectors_pme(c[0], mesh)[0],
                                                                 k_squared=generate_k_vectors_pme(c[0], mesh)[1], **kw), P, Cc[None])
    _close(w_k, ref_k, 1e-9, "caller k")
    _close(w_k, ref, 1e-9, "caller k vs cell k")
    monkeypatch.setattr(PM, "_FORCE_DFT", True)
    monkeypatch.setattr(PM, "_MESH_SOLVE", False)
    monkeypatch.setattr(PM, "_FFT_LDS", False)
    e, w = pme_reciprocal_space_with_virial(P, Q, Cc[None], alpha, **kw)
    assert _same(e, pme_reciprocal_space(P, Q, Cc[None], alpha, **kw))
    _close(w, ref, 1e-9, "dense DFT")


# ---------------------------------------------------------------------------------------------------------------------- explicit-k Ewald
@pytest.mark.parametrize("batched", [False, True])
def test_ewald_reciprocal_matches_strain_derivative(batched):
    from nvalchemiops.interactions.electrostatics import (ewald_reciprocal_space, ewald_reciprocal_space_with_virial,
                                                          generate_k_vectors_ewald_summation)

    P, Cc, Q, bi = _pme_case(batched, n=80)
    cells = Cc if batched else Cc[None]
    alpha = torch.full((cells.shape[0],), 0.45, dtype=F64, device=DEV)
    kv = generate_k_vectors_ewald_summation(cells, 6.0)
    e, f, w = ewald_reciprocal_space_with_virial(P, Q, cells, kv, alpha, batch_idx=bi, compute_forces=True)
    e0, f0 = ewald_reciprocal_space(P, Q, cells, kv, alpha, batch_idx=bi, compute_forces=True)
    assert torch.equal(e, e0) and torch.equal(f, f0)
    ref = _strain_derivative(lambda p, c: ewald_reciprocal_space(p, Q, c, generate_k_vectors_ewald_summation(c, 6.0), alpha, batch_idx=bi),
                             P, cells, batch_idx=bi)
    _close(w, ref, 1e-10, "explicit k")


# ------------------------------------------------------------------------------------------------------------------------------ totals
def _pme_total_inputs(n=300, seed=8, box=14.0, rc=7.0):
    from nvalchemiops.neighborlist import neighbor_list

    pos, cell, q = _system(n, seed=seed, box=box)
    P, Cc, Q = _t(pos), _t(cell), _t(q)
    nm, num, sh = neighbor_list(P, rc, cell=Cc, pbc=torch.tensor([True] * 3, device=DEV), method="cell_list", max_neighbors=256)
    return P, Cc, Q, nm, sh


def test_totals_bit_equal_and_sum_of_parts():
    from nvalchemiops.interactions.electrostatics import (ewald_real_space_with_virial, ewald_reciprocal_space_with_virial, ewald_summation,
                                                          ewald_summation_with_virial, generate_k_vectors_ewald_summation, particle_mesh_ewald,
                                                          particle_mesh_ewald_with_virial, pme_reciprocal_space_with_virial)

    P, Cc, Q, nm, sh = _pme_total_inputs()
    kw = dict(alpha=0.4, mesh_dimensions=(30, 30, 30), spline_order=5, neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    e, f, w = particle_mesh_ewald_with_virial(P, Q, Cc, compute_forces=True, **kw)
    e0, f0 = particle_mesh_ewald(P, Q, Cc, compute_forces=True, **kw)
    assert _same(e, e0) and _same(f, f0)
    alpha = torch.tensor([0.4], dtype=F64, device=DEV)
    w_r = ewald_real_space_with_virial(P, Q, Cc[None], alpha, neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=P.shape[0])[-1]
    w_k = pme_reciprocal_space_with_virial(P, Q, Cc[None], alpha, mesh_dimensions=(30, 30, 30), spline_order=5)[-1]
    _close(w, w_r + w_k, 1e-13, "PME total vs parts")
    kv = generate_k_vectors_ewald_summation(Cc[None], 5.0)
    kw2 = dict(alpha=0.4, k_vectors=kv, neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    e, f, w = ewald_summation_with_virial(P, Q, Cc, compute_forces=True, **kw2)
    e0, f0 = ewald_summation(P, Q, Cc, compute_forces=True, **kw2)
    assert torch.equal(e, e0) and torch.equal(f, f0)
    w_k = ewald_reciprocal_space_with_virial(P, Q, Cc[None], kv, alpha)[-1]
    _close(w, w_r + w_k, 1e-13, "Ewald total vs parts")


def test_pme_total_matches_strain_derivative():
    from nvalchemiops.interactions.electrostatics import particle_mesh_ewald, particle_mesh_ewald_with_virial

    P, Cc, Q, nm, sh = _pme_total_inputs()
    kw = dict(alpha=0.4, mesh_dimensions=(30, 30, 30), spline_order=5, neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    w = particle_mesh_ewald_with_virial(P, Q, Cc, **kw)[-1]
    ref = _strain_derivative(lambda p, c: particle_mesh_ewald(p, Q, c, **kw), P, Cc)
    _close(w, ref, 1e-9, "PME total")


# ------------------------------------------------------------------------------------------------------------------------ physics anchors
def _ewald_full(pos, cell, q, accuracy):
    from nvalchemiops.interactions.electrostatics import estimate_ewald_parameters, ewald_summation_with_virial
    from nvalchemiops.neighborlist import neighbor_list

    P, Cc, Q = _t(pos), _t(cell), _t(q)
    prm = estimate_ewald_parameters(P, Cc[None], None, accuracy)
    rc = float(prm.real_space_cutoff.reshape(-1)[0])
    nm, num, sh = neighbor_list(P, rc, cell=Cc, pbc=torch.tensor([True] * 3, device=DEV), method="cell_list", max_neighbors=2048)
    assert int(num.max()) <= 2048
    e, w = ewald_summation_with_virial(P, Q, Cc, neighbor_matrix=nm, neighbor_matrix_shifts=sh, accuracy=accuracy)
    return P, Cc, Q, nm, sh, e, w


@pytest.mark.parametrize("charged", [False, True])
def test_trace_equals_energy_ewald(charged):
    pos, cell, q = _system(64, seed=41, box=9.0, charged=charged)
    *_, e, w = _ewald_full(pos, cell, q, 1e-8)
    tr, etot = float(torch.diagonal(w[0]).sum()), float(e.sum())
    assert abs(tr - etot) <= 1e-6 * abs(etot), (tr, etot)


def test_trace_equals_energy_pme():
    from nvalchemiops.interactions.electrostatics import estimate_ewald_parameters, particle_mesh_ewald_with_virial

    pos, cell, q = _system(64, seed=41, box=9.0)
    P, Cc, Q, nm, sh, e_ew, _ = _ewald_full(pos, cell, q, 1e-8)
    alpha = float(estimate_ewald_parameters(P, Cc[None], None, 1e-8).alpha.reshape(-1)[0])
    e, w = particle_mesh_ewald_with_virial(P, Q, Cc, alpha=alpha, mesh_dimensions=(48, 48, 48), spline_order=6, neighbor_matrix=nm,
                                           neighbor_matrix_shifts=sh, mask_value=P.shape[0])
    gap = abs(float(e.sum()) - float(e_ew.sum())) / abs(float(e_ew.sum()))
    tr, etot = float(torch.diagonal(w[0]).sum()), float(e.sum())
    assert abs(tr - etot) <= max(10 * gap, 1e-12) * abs(etot), (tr, etot, gap)


def test_nacl_isotropic():
    from nvalchemiops.interactions.electrostatics import ewald_summation_with_virial
    from nvalchemiops.neighborlist import neighbor_list

    a, nc = 5.64, 2
    ijk = np.stack(np.meshgrid(*[np.arange(2 * nc)] * 3, indexing="ij"), -1).reshape(-1, 3)
    pos = ijk * (a / 2)
    q = np.where(ijk.sum(1) % 2 == 0, 1.0, -1.0)
    cell = np.eye(3) * a * nc
    P, Cc, Q = _t(pos), _t(cell), _t(q)
    nm, num, sh = neighbor_list(P, 9.0, cell=Cc, pbc=torch.tensor([True] * 3, device=DEV), method="cell_list", max_neighbors=512)
    e, w = ewald_summation_with_virial(P, Q, Cc, alpha=0.45, k_cutoff=9.0, neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    iso = float(e.sum()) / 3.0 * torch.eye(3, dtype=F64)
    _close(w[0], iso, 1e-6, "NaCl")


def test_finite_differences_each_function():
    from nvalchemiops.interactions.electrostatics import (ewald_real_space, ewald_real_space_with_virial, ewald_reciprocal_space,
                                                          ewald_reciprocal_space_with_virial, ewald_summation, ewald_summation_with_virial,
                                                          generate_k_vectors_ewald_summation, particle_mesh_ewald, particle_mesh_ewald_with_virial,
                                                          pme_reciprocal_space, pme_reciprocal_space_with_virial)

    P, Cc, Q, nm, sh = _pme_total_inputs(n=96, box=10.0, rc=6.0)
    al = torch.tensor([0.45], dtype=F64, device=DEV)
    nl = dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=P.shape[0])
    pk = dict(mesh_dimensions=(24, 24, 24), spline_order=5)
    miller = generate_k_vectors_ewald_summation(Cc[None], 5.0)[0] @ Cc.T / (2 * math.pi)   # fixed Miller set
    kv_of = lambda c: (miller @ torch.linalg.inv(c.reshape(3, 3)).T * 2 * math.pi)[None]  # noqa: E731
    cases = {
        "real": (lambda p, c: ewald_real_space(p, Q, c.reshape(1, 3, 3), al, **nl), ewald_real_space_with_virial(P, Q, Cc[None], al, **nl)[-1]),
        "pme_recip": (lambda p, c: pme_reciprocal_space(p, Q, c.reshape(1, 3, 3), al, **pk),
                      pme_reciprocal_space_with_virial(P, Q, Cc[None], al, **pk)[-1]),
        "pme": (lambda p, c: particle_mesh_ewald(p, Q, c.reshape(3, 3), alpha=0.45, **pk, **nl),
                particle_mesh_ewald_with_virial(P, Q, Cc, alpha=0.45, **pk, **nl)[-1]),
        "ewald_recip": (lambda p, c: ewald_reciprocal_space(p, Q, c.reshape(1, 3, 3), kv_of(c), al),
                        ewald_reciprocal_space_with_virial(P, Q, Cc[None], kv_of(Cc), al)[-1]),
        "ewald": (lambda p, c: ewald_summation(p, Q, c.reshape(1, 3, 3), alpha=0.45, k_vectors=kv_of(c), **nl),
                  ewald_summation_with_virial(P, Q, Cc[None], alpha=0.45, k_vectors=kv_of(Cc), **nl)[-1]),
    }
    # the pair energy uses the Abramowitz-Stegun erfc polynomial (as the reference does) while forces and virial use the exact derivative of
    # erfc: finite differences of the computed energy see that ~1e-7 gap, so the parts with a real-space sum get 1e-5
    for name, (fn, w) in cases.items():
        _close(w[0], _strain_fd(fn, P, Cc), 1e-6 if name in ("pme_recip", "ewald_recip") else 1e-5, name)


# ------------------------------------------------------------------------------------------------------------------------- config-4 box
def test_config4_box():
    from nvalchemiops.interactions.electrostatics import particle_mesh_ewald, particle_mesh_ewald_with_virial
    from nvalchemiops.neighborlist import neighbor_list

    pos, cell, q, _ = S.fcc_box(100000, seed=1234, dtype=np.float64)
    P, Cc, Q = _t(pos), _t(cell), _t(q)
    nm, num, sh = neighbor_list(P, 9.0, cell=Cc, pbc=torch.tensor([True] * 3, device=DEV), method="cell_list", max_neighbors=256)
    kw = dict(alpha=0.35, mesh_dimensions=(128, 128, 128), spline_order=5, neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    e, f, w = particle_mesh_ewald_with_virial(P, Q, Cc, compute_forces=True, **kw)
    e0, f0 = particle_mesh_ewald(P, Q, Cc, compute_forces=True, **kw)
    assert _same(e, e0) and _same(f, f0)
    ref = _strain_derivative(lambda p, c: particle_mesh_ewald(p, Q, c, **kw), P, Cc)
    _close(w, ref, 1e-8, "config 4")
    tr, etot = float(torch.diagonal(w[0]).sum()), float(e.sum())
    assert abs(tr - etot) <= 1e-3 * abs(etot), (tr, etot)


# ------------------------------------------------------------------------------------------------------------------------- convention
def test_dftd3_virial_convention():
    from nvalchemiops.interactions.dispersion import D3Parameters, dftd3
    from nvalchemiops.neighborlist import neighbor_list

    pos, cell, _, numbers = S.fcc_box(256, dtype=np.float64)
    tables = S.d3_test_tables(17)
    params = D3Parameters(rcov=_t(tables["rcov"]), r4r2=_t(tables["r4r2"]), c6ab=_t(tables["c6ab"]), cn_ref=_t(tables["cn_ref"]))
    p32, c32 = _t(pos.astype(np.float32)), _t(cell.astype(np.float32))
    Z = _t(numbers)
    bj = dict(a1=0.4289, a2=4.4407, s8=0.7875)

    nm, num, sh = neighbor_list(p32, 12.0, cell=c32, pbc=torch.tensor([True] * 3, device=DEV), method="cell_list", max_neighbors=512)

    def energy(p, c):  # the same list and shifts under the strain (no pair crosses the cut-off between the two sides of a difference)
        return dftd3(p, Z, d3_params=params, neighbor_matrix=nm, neighbor_matrix_shifts=sh, cell=c.reshape(1, 3, 3), **bj)[0]

    vir = dftd3(p32, Z, d3_params=params, neighbor_matrix=nm, neighbor_matrix_shifts=sh, cell=c32[None], compute_virial=True, **bj)[3]
    fd = _strain_fd(energy, p32, c32, h=1e-3)
    v = vir[0].to(F64).cpu()
    diag = torch.diagonal(v)
    assert torch.all(torch.sign(diag) == torch.sign(torch.diagonal(fd))), (v, fd)
    assert float((v - fd).abs().max()) <= 0.01 * float(fd.abs().max()), (v, fd)


# ---------------------------------------------------------------------------------------------------------------- autograd and compile
def test_autograd_gradients_and_virial_backward_raises():
    from nvalchemiops.interactions.electrostatics import (ewald_real_space, ewald_real_space_with_virial, particle_mesh_ewald,
                                                          particle_mesh_ewald_with_virial)

    P, Cc, Q, nm, sh = _pme_total_inputs()
    kw = dict(alpha=0.4, mesh_dimensions=(30, 30, 30), spline_order=5, neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    grads = []
    for fn in (particle_mesh_ewald, particle_mesh_ewald_with_virial):
        p, q = P.clone().requires_grad_(True), Q.clone().requires_grad_(True)
        out = fn(p, q, Cc, compute_forces=True, **kw)
        loss = out[0].sum() + (out[1] ** 2).sum()
        grads.append(torch.autograd.grad(loss, (p, q)))
    for a, b in zip(*grads):
        assert _same(a, b)
    p = P.clone().requires_grad_(True)
    w = particle_mesh_ewald_with_virial(p, Q, Cc, **kw)[-1]
    with pytest.raises(NotImplementedError):
        torch.autograd.grad(w.sum(), p)
    alpha = torch.tensor([0.4], dtype=F64, device=DEV)
    p = P.clone().requires_grad_(True)
    e, w = ewald_real_space_with_virial(p, Q, Cc[None], alpha, neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=P.shape[0])
    g = torch.autograd.grad(e.sum(), p, retain_graph=True)[0]
    p2 = P.clone().requires_grad_(True)
    g0 = torch.autograd.grad(ewald_real_space(p2, Q, Cc[None], alpha, neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=P.shape[0]).sum(), p2)[0]
    assert torch.equal(g, g0)
    with pytest.raises(NotImplementedError):
        torch.autograd.grad(w.sum(), p)


def test_compile_fullgraph_matches_eager():
    from nvalchemiops.interactions.electrostatics import (ewald_real_space_with_virial, ewald_reciprocal_space_with_virial,
                                                          generate_k_vectors_ewald_summation, particle_mesh_ewald_with_virial,
                                                          pme_reciprocal_space_with_virial)

    torch._dynamo.reset()
    P, Cc, Q, nm, sh = _pme_total_inputs()
    alpha = torch.tensor([0.4], dtype=F64, device=DEV)
    kv = generate_k_vectors_ewald_summation(Cc[None], 5.0)
    fns = {
        "real": lambda p: ewald_real_space_with_virial(p, Q, Cc[None], alpha, neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=P.shape[0],
                                                       compute_forces=True),
        "pme_recip": lambda p: pme_reciprocal_space_with_virial(p, Q, Cc[None], alpha, mesh_dimensions=(30, 30, 30), spline_order=5),
        "pme": lambda p: particle_mesh_ewald_with_virial(p, Q, Cc, alpha=alpha, mesh_dimensions=(30, 30, 30), spline_order=5, neighbor_matrix=nm,
                                                         neighbor_matrix_shifts=sh, compute_forces=True),
        "ewald_recip": lambda p: ewald_reciprocal_space_with_virial(p, Q, Cc[None], kv, alpha),
    }
    for name, fn in fns.items():
        eager = fn(P)
        compiled = torch.compile(fn, fullgraph=True)(P)
        for a, b in zip(eager, compiled):
            torch.testing.assert_close(b, a, rtol=1e-10, atol=1e-12, msg=name)
