"""GPU parity of the HIP electrostatics path (real-space erfc sum, B-spline spread/gather, k-space kernels, full PME)
against the CPU oracle, an independent explicit Ewald sum and Madelung constants.

Tolerances: fp64 -- same algorithm, differences only from atomic/FFT summation order: energies rtol 1e-10 of the
largest |E_i|, forces 1e-9 of the largest |F|; fp32 -- rtol 1e-4 / atol 1e-5 (reference's own fp32-vs-fp64 tolerance,
test/interactions/electrostatics/test_pme.py:258-261)."""
import os

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import systems as S

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["tile", "auto"])
def spread_path(request, monkeypatch):
    """Every test of this module runs twice: with the tile pipeline forced wherever the mesh allows it (the kernels of the large-system path, driven
    here by small inputs) and with the library's own policy (small systems: zero-fill + atomic spread + per-atom gather)."""
    from nvalchemiops import spline

    monkeypatch.setattr(spline, "_SPREAD_PATH", request.param)

DEV = "cuda:0"


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _close(got, ref, dtype, what, scale=None):
    got = got.detach().cpu().numpy()
    scale = np.abs(ref).max() if scale is None else scale
    tol = (1e-10 if dtype == np.float64 else 1e-4) * scale + (1e-12 if dtype == np.float64 else 1e-5)
    err = np.abs(got - ref).max()
    assert err <= tol, f"{what}: max err {err:.3e} > {tol:.3e}"


def _system(n, dtype, triclinic=False, seed=0, box=12.0):
    g = np.random.default_rng(seed)
    cell = np.eye(3) * box
    if triclinic:
        cell = np.array([[box, 0, 0], [0.2 * box, 0.9 * box, 0], [0.1 * box, -0.15 * box, 1.1 * box]])
    pos = g.uniform(0, 1, (n, 3)) @ cell
    q = g.normal(size=n)
    q -= q.mean()
    return pos.astype(dtype), cell.astype(dtype), q.astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_spline_ops_match_oracle(dtype, order):
    from nvalchemiops.spline import spline_gather, spline_gather_vec3, spline_spread

    pos, cell, q = _system(300, dtype, triclinic=True, seed=order)
    dims = (16, 12, 20)
    mesh = spline_spread(_t(pos), _t(q), _t(cell), dims, order)
    omesh = O.spline_spread(pos, q, cell, dims, order)
    _close(mesh, omesh, dtype, "spread")
    assert abs(float(mesh.sum()) - q.sum()) < (1e-9 if dtype == np.float64 else 1e-3)  # charge conservation
    g = np.random.default_rng(1)
    field = g.normal(size=dims).astype(dtype)
    _close(spline_gather(_t(pos), _t(field), _t(cell), order), O.spline_gather(pos, field, cell, order), dtype, "gather")
    vfield = g.normal(size=dims + (3,)).astype(dtype)
    _close(spline_gather_vec3(_t(pos), _t(q), _t(vfield), _t(cell), order), O.spline_gather_vec3(pos, q, vfield, cell, order), dtype,
           "gather_vec3")
    ones = spline_gather(_t(pos), torch.ones(dims, dtype=_t(pos).dtype, device=DEV), _t(cell), order)
    assert float((ones - 1).abs().max()) < (1e-6 if dtype == np.float64 else 1e-5)  # partition of unity (weights <= 1e-8 are dropped)
    # batch kernels (threshold w > 1e-8) on two copies with different cells
    pos2 = np.concatenate([pos, pos * 0.9]).astype(dtype)
    q2 = np.concatenate([q, -q]).astype(dtype)
    cells = np.stack([cell, cell * 0.9]).astype(dtype)
    bi = np.repeat(np.arange(2, dtype=np.int32), len(pos))
    bm = spline_spread(_t(pos2), _t(q2), _t(cells), dims, order, batch_idx=_t(bi))
    _close(bm, O.spline_spread(pos2, q2, cells, dims, order, batch_idx=bi), dtype, "batch spread")


@pytest.mark.parametrize("order", [5, 6])
def test_spline_high_order_properties(order):
    """Orders 5/6: the reference returns zero weights; here they are true B-splines -- checked through
    partition of unity, charge conservation and adjointness (test/test_spline.py:46,179,637)."""
    from nvalchemiops.spline import spline_gather, spline_spread

    pos, cell, q = _system(200, np.float64, seed=3)
    dims = (14, 16, 18)
    mesh = spline_spread(_t(pos), _t(q), _t(cell), dims, order)
    assert abs(float(mesh.sum()) - q.sum()) < 1e-10
    ones = spline_gather(_t(pos), torch.ones(dims, dtype=torch.float64, device=DEV), _t(cell), order)
    assert float((ones - 1).abs().max()) < 1e-6  # weights <= 1e-8 are dropped by the gather (spline.py:608)
    field = torch.randn(dims, dtype=torch.float64, device=DEV)
    assert abs(float((mesh * field).sum() - (_t(q) * spline_gather(_t(pos), field, _t(cell), order)).sum())) < 1e-6  # gather drops w <= 1e-8


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_green_structure_factor_and_corrections(dtype):
    from nvalchemiops.interactions.electrostatics import (generate_k_vectors_pme, pme_energy_corrections_with_charge_grad,
                                                          pme_green_structure_factor)

    pos, cell, q = _system(50, dtype, triclinic=True)
    dims = (12, 10, 16)
    kv, k2 = generate_k_vectors_pme(_t(cell), dims)
    okv, ok2 = O.generate_k_vectors_pme(cell, dims)
    _close(k2, ok2, dtype, "k2")
    alpha = torch.tensor([0.37], dtype=_t(pos).dtype, device=DEV)
    for order in (2, 4):
        g, sf2 = pme_green_structure_factor(k2, dims, alpha, _t(cell), order)
        og, osf2 = O.pme_green_structure_factor(ok2, dims, 0.37, cell, order)
        _close(g, og, dtype, "green")
        _close(sf2, osf2, dtype, "sf2")
    raw = np.random.default_rng(2).normal(size=50).astype(dtype)
    e, cg = pme_energy_corrections_with_charge_grad(_t(raw), _t(q), _t(cell), alpha)
    oe, ocg = O.pme_energy_corrections(raw, q, cell, 0.37, with_charge_grad=True)
    _close(e, oe, dtype, "corrections")
    _close(cg, ocg, dtype, "charge grad")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("fmt", ["matrix", "csr"])
def test_real_space_matches_oracle(dtype, fmt):
    from nvalchemiops.interactions.electrostatics import ewald_real_space
    from nvalchemiops.neighborlist import cell_list

    pos, cell, q = _system(250, dtype, triclinic=True, seed=4)
    pbc = torch.tensor([True] * 3, device=DEV)
    alpha = torch.tensor([0.4], dtype=_t(pos).dtype, device=DEV)
    if fmt == "matrix":
        nm, num, sh = cell_list(_t(pos), 7.0, _t(cell), pbc, max_neighbors=320)
        assert int(num.max()) <= 320
        out = ewald_real_space(_t(pos), _t(q), _t(cell)[None], alpha, neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=250,
                               compute_forces=True, compute_charge_gradients=True)
        ref = O.ewald_real_space(pos, q, cell, 0.4, neighbor_matrix=nm.cpu().numpy(), neighbor_matrix_shifts=sh.cpu().numpy(), mask_value=250,
                                 compute_forces=True, compute_charge_gradients=True)
    else:
        lst, nptr, lsh = cell_list(_t(pos), 7.0, _t(cell), pbc, return_neighbor_list=True)
        out = ewald_real_space(_t(pos), _t(q), _t(cell)[None], alpha, neighbor_list=lst, neighbor_ptr=nptr, neighbor_shifts=lsh,
                               compute_forces=True, compute_charge_gradients=True)
        ref = O.ewald_real_space(pos, q, cell, 0.4, idx_j=lst[1].cpu().numpy(), neighbor_ptr=nptr.cpu().numpy(),
                                 neighbor_shifts=lsh.cpu().numpy(), compute_forces=True, compute_charge_gradients=True)
    for o, r, w in zip(out, ref, ("energies", "forces", "charge_grads")):
        _close(o, r, dtype, w)
    e_only = ewald_real_space(_t(pos), _t(q), _t(cell)[None], alpha, neighbor_matrix=cell_list(_t(pos), 7.0, _t(cell), pbc, max_neighbors=320)[0],
                              neighbor_matrix_shifts=cell_list(_t(pos), 7.0, _t(cell), pbc, max_neighbors=320)[2], mask_value=250)
    _close(e_only, ref[0], dtype, "energies only")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["half", "truncated", "one_sided_csr"])
def test_real_space_on_lists_that_are_not_symmetric(dtype, kind):
    """The reference scatters -f to atom i and +f to atom j (and the charge gradient to both ends) for EVERY stored entry
    (ewald_kernels.py:518-544, :864-873), so half lists, rows truncated by max_neighbors overflow and one-sided lists have a defined
    result; the owner-only fast path is exact for symmetric lists only, the device-side symmetry check must route everything else
    through the scatter fix-up.  Oracle = the restatement, which scatters like the reference."""
    from nvalchemiops.interactions.electrostatics import ewald_real_space
    from nvalchemiops.neighborlist import cell_list

    pos, cell, q = _system(250, dtype, triclinic=True, seed=4)
    pbc = torch.tensor([True] * 3, device=DEV)
    alpha = torch.tensor([0.4], dtype=_t(pos).dtype, device=DEV)
    if kind == "one_sided_csr":
        lst, nptr, lsh = cell_list(_t(pos), 7.0, _t(cell), pbc, return_neighbor_list=True, half_fill=True)
        out = ewald_real_space(_t(pos), _t(q), _t(cell)[None], alpha, neighbor_list=lst, neighbor_ptr=nptr, neighbor_shifts=lsh,
                               compute_forces=True, compute_charge_gradients=True)
        ref = O.ewald_real_space(pos, q, cell, 0.4, idx_j=lst[1].cpu().numpy(), neighbor_ptr=nptr.cpu().numpy(),
                                 neighbor_shifts=lsh.cpu().numpy(), compute_forces=True, compute_charge_gradients=True)
    else:
        kw = dict(half_fill=True, max_neighbors=160) if kind == "half" else dict(max_neighbors=40)  # 40 < fullest row: truncation
        nm, num, sh = cell_list(_t(pos), 7.0, _t(cell), pbc, **kw)
        if kind == "truncated":
            assert int(num.max()) > 40
        out = ewald_real_space(_t(pos), _t(q), _t(cell)[None], alpha, neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=250,
                               compute_forces=True, compute_charge_gradients=True)
        ref = O.ewald_real_space(pos, q, cell, 0.4, neighbor_matrix=nm.cpu().numpy(), neighbor_matrix_shifts=sh.cpu().numpy(), mask_value=250,
                                 compute_forces=True, compute_charge_gradients=True)
    for o, r, w in zip(out, ref, ("energies", "forces", "charge_grads")):
        _close(o, r, dtype, w, scale=np.abs(r).max() * (10 if dtype == np.float32 else 1))
    # Newton's third law holds entry by entry whatever the list
    assert float(out[1].sum(0).abs().max()) <= (1e-10 if dtype == np.float64 else 2e-4) * float(out[1].abs().max()) * 16


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("order", [2, 3, 4])
def test_pme_reciprocal_matches_oracle(dtype, order):
    from nvalchemiops.interactions.electrostatics import generate_k_vectors_pme, pme_reciprocal_space

    pos, cell, q = _system(200, dtype, triclinic=True, seed=order)
    dims = (24, 20, 28)
    ref = O.pme_reciprocal_space(pos, q, cell, 0.35, dims, order, compute_forces=True, compute_charge_gradients=True)
    out = pme_reciprocal_space(_t(pos), _t(q), _t(cell), 0.35, mesh_dimensions=dims, spline_order=order, compute_forces=True,
                               compute_charge_gradients=True)
    for o, r, w in zip(out, ref, ("energies", "forces", "charge_grads")):
        _close(o, r, dtype, w)
    # caller-supplied k arrays take the unfused composition (pme.py:1338-1479) and must agree
    kv, k2 = generate_k_vectors_pme(_t(cell), dims)
    out2 = pme_reciprocal_space(_t(pos), _t(q), _t(cell), 0.35, mesh_dimensions=dims, spline_order=order, compute_forces=True,
                                k_vectors=kv, k_squared=k2)
    _close(out2[0], ref[0], dtype, "energies (k arrays)")
    _close(out2[1], ref[1], dtype, "forces (k arrays)")
    e_only = pme_reciprocal_space(_t(pos), _t(q), _t(cell), 0.35, mesh_dimensions=dims, spline_order=order)
    _close(e_only, ref[0], dtype, "energies only")


def test_caller_supplied_k_arrays_are_shape_checked():
    """The fused k-space pass reads caller-supplied k arrays through raw pointers ([nx, ny, nz/2+1(, 3)], optionally with a leading batch
    dimension): anything else must raise before the launch instead of mis-indexing on the device (round-2 ADVICE)."""
    from nvalchemiops.interactions.electrostatics import generate_k_vectors_pme, pme_reciprocal_space

    pos, cell, q = _system(64, np.float64, seed=3)
    dims = (12, 10, 14)
    kv, k2 = generate_k_vectors_pme(_t(cell), dims)
    kw = dict(mesh_dimensions=dims, spline_order=4, compute_forces=True)
    ok = pme_reciprocal_space(_t(pos), _t(q), _t(cell), 0.4, k_vectors=kv, k_squared=k2, **kw)
    assert torch.isfinite(ok[0]).all()
    full = torch.zeros(dims, dtype=torch.float64, device=DEV)  # the full-FFT grid instead of the rfft half grid
    with pytest.raises(ValueError, match="k_squared must have shape"):
        pme_reciprocal_space(_t(pos), _t(q), _t(cell), 0.4, k_vectors=kv, k_squared=full, **kw)
    with pytest.raises(ValueError, match="k_vectors must have shape"):
        pme_reciprocal_space(_t(pos), _t(q), _t(cell), 0.4, k_vectors=kv[..., :2], k_squared=k2, **kw)
    with pytest.raises(ValueError, match="k_squared must have shape"):
        pme_reciprocal_space(_t(pos), _t(q), _t(cell), 0.4, k_vectors=kv, k_squared=k2.unsqueeze(0).expand(3, -1, -1, -1).contiguous(), **kw)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pme_batch_matches_oracle_and_single(dtype):
    from nvalchemiops.interactions.electrostatics import particle_mesh_ewald
    from nvalchemiops.neighborlist import batch_cell_list

    parts = [_system(n, dtype, triclinic=(s == 1), seed=10 + s, box=10.0 + s) for s, n in enumerate((120, 80, 150))]
    pos = np.concatenate([p[0] for p in parts])
    q = np.concatenate([p[2] for p in parts])
    cells = np.stack([p[1] for p in parts])
    bi = np.concatenate([np.full(len(p[0]), s, np.int32) for s, p in enumerate(parts)])
    alpha = np.array([0.4, 0.42, 0.38], dtype)
    dims = (20, 20, 20)
    nm, num, sh = batch_cell_list(_t(pos), 6.5, _t(cells), torch.ones((3, 3), dtype=torch.bool, device=DEV), _t(bi), max_neighbors=256)
    assert int(num.max()) <= 256
    out = particle_mesh_ewald(_t(pos), _t(q), _t(cells), alpha=_t(alpha), mesh_dimensions=dims, spline_order=4, batch_idx=_t(bi),
                              neighbor_matrix=nm, neighbor_matrix_shifts=sh, compute_forces=True)
    ref = O.particle_mesh_ewald(pos, q, cells, alpha, dims, 4, batch_idx=bi, neighbor_matrix=nm.cpu().numpy(),
                                neighbor_matrix_shifts=sh.cpu().numpy(), compute_forces=True)
    _close(out[0], ref[0], dtype, "batch energies")
    _close(out[1], ref[1], dtype, "batch forces")


def test_pme_madelung_and_explicit_ewald():
    """External anchors (the reference holds no PME numbers): NaCl Madelung constant 1.747565 and an independent
    structure-factor Ewald sum; order 5 (true B-spline here) must beat order 4 at fixed mesh."""
    from nvalchemiops.interactions.electrostatics import particle_mesh_ewald
    from nvalchemiops.neighborlist import cell_list

    a = 5.64
    base = np.array([[0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5], [.5, 0, 0], [0, .5, 0], [0, 0, .5], [.5, .5, .5]]) * a
    q = np.array([1, 1, 1, 1, -1, -1, -1, -1.0])
    cell = np.eye(3) * a
    pbc = torch.tensor([True] * 3, device=DEV)
    nm, num, sh = cell_list(_t(base), 9.0, _t(cell), pbc, max_neighbors=160)
    e, f = particle_mesh_ewald(_t(base), _t(q), _t(cell), alpha=0.45, mesh_dimensions=(32, 32, 32), spline_order=4, neighbor_matrix=nm,
                               neighbor_matrix_shifts=sh, compute_forces=True)
    assert abs(-float(e.sum()) / 4 * (a / 2) - 1.747565) < 1e-5
    assert float(f.abs().max()) < 1e-9
    pos, cell, q = _system(40, np.float64, triclinic=True, seed=0, box=10.0)
    ee, fe = O.explicit_ewald(pos, q, cell, 0.4, kmax=9)
    lst, nptr, lsh = cell_list(_t(pos), 11.0, _t(cell), pbc, return_neighbor_list=True)
    errs = {}
    for order in (4, 5, 6):
        e, f = particle_mesh_ewald(_t(pos), _t(q), _t(cell), alpha=0.4, mesh_dimensions=(24, 24, 24), spline_order=order,
                                   neighbor_list=lst, neighbor_ptr=nptr, neighbor_shifts=lsh, compute_forces=True)
        errs[order] = (abs(float(e.sum()) - ee), float(np.abs(f.cpu().numpy() - fe).max()))
    assert errs[4][0] < 2e-3 and errs[5][0] < errs[4][0] and errs[6][0] < errs[4][0], errs
    assert errs[5][1] < errs[4][1], errs


def test_config4_100k_fp64_properties():
    """BASELINE config 4 (100k-atom periodic box with charges, nlist + PME, fp64): size-independent properties --
    zero net reciprocal force (to mesh accuracy), real-space Newton's third law, translation invariance under a lattice
    vector; the 4k-atom version AND the full 100k-atom configuration (mesh 128^3, order 4) are compared with the oracle."""
    from nvalchemiops.interactions.electrostatics import particle_mesh_ewald
    from nvalchemiops.neighborlist import cell_list

    pbc = torch.tensor([True] * 3, device=DEV)
    pos, cell, q, _ = S.fcc_box(4000, dtype=np.float64)
    nm, num, sh = cell_list(_t(pos), 9.0, _t(cell), pbc, max_neighbors=256)
    out = particle_mesh_ewald(_t(pos), _t(q), _t(cell), alpha=0.35, mesh_dimensions=(48, 48, 48), spline_order=4, neighbor_matrix=nm,
                              neighbor_matrix_shifts=sh, compute_forces=True)
    ref = O.particle_mesh_ewald(pos, q, cell, 0.35, (48, 48, 48), 4, neighbor_matrix=nm.cpu().numpy(), neighbor_matrix_shifts=sh.cpu().numpy(),
                                compute_forces=True)
    _close(out[0], ref[0], np.float64, "4k energies")
    _close(out[1], ref[1], np.float64, "4k forces")
    pos, cell, q, _ = S.fcc_box(100000, dtype=np.float64)
    tp, tc, tq = _t(pos), _t(cell), _t(q)
    nm, num, sh = cell_list(tp, 9.0, tc, pbc, max_neighbors=256)
    assert int(num.max()) <= 256
    e, f = particle_mesh_ewald(tp, tq, tc, alpha=0.35, mesh_dimensions=(128, 128, 128), spline_order=4, neighbor_matrix=nm,
                               neighbor_matrix_shifts=sh, compute_forces=True)
    assert torch.isfinite(e).all() and torch.isfinite(f).all()
    assert float(f.sum(0).abs().max()) < 1e-3 * float(f.abs().max()) * 100
    # the FULL-size configuration against the oracle as well (5 s of oracle time on the device-built list): same tolerances as the small cases
    ref = O.particle_mesh_ewald(pos, q, cell, 0.35, (128, 128, 128), 4, neighbor_matrix=nm.cpu().numpy(), neighbor_matrix_shifts=sh.cpu().numpy(),
                                mask_value=100000, compute_forces=True)
    _close(e, ref[0], np.float64, "100k energies")
    _close(f, ref[1], np.float64, "100k forces")
    shift = tc[0] * 1.0  # translate every atom by one lattice vector: same energies (atoms leave the box -> wrap bookkeeping)
    nm2, num2, sh2 = cell_list(tp + shift, 9.0, tc, pbc, max_neighbors=256)
    e2, f2 = particle_mesh_ewald(tp + shift, tq, tc, alpha=0.35, mesh_dimensions=(128, 128, 128), spline_order=4, neighbor_matrix=nm2,
                                 neighbor_matrix_shifts=sh2, compute_forces=True)
    assert torch.equal(num, num2)
    assert float((e - e2).abs().max()) < 1e-9 * float(e.abs().max()) * 10
    assert float((f - f2).abs().max()) < 1e-8 * float(f.abs().max()) * 10


def test_pme_is_equivariant_under_a_permutation_of_the_atoms():
    """The gather epilogue walks the atoms tile by tile when the caller's atom order is not spatially coherent (the tile-owned spread of
    the same call measures that and leaves the tile-grouped ids behind, csrc/pme.hip): a randomly permuted 20k-atom box gives the permuted
    energies / forces / charge gradients of the lattice-ordered one (fp64: the mesh sums differ only in the order of the tile kernel's
    LDS atomics)."""
    from nvalchemiops.interactions.electrostatics import particle_mesh_ewald
    from nvalchemiops.neighborlist import cell_list

    pbc = torch.tensor([True] * 3, device=DEV)
    n = 20000
    pos, cell, q, _ = S.fcc_box(n, dtype=np.float64)
    perm = np.random.default_rng(11).permutation(n)

    def run(pos_, q_):
        nm, num, sh = cell_list(_t(pos_), 9.0, _t(cell), pbc, max_neighbors=256)
        return particle_mesh_ewald(_t(pos_), _t(q_), _t(cell), alpha=0.35, mesh_dimensions=(64, 64, 64), spline_order=5, neighbor_matrix=nm,
                                   neighbor_matrix_shifts=sh, compute_forces=True, compute_charge_gradients=True)

    a, b = run(pos, q), run(pos[perm], q[perm])
    for x, y, what in zip(a, b, ("energies", "forces", "charge gradients")):
        x = x.cpu().numpy()[perm]
        y = y.cpu().numpy()
        assert np.abs(x - y).max() < 1e-10 * max(1.0, np.abs(x).max()), what


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("order", [5, 6])
def test_orders_5_6_vs_extended_oracle(dtype, order):
    """Orders 5/6 against the oracle's extended mode (closed-form truncated-power B-splines, structure-factor exponent = order;
    pinned on Madelung + explicit Ewald in tests/test_oracle_golden.py): spread mesh, gathers, full PME, single + batch, triclinic."""
    from nvalchemiops.interactions.electrostatics import particle_mesh_ewald
    from nvalchemiops.neighborlist import cell_list
    from nvalchemiops.spline import spline_gather, spline_spread

    pbc = torch.tensor([True] * 3, device=DEV)
    pos, cell, q = _system(300, dtype, triclinic=True, seed=3, box=14.0)
    dims = (16, 20, 24)
    with O.extended_splines():
        ref_mesh = O.spline_spread(pos, q, cell, dims, order)
        field = np.random.default_rng(1).normal(size=dims).astype(dtype)
        ref_g = O.spline_gather(pos, field, cell, order)
    _close(spline_spread(_t(pos), _t(q), _t(cell), dims, order), ref_mesh, dtype, "spread")
    _close(spline_gather(_t(pos), _t(field), _t(cell), order), ref_g, dtype, "gather")
    nm, num, sh = cell_list(_t(pos), 6.0, _t(cell), pbc, max_neighbors=160)
    assert int(num.max()) <= 160
    e, f = particle_mesh_ewald(_t(pos), _t(q), _t(cell), alpha=0.4, mesh_dimensions=dims, spline_order=order, neighbor_matrix=nm,
                               neighbor_matrix_shifts=sh, compute_forces=True)
    with O.extended_splines():
        ref = O.particle_mesh_ewald(pos, q, cell, 0.4, dims, order, neighbor_matrix=nm.cpu().numpy(), neighbor_matrix_shifts=sh.cpu().numpy(),
                                    mask_value=len(pos), compute_forces=True)
    _close(e, ref[0], dtype, "energies")
    _close(f, ref[1], dtype, "forces")


def test_headline_pme_order5_100k_vs_extended_oracle():
    """The configuration bench.py times (100k atoms, fp64, 9 A list M = 256, alpha 0.35, mesh 128^3, spline ORDER 5, E + F) against
    the extended oracle at full size -- the 125-point-stencil tile path of the headline number."""
    from nvalchemiops.interactions.electrostatics import particle_mesh_ewald
    from nvalchemiops.neighborlist import cell_list

    pbc = torch.tensor([True] * 3, device=DEV)
    pos, cell, q, _ = S.fcc_box(100000, dtype=np.float64)
    tp, tc, tq = _t(pos), _t(cell), _t(q)
    nm, num, sh = cell_list(tp, 9.0, tc, pbc, max_neighbors=256)
    assert int(num.max()) <= 256
    e, f = particle_mesh_ewald(tp, tq, tc, alpha=0.35, mesh_dimensions=(128, 128, 128), spline_order=5, neighbor_matrix=nm,
                               neighbor_matrix_shifts=sh, compute_forces=True)
    with O.extended_splines():
        ref = O.particle_mesh_ewald(pos, q, cell, 0.35, (128, 128, 128), 5, neighbor_matrix=nm.cpu().numpy(), neighbor_matrix_shifts=sh.cpu().numpy(),
                                    mask_value=100000, compute_forces=True)
    _close(e, ref[0], np.float64, "100k order-5 energies")
    _close(f, ref[1], np.float64, "100k order-5 forces")
    # and order 5 is closer to order 6 than order 4 is (convergence with the spline order on the same mesh)
    e4 = particle_mesh_ewald(tp, tq, tc, alpha=0.35, mesh_dimensions=(128, 128, 128), spline_order=4, neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    e6 = particle_mesh_ewald(tp, tq, tc, alpha=0.35, mesh_dimensions=(128, 128, 128), spline_order=6, neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    assert float((e.sum() - e6.sum()).abs()) < float((e4.sum() - e6.sum()).abs())


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("order", [5, 6])
def test_reference_spline_orders_switch_vs_default_oracle(dtype, order):
    """`reference_spline_orders()`: orders 5 / 6 evaluated as the REFERENCE evaluates them -- weights identically zero
    (spline.py:150-193 has cases for orders 1-4 only), structure-factor exponent min(order, 4) (pme_kernels.py:213-225) -- against the
    oracle's DEFAULT mode, which restates exactly that.  Spread, gathers, Green function / structure factor, reciprocal part and the
    full PME (energies, forces, charge gradients; single + batch; the fused path and the custom-op composition)."""
    from nvalchemiops.interactions.electrostatics import particle_mesh_ewald, pme_reciprocal_space
    from nvalchemiops.interactions.electrostatics.k_vectors import generate_k_vectors_pme
    from nvalchemiops.interactions.electrostatics.pme import pme_green_structure_factor
    from nvalchemiops.neighborlist import cell_list
    from nvalchemiops.spline import reference_spline_orders, spline_gather, spline_gather_vec3, spline_spread

    pbc = torch.tensor([True] * 3, device=DEV)
    pos, cell, q = _system(300, dtype, triclinic=True, seed=3, box=14.0)
    dims = (16, 20, 24)
    tp, tq, tc = _t(pos), _t(q), _t(cell)
    field = np.random.default_rng(1).normal(size=dims).astype(dtype)
    vec = np.random.default_rng(2).normal(size=dims + (3,)).astype(dtype)
    nm, num, sh = cell_list(tp, 6.0, tc, pbc, max_neighbors=160)
    kw = dict(alpha=0.4, mesh_dimensions=dims, spline_order=order, neighbor_matrix=nm, neighbor_matrix_shifts=sh, compute_forces=True,
              compute_charge_gradients=True)
    true_e = particle_mesh_ewald(tp, tq, tc, **kw)[0]
    with reference_spline_orders():
        mesh = spline_spread(tp, tq, tc, dims, order)
        g = spline_gather(tp, _t(field), tc, order)
        g3 = spline_gather_vec3(tp, tq, _t(vec), tc, order)
        kv, k2 = generate_k_vectors_pme(tc, dims)
        green, sf2 = pme_green_structure_factor(k2, dims, torch.tensor([0.4], dtype=tp.dtype, device=DEV), tc, spline_order=order)
        e, f, cg = particle_mesh_ewald(tp, tq, tc, **kw)
        er, fr = pme_reciprocal_space(tp, tq, tc, alpha=0.4, mesh_dimensions=dims, spline_order=order, compute_forces=True)
        tp_g = tp.clone().requires_grad_(True)  # an input that requires grad takes the custom-op composition: same numbers
        eg, fg, cgg = particle_mesh_ewald(tp_g, tq, tc, **kw)
        e4 = particle_mesh_ewald(tp, tq, tc, **dict(kw, spline_order=4))[0]
    assert float(mesh.abs().max()) == 0.0 and float(g.abs().max()) == 0.0 and float(g3.abs().max()) == 0.0 and float(fr.abs().max()) == 0.0
    ref_mesh = O.spline_spread(pos, q, cell, dims, order)  # the oracle's default mode IS the reference's evaluation
    assert np.abs(ref_mesh).max() == 0.0
    ref_green, ref_sf2 = O.pme_green_structure_factor(k2.cpu().numpy(), dims, np.array([0.4]), cell, order)
    _close(green, ref_green.reshape(green.shape), dtype, "green")
    _close(sf2, ref_sf2.reshape(sf2.shape), dtype, "sf^2 with the exponent capped at 4")
    ref = O.particle_mesh_ewald(pos, q, cell, 0.4, dims, order, neighbor_matrix=nm.cpu().numpy(), neighbor_matrix_shifts=sh.cpu().numpy(),
                                mask_value=len(pos), compute_forces=True, compute_charge_gradients=True)
    for got, want, what in ((e, ref[0], "energies"), (f, ref[1], "forces"), (cg, ref[2], "charge gradients"), (eg, ref[0], "energies (ops)"),
                            (fg, ref[1], "forces (ops)"), (cgg, ref[2], "charge gradients (ops)")):
        _close(got.detach(), want, dtype, what)
    ref_r = O.pme_reciprocal_space(pos, q, cell, 0.4, dims, order)
    _close(er, ref_r, dtype, "reciprocal part = the corrections alone")
    # the switch changes orders 5 / 6 only, and only while it is on (allclose, not equal: the tile-owned spread adds in LDS-atomic order)
    eps = 1e-12 if dtype == np.float64 else 1e-5
    assert torch.allclose(e4, particle_mesh_ewald(tp, tq, tc, **dict(kw, spline_order=4))[0], rtol=eps, atol=eps)
    assert torch.allclose(true_e, particle_mesh_ewald(tp, tq, tc, **kw)[0], rtol=eps, atol=eps) and float((true_e - e).abs().max()) > 1e-3
    # batch of two systems through the batch kernels
    p2, c2, q2 = _system(200, dtype, seed=4, box=12.0)
    bp, bq, bc = _t(np.concatenate([pos, p2])), _t(np.concatenate([q, q2])), _t(np.stack([cell, c2]))
    bi = torch.tensor([0] * 300 + [1] * 200, dtype=torch.int32, device=DEV)
    from nvalchemiops.neighborlist import batch_cell_list

    bnm, bnum, bsh = batch_cell_list(bp, 6.0, bc, torch.ones((2, 3), dtype=torch.bool, device=DEV), bi, max_neighbors=160)
    with reference_spline_orders():
        be, bf = particle_mesh_ewald(bp, bq, bc, alpha=0.4, mesh_dimensions=dims, spline_order=order, batch_idx=bi, neighbor_matrix=bnm,
                                     neighbor_matrix_shifts=bsh, compute_forces=True)
    bref = O.particle_mesh_ewald(np.concatenate([pos, p2]), np.concatenate([q, q2]), np.stack([cell, c2]), 0.4, dims, order,
                                 batch_idx=bi.cpu().numpy(), neighbor_matrix=bnm.cpu().numpy(), neighbor_matrix_shifts=bsh.cpu().numpy(),
                                 mask_value=500, compute_forces=True)
    _close(be, bref[0], dtype, "batch energies")
    _close(bf, bref[1], dtype, "batch forces")


@pytest.mark.parametrize("order", [5, 6])
@pytest.mark.parametrize("where", ["inside", "outside"])
def test_backward_keeps_the_spline_evaluation_of_its_forward(order, where):
    """`reference_spline_orders()` is a context variable of the CALLING thread, and the autograd engine runs the backward of
    device tensors on its own worker thread, where that context does not exist.  The switch is therefore read once, in the forward, and
    travels with the order value into every saved context: a forward evaluated the reference way (zero mesh for orders 5 / 6: the
    reciprocal energies are the self / background corrections, which do not depend on the positions) has a ZERO position gradient --
    whether `backward()` runs inside the `with` block or after it -- and equals -forces of the same call; a forward evaluated with the
    true B-splines keeps them in its backward even when that runs inside a `with reference_spline_orders()` block entered later."""
    from nvalchemiops.interactions.electrostatics import pme_reciprocal_space
    from nvalchemiops.spline import reference_spline_orders, spline_gather, spline_spread

    dtype = np.float64
    pos, cell, q = _system(300, dtype, triclinic=True, seed=5, box=14.0)
    dims = (16, 20, 24)
    tq, tc = _t(q), _t(cell)
    field = _t(np.random.default_rng(1).normal(size=dims).astype(dtype))

    def grads(enter_for_forward, enter_for_backward):
        tp = _t(pos).requires_grad_(True)
        tv = _t(q).requires_grad_(True)
        ctx_f = reference_spline_orders() if enter_for_forward else reference_spline_orders(False)
        ctx_b = reference_spline_orders() if enter_for_backward else reference_spline_orders(False)
        with ctx_f:
            e = pme_reciprocal_space(tp, tv, tc, alpha=0.4, mesh_dimensions=dims, spline_order=order)
            g = spline_gather(tp, field, tc, order)
            m = spline_spread(tp, tv, tc, dims, order)
            loss = e.sum() + (g * g).sum() + (m * field).sum()
            if where == "inside":
                loss.backward()
        if where == "outside":
            with ctx_b:
                loss.backward()
        return tp.grad.clone(), tv.grad.clone(), e.detach()

    # forward the reference way: nothing depends on the positions through the mesh, whatever the backward's surroundings say
    gp, gq, e_ref = grads(True, False)
    assert float(gp.abs().max()) == 0.0
    # forward with the true splines: the gradient is that of the true splines, even if the backward runs inside a reference block
    gp_t, gq_t, e_true = grads(False, True)
    gp_t2, gq_t2, _ = grads(False, False)
    assert float(gp_t.abs().max()) > 1e-3 and torch.allclose(gp_t, gp_t2, rtol=1e-12, atol=1e-12) and torch.allclose(gq_t, gq_t2, rtol=1e-12, atol=1e-12)
    assert float((e_true - e_ref).abs().max()) > 1e-3


# ---- explicit-k Ewald ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("triclinic", [False, True])
def test_ewald_reciprocal_space_vs_oracle(dtype, triclinic):
    from nvalchemiops.interactions.electrostatics import ewald_reciprocal_space, generate_k_vectors_ewald_summation

    pos, cell, q = _system(150, dtype, triclinic, seed=4)
    q[0] += 0.7  # net charge: exercises the background term
    alpha = 0.4
    kv = generate_k_vectors_ewald_summation(_t(cell), 3.0)
    okv = O.generate_k_vectors_ewald_summation(cell, 3.0)
    np.testing.assert_allclose(kv.cpu().numpy(), okv, rtol=0, atol=1e-5 if dtype == np.float32 else 1e-13)
    al = torch.tensor([alpha], dtype=_t(pos).dtype, device=DEV)
    e, f, cg = ewald_reciprocal_space(_t(pos), _t(q), _t(cell), kv, al, compute_forces=True, compute_charge_gradients=True)
    assert e.dtype == _t(pos).dtype and f.shape == (150, 3)
    # oracle on the inputs the kernel sees (k-vectors in the input dtype, float64 arithmetic)
    oe, of, ocg = O.ewald_reciprocal_space(pos, q, cell, kv.cpu().numpy(), alpha)
    _close(e, oe, dtype, "energies")
    _close(f, of, dtype, "forces")
    _close(cg, ocg, dtype, "charge gradients")
    e_only = ewald_reciprocal_space(_t(pos), _t(q), _t(cell), kv, al)
    assert torch.equal(e_only, e)
    e2, cg2 = ewald_reciprocal_space(_t(pos), _t(q), _t(cell), kv, al, compute_charge_gradients=True)
    assert torch.equal(cg2, cg)


def test_ewald_reciprocal_space_batch_and_summation():
    from nvalchemiops.interactions.electrostatics import ewald_reciprocal_space, ewald_summation, generate_k_vectors_ewald_summation
    from nvalchemiops.neighborlist import neighbor_list

    pa, ca, qa = _system(90, np.float64, True, seed=1, box=11.0)
    pb, cb, qb = _system(5000, np.float64, False, seed=2, box=30.0)   # > one 4096-atom chunk: atomics across chunks
    pos, q = np.concatenate([pa, pb]), np.concatenate([qa, qb])
    cells = np.stack([ca, cb])
    bi = torch.tensor([0] * 90 + [1] * 5000, dtype=torch.int32, device=DEV)
    alpha = torch.tensor([0.4, 0.3], dtype=torch.float64, device=DEV)
    kv = generate_k_vectors_ewald_summation(_t(cells), 1.6)
    assert kv.dim() == 3 and kv.shape[0] == 2
    e, f = ewald_reciprocal_space(_t(pos), _t(q), _t(cells), kv, alpha, batch_idx=bi, compute_forces=True)
    kvn = kv.cpu().numpy()
    ea, fa, _ = O.ewald_reciprocal_space(pa, qa, ca, kvn[0], 0.4)
    eb, fb, _ = O.ewald_reciprocal_space(pb, qb, cb, kvn[1], 0.3)
    _close(e, np.concatenate([ea, eb]), np.float64, "batch energies")
    _close(f, np.concatenate([fa, fb]), np.float64, "batch forces")
    # full Ewald sum (automatic alpha / k-cutoff) against the independent explicit sum
    pos, cell, q = _system(60, np.float64, True, seed=9, box=10.0)
    tp, tc, tq = _t(pos), _t(cell), _t(q)
    from nvalchemiops.interactions.electrostatics import estimate_ewald_parameters
    prm = estimate_ewald_parameters(tp, tc.unsqueeze(0), accuracy=1e-7)
    nm, num, sh = neighbor_list(tp, float(prm.real_space_cutoff), cell=tc, pbc=torch.tensor([True] * 3, device=DEV), method="cell_list",
                                max_neighbors=700)
    assert int(num.max()) < 700
    e, f = ewald_summation(tp, tq, tc, neighbor_matrix=nm, neighbor_matrix_shifts=sh, compute_forces=True, accuracy=1e-7)
    ee, fe = O.explicit_ewald(pos, q, cell, float(prm.alpha), kmax=10, exact_erfc=False)
    assert abs(e.sum().item() - ee) < 2e-6 * abs(ee) + 2e-6
    np.testing.assert_allclose(f.cpu().numpy(), fe, atol=3e-5)


def test_ewald_reciprocal_space_autograd():
    """dL/dr and dL/dq of L = sum_i g_i E_i through the hand-written adjoint vs central differences of the HIP forward."""
    from nvalchemiops.interactions.electrostatics import ewald_reciprocal_space, generate_k_vectors_ewald_summation

    pos, cell, q = _system(40, np.float64, True, seed=6, box=9.0)
    q[3] += 0.5
    tc = _t(cell)
    kv = generate_k_vectors_ewald_summation(tc, 2.5)
    al = torch.tensor([0.45], dtype=torch.float64, device=DEV)
    g = torch.linspace(0.5, 1.5, 40, dtype=torch.float64, device=DEV)
    tp, tq = _t(pos).requires_grad_(True), _t(q).requires_grad_(True)
    e, f = ewald_reciprocal_space(tp, tq, tc, kv, al, compute_forces=True)
    (e * g).sum().backward()
    # unweighted: -dE/dr equals the explicit forces
    tp2 = _t(pos).requires_grad_(True)
    ewald_reciprocal_space(tp2, _t(q), tc, kv, al).sum().backward()
    np.testing.assert_allclose(-tp2.grad.cpu().numpy(), f.detach().cpu().numpy(), atol=1e-10)

    def loss(p_, q_):
        return float((ewald_reciprocal_space(_t(p_), _t(q_), tc, kv, al) * g).sum())

    h = 1e-5
    for i, d in ((0, 0), (17, 2), (39, 1)):
        pp, pm = pos.copy(), pos.copy()
        pp[i, d] += h
        pm[i, d] -= h
        assert abs((loss(pp, q) - loss(pm, q)) / (2 * h) - tp.grad[i, d].item()) < 1e-7
    for i in (3, 20):
        qp, qm = q.copy(), q.copy()
        qp[i] += h
        qm[i] -= h
        assert abs((loss(pos, qp) - loss(pos, qm)) / (2 * h) - tq.grad[i].item()) < 1e-7


@pytest.mark.parametrize("batched", [False, True])
def test_ewald_reciprocal_space_cell_alpha_kvector_gradients(batched):
    """Cell (through k_vectors and the volume), alpha and raw k-vector gradients of L = sum_i g_i E_i against central differences of
    the HIP forward -- the gradient the reference's test_ewald.py:2117 (`test_cell_gradients`) asks for."""
    from nvalchemiops.interactions.electrostatics import ewald_reciprocal_space, generate_k_vectors_ewald_summation

    p0, c0, q0 = _system(30, np.float64, True, seed=16, box=9.0)
    q0[2] += 0.7  # net charge: the background term depends on alpha and V
    if batched:
        p1, c1, q1 = _system(22, np.float64, False, seed=17, box=8.0)
        pos, q, cells = np.concatenate([p0, p1]), np.concatenate([q0, q1]), np.stack([c0, c1])
        bi = _t(np.concatenate([np.zeros(30, np.int32), np.ones(22, np.int32)]))
        alpha0 = np.array([0.45, 0.5])
    else:
        pos, q, cells, bi, alpha0 = p0, q0, c0[None], None, np.array([0.45])
    n = pos.shape[0]
    g = torch.linspace(0.5, 1.5, n, dtype=torch.float64, device=DEV)
    tp, tq = _t(pos), _t(q)

    def loss(cell_t, alpha_t, kv=None):
        kv = generate_k_vectors_ewald_summation(cell_t, 2.2) if kv is None else kv
        return (ewald_reciprocal_space(tp, tq, cell_t, kv, alpha_t, batch_idx=bi) * g).sum()

    tc, ta = _t(cells).requires_grad_(True), _t(alpha0).requires_grad_(True)
    loss(tc, ta).backward()
    assert tc.grad is not None and torch.isfinite(tc.grad).all()
    h = 1e-5
    with torch.no_grad():
        for s in range(cells.shape[0]):
            for a, b in ((0, 0), (1, 0), (2, 1), (1, 2), (2, 2)):
                d = torch.zeros_like(tc); d[s, a, b] = h
                fd = float(loss(tc + d, ta) - loss(tc - d, ta)) / (2 * h)
                assert abs(fd - float(tc.grad[s, a, b])) < 2e-7 * max(1.0, abs(fd)), ("cell", s, a, b, fd, float(tc.grad[s, a, b]))
            d = torch.zeros_like(ta); d[s] = h
            fd = float(loss(tc, ta + d) - loss(tc, ta - d)) / (2 * h)
            assert abs(fd - float(ta.grad[s])) < 2e-7 * max(1.0, abs(fd)), ("alpha", s, fd, float(ta.grad[s]))
    # k-vectors as an independent leaf (cell fixed)
    kv = generate_k_vectors_ewald_summation(_t(cells), 2.2).detach().requires_grad_(True)
    loss(_t(cells), _t(alpha0), kv).backward()
    k2 = (kv.detach() ** 2).sum(-1).reshape(-1)
    flat = kv.grad.reshape(-1, 3)
    with torch.no_grad():
        for idx in torch.argsort(k2)[:4].tolist() + [int(k2.numel() // 2)]:
            for c in range(3):
                d = torch.zeros_like(kv); d.reshape(-1, 3)[idx, c] = h
                fd = float(loss(_t(cells), _t(alpha0), kv + d) - loss(_t(cells), _t(alpha0), kv - d)) / (2 * h)
                assert abs(fd - float(flat[idx, c])) < 2e-7 * max(1.0, abs(fd)), ("k", idx, c, fd, float(flat[idx, c]))


def test_out_of_range_indices_are_padding():
    """The reference's `test_default_mask_value_pme` (test_pme.py:2201) pads a neighbour matrix with -1 while mask_value defaults
    to N: the reference reads positions[-1]; here any index outside [0, N) is padding, so the result equals the N-padded matrix."""
    from nvalchemiops.interactions.electrostatics import ewald_real_space, particle_mesh_ewald

    g = np.random.default_rng(3)
    pos, q = _t(g.uniform(0, 10, (5, 3))), _t(g.normal(size=5))
    cell = torch.eye(3, dtype=torch.float64, device=DEV) * 10
    nm_neg = torch.tensor([[1, -1], [0, 2], [1, 3], [2, 4], [3, -1]], dtype=torch.int32, device=DEV)
    nm_pad = torch.where(nm_neg < 0, torch.full_like(nm_neg, 5), nm_neg)
    sh = torch.zeros((5, 2, 3), dtype=torch.int32, device=DEV)
    kw = dict(alpha=0.3, mesh_dimensions=(16, 16, 16), neighbor_matrix_shifts=sh, compute_forces=True)
    e, f = particle_mesh_ewald(pos, q, cell, neighbor_matrix=nm_neg, **kw)
    e2, f2 = particle_mesh_ewald(pos, q, cell, neighbor_matrix=nm_pad, **kw)
    assert e.shape == (5,) and f.shape == (5, 3) and torch.isfinite(e).all() and torch.isfinite(f).all()
    assert torch.equal(e, e2) and torch.equal(f, f2)
    al = torch.tensor([0.3], dtype=torch.float64, device=DEV)
    huge = torch.tensor([[1, 7], [0, 2], [1, 3], [2, 4], [3, 1 << 30]], dtype=torch.int32, device=DEV)
    assert torch.equal(ewald_real_space(pos, q, cell, al, neighbor_matrix=huge, neighbor_matrix_shifts=sh, mask_value=5),
                       ewald_real_space(pos, q, cell, al, neighbor_matrix=nm_pad, neighbor_matrix_shifts=sh, mask_value=5))


def test_spline_gather_gradient_and_channels():
    """`spline_gather_gradient` (spline.py:2733) against central differences of `spline_gather` and its uniform-mesh zero
    (test_spline.py:385); the multi-channel wrappers (:2788, :2863) against the scalar ops; one 2-D cell shared by a batch
    (test_spline.py:1768-1960)."""
    from nvalchemiops.spline import (spline_gather, spline_gather_channels, spline_gather_gradient, spline_spread, spline_spread_channels)

    pos, cell, q = _system(40, np.float64, True, seed=21, box=9.0)
    tp, tq, tc = _t(pos), _t(q), _t(cell)
    g = np.random.default_rng(5)
    dims = (12, 10, 14)
    mesh = _t(g.normal(size=dims))
    f = spline_gather_gradient(tp, tq, mesh, tc, spline_order=4)
    assert f.shape == (40, 3)
    h = 1e-5
    for d in range(3):
        dp = torch.zeros_like(tp); dp[:, d] = h
        fd = (spline_gather(tp + dp, mesh, tc, 4) - spline_gather(tp - dp, mesh, tc, 4)) / (2 * h)
        # the gather drops weights <= 1e-8 (spline.py:608) and the cubic spline's third derivative jumps at the knots: FD noise ~1e-6
        assert float((f[:, d] + tq * fd).abs().max()) < 5e-6 * max(1.0, float(f.abs().max()))
    assert float(spline_gather_gradient(tp, tq, torch.ones(dims, dtype=torch.float64, device=DEV), tc, 4).abs().max()) < 1e-9
    # channels == per-channel scalar ops
    vals = _t(g.normal(size=(40, 3)))
    mc = spline_spread_channels(tp, vals, tc, dims, spline_order=3)
    assert mc.shape == (3,) + dims
    for ch in range(3):
        assert torch.allclose(mc[ch], spline_spread(tp, vals[:, ch].contiguous(), tc, dims, 3), rtol=0, atol=1e-13)  # atomic-add order (mesh not 8-aligned)
    assert abs(float(mc.sum()) - float(vals.sum())) < 1e-9
    back = spline_gather_channels(tp, mc, tc, spline_order=3)
    assert back.shape == (40, 3) and torch.equal(back[:, 1], spline_gather(tp, mc[1], tc, 3))
    # batch with one shared 2-D cell: two copies of the system give two copies of the mesh
    bi = torch.tensor([0] * 40 + [1] * 40, dtype=torch.int32, device=DEV)
    pp, qq = torch.cat([tp, tp]), torch.cat([tq, tq])
    mb = spline_spread(pp, qq, tc, dims, 4, batch_idx=bi)
    assert mb.shape == (2,) + dims and torch.allclose(mb[0], mb[1], rtol=0, atol=1e-14)
    # the reference's batch spread kernels drop weights <= 1e-8, the single-system kernel keeps every w > 0 (spline.py:608 vs :563)
    np.testing.assert_allclose(mb[0].cpu().numpy(), spline_spread(tp, tq, tc, dims, 4).cpu().numpy(), atol=1e-7)
    fb = spline_gather_gradient(pp, qq, torch.stack([mesh, mesh]), tc, 4, batch_idx=bi)
    np.testing.assert_allclose(fb[40:].cpu().numpy(), f.cpu().numpy(), atol=1e-12)
    mcb = spline_spread_channels(pp, torch.cat([vals, vals]), tc, dims, 3, batch_idx=bi)
    assert mcb.shape == (2, 3) + dims
    vb = spline_gather_channels(pp, mcb, tc, 3, batch_idx=bi)
    assert vb.shape == (80, 3) and torch.allclose(vb[:40], vb[40:], atol=1e-13)
    # autograd flows through the channel wrappers (test_spline.py:1439-1530)
    v2 = vals.clone().requires_grad_(True)
    spline_spread_channels(tp, v2, tc, dims, 3).pow(2).sum().backward()
    assert v2.grad is not None and torch.isfinite(v2.grad).all()


def test_hip_path_against_committed_oracle_vectors():
    """HIP nlist / D3 / PME / explicit-k Ewald against tests/golden/oracle_vectors.npz (made by tests/golden/make_golden.py)."""
    import os

    from nvalchemiops.interactions.dispersion import D3Parameters, dftd3
    from nvalchemiops.interactions.electrostatics import ewald_reciprocal_space, particle_mesh_ewald
    from nvalchemiops.neighborlist import cell_list

    v = np.load(os.path.join(os.path.dirname(__file__), "golden", "oracle_vectors.npz"))
    nm, num, sh = cell_list(_t(v["nl_pos"]), 3.3, _t(v["nl_cell"]), torch.tensor([True, True, False], device=DEV), max_neighbors=128)
    assert np.array_equal(num.cpu().numpy(), v["nl_num"])
    assert np.array_equal(O.canonical_pairs(nm.cpu().numpy(), num.cpu().numpy(), sh.cpu().numpy()), v["nl_pairs"])  # bit-exact
    t = O.d3_test_tables(17)
    prm = D3Parameters(rcov=_t(t["rcov"]), r4r2=_t(t["r4r2"]), c6ab=_t(t["c6ab"]), cn_ref=_t(t["cn_ref"]))
    e, f, cn, vir = dftd3(_t(v["d3_pos"]), _t(v["d3_numbers"]), 0.4, 4.0, 0.8, d3_params=prm, neighbor_matrix=_t(v["d3_nm"]),
                          neighbor_matrix_shifts=_t(v["d3_shifts"]), cell=_t(v["d3_cell"])[None], compute_virial=True)
    np.testing.assert_allclose(e.cpu().numpy(), v["d3_energy"], rtol=2e-6, atol=1e-6)                 # fp32 tolerances of test_d3_gpu.py
    np.testing.assert_allclose(f.cpu().numpy(), v["d3_forces"], rtol=1e-5, atol=1e-6 + 5e-6 * np.abs(v["d3_forces"]).max())
    np.testing.assert_allclose(cn.cpu().numpy(), v["d3_cn"], rtol=5e-6, atol=1e-6)
    np.testing.assert_allclose(vir.cpu().numpy(), v["d3_virial"], rtol=1e-5, atol=2e-6 + 1e-5 * np.abs(v["d3_virial"]).max())
    ep, fp = particle_mesh_ewald(_t(v["pme_pos"]), _t(v["pme_q"]), _t(v["pme_cell"]), alpha=0.4, mesh_dimensions=(24, 24, 24), spline_order=4,
                                 neighbor_matrix=_t(v["pme_nm"]), neighbor_matrix_shifts=_t(v["pme_shifts"]), compute_forces=True)
    _close(ep, v["pme_energies"], np.float64, "pme energies")
    _close(fp, v["pme_forces"], np.float64, "pme forces")
    er, fr, cg = ewald_reciprocal_space(_t(v["pme_pos"]), _t(v["pme_q"]), _t(v["pme_cell"]), _t(v["ewald_kvec"]),
                                        torch.tensor([0.4], dtype=torch.float64, device=DEV), compute_forces=True, compute_charge_gradients=True)
    _close(er, v["ewald_energies"], np.float64, "ewald energies")
    _close(fr, v["ewald_forces"], np.float64, "ewald forces")
    _close(cg, v["ewald_cgrad"], np.float64, "ewald charge gradients")


@pytest.mark.parametrize("dims", [(8, 8, 8), (16, 8, 24), (32, 32, 32), (30, 36, 45), (12, 10, 14), (31, 9, 6)])
@pytest.mark.parametrize("order", [1, 3, 4, 6])
def test_tile_owned_spread(dims, order):
    """Meshes take the tile-owned spread (no global atomics) when every dimension has a divisor e with max(order - 1, 2) <= e <= 8 (the
    per-axis tile edge; one tile per axis wraps onto itself for n = e) and the atomic kernel otherwise (31 is prime; 9 -> e = 3 only
    carries order <= 4): against the oracle for orders <= 4, charge conservation + adjointness with the gather for order 6; atoms
    outside the cell, fp32 and fp64, single system and batch."""
    from nvalchemiops.spline import spline_gather, spline_spread

    for dtype in (np.float64, np.float32):
        pos, cell, q = _system(260, dtype, triclinic=True, seed=order + dims[0])
        pos = (pos + np.random.default_rng(5).integers(-1, 2, (260, 1)) * cell[0]).astype(dtype)  # some atoms outside the cell
        mesh = spline_spread(_t(pos), _t(q), _t(cell), dims, order)
        tol = 1e-9 if dtype == np.float64 else 2e-3
        assert abs(float(mesh.sum()) - q.sum()) < tol
        if order <= 4:
            _close(mesh, O.spline_spread(pos, q, cell, dims, order), dtype, "tiled spread")
        else:
            # a seeded field: the gather drops weights <= 1e-8 that the single-system spread keeps (spline.py:548 vs :608), so the gap is
            # not zero but a few 1e-7 whose size depends on the field -- a field from the global generator made the outcome depend on test order
            gen = torch.Generator(device=DEV).manual_seed(order * 100 + dims[0])
            field = torch.randn(dims, dtype=_t(pos).dtype, device=DEV, generator=gen)
            lhs, rhs = float((mesh * field).sum()), float((_t(q) * spline_gather(_t(pos), field, _t(cell), order)).sum())
            assert abs(lhs - rhs) < (1e-6 if dtype == np.float64 else 1e-2)
        pos2, q2 = np.concatenate([pos, pos * 0.8]).astype(dtype), np.concatenate([q, 2 * q]).astype(dtype)
        cells = np.stack([cell, cell * 0.8]).astype(dtype)
        bi = np.repeat(np.arange(2, dtype=np.int32), len(pos))
        bm = spline_spread(_t(pos2), _t(q2), _t(cells), dims, order, batch_idx=_t(bi))
        if order <= 4:
            _close(bm, O.spline_spread(pos2, q2, cells, dims, order, batch_idx=bi), dtype, "tiled batch spread")
        else:
            # the batch kernels drop weights <= 1e-8 (reference semantics, spline.py:820): conservation only to that level
            assert abs(float(bm[1].sum()) - 2 * q.sum()) < max(tol, 1e-4)


@pytest.mark.parametrize("dims", [(8, 8, 8), (16, 8, 24), (30, 36, 45), (12, 10, 14), (31, 9, 6)])
@pytest.mark.parametrize("order", [3, 4])
def test_tile_staged_gather_epilogue(dims, order):
    """The fused reciprocal pipeline on small / odd meshes: the tile-staged gather epilogue (mesh boxes through LDS, fed by the spread's
    workspace; one tile per axis wraps onto itself for n = e) and its per-atom fallback (31 is prime, 9 -> e = 3 carries order <= 4 only)
    against the oracle -- energies, forces and charge gradients, atoms outside the cell, fp64 and fp32, single system and a batch of two."""
    from nvalchemiops.interactions.electrostatics import pme_reciprocal_space

    for dtype in (np.float64, np.float32):
        pos, cell, q = _system(220, dtype, triclinic=True, seed=order + dims[1])
        pos = (pos + np.random.default_rng(6).integers(-1, 2, (220, 1)) * cell[1]).astype(dtype)  # some atoms outside the cell
        e, f, cg = pme_reciprocal_space(_t(pos), _t(q), _t(cell), 0.4, mesh_dimensions=dims, spline_order=order, compute_forces=True,
                                        compute_charge_gradients=True)
        ref = O.pme_reciprocal_space(pos, q, cell, 0.4, dims, order, compute_forces=True, compute_charge_gradients=True)
        for got, want, what in zip((e, f, cg), ref, ("energies", "forces", "charge gradients")):
            _close(got, want, dtype, f"{what} {dims} order {order}")
        pos2, q2 = np.concatenate([pos, pos * 0.8]).astype(dtype), np.concatenate([q, 2 * q]).astype(dtype)
        cells = np.stack([cell, cell * 0.8]).astype(dtype)
        bi = np.repeat(np.arange(2, dtype=np.int32), len(pos))
        be, bf = pme_reciprocal_space(_t(pos2), _t(q2), _t(cells), torch.tensor([0.4, 0.5], dtype=_t(pos).dtype, device=DEV), mesh_dimensions=dims,
                                      spline_order=order, batch_idx=_t(bi), compute_forces=True)
        bref = O.pme_reciprocal_space(pos2, q2, cells, np.array([0.4, 0.5]), dims, order, batch_idx=bi, compute_forces=True)
        _close(be, bref[0], dtype, f"batch energies {dims}")
        _close(bf, bref[1], dtype, f"batch forces {dims}")


@pytest.mark.parametrize("dims", [(8, 8, 8), (16, 8, 32), (8, 64, 16), (32, 32, 32), (64, 16, 128), (16, 256, 8), (128, 128, 128),
                                  # round 6, mixed radix (sizes that are products of 2, 3, 5; nz even): what a `mesh_spacing=` caller typically gets
                                  (12, 10, 18), (20, 18, 24), (10, 12, 30), (48, 48, 48), (96, 100, 120), (120, 96, 100)])
@pytest.mark.parametrize("order", [4, 5])
def test_fused_mesh_solve(dims, order, monkeypatch):
    """Meshes whose sizes are products of 2, 3 and 5 (round 6; powers of two before) take the library's fused mesh solve (`mi_pme_solve`: plane / column FFTs in LDS with the Green function, the
    B-spline moduli and -i k_d between the forward and inverse x transforms, csrc/fft_lds.h) instead of hipFFT R2C -> `mi_pme_convolve` ->
    hipFFT C2R: same energies / forces / charge gradients from both, and both against the oracle (numpy FFTs); triclinic cell, fp64 and fp32,
    energies only (one channel) and with forces (four), single system and a batch of three with their own alpha."""
    from nvalchemiops import _capi as C
    from nvalchemiops.interactions.electrostatics import pme as P
    from nvalchemiops.interactions.electrostatics import pme_reciprocal_space

    for dtype in (np.float64, np.float32):
        assert C.lib().mi_pme_solve_supported(1, *dims, C.dtype_code(torch.float64 if dtype == np.float64 else torch.float32)) == 1
        n = 300 if max(dims) < 128 else 3000
        pos, cell, q = _system(n, dtype, triclinic=True, seed=order + dims[2])
        tol = dict(rtol=1e-10, atol=1e-12) if dtype == np.float64 else dict(rtol=2e-4, atol=2e-5)
        out = {}
        # A/B against the hipFFT-plan path for EVERY mesh (round 5).  A library plan that does not reproduce an impulse is replaced by torch.fft
        # at creation (`pme._fft_plan`, fail-safe), so the plan path can no longer return a wrong transform: any disagreement fails here.
        for solve in (True, False):
            monkeypatch.setattr(P, "_MESH_SOLVE", solve)
            e0 = pme_reciprocal_space(_t(pos), _t(q), _t(cell), 0.4, mesh_dimensions=dims, spline_order=order)
            e, f, cg = pme_reciprocal_space(_t(pos), _t(q), _t(cell), 0.4, mesh_dimensions=dims, spline_order=order, compute_forces=True,
                                            compute_charge_gradients=True)
            out[solve] = (e0, e, f, cg)
        if max(dims) < 128:  # both paths against the oracle
            with O.extended_splines():
                ref0 = O.pme_reciprocal_space(pos, q, cell, 0.4, dims, order)
            _close(out[True][0], ref0, dtype, f"fused solve, energies only {dims} order {order}")
            _close(out[False][0], ref0, dtype, f"FFT-plan path, energies only {dims} order {order}")
        for a, b in zip(out[True], out[False]):
            scale = float(b.abs().max())
            assert torch.allclose(a, b, rtol=tol["rtol"], atol=tol["atol"] * max(scale, 1.0)), (dims, order, dtype, float((a - b).abs().max()), scale)
        monkeypatch.setattr(P, "_MESH_SOLVE", True)
        if max(dims) < 128:
            with O.extended_splines():
                ref = O.pme_reciprocal_space(pos, q, cell, 0.4, dims, order, compute_forces=True, compute_charge_gradients=True)
            for got, want, what in zip(out[True][1:], ref, ("energies", "forces", "charge gradients")):
                _close(got, want, dtype, f"{what} {dims} order {order}")
            pos3 = np.concatenate([pos, pos * 0.8, pos * 1.1]).astype(dtype)
            q3 = np.concatenate([q, 2 * q, -q]).astype(dtype)
            cells = np.stack([cell, cell * 0.8, cell * 1.1]).astype(dtype)
            bi = np.repeat(np.arange(3, dtype=np.int32), len(pos))
            al = np.array([0.4, 0.5, 0.35])
            be, bf = pme_reciprocal_space(_t(pos3), _t(q3), _t(cells), torch.tensor(al, dtype=_t(pos).dtype, device=DEV), mesh_dimensions=dims,
                                          spline_order=order, batch_idx=_t(bi), compute_forces=True)
            with O.extended_splines():
                bref = O.pme_reciprocal_space(pos3, q3, cells, al, dims, order, batch_idx=bi, compute_forces=True)
            _close(be, bref[0], dtype, f"batch energies {dims}")
            _close(bf, bref[1], dtype, f"batch forces {dims}")


@pytest.mark.parametrize("dims", [(8, 8, 8), (16, 16, 16), (16, 8, 32), (32, 64, 16), (128, 128, 128), (64, 128, 256), (12, 10, 18), (20, 18, 24), (96, 100, 120),
                                  (120, 96, 100), (240, 8, 10)])
def test_in_lds_transforms_equal_numpy(dims):
    """`mi_fft_lds` (round 6): the mesh solve's kernels as unscaled rfftn / irfftn in natural order, against numpy on the host (no rocFFT on
    either side); batches of 1 and 3, fp64 and fp32; the C2R leaves its input untouched; and `_fft_plan` hands these out wherever the mesh
    solve is supported (what the autograd node's backward runs, pme.py:1398 / :1422 / :1455-1457)."""
    from nvalchemiops import _capi as C
    from nvalchemiops.interactions.electrostatics import pme as P

    nx, ny, nz = dims
    rng = np.random.default_rng(sum(dims))
    for rdt, cdt, tol in ((torch.float64, torch.complex128, 1e-12), (torch.float32, torch.complex64, 2e-5)):
        code = C.dtype_code(rdt)
        if not C.lib().mi_pme_solve_supported(1, nx, ny, nz, code):
            assert rdt == torch.float64 and dims == (64, 128, 256)  # fp64: the 128 x 129 complex plane is beyond LDS
            assert isinstance(P._fft_plan(torch.device(DEV), dims, 1, code, False), (P._FftPlan, P._DenseDft))
            continue
        for batch in (1, 3):
            if batch == 3 and nx * ny * nz > 2 ** 21:
                continue
            fwd, inv = P._fft_plan(torch.device(DEV), dims, batch, code, False), P._fft_plan(torch.device(DEV), dims, batch, code, True)
            assert isinstance(fwd, P._LdsFft) and isinstance(inv, P._LdsFft)
            mesh = rng.standard_normal((batch, nx, ny, nz))
            want = np.fft.rfftn(mesh, axes=(1, 2, 3))
            spec = torch.empty((batch, nx, ny, nz // 2 + 1), dtype=cdt, device=DEV)
            fwd(torch.as_tensor(mesh, dtype=rdt, device=DEV), spec)
            scale = float(np.abs(want).max())
            assert np.abs(spec.cpu().numpy() - want).max() <= tol * scale * 8, (dims, rdt, batch)
            # an arbitrary half spectrum back: numpy's irfftn * N; the input survives
            sp = want + rng.standard_normal(want.shape) + 1j * rng.standard_normal(want.shape)
            tsp = torch.as_tensor(sp, dtype=cdt, device=DEV)
            keep = tsp.clone()
            back = torch.empty((batch, nx, ny, nz), dtype=rdt, device=DEV)
            inv(tsp, back)
            ref = np.fft.irfftn(sp, dims, axes=(1, 2, 3)) * float(nx * ny * nz)
            assert np.abs(back.cpu().numpy() - ref).max() <= tol * float(np.abs(ref).max()) * 8, (dims, rdt, batch)
            assert torch.equal(tsp, keep)


def test_fused_mesh_solve_support_table():
    """What the fused solve takes: powers of two whose (ny, nz/2+1) plane fits LDS; everything else keeps hipFFT."""
    from nvalchemiops import _capi as C

    ok = C.lib().mi_pme_solve_supported
    f64, f32 = C.dtype_code(torch.float64), C.dtype_code(torch.float32)
    assert ok(1, 128, 128, 128, f64) == 1 and ok(128, 32, 32, 32, f64) == 1 and ok(1, 256, 64, 256, f64) == 1
    assert ok(1, 256, 256, 256, f64) == 0 and ok(1, 128, 256, 128, f64) == 0      # plane larger than 160 KB
    assert ok(1, 128, 256, 128, f32) == 1 and ok(1, 256, 256, 256, f32) == 0
    assert ok(1, 30, 36, 45, f64) == 0 and ok(1, 4, 8, 8, f64) == 0        # odd nz (real rows are packed in pairs); an axis below 8
    # round 6: products of 2, 3 and 5 -- 96 / 100 / 120 are what `mesh_spacing=` callers get -- but no other prime factor
    assert ok(1, 48, 48, 48, f64) == 1 and ok(1, 96, 100, 120, f64) == 1 and ok(1, 20, 18, 24, f64) == 1 and ok(1, 10, 12, 30, f32) == 1
    assert ok(1, 14, 22, 26, f64) == 0 and ok(1, 12, 10, 14, f64) == 0 and ok(1, 21, 16, 16, f64) == 0
    pref = C.lib().mi_pme_solve_preferred   # measured policy (round 5): wherever it is supported, batches of small meshes included
    assert pref(1, 32, 32, 32, f64) == 1 and pref(128, 32, 32, 32, f64) == 1 and pref(8, 64, 64, 64, f64) == 1 and pref(2, 128, 128, 128, f64) == 1
    assert pref(1, 48, 48, 48, f64) == 1 and pref(1, 14, 22, 26, f64) == 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_failing_fft_plan_is_replaced_not_used(dtype, monkeypatch):
    """Fail-safe of the library-owned hipFFT plans (round 5): every plan created here computes a WRONG transform (its
    result scaled by 1.6, injected below the self-test).  The impulse test at creation catches it, the plan is destroyed, the shape runs
    through the library's dense DFT (`mi_dft3d`) -- energies and forces still equal the oracle's -- and the failure is on record.  A wrong plan is never run on user data."""
    import collections
    import warnings

    from nvalchemiops.interactions.electrostatics import pme as P
    from nvalchemiops.interactions.electrostatics import pme_reciprocal_space

    real_call = P._FftPlan.__call__

    def off_by_60_percent(self, src, dst):
        real_call(self, src, dst)
        dst.mul_(1.6)

    monkeypatch.setattr(P._FftPlan, "__call__", off_by_60_percent)
    monkeypatch.setattr(P, "_FFT_PLANS", collections.OrderedDict())
    monkeypatch.setattr(P, "_FFT_FALLBACKS", [])
    dims, order = (14, 22, 26), 4  # sizes with the prime factors 7, 11, 13: the fused mesh solve cannot take it, the plan path must
    pos, cell, q = _system(300, dtype, triclinic=True, seed=11)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        e, f = pme_reciprocal_space(_t(pos), _t(q), _t(cell), 0.4, mesh_dimensions=dims, spline_order=order, compute_forces=True)
    msgs = [str(w.message) for w in caught if "impulse test" in str(w.message)]
    assert len(msgs) == 2 and len(P._FFT_FALLBACKS) == 2, msgs  # the R2C and the C2R plan
    assert all(isinstance(p, P._DenseDft) for p in P._FFT_PLANS.values())
    ref = O.pme_reciprocal_space(pos, q, cell, 0.4, dims, order, compute_forces=True)
    _close(e, ref[0], dtype, "energies through the fallback")
    _close(f, ref[1], dtype, "forces through the fallback")
    with warnings.catch_warnings(record=True) as caught:  # cached: no second warning, same answer
        warnings.simplefilter("always")
        e2, f2 = pme_reciprocal_space(_t(pos), _t(q), _t(cell), 0.4, mesh_dimensions=dims, spline_order=order, compute_forces=True)
    assert not [w for w in caught if "impulse test" in str(w.message)]
    _close(e2, ref[0], dtype, "energies through the cached fallback")  # (not bitwise: a 300-atom system takes the atomic spread)
    _close(f2, ref[1], dtype, "forces through the cached fallback")


def test_fft_plan_cache_is_bounded_on_the_device(monkeypatch):
    """Twelve mesh shapes through a plan cache of capacity 4: the evicted plans are destroyed (hipfftDestroy) while later shapes keep
    matching the oracle, and a shape that returns is planned -- and self-tested -- again."""
    import collections

    from nvalchemiops.interactions.electrostatics import pme as P
    from nvalchemiops.interactions.electrostatics import pme_reciprocal_space

    monkeypatch.setattr(P, "_FFT_PLANS", collections.OrderedDict())
    monkeypatch.setattr(P, "_FFT_PLAN_CAP", 4)
    monkeypatch.setattr(P, "_FFT_FALLBACKS", [])
    monkeypatch.setattr(P, "_MESH_SOLVE", False)
    pos, cell, q = _system(200, np.float64, triclinic=True, seed=5)
    shapes = [(8, 8, 8), (16, 8, 24), (30, 36, 45), (12, 10, 14), (31, 9, 6), (8, 64, 16), (32, 16, 8), (32, 8, 16), (16, 8, 32), (8, 16, 32),
              (24, 16, 8), (8, 8, 8)]
    for dims in shapes:
        e = pme_reciprocal_space(_t(pos), _t(q), _t(cell), 0.4, mesh_dimensions=dims, spline_order=4)
        assert len(P._FFT_PLANS) <= 4
        ref = O.pme_reciprocal_space(pos, q, cell, 0.4, dims, 4)
        _close(e, ref, np.float64, f"energies {dims} with {len(P._FFT_PLANS)} live plans")
    if P._FFT_FALLBACKS:  # still correct (checked above): on record whether the rocFFT defect shows up under this churn at all
        import warnings

        warnings.warn(f"hipFFT plans replaced by the dense DFT under plan churn: {P._FFT_FALLBACKS}")


@pytest.mark.parametrize("dims,batch", [((8, 8, 8), 1), ((7, 11, 13), 2), ((30, 36, 45), 1), ((16, 8, 32), 3), ((32, 8, 16), 1), ((1, 5, 4), 2),
                                        ((31, 9, 6), 4), ((64, 16, 128), 1), ((20, 18, 24), 5), ((3, 2, 1), 2), ((128, 128, 128), 1), ((257, 4, 6), 1)])
def test_dense_dft_matches_numpy(dims, batch):
    """`mi_dft3d` (csrc/dft.hip): the 3-D real <-> complex transform from its definition, any mesh size -- primes, odd and even last
    dimensions, a length of one, batches -- against numpy.fft in both directions and both precisions (unscaled, like the plan path)."""
    import ctypes  # noqa: F401

    from nvalchemiops import _capi as C

    nx, ny, nz = dims
    g = np.random.default_rng(nx * 131 + ny * 17 + nz)
    for dt, cdt, tol in ((torch.float64, torch.complex128, 2e-13), (torch.float32, torch.complex64, 2e-5)):
        x = g.standard_normal((batch, nx, ny, nz))
        want = np.fft.rfftn(x, axes=(1, 2, 3))
        tx = torch.as_tensor(x, dtype=dt, device=DEV).contiguous()
        spec = torch.empty((batch, nx, ny, nz // 2 + 1), dtype=cdt, device=DEV)
        C.check(C.lib().mi_dft3d(C.ptr(tx), C.ptr(spec), nx, ny, nz, batch, C.dtype_code(dt), 0, C.stream_of(tx)), "mi_dft3d")
        scale = np.abs(want).max()
        assert np.abs(spec.cpu().numpy() - want).max() <= tol * scale * max(1.0, np.sqrt(max(dims)) / 4), (dims, dt)
        # inverse of a Hermitian half spectrum with junk in the imaginary parts of the DC / Nyquist terms (which a C2R transform ignores)
        s = (g.standard_normal(want.shape) + 1j * g.standard_normal(want.shape))
        back_want = np.fft.irfftn(s, s=dims, axes=(1, 2, 3)) * (nx * ny * nz)
        ts = torch.as_tensor(s, dtype=cdt, device=DEV).contiguous()
        back = torch.empty((batch, nx, ny, nz), dtype=dt, device=DEV)
        C.check(C.lib().mi_dft3d(C.ptr(ts), C.ptr(back), nx, ny, nz, batch, C.dtype_code(dt), 1, C.stream_of(ts)), "mi_dft3d")
        assert np.abs(back.cpu().numpy() - back_want).max() <= tol * np.abs(back_want).max() * max(1.0, np.sqrt(max(dims)) / 4), (dims, dt, "inverse")


@pytest.mark.parametrize("dims", [(20, 18, 24), (16, 8, 32), (32, 8, 16), (30, 36, 45)])
def test_pme_through_the_dense_dft(dims, monkeypatch):
    """NVALCHEMIOPS_PME_FFT=dft: the reciprocal-space sum with no rocFFT anywhere (spread -> mi_dft3d -> fused k-space pass -> mi_dft3d ->
    gather), single system and a batch of three, against the oracle -- the shapes include the two for which rocFFT has returned wrong
    transforms on this stack."""
    import collections

    from nvalchemiops.interactions.electrostatics import pme as P
    from nvalchemiops.interactions.electrostatics import pme_reciprocal_space

    monkeypatch.setattr(P, "_FFT_PLANS", collections.OrderedDict())
    monkeypatch.setattr(P, "_FORCE_DFT", True)
    monkeypatch.setattr(P, "_MESH_SOLVE", False)
    for dtype in (np.float64, np.float32):
        pos, cell, q = _system(250, dtype, triclinic=True, seed=dims[0])
        e, f = pme_reciprocal_space(_t(pos), _t(q), _t(cell), 0.4, mesh_dimensions=dims, spline_order=4, compute_forces=True)
        assert all(isinstance(p, P._DenseDft) for p in P._FFT_PLANS.values()) and len(P._FFT_PLANS) >= 2
        ref = O.pme_reciprocal_space(pos, q, cell, 0.4, dims, 4, compute_forces=True)
        _close(e, ref[0], dtype, f"energies {dims}")
        _close(f, ref[1], dtype, f"forces {dims}")
        pos3 = np.concatenate([pos, pos * 0.8, pos * 1.1]).astype(dtype)
        q3 = np.concatenate([q, 2 * q, -q]).astype(dtype)
        cells = np.stack([cell, cell * 0.8, cell * 1.1]).astype(dtype)
        bi = np.repeat(np.arange(3, dtype=np.int32), len(pos))
        al = np.array([0.4, 0.5, 0.35])
        be, bf = pme_reciprocal_space(_t(pos3), _t(q3), _t(cells), torch.tensor(al, dtype=_t(pos).dtype, device=DEV), mesh_dimensions=dims,
                                      spline_order=4, batch_idx=_t(bi), compute_forces=True)
        bref = O.pme_reciprocal_space(pos3, q3, cells, al, dims, 4, batch_idx=bi, compute_forces=True)
        _close(be, bref[0], dtype, f"batch energies {dims}")
        _close(bf, bref[1], dtype, f"batch forces {dims}")


@pytest.mark.parametrize("dims,batch", [((8, 6, 10), 1), ((7, 11, 13), 2), ((16, 8, 32), 1), ((20, 18, 24), 3), ((5, 4, 9), 1)])
def test_guarded_fft_ops_and_their_adjoints_equal_torch_fft(dims, batch):
    """`nvalchemiops::mesh_rfftn` / `::mesh_irfftn` (the composition's FFTs since round 5: self-tested plans or the dense DFT instead of a
    direct torch.fft call): values, first derivatives and a second derivative against torch.fft's own, even and odd last dimensions."""
    from nvalchemiops import _eops as E

    nx, ny, nz = dims
    g = torch.Generator(device=DEV).manual_seed(nx * 7 + nz)
    for dt, cdt, tol in ((torch.float64, torch.complex128, 1e-11), (torch.float32, torch.complex64, 2e-4)):
        x = torch.randn((batch, nx, ny, nz), dtype=dt, device=DEV, generator=g)
        wr = torch.randn((batch, nx, ny, nz // 2 + 1), dtype=dt, device=DEV, generator=g)
        wi = torch.randn((batch, nx, ny, nz // 2 + 1), dtype=dt, device=DEV, generator=g)
        w = torch.complex(wr, wi)
        xs = torch.randn((batch, nx, ny, nz), dtype=dt, device=DEV, generator=g)

        def loss_r2c(fft, inp):
            y = fft(inp)
            return (y * w).real.sum() + (y.abs() ** 2).sum() * 0.01  # linear + quadratic: the second derivative is not identically zero

        def loss_c2r(ifft, sp):
            return (ifft(sp) * xs).sum() + (ifft(sp) ** 2).sum() * 0.01

        a = x.clone().requires_grad_(True)
        b = x.clone().requires_grad_(True)
        la = loss_r2c(E.mesh_rfftn, a)
        lb = loss_r2c(lambda m: torch.fft.rfftn(m, norm="backward", dim=(1, 2, 3)), b)
        (ga,), (gb,) = torch.autograd.grad(la, a, create_graph=True), torch.autograd.grad(lb, b, create_graph=True)
        scale = float(gb.detach().abs().max())
        assert abs(float(la.detach()) - float(lb.detach())) <= tol * abs(float(lb.detach())) + tol and float((ga - gb).detach().abs().max()) <= tol * scale, (dims, dt, "r2c")
        (ha,), (hb,) = torch.autograd.grad((ga * xs).sum(), a), torch.autograd.grad((gb * xs).sum(), b)
        assert float((ha - hb).abs().max()) <= tol * max(float(hb.abs().max()), 1.0), (dims, dt, "r2c second derivative")

        s0 = torch.fft.rfftn(x, norm="backward", dim=(1, 2, 3)) + w  # a generic half spectrum (not Hermitian-consistent: C2R semantics matter)
        a = s0.clone().requires_grad_(True)
        b = s0.clone().requires_grad_(True)
        la = loss_c2r(lambda sp: E.mesh_irfftn(sp, nz), a)
        lb = loss_c2r(lambda sp: torch.fft.irfftn(sp, norm="forward", s=dims, dim=(1, 2, 3)), b)
        (ga,), (gb,) = torch.autograd.grad(la, a, create_graph=True), torch.autograd.grad(lb, b, create_graph=True)
        assert abs(float(la.detach()) - float(lb.detach())) <= tol * abs(float(lb.detach())) + tol, (dims, dt, "c2r value")
        assert float((ga - gb).detach().abs().max()) <= tol * float(gb.detach().abs().max()), (dims, dt, "c2r")
        (ha,), (hb,) = torch.autograd.grad((ga * w.conj()).real.sum(), a), torch.autograd.grad((gb * w.conj()).real.sum(), b)
        assert float((ha - hb).abs().max()) <= tol * max(float(hb.abs().max()), 1.0), (dims, dt, "c2r second derivative")


def test_hipfft_defect_reproduces_without_this_library(tmp_path):
    """Why the plan cache self-tests every hipFFT plan: tests/native/hipfft_repro.cpp -- hipFFT and the HIP runtime, not one
    line of this repository -- plans (16, 16, 16) and then (16, 8, 32) in one process, and the second plan computes a transform ~59 % off
    its definition (each shape alone is exact).  The test documents the state of the INSTALLED rocFFT: it passes when the defect shows (the
    guard is needed) and when it does not (a fixed rocFFT: the guard costs one known-answer test per new plan), and fails only if the
    reproducer itself cannot run.  The outcome is written to gpurun_out/hipfft_repro_status.txt."""
    import os
    import shutil
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    exe = str(tmp_path / "hipfft_repro")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", os.path.join(root, "tests", "native", "hipfft_repro.cpp"), "-o", exe, "-lhipfft"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    alone = subprocess.run([exe, "seq", "explicit", "16", "8", "32"], capture_output=True, text=True, timeout=300)
    assert alone.returncode == 0 and " ok" in alone.stdout, alone.stdout + alone.stderr  # a fresh process: exact
    pair = subprocess.run([exe, "seq", "explicit", "16", "16", "16", "16", "8", "32"], capture_output=True, text=True, timeout=300)
    assert pair.returncode in (0, 1), pair.stdout + pair.stderr
    status = "DEFECT PRESENT: " if pair.returncode == 1 else "defect not reproduced: "
    out = os.path.join(root, "gpurun_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "hipfft_repro_status.txt"), "w") as f:
        f.write(status + pair.stdout.strip().splitlines()[-1] + "\n")
