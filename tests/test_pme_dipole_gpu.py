"""Particle-mesh Ewald for point dipoles on the device against its float64 restatement (tests/pme_dipole_reference.py, itself checked in
tests/test_pme_dipole_reference_cpu.py) on the same mesh and order.

fp64: 1e-10 of the largest |value| of each output, the bar tests/test_pme_gpu.py holds for the mesh path.  fp32: the bar is not fixed in
advance; per output it is 4 x the error of the restatement's own float32 mode against its float64 mode on the same inputs (the margin covers
another summation order in the spread and another FFT factorisation).  The spread uses float atomics, so two runs agree to the last bits
only: everything that compares two device results uses a relative bar (1e-12 in fp64), never equality.

Shapes: 37 atoms in a triclinic cell (at order 5 a spread block holds 10 atoms: a partial last block; the gather's 8-lane groups do not fill
a wave), four of them at fractional coordinates below 0 and above 1, stencils crossing every periodic face, an unequal mesh (12, 10, 16) that
takes the fused solve and (14, 12, 16) whose factor 7 takes the FFT plans (or their dense-DFT replacement: the test does not depend on
which), and a batch of 7 + 1 + 12 atoms with different cells and per-system alpha."""
import functools

import numpy as np
import pytest
import torch

from tests import pme_dipole_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("energies", "forces", "charge_grads", "dipole_grads", "virial")
ALL = dict(compute_forces=True, compute_charge_gradients=True, compute_dipole_gradients=True, compute_virial=True)
CELL = np.array([[8.0, 0.0, 0.0], [0.7, 8.8, 0.0], [-0.4, 0.5, 7.2]])
ALPHA = 0.35
MESH, MESH_PLAN = (12, 10, 16), (14, 12, 16)
CASES = [(4, MESH), (5, MESH), (6, MESH), (5, MESH_PLAN)]


def _t(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


def _np(x):
    return x.detach().cpu().numpy().astype(np.float64)


def _close(got, ref, what, rel):
    got = _np(got) if isinstance(got, torch.Tensor) else got
    ref = _np(ref) if isinstance(ref, torch.Tensor) else ref
    assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max()
    print(f"{what:56s} rel err {err / scale:.2e} (bar {rel:.2e})")
    assert err <= rel * scale, f"{what}: max err {err:.3e} > {rel * scale:.3e}"


def _api():
    from nvalchemiops.interactions.electrostatics import pme_dipole_correction, pme_dipole_reciprocal_space

    return pme_dipole_correction, pme_dipole_reciprocal_space


@functools.lru_cache(maxsize=None)
def _system():
    """37 atoms: four outside the cell, six whose stencils cross one periodic face each, the rest anywhere."""
    g = np.random.default_rng(3)
    frac = g.uniform(0, 1, (37, 3))
    frac[:4] = [[-0.27, 0.4, 1.6], [1.35, -0.6, 0.2], [0.5, 1.02, -0.01], [2.2, 0.97, 0.03]]
    for d in range(3):
        frac[4 + 2 * d, d], frac[5 + 2 * d, d] = 0.01, 0.99
    inside = frac[4:]
    for d in range(3):
        assert (inside[:, d] < 0.05).any() and (inside[:, d] > 0.95).any()
    assert ((frac < 0) | (frac > 1)).any(axis=1).sum() == 4
    pos = frac @ CELL
    q = g.normal(size=37) + 0.05
    mu = 0.5 * g.normal(size=(37, 3)) / np.sqrt(3.0)
    mu[11] = 0.0  # one atom without a dipole
    return pos, q, mu


@functools.lru_cache(maxsize=None)
def _reference(order, dims, dtype=torch.float64):
    pos, q, mu = _system()
    t = lambda a: torch.tensor(a, dtype=torch.float64)  # noqa: E731
    return R.evaluate(t(pos), t(q), t(mu), t(CELL), ALPHA, dims, order, dtype=dtype)


def _inputs(dtype=torch.float64):
    pos, q, mu = _system()
    return _t(pos, dtype), _t(q, dtype), _t(mu, dtype), _t(CELL, dtype).reshape(1, 3, 3)


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,dims", CASES)
def test_parity_fp64(order, dims):
    _, recip = _api()
    ref = _reference(order, dims)
    out = recip(*_inputs(), ALPHA, mesh_dimensions=dims, spline_order=order, **ALL)
    assert len(out) == 5 and all(o.dtype == torch.float64 for o in out)
    for name, o in zip(NAMES, out):
        _close(o, ref[name], f"order {order} mesh {dims} fp64 {name}", 1e-10)
    vir = ref["virial"][0]
    assert np.abs(vir - vir.T).max() > 1e-3 * np.abs(vir).max()  # far above the bar: a symmetrised virial fails the comparison


@pytest.mark.parametrize("order,dims", CASES)
def test_parity_fp32(order, dims):
    _, recip = _api()
    ref, ref32 = _reference(order, dims), _reference(order, dims, torch.float32)
    out = recip(*_inputs(torch.float32), ALPHA, mesh_dimensions=dims, spline_order=order, **ALL)
    assert all(o.dtype == torch.float32 for o in out)
    for name, o in zip(NAMES, out):
        own = np.abs(ref32[name] - ref[name]).max() / np.abs(ref[name]).max()  # the restatement's float32 mode against its float64 mode
        err = np.abs(_np(o).reshape(ref[name].shape) - ref[name]).max() / np.abs(ref[name]).max()
        print(f"order {order} mesh {dims} fp32 {name:13s} kernel {err:.2e}  reference float32 mode {own:.2e}  ratio {err / own:.2f}")
    for name, o in zip(NAMES, out):
        own = np.abs(ref32[name] - ref[name]).max() / np.abs(ref[name]).max()
        _close(o, ref[name], f"order {order} mesh {dims} fp32 {name}", 4.0 * own)


def test_only_what_was_asked_for_is_returned():
    _, recip = _api()
    ref = _reference(5, MESH)
    args = _inputs()
    e = recip(*args, ALPHA, mesh_dimensions=MESH)
    assert isinstance(e, torch.Tensor) and e.shape == (37,)
    _close(e, ref["energies"], "energies alone", 1e-10)
    for k, (flag, name) in enumerate(zip(ALL, NAMES[1:])):
        out = recip(*args, ALPHA, mesh_dimensions=MESH, **{flag: True})
        assert isinstance(out, tuple) and len(out) == 2
        _close(out[1], ref[name], f"{name} alone", 1e-10)
    e, cg, vir = recip(*args, ALPHA, mesh_dimensions=MESH, compute_charge_gradients=True, compute_virial=True)
    _close(cg, ref["charge_grads"], "charge_grads with the virial", 1e-10)
    _close(vir, ref["virial"], "virial with charge_grads", 1e-10)


# ---- 2. batch -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch():
    g = np.random.default_rng(8)
    counts = (7, 1, 12)
    cells = np.stack([CELL, 1.1 * CELL[[1, 2, 0]][:, [1, 2, 0]], np.diag([7.5, 9.0, 8.2]) + 0.3 * np.triu(g.normal(size=(3, 3)), 1).T])
    alpha = np.array([0.35, 0.42, 0.3])
    pos = np.concatenate([g.uniform(-0.2, 1.2, (c, 3)) @ cells[b] for b, c in enumerate(counts)])
    n = sum(counts)
    q, mu = g.normal(size=n), 0.5 * g.normal(size=(n, 3)) / np.sqrt(3.0)
    bi = np.repeat(np.arange(3), counts)
    return pos, q, mu, cells, alpha, bi


def test_batch_against_single_calls_and_the_restatement():
    _, recip = _api()
    pos, q, mu, cells, alpha, bi = _batch()
    t = lambda a: torch.tensor(a, dtype=torch.float64)  # noqa: E731
    ref = R.evaluate(t(pos), t(q), t(mu), t(cells), t(alpha), MESH, 5, batch_idx=torch.tensor(bi))
    BI = torch.as_tensor(bi, device=DEV, dtype=torch.int32)
    out = recip(_t(pos), _t(q), _t(mu), _t(cells), _t(alpha), mesh_dimensions=MESH, spline_order=5, batch_idx=BI, **ALL)
    assert out[4].shape == (3, 3, 3)
    for name, o in zip(NAMES, out):
        _close(o, ref[name], f"batch {name}", 1e-10)
    for b in range(3):
        own = bi == b
        single = recip(_t(pos[own]), _t(q[own]), _t(mu[own]), _t(cells[b:b + 1]), float(alpha[b]), mesh_dimensions=MESH, spline_order=5, **ALL)
        for name, o, full in zip(NAMES, single, out):
            part = full[b:b + 1] if name == "virial" else full[torch.as_tensor(own, device=DEV)]
            # per-system scale: the bar is 1e-10 of the largest |value| of the output of THIS system
            _close(o, part, f"system {b} alone vs in the batch {name}", 1e-10)


# ---- 3. autograd --------------------------------------------------------------------------------------------------------------------------
def test_weighted_loss_against_the_restatement():
    _, recip = _api()
    pos, q, mu = _system()
    g = np.random.default_rng(21).normal(size=37)
    t = lambda a: torch.tensor(a, dtype=torch.float64)  # noqa: E731
    ref = R.evaluate(t(pos), t(q), t(mu), t(CELL), ALPHA, MESH, 5, weights=t(g), virial=False)
    P, Q, M, C = _inputs()
    P, Q, M = (x.clone().requires_grad_(True) for x in (P, Q, M))
    e = recip(P, Q, M, C, ALPHA, mesh_dimensions=MESH, spline_order=5)
    (e * _t(g)).sum().backward()
    _close(e, ref["energies"], "energies under autograd", 1e-10)
    _close(-P.grad, ref["forces"], "dL/dpositions", 1e-10)
    _close(Q.grad, ref["charge_grads"], "dL/dcharges", 1e-10)
    _close(M.grad, ref["dipole_grads"], "dL/ddipoles", 1e-10)


def test_backward_equals_the_explicit_outputs_of_the_same_call():
    _, recip = _api()
    P, Q, M, C = _inputs()
    P, Q, M = (x.clone().requires_grad_(True) for x in (P, Q, M))
    e, f, cg, dg = recip(P, Q, M, C, ALPHA, mesh_dimensions=MESH_PLAN, spline_order=5, compute_forces=True, compute_charge_gradients=True,
                         compute_dipole_gradients=True)
    e.sum().backward()
    _close(-P.grad, f, "-dE/dr vs forces", 1e-10)
    _close(Q.grad, cg, "dE/dq vs charge_grads", 1e-10)
    _close(M.grad, dg, "dE/dmu vs dipole_grads", 1e-10)


def test_second_order_and_out_of_scope_gradients_are_refused():
    _, recip = _api()
    P, Q, M, C = _inputs()
    for flag in ALL:
        p = P.clone().requires_grad_(True)
        _, explicit = recip(p, Q, M, C, ALPHA, mesh_dimensions=MESH, **{flag: True})
        with pytest.raises(NotImplementedError, match="second derivatives"):
            explicit.sum().backward()
    m = M.clone().requires_grad_(True)
    e = recip(P, Q, m, C, ALPHA, mesh_dimensions=MESH)
    (g,) = torch.autograd.grad(e.sum(), [m], create_graph=True)
    with pytest.raises(NotImplementedError, match="second derivatives"):
        g.sum().backward()
    A = torch.tensor([ALPHA], dtype=torch.float64, device=DEV)
    for cell, alpha in ((C.clone().requires_grad_(True), A), (C, A.clone().requires_grad_(True))):
        e = recip(P, Q, M, cell, alpha, mesh_dimensions=MESH)
        with pytest.raises(NotImplementedError, match="use compute_virial"):
            e.sum().backward()


# ---- 4. the explicit routine --------------------------------------------------------------------------------------------------------------
def test_correction_agrees_with_the_explicit_ewald_routine():
    """Same list, same alpha: the real-space halves are the same kernel, the reciprocal halves differ by the mesh error.  Bar: 10 x the relative
    mesh error that tests/test_pme_dipole_reference_cpu.py measures for this order and mesh on its 6-atom system (the factor covers the larger
    system); it is a number of the yardstick, not of the code under test."""
    from nvalchemiops.interactions.electrostatics import ewald_dipole_correction, generate_k_vectors_ewald_summation
    from nvalchemiops.neighborlist import neighbor_list
    from tests.test_pme_dipole_reference_cpu import mesh_error

    both, _ = _api()
    order, dims = 6, (24, 24, 24)
    bar = 10.0 * mesh_error(order, dims)
    P, Q, M, C = _inputs()
    pbc = torch.ones((1, 3), dtype=torch.bool, device=DEV)
    nm, num, sh = neighbor_list(P, 6.0, cell=C, pbc=pbc, max_neighbors=200, method="cell_list")
    assert int(num.max()) <= 200
    lists = dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=37)
    kv = generate_k_vectors_ewald_summation(C, 4.5)  # exp(-k^2 / 4 alpha^2) = 1e-18 at the cutoff: converged
    want = ewald_dipole_correction(P, Q, M, C, ALPHA, kv, **lists, **ALL)
    got = both(P, Q, M, C, ALPHA, mesh_dimensions=dims, spline_order=order, **lists, **ALL)
    for name, a, b in zip(NAMES, got, want):
        err = float((a - b).abs().max() / b.abs().max())
        print(f"mesh vs explicit {name:13s} rel diff {err:.2e} (bar on the energies {bar:.2e})")
    _close(got[0], want[0], "per-atom energies, mesh vs explicit", bar)
    assert abs(float(got[0].sum() - want[0].sum())) <= bar * float(want[0].abs().max())


# ---- 5. trace -----------------------------------------------------------------------------------------------------------------------------
def test_compile_fullgraph_equals_eager():
    from nvalchemiops.neighborlist import neighbor_list

    both, recip = _api()
    P, Q, M, C = _inputs()
    pbc = torch.ones((1, 3), dtype=torch.bool, device=DEV)
    nm, num, sh = neighbor_list(P, 6.0, cell=C, pbc=pbc, max_neighbors=200, method="cell_list")

    def fn(p, q, m):
        e, frc, dg, vir = both(p, q, m, C, ALPHA, mesh_dimensions=MESH, spline_order=5, neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=37,
                               compute_forces=True, compute_dipole_gradients=True, compute_virial=True)
        return e * 2.0, frc, dg, vir

    torch._dynamo.reset()
    got = torch.compile(fn, mode="default", fullgraph=True)(P, Q, M)
    for name, a, b in zip(("energies", "forces", "dipole_grads", "virial"), got, fn(P, Q, M)):
        _close(a, b, f"compiled vs eager {name}", 1e-12)
