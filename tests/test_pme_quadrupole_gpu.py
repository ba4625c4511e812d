"""Particle-mesh Ewald for point quadrupoles on the device against its float64 restatement (tests/pme_quadrupole_reference.py, itself checked
in tests/test_pme_quadrupole_reference_cpu.py) on the same mesh and order.

fp64: 1e-10 of the largest |value| of each output, the bar of tests/test_pme_gpu.py and tests/test_pme_dipole_gpu.py.  fp32: the bar is not
fixed in advance; per output it is 4 x the error of the restatement's own float32 mode against its float64 mode on the same inputs (the
margin covers another summation order in the spread and another FFT factorisation).  The spread uses float atomics, so two runs agree to the
last bits only: everything that compares two device results uses a relative bar (1e-12 in fp64), never equality.

Shapes: the 37-atom triclinic system of tests/test_pme_dipole_gpu.py (same construction: four atoms outside the cell, stencils across every
periodic face; at order 5 a spread block holds 10 atoms and at order 6 it holds 7 with idle threads, both with a partial last block; the
gather's 8-lane groups do not fill a wave) with Q = 0.3 normal, four of them unsymmetric, one atom without a dipole and three without a
quadrupole.  Meshes: (12, 10, 16) takes the fused solve, (14, 12, 16) the FFT plans, (12, 10, 15) has an odd axis without a Nyquist plane,
and (5, 6, 7) at order 5 and (6, 7, 8) at order 6 have an axis equal to the order, so that the stencil wraps onto the whole axis.  A batch of 7 + 1 + 12 atoms with
different cells and per-system alpha.

The fp64 parity cases and the weighted-loss case run a second time on poisoned scratch (tests/poison.py): a mesh or a partial table that a
kernel reads before anything wrote it then fails its own comparison."""
import functools

import numpy as np
import pytest
import torch

from tests import pme_quadrupole_reference as R
from tests import poison

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("energies", "forces", "charge_grads", "dipole_grads", "quadrupole_grads", "virial")
ALL = dict(compute_forces=True, compute_charge_gradients=True, compute_dipole_gradients=True, compute_quadrupole_gradients=True,
           compute_virial=True)
CELL = np.array([[8.0, 0.0, 0.0], [0.7, 8.8, 0.0], [-0.4, 0.5, 7.2]])
ALPHA = 0.35
MESH, MESH_PLAN, MESH_ODD, MESH_WRAP = (12, 10, 16), (14, 12, 16), (12, 10, 15), (5, 6, 7)
MESH_WRAP6 = (6, 7, 8)
CASES = [(order, dims) for dims in (MESH, MESH_PLAN, MESH_ODD) for order in (5, 6)] + [(5, MESH_WRAP), (6, MESH_WRAP6)]
N = 37


@pytest.fixture(autouse=True)
def _device_guard(request):
    with poison.device_guard(request.node.nodeid):
        yield


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
    print(f"{what:60s} rel err {err / scale:.2e} (bar {rel:.2e})")
    assert err <= rel * scale, f"{what}: max err {err:.3e} > {rel * scale:.3e}"


def _api():
    from nvalchemiops.interactions.electrostatics import pme_quadrupole_correction, pme_quadrupole_reciprocal_space

    return pme_quadrupole_correction, pme_quadrupole_reciprocal_space


@functools.lru_cache(maxsize=None)
def _system():
    """37 atoms: four outside the cell, six whose stencils cross one periodic face each, the rest anywhere (the construction of
    tests/test_pme_dipole_gpu.py), then the quadrupoles."""
    g = np.random.default_rng(3)
    frac = g.uniform(0, 1, (N, 3))
    frac[:4] = [[-0.27, 0.4, 1.6], [1.35, -0.6, 0.2], [0.5, 1.02, -0.01], [2.2, 0.97, 0.03]]
    for d in range(3):
        frac[4 + 2 * d, d], frac[5 + 2 * d, d] = 0.01, 0.99
    inside = frac[4:]
    for d in range(3):
        assert (inside[:, d] < 0.05).any() and (inside[:, d] > 0.95).any()
    assert ((frac < 0) | (frac > 1)).any(axis=1).sum() == 4
    pos = frac @ CELL
    q = g.normal(size=N) + 0.05
    mu = 0.5 * g.normal(size=(N, 3)) / np.sqrt(3.0)
    mu[11] = 0.0  # one atom without a dipole
    Q = 0.3 * g.normal(size=(N, 3, 3))
    unsymmetric = (2, 9, 20, 33)
    for i in range(N):
        if i not in unsymmetric:
            Q[i] = 0.5 * (Q[i] + Q[i].T)
    Q[[5, 11, 30]] = 0.0  # three atoms without a quadrupole (one of them the atom without a dipole)
    assert sum(bool(np.abs(Q[i] - Q[i].T).max() > 1e-3) for i in range(N)) == 4
    return pos, q, mu, Q


@functools.lru_cache(maxsize=None)
def _reference(order, dims, dtype=torch.float64):
    t = lambda a: torch.tensor(a, dtype=torch.float64)  # noqa: E731
    return R.evaluate(*(t(a) for a in _system()), t(CELL), ALPHA, dims, order, dtype=dtype)


def _inputs(dtype=torch.float64):
    return tuple(_t(a, dtype) for a in _system()) + (_t(CELL, dtype).reshape(1, 3, 3),)


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------------------
def _parity_fp64(order, dims):
    _, recip = _api()
    ref = _reference(order, dims)
    out = recip(*_inputs(), ALPHA, mesh_dimensions=dims, spline_order=order, **ALL)
    assert len(out) == 6 and all(o.dtype == torch.float64 for o in out)
    for name, o in zip(NAMES, out):
        _close(o, ref[name], f"order {order} mesh {dims} fp64 {name}", 1e-10)
    return out


@pytest.mark.parametrize("order,dims", CASES)
def test_parity_fp64(order, dims):
    _parity_fp64(order, dims)


@pytest.mark.parametrize("order,dims", CASES)
def test_virial_is_not_symmetric_and_quadrupole_grads_are(order, dims):
    vir = _reference(order, dims)["virial"][0]
    assert np.abs(vir - vir.T).max() > 1e-3 * np.abs(vir).max()  # far above the bar: a symmetrised virial fails the comparison
    _, recip = _api()
    _, qg = recip(*_inputs(), ALPHA, mesh_dimensions=dims, spline_order=order, compute_quadrupole_gradients=True)
    assert torch.equal(qg, qg.transpose(1, 2))


@pytest.mark.parametrize("order,dims", CASES)
def test_parity_fp32(order, dims):
    _, recip = _api()
    ref, ref32 = _reference(order, dims), _reference(order, dims, torch.float32)
    out = recip(*_inputs(torch.float32), ALPHA, mesh_dimensions=dims, spline_order=order, **ALL)
    assert all(o.dtype == torch.float32 for o in out)
    own = {name: np.abs(ref32[name] - ref[name]).max() / np.abs(ref[name]).max() for name in NAMES}  # float32 mode against float64 mode
    for name, o in zip(NAMES, out):
        err = np.abs(_np(o).reshape(ref[name].shape) - ref[name]).max() / np.abs(ref[name]).max()
        print(f"order {order} mesh {dims} fp32 {name:16s} kernel {err:.2e}  reference float32 mode {own[name]:.2e}  ratio {err / own[name]:.2f}")
    for name, o in zip(NAMES, out):
        _close(o, ref[name], f"order {order} mesh {dims} fp32 {name}", 4.0 * own[name])


# ---- 2. contracts -------------------------------------------------------------------------------------------------------------------------
def test_only_what_was_asked_for_is_returned():
    _, recip = _api()
    ref = _reference(5, MESH)
    args = _inputs()
    e = recip(*args, ALPHA, mesh_dimensions=MESH)
    assert isinstance(e, torch.Tensor) and e.shape == (N,)
    _close(e, ref["energies"], "energies alone", 1e-10)
    for flag, name in zip(ALL, NAMES[1:]):
        out = recip(*args, ALPHA, mesh_dimensions=MESH, **{flag: True})
        assert isinstance(out, tuple) and len(out) == 2
        _close(out[1], ref[name], f"{name} alone", 1e-10)
    e, cg, qg, vir = recip(*args, ALPHA, mesh_dimensions=MESH, compute_charge_gradients=True, compute_quadrupole_gradients=True, compute_virial=True)
    _close(cg, ref["charge_grads"], "charge_grads with quadrupole_grads and the virial", 1e-10)
    _close(qg, ref["quadrupole_grads"], "quadrupole_grads with charge_grads and the virial", 1e-10)
    _close(vir, ref["virial"], "virial with charge_grads and quadrupole_grads", 1e-10)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_zero_quadrupoles_give_exact_zeros_but_a_field_gradient(dtype):
    _, recip = _api()
    P, Q, M, T, C = _inputs(dtype)
    e, f, cg, dg, qg, vir = recip(P, Q, M, torch.zeros_like(T), C, ALPHA, mesh_dimensions=MESH, spline_order=5, **ALL)
    for name, o in (("energies", e), ("forces", f), ("charge_grads", cg), ("dipole_grads", dg), ("virial", vir)):
        assert torch.equal(o, torch.zeros_like(o)), name
    assert float(qg.abs().max()) > 1e-3 and bool(torch.isfinite(qg).all())


def test_no_dipoles_and_dipole_independence_of_the_dipole_gradients():
    _, recip = _api()
    P, Q, M, T, C = _inputs()
    none = recip(P, Q, None, T, C, ALPHA, mesh_dimensions=MESH, **ALL)
    zero = recip(P, Q, torch.zeros_like(M), T, C, ALPHA, mesh_dimensions=MESH, **ALL)
    for name, a, b in zip(NAMES, none, zero):
        _close(a, b, f"dipoles=None vs zero dipoles {name}", 1e-12)
    _, dg = recip(P, Q, M, T, C, ALPHA, mesh_dimensions=MESH, compute_dipole_gradients=True)
    _, other = recip(P, Q, -3.0 * M.flip(0), T, C, ALPHA, mesh_dimensions=MESH, compute_dipole_gradients=True)
    _close(other, dg, "dipole_grads for two dipole arrays", 1e-12)
    _close(none[3], dg, "dipole_grads without dipoles", 1e-12)


# ---- 3. batch -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch():
    g = np.random.default_rng(8)
    counts = (7, 1, 12)
    cells = np.stack([CELL, 1.1 * CELL[[1, 2, 0]][:, [1, 2, 0]], np.diag([7.5, 9.0, 8.2]) + 0.3 * np.triu(g.normal(size=(3, 3)), 1).T])
    alpha = np.array([0.35, 0.42, 0.3])
    pos = np.concatenate([g.uniform(-0.2, 1.2, (c, 3)) @ cells[b] for b, c in enumerate(counts)])
    n = sum(counts)
    q, mu, Q = g.normal(size=n), 0.5 * g.normal(size=(n, 3)) / np.sqrt(3.0), 0.3 * g.normal(size=(n, 3, 3))
    bi = np.repeat(np.arange(3), counts)
    return pos, q, mu, Q, cells, alpha, bi


def test_batch_against_single_calls_and_the_restatement():
    _, recip = _api()
    pos, q, mu, Q, cells, alpha, bi = _batch()
    t = lambda a: torch.tensor(a, dtype=torch.float64)  # noqa: E731
    ref = R.evaluate(t(pos), t(q), t(mu), t(Q), t(cells), t(alpha), MESH, 5, batch_idx=torch.tensor(bi))
    BI = torch.as_tensor(bi, device=DEV, dtype=torch.int32)
    out = recip(_t(pos), _t(q), _t(mu), _t(Q), _t(cells), _t(alpha), mesh_dimensions=MESH, spline_order=5, batch_idx=BI, **ALL)
    assert out[5].shape == (3, 3, 3)
    for name, o in zip(NAMES, out):
        _close(o, ref[name], f"batch {name}", 1e-10)
    for b in range(3):
        own = bi == b
        single = recip(_t(pos[own]), _t(q[own]), _t(mu[own]), _t(Q[own]), _t(cells[b:b + 1]), float(alpha[b]), mesh_dimensions=MESH,
                       spline_order=5, **ALL)
        for name, o, full in zip(NAMES, single, out):
            part = full[b:b + 1] if name == "virial" else full[torch.as_tensor(own, device=DEV)]
            _close(o, part, f"system {b} alone vs in the batch {name}", 1e-12)  # relative, never equality: the spread adds in arrival order


# ---- 4. autograd --------------------------------------------------------------------------------------------------------------------------
def _weighted_loss():
    _, recip = _api()
    g = np.random.default_rng(21).normal(size=N)
    ref = _weighted_reference()
    P, Q, M, T, C = _inputs()
    P, Q, M, T = (x.clone().requires_grad_(True) for x in (P, Q, M, T))
    e = recip(P, Q, M, T, C, ALPHA, mesh_dimensions=MESH, spline_order=5)
    (e * _t(g)).sum().backward()
    _close(e, ref["energies"], "energies under autograd", 1e-10)
    _close(-P.grad, ref["forces"], "dL/dpositions", 1e-10)
    _close(Q.grad, ref["charge_grads"], "dL/dcharges", 1e-10)
    _close(M.grad, ref["dipole_grads"], "dL/ddipoles", 1e-10)
    _close(T.grad, ref["quadrupole_grads"], "dL/dquadrupoles", 1e-10)


@functools.lru_cache(maxsize=None)
def _weighted_reference():
    g = np.random.default_rng(21).normal(size=N)
    t = lambda a: torch.tensor(a, dtype=torch.float64)  # noqa: E731
    return R.evaluate(*(t(a) for a in _system()), t(CELL), ALPHA, MESH, 5, weights=t(g), virial=False)


def test_weighted_loss_against_the_restatement():
    _weighted_loss()


def test_backward_equals_the_explicit_outputs_of_the_same_call():
    _, recip = _api()
    P, Q, M, T, C = _inputs()
    P, Q, M, T = (x.clone().requires_grad_(True) for x in (P, Q, M, T))
    e, f, cg, dg, qg = recip(P, Q, M, T, C, ALPHA, mesh_dimensions=MESH_PLAN, spline_order=6, compute_forces=True, compute_charge_gradients=True,
                             compute_dipole_gradients=True, compute_quadrupole_gradients=True)
    e.sum().backward()
    _close(-P.grad, f, "-dE/dr vs forces", 1e-10)
    _close(Q.grad, cg, "dE/dq vs charge_grads", 1e-10)
    _close(M.grad, dg, "dE/dmu vs dipole_grads", 1e-10)
    _close(T.grad, qg, "dE/dQ vs quadrupole_grads", 1e-10)


def test_second_order_and_out_of_scope_gradients_are_refused():
    _, recip = _api()
    P, Q, M, T, C = _inputs()
    for flag in ALL:
        p = P.clone().requires_grad_(True)
        _, explicit = recip(p, Q, M, T, C, ALPHA, mesh_dimensions=MESH, **{flag: True})
        with pytest.raises(NotImplementedError, match="second derivatives"):
            explicit.sum().backward()
    qd = T.clone().requires_grad_(True)
    e = recip(P, Q, M, qd, C, ALPHA, mesh_dimensions=MESH)
    (g,) = torch.autograd.grad(e.sum(), [qd], create_graph=True)
    with pytest.raises(NotImplementedError, match="second derivatives"):
        g.sum().backward()
    A = torch.tensor([ALPHA], dtype=torch.float64, device=DEV)
    for cell, alpha in ((C.clone().requires_grad_(True), A), (C, A.clone().requires_grad_(True))):
        e = recip(P, Q, M, T, cell, alpha, mesh_dimensions=MESH)
        with pytest.raises(NotImplementedError, match="use compute_virial"):
            e.sum().backward()


# ---- 5. the explicit routine --------------------------------------------------------------------------------------------------------------
def _neighbours(P, C):
    from nvalchemiops.neighborlist import neighbor_list

    pbc = torch.ones((1, 3), dtype=torch.bool, device=DEV)
    nm, num, sh = neighbor_list(P, 6.0, cell=C, pbc=pbc, max_neighbors=200, method="cell_list")
    assert int(num.max()) <= 200
    return dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=N)


def test_correction_agrees_with_the_explicit_ewald_routine():
    """Same full list, same alpha: the real-space halves are the same kernel, the reciprocal halves differ by the mesh error.  Bar: 10 x the
    relative mesh error that tests/test_pme_quadrupole_reference_cpu.py measures for order 6 on 32^3 on its 6-atom system (the factor covers
    the larger system; the rule of tests/test_pme_dipole_gpu.py); it is a number of the yardstick, not of the code under test."""
    from nvalchemiops.interactions.electrostatics import ewald_quadrupole_correction, generate_k_vectors_ewald_summation
    from tests.test_pme_quadrupole_reference_cpu import mesh_error

    both, _ = _api()
    order, dims = 6, (32, 32, 32)
    bar = 10.0 * mesh_error(order, dims)
    P, Q, M, T, C = _inputs()
    lists = _neighbours(P, C)
    kv = generate_k_vectors_ewald_summation(C, 4.5)  # exp(-k^2 / 4 alpha^2) = 1e-18 at the cutoff: converged
    want = ewald_quadrupole_correction(P, Q, M, T, C, ALPHA, kv, **lists, **ALL)
    got = both(P, Q, M, T, C, ALPHA, mesh_dimensions=dims, spline_order=order, **lists, **ALL)
    for name, a, b in zip(NAMES, got, want):
        err = float((a - b).abs().max() / b.abs().max())
        print(f"mesh vs explicit {name:16s} rel diff {err:.2e} (bar on the energies {bar:.2e})")
    _close(got[0], want[0], "per-atom energies, mesh vs explicit", bar)
    assert abs(float(got[0].sum() - want[0].sum())) <= bar * float(want[0].abs().max())


# ---- 6. trace -----------------------------------------------------------------------------------------------------------------------------
def test_compile_fullgraph_equals_eager():
    both, _ = _api()
    P, Q, M, T, C = _inputs()
    lists = _neighbours(P, C)

    def fn(p, q, m, t):
        e, frc, qg, vir = both(p, q, m, t, C, ALPHA, mesh_dimensions=MESH, spline_order=5, compute_forces=True, compute_quadrupole_gradients=True,
                               compute_virial=True, **lists)
        return e * 2.0, frc, qg, vir

    torch._dynamo.reset()
    got = torch.compile(fn, mode="default", fullgraph=True)(P, Q, M, T)
    for name, a, b in zip(("energies", "forces", "quadrupole_grads", "virial"), got, fn(P, Q, M, T)):
        _close(a, b, f"compiled vs eager {name}", 1e-12)


# ---- 7. poisoned scratch ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,dims", CASES)
def test_poisoned__parity_fp64(order, dims, request):
    with poison.poisoned_case(request.node.nodeid):
        _parity_fp64(order, dims)


def test_poisoned__weighted_loss_against_the_restatement(request):
    with poison.poisoned_case(request.node.nodeid):
        _weighted_loss()
