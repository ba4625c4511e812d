"""The yardstick of tests/test_pme_quadrupole_gpu.py checked on its own: tests/pme_quadrupole_reference.py (mesh sum for point quadrupoles,
restated from the definition) against the explicit reciprocal sum of tests/quadrupole_reference.py over a converged k set, against finite
differences of its own energy, against the closed virial formula the device code uses, and against the symmetries of the model.  No device,
no library.

The system is the 6-atom box of tests/test_pme_dipole_reference_cpu.py (same generator, same order of draws) with Q = 0.3 normal(6, 3, 3),
symmetrised, drawn next.  Relative errors are max |difference| of the per-atom energies over max |per-atom energy| of the explicit sum.
Measured (order: 16^3, 24^3, 32^3):  4: 1.1e-2 6.4e-3 3.9e-3;  5: 5.0e-4 6.6e-5 6.0e-5;  6: 5.0e-5 1.5e-5 4.2e-6."""
import functools
import math

import numpy as np
import torch

from tests import pme_quadrupole_reference as R
from tests import quadrupole_reference as QR
from tests.gaussian_reference import brute_force_entries
from tests.test_pme_dipole_reference_cpu import ALPHA, CELL, half_space_k
from tests.test_pme_dipole_reference_cpu import system as dipole_system

F64 = torch.float64
MESHES = ((16, 16, 16), (24, 24, 24), (32, 32, 32))


@functools.lru_cache(maxsize=None)
def system():
    g = np.random.default_rng(11)
    pos = g.uniform(0, 1, (6, 3)) @ CELL
    q = g.normal(size=6)
    q -= q.mean()
    mu = 0.5 * g.normal(size=(6, 3)) / math.sqrt(3.0)
    Q = 0.3 * g.normal(size=(6, 3, 3))
    Q = 0.5 * (Q + Q.transpose(0, 2, 1))
    t = lambda a: torch.tensor(a, dtype=F64)  # noqa: E731
    out = t(pos), t(q), t(mu), t(Q), t(CELL)
    for mine, theirs in zip((out[0], out[1], out[2], out[4]), dipole_system()):
        assert torch.equal(mine, theirs)
    return out


@functools.lru_cache(maxsize=None)
def explicit(alpha=ALPHA):
    pos, q, mu, Q, cell = system()
    return QR.recip_energies(pos, q, mu, Q, cell, half_space_k(CELL), alpha).detach()


@functools.lru_cache(maxsize=None)
def mesh_error(order, dims, alpha=ALPHA):
    """Relative error of the mesh energies against the converged explicit sum: THE number the bars of the GPU file are built on."""
    pos, q, mu, Q, cell = system()
    ref = explicit(alpha)
    e = R.energies(pos, q, mu, Q, cell, alpha, dims, order).detach()
    return float((e - ref).abs().max() / ref.abs().max())


def total(pos, q, mu, Q, cell, dims=(16, 16, 16), order=5, alpha=ALPHA):
    return R.energies(pos, q, mu, Q, cell, alpha, dims, order).sum().detach()


def test_converges_to_the_explicit_sum():
    errs = {(o, d): mesh_error(o, d) for o in (4, 5, 6) for d in MESHES}
    for o in (4, 5, 6):
        print(f"order {o}: " + "  ".join(f"{d[0]}^3 {errs[(o, d)]:.2e}" for d in MESHES))
    assert errs[(6, MESHES[2])] < errs[(6, MESHES[1])] < errs[(6, MESHES[0])]
    assert errs[(5, MESHES[1])] < errs[(5, MESHES[0])]
    assert errs[(6, MESHES[2])] < 1e-5


def test_zero_quadrupoles_give_exactly_zero():
    pos, q, mu, Q, cell = system()
    e = R.energies(pos, q, mu, torch.zeros_like(Q), cell, ALPHA, (16, 16, 16), 5)
    assert torch.equal(e, torch.zeros_like(e))


def test_dipole_gradients_do_not_depend_on_the_dipoles():
    """dE/dmu_i = 2 grad W_i . phi_T holds no dipole: two dipole arrays give the same numbers (measured: difference 0.0; the bar is the
    rounding of float64, since autograd may order the two equal contributions differently)."""
    pos, q, mu, Q, cell = system()
    a = R.evaluate(pos, q, mu, Q, cell, ALPHA, (12, 10, 16), 5, virial=False)["dipole_grads"]
    b = R.evaluate(pos, q, -3.0 * mu.flip(0), Q, cell, ALPHA, (12, 10, 16), 5, virial=False)["dipole_grads"]
    print(f"dipole_grads for two dipole arrays: difference {np.abs(a - b).max():.1e}")
    assert np.abs(a).max() > 1e-3
    assert np.abs(a - b).max() <= 1e-14 * np.abs(a).max()


def test_linear_and_quadratic_parts_in_the_quadrupoles():
    pos, q, mu, Q, cell = system()
    full, double = float(total(pos, q, mu, Q, cell)), float(total(pos, q, mu, 2.0 * Q, cell))
    qq = float(total(pos, 0.0 * q, 0.0 * mu, Q, cell))  # E = E_lin (charge- and dipole-quadrupole) + E_QQ
    lin = full - qq
    assert abs(double - (2.0 * lin + 4.0 * qq)) <= 1e-12 * abs(full)
    assert abs(lin) > 1e-3 * abs(qq) and abs(qq) > 1e-3 * abs(lin)  # both parts are there


def test_lattice_translation_of_one_atom():
    pos, q, mu, Q, cell = system()
    ref = R.energies(pos, q, mu, Q, cell, ALPHA, (16, 16, 16), 5).detach()
    moved = pos.clone()
    moved[2] += cell[0] - 2.0 * cell[1] + cell[2]
    e = R.energies(moved, q, mu, Q, cell, ALPHA, (16, 16, 16), 5).detach()
    assert float((e - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_derivatives_against_central_differences():
    pos, q, mu, Q, cell = system()
    dims, order, h = (12, 10, 16), 5, 1e-5
    out = R.evaluate(pos, q, mu, Q, cell, ALPHA, dims, order, virial=False)
    f = lambda p, c, m, t: float(total(p, c, m, t, cell, dims, order))  # noqa: E731

    def fd(which, idx):
        args = [pos.clone(), q.clone(), mu.clone(), Q.clone()]
        args[which][idx] += h
        up = f(*args)
        args[which][idx] -= 2 * h
        return (up - f(*args)) / (2 * h)

    scale = {k: np.abs(v).max() for k, v in out.items()}
    assert np.abs(out["quadrupole_grads"] - out["quadrupole_grads"].transpose(0, 2, 1)).max() <= 1e-14 * scale["quadrupole_grads"]
    for i in range(6):
        for a in range(3):
            assert abs(-fd(0, (i, a)) - out["forces"][i, a]) <= 1e-8 * scale["forces"]
            assert abs(fd(2, (i, a)) - out["dipole_grads"][i, a]) <= 1e-8 * scale["dipole_grads"]
            for b in range(a, 3):  # the gradient is symmetric (asserted above) and Q_ab, Q_ba enter through their mean
                assert abs(fd(3, (i, a, b)) - out["quadrupole_grads"][i, a, b]) <= 1e-8 * scale["quadrupole_grads"]
        assert abs(fd(1, i) - out["charge_grads"][i]) <= 1e-8 * scale["charge_grads"]


def test_virial_against_finite_strain():
    pos, q, mu, Q, cell = system()
    dims, order, h = (12, 10, 16), 5, 1e-5
    vir = R.evaluate(pos, q, mu, Q, cell, ALPHA, dims, order)["virial"][0]

    def strained(a, b, step):
        defo = torch.eye(3, dtype=F64)
        defo[a, b] += step
        return float(total(pos @ defo.T, q, mu, Q, cell @ defo.T, dims, order))

    for a in range(3):
        for b in range(3):
            fd = -(strained(a, b, h) - strained(a, b, -h)) / (2 * h)
            assert abs(fd - vir[a, b]) <= 1e-8 * np.abs(vir).max(), (a, b, fd, vir[a, b])
    assert np.abs(vir - vir.T).max() > 1e-3 * np.abs(vir).max()  # multipoles fixed in the laboratory frame: not symmetric


def test_closed_virial_formula_against_strain_autograd():
    """The formula of the device code -- k-space sum of the cross spectrum + sum (dE/dmu)_a mu_b + 2 sum (G Q)_ab -- on an odd mesh.  Both
    sides are float64 sums of a few thousand terms of the size of the result: 1e-12 (measured 8e-16).  With the factor 2 of the last term
    replaced by 1 the virial is 43 % off."""
    pos, q, mu, Q, cell = system()
    dims, order = (12, 10, 15), 5
    vir = R.evaluate(pos, q, mu, Q, cell, ALPHA, dims, order)["virial"][0]
    closed = R.closed_virial(pos, q, mu, Q, cell, ALPHA, dims, order)
    err = np.abs(closed - vir).max() / np.abs(vir).max()
    print(f"closed virial formula vs strain autograd: {err:.1e}")
    assert err <= 1e-12


def test_odd_meshes_are_as_accurate_as_their_even_neighbours():
    """On an odd axis the rfft half grid has no Nyquist plane and the Miller index of the upper half starts one later: a wrong half-spectrum
    weight or index there costs orders of magnitude, not the 50 % allowed here (the bar of tests/test_pme_dipole_reference_cpu.py)."""
    for n in (15, 21):
        for order in (5, 6):
            odd, even = mesh_error(order, (n, n, n)), mesh_error(order, (n - 1, n - 1, n - 1))
            print(f"order {order}: mesh {n}^3 {odd:.2e}, mesh {n - 1}^3 {even:.2e}, ratio {odd / even:.2f}")
            assert odd <= 1.5 * even, (order, n)


def test_real_plus_mesh_does_not_depend_on_alpha():
    pos, q, mu, Q, cell = system()
    dims, order = MESHES[1], 6
    i, j, S = brute_force_entries(pos.numpy(), CELL, 16.0, 3)  # erfc(0.35 x 16) = 2e-15: the real-space sum is converged
    sums = []
    for alpha in (0.35, 0.40):
        sums.append((QR.real_energies(pos, q, mu, Q, cell, alpha, i, j, S) + R.energies(pos, q, mu, Q, cell, alpha, dims, order)).detach())
    bar = 2.0 * max(mesh_error(order, dims, 0.35), mesh_error(order, dims, 0.40))  # each sum is off by its own mesh error
    err = float((sums[0] - sums[1]).abs().max() / sums[0].abs().max())
    print(f"alpha 0.35 vs 0.40: relative difference {err:.2e} (bar {bar:.2e})")
    assert err <= bar
