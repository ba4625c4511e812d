"""The float64 restatement of the Thole correction (tests/thole_reference.py) checked against the definition of the model on the CPU, and the
condition the systems of the damped solver tests (tests/thole_cases.py) have to meet: D^1/2 H D^1/2 positive definite with damping.

Measured with this reference, smallest eigenvalue of D^1/2 H D^1/2 (D = diag(a)), undamped / damped at a_T = 0.39:
    two atoms (d = 1.5, a = d^3)      -1.064 /  0.673
    l27                                0.653 /  0.715
    l27, polarisabilities x 4         -0.389 /  0.502        (x 6: -1.084 / 0.484,  x 8: -1.779 / 0.469,  x 12: -3.168 / 0.433)
    l64                                (0.72) /  0.750       (undamped: tests/test_induced_reference_cpu.py)
    lone atom                                 /  0.977
so the large-a variant exists for the lattice and the two-atom case is not needed in its place."""
import numpy as np
import pytest
import torch

from tests import induced_reference as IR
from tests import thole_cases as TC
from tests import thole_reference as TR

F64 = torch.float64


def _t(a):
    return torch.as_tensor(a, dtype=F64)


def test_lambda3_is_the_enclosed_charge_of_the_smearing_density():
    """l3(u) = int_0^u 4 pi s^2 (3 a_T / 4 pi) exp(-a_T s^3) ds, by Gauss-Legendre quadrature (96 nodes on [0, u]: the integrand is smooth)."""
    x, w = np.polynomial.legendre.leggauss(96)
    for a_t in (0.39, 0.1, 2.0):
        for u in (0.05, 0.5, 1.0, 1.7, 3.0):
            s = 0.5 * u * (x + 1.0)
            charge = float(np.sum(0.5 * u * w * 4.0 * np.pi * s * s * (3.0 * a_t / (4.0 * np.pi)) * np.exp(-a_t * s**3)))
            l3 = float(TR.lambdas(_t(a_t * u**3))[0])
            assert abs(l3 - charge) <= 1e-13, (a_t, u, l3, charge)


def test_lambda5_and_lambda7_follow_the_recursion():
    """l_{2n+3} = l_{2n+1} - (r / (2n + 1)) dl_{2n+1}/dr with E = a_T r^3 / s^3, the derivative by autograd."""
    a_t, s3 = 0.39, 1.7
    r = torch.linspace(0.05, 4.0, 80, dtype=F64).requires_grad_(True)
    l3, l5, l7 = TR.lambdas(a_t * r**3 / s3)
    (d3,) = torch.autograd.grad(l3.sum(), r, retain_graph=True)
    (d5,) = torch.autograd.grad(l5.sum(), r, retain_graph=True)
    assert float((l5 - (l3 - r / 3.0 * d3)).detach().abs().max()) <= 1e-14
    assert float((l7 - (l5 - r / 5.0 * d5)).detach().abs().max()) <= 1e-14


def _pair(seed=3):
    g = np.random.default_rng(seed)
    pos = _t(np.array([[0.0, 0.0, 0.0], [0.9, -0.7, 1.1]]))
    entries = (torch.tensor([0, 1]), torch.tensor([1, 0]), torch.zeros((2, 3), dtype=torch.long))
    return pos, _t(g.normal(size=2)), _t(g.normal(size=(2, 3))), _t(np.array([1.3, 0.8])), entries


def test_forces_of_a_pair_are_the_closed_form_with_lambda7():
    """-dE/dr of the reference (autograd) against dU/dR of the kernel's header with D_n = (l_{2n+1} - 1) (2n - 1)!! / r^(2n+1)."""
    pos, q, mu, polar, entries = _pair()
    ref = TR.evaluate(pos, q, mu, polar, None, 0.39, entries)
    R = pos[1] - pos[0]
    r = torch.sqrt((R * R).sum())
    l3, l5, l7 = TR.lambdas(0.39 * r**3 / torch.sqrt(polar[0] * polar[1]))
    D1, D2, D3 = (l3 - 1) / r**3, 3 * (l5 - 1) / r**5, 15 * (l7 - 1) / r**7
    ci, cj, d = mu[0] @ R, mu[1] @ R, mu[0] @ mu[1]
    A = q[1] * ci - q[0] * cj + d
    dUdR = (-D2 * A + D3 * ci * cj) * R + (D1 * q[1] - D2 * cj) * mu[0] - (D1 * q[0] + D2 * ci) * mu[1]
    assert abs(float(ref["energies"].sum()) - float(D1 * A - D2 * ci * cj)) <= 1e-15
    assert float(np.abs(ref["forces"][0] - dUdR.numpy()).max()) <= 1e-14 and float(np.abs(ref["forces"].sum(0)).max()) <= 1e-15
    # dU/da_i = X (-E / (2 a_i)) with X = dU/dE at fixed R
    E = 0.39 * r**3 / torch.sqrt(polar[0] * polar[1])
    X = torch.exp(-E) / r**3 * A - 3 * E * torch.exp(-E) / r**5 * ci * cj
    assert float(np.abs(ref["polar_grads"] - (X * (-E / (2 * polar))).numpy()).max()) <= 1e-14


def test_correction_vanishes_for_a_wide_width_and_for_non_polarisable_atoms():
    pos, q, mu, polar, entries = _pair()
    full = TR.evaluate(pos, q, mu, polar, None, 0.39, entries)
    assert float(np.abs(full["energies"]).max()) > 1e-3
    for a_t, bar in ((1e2, 1e-30), (1e6, 0.0)):
        out = TR.evaluate(pos, q, mu, polar, None, a_t, entries)
        assert all(float(np.abs(v).max()) <= bar for v in out.values()), a_t
    for bad in (0.0, -1.0, float("nan")):
        out = TR.evaluate(pos, q, mu, _t(np.array([1.3, bad])), None, 0.39, entries)
        assert all(float(np.abs(v).max()) == 0.0 for v in out.values()), bad


def test_damped_pair_tensor_is_finite_at_contact():
    """(l3 / r^3) I - (3 l5 / r^5) R R^T -> (a_T / s^3) I as r -> 0, s^3 = sqrt(a_i a_j): the first neglected terms are of relative order E."""
    a_i, a_j, a_t = 1.3, 0.8, 0.39
    limit = a_t / (a_i * a_j) ** 0.5
    axis = _t(np.array([0.6, -0.48, 0.64]))
    for r in (1e-1, 1e-2, 1e-3, 1e-5):
        T = TR.pair_tensor(r * axis, a_i, a_j, a_t)
        E = a_t * r**3 / (a_i * a_j) ** 0.5
        assert bool(torch.isfinite(T).all())
        assert float((T - limit * torch.eye(3, dtype=F64)).abs().max()) <= 4.0 * E * limit + 1e-15, r
    # and it is the Hessian of (bare + correction) in the dipoles: the correction's Hessian is the pair tensor minus the bare tensor
    pos, q, mu, polar, entries = _pair()
    R = pos[1] - pos[0]
    r = torch.sqrt((R * R).sum())
    bare = torch.eye(3, dtype=F64) / r**3 - 3.0 * torch.outer(R, R) / r**5
    hess, _ = IR.quadratic_form(lambda m: TR.energies(pos, q, m, polar, None, a_t, *entries).sum(), 2, "cpu")
    assert float((hess[:3, 3:] - (TR.pair_tensor(R, 1.3, 0.8, a_t) - bare)).abs().max()) <= 1e-15


def test_float32_distance_mode_differs_by_float32_rounding_only():
    pos, q, mu, polar, entries = _pair()
    a = TR.evaluate(pos, q, mu, polar, None, 0.39, entries)
    b = TR.evaluate(pos, q, mu, polar, None, 0.39, entries, distance_dtype=torch.float32)
    for k in a:
        dev = float(np.abs(a[k] - b[k]).max()) / float(np.abs(a[k]).max())
        assert 0.0 < dev <= 1e-5, (k, dev)


CASES = {"two_atoms": TC.two_atoms, "lone_atom": TC.lone_atom, "l27": lambda: TC.lattice("l27"), "l64": lambda: TC.lattice("l64"),
         "l27_large": lambda: TC.lattice("l27", large=True)}
INDEFINITE_UNDAMPED = ("two_atoms", "l27_large")


@pytest.mark.parametrize("name", list(CASES))
def test_damped_operator_of_every_solver_case_is_positive_definite(name):
    """What entitles the CG of the GPU tests to converge.  The two-atom case and the large-a lattice are indefinite without damping."""
    case = CASES[name]()
    damped = TC.dense(case, TC.THOLE)
    assert float((damped["T"] - damped["T"].T).abs().max()) <= 1e-14
    ev = IR.scaled_spectrum(damped["H"], damped["polar"])
    line = f"{name}: D^1/2 H D^1/2 damped in [{float(ev.min()):.3f}, {float(ev.max()):.3f}]"
    if name in INDEFINITE_UNDAMPED:
        plain = TC.dense(case, None)
        ev0 = IR.scaled_spectrum(plain["H"], plain["polar"])
        line += f", undamped in [{float(ev0.min()):.3f}, {float(ev0.max()):.3f}]"
        assert float(ev0.min()) < 0, "the undamped H must be indefinite"
    print(line)
    assert float(ev.min()) > 0.25  # a condition on the inputs, not a measurement
