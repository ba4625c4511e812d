"""The float64 restatement of the dispersion PME (tests/pme_dispersion_reference.py) against the explicit sum it must converge to, against a
finite difference of its own strained energy, and at the k = 0 element of its operator."""
import math

import numpy as np
import pytest
import torch

from nvalchemiops.interactions.electrostatics.k_vectors import generate_k_vectors_ewald_summation
from tests import dispersion_ewald_reference as X
from tests import pme_dispersion_reference as R

F64 = torch.float64
G = torch.Generator().manual_seed(11)
CELL = torch.tensor([[9.0, 0, 0], [1.1, 8.6, 0], [0.5, -0.8, 9.3]], dtype=F64)
POS = torch.rand(12, 3, generator=G, dtype=F64) @ CELL
COEF = 0.5 + torch.rand(12, generator=G, dtype=F64)
BETA = 0.35


def test_converges_to_the_explicit_sum_with_the_mesh():
    """12 atoms, order 6, against the explicit reciprocal sum at |k| <= 13 beta (f < 1e-19 beyond).  Relative errors (largest |difference| over
    largest |value|) measured when this test was written, meshes 12^3, 16^3, 24^3:
        energies 9.99e-07, 2.09e-07, 9.93e-09      forces 2.87e-05, 1.03e-05, 9.46e-07
    The bar at 24^3 is 3 x those values; the factor covers another libm only."""
    exact = X.evaluate(POS, COEF, CELL, BETA, k_vectors=generate_k_vectors_ewald_summation(CELL, 13.0 * BETA))
    errs = {"energies": [], "forces": []}
    for n in (12, 16, 24):
        mesh = R.evaluate(POS, COEF, CELL, BETA, (n, n, n), 6, virial=False)
        for name, e in errs.items():
            ref = exact[name].numpy()
            e.append(np.abs(mesh[name] - ref).max() / np.abs(ref).max())
    print(errs)
    for name, bar in (("energies", 3 * 9.93e-09), ("forces", 3 * 9.46e-07)):
        e = errs[name]
        assert e[0] > e[1] > e[2], (name, e)
        assert e[2] < bar, (name, e[2], bar)


@pytest.mark.parametrize("order,dims", [(4, (12, 10, 16)), (5, (9, 12, 10)), (6, (12, 12, 12))])
def test_virial_is_the_strain_derivative(order, dims):
    def total(eps):
        defo = torch.eye(3, dtype=F64) + eps
        return float(R.system_energies(POS @ defo.T, COEF, CELL @ defo.T, BETA, dims, order).sum())

    vir = R.evaluate(POS, COEF, CELL, BETA, dims, order)["virial"][0]
    h = 1e-5
    fd = np.zeros((3, 3))
    for a in range(3):
        for b in range(3):
            eps = torch.zeros(3, 3, dtype=F64)
            eps[a, b] = h
            fd[a, b] = -(total(eps) - total(-eps)) / (2 * h)
    assert np.abs(vir - fd).max() <= 1e-6 * np.abs(fd).max(), (vir, fd)
    assert np.abs(vir - vir.T).max() <= 1e-12 * np.abs(vir).max()


def test_origin_of_the_operator_is_the_k0_term():
    d = R.influence(CELL, BETA, (12, 10, 16), 5)
    want = -math.pi ** 1.5 * BETA ** 3 / (6.0 * float(torch.linalg.det(CELL).abs()))
    assert abs(float(d[0, 0, 0]) - want) <= 1e-15 * abs(want)
