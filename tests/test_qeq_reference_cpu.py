"""The float64 restatement of charge equilibration (tests/qeq_reference.py) against results that involve no Ewald split and no erfc: this
file tests the yardstick the GPU tests use, on the CPU."""
import math

import numpy as np
import torch

from tests import gaussian_reference as GR
from tests import qeq_reference as R

F64 = torch.float64


def _box(n=10, seed=3, box=6.0):
    g = np.random.default_rng(seed)
    cell = np.array([[box, 0, 0], [0.2 * box, 0.9 * box, 0], [0.1 * box, -0.15 * box, 1.1 * box]])
    pos = g.uniform(0, 1, (n, 3)) @ cell
    return pos, cell, g.uniform(0.4, 0.8, n), g.normal(size=n), g.uniform(0.5, 1.5, n)


def test_ewald_split_charges_equal_exact_k_space_charges():
    """Charged (Q = 1.7) triclinic 10-atom box, all sigma > 0.  H from the Ewald split (exact erfc, alpha = 0.6, real-space images to 14 A,
    full k set to Miller index 9, self, background and Gaussian terms) against diag(J) + the exact A_ij =
    (4 pi / V) sum_{k != 0} exp(-k^2 (sigma_i^2 + sigma_j^2) / 2) cos(k . r_ij) / k^2 (Miller index 20), which has no erfc and no alpha.
    Measured on the CPU: largest charge difference 4.4e-16 on charges up to 1.25 (two ulp; chemical potential: identical to the last bit).
    The bar is a decade above the measured gap: 4.5e-15 on the charges, and the same for the chemical potential (|lambda| = 0.3), whose
    measured gap of zero gives no decade to add."""
    pos, cell, sigma, chi, hard = _box()
    alpha = 0.6
    i, j, S = GR.brute_force_entries(pos, cell, 14.0, 4)
    P, C, Sg, X, J = (torch.as_tensor(a, dtype=F64) for a in (pos, cell, sigma, chi, hard))
    rng = torch.arange(-9, 10, dtype=F64)
    miller = torch.stack(torch.meshgrid(rng, rng, rng, indexing="ij"), dim=-1).reshape(-1, 3)
    kv = miller[(miller != 0).any(-1)] @ (2.0 * math.pi * torch.linalg.inv(C).T)
    h_split = R.dense_operator(P, Sg, J, C, torch.tensor([alpha], dtype=F64), kv, i, j, S, half_space=False)
    h_exact = torch.diag(J) + R.exact_gaussian_operator(P, Sg, C, 20)
    q_split, lam_split = R.solve(h_split, X, 1.7)
    q_exact, lam_exact = R.solve(h_exact, X, 1.7)
    gap = float((q_split - q_exact).abs().max())
    scale = float(q_exact.abs().max())
    print(f"charge gap {gap:.2e} on max |q| {scale:.2f}; lambda gap {abs(float(lam_split - lam_exact)):.2e} on {float(lam_exact):.3f}")
    assert abs(float(q_exact.sum()) - 1.7) < 1e-13 and abs(float(q_split.sum()) - 1.7) < 1e-13
    assert gap <= 4.5e-15
    assert abs(float(lam_split - lam_exact)) <= 4.5e-15
    assert float(R.projected_residual(h_exact, X, q_split)[0]) <= 1e-12 * float(torch.linalg.norm(X))
    # the half-space form of the same k set (weight 2) is the same operator
    half = miller[(miller[:, 0] > 0) | ((miller[:, 0] == 0) & (miller[:, 1] > 0)) | ((miller[:, 0] == 0) & (miller[:, 1] == 0) & (miller[:, 2] > 0))]
    h_half = R.dense_operator(P, Sg, J, C, torch.tensor([alpha], dtype=F64), half @ (2.0 * math.pi * torch.linalg.inv(C).T), i, j, S)
    assert float((h_half - h_split).abs().max()) <= 1e-13 * float(h_split.abs().max())


def test_neutral_two_atom_cluster_closed_form():
    """Two Gaussian charges +q, -q at distance r without a cell: q = -(chi_1 - chi_2) / (d_1 + d_2 - 2 erf(r / g) / r),
    d_i = J_i + 1 / (sqrt(pi) sigma_i), and lambda = chi_1 + (d_1 - erf(r / g) / r) q."""
    pos = torch.tensor([[0.0, 0.0, 0.0], [0.9, 0.4, -0.3]], dtype=F64)
    sigma, chi, hard = torch.tensor([0.5, 0.7], dtype=F64), torch.tensor([0.3, -0.45], dtype=F64), torch.tensor([1.1, 0.8], dtype=F64)
    i, j, S = torch.tensor([0, 1]), torch.tensor([1, 0]), torch.zeros((2, 3), dtype=torch.long)
    h = R.dense_operator(pos, sigma, hard, None, None, None, i, j, S)
    q, lam = R.solve(h, chi, 0.0)
    r = float(torch.linalg.norm(pos[1] - pos[0]))
    gam = math.sqrt(2.0 * (0.25 + 0.49))
    d = [1.1 + 1.0 / (math.sqrt(math.pi) * 0.5), 0.8 + 1.0 / (math.sqrt(math.pi) * 0.7)]
    pair = math.erf(r / gam) / r
    want = -(0.3 + 0.45) / (d[0] + d[1] - 2.0 * pair)
    assert abs(float(q[0]) - want) <= 1e-15 and abs(float(q[1]) + want) <= 1e-15
    assert abs(float(lam[0]) - (0.3 + (d[0] - pair) * want)) <= 1e-15
    # a point charge (sigma = 0) next to a cloud: g = sqrt(2) sigma_2, no self term for atom 0; two point charges: plain 1 / r
    h0 = R.dense_operator(pos, torch.tensor([0.0, 0.7], dtype=F64), hard, None, None, None, i, j, S)
    assert abs(float(h0[0, 0]) - 1.1) <= 1e-15 and abs(float(h0[0, 1]) - math.erf(r / (math.sqrt(2.0) * 0.7)) / r) <= 1e-15
    h00 = R.dense_operator(pos, torch.zeros(2, dtype=F64), hard, None, None, None, i, j, S)
    assert abs(float(h00[0, 1]) - 1.0 / r) <= 1e-15


def test_polynomial_erfc_and_float32_distance_models():
    """The two arithmetic models the GPU tests select: the A-S polynomial is within its published 1.5e-7 of erfc, and the float32-distance
    coefficients are within float32 resolution of the float64 ones while their derivatives are those of the float64 expressions."""
    x = torch.linspace(0.0, 6.0, 601, dtype=F64)
    assert float((R.erfc_as(x) - torch.erfc(x)).abs().max()) <= 1.5e-7
    pos, cell, sigma, _, _ = _box()
    i, j, S = GR.brute_force_entries(pos, cell, 5.0, 2)
    P, C, Sg = (torch.as_tensor(a, dtype=F64) for a in (pos, cell, sigma))
    al = torch.tensor([0.5], dtype=F64)
    c64 = R.pair_coefficients(P, Sg, C, al, i, j, S)
    c32 = R.pair_coefficients(P, Sg, C, al, i, j, S, distance_dtype=torch.float32)
    assert 0.0 < float((c32 - c64).abs().max()) <= 2e-6 * float(c64.abs().max())
    p1, p2 = P.clone().requires_grad_(True), P.clone().requires_grad_(True)
    g64 = torch.autograd.grad(R.pair_coefficients(p1, Sg, C, al, i, j, S).sum(), p1)[0]
    g32 = torch.autograd.grad(R.pair_coefficients(p2, Sg, C, al, i, j, S, distance_dtype=torch.float32).sum(), p2)[0]
    assert float((g32 - g64).abs().max()) <= 1e-5 * float(g64.abs().max())
