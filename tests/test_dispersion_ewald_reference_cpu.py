"""Pins tests/dispersion_ewald_reference.py, the yardstick of tests/test_dispersion_ewald_gpu.py, without a GPU: the dispersion Ewald sum
converges absolutely, so the split can be checked against a brute-force lattice sum."""
import math

import torch

from nvalchemiops.interactions.electrostatics.k_vectors import generate_k_vectors_ewald_summation
from tests import dispersion_ewald_reference as R
from tests import vdw_reference as V

F64 = torch.float64
CELL = torch.tensor([[6.0, 0, 0], [1.2, 5.4, 0], [0.6, -0.9, 6.6]], dtype=F64)
G = torch.Generator().manual_seed(5)
POS = (torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]], dtype=F64) * 0.5 + 0.1 + 0.15 * torch.rand(5, 3, generator=G, dtype=F64)) @ CELL
RADII, EPS = 2.6 + 0.6 * torch.rand(5, generator=G, dtype=F64), 0.05 + 0.25 * torch.rand(5, generator=G, dtype=F64)
COEF = torch.sqrt(2.0 * EPS) * RADII ** 3


def _total(beta, counted=None, entries=None):
    """Converged: g(7.5) = 2e-21 of the pair term at the real cutoff, f(6.5) = 1e-19 at the k cutoff."""
    entries = R.entries_within(POS, CELL, 7.5 / beta) if entries is None else entries
    kv = generate_k_vectors_ewald_summation(CELL, 13.0 * beta)
    return float(R.real_energies(POS, COEF, CELL, beta, *entries, counted=counted).sum() + R.recip_energies(POS, COEF, CELL, kv, beta).sum())


def test_total_does_not_depend_on_beta_and_is_the_direct_lattice_sum():
    totals = [_total(beta) for beta in (0.3, 0.45, 0.6)]
    spread = (max(totals) - min(totals)) / abs(totals[0])
    print(f"totals {totals}: spread {spread:.2e}")
    assert spread <= 1e-13  # some thousand terms of one sign, each right to a few ulp
    # The direct sum is cut at a sphere and closed with the continuum tail t(R) = -1/2 (sum c)^2 4 pi / (3 V R^3).  The continuum stands for
    # whole cells, so it cannot know the surface better than one cell: its next-order term is what the tail changes over the longest cell
    # edge h, |t(R) - t(R + h)|.  Measured gap at R = 60: 7.9e-8 on a total of -2.666 (3e-8 of it), the bar is 5.5e-5 (2e-5 of it); a wrong
    # k = 0 or reciprocal prefactor (1/24 for 1/6) moves the total by 0.1 of itself.
    radius, h = 60.0, float(CELL.norm(dim=1).max())
    tail = lambda r: 0.5 * float(COEF.sum()) ** 2 * 4.0 * math.pi / (3.0 * float(torch.linalg.det(CELL).abs()) * r ** 3)  # noqa: E731
    gap = abs(R.lattice_sum(POS, COEF, CELL, radius) - totals[0])
    print(f"gap to the direct sum {gap:.3e}, bar {tail(radius) - tail(radius + h):.3e}, total {totals[0]:.6e}")
    assert gap <= tail(radius) - tail(radius + h)


def test_counted_part_plus_truncated_lennard_jones_is_the_lattice_sum():
    """LJ(cutoff, taper) + counted correction = the tapered r^-12 part alone + the uncounted correction, geometric rules."""
    cutoff, taper, beta = 5.5, 4.5, 0.35
    i, j, S = entries = R.entries_within(POS, CELL, 7.5 / beta)
    lj = V.energies("lennard_jones", POS, RADII, EPS, CELL, i, j, S, cutoff=cutoff, taper=taper, radius_rule="geometric", epsilon_rule="geometric")
    rvec = POS[j] - POS[i] + S.to(F64) @ CELL
    r = rvec.norm(dim=1)
    Rij, eij = V.combine(RADII, EPS, i, j, "geometric", "geometric")
    repulsion = (0.5 * eij * (1.0 - R.one_minus_switch(r, cutoff, taper)) * (r / Rij) ** -12).sum()
    assert int(((r > taper) & (r < cutoff)).sum()) > 0 and int((r < taper).sum()) > 0
    lhs, rhs = float(lj.sum()) + _total(beta, (cutoff, taper), entries), float(repulsion) + _total(beta, None, entries)
    print(f"counted {lhs:.15e} uncounted {rhs:.15e}")
    assert abs(lhs - rhs) <= 1e-13 * (abs(float(lj.sum())) + abs(float(repulsion)))


def test_series_and_direct_branch_of_one_minus_g_agree_across_the_threshold():
    """The difference 1 - g carries the rounding of g, at most 2 ulp of 1 (exp, the polynomial and their product), whatever is left of it; the
    series carries a few ulp of itself.  So the branches agree to 4 eps absolutely, and the difference form is 4 eps / (1 - g) relatively:
    3e-15 at a^2 = 1, where 1 - g = 0.080 (measured: 4e-16), growing as 6 / a^6 below it -- hence the series there."""
    a2 = torch.linspace(0.5, 1.5, 201, dtype=F64)
    assert float((R.one_minus_g_series(a2) - R.one_minus_g_direct(a2)).abs().max()) <= 4.0 * torch.finfo(F64).eps
    edge = torch.tensor([R.SERIES_BELOW], dtype=F64)
    below, above = R.one_minus_g(torch.nextafter(edge, edge - 1.0)), R.one_minus_g(edge)
    assert abs(float(below - above)) <= 4.0 * torch.finfo(F64).eps
    tiny = torch.tensor([1e-4], dtype=F64)
    assert abs(float(R.one_minus_g(tiny)) / (1e-12 / 6.0 * (1.0 - 0.75e-4)) - 1.0) <= 1e-7  # a^6 / 6 (1 - 3 a^2 / 4 + ...)


def test_counted_cutoff_without_a_taper_is_the_limit_of_a_narrow_one():
    """counted = (rc, None): the step at rc, what a taper window of 1e-9 gives on entries outside it; and not the plain sum."""
    from tests import sweep_cases as W

    c = W.dispersion_case("sweep", 5)
    rc = c["counted"][0]
    assert c["counted"][1] is None
    a = W.dispersion_reference(c, "real", torch.float64)
    b = W.dispersion_reference(dict(c, counted=(rc, rc - 1e-9)), "real", torch.float64)
    plain = W.dispersion_reference(dict(c, counted=None), "real", torch.float64)
    for k in W.DE_NAMES:
        assert torch.equal(a[k], b[k]) and not torch.equal(a[k], plain[k]), k


def test_a_k_vector_below_the_threshold_weighs_nothing():
    """|k|^2 < 1e-10: the restatement on the edge case's set with (1e-6, 0, 0) appended is the restatement on the set without it, every output;
    a vector just above the threshold does weigh."""
    from tests import sweep_cases as W

    c = W.dispersion_case("edge")
    plain = W.dispersion_reference(c, "recip", torch.float64)
    tiny = W.dispersion_reference(dict(c, k_vectors=c["k_tiny"]), "recip", torch.float64)
    above = torch.cat([c["k_vectors"], torch.tensor([[[2e-5, 0.0, 0.0]]], dtype=torch.float64)], dim=1)
    heavy = W.dispersion_reference(dict(c, k_vectors=above), "recip", torch.float64)
    for k in W.DE_NAMES:
        assert torch.equal(plain[k], tiny[k]), k
    assert not torch.equal(plain["energies"], heavy["energies"])
