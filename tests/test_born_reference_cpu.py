"""tests/born_reference.py, the reference of `generalized_born`, against what is known independently of it: the volume integral behind the
descreening closed form (one point in each branch), one ion, two atoms written out, and the Coulomb-screening limit.  No GPU."""
import math

import pytest
import torch

from tests import born_reference as R

T = lambda v, dtype=torch.float64: torch.tensor(v, dtype=dtype)  # noqa: E731
KW = dict(solute_dielectric=2.0, solvent_dielectric=80.0, coulomb_constant=332.0)
PREF = -0.5 * 332.0 * (1 / 2.0 - 1 / 80.0)


def test_public_name_is_exported():
    from nvalchemiops.interactions import electrostatics as E
    from nvalchemiops.interactions.electrostatics.born import generalized_born

    assert "generalized_born" in E.__all__ and E.generalized_born is generalized_born


# (r, rho, S): separate spheres; overlapping with L = rho; overlapping with L = |r - S|; atom buried in the sphere; sphere engulfed by the atom
@pytest.mark.parametrize("r, rho, S", [(4.0, 1.2, 1.0), (1.5, 1.2, 1.0), (2.0, 0.7, 1.0), (0.4, 0.5, 1.5), (0.3, 1.5, 1.0)],
                         ids=["separate", "overlap_rho", "overlap_diff", "buried", "engulfed"])
def test_closed_form_is_the_volume_integral(r, rho, S):
    got, want = float(R.descreen(T(r), T(rho), T(S))), R.descreen_quadrature(r, rho, S)
    if r + S <= rho:
        assert got == 0.0 and want == 0.0
    else:
        assert want > 0 and abs(got - want) <= 1e-13 * want


def test_one_ion_is_the_born_formula():
    out = R.evaluate(torch.zeros(1, 3), T([1.5]), T([2.0]), T([0.8]), T([], torch.long), T([], torch.long), **KW)
    assert abs(float(out["born_radii"][0]) - 1.91) < 1e-15
    assert abs(float(out["energies"][0]) - PREF * 1.5**2 / 1.91) < 1e-12 and float(out["forces"].abs().max()) == 0.0


@pytest.mark.parametrize("obc", [R.OBC1, R.OBC2], ids=["obc1", "obc2"])
def test_two_atoms_against_the_written_out_formula(obc):
    r, (q0, q1), rad, scr, off = 2.3, (0.7, -1.1), (1.7, 1.2), (0.85, 0.72), 0.09
    out = R.evaluate(T([[0.0, 0, 0], [0, r, 0]]), T([q0, q1]), T(rad), T(scr), T([0, 1], torch.long), T([1, 0], torch.long), obc=obc, surface_tension=0.0054, **KW)
    rho = [x - off for x in rad]
    born = []
    for a, b in ((0, 1), (1, 0)):
        psi = rho[a] * R.descreen_quadrature(r, rho[a], scr[b] * rho[b])
        born.append(1 / (1 / rho[a] - math.tanh(obc[0] * psi - obc[1] * psi**2 + obc[2] * psi**3) / rad[a]))
    f = math.sqrt(r * r + born[0] * born[1] * math.exp(-r * r / (4 * born[0] * born[1])))
    want = [PREF * (q * q / B + q0 * q1 / f) + 4 * math.pi * 0.0054 * (Ri + 1.4) ** 2 * (Ri / B) ** 6 for q, B, Ri in zip((q0, q1), born, rad)]
    assert torch.allclose(out["energies"], T(want), rtol=1e-12, atol=0)
    assert float((out["forces"][0] + out["forces"][1]).abs().max()) < 1e-12 and abs(float(out["forces"][0, 1])) > 1e-3


def test_far_apart_the_pair_term_screens_coulomb():
    pos = T([[0.0, 0, 0], [300.0, 0, 0], [0, 400.0, 0]])
    q, i, j = T([1.0, -0.6, 0.8]), T([0, 0, 1, 1, 2, 2], torch.long), T([1, 2, 0, 2, 0, 1], torch.long)
    out = R.evaluate(pos, q, T([1.5, 1.8, 1.2]), T([0.8, 0.8, 0.8]), i, j, **KW)
    self_term = PREF * q**2 / out["born_radii"]
    coulomb = PREF * (q[i] * q[j] / (pos[j] - pos[i]).norm(dim=1)).sum()
    assert abs(float((out["energies"] - self_term).sum() - coulomb)) < 1e-5 * abs(float(coulomb))  # f = r (1 + O(B^2 / r^2))
