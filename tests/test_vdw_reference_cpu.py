"""Closed forms that pin tests/vdw_reference.py, the yardstick of tests/test_vdw_gpu.py.  No device."""
import pytest
import torch

from tests import vdw_reference as R

F64 = torch.float64
PAIR = (torch.tensor([0, 1]), torch.tensor([1, 0]), torch.zeros((2, 3), dtype=torch.long))  # two atoms, stored from both ends


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("radius_rule", ["arithmetic", "geometric", "cubic-mean"])
@pytest.mark.parametrize("epsilon_rule", ["geometric", "hhg"])
def test_two_atoms_at_the_minimum_give_minus_epsilon(kind, radius_rule, epsilon_rule):
    radii, eps = torch.tensor([3.1, 3.9], dtype=F64), torch.tensor([0.11, 0.27], dtype=F64)
    Rij, eij = R.combine(radii, eps, torch.tensor([0]), torch.tensor([1]), radius_rule, epsilon_rule)
    pos = torch.tensor([[0.0, 0, 0], [0, 0, float(Rij)]], dtype=F64)
    out = R.evaluate(kind, pos, radii, eps, None, *PAIR, cutoff=9.0, radius_rule=radius_rule, epsilon_rule=epsilon_rule)
    assert abs(float(out["energies"].sum()) + float(eij)) <= 1e-14
    if kind == "lennard_jones":  # rho = 1 is the minimum of the 12-6 form; the buffered 14-7 has U(R) = -eps slightly off its minimum
        assert float(out["forces"].abs().max()) <= 1e-13


@pytest.mark.parametrize("kind", R.KINDS)
def test_taper_is_one_at_r_on_zero_at_the_cutoff_and_the_force_is_continuous(kind):
    radii, eps = torch.tensor([3.0, 3.4], dtype=F64), torch.tensor([0.2, 0.1], dtype=F64)
    r = torch.tensor([5.4, 6.0], dtype=F64)
    assert torch.equal(R.switch(r, 6.0, 5.4), torch.tensor([1.0, 0.0], dtype=F64))

    def force(dist, taper):
        pos = torch.tensor([[0.0, 0, 0], [dist, 0, 0]], dtype=F64)
        return float(R.evaluate(kind, pos, radii, eps, None, *PAIR, cutoff=6.0, taper=taper)["forces"][0, 0])

    h = 1e-7
    assert abs(force(5.4 + h, 5.4) - force(5.4 - h, 5.4)) <= 1e-6 * abs(force(5.4, None))  # T'(r_on) = 0
    assert abs(force(6.0 - h, 5.4)) <= 1e-6 * abs(force(5.4, None)) and force(6.0 + h, 5.4) == 0.0  # T(cutoff) = T'(cutoff) = 0


@pytest.mark.parametrize("kind", R.KINDS)
def test_reduced_sites_no_net_force_or_torque_and_virial_is_the_site_pair_sum(kind):
    g = torch.Generator().manual_seed(3)  # two water-like molecules with reduced hydrogens and a lone atom, all pairs between different molecules
    pos = torch.tensor([[0.0, 0, 0], [0.9, 0.3, 0], [-0.2, 0.95, 0.1], [3.6, 0.4, 0.2], [4.4, 0.9, 0.1], [3.5, -0.5, 0.6], [1.5, 3.9, 0.5]], dtype=F64)
    mol = torch.tensor([0, 0, 0, 1, 1, 1, 2])
    sites = (torch.tensor([-1, 0, 0, 3, 3, 3, -1]), 0.8 + 0.15 * torch.rand(7, generator=g, dtype=F64))
    i, j = torch.nonzero(mol[:, None] != mol[None, :], as_tuple=True)
    radii, eps = 3.0 + torch.rand(7, generator=g, dtype=F64), 0.1 + 0.2 * torch.rand(7, generator=g, dtype=F64)
    cell = torch.eye(3, dtype=F64) * 30.0
    S = torch.zeros((len(i), 3), dtype=torch.long)
    out = R.evaluate(kind, pos, radii, eps, cell, i, j, S, cutoff=9.0, taper=8.0, sites=sites)
    f, vir = out["forces"], out["virial"][0]
    scale = float(f.abs().max())
    assert scale > 1e-3
    assert float(f.sum(0).abs().max()) <= 1e-13 * scale
    assert float(torch.linalg.cross(pos, f).sum(0).abs().max()) <= 1e-12 * scale
    site = R.site_positions(pos, cell[None], torch.zeros(7, dtype=torch.long), sites).detach().requires_grad_(True)
    e = R.energies(kind, site, radii, eps, None, i, j, S, cutoff=9.0, taper=8.0).sum()  # the sites as atoms: dE/dsite
    fsite = -torch.autograd.grad(e, site)[0]
    # with f_ij the force of site j on site i and d = site_j - site_i:  -sum_pairs d (x) f_ij = sum_pairs (site_i - site_j) (x) f_ij = sum_i site_i (x) F_i
    want = torch.einsum("na,nb->ab", site.detach(), fsite)
    assert float((vir - want).abs().max()) <= 1e-12 * float(want.abs().max())
