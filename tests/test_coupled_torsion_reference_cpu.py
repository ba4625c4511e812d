"""Pins tests/coupled_torsion_reference.py by properties and closed forms, and checks the new table and argument errors by message."""
import math

import pytest
import torch

from nvalchemiops.interactions.valence import (TorsionTorsionMaps, TorsionTorsionTerms, ValenceTerms, WideValenceTerms, angle_torsion, pi_torsion,
                                               stretch_torsion, torsion_torsion)
from tests import coupled_torsion_reference as CR
from tests import valence_reference as VR

F64 = torch.float64
T = lambda rows: torch.tensor(rows, dtype=F64)  # noqa: E731
GRID = torch.meshgrid(-math.pi + 2 * math.pi * torch.arange(24, dtype=F64) / 24, -math.pi + 2 * math.pi * torch.arange(16, dtype=F64) / 16, indexing="ij")
SMOOTH = (torch.sin(GRID[0] + 0.3) * torch.cos(2 * GRID[1]) + 0.5 * torch.cos(GRID[0] - GRID[1] + 0.7))[None]  # [1, 24, 16], not separable
FIVE, ONE = torch.arange(5)[None], torch.tensor([0])


def test_interpolant_reproduces_the_nodes_and_is_c1():
    f, f1, f2, f12 = CR.node_records(SMOOTH)
    x, y = (g.reshape(-1).clone().requires_grad_(True) for g in GRID)
    F = CR.bicubic(SMOOTH, torch.zeros(x.shape[0]), x, y)
    Fx, Fy = torch.autograd.grad(F.sum(), (x, y), create_graph=True)
    for got, want in ((F, f), (Fx, f1), (Fy, f2), (torch.autograd.grad(Fx.sum(), y)[0], f12)):
        assert torch.allclose(got.detach(), want.reshape(-1), atol=1e-13)
    edge, d = -math.pi + 5 * 2 * math.pi / 24, 1e-9  # pairs of points on either side of a cell edge and of the seam at +-pi, in both directions
    x, y = T([edge - d, edge + d, 0.7, 0.7, math.pi - d, -math.pi + d]).requires_grad_(True), T([0.4, 0.4, math.pi - d, -math.pi + d, 0.4, 0.4]).requires_grad_(True)
    F = CR.bicubic(SMOOTH, torch.zeros(6), x, y)
    sides = torch.stack([F.detach(), *torch.autograd.grad(F.sum(), (x, y))])
    assert torch.allclose(sides[:, 0::2], sides[:, 1::2], atol=1e-7)  # value and gradient; second derivatives are O(1), the step 2e-9


@pytest.mark.parametrize("kind,row,col", [("stretch_torsion", 0, 1), ("stretch_torsion", 2, 2), ("angle_torsion", 1, 0)])
def test_one_coupling_constant_is_a_torsion_times_its_coordinate(kind, row, col):
    rows = 3 if kind == "stretch_torsion" else 2
    pos, atoms = T([[0.1, 1.2, 0.0], [0, 0, 0], [1.4, 0.1, 0], [1.9, 0.8, 0.9]]), torch.arange(4)[None]
    par, tors = torch.zeros((1, 4 * rows + 3), dtype=F64), torch.zeros((1, 6), dtype=F64)
    par[0, 3 * row + col], par[0, 3 * rows + row], par[0, 4 * rows + col] = 0.8, 0.7, 0.3
    tors[0, col], tors[0, 3 + col] = 0.8, 0.3
    b = pos[1:] - pos[:-1]
    coord = b[row].norm() if rows == 3 else VR._angle(-b[row], b[row + 1])
    assert torch.allclose(CR.term_energies(kind, pos, atoms, par), (coord - 0.7) * VR.term_energies("torsion", pos, atoms, tors), atol=1e-14)


@pytest.mark.parametrize("twist,want", [(0.0, 0.0), (math.pi / 2, 2 * 1.7)])
def test_pi_torsion_of_a_twisted_ethylene(twist, want):
    c, s = math.cos(twist), math.sin(twist)  # a, b on c and e, f on d; the CH2 group of d turned about the c-d bond
    pos = T([[-0.5, 0.9, 0], [-0.5, -0.9, 0], [0, 0, 0], [1.3, 0, 0], [1.8, 0.9 * c, 0.9 * s], [1.8, -0.9 * c, -0.9 * s]])
    assert abs(float(CR.term_energies("pi_torsion", pos, torch.arange(6)[None], T([[1.7]]))) - want) < 1e-14


@pytest.mark.parametrize("error,build,message", [
    (ValueError, lambda: WideValenceTerms(torch.zeros((1, 4), dtype=torch.long), 5), r"atoms must have shape \[num_terms, A\] with A = 5 or 6"),
    (ValueError, lambda: TorsionTorsionTerms(FIVE, torch.tensor([-1]), 5), "term 0: map_index -1 is negative"),
    (ValueError, lambda: TorsionTorsionTerms(FIVE, ONE, 5, signs=torch.tensor([0.5])), r"term 0: sign 0.5 is not \+1 or -1"),
    (ValueError, lambda: TorsionTorsionMaps(torch.zeros(1, 2, 24)), "at least one map of at least 3 x 3 nodes"),
    (ValueError, lambda: torsion_torsion(torch.zeros(5, 3), TorsionTorsionTerms(FIVE, torch.tensor([1]), 5), TorsionTorsionMaps(SMOOTH)), "terms name map 1 but maps holds 1"),
    (ValueError, lambda: pi_torsion(torch.zeros(6, 3), ValenceTerms(torch.arange(4)[None], 6), torch.zeros(1, 1)), "pi_torsion takes terms of 6 atoms, got a table of 4"),
    (ValueError, lambda: stretch_torsion(torch.zeros(4, 3), ValenceTerms(torch.arange(4)[None], 4), torch.zeros(1, 11)), "stretch_torsion takes 15 parameters per term, got P = 11"),
    (ValueError, lambda: angle_torsion(torch.zeros(4, 3), ValenceTerms(torch.arange(4)[None], 4), torch.zeros(1, 15)), "angle_torsion takes 11 parameters per term, got P = 15"),
    (TypeError, lambda: torsion_torsion(torch.zeros(5, 3), WideValenceTerms(FIVE, 5), TorsionTorsionMaps(SMOOTH)), "terms must be a TorsionTorsionTerms"),
])
def test_errors(error, build, message):
    with pytest.raises(error, match=message):
        build()
    assert torsion_torsion(torch.rand(0, 3), TorsionTorsionTerms(FIVE[:0], ONE[:0], 0), TorsionTorsionMaps(SMOOTH)).shape == (0,)
