"""Pins tests/valence_reference.py by closed forms, and checks what `nvalchemiops.interactions.valence` does on the host: the CSR of
`ValenceTerms`, every ValueError of the container and of the five functions by message, NativeLibraryError on CPU tensors."""
import math

import pytest
import torch

from nvalchemiops._capi import NativeLibraryError
from nvalchemiops.interactions import valence as V
from tests import valence_reference as VR

F64 = torch.float64
T = lambda rows: torch.tensor(rows, dtype=F64)  # noqa: E731
C = (0.3, -0.2, 0.1, 0.05)
poly = lambda D, k, c=C: k * D ** 2 * (1 + c[0] * D + c[1] * D ** 2 + c[2] * D ** 3 + c[3] * D ** 4)  # noqa: E731
H = 0.4  # height of the pyramid's apex over the plane of a, b, c


def _butane(phi):
    """a-b-c-d with unit bonds, right bond angles and dihedral phi (IUPAC: trans = pi)."""
    return T([[0, 1, 0], [0, 0, 0], [1, 0, 0], [1, math.cos(phi), math.sin(phi)]])


CLOSED = [  # kind, positions, parameters, model, expected E_t
    ("bond_stretch", [[0, 0, 0], [0, 0, 1.3]], [2.0, 1.1], dict(consts=(0.3, -0.2, 0, 0)), poly(0.2, 2.0, (0.3, -0.2, 0, 0))),
    ("angle_bend", [[2, 0, 0], [0, 0, 0], [0, 3, 0]], [1.5, 1.2], dict(consts=C), poly(math.pi / 2 - 1.2, 1.5)),
    ("stretch_bend", [[2, 0, 0], [0, 0, 0], [0, 3, 0]], [0.7, 0.9, 1.5, 2.5, 1.2], {}, (0.7 * 0.5 + 0.9 * 0.5) * (math.pi / 2 - 1.2)),
    ("out_of_plane_bend", [[1, 0, 0], [0, 0, 0], [0, 1, 0], [-1, -1, 0]], [3.0], dict(plane="wdc"), 0.0),
    ("out_of_plane_bend", [[1, 0, 0], [0, 0, 0], [0, 1, 0], [-1, -1, 0]], [3.0], dict(plane="allinger"), 0.0),
    ("out_of_plane_bend", [[1, 0, 0], [0, 0, 0], [0, 1, 0], [-1, -1, H]], [3.0], dict(plane="wdc", consts=C), poly(math.asin(H / math.sqrt(2 + H * H)), 3.0)),
    ("torsion", _butane(math.pi), [1.0, 0.5, 0.0, 0.0], {}, 1.0 * (1 - 1) + 0.5 * (1 + 1)),
    ("torsion", _butane(0.0), [1.0, 0.5, 0.0, 0.0], {}, 1.0 * 2 + 0.5 * 2),
    ("torsion", _butane(math.pi / 3), [1.0, 0.5, 0.2, 0.3], {}, 1 + math.cos(math.pi / 3 - 0.2) + 0.5 * (1 + math.cos(2 * math.pi / 3 - 0.3))),
    ("torsion", _butane(-math.pi / 3), [1.0, 0.0, 0.2, 0.0], {}, 1 + math.cos(-math.pi / 3 - 0.2)),
]


@pytest.mark.parametrize("kind,pos,par,model,want", CLOSED, ids=[f"{i}-{c[0]}" for i, c in enumerate(CLOSED)])
def test_reference_closed_forms(kind, pos, par, model, want):
    pos, par = torch.as_tensor(pos, dtype=F64), T([par])
    atoms = torch.arange(VR.ARITY[kind])[None]
    got = VR.evaluate(kind, pos, atoms, par, **model)
    assert abs(float(got["energies"].sum()) - want) <= 1e-14 * max(1.0, abs(want))
    assert torch.allclose(got["energies"], torch.full_like(got["energies"], want / VR.ARITY[kind]), atol=1e-15)
    assert float(got["forces"].sum(0).abs().max()) <= 1e-13  # no net force
    cell = torch.eye(3, dtype=F64) * 20.0  # the same molecule across a face of a cell, with the virial = -sum_i dE/dr_i (x) r_i of a cluster
    moved = pos.clone()
    moved[0] += cell[0]
    per = VR.evaluate(kind, moved, atoms, par, cell=cell, **model)
    assert torch.allclose(per["energies"], got["energies"], atol=1e-14) and torch.allclose(per["forces"], got["forces"], atol=1e-13)
    assert torch.allclose(per["virial"][0], torch.einsum("np,nq->pq", got["forces"], pos), atol=1e-13)


def test_reference_bond_force_and_fold_truncation():
    got = VR.evaluate("bond_stretch", T([[0, 0, 0], [0, 0, 1.3]]), torch.tensor([[0, 1]]), T([[2.0, 1.1]]))
    assert torch.allclose(got["forces"], T([[0, 0, 0.8], [0, 0, -0.8]]), atol=1e-14)  # -dE/dr = -2 k D along the bond
    assert torch.allclose(got["parameter_grads"], T([[0.04, -0.8]]), atol=1e-14)
    pos, atoms = _butane(1.1), torch.arange(4)[None]
    one = VR.evaluate("torsion", pos, atoms, T([[0.8, 0.4]]))
    six = VR.evaluate("torsion", pos, atoms, T([[0.8, 0, 0, 0, 0, 0, 0.4, 0.1, 0.2, 0.3, 0.4, 0.5]]))
    assert torch.equal(one["forces"], six["forces"]) and torch.equal(one["energies"], six["energies"])


def test_valence_terms_csr():
    terms = V.ValenceTerms(torch.tensor([[2, 0, 1], [3, 2, 0], [1, 2, 4]]), 6)
    assert (terms.num_terms, terms.arity, terms.num_atoms, terms.device.type) == (3, 3, 6, "cpu")
    assert terms.slot_ptr.tolist() == [0, 2, 4, 7, 8, 9, 9] and terms.slot_idx.tolist() == [1, 5, 2, 6, 0, 4, 7, 3, 8]
    assert terms.atoms.dtype == terms.slot_ptr.dtype == terms.slot_idx.dtype == torch.int32 and terms.atoms.is_contiguous()
    loose = V.ValenceTerms(torch.tensor([[0, 6], [1, 0], [-1, 1]]), 2, validate=False)  # slots of indices outside [0, N) are left out
    assert loose.slot_ptr.tolist() == [0, 2, 4] and loose.slot_idx.tolist() == [0, 3, 2, 5]
    assert "num_terms=3" in repr(terms) and "arity=3" in repr(terms) and terms.to("cpu").slot_idx.tolist() == terms.slot_idx.tolist()


@pytest.mark.parametrize("atoms,n,batch,message", [
    ([[0, 1], [1, 5]], 5, None, r"term 1: atom index 5 is outside \[0, 5\)"),
    ([[0, 1], [-1, 2]], 5, None, r"term 1: atom index -1 is outside \[0, 5\)"),
    ([[0, 1, 2], [3, 4, 3]], 5, None, r"term 1: an atom appears twice in \[3, 4, 3\]"),
    ([[0, 1], [1, 2]], 3, [0, 0, 1], r"term 1: its atoms \[1, 2\] are in different systems \[0, 1\]"),
    ([[0, 1, 2, 3, 4]], 5, None, r"atoms must have shape \[num_terms, A\] with A = 2, 3 or 4"),
    ([[0.0, 1.0]], 5, None, r"atoms must be an int32 \(or int64\) tensor"),
])
def test_valence_terms_errors(atoms, n, batch, message):
    with pytest.raises(ValueError, match=message):
        V.ValenceTerms(torch.tensor(atoms), n, batch_idx=None if batch is None else torch.tensor(batch))


@pytest.mark.parametrize("name,arity,shape,kwargs,message", [
    ("bond_stretch", 3, (2, 2), {}, "bond_stretch takes terms of 2 atoms, got a table of 3"),
    ("angle_bend", 3, (2, 3), {}, "angle_bend takes 2 parameters per term, got P = 3"),
    ("stretch_bend", 3, (3, 5), {}, r"parameters must have shape \[2, P\]"),
    ("out_of_plane_bend", 4, (2, 1), dict(plane="teepee"), "unknown plane 'teepee'"),
    ("torsion", 4, (2, 5), {}, "P = 2 F with F in 1..6, got P = 5"),
    ("torsion", 4, (2, 14), {}, "P = 2 F with F in 1..6, got P = 14"),
    ("torsion", 4, (2, 2), dict(compute_virial=True), "compute_virial needs a cell"),
    ("torsion", 4, (2, 2), dict(cell=torch.zeros(2, 3, 3)), "cell holds 2 systems: batch_idx is required"),
])
def test_function_errors(name, arity, shape, kwargs, message):
    terms = V.ValenceTerms(torch.arange(2 * arity).reshape(2, arity), 8)
    with pytest.raises(ValueError, match=message):
        getattr(V, name)(torch.zeros(8, 3), terms, torch.zeros(shape), **kwargs)
    with pytest.raises(ValueError, match="terms describes 8 atoms but positions has 9"):
        getattr(V, name)(torch.zeros(9, 3), terms, torch.zeros(shape))


@pytest.mark.parametrize("name", VR.KINDS)
def test_cpu_tensors_raise(name):
    A = VR.ARITY[name]
    terms = V.ValenceTerms(torch.arange(A)[None], 4)
    P = {"bond_stretch": 2, "angle_bend": 2, "stretch_bend": 5, "out_of_plane_bend": 1, "torsion": 4}[name]
    with pytest.raises(NativeLibraryError):
        getattr(V, name)(torch.rand(4, 3), terms, torch.ones(1, P))
    assert getattr(V, name)(torch.rand(0, 3), V.ValenceTerms(torch.zeros((0, A), dtype=torch.int64), 0), torch.ones(0, P)).shape == (0,)
