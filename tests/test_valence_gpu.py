"""`mi_valence` and the five public functions of nvalchemiops.interactions.valence on the device, against the float64 autograd reference
tests/valence_reference.py (itself pinned in tests/test_valence_reference_cpu.py).

Geometries are stretches of one stored random walk (tests/golden/valence_walk.npy; `_walk` asserts on the CPU: bond lengths in [0.9, 1.6],
bond angles in [60, 150] degrees, chi of every four consecutive atoms in [0.05, 0.6] rad for both plane types -- conditions on the inputs,
nothing the kernel relies on).  Cases: "t<T>", T terms on T + A - 1 consecutive atoms (the edges of the term pass's blocks of 256; N crosses
256 and 512 for the gather pass); "hub": 64 seven-atom stretches that share their middle atom, term k holding it in position k mod A, rows
listed last stretch first, every other group of A bonds, angles and torsions reversed, plus an atom no term names; "triclinic": 60 atoms
wrapped atom by atom into a triclinic cell, also against "whole", the unwrapped molecule evaluated WITHOUT a cell (in float32 the molecule
that the rounded wrapped inputs describe, their positions plus lattice translations: rounding a coordinate near 9 and near 0 differs by more
than the bar allows the result to); "batch": three systems with different cells and sizes, the middle one empty.  Bars are
tests/test_cluster_multipole_gpu.py::_close's: 1e-11 of the largest reference component for float64, 1e-6 for float32 at the rounded inputs.

Measured on the MI355X, largest over all cases: float64 energies <= 3.0e-15, forces <= 1.5e-15 (out-of-plane 2.5e-14), parameter gradients
and virial <= 4.5e-15, backward <= 1.3e-15, against "whole" <= 4.2e-15; float32 <= 5.6e-8 for every output; everything else bit-identical /
exact zeros.  DESIGN 3.39 has the table."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from nvalchemiops.interactions import valence as V
from tests import poison
from tests import valence_reference as VR
from tests.test_cluster_multipole_gpu import _close  # the project's bar for its fp64-arithmetic kernels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
CASES = ("t1", "t255", "t256", "t257", "t513", "hub", "triclinic", "batch")
CELLS = torch.tensor([[[9.0, 0.0, 0.0], [1.5, 8.0, 0.0], [-1.0, 2.0, 7.5]], [[12.5, 0, 0], [0, 12.5, 0], [0, 0, 12.5]],
                      [[7.0, 0.5, 0.0], [0.0, 8.5, -0.5], [1.0, 0.0, 9.5]]], dtype=F64)
CONSTS = (0.3, -0.2, 0.1, 0.05)
BAR = {F64: 1e-11, F32: 1e-6}
OUTPUTS = ("energies", "forces", "parameter_grads", "virial")
ALL = dict(compute_forces=True, compute_parameter_gradients=True)
PARITY = ([(k, n, d, 3, "wdc", None) for k in VR.KINDS for n in CASES for d in (F64, F32)] + [(k, "t257", F64, 3, "wdc", F32) for k in VR.KINDS]
          + [(k, n, d, f, p, None) for k, f, p in (("torsion", 1, "wdc"), ("torsion", 6, "wdc"), ("out_of_plane_bend", 3, "allinger"))
             for n, d in (("t257", F64), ("hub", F32))])


@functools.lru_cache(maxsize=None)
def _walk():
    pos = torch.from_numpy(np.load(os.path.join(os.path.dirname(__file__), "golden", "valence_walk.npy")))
    b = pos[1:] - pos[:-1]
    lengths = b.norm(dim=-1)
    ang = torch.rad2deg(torch.acos(-(b[1:] * b[:-1]).sum(-1) / (lengths[1:] * lengths[:-1])))
    q = torch.arange(pos.shape[0] - 3)[:, None] + torch.arange(4)
    chi = torch.cat([VR.term_energies("out_of_plane_bend", pos, q, torch.ones((q.shape[0], 1), dtype=F64), plane=p).sqrt() for p in ("wdc", "allinger")])
    assert 0.9 <= float(lengths.min()) and float(lengths.max()) <= 1.6 and 60 <= float(ang.min()) and float(ang.max()) <= 150
    assert float(torch.sin(torch.deg2rad(ang)).min()) >= 0.5 and 0.05 <= float(chi.min()) and float(chi.max()) <= 0.6
    return pos


def _wrap(pos, cell):
    frac = pos @ torch.linalg.inv(cell)
    return (frac - torch.floor(frac)) @ cell


@functools.lru_cache(maxsize=None)
def _case(kind, name, folds=3):
    """dict(pos, atoms [T, A], par [T, P], cell, batch, weights, whole) of float64 / int64 CPU tensors, parameters near the geometry's own values."""
    walk, A, cell, batch, whole = _walk(), VR.ARITY[kind], None, None, None
    win = lambda n, lo=0: lo + torch.arange(n - A + 1)[:, None] + torch.arange(A)  # noqa: E731
    if name == "hub":  # atom 0 is the middle of stretch k = walk[520 + 7 k :][:7], atoms 1 + 6 k .. are its other six, the last atom is nobody's
        arms = walk[520:].reshape(64, 7, 3)
        arms = arms - arms[:, 3:4]
        pos = torch.cat([torch.zeros((1, 3), dtype=F64), torch.cat([arms[:, :3], arms[:, 4:]], 1).reshape(-1, 3), torch.full((1, 3), 30.0, dtype=F64)])
        own = torch.arange(1, 385).reshape(64, 6)
        rows = torch.cat([own[:, :3], torch.zeros((64, 1), dtype=torch.long), own[:, 3:]], 1)
        atoms = torch.stack([rows[k, 3 - k % A:3 - k % A + A] for k in range(64)])  # term k holds the hub in position k mod A
        if kind in ("bond_stretch", "angle_bend", "torsion"):  # every other full group of A terms with its atoms reversed
            odd = torch.tensor([(k // A) % 2 == 1 and k < 64 // A * A for k in range(64)])
            atoms[odd] = atoms[odd].flip(1)
        atoms = atoms.flip(0)
        assert sorted(torch.nonzero(atoms == 0)[:, 1].tolist()) == sorted(k % A for k in range(64)) and 385 not in atoms
    elif name == "triclinic":
        whole, cell, atoms = walk[:60] + 4.0, CELLS[0], win(60)
        pos = _wrap(whole, cell)
        assert float((pos - whole).norm(dim=-1).max()) > 5.0, "the chain does not cross a face"
    elif name == "batch":
        pos, atoms, cell = torch.cat([_wrap(walk[:40] + 3.0, CELLS[0]), _wrap(walk[100:123], CELLS[2])]), torch.cat([win(40), win(23, 40)]), CELLS
        batch = torch.cat([torch.zeros(40, dtype=torch.int32), torch.full((23,), 2, dtype=torch.int32)])
    else:
        pos = walk[:int(name[1:]) + A - 1]
        atoms = win(pos.shape[0])
    T = atoms.shape[0]
    gen = torch.Generator().manual_seed(1000 + T + A)
    u = lambda *s: torch.rand(s, dtype=F64, generator=gen)  # noqa: E731
    par = {"bond_stretch": lambda: torch.cat([1 + u(T, 1), 1.1 + 0.3 * u(T, 1)], 1),
           "angle_bend": lambda: torch.cat([1 + u(T, 1), 1.7 + 0.4 * u(T, 1)], 1),
           "stretch_bend": lambda: torch.cat([0.5 + u(T, 2), 1.1 + 0.3 * u(T, 2), 1.7 + 0.4 * u(T, 1)], 1),
           "out_of_plane_bend": lambda: 1 + u(T, 1),
           "torsion": lambda: torch.cat([u(T, folds) - 0.5, 2 * math.pi * u(T, folds)], 1)}[kind]()
    return dict(pos=pos, atoms=atoms.contiguous(), par=par, cell=cell, batch=batch, weights=0.5 + u(pos.shape[0]), whole=whole)


def _model(kind, plane="wdc"):
    """(keywords of the reference, keywords of the public function): nonzero anharmonic constants wherever the kind takes them."""
    n = {"bond_stretch": 2, "angle_bend": 4, "out_of_plane_bend": 4}.get(kind, 0)
    consts = CONSTS[:n] + (0.0,) * (4 - n)
    api = dict(zip(("cubic", "quartic", "pentic", "sextic")[:n], consts))
    return dict(consts=consts, plane=plane), dict(api, plane=plane) if kind == "out_of_plane_bend" else api


@functools.lru_cache(maxsize=None)
def _reference(kind, name, dtype, folds=3, plane="wdc", par_dtype=None):
    """The float64 reference at the inputs rounded to `dtype`, computed once on the CPU and shared.  "whole": see the module docstring."""
    c = _case(kind, "triclinic" if name == "whole" else name, folds)
    r = lambda x, d=dtype: None if x is None else x.to(d).to(F64)  # noqa: E731
    pos, cell = r(c["pos"]), r(c["cell"])
    if name == "whole":  # the cell's entries are exact in float32
        pos, cell = pos + torch.round((c["whole"] - c["pos"]) @ torch.linalg.inv(c["cell"])) @ c["cell"], None
    return VR.evaluate(kind, pos, c["atoms"], r(c["par"], par_dtype or dtype), cell, c["batch"], r(c["weights"]), **_model(kind, plane)[0])


def _run(kind, c, dtype, plane="wdc", par_dtype=None, validate=True, **flags):
    dev = lambda x, d=None: None if x is None else x.to(DEV, d)  # noqa: E731
    terms = V.ValenceTerms(dev(c["atoms"]), c["pos"].shape[0], batch_idx=dev(c["batch"]), validate=validate)
    return getattr(V, kind)(dev(c["pos"], dtype), terms, dev(c["par"], par_dtype or dtype), dev(c["cell"], dtype), batch_idx=dev(c["batch"]),
                            **_model(kind, plane)[1], **flags)


@pytest.mark.parametrize("kind,name,dtype,folds,plane,par_dtype", PARITY)
def test_parity(kind, name, dtype, folds, plane, par_dtype):
    c = _case(kind, name, folds)
    got = _run(kind, c, dtype, plane, par_dtype, compute_virial=c["cell"] is not None, **ALL)
    for ref_name in (name, "whole")[:2 if name == "triclinic" else 1]:
        ref = _reference(kind, ref_name, dtype, folds, plane, par_dtype)
        for what, g in zip(OUTPUTS, got):
            if ref[what] is not None:  # the cluster "whole" has no virial
                assert g.dtype == dtype
                _close(g, ref[what], f"{kind} {name} {what} against {ref_name}", BAR[dtype])


@pytest.mark.parametrize("kind", VR.KINDS)
def test_unvalidated_index_outside_the_table_is_an_exact_zero(kind):
    c = _case(kind, "t257")
    keep = torch.arange(257) != 100
    want = _run(kind, dict(c, atoms=c["atoms"][keep], par=c["par"][keep]), F64, **ALL)
    for bad in (c["pos"].shape[0], -1):
        atoms = c["atoms"].clone()
        atoms[100, 1] = bad
        e, f, pg = _run(kind, dict(c, atoms=atoms), F64, validate=False, **ALL)
        assert torch.equal(e, want[0]) and torch.equal(f, want[1]) and torch.equal(pg[keep.to(DEV)], want[2])
        assert torch.equal(pg[100], torch.zeros_like(pg[100]))


@pytest.mark.parametrize("plane", ["wdc", "allinger"])
def test_planar_centre_is_an_exact_zero(plane):
    pos = torch.tensor([[1.0, 0, 0], [0, 0, 0], [0, 1.2, 0], [-0.9, -1.1, 0]], dtype=F64)
    e, f = _run("out_of_plane_bend", dict(pos=pos, atoms=torch.arange(4)[None], par=torch.ones((1, 1), dtype=F64), cell=None, batch=None), F64, plane,
                compute_forces=True)
    assert torch.equal(e, torch.zeros_like(e)) and torch.equal(f, torch.zeros_like(f))


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["hub", "batch"])
@pytest.mark.parametrize("kind", VR.KINDS)
def test_autograd(kind, name, dtype):
    c, ref = _case(kind, name), _reference(kind, name, dtype)
    pos, par = c["pos"].to(DEV, dtype).requires_grad_(True), c["par"].to(DEV, dtype).requires_grad_(True)
    cell, batch = (None if c[k] is None else c[k].to(DEV) for k in ("cell", "batch"))
    terms = V.ValenceTerms(c["atoms"].to(DEV), pos.shape[0])
    fn = lambda **kw: getattr(V, kind)(pos, terms, par, None if cell is None else cell.to(dtype), batch_idx=batch, **_model(kind)[1], **kw)  # noqa: E731
    for weights, wants in ((None, (-ref["forces"], ref["parameter_grads"])), (c["weights"].to(DEV, dtype), (ref["positions_grad"], ref["parameters_grad"]))):
        pos.grad = par.grad = None
        (fn() if weights is None else weights * fn()).sum().backward()
        _close(pos.grad, wants[0], f"{kind} {name} positions.grad, weights {weights is not None}", BAR[dtype])
        _close(par.grad, wants[1], f"{kind} {name} parameters.grad, weights {weights is not None}", BAR[dtype])
    with pytest.raises(NotImplementedError, match="second derivatives"):
        fn(compute_forces=True)[1].sum().backward()


@pytest.mark.parametrize("kind", VR.KINDS)
def test_reproducible_and_poisoned(kind, request):
    c = _case(kind, "batch")
    run = lambda: _run(kind, c, F64, compute_virial=True, **ALL)  # noqa: E731
    first = run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = run()
    side.synchronize()
    compiled = torch.compile(lambda pos, terms, par, cell, batch: getattr(V, kind)(
        pos, terms, par, cell, batch_idx=batch, compute_virial=True, **_model(kind)[1], **ALL), fullgraph=True)
    dev = lambda x: x.to(DEV)  # noqa: E731
    traced = compiled(dev(c["pos"]), V.ValenceTerms(dev(c["atoms"]), c["pos"].shape[0]), dev(c["par"]), dev(c["cell"]), dev(c["batch"]))
    with poison.poisoned_case(request.node.nodeid):
        poisoned = run()
    for other in (run(), on_side, traced, poisoned):
        assert all(torch.equal(a, b) for a, b in zip(first, other))
