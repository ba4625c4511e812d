"""`stretch_torsion`, `angle_torsion`, `pi_torsion` and `torsion_torsion` on the device against tests/coupled_torsion_reference.py, on stretches of
the stored walk; `_case` builds the cases and asserts the conditions on its inputs.  Bars: tests/test_cluster_multipole_gpu.py::_close.

Measured on the MI355X, largest over all cases: float64 energies <= 2.4e-15, forces <= 1.6e-14 (torsion_torsion; the others <= 8.2e-16),
parameter gradients <= 6.7e-16, virial <= 8.9e-15, backward <= 3.2e-15, against the whole molecule <= 7.7e-15; float32 <= 5.6e-8 everywhere."""
import functools
import math

import pytest
import torch

from nvalchemiops.interactions import valence as V
from tests import coupled_torsion_reference as CR
from tests import poison
from tests.test_cluster_multipole_gpu import _close  # the project's bar for its fp64-arithmetic kernels
from tests.test_valence_gpu import CELLS, _walk, _wrap

pytestmark = pytest.mark.gpu
DEV, F64, F32, TT = "cuda:0", torch.float64, torch.float32, "torsion_torsion"
BAR = {F64: 1e-11, F32: 1e-6}  # of the largest reference component; float32 at the rounded inputs
PARITY = ([(k, n, d, (24, 24)) for k in CR.KINDS for n in ("t1", "t257", "hub", "triclinic", "batch") for d in (F64, F32)]
          + [(TT, "t257", F64, (12, 16)), (TT, "hub", F32, (12, 16))] + [(TT, z, F64, g) for z in ("zigzag+", "zigzag-") for g in ((24, 24), (12, 16))])


def _maps(grid):  # two smooth maps, neither a product of functions of one angle
    x, y = torch.meshgrid(*(-math.pi + 2 * math.pi * torch.arange(n, dtype=F64) / n for n in grid), indexing="ij")
    return torch.stack([torch.sin(x + 0.3) * torch.cos(2 * y) + 0.5 * torch.cos(x - y + 0.7), torch.cos(x + 2 * y) - 0.4 * torch.sin(2 * x - 0.2)])


@functools.lru_cache(maxsize=None)
def _case(kind, name):
    """The inputs of a case on the CPU.  "t1"; "t257": two term blocks, N crosses 256; "hub": atom 0 sits in position k mod A of term k, rows listed
    last first, the last atom is nobody's; "triclinic": wrapped atom by atom (`whole`: the unwrapped molecule); "batch": three systems, the middle
    one empty; "zigzag+-": planar, phi_1 = +-pi (the seam), phi_2 = +-0 (a node) exactly.  Map and sign alternate with the term and every second term."""
    walk, A, cell, batch, whole = _walk(), CR.ARITY[kind], None, None, None
    win = lambda n, lo=0: lo + torch.arange(n - A + 1)[:, None] + torch.arange(A)  # noqa: E731
    if name == "hub":
        spot = torch.arange(24) % A
        arms, others = walk[300:300 + 24 * A].reshape(24, A, 3), torch.arange(A)[None] != spot[:, None]
        pos = torch.cat([torch.zeros((1, 3), dtype=F64), (arms - arms[torch.arange(24), spot][:, None])[others], torch.full((1, 3), 30.0, dtype=F64)])
        atoms = torch.zeros((24, A), dtype=torch.long)
        atoms[others] = torch.arange(1, 1 + 24 * (A - 1))
    elif name == "triclinic":
        whole, cell, atoms, pos = walk[:60] + 4.0, CELLS[0], win(60), _wrap(walk[:60] + 4.0, CELLS[0])
        assert float((pos - whole).norm(dim=-1).max()) > 5.0, "the chain does not cross a face"
    elif name == "batch":
        pos, atoms, cell = torch.cat([_wrap(walk[:40] + 3.0, CELLS[0]), _wrap(walk[100:123], CELLS[2])]), torch.cat([win(40), win(23, 40)]), CELLS
        batch, whole = torch.cat([torch.zeros(40, dtype=torch.int32), torch.full((23,), 2, dtype=torch.int32)]), torch.cat([walk[:40], walk[100:123]])
    elif name.startswith("zigzag"):
        pos = torch.tensor([[-0.5, 1.2, 0], [0, 0, 0], [1.5, 0, 0], [2.0, -1.2, 0], [0.6, -1.5, 0]], dtype=F64)
        atoms, b = win(5), pos[1:] - pos[:-1]
        assert abs(float(CR._dihedral(b[0], b[1], b[2]))) == math.pi and float(CR._dihedral(b[1], b[2], b[3])) == 0.0
    else:
        pos, atoms = walk[:int(name[1:]) + A - 1], win(int(name[1:]) + A - 1)
    r = (pos if whole is None else whole)[atoms]  # the conditions on the inputs, on the unwrapped molecule
    v = torch.stack([r[:, 0] - r[:, 3], r[:, 1] - r[:, 3], r[:, 4] - r[:, 2], r[:, 5] - r[:, 2], r[:, 3] - r[:, 2]], 1) if A == 6 else r[:, 1:] - r[:, :-1]
    normals = torch.stack([-torch.linalg.cross(v[:, 0], v[:, 1]), v[:, 4], torch.linalg.cross(v[:, 2], v[:, 3])], 1) if A == 6 else v
    assert min(float(torch.linalg.cross(normals[:, :-1], normals[:, 1:]).norm(dim=-1).min()), float(normals.norm(dim=-1).min())) >= 0.05, "pick another window"
    if cell is not None:
        cells = cell.reshape(-1, 3, 3)[batch.long()[atoms[:, 0]] if batch is not None else torch.zeros(atoms.shape[0], dtype=torch.long)]
        assert float(torch.einsum("tvk,tkc->tvc", v, torch.linalg.inv(cells)).abs().max()) <= 0.45
    T, gen = atoms.shape[0], torch.Generator().manual_seed(2000 + atoms.shape[0] + A)
    u = lambda *s: torch.rand(s, dtype=F64, generator=gen)  # noqa: E731
    par = {"stretch_torsion": lambda: torch.cat([u(T, 9) - 0.5, 1.1 + 0.3 * u(T, 3), 2 * math.pi * u(T, 3)], 1),
           "angle_torsion": lambda: torch.cat([u(T, 6) - 0.5, 1.7 + 0.4 * u(T, 2), 2 * math.pi * u(T, 3)], 1),
           "pi_torsion": lambda: 1 + u(T, 1), TT: lambda: None}[kind]()
    k = torch.arange(T)  # (the rows of the hub are listed last first)
    return dict(pos=pos, atoms=(atoms.flip(0) if name == "hub" else atoms).contiguous(), par=par, cell=cell, batch=batch, weights=0.5 + u(pos.shape[0]), whole=whole,
                map_index=k % 2, signs=(1 - 2 * ((k // 2) % 2)).to(F64) * (-1.0 if name == "zigzag-" else 1.0))


@functools.lru_cache(maxsize=None)
def _reference(kind, name, dtype, grid=(24, 24), whole=False):
    c = _case(kind, name)
    r = lambda x: None if x is None else x.to(dtype).to(F64)  # noqa: E731
    pos, cell = r(c["pos"]), r(c["cell"])
    if whole:
        pos, cell = pos + torch.round((c["whole"] - c["pos"]) @ torch.linalg.inv(c["cell"])) @ c["cell"], None
    return CR.evaluate(kind, pos, c["atoms"], r(c["par"]), cell, c["batch"], r(c["weights"]),
                       **(dict(maps=_maps(grid), map_index=c["map_index"], signs=c["signs"]) if kind == TT else {}))


def _run(kind, c, dtype, grid=(24, 24), validate=True, call=True, **flags):  # the public function on the device; `call=False`: its arguments
    dev = lambda x, d=None: None if x is None else x.to(DEV, d)  # noqa: E731
    batch, table = dev(c["batch"]), V.TorsionTorsionTerms if kind == TT else V.WideValenceTerms if CR.ARITY[kind] > 4 else V.ValenceTerms
    more = dict(batch_idx=batch, validate=validate, **(dict(signs=dev(c["signs"])) if kind == TT else {}))
    terms = table(dev(c["atoms"]), *([dev(c["map_index"])] if kind == TT else []), c["pos"].shape[0], **more)
    third = V.TorsionTorsionMaps(dev(_maps(grid))) if kind == TT else dev(c["par"], dtype)
    args, kw = (dev(c["pos"], dtype), terms, third, dev(c["cell"], dtype)), dict(batch_idx=batch, **({} if kind == TT else dict(compute_parameter_gradients=True)))
    return getattr(V, kind)(*args, **kw, compute_forces=True, **flags) if call else (args, kw)


@pytest.mark.parametrize("kind,name,dtype,grid", PARITY)
def test_parity(kind, name, dtype, grid, request):
    c = _case(kind, name)
    got = _run(kind, c, dtype, grid, compute_virial=c["cell"] is not None)
    names = ("energies", "forces") + (() if kind == TT else ("parameter_grads",)) + ("virial",)
    for whole in (False, True)[:2 if name == "triclinic" else 1]:
        ref = _reference(kind, name, dtype, grid, whole)
        for what, g in zip(names, got):
            if ref[what] is not None:  # the cluster has no virial
                assert g.dtype == dtype
                _close(g, ref[what], f"{kind} {name} {what}, whole {whole}", BAR[dtype])
    if (name, dtype) == ("batch", F64):  # a second call, a compiled call and a call on poisoned scratch give the same bits
        args, kw = _run(kind, c, dtype, grid, call=False)
        compiled = torch.compile(getattr(V, kind), fullgraph=True)(*args, **kw, compute_forces=True, compute_virial=True)
        with poison.poisoned_case(request.node.nodeid):
            poisoned = _run(kind, c, dtype, grid, compute_virial=True)
        assert all(torch.equal(a, b) for other in (_run(kind, c, dtype, grid, compute_virial=True), compiled, poisoned) for a, b in zip(got, other))


@pytest.mark.parametrize("kind", CR.KINDS)
def test_unvalidated_index_outside_the_table_is_an_exact_zero(kind):
    c, keep = _case(kind, "t257"), torch.arange(257) != 100
    want = _run(kind, {k: v[keep] if k in ("atoms", "par", "map_index", "signs") and v is not None else v for k, v in c.items()}, F64)
    for key, where, bads in (("atoms", (100, 1), (c["pos"].shape[0], -1)), ("map_index", (100,), (2, -1)))[:2 if kind == TT else 1]:
        for bad in bads:
            broken = c[key].index_put(tuple(torch.tensor(w) for w in where), torch.tensor(bad))
            got = _run(kind, dict(c, **{key: broken}), F64, validate=False)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
            assert kind == TT or (torch.equal(got[2][keep.to(DEV)], want[2]) and not got[2][100].any())


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["hub", "batch"])
@pytest.mark.parametrize("kind", CR.KINDS)
def test_autograd(kind, name, dtype):
    c, ref = _case(kind, name), _reference(kind, name, dtype)
    (pos, terms, third, cell), kw = _run(kind, c, dtype, call=False)
    leaves = [pos.requires_grad_(True)] + ([] if kind == TT else [third.requires_grad_(True)])
    fn = lambda **flags: getattr(V, kind)(pos, terms, third, cell, batch_idx=kw["batch_idx"], **flags)  # noqa: E731
    for weights, wants in ((None, (-ref["forces"], ref["parameter_grads"])), (c["weights"].to(DEV, dtype), (ref["positions_grad"], ref["parameters_grad"]))):
        grads = torch.autograd.grad((fn() if weights is None else weights * fn()).sum(), leaves)
        for g, want, what in zip(grads, wants, ("positions", "parameters")):
            _close(g, want, f"{kind} {name} {what}.grad, weights {weights is not None}", BAR[dtype])
    with pytest.raises(NotImplementedError, match="second derivatives"):
        fn(compute_forces=True)[1].sum().backward()
