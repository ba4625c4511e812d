"""`buffered_14_7`, `lennard_jones` and `ReducedSites`: what can be checked without a GPU -- every argument error of `vdw/pair.py::_check`,
of the `ReducedSites` constructor and of its `_validate` by message (all raised before anything is launched), the `compute_virial` rules, the
returns for N = 0 and for a list without entries with their shapes and dtypes, and the absence of a CPU path."""
import pytest
import torch

from nvalchemiops import _capi as C
from nvalchemiops.interactions import ReducedSites, buffered_14_7, lennard_jones

FNS = [buffered_14_7, lennard_jones]
I32 = torch.int32


def _args(n=4, m=6):
    """positions, radii, epsilons, cell, and a matrix of padding only with its shifts."""
    return torch.rand(n, 3), torch.rand(n) + 1, torch.rand(n) + 0.1, torch.eye(3)[None] * 10, torch.full((n, m), n, dtype=I32), torch.zeros((n, m, 3), dtype=I32)


@pytest.mark.parametrize("fn", FNS)
def test_model_errors(fn):
    pos, radii, eps, cell, nm, sh = _args()
    ok = dict(cutoff=4.0, neighbor_matrix=nm)
    with pytest.raises(ValueError, match="unknown radius_rule 'harmonic': expected one of"):
        fn(pos, radii, eps, **ok, radius_rule="harmonic")
    with pytest.raises(ValueError, match="unknown epsilon_rule 'arithmetic': expected one of"):
        fn(pos, radii, eps, **ok, epsilon_rule="arithmetic")
    with pytest.raises(ValueError, match=r"positions must have shape \[num_atoms, 3\]"):
        fn(pos[:, :2], radii, eps, **ok)
    for name, bad in (("radii", (radii[:3], eps)), ("epsilons", (radii, eps[:3])), ("radii", (radii[:, None], eps)), ("radii", (1.5, eps))):
        with pytest.raises(ValueError, match=rf"{name} must have one entry per atom: expected shape \[4\]"):
            fn(pos, *bad, **ok)
    for cutoff in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="cutoff must be positive"):
            fn(pos, radii, eps, cutoff=cutoff, neighbor_matrix=nm)
    for taper in (0.0, 4.0, 5.0, -1.0):
        with pytest.raises(ValueError, match=r"taper must lie inside \(0, cutoff = 4.0\)"):
            fn(pos, radii, eps, **ok, taper=taper)
    with pytest.raises(TypeError, match="sites must be a ReducedSites"):
        fn(pos, radii, eps, **ok, sites=(torch.zeros(4, dtype=I32), torch.ones(4)))
    with pytest.raises(ValueError, match="sites describes 3 atoms but positions has 4"):
        fn(pos, radii, eps, **ok, sites=ReducedSites(torch.full((3,), -1, dtype=I32), torch.ones(3)))
    with pytest.raises(TypeError):  # cutoff and the lists are keyword-only
        fn(pos, radii, eps, None, 4.0)


def test_delta_and_gamma_must_be_positive():
    pos, radii, eps, cell, nm, sh = _args()
    for kw in (dict(delta=0.0), dict(gamma=0.0), dict(delta=-0.07), dict(gamma=float("nan"))):
        with pytest.raises(ValueError, match="delta and gamma must be positive"):
            buffered_14_7(pos, radii, eps, cutoff=4.0, neighbor_matrix=nm, **kw)
    with pytest.raises(TypeError):  # Lennard-Jones has no buffers
        lennard_jones(pos, radii, eps, cutoff=4.0, neighbor_matrix=nm, delta=0.07)


@pytest.mark.parametrize("fn", FNS)
def test_pair_scale_errors(fn):
    pos, radii, eps, cell, nm, sh = _args()
    lst, ptr = torch.zeros((2, 3), dtype=I32), torch.zeros(5, dtype=I32)
    for bad in (torch.zeros(4, 5), torch.zeros(24), torch.zeros(3, 6)):
        with pytest.raises(ValueError, match=r"pair_scales must have the shape of the index array \[4, 6\]"):
            fn(pos, radii, eps, cutoff=4.0, neighbor_matrix=nm, pair_scales=bad)
    for bad in (torch.zeros(2), torch.zeros(2, 3)):
        with pytest.raises(ValueError, match=r"pair_scales must have the shape of the index array \[3\]"):
            fn(pos, radii, eps, cutoff=4.0, neighbor_list=lst, neighbor_ptr=ptr, pair_scales=bad)
    for bad in (torch.zeros(4, 6, dtype=I32), torch.zeros(4, 6).half()):
        with pytest.raises(ValueError, match="pair_scales must be float32 or float64"):
            fn(pos, radii, eps, cutoff=4.0, neighbor_matrix=nm, pair_scales=bad)


@pytest.mark.parametrize("fn", FNS)
def test_list_errors_and_the_virial_rules(fn):
    pos, radii, eps, cell, nm, sh = _args()
    lst, ptr = torch.zeros((2, 3), dtype=I32), torch.zeros(5, dtype=I32)
    with pytest.raises(ValueError, match="Either neighbor_list or neighbor_matrix must be provided"):
        fn(pos, radii, eps, cutoff=4.0)
    with pytest.raises(ValueError, match="neighbor_ptr is required"):
        fn(pos, radii, eps, cutoff=4.0, neighbor_list=lst)
    with pytest.raises(ValueError, match="neighbor shifts need a cell"):
        fn(pos, radii, eps, cutoff=4.0, neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    with pytest.raises(ValueError, match="compute_virial needs a cell"):  # a cluster has no virial
        fn(pos, radii, eps, cutoff=4.0, neighbor_matrix=nm, compute_virial=True)
    with pytest.raises(ValueError, match=r"neighbor_matrix must have shape \[4, max_neighbors\]"):
        fn(pos, radii, eps, cell, cutoff=4.0, neighbor_matrix=nm[:3])
    with pytest.raises(ValueError, match=r"neighbor_ptr must have shape \[5\]"):
        fn(pos, radii, eps, cell, cutoff=4.0, neighbor_list=lst, neighbor_ptr=ptr[:4])
    with pytest.raises(ValueError, match="batch_idx must have one entry per atom"):
        fn(pos, radii, eps, cell, cutoff=4.0, neighbor_matrix=nm, batch_idx=torch.zeros(3, dtype=I32))


def test_reduced_sites_constructor_errors():
    par, kap = torch.full((4,), -1, dtype=I32), torch.full((4,), 0.9)
    for bad in (par[:, None], [0, 1], None):
        with pytest.raises(ValueError, match=r"parent must have shape \[num_atoms\]"):
            ReducedSites(bad, kap)
    for bad in (par.float(), par.to(torch.int16), par.bool()):
        with pytest.raises(ValueError, match=r"parent must be an int32 \(or int64\) tensor"):
            ReducedSites(bad, kap)
    for bad in (kap[:3], kap[:, None], 0.9):
        with pytest.raises(ValueError, match=r"reduction must have one entry per atom: expected shape \[4\]"):
            ReducedSites(par, bad)
    with pytest.raises(ValueError, match="reduction must be a floating-point tensor"):
        ReducedSites(par, torch.ones(4, dtype=I32))
    with pytest.raises(ValueError, match="tensors on different devices"):
        ReducedSites(par, kap.to("meta"))
    with pytest.raises(ValueError, match="batch_idx must have one entry per atom"):
        ReducedSites(par, kap, batch_idx=torch.zeros(3, dtype=I32))


def test_reduced_sites_value_errors_name_the_first_offending_atom():
    kap = torch.full((5,), 0.9)
    t = lambda *v: torch.tensor(v, dtype=I32)  # noqa: E731
    for bad, index in ((t(-1, 0, 5, 0, 9), 5), (t(-1, -2, 0, 0, 0), -2)):
        with pytest.raises(ValueError, match=rf"atom {1 if index == -2 else 2}: parent index {index} is outside \[-1, 5\)"):
            ReducedSites(bad, kap)
    with pytest.raises(ValueError, match=r"atom 2: its parent 1 is itself reduced \(parent 0\); a parent must be its own site"):
        ReducedSites(t(-1, 0, 1, 3, -1), kap)
    with pytest.raises(ValueError, match=r"atom 3 \(system 1\): its parent 0 is in another system \(0\)"):
        ReducedSites(t(-1, 0, 2, 0, 4), kap, batch_idx=t(0, 0, 0, 1, 1))
    ReducedSites(t(-1, 0, 2, 0, 4), kap, batch_idx=None)  # the same table is fine without systems
    # validate=False skips the read: the table is built with such parents as "none", for int64 as for int32
    for dtype in (I32, torch.int64):
        s = ReducedSites(t(-1, 0, 5, 0, -7).to(dtype), kap, validate=False)
        assert s.parent.dtype == I32 and s.parent.tolist() == [-1, 0, -1, 0, -1] and s.reduction.tolist() == pytest.approx([1.0, 0.9, 1.0, 0.9, 1.0])
        assert s.child_ptr.tolist() == [0, 2, 2, 2, 2, 2] and s.child_idx.tolist() == [1, 3] and s.num_atoms == 5 and "reduced=2" in repr(s)
    moved = s.to("meta")
    assert moved.num_atoms == 5 and all(getattr(moved, k).device.type == "meta" for k in ("parent", "reduction", "child_ptr", "child_idx")) and s.device.type == "cpu"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("fn", FNS)
def test_empty_inputs_return_zeros_of_the_documented_shapes(fn, dtype):
    flags = dict(compute_forces=True, compute_radius_gradients=True, compute_epsilon_gradients=True, compute_virial=True)
    pos, radii, eps, cell, nm, sh = _args()
    pos, radii, eps = pos.to(dtype), radii.to(dtype), eps.to(dtype)
    cells, bi = cell.repeat(2, 1, 1).to(dtype), torch.tensor([0, 0, 1, 1], dtype=I32)
    calls = [(4, 2, dict(neighbor_matrix=nm[:, :0], neighbor_matrix_shifts=sh[:, :0], batch_idx=bi), (pos, radii, eps, cells)),
             (4, 1, dict(neighbor_list=torch.zeros((2, 0), dtype=I32), neighbor_ptr=torch.zeros(5, dtype=I32)), (pos, radii, eps, cell.to(dtype))),
             (0, 2, dict(neighbor_matrix=nm[:0], batch_idx=bi[:0]), (pos[:0], radii[:0], eps[:0], cells))]
    for n, nsys, kw, atoms in calls:
        out = fn(*atoms, cutoff=4.0, taper=3.6, **kw, **flags)
        assert [tuple(o.shape) for o in out] == [(n,), (n, 3), (n,), (n,), (nsys, 3, 3)] and all(o.dtype == dtype and not o.any() for o in out)
        assert tuple(fn(*atoms, cutoff=4.0, **kw).shape) == (n,)


@pytest.mark.parametrize("fn", FNS)
def test_cpu_tensors_raise_native_library_error(fn):
    pos, radii, eps, cell, nm, sh = _args()
    nm = nm.clone()
    nm[0, 0], nm[1, 0] = 1, 0
    with pytest.raises(C.NativeLibraryError):
        fn(pos, radii, eps, cell, cutoff=4.0, neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    with pytest.raises(C.NativeLibraryError):
        fn(pos, radii, eps, cutoff=4.0, neighbor_matrix=nm, sites=ReducedSites(torch.tensor([-1, 0, -1, 2], dtype=I32), torch.full((4,), 0.9)))
