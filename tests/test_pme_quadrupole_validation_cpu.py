"""Particle-mesh Ewald for point quadrupoles: what can be checked without a GPU -- exports, signatures against the dipole and
Ewald-quadrupole siblings, every argument error (all raised before any launch, on CPU tensors), the absence of a CPU path, empty inputs, the C
ABI (declared, exported, argument checks that return before any device call) and the custom ops."""
import ctypes
import inspect

import pytest
import torch

from nvalchemiops import _capi as C

MI_OK, MI_EINVAL = 0, -1  # include/nvalchemiops_hip.h
P = ctypes.c_void_p(4096)  # a non-null pointer that is never dereferenced: every call below fails its checks first
FLAGS = ("compute_forces", "compute_charge_gradients", "compute_dipole_gradients", "compute_quadrupole_gradients", "compute_virial")
MESH = (8, 8, 8)


def _api():
    from nvalchemiops.interactions.electrostatics import pme_quadrupole_correction, pme_quadrupole_reciprocal_space

    return pme_quadrupole_correction, pme_quadrupole_reciprocal_space


def _args(n=4, m=6):
    pos, q, mu, qd, cell = torch.rand(n, 3), torch.rand(n), torch.rand(n, 3), torch.rand(n, 3, 3), torch.eye(3)[None] * 10
    return pos, q, mu, qd, cell, torch.full((n, m), n, dtype=torch.int32), torch.zeros((n, m, 3), dtype=torch.int32)


def test_exported_with_the_signatures_of_the_siblings():
    import nvalchemiops.interactions.electrostatics as E
    from nvalchemiops.interactions.electrostatics import pme_quadrupole as D

    for name in ("pme_quadrupole_reciprocal_space", "pme_quadrupole_correction"):
        assert name in E.__all__ and name in D.__all__ and getattr(E, name) is getattr(D, name)

    def with_quadrupoles(names):  # a dipole signature with `quadrupoles` after `dipoles` and its flag before `compute_virial`
        names = list(names)
        names.insert(names.index("dipoles") + 1, "quadrupoles")
        names.insert(names.index("compute_virial"), "compute_quadrupole_gradients")
        return names

    recip = inspect.signature(D.pme_quadrupole_reciprocal_space).parameters
    both = inspect.signature(D.pme_quadrupole_correction).parameters
    assert list(recip) == with_quadrupoles(inspect.signature(E.pme_dipole_reciprocal_space).parameters)
    assert list(both) == with_quadrupoles(inspect.signature(E.pme_dipole_correction).parameters)
    for mine, sibling in ((recip, E.pme_dipole_reciprocal_space), (both, E.pme_dipole_correction)):
        for name, param in inspect.signature(sibling).parameters.items():
            assert mine[name].default == param.default or (mine[name].default is param.default), name
    # the multipole arguments and the flags are those of the explicit routine, in its order
    explicit = list(inspect.signature(E.ewald_quadrupole_correction).parameters)
    assert [n for n in both if n in explicit] == [n for n in explicit if n in both]
    assert list(both)[:5] == explicit[:5] and [n for n in both if n.startswith("compute_")] == list(FLAGS)
    for params in (recip, both):
        assert params["spline_order"].default == 5 and all(params[f].default is False for f in FLAGS)
    for fn in (D.pme_quadrupole_reciprocal_space, D.pme_quadrupole_correction):
        doc = fn.__doc__
        assert "MODEL" not in doc and "RETURNS" not in doc
        for phrase in ("Theta_i W_i . phi_L", "4 alpha^5 / (5 sqrt(pi))", "tin-foil", "ADDED", "NOT symmetric", "5 or", "converge more slowly",
                       "arrival order", "external_field", "exactly 0.0"):
            assert phrase in doc, (fn.__name__, phrase)
    assert "pme_dipole_correction" in D.pme_quadrupole_correction.__doc__ and "MUST BE FULL" in D.pme_quadrupole_correction.__doc__


def test_the_siblings_point_to_the_mesh_routine_and_are_otherwise_untouched():
    import nvalchemiops.interactions.electrostatics as E

    for fn in (E.ewald_quadrupole_correction, E.ewald_quadrupole_reciprocal_space, E.pme_dipole_correction, E.pme_dipole_reciprocal_space,
               E.induced_dipoles):
        assert "pme_quadrupole_correction" in fn.__doc__, fn.__name__
    assert "quadrupoles" not in inspect.signature(E.pme_dipole_correction).parameters
    assert "mesh_dimensions" not in inspect.signature(E.ewald_quadrupole_correction).parameters


def test_spline_order_four_and_below_is_refused_with_the_reason():
    both, recip = _api()
    pos, q, mu, qd, cell, nm, sh = _args()
    for order in (1, 2, 3, 4, 7):
        with pytest.raises(ValueError, match="spline_order must be 5 or 6 .*third derivative.*discontinuous at order 4"):
            recip(pos, q, mu, qd, cell, 0.3, mesh_dimensions=MESH, spline_order=order)
        with pytest.raises(ValueError, match="spline_order must be 5 or 6 .*third derivative.*discontinuous at order 4"):
            both(pos, q, mu, qd, cell, 0.3, mesh_dimensions=MESH, spline_order=order, neighbor_matrix=nm, neighbor_matrix_shifts=sh)


def test_argument_errors_come_before_any_launch():
    both, recip = _api()
    pos, q, mu, qd, cell, nm, sh = _args()
    lists = dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    for bad in (torch.rand(4, 3), torch.rand(4, 9), torch.rand(3, 3, 3), torch.rand(4, 3, 2), None):
        with pytest.raises(ValueError, match="quadrupoles must have one 3 x 3 tensor per atom"):
            recip(pos, q, mu, bad, cell, 0.3, mesh_dimensions=MESH)
        with pytest.raises(ValueError, match="quadrupoles must have one 3 x 3 tensor per atom"):
            both(pos, q, mu, bad, cell, 0.3, mesh_dimensions=MESH, **lists)
    for bad in (torch.rand(4), torch.rand(4, 2), torch.rand(3, 3)):
        with pytest.raises(ValueError, match="dipoles must have one vector per atom"):
            recip(pos, q, bad, qd, cell, 0.3, mesh_dimensions=MESH)
        with pytest.raises(ValueError, match="dipoles must have one vector per atom"):
            both(pos, q, bad, qd, cell, 0.3, mesh_dimensions=MESH, **lists)
    with pytest.raises(ValueError, match="cell is required"):
        recip(pos, q, mu, qd, None, 0.3, mesh_dimensions=MESH)
    with pytest.raises(ValueError, match="cell is required"):
        both(pos, q, mu, qd, None, 0.3, mesh_dimensions=MESH, **lists)
    for dims, order in (((8, 4, 8), 5), ((5, 8, 8), 6), ((8, 8, 5), 6)):
        with pytest.raises(ValueError, match="at least the spline order"):
            recip(pos, q, mu, qd, cell, 0.3, mesh_dimensions=dims, spline_order=order)
        with pytest.raises(ValueError, match="at least the spline order"):
            both(pos, q, mu, qd, cell, 0.3, mesh_dimensions=dims, spline_order=order, **lists)
    with pytest.raises(ValueError, match="mesh_dimensions or mesh_spacing"):
        recip(pos, q, mu, qd, cell, 0.3)
    with pytest.raises(ValueError, match="mesh_dimensions must hold three integers"):
        recip(pos, q, mu, qd, cell, 0.3, mesh_dimensions=(8, 8))
    with pytest.raises(ValueError, match="alpha has 2 values but there are 1 systems"):
        recip(pos, q, mu, qd, cell, torch.tensor([0.3, 0.4]), mesh_dimensions=MESH)
    with pytest.raises(ValueError, match="alpha has 2 values but there are 1 systems"):
        both(pos, q, mu, qd, cell, torch.tensor([0.3, 0.4]), mesh_dimensions=MESH, **lists)
    with pytest.raises(ValueError, match="charges must have one entry per atom"):
        recip(pos, q[:3], mu, qd, cell, 0.3, mesh_dimensions=MESH)
    with pytest.raises((ValueError, TypeError), match="float32 or float64|dtype"):
        recip(pos.to(torch.float16), q, mu, qd, cell, 0.3, mesh_dimensions=MESH)
    with pytest.raises(ValueError, match="compute_virial needs the shifts"):
        both(pos, q, mu, qd, cell, 0.3, mesh_dimensions=MESH, neighbor_matrix=nm, compute_virial=True)
    with pytest.raises(ValueError, match="Either neighbor_list or neighbor_matrix"):
        both(pos, q, mu, qd, cell, 0.3, mesh_dimensions=MESH)


def test_reference_spline_orders_are_refused():
    from nvalchemiops.spline import reference_spline_orders

    both, recip = _api()
    pos, q, mu, qd, cell, nm, sh = _args()
    with reference_spline_orders():
        with pytest.raises(ValueError, match="no reference evaluation"):
            recip(pos, q, mu, qd, cell, 0.3, mesh_dimensions=MESH)
        with pytest.raises(ValueError, match="no reference evaluation"):
            both(pos, q, mu, qd, cell, 0.3, mesh_dimensions=MESH, neighbor_matrix=nm, neighbor_matrix_shifts=sh)


def test_cpu_tensors_have_no_fallback_and_empty_inputs_need_no_device():
    both, recip = _api()
    pos, q, mu, qd, cell, nm, sh = _args()
    with pytest.raises(C.NativeLibraryError, match="no CPU path"):
        recip(pos, q, mu, qd, cell, 0.3, mesh_dimensions=MESH)
    with pytest.raises(C.NativeLibraryError, match="no CPU path"):
        recip(pos, q, None, qd, cell, 0.3, mesh_dimensions=MESH)
    with pytest.raises(C.NativeLibraryError, match="no CPU path"):
        both(pos, q, mu, qd, cell, 0.3, mesh_dimensions=MESH, neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    with pytest.raises(C.NativeLibraryError, match="no CPU path"):
        recip(pos, q, mu, qd.requires_grad_(True), cell, 0.3, mesh_dimensions=MESH)
    none = torch.zeros((0, 3)), torch.zeros(0), torch.zeros((0, 3)), torch.zeros((0, 3, 3))
    e, f, cg, dg, qg, vir = recip(*none, cell, 0.3, mesh_dimensions=MESH, **{flag: True for flag in FLAGS})
    assert (e.shape, f.shape, cg.shape, dg.shape, qg.shape, vir.shape) == ((0,), (0, 3), (0,), (0, 3), (0, 3, 3), (1, 3, 3))
    assert recip(*none, cell, 0.3, mesh_dimensions=MESH).shape == (0,)


def test_c_abi_is_declared_exported_and_checks_its_arguments():
    from tools.abi_symbols import declared_symbols

    L = C.lib()
    names = ("mi_pme_quadrupole_spread", "mi_pme_quadrupole_gather", "mi_pme_quadrupole_virial", "mi_pme_quadrupole_virial_blocks")
    declared = declared_symbols()
    for name in names:
        assert name in declared and hasattr(L, name)
    assert int(L.mi_pme_quadrupole_virial_blocks()) >= 1
    s = ctypes.c_void_p(0)
    # spread: order (4 is refused), mesh below the order, dtype, null pointers -- each returns MI_EINVAL before any device call
    assert L.mi_pme_quadrupole_spread(P, P, P, P, None, None, P, 4, 1, 8, 8, 8, 4, C.MI_F64, P, s) == MI_EINVAL
    assert b"5 or 6" in L.mi_last_error()
    assert L.mi_pme_quadrupole_spread(P, P, P, P, None, None, P, 4, 1, 8, 8, 8, 5 | C.SPLINE_REFERENCE_ORDERS, C.MI_F64, P, s) == MI_EINVAL
    assert L.mi_pme_quadrupole_spread(P, P, P, P, None, None, P, 4, 1, 8, 4, 8, 5, C.MI_F64, P, s) == MI_EINVAL
    assert L.mi_pme_quadrupole_spread(P, P, P, P, None, None, P, 4, 1, 8, 8, 8, 5, 7, P, s) == MI_EINVAL
    assert L.mi_pme_quadrupole_spread(P, P, P, P, None, None, P, 4, 1, 8, 8, 8, 5, C.MI_F64, None, s) == MI_EINVAL
    assert L.mi_pme_quadrupole_spread(P, P, P, None, None, None, P, 4, 1, 8, 8, 8, 5, C.MI_F64, P, s) == MI_EINVAL
    # gather
    none = (None,) * 5
    assert L.mi_pme_quadrupole_gather(P, P, P, P, None, None, P, P, P, P, 4, 1, 8, 8, 8, 4, C.MI_F64, 0, *none, s) == MI_EINVAL
    assert L.mi_pme_quadrupole_gather(P, P, P, P, None, None, P, P, P, P, 4, 1, 8, 8, 3, 5, C.MI_F64, 0, *none, s) == MI_EINVAL
    assert L.mi_pme_quadrupole_gather(P, P, P, P, P, None, P, P, P, P, 4, 1, 8, 8, 8, 5, C.MI_F64, 1, *none, s) == MI_EINVAL
    assert b"accumulate" in L.mi_last_error()
    assert L.mi_pme_quadrupole_gather(P, P, P, None, None, None, P, P, P, P, 4, 1, 8, 8, 8, 5, C.MI_F64, 0, *none, s) == MI_EINVAL
    assert L.mi_pme_quadrupole_gather(P, P, P, P, None, None, P, None, P, P, 4, 1, 8, 8, 8, 5, C.MI_F64, 0, *none, s) == MI_EINVAL
    assert L.mi_pme_quadrupole_gather(P, P, P, P, None, None, P, P, P, P, 0, 1, 8, 8, 8, 5, C.MI_F64, 0, *none, s) == MI_OK  # no atoms
    # virial
    assert L.mi_pme_quadrupole_virial(P, None, P, P, P, 1, 8, 8, 8, 5, C.MI_F64, P, s) == MI_EINVAL
    assert L.mi_pme_quadrupole_virial(P, P, P, P, P, 1, 8, 8, 8, 5, C.MI_F64, None, s) == MI_EINVAL
    assert L.mi_pme_quadrupole_virial(P, P, P, P, P, 1, 8, 8, 8, 4, C.MI_F64, P, s) == MI_EINVAL


def test_ops_are_registered_with_fake_implementations():
    from nvalchemiops import _eops

    assert hasattr(torch.ops.alchemiops, "_pme_quadrupole_reciprocal_space") and _eops.pme_quadrupole_reciprocal_space_op is not None
    assert hasattr(torch.ops.nvalchemiops, "pme_quadrupole_reciprocal_space_backward")
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        pos, q, mu, qd, cell = torch.empty(5, 3), torch.empty(5), torch.empty(5, 3), torch.empty(5, 3, 3), torch.empty(1, 3, 3)
        op = torch.ops.alchemiops._pme_quadrupole_reciprocal_space
        out = op(pos, q, mu, qd, cell, torch.empty(1), None, 8, 8, 8, 5, True, False, True, True, True)
        assert [tuple(o.shape) for o in out] == [(5,), (5, 3), (0,), (5, 3), (5, 3, 3), (1, 3, 3)]
        bi = torch.empty(5, dtype=torch.int32)
        out = op(pos, q, mu, qd, torch.empty(3, 3, 3), torch.empty(3), bi, 8, 8, 8, 6, False, True, False, False, True)
        assert [tuple(o.shape) for o in out] == [(5,), (0,), (5,), (0,), (0,), (3, 3, 3)]
        grads = torch.ops.nvalchemiops.pme_quadrupole_reciprocal_space_backward(pos, q, mu, qd, cell, torch.empty(1), None, 8, 8, 8, 5, torch.empty(5))
        assert [tuple(g.shape) for g in grads] == [(5, 3), (5,), (5, 3), (5, 3, 3)] and all(g.dtype == torch.float64 for g in grads)
