"""Particle-mesh Ewald for point dipoles: what can be checked without a GPU -- exports, signatures, every argument error (all raised before any
launch, on CPU tensors), the absence of a CPU path, empty inputs, the C ABI (declared, exported, argument checks that return before any device
call) and the custom ops."""
import ctypes
import inspect

import pytest
import torch

from nvalchemiops import _capi as C

MI_OK, MI_EINVAL = 0, -1  # include/nvalchemiops_hip.h
P = ctypes.c_void_p(4096)  # a non-null pointer that is never dereferenced: every call below fails its checks first
FLAGS = ("compute_forces", "compute_charge_gradients", "compute_dipole_gradients", "compute_virial")
LISTS = ["neighbor_list", "neighbor_ptr", "neighbor_shifts", "neighbor_matrix", "neighbor_matrix_shifts"]
MESH = (8, 8, 8)


def _api():
    from nvalchemiops.interactions.electrostatics import pme_dipole_correction, pme_dipole_reciprocal_space

    return pme_dipole_correction, pme_dipole_reciprocal_space


def _args(n=4, m=6):
    pos, q, mu, cell = torch.rand(n, 3), torch.rand(n), torch.rand(n, 3), torch.eye(3)[None] * 10
    return pos, q, mu, cell, torch.full((n, m), n, dtype=torch.int32), torch.zeros((n, m, 3), dtype=torch.int32)


def test_exported_with_the_documented_signatures():
    import nvalchemiops.interactions.electrostatics as E
    from nvalchemiops.interactions.electrostatics import pme_dipole as D

    for name in ("pme_dipole_reciprocal_space", "pme_dipole_correction"):
        assert name in E.__all__ and name in D.__all__ and getattr(E, name) is getattr(D, name)
    recip = inspect.signature(D.pme_dipole_reciprocal_space).parameters
    assert list(recip) == ["positions", "charges", "dipoles", "cell", "alpha", "mesh_dimensions", "mesh_spacing", "spline_order", "batch_idx"] + list(FLAGS)
    both = inspect.signature(D.pme_dipole_correction).parameters
    assert list(both) == (["positions", "charges", "dipoles", "cell", "alpha", "mesh_spacing", "mesh_dimensions", "spline_order", "batch_idx"] + LISTS
                          + ["mask_value"] + list(FLAGS) + ["accuracy"])
    assert both["alpha"].default is None and both["mask_value"].default is None and both["accuracy"].default == 1e-6
    for params in (recip, both):
        assert params["spline_order"].default == 5 and all(params[f].default is False for f in FLAGS)
    for fn in (D.pme_dipole_reciprocal_space, D.pme_dipole_correction):
        doc = fn.__doc__
        assert "MODEL" not in doc and "RETURNS" not in doc
        for phrase in ("mu_i . grad W_i", "2 alpha^3 / (3 sqrt(pi))", "tin-foil", "ADDED", "NOT symmetric", "quadrupoles", "arrival order", "4, 5"):
            assert phrase in doc, (fn.__name__, phrase)
    assert "particle_mesh_ewald" in D.pme_dipole_correction.__doc__ and "MUST BE FULL" in D.pme_dipole_correction.__doc__


def test_existing_routines_are_untouched():
    from nvalchemiops.interactions.electrostatics import ewald_dipole_correction, particle_mesh_ewald

    assert "dipoles" not in inspect.signature(particle_mesh_ewald).parameters
    assert "mesh_dimensions" not in inspect.signature(ewald_dipole_correction).parameters
    assert "a PME path for dipoles" not in ewald_dipole_correction.__doc__ and "quadrupoles" in ewald_dipole_correction.__doc__


def test_argument_errors_come_before_any_launch():
    both, recip = _api()
    pos, q, mu, cell, nm, sh = _args()
    lists = dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    for bad in (torch.rand(4), torch.rand(4, 2), torch.rand(3, 3), torch.rand(4, 3, 1)):
        with pytest.raises(ValueError, match="dipoles must have one vector per atom"):
            recip(pos, q, bad, cell, 0.3, mesh_dimensions=MESH)
        with pytest.raises(ValueError, match="dipoles must have one vector per atom"):
            both(pos, q, bad, cell, 0.3, mesh_dimensions=MESH, **lists)
    with pytest.raises(ValueError, match="cell is required"):
        recip(pos, q, mu, None, 0.3, mesh_dimensions=MESH)
    with pytest.raises(ValueError, match="cell is required"):
        both(pos, q, mu, None, 0.3, mesh_dimensions=MESH, **lists)
    for order in (1, 2, 3, 7):
        with pytest.raises(ValueError, match="spline_order must be 4, 5 or 6"):
            recip(pos, q, mu, cell, 0.3, mesh_dimensions=MESH, spline_order=order)
        with pytest.raises(ValueError, match="spline_order must be 4, 5 or 6"):
            both(pos, q, mu, cell, 0.3, mesh_dimensions=MESH, spline_order=order, **lists)
    for dims, order in (((8, 4, 8), 5), ((3, 8, 8), 4), ((8, 8, 5), 6)):
        with pytest.raises(ValueError, match="at least the spline order"):
            recip(pos, q, mu, cell, 0.3, mesh_dimensions=dims, spline_order=order)
        with pytest.raises(ValueError, match="at least the spline order"):
            both(pos, q, mu, cell, 0.3, mesh_dimensions=dims, spline_order=order, **lists)
    with pytest.raises(ValueError, match="mesh_dimensions or mesh_spacing"):
        recip(pos, q, mu, cell, 0.3)
    with pytest.raises(ValueError, match="alpha has 2 values but there are 1 systems"):
        recip(pos, q, mu, cell, torch.tensor([0.3, 0.4]), mesh_dimensions=MESH)
    with pytest.raises(ValueError, match="alpha has 2 values but there are 1 systems"):
        both(pos, q, mu, cell, torch.tensor([0.3, 0.4]), mesh_dimensions=MESH, **lists)
    with pytest.raises(ValueError, match="charges must have one entry per atom"):
        recip(pos, q[:3], mu, cell, 0.3, mesh_dimensions=MESH)
    with pytest.raises(ValueError, match="compute_virial needs the shifts"):
        both(pos, q, mu, cell, 0.3, mesh_dimensions=MESH, neighbor_matrix=nm, compute_virial=True)
    with pytest.raises(ValueError, match="Either neighbor_list or neighbor_matrix"):
        both(pos, q, mu, cell, 0.3, mesh_dimensions=MESH)
    with pytest.raises(ValueError, match="ONE format"):
        both(pos, q, mu, cell, 0.3, mesh_dimensions=MESH, neighbor_list=torch.zeros((2, 3), dtype=torch.int32),
             neighbor_ptr=torch.zeros(5, dtype=torch.int32), **lists)


def test_reference_spline_orders_are_refused():
    from nvalchemiops.spline import reference_spline_orders

    both, recip = _api()
    pos, q, mu, cell, nm, sh = _args()
    with reference_spline_orders():
        with pytest.raises(ValueError, match="no reference evaluation"):
            recip(pos, q, mu, cell, 0.3, mesh_dimensions=MESH)
        with pytest.raises(ValueError, match="no reference evaluation"):
            both(pos, q, mu, cell, 0.3, mesh_dimensions=MESH, neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    with pytest.raises(ValueError, match="no reference evaluation"):
        recip(pos, q, mu, cell, 0.3, mesh_dimensions=MESH, spline_order=5 | C.SPLINE_REFERENCE_ORDERS)


def test_cpu_tensors_have_no_fallback_and_empty_inputs_need_no_device():
    both, recip = _api()
    pos, q, mu, cell, nm, sh = _args()
    with pytest.raises(C.NativeLibraryError, match="no CPU path"):
        recip(pos, q, mu, cell, 0.3, mesh_dimensions=MESH)
    with pytest.raises(C.NativeLibraryError, match="no CPU path"):
        both(pos, q, mu, cell, 0.3, mesh_dimensions=MESH, neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    with pytest.raises(C.NativeLibraryError, match="no CPU path"):
        recip(pos.requires_grad_(True), q, mu, cell, 0.3, mesh_dimensions=MESH)
    e, f, cg, dg, vir = recip(torch.zeros((0, 3)), torch.zeros(0), torch.zeros((0, 3)), cell, 0.3, mesh_dimensions=MESH, compute_forces=True,
                              compute_charge_gradients=True, compute_dipole_gradients=True, compute_virial=True)
    assert e.shape == (0,) and f.shape == (0, 3) and cg.shape == (0,) and dg.shape == (0, 3) and vir.shape == (1, 3, 3)
    assert recip(torch.zeros((0, 3)), torch.zeros(0), torch.zeros((0, 3)), cell, 0.3, mesh_dimensions=MESH).shape == (0,)


def test_c_abi_is_declared_exported_and_checks_its_arguments():
    from tools.abi_symbols import declared_symbols

    L = C.lib()
    names = ("mi_pme_dipole_spread", "mi_pme_dipole_gather", "mi_pme_dipole_virial", "mi_pme_dipole_virial_blocks")
    declared = declared_symbols()
    for name in names:
        assert name in declared and hasattr(L, name)
    assert int(L.mi_pme_dipole_virial_blocks()) >= 1
    s = ctypes.c_void_p(0)
    # spread: order, mesh below the order, dtype, null meshes -- each returns MI_EINVAL before any device call
    assert L.mi_pme_dipole_spread(P, P, P, None, None, P, 4, 1, 8, 8, 8, 3, C.MI_F64, P, s) == MI_EINVAL
    assert b"4..6" in L.mi_last_error()
    assert L.mi_pme_dipole_spread(P, P, P, None, None, P, 4, 1, 8, 8, 8, 5 | C.SPLINE_REFERENCE_ORDERS, C.MI_F64, P, s) == MI_EINVAL
    assert L.mi_pme_dipole_spread(P, P, P, None, None, P, 4, 1, 8, 4, 8, 5, C.MI_F64, P, s) == MI_EINVAL
    assert L.mi_pme_dipole_spread(P, P, P, None, None, P, 4, 1, 8, 8, 8, 5, 7, P, s) == MI_EINVAL
    assert L.mi_pme_dipole_spread(P, P, P, None, None, P, 4, 1, 8, 8, 8, 5, C.MI_F64, None, s) == MI_EINVAL
    assert L.mi_pme_dipole_spread(None, P, P, None, None, P, 4, 1, 8, 8, 8, 5, C.MI_F64, P, s) == MI_EINVAL
    # gather
    assert L.mi_pme_dipole_gather(P, P, P, None, None, P, P, P, P, 4, 1, 8, 8, 8, 7, C.MI_F64, 0, None, None, None, None, s) == MI_EINVAL
    assert L.mi_pme_dipole_gather(P, P, P, None, None, P, P, P, P, 4, 1, 8, 8, 3, 4, C.MI_F64, 0, None, None, None, None, s) == MI_EINVAL
    assert L.mi_pme_dipole_gather(P, P, P, P, None, P, P, P, P, 4, 1, 8, 8, 8, 5, C.MI_F64, 1, None, None, None, None, s) == MI_EINVAL
    assert b"accumulate" in L.mi_last_error()
    assert L.mi_pme_dipole_gather(P, P, P, None, None, P, None, P, P, 4, 1, 8, 8, 8, 5, C.MI_F64, 0, None, None, None, None, s) == MI_EINVAL
    assert L.mi_pme_dipole_gather(P, P, P, None, None, P, P, P, P, 0, 1, 8, 8, 8, 5, C.MI_F64, 0, None, None, None, None, s) == MI_OK  # no atoms
    # virial
    assert L.mi_pme_dipole_virial(P, None, P, P, P, 1, 8, 8, 8, 5, C.MI_F64, P, s) == MI_EINVAL
    assert L.mi_pme_dipole_virial(P, P, P, P, P, 1, 8, 8, 8, 5, C.MI_F64, None, s) == MI_EINVAL
    assert L.mi_pme_dipole_virial(P, P, P, P, P, 1, 8, 8, 8, 3, C.MI_F64, P, s) == MI_EINVAL


def test_ops_are_registered_with_fake_implementations():
    from nvalchemiops import _eops

    assert _eops.pme_dipole_reciprocal_space_op is torch.ops.alchemiops._pme_dipole_reciprocal_space.default or hasattr(
        torch.ops.alchemiops, "_pme_dipole_reciprocal_space")
    assert hasattr(torch.ops.nvalchemiops, "pme_dipole_reciprocal_space_backward")
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        pos, q, mu, cell = torch.empty(5, 3), torch.empty(5), torch.empty(5, 3), torch.empty(1, 3, 3)
        out = torch.ops.alchemiops._pme_dipole_reciprocal_space(pos, q, mu, cell, torch.empty(1), None, 8, 8, 8, 5, True, False, True, True)
        assert [tuple(o.shape) for o in out] == [(5,), (5, 3), (0,), (5, 3), (1, 3, 3)]
        bi = torch.empty(5, dtype=torch.int32)
        out = torch.ops.alchemiops._pme_dipole_reciprocal_space(pos, q, mu, torch.empty(3, 3, 3), torch.empty(3), bi, 8, 8, 8, 5, False, True, False, True)
        assert [tuple(o.shape) for o in out] == [(5,), (0,), (5,), (0,), (3, 3, 3)]
        grads = torch.ops.nvalchemiops.pme_dipole_reciprocal_space_backward(pos, q, mu, cell, torch.empty(1), None, 8, 8, 8, 5, torch.empty(5))
        assert [tuple(g.shape) for g in grads] == [(5, 3), (5,), (5, 3)] and all(g.dtype == torch.float64 for g in grads)
