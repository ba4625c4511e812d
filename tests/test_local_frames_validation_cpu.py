"""Argument errors of `LocalFrames`, `rotate_multipoles` and `multipole_frame_forces`, raised before anything is launched (CPU tensors are
enough to reach them), the inverse map of the constructor, the exported names, the declared ABI symbols and the build row."""
import os

import pytest
import torch

from tests import local_frames_reference as LR

I32 = torch.int32


def _api():
    from nvalchemiops.interactions.electrostatics import LocalFrames, multipole_frame_forces, rotate_multipoles

    return LocalFrames, rotate_multipoles, multipole_frame_forces


def _water_frames(**kw):
    LocalFrames = _api()[0]
    pos, atoms, kinds = LR.water()
    return pos, LocalFrames(atoms, kinds, **kw)


def test_names_are_exported():
    from nvalchemiops.interactions import electrostatics as E
    from nvalchemiops.interactions.electrostatics import frames as FR

    for name in ("LocalFrames", "rotate_multipoles", "multipole_frame_forces", "FRAME_NONE", "FRAME_Z_ONLY", "FRAME_Z_THEN_X", "FRAME_BISECTOR",
                 "FRAME_Z_BISECT", "FRAME_THREE_FOLD"):
        assert name in E.__all__ and name in FR.__all__ and getattr(E, name) is getattr(FR, name)
    assert (E.FRAME_NONE, E.FRAME_Z_ONLY, E.FRAME_Z_THEN_X, E.FRAME_BISECTOR, E.FRAME_Z_BISECT, E.FRAME_THREE_FOLD) == (0, 1, 2, 3, 4, 5)
    assert (LR.NONE, LR.Z_ONLY, LR.Z_THEN_X, LR.BISECTOR, LR.Z_BISECT, LR.THREE_FOLD) == (0, 1, 2, 3, 4, 5)
    from nvalchemiops import _eops

    for name in ("rotate_multipoles_op", "rotate_multipoles_bwd_op"):
        assert name in _eops.__all__ and hasattr(_eops, name)


def test_abi_symbols_are_declared_and_the_source_is_listed():
    import importlib.util

    from tools.abi_symbols import declared_symbols

    declared = declared_symbols()
    for name in ("mi_frame_rotate", "mi_frame_adjoint", "mi_frame_gather", "mi_frame_blocks", "mi_frame_block_threads"):
        assert name in declared, name
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("build_native_for_test", os.path.join(root, "nvalchemi-toolkit-ops_amd", "build_native.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.SOURCES["frames.hip"] == [] and os.path.exists(os.path.join(mod.CSRC, "frames.hip"))


def test_docstrings_point_at_the_torque_routine():
    """The two sentences about torques in the operators' docstrings name the routine that turns them into forces."""
    from nvalchemiops.interactions.electrostatics import ewald_dipole_real_space, ewald_quadrupole_real_space

    assert "multipole_frame_forces" in ewald_dipole_real_space.__doc__
    assert "multipole_frame_forces" in ewald_quadrupole_real_space.__doc__


# ---- the constructor ------------------------------------------------------------------------------------------------------------------------
def test_inverse_map_lists_who_names_each_atom_in_ascending_order():
    LocalFrames = _api()[0]
    pos, atoms, kinds, _ = LR.join([LR.molecule(m) for m in ("none", "z_only", "water", "ammonia", "z_bisect", "chiral")])
    fr = LocalFrames(atoms, kinds)
    n = pos.shape[0]
    assert fr.num_atoms == n and fr.frame_atoms.dtype == I32 and fr.frame_kinds.dtype == I32
    assert fr.inverse_ptr.dtype == I32 and fr.inverse_slots.dtype == I32 and tuple(fr.inverse_ptr.shape) == (n + 1,)
    ptr, slots = fr.inverse_ptr.tolist(), fr.inverse_slots.tolist()
    assert ptr[0] == 0 and ptr[-1] == len(slots) == int((fr.frame_atoms >= 0).sum())
    for i in range(n):
        row = slots[ptr[i]:ptr[i + 1]]
        assert row == sorted(row)
        want = sorted(4 * j + 1 + s for j in range(n) for s in range(3) if int(fr.frame_atoms[j, s]) == i)
        assert row == want, (i, row, want)
    assert ptr[1] == ptr[0], "the NONE atom is named by no one"


def test_slots_a_kind_does_not_use_are_dropped():
    LocalFrames = _api()[0]
    E = __import__("nvalchemiops.interactions.electrostatics", fromlist=["x"])
    atoms = torch.tensor([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2], [0, 1, 2], [0, 1, 2]], dtype=I32)
    kinds = torch.tensor([E.FRAME_NONE, E.FRAME_Z_ONLY, E.FRAME_Z_THEN_X, E.FRAME_BISECTOR, E.FRAME_Z_BISECT, E.FRAME_THREE_FOLD], dtype=I32)
    fr = LocalFrames(atoms, kinds)
    assert fr.frame_atoms.tolist() == [[-1, -1, -1], [0, -1, -1], [0, 1, 3], [0, 1, -1], [0, 1, 2], [0, 1, 2]]
    assert LocalFrames(atoms.long(), kinds.long()).frame_atoms.dtype == I32


@pytest.mark.parametrize("atoms, kinds, batch, match", [
    ([[1, 2, -1], [0, 3, -1], [0, 1, -1]], [3, 2, 2], None, r"atom 1: frame atom index 3 in slot x is outside \[-1, 3\)"),
    ([[1, -2, -1], [0, 2, -1], [0, 1, -1]], [3, 2, 2], None, r"atom 0: frame atom index -2 in slot x is outside"),
    ([[1, -1, -1], [0, 2, -1], [0, 1, -1]], [3, 2, 2], None, r"atom 0: kind FRAME_BISECTOR requires a x atom"),
    ([[1, 2, -1], [0, 2, -1], [0, 1, -1]], [4, 2, 2], None, r"atom 0: kind FRAME_Z_BISECT requires a y atom"),
    ([[-1, -1, -1], [0, 2, -1], [0, 1, -1]], [1, 2, 2], None, r"atom 0: kind FRAME_Z_ONLY requires a z atom"),
    ([[1, 2, -1], [1, 2, -1], [0, 1, -1]], [3, 2, 2], None, r"atom 1: names itself as its z atom"),
    ([[1, 2, -1], [0, 2, -1], [0, 1, 2]], [3, 2, 2], None, r"atom 2: names itself as its y atom"),
    ([[1, 1, -1], [0, 2, -1], [0, 1, -1]], [3, 2, 2], None, r"atom 0: a frame atom appears twice"),
    ([[1, 2, 2], [0, 2, -1], [0, 1, -1]], [5, 2, 2], None, r"atom 0: a frame atom appears twice"),
    ([[1, 2, -1], [0, 2, -1], [0, 1, -1]], [3, 6, 2], None, r"atom 1: unknown frame kind 6"),
    ([[1, 2, -1], [0, 2, -1], [0, 1, -1]], [3, -1, 2], None, r"atom 1: unknown frame kind -1"),
    ([[1, 2, -1], [0, 2, -1], [0, 1, -1]], [3, 2, 2], [0, 0, 1], r"atom 0 \(system 0\): its x atom 2 is in another system \(1\)"),
])
def test_constructor_value_errors(atoms, kinds, batch, match):
    LocalFrames = _api()[0]
    a, k = torch.tensor(atoms, dtype=I32), torch.tensor(kinds, dtype=I32)
    b = None if batch is None else torch.tensor(batch, dtype=I32)
    with pytest.raises(ValueError, match=match):
        LocalFrames(a, k, batch_idx=b)
    fr = LocalFrames(a, k, batch_idx=b, validate=False)  # no read of the values: the tables are sanitised instead
    assert int(fr.frame_atoms.max()) < 3 and int(fr.frame_atoms.min()) >= -1 and int(fr.frame_kinds.max()) <= 5 and int(fr.frame_kinds.min()) >= 0
    assert int(fr.inverse_ptr[-1]) == fr.inverse_slots.shape[0] == int((fr.frame_atoms >= 0).sum())


def test_a_slot_that_is_not_used_is_not_validated():
    LocalFrames = _api()[0]
    # the y slot of a bisector and every slot of NONE are not looked at: an atom may "name itself" there
    fr = LocalFrames(torch.tensor([[1, 2, 0], [1, 1, 1], [0, 1, -1]], dtype=I32), torch.tensor([3, 0, 2], dtype=I32))
    assert fr.frame_atoms.tolist() == [[1, 2, -1], [-1, -1, -1], [0, 1, -1]]


@pytest.mark.parametrize("atoms, kinds, match", [
    (torch.zeros((3, 2), dtype=I32), torch.zeros(3, dtype=I32), "frame_atoms must have shape"),
    (torch.zeros(3, dtype=I32), torch.zeros(3, dtype=I32), "frame_atoms must have shape"),
    (torch.zeros((3, 3), dtype=I32), torch.zeros(4, dtype=I32), "frame_kinds must have one entry per atom"),
    (torch.zeros((3, 3), dtype=torch.float32), torch.zeros(3, dtype=I32), "frame_atoms must be an int32"),
    (torch.zeros((3, 3), dtype=I32), torch.zeros(3, dtype=torch.float64), "frame_kinds must be an int32"),
])
def test_constructor_shape_and_dtype_errors(atoms, kinds, match):
    with pytest.raises(ValueError, match=match):
        _api()[0](atoms, kinds)
    with pytest.raises(ValueError, match="batch_idx must have one entry per atom"):
        _api()[0](torch.full((3, 3), -1, dtype=I32), torch.zeros(3, dtype=I32), batch_idx=torch.zeros(2, dtype=I32))


def test_empty_topology():
    fr = _api()[0](torch.zeros((0, 3), dtype=I32), torch.zeros(0, dtype=I32))
    assert fr.num_atoms == 0 and fr.inverse_ptr.tolist() == [0] and fr.inverse_slots.numel() == 0


# ---- the two functions ----------------------------------------------------------------------------------------------------------------------
def test_function_value_errors():
    _, rotate, forces = _api()
    pos, fr = _water_frames()
    mu, quad = LR.local_multipoles(3, 1)
    cell = torch.eye(3, dtype=torch.float64) * 10.0
    g_mu, g_q = torch.zeros_like(mu), torch.zeros_like(quad)
    for fn, tail in ((rotate, ()), (forces, (g_mu, g_q))):
        with pytest.raises(ValueError, match="positions must have shape"):
            fn(pos[:, :2], mu, quad, fr, *tail)
        with pytest.raises(ValueError, match="frames describes 3 atoms but positions has 4"):
            fn(torch.zeros((4, 3), dtype=torch.float64), None, None, fr, *[None] * len(tail))
        with pytest.raises(ValueError, match="local_dipoles must have one vector per atom"):
            fn(pos, mu[:2], quad, fr, *tail)
        with pytest.raises(ValueError, match="local_quadrupoles must have one 3 x 3 tensor per atom"):
            fn(pos, mu, quad.reshape(3, 9), fr, *tail)
        with pytest.raises(ValueError, match="local_dipoles must be a floating-point tensor"):
            fn(pos, mu.long(), quad, fr, *tail)
        with pytest.raises(ValueError, match="Unsupported dtype"):
            fn(pos.half(), mu, quad, fr, *tail)
        with pytest.raises(TypeError, match="frames must be a LocalFrames"):
            fn(pos, mu, quad, (fr.frame_atoms, fr.frame_kinds), *tail)
        with pytest.raises(ValueError, match=r"cell must have shape \[3, 3\] or \[num_systems, 3, 3\]"):
            fn(pos, mu, quad, fr, *tail, cell[:2])
        with pytest.raises(ValueError, match="batch_idx is required"):
            fn(pos, mu, quad, fr, *tail, cell.repeat(2, 1, 1))
        with pytest.raises(ValueError, match="batch_idx must have one entry per atom"):
            fn(pos, mu, quad, fr, *tail, cell, batch_idx=torch.zeros(2, dtype=I32))
    with pytest.raises(ValueError, match="compute_virial needs a cell"):
        forces(pos, mu, quad, fr, g_mu, g_q, compute_virial=True)
    with pytest.raises(ValueError, match=r"dipole_grads must have shape \[3, 3\]"):
        forces(pos, mu, quad, fr, g_mu[:2], g_q)
    with pytest.raises(ValueError, match=r"quadrupole_grads must have shape \[3, 3, 3\]"):
        forces(pos, mu, quad, fr, g_mu, g_q.reshape(3, 9))
    with pytest.raises(ValueError, match="dipole_grads is required when local_dipoles is given"):
        forces(pos, mu, None, fr, None, None)
    with pytest.raises(ValueError, match="quadrupole_grads is required when local_quadrupoles is given"):
        forces(pos, None, quad, fr, None, None)


def test_cpu_tensors_have_no_fallback():
    from nvalchemiops._capi import NativeLibraryError

    _, rotate, forces = _api()
    pos, fr = _water_frames()
    mu, quad = LR.local_multipoles(3, 1)
    with pytest.raises(NativeLibraryError):
        rotate(pos, mu, quad, fr)
    with pytest.raises(NativeLibraryError):
        forces(pos, mu, quad, fr, mu, quad)


def test_no_atoms_launch_nothing():
    LocalFrames, rotate, forces = _api()
    fr = LocalFrames(torch.zeros((0, 3), dtype=I32), torch.zeros(0, dtype=I32))
    pos, mu, quad = torch.zeros((0, 3)), torch.zeros((0, 3)), torch.zeros((0, 3, 3))
    m, q = rotate(pos, mu, quad, fr)
    assert tuple(m.shape) == (0, 3) and tuple(q.shape) == (0, 3, 3) and m.dtype == torch.float32
    assert rotate(pos, None, quad, fr)[0] is None and rotate(pos, mu, None, fr)[1] is None
    f, lm, lq, vir = forces(pos, mu, quad, fr, mu, quad, torch.eye(3), compute_local_gradients=True, compute_virial=True)
    assert tuple(f.shape) == (0, 3) and tuple(lm.shape) == (0, 3) and tuple(lq.shape) == (0, 3, 3)
    assert tuple(vir.shape) == (1, 3, 3) and float(vir.abs().max()) == 0.0
