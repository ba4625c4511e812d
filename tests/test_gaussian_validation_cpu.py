"""`gaussian_charge_correction`: what can be checked without a GPU -- export, signature, every argument error and its message, the absence of
a CPU path, empty inputs, and the argument checks of the C entry point (which return before any device call)."""
import ctypes
import inspect
import os

import pytest
import torch

from nvalchemiops import _capi as C

MI_OK, MI_EINVAL = 0, -1  # include/nvalchemiops_hip.h
P = ctypes.c_void_p(4096)  # a non-null pointer that is never dereferenced: every call below fails its checks first


def _args(n=4, m=6):
    pos, q, cell = torch.rand(n, 3), torch.rand(n), torch.eye(3)[None] * 10
    nm = torch.full((n, m), n, dtype=torch.int32)
    return pos, q, torch.full((n,), 0.5), cell, nm, torch.zeros((n, m, 3), dtype=torch.int32)


def test_exported_with_the_documented_signature():
    import nvalchemiops.interactions.electrostatics as E
    from nvalchemiops.interactions.electrostatics.gaussian import gaussian_charge_correction

    assert "gaussian_charge_correction" in E.__all__ and E.gaussian_charge_correction is gaussian_charge_correction
    params = inspect.signature(gaussian_charge_correction).parameters
    assert list(params) == ["positions", "charges", "sigma", "cell", "neighbor_list", "neighbor_ptr", "neighbor_shifts", "neighbor_matrix",
                            "neighbor_matrix_shifts", "mask_value", "batch_idx", "self_energy", "neutralizing_background", "compute_forces",
                            "compute_charge_gradients", "compute_sigma_gradients", "compute_virial"]
    assert params["cell"].default is None and params["cell"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    for name in list(params)[4:]:
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert params["mask_value"].default == -1 and params["self_energy"].default is True and params["neutralizing_background"].default is True
    for name in ("compute_forces", "compute_charge_gradients", "compute_sigma_gradients", "compute_virial"):
        assert params[name].default is False
    assert "FULL" in gaussian_charge_correction.__doc__  # the full-list requirement is stated


def test_existing_signatures_are_untouched():
    from nvalchemiops.interactions.electrostatics import ewald_summation, particle_mesh_ewald

    assert "sigma" not in inspect.signature(ewald_summation).parameters and "sigma" not in inspect.signature(particle_mesh_ewald).parameters


def test_argument_errors_carry_ewald_real_space_messages():
    from nvalchemiops.interactions.electrostatics import ewald_real_space, gaussian_charge_correction as gcc

    pos, q, sig, cell, nm, sh = _args()
    lst, ptr, lsh = torch.zeros((2, 3), dtype=torch.int32), torch.zeros(5, dtype=torch.int32), torch.zeros((3, 3), dtype=torch.int32)
    alpha = torch.tensor([0.3])
    # the same misuse raises the same message from both functions
    for kw in (dict(), dict(neighbor_list=lst), dict(neighbor_matrix=nm[:3], neighbor_matrix_shifts=sh),
               dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh[:, :5]), dict(neighbor_list=lst[:1], neighbor_ptr=ptr),
               dict(neighbor_list=lst, neighbor_ptr=ptr[:4], neighbor_shifts=lsh), dict(neighbor_list=lst, neighbor_ptr=ptr, neighbor_shifts=lsh[:2]),
               dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh, batch_idx=torch.zeros(3, dtype=torch.int32))):
        with pytest.raises(ValueError) as theirs:
            ewald_real_space(pos, q, cell, alpha, **kw)
        with pytest.raises(ValueError) as ours:
            gcc(pos, q, sig, cell, **kw)
        assert str(ours.value) == str(theirs.value), kw
    with pytest.raises(ValueError, match="Either neighbor_list or neighbor_matrix must be provided"):
        gcc(pos, q, sig, cell)
    with pytest.raises(ValueError, match="neighbor_ptr is required when using neighbor_list format"):
        gcc(pos, q, sig, cell, neighbor_list=lst)
    with pytest.raises(ValueError, match=r"charges must have one entry per atom: expected shape \[4\]"):
        gcc(pos, q[:3], sig, cell, neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    with pytest.raises(ValueError, match=r"cell must have shape \[3, 3\] or \[num_systems, 3, 3\]"):
        gcc(pos, q, sig, torch.eye(4), neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    with pytest.raises(ValueError, match="Unsupported dtype"):
        gcc(pos.half(), q, sig, cell, neighbor_matrix=nm, neighbor_matrix_shifts=sh)


def test_sigma_shape_and_cell_less_rules():
    from nvalchemiops.interactions.electrostatics import gaussian_charge_correction as gcc

    pos, q, sig, cell, nm, sh = _args()
    for bad in (sig[:3], torch.full((5,), 0.5), torch.full((4, 1), 0.5)):
        with pytest.raises(ValueError, match=r"sigma must have one entry per atom: expected shape \[4\]"):
            gcc(pos, q, bad, cell, neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    with pytest.raises(ValueError, match="neighbor shifts need a cell"):
        gcc(pos, q, sig, None, neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    with pytest.raises(ValueError, match="neighbor shifts need a cell"):
        gcc(pos, q, sig, neighbor_list=torch.zeros((2, 3), dtype=torch.int32), neighbor_ptr=torch.zeros(5, dtype=torch.int32),
            neighbor_shifts=torch.zeros((3, 3), dtype=torch.int32))
    with pytest.raises(ValueError, match="compute_virial needs a cell"):
        gcc(pos, q, sig, None, neighbor_matrix=nm, compute_virial=True)
    with pytest.raises(ValueError, match="compute_virial needs a cell"):  # ... also for an empty system
        gcc(pos[:0], q[:0], sig[:0], None, neighbor_matrix=nm[:0], compute_virial=True)


def test_no_cpu_fallback():
    from nvalchemiops.interactions.electrostatics import gaussian_charge_correction as gcc

    pos, q, sig, cell, nm, sh = _args()
    for sigma in (sig, 0.5, torch.tensor(0.5)):  # [N], Python float, 0-d tensor all get as far as the device check
        with pytest.raises(C.NativeLibraryError, match="ROCm devices only"):
            gcc(pos, q, sigma, cell, neighbor_matrix=nm, neighbor_matrix_shifts=sh, compute_forces=True)
    with pytest.raises(C.NativeLibraryError):
        gcc(pos, q, sig, None, neighbor_list=torch.zeros((2, 0), dtype=torch.int32), neighbor_ptr=torch.zeros(5, dtype=torch.int32))
    with pytest.raises(C.NativeLibraryError):  # through the autograd op as well
        gcc(pos.clone().requires_grad_(True), q, sig, cell, neighbor_matrix=nm, neighbor_matrix_shifts=sh)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_zero_atoms_and_empty_lists_return_zeros_of_the_right_shapes(dtype):
    from nvalchemiops.interactions.electrostatics import gaussian_charge_correction as gcc

    every = dict(compute_forces=True, compute_charge_gradients=True, compute_sigma_gradients=True, compute_virial=True)
    z = torch.zeros(0, dtype=dtype)
    cell2 = torch.eye(3, dtype=dtype).repeat(2, 1, 1) * 9
    out = gcc(torch.zeros((0, 3), dtype=dtype), z, z, cell2, neighbor_matrix=torch.zeros((0, 5), dtype=torch.int32),
              neighbor_matrix_shifts=torch.zeros((0, 5, 3), dtype=torch.int32), batch_idx=torch.zeros(0, dtype=torch.int32), **every)
    assert [tuple(o.shape) for o in out] == [(0,), (0, 3), (0,), (0,), (2, 3, 3)] and all(o.dtype == dtype for o in out)
    e = gcc(torch.zeros((0, 3), dtype=dtype), z, 0.5, neighbor_list=torch.zeros((2, 0), dtype=torch.int32), neighbor_ptr=torch.zeros(1, dtype=torch.int32))
    assert isinstance(e, torch.Tensor) and e.shape == (0,)
    e, cg = gcc(torch.zeros((0, 3), dtype=dtype), z, z, neighbor_matrix=torch.zeros((0, 0), dtype=torch.int32), compute_charge_gradients=True)
    assert e.shape == (0,) and cg.shape == (0,)
    # an empty list: no pair term.  With the self and background terms switched off nothing is left, and nothing is launched
    pos, q, sig = torch.rand(4, 3, dtype=dtype), torch.rand(4, dtype=dtype), torch.full((4,), 0.5, dtype=dtype)
    for kw in (dict(neighbor_list=torch.zeros((2, 0), dtype=torch.int32), neighbor_ptr=torch.zeros(5, dtype=torch.int32)),
               dict(neighbor_matrix=torch.zeros((4, 0), dtype=torch.int32), neighbor_matrix_shifts=torch.zeros((4, 0, 3), dtype=torch.int32))):
        out = gcc(pos, q, sig, cell2[:1], self_energy=False, neutralizing_background=False, **every, **kw)
        assert [tuple(o.shape) for o in out] == [(4,), (4, 3), (4,), (4,), (1, 3, 3)]
        assert all(o.dtype == dtype and float(o.abs().max()) == 0.0 for o in out)


def _call(**over):
    a = dict(pos=P, q=P, sigma=P, cell=P, bi=None, w=None, n=4, nsys=1, dtype=C.MI_F64, idx=P, ush=P, nptr=None, m=6, mask=-1, flags=1, e=P, f=P,
             cg=None, sg=None, part=None, scratch=P, sbytes=1 << 20)
    a.update(over)
    return C.lib().mi_gaussian_charges(a["pos"], a["q"], a["sigma"], a["cell"], a["bi"], a["w"], a["n"], a["nsys"], a["dtype"], a["idx"], a["ush"],
                                       a["nptr"], a["m"], a["mask"], a["flags"], a["e"], a["f"], a["cg"], a["sg"], a["part"], a["scratch"],
                                       ctypes.c_size_t(a["sbytes"]), None)


def test_c_entry_point_rejects_bad_arguments_before_any_device_call():
    err = lambda: C.lib().mi_last_error().decode()  # noqa: E731
    for bad, fragment in ((dict(n=-1), "n_atoms"), (dict(nsys=0), "n_systems"), (dict(nsys=-3), "n_systems"), (dict(m=-1), "max_neighbors"),
                          (dict(dtype=2), "dtype"), (dict(dtype=-1), "dtype"), (dict(pos=None), "null pointer"), (dict(q=None), "null pointer"),
                          (dict(sigma=None), "null pointer"), (dict(idx=None), "null pointer"), (dict(f=None), "forces output"),
                          (dict(flags=2), "charge gradient output"), (dict(flags=4), "sigma gradient output"), (dict(flags=8), "system_partial"),
                          (dict(flags=16, cell=None, ush=None, part=P), "cell"), (dict(flags=24, part=P), "separate modes"),
                          (dict(nsys=2), "batch_idx"), (dict(cell=None), "unit_shifts without a cell"), (dict(scratch=None), "scratch"),
                          (dict(sbytes=16), "scratch"), (dict(e=None, flags=0), "nothing to compute")):
        assert _call(**bad) == MI_EINVAL, bad
        assert "invalid argument" in err() and fragment in err(), (bad, err())
    # nothing to do: MI_OK without looking at the pointers
    assert _call(n=0, pos=None, q=None, sigma=None, idx=None, e=None, f=None, scratch=None, sbytes=0) == MI_OK
    lib = C.lib()
    sums = lambda q=P, sg=P, bi=None, n=4, nsys=1, dtype=C.MI_F64, part=P: lib.mi_gaussian_charges_system_sums(q, sg, None, bi, n, nsys, dtype, part, None)  # noqa: E731
    for bad, fragment in ((dict(n=-1), "n_atoms"), (dict(nsys=0), "n_systems"), (dict(dtype=3), "dtype"), (dict(nsys=2), "batch_idx"),
                          (dict(q=None), "null pointer"), (dict(sg=None), "null pointer"), (dict(part=None), "null pointer")):
        assert sums(**bad) == MI_EINVAL and fragment in err(), (bad, err())
    assert lib.mi_gaussian_charges_scratch_bytes(0, C.MI_F64) == 0 and lib.mi_gaussian_charges_scratch_bytes(-5, C.MI_F32) == 0
    b32, b64 = lib.mi_gaussian_charges_scratch_bytes(1000, C.MI_F32), lib.mi_gaussian_charges_scratch_bytes(1000, C.MI_F64)
    words = lib.mi_gaussian_charges_row_words()
    assert words >= 9 and lib.mi_gaussian_charges_blocks() >= 1 and b64 > b32 >= 1000 * (5 * 4 + words * 8)


def test_header_declares_and_library_exports_the_entry_points():
    from tools.abi_symbols import declared_symbols

    declared = declared_symbols()
    for name in ("mi_gaussian_charges", "mi_gaussian_charges_scratch_bytes", "mi_gaussian_charges_blocks", "mi_gaussian_charges_row_words",
                 "mi_gaussian_charges_system_sums"):
        assert name in declared and hasattr(C.lib(), name), name
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nvalchemiops_hip.h")).read()
    for flag in ("MI_GC_FORCES 1", "MI_GC_CHARGE_GRAD 2", "MI_GC_SIGMA_GRAD 4", "MI_GC_VIRIAL 8", "MI_GC_CELL_GRAD 16"):
        assert "#define " + flag in header


def test_custom_ops_are_registered_with_fake_implementations():
    from nvalchemiops import _eops  # noqa: F401

    schema = str(torch.ops.alchemiops._gaussian_charge_correction.default._schema)
    for arg in ("Tensor sigma", "Tensor? cell", "Tensor? batch_idx", "Tensor? neighbor_list", "Tensor? neighbor_matrix", "Int mask_value",
                "bool self_energy", "bool compute_virial"):
        assert arg in schema, (arg, schema)
    assert "Tensor grad_energies" in str(torch.ops.nvalchemiops.gaussian_charge_correction_backward.default._schema)
    # fake (meta) implementations give the shapes and the dtype of the inputs
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        pos, q, sig, cell = torch.empty((7, 3)), torch.empty(7), torch.empty(7), torch.empty((2, 3, 3))
        bi, nm, sh = torch.empty(7, dtype=torch.int32), torch.empty((7, 5), dtype=torch.int32), torch.empty((7, 5, 3), dtype=torch.int32)
        out = torch.ops.alchemiops._gaussian_charge_correction(pos, q, sig, cell, bi, None, None, None, nm, sh, -1, True, True, True, False, True, True)
        assert [tuple(o.shape) for o in out] == [(7,), (7, 3), (0,), (7,), (2, 3, 3)] and all(o.dtype == torch.float32 for o in out)
        g = torch.ops.nvalchemiops.gaussian_charge_correction_backward(pos, q, sig, None, None, None, None, None, nm, None, -1, True, False, q)
        assert [tuple(o.shape) for o in g] == [(7, 3), (7,), (7,), (0,)] and all(o.dtype == torch.float64 for o in g)
