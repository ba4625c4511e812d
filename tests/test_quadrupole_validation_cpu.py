"""The point-quadrupole Ewald term: what can be checked without a GPU -- exports, signatures, every argument error and its message (those of the
dipole routines), the quadrupole shape error, the doc-string phrases, the absence of a CPU path, empty inputs, the C ABI (declared, exported,
sized, argument checks that return before any device call) and the custom ops."""
import ctypes
import inspect
import os

import pytest
import torch

from nvalchemiops import _capi as C

MI_OK, MI_EINVAL = 0, -1  # include/nvalchemiops_hip.h
P = ctypes.c_void_p(4096)  # a non-null pointer that is never dereferenced: every call below fails its checks first
FLAGS = ("compute_forces", "compute_charge_gradients", "compute_dipole_gradients", "compute_quadrupole_gradients", "compute_virial")
LISTS = ["neighbor_list", "neighbor_ptr", "neighbor_shifts", "neighbor_matrix", "neighbor_matrix_shifts"]


def _args(n=4, m=6):
    pos, q, mu, qd, cell = torch.rand(n, 3), torch.rand(n), torch.rand(n, 3), torch.rand(n, 3, 3), torch.eye(3)[None] * 10
    return pos, q, mu, qd, cell, torch.full((n, m), n, dtype=torch.int32), torch.zeros((n, m, 3), dtype=torch.int32)


def _api():
    from nvalchemiops.interactions.electrostatics import (ewald_quadrupole_correction, ewald_quadrupole_real_space,
                                                          ewald_quadrupole_reciprocal_space)

    return ewald_quadrupole_correction, ewald_quadrupole_real_space, ewald_quadrupole_reciprocal_space


def test_exported_with_the_documented_signatures():
    import nvalchemiops.interactions.electrostatics as E
    from nvalchemiops.interactions.electrostatics import dipole as D
    from nvalchemiops.interactions.electrostatics import quadrupole as Q

    for name in ("ewald_quadrupole_real_space", "ewald_quadrupole_reciprocal_space", "ewald_quadrupole_correction"):
        assert name in E.__all__ and name in Q.__all__ and getattr(E, name) is getattr(Q, name)
    real = inspect.signature(Q.ewald_quadrupole_real_space).parameters
    assert list(real) == ["positions", "charges", "dipoles", "quadrupoles", "cell", "alpha"] + LISTS + ["mask_value", "batch_idx"] + list(FLAGS)
    assert real["mask_value"].default == -1
    recip = inspect.signature(Q.ewald_quadrupole_reciprocal_space).parameters
    assert list(recip) == ["positions", "charges", "dipoles", "quadrupoles", "cell", "k_vectors", "alpha", "batch_idx"] + list(FLAGS)
    both = inspect.signature(Q.ewald_quadrupole_correction).parameters
    assert list(both) == (["positions", "charges", "dipoles", "quadrupoles", "cell", "alpha", "k_vectors", "k_cutoff", "batch_idx"] + LISTS
                          + ["mask_value"] + list(FLAGS) + ["accuracy"])
    assert both["alpha"].default is None and both["mask_value"].default is None and both["accuracy"].default == 1e-6
    for params in (real, recip, both):
        assert all(params[f].default is False for f in FLAGS)
    # the dipole routines' arguments, with `quadrupoles` after `dipoles` and its flag after the dipole flag
    without = lambda sig: [p for p in sig if p not in ("quadrupoles", "compute_quadrupole_gradients")]  # noqa: E731
    assert without(real) == list(inspect.signature(D.ewald_dipole_real_space).parameters)
    assert without(recip) == list(inspect.signature(D.ewald_dipole_reciprocal_space).parameters)
    assert without(both) == list(inspect.signature(D.ewald_dipole_correction).parameters)
    for fn in (Q.ewald_quadrupole_real_space, Q.ewald_quadrupole_correction):
        assert "MUST BE FULL" in fn.__doc__
    for fn in (Q.ewald_quadrupole_real_space, Q.ewald_quadrupole_reciprocal_space, Q.ewald_quadrupole_correction):
        doc = fn.__doc__
        assert "MODEL" not in doc and "RETURNS" not in doc
        for phrase in ("Q = Theta / 3", "1/2 sum q d d", "ADDED", "NOT symmetric", "4 alpha^3 / (3 sqrt(pi))", "4 alpha^5 / (5 sqrt(pi))",
                       "1/2 (Q + Q^T)", "tin-foil", "B4 s_i s_j", "does not depend on the dipoles", "external_field", "dipoles=None",
                       "cell and alpha\n    are out of scope", "quadrupoles on the mesh"):
            assert phrase in doc, (fn.__name__, phrase)
    doc = Q.ewald_quadrupole_correction.__doc__
    assert all(name in doc for name in ("ewald_summation", "particle_mesh_ewald", "ewald_dipole_correction", "pme_dipole_correction"))
    # the older doc strings point to the new routine and keep their word
    for fn in (D.ewald_dipole_correction, E.pme_dipole_correction, E.induced_dipoles):
        assert "quadrupoles" in fn.__doc__ and "ewald_quadrupole_correction" in fn.__doc__, fn.__name__


def test_argument_errors_carry_the_dipole_routines_messages():
    from nvalchemiops.interactions.electrostatics import ewald_dipole_correction, ewald_dipole_real_space

    both, real, recip = _api()
    pos, q, mu, qd, cell, nm, sh = _args()
    lst, ptr, lsh = torch.zeros((2, 3), dtype=torch.int32), torch.zeros(5, dtype=torch.int32), torch.zeros((3, 3), dtype=torch.int32)
    for kw in (dict(), dict(neighbor_list=lst), dict(neighbor_matrix=nm[:3], neighbor_matrix_shifts=sh),
               dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh[:, :5]), dict(neighbor_list=lst[:1], neighbor_ptr=ptr),
               dict(neighbor_list=lst, neighbor_ptr=ptr[:4], neighbor_shifts=lsh), dict(neighbor_list=lst, neighbor_ptr=ptr, neighbor_shifts=lsh[:2]),
               dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh, batch_idx=torch.zeros(3, dtype=torch.int32)),
               dict(neighbor_matrix=nm, compute_virial=True)):
        with pytest.raises(ValueError) as theirs:
            ewald_dipole_real_space(pos, q, mu, cell, 0.3, **kw)
        for ours in (lambda: real(pos, q, mu, qd, cell, 0.3, **kw), lambda: both(pos, q, mu, qd, cell, 0.3, **kw),
                     lambda: real(pos, q, None, qd, cell, 0.3, **kw)):
            with pytest.raises(ValueError) as err:
                ours()
            assert str(err.value) == str(theirs.value), kw
    ok = dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    kv = torch.rand(5, 3)
    with pytest.raises(ValueError, match=r"charges must have one entry per atom: expected shape \[4\]"):
        real(pos, q[:3], mu, qd, cell, 0.3, **ok)
    with pytest.raises(ValueError, match="Unsupported dtype"):
        real(pos.half(), q, mu, qd, cell, 0.3, **ok)
    with pytest.raises(ValueError) as theirs:
        ewald_dipole_real_space(pos, q, mu, None, 0.3, neighbor_matrix=nm)
    for call in (lambda: real(pos, q, mu, qd, None, 0.3, neighbor_matrix=nm), lambda: recip(pos, q, mu, qd, None, kv, 0.3),
                 lambda: both(pos, q, mu, qd, None, 0.3, kv, neighbor_matrix=nm)):
        with pytest.raises(ValueError) as err:
            call()
        assert str(err.value) == str(theirs.value)
    with pytest.raises(ValueError, match=r"cell must have shape \[3, 3\] or \[num_systems, 3, 3\]"):
        real(pos, q, mu, qd, torch.eye(4), 0.3, **ok)
    with pytest.raises(ValueError, match="alpha has 3 values but there are 1 systems"):
        real(pos, q, mu, qd, cell, torch.tensor([0.3, 0.3, 0.3]), **ok)
    with pytest.raises(ValueError, match=r"dipoles must have one vector per atom: expected shape \[4, 3\]"):
        both(pos, q, mu[:3], qd, cell, 0.3, kv, **ok)
    with pytest.raises(ValueError, match=r"k_vectors must have shape \[K, 3\] or \[1, K, 3\]"):
        recip(pos, q, mu, qd, cell, torch.rand(5, 2), 0.3)
    with pytest.raises(ValueError, match=r"charges must have one entry per atom"):
        recip(pos, q[:2], mu, qd, cell, kv, 0.3)
    with pytest.raises(ValueError) as theirs:
        ewald_dipole_correction(pos, q, mu, cell, 0.3, kv, compute_virial=True, neighbor_list=lst, neighbor_ptr=ptr)
    with pytest.raises(ValueError) as err:
        both(pos, q, mu, qd, cell, 0.3, kv, compute_virial=True, neighbor_list=lst, neighbor_ptr=ptr)
    assert str(err.value) == str(theirs.value)


def test_quadrupole_shape_error():
    both, real, recip = _api()
    pos, q, mu, qd, cell, nm, sh = _args()
    kv = torch.rand(5, 3)
    for bad in (qd[:3], qd[:, :2], qd.reshape(4, 9), qd[:, :, :2], torch.rand(4, 6), torch.rand(5, 3, 3), torch.rand(4, 3, 3, 1)):
        for call in (lambda: real(pos, q, mu, bad, cell, 0.3, neighbor_matrix=nm, neighbor_matrix_shifts=sh),
                     lambda: recip(pos, q, mu, bad, cell, kv, 0.3),
                     lambda: both(pos, q, None, bad, cell, 0.3, kv, neighbor_matrix=nm, neighbor_matrix_shifts=sh)):
            with pytest.raises(ValueError, match=r"quadrupoles must have one 3 x 3 tensor per atom: expected shape \[4, 3, 3\]"):
                call()


def test_no_cpu_fallback():
    both, real, recip = _api()
    pos, q, mu, qd, cell, nm, sh = _args()
    kv = torch.rand(5, 3)
    ok = dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    with pytest.raises(C.NativeLibraryError, match="ROCm devices only"):
        real(pos, q, mu, qd, cell, 0.3, compute_forces=True, **ok)
    with pytest.raises(C.NativeLibraryError, match="ROCm devices only"):
        recip(pos, q, None, qd, cell, kv, 0.3, compute_quadrupole_gradients=True)
    with pytest.raises(C.NativeLibraryError, match="ROCm devices only"):
        both(pos, q, mu, qd, cell, 0.3, kv, **ok)
    with pytest.raises(C.NativeLibraryError, match="ROCm devices only"):  # ... before the parameters are estimated
        both(pos, q, mu, qd, cell, **ok)
    with pytest.raises(C.NativeLibraryError):  # through the autograd ops as well
        real(pos, q, mu, qd.clone().requires_grad_(True), cell, 0.3, **ok)
    with pytest.raises(C.NativeLibraryError):
        recip(pos.clone().requires_grad_(True), q, mu, qd, cell, kv, 0.3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_zero_atoms_return_zeros_of_the_right_shapes(dtype):
    both, real, recip = _api()
    every = {f: True for f in FLAGS}
    z, z3, z33 = torch.zeros(0, dtype=dtype), torch.zeros((0, 3), dtype=dtype), torch.zeros((0, 3, 3), dtype=dtype)
    cell2 = torch.eye(3, dtype=dtype).repeat(2, 1, 1) * 9
    lists = dict(neighbor_matrix=torch.zeros((0, 5), dtype=torch.int32), neighbor_matrix_shifts=torch.zeros((0, 5, 3), dtype=torch.int32))
    bi = torch.zeros(0, dtype=torch.int32)
    kv = torch.rand(2, 7, 3, dtype=dtype)
    for out in (real(z3, z, z3, z33, cell2, 0.3, batch_idx=bi, **lists, **every), recip(z3, z, z3, z33, cell2, kv, 0.3, batch_idx=bi, **every),
                both(z3, z, None, z33, cell2, 0.3, kv, batch_idx=bi, **lists, **every)):
        assert [tuple(o.shape) for o in out] == [(0,), (0, 3), (0,), (0, 3), (0, 3, 3), (2, 3, 3)] and all(o.dtype == dtype for o in out)
    e = real(z3, z, z3, z33, cell2[:1], 0.3, **lists)
    assert isinstance(e, torch.Tensor) and e.shape == (0,)
    e, qg = recip(z3, z, z3, z33, cell2[:1], kv[0], 0.3, compute_quadrupole_gradients=True)
    assert e.shape == (0,) and qg.shape == (0, 3, 3)


def _real(**over):
    a = dict(pos=P, q=P, mu=P, qd=P, cell=P, alpha=P, bi=None, w=None, n=4, nsys=1, dtype=C.MI_F64, idx=P, ush=P, nptr=None, m=6, mask=-1, flags=1,
             e=P, f=P, cg=None, dg=None, qg=None, part=None, scratch=P, sbytes=1 << 20)
    a.update(over)
    return C.lib().mi_ewald_quadrupole_real(a["pos"], a["q"], a["mu"], a["qd"], a["cell"], a["alpha"], a["bi"], a["w"], a["n"], a["nsys"], a["dtype"],
                                            a["idx"], a["ush"], a["nptr"], a["m"], a["mask"], a["flags"], a["e"], a["f"], a["cg"], a["dg"], a["qg"],
                                            a["part"], a["scratch"], ctypes.c_size_t(a["sbytes"]), None)


def test_c_entry_points_reject_bad_arguments_before_any_device_call():
    lib = C.lib()
    err = lambda: lib.mi_last_error().decode()  # noqa: E731
    for bad, fragment in ((dict(n=-1), "n_atoms"), (dict(nsys=0), "n_systems"), (dict(nsys=70000, bi=P), "n_systems"), (dict(m=-1), "max_neighbors"),
                          (dict(dtype=2), "dtype"), (dict(dtype=-1), "dtype"), (dict(pos=None), "null pointer"), (dict(q=None), "null pointer"),
                          (dict(mu=None), "null pointer"), (dict(qd=None), "null pointer"), (dict(cell=None), "null pointer"),
                          (dict(alpha=None), "null pointer"), (dict(idx=None), "null pointer"), (dict(f=None), "forces output"),
                          (dict(flags=2), "charge gradient output"), (dict(flags=4), "dipole gradient output"),
                          (dict(flags=16), "quadrupole gradient output"), (dict(flags=8), "virial_partial"),
                          (dict(flags=8, part=P, ush=None), "unit_shifts"), (dict(nsys=2), "batch_idx"), (dict(scratch=None), "scratch"),
                          (dict(sbytes=16), "scratch"), (dict(e=None, flags=0), "nothing to compute")):
        assert _real(**bad) == MI_EINVAL, bad
        assert "invalid argument" in err() and fragment in err(), (bad, err())
    assert _real(n=0, pos=None, q=None, mu=None, qd=None, idx=None, e=None, f=None, scratch=None, sbytes=0) == MI_OK  # nothing to do
    sf = lambda pos=P, q=P, mu=P, qd=P, kv=P, sp=None, n=4, nsys=1, nk=3, dtype=C.MI_F64, table=P: lib.mi_ewald_quadrupole_structure_factors(  # noqa: E731
        pos, q, mu, qd, None, kv, sp, n, nsys, nk, dtype, table, None, None)
    for bad, fragment in ((dict(n=-1), "n_atoms"), (dict(nk=-1), "n_k"), (dict(nsys=0), "n_systems"), (dict(nsys=2), "system_ptr"),
                          (dict(dtype=5), "dtype"), (dict(table=None), "null pointer"), (dict(kv=None), "null pointer"), (dict(mu=None), "null pointer"),
                          (dict(qd=None), "null pointer")):
        assert sf(**bad) == MI_EINVAL and fragment in err(), (bad, err())
    assert sf(nk=0, table=None, kv=None) == MI_OK
    ga = lambda pos=P, qd=P, kv=P, cell=P, bi=None, table=P, tg=None, w=None, n=4, nsys=1, nk=3, dtype=C.MI_F64, e=P: lib.mi_ewald_quadrupole_recip_gather(  # noqa: E731
        pos, P, P, qd, kv, cell, P, bi, table, tg, w, n, nsys, nk, dtype, e, None, None, None, None, None)
    for bad, fragment in ((dict(dtype=2), "dtype"), (dict(n=-1), "n_atoms"), (dict(nsys=0), "n_systems"), (dict(nsys=2), "batch_idx"),
                          (dict(tg=P), "come together"), (dict(w=P), "come together"), (dict(pos=None), "null pointer"), (dict(qd=None), "null pointer"),
                          (dict(cell=None), "null pointer"), (dict(table=None), "null pointer"), (dict(kv=None), "null pointer"),
                          (dict(e=None), "nothing to compute")):
        assert ga(**bad) == MI_EINVAL and fragment in err(), (bad, err())
    assert ga(n=0, pos=None) == MI_OK
    vi = lambda table=P, tv=P, kv=P, cell=P, alpha=P, nsys=1, nk=3, dtype=C.MI_F64, out=P: lib.mi_ewald_quadrupole_recip_virial(  # noqa: E731
        table, tv, kv, cell, alpha, nsys, nk, dtype, out, None)
    for bad, fragment in ((dict(dtype=2), "dtype"), (dict(nsys=0), "n_systems"), (dict(nk=-1), "n_k"), (dict(out=None), "null pointer"),
                          (dict(table=None), "null pointer"), (dict(tv=None), "null pointer"), (dict(cell=None), "null pointer"),
                          (dict(alpha=None), "null pointer")):
        assert vi(**bad) == MI_EINVAL and fragment in err(), (bad, err())
    # sizes: one 64 / 128 byte record and nine virial words per atom; the fold is in blocks
    assert lib.mi_ewald_quadrupole_real_scratch_bytes(0, C.MI_F64) == 0 and lib.mi_ewald_quadrupole_real_scratch_bytes(-5, C.MI_F32) == 0
    b32, b64 = lib.mi_ewald_quadrupole_real_scratch_bytes(1000, C.MI_F32), lib.mi_ewald_quadrupole_real_scratch_bytes(1000, C.MI_F64)
    assert 1000 * (64 + 72) <= b32 < 1000 * (64 + 72) + 1024 and 1000 * (128 + 72) <= b64 < 1000 * (128 + 72) + 1024
    assert lib.mi_ewald_quadrupole_blocks() >= 1


def test_header_declares_and_library_exports_the_entry_points():
    from tools.abi_symbols import declared_symbols

    declared = declared_symbols()
    for name in ("mi_ewald_quadrupole_real", "mi_ewald_quadrupole_real_scratch_bytes", "mi_ewald_quadrupole_blocks",
                 "mi_ewald_quadrupole_structure_factors", "mi_ewald_quadrupole_recip_gather", "mi_ewald_quadrupole_recip_virial"):
        assert name in declared and hasattr(C.lib(), name), name
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "nvalchemiops_hip.h")).read()
    for flag in ("MI_QD_FORCES 1", "MI_QD_CHARGE_GRAD 2", "MI_QD_DIPOLE_GRAD 4", "MI_QD_VIRIAL 8", "MI_QD_QUADRUPOLE_GRAD 16"):
        assert "#define " + flag in header
    import importlib.util

    spec = importlib.util.spec_from_file_location("build_native", os.path.join(root, "nvalchemi-toolkit-ops_amd", "build_native.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.SOURCES["quadrupole.hip"] == [] and os.path.exists(os.path.join(mod.CSRC, "quadrupole.hip"))


def test_custom_ops_are_registered_with_fake_implementations():
    from nvalchemiops import _eops  # noqa: F401

    real = str(torch.ops.alchemiops._ewald_quadrupole_real_space.default._schema)
    for arg in ("Tensor dipoles", "Tensor quadrupoles", "Tensor cell", "Tensor alpha", "Tensor? batch_idx", "Tensor? neighbor_list",
                "Tensor? neighbor_matrix_shifts", "int mask_value", "bool compute_quadrupole_gradients", "bool compute_virial"):
        assert arg.lower() in real.lower(), (arg, real)
    recip = str(torch.ops.alchemiops._ewald_quadrupole_reciprocal_space.default._schema)
    for arg in ("Tensor quadrupoles", "Tensor k_vectors", "Tensor alpha", "Tensor? batch_idx", "bool compute_quadrupole_gradients", "bool compute_virial"):
        assert arg in recip, (arg, recip)
    assert "Tensor grad_energies" in str(torch.ops.nvalchemiops.ewald_quadrupole_real_space_backward.default._schema)
    assert "Tensor grad_energies" in str(torch.ops.nvalchemiops.ewald_quadrupole_reciprocal_space_backward.default._schema)
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        pos, q, mu, qd, cell, al = torch.empty((7, 3)), torch.empty(7), torch.empty((7, 3)), torch.empty((7, 3, 3)), torch.empty((2, 3, 3)), torch.empty(2)
        bi, nm, sh = torch.empty(7, dtype=torch.int32), torch.empty((7, 5), dtype=torch.int32), torch.empty((7, 5, 3), dtype=torch.int32)
        out = torch.ops.alchemiops._ewald_quadrupole_real_space(pos, q, mu, qd, cell, al, bi, None, None, None, nm, sh, -1, True, False, True, True, True)
        assert [tuple(o.shape) for o in out] == [(7,), (7, 3), (0,), (7, 3), (7, 3, 3), (2, 3, 3)] and all(o.dtype == torch.float32 for o in out)
        out = torch.ops.alchemiops._ewald_quadrupole_reciprocal_space(pos, q, mu, qd, cell, torch.empty((2, 11, 3)), al, bi, False, True, False, True, True)
        assert [tuple(o.shape) for o in out] == [(7,), (0,), (7,), (0,), (7, 3, 3), (2, 3, 3)] and all(o.dtype == torch.float32 for o in out)
        g = torch.ops.nvalchemiops.ewald_quadrupole_real_space_backward(pos, q, mu, qd, cell, al, None, None, None, None, nm, None, -1, q)
        assert [tuple(o.shape) for o in g] == [(7, 3), (7,), (7, 3), (7, 3, 3)] and all(o.dtype == torch.float64 for o in g)
        g = torch.ops.nvalchemiops.ewald_quadrupole_reciprocal_space_backward(pos, q, mu, qd, cell, torch.empty((2, 11, 3)), al, bi, q)
        assert [tuple(o.shape) for o in g] == [(7, 3), (7,), (7, 3), (7, 3, 3)] and all(o.dtype == torch.float64 for o in g)
