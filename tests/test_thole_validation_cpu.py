"""`thole_dipole_correction` and `thole_induced_dipoles`: what can be checked without a GPU -- export, signature, every argument error (raised
before anything is launched), the absence of a CPU path, empty inputs, and the argument checks of the C entry points (which return before
any device call)."""
import ctypes
import inspect

import pytest
import torch

from nvalchemiops import _capi as C

MI_OK, MI_EINVAL = 0, -1  # include/nvalchemiops_hip.h
P = ctypes.c_void_p(4096)  # a non-null pointer that is never dereferenced: every call below fails its checks first
THOLE_SYMBOLS = ("mi_thole_dipole", "mi_thole_dipole_scratch_bytes", "mi_thole_dipole_blocks", "mi_thole_induced_pair_tensors")


def _args(n=4, m=6):
    pos, q, mu, cell = torch.rand(n, 3), torch.rand(n), torch.rand(n, 3), torch.eye(3)[None] * 10
    nm = torch.full((n, m), n, dtype=torch.int32)
    return pos, q, mu, torch.full((n,), 0.2), cell, nm, torch.zeros((n, m, 3), dtype=torch.int32)


def _api():
    from nvalchemiops.interactions.electrostatics import thole_dipole_correction, thole_induced_dipoles

    return thole_dipole_correction, thole_induced_dipoles


def test_exported_with_the_documented_signature():
    import nvalchemiops.interactions.electrostatics as E
    from nvalchemiops.interactions.electrostatics.thole import thole_dipole_correction

    assert "thole_dipole_correction" in E.__all__ and E.thole_dipole_correction is thole_dipole_correction
    params = inspect.signature(thole_dipole_correction).parameters
    assert list(params) == ["positions", "charges", "dipoles", "polarizability", "cell", "thole", "neighbor_list", "neighbor_ptr", "neighbor_shifts",
                            "neighbor_matrix", "neighbor_matrix_shifts", "mask_value", "batch_idx", "compute_forces", "compute_charge_gradients",
                            "compute_dipole_gradients", "compute_polarizability_gradients", "compute_virial"]
    for name in list(params)[5:]:
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert params["thole"].default == 0.39 and params["cell"].default is None and params["mask_value"].default == -1
    assert all(params[name].default is False for name in params if name.startswith("compute_"))
    # the damped solve: the arguments of `induced_dipoles`, which keeps its own list, plus `thole` as the first keyword
    assert "thole_induced_dipoles" in E.__all__
    plain, damped = inspect.signature(E.induced_dipoles).parameters, inspect.signature(E.thole_induced_dipoles).parameters
    assert "thole" not in plain and list(damped) == list(plain)[:4] + ["thole"] + list(plain)[4:]
    assert damped["thole"].default == 0.39 and damped["thole"].kind is inspect.Parameter.KEYWORD_ONLY
    assert all(damped[k].default == plain[k].default and damped[k].kind == plain[k].kind for k in plain)
    assert "thole_dipole_correction" in E.thole_induced_dipoles.__doc__ and "thole_induced_dipoles" in E.induced_dipoles.__doc__
    assert "FULL" in thole_dipole_correction.__doc__


def test_thole_width_must_be_finite_and_positive():
    th, ind = _api()
    pos, q, mu, a, cell, nm, sh = _args()
    per = dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    for bad in (0.0, -0.39, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="thole must be finite and positive"):
            th(pos, q, mu, a, cell, thole=bad, **per)
        with pytest.raises(ValueError, match="thole must be finite and positive"):
            ind(pos, q, a, cell, thole=bad, **per)
    for bad in ("0.39", None, True, torch.tensor(0.39)):
        with pytest.raises(TypeError, match="thole must be a number"):
            th(pos, q, mu, a, cell, thole=bad, **per)
    for bad in ("0.39", True):
        with pytest.raises(TypeError, match="thole must be a number"):
            ind(pos, q, a, cell, thole=bad, **per)


def test_list_errors_carry_the_messages_of_the_dipole_functions():
    from nvalchemiops.interactions.electrostatics import ewald_dipole_real_space as real

    th, _ = _api()
    pos, q, mu, a, cell, nm, sh = _args()
    lst, ptr, lsh = torch.zeros((2, 3), dtype=torch.int32), torch.zeros(5, dtype=torch.int32), torch.zeros((3, 3), dtype=torch.int32)
    for kw in (dict(), dict(neighbor_list=lst), dict(neighbor_matrix=nm[:3], neighbor_matrix_shifts=sh),
               dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh[:, :5]), dict(neighbor_list=lst[:1], neighbor_ptr=ptr),
               dict(neighbor_list=lst, neighbor_ptr=ptr[:4], neighbor_shifts=lsh), dict(neighbor_list=lst, neighbor_ptr=ptr, neighbor_shifts=lsh[:2]),
               dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh, batch_idx=torch.zeros(3, dtype=torch.int32)),
               dict(neighbor_matrix=nm, compute_virial=True), dict(neighbor_list=lst, neighbor_ptr=ptr, compute_virial=True)):  # a virial without shifts
        with pytest.raises(ValueError) as theirs:
            real(pos, q, mu, cell, 0.3, **kw)
        with pytest.raises(ValueError) as ours:
            th(pos, q, mu, a, cell, **kw)
        assert str(ours.value) == str(theirs.value), kw
    with pytest.raises(ValueError, match="compute_virial needs the shifts of the list"):
        th(pos, q, mu, a, cell, neighbor_matrix=nm, compute_virial=True)
    with pytest.raises(ValueError, match="ONE format"):
        th(pos, q, mu, a, cell, neighbor_matrix=nm, neighbor_list=lst, neighbor_ptr=ptr)
    with pytest.raises(ValueError, match=r"cell must have shape \[3, 3\] or \[num_systems, 3, 3\]"):
        th(pos, q, mu, a, torch.eye(4), neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    with pytest.raises(ValueError, match="Unsupported dtype"):
        th(pos.half(), q, mu, a, cell, neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    # a cluster: no shifts, no virial
    with pytest.raises(ValueError, match="neighbor shifts need a cell"):
        th(pos, q, mu, a, None, neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    with pytest.raises(ValueError, match="neighbor shifts need a cell"):
        th(pos, q, mu, a, None, neighbor_list=lst, neighbor_ptr=ptr, neighbor_shifts=lsh)
    with pytest.raises(ValueError, match="compute_virial needs a cell"):
        th(pos, q, mu, a, None, neighbor_matrix=nm, compute_virial=True)


def test_shape_errors_of_the_per_atom_arguments():
    th, ind = _api()
    pos, q, mu, a, cell, nm, sh = _args()
    per = dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    with pytest.raises(ValueError, match=r"positions must have shape \[num_atoms, 3\]"):
        th(pos[:, :2], q, mu, a, cell, **per)
    with pytest.raises(ValueError, match=r"charges must have one entry per atom: expected shape \[4\]"):
        th(pos, q[:3], mu, a, cell, **per)
    for bad in (mu[:3], torch.zeros(4), torch.zeros(4, 4)):
        with pytest.raises(ValueError, match=r"dipoles must have one vector per atom: expected shape \[4, 3\]"):
            th(pos, q, bad, a, cell, **per)
    for bad in (a[:3], torch.full((5,), 0.2), torch.full((4, 1), 0.2)):
        with pytest.raises(ValueError, match=r"polarizability must have one entry per atom: expected shape \[4\]"):
            th(pos, q, mu, bad, cell, **per)
        with pytest.raises(ValueError, match=r"polarizability must have one entry per atom: expected shape \[4\]"):
            ind(pos, q, bad, cell, thole=0.39, **per)
    with pytest.raises(TypeError, match="polarizability must be a number or torch.Tensor"):
        th(pos, q, mu, "soft", cell, **per)


def test_no_cpu_fallback():
    th, ind = _api()
    pos, q, mu, a, cell, nm, sh = _args()
    lst, ptr, lsh = torch.zeros((2, 3), dtype=torch.int32), torch.tensor([0, 1, 2, 3, 3], dtype=torch.int32), torch.zeros((3, 3), dtype=torch.int32)
    for polar in (a, 0.2, torch.tensor(0.2)):  # [N], Python float, 0-d tensor all get as far as the device check
        for kw in (dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh), dict(neighbor_list=lst, neighbor_ptr=ptr, neighbor_shifts=lsh)):
            with pytest.raises(C.NativeLibraryError, match="ROCm devices only"):
                th(pos, q, mu, polar, cell, **kw)
            with pytest.raises(C.NativeLibraryError, match="ROCm devices only"):
                ind(pos, q, polar, cell, thole=0.39, alpha=0.3, mesh_dimensions=(8, 8, 8), **kw)
    with pytest.raises(C.NativeLibraryError, match="ROCm devices only"):  # a cluster
        th(pos, q, mu, a, neighbor_matrix=nm)
    with pytest.raises(C.NativeLibraryError):  # under autograd as well
        th(pos, q, mu, a.clone().requires_grad_(True), cell, neighbor_matrix=nm)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_zero_atoms(dtype):
    th, ind = _api()
    z, z3 = torch.zeros(0, dtype=dtype), torch.zeros((0, 3), dtype=dtype)
    cell = torch.eye(3, dtype=dtype) * 9
    nm, sh = torch.zeros((0, 5), dtype=torch.int32), torch.zeros((0, 5, 3), dtype=torch.int32)
    e = th(z3, z, z3, z, cell, neighbor_matrix=nm)
    assert e.shape == (0,) and e.dtype == dtype
    out = th(z3, z, z3, 0.1, cell.repeat(2, 1, 1), neighbor_matrix=nm, neighbor_matrix_shifts=sh, batch_idx=torch.zeros(0, dtype=torch.int32),
             compute_forces=True, compute_charge_gradients=True, compute_dipole_gradients=True, compute_polarizability_gradients=True,
             compute_virial=True)
    assert [tuple(o.shape) for o in out] == [(0,), (0, 3), (0,), (0, 3), (0,), (2, 3, 3)] and all(o.dtype == dtype for o in out)
    e, pg = th(z3, z, z3, z, None, neighbor_matrix=nm, compute_polarizability_gradients=True)
    assert e.shape == (0,) and pg.shape == (0,)
    assert ind(z3, z, z, cell, thole=0.39, neighbor_matrix=nm).shape == (0, 3)


def test_c_entry_points_reject_bad_arguments_before_any_device_call():
    lib = C.lib()
    err = lambda: lib.mi_last_error().decode()  # noqa: E731

    def check(call, cases):
        for bad, fragment in cases:
            assert call(**bad) == MI_EINVAL, bad
            assert "invalid argument" in err() and fragment in err(), (bad, err())

    def thole(**over):
        a = dict(pos=P, q=P, mu=P, cell=P, pol=P, a_t=0.39, bi=None, w=None, n=4, nsys=1, dtype=C.MI_F64, idx=P, ush=P, nptr=None, m=6, mask=-1, flags=0,
                 e=P, f=None, cg=None, dg=None, pg=None, vir=None, scratch=P, nbytes=1 << 20)
        a.update(over)
        return lib.mi_thole_dipole(a["pos"], a["q"], a["mu"], a["cell"], a["pol"], ctypes.c_double(a["a_t"]), a["bi"], a["w"], a["n"], a["nsys"],
                                   a["dtype"], a["idx"], a["ush"], a["nptr"], a["m"], a["mask"], a["flags"], a["e"], a["f"], a["cg"], a["dg"], a["pg"],
                                   a["vir"], a["scratch"], ctypes.c_size_t(a["nbytes"]), None)

    check(thole, ((dict(n=-1), "n_atoms"), (dict(nsys=0), "n_systems"), (dict(nsys=65536, bi=P), "n_systems"), (dict(m=-1), "max_neighbors"),
                  (dict(dtype=2), "dtype"), (dict(nsys=2), "batch_idx"), (dict(a_t=0.0), "thole_a"), (dict(a_t=-1.0), "thole_a"),
                  (dict(a_t=float("nan")), "thole_a"), (dict(a_t=float("inf")), "thole_a"), (dict(cell=None), "unit_shifts need a cell"),
                  (dict(flags=8), "virial"), (dict(flags=8, vir=P, ush=None), "virial"), (dict(pos=None), "null pointer"),
                  (dict(q=None), "null pointer"), (dict(mu=None), "null pointer"), (dict(pol=None), "null pointer"), (dict(idx=None), "null pointer"),
                  (dict(e=None), "nothing to compute"), (dict(flags=1), "forces output"), (dict(flags=2), "charge gradient output"),
                  (dict(flags=4), "dipole gradient output"), (dict(flags=16), "polarizability gradient output"),
                  (dict(scratch=None), "scratch"), (dict(nbytes=8), "scratch")))
    assert thole(n=0, pos=None, q=None, mu=None, pol=None, idx=None, e=None, scratch=None) == MI_OK  # nothing to do
    assert lib.mi_thole_dipole_blocks() == lib.mi_ewald_dipole_blocks() == 64
    for n in (0, 1, 1000):
        for dt in (C.MI_F32, C.MI_F64):
            assert lib.mi_thole_dipole_scratch_bytes(n, dt) == lib.mi_ewald_dipole_real_scratch_bytes(n, dt)

    def tensors(**over):
        a = dict(pos=P, pol=P, cell=P, alpha=P, bi=None, n=4, nsys=1, dtype=C.MI_F64, idx=P, ush=P, nptr=None, m=6, mask=-1, slots=24, t=P, nb=P, d=P,
                 pc=P, a_t=0.39)
        a.update(over)
        return lib.mi_thole_induced_pair_tensors(a["pos"], a["pol"], a["cell"], a["alpha"], a["bi"], a["n"], a["nsys"], a["dtype"], a["idx"], a["ush"],
                                                 a["nptr"], a["m"], a["mask"], a["slots"], a["t"], a["nb"], a["d"], a["pc"], ctypes.c_double(a["a_t"]),
                                                 None)

    check(tensors, ((dict(n=-1), "n_atoms"), (dict(nsys=0), "n_systems"), (dict(m=-1), "max_neighbors"), (dict(dtype=2), "dtype"),
                    (dict(nsys=2), "batch_idx"), (dict(slots=-1), "n_slots"), (dict(slots=23), "n_atoms * max_neighbors"),
                    (dict(a_t=0.0), "thole_a"), (dict(a_t=float("nan")), "thole_a"), (dict(a_t=float("inf")), "thole_a"),
                    (dict(pos=None), "null pointer"), (dict(pol=None), "null pointer"), (dict(cell=None), "null pointer"),
                    (dict(alpha=None), "null pointer"), (dict(idx=None), "null pointer"), (dict(t=None), "null pointer"),
                    (dict(nb=None), "null pointer"), (dict(d=None), "null pointer"), (dict(pc=None), "null pointer")))
    assert tensors(n=0, slots=0, pos=None, pol=None, idx=None, t=None, nb=None, d=None, pc=None) == MI_OK  # nothing to do


def test_header_declares_and_library_exports_the_entry_points():
    from tools.abi_symbols import declared_symbols

    declared = declared_symbols()
    assert set(THOLE_SYMBOLS) <= set(declared)
    assert {s for s in declared if s.startswith("mi_thole_")} == set(THOLE_SYMBOLS)
    for name in THOLE_SYMBOLS:
        assert hasattr(C.lib(), name), name
