"""`induced_dipoles`: what can be checked without a GPU -- export, signature, every argument error (raised before anything is launched), the
absence of a CPU path, empty inputs, the refusal to be traced, and the argument checks of the C entry points (which return before any
device call)."""
import ctypes
import inspect

import pytest
import torch

from nvalchemiops import _capi as C

MI_OK, MI_EINVAL = 0, -1  # include/nvalchemiops_hip.h
P = ctypes.c_void_p(4096)  # a non-null pointer that is never dereferenced: every call below fails its checks first
P2 = ctypes.c_void_p(8192)
INDUCED_SYMBOLS = ("mi_induced_pair_tensors", "mi_induced_apply", "mi_induced_dot", "mi_induced_cg_update", "mi_induced_cg_direction",
                   "mi_induced_blocks", "mi_induced_state_words", "mi_induced_tensor_words", "mi_induced_unroll_depth")


def _args(n=4, m=6):
    pos, q, cell = torch.rand(n, 3), torch.rand(n), torch.eye(3)[None] * 10
    nm = torch.full((n, m), n, dtype=torch.int32)
    return pos, q, torch.full((n,), 0.2), cell, nm, torch.zeros((n, m, 3), dtype=torch.int32)


def test_exported_with_the_documented_signature():
    import nvalchemiops.interactions.electrostatics as E
    from nvalchemiops.interactions.electrostatics.induced import InducedDipoleError, InducedDipoleResult, induced_dipoles

    for name in ("induced_dipoles", "InducedDipoleError", "InducedDipoleResult"):
        assert name in E.__all__, name
    assert E.induced_dipoles is induced_dipoles and E.InducedDipoleError is InducedDipoleError and E.InducedDipoleResult is InducedDipoleResult
    assert issubclass(InducedDipoleError, RuntimeError)
    assert InducedDipoleResult._fields == ("dipoles", "polarization_energy", "iterations", "residual")
    params = inspect.signature(induced_dipoles).parameters
    assert list(params) == ["positions", "charges", "polarizability", "cell", "external_field", "batch_idx", "neighbor_list", "neighbor_ptr",
                            "neighbor_shifts", "neighbor_matrix", "neighbor_matrix_shifts", "mask_value", "reciprocal", "alpha", "mesh_dimensions",
                            "mesh_spacing", "spline_order", "k_vectors", "k_cutoff", "accuracy", "tolerance", "max_iterations", "check_interval",
                            "initial_dipoles", "return_info"]
    for name in list(params)[4:]:
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    want = dict(reciprocal="pme", spline_order=5, accuracy=1e-6, tolerance=1e-8, max_iterations=200, check_interval=4, return_info=False)
    for name, value in want.items():
        assert params[name].default == value, name
    for name in ("external_field", "batch_idx", "mask_value", "alpha", "mesh_dimensions", "mesh_spacing", "k_vectors", "k_cutoff", "initial_dipoles"):
        assert params[name].default is None, name
    doc = induced_dipoles.__doc__
    assert "FULL" in doc and "float32" in doc and "Thole" in doc and "bit-identical" in doc


def test_list_errors_carry_the_messages_of_the_dipole_functions():
    from nvalchemiops.interactions.electrostatics import ewald_dipole_correction as edc, induced_dipoles as ind

    pos, q, a, cell, nm, sh = _args()
    mu = torch.zeros(4, 3)
    lst, ptr, lsh = torch.zeros((2, 3), dtype=torch.int32), torch.zeros(5, dtype=torch.int32), torch.zeros((3, 3), dtype=torch.int32)
    for kw in (dict(), dict(neighbor_list=lst), dict(neighbor_matrix=nm[:3], neighbor_matrix_shifts=sh),
               dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh[:, :5]), dict(neighbor_list=lst[:1], neighbor_ptr=ptr),
               dict(neighbor_list=lst, neighbor_ptr=ptr[:4], neighbor_shifts=lsh), dict(neighbor_list=lst, neighbor_ptr=ptr, neighbor_shifts=lsh[:2]),
               dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh, batch_idx=torch.zeros(3, dtype=torch.int32))):
        with pytest.raises(ValueError) as theirs:
            edc(pos, q, mu, cell, 0.3, **kw)
        with pytest.raises(ValueError) as ours:
            ind(pos, q, a, cell, alpha=0.3, **kw)
        assert str(ours.value) == str(theirs.value), kw
    with pytest.raises(ValueError) as theirs:
        edc(pos, q, mu, None, 0.3, neighbor_matrix=nm)
    with pytest.raises(ValueError, match="cell is required") as ours:
        ind(pos, q, a, None, neighbor_matrix=nm)
    assert str(ours.value) == str(theirs.value)
    with pytest.raises(ValueError, match="ONE format"):
        ind(pos, q, a, cell, neighbor_matrix=nm, neighbor_list=lst, neighbor_ptr=ptr)
    with pytest.raises(ValueError, match=r"cell must have shape \[3, 3\] or \[num_systems, 3, 3\]"):
        ind(pos, q, a, torch.eye(4), neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    with pytest.raises(ValueError, match="Unsupported dtype"):
        ind(pos.half(), q, a, cell, neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    with pytest.raises(ValueError, match=r"charges must have one entry per atom: expected shape \[4\]"):
        ind(pos, q[:3], a, cell, neighbor_matrix=nm, neighbor_matrix_shifts=sh)


def test_argument_errors_of_its_own():
    from nvalchemiops.interactions.electrostatics import induced_dipoles as ind

    pos, q, a, cell, nm, sh = _args()
    per = dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    with pytest.raises(ValueError, match=r"positions must have shape \[num_atoms, 3\]"):
        ind(pos[:, :2], q, a, cell, **per)
    for bad in (a[:3], torch.full((5,), 0.2), torch.full((4, 1), 0.2)):
        with pytest.raises(ValueError, match=r"polarizability must have one entry per atom: expected shape \[4\]"):
            ind(pos, q, bad, cell, **per)
    with pytest.raises(TypeError, match="polarizability must be a number or torch.Tensor"):
        ind(pos, q, "soft", cell, **per)
    for name in ("external_field", "initial_dipoles"):
        for bad in (torch.zeros(3, 3), torch.zeros(4), torch.zeros(4, 4)):
            with pytest.raises(ValueError, match=rf"{name} must have one vector per atom: expected shape \[4, 3\]"):
                ind(pos, q, a, cell, **{name: bad}, **per)
    with pytest.raises(ValueError, match="reciprocal must be 'pme' or 'ewald'"):
        ind(pos, q, a, cell, reciprocal="spme", **per)
    # the combinations charge_equilibration refuses, with its wording
    with pytest.raises(ValueError, match="k_cutoff belongs to reciprocal='ewald'"):
        ind(pos, q, a, cell, k_cutoff=2.0, **per)
    with pytest.raises(ValueError, match="belong to reciprocal='pme'"):
        ind(pos, q, a, cell, reciprocal="ewald", mesh_dimensions=(8, 8, 8), **per)
    with pytest.raises(ValueError, match="belong to reciprocal='pme'"):
        ind(pos, q, a, cell, reciprocal="ewald", mesh_spacing=0.5, **per)
    with pytest.raises(ValueError, match="k_vectors belong to reciprocal='ewald'"):
        ind(pos, q, a, cell, k_vectors=torch.zeros(5, 3), **per)
    with pytest.raises(ValueError, match=r"k_vectors must have shape \[K, 3\] or \[1, K, 3\]"):
        ind(pos, q, a, cell, reciprocal="ewald", k_vectors=torch.zeros(5, 2), **per)
    with pytest.raises(ValueError, match="spline_order must be 4, 5 or 6"):
        ind(pos, q, a, cell, spline_order=3, **per)
    with pytest.raises(ValueError, match="every mesh dimension must be at least the spline order"):
        ind(pos, q, a, cell, mesh_dimensions=(4, 8, 8), **per)
    with pytest.raises(ValueError, match="batch_idx is required for 2 systems"):
        ind(pos, q, a, cell.repeat(2, 1, 1), **per)
    with pytest.raises(ValueError, match=r"alpha has 2 values but there are 1 systems"):
        ind(pos, q, a, cell, alpha=torch.tensor([0.3, 0.4]), **per)
    for kw, msg in ((dict(tolerance=0.0), "tolerance must be positive"), (dict(tolerance=float("nan")), "tolerance must be positive"),
                    (dict(max_iterations=0), "max_iterations must be at least 1"), (dict(check_interval=0), "check_interval must be at least 1")):
        with pytest.raises(ValueError, match=msg):
            ind(pos, q, a, cell, **kw, **per)


def test_no_cpu_fallback():
    from nvalchemiops.interactions.electrostatics import induced_dipoles as ind

    pos, q, a, cell, nm, sh = _args()
    for polar in (a, 0.2, torch.tensor(0.2)):  # [N], Python float, 0-d tensor all get as far as the device check
        with pytest.raises(C.NativeLibraryError, match="ROCm devices only"):
            ind(pos, q, polar, cell, neighbor_matrix=nm, neighbor_matrix_shifts=sh, alpha=0.3, mesh_dimensions=(8, 8, 8))
    with pytest.raises(C.NativeLibraryError):
        ind(pos, q, a, cell, reciprocal="ewald", alpha=0.3, k_cutoff=2.0, neighbor_list=torch.zeros((2, 0), dtype=torch.int32),
            neighbor_ptr=torch.zeros(5, dtype=torch.int32))
    with pytest.raises(C.NativeLibraryError):  # under autograd as well
        ind(pos, q.clone().requires_grad_(True), a, cell, neighbor_matrix=nm, alpha=0.3, mesh_dimensions=(8, 8, 8))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_zero_atoms(dtype):
    from nvalchemiops.interactions.electrostatics import induced_dipoles as ind

    z = torch.zeros(0, dtype=dtype)
    cell = torch.eye(3, dtype=dtype) * 9
    mu = ind(torch.zeros((0, 3), dtype=dtype), z, z, cell, neighbor_matrix=torch.zeros((0, 5), dtype=torch.int32))
    assert mu.shape == (0, 3) and mu.dtype == dtype
    out = ind(torch.zeros((0, 3), dtype=dtype), z, 0.1, cell.repeat(2, 1, 1), neighbor_matrix=torch.zeros((0, 5), dtype=torch.int32),
              neighbor_matrix_shifts=torch.zeros((0, 5, 3), dtype=torch.int32), batch_idx=torch.zeros(0, dtype=torch.int32), return_info=True)
    assert out._fields == ("dipoles", "polarization_energy", "iterations", "residual")
    assert [tuple(o.shape) for o in out] == [(0, 3), (2,), (2,), (2,)] and out.iterations.dtype == torch.int64


def test_tracing_is_refused_with_a_clear_error():
    from nvalchemiops.interactions.electrostatics import induced_dipoles as ind

    pos, q, a, cell, nm, sh = _args()
    fn = torch.compile(lambda p: ind(p, q, a, cell, neighbor_matrix=nm), backend="eager", fullgraph=True)
    with pytest.raises(Exception) as err:
        fn(pos)
    assert "cannot be traced by torch.compile" in str(err.value)


def test_c_entry_points_reject_bad_arguments_before_any_device_call():
    lib = C.lib()
    err = lambda: lib.mi_last_error().decode()  # noqa: E731

    def check(call, cases):
        for bad, fragment in cases:
            assert call(**bad) == MI_EINVAL, bad
            assert "invalid argument" in err() and fragment in err(), (bad, err())

    def tensors(**over):
        a = dict(pos=P, pol=P, cell=P, alpha=P, bi=None, n=4, nsys=1, dtype=C.MI_F64, idx=P, ush=P, nptr=None, m=6, mask=-1, slots=24, t=P, nb=P, d=P,
                 pc=P)
        a.update(over)
        return lib.mi_induced_pair_tensors(a["pos"], a["pol"], a["cell"], a["alpha"], a["bi"], a["n"], a["nsys"], a["dtype"], a["idx"], a["ush"],
                                           a["nptr"], a["m"], a["mask"], a["slots"], a["t"], a["nb"], a["d"], a["pc"], None)

    check(tensors, ((dict(n=-1), "n_atoms"), (dict(nsys=0), "n_systems"), (dict(m=-1), "max_neighbors"), (dict(dtype=2), "dtype"),
                    (dict(nsys=2), "batch_idx"), (dict(slots=-1), "n_slots"), (dict(slots=23), "n_atoms * max_neighbors"),
                    (dict(pos=None), "null pointer"), (dict(pol=None), "null pointer"), (dict(cell=None), "null pointer"),
                    (dict(alpha=None), "null pointer"), (dict(idx=None), "null pointer"), (dict(t=None), "null pointer"),
                    (dict(nb=None), "null pointer"), (dict(d=None), "null pointer"), (dict(pc=None), "null pointer")))
    assert tensors(n=0, slots=0, pos=None, pol=None, idx=None, t=None, nb=None, d=None, pc=None) == MI_OK  # nothing to do

    def apply(**over):
        a = dict(t=P, nb=P, d=P, x=P, yin=None, bi=None, n=4, nsys=1, nptr=None, m=6, slots=24, y=P2, part=None)
        a.update(over)
        return lib.mi_induced_apply(a["t"], a["nb"], a["d"], a["x"], a["yin"], a["bi"], a["n"], a["nsys"], a["nptr"], a["m"], a["slots"],
                                    a["y"], a["part"], None)

    check(apply, ((dict(n=-1), "n_atoms"), (dict(nsys=0), "n_systems"), (dict(m=-1), "max_neighbors"), (dict(nsys=2, part=P), "batch_idx"),
                  (dict(nsys=65536, part=P, bi=P), "65535"), (dict(slots=-1), "n_slots"), (dict(slots=25), "n_atoms * max_neighbors"),
                  (dict(t=None), "null pointer"), (dict(nb=None), "null pointer"),
                  (dict(d=None), "null pointer"), (dict(x=None), "null pointer"), (dict(y=None), "null pointer"), (dict(y=P), "must not overlap"),
                  (dict(yin=P2), "must not overlap")))

    def dot(**over):
        a = dict(x=P, y=P2, bi=None, n=4, nsys=1, part=P)
        a.update(over)
        return lib.mi_induced_dot(a["x"], a["y"], a["bi"], a["n"], a["nsys"], a["part"], None)

    check(dot, ((dict(n=-1), "n_atoms"), (dict(nsys=0), "n_systems"), (dict(nsys=65536, bi=P), "65535"), (dict(nsys=2), "batch_idx"),
                (dict(x=None), "null pointer"), (dict(y=None), "null pointer"), (dict(part=None), "null pointer")))

    def update(**over):
        a = dict(y=P, py=P, pc=P, bi=None, n=4, nsys=1, mode=0, x=ctypes.c_void_p(12288), r=ctypes.c_void_p(16384), p=P, sin=P, sout=P2, prr=P)
        a.update(over)
        return lib.mi_induced_cg_update(a["y"], a["py"], a["pc"], a["bi"], a["n"], a["nsys"], a["mode"], a["x"], a["r"], a["p"], a["sin"],
                                        a["sout"], a["prr"], None)

    check(update, ((dict(n=-1), "n_atoms"), (dict(nsys=0), "n_systems"), (dict(nsys=65536, bi=P), "65535"), (dict(mode=2), "mode"),
                   (dict(nsys=3), "batch_idx"), (dict(py=None), "null pointer"), (dict(pc=None), "null pointer"),
                   (dict(prr=None), "null pointer"), (dict(sout=P), "must differ"), (dict(x=None), "null pointer"), (dict(y=None), "null pointer"),
                   (dict(r=None), "null pointer"), (dict(r=P), "must not overlap"), (dict(x=P), "must not overlap")))

    def direction(**over):
        a = dict(prr=P, pc=P, bi=None, n=4, nsys=1, mode=0, tol=1e-8, r=P, p=P2, sin=P, sout=P2)
        a.update(over)
        return lib.mi_induced_cg_direction(a["prr"], a["pc"], a["bi"], a["n"], a["nsys"], a["mode"], ctypes.c_double(a["tol"]), a["r"],
                                           a["p"], a["sin"], a["sout"], None)

    check(direction, ((dict(n=-1), "n_atoms"), (dict(nsys=0), "n_systems"), (dict(nsys=65536, bi=P), "65535"), (dict(mode=3), "mode"),
                      (dict(tol=-1.0), "tolerance"), (dict(tol=float("nan")), "tolerance"), (dict(nsys=2), "batch_idx"),
                      (dict(prr=None), "null pointer"), (dict(pc=None), "null pointer"), (dict(sout=P), "must differ"), (dict(r=None), "null pointer"),
                      (dict(p=None), "null pointer"), (dict(p=P), "must not overlap")))
    assert lib.mi_induced_blocks() == 64 and lib.mi_induced_state_words() >= 8 and lib.mi_induced_tensor_words() == 5
    assert lib.mi_induced_unroll_depth() >= 1


def test_header_declares_and_library_exports_the_entry_points():
    from tools.abi_symbols import declared_symbols

    declared = declared_symbols()
    assert set(INDUCED_SYMBOLS) <= set(declared)
    assert {s for s in declared if s.startswith("mi_induced_")} == set(INDUCED_SYMBOLS)
    for name in INDUCED_SYMBOLS:
        assert hasattr(C.lib(), name), name
