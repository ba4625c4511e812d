"""`charge_equilibration`: what can be checked without a GPU -- export, signature, every argument error (raised before anything is launched),
the absence of a CPU path, empty inputs, the refusal to be traced, and the argument checks of the C entry points (which return before any
device call)."""
import ctypes
import inspect

import pytest
import torch

from nvalchemiops import _capi as C

MI_OK, MI_EINVAL = 0, -1  # include/nvalchemiops_hip.h
P = ctypes.c_void_p(4096)  # a non-null pointer that is never dereferenced: every call below fails its checks first
QEQ_SYMBOLS = ("mi_qeq_pair_coefficients", "mi_qeq_apply", "mi_qeq_cg_update", "mi_qeq_cg_direction", "mi_qeq_blocks", "mi_qeq_state_words")


def _args(n=4, m=6):
    pos, chi, hard, cell = torch.rand(n, 3), torch.rand(n), torch.rand(n) + 0.5, torch.eye(3)[None] * 10
    nm = torch.full((n, m), n, dtype=torch.int32)
    return pos, chi, hard, torch.full((n,), 0.5), cell, nm, torch.zeros((n, m, 3), dtype=torch.int32)


def test_exported_with_the_documented_signature():
    import nvalchemiops.interactions.electrostatics as E
    from nvalchemiops.interactions.electrostatics.qeq import ChargeEquilibrationError, charge_equilibration

    assert "charge_equilibration" in E.__all__ and E.charge_equilibration is charge_equilibration
    assert issubclass(ChargeEquilibrationError, RuntimeError) and E.ChargeEquilibrationError is ChargeEquilibrationError
    params = inspect.signature(charge_equilibration).parameters
    assert list(params) == ["positions", "electronegativity", "hardness", "sigma", "cell", "total_charge", "batch_idx", "num_systems",
                            "neighbor_list", "neighbor_ptr", "neighbor_shifts", "neighbor_matrix", "neighbor_matrix_shifts", "mask_value",
                            "reciprocal", "alpha", "mesh_dimensions", "mesh_spacing", "spline_order", "k_vectors", "k_cutoff", "accuracy",
                            "tolerance", "max_iterations", "check_interval", "initial_charges", "return_info"]
    assert params["cell"].default is None and params["cell"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    for name in list(params)[5:]:
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    want = dict(total_charge=0.0, mask_value=-1, reciprocal="pme", spline_order=4, accuracy=1e-6, tolerance=1e-8, max_iterations=200,
                check_interval=4, return_info=False)
    for name, value in want.items():
        assert params[name].default == value, name
    for name in ("batch_idx", "num_systems", "alpha", "mesh_dimensions", "mesh_spacing", "k_vectors", "k_cutoff", "initial_charges"):
        assert params[name].default is None, name
    assert "FULL" in charge_equilibration.__doc__  # the full-list requirement is stated


def test_list_errors_carry_the_messages_of_gaussian_charge_correction():
    from nvalchemiops.interactions.electrostatics import charge_equilibration as qeq, gaussian_charge_correction as gcc

    pos, chi, hard, sig, cell, nm, sh = _args()
    lst, ptr, lsh = torch.zeros((2, 3), dtype=torch.int32), torch.zeros(5, dtype=torch.int32), torch.zeros((3, 3), dtype=torch.int32)
    for kw in (dict(), dict(neighbor_list=lst), dict(neighbor_matrix=nm[:3], neighbor_matrix_shifts=sh),
               dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh[:, :5]), dict(neighbor_list=lst[:1], neighbor_ptr=ptr),
               dict(neighbor_list=lst, neighbor_ptr=ptr[:4], neighbor_shifts=lsh), dict(neighbor_list=lst, neighbor_ptr=ptr, neighbor_shifts=lsh[:2]),
               dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh, batch_idx=torch.zeros(3, dtype=torch.int32))):
        with pytest.raises(ValueError) as theirs:
            gcc(pos, chi, sig, cell, **kw)
        with pytest.raises(ValueError) as ours:
            qeq(pos, chi, hard, sig, cell, **kw)
        assert str(ours.value) == str(theirs.value), kw
    for bad in (sig[:3], torch.full((5,), 0.5), torch.full((4, 1), 0.5)):
        with pytest.raises(ValueError, match=r"sigma must have one entry per atom: expected shape \[4\]"):
            qeq(pos, chi, hard, bad, cell, neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    with pytest.raises(ValueError, match="neighbor shifts need a cell"):
        qeq(pos, chi, hard, sig, None, neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    with pytest.raises(ValueError, match="neighbor shifts need a cell"):
        qeq(pos, chi, hard, sig, neighbor_list=lst, neighbor_ptr=ptr, neighbor_shifts=lsh)
    with pytest.raises(ValueError, match=r"cell must have shape \[3, 3\] or \[num_systems, 3, 3\]"):
        qeq(pos, chi, hard, sig, torch.eye(4), neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    with pytest.raises(ValueError, match="Unsupported dtype"):
        qeq(pos.half(), chi, hard, sig, cell, neighbor_matrix=nm, neighbor_matrix_shifts=sh)


def test_argument_errors_of_its_own():
    from nvalchemiops.interactions.electrostatics import charge_equilibration as qeq

    pos, chi, hard, sig, cell, nm, sh = _args()
    per = dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    with pytest.raises(ValueError, match=r"positions must have shape \[num_atoms, 3\]"):
        qeq(pos[:, :2], chi, hard, sig, cell, **per)
    for name, kw in (("electronegativity", dict(chi=chi[:3])), ("hardness", dict(hard=hard[:3])), ("electronegativity", dict(chi=chi[:, None])),
                     ("hardness", dict(hard=torch.tensor(1.0)))):
        with pytest.raises(ValueError, match=rf"{name} must have one entry per atom: expected shape \[4\]"):
            qeq(pos, kw.get("chi", chi), kw.get("hard", hard), sig, cell, **per)
    with pytest.raises(ValueError, match=r"initial_charges must have one entry per atom: expected shape \[4\]"):
        qeq(pos, chi, hard, sig, cell, initial_charges=torch.zeros(5), **per)
    with pytest.raises(ValueError, match="reciprocal must be 'pme' or 'ewald'"):
        qeq(pos, chi, hard, sig, cell, reciprocal="spme", **per)
    # without a cell there is no reciprocal-space part: none of its arguments may be passed
    for kw in (dict(alpha=0.3), dict(mesh_dimensions=(8, 8, 8)), dict(mesh_spacing=0.5), dict(k_vectors=torch.zeros((3, 3))), dict(k_cutoff=2.0)):
        with pytest.raises(ValueError, match=f"{next(iter(kw))} need a cell"):
            qeq(pos, chi, hard, sig, None, neighbor_matrix=nm, **kw)
    with pytest.raises(ValueError, match="k_cutoff belongs to reciprocal='ewald'"):
        qeq(pos, chi, hard, sig, cell, k_cutoff=2.0, **per)
    with pytest.raises(ValueError, match="belong to reciprocal='pme'"):
        qeq(pos, chi, hard, sig, cell, reciprocal="ewald", mesh_dimensions=(8, 8, 8), **per)
    # the number of systems: cells first; without a cell num_systems, then the length of total_charge -- and more than one needs batch_idx
    with pytest.raises(ValueError, match=r"cell must have shape \[3, 3, 3\] \(one per system\)"):
        qeq(pos, chi, hard, sig, cell, num_systems=3, **per)
    with pytest.raises(ValueError, match="batch_idx is required for 2 systems"):
        qeq(pos, chi, hard, sig, cell.repeat(2, 1, 1), **per)
    with pytest.raises(ValueError, match="batch_idx is required for 3 systems"):
        qeq(pos, chi, hard, sig, None, neighbor_matrix=nm, total_charge=torch.zeros(3))
    with pytest.raises(ValueError, match="batch_idx is required for 2 systems"):
        qeq(pos, chi, hard, sig, None, neighbor_matrix=nm, num_systems=2)
    with pytest.raises(ValueError, match="num_systems must be at least 1"):
        qeq(pos, chi, hard, sig, None, neighbor_matrix=nm, num_systems=0)
    with pytest.raises(ValueError, match=r"total_charge must be a number or have shape \[1\]"):
        qeq(pos, chi, hard, sig, cell, total_charge=torch.zeros(2), **per)
    with pytest.raises(ValueError, match=r"total_charge must be a number or have shape \[2\]"):
        qeq(pos, chi, hard, sig, None, neighbor_matrix=nm, num_systems=2, batch_idx=torch.zeros(4, dtype=torch.int32), total_charge=torch.zeros((2, 1)))
    with pytest.raises(TypeError, match="total_charge must be a number or torch.Tensor"):
        qeq(pos, chi, hard, sig, cell, total_charge="neutral", **per)
    with pytest.raises(ValueError, match=r"alpha has 2 values but there are 1 systems"):
        qeq(pos, chi, hard, sig, cell, alpha=torch.tensor([0.3, 0.4]), **per)
    for kw, msg in ((dict(tolerance=0.0), "tolerance must be positive"), (dict(tolerance=float("nan")), "tolerance must be positive"),
                    (dict(max_iterations=0), "max_iterations must be at least 1"), (dict(check_interval=0), "check_interval must be at least 1")):
        with pytest.raises(ValueError, match=msg):
            qeq(pos, chi, hard, sig, cell, **kw, **per)


def test_no_cpu_fallback():
    from nvalchemiops.interactions.electrostatics import charge_equilibration as qeq

    pos, chi, hard, sig, cell, nm, sh = _args()
    for sigma in (sig, 0.5, torch.tensor(0.5)):  # [N], Python float, 0-d tensor all get as far as the device check
        with pytest.raises(C.NativeLibraryError, match="ROCm devices only"):
            qeq(pos, chi, hard, sigma, cell, neighbor_matrix=nm, neighbor_matrix_shifts=sh, alpha=0.3, mesh_dimensions=(8, 8, 8))
    with pytest.raises(C.NativeLibraryError):
        qeq(pos, chi, hard, sig, None, neighbor_list=torch.zeros((2, 0), dtype=torch.int32), neighbor_ptr=torch.zeros(5, dtype=torch.int32))
    with pytest.raises(C.NativeLibraryError):  # under autograd as well
        qeq(pos, chi.clone().requires_grad_(True), hard, sig, None, neighbor_matrix=nm)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_zero_atoms(dtype):
    from nvalchemiops.interactions.electrostatics import charge_equilibration as qeq

    z = torch.zeros(0, dtype=dtype)
    q = qeq(torch.zeros((0, 3), dtype=dtype), z, z, z, neighbor_matrix=torch.zeros((0, 5), dtype=torch.int32))
    assert q.shape == (0,) and q.dtype == dtype
    out = qeq(torch.zeros((0, 3), dtype=dtype), z, z, 0.5, torch.eye(3, dtype=dtype).repeat(2, 1, 1) * 9,
              neighbor_matrix=torch.zeros((0, 5), dtype=torch.int32), neighbor_matrix_shifts=torch.zeros((0, 5, 3), dtype=torch.int32),
              batch_idx=torch.zeros(0, dtype=torch.int32), return_info=True)
    assert out._fields == ("charges", "chemical_potential", "iterations", "residual")
    assert [tuple(o.shape) for o in out] == [(0,), (2,), (2,), (2,)] and out.iterations.dtype == torch.int64


def test_tracing_is_refused_with_a_clear_error():
    from nvalchemiops.interactions.electrostatics import charge_equilibration as qeq

    pos, chi, hard, sig, cell, nm, sh = _args()
    fn = torch.compile(lambda p: qeq(p, chi, hard, sig, None, neighbor_matrix=nm), backend="eager", fullgraph=True)
    with pytest.raises(Exception) as err:
        fn(pos)
    assert "cannot be traced by torch.compile" in str(err.value)


def test_c_entry_points_reject_bad_arguments_before_any_device_call():
    lib = C.lib()
    err = lambda: lib.mi_last_error().decode()  # noqa: E731

    def coef(**over):
        a = dict(pos=P, sigma=P, hard=P, cell=P, alpha=P, bi=None, n=4, nsys=1, dtype=C.MI_F64, idx=P, ush=P, nptr=None, m=6, mask=-1, c=P, nb=P, d=P)
        a.update(over)
        return lib.mi_qeq_pair_coefficients(a["pos"], a["sigma"], a["hard"], a["cell"], a["alpha"], a["bi"], a["n"], a["nsys"], a["dtype"], a["idx"],
                                            a["ush"], a["nptr"], a["m"], a["mask"], a["c"], a["nb"], a["d"], None)

    for bad, fragment in ((dict(n=-1), "n_atoms"), (dict(nsys=0), "n_systems"), (dict(m=-1), "max_neighbors"), (dict(dtype=2), "dtype"),
                          (dict(nsys=2), "batch_idx"), (dict(cell=None), "unit_shifts without a cell"), (dict(alpha=None), "alpha"),
                          (dict(pos=None), "null pointer"), (dict(sigma=None), "null pointer"), (dict(hard=None), "null pointer"),
                          (dict(idx=None), "null pointer"), (dict(c=None), "null pointer"), (dict(nb=None), "null pointer"), (dict(d=None), "null pointer")):
        assert coef(**bad) == MI_EINVAL, bad
        assert "invalid argument" in err() and fragment in err(), (bad, err())
    assert coef(n=0, pos=None, sigma=None, hard=None, idx=None, c=None, nb=None, d=None) == MI_OK  # nothing to do

    def apply(**over):
        a = dict(c=P, nb=P, d=P, x=P, yin=None, bi=None, n=4, nsys=1, nptr=None, m=6, y=ctypes.c_void_p(8192), part=None)
        a.update(over)
        return lib.mi_qeq_apply(a["c"], a["nb"], a["d"], a["x"], a["yin"], a["bi"], a["n"], a["nsys"], a["nptr"], a["m"], a["y"], a["part"], None)

    for bad, fragment in ((dict(n=-1), "n_atoms"), (dict(nsys=0), "n_systems"), (dict(m=-1), "max_neighbors"), (dict(nsys=2, part=P), "batch_idx"),
                          (dict(nsys=65536, part=P, bi=P), "65535"), (dict(c=None), "null pointer"), (dict(nb=None), "null pointer"), (dict(d=None), "null pointer"), (dict(x=None), "null pointer"),
                          (dict(y=None), "null pointer"), (dict(y=P), "must not overlap")):
        assert apply(**bad) == MI_EINVAL, bad
        assert "invalid argument" in err() and fragment in err(), (bad, err())

    def update(**over):
        a = dict(y=P, py=P, cnt=P, bi=None, n=4, nsys=1, mode=0, q=P, r=P, p=P, sin=P, sout=ctypes.c_void_p(8192), prr=P)
        a.update(over)
        return lib.mi_qeq_cg_update(a["y"], a["py"], a["cnt"], a["bi"], a["n"], a["nsys"], a["mode"], a["q"], a["r"], a["p"], a["sin"], a["sout"],
                                    a["prr"], None)

    for bad, fragment in ((dict(n=-1), "n_atoms"), (dict(nsys=0), "n_systems"), (dict(nsys=65536, bi=P), "65535"), (dict(mode=2), "mode"), (dict(nsys=3), "batch_idx"),
                          (dict(py=None), "null pointer"), (dict(cnt=None), "null pointer"), (dict(prr=None), "null pointer"),
                          (dict(sout=P), "must differ"), (dict(q=None), "null pointer"), (dict(y=None), "null pointer")):
        assert update(**bad) == MI_EINVAL, bad
        assert "invalid argument" in err() and fragment in err(), (bad, err())

    def direction(**over):
        a = dict(prr=P, bi=None, n=4, nsys=1, mode=0, tol=1e-8, r=P, p=P, sin=P, sout=ctypes.c_void_p(8192))
        a.update(over)
        return lib.mi_qeq_cg_direction(a["prr"], a["bi"], a["n"], a["nsys"], a["mode"], ctypes.c_double(a["tol"]), a["r"], a["p"], a["sin"], a["sout"], None)

    for bad, fragment in ((dict(n=-1), "n_atoms"), (dict(nsys=0), "n_systems"), (dict(nsys=65536, bi=P), "65535"), (dict(mode=3), "mode"), (dict(tol=-1.0), "tolerance"),
                          (dict(tol=float("nan")), "tolerance"), (dict(nsys=2), "batch_idx"), (dict(prr=None), "null pointer"),
                          (dict(sout=P), "must differ"), (dict(r=None), "null pointer"), (dict(p=None), "null pointer")):
        assert direction(**bad) == MI_EINVAL, bad
        assert "invalid argument" in err() and fragment in err(), (bad, err())
    assert lib.mi_qeq_blocks() == 64 and lib.mi_qeq_state_words() >= 6


def test_header_declares_and_library_exports_the_entry_points():
    from tools.abi_symbols import declared_symbols

    declared = declared_symbols()
    assert set(QEQ_SYMBOLS) <= set(declared)
    assert {s for s in declared if s.startswith("mi_qeq_")} == set(QEQ_SYMBOLS)
    for name in QEQ_SYMBOLS:
        assert hasattr(C.lib(), name), name
