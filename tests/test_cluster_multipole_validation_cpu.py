"""`coulomb_dipole_correction`, `coulomb_quadrupole_correction` and `cluster_induced_dipoles`: what can be checked without a GPU -- exports,
signatures, every argument error (raised before anything is launched), the absence of a CPU path, empty inputs, the argument checks of the C
entry points (which return before any device call), and that the periodic routines still refuse `cell=None`."""
import ctypes
import inspect

import pytest
import torch

from nvalchemiops import _capi as C

MI_OK, MI_EINVAL = 0, -1  # include/nvalchemiops_hip.h
P = ctypes.c_void_p(4096)  # a non-null pointer that is never dereferenced: every call below fails its checks first
SYMBOLS = ("mi_coulomb_dipole", "mi_coulomb_dipole_scratch_bytes", "mi_coulomb_dipole_blocks", "mi_coulomb_quadrupole",
           "mi_coulomb_quadrupole_scratch_bytes", "mi_coulomb_quadrupole_blocks", "mi_cluster_induced_pair_tensors")
NAMES = ("coulomb_dipole_correction", "coulomb_quadrupole_correction", "cluster_induced_dipoles")
LISTS = ["neighbor_list", "neighbor_ptr", "neighbor_shifts", "neighbor_matrix", "neighbor_matrix_shifts"]


def _args(n=4, m=6):
    pos, q, mu, quad, cell = torch.rand(n, 3), torch.rand(n), torch.rand(n, 3), torch.rand(n, 3, 3), torch.eye(3)[None] * 10
    nm = torch.full((n, m), n, dtype=torch.int32)
    return pos, q, mu, quad, cell, nm, torch.zeros((n, m, 3), dtype=torch.int32)


def _api():
    from nvalchemiops.interactions.electrostatics import cluster_induced_dipoles, coulomb_dipole_correction, coulomb_quadrupole_correction

    return coulomb_dipole_correction, coulomb_quadrupole_correction, cluster_induced_dipoles


def test_exported_with_the_documented_signatures():
    import nvalchemiops.interactions.electrostatics as E
    from nvalchemiops.interactions.electrostatics import cluster as CL

    for name in NAMES:
        assert name in E.__all__ and name in CL.__all__ and getattr(E, name) is getattr(CL, name)
    flags = ["compute_forces", "compute_charge_gradients", "compute_dipole_gradients", "compute_virial"]
    dp = inspect.signature(CL.coulomb_dipole_correction).parameters
    assert list(dp) == ["positions", "charges", "dipoles", "cell"] + LISTS + ["mask_value", "batch_idx"] + flags
    qd = inspect.signature(CL.coulomb_quadrupole_correction).parameters
    assert list(qd) == (["positions", "charges", "dipoles", "quadrupoles", "cell"] + LISTS + ["mask_value", "batch_idx"] + flags[:3]
                        + ["compute_quadrupole_gradients", "compute_virial"])
    for params, first_keyword in ((dp, 4), (qd, 5)):
        assert params["cell"].default is None and params["mask_value"].default == -1
        assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(params)[first_keyword:])
        assert all(params[k].default is False for k in params if k.startswith("compute_"))
        assert "cutoff" not in params and "alpha" not in params
    sv = inspect.signature(CL.cluster_induced_dipoles).parameters
    assert list(sv) == ["positions", "charges", "polarizability", "thole", "external_field", "batch_idx", "num_systems", "neighbor_list",
                        "neighbor_ptr", "neighbor_matrix", "mask_value", "tolerance", "max_iterations", "check_interval", "initial_dipoles",
                        "return_info"]
    assert all(sv[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sv)[3:])
    plain = inspect.signature(E.induced_dipoles).parameters
    assert all(sv[k].default == plain[k].default for k in ("tolerance", "max_iterations", "check_interval", "initial_dipoles", "return_info",
                                                           "mask_value", "external_field"))
    assert sv["thole"].default is None and sv["num_systems"].default is None
    # cross-references live in the new docstrings
    assert "coulomb_energy(alpha=0)" in CL.coulomb_dipole_correction.__doc__ and "FULL" in CL.coulomb_dipole_correction.__doc__
    assert "Theta / 3" in CL.coulomb_quadrupole_correction.__doc__ and "cluster_induced_dipoles" in CL.coulomb_quadrupole_correction.__doc__
    doc = CL.cluster_induced_dipoles.__doc__
    assert "bit-identical" in doc and "external_field = -coulomb_quadrupole_correction" in doc and "thole_dipole_correction" in doc


def test_periodic_routines_still_refuse_a_cluster():
    import nvalchemiops.interactions.electrostatics as E

    pos, q, mu, quad, cell, nm, sh = _args()
    msg = "cell is required"
    with pytest.raises(ValueError, match=msg):
        E.ewald_dipole_real_space(pos, q, mu, None, 0.3, neighbor_matrix=nm)
    with pytest.raises(ValueError, match=msg):
        E.ewald_dipole_correction(pos, q, mu, None, alpha=0.3, neighbor_matrix=nm)
    with pytest.raises(ValueError, match=msg):
        E.pme_dipole_correction(pos, q, mu, None, alpha=0.3, mesh_dimensions=(8, 8, 8), neighbor_matrix=nm)
    with pytest.raises(ValueError, match=msg):
        E.ewald_quadrupole_real_space(pos, q, mu, quad, None, 0.3, neighbor_matrix=nm)
    with pytest.raises(ValueError, match=msg):
        E.ewald_quadrupole_correction(pos, q, mu, quad, None, alpha=0.3, neighbor_matrix=nm)
    with pytest.raises(ValueError, match=msg):
        E.pme_quadrupole_correction(pos, q, mu, quad, None, alpha=0.3, mesh_dimensions=(8, 8, 8), neighbor_matrix=nm)
    with pytest.raises(ValueError, match=msg):
        E.induced_dipoles(pos, q, 0.2, None, neighbor_matrix=nm)
    with pytest.raises(ValueError, match=msg):
        E.thole_induced_dipoles(pos, q, 0.2, None, neighbor_matrix=nm)
    for fn in (E.ewald_dipole_correction, E.induced_dipoles, E.ewald_quadrupole_correction):
        assert "clusters" in fn.__doc__  # their docstrings are as they were


def test_list_errors_carry_the_messages_of_the_dipole_functions():
    from nvalchemiops.interactions.electrostatics import ewald_dipole_real_space as real

    dp, qd, _ = _api()
    pos, q, mu, quad, cell, nm, sh = _args()
    lst, ptr, lsh = torch.zeros((2, 3), dtype=torch.int32), torch.zeros(5, dtype=torch.int32), torch.zeros((3, 3), dtype=torch.int32)
    for kw in (dict(), dict(neighbor_list=lst), dict(neighbor_matrix=nm[:3], neighbor_matrix_shifts=sh),
               dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh[:, :5]), dict(neighbor_list=lst[:1], neighbor_ptr=ptr),
               dict(neighbor_list=lst, neighbor_ptr=ptr[:4], neighbor_shifts=lsh), dict(neighbor_list=lst, neighbor_ptr=ptr, neighbor_shifts=lsh[:2]),
               dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh, batch_idx=torch.zeros(3, dtype=torch.int32)),
               dict(neighbor_matrix=nm, compute_virial=True), dict(neighbor_list=lst, neighbor_ptr=ptr, compute_virial=True)):  # a virial without shifts
        with pytest.raises(ValueError) as theirs:
            real(pos, q, mu, cell, 0.3, **kw)
        for call in (lambda: dp(pos, q, mu, cell, **kw), lambda: qd(pos, q, mu, quad, cell, **kw), lambda: qd(pos, q, None, quad, cell, **kw)):
            with pytest.raises(ValueError) as ours:
                call()
            assert str(ours.value) == str(theirs.value), kw
    for call in (lambda **kw: dp(pos, q, mu, **kw), lambda **kw: qd(pos, q, mu, quad, **kw)):
        with pytest.raises(ValueError, match="ONE format"):
            call(neighbor_matrix=nm, neighbor_list=lst, neighbor_ptr=ptr)
        with pytest.raises(ValueError, match=r"cell must have shape \[3, 3\] or \[num_systems, 3, 3\]"):
            call(cell=torch.eye(4), neighbor_matrix=nm, neighbor_matrix_shifts=sh)
        # a cluster: a list is needed, no shifts, no virial
        with pytest.raises(ValueError, match="Either neighbor_list or neighbor_matrix must be provided"):
            call()
        with pytest.raises(ValueError, match="neighbor_ptr is required"):
            call(neighbor_list=lst)
        with pytest.raises(ValueError, match="neighbor shifts need a cell"):
            call(neighbor_matrix=nm, neighbor_matrix_shifts=sh)
        with pytest.raises(ValueError, match="neighbor shifts need a cell"):
            call(neighbor_list=lst, neighbor_ptr=ptr, neighbor_shifts=lsh)
        with pytest.raises(ValueError, match="compute_virial needs a cell"):
            call(neighbor_matrix=nm, compute_virial=True)
    with pytest.raises(ValueError, match="Unsupported dtype"):
        dp(pos.half(), q, mu, neighbor_matrix=nm)
    with pytest.raises(TypeError):  # the lists are keyword-only: there is no alpha or cutoff to pass by position
        dp(pos, q, mu, None, 0.3)


def test_shape_errors_of_the_per_atom_arguments():
    dp, qd, sv = _api()
    pos, q, mu, quad, cell, nm, sh = _args()
    per = dict(neighbor_matrix=nm)
    for call in (lambda p, c, m: dp(p, c, m, **per), lambda p, c, m: qd(p, c, m, quad, **per)):
        with pytest.raises(ValueError, match=r"positions must have shape \[num_atoms, 3\]"):
            call(pos[:, :2], q, mu)
        with pytest.raises(ValueError, match=r"charges must have one entry per atom: expected shape \[4\]"):
            call(pos, q[:3], mu)
        for bad in (mu[:3], torch.zeros(4), torch.zeros(4, 4)):
            with pytest.raises(ValueError, match=r"dipoles must have one vector per atom: expected shape \[4, 3\]"):
                call(pos, q, bad)
    for bad in (quad[:3], torch.zeros(4, 3), torch.zeros(4, 9), None):
        with pytest.raises(ValueError, match=r"quadrupoles must have one 3 x 3 tensor per atom: expected shape \[4, 3, 3\]"):
            qd(pos, q, mu, bad, **per)
    # the solver
    with pytest.raises(ValueError, match=r"positions must have shape \[num_atoms, 3\]"):
        sv(pos[:, :2], q, 0.2, **per)
    with pytest.raises(ValueError, match=r"charges must have one entry per atom: expected shape \[4\]"):
        sv(pos, q[:3], 0.2, **per)
    for bad in (torch.full((3,), 0.2), torch.full((4, 1), 0.2)):
        with pytest.raises(ValueError, match=r"polarizability must have one entry per atom: expected shape \[4\]"):
            sv(pos, q, bad, **per)
    with pytest.raises(TypeError, match="polarizability must be a number or torch.Tensor"):
        sv(pos, q, "soft", **per)
    for name in ("external_field", "initial_dipoles"):
        with pytest.raises(ValueError, match=name + r" must have one vector per atom: expected shape \[4, 3\]"):
            sv(pos, q, 0.2, **{name: torch.zeros(3, 3)}, **per)


def test_solver_argument_errors():
    _, _, sv = _api()
    pos, q, mu, quad, cell, nm, sh = _args()
    lst, ptr = torch.zeros((2, 3), dtype=torch.int32), torch.zeros(5, dtype=torch.int32)
    per = dict(neighbor_matrix=nm)
    with pytest.raises(ValueError, match="Either neighbor_list or neighbor_matrix must be provided"):
        sv(pos, q, 0.2)
    with pytest.raises(ValueError, match="neighbor_ptr is required"):
        sv(pos, q, 0.2, neighbor_list=lst)
    with pytest.raises(ValueError, match="ONE format"):
        sv(pos, q, 0.2, neighbor_list=lst, neighbor_ptr=ptr, **per)
    with pytest.raises(TypeError):  # there is no cell and there are no shifts
        sv(pos, q, 0.2, cell=cell, **per)
    with pytest.raises(TypeError):
        sv(pos, q, 0.2, neighbor_matrix_shifts=sh, **per)
    for bad in (0.0, -0.39, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="thole must be finite and positive"):
            sv(pos, q, 0.2, thole=bad, **per)
    for bad in ("0.39", True):
        with pytest.raises(TypeError, match="thole must be a number"):
            sv(pos, q, 0.2, thole=bad, **per)
    with pytest.raises(ValueError, match="batch_idx is required for 2 systems"):
        sv(pos, q, 0.2, num_systems=2, **per)
    for bad in (0, -1, 65536):
        with pytest.raises(ValueError, match=r"num_systems must be in \[1, 65535\]"):
            sv(pos, q, 0.2, num_systems=bad, batch_idx=torch.zeros(4, dtype=torch.int32), **per)
    for bad in (2.0, True, torch.tensor(2)):
        with pytest.raises(TypeError, match="num_systems must be an int"):
            sv(pos, q, 0.2, num_systems=bad, batch_idx=torch.zeros(4, dtype=torch.int32), **per)
    with pytest.raises(ValueError, match="batch_idx"):
        sv(pos, q, 0.2, num_systems=2, batch_idx=torch.zeros(3, dtype=torch.int32), **per)
    with pytest.raises(ValueError, match="tolerance must be positive"):
        sv(pos, q, 0.2, tolerance=0.0, **per)
    with pytest.raises(ValueError, match="max_iterations must be at least 1"):
        sv(pos, q, 0.2, max_iterations=0, **per)
    with pytest.raises(ValueError, match="check_interval must be at least 1"):
        sv(pos, q, 0.2, check_interval=0, **per)


def test_the_solver_is_not_traceable():
    _, _, sv = _api()
    pos, q, mu, quad, cell, nm, sh = _args()
    fn = torch.compile(lambda p: sv(p, q, 0.2, neighbor_matrix=nm), backend="eager", fullgraph=True)
    with pytest.raises(Exception) as err:
        fn(pos)
    assert "cluster_induced_dipoles cannot be traced by torch.compile" in str(err.value)


def test_no_cpu_fallback():
    dp, qd, sv = _api()
    pos, q, mu, quad, cell, nm, sh = _args()
    lst, ptr, lsh = torch.zeros((2, 3), dtype=torch.int32), torch.tensor([0, 1, 2, 3, 3], dtype=torch.int32), torch.zeros((3, 3), dtype=torch.int32)
    for kw in (dict(neighbor_matrix=nm), dict(neighbor_list=lst, neighbor_ptr=ptr), dict(cell=cell, neighbor_matrix=nm, neighbor_matrix_shifts=sh),
               dict(cell=cell, neighbor_list=lst, neighbor_ptr=ptr, neighbor_shifts=lsh)):
        with pytest.raises(C.NativeLibraryError, match="ROCm devices only"):
            dp(pos, q, mu, **kw)
        with pytest.raises(C.NativeLibraryError, match="ROCm devices only"):
            qd(pos, q, None, quad, **kw)
    with pytest.raises(C.NativeLibraryError):  # under autograd as well
        dp(pos, q, mu.clone().requires_grad_(True), neighbor_matrix=nm)
    with pytest.raises(C.NativeLibraryError):
        qd(pos, q, mu, quad.clone().requires_grad_(True), neighbor_matrix=nm)
    for polar in (torch.full((4,), 0.2), 0.2, torch.tensor(0.2)):
        for thole in (None, 0.39):
            with pytest.raises(C.NativeLibraryError, match="ROCm devices only"):
                sv(pos, q, polar, thole=thole, neighbor_matrix=nm)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_zero_atoms(dtype):
    dp, qd, sv = _api()
    z, z3, z33 = torch.zeros(0, dtype=dtype), torch.zeros((0, 3), dtype=dtype), torch.zeros((0, 3, 3), dtype=dtype)
    cell = torch.eye(3, dtype=dtype) * 9
    nm, sh = torch.zeros((0, 5), dtype=torch.int32), torch.zeros((0, 5, 3), dtype=torch.int32)
    e = dp(z3, z, z3, neighbor_matrix=nm)
    assert e.shape == (0,) and e.dtype == dtype
    out = dp(z3, z, z3, cell.repeat(2, 1, 1), neighbor_matrix=nm, neighbor_matrix_shifts=sh, batch_idx=torch.zeros(0, dtype=torch.int32),
             compute_forces=True, compute_charge_gradients=True, compute_dipole_gradients=True, compute_virial=True)
    assert [tuple(o.shape) for o in out] == [(0,), (0, 3), (0,), (0, 3), (2, 3, 3)] and all(o.dtype == dtype for o in out)
    out = qd(z3, z, None, z33, neighbor_matrix=nm, compute_forces=True, compute_charge_gradients=True, compute_dipole_gradients=True,
             compute_quadrupole_gradients=True)
    assert [tuple(o.shape) for o in out] == [(0,), (0, 3), (0,), (0, 3), (0, 3, 3)] and all(o.dtype == dtype for o in out)
    assert sv(z3, z, z, neighbor_matrix=nm).shape == (0, 3)
    res = sv(z3, z, 0.2, thole=0.39, num_systems=3, batch_idx=torch.zeros(0, dtype=torch.int32), neighbor_matrix=nm, return_info=True)
    assert res.dipoles.shape == (0, 3) and res.polarization_energy.shape == (3,) and res.iterations.dtype == torch.int64


def test_c_entry_points_reject_bad_arguments_before_any_device_call():
    lib = C.lib()
    err = lambda: lib.mi_last_error().decode()  # noqa: E731

    def check(call, cases):
        for bad, fragment in cases:
            assert call(**bad) == MI_EINVAL, bad
            assert "invalid argument" in err() and fragment in err(), (bad, err())

    def dipole(**over):
        a = dict(pos=P, q=P, mu=P, cell=P, bi=None, w=None, n=4, nsys=1, dtype=C.MI_F64, idx=P, ush=P, nptr=None, m=6, mask=-1, flags=0, e=P, f=None,
                 cg=None, dg=None, vir=None, scratch=P, nbytes=1 << 20)
        a.update(over)
        return lib.mi_coulomb_dipole(a["pos"], a["q"], a["mu"], a["cell"], a["bi"], a["w"], a["n"], a["nsys"], a["dtype"], a["idx"], a["ush"],
                                     a["nptr"], a["m"], a["mask"], a["flags"], a["e"], a["f"], a["cg"], a["dg"], a["vir"], a["scratch"],
                                     ctypes.c_size_t(a["nbytes"]), None)

    def quadrupole(**over):
        a = dict(pos=P, q=P, mu=P, qd=P, cell=P, bi=None, w=None, n=4, nsys=1, dtype=C.MI_F64, idx=P, ush=P, nptr=None, m=6, mask=-1, flags=0, e=P,
                 f=None, cg=None, dg=None, qg=None, vir=None, scratch=P, nbytes=1 << 20)
        a.update(over)
        return lib.mi_coulomb_quadrupole(a["pos"], a["q"], a["mu"], a["qd"], a["cell"], a["bi"], a["w"], a["n"], a["nsys"], a["dtype"], a["idx"],
                                         a["ush"], a["nptr"], a["m"], a["mask"], a["flags"], a["e"], a["f"], a["cg"], a["dg"], a["qg"], a["vir"],
                                         a["scratch"], ctypes.c_size_t(a["nbytes"]), None)

    common = ((dict(n=-1), "n_atoms"), (dict(nsys=0), "n_systems"), (dict(nsys=65536, bi=P), "n_systems"), (dict(m=-1), "max_neighbors"),
              (dict(dtype=2), "dtype"), (dict(nsys=2), "batch_idx"), (dict(cell=None), "unit_shifts need a cell"), (dict(flags=8), "virial"),
              (dict(flags=8, vir=P, ush=None), "virial"), (dict(flags=8, vir=P, ush=None, cell=None), "virial"), (dict(pos=None), "null pointer"),
              (dict(q=None), "null pointer"), (dict(mu=None), "null pointer"), (dict(idx=None), "null pointer"), (dict(e=None), "nothing to compute"),
              (dict(flags=1), "forces output"), (dict(flags=2), "charge gradient output"), (dict(flags=4), "dipole gradient output"),
              (dict(scratch=None), "scratch"), (dict(nbytes=8), "scratch"))
    check(dipole, common + ((dict(flags=16), "unknown flag"), (dict(flags=32), "unknown flag")))
    check(quadrupole, common + ((dict(qd=None), "null pointer"), (dict(flags=16), "quadrupole gradient output"), (dict(flags=32), "unknown flag")))
    for call in (dipole, quadrupole):
        assert call(n=0, pos=None, q=None, mu=None, idx=None, e=None, scratch=None) == MI_OK  # nothing to do
        assert call(n=0, cell=None, ush=None, pos=None, q=None, mu=None, idx=None, e=None, scratch=None) == MI_OK  # a cluster
    assert lib.mi_coulomb_dipole_blocks() == lib.mi_ewald_dipole_blocks() == lib.mi_coulomb_quadrupole_blocks() == 64
    for n in (0, 1, 1000):
        for dt in (C.MI_F32, C.MI_F64):
            assert lib.mi_coulomb_dipole_scratch_bytes(n, dt) == lib.mi_ewald_dipole_real_scratch_bytes(n, dt)
            assert lib.mi_coulomb_quadrupole_scratch_bytes(n, dt) == lib.mi_ewald_quadrupole_real_scratch_bytes(n, dt)

    def tensors(**over):
        a = dict(pos=P, pol=P, n=4, dtype=C.MI_F64, idx=P, nptr=None, m=6, mask=-1, slots=24, t=P, nb=P, d=P, pc=P, a_t=0.0)
        a.update(over)
        return lib.mi_cluster_induced_pair_tensors(a["pos"], a["pol"], a["n"], a["dtype"], a["idx"], a["nptr"], a["m"], a["mask"], a["slots"], a["t"],
                                                   a["nb"], a["d"], a["pc"], ctypes.c_double(a["a_t"]), None)

    check(tensors, ((dict(n=-1), "n_atoms"), (dict(m=-1), "max_neighbors"), (dict(dtype=2), "dtype"), (dict(slots=-1), "n_slots"),
                    (dict(slots=23), "n_atoms * max_neighbors"), (dict(a_t=-0.39), "thole_a"), (dict(a_t=float("nan")), "thole_a"),
                    (dict(a_t=float("inf")), "thole_a"), (dict(a_t=-float("inf")), "thole_a"), (dict(pos=None), "null pointer"),
                    (dict(pol=None), "null pointer"), (dict(idx=None), "null pointer"), (dict(t=None), "null pointer"),
                    (dict(nb=None), "null pointer"), (dict(d=None), "null pointer"), (dict(pc=None), "null pointer"),
                    (dict(a_t=0.39, pos=None), "null pointer")))
    assert tensors(n=0, slots=0, pos=None, pol=None, idx=None, t=None, nb=None, d=None, pc=None) == MI_OK  # nothing to do
    assert tensors(n=0, slots=0, a_t=0.39, pos=None, pol=None, idx=None, t=None, nb=None, d=None, pc=None) == MI_OK


def test_header_declares_and_library_exports_the_entry_points():
    from tools.abi_symbols import declared_symbols

    declared = declared_symbols()
    assert set(SYMBOLS) <= set(declared)
    assert {s for s in declared if s.startswith(("mi_coulomb_dipole", "mi_coulomb_quadrupole", "mi_cluster_"))} == set(SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(C.lib(), name), name


def test_ops_are_registered_with_fake_implementations():
    from nvalchemiops import _eops

    for name in ("coulomb_dipole_correction_op", "coulomb_quadrupole_correction_op", "coulomb_dipole_bwd_op", "coulomb_quadrupole_bwd_op"):
        assert name in _eops.__all__ and hasattr(_eops, name)
    assert hasattr(torch.ops.alchemiops, "_coulomb_dipole_correction") and hasattr(torch.ops.alchemiops, "_coulomb_quadrupole_correction")
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        pos, q, mu, quad = torch.empty(5, 3), torch.empty(5), torch.empty(5, 3), torch.empty(5, 3, 3)
        nm = torch.empty((5, 4), dtype=torch.int32)
        out = _eops.coulomb_dipole_correction_op(pos, q, mu, None, None, None, None, None, nm, None, 5, True, False, True, False)
        assert [tuple(o.shape) for o in out] == [(5,), (5, 3), (0,), (5, 3), (0,)]
        out = _eops.coulomb_quadrupole_correction_op(pos, q, mu, quad, None, None, None, None, None, nm, None, 5, False, True, False, True, False)
        assert [tuple(o.shape) for o in out] == [(5,), (0,), (5,), (0,), (5, 3, 3), (0,)]
