"""`pair_scale_correction`: what can be checked without a GPU -- export and signature, every argument error (raised before anything is
launched), the absence of a CPU path, empty inputs, the argument checks of the C entry point (which return before any device call), the
header / library / build list, and the two custom ops under FakeTensorMode."""
import ctypes
import inspect
import os

import pytest
import torch

from nvalchemiops import _capi as C

MI_OK, MI_EINVAL = 0, -1  # include/nvalchemiops_hip.h
P = ctypes.c_void_p(4096)  # a non-null pointer that is never dereferenced: every call below fails its checks first
SYMBOLS = ("mi_pair_scale", "mi_pair_scale_scratch_bytes", "mi_pair_scale_blocks")
LISTS = ["neighbor_list", "neighbor_ptr", "neighbor_shifts", "neighbor_matrix", "neighbor_matrix_shifts"]


def _fn():
    from nvalchemiops.interactions.electrostatics import pair_scale_correction

    return pair_scale_correction


def _args(n=4, m=6):
    pos, q, mu, quad, cell = torch.rand(n, 3), torch.rand(n), torch.rand(n, 3), torch.rand(n, 3, 3), torch.eye(3)[None] * 10
    nm = torch.full((n, m), n, dtype=torch.int32)
    return pos, q, mu, quad, torch.zeros(n, m), cell, nm, torch.zeros((n, m, 3), dtype=torch.int32)


def test_exported_with_the_documented_signature():
    import nvalchemiops.interactions.electrostatics as E
    from nvalchemiops.interactions.electrostatics import pair_scale as PS

    for name in ("pair_scale_correction", "bonded_pair_scales"):
        assert name in E.__all__ and name in PS.__all__ and getattr(E, name) is getattr(PS, name)
    p = inspect.signature(PS.pair_scale_correction).parameters
    assert list(p) == (["positions", "charges", "dipoles", "quadrupoles", "pair_scales", "cell"] + LISTS
                       + ["mask_value", "batch_idx", "minimum_image", "compute_forces", "compute_charge_gradients", "compute_dipole_gradients",
                          "compute_quadrupole_gradients", "compute_virial"])
    assert p["cell"].default is None and p["mask_value"].default == -1 and p["minimum_image"].default is False
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[6:])
    assert all(p[k].default is False for k in p if k.startswith("compute_"))
    doc = PS.pair_scale_correction.__doc__
    for words in ("ADD", "FULL", "SYMMETRIC", "exclusion", "minimum image", "external_field += dipole_grads", "polarisation groups", "dE/ds",
                  "Thole-damped", "induced_dipoles"):
        assert words in doc, words


def test_scale_and_image_errors():
    fn = _fn()
    pos, q, mu, quad, s, cell, nm, sh = _args()
    lst, ptr, lsh = torch.zeros((2, 3), dtype=torch.int32), torch.zeros(5, dtype=torch.int32), torch.zeros((3, 3), dtype=torch.int32)
    for bad in (s[:3], s[:, :5], s.reshape(-1), torch.zeros(3)):
        with pytest.raises(ValueError, match="pair_scales must have the shape of the index array"):
            fn(pos, q, mu, quad, bad, neighbor_matrix=nm)
    for bad in (torch.zeros(2), torch.zeros(4), torch.zeros((2, 3))):
        with pytest.raises(ValueError, match=r"pair_scales must have the shape of the index array: expected \[3\]"):
            fn(pos, q, mu, quad, bad, neighbor_list=lst, neighbor_ptr=ptr)
    for bad in (s.to(torch.int32), s.half()):
        with pytest.raises(ValueError, match="pair_scales must be float32 or float64"):
            fn(pos, q, mu, quad, bad, neighbor_matrix=nm)
    with pytest.raises(ValueError, match="pair_scales must be a tensor"):
        fn(pos, q, mu, quad, 0.5, neighbor_matrix=nm)
    with pytest.raises(NotImplementedError, match="pair_scales is not differentiable"):
        fn(pos, q, mu, quad, s.clone().requires_grad_(True), neighbor_matrix=nm)
    with pytest.raises(ValueError, match="minimum_image needs a cell"):
        fn(pos, q, mu, quad, s, neighbor_matrix=nm, minimum_image=True)
    with pytest.raises(ValueError, match="minimum_image takes a list without shifts"):
        fn(pos, q, mu, quad, s, cell, neighbor_matrix=nm, neighbor_matrix_shifts=sh, minimum_image=True)
    with pytest.raises(ValueError, match="minimum_image takes a list without shifts"):
        fn(pos, q, mu, quad, torch.zeros(3), cell, neighbor_list=lst, neighbor_ptr=ptr, neighbor_shifts=lsh, minimum_image=True)
    with pytest.raises(TypeError):  # the lists are keyword-only
        fn(pos, q, mu, quad, s, cell, nm)


def test_list_and_shape_errors_are_those_of_coulomb_quadrupole_correction():
    from nvalchemiops.interactions.electrostatics import coulomb_quadrupole_correction as qd

    fn = _fn()
    pos, q, mu, quad, s, cell, nm, sh = _args()
    lst, ptr, lsh = torch.zeros((2, 3), dtype=torch.int32), torch.zeros(5, dtype=torch.int32), torch.zeros((3, 3), dtype=torch.int32)
    s3 = torch.zeros(3)
    cases = [((pos, q, mu, quad), dict()), ((pos, q, mu, quad), dict(neighbor_list=lst)),
             ((pos, q, mu, quad), dict(neighbor_matrix=nm, neighbor_list=lst, neighbor_ptr=ptr)),
             ((pos, q, mu, quad), dict(cell=cell, neighbor_matrix=nm[:3], neighbor_matrix_shifts=sh)),
             ((pos, q, mu, quad), dict(cell=cell, neighbor_matrix=nm, neighbor_matrix_shifts=sh[:, :5])),
             ((pos, q, mu, quad), dict(cell=cell, neighbor_list=lst, neighbor_ptr=ptr[:4], neighbor_shifts=lsh)),
             ((pos, q, mu, quad), dict(cell=cell, neighbor_matrix=nm, neighbor_matrix_shifts=sh, batch_idx=torch.zeros(3, dtype=torch.int32))),
             ((pos, q, mu, quad), dict(cell=cell, neighbor_matrix=nm, compute_virial=True)),
             ((pos, q, mu, quad), dict(cell=cell, neighbor_list=lst, neighbor_ptr=ptr, compute_virial=True)),
             ((pos, q, mu, quad), dict(cell=torch.eye(4), neighbor_matrix=nm, neighbor_matrix_shifts=sh)),
             ((pos, q, mu, quad), dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh)),
             ((pos, q, mu, quad), dict(neighbor_list=lst, neighbor_ptr=ptr, neighbor_shifts=lsh)),
             ((pos, q, mu, quad), dict(neighbor_matrix=nm, compute_virial=True)),
             ((pos[:, :2], q, mu, quad), dict(neighbor_matrix=nm)), ((pos, q[:3], mu, quad), dict(neighbor_matrix=nm)),
             ((pos, q, mu[:3], quad), dict(neighbor_matrix=nm)), ((pos, q, torch.zeros(4, 4), quad), dict(neighbor_matrix=nm)),
             ((pos, q, mu, quad[:3]), dict(neighbor_matrix=nm)), ((pos, q, mu, torch.zeros(4, 9)), dict(neighbor_matrix=nm)),
             ((pos.half(), q, mu, quad), dict(neighbor_matrix=nm))]
    for (a, b, c, d), kw in cases:
        with pytest.raises(ValueError) as theirs:
            qd(a, b, c, d, **kw)
        with pytest.raises(ValueError) as ours:
            fn(a, b, c, d, s3 if "neighbor_list" in kw and "neighbor_matrix" not in kw else s, **kw)
        assert str(ours.value) == str(theirs.value), kw
    # under minimum_image the virial needs no shifts: the call gets as far as the device check
    with pytest.raises(C.NativeLibraryError, match="ROCm devices only"):
        fn(pos, q, mu, quad, s, cell, neighbor_matrix=nm, minimum_image=True, compute_virial=True)


def test_no_cpu_fallback():
    fn = _fn()
    pos, q, mu, quad, s, cell, nm, sh = _args()
    lst, ptr, lsh = torch.zeros((2, 3), dtype=torch.int32), torch.tensor([0, 1, 2, 3, 3], dtype=torch.int32), torch.zeros((3, 3), dtype=torch.int32)
    s3 = torch.zeros(3, dtype=torch.float64)
    for sc, kw in ((s, dict(neighbor_matrix=nm)), (s3, dict(neighbor_list=lst, neighbor_ptr=ptr)),
                   (s, dict(cell=cell, neighbor_matrix=nm, neighbor_matrix_shifts=sh)), (s, dict(cell=cell, neighbor_matrix=nm, minimum_image=True)),
                   (s3, dict(cell=cell, neighbor_list=lst, neighbor_ptr=ptr, neighbor_shifts=lsh))):
        for d, qq in ((mu, quad), (None, quad), (mu, None), (None, None)):
            with pytest.raises(C.NativeLibraryError, match="ROCm devices only"):
                fn(pos, q, d, qq, sc, **kw)
    with pytest.raises(C.NativeLibraryError):  # under autograd as well
        fn(pos, q, mu, quad.clone().requires_grad_(True), s, neighbor_matrix=nm)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_zero_atoms(dtype):
    fn = _fn()
    z, z3, z33 = torch.zeros(0, dtype=dtype), torch.zeros((0, 3), dtype=dtype), torch.zeros((0, 3, 3), dtype=dtype)
    nm, sh, s = torch.zeros((0, 5), dtype=torch.int32), torch.zeros((0, 5, 3), dtype=torch.int32), torch.zeros((0, 5))
    e = fn(z3, z, None, None, s, neighbor_matrix=nm)
    assert e.shape == (0,) and e.dtype == dtype
    every = dict(compute_forces=True, compute_charge_gradients=True, compute_dipole_gradients=True, compute_quadrupole_gradients=True)
    out = fn(z3, z, z3, z33, s, torch.eye(3, dtype=dtype).repeat(2, 1, 1) * 9, neighbor_matrix=nm, neighbor_matrix_shifts=sh,
             batch_idx=torch.zeros(0, dtype=torch.int32), compute_virial=True, **every)
    assert [tuple(o.shape) for o in out] == [(0,), (0, 3), (0,), (0, 3), (0, 3, 3), (2, 3, 3)] and all(o.dtype == dtype for o in out)
    out = fn(z3, z, None, z33, s, neighbor_matrix=nm, **every)
    assert [tuple(o.shape) for o in out] == [(0,), (0, 3), (0,), (0, 3), (0, 3, 3)]


def test_c_entry_point_rejects_bad_arguments_before_any_device_call():
    lib = C.lib()
    err = lambda: lib.mi_last_error().decode()  # noqa: E731

    def call(**over):
        a = dict(pos=P, q=P, mu=P, qd=P, cell=P, bi=None, w=None, scl=P, n=4, nsys=1, dtype=C.MI_F64, idx=P, ush=P, nptr=None, m=6, mask=-1, mi=0,
                 flags=0, e=P, f=None, cg=None, dg=None, qg=None, vir=None, scratch=P, nbytes=1 << 20)
        a.update(over)
        return lib.mi_pair_scale(a["pos"], a["q"], a["mu"], a["qd"], a["cell"], a["bi"], a["w"], a["scl"], a["n"], a["nsys"], a["dtype"], a["idx"],
                                 a["ush"], a["nptr"], a["m"], a["mask"], a["mi"], a["flags"], a["e"], a["f"], a["cg"], a["dg"], a["qg"], a["vir"],
                                 a["scratch"], ctypes.c_size_t(a["nbytes"]), None)

    for bad, fragment in ((dict(n=-1), "n_atoms"), (dict(nsys=0), "n_systems"), (dict(nsys=65536, bi=P), "n_systems"), (dict(m=-1), "max_neighbors"),
                          (dict(dtype=2), "dtype"), (dict(nsys=2), "batch_idx"), (dict(cell=None), "unit_shifts need a cell"),
                          (dict(flags=32), "unknown flag"), (dict(flags=64), "unknown flag"),
                          (dict(mi=1, cell=None, ush=None), "minimum_image needs a cell"), (dict(mi=1), "without unit_shifts"),
                          (dict(flags=8), "virial"), (dict(flags=8, vir=P, ush=None), "virial"), (dict(flags=8, ush=None, mi=1), "virial"),
                          (dict(pos=None), "null pointer"), (dict(q=None), "null pointer"), (dict(idx=None), "null pointer"),
                          (dict(scl=None), "null pointer"), (dict(e=None), "nothing to compute"), (dict(flags=1), "forces output"),
                          (dict(flags=2), "charge gradient output"), (dict(flags=4), "dipole gradient output"),
                          (dict(flags=16), "quadrupole gradient output"), (dict(scratch=None), "scratch"), (dict(nbytes=8), "scratch")):
        assert call(**bad) == MI_EINVAL, bad
        assert "invalid argument" in err() and fragment in err(), (bad, err())
    assert call(n=0, pos=None, q=None, mu=None, qd=None, idx=None, scl=None, e=None, scratch=None) == MI_OK  # nothing to do
    assert call(n=0, cell=None, ush=None, pos=None, q=None, idx=None, scl=None, e=None, scratch=None) == MI_OK  # a cluster
    assert call(n=0, ush=None, mi=1, flags=8, vir=P, pos=None, q=None, idx=None, scl=None, scratch=None) == MI_OK  # minimum image with a virial
    assert lib.mi_pair_scale_blocks() == lib.mi_coulomb_quadrupole_blocks() == 64
    for n in (0, 1, 1000):
        for dt in (C.MI_F32, C.MI_F64):
            assert lib.mi_pair_scale_scratch_bytes(n, dt) == lib.mi_coulomb_quadrupole_scratch_bytes(n, dt)


def test_header_declares_library_exports_and_the_build_lists_the_source():
    from tools.abi_symbols import declared_symbols

    declared = declared_symbols()
    assert {s for s in declared if s.startswith("mi_pair_scale")} == set(SYMBOLS)
    for name in SYMBOLS:
        assert hasattr(C.lib(), name), name
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import importlib.util

    spec = importlib.util.spec_from_file_location("build_native", os.path.join(root, "nvalchemi-toolkit-ops_amd", "build_native.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.SOURCES["pair_scale.hip"] == [] and os.path.exists(os.path.join(mod.CSRC, "pair_scale.hip"))
    assert os.path.exists(os.path.join(mod.CSRC, "qd_record.h"))
    src = open(os.path.join(mod.CSRC, "pair_scale.hip")).read()
    assert '#include "qd_record.h"' in src and '#include "qd_record.h"' in open(os.path.join(mod.CSRC, "quadrupole.hip")).read()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_ops_under_fake_tensors(dtype):
    """Output shapes with every flag on, the (0,) placeholders with every flag off, the positions dtype, float64 gradients in the shapes of the
    differentiable inputs; 7 atoms, with two cells and without one; matrix and CSR scales."""
    from torch._subclasses.fake_tensor import FakeTensorMode

    from nvalchemiops import _eops

    for name in ("pair_scale_correction_op", "pair_scale_bwd_op"):
        assert name in _eops.__all__ and hasattr(_eops, name)
    forward, backward = torch.ops.alchemiops._pair_scale_correction, torch.ops.nvalchemiops.pair_scale_correction_backward
    assert "Tensor pair_scales" in str(forward.default._schema) and "bool minimum_image" in str(forward.default._schema)
    n, b, w, i32 = 7, 2, 6, torch.int32
    per_atom = [(), (3,), (), (3,), (3, 3)]
    for with_cell, min_image in ((True, False), (True, True), (False, False)):
        with FakeTensorMode():
            lead = [torch.empty((n,) + s, dtype=dtype) for s in ((3,), (), (3,), (3, 3))]
            cell = torch.empty((b, 3, 3), dtype=dtype) if with_cell else None
            bi = torch.empty(n, dtype=i32) if with_cell else None
            sh = torch.empty((n, w, 3), dtype=i32) if with_cell and not min_image else None
            args = lead + [torch.empty((n, w), dtype=torch.float32), cell, bi, None, None, None, torch.empty((n, w), dtype=i32), sh, n + 3, min_image]
            on, off = forward(*args, *[True] * 5), forward(*args, *[False] * 5)
            grads = backward(*args, torch.empty(n, dtype=dtype))
            csr = lead + [torch.empty(11, dtype=torch.float64), cell, bi, torch.empty((2, 11), dtype=i32), torch.empty(n + 1, dtype=i32), None, None,
                          None, -1, min_image]
            on_csr = forward(*csr, *[True] * 5)
        nsys = b if with_cell else 1
        for out in (on, on_csr):
            assert [tuple(o.shape) for o in out] == [(n,) + s for s in per_atom] + [(nsys, 3, 3)]
        assert [tuple(o.shape) for o in off] == [(n,)] + [(0,)] * 5
        assert all(o.dtype == dtype for o in on + off)
        assert [tuple(g.shape) for g in grads] == [(n, 3), (n,), (n, 3), (n, 3, 3)] and all(g.dtype == torch.float64 for g in grads)
