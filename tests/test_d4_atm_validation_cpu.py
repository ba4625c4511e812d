"""`dftd4_atm` without a GPU: exports, the C ABI (declared, exported, sized), argument errors (`dftd4`'s messages and types), the refusal
to compute on CPU tensors, the empty-input contract and the registration of the two custom ops with shape-only implementations."""
import ctypes
import os

import pytest
import torch

from tests import d4_reference as R


def _params(**override):
    from nvalchemiops.interactions.dispersion import D4Parameters

    t = {k: torch.as_tensor(v) for k, v in R.d4_test_tables(9).items()}
    t.update(override)
    return D4Parameters(**t)


def _call(**kw):
    from nvalchemiops.interactions.dispersion import dftd4_atm

    n = 4
    args = dict(positions=torch.zeros((n, 3)), numbers=torch.ones(n, dtype=torch.int32), a1=0.4, a2=4.0, three_body_cutoff=8.0,
                d4_params=_params(), neighbor_matrix=torch.full((n, 3), n, dtype=torch.int32))
    args.update(kw)
    return dftd4_atm(**args)


def test_exports():
    import nvalchemiops.interactions.dispersion as D
    from nvalchemiops.interactions.dispersion.dftd4 import atm_tile, dftd4_atm

    assert "dftd4_atm" in D.__all__ and D.dftd4_atm is dftd4_atm and callable(dftd4_atm)
    assert {"dftd3", "dftd3_atm", "dftd3_zero", "dftd3_zero_atm", "dftd4", "D3Parameters", "D4Parameters"} <= set(D.__all__)
    assert atm_tile() >= 64


def test_abi_declares_exports_and_sizes_the_four_entry_points():
    from nvalchemiops import _capi as C
    from tools.abi_symbols import declared_symbols

    want = {"mi_d4_atm", "mi_d4_atm_workspace_bytes", "mi_d4_atm_visits_offset", "mi_d4_atm_tile"}
    assert want <= set(declared_symbols())
    if not os.path.exists(C._LIB_PATH):
        pytest.fail("libnvalchemiops_hip.so is not built: run build() first")
    lib = C.lib()
    assert all(hasattr(lib, s) for s in want)
    assert lib.mi_d4_atm_tile() >= 64
    small, large = lib.mi_d4_atm_workspace_bytes(10, 2, 20), lib.mi_d4_atm_workspace_bytes(1000, 2, 20)
    assert large > small > 0
    assert lib.mi_d4_atm_workspace_bytes(-1, 1, 20) == 0 and lib.mi_d4_atm_visits_offset(-1, 1, 20) == 0
    base = lib.mi_d4_workspace_bytes(1000, 2, 20)
    off = lib.mi_d4_atm_visits_offset(1000, 2, 20)
    assert large >= base + 3 * 4000 and base <= off <= large - 4000  # zeroed charges, float CN and the counters behind mi_d4's own layout


def test_entry_point_checks_its_arguments_before_any_launch():
    """Every check of `mi_d4_atm` fails on the host, before anything is launched: no device is needed to see its code and message.  All
    pointers, the element tables included, are fake non-null values (never dereferenced), so each case reaches its OWN check."""
    from nvalchemiops import _capi as C

    lib = C.lib()
    fake = 256
    tables = {k: fake for k in ("rcov", "en", "r4r2", "zeff", "gam", "n_ref", "ngw", "cn_ref", "q_ref", "c6_ref")}
    f = ctypes.c_float
    need = int(lib.mi_d4_atm_workspace_bytes(4, 1, 10))

    def call(n=4, nsys=1, s9=1.0, alpha=16.0, rc3=8.0, virial=0, ws_bytes=None, nz=10, k6=1.0, null=(), cell=0, shifts=0, virial_out=0, csr=0, width=3):
        par = C.MiD4Params(nz=nz, a1=0.4, a2=4.0, k_cn=7.5, k4=1.0, k5=1.0, k6=k6, wf=6.0, ga=3.0, gc=2.0, **{k: (None if k in null else v) for k, v in tables.items()})
        p = lambda name, on=1: ctypes.c_void_p(fake) if on and name not in null else None  # noqa: E731
        return lib.mi_d4_atm(p("positions"), p("numbers"), n, C.MI_F32, p("idx_j"), p("shifts", shifts), p("nptr", csr), width, n, p("cell", cell),
                             None, nsys, ctypes.byref(par), f(s9), f(alpha), f(rc3), virial, p("energy"), p("forces"), p("virial", virial_out),
                             p("workspace"), ctypes.c_size_t(need if ws_bytes is None else ws_bytes), None)

    EINVAL, EWORKSPACE = -1, -3  # MI_EINVAL, MI_EWORKSPACE of include/nvalchemiops_hip.h
    cases = [
        (dict(n=-1), "sizes"), (dict(nsys=0), "sizes"), (dict(width=-1), "max_neighbors"), (dict(nsys=2), "batch_idx is required"),
        (dict(rc3=0.0), "three_body_cutoff and alpha"), (dict(rc3=-1.0), "three_body_cutoff and alpha"),
        (dict(rc3=float("inf")), "three_body_cutoff and alpha"), (dict(rc3=float("nan")), "three_body_cutoff and alpha"),
        (dict(alpha=0.0), "three_body_cutoff and alpha"), (dict(alpha=float("nan")), "three_body_cutoff and alpha"),
        (dict(s9=float("inf")), "s9 must be finite"),
        (dict(null=("positions",)), "null pointer"), (dict(null=("numbers",)), "null pointer"), (dict(null=("energy",)), "null pointer"),
        (dict(null=("forces",)), "null pointer"), (dict(null=("workspace",)), "null pointer"), (dict(null=("idx_j",)), "idx_j is NULL"),
        (dict(null=("c6_ref",)), "D4 parameter tables"), (dict(null=("q_ref",)), "D4 parameter tables"), (dict(nz=1), "D4 parameter tables"),
        (dict(k6=0.0), "k6 must be positive"),
        (dict(virial=1), "virial needs its output, a cell and unit shifts"),                          # nothing of the three
        (dict(virial=1, virial_out=1), "virial needs its output, a cell and unit shifts"),            # no cell, no shifts
        (dict(virial=1, virial_out=1, cell=1), "virial needs its output, a cell and unit shifts"),    # no shifts
        (dict(virial=1, cell=1, shifts=1), "virial needs its output, a cell and unit shifts"),        # no output
        (dict(shifts=1), "unit_shifts without a cell"),
    ]
    for kw, message in cases:
        rc = call(**kw)
        text = lib.mi_last_error().decode()
        assert rc == EINVAL and "invalid argument" in text and message in text, (kw, rc, text)
    for short in (0, need - 1):
        rc = call(ws_bytes=short)
        assert rc == EWORKSPACE and "workspace too small" in lib.mi_last_error().decode(), (short, rc)
    assert call(n=0) == 0 and call(n=0, null=("positions", "energy", "workspace")) == 0  # no atoms: nothing to do, nothing is read


def test_list_and_argument_errors_are_dftd4s():
    n = 4
    nl = torch.zeros((2, 0), dtype=torch.int32)
    with pytest.raises(ValueError, match="Cannot provide both neighbor_matrix and neighbor_list"):
        _call(neighbor_list=nl, neighbor_ptr=torch.zeros(n + 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="Must provide either neighbor_matrix or neighbor_list"):
        _call(neighbor_matrix=None)
    with pytest.raises(ValueError, match="neighbor_ptr must be provided"):
        _call(neighbor_matrix=None, neighbor_list=nl)
    with pytest.raises(ValueError, match="unit_shifts is for neighbor_list format"):
        _call(unit_shifts=torch.zeros((0, 3), dtype=torch.int32))
    with pytest.raises(ValueError, match="Virial computation requires periodic boundary conditions"):
        _call(compute_virial=True)
    with pytest.raises(ValueError, match="provide neighbor_matrix_shifts along with cell"):
        _call(compute_virial=True, cell=torch.eye(3)[None])
    with pytest.raises(ValueError, match="a1 and a2 must be provided"):
        _call(a1=None)
    with pytest.raises(ValueError, match="a1 and a2 must be provided"):
        _call(a2=None)
    with pytest.raises(ValueError, match="three_body_cutoff must be provided"):
        _call(three_body_cutoff=None)
    with pytest.raises(ValueError, match="three_body_cutoff must be positive"):
        _call(three_body_cutoff=0.0)
    with pytest.raises(ValueError, match="alpha must be positive"):
        _call(alpha=-1.0)
    with pytest.raises(RuntimeError, match="DFT-D4 parameters must be explicitly provided"):
        _call(d4_params=None)
    with pytest.raises(ValueError, match="Must provide either"):  # the list checks come first, as in dftd4
        _call(d4_params=None, neighbor_matrix=None)
    with pytest.raises(ValueError, match=r"neighbor_matrix must have shape \[4, max_neighbors\]"):
        _call(neighbor_matrix=torch.full((3, 3), n, dtype=torch.int32))
    with pytest.raises(ValueError, match="numbers must have one entry per atom"):
        _call(numbers=torch.ones(3, dtype=torch.int32))
    with pytest.raises(KeyError):
        _call(d4_params={"rcov": torch.zeros(10)})
    with pytest.raises(TypeError):
        _call(charges=torch.zeros(n))  # the term is evaluated at q = 0: there is no such argument


def test_cpu_tensors_raise_native_library_error_and_empty_input_returns_zeros():
    from nvalchemiops._capi import NativeLibraryError

    with pytest.raises(NativeLibraryError, match="no CPU path"):
        _call()
    empty = dict(positions=torch.zeros((0, 3)), numbers=torch.zeros(0, dtype=torch.int32), neighbor_matrix=torch.zeros((0, 3), dtype=torch.int32))
    out = _call(**empty)
    assert len(out) == 2 and out[0].shape == (1,) and out[1].shape == (0, 3)
    assert all(o.dtype == torch.float32 for o in out) and float(out[0]) == 0.0
    out = _call(**empty, compute_virial=True, cell=torch.eye(3)[None], neighbor_matrix_shifts=torch.zeros((0, 3, 3), dtype=torch.int32))
    assert len(out) == 3 and out[2].shape == (0, 3, 3)


def test_custom_ops_are_registered_with_shape_only_implementations():
    import nvalchemiops  # noqa: F401

    p = _params()
    n, m = 5, 7
    meta = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device="meta")  # noqa: E731
    tables = [getattr(p, k).to("meta") for k in R.TABLE_KEYS]
    out = (meta(1), meta(n, 3), meta(1, 3, 3))
    for name in ("dftd4_atm_nm", "dftd4_atm_nl"):
        op = getattr(torch.ops.nvalchemiops, name)
        schema = str(op.default._schema)
        assert "Tensor(a" in schema and "energy" in schema and "three_body_cutoff" in schema and "charges" not in schema  # mutation-annotated outputs
    # a shape-only run: nothing is launched (there is no device), nothing is returned, the outputs keep their shapes
    assert torch.ops.nvalchemiops.dftd4_atm_nm(meta(n, 3), meta(n, dtype=torch.int32), meta(n, m, dtype=torch.int32), *tables, 0.4, 4.0, 8.0,
                                               *out) is None
    assert torch.ops.nvalchemiops.dftd4_atm_nl(meta(n, 3), meta(n, dtype=torch.int32), meta(11, dtype=torch.int32),
                                               meta(n + 1, dtype=torch.int32), *tables, 0.4, 4.0, 8.0, *out, compute_virial=True,
                                               cell=meta(1, 3, 3), unit_shifts=meta(11, 3, dtype=torch.int32)) is None
    assert out[0].shape == (1,) and out[1].shape == (n, 3) and out[2].shape == (1, 3, 3)
