"""`dftd3_zero` / `dftd3_zero_atm`: argument validation (dftd3's messages for the same misuse, plus the zero-damping parameters and the table of pair cutoff
radii), parameter resolution, empty input, no CPU fallback, and the C ABI of the zero-damping entry points.  Runs without a GPU: everything
here is raised before any device work."""
import inspect
import os

import pytest
import torch


def _args(n=4, nz=10):
    r = torch.rand
    tables = dict(rcov=r(nz), r4r2=r(nz), c6ab=r(nz, nz, 5, 5), cn_ref=r(nz, nz, 5, 5))
    nm = torch.full((n, 6), n, dtype=torch.int32)
    return torch.rand(n, 3), torch.ones(n, dtype=torch.int32), tables, r(nz, nz) + 3.0, nm


def test_names_are_exported_and_the_signature_is_the_documented_one():
    import nvalchemiops.interactions.dispersion as D
    from nvalchemiops.interactions.dispersion import dftd3, dftd3_zero

    assert "dftd3_zero" in D.__all__ and "dftd3_zero_atm" in D.__all__ and callable(D.dftd3_zero_atm)
    sig = inspect.signature(dftd3_zero)
    assert list(sig.parameters) == [
        "positions", "numbers", "rs6", "s8", "rs8", "alpha", "beta", "k1", "k3", "s6", "s5_smoothing_on", "s5_smoothing_off", "fill_value",
        "d3_params", "covalent_radii", "r4r2", "c6_reference", "coord_num_ref", "cutoff_radii", "batch_idx", "cell", "neighbor_matrix",
        "neighbor_matrix_shifts", "neighbor_list", "neighbor_ptr", "unit_shifts", "compute_virial", "num_systems", "device"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["rs8"], d["alpha"], d["beta"], d["s6"], d["k1"], d["k3"]) == (1.0, 14.0, 0.0, 1.0, 16.0, -4.0)
    assert d["rs6"] is inspect.Parameter.empty and d["s8"] is inspect.Parameter.empty and d["cutoff_radii"] is None
    two_body = inspect.signature(dftd3).parameters
    for name in two_body:  # everything dftd3 takes besides its own damping parameters, with the same defaults
        if name not in ("a1", "a2", "s8"):
            assert sig.parameters[name].default == two_body[name].default, name


def test_dftd3_signature_is_untouched():
    from nvalchemiops.interactions.dispersion import dftd3

    names = list(inspect.signature(dftd3).parameters)
    assert names[:5] == ["positions", "numbers", "a1", "a2", "s8"] and "cutoff_radii" not in names


def test_misuse_raises_dftd3_messages():
    from nvalchemiops.interactions.dispersion import dftd3_zero

    pos, z, tables, r0ab, nm = _args()
    lst, ptr = torch.zeros((2, 0), dtype=torch.int32), torch.zeros(5, dtype=torch.int32)
    ok = dict(rs6=1.2, s8=0.7, d3_params=tables, cutoff_radii=r0ab)
    cases = [
        (ValueError, "Cannot provide both neighbor_matrix and neighbor_list", dict(neighbor_matrix=nm, neighbor_list=lst, neighbor_ptr=ptr)),
        (ValueError, "Must provide either neighbor_matrix or neighbor_list", {}),
        (ValueError, "unit_shifts is for neighbor_list format", dict(neighbor_matrix=nm, unit_shifts=torch.zeros((0, 3), dtype=torch.int32))),
        (ValueError, "neighbor_matrix_shifts is for neighbor_matrix format",
         dict(neighbor_list=lst, neighbor_ptr=ptr, neighbor_matrix_shifts=torch.zeros((4, 6, 3), dtype=torch.int32))),
        (ValueError, "neighbor_ptr must be provided when using neighbor_list format", dict(neighbor_list=lst)),
        (ValueError, "Virial computation requires periodic boundary conditions", dict(neighbor_matrix=nm, compute_virial=True)),
        (ValueError, "Please provide neighbor_matrix_shifts along with cell", dict(neighbor_matrix=nm, compute_virial=True, cell=torch.eye(3)[None])),
        (ValueError, "Please provide unit_shifts along with cell", dict(neighbor_list=lst, neighbor_ptr=ptr, compute_virial=True, cell=torch.eye(3)[None])),
    ]
    for exc, match, kw in cases:
        with pytest.raises(exc, match=match):
            dftd3_zero(pos, z, **ok, **kw)
    with pytest.raises(RuntimeError, match="DFT-D3 parameters must be explicitly provided"):
        dftd3_zero(pos, z, rs6=1.2, s8=0.7, cutoff_radii=r0ab, neighbor_matrix=nm)


def test_new_error_paths():
    from nvalchemiops.interactions.dispersion import D3Parameters, dftd3_zero

    pos, z, tables, r0ab, nm = _args()
    for kw in (dict(rs6=None, s8=0.7), dict(rs6=1.2, s8=None)):
        with pytest.raises(ValueError, match="Functional parameters rs6 and s8 must be provided"):
            dftd3_zero(pos, z, d3_params=tables, cutoff_radii=r0ab, neighbor_matrix=nm, **kw)
    with pytest.raises(TypeError):  # rs6 / s8 have no default
        dftd3_zero(pos, z, d3_params=tables, cutoff_radii=r0ab, neighbor_matrix=nm)
    for bad in (0.0, -14.0):
        with pytest.raises(ValueError, match="alpha must be positive"):
            dftd3_zero(pos, z, rs6=1.2, s8=0.7, alpha=bad, d3_params=tables, cutoff_radii=r0ab, neighbor_matrix=nm)
    # radii: missing (no explicit tensor, a dict without the key, a D3Parameters instance, which never carries them)
    params = D3Parameters(**tables)
    for src in (tables, params):
        with pytest.raises(RuntimeError, match="pair cutoff radii must be explicitly provided"):
            dftd3_zero(pos, z, rs6=1.2, s8=0.7, d3_params=src, neighbor_matrix=nm)
    # radii: wrong shape
    for shape in ((9, 9), (10,), (10, 10, 1), (10, 11)):
        with pytest.raises(ValueError, match=r"cutoff_radii must have shape \[10, 10\] to match rcov"):
            dftd3_zero(pos, z, rs6=1.2, s8=0.7, d3_params=tables, cutoff_radii=torch.ones(shape), neighbor_matrix=nm)
    with pytest.raises(TypeError, match="cutoff_radii"):
        dftd3_zero(pos, z, rs6=1.2, s8=0.7, d3_params=tables, cutoff_radii=torch.ones((10, 10), dtype=torch.int32), neighbor_matrix=nm)


def test_radii_resolve_from_dict_key_and_next_to_d3parameters_and_no_cpu_fallback():
    """Resolution succeeds (the call gets as far as the device check, which CPU tensors fail) for: the "r0ab" key of a dict, an explicit
    table next to a dict, an explicit table next to a D3Parameters instance, explicit tables only; float64 tables are accepted."""
    from nvalchemiops import _capi as C
    from nvalchemiops.interactions.dispersion import D3Parameters, dftd3_zero

    pos, z, tables, r0ab, nm = _args()
    with_key = dict(tables, r0ab=r0ab)
    explicit = dict(covalent_radii=tables["rcov"], r4r2=tables["r4r2"], c6_reference=tables["c6ab"], coord_num_ref=tables["cn_ref"])
    for kw in (dict(d3_params=with_key), dict(d3_params=tables, cutoff_radii=r0ab), dict(d3_params=D3Parameters(**tables), cutoff_radii=r0ab),
               dict(cutoff_radii=r0ab.double(), **explicit), dict(d3_params=with_key, cutoff_radii=r0ab + 1.0)):
        with pytest.raises(C.NativeLibraryError, match="no CPU path"):
            dftd3_zero(pos, z, rs6=1.2, s8=0.7, neighbor_matrix=nm, **kw)
    # an explicit table wins over the dict entry: a mis-shaped explicit one is what gets checked
    with pytest.raises(ValueError, match="cutoff_radii must have shape"):
        dftd3_zero(pos, z, rs6=1.2, s8=0.7, d3_params=with_key, cutoff_radii=torch.ones(3, 3), neighbor_matrix=nm)


def test_empty_input():
    from nvalchemiops.interactions.dispersion import dftd3_zero

    _, _, tables, r0ab, _ = _args()
    e, f, cn = dftd3_zero(torch.zeros((0, 3)), torch.zeros(0, dtype=torch.int32), rs6=1.2, s8=0.7, d3_params=tables, cutoff_radii=r0ab,
                          neighbor_matrix=torch.zeros((0, 4), dtype=torch.int32))
    assert e.shape == (1,) and f.shape == (0, 3) and cn.shape == (0,) and float(e) == 0.0
    assert e.dtype == f.dtype == cn.dtype == torch.float32
    out = dftd3_zero(torch.zeros((0, 3)), torch.zeros(0, dtype=torch.int32), rs6=1.2, s8=0.7, d3_params=tables, cutoff_radii=r0ab,
                     neighbor_matrix=torch.zeros((0, 4), dtype=torch.int32), neighbor_matrix_shifts=torch.zeros((0, 4, 3), dtype=torch.int32),
                     cell=torch.eye(3)[None], compute_virial=True)
    assert len(out) == 4 and out[3].shape == (0, 3, 3)


def test_abi_declares_and_exports_the_zero_damping_entry_points():
    import ctypes

    from nvalchemiops import _capi as C
    from tools.abi_symbols import declared_symbols

    want = {"mi_d3_zero", "mi_d3_zero_packed_cn", "mi_d3_zero_atm"}
    assert want <= set(declared_symbols())
    if not os.path.exists(C._LIB_PATH):
        pytest.fail("libnvalchemiops_hip.so is not built: run build() first")
    lib = C.lib()
    assert all(hasattr(lib, s) for s in want)
    assert lib.mi_version() == 1
    # the struct of the header: four floats, then the table pointer
    assert [n for n, _ in C.MiD3ZeroParams._fields_] == ["rs6", "rs8", "alpha", "beta", "r0ab"]
    assert ctypes.sizeof(C.MiD3ZeroParams) == 24 and C.MiD3ZeroParams.r0ab.offset == 16
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nvalchemiops_hip.h")).read()
    assert "mi_d3_zero_params" in header and "float rs6, rs8, alpha, beta;" in header


def test_custom_ops_are_registered():
    import nvalchemiops  # noqa: F401

    for name, arg in (("dftd3_zero_nm", "rs6"), ("dftd3_zero_nl", "rs6"), ("dftd3_zero_atm_nm", "rs9"), ("dftd3_zero_atm_nl", "rs9")):
        op = getattr(torch.ops.nvalchemiops, name)
        schema = str(op.default._schema)
        assert "Tensor(a" in schema and "energy" in schema and "cutoff_radii" in schema and arg in schema  # mutation-annotated outputs


def test_three_body_signature_validation_empty_input_and_no_cpu_fallback():
    from nvalchemiops import _capi as C
    from nvalchemiops.interactions.dispersion import D3Parameters, dftd3_atm, dftd3_zero_atm

    sig = inspect.signature(dftd3_zero_atm)
    names = list(sig.parameters)
    assert names[:4] == ["positions", "numbers", "three_body_cutoff", "cutoff_radii"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["rs9"] == 4.0 / 3.0 and d["s9"] == 1.0 and d["alpha"] == 16.0 and d["cutoff_radii"] is None
    bj = inspect.signature(dftd3_atm).parameters
    for name in bj:  # everything dftd3_atm takes besides a1 / a2, with the same defaults
        if name not in ("a1", "a2"):
            assert sig.parameters[name].default == bj[name].default, name
    pos, z, tables, r0ab, nm = _args()
    ok = dict(d3_params=tables, cutoff_radii=r0ab, neighbor_matrix=nm)
    with pytest.raises(ValueError, match="three_body_cutoff must be provided"):
        dftd3_zero_atm(pos, z, None, **ok)
    for bad in (0.0, -3.0):
        with pytest.raises(ValueError, match="three_body_cutoff must be positive"):
            dftd3_zero_atm(pos, z, bad, **ok)
    with pytest.raises(ValueError, match="alpha must be positive"):
        dftd3_zero_atm(pos, z, 5.0, alpha=0.0, **ok)
    with pytest.raises(ValueError, match="rs9 must be positive"):
        dftd3_zero_atm(pos, z, 5.0, rs9=0.0, **ok)
    for src in (tables, D3Parameters(**tables)):
        with pytest.raises(RuntimeError, match="pair cutoff radii must be explicitly provided"):
            dftd3_zero_atm(pos, z, 5.0, d3_params=src, neighbor_matrix=nm)
    with pytest.raises(ValueError, match="cutoff_radii must have shape"):
        dftd3_zero_atm(pos, z, 5.0, d3_params=tables, cutoff_radii=torch.ones(4, 4), neighbor_matrix=nm)
    with pytest.raises(ValueError, match="Must provide either neighbor_matrix or neighbor_list"):
        dftd3_zero_atm(pos, z, 5.0, d3_params=tables, cutoff_radii=r0ab)
    e, f = dftd3_zero_atm(torch.zeros((0, 3)), torch.zeros(0, dtype=torch.int32), 5.0, d3_params=tables, cutoff_radii=r0ab,
                          neighbor_matrix=torch.zeros((0, 4), dtype=torch.int32))
    assert e.shape == (1,) and f.shape == (0, 3) and e.dtype == torch.float32 and float(e) == 0.0
    for kw in (dict(d3_params=dict(tables, r0ab=r0ab)), dict(d3_params=D3Parameters(**tables), cutoff_radii=r0ab)):
        with pytest.raises(C.NativeLibraryError, match="no CPU path"):
            dftd3_zero_atm(pos, z, 5.0, neighbor_matrix=nm, **kw)
