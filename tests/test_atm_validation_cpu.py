"""`dftd3_atm`: argument validation (dftd3's messages for the same misuse, plus the three-body cutoff), no CPU fallback, and the C ABI of
the three-body entry points.  Runs without a GPU: everything here is raised before any device work."""
import inspect
import os

import pytest
import torch


def _args(n=4):
    r = torch.rand
    tables = dict(rcov=r(10), r4r2=r(10), c6ab=r(10, 10, 5, 5), cn_ref=r(10, 10, 5, 5))
    nm = torch.full((n, 6), n, dtype=torch.int32)
    return torch.rand(n, 3), torch.ones(n, dtype=torch.int32), tables, nm


def test_signature_sits_next_to_dftd3():
    from nvalchemiops.interactions.dispersion import dftd3, dftd3_atm

    sig = inspect.signature(dftd3_atm)
    names = list(sig.parameters)
    assert names[:5] == ["positions", "numbers", "a1", "a2", "three_body_cutoff"]
    assert sig.parameters["s9"].default == 1.0 and sig.parameters["alpha"].default == 16.0
    assert sig.parameters["k1"].default == 16.0 and sig.parameters["k3"].default == -4.0
    shared = ["fill_value", "d3_params", "covalent_radii", "r4r2", "c6_reference", "coord_num_ref", "batch_idx", "cell", "neighbor_matrix",
              "neighbor_matrix_shifts", "neighbor_list", "neighbor_ptr", "unit_shifts", "compute_virial", "num_systems"]
    two_body = inspect.signature(dftd3).parameters
    for name in shared:
        assert name in sig.parameters and name in two_body
        assert sig.parameters[name].default == two_body[name].default


def test_misuse_raises_dftd3_messages():
    from nvalchemiops.interactions.dispersion import dftd3_atm

    pos, z, tables, nm = _args()
    lst, ptr = torch.zeros((2, 0), dtype=torch.int32), torch.zeros(5, dtype=torch.int32)
    ok = dict(a1=0.4, a2=4.0, three_body_cutoff=10.0, d3_params=tables)
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
            dftd3_atm(pos, z, **ok, **kw)
    with pytest.raises(RuntimeError, match="DFT-D3 parameters must be explicitly provided"):
        dftd3_atm(pos, z, a1=0.4, a2=4.0, three_body_cutoff=10.0, neighbor_matrix=nm)
    with pytest.raises(ValueError, match="Functional parameters a1 and a2 must be provided"):
        dftd3_atm(pos, z, a1=None, a2=4.0, three_body_cutoff=10.0, d3_params=tables, neighbor_matrix=nm)


def test_three_body_cutoff_is_required_and_positive():
    from nvalchemiops.interactions.dispersion import dftd3_atm

    pos, z, tables, nm = _args()
    with pytest.raises(TypeError, match="three_body_cutoff"):
        dftd3_atm(pos, z, a1=0.4, a2=4.0, d3_params=tables, neighbor_matrix=nm)
    with pytest.raises(ValueError, match="three_body_cutoff must be provided"):
        dftd3_atm(pos, z, a1=0.4, a2=4.0, three_body_cutoff=None, d3_params=tables, neighbor_matrix=nm)
    for bad in (0.0, -3.0):
        with pytest.raises(ValueError, match="three_body_cutoff must be positive"):
            dftd3_atm(pos, z, a1=0.4, a2=4.0, three_body_cutoff=bad, d3_params=tables, neighbor_matrix=nm)
    with pytest.raises(ValueError, match="alpha must be positive"):
        dftd3_atm(pos, z, a1=0.4, a2=4.0, three_body_cutoff=5.0, alpha=0.0, d3_params=tables, neighbor_matrix=nm)


def test_empty_input_and_no_cpu_fallback():
    from nvalchemiops import _capi as C
    from nvalchemiops.interactions.dispersion import dftd3_atm

    pos, z, tables, nm = _args()
    e, f = dftd3_atm(torch.zeros((0, 3)), torch.zeros(0, dtype=torch.int32), a1=0.4, a2=4.0, three_body_cutoff=5.0, d3_params=tables,
                     neighbor_matrix=torch.zeros((0, 4), dtype=torch.int32))
    assert e.shape == (1,) and f.shape == (0, 3) and e.dtype == torch.float32 and float(e) == 0.0
    e, f, v = dftd3_atm(torch.zeros((0, 3)), torch.zeros(0, dtype=torch.int32), a1=0.4, a2=4.0, three_body_cutoff=5.0, d3_params=tables,
                        neighbor_matrix=torch.zeros((0, 4), dtype=torch.int32), neighbor_matrix_shifts=torch.zeros((0, 4, 3), dtype=torch.int32),
                        cell=torch.eye(3)[None], compute_virial=True)
    assert v.shape == (0, 3, 3)
    with pytest.raises(C.NativeLibraryError, match="no CPU path"):
        dftd3_atm(pos, z, a1=0.4, a2=4.0, three_body_cutoff=5.0, d3_params=tables, neighbor_matrix=nm)


def test_abi_declares_and_exports_the_three_body_entry_points():
    from nvalchemiops import _capi as C
    from tools.abi_symbols import declared_symbols

    want = {"mi_d3_atm", "mi_d3_atm_workspace_bytes", "mi_d3_atm_visits_offset", "mi_d3_atm_tile"}
    assert want <= set(declared_symbols())
    if not os.path.exists(C._LIB_PATH):
        pytest.fail("libnvalchemiops_hip.so is not built: run build() first")
    lib = C.lib()
    assert all(hasattr(lib, s) for s in want)
    assert lib.mi_d3_atm_tile() >= 64
    base, atm = lib.mi_d3_workspace_bytes(1000, 2, 18), lib.mi_d3_atm_workspace_bytes(1000, 2, 18)
    off = lib.mi_d3_atm_visits_offset(1000, 2, 18)
    assert atm >= base + 8000 and base <= off <= atm - 4000
    assert lib.mi_d3_atm_workspace_bytes(-1, 1, 18) == 0


def test_custom_ops_are_registered():
    import nvalchemiops  # noqa: F401

    for name in ("dftd3_atm_nm", "dftd3_atm_nl"):
        op = getattr(torch.ops.nvalchemiops, name)
        schema = str(op.default._schema)
        assert "Tensor(a" in schema and "energy" in schema and "three_body_cutoff" in schema  # mutation-annotated outputs
