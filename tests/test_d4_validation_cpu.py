"""`dftd4` / `D4Parameters` without a GPU: exports, table validation, list and argument errors (`dftd3`'s messages), and the refusal to
compute on CPU tensors."""
import numpy as np
import pytest
import torch

from tests import d4_reference as R


def _params(**override):
    from nvalchemiops.interactions.dispersion import D4Parameters

    t = {k: torch.as_tensor(v) for k, v in R.d4_test_tables(9).items()}
    t.update(override)
    return D4Parameters(**t)


def _call(**kw):
    from nvalchemiops.interactions.dispersion import dftd4

    n = 4
    args = dict(positions=torch.zeros((n, 3)), numbers=torch.ones(n, dtype=torch.int32), charges=torch.zeros(n), a1=0.4, a2=4.0, s8=0.8,
                d4_params=_params(), neighbor_matrix=torch.full((n, 3), n, dtype=torch.int32))
    args.update(kw)
    return dftd4(**args)


def test_exports():
    import nvalchemiops.interactions.dispersion as D
    from nvalchemiops import _capi
    from nvalchemiops.interactions.dispersion.dftd4 import D4Parameters, dftd4, species_slots

    assert "dftd4" in D.__all__ and "D4Parameters" in D.__all__ and D.dftd4 is dftd4 and D.D4Parameters is D4Parameters
    assert {"dftd3", "dftd3_atm", "dftd3_zero", "dftd3_zero_atm", "D3Parameters"} <= set(D.__all__)
    lib = _capi.lib()
    assert species_slots() == lib.mi_d4_species_slots() >= 1
    assert lib.mi_d4_fold_blocks() == 64  # tests/test_fold_sizes_gpu.py sizes its systems by it, beside mi_qeq_blocks / mi_gaussian_charges_blocks
    assert lib.mi_d4_workspace_bytes(1000, 2, 20) > lib.mi_d4_workspace_bytes(10, 2, 20) > 0 and lib.mi_d4_workspace_bytes(-1, 1, 20) == 0
    assert hasattr(torch.ops.nvalchemiops, "dftd4_nm") and hasattr(torch.ops.nvalchemiops, "dftd4_nl")


def test_parameters_container():
    p = _params()
    assert p.max_z == 9 and p.device == torch.device("cpu")
    p64 = p.to(dtype=torch.float64)
    assert p64.c6_ref.dtype == torch.float64 and p64.cn_ref.dtype == torch.float64 and p64.n_ref.dtype == torch.int32 and p64.ngw.dtype == torch.int32
    assert _params(n_ref=p.n_ref.long()).n_ref.dtype == torch.int64
    with pytest.raises(TypeError, match="must be a torch.Tensor"):
        _params(en=np.zeros(10, np.float32))
    with pytest.raises(TypeError, match="float32 or float64"):
        _params(gam=torch.zeros(10, dtype=torch.float16))
    with pytest.raises(TypeError, match="int32 or int64"):
        _params(n_ref=torch.ones(10))
    with pytest.raises(ValueError, match="rcov must be 1D"):
        _params(rcov=torch.zeros((10, 1)))
    with pytest.raises(ValueError, match="at least 2 elements"):
        _params(rcov=torch.zeros(1))
    for name in ("en", "r4r2", "zeff", "gam"):
        with pytest.raises(ValueError, match=f"{name} must have shape"):
            _params(**{name: torch.zeros(9)})
    with pytest.raises(ValueError, match="n_ref must have shape"):
        _params(n_ref=torch.ones(9, dtype=torch.int32))
    for name in ("cn_ref", "q_ref"):
        with pytest.raises(ValueError, match=f"{name} must have shape"):
            _params(**{name: torch.zeros((10, 5))})
    with pytest.raises(ValueError, match="ngw must have shape"):
        _params(ngw=torch.ones((10, 5), dtype=torch.int32))
    with pytest.raises(ValueError, match="c6_ref must have shape"):
        _params(c6_ref=torch.zeros((10, 10, 5, 5)))
    with pytest.raises(ValueError, match="same device"):
        _params(en=torch.zeros(10, device="meta"))


def test_list_and_argument_errors_are_dftd3s():
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
    with pytest.raises(ValueError, match="a1, a2, and s8 must be provided"):
        _call(s8=None)
    with pytest.raises(RuntimeError, match="DFT-D4 parameters must be explicitly provided"):
        _call(d4_params=None)
    with pytest.raises(ValueError, match="Must provide either"):  # the list checks come first, as in dftd3
        _call(d4_params=None, neighbor_matrix=None)
    with pytest.raises(ValueError, match=r"neighbor_matrix must have shape \[4, max_neighbors\]"):
        _call(neighbor_matrix=torch.full((3, 3), n, dtype=torch.int32))
    with pytest.raises(ValueError, match="numbers must have one entry per atom"):
        _call(numbers=torch.ones(3, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"charges must have one entry per atom: expected shape \[4\]"):
        _call(charges=torch.zeros(5))
    with pytest.raises(ValueError, match="charges must have one entry per atom"):
        _call(charges=torch.zeros((4, 1)))
    with pytest.raises(TypeError, match="charges must be float32 or float64"):
        _call(charges=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(KeyError):
        _call(d4_params={"rcov": torch.zeros(10)})


def test_cpu_tensors_raise_native_library_error_and_empty_input_returns_zeros():
    from nvalchemiops._capi import NativeLibraryError

    with pytest.raises(NativeLibraryError, match="no CPU path"):
        _call()
    out = _call(positions=torch.zeros((0, 3)), numbers=torch.zeros(0, dtype=torch.int32), charges=torch.zeros(0),
                neighbor_matrix=torch.zeros((0, 3), dtype=torch.int32))
    assert len(out) == 4 and out[0].shape == (1,) and out[1].shape == (0, 3) and out[2].shape == (0,) and out[3].shape == (0,)
    assert all(o.dtype == torch.float32 for o in out) and float(out[0]) == 0.0
