"""Host-side contract of the dispersion PME: argument errors before any launch, no CPU path, the ABI symbols and the public names."""
import inspect
import os

import pytest
import torch

CELL = torch.tensor([[9.0, 0, 0], [1.1, 8.6, 0], [0.5, -0.8, 9.3]], dtype=torch.float64)
POS = torch.rand(5, 3, generator=torch.Generator().manual_seed(2), dtype=torch.float64) @ CELL
COEF = torch.ones(5, dtype=torch.float64)
NM = torch.full((5, 1), -1, dtype=torch.int32)


def _both():
    from nvalchemiops.interactions.vdw import pme_dispersion_correction, pme_dispersion_reciprocal_space

    return (pme_dispersion_reciprocal_space, {}), (pme_dispersion_correction, dict(neighbor_matrix=NM))


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("change,message", [
    (dict(cell=None), "cell is required"),
    (dict(alpha=None), "alpha is required"),
    (dict(mesh_dimensions=None), "Either mesh_dimensions or mesh_spacing"),
    (dict(spline_order=3), "spline_order must be 4, 5 or 6"),
    (dict(spline_order=7), "spline_order must be 4, 5 or 6"),
    (dict(mesh_dimensions=(12, 4, 12)), "at least the spline order 5"),
    (dict(mesh_dimensions=(12, 12)), "three integers"),
    (dict(coefficients=torch.ones(4, dtype=torch.float64)), "one entry per atom"),
])
def test_argument_errors(which, change, message):
    fn, lists = _both()[which]
    kw = dict(positions=POS, coefficients=COEF, cell=CELL, alpha=0.35, mesh_dimensions=(12, 12, 12), **lists)
    kw.update(change)
    with pytest.raises(ValueError, match=message):
        fn(kw.pop("positions"), kw.pop("coefficients"), kw.pop("cell"), kw.pop("alpha"), **kw)


@pytest.mark.parametrize("which", [0, 1])
def test_cpu_tensors_raise_and_no_atoms_return_zeros(which):
    from nvalchemiops._capi import NativeLibraryError

    fn, lists = _both()[which]
    with pytest.raises(NativeLibraryError, match="no CPU path"):
        fn(POS, COEF, CELL, 0.35, mesh_dimensions=(12, 12, 12), **lists)
    if lists:
        lists = dict(neighbor_matrix=NM[:0], neighbor_matrix_shifts=torch.zeros((0, 1, 3), dtype=torch.int32))
    e, f, cg, vir = fn(POS[:0], COEF[:0], CELL, 0.35, mesh_spacing=0.8, compute_forces=True, compute_coefficient_gradients=True,
                       compute_virial=True, **lists)
    assert (e.shape, f.shape, cg.shape, vir.shape) == ((0,), (0, 3), (0,), (1, 3, 3)) and not vir.any()


def test_symbols_names_and_defaults():
    import nvalchemiops.interactions as I
    from nvalchemiops import _capi as C
    from nvalchemiops.interactions import vdw
    from nvalchemiops.interactions.vdw import pme
    from tools.abi_symbols import declared_symbols

    want = {"mi_pme_dispersion_convolve", "mi_pme_dispersion_gather", "mi_pme_dispersion_virial_blocks"}
    assert want <= set(declared_symbols())
    if not os.path.exists(C._LIB_PATH):
        pytest.fail("libnvalchemiops_hip.so is not built: run build() first")
    assert all(hasattr(C.lib(), s) for s in want)
    assert 1 <= C.lib().mi_pme_dispersion_virial_blocks() <= 1024
    for name in ("pme_dispersion_reciprocal_space", "pme_dispersion_correction"):
        assert name in pme.__all__ and name in vdw.__all__ and name in I.__all__ and getattr(I, name) is getattr(pme, name)
        d = {k: v.default for k, v in inspect.signature(getattr(pme, name)).parameters.items()}
        assert d["alpha"] is inspect.Parameter.empty and d["spline_order"] == 5 and d["mesh_dimensions"] is None and d["mesh_spacing"] is None
        assert [k for k in d if k.startswith("compute_")] == ["compute_forces", "compute_coefficient_gradients", "compute_virial"]
        assert not any(d[k] for k in d if k.startswith("compute_"))
