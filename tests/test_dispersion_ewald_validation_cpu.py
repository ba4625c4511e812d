"""`ewald_dispersion_real_space`, `ewald_dispersion_reciprocal_space` and `ewald_dispersion_correction`: what can be checked without a GPU --
every argument error of `_check_common`, `_check_counted`, the `k_vectors` shape check and "one of k_vectors / k_cutoff" by message (all
raised before anything is launched), the `compute_virial` rule of the real half, the returns for N = 0 with their shapes and dtypes, and
the absence of a CPU path."""
import pytest
import torch

from nvalchemiops import _capi as C
from nvalchemiops.interactions import ewald_dispersion_correction, ewald_dispersion_real_space, ewald_dispersion_reciprocal_space

I32 = torch.int32
FLAGS = dict(compute_forces=True, compute_coefficient_gradients=True, compute_virial=True)


def _args(n=4, m=6):
    """positions, coefficients, cell, and a matrix with one pair and its shifts."""
    nm = torch.full((n, m), n, dtype=I32)
    nm[0, 0], nm[1, 0] = 1, 0
    return torch.rand(n, 3), torch.rand(n) + 1, torch.eye(3)[None] * 10, nm, torch.zeros((n, m, 3), dtype=I32)


def _each(pos, c, cell, alpha, lists, **kw):
    """The three entry points on the same arguments (the reciprocal half without the lists)."""
    kv = torch.zeros((5, 3))
    return [lambda: ewald_dispersion_real_space(pos, c, cell, alpha, **lists, **kw),
            lambda: ewald_dispersion_reciprocal_space(pos, c, cell, kv, alpha, **kw),
            lambda: ewald_dispersion_correction(pos, c, cell, alpha, k_vectors=kv, **lists, **kw)]


def test_common_errors_of_all_three():
    pos, c, cell, nm, sh = _args()
    lists = dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    cases = [((pos, c, None, 0.3), {}, "cell is required: the dispersion Ewald sum is periodic"),
             ((pos[:, :2], c, cell, 0.3), {}, r"positions must have shape \[num_atoms, 3\]"),
             ((pos, c[:3], cell, 0.3), {}, r"coefficients must have one entry per atom: expected shape \[4\]"),
             ((pos, c[:, None], cell, 0.3), {}, r"coefficients must have one entry per atom: expected shape \[4\]"),
             ((pos, 2.0, cell, 0.3), {}, r"coefficients must have one entry per atom: expected shape \[4\]"),
             ((pos, c, cell, 0.3), dict(batch_idx=torch.zeros(3, dtype=I32)), "batch_idx must have one entry per atom"),
             ((pos, c, torch.eye(3)[:2], 0.3), {}, r"cell must have shape \[3, 3\] or \[num_systems, 3, 3\]"),
             ((pos, c, cell, None), {}, "alpha is required: the Coulomb accuracy estimate does not transfer"),
             ((pos, c, cell, torch.tensor([0.3, 0.4])), {}, "alpha has 2 values but there are 1 systems")]
    for atoms, kw, message in cases:
        for call in _each(*atoms, lists, **kw):
            with pytest.raises(ValueError, match=message):
                call()
    with pytest.raises(ValueError, match="Unsupported dtype"):
        ewald_dispersion_reciprocal_space(pos.half(), c, cell, torch.zeros((5, 3)), 0.3)


def test_counted_errors():
    pos, c, cell, nm, sh = _args()
    lists = dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh)
    for fn, extra in ((ewald_dispersion_real_space, {}), (ewald_dispersion_correction, dict(k_cutoff=1.0))):
        with pytest.raises(ValueError, match="counted_taper needs counted_cutoff"):
            fn(pos, c, cell, 0.3, **lists, **extra, counted_taper=3.6)
        for rc in (0.0, -4.0, float("nan")):
            with pytest.raises(ValueError, match="counted_cutoff must be positive"):
                fn(pos, c, cell, 0.3, **lists, **extra, counted_cutoff=rc)
        for rt in (0.0, 4.0, 4.5, -1.0):
            with pytest.raises(ValueError, match=r"counted_taper must lie inside \(0, counted_cutoff = 4.0\)"):
                fn(pos, c, cell, 0.3, **lists, **extra, counted_cutoff=4.0, counted_taper=rt)


def test_k_vector_errors():
    pos, c, cell, nm, sh = _args()
    cells = cell.repeat(2, 1, 1)
    bi = torch.tensor([0, 0, 1, 1], dtype=I32)
    for bad in (torch.zeros((5, 2)), torch.zeros(3), torch.zeros((1, 1, 5, 3)), torch.zeros((3, 5, 3))):
        with pytest.raises(ValueError, match=r"k_vectors must have shape \[K, 3\] or \[2, K, 3\]"):
            ewald_dispersion_reciprocal_space(pos, c, cells, bad, 0.3, batch_idx=bi)
    with pytest.raises(ValueError, match=r"k_vectors must have shape \[K, 3\] or \[1, K, 3\]"):
        ewald_dispersion_reciprocal_space(pos, c, cell, torch.zeros((2, 5, 3)), 0.3)
    with pytest.raises(ValueError, match="one of k_vectors / k_cutoff is required"):
        ewald_dispersion_correction(pos, c, cell, 0.3, neighbor_matrix=nm, neighbor_matrix_shifts=sh)


def test_list_errors_and_the_virial_rule_of_the_real_half():
    pos, c, cell, nm, sh = _args()
    lst, ptr = torch.zeros((2, 3), dtype=I32), torch.zeros(5, dtype=I32)
    for fn, extra in ((ewald_dispersion_real_space, {}), (ewald_dispersion_correction, dict(k_cutoff=1.0))):
        with pytest.raises(ValueError, match="Either neighbor_list or neighbor_matrix must be provided"):
            fn(pos, c, cell, 0.3, **extra)
        with pytest.raises(ValueError, match="neighbor_ptr is required"):
            fn(pos, c, cell, 0.3, neighbor_list=lst, **extra)
        with pytest.raises(ValueError, match="compute_virial needs the shifts of the list"):
            fn(pos, c, cell, 0.3, neighbor_matrix=nm, compute_virial=True, **extra)
        with pytest.raises(ValueError, match="compute_virial needs the shifts of the list"):
            fn(pos, c, cell, 0.3, neighbor_list=lst, neighbor_ptr=ptr, compute_virial=True, **extra)
        with pytest.raises(ValueError, match=r"neighbor_matrix_shifts must have shape \[4, 6, 3\]"):
            fn(pos, c, cell, 0.3, neighbor_matrix=nm, neighbor_matrix_shifts=sh[:, :5], **extra)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_no_atoms_return_zeros_of_the_documented_shapes(dtype):
    pos, c, cell, nm, sh = _args()
    cells = cell.repeat(2, 1, 1).to(dtype)
    empty = (pos[:0].to(dtype), c[:0].to(dtype), cells, torch.tensor([0.3, 0.4], dtype=dtype))
    lists = dict(neighbor_matrix=nm[:0], neighbor_matrix_shifts=sh[:0], batch_idx=torch.zeros(0, dtype=I32))
    for out in (ewald_dispersion_real_space(*empty, **lists, **FLAGS),
                ewald_dispersion_reciprocal_space(*empty[:3], torch.zeros((2, 5, 3), dtype=dtype), empty[3], batch_idx=lists["batch_idx"], **FLAGS),
                ewald_dispersion_correction(*empty, k_vectors=torch.zeros((5, 3), dtype=dtype), **lists, **FLAGS)):
        assert [tuple(o.shape) for o in out] == [(0,), (0, 3), (0,), (2, 3, 3)] and all(o.dtype == dtype and not o.any() for o in out)
    assert tuple(ewald_dispersion_real_space(*empty, **lists).shape) == (0,)
    assert tuple(ewald_dispersion_reciprocal_space(*empty[:3], None, 0.3, batch_idx=lists["batch_idx"]).shape) == (0,)


def test_cpu_tensors_raise_native_library_error():
    pos, c, cell, nm, sh = _args()
    for call in _each(pos, c, cell, 0.3, dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh)):
        with pytest.raises(C.NativeLibraryError):
            call()
    with pytest.raises(C.NativeLibraryError):  # without k-vectors too: the k = 0 and self terms are computed on the device
        ewald_dispersion_reciprocal_space(pos, c, cell, None, 0.3)
