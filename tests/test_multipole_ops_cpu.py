"""The eighteen custom ops of the nine point-multipole operator halves under FakeTensorMode: output shapes with every flag on, the (0,)
placeholders with every flag off, the positions dtype, and float64 gradients in the shapes of the differentiable inputs from the backward
ops.  7 atoms in 2 systems; the cluster and Thole ops also without a cell (1 system).  The expectations below are written out per op and do
not read the table the ops are built from."""
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

N, B, K, W = 7, 2, 5, 6
PER_ATOM = {"positions": (3,), "charges": (), "dipoles": (3,), "quadrupoles": (3, 3), "polarizability": ()}
DP, QD, TH = ("positions", "charges", "dipoles"), ("positions", "charges", "dipoles", "quadrupoles"), ("positions", "charges", "dipoles",
                                                                                                         "polarizability")
LISTS = ("batch_idx", "neighbor_list", "neighbor_ptr", "neighbor_shifts", "neighbor_matrix", "neighbor_matrix_shifts", "mask_value")
MESH = ("cell", "alpha", "batch_idx", "nx", "ny", "nz", "spline_order")
KSUM = ("cell", "k_vectors", "alpha", "batch_idx")
# op: (differentiable inputs, the arguments after them, the extra output's per-atom shape | None, may the cell be None)
OPS = {
    "ewald_dipole_real_space": (DP, ("cell", "alpha") + LISTS, None, False),
    "ewald_dipole_reciprocal_space": (DP, KSUM, None, False),
    "pme_dipole_reciprocal_space": (DP, MESH, None, False),
    "thole_dipole_correction": (TH, ("cell",) + LISTS + ("thole",), (), True),
    "ewald_quadrupole_real_space": (QD, ("cell", "alpha") + LISTS, (3, 3), False),
    "ewald_quadrupole_reciprocal_space": (QD, KSUM, (3, 3), False),
    "pme_quadrupole_reciprocal_space": (QD, MESH, (3, 3), False),
    "coulomb_dipole_correction": (DP, ("cell",) + LISTS, None, True),
    "coulomb_quadrupole_correction": (QD, ("cell",) + LISTS, (3, 3), True),
}


def _value(name, dtype, with_cell):
    i32 = torch.int32
    if name in PER_ATOM:
        return torch.empty((N,) + PER_ATOM[name], dtype=dtype)
    return {"cell": torch.empty((B, 3, 3), dtype=dtype) if with_cell else None, "alpha": torch.empty(B, dtype=dtype),
            "k_vectors": torch.empty((B, K, 3), dtype=dtype), "batch_idx": torch.empty(N, dtype=i32) if with_cell else None,
            "neighbor_list": None, "neighbor_ptr": None, "neighbor_shifts": None, "neighbor_matrix": torch.empty((N, W), dtype=i32),
            "neighbor_matrix_shifts": torch.empty((N, W, 3), dtype=i32) if with_cell else None, "mask_value": N + 3, "thole": 0.39,
            "nx": 8, "ny": 10, "nz": 12, "spline_order": 5}[name]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", sorted(OPS))
def test_multipole_ops_under_fake_tensors(name, dtype):
    import nvalchemiops  # noqa: F401
    from nvalchemiops import _eops  # noqa: F401  (registers the ops)

    diff, rest, extra, cell_optional = OPS[name]
    forward, backward = getattr(torch.ops.alchemiops, f"_{name}"), getattr(torch.ops.nvalchemiops, f"{name}_backward")
    per_atom = [(), (3,), (), (3,)] + ([extra] if extra is not None else [])
    for with_cell in (True, False) if cell_optional else (True,):
        nsys = B if with_cell else 1
        with FakeTensorMode():
            args = [_value(a, dtype, with_cell) for a in diff + rest]
            on = forward(*args, *[True] * len(per_atom))
            off = forward(*args, *[False] * len(per_atom))
            grads = backward(*args, torch.empty(N, dtype=dtype))
        assert [tuple(o.shape) for o in on] == [(N,) + s for s in per_atom] + [(nsys, 3, 3)], (name, with_cell)
        assert [tuple(o.shape) for o in off] == [(N,)] + [(0,)] * len(per_atom), (name, with_cell)
        assert all(o.dtype == dtype for o in on + off), (name, with_cell)
        assert [tuple(g.shape) for g in grads] == [(N,) + PER_ATOM[d] for d in diff] and all(g.dtype == torch.float64 for g in grads), name
