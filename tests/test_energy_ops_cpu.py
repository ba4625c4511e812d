"""The twenty-six custom ops of the thirteen energy op pairs outside tests/test_multipole_ops_cpu.py under FakeTensorMode: output shapes
with every flag on (the virial is [nsys, 3, 3]), the (0,) placeholders with every flag off, the positions dtype, and float64 gradients in
the shapes of the differentiable inputs from the backward ops.  7 atoms in 2 systems; the ops whose cell is optional also without one
(1 system).  The valence ops get a [5, 3] parameter table, so their parameter gradients cannot pass for a per-atom shape.  The Gaussian
backward op also returns the cell gradient: [2, 3, 3] with a cell, [0] without.  The expectations below are written out per op and do not
read the table the ops are built from."""
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

N, B, K, W, T = 7, 2, 5, 6, 5
LISTS = ("batch_idx", "neighbor_list", "neighbor_ptr", "neighbor_shifts", "neighbor_matrix", "neighbor_matrix_shifts", "mask_value")
VDW = (("positions", "radii", "epsilons"), ("cell", "batch_idx", "parent", "reduction", "child_ptr", "child_idx", "pair_scales") + LISTS[1:]
       + ("cutoff", "taper", "delta", "gamma", "radius_rule", "epsilon_rule"), [(N,), (N, 3), (N,), (N,)], [(N, 3), (N,), (N,)], True)
VALENCE = (("positions", "parameters"), ("cell", "batch_idx", "atoms", "slot_ptr", "slot_idx", "cubic", "quartic", "pentic", "sextic", "plane"),
           [(N,), (N, 3), (T, 3)], [(N, 3), (T, 3)], True)
DISPERSION = ([(N,), (N, 3), (N,)], [(N, 3), (N,)], False)
# op: (differentiable inputs, the arguments after them, output shapes before the virial with every flag on, gradient shapes of the backward
# op with a cell, may the cell be None)
OPS = {
    "gaussian_charge_correction": (("positions", "charges", "sigma", "cell"), LISTS + ("self_energy", "neutralizing_background"),
                                   [(N,), (N, 3), (N,), (N,)], [(N, 3), (N,), (N,), (B, 3, 3)], True),
    "pair_scale_correction": (("positions", "charges", "dipoles", "quadrupoles"), ("pair_scales", "cell") + LISTS + ("minimum_image",),
                              [(N,), (N, 3), (N,), (N, 3), (N, 3, 3)], [(N, 3), (N,), (N, 3), (N, 3, 3)], True),
    "dipole_pair_scale_correction": (("positions", "charges", "dipoles", "polarizability"),
                                     ("direct_scales", "mutual_scales", "cell") + LISTS + ("minimum_image", "thole"),
                                     [(N,), (N, 3), (N,), (N, 3), (N,)], [(N, 3), (N,), (N, 3), (N,)], True),
    "buffered_14_7": VDW,
    "lennard_jones": VDW,
    "bond_stretch": VALENCE,
    "angle_bend": VALENCE,
    "stretch_bend": VALENCE,
    "out_of_plane_bend": VALENCE,
    "torsion": VALENCE,
    "ewald_dispersion_real_space": (("positions", "coefficients"), ("cell", "alpha") + LISTS + ("counted_cutoff", "counted_taper")) + DISPERSION,
    "ewald_dispersion_reciprocal_space": (("positions", "coefficients"), ("cell", "k_vectors", "alpha", "batch_idx")) + DISPERSION,
    "pme_dispersion_reciprocal_space": (("positions", "coefficients"), ("cell", "alpha", "batch_idx", "nx", "ny", "nz", "order")) + DISPERSION,
}
PER_ATOM = {"positions": (3,), "charges": (), "sigma": (), "dipoles": (3,), "quadrupoles": (3, 3), "polarizability": (), "radii": (),
            "epsilons": (), "coefficients": ()}


def _value(name, dtype, with_cell):
    i32 = torch.int32
    if name in PER_ATOM:
        return torch.empty((N,) + PER_ATOM[name], dtype=dtype)
    return {"cell": torch.empty((B, 3, 3), dtype=dtype) if with_cell else None, "alpha": torch.empty(B, dtype=dtype),
            "k_vectors": torch.empty((B, K, 3), dtype=dtype), "batch_idx": torch.empty(N, dtype=i32) if with_cell else None,
            "neighbor_list": None, "neighbor_ptr": None, "neighbor_shifts": None, "neighbor_matrix": torch.empty((N, W), dtype=i32),
            "neighbor_matrix_shifts": torch.empty((N, W, 3), dtype=i32) if with_cell else None, "mask_value": N + 3, "thole": 0.39,
            "nx": 8, "ny": 10, "nz": 12, "order": 5, "self_energy": True, "neutralizing_background": with_cell, "minimum_image": with_cell,
            "pair_scales": torch.empty((N, W), dtype=dtype), "direct_scales": torch.empty((N, W), dtype=dtype), "mutual_scales": None,
            "parent": torch.empty(N, dtype=i32), "reduction": torch.empty(N, dtype=dtype), "child_ptr": torch.empty(N + 1, dtype=i32),
            "child_idx": torch.empty(N, dtype=i32), "cutoff": 9.0, "taper": 8.1, "delta": 0.07, "gamma": 0.12, "radius_rule": 2,
            "epsilon_rule": 3, "parameters": torch.empty((T, 3), dtype=dtype), "atoms": torch.empty((T, 3), dtype=i32),
            "slot_ptr": torch.empty(N + 1, dtype=i32), "slot_idx": torch.empty(3 * T, dtype=i32), "cubic": -0.014, "quartic": 5.6e-5,
            "pentic": -7.0e-7, "sextic": 2.2e-8, "plane": 1, "counted_cutoff": 9.0, "counted_taper": -1.0}[name]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", sorted(OPS))
def test_energy_ops_under_fake_tensors(name, dtype):
    import nvalchemiops  # noqa: F401
    from nvalchemiops import _eops  # noqa: F401  (registers the ops)

    diff, rest, shapes, grad_shapes, cell_optional = OPS[name]
    forward, backward = getattr(torch.ops.alchemiops, f"_{name}"), getattr(torch.ops.nvalchemiops, f"{name}_backward")
    n_flags = len(shapes)  # one per output after the energies, the virial's last
    for with_cell in (True, False) if cell_optional else (True,):
        nsys = B if with_cell else 1
        with FakeTensorMode():
            args = [_value(a, dtype, with_cell) for a in diff + rest]
            on = forward(*args, *[True] * n_flags)
            off = forward(*args, *[False] * n_flags)
            grads = backward(*args, torch.empty(N, dtype=dtype))
        assert [tuple(o.shape) for o in on] == shapes + [(nsys, 3, 3)], (name, with_cell)
        assert [tuple(o.shape) for o in off] == [(N,)] + [(0,)] * n_flags, (name, with_cell)
        assert all(o.dtype == dtype for o in on + off), (name, with_cell)
        want = [(0,) if (d == "cell" and not with_cell) else s for d, s in zip(diff, grad_shapes)]
        assert [tuple(g.shape) for g in grads] == want and all(g.dtype == torch.float64 for g in grads), (name, with_cell)
