"""What the pair-sum operators over a FULL neighbour list (`gaussian_charge_correction`, the point-dipole sums, `charge_equilibration`) share
on the Python side: list checks, launch tensors, the flag word of their kernels, the eager / op dispatch test and the selection of outputs.
The device-side counterpart is csrc/pair_row.h; the dispersion operators have theirs in dispersion/_call.py."""
from __future__ import annotations

import torch

from nvalchemiops import _capi as C

# MI_GC_* / MI_DP_* / MI_QD_*: the third gradient is dE/dsigma or dE/dmu, the fourth dE/dQ (MI_QD_QUADRUPOLE_GRAD) or dE/da (MI_DP_POLAR_GRAD)
FORCES, CHARGE_GRAD, THIRD_GRAD, VIRIAL, FOURTH_GRAD = 1, 2, 4, 8, 16


def check_lists(positions, charges, sigma, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, batch_idx,
                compute_virial):
    """Every argument error, before anything is launched: `ewald_real_space`'s messages for the same misuse, plus sigma and the cell-less rules."""
    if neighbor_list is None and neighbor_matrix is None:
        raise ValueError("Either neighbor_list or neighbor_matrix must be provided")
    if neighbor_list is not None and neighbor_ptr is None:
        raise ValueError("neighbor_ptr is required when using neighbor_list format")
    C.dtype_code(positions.dtype)
    if cell is None:
        if neighbor_shifts is not None or neighbor_matrix_shifts is not None:
            raise ValueError("neighbor shifts need a cell: pass cell, or a list without shifts for a non-periodic system")
        if compute_virial:
            raise ValueError("compute_virial needs a cell")
    C.check_neighbor_data(positions.shape[0], neighbor_matrix=neighbor_matrix, neighbor_matrix_shifts=neighbor_matrix_shifts,
                          neighbor_list=neighbor_list, neighbor_ptr=neighbor_ptr, neighbor_shifts=neighbor_shifts, cell=cell,
                          charges=charges, batch_idx=batch_idx)
    if isinstance(sigma, torch.Tensor) and sigma.dim() > 0:
        C.check_per_atom(positions.shape[0], sigma=sigma)
        if sigma.dim() != 1:
            raise ValueError(f"sigma must have one entry per atom: expected shape [{positions.shape[0]}], got {tuple(sigma.shape)}")


def check_dipoles(positions, dipoles):
    n = positions.shape[0]
    if dipoles.dim() != 2 or tuple(dipoles.shape) != (n, 3):
        raise ValueError(f"dipoles must have one vector per atom: expected shape [{n}, 3], got {tuple(dipoles.shape)}")


def check_dipole_lists(positions, charges, dipoles, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts,
                       batch_idx, alpha, compute_virial):
    """`check_lists` for the real-space dipole term, plus the dipole shape, the required cell and the shifts a virial needs."""
    if cell is None:
        raise ValueError("cell is required: the point-dipole Ewald sum is periodic (cell=None clusters are out of scope)")
    check_lists(positions, charges, 0.0, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, batch_idx,
                compute_virial)
    check_dipoles(positions, dipoles)
    if compute_virial and (neighbor_shifts if neighbor_list is not None else neighbor_matrix_shifts) is None:
        raise ValueError("compute_virial needs the shifts of the list: pass neighbor_shifts with neighbor_list, neighbor_matrix_shifts with neighbor_matrix")
    n_cells = cell.shape[0] if cell.dim() == 3 else 1
    if isinstance(alpha, torch.Tensor) and alpha.numel() > 1 and alpha.numel() != n_cells:
        raise ValueError(f"alpha has {alpha.numel()} values but there are {n_cells} systems")


def num_systems(cell, batch_idx) -> int:
    return cell.reshape(-1, 3, 3).shape[0] if batch_idx is not None else 1


def list_inputs(neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts) -> dict:
    """A CSR list or a matrix as launched: int32 `idx`, `nptr` (None: matrix), row width `m` (0: list), int32 `sh` | None, slots `n_entries`."""
    if neighbor_list is not None:
        idx, nptr, m, sh = C.i32(neighbor_list[1]), C.i32(neighbor_ptr), 0, neighbor_shifts
    else:
        idx, nptr, m, sh = C.i32(neighbor_matrix), None, neighbor_matrix.shape[1], neighbor_matrix_shifts
    return dict(idx=idx, nptr=nptr, m=m, sh=None if sh is None else C.i32(sh), n_entries=idx.numel())


def launch_inputs(positions, charges, cell, batch_idx, lists, mask=None, **per_atom):
    """Detached, contiguous launch tensors in the positions dtype (device check included; shapes were checked before): `list_inputs(*lists)`
    plus pos, q, cells | None, bi | None (int32, only with a cell), nsys, the caller's own arrays under their keywords, and `mask`, the
    list's padding value as the operators that keep it in this dict pass it."""
    dt = positions.dtype
    C.require_device(positions, charges, *per_atom.values(), cell, *lists, batch_idx)
    conv = lambda t: t.detach().to(dt).contiguous()  # noqa: E731
    cells = None if cell is None else conv(cell.reshape(-1, 3, 3))
    batched = batch_idx is not None and cells is not None
    return dict(pos=positions.detach().contiguous(), q=conv(charges), cells=cells, bi=C.i32(batch_idx) if batched else None,
                nsys=cells.shape[0] if batched else 1, mask=mask, **{k: conv(v) for k, v in per_atom.items()}, **list_inputs(*lists))


def flag_bits(want) -> int:
    """The flag word of a pair kernel for `want` = (energies, forces, charge gradient, third gradient[, fourth gradient], virial)."""
    bits = (FORCES if want[1] else 0) | (CHARGE_GRAD if want[2] else 0) | (THIRD_GRAD if want[3] else 0) | (VIRIAL if want[-1] else 0)
    return bits | FOURTH_GRAD if len(want) == 6 and want[4] else bits


def needs_op(*tensors) -> bool:
    """True when the call has to go through its `alchemiops::` op: under torch.compile, or when autograd has to record it."""
    return C.tracing() or (torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors))


def zeros(n, nsys, dt, dev, *grads):
    """All outputs of an operator as zeros: energies, forces, one gradient per per-atom shape in `grads` (() charges or sigma, (3,) dipoles,
    (3, 3) quadrupoles), virial."""
    z = lambda *shape: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    return (z(n), z(n, 3)) + tuple(z(n, *s) for s in grads) + (z(nsys, 3, 3),)


def select(res, want):
    """The items of `res` that were asked for: a tuple, or the energies alone."""
    out = tuple(r for r, w in zip(res, want) if w)
    return out if len(out) > 1 else out[0]
