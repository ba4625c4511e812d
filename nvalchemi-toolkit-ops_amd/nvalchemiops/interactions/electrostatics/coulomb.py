"""Cut-off Coulomb energies / forces -- drop-in for `coulomb_energy`, `coulomb_forces`, `coulomb_energy_forces`
(interactions/electrostatics/coulomb.py:1336-1691) and the eight `alchemiops::_[batch_]coulomb_*` ops behind them (:716-1330).

One HIP kernel family (csrc/ewald.hip, `mi_coulomb` / `mi_coulomb_bwd`) covers list / matrix x single / batch x energy / +forces.
As in the reference every input is upcast to float64 before the launch and the results are cast back to the positions dtype
(:1423-1426, :1489).  Forces follow the reference's scatter (+f on the row owner, -f on atom j), so full, half and asymmetric
lists all give the reference's numbers.  Energies AND explicit forces are differentiable w.r.t. positions, charges and cell through a hand-written
adjoint kernel (the reference records a Warp tape); when something requires grad, or under torch.compile, the call goes through the
registered `nvalchemiops::_[batch_]coulomb_*` ops (nvalchemiops/_eops.py), otherwise straight to the C ABI.

Reference behaviour kept on purpose: the energy-only MATRIX kernels use q_i q_j without the 1/2 that every other Coulomb kernel
applies (coulomb.py:340, :623 vs :192, :400), so `coulomb_energy(neighbor_matrix=...)` returns twice the energies that
`coulomb_energy_forces(neighbor_matrix=...)` returns on the same input.  Identical results are the bar here, so the quirk is
reproduced.
"""
from __future__ import annotations

import torch

from nvalchemiops import _capi as C


def _launch(pos, q, cells, bi, idx, sh, nptr, m, fill_value, cutoff, alpha, epref, want_forces):
    n = pos.shape[0]
    energies = torch.empty(n, dtype=torch.float64, device=pos.device)
    forces = torch.empty((n, 3), dtype=torch.float64, device=pos.device) if want_forces else None
    rc = C.lib().mi_coulomb(C.ptr(pos), C.ptr(q), C.ptr(cells), C.ptr(bi), n, C.ptr(idx), C.ptr(sh), C.ptr(nptr), int(m), int(fill_value),
                            C.cdouble(cutoff), C.cdouble(alpha), C.cdouble(epref), C.ptr(energies), C.ptr(forces), C.stream_of(pos))
    C.check(rc, "mi_coulomb")
    return energies, forces


def _adjoint(pos, q, cells, bi, idx, sh, nptr, m, fill_value, cutoff, alpha, epref, g_e):
    """(dL/dpositions, dL/dcharges, dL/dcell) of L = sum_i g_i E_i: the adjoint kernel `mi_coulomb_bwd` (the reference records a Warp tape)."""
    g = g_e.detach().to(torch.float64).contiguous()
    gpos, gq, gcell = torch.empty_like(pos), torch.empty_like(q), torch.empty_like(cells)
    rc = C.lib().mi_coulomb_bwd(C.ptr(pos), C.ptr(q), C.ptr(cells), C.ptr(bi), pos.shape[0], cells.shape[0], C.ptr(idx), C.ptr(sh), C.ptr(nptr),
                                int(m), int(fill_value), C.cdouble(cutoff), C.cdouble(alpha), C.cdouble(epref), C.ptr(g), C.ptr(gpos), C.ptr(gq),
                                C.ptr(gcell), C.stream_of(pos))
    C.check(rc, "mi_coulomb_bwd")
    return gpos, gq, gcell


def _force_adjoint(pos, q, cells, bi, idx, sh, nptr, m, fill_value, cutoff, alpha, g_f):
    """(dL/dpositions, dL/dcharges, dL/dcell) of L = sum_k g_k . F_k: `mi_coulomb_forces_bwd` (second derivatives of the pair term)."""
    g = g_f.detach().to(torch.float64).contiguous()
    gpos, gq, gcell = torch.empty_like(pos), torch.empty_like(q), torch.empty_like(cells)
    rc = C.lib().mi_coulomb_forces_bwd(C.ptr(pos), C.ptr(q), C.ptr(cells), C.ptr(bi), pos.shape[0], cells.shape[0], C.ptr(idx), C.ptr(sh), C.ptr(nptr),
                                       int(m), int(fill_value), C.cdouble(cutoff), C.cdouble(alpha), C.ptr(g), C.ptr(gpos), C.ptr(gq), C.ptr(gcell),
                                       C.stream_of(pos))
    C.check(rc, "mi_coulomb_forces_bwd")
    return gpos, gq, gcell


def _lists(n, dev, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, fill_value, want_forces, atoms):
    """(idx, shifts, row pointer | None, row width, fill value, energy prefactor) of either neighbour format.  Every launch of this module
    comes through here, so this is where `atoms` = (positions, charges, cell, batch_idx) and the neighbour data are checked: shapes
    first (`_capi.check_neighbor_data`; a neighbor_ptr SHORTER than N + 1 stays legal, see below), then the device."""
    positions, charges, cell, batch_idx = atoms
    C.check_neighbor_data(n, neighbor_matrix=neighbor_matrix, neighbor_matrix_shifts=neighbor_matrix_shifts, neighbor_list=neighbor_list,
                          neighbor_ptr=neighbor_ptr, neighbor_shifts=neighbor_shifts, short_ptr_ok=True, charges=charges, batch_idx=batch_idx)
    if n > 0:
        C.require_device(positions, charges, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, batch_idx)
    if neighbor_list is not None:
        idx, sh, nptr, m, fv = C.i32(neighbor_list[1]), C.i32(neighbor_shifts), C.i32(neighbor_ptr), 0, 0
        if nptr.numel() < n + 1:
            # the reference's own fixture passes a short neighbor_ptr (test_coulomb.py:50: 2 entries for 2 atoms) and reads past its
            # end; here the missing rows are defined as empty instead
            last = nptr[-1:] if nptr.numel() else torch.zeros(1, dtype=torch.int32, device=dev)
            nptr = torch.cat([nptr, last.expand(n + 1 - nptr.numel())]).contiguous()
        return idx, sh, nptr, m, fv, 0.5
    idx, sh, m = C.i32(neighbor_matrix), C.i32(neighbor_matrix_shifts), neighbor_matrix.shape[1]
    fv = n if fill_value is None else int(fill_value)
    return idx, sh, None, m, fv, (0.5 if want_forces else 1.0)  # coulomb.py:340 / :623 -- see the module docstring


def _forward(positions, charges, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts,
             fill_value, cutoff, alpha, want_forces):
    """float64 (energies, forces | None) of float64 inputs, no autograd graph: body of the eight `nvalchemiops::_[batch_]coulomb_*` ops
    (nvalchemiops/_eops.py) and of the plain eager call."""
    n, dev = positions.shape[0], positions.device
    idx, sh, nptr, m, fv, epref = _lists(n, dev, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, fill_value,
                                         want_forces, (positions, charges, cell, batch_idx))
    if n == 0 or idx.numel() == 0:
        return torch.zeros(n, dtype=torch.float64, device=dev), (torch.zeros((n, 3), dtype=torch.float64, device=dev) if want_forces else None)
    bi = None if batch_idx is None else C.i32(batch_idx)
    return _launch(positions.detach().contiguous(), charges.detach().contiguous(), cell.detach().reshape(-1, 3, 3).contiguous(), bi, idx, sh, nptr, m,
                   fv, float(cutoff), float(alpha), epref, want_forces)


def _backward(positions, charges, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts,
              fill_value, cutoff, alpha, want_forces, grad_energies):
    n, dev = positions.shape[0], positions.device
    idx, sh, nptr, m, fv, epref = _lists(n, dev, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, fill_value,
                                         want_forces, (positions, charges, cell, batch_idx))
    cells = cell.detach().reshape(-1, 3, 3).contiguous()
    if n == 0 or idx.numel() == 0:  # nothing stored: zero gradients, as the reference's tape gives (test_coulomb.py:964-996, :1954-2175)
        return torch.zeros((n, 3), dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros_like(cells)
    bi = None if batch_idx is None else C.i32(batch_idx)
    return _adjoint(positions.detach().contiguous(), charges.detach().contiguous(), cells, bi, idx, sh, nptr, m, fv, float(cutoff), float(alpha),
                    epref, grad_energies)


def _forces_backward(positions, charges, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts,
                     fill_value, cutoff, alpha, grad_forces):
    n, dev = positions.shape[0], positions.device
    idx, sh, nptr, m, fv, _ = _lists(n, dev, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, fill_value, True, (positions, charges, cell, batch_idx))
    cells = cell.detach().reshape(-1, 3, 3).contiguous()
    if n == 0 or idx.numel() == 0:
        return torch.zeros((n, 3), dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros_like(cells)
    bi = None if batch_idx is None else C.i32(batch_idx)
    return _force_adjoint(positions.detach().contiguous(), charges.detach().contiguous(), cells, bi, idx, sh, nptr, m, fv, float(cutoff), float(alpha),
                          grad_forces)


def _run(positions, charges, cell, cutoff, alpha, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts,
         fill_value, batch_idx, want_forces):
    use_list = neighbor_list is not None and neighbor_shifts is not None
    use_matrix = neighbor_matrix is not None and neighbor_matrix_shifts is not None
    if not use_list and not use_matrix:
        raise ValueError("Must provide either neighbor_list/neighbor_shifts or neighbor_matrix/neighbor_matrix_shifts")
    if use_list and use_matrix:
        raise ValueError("Cannot provide both neighbor list and neighbor matrix formats")
    if use_list and neighbor_ptr is None:
        raise ValueError("neighbor_ptr is required when using neighbor_list format")
    n = positions.shape[0]
    pos = positions.to(torch.float64)
    q = charges.to(torch.float64)
    cells = cell.to(torch.float64).reshape(-1, 3, 3)
    if C.tracing() or (torch.is_grad_enabled() and any(t.requires_grad for t in (pos, q, cells))):
        from nvalchemiops import _eops

        op = _eops.coulomb_op(batch_idx is not None, "list" if use_list else "matrix", want_forces)
        lists = (neighbor_list, neighbor_ptr, neighbor_shifts) if use_list else (neighbor_matrix, neighbor_matrix_shifts)
        tail = (float(cutoff), float(alpha)) + (() if use_list else (n if fill_value is None else int(fill_value),))
        out = op(pos, q, cells, *lists, *((batch_idx,) if batch_idx is not None else ()), *tail)
        return out if want_forces else (out, None)
    if not use_list:
        neighbor_list = neighbor_ptr = neighbor_shifts = None
    else:
        neighbor_matrix = neighbor_matrix_shifts = None
    return _forward(pos, q, cells, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, fill_value,
                    cutoff, alpha, want_forces)


@C.traceable
def coulomb_energy(positions: torch.Tensor, charges: torch.Tensor, cell: torch.Tensor, cutoff: float, alpha: float = 0.0,
                   neighbor_list: torch.Tensor | None = None, neighbor_ptr: torch.Tensor | None = None,
                   neighbor_shifts: torch.Tensor | None = None, neighbor_matrix: torch.Tensor | None = None,
                   neighbor_matrix_shifts: torch.Tensor | None = None, fill_value: int | None = None,
                   batch_idx: torch.Tensor | None = None) -> torch.Tensor:
    """Per-atom energies E_i = c sum_j q_i q_j phi(r_ij), phi = erfc(alpha r)/r (alpha > 0) or 1/r, over listed pairs with
    1e-10 <= r < cutoff; c = 1/2 for the list format and 1 for the matrix format (reference behaviour, see module docstring).
    Differentiable w.r.t. positions, charges and cell (coulomb.py:1336-1489)."""
    e, _ = _run(positions, charges, cell, cutoff, alpha, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts,
                fill_value, batch_idx, want_forces=False)
    return e.to(positions.dtype)


@C.traceable
def coulomb_energy_forces(positions: torch.Tensor, charges: torch.Tensor, cell: torch.Tensor, cutoff: float, alpha: float = 0.0,
                          neighbor_list: torch.Tensor | None = None, neighbor_ptr: torch.Tensor | None = None,
                          neighbor_shifts: torch.Tensor | None = None, neighbor_matrix: torch.Tensor | None = None,
                          neighbor_matrix_shifts: torch.Tensor | None = None, fill_value: int | None = None,
                          batch_idx: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """``(energies[N], forces[N,3])`` with the 1/2 prefactor in both formats; every stored entry (i, j) adds +f_ij to atom i and
    -f_ij to atom j (coulomb.py:1540-1691)."""
    e, f = _run(positions, charges, cell, cutoff, alpha, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts,
                fill_value, batch_idx, want_forces=True)
    return e.to(positions.dtype), f.to(positions.dtype)


@C.traceable
def coulomb_forces(positions: torch.Tensor, charges: torch.Tensor, cell: torch.Tensor, cutoff: float, alpha: float = 0.0,
                   neighbor_list: torch.Tensor | None = None, neighbor_ptr: torch.Tensor | None = None,
                   neighbor_shifts: torch.Tensor | None = None, neighbor_matrix: torch.Tensor | None = None,
                   neighbor_matrix_shifts: torch.Tensor | None = None, fill_value: int | None = None,
                   batch_idx: torch.Tensor | None = None) -> torch.Tensor:
    """Forces only (coulomb.py:1492-1537: the energy+forces launch with the energies dropped)."""
    _, forces = coulomb_energy_forces(positions=positions, charges=charges, cell=cell, cutoff=cutoff, alpha=alpha, neighbor_list=neighbor_list,
                                      neighbor_ptr=neighbor_ptr, neighbor_shifts=neighbor_shifts, neighbor_matrix=neighbor_matrix,
                                      neighbor_matrix_shifts=neighbor_matrix_shifts, fill_value=fill_value, batch_idx=batch_idx)
    return forces


__all__ = ["coulomb_energy", "coulomb_forces", "coulomb_energy_forces"]
