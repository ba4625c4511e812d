"""Thole damping of point dipoles: the short-ranged real-space correction that smears the charge-dipole and dipole-dipole interactions of
polarisable atoms at short range, in the exponential form AMOEBA uses.

Undamped point dipoles polarise each other without bound once a polarisability approaches the cube of a neighbour distance (the
polarisation catastrophe `induced_dipoles` reports), and bonded and close atoms sit at such distances in every real polarisable model.
`thole_dipole_correction` returns what the smearing changes and is ADDED to `ewald_dipole_correction` / `pme_dipole_correction`, as
`gaussian_charge_correction` is added to a point-charge energy.  It does not depend on the Ewald alpha and needs no mesh or k-space work.
The reference package has no counterpart.

One HIP kernel (csrc/dipole.hip): `mi_thole_dipole`, the second radial kind of the pair kernel of `mi_ewald_dipole_real` (one wave per row of a
full list).  Forward and adjoint are the same launch without and with per-atom weights; nothing uses floating-point atomics, so every output
is bit-reproducible.
"""
from __future__ import annotations

import ctypes
import math

import torch

from nvalchemiops import _capi as C
from nvalchemiops.interactions.electrostatics import _multipoles as M
from nvalchemiops.interactions.electrostatics import _pairs as P

DEFAULT_THOLE = 0.39


def check_thole(thole) -> float:
    """The Thole width as a float: a finite number > 0 (ValueError otherwise)."""
    if isinstance(thole, bool) or not isinstance(thole, (int, float)):
        raise TypeError(f"thole must be a number, got {type(thole)}")
    if not (math.isfinite(thole) and thole > 0.0):
        raise ValueError(f"thole must be finite and positive, got {thole}")
    return float(thole)


def check_polarizability(n: int, polarizability) -> None:
    if isinstance(polarizability, torch.Tensor) and polarizability.dim() > 0:
        C.check_per_atom(n, polarizability=polarizability)
        if polarizability.dim() != 1:
            raise ValueError(f"polarizability must have one entry per atom: expected shape [{n}], got {tuple(polarizability.shape)}")
    elif isinstance(polarizability, bool) or not isinstance(polarizability, (int, float, torch.Tensor)):
        raise TypeError(f"polarizability must be a number or torch.Tensor, got {type(polarizability)}")


def _check(positions, charges, dipoles, polarizability, cell, thole, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
           neighbor_matrix_shifts, batch_idx, compute_virial) -> float:
    """Every argument error, before anything is launched: `_pairs.check_dipole_lists` with a cell, the cell-less rules of `_pairs.check_lists`
    without one, plus the polarisabilities and the Thole width."""
    M.check_positions_and_format(positions, neighbor_list, neighbor_matrix)
    thole = check_thole(thole)
    M.check_optional_cell_lists(positions, charges, dipoles, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                                neighbor_matrix_shifts, batch_idx, compute_virial)
    check_polarizability(positions.shape[0], polarizability)
    return thole


def _polar_tensor(polarizability, n, dt, dev):
    if isinstance(polarizability, torch.Tensor):
        return polarizability if polarizability.dim() > 0 else polarizability.to(dt).expand(n)
    return torch.full((n,), float(polarizability), dtype=dt, device=dev)


def _inputs(positions, charges, dipoles, polar, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
            neighbor_matrix_shifts, mask_value, thole):
    lists = (neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts)
    p = P.launch_inputs(positions, charges, cell, batch_idx, lists, int(mask_value), mu=dipoles, pol=polar)
    p["thole"] = thole
    return p


def _launch(p, flags: int, weights=None, energies: bool = True):
    """One `mi_thole_dipole` launch: float64 (energies | None, forces in the positions dtype | None, charge sums | None, dipole sums | None,
    polarisability sums | None, virial block partials [nsys, blocks, 9] | None)."""
    pos = p["pos"]
    n, dt = pos.shape[0], pos.dtype
    L = C.lib()
    e, f, cg, dg, pg = M.allocate(pos, M.THOLE, (energies, flags & P.FORCES, flags & P.CHARGE_GRAD, flags & P.THIRD_GRAD, flags & P.FOURTH_GRAD))
    nbytes = int(L.mi_thole_dipole_scratch_bytes(n, C.dtype_code(dt)))
    part, scratch = M.pair_scratch(p, flags, int(L.mi_thole_dipole_blocks()), nbytes)
    rc = L.mi_thole_dipole(C.ptr(pos), C.ptr(p["q"]), C.ptr(p["mu"]), C.ptr(p["cells"]), C.ptr(p["pol"]), C.cdouble(p["thole"]), C.ptr(p["bi"]),
                           C.ptr(weights), n, int(p["nsys"]), C.dtype_code(dt), C.ptr(p["idx"]), C.ptr(p["sh"]), C.ptr(p["nptr"]), int(p["m"]),
                           p["mask"], int(flags), C.ptr(e), C.ptr(f), C.ptr(cg), C.ptr(dg), C.ptr(pg), C.ptr(part), C.ptr(scratch),
                           ctypes.c_size_t(nbytes), C.stream_of(pos))
    C.check(rc, "mi_thole_dipole")
    return e, f, cg, dg, pg, part


def _forward(positions, charges, dipoles, polar, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
             neighbor_matrix_shifts, mask_value, thole, forces, cgrads, dgrads, pgrads, virial):
    """(energies, forces | None, charge_grads | None, dipole_grads | None, polarizability_grads | None, virial | None) in the positions dtype, no
    autograd graph: what the eager call and the `alchemiops::_thole_dipole_correction` op both run."""
    p = _inputs(positions, charges, dipoles, polar, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                neighbor_matrix_shifts, mask_value, thole)
    return M.pair_forward(p, _launch, M.THOLE, (True, forces, cgrads, dgrads, pgrads, virial))


def _adjoint(positions, charges, dipoles, polar, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
             neighbor_matrix_shifts, mask_value, thole, grad_energies):
    """Float64 (dL/dpositions, dL/dcharges, dL/ddipoles, dL/dpolarizability) of L = sum_i g_i E_i: the forward kernel with weights."""
    p = _inputs(positions, charges, dipoles, polar, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                neighbor_matrix_shifts, mask_value, thole)
    return M.pair_adjoint(p, _launch, M.THOLE, grad_energies)


@C.traceable
def thole_dipole_correction(positions: torch.Tensor, charges: torch.Tensor, dipoles: torch.Tensor, polarizability,
                            cell: torch.Tensor | None = None, *, thole: float = DEFAULT_THOLE, neighbor_list: torch.Tensor | None = None,
                            neighbor_ptr: torch.Tensor | None = None, neighbor_shifts: torch.Tensor | None = None,
                            neighbor_matrix: torch.Tensor | None = None, neighbor_matrix_shifts: torch.Tensor | None = None,
                            mask_value: int = -1, batch_idx: torch.Tensor | None = None, compute_forces: bool = False,
                            compute_charge_gradients: bool = False, compute_dipole_gradients: bool = False,
                            compute_polarizability_gradients: bool = False, compute_virial: bool = False):
    """What has to be ADDED to the energy of undamped point dipoles (`ewald_dipole_correction`, `pme_dipole_correction`) so that the
    charge-dipole and dipole-dipole interactions are Thole-damped: every atom's dipole (and the charge seen by a dipole) is smeared over the
    density (3 a_T / 4 pi) exp(-a_T u^3), u = r / (a_i a_j)^(1/6), the exponential form AMOEBA uses.  Charge-charge terms are not touched.
    With R = r_j - r_i + S . cell and r = |R| for every stored entry (i, j, S), a = `polarizability` ([N], or a number), a_T = `thole`:

        E  = a_T r^3 / sqrt(a_i a_j)
        l3 = 1 - e^-E,   l5 = 1 - (1 + E) e^-E,   l7 = 1 - (1 + E + 3/5 E^2) e^-E        (damping factors of 1/r^3, 3/r^5, 15/r^7)
        D1 = -e^-E / r^3,   D2 = -3 (1 + E) e^-E / r^5,   c_i = mu_i . R, c_j = mu_j . R, d = mu_i . mu_j
        E_i = 1/2 sum_{entries of row i} [D1 (q_j c_i - q_i c_j + d) - D2 c_i c_j]

    which is the pair energy of `ewald_dipole_real_space` with D_n in place of B_n.  An entry is not damped (contributes exactly 0) when
    either atom has a <= 0 or NaN (not polarisable, the rule of `induced_dipoles`) or r <= 1e-8, and entries with E >= 50 are skipped (their
    damping is below 4e-19 of the undamped term), so the correction is short-ranged: the list has to reach about (50 / a_T)^(1/3)
    (a_i a_j)^(1/6) only, and may be the list of the real-space Ewald term.

    THE LIST MUST BE FULL (symmetric: every pair stored from both ends), matrix or CSR, single or batched, with the conventions of
    `ewald_dipole_real_space`; a half or truncated list is not detected.  A matrix entry equal to `mask_value` or outside [0, N) is padding.
    Self-image entries (i, i, S != 0) count.  `cell=None` is a cluster: no shifts may be passed and `compute_virial` raises; with a periodic
    list `compute_virial` needs the shifts.  With `batch_idx`, `cell` is [num_systems, 3, 3].

    Returns ``energies`` [N], or a tuple holding only what was asked for, in this order: energies, forces [N, 3], charge_grads [N],
    dipole_grads [N, 3], polarizability_grads [N], virial [num_systems, 3, 3]; all in the positions dtype (sums in float64).  forces = -dE/dr,
    charge_grads = dE/dq, dipole_grads = dE/dmu, polarizability_grads = dE/da of the total E = sum_i E_i; virial = -dE/d(strain) with the
    dipoles fixed in the laboratory frame: nine independent components, not symmetric.

    Energies are differentiable once w.r.t. positions, charges, dipoles and polarizability, for any upstream gradient on the per-atom
    energies (the same kernel runs as its own adjoint); the call then goes through the `alchemiops::_thole_dipole_correction` op, as it does
    under `torch.compile`.  Differentiating the explicit forces, gradients or virial raises NotImplementedError, and so does a gradient
    w.r.t. cell: use `compute_virial`.  Out of scope: per-pair or per-element widths, the linear Thole form, AMOEBA's separate direct-field
    damping and polarisation groups, anisotropic polarisabilities.  CPU tensors raise NativeLibraryError: there is no fallback."""
    thole = _check(positions, charges, dipoles, polarizability, cell, thole, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                   neighbor_matrix_shifts, batch_idx, compute_virial)
    n, dev, dt = positions.shape[0], positions.device, positions.dtype
    want = (True, compute_forces, compute_charge_gradients, compute_dipole_gradients, compute_polarizability_gradients, compute_virial)
    if n == 0:
        return M.no_atoms(positions, M.num_systems(cell, batch_idx), M.THOLE, want)
    return M.dispatch("thole_dipole_correction_op", _forward, (positions, charges, dipoles, _polar_tensor(polarizability, n, dt, dev)), (cell,),
                      (batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, int(mask_value),
                       thole), want)


__all__ = ["thole_dipole_correction"]
