"""Generalized Born implicit solvent (GB-OBC) with an ACE-type surface term: the solvent for the cluster operators.

Every `cell=None` operator of this package computes a system in vacuum.  `generalized_born` adds the standard continuum solvent: Born
radii by pairwise descreening (Hawkins, Cramer, Truhlar) with the rescaling of Onufriev, Bashford and Case, the pair function of Still et al.,
and optionally a surface term gamma (R_i + probe)^2 (R_i / B_i)^6 per atom.  It returns that term alone; add it to whatever `coulomb_*`, a
machine-learned potential or `charge_equilibration` gives, as `gaussian_charge_correction` is added to an Ewald energy.  The reference
package has no counterpart.

Three HIP passes (csrc/born.hip: `mi_born_radii`, `mi_born_energy`, `mi_born_chain`) -- atom property, energy and dE/dproperty, chain-rule
forces, the structure of `dftd3` -- each one wave per row of a full list, owner-only sums, no atomics: every output is bit-reproducible.
Forward and adjoint are the same launches with and without per-atom weights.
"""
from __future__ import annotations

import ctypes
import math

import torch

from nvalchemiops import _capi as C
from nvalchemiops.interactions.electrostatics import _pairs as P

GB_FORCES, GB_CHARGE_GRAD, GB_VIRIAL = P.FORCES, P.CHARGE_GRAD, P.VIRIAL  # MI_GB_*


def _per_atom(x, n: int, dtype, device) -> torch.Tensor:
    """[N] values in the positions dtype from a Python number, a 0-d tensor or an [N] tensor."""
    if not isinstance(x, torch.Tensor):
        return torch.full((n,), float(x), dtype=dtype, device=device)
    return (x.expand(n) if x.dim() == 0 else x).to(dtype=dtype, device=device)


def _inputs(positions, charges, radii, screening, cell, batch_idx, *lists):
    p = P.launch_inputs(positions, charges, cell, batch_idx, lists, radii=radii, screening=screening)
    if p["n_entries"] == 0:  # rows without entries: the self and surface terms remain.  A matrix of width 0 reads no index
        p.update(idx=None, nptr=None, sh=None, m=0)
    return p


def _consts(solute_dielectric, solvent_dielectric, coulomb_constant, offset, obc_alpha, obc_beta, obc_gamma, surface_tension, probe_radius):
    """The MI_BORN_PARAMS host doubles of the kernels."""
    pref = -0.5 * coulomb_constant * (1.0 / solute_dielectric - 1.0 / solvent_dielectric)
    return (ctypes.c_double * 7)(offset, obc_alpha, obc_beta, obc_gamma, pref, 4.0 * math.pi * surface_tension, probe_radius)


def _launch(p, mask_value: int, consts, flags: int, weights=None, energies: bool = True):
    """The passes of one evaluation: float64 (energies | None, forces in the positions dtype | None, charge sums | None, Born radii,
    per-system virial partials [nsys, blocks, words] | None).  Pass 3 runs only for forces or the virial."""
    pos = p["pos"]
    n, dev, dt = pos.shape[0], pos.device, pos.dtype
    L = C.lib()
    f64 = dict(dtype=torch.float64, device=dev)
    born = torch.empty(n, **f64)
    e = torch.empty(n, **f64) if energies else None
    f = torch.empty((n, 3), dtype=dt, device=dev) if flags & GB_FORCES else None
    cg = torch.empty(n, **f64) if flags & GB_CHARGE_GRAD else None
    part = torch.empty((p["nsys"], int(L.mi_born_blocks()), int(L.mi_born_row_words())), **f64) if flags & GB_VIRIAL else None
    nbytes = int(L.mi_born_scratch_bytes(n, C.dtype_code(dt)))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    cells, bi, stream = C.ptr(p["cells"]), C.ptr(p["bi"]), C.stream_of(pos)
    lists = (n, int(p["nsys"]), C.dtype_code(dt), C.ptr(p["idx"]), C.ptr(p["sh"]), C.ptr(p["nptr"]), int(p["m"]), int(mask_value), consts, int(flags))
    tail = (C.ptr(scratch), ctypes.c_size_t(nbytes), stream)
    C.check(L.mi_born_radii(C.ptr(pos), C.ptr(p["q"]), C.ptr(p["radii"]), C.ptr(p["screening"]), cells, bi, *lists, C.ptr(born), *tail), "mi_born_radii")
    C.check(L.mi_born_energy(cells, bi, C.ptr(weights), *lists, C.ptr(born), C.ptr(e), C.ptr(cg), *tail), "mi_born_energy")
    if flags & (GB_FORCES | GB_VIRIAL):
        C.check(L.mi_born_chain(cells, bi, *lists, C.ptr(f), C.ptr(part), *tail), "mi_born_chain")
    return e, f, cg, born, part


def _forward(positions, charges, radii, screening, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
             neighbor_matrix_shifts, mask_value, solute_dielectric, solvent_dielectric, coulomb_constant, offset, obc_alpha, obc_beta, obc_gamma,
             surface_tension, probe_radius, forces, cgrads, born_radii, virial):
    """(energies, forces | None, charge_grads | None, born_radii | None, virial | None) in the positions dtype, no autograd graph: what the
    eager call and the `alchemiops::_generalized_born` op both run."""
    p = _inputs(positions, charges, radii, screening, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts)
    dt = positions.dtype
    consts = _consts(solute_dielectric, solvent_dielectric, coulomb_constant, offset, obc_alpha, obc_beta, obc_gamma, surface_tension, probe_radius)
    e, f, cg, born, part = _launch(p, mask_value, consts, P.flag_bits((True, forces, cgrads, False, virial)))
    return (e.to(dt), f, cg.to(dt) if cgrads else None, born.to(dt) if born_radii else None, C.fold_virial(part).to(dt) if virial else None)


def _adjoint(positions, charges, radii, screening, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
             neighbor_matrix_shifts, mask_value, solute_dielectric, solvent_dielectric, coulomb_constant, offset, obc_alpha, obc_beta, obc_gamma,
             surface_tension, probe_radius, grad_energies):
    """Float64 (dL/dpositions, dL/dcharges) of L = sum_i g_i E_i: the forward passes with weights."""
    p = _inputs(positions, charges, radii, screening, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts)
    n, dev = positions.shape[0], positions.device
    if n == 0:
        return torch.zeros((0, 3), dtype=torch.float64, device=dev), torch.zeros(0, dtype=torch.float64, device=dev)
    g = grad_energies.detach().to(torch.float64).contiguous()
    consts = _consts(solute_dielectric, solvent_dielectric, coulomb_constant, offset, obc_alpha, obc_beta, obc_gamma, surface_tension, probe_radius)
    _, f, gq, _, _ = _launch(p, mask_value, consts, GB_FORCES | GB_CHARGE_GRAD, weights=g, energies=False)
    return -f.to(torch.float64), gq


@C.traceable
def generalized_born(positions: torch.Tensor, charges: torch.Tensor, radii, screening, cell: torch.Tensor | None = None, *,
                     neighbor_list: torch.Tensor | None = None, neighbor_ptr: torch.Tensor | None = None,
                     neighbor_shifts: torch.Tensor | None = None, neighbor_matrix: torch.Tensor | None = None,
                     neighbor_matrix_shifts: torch.Tensor | None = None, mask_value: int = -1, batch_idx: torch.Tensor | None = None,
                     solute_dielectric: float = 1.0, solvent_dielectric: float = 78.5, coulomb_constant: float = 1.0, offset: float = 0.09,
                     obc=(1.0, 0.8, 4.85), surface_tension: float | None = None, probe_radius: float = 1.4, compute_forces: bool = False,
                     compute_charge_gradients: bool = False, compute_born_radii: bool = False, compute_virial: bool = False):
    """The generalized Born solvation energy of charges `q_i` in cavities of intrinsic radii `R_i` (`radii`) with descreening factors
    `screening`; both are [N], or a number / 0-d tensor for all atoms.  Lengths (`offset` and `probe_radius` too) are in the unit of
    `positions`; the defaults are in Angstrom.  With rho_i = R_i - offset, S_j = screening_j rho_j and r = |r_j - r_i + S . cell| over the
    stored entries (i, j, S) of the list:

        I(r; rho, S) = (1/4pi) integral of |x|^-4 over the part of the sphere S at distance r outside the sphere rho about the origin
                     = 0 if r + S <= rho, else with L = max(rho, |r - S|), U = r + S
                       1/2 [1/L - 1/U + (r/4)(1/U^2 - 1/L^2) + ln(L/U)/(2r) + (S^2/(4r))(1/L^2 - 1/U^2)]   (+ 1/rho - 1/L if rho < S - r)
        Psi_i = rho_i sum_row I(r; rho_i, S_j),      1/B_i = 1/rho_i - tanh(a Psi - b Psi^2 + c Psi^3) / R_i,      (a, b, c) = obc
        E_i   = -1/2 k tau [q_i^2 / B_i + sum_row q_i q_j / f],   f = sqrt(r^2 + B_i B_j exp(-r^2 / (4 B_i B_j)))
                + 4 pi surface_tension (R_i + probe_radius)^2 (R_i / B_i)^6          if surface_tension is given

    with tau = 1/solute_dielectric - 1/solvent_dielectric and k = coulomb_constant.  `obc` defaults to OBC-II; OBC-I is (0.8, 0, 2.909125).

    THE LIST MUST BE FULL (symmetric: every pair stored from both ends), matrix or CSR, single or batched; a half list is not detected.
    The list is the sum: with `cell=None` it is a cluster (no shifts, no virial, the list confines pairs to their systems, `batch_idx` is not
    needed); with a cell and shifts it is the truncated sum over the listed images, as in `coulomb_dipole_correction`.  Entries with
    r <= 1e-8 are skipped; a matrix entry equal to `mask_value` or outside [0, N) is padding.  R_i <= offset raises ValueError (checked on
    the host in eager calls, one device read; not under torch.compile).

    Returns ``energies`` [N], or a tuple (energies, forces [N, 3], charge_grads [N], born_radii [N], virial [num_systems, 3, 3]) holding only
    the items asked for, all in the positions dtype (pair math and sums in float64).  forces = -dE/dr and virial = -dE/d(strain) of the total
    E = sum_i E_i, including the path through the Born radii; charge_grads = dE/dq at fixed positions.  Energies are differentiable once
    w.r.t. positions and charges (through the `alchemiops::_generalized_born` op, as under `torch.compile`); gradients w.r.t. radii,
    screening and cell raise NotImplementedError, and so does differentiating the explicit outputs.  CPU tensors raise NativeLibraryError:
    there is no fallback."""
    n, dev, dt = positions.shape[0], positions.device, positions.dtype
    P.check_lists(positions, charges, 0.0, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, batch_idx,
                  compute_virial)
    for name, x in (("radii", radii), ("screening", screening)):
        if isinstance(x, torch.Tensor) and x.dim() > 0 and tuple(x.shape) != (n,):
            raise ValueError(f"{name} must have one entry per atom: expected shape [{n}], got {tuple(x.shape)}")
    if len(obc) != 3:
        raise ValueError(f"obc must be the three coefficients (alpha, beta, gamma), got {obc!r}")
    if not (solute_dielectric > 0 and solvent_dielectric > 0):
        raise ValueError("solute_dielectric and solvent_dielectric must be positive")
    if offset < 0:
        raise ValueError(f"offset must not be negative, got {offset}")
    want = (True, compute_forces, compute_charge_gradients, compute_born_radii, compute_virial)
    nsys = cell.reshape(-1, 3, 3).shape[0] if (cell is not None and batch_idx is not None) else 1
    if n == 0:
        return P.select(P.zeros(n, nsys, dt, dev, (), ()), want)
    rad, scr = _per_atom(radii, n, dt, dev), _per_atom(screening, n, dt, dev)
    if not C.tracing() and bool((rad.detach() <= offset).any()):
        raise ValueError(f"every radius must exceed offset = {offset}: rho_i = R_i - offset has to be positive")
    lists = (neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts)
    scalars = (float(solute_dielectric), float(solvent_dielectric), float(coulomb_constant), float(offset), float(obc[0]), float(obc[1]),
               float(obc[2]), 0.0 if surface_tension is None else float(surface_tension), float(probe_radius))
    flags = (bool(compute_forces), bool(compute_charge_gradients), bool(compute_born_radii), bool(compute_virial))
    args = (positions, charges.to(dt), rad, scr, cell, batch_idx, *lists, int(mask_value), *scalars, *flags)
    return P.dispatch("generalized_born_op", _forward, args, (positions, charges, rad, scr, cell), want)


__all__ = ["generalized_born"]
