"""Gaussian-smeared charge electrostatics: the correction that turns a point-charge energy into the energy of Gaussian charge clouds.

Machine-learned potentials with learned charges (4G-HDNNP, charge equilibration, latent Ewald) place a Gaussian cloud of width sigma_i on
every atom: two clouds interact as q_i q_j erf(r / g_ij) / r with g_ij = sqrt(2 (sigma_i^2 + sigma_j^2)), and a cloud has the finite
self-energy q_i^2 / (2 sqrt(pi) sigma_i).  Since erf = 1 - erfc, the periodic Gaussian-charge energy is the point-charge Ewald / PME energy
plus a short-ranged pair sum, a self term and -- for a charged cell -- a neutralising-background term.  `gaussian_charge_correction` returns
that sum alone; add it to whatever `ewald_summation` / `particle_mesh_ewald` / `coulomb_*` returns, as `dftd3_atm` is added to `dftd3`.
The reference package has no counterpart.

The pair sum runs on one HIP kernel (csrc/gaussian.hip, `mi_gaussian_charges`): forward and adjoint are the same launch with and without
per-atom weights.  Self and background terms are O(N) elementwise torch on top; the per-system sums are a fixed-order fold
(`mi_gaussian_charges_system_sums`), so every output is bit-reproducible.
"""
from __future__ import annotations

import ctypes
import math

import torch

from nvalchemiops import _capi as C
from nvalchemiops.interactions.electrostatics import _pairs as P

GC_FORCES, GC_CHARGE_GRAD, GC_SIGMA_GRAD, GC_VIRIAL, GC_CELL_GRAD = P.FORCES, P.CHARGE_GRAD, P.THIRD_GRAD, P.VIRIAL, 16
_SQRT_PI = math.sqrt(math.pi)


def _sigma_tensor(sigma, n: int, dtype, device) -> torch.Tensor:
    """[N] widths in the positions dtype from a Python number, a 0-d tensor or an [N] tensor."""
    if not isinstance(sigma, torch.Tensor):
        return torch.full((n,), float(sigma), dtype=dtype, device=device)
    return (sigma.expand(n) if sigma.dim() == 0 else sigma).to(dtype=dtype, device=device)


def _inputs(positions, charges, sigma, cell, batch_idx, *lists):
    return P.launch_inputs(positions, charges, cell, batch_idx, lists, sigma=sigma)


def _launch(p, mask_value: int, flags: int, weights=None, energies: bool = True):
    """One `mi_gaussian_charges` launch: float64 (energies | None, forces in the positions dtype | None, charge sums | None, sigma sums | None,
    per-system tensor partials [nsys, blocks, words] | None)."""
    pos = p["pos"]
    n, dev, dt = pos.shape[0], pos.device, pos.dtype
    L = C.lib()
    f64 = dict(dtype=torch.float64, device=dev)
    e = torch.empty(n, **f64) if energies else None
    f = torch.empty((n, 3), dtype=dt, device=dev) if flags & GC_FORCES else None
    cg = torch.empty(n, **f64) if flags & GC_CHARGE_GRAD else None
    sg = torch.empty(n, **f64) if flags & GC_SIGMA_GRAD else None
    part = None
    if flags & (GC_VIRIAL | GC_CELL_GRAD):
        part = torch.empty((p["nsys"], int(L.mi_gaussian_charges_blocks()), int(L.mi_gaussian_charges_row_words())), **f64)
    nbytes = int(L.mi_gaussian_charges_scratch_bytes(n, C.dtype_code(dt)))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rc = L.mi_gaussian_charges(C.ptr(pos), C.ptr(p["q"]), C.ptr(p["sigma"]), C.ptr(p["cells"]), C.ptr(p["bi"]), C.ptr(weights), n, int(p["nsys"]),
                               C.dtype_code(dt), C.ptr(p["idx"]), C.ptr(p["sh"]), C.ptr(p["nptr"]), int(p["m"]), int(mask_value), int(flags), C.ptr(e),
                               C.ptr(f), C.ptr(cg), C.ptr(sg), C.ptr(part), C.ptr(scratch), ctypes.c_size_t(nbytes), C.stream_of(pos))
    C.check(rc, "mi_gaussian_charges")
    return e, f, cg, sg, part


def _system_sums(p, weights=None):
    """Float64 [nsys] (sum q, sum q s, sum g q s) per system, s = max(sigma, 0)^2, g = weights or 1: `mi_gaussian_charges_system_sums`, a
    fixed-order fold.  (`mi_segment_sum` adds one atomic per wave, so its last bit depends on arrival order; the outputs of this function
    are bit-reproducible -- between calls, streams and the eager and compiled paths -- and the background term must not be the exception.)"""
    L, q = C.lib(), p["q"]
    part = torch.empty((p["nsys"], int(L.mi_gaussian_charges_blocks()), 3), dtype=torch.float64, device=q.device)
    rc = L.mi_gaussian_charges_system_sums(C.ptr(q), C.ptr(p["sigma"]), C.ptr(weights), C.ptr(p["bi"]), q.shape[0], int(p["nsys"]),
                                           C.dtype_code(q.dtype), C.ptr(part), C.stream_of(q))
    C.check(rc, "mi_gaussian_charges_system_sums")
    return part.sum(1).unbind(-1)


def _atoms(x, p):
    """A per-system [nsys] value at every atom."""
    return x[p["bi"].long()] if p["bi"] is not None else x


def _forward(positions, charges, sigma, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts,
             mask_value, self_energy, neutralizing_background, forces, cgrads, sgrads, virial):
    """(energies, forces | None, charge_grads | None, sigma_grads | None, virial | None) in the positions dtype, no autograd graph: what the
    eager call and the `alchemiops::_gaussian_charge_correction` op both run."""
    p = _inputs(positions, charges, sigma, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts)
    n, dev, dt = positions.shape[0], positions.device, positions.dtype
    f64 = dict(dtype=torch.float64, device=dev)
    flags = P.flag_bits((True, forces, cgrads, sgrads, virial))
    if p["n_entries"] == 0:
        e = torch.zeros(n, **f64)
        f = torch.zeros((n, 3), dtype=dt, device=dev) if forces else None
        cg = torch.zeros(n, **f64) if cgrads else None
        sg = torch.zeros(n, **f64) if sgrads else None
        vir = torch.zeros((p["nsys"], 3, 3), **f64) if virial else None
    else:
        e, f, cg, sg, part = _launch(p, mask_value, flags)
        vir = C.fold_virial(part[..., :6]) if virial else None
    q, sig = p["q"].to(torch.float64), p["sigma"].to(torch.float64)
    if self_energy:
        smeared = sig > 0
        safe = torch.where(smeared, sig, torch.ones_like(sig))
        zero = torch.zeros_like(sig)
        e = e + torch.where(smeared, q * q / (2.0 * _SQRT_PI * safe), zero)
        if cgrads:
            cg = cg + torch.where(smeared, q / (_SQRT_PI * safe), zero)
        if sgrads:
            sg = sg - torch.where(smeared, q * q / (2.0 * _SQRT_PI * safe * safe), zero)
    if neutralizing_background and p["cells"] is not None:
        sp = torch.clamp(sig, min=0.0)
        s = sp * sp
        pref = 2.0 * math.pi / torch.abs(torch.linalg.det(p["cells"].to(torch.float64)))  # [nsys]
        qsum, qssum, _ = _system_sums(p)
        pq = _atoms(pref * qsum, p)
        e = e + pq * q * s
        if cgrads:
            cg = cg + _atoms(pref * qssum, p) + pq * s
        if sgrads:
            sg = sg + 2.0 * pq * q * sp
        if virial:  # E_bg scales as 1/V: -dE/d(strain) = +E_bg I
            vir = vir + (pref * qsum * qssum).reshape(-1, 1, 1) * torch.eye(3, **f64)
    return (e.to(dt), f, cg.to(dt) if cgrads else None, sg.to(dt) if sgrads else None, vir.to(dt) if virial else None)


def _adjoint(positions, charges, sigma, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts,
             mask_value, self_energy, neutralizing_background, grad_energies):
    """Float64 (dL/dpositions, dL/dcharges, dL/dsigma, dL/dcell [nsys, 3, 3] | None) of L = sum_i g_i E_i: the forward kernel with weights."""
    p = _inputs(positions, charges, sigma, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts)
    n, dev = positions.shape[0], positions.device
    f64 = dict(dtype=torch.float64, device=dev)
    g = grad_energies.detach().to(torch.float64).contiguous()
    periodic = p["cells"] is not None
    if n == 0 or p["n_entries"] == 0:
        gpos, gq, gs = torch.zeros((n, 3), **f64), torch.zeros(n, **f64), torch.zeros(n, **f64)
        gcell = torch.zeros((p["nsys"], 3, 3), **f64) if periodic else None
    else:
        flags = GC_FORCES | GC_CHARGE_GRAD | GC_SIGMA_GRAD | (GC_CELL_GRAD if periodic and p["sh"] is not None else 0)
        _, f, gq, gs, part = _launch(p, mask_value, flags, weights=g, energies=False)
        gpos = -f.to(torch.float64)
        gcell = (part.sum(1).reshape(-1, 3, 3) if part is not None else torch.zeros((p["nsys"], 3, 3), **f64)) if periodic else None
    q, sig = p["q"].to(torch.float64), p["sigma"].to(torch.float64)
    if self_energy:
        smeared = sig > 0
        safe = torch.where(smeared, sig, torch.ones_like(sig))
        zero = torch.zeros_like(sig)
        gq = gq + g * torch.where(smeared, q / (_SQRT_PI * safe), zero)
        gs = gs - g * torch.where(smeared, q * q / (2.0 * _SQRT_PI * safe * safe), zero)
    if neutralizing_background and periodic:
        sp = torch.clamp(sig, min=0.0)
        s = sp * sp
        cells64 = p["cells"].to(torch.float64)
        pref = 2.0 * math.pi / torch.abs(torch.linalg.det(cells64))
        qsum, _, gqs = _system_sums(p, weights=g)
        pq = _atoms(pref * qsum, p)
        gq = gq + _atoms(pref * gqs, p) + pq * g * s
        gs = gs + 2.0 * pq * g * q * sp
        # L_bg = (2 pi / V) Q sum_i g_i q_i s_i per system and d|det C|/dC = |det C| C^-T:  dL_bg/dC = -L_bg C^-T
        gcell = gcell - (pref * qsum * gqs).reshape(-1, 1, 1) * torch.linalg.inv(cells64).transpose(-1, -2)
    return gpos, gq, gs, gcell


@C.traceable
def gaussian_charge_correction(positions: torch.Tensor, charges: torch.Tensor, sigma, cell: torch.Tensor | None = None, *,
                               neighbor_list: torch.Tensor | None = None, neighbor_ptr: torch.Tensor | None = None,
                               neighbor_shifts: torch.Tensor | None = None, neighbor_matrix: torch.Tensor | None = None,
                               neighbor_matrix_shifts: torch.Tensor | None = None, mask_value: int = -1, batch_idx: torch.Tensor | None = None,
                               self_energy: bool = True, neutralizing_background: bool = True, compute_forces: bool = False,
                               compute_charge_gradients: bool = False, compute_sigma_gradients: bool = False, compute_virial: bool = False):
    """What has to be ADDED to a point-charge electrostatic energy (`ewald_summation`, `particle_mesh_ewald`, `coulomb_*`) so that it becomes
    the energy of Gaussian charge clouds of per-atom width `sigma` (same length unit as `positions`).  With s_i = max(sigma_i, 0)^2,
    g_ij = sqrt(2 (s_i + s_j)) and r = r_j - r_i + S . cell over the stored entries (i, j, S) of the list:

        E_i = -1/2 sum_{entries of row i} q_i q_j erfc(r / g_ij) / r
              + q_i^2 / (2 sqrt(pi) sigma_i)            if self_energy and sigma_i > 0
              + (2 pi / V_s) Q_s q_i s_i                if neutralizing_background and a cell is given (Q_s, V_s: charge and volume of i's system)

    THE LIST MUST BE FULL (symmetric: every pair stored from both ends), as for `dftd3` and `dftd3_atm`; a half or truncated list is not
    detected and gives wrong forces and gradients.  It must reach every pair with r < 6 g_ij: entries beyond that (erfc(6) = 2.2e-17) and
    entries with r <= 1e-8 are skipped.  sigma_i <= 0 is a point charge: no self term, no contribution from pairs of two point charges,
    dE/dsigma_i = 0.  A matrix entry equal to `mask_value` or outside [0, N) is padding.  `sigma` is [N], or a number / 0-d tensor for all atoms.

    `cell=None` is the non-periodic use beside `coulomb_*`: no shifts may be passed, there is no background term, `compute_virial` raises.
    Without entries (or atoms) the pair term is zero; self and background terms are still added when they are switched on.

    Returns ``energies`` [N], or a tuple (energies, forces [N, 3], charge_grads [N], sigma_grads [N], virial [num_systems, 3, 3]) holding only
    the items asked for, all in the positions dtype (sums in float64).  forces = -dE/dr, charge_grads = dE/dq, sigma_grads = dE/dsigma of the
    total E = sum_i E_i; virial = -dE/d(strain) under x -> (I + eps) x, the convention of `dftd3(compute_virial=True)` and `*_with_virial`.
    Energies are differentiable w.r.t. positions, charges, sigma and cell (the same kernel run as its own adjoint); the call then goes through
    the `alchemiops::_gaussian_charge_correction` op, as it does under `torch.compile`.  Differentiating the explicit forces, gradients or
    virial raises NotImplementedError.  CPU tensors raise NativeLibraryError: there is no fallback."""
    n, dev, dt = positions.shape[0], positions.device, positions.dtype
    P.check_lists(positions, charges, sigma, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, batch_idx,
                  compute_virial)
    want = (True, compute_forces, compute_charge_gradients, compute_sigma_gradients, compute_virial)
    nsys = cell.reshape(-1, 3, 3).shape[0] if (cell is not None and batch_idx is not None) else 1
    n_entries = neighbor_list.shape[1] if neighbor_list is not None else neighbor_matrix.numel()
    background = bool(neutralizing_background) and cell is not None
    if n == 0 or (n_entries == 0 and not self_energy and not background):
        return P.select(P.zeros(n, nsys, dt, dev, (), ()), want)
    sig = _sigma_tensor(sigma, n, dt, dev)
    lists = (neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts)
    flags = (bool(self_energy), background, bool(compute_forces), bool(compute_charge_gradients), bool(compute_sigma_gradients), bool(compute_virial))
    if P.needs_op(positions, charges, sig, cell):
        from nvalchemiops import _eops

        res = _eops.gaussian_charge_correction_op(positions, charges.to(dt), sig, cell, batch_idx, *lists, int(mask_value), *flags)
    else:
        res = _forward(positions, charges, sig, cell, batch_idx, *lists, int(mask_value), *flags)
    return P.select(res, want)


__all__ = ["gaussian_charge_correction"]
