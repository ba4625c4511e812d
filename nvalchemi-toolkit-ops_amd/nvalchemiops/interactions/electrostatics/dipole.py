"""Point-dipole Ewald sum: what atomic point dipoles add to the periodic electrostatic energy of point charges.

Machine-learned potentials that predict atomic dipoles, and every induced-dipole (polarisable) model, need the periodic energy of point
charges q_i PLUS point dipoles mu_i, and its derivative with respect to the dipoles (minus the electric field at each atom).  The charge
routines of this package (`ewald_summation`, `particle_mesh_ewald`) know charges only; `ewald_dipole_correction` returns the rest -- the
charge-dipole and dipole-dipole energy by explicit Ewald summation -- and is ADDED to what they return, as `gaussian_charge_correction` and
`dftd3_atm` are added to their base terms.  The reference package has no counterpart.

Four HIP kernels (csrc/dipole.hip): `mi_ewald_dipole_real` (one wave per row of a full list), `mi_ewald_dipole_structure_factors` (the
unscaled table {S_q, M_x, M_y, M_z} per k), `mi_ewald_dipole_recip_gather` (one wave per atom) and `mi_ewald_dipole_recip_virial`.  Forward
and adjoint are the same launches without and with per-atom weights; nothing uses floating-point atomics, so every output is
bit-reproducible.
"""
from __future__ import annotations

import ctypes

import torch

from nvalchemiops import _capi as C
from nvalchemiops.interactions.electrostatics import _multipoles as M
from nvalchemiops.interactions.electrostatics import _pairs as P
from nvalchemiops.interactions.electrostatics.ewald import _prepare_alpha, _prepare_cell

_TABLE_WORDS = 8  # {Re S_q, Im S_q, Re M_x, Im M_x, Re M_y, Im M_y, Re M_z, Im M_z}

_MODEL = """With R = r_j - r_i + S . cell and r = |R| for every stored entry (i, j, S), B0 = erfc(alpha r) / r,
    B_n = [(2n - 1) B_{n-1} + (2 alpha^2)^n / (alpha sqrt(pi)) exp(-alpha^2 r^2)] / r^2, c_i = mu_i . R, c_j = mu_j . R, d = mu_i . mu_j:

        U_ij = (q_i + mu_i . grad_i)(q_j + mu_j . grad_j) erfc(alpha r) / r  minus its charge-charge part
             = B1 (q_j c_i - q_i c_j + d) - B2 c_i c_j
        real space:        E_i = 1/2 sum_{entries of row i} U_ij                     (entries with r <= 1e-8 skipped; the list is the cutoff)
        reciprocal space:  E_i = 1/2 sum_k G_k { Re[A_i S] - q_i Re[e^{-i k.r_i} S_q] } - (2 alpha^3 / (3 sqrt(pi))) |mu_i|^2
                           G_k = (8 pi / V) exp(-k^2 / 4 alpha^2) / k^2 over the half-space k set of `generate_k_vectors_ewald_summation`,
                           S_q = sum_j q_j e^{i k.r_j},  M = sum_j mu_j e^{i k.r_j},  S = S_q + i k.M,  A_i = (q_i - i k.mu_i) e^{-i k.r_i}

    Gaussian units, tin-foil boundary: no surface term and no background term; the last term is the dipolar self energy."""

_RETURNS = """Returns ``energies`` [N], or a tuple holding only what was asked for, in this order: energies, forces [N, 3], charge_grads [N],
    dipole_grads [N, 3], virial [num_systems, 3, 3]; all in the positions dtype (sums in float64).  forces = -dE/dr, charge_grads = dE/dq,
    dipole_grads = dE/dmu of the total E = sum_i E_i: dipole_grads is minus the electric field at the atom (it does not vanish for zero
    dipoles), and the torque on a dipole is mu x (-dipole_grads).  virial = -dE/d(strain) under x -> (I + eps) x with the dipoles held fixed in
    the laboratory frame: dU/dR is then not parallel to R, so the virial has nine independent components and is NOT symmetric.  For dipoles
    defined in local frames (`rotate_multipoles`), `multipole_frame_forces` turns that torque into forces on the frame atoms and returns the
    term the virial lacks.

    Energies are differentiable once w.r.t. positions, charges and dipoles, for any upstream gradient on the per-atom energies (the same
    kernels run as their own adjoint); the call then goes through an `alchemiops::_ewald_dipole_*` op, as it does under `torch.compile`.
    Differentiating the explicit forces, gradients or virial raises NotImplementedError.  Gradients w.r.t. cell and alpha are out of scope
    (NotImplementedError at backward): use `compute_virial`.  Also out of scope: quadrupoles (`ewald_quadrupole_correction` adds them), `cell=None` clusters,
    surface (non-tin-foil) terms.  CPU tensors raise NativeLibraryError: there is no fallback."""


# ---- real space ---------------------------------------------------------------------------------------------------------------------------
def _real_inputs(positions, charges, dipoles, cell, alpha, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                 neighbor_matrix_shifts, mask_value):
    lists = (neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts)
    return P.launch_inputs(positions, charges, cell, batch_idx, lists, int(mask_value), mu=dipoles, al=alpha.reshape(-1))


def _real_launch(p, flags: int, weights=None, energies: bool = True):
    """One `mi_ewald_dipole_real` launch: float64 (energies | None, forces in the positions dtype | None, charge sums | None, dipole sums | None,
    virial block partials [nsys, blocks, 9] | None)."""
    pos = p["pos"]
    n, dt = pos.shape[0], pos.dtype
    L = C.lib()
    e, f, cg, dg = M.allocate(pos, M.DIPOLE, (energies, flags & P.FORCES, flags & P.CHARGE_GRAD, flags & P.THIRD_GRAD))
    nbytes = int(L.mi_ewald_dipole_real_scratch_bytes(n, C.dtype_code(dt)))
    part, scratch = M.pair_scratch(p, flags, int(L.mi_ewald_dipole_blocks()), nbytes)
    rc = L.mi_ewald_dipole_real(C.ptr(pos), C.ptr(p["q"]), C.ptr(p["mu"]), C.ptr(p["cells"]), C.ptr(p["al"]), C.ptr(p["bi"]), C.ptr(weights), n,
                                int(p["nsys"]), C.dtype_code(dt), C.ptr(p["idx"]), C.ptr(p["sh"]), C.ptr(p["nptr"]), int(p["m"]), p["mask"],
                                int(flags), C.ptr(e), C.ptr(f), C.ptr(cg), C.ptr(dg), C.ptr(part), C.ptr(scratch), ctypes.c_size_t(nbytes),
                                C.stream_of(pos))
    C.check(rc, "mi_ewald_dipole_real")
    return e, f, cg, dg, part


def _real_forward(positions, charges, dipoles, cell, alpha, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                  neighbor_matrix_shifts, mask_value, forces, cgrads, dgrads, virial):
    """(energies, forces | None, charge_grads | None, dipole_grads | None, virial | None) in the positions dtype, no autograd graph: what the
    eager call and the `alchemiops::_ewald_dipole_real_space` op both run."""
    p = _real_inputs(positions, charges, dipoles, cell, alpha, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                     neighbor_matrix_shifts, mask_value)
    return M.pair_forward(p, _real_launch, M.DIPOLE, (True, forces, cgrads, dgrads, virial))


def _real_adjoint(positions, charges, dipoles, cell, alpha, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                  neighbor_matrix_shifts, mask_value, grad_energies):
    """Float64 (dL/dpositions, dL/dcharges, dL/ddipoles) of L = sum_i g_i E_i: the forward kernel with weights."""
    p = _real_inputs(positions, charges, dipoles, cell, alpha, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                     neighbor_matrix_shifts, mask_value)
    return M.pair_adjoint(p, _real_launch, M.DIPOLE, grad_energies)


@C.traceable
def ewald_dipole_real_space(positions: torch.Tensor, charges: torch.Tensor, dipoles: torch.Tensor, cell: torch.Tensor, alpha,
                            neighbor_list: torch.Tensor | None = None, neighbor_ptr: torch.Tensor | None = None,
                            neighbor_shifts: torch.Tensor | None = None, neighbor_matrix: torch.Tensor | None = None,
                            neighbor_matrix_shifts: torch.Tensor | None = None, mask_value: int = -1, batch_idx: torch.Tensor | None = None,
                            compute_forces: bool = False, compute_charge_gradients: bool = False, compute_dipole_gradients: bool = False,
                            compute_virial: bool = False):
    """Real-space half of the point-dipole Ewald term: what has to be ADDED to `ewald_real_space` when the atoms carry point dipoles
    `dipoles` [N, 3] beside their charges.  MODEL

    THE LIST MUST BE FULL (symmetric: every pair stored from both ends), as for `gaussian_charge_correction`; a half or truncated list is not
    detected and gives wrong forces and gradients.  A matrix entry equal to `mask_value` or outside [0, N) is padding.  Over a full list
    forces_i = sum_row dU/dR, charge_grads_i = sum_row dU/dq_i, dipole_grads_i = sum_row dU/dmu_i, virial[a][b] = -1/2 sum_entries (dU/dR)_a R_b
    (`compute_virial` needs the shifts of the list).  `alpha` is a number, or a tensor with one value per system; with `batch_idx`, `cell` is
    [num_systems, 3, 3].

    RETURNS"""
    P.check_dipole_lists(positions, charges, dipoles, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts,
                         batch_idx, alpha, compute_virial)
    want = (True, compute_forces, compute_charge_gradients, compute_dipole_gradients, compute_virial)
    if positions.shape[0] == 0:
        return M.no_atoms(positions, P.num_systems(cell, batch_idx), M.DIPOLE, want)
    alpha_t = _prepare_alpha(alpha, _prepare_cell(cell)[1], positions.dtype, positions.device)
    return M.dispatch("ewald_dipole_real_space_op", _real_forward, (positions, charges, dipoles), (cell, alpha_t),
                      (batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts,
                       int(mask_value)), want)


# ---- reciprocal space ---------------------------------------------------------------------------------------------------------------------
def _recip_inputs(positions, charges, dipoles, cell, k_vectors, alpha, batch_idx):
    """Launch arguments of the reciprocal sum: detached contiguous arrays in the positions dtype, [B, K, 3] k-vectors, [B] alpha, and for a
    batch the CSR system pointer (atoms of a system are contiguous, as for `ewald_reciprocal_space`)."""
    n, dev, dt = positions.shape[0], positions.device, positions.dtype
    C.dtype_code(dt)
    C.require_device(positions, charges, dipoles, cell, k_vectors, alpha, batch_idx)
    cells, n_sys = _prepare_cell(cell)
    kv = k_vectors if k_vectors.dim() == 3 else k_vectors.unsqueeze(0)
    if kv.shape[0] != n_sys:
        kv = kv.expand(n_sys, -1, -1)
    p = dict(nsys=n_sys, n_k=kv.shape[1], pos=positions.detach().contiguous(), q=charges.detach().to(dt).contiguous(),
             mu=dipoles.detach().to(dt).contiguous(), cells=cells.detach().to(dt).contiguous(), kv=kv.detach().to(dt).contiguous(),
             al=_prepare_alpha(alpha, n_sys, dt, dev).detach().contiguous(), bi=None, sptr=None)
    if batch_idx is not None and n > 0 and n_sys > 1:
        p["bi"] = C.i32(batch_idx)
        sptr = torch.zeros(n_sys + 1, dtype=torch.int32, device=dev)
        sptr[1:] = torch.cumsum(torch.bincount(batch_idx.long(), minlength=n_sys)[:n_sys], dim=0)
        p["sptr"] = sptr
    return p


def _table(p, weights=None):
    """[B, K, 8] float64 unscaled {S_q, M_x, M_y, M_z} (`mi_ewald_dipole_structure_factors`); None without k-vectors."""
    if p["n_k"] == 0:
        return None
    pos = p["pos"]
    table = torch.empty((p["nsys"], p["n_k"], _TABLE_WORDS), dtype=torch.float64, device=pos.device)
    rc = C.lib().mi_ewald_dipole_structure_factors(C.ptr(pos), C.ptr(p["q"]), C.ptr(p["mu"]), C.ptr(weights), C.ptr(p["kv"]), C.ptr(p["sptr"]),
                                                   pos.shape[0], int(p["nsys"]), int(p["n_k"]), C.dtype_code(pos.dtype), C.ptr(table),
                                                   C.stream_of(pos))
    C.check(rc, "mi_ewald_dipole_structure_factors")
    return table


def _gather(p, table, want, table_g=None, weights=None):
    """`want` = (energies, forces, charge sums, dipole sums), as `_multipoles.allocate` takes it."""
    pos = p["pos"]
    n = pos.shape[0]
    e, f, cg, dg = M.allocate(pos, M.DIPOLE, want)
    adjoint = weights is not None and table_g is not None
    rc = C.lib().mi_ewald_dipole_recip_gather(C.ptr(pos), C.ptr(p["q"]), C.ptr(p["mu"]), C.ptr(p["kv"]) if p["n_k"] else None, C.ptr(p["cells"]),
                                              C.ptr(p["al"]), C.ptr(p["bi"]), C.ptr(table), C.ptr(table_g) if adjoint else None,
                                              C.ptr(weights) if adjoint else None, n, int(p["nsys"]), int(p["n_k"]), C.dtype_code(pos.dtype),
                                              C.ptr(e), C.ptr(f), C.ptr(cg), C.ptr(dg), C.stream_of(pos))
    C.check(rc, "mi_ewald_dipole_recip_gather")
    return e, f, cg, dg


def _recip_forward(positions, charges, dipoles, cell, k_vectors, alpha, batch_idx, forces, cgrads, dgrads, virial):
    """(energies, forces | None, charge_grads | None, dipole_grads | None, virial | None) in the positions dtype, no autograd graph."""
    n, dev, dt = positions.shape[0], positions.device, positions.dtype
    want = (True, forces, cgrads, dgrads, virial)
    if n == 0:
        return M.if_wanted(P.zeros(0, _prepare_cell(cell)[1], dt, dev, *M.DIPOLE), want)
    p = _recip_inputs(positions, charges, dipoles, cell, k_vectors, alpha, batch_idx)
    table = _table(p)
    sums = _gather(p, table, want[:-1])
    vir = None
    if virial:
        vir = torch.empty((p["nsys"], 9), dtype=torch.float64, device=dev)
        rc = C.lib().mi_ewald_dipole_recip_virial(C.ptr(table), C.ptr(p["kv"]) if p["n_k"] else None, C.ptr(p["cells"]), C.ptr(p["al"]),
                                                  int(p["nsys"]), int(p["n_k"]), C.dtype_code(dt), C.ptr(vir), C.stream_of(p["pos"]))
        C.check(rc, "mi_ewald_dipole_recip_virial")
        vir = vir.reshape(-1, 3, 3)
    return M.finish(sums, vir, want, dt)


def _recip_adjoint(positions, charges, dipoles, cell, k_vectors, alpha, batch_idx, grad_energies):
    """Float64 (dL/dpositions, dL/dcharges, dL/ddipoles) of L = sum_i g_i E_i: a second table summed with the weights g, and the gather in its
    adjoint form (dL/dtheta_i = 1/2 sum_k G_k Re[dA_i/dtheta (g_i S + S^g)] minus the charge part, self term times g_i)."""
    n, dev = positions.shape[0], positions.device
    if n == 0:
        return M.zero_gradients(0, dev, M.DIPOLE)
    p = _recip_inputs(positions, charges, dipoles, cell, k_vectors, alpha, batch_idx)
    g = M.weights_of(grad_energies)
    table = _table(p)
    if table is None:  # no k-vectors: the self term alone, -g_i 4 alpha^3 / (3 sqrt(pi)) mu_i, which is g_i times the plain dipole gradient
        dg = _gather(p, None, (False, False, False, True))[3]
        return M.zero_gradients(n, dev, M.DIPOLE[:1]) + (g.unsqueeze(1) * dg,)
    _, f, gq, gmu = _gather(p, table, (False, True, True, True), table_g=_table(p, weights=g), weights=g)
    return -f.to(torch.float64), gq, gmu


@C.traceable
def ewald_dipole_reciprocal_space(positions: torch.Tensor, charges: torch.Tensor, dipoles: torch.Tensor, cell: torch.Tensor,
                                  k_vectors: torch.Tensor, alpha, batch_idx: torch.Tensor | None = None, compute_forces: bool = False,
                                  compute_charge_gradients: bool = False, compute_dipole_gradients: bool = False, compute_virial: bool = False):
    """Reciprocal-space half of the point-dipole Ewald term, the dipolar self term included: what has to be ADDED to `ewald_reciprocal_space`
    when the atoms carry point dipoles `dipoles` [N, 3] beside their charges.  MODEL

    `k_vectors` is [K, 3] (one system) or [num_systems, K, 3] and is taken as a set of reciprocal vectors of `cell` (the virial lets it
    follow the strained cell: d(k.mu)/d eps_ab = -k_a mu_b); `alpha` is a number or one value per system.  Without k-vectors the result is
    the self term alone.  Atoms of one system are contiguous in a batch, as for `ewald_reciprocal_space`.

    RETURNS"""
    if cell is None:
        raise ValueError("cell is required: the point-dipole Ewald sum is periodic (cell=None clusters are out of scope)")
    C.dtype_code(positions.dtype)
    C.check_per_atom(positions.shape[0], charges=charges, batch_idx=batch_idx)
    P.check_dipoles(positions, dipoles)
    C.check_neighbor_data(positions.shape[0], cell=cell)
    n, dev, dt = positions.shape[0], positions.device, positions.dtype
    cells, n_sys = _prepare_cell(cell)
    if k_vectors.shape[-1] != 3 or k_vectors.dim() not in (2, 3) or (k_vectors.dim() == 3 and k_vectors.shape[0] not in (1, n_sys)):
        raise ValueError(f"k_vectors must have shape [K, 3] or [{n_sys}, K, 3], got {tuple(k_vectors.shape)}")
    want = (True, compute_forces, compute_charge_gradients, compute_dipole_gradients, compute_virial)
    if n == 0:
        return M.no_atoms(positions, n_sys, M.DIPOLE, want)
    return M.dispatch("ewald_dipole_reciprocal_space_op", _recip_forward, (positions, charges, dipoles),
                      (cells, k_vectors, _prepare_alpha(alpha, n_sys, dt, dev)), (batch_idx,), want)


@C.traceable
def ewald_dipole_correction(positions: torch.Tensor, charges: torch.Tensor, dipoles: torch.Tensor, cell: torch.Tensor, alpha=None,
                            k_vectors: torch.Tensor | None = None, k_cutoff: float | None = None, batch_idx: torch.Tensor | None = None,
                            neighbor_list: torch.Tensor | None = None, neighbor_ptr: torch.Tensor | None = None,
                            neighbor_shifts: torch.Tensor | None = None, neighbor_matrix: torch.Tensor | None = None,
                            neighbor_matrix_shifts: torch.Tensor | None = None, mask_value: int | None = None, compute_forces: bool = False,
                            compute_charge_gradients: bool = False, compute_dipole_gradients: bool = False, compute_virial: bool = False,
                            accuracy: float = 1e-6):
    """What has to be ADDED to a point-charge periodic energy (`ewald_summation`, `particle_mesh_ewald`) so that it becomes the energy of point
    charges plus point dipoles `dipoles` [N, 3]: the charge-dipole and dipole-dipole energy by explicit Ewald summation,
    `ewald_dipole_real_space` + `ewald_dipole_reciprocal_space`.  MODEL

    `alpha`, `k_cutoff` and `k_vectors` are estimated exactly as `ewald_summation` estimates them when not given (`accuracy`); pass the values
    the charge routine used, or any others: the sum of both routines does not depend on alpha beyond the truncation error.  Under
    `torch.compile(fullgraph=True)` pass `alpha` and `k_vectors` (the estimate reads device data).  THE LIST MUST BE FULL (symmetric); a half or
    truncated list is not detected.  A matrix entry equal to `mask_value` (default: N) or outside [0, N) is padding.

    RETURNS"""
    if mask_value is None:
        mask_value = positions.shape[0]
    P.check_dipole_lists(positions, charges, dipoles, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts,
                         batch_idx, alpha, compute_virial)
    return M.ewald_correction(_EWALD, (positions, charges, dipoles), cell, alpha, k_vectors, k_cutoff, batch_idx,
                              (neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts), mask_value,
                              (True, compute_forces, compute_charge_gradients, compute_dipole_gradients, compute_virial), accuracy)


FLAGS = ("compute_forces", "compute_charge_gradients", "compute_dipole_gradients", "compute_virial")
_EWALD = dict(grads=M.DIPOLE, flags=FLAGS, real=ewald_dipole_real_space, recip=ewald_dipole_reciprocal_space)

for _fn in (ewald_dipole_real_space, ewald_dipole_reciprocal_space, ewald_dipole_correction):
    _fn.__doc__ = _fn.__doc__.replace("MODEL", _MODEL).replace("RETURNS", _RETURNS)
del _fn

__all__ = ["ewald_dipole_real_space", "ewald_dipole_reciprocal_space", "ewald_dipole_correction"]
