"""Point-quadrupole Ewald sum: what atomic point quadrupoles add to the periodic electrostatic energy of point charges and point dipoles.

AMOEBA-class force fields, and machine-learned potentials that predict atomic multipoles, stop at the quadrupole.  The charge routines of this
package (`ewald_summation`, `particle_mesh_ewald`) know charges only and the dipole routines (`ewald_dipole_correction`,
`pme_dipole_correction`) add the charge-dipole and dipole-dipole energy; `ewald_quadrupole_correction` returns the rest -- the
charge-quadrupole, dipole-quadrupole and quadrupole-quadrupole energy by explicit Ewald summation -- and is ADDED to what they return.  None of
them changes.  The reference package has no counterpart.

Four HIP kernels (csrc/quadrupole.hip): `mi_ewald_quadrupole_real` (one wave per row of a full list), `mi_ewald_quadrupole_structure_factors`
(the unscaled table {S_q, M_x, M_y, M_z, T} per k), `mi_ewald_quadrupole_recip_gather` (one wave per atom) and
`mi_ewald_quadrupole_recip_virial`.  Forward and adjoint are the same launches without and with per-atom weights; nothing uses floating-point
atomics, so every output is bit-reproducible.
"""
from __future__ import annotations

import ctypes

import torch

from nvalchemiops import _capi as C
from nvalchemiops.interactions.electrostatics import _multipoles as M
from nvalchemiops.interactions.electrostatics import _pairs as P
from nvalchemiops.interactions.electrostatics.ewald import _prepare_alpha, _prepare_cell

_TABLE_WORDS, _V_WORDS = 10, 6  # {Re, Im} of {S_q, M_x, M_y, M_z, T}; {Re, Im} of V = sum_j (Q_j k) e^{i k.r_j} (virial only)

_MODEL = """Atom i carries q_i, mu_i and a symmetric Cartesian quadrupole Q_i, `quadrupoles` [N, 3, 3]: the second Taylor coefficient
    1/2 sum q d d of the atom's charge distribution, so that the multipole operator is L_i = q_i + mu_i . grad_i + Q_i : grad_i grad_i.  A
    traceless AMOEBA / Stone quadrupole Theta enters as Q = Theta / 3.  Tracelessness is not required, and 1/2 (Q + Q^T) of what is given is
    used.  The periodic energy is 1/2 sum' L_i L_j psi(r_ij) with psi the Ewald potential; returned is exactly the part of it in which at least
    one quadrupole appears.  With R = r_j - r_i + S . cell and r = |R| for every stored entry (i, j, S), B0 = erfc(alpha r) / r,
    B_n = [(2n - 1) B_{n-1} + (2 alpha^2)^n / (alpha sqrt(pi)) exp(-alpha^2 r^2)] / r^2, c_i = mu_i . R, t_i = tr Q_i, s_i = R . Q_i . R:

        U_ij =   q_i (B2 s_j - B1 t_j) + q_j (B2 s_i - B1 t_i)
               + B3 c_i s_j - B2 (2 mu_i.Q_j.R + t_j c_i) - B3 c_j s_i + B2 (2 mu_j.Q_i.R + t_i c_j)
               + B4 s_i s_j - B3 (t_i s_j + t_j s_i + 4 R.Q_i.Q_j.R) + B2 (t_i t_j + 2 Q_i:Q_j)
        real space:        E_i = 1/2 sum_{entries of row i} U_ij                     (entries with r <= 1e-8 skipped; the list is the cutoff)
        reciprocal space:  E_i = 1/2 sum_k G_k { tau_i Re[e^{-i k.r_i} (T - S')] - Re[(q_i - i k.mu_i) e^{-i k.r_i} T] }
                                 + (4 alpha^3 / (3 sqrt(pi))) q_i tr Q_i - (4 alpha^5 / (5 sqrt(pi))) (2 Q_i:Q_i + (tr Q_i)^2)
                           G_k = (8 pi / V) exp(-k^2 / 4 alpha^2) / k^2 over the half-space k set of `generate_k_vectors_ewald_summation`,
                           tau_j = k . Q_j . k,  T = sum_j tau_j e^{i k.r_j},  S' = sum_j (q_j + i k.mu_j) e^{i k.r_j}

    i.e. 1/2 G_k (|T|^2 - 2 Re[conj(S') T]) per k, assembled from these products (zero quadrupoles give exact zeros).  Gaussian units, tin-foil
    boundary: no surface term and no new background term; the last line is the self energy of the quadrupoles."""

_RETURNS = """Returns ``energies`` [N], or a tuple holding only what was asked for, in this order: energies, forces [N, 3], charge_grads [N],
    dipole_grads [N, 3], quadrupole_grads [N, 3, 3], virial [num_systems, 3, 3]; all in the positions dtype (sums in float64).  forces = -dE/dr,
    charge_grads = dE/dq, dipole_grads = dE/dmu, quadrupole_grads = dE/dQ of the total E = sum_i E_i.  quadrupole_grads is symmetric:
    dE = sum_ab G_ab dQ_ab for a symmetric dQ (it is the field gradient at the atom and does not vanish for zero quadrupoles).  dipole_grads of
    this correction does not depend on the dipoles (the dipole-quadrupole term is linear in mu): minus dipole_grads is the electric field of
    the quadrupoles at each atom, which is what `induced_dipoles(external_field=...)` takes.  virial = -dE/d(strain) under x -> (I + eps) x
    with the multipoles held fixed in the laboratory frame: dU/dR is then not parallel to R, so the virial has nine independent components and
    is NOT symmetric.  For multipoles defined in local frames (`rotate_multipoles`), `multipole_frame_forces` turns the torques on them into
    forces on the frame atoms and returns the term the virial lacks.

    Energies are differentiable once w.r.t. positions, charges, dipoles and quadrupoles, for any upstream gradient on the per-atom energies
    (the same kernels run as their own adjoint); the call then goes through an `alchemiops::_ewald_quadrupole_*` op, as it does under
    `torch.compile`.  Differentiating the explicit forces, gradients or virial raises NotImplementedError.  Gradients w.r.t. cell and alpha
    are out of scope (NotImplementedError at backward): use `compute_virial`.  Also out of scope: quadrupoles on the mesh (`pme_quadrupole_correction` is the mesh counterpart of this routine), `cell=None`
    clusters, octupoles, spherical-tensor input, surface (non-tin-foil) terms.  CPU tensors raise NativeLibraryError: there is no fallback."""


def check_quadrupoles(positions, quadrupoles):
    n = positions.shape[0]
    if not isinstance(quadrupoles, torch.Tensor) or tuple(quadrupoles.shape) != (n, 3, 3):
        got = tuple(quadrupoles.shape) if isinstance(quadrupoles, torch.Tensor) else type(quadrupoles).__name__
        raise ValueError(f"quadrupoles must have one 3 x 3 tensor per atom: expected shape [{n}, 3, 3], got {got}")


def _dipoles_or_zeros(positions, dipoles):
    return torch.zeros((positions.shape[0], 3), dtype=positions.dtype, device=positions.device) if dipoles is None else dipoles


# ---- real space ---------------------------------------------------------------------------------------------------------------------------
def _real_inputs(positions, charges, dipoles, quadrupoles, cell, alpha, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                 neighbor_matrix_shifts, mask_value):
    lists = (neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts)
    return P.launch_inputs(positions, charges, cell, batch_idx, lists, int(mask_value), mu=dipoles, qd=quadrupoles, al=alpha.reshape(-1))


def _real_launch(p, flags: int, weights=None, energies: bool = True):
    """One `mi_ewald_quadrupole_real` launch: float64 (energies | None, forces in the positions dtype | None, charge sums | None, dipole sums |
    None, quadrupole sums [n, 3, 3] | None, virial block partials [nsys, blocks, 9] | None)."""
    pos = p["pos"]
    n, dt = pos.shape[0], pos.dtype
    L = C.lib()
    e, f, cg, dg, qg = M.allocate(pos, M.QUADRUPOLE, (energies, flags & P.FORCES, flags & P.CHARGE_GRAD, flags & P.THIRD_GRAD,
                                                      flags & P.FOURTH_GRAD))
    nbytes = int(L.mi_ewald_quadrupole_real_scratch_bytes(n, C.dtype_code(dt)))
    part, scratch = M.pair_scratch(p, flags, int(L.mi_ewald_quadrupole_blocks()), nbytes)
    rc = L.mi_ewald_quadrupole_real(C.ptr(pos), C.ptr(p["q"]), C.ptr(p["mu"]), C.ptr(p["qd"]), C.ptr(p["cells"]), C.ptr(p["al"]), C.ptr(p["bi"]),
                                    C.ptr(weights), n, int(p["nsys"]), C.dtype_code(dt), C.ptr(p["idx"]), C.ptr(p["sh"]), C.ptr(p["nptr"]),
                                    int(p["m"]), p["mask"], int(flags), C.ptr(e), C.ptr(f), C.ptr(cg), C.ptr(dg), C.ptr(qg), C.ptr(part),
                                    C.ptr(scratch), ctypes.c_size_t(nbytes), C.stream_of(pos))
    C.check(rc, "mi_ewald_quadrupole_real")
    return e, f, cg, dg, qg, part


def _real_forward(positions, charges, dipoles, quadrupoles, cell, alpha, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                  neighbor_matrix_shifts, mask_value, forces, cgrads, dgrads, qgrads, virial):
    """(energies, forces | None, charge_grads | None, dipole_grads | None, quadrupole_grads | None, virial | None) in the positions dtype, no
    autograd graph: what the eager call and the `alchemiops::_ewald_quadrupole_real_space` op both run."""
    p = _real_inputs(positions, charges, dipoles, quadrupoles, cell, alpha, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts,
                     neighbor_matrix, neighbor_matrix_shifts, mask_value)
    return M.pair_forward(p, _real_launch, M.QUADRUPOLE, (True, forces, cgrads, dgrads, qgrads, virial))


def _real_adjoint(positions, charges, dipoles, quadrupoles, cell, alpha, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                  neighbor_matrix_shifts, mask_value, grad_energies):
    """Float64 (dL/dpositions, dL/dcharges, dL/ddipoles, dL/dquadrupoles) of L = sum_i g_i E_i: the forward kernel with weights."""
    p = _real_inputs(positions, charges, dipoles, quadrupoles, cell, alpha, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts,
                     neighbor_matrix, neighbor_matrix_shifts, mask_value)
    return M.pair_adjoint(p, _real_launch, M.QUADRUPOLE, grad_energies)


def _check_real(positions, charges, dipoles, quadrupoles, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                neighbor_matrix_shifts, batch_idx, alpha, compute_virial):
    """Every argument error of the dipole routine, with its messages, plus the quadrupole shape."""
    P.check_dipole_lists(positions, charges, dipoles, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts,
                         batch_idx, alpha, compute_virial)
    check_quadrupoles(positions, quadrupoles)


@C.traceable
def ewald_quadrupole_real_space(positions: torch.Tensor, charges: torch.Tensor, dipoles: torch.Tensor | None, quadrupoles: torch.Tensor,
                                cell: torch.Tensor, alpha, neighbor_list: torch.Tensor | None = None, neighbor_ptr: torch.Tensor | None = None,
                                neighbor_shifts: torch.Tensor | None = None, neighbor_matrix: torch.Tensor | None = None,
                                neighbor_matrix_shifts: torch.Tensor | None = None, mask_value: int = -1, batch_idx: torch.Tensor | None = None,
                                compute_forces: bool = False, compute_charge_gradients: bool = False, compute_dipole_gradients: bool = False,
                                compute_quadrupole_gradients: bool = False, compute_virial: bool = False):
    """Real-space half of the point-quadrupole Ewald term: what has to be ADDED to `ewald_real_space` + `ewald_dipole_real_space` when the atoms
    carry point quadrupoles `quadrupoles` [N, 3, 3] beside their charges and dipoles (`dipoles=None`: no dipoles).  MODEL

    THE LIST MUST BE FULL (symmetric: every pair stored from both ends), as for `ewald_dipole_real_space`; a half or truncated list is not
    detected and gives wrong forces and gradients.  A matrix entry equal to `mask_value` or outside [0, N) is padding.  Over a full list
    forces_i = sum_row dU/dR, the gradients are the row sums of dU/dq_i, dU/dmu_i, dU/dQ_i, virial[a][b] = -1/2 sum_entries (dU/dR)_a R_b
    (`compute_virial` needs the shifts of the list).  `alpha` is a number, or a tensor with one value per system; with `batch_idx`, `cell` is
    [num_systems, 3, 3].

    RETURNS"""
    dipoles = _dipoles_or_zeros(positions, dipoles)
    _check_real(positions, charges, dipoles, quadrupoles, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                neighbor_matrix_shifts, batch_idx, alpha, compute_virial)
    want = (True, compute_forces, compute_charge_gradients, compute_dipole_gradients, compute_quadrupole_gradients, compute_virial)
    if positions.shape[0] == 0:
        return M.no_atoms(positions, P.num_systems(cell, batch_idx), M.QUADRUPOLE, want)
    alpha_t = _prepare_alpha(alpha, _prepare_cell(cell)[1], positions.dtype, positions.device)
    return M.dispatch("ewald_quadrupole_real_space_op", _real_forward, (positions, charges, dipoles, quadrupoles), (cell, alpha_t),
                      (batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts,
                       int(mask_value)), want)


# ---- reciprocal space ---------------------------------------------------------------------------------------------------------------------
def _recip_inputs(positions, charges, dipoles, quadrupoles, cell, k_vectors, alpha, batch_idx):
    """Launch arguments of the reciprocal sum: those of the dipole routine plus the quadrupoles."""
    from nvalchemiops.interactions.electrostatics.dipole import _recip_inputs as dipole_inputs

    C.require_device(quadrupoles)
    p = dipole_inputs(positions, charges, dipoles, cell, k_vectors, alpha, batch_idx)
    p["qd"] = quadrupoles.detach().to(positions.dtype).contiguous()
    return p


def _table(p, weights=None, with_v: bool = False):
    """([B, K, 10] float64 unscaled {S_q, M_x, M_y, M_z, T}, [B, K, 6] V | None) (`mi_ewald_quadrupole_structure_factors`); (None, None)
    without k-vectors."""
    if p["n_k"] == 0:
        return None, None
    pos = p["pos"]
    table = torch.empty((p["nsys"], p["n_k"], _TABLE_WORDS), dtype=torch.float64, device=pos.device)
    table_v = torch.empty((p["nsys"], p["n_k"], _V_WORDS), dtype=torch.float64, device=pos.device) if with_v else None
    rc = C.lib().mi_ewald_quadrupole_structure_factors(C.ptr(pos), C.ptr(p["q"]), C.ptr(p["mu"]), C.ptr(p["qd"]), C.ptr(weights), C.ptr(p["kv"]),
                                                       C.ptr(p["sptr"]), pos.shape[0], int(p["nsys"]), int(p["n_k"]), C.dtype_code(pos.dtype),
                                                       C.ptr(table), C.ptr(table_v), C.stream_of(pos))
    C.check(rc, "mi_ewald_quadrupole_structure_factors")
    return table, table_v


def _gather(p, table, want, table_g=None, weights=None):
    """`want` = (energies, forces, charge sums, dipole sums, quadrupole sums), as `_multipoles.allocate` takes it."""
    pos = p["pos"]
    n = pos.shape[0]
    e, f, cg, dg, qg = M.allocate(pos, M.QUADRUPOLE, want)
    adjoint = weights is not None and table_g is not None
    rc = C.lib().mi_ewald_quadrupole_recip_gather(C.ptr(pos), C.ptr(p["q"]), C.ptr(p["mu"]), C.ptr(p["qd"]), C.ptr(p["kv"]) if p["n_k"] else None,
                                                  C.ptr(p["cells"]), C.ptr(p["al"]), C.ptr(p["bi"]), C.ptr(table),
                                                  C.ptr(table_g) if adjoint else None, C.ptr(weights) if adjoint else None, n, int(p["nsys"]),
                                                  int(p["n_k"]), C.dtype_code(pos.dtype), C.ptr(e), C.ptr(f), C.ptr(cg), C.ptr(dg), C.ptr(qg),
                                                  C.stream_of(pos))
    C.check(rc, "mi_ewald_quadrupole_recip_gather")
    return e, f, cg, dg, qg


def _recip_forward(positions, charges, dipoles, quadrupoles, cell, k_vectors, alpha, batch_idx, forces, cgrads, dgrads, qgrads, virial):
    """(energies, forces | None, charge_grads | None, dipole_grads | None, quadrupole_grads | None, virial | None) in the positions dtype, no
    autograd graph."""
    n, dev, dt = positions.shape[0], positions.device, positions.dtype
    want = (True, forces, cgrads, dgrads, qgrads, virial)
    if n == 0:
        return M.if_wanted(P.zeros(0, _prepare_cell(cell)[1], dt, dev, *M.QUADRUPOLE), want)
    p = _recip_inputs(positions, charges, dipoles, quadrupoles, cell, k_vectors, alpha, batch_idx)
    table, table_v = _table(p, with_v=bool(virial))
    sums = _gather(p, table, want[:-1])
    vir = None
    if virial:
        vir = torch.empty((p["nsys"], 9), dtype=torch.float64, device=dev)
        rc = C.lib().mi_ewald_quadrupole_recip_virial(C.ptr(table), C.ptr(table_v), C.ptr(p["kv"]) if p["n_k"] else None, C.ptr(p["cells"]),
                                                      C.ptr(p["al"]), int(p["nsys"]), int(p["n_k"]), C.dtype_code(dt), C.ptr(vir),
                                                      C.stream_of(p["pos"]))
        C.check(rc, "mi_ewald_quadrupole_recip_virial")
        vir = vir.reshape(-1, 3, 3)
    return M.finish(sums, vir, want, dt)


def _recip_adjoint(positions, charges, dipoles, quadrupoles, cell, k_vectors, alpha, batch_idx, grad_energies):
    """Float64 (dL/dpositions, dL/dcharges, dL/ddipoles, dL/dquadrupoles) of L = sum_i g_i E_i: a second table summed with the weights g, and
    the gather in its adjoint form (the bilinear form of atom i's factor with g_i S + S^g, halved; self term times g_i)."""
    n, dev = positions.shape[0], positions.device
    if n == 0:
        return M.zero_gradients(0, dev, M.QUADRUPOLE)
    p = _recip_inputs(positions, charges, dipoles, quadrupoles, cell, k_vectors, alpha, batch_idx)
    g = M.weights_of(grad_energies)
    table, _ = _table(p)
    if table is None:  # no k-vectors: the self term alone, whose gradients are g_i times the plain ones
        _, _, cg, _, qg = _gather(p, None, (False, False, True, False, True))
        no_force, no_dipole_gradient = M.zero_gradients(n, dev, ((3,),))
        return no_force, g * cg, no_dipole_gradient, g.reshape(-1, 1, 1) * qg
    _, f, gq, gmu, gqd = _gather(p, table, (False, True, True, True, True), table_g=_table(p, weights=g)[0], weights=g)
    return -f.to(torch.float64), gq, gmu, gqd


@C.traceable
def ewald_quadrupole_reciprocal_space(positions: torch.Tensor, charges: torch.Tensor, dipoles: torch.Tensor | None, quadrupoles: torch.Tensor,
                                      cell: torch.Tensor, k_vectors: torch.Tensor, alpha, batch_idx: torch.Tensor | None = None,
                                      compute_forces: bool = False, compute_charge_gradients: bool = False,
                                      compute_dipole_gradients: bool = False, compute_quadrupole_gradients: bool = False,
                                      compute_virial: bool = False):
    """Reciprocal-space half of the point-quadrupole Ewald term, the quadrupolar self term included: what has to be ADDED to
    `ewald_reciprocal_space` + `ewald_dipole_reciprocal_space` when the atoms carry point quadrupoles `quadrupoles` [N, 3, 3] beside their
    charges and dipoles (`dipoles=None`: no dipoles).  MODEL

    `k_vectors` is [K, 3] (one system) or [num_systems, K, 3] and is taken as a set of reciprocal vectors of `cell` (the virial lets it
    follow the strained cell: d(k.mu)/d eps_ab = -k_a mu_b, d(k.Q.k)/d eps_ab = -2 k_a (Q k)_b); `alpha` is a number or one value per system.
    Without k-vectors the result is the self term alone.  Atoms of one system are contiguous in a batch, as for `ewald_reciprocal_space`.

    RETURNS"""
    if cell is None:
        raise ValueError("cell is required: the point-dipole Ewald sum is periodic (cell=None clusters are out of scope)")
    dipoles = _dipoles_or_zeros(positions, dipoles)
    C.dtype_code(positions.dtype)
    C.check_per_atom(positions.shape[0], charges=charges, batch_idx=batch_idx)
    P.check_dipoles(positions, dipoles)
    check_quadrupoles(positions, quadrupoles)
    C.check_neighbor_data(positions.shape[0], cell=cell)
    n, dev, dt = positions.shape[0], positions.device, positions.dtype
    cells, n_sys = _prepare_cell(cell)
    if k_vectors.shape[-1] != 3 or k_vectors.dim() not in (2, 3) or (k_vectors.dim() == 3 and k_vectors.shape[0] not in (1, n_sys)):
        raise ValueError(f"k_vectors must have shape [K, 3] or [{n_sys}, K, 3], got {tuple(k_vectors.shape)}")
    want = (True, compute_forces, compute_charge_gradients, compute_dipole_gradients, compute_quadrupole_gradients, compute_virial)
    if n == 0:
        return M.no_atoms(positions, n_sys, M.QUADRUPOLE, want)
    return M.dispatch("ewald_quadrupole_reciprocal_space_op", _recip_forward, (positions, charges, dipoles, quadrupoles),
                      (cells, k_vectors, _prepare_alpha(alpha, n_sys, dt, dev)), (batch_idx,), want)


@C.traceable
def ewald_quadrupole_correction(positions: torch.Tensor, charges: torch.Tensor, dipoles: torch.Tensor | None, quadrupoles: torch.Tensor,
                                cell: torch.Tensor, alpha=None, k_vectors: torch.Tensor | None = None, k_cutoff: float | None = None,
                                batch_idx: torch.Tensor | None = None, neighbor_list: torch.Tensor | None = None,
                                neighbor_ptr: torch.Tensor | None = None, neighbor_shifts: torch.Tensor | None = None,
                                neighbor_matrix: torch.Tensor | None = None, neighbor_matrix_shifts: torch.Tensor | None = None,
                                mask_value: int | None = None, compute_forces: bool = False, compute_charge_gradients: bool = False,
                                compute_dipole_gradients: bool = False, compute_quadrupole_gradients: bool = False, compute_virial: bool = False,
                                accuracy: float = 1e-6):
    """What has to be ADDED to the periodic energy of point charges and point dipoles (`ewald_summation` or `particle_mesh_ewald`, plus
    `ewald_dipole_correction` or `pme_dipole_correction`) so that it becomes the energy of charges, dipoles and point quadrupoles
    `quadrupoles` [N, 3, 3]: the charge-quadrupole, dipole-quadrupole and quadrupole-quadrupole energy by explicit Ewald summation,
    `ewald_quadrupole_real_space` + `ewald_quadrupole_reciprocal_space`.  `dipoles=None` means no dipoles.  MODEL

    `alpha`, `k_cutoff` and `k_vectors` are estimated exactly as `ewald_dipole_correction` estimates them when not given (`accuracy`); pass
    the values the other routines used, or any others: the sum of all routines does not depend on alpha beyond the truncation error.  Under
    `torch.compile(fullgraph=True)` pass `alpha` and `k_vectors` (the estimate reads device data).  THE LIST MUST BE FULL (symmetric); a half or
    truncated list is not detected.  A matrix entry equal to `mask_value` (default: N) or outside [0, N) is padding.

    RETURNS"""
    if mask_value is None:
        mask_value = positions.shape[0]
    dipoles = _dipoles_or_zeros(positions, dipoles)
    _check_real(positions, charges, dipoles, quadrupoles, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                neighbor_matrix_shifts, batch_idx, alpha, compute_virial)
    want = (True, compute_forces, compute_charge_gradients, compute_dipole_gradients, compute_quadrupole_gradients, compute_virial)
    return M.ewald_correction(_EWALD, (positions, charges, dipoles, quadrupoles), cell, alpha, k_vectors, k_cutoff, batch_idx,
                              (neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts), mask_value, want, accuracy)


FLAGS = ("compute_forces", "compute_charge_gradients", "compute_dipole_gradients", "compute_quadrupole_gradients", "compute_virial")
_EWALD = dict(grads=M.QUADRUPOLE, flags=FLAGS, real=ewald_quadrupole_real_space, recip=ewald_quadrupole_reciprocal_space)

for _fn in (ewald_quadrupole_real_space, ewald_quadrupole_reciprocal_space, ewald_quadrupole_correction):
    _fn.__doc__ = _fn.__doc__.replace("MODEL", _MODEL).replace("RETURNS", _RETURNS)
del _fn

__all__ = ["ewald_quadrupole_real_space", "ewald_quadrupole_reciprocal_space", "ewald_quadrupole_correction"]
