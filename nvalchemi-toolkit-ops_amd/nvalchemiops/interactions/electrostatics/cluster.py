"""Cluster point multipoles: the bare (undamped, 1/r) dipole and quadrupole pair sums, and the induced-dipole solve on them.

Isolated molecules and clusters have no cell, and the Ewald and mesh routines of this package (`ewald_dipole_correction`,
`ewald_quadrupole_correction`, `pme_dipole_correction`, `pme_quadrupole_correction`, `induced_dipoles`) are periodic by construction: their
real-space kernels form 1 / (alpha sqrt(pi)), so alpha = 0 is not a way in.  For charges the package already covers the case
(`coulomb_energy(alpha=0)`, `gaussian_charge_correction`, `charge_equilibration` and `thole_dipole_correction` take `cell=None`); this module
adds the same column for point dipoles, point quadrupoles and induced dipoles:

    coulomb_dipole_correction       charge-dipole + dipole-dipole energy, ADDED to `coulomb_energy(alpha=0)`
    coulomb_quadrupole_correction   the terms with at least one quadrupole, ADDED to the two above
    cluster_induced_dipoles         the induced dipoles of a cluster, optionally Thole-damped

The radial factors are the alpha -> 0 limit of the Ewald B_n: B1 = 1 / r^3, B_{n+1} = (2n + 1) B_n / r^2.  The reference package has no
counterpart.

No kernel of its own: `mi_coulomb_dipole` and `mi_coulomb_quadrupole` are one more radial kind of the pair kernels of `mi_ewald_dipole_real`
and `mi_ewald_quadrupole_real` (csrc/dipole.hip, csrc/quadrupole.hip: one wave per row of a full list), and `mi_cluster_induced_pair_tensors`
is one more kind of the stored operator of `induced_dipoles` (csrc/induced.hip), whose product and CG kernels are used unchanged.  Forward and
adjoint are the same launch without and with per-atom weights; nothing uses floating-point atomics, so every output is bit-reproducible.
"""
from __future__ import annotations

import ctypes

import torch

from nvalchemiops import _capi as C
from nvalchemiops.interactions.electrostatics import _multipoles as M
from nvalchemiops.interactions.electrostatics import _pairs as P
from nvalchemiops.interactions.electrostatics import induced as I
from nvalchemiops.interactions.electrostatics import quadrupole as Q
from nvalchemiops.interactions.electrostatics import thole as TH

_LISTS = """THE LIST MUST BE FULL (symmetric: every pair stored from both ends), matrix or CSR, single or batched, with the conventions of
    `ewald_dipole_real_space`; a half or truncated list is not detected.  A matrix entry equal to `mask_value` or outside [0, N) is padding;
    entries with r <= 1e-8 are skipped; self-image entries (i, i, S != 0) count.  There is no cutoff argument: the list is the sum.
    `cell=None` is a cluster: no shifts may be passed, `compute_virial` raises, and `batch_idx` is not needed (the list confines pairs to
    systems: an all-pairs list per molecule is the exact cluster energy).  With a cell and shifts the result is the cut-off sum over the listed
    images, the periodic meaning `coulomb_energy` has; `compute_virial` then needs the shifts, and with `batch_idx`, `cell` is
    [num_systems, 3, 3]."""


def _check(positions, charges, dipoles, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, batch_idx,
           compute_virial):
    """Every argument error, before anything is launched."""
    M.check_positions_and_format(positions, neighbor_list, neighbor_matrix)
    M.check_optional_cell_lists(positions, charges, dipoles, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                                neighbor_matrix_shifts, batch_idx, compute_virial)


# ---- dipoles ------------------------------------------------------------------------------------------------------------------------------
def _dipole_inputs(positions, charges, dipoles, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                   neighbor_matrix_shifts, mask_value):
    lists = (neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts)
    return P.launch_inputs(positions, charges, cell, batch_idx, lists, int(mask_value), mu=dipoles)


def _dipole_launch(p, flags: int, weights=None, energies: bool = True):
    """One `mi_coulomb_dipole` launch: float64 (energies | None, forces in the positions dtype | None, charge sums | None, dipole sums | None,
    virial block partials [nsys, blocks, 9] | None)."""
    pos = p["pos"]
    n, dt = pos.shape[0], pos.dtype
    L = C.lib()
    e, f, cg, dg = M.allocate(pos, M.DIPOLE, (energies, flags & P.FORCES, flags & P.CHARGE_GRAD, flags & P.THIRD_GRAD))
    nbytes = int(L.mi_coulomb_dipole_scratch_bytes(n, C.dtype_code(dt)))
    part, scratch = M.pair_scratch(p, flags, int(L.mi_coulomb_dipole_blocks()), nbytes)
    rc = L.mi_coulomb_dipole(C.ptr(pos), C.ptr(p["q"]), C.ptr(p["mu"]), C.ptr(p["cells"]), C.ptr(p["bi"]), C.ptr(weights), n, int(p["nsys"]),
                             C.dtype_code(dt), C.ptr(p["idx"]), C.ptr(p["sh"]), C.ptr(p["nptr"]), int(p["m"]), p["mask"], int(flags),
                             C.ptr(e), C.ptr(f), C.ptr(cg), C.ptr(dg), C.ptr(part), C.ptr(scratch), ctypes.c_size_t(nbytes), C.stream_of(pos))
    C.check(rc, "mi_coulomb_dipole")
    return e, f, cg, dg, part


def _dipole_forward(positions, charges, dipoles, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                    neighbor_matrix_shifts, mask_value, forces, cgrads, dgrads, virial):
    """(energies, forces | None, charge_grads | None, dipole_grads | None, virial | None) in the positions dtype, no autograd graph: what the
    eager call and the `alchemiops::_coulomb_dipole_correction` op both run."""
    p = _dipole_inputs(positions, charges, dipoles, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                       neighbor_matrix_shifts, mask_value)
    return M.pair_forward(p, _dipole_launch, M.DIPOLE, (True, forces, cgrads, dgrads, virial))


def _dipole_adjoint(positions, charges, dipoles, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                    neighbor_matrix_shifts, mask_value, grad_energies):
    """Float64 (dL/dpositions, dL/dcharges, dL/ddipoles) of L = sum_i g_i E_i: the forward kernel with weights."""
    p = _dipole_inputs(positions, charges, dipoles, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                       neighbor_matrix_shifts, mask_value)
    return M.pair_adjoint(p, _dipole_launch, M.DIPOLE, grad_energies)


@C.traceable
def coulomb_dipole_correction(positions: torch.Tensor, charges: torch.Tensor, dipoles: torch.Tensor, cell: torch.Tensor | None = None, *,
                              neighbor_list: torch.Tensor | None = None, neighbor_ptr: torch.Tensor | None = None,
                              neighbor_shifts: torch.Tensor | None = None, neighbor_matrix: torch.Tensor | None = None,
                              neighbor_matrix_shifts: torch.Tensor | None = None, mask_value: int = -1, batch_idx: torch.Tensor | None = None,
                              compute_forces: bool = False, compute_charge_gradients: bool = False, compute_dipole_gradients: bool = False,
                              compute_virial: bool = False):
    """What has to be ADDED to the bare Coulomb energy of point charges (`coulomb_energy(alpha=0)`) when the atoms carry point dipoles
    `dipoles` [N, 3] beside their charges: the undamped charge-dipole and dipole-dipole energy over the stored entries of a full list, as
    `ewald_dipole_correction` is added to `ewald_summation` for a periodic system.  With R = r_j - r_i (+ S . cell) and r = |R| for every
    stored entry, B1 = 1 / r^3, B2 = 3 / r^5 (the alpha -> 0 limit of the B_n of `ewald_dipole_real_space`; no erfc, no exp),
    c_i = mu_i . R, c_j = mu_j . R, d = mu_i . mu_j:

        U_ij = (q_i + mu_i . grad_i)(q_j + mu_j . grad_j) (1 / r)  minus its charge-charge part  = B1 (q_j c_i - q_i c_j + d) - B2 c_i c_j
        E_i  = 1/2 sum_{entries of row i} U_ij

    LISTS

    Returns ``energies`` [N], or a tuple holding only what was asked for, in this order: energies, forces [N, 3], charge_grads [N],
    dipole_grads [N, 3], virial [num_systems, 3, 3]; all in the positions dtype (sums in float64), with the meanings they have in
    `ewald_dipole_real_space`: forces = -dE/dr, charge_grads = dE/dq, dipole_grads = dE/dmu (minus the electric field at the atom; it does
    not vanish for zero dipoles), virial = -dE/d(strain) with the dipoles fixed in the laboratory frame (nine independent components, not
    symmetric).

    Energies are differentiable once w.r.t. positions, charges and dipoles, for any upstream gradient on the per-atom energies (the same
    kernel runs as its own adjoint); the call then goes through the `alchemiops::_coulomb_dipole_correction` op, as it does under
    `torch.compile`.  Differentiating the explicit forces, gradients or virial raises NotImplementedError, and so does a gradient w.r.t.
    cell: use `compute_virial`.  Thole damping is `thole_dipole_correction` (which takes `cell=None` too) added to this; quadrupoles are
    `coulomb_quadrupole_correction`; induced dipoles are `cluster_induced_dipoles`.  Out of scope: a cutoff switching function or reaction
    field, octupoles.  CPU tensors raise NativeLibraryError: there is no fallback."""
    _check(positions, charges, dipoles, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, batch_idx,
           compute_virial)
    want = (True, compute_forces, compute_charge_gradients, compute_dipole_gradients, compute_virial)
    if positions.shape[0] == 0:
        return M.no_atoms(positions, M.num_systems(cell, batch_idx), M.DIPOLE, want)
    return M.dispatch("coulomb_dipole_correction_op", _dipole_forward, (positions, charges, dipoles), (cell,),
                      (batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, int(mask_value)), want)


# ---- quadrupoles --------------------------------------------------------------------------------------------------------------------------
def _quadrupole_inputs(positions, charges, dipoles, quadrupoles, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                       neighbor_matrix_shifts, mask_value):
    lists = (neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts)
    return P.launch_inputs(positions, charges, cell, batch_idx, lists, int(mask_value), mu=dipoles, qd=quadrupoles)


def _quadrupole_launch(p, flags: int, weights=None, energies: bool = True):
    """One `mi_coulomb_quadrupole` launch: float64 (energies | None, forces in the positions dtype | None, charge sums | None, dipole sums |
    None, quadrupole sums [n, 3, 3] | None, virial block partials [nsys, blocks, 9] | None)."""
    pos = p["pos"]
    n, dt = pos.shape[0], pos.dtype
    L = C.lib()
    e, f, cg, dg, qg = M.allocate(pos, M.QUADRUPOLE, (energies, flags & P.FORCES, flags & P.CHARGE_GRAD, flags & P.THIRD_GRAD,
                                                      flags & P.FOURTH_GRAD))
    nbytes = int(L.mi_coulomb_quadrupole_scratch_bytes(n, C.dtype_code(dt)))
    part, scratch = M.pair_scratch(p, flags, int(L.mi_coulomb_quadrupole_blocks()), nbytes)
    rc = L.mi_coulomb_quadrupole(C.ptr(pos), C.ptr(p["q"]), C.ptr(p["mu"]), C.ptr(p["qd"]), C.ptr(p["cells"]), C.ptr(p["bi"]), C.ptr(weights), n,
                                 int(p["nsys"]), C.dtype_code(dt), C.ptr(p["idx"]), C.ptr(p["sh"]), C.ptr(p["nptr"]), int(p["m"]),
                                 p["mask"], int(flags), C.ptr(e), C.ptr(f), C.ptr(cg), C.ptr(dg), C.ptr(qg), C.ptr(part), C.ptr(scratch),
                                 ctypes.c_size_t(nbytes), C.stream_of(pos))
    C.check(rc, "mi_coulomb_quadrupole")
    return e, f, cg, dg, qg, part


def _quadrupole_forward(positions, charges, dipoles, quadrupoles, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                        neighbor_matrix_shifts, mask_value, forces, cgrads, dgrads, qgrads, virial):
    """(energies, forces | None, charge_grads | None, dipole_grads | None, quadrupole_grads | None, virial | None) in the positions dtype, no
    autograd graph: what the eager call and the `alchemiops::_coulomb_quadrupole_correction` op both run."""
    p = _quadrupole_inputs(positions, charges, dipoles, quadrupoles, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts,
                           neighbor_matrix, neighbor_matrix_shifts, mask_value)
    return M.pair_forward(p, _quadrupole_launch, M.QUADRUPOLE, (True, forces, cgrads, dgrads, qgrads, virial))


def _quadrupole_adjoint(positions, charges, dipoles, quadrupoles, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                        neighbor_matrix_shifts, mask_value, grad_energies):
    """Float64 (dL/dpositions, dL/dcharges, dL/ddipoles, dL/dquadrupoles) of L = sum_i g_i E_i: the forward kernel with weights."""
    p = _quadrupole_inputs(positions, charges, dipoles, quadrupoles, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts,
                           neighbor_matrix, neighbor_matrix_shifts, mask_value)
    return M.pair_adjoint(p, _quadrupole_launch, M.QUADRUPOLE, grad_energies)


@C.traceable
def coulomb_quadrupole_correction(positions: torch.Tensor, charges: torch.Tensor, dipoles: torch.Tensor | None, quadrupoles: torch.Tensor,
                                  cell: torch.Tensor | None = None, *, neighbor_list: torch.Tensor | None = None,
                                  neighbor_ptr: torch.Tensor | None = None, neighbor_shifts: torch.Tensor | None = None,
                                  neighbor_matrix: torch.Tensor | None = None, neighbor_matrix_shifts: torch.Tensor | None = None,
                                  mask_value: int = -1, batch_idx: torch.Tensor | None = None, compute_forces: bool = False,
                                  compute_charge_gradients: bool = False, compute_dipole_gradients: bool = False,
                                  compute_quadrupole_gradients: bool = False, compute_virial: bool = False):
    """What has to be ADDED to `coulomb_energy(alpha=0)` + `coulomb_dipole_correction` when the atoms carry point quadrupoles `quadrupoles`
    [N, 3, 3] beside their charges and dipoles (`dipoles=None`: no dipoles): the undamped charge-quadrupole, dipole-quadrupole and
    quadrupole-quadrupole energy over the stored entries of a full list, under the conventions of `ewald_quadrupole_real_space`.  Q_i is the
    second Taylor coefficient 1/2 sum q d d of the atom's charge distribution (multipole operator L_i = q_i + mu_i . grad_i +
    Q_i : grad_i grad_i); a traceless AMOEBA / Stone quadrupole Theta enters as Q = Theta / 3; tracelessness is not required and
    1/2 (Q + Q^T) of what is given is used.  With R = r_j - r_i (+ S . cell), r = |R|, B1 = 1 / r^3, B_{n+1} = (2n + 1) B_n / r^2 (the
    alpha -> 0 limit of the B_n of `ewald_quadrupole_real_space`; no erfc, no exp), c_i = mu_i . R, t_i = tr Q_i, s_i = R . Q_i . R:

        U_ij =   q_i (B2 s_j - B1 t_j) + q_j (B2 s_i - B1 t_i)
               + B3 c_i s_j - B2 (2 mu_i.Q_j.R + t_j c_i) - B3 c_j s_i + B2 (2 mu_j.Q_i.R + t_i c_j)
               + B4 s_i s_j - B3 (t_i s_j + t_j s_i + 4 R.Q_i.Q_j.R) + B2 (t_i t_j + 2 Q_i:Q_j)
        E_i  = 1/2 sum_{entries of row i} U_ij                      (for a traceless Q and one charge: q (3 R.Q.R / r^5 - tr Q / r^3))

    LISTS

    Returns ``energies`` [N], or a tuple holding only what was asked for, in this order: energies, forces [N, 3], charge_grads [N],
    dipole_grads [N, 3], quadrupole_grads [N, 3, 3], virial [num_systems, 3, 3]; all in the positions dtype (sums in float64), with the
    meanings they have in `ewald_quadrupole_real_space`.  quadrupole_grads is symmetric and does not vanish for zero quadrupoles (it is the
    field gradient at the atom); every other output is exactly zero then.  dipole_grads of this correction does not depend on the dipoles:
    minus dipole_grads is the electric field of the quadrupoles at each atom, which is what `cluster_induced_dipoles(external_field=...)`
    takes.

    Energies are differentiable once w.r.t. positions, charges, dipoles and quadrupoles, for any upstream gradient on the per-atom energies
    (the same kernel runs as its own adjoint); the call then goes through the `alchemiops::_coulomb_quadrupole_correction` op, as it does
    under `torch.compile`.  Differentiating the explicit forces, gradients or virial raises NotImplementedError, and so does a gradient
    w.r.t. cell: use `compute_virial`.  Out of scope: a cutoff switching function or reaction field, octupoles, spherical-tensor input.  CPU
    tensors raise NativeLibraryError: there is no fallback."""
    dipoles = Q._dipoles_or_zeros(positions, dipoles)
    _check(positions, charges, dipoles, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, batch_idx,
           compute_virial)
    Q.check_quadrupoles(positions, quadrupoles)
    want = (True, compute_forces, compute_charge_gradients, compute_dipole_gradients, compute_quadrupole_gradients, compute_virial)
    if positions.shape[0] == 0:
        return M.no_atoms(positions, M.num_systems(cell, batch_idx), M.QUADRUPOLE, want)
    return M.dispatch("coulomb_quadrupole_correction_op", _quadrupole_forward, (positions, charges, dipoles, quadrupoles), (cell,),
                      (batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, int(mask_value)), want)


for _fn in (coulomb_dipole_correction, coulomb_quadrupole_correction):
    _fn.__doc__ = _fn.__doc__.replace("LISTS", _LISTS)
del _fn


# ---- induced dipoles ----------------------------------------------------------------------------------------------------------------------
def _check_solve(positions, charges, polarizability, external_field, batch_idx, num_systems, neighbor_list, neighbor_ptr, neighbor_matrix,
                 tolerance, max_iterations, check_interval, initial_dipoles, thole) -> int:
    """Every argument error, before anything is launched.  Returns the number of systems: `num_systems` when given, else 1 (the rule of
    `charge_equilibration`; `batch_idx` is never read on the host)."""
    if positions.dim() != 2 or positions.shape[1] != 3:
        raise ValueError(f"positions must have shape [num_atoms, 3], got {tuple(positions.shape)}")
    n = positions.shape[0]
    if neighbor_list is not None and neighbor_matrix is not None:
        raise ValueError("pass the list in ONE format: neighbor_list (with neighbor_ptr) or neighbor_matrix, not both")
    P.check_lists(positions, charges, 0.0, None, neighbor_list, neighbor_ptr, None, neighbor_matrix, None, batch_idx, False)
    TH.check_polarizability(n, polarizability)
    for name, t in (("external_field", external_field), ("initial_dipoles", initial_dipoles)):
        if t is not None and tuple(t.shape) != (n, 3):
            raise ValueError(f"{name} must have one vector per atom: expected shape [{n}, 3], got {tuple(t.shape)}")
    if thole is not None:
        TH.check_thole(thole)
    if num_systems is None:
        nsys = 1
    else:
        if isinstance(num_systems, bool) or not isinstance(num_systems, int):
            raise TypeError(f"num_systems must be an int, got {type(num_systems)}")
        if not 1 <= num_systems <= 65535:
            raise ValueError(f"num_systems must be in [1, 65535], got {num_systems}")
        nsys = num_systems
    if nsys > 1 and batch_idx is None:
        raise ValueError(f"batch_idx is required for {nsys} systems")
    if not float(tolerance) > 0.0:
        raise ValueError(f"tolerance must be positive, got {tolerance}")
    if int(max_iterations) < 1:
        raise ValueError(f"max_iterations must be at least 1, got {max_iterations}")
    if int(check_interval) < 1:
        raise ValueError(f"check_interval must be at least 1, got {check_interval}")
    return nsys


def cluster_induced_dipoles(positions: torch.Tensor, charges: torch.Tensor, polarizability, *, thole: float | None = None,
                            external_field: torch.Tensor | None = None, batch_idx: torch.Tensor | None = None, num_systems: int | None = None,
                            neighbor_list: torch.Tensor | None = None, neighbor_ptr: torch.Tensor | None = None,
                            neighbor_matrix: torch.Tensor | None = None, mask_value: int | None = None, tolerance: float = 1e-8,
                            max_iterations: int = 200, check_interval: int = 4, initial_dipoles: torch.Tensor | None = None,
                            return_info: bool = False):
    """Induced point dipoles of a cluster (no cell): the minimiser, per system, of

        U(mu) = sum_i |mu_i|^2 / (2 a_i) + E(q, mu) - sum_i mu_i . F_i

    q = `charges` [N], a = `polarizability` ([N], or a number; isotropic), F = `external_field` [N, 3] (optional) and E the bare
    charge-dipole and dipole-dipole energy `coulomb_dipole_correction`, plus `thole_dipole_correction` (exponential Thole damping of width
    `thole`; AMOEBA uses 0.39) when `thole` is given.  The result satisfies mu_i / a_i + dE/dmu_i - F_i = 0: the `dipole_grads` of
    `coulomb_dipole_correction` (+ `thole_dipole_correction`) at the returned dipoles, plus mu / a - F, vanish, so the forces of a
    polarisable step are those routines' `compute_forces=True` at the returned dipoles with no response term.  An atom with a_i <= 0 (or
    NaN) is not polarisable: its dipole is exactly 0.  The field of permanent quadrupoles enters through `external_field`:

        external_field = -coulomb_quadrupole_correction(positions, charges, None, quadrupoles, ..., compute_dipole_gradients=True)[1]

    (dipole_grads of that correction does not depend on the dipoles).  This is `induced_dipoles` / `thole_induced_dipoles` without a
    reciprocal part: the same stored operator layout (`mi_cluster_induced_pair_tensors` stores 1 / r^3 and 3 / r^5, plus the Thole D_n when
    damped), the same product and CG kernels, the same solver, and H x is the stored-operator product alone.

    THE LIST MUST BE FULL, matrix or CSR, without shifts; an entry equal to `mask_value` (default: N) or outside [0, N) is padding; entries
    with r <= 1e-8 are skipped.  The list confines pairs to systems.  The number of systems is `num_systems` when given, else 1 (`batch_idx`
    is never read on the host); `batch_idx` [N] is required when it exceeds 1.  The systems of a batch converge, and are reported,
    separately.

    Solver, `tolerance`, `max_iterations`, `check_interval`, `initial_dipoles` (warm start) and `InducedDipoleError` with both of its
    messages -- no convergence, and "not positive definite" when a search direction p with p.Hp <= 0 is met (the polarisation catastrophe
    of undamped point dipoles: two atoms at distance r are beyond it for a > r^3 / 2) -- are those of `induced_dipoles`.  All solver
    arithmetic is float64.  Nothing in the loop uses atomics and every sum is a fixed-order fold: two identical calls, and a call on a side
    stream, give bit-identical dipoles.

    Returns `dipoles` [N, 3] in the positions dtype; with `return_info=True` the named tuple `InducedDipoleResult` (dipoles,
    polarization_energy [num_systems] = -1/2 sum mu . b = U at the solution, iterations [num_systems], residual [num_systems]).  `dipoles`
    is differentiable with respect to positions, charges, polarizability and external_field by implicit differentiation (one more solve with
    the same stored operator and two evaluations of the public energy functions).  Differentiating twice raises NotImplementedError, and
    so does tracing with torch.compile: the solve has a data-dependent trip count.  CPU tensors raise NativeLibraryError: there is no
    fallback.

    Out of scope: a cell (use `induced_dipoles`), anisotropic polarisabilities, per-pair Thole widths, AMOEBA's separate direct-field damping
    and polarisation groups, a cutoff switching function or reaction field."""
    if C.tracing():
        raise NotImplementedError("cluster_induced_dipoles cannot be traced by torch.compile: the solve iterates until a device-side "
                                  "convergence flag is set.  Call it outside the compiled region (torch.compiler.disable).")
    nsys = _check_solve(positions, charges, polarizability, external_field, batch_idx, num_systems, neighbor_list, neighbor_ptr, neighbor_matrix,
                        tolerance, max_iterations, check_interval, initial_dipoles, thole)
    n, dev, dt = positions.shape[0], positions.device, positions.dtype
    if mask_value is None:
        mask_value = n
    per_atom_polar = isinstance(polarizability, torch.Tensor) and polarizability.dim() > 0
    if n == 0:
        return I._empty_result(nsys, dt, dev, return_info)
    C.require_device(positions, charges, polarizability if per_atom_polar else None, external_field, batch_idx, neighbor_list, neighbor_ptr,
                     neighbor_matrix, initial_dipoles)
    with torch.cuda.device(dev):
        polar = TH._polar_tensor(polarizability, n, dt, dev)
        lists = (neighbor_list, neighbor_ptr, None, neighbor_matrix, None)
        op = I._Operator(positions, polar, None, batch_idx, nsys, lists, mask_value, None, None, None, None, None, None, None, None, thole)
        op.name = "cluster_induced_dipoles"
        return I._run(op, positions, charges, polar, external_field, lists, int(mask_value), (float(tolerance), int(max_iterations),
                                                                                               int(check_interval)), initial_dipoles, return_info)


__all__ = ["coulomb_dipole_correction", "coulomb_quadrupole_correction", "cluster_induced_dipoles"]
