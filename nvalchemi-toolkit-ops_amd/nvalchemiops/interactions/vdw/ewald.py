"""Dispersion Ewald sum: the r^-6 tail of a Lennard-Jones-type potential summed over the lattice.

`lennard_jones` and `buffered_14_7` sum over a list and stop at their cutoff.  For a homogeneous liquid the rest is an isotropic tail
correction; for interfaces, membranes, slabs, crystals and small cells there is none, and the r^-6 tail has to be summed over the lattice
(LJ-PME, `ewald/disp` in other MD codes).  `ewald_dispersion_correction` is that sum by explicit Ewald summation, for per-atom dispersion
coefficients c_i with C6_ij = c_i c_j, and is ADDED to what `lennard_jones` returns.  The reference package has no counterpart.

HIP kernels (csrc/dispersion_ewald.hip): `mi_ewald_dispersion_real` (one wave per row of a full list), `mi_ewald_dispersion_structure_factors`
(a thread per k-vector over LDS tiles of atoms), `mi_ewald_dispersion_recip_gather` (a thread per atom over LDS tiles of k records) and
`mi_ewald_dispersion_recip_virial`.  Forward and adjoint are the same launches without and with per-atom weights; nothing uses floating-point
atomics and every summation order is fixed, so every output is bit-reproducible."""
from __future__ import annotations

import ctypes

import torch

from nvalchemiops import _capi as C
from nvalchemiops.interactions.electrostatics import _pairs as P
from nvalchemiops.interactions.electrostatics.ewald import _prepare_alpha, _prepare_cell

_MODEL = """The lattice sum is E = -1/2 sum'_{i, j, n} c_i c_j / |r_j - r_i + n|^6 with `coefficients` c [N], C6_ij = c_i c_j.  With beta = `alpha`,
    a = beta r and g(a) = exp(-a^2) (1 + a^2 + a^4 / 2) it splits into

        real space:        E_i = -1/2 sum_{entries of row i} c_i c_j (g(beta r) - T_c(r)) / r^6      (r <= 1e-8 skipped; the list is the cutoff)
        reciprocal space:  E_i = -(pi^1.5 beta^3 / (3 V)) sum_{k in half space} f(b) c_i Re[e^{-i k.r_i} S(k)]
                                 - (pi^1.5 beta^3 / (6 V)) c_i sum_j c_j + (beta^6 / 12) c_i^2
                           b = |k| / (2 beta),  f(b) = (1 - 2 b^2) exp(-b^2) + 2 sqrt(pi) b^3 erfc(b),  S(k) = sum_j c_j e^{i k.r_j}

    over the half-space k set of `generate_k_vectors_ewald_summation`; the last two terms are the k = 0 and the self term.  The sum converges
    absolutely and does not depend on alpha beyond the truncation error.  T_c = 0 unless `counted_cutoff` is given.

    For Lennard-Jones in its R_min form, U = eps_ij (rho^-12 - 2 rho^-6), the geometric rules give C6_ij = 2 eps_ij R_ij^6 = c_i c_j with
    c_i = sqrt(2 eps_i) R_i^3 (`lennard_jones_dispersion_coefficients`).  For other combining rules the tail summed here is this geometric
    approximation of C6_ij, which is the usual LJ-PME practice; the 7-term expansion of the arithmetic rule is out of scope.  The tail acts
    between ATOMS: reduced sites are not displaced."""

_RETURNS = """Returns ``energies`` [N], or a tuple holding only what was asked for, in this order: energies, forces [N, 3], coefficient_grads [N],
    virial [num_systems, 3, 3]; all in the positions dtype (sums in float64).  forces = -dE/dr and coefficient_grads = dE/dc of the total
    E = sum_i E_i; virial = -dE/d(strain) under x -> (I + eps) x with cell, positions and k-vectors strained together (symmetric).

    Energies are differentiable once w.r.t. positions and coefficients, for any upstream gradient on the per-atom energies (the same kernels
    run as their own adjoint); the call then goes through an `alchemiops::_ewald_dispersion_*` op, as it does under `torch.compile`.
    Differentiating the explicit forces, gradients or virial raises NotImplementedError.  Gradients w.r.t. cell, k-vectors and alpha are out of
    scope (NotImplementedError at backward): use `compute_virial`.  Also out of scope: an alpha / k_cutoff estimator, `cell=None` clusters
    (the mesh form is `pme_dispersion_correction`).  CPU tensors raise NativeLibraryError: there is no fallback."""

_NO_CELL = "cell is required: the dispersion Ewald sum is periodic (cell=None clusters are out of scope)"
_NONE4 = (None, None, None, None)


def _check_common(positions, coefficients, cell, batch_idx, alpha):
    if cell is None:
        raise ValueError(_NO_CELL)
    if positions.dim() != 2 or positions.shape[1] != 3:
        raise ValueError(f"positions must have shape [num_atoms, 3], got {tuple(positions.shape)}")
    C.dtype_code(positions.dtype)
    n = positions.shape[0]
    if not isinstance(coefficients, torch.Tensor) or coefficients.dim() != 1 or coefficients.shape[0] != n:
        raise ValueError(f"coefficients must have one entry per atom: expected shape [{n}], got {tuple(getattr(coefficients, 'shape', ()))}")
    C.check_per_atom(n, batch_idx=batch_idx)
    C.check_neighbor_data(n, cell=cell)
    if alpha is None:
        raise ValueError("alpha is required: the Coulomb accuracy estimate does not transfer to the dispersion sum")
    n_cells = cell.shape[0] if cell.dim() == 3 else 1
    if isinstance(alpha, torch.Tensor) and alpha.numel() > 1 and alpha.numel() != n_cells:
        raise ValueError(f"alpha has {alpha.numel()} values but there are {n_cells} systems")


def _check_counted(counted_cutoff, counted_taper):
    """(cutoff, taper) as the ABI takes them: not positive = none."""
    if counted_cutoff is None:
        if counted_taper is not None:
            raise ValueError("counted_taper needs counted_cutoff")
        return -1.0, -1.0
    if not float(counted_cutoff) > 0.0:
        raise ValueError(f"counted_cutoff must be positive, got {counted_cutoff}")
    if counted_taper is not None and not 0.0 < float(counted_taper) < float(counted_cutoff):
        raise ValueError(f"counted_taper must lie inside (0, counted_cutoff = {counted_cutoff}), got {counted_taper}")
    return float(counted_cutoff), -1.0 if counted_taper is None else float(counted_taper)


def _zeros(n, nsys, dt, dev, want):
    return tuple(r if w else None for r, w in zip(P.zeros(n, nsys, dt, dev, ()), want))


# ---- real space ---------------------------------------------------------------------------------------------------------------------------
def _real_launch(p, counted, flags: int, weights=None, energies: bool = True):
    """One `mi_ewald_dispersion_real` launch: float64 (energies | None, forces in the positions dtype | None, coefficient sums | None, virial
    block partials [nsys, blocks, words] | None)."""
    pos = p["pos"]
    n, dev, dt = pos.shape[0], pos.device, pos.dtype
    L = C.lib()
    f64 = dict(dtype=torch.float64, device=dev)
    e = torch.empty(n, **f64) if energies else None
    f = torch.empty((n, 3), dtype=dt, device=dev) if flags & P.FORCES else None
    cg = torch.empty(n, **f64) if flags & P.CHARGE_GRAD else None
    part = (torch.empty((p["nsys"], int(L.mi_ewald_dispersion_blocks()), int(L.mi_ewald_dispersion_row_words())), **f64)
            if flags & P.VIRIAL else None)
    nbytes = int(L.mi_ewald_dispersion_real_scratch_bytes(n, C.dtype_code(dt)))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rc = L.mi_ewald_dispersion_real(C.ptr(pos), C.ptr(p["q"]), C.ptr(p["cells"]), C.ptr(p["al"]), C.ptr(p["bi"]), C.ptr(weights), n,
                                    int(p["nsys"]), C.dtype_code(dt), C.cdouble(counted[0]), C.cdouble(counted[1]), C.ptr(p["idx"]),
                                    C.ptr(p["sh"]), C.ptr(p["nptr"]), int(p["m"]), int(p["mask"]), int(flags), C.ptr(e), C.ptr(f), C.ptr(cg),
                                    C.ptr(part), C.ptr(scratch), ctypes.c_size_t(nbytes), C.stream_of(pos))
    C.check(rc, "mi_ewald_dispersion_real")
    return e, f, cg, part


def _real_inputs(positions, coefficients, cell, alpha, batch_idx, lists, mask_value):
    return P.launch_inputs(positions, coefficients, cell, batch_idx, lists, int(mask_value), al=alpha.reshape(-1))


def _real_forward(positions, coefficients, cell, alpha, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                  neighbor_matrix_shifts, mask_value, counted_cutoff, counted_taper, forces, cgrads, virial):
    """(energies, forces | None, coefficient_grads | None, virial | None) in the positions dtype, no autograd graph: what the eager call and
    the `alchemiops::_ewald_dispersion_real_space` op both run."""
    p = _real_inputs(positions, coefficients, cell, alpha, batch_idx,
                     (neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts), mask_value)
    n, dt = positions.shape[0], positions.dtype
    want = (True, forces, cgrads, virial)
    if n == 0 or p["n_entries"] == 0:
        return _zeros(n, p["nsys"], dt, positions.device, want)
    e, f, cg, part = _real_launch(p, (counted_cutoff, counted_taper), P.flag_bits((True, forces, cgrads, False, virial)))
    return e.to(dt), f, cg.to(dt) if cgrads else None, C.fold_virial(part).to(dt) if virial else None


def _real_adjoint(positions, coefficients, cell, alpha, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                  neighbor_matrix_shifts, mask_value, counted_cutoff, counted_taper, grad_energies):
    """Float64 (dL/dpositions, dL/dcoefficients) of L = sum_i g_i E_i: the forward kernel with weights."""
    p = _real_inputs(positions, coefficients, cell, alpha, batch_idx,
                     (neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts), mask_value)
    n, dev = positions.shape[0], positions.device
    if n == 0 or p["n_entries"] == 0:
        return torch.zeros((n, 3), dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev)
    g = grad_energies.detach().to(torch.float64).contiguous()
    _, f, cg, _ = _real_launch(p, (counted_cutoff, counted_taper), P.FORCES | P.CHARGE_GRAD, weights=g, energies=False)
    return -f.to(torch.float64), cg


@C.traceable
def ewald_dispersion_real_space(positions: torch.Tensor, coefficients: torch.Tensor, cell: torch.Tensor, alpha, *,
                                neighbor_list: torch.Tensor | None = None, neighbor_ptr: torch.Tensor | None = None,
                                neighbor_shifts: torch.Tensor | None = None, neighbor_matrix: torch.Tensor | None = None,
                                neighbor_matrix_shifts: torch.Tensor | None = None, mask_value: int = -1, batch_idx: torch.Tensor | None = None,
                                counted_cutoff: float | None = None, counted_taper: float | None = None, compute_forces: bool = False,
                                compute_coefficient_gradients: bool = False, compute_virial: bool = False):
    """Real-space half of the dispersion Ewald sum.  MODEL

    `counted_cutoff=rc, counted_taper=rt` names the part `lennard_jones(cutoff=rc, taper=rt)` has already summed on the same list:
    T_c is then Tinker's quintic switch as that function forms it (1 below rt, 0 at and beyond rc; `counted_taper=None`: 1 below rc), so that
    `lennard_jones` with `radius_rule="geometric", epsilon_rule="geometric"` plus this correction is the lattice sum.  Bonded exclusions and
    1-4 factors keep working through `lennard_jones`'s own `pair_scales` as long as those pairs sit below the taper.  Where T_c = 1 the
    factor g - 1 is summed as a series of one sign for a^2 < 1, never formed as a difference there.

    THE LIST MUST BE FULL (symmetric: every pair stored from both ends); a half or truncated list is not detected.  A matrix entry equal to
    `mask_value` or outside [0, N) is padding.  `compute_virial` needs the shifts of the list.  `alpha` is a number, or a tensor with one
    value per system; with `batch_idx`, `cell` is [num_systems, 3, 3].

    RETURNS"""
    _check_common(positions, coefficients, cell, batch_idx, alpha)
    P.check_lists(positions, None, 0.0, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, batch_idx,
                  compute_virial)
    if compute_virial and (neighbor_shifts if neighbor_list is not None else neighbor_matrix_shifts) is None:
        raise ValueError("compute_virial needs the shifts of the list: pass neighbor_shifts with neighbor_list, neighbor_matrix_shifts with neighbor_matrix")
    counted = _check_counted(counted_cutoff, counted_taper)
    want = (True, compute_forces, compute_coefficient_gradients, compute_virial)
    n, dt, dev = positions.shape[0], positions.dtype, positions.device
    if n == 0:
        return P.select(P.zeros(0, P.num_systems(cell, batch_idx), dt, dev, ()), want)
    alpha_t = _prepare_alpha(alpha, _prepare_cell(cell)[1], dt, dev)
    args = (positions, coefficients.to(dt), cell, alpha_t, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
            neighbor_matrix_shifts, int(mask_value), *counted, bool(compute_forces), bool(compute_coefficient_gradients), bool(compute_virial))
    return P.dispatch("ewald_dispersion_real_space_op", _real_forward, args, (positions, coefficients, cell, alpha_t), want)


# ---- reciprocal space ---------------------------------------------------------------------------------------------------------------------
def _recip_inputs(positions, coefficients, cell, k_vectors, alpha, batch_idx):
    """Launch arguments of the reciprocal sum: detached contiguous arrays in the positions dtype, [B, K, 3] k-vectors, [B] alpha, and for a
    batch the CSR system pointer (atoms of a system are contiguous, as for `ewald_reciprocal_space`)."""
    n, dev, dt = positions.shape[0], positions.device, positions.dtype
    C.require_device(positions, coefficients, cell, k_vectors, alpha, batch_idx)
    cells, n_sys = _prepare_cell(cell)
    kv = k_vectors if k_vectors.dim() == 3 else k_vectors.unsqueeze(0)
    if kv.shape[0] != n_sys:
        kv = kv.expand(n_sys, -1, -1)
    p = dict(nsys=n_sys, n_k=kv.shape[1], pos=positions.detach().contiguous(), c=coefficients.detach().to(dt).contiguous(),
             cells=cells.detach().to(dt).contiguous(), kv=kv.detach().to(dt).contiguous(),
             al=_prepare_alpha(alpha, n_sys, dt, dev).detach().contiguous(), bi=None, sptr=None)
    if batch_idx is not None and n_sys > 1:
        p["bi"] = C.i32(batch_idx)
        sptr = torch.zeros(n_sys + 1, dtype=torch.int32, device=dev)
        sptr[1:] = torch.cumsum(torch.bincount(batch_idx.long(), minlength=n_sys)[:n_sys], dim=0)
        p["sptr"] = sptr
    return p


def _tables(p, weights=None):
    """(table [B, K + 1, 2], records [B, K + 1, words]) float64 of `mi_ewald_dispersion_structure_factors`; slot K is k = 0."""
    pos = p["pos"]
    n, dev = pos.shape[0], pos.device
    L = C.lib()
    slots = (p["nsys"], p["n_k"] + 1)
    table = torch.empty(slots + (2,), dtype=torch.float64, device=dev)
    records = torch.empty(slots + (int(L.mi_ewald_dispersion_record_words()),), dtype=torch.float64, device=dev)
    nbytes = int(L.mi_ewald_dispersion_sf_scratch_bytes(n, int(p["nsys"]), int(p["n_k"])))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rc = L.mi_ewald_dispersion_structure_factors(C.ptr(pos), C.ptr(p["c"]), C.ptr(weights), C.ptr(p["kv"]) if p["n_k"] else None,
                                                 C.ptr(p["cells"]), C.ptr(p["al"]), C.ptr(p["sptr"]), n, int(p["nsys"]), int(p["n_k"]),
                                                 C.dtype_code(pos.dtype), C.ptr(table), C.ptr(records), C.ptr(scratch), ctypes.c_size_t(nbytes),
                                                 C.stream_of(pos))
    C.check(rc, "mi_ewald_dispersion_structure_factors")
    return table, records


def _gather(p, records, want, records_g=None, weights=None):
    """`want` = (energies, forces, coefficient sums): float64 sums, forces in the positions dtype, None for what is not asked for."""
    pos = p["pos"]
    n, dev = pos.shape[0], pos.device
    e = torch.empty(n, dtype=torch.float64, device=dev) if want[0] else None
    f = torch.empty((n, 3), dtype=pos.dtype, device=dev) if want[1] else None
    cg = torch.empty(n, dtype=torch.float64, device=dev) if want[2] else None
    rc = C.lib().mi_ewald_dispersion_recip_gather(C.ptr(pos), C.ptr(p["c"]), C.ptr(p["al"]), C.ptr(p["bi"]), C.ptr(records), C.ptr(records_g),
                                                  C.ptr(weights), n, int(p["nsys"]), int(p["n_k"]), C.dtype_code(pos.dtype), C.ptr(e), C.ptr(f),
                                                  C.ptr(cg), C.stream_of(pos))
    C.check(rc, "mi_ewald_dispersion_recip_gather")
    return e, f, cg


def _recip_forward(positions, coefficients, cell, k_vectors, alpha, batch_idx, forces, cgrads, virial):
    """(energies, forces | None, coefficient_grads | None, virial | None) in the positions dtype, no autograd graph."""
    n, dev, dt = positions.shape[0], positions.device, positions.dtype
    want = (True, forces, cgrads, virial)
    if n == 0:
        return _zeros(0, _prepare_cell(cell)[1], dt, dev, want)
    p = _recip_inputs(positions, coefficients, cell, k_vectors, alpha, batch_idx)
    table, records = _tables(p)
    e, f, cg = _gather(p, records, want[:3])
    vir = None
    if virial:
        words = torch.empty((p["nsys"], 1, 6), dtype=torch.float64, device=dev)
        rc = C.lib().mi_ewald_dispersion_recip_virial(C.ptr(table), C.ptr(p["kv"]) if p["n_k"] else None, C.ptr(p["cells"]), C.ptr(p["al"]),
                                                      int(p["nsys"]), int(p["n_k"]), C.dtype_code(dt), C.ptr(words), C.stream_of(p["pos"]))
        C.check(rc, "mi_ewald_dispersion_recip_virial")
        vir = C.fold_virial(words).to(dt)
    return e.to(dt), f, cg.to(dt) if cgrads else None, vir


def _recip_adjoint(positions, coefficients, cell, k_vectors, alpha, batch_idx, grad_energies):
    """Float64 (dL/dpositions, dL/dcoefficients) of L = sum_i g_i E_i: a second table summed with the weights g, and the gather in its
    adjoint form over g_i S + S^g (self term times g_i)."""
    n, dev = positions.shape[0], positions.device
    if n == 0:
        return torch.zeros((0, 3), dtype=torch.float64, device=dev), torch.zeros(0, dtype=torch.float64, device=dev)
    p = _recip_inputs(positions, coefficients, cell, k_vectors, alpha, batch_idx)
    g = grad_energies.detach().to(torch.float64).contiguous()
    _, f, cg = _gather(p, _tables(p)[1], (False, True, True), records_g=_tables(p, weights=g)[1], weights=g)
    return -f.to(torch.float64), cg


@C.traceable
def ewald_dispersion_reciprocal_space(positions: torch.Tensor, coefficients: torch.Tensor, cell: torch.Tensor, k_vectors: torch.Tensor | None,
                                      alpha, batch_idx: torch.Tensor | None = None, compute_forces: bool = False,
                                      compute_coefficient_gradients: bool = False, compute_virial: bool = False):
    """Reciprocal-space half of the dispersion Ewald sum, the k = 0 and self terms included.  MODEL

    `k_vectors` is [K, 3] (one system) or [num_systems, K, 3], a half-space set of reciprocal vectors of `cell` (the virial lets it follow
    the strained cell); `alpha` is a number or one value per system.  Without k-vectors (None, or K = 0) the result is the k = 0 and self
    terms alone.  Atoms of one system are contiguous in a batch, as for `ewald_reciprocal_space`.

    RETURNS"""
    _check_common(positions, coefficients, cell, batch_idx, alpha)
    n, dev, dt = positions.shape[0], positions.device, positions.dtype
    cells, n_sys = _prepare_cell(cell)
    if k_vectors is None:
        k_vectors = positions.new_zeros((0, 3))
    if k_vectors.shape[-1] != 3 or k_vectors.dim() not in (2, 3) or (k_vectors.dim() == 3 and k_vectors.shape[0] not in (1, n_sys)):
        raise ValueError(f"k_vectors must have shape [K, 3] or [{n_sys}, K, 3], got {tuple(k_vectors.shape)}")
    want = (True, compute_forces, compute_coefficient_gradients, compute_virial)
    if n == 0:
        return P.select(P.zeros(0, n_sys, dt, dev, ()), want)
    alpha_t = _prepare_alpha(alpha, n_sys, dt, dev)
    args = (positions, coefficients.to(dt), cells, k_vectors, alpha_t, batch_idx, bool(compute_forces), bool(compute_coefficient_gradients),
            bool(compute_virial))
    return P.dispatch("ewald_dispersion_reciprocal_space_op", _recip_forward, args, (positions, coefficients, cells, k_vectors, alpha_t), want)


@C.traceable
def ewald_dispersion_correction(positions: torch.Tensor, coefficients: torch.Tensor, cell: torch.Tensor, alpha, *,
                                k_vectors: torch.Tensor | None = None, k_cutoff: float | None = None, neighbor_list: torch.Tensor | None = None,
                                neighbor_ptr: torch.Tensor | None = None, neighbor_shifts: torch.Tensor | None = None,
                                neighbor_matrix: torch.Tensor | None = None, neighbor_matrix_shifts: torch.Tensor | None = None,
                                mask_value: int = -1, batch_idx: torch.Tensor | None = None, counted_cutoff: float | None = None,
                                counted_taper: float | None = None, compute_forces: bool = False, compute_coefficient_gradients: bool = False,
                                compute_virial: bool = False):
    """The r^-6 lattice sum of a dispersion potential, `ewald_dispersion_real_space` + `ewald_dispersion_reciprocal_space`: what has to be
    ADDED to a `lennard_jones` energy truncated at `counted_cutoff` (tapered from `counted_taper`) on the same list so that its attractive
    part becomes the sum over the lattice.  MODEL

    `alpha` is required, and so is one of `k_vectors` / `k_cutoff` (the k set is then `generate_k_vectors_ewald_summation(cell, k_cutoff)`):
    the Coulomb accuracy estimate does not transfer, and an estimator is out of scope.  Under `torch.compile(fullgraph=True)` pass
    `k_vectors`.  THE LIST MUST BE FULL (symmetric); a half or truncated list is not detected.  A matrix entry equal to `mask_value` or
    outside [0, N) is padding.

    RETURNS"""
    _check_common(positions, coefficients, cell, batch_idx, alpha)
    if k_vectors is None and k_cutoff is None:
        raise ValueError("one of k_vectors / k_cutoff is required: the Coulomb accuracy estimate does not transfer to the dispersion sum")
    flags = dict(compute_forces=compute_forces, compute_coefficient_gradients=compute_coefficient_gradients, compute_virial=compute_virial)
    real = ewald_dispersion_real_space(positions, coefficients, cell, alpha, neighbor_list=neighbor_list, neighbor_ptr=neighbor_ptr,
                                       neighbor_shifts=neighbor_shifts, neighbor_matrix=neighbor_matrix,
                                       neighbor_matrix_shifts=neighbor_matrix_shifts, mask_value=mask_value, batch_idx=batch_idx,
                                       counted_cutoff=counted_cutoff, counted_taper=counted_taper, **flags)
    if k_vectors is None:
        from nvalchemiops.interactions.electrostatics.k_vectors import generate_k_vectors_ewald_summation

        k_vectors = generate_k_vectors_ewald_summation(_prepare_cell(cell)[0], k_cutoff)
    rec = ewald_dispersion_reciprocal_space(positions, coefficients, cell, k_vectors, alpha, batch_idx=batch_idx, **flags)
    if isinstance(real, tuple):
        return tuple(a + b for a, b in zip(real, rec))
    return real + rec


def lennard_jones_dispersion_coefficients(radii: torch.Tensor, epsilons: torch.Tensor) -> torch.Tensor:
    """c_i = sqrt(2 eps_i) R_i^3 with R the minimum-energy distance, as in `lennard_jones`: C6_ij = c_i c_j is the r^-6 coefficient of
    U = eps_ij (rho^-12 - 2 rho^-6) under the geometric rules.  An atom without a site (R <= 0, eps <= 0 or NaN) gets 0 and contributes exact
    zeros.  Differentiable torch code."""
    site = (radii > 0) & (epsilons > 0)
    one = torch.ones_like(radii)
    return torch.where(site, torch.sqrt(2.0 * torch.where(site, epsilons, one)) * torch.where(site, radii, one) ** 3, torch.zeros_like(radii))


for _fn in (ewald_dispersion_real_space, ewald_dispersion_reciprocal_space, ewald_dispersion_correction):
    _fn.__doc__ = _fn.__doc__.replace("MODEL", _MODEL).replace("RETURNS", _RETURNS)
del _fn

__all__ = ["ewald_dispersion_real_space", "ewald_dispersion_reciprocal_space", "ewald_dispersion_correction",
           "lennard_jones_dispersion_coefficients"]
