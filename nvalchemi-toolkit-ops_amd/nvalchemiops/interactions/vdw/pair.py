"""Van der Waals pair potentials over a neighbour list: Halgren's buffered 14-7 (AMOEBA) and Lennard-Jones, between reduced sites.

The electrostatics package covers the permanent and induced multipoles of AMOEBA-class force fields; this module is their other non-bonded
term.  AMOEBA's vdW is not a pair sum over atoms: it acts between SITES, a hydrogen's site sits on the bond to its heavy atom
(`ReducedSites`), and the force on a site is shared between the two atoms.  Both functions run on one HIP kernel family (csrc/vdw.hip,
`mi_vdw`): a pack kernel writes one record per site, a wave-per-row pair kernel sums the row owner's energy, site force, parameter gradients
and virial words without atomics, a gather kernel redistributes the site forces to the atoms.  Forward and adjoint are the same launch with
and without per-atom weights, so every output is bit-reproducible.  The reference package has no counterpart."""
from __future__ import annotations

import ctypes
import functools

import torch

from nvalchemiops import _capi as C
from nvalchemiops.interactions.electrostatics import _pairs as P
from nvalchemiops.interactions.vdw.sites import ReducedSites

BUFFERED_14_7, LENNARD_JONES = 0, 1
RADIUS_RULES = {"arithmetic": 0, "geometric": 1, "cubic-mean": 2}
EPSILON_RULES = {"geometric": 0, "hhg": 1}
VDW_FORCES, VDW_RADIUS_GRAD, VDW_EPSILON_GRAD, VDW_VIRIAL = P.FORCES, P.CHARGE_GRAD, P.THIRD_GRAD, P.VIRIAL

_COMMON_DOC = """`radii[i]` is the MINIMUM-ENERGY distance of the like pair (R_min, not sigma; R_min = 2^(1/6) sigma for Lennard-Jones) for both kinds, so
    U(R_ij) = -eps_ij, and `epsilons[i]` its well depth.  Combining rules:

        radius_rule    "arithmetic" (R_i + R_j) / 2      "geometric" sqrt(R_i R_j)      "cubic-mean" (R_i^3 + R_j^3) / (R_i^2 + R_j^2)
        epsilon_rule   "geometric" sqrt(eps_i eps_j)     "hhg" 4 eps_i eps_j / (sqrt(eps_i) + sqrt(eps_j))^2

    (anything else raises ValueError).  An atom with R <= 0, eps <= 0 or NaN has no vdW site: its entries are skipped from both ends and its
    energy and parameter gradients are exactly 0; its force is what its children's sites hand to it, exactly 0 when it has none.

    `taper=None` truncates at `cutoff`; `taper=r_on` with 0 < r_on < cutoff multiplies by Tinker's quintic switch
    T = 1 - 10 t^3 + 15 t^4 - 6 t^5, t = (r - r_on) / (cutoff - r_on), for r > r_on (AMOEBA: r_on = 0.9 cutoff); forces, gradients and virial
    include T'.  Entries with r >= cutoff or r <= 1e-8 contribute exactly 0.

    `pair_scales` (None: 1) has the shape of the index array -- `neighbor_matrix` [N, M], or [num_pairs] with `neighbor_list` -- float32 or
    float64, multiplies each entry, must be symmetric and is not differentiable.  Exclusions and 1-4 factors follow the package's ADD pattern:
    one call on the non-bonded list plus one call on the bonded-pair list with `pair_scales = s - 1`.

    `sites` (a `ReducedSites`; None: sites are atoms) places the site of a reduced atom at r_i - (1 - kappa) (r_i - r_p), the point at kappa
    of the bond.  With a cell, r_i - r_p is the minimum image and the site stays at the atom's OWN image, the one the list's shifts belong
    to, so coordinates wrapped atom by atom and whole molecules give the same result.  THE LIST is the caller's ATOM list and must be FULL (symmetric); `cutoff`
    applies to SITE distances, so the list must reach `cutoff` plus twice the largest site displacement (1 - kappa) |r_i - r_p|.  A shorter,
    half or truncated list is not detected.  A matrix entry equal to `mask_value` or outside [0, N) is padding.

    `cell=None` is a cluster: no shifts may be passed and `compute_virial` raises.

    Returns ``energies`` [N], or a tuple (energies, forces [N, 3], radius_grads [N], epsilon_grads [N], virial [num_systems, 3, 3]) holding
    only the items asked for, all in the positions dtype (sums in float64).  forces = -dE/dr are on ATOMS, already redistributed: atom a
    receives kappa_a F_a + sum over its children (1 - kappa_c) F_c of the site forces.  radius_grads = dE/dR, epsilon_grads = dE/deps of the
    total E = sum_i E_i; virial = -dE/d(strain) under x -> (I + eps) x, cell and positions strained together.  Energies are differentiable
    once w.r.t. positions, radii and epsilons (the same kernel run as its own adjoint); the call then goes through its `alchemiops::` op, as
    it does under `torch.compile`.  Differentiating the explicit forces, gradients or virial raises NotImplementedError; kappa, the scales
    and the cell have no gradient.  CPU tensors raise NativeLibraryError: there is no fallback."""


def _check(positions, radii, epsilons, cell, cutoff, taper, sites, pair_scales, delta, gamma, radius_rule, epsilon_rule, neighbor_list,
           neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, batch_idx, compute_virial):
    """Every argument error, before anything is launched: the siblings' list checks plus the model's own.  Returns the two rule codes."""
    if radius_rule not in RADIUS_RULES:
        raise ValueError(f"unknown radius_rule {radius_rule!r}: expected one of {sorted(RADIUS_RULES)}")
    if epsilon_rule not in EPSILON_RULES:
        raise ValueError(f"unknown epsilon_rule {epsilon_rule!r}: expected one of {sorted(EPSILON_RULES)}")
    if positions.dim() != 2 or positions.shape[1] != 3:
        raise ValueError(f"positions must have shape [num_atoms, 3], got {tuple(positions.shape)}")
    P.check_lists(positions, None, 0.0, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, batch_idx,
                  compute_virial)
    n = positions.shape[0]
    for name, t in (("radii", radii), ("epsilons", epsilons)):
        if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.shape[0] != n:
            raise ValueError(f"{name} must have one entry per atom: expected shape [{n}], got {tuple(getattr(t, 'shape', ()))}")
    if not float(cutoff) > 0.0:
        raise ValueError(f"cutoff must be positive, got {cutoff}")
    if taper is not None and not 0.0 < float(taper) < float(cutoff):
        raise ValueError(f"taper must lie inside (0, cutoff = {cutoff}), got {taper}")
    if not (float(delta) > 0.0 and float(gamma) > 0.0):
        raise ValueError(f"delta and gamma must be positive, got {delta} and {gamma}")
    if sites is not None:
        if not isinstance(sites, ReducedSites):
            raise TypeError(f"sites must be a ReducedSites, got {type(sites)}")
        if sites.num_atoms != n:
            raise ValueError(f"sites describes {sites.num_atoms} atoms but positions has {n}")
    if pair_scales is not None:
        want = tuple(neighbor_list.shape[1:]) if neighbor_list is not None else tuple(neighbor_matrix.shape)
        if tuple(pair_scales.shape) != want:
            raise ValueError(f"pair_scales must have the shape of the index array {list(want)}, got {tuple(pair_scales.shape)}")
        if pair_scales.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"pair_scales must be float32 or float64, got {pair_scales.dtype}")
    return RADIUS_RULES[radius_rule], EPSILON_RULES[epsilon_rule]


def _launch(kind, p, model, flags, weights=None, energies: bool = True):
    """One `mi_vdw` launch: float64 (energies | None, forces in the positions dtype | None, radius sums | None, epsilon sums | None, per-system
    virial partials [nsys, blocks, words] | None)."""
    pos = p["pos"]
    n, dev, dt = pos.shape[0], pos.device, pos.dtype
    L = C.lib()
    f64 = dict(dtype=torch.float64, device=dev)
    e = torch.empty(n, **f64) if energies else None
    f = torch.empty((n, 3), dtype=dt, device=dev) if flags & VDW_FORCES else None
    rg = torch.empty(n, **f64) if flags & VDW_RADIUS_GRAD else None
    eg = torch.empty(n, **f64) if flags & VDW_EPSILON_GRAD else None
    part = torch.empty((p["nsys"], int(L.mi_vdw_blocks()), int(L.mi_vdw_row_words())), **f64) if flags & VDW_VIRIAL else None
    with_sites = p["parent"] is not None
    nbytes = int(L.mi_vdw_scratch_bytes(n, C.dtype_code(dt), int(with_sites)))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ps = p["scales"]
    cutoff, taper, delta, gamma, rrule, erule = model
    rc = L.mi_vdw(C.ptr(pos), C.ptr(p["q"]), C.ptr(p["eps"]), C.ptr(p["cells"]), C.ptr(p["bi"]), C.ptr(weights), C.ptr(p["parent"]),
                  C.ptr(p["reduction"]), C.ptr(p["child_ptr"]), C.ptr(p["child_idx"]),
                  ctypes.c_longlong(p["child_idx"].shape[0] if with_sites else 0), C.ptr(ps), C.dtype_code(ps.dtype) if ps is not None else 0, n,
                  int(p["nsys"]), C.dtype_code(dt), int(kind), int(rrule), int(erule), C.cdouble(delta), C.cdouble(gamma), C.cdouble(cutoff),
                  C.cdouble(taper), C.ptr(p["idx"]), C.ptr(p["sh"]), C.ptr(p["nptr"]), int(p["m"]), int(p["mask"]), int(flags), C.ptr(e), C.ptr(f),
                  C.ptr(rg), C.ptr(eg), C.ptr(part), C.ptr(scratch), ctypes.c_size_t(nbytes), C.stream_of(pos))
    C.check(rc, "mi_vdw")
    return e, f, rg, eg, part


def _inputs(positions, radii, epsilons, cell, batch_idx, parent, reduction, child_ptr, child_idx, pair_scales, lists, mask_value):
    """Launch tensors: `P.launch_inputs` (radii under "q") plus the site tables and the scales."""
    p = P.launch_inputs(positions, radii, cell, batch_idx, lists, mask=int(mask_value), eps=epsilons)
    C.require_device(positions, parent, reduction, child_ptr, child_idx, pair_scales)
    p["parent"], p["child_ptr"], p["child_idx"] = C.i32(parent), C.i32(child_ptr), C.i32(child_idx)
    p["reduction"] = None if reduction is None else reduction.detach().to(positions.dtype).contiguous()
    p["scales"] = None if pair_scales is None else pair_scales.detach().contiguous()
    return p


def _forward(kind, positions, radii, epsilons, cell, batch_idx, parent, reduction, child_ptr, child_idx, pair_scales, neighbor_list, neighbor_ptr,
             neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, mask_value, cutoff, taper, delta, gamma, radius_rule, epsilon_rule, forces,
             rgrads, egrads, virial):
    """(energies, forces | None, radius_grads | None, epsilon_grads | None, virial | None) in the positions dtype, no autograd graph: what the
    eager call and the op both run.  `taper` < 0: none."""
    lists = (neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts)
    p = _inputs(positions, radii, epsilons, cell, batch_idx, parent, reduction, child_ptr, child_idx, pair_scales, lists, mask_value)
    n, dev, dt = positions.shape[0], positions.device, positions.dtype
    if n == 0 or p["n_entries"] == 0:
        e, f, rg, eg, vir = P.zeros(n, p["nsys"], dt, dev, (), ())
        return e, f if forces else None, rg if rgrads else None, eg if egrads else None, vir if virial else None
    flags = P.flag_bits((True, forces, rgrads, egrads, virial))
    e, f, rg, eg, part = _launch(kind, p, (cutoff, taper, delta, gamma, radius_rule, epsilon_rule), flags)
    vir = C.fold_virial(part).to(dt) if virial else None
    return e.to(dt), f, rg.to(dt) if rgrads else None, eg.to(dt) if egrads else None, vir


def _adjoint(kind, positions, radii, epsilons, cell, batch_idx, parent, reduction, child_ptr, child_idx, pair_scales, neighbor_list, neighbor_ptr,
             neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, mask_value, cutoff, taper, delta, gamma, radius_rule, epsilon_rule,
             grad_energies):
    """Float64 (dL/dpositions, dL/dradii, dL/depsilons) of L = sum_i g_i E_i: the forward kernels with weights."""
    lists = (neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts)
    p = _inputs(positions, radii, epsilons, cell, batch_idx, parent, reduction, child_ptr, child_idx, pair_scales, lists, mask_value)
    n, dev = positions.shape[0], positions.device
    f64 = dict(dtype=torch.float64, device=dev)
    if n == 0 or p["n_entries"] == 0:
        return torch.zeros((n, 3), **f64), torch.zeros(n, **f64), torch.zeros(n, **f64)
    g = grad_energies.detach().to(torch.float64).contiguous()
    _, f, rg, eg, _ = _launch(kind, p, (cutoff, taper, delta, gamma, radius_rule, epsilon_rule), VDW_FORCES | VDW_RADIUS_GRAD | VDW_EPSILON_GRAD,
                              weights=g, energies=False)
    return -f.to(torch.float64), rg, eg


def _call(kind, positions, radii, epsilons, cell, cutoff, taper, sites, pair_scales, delta, gamma, radius_rule, epsilon_rule, neighbor_list,
          neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, mask_value, batch_idx, compute_forces, compute_radius_gradients,
          compute_epsilon_gradients, compute_virial):
    rrule, erule = _check(positions, radii, epsilons, cell, cutoff, taper, sites, pair_scales, delta, gamma, radius_rule, epsilon_rule,
                          neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, batch_idx, compute_virial)
    n, dev, dt = positions.shape[0], positions.device, positions.dtype
    want = (True, compute_forces, compute_radius_gradients, compute_epsilon_gradients, compute_virial)
    nsys = cell.reshape(-1, 3, 3).shape[0] if (cell is not None and batch_idx is not None) else 1
    n_entries = neighbor_list.shape[1] if neighbor_list is not None else neighbor_matrix.numel()
    if n == 0 or n_entries == 0:
        return P.select(P.zeros(n, nsys, dt, dev, (), ()), want)
    tables = (None,) * 4 if sites is None else (sites.parent, sites.reduction, sites.child_ptr, sites.child_idx)
    args = (positions, radii.to(dt), epsilons.to(dt), cell, batch_idx, *tables, pair_scales, neighbor_list, neighbor_ptr, neighbor_shifts,
            neighbor_matrix, neighbor_matrix_shifts, int(mask_value), float(cutoff), -1.0 if taper is None else float(taper), float(delta),
            float(gamma), rrule, erule, bool(compute_forces), bool(compute_radius_gradients), bool(compute_epsilon_gradients), bool(compute_virial))
    return P.dispatch("VDW_OPS", functools.partial(_forward, kind), args, (positions, radii, epsilons), want, kind)


@C.traceable
def buffered_14_7(positions: torch.Tensor, radii: torch.Tensor, epsilons: torch.Tensor, cell: torch.Tensor | None = None, *, cutoff: float,
                  taper: float | None = None, sites: ReducedSites | None = None, pair_scales: torch.Tensor | None = None, delta: float = 0.07,
                  gamma: float = 0.12, radius_rule: str = "cubic-mean", epsilon_rule: str = "hhg", neighbor_list: torch.Tensor | None = None,
                  neighbor_ptr: torch.Tensor | None = None, neighbor_shifts: torch.Tensor | None = None, neighbor_matrix: torch.Tensor | None = None,
                  neighbor_matrix_shifts: torch.Tensor | None = None, mask_value: int = -1, batch_idx: torch.Tensor | None = None,
                  compute_forces: bool = False, compute_radius_gradients: bool = False, compute_epsilon_gradients: bool = False,
                  compute_virial: bool = False):
    """Halgren's buffered 14-7 van der Waals energy (the vdW term of AMOEBA) between sites.  Over the stored entries (i, j, S) of the list, with
    d the separation of the two SITES, r = |d| and rho = r / R_ij:

        E_i = 1/2 sum_{entries of row i} s_e T(r) U_ij(r),    U = eps_ij ((1 + delta) / (rho + delta))^7 ((1 + gamma) / (rho^7 + gamma) - 2)

    COMMON"""
    return _call(BUFFERED_14_7, positions, radii, epsilons, cell, cutoff, taper, sites, pair_scales, delta, gamma, radius_rule, epsilon_rule,
                 neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, mask_value, batch_idx, compute_forces,
                 compute_radius_gradients, compute_epsilon_gradients, compute_virial)


@C.traceable
def lennard_jones(positions: torch.Tensor, radii: torch.Tensor, epsilons: torch.Tensor, cell: torch.Tensor | None = None, *, cutoff: float,
                  taper: float | None = None, sites: ReducedSites | None = None, pair_scales: torch.Tensor | None = None,
                  radius_rule: str = "arithmetic", epsilon_rule: str = "geometric", neighbor_list: torch.Tensor | None = None,
                  neighbor_ptr: torch.Tensor | None = None, neighbor_shifts: torch.Tensor | None = None, neighbor_matrix: torch.Tensor | None = None,
                  neighbor_matrix_shifts: torch.Tensor | None = None, mask_value: int = -1, batch_idx: torch.Tensor | None = None,
                  compute_forces: bool = False, compute_radius_gradients: bool = False, compute_epsilon_gradients: bool = False,
                  compute_virial: bool = False):
    """The 12-6 Lennard-Jones energy between sites, in its R_min form.  Over the stored entries (i, j, S) of the list, with d the separation of
    the two SITES, r = |d| and rho = r / R_ij:

        E_i = 1/2 sum_{entries of row i} s_e T(r) U_ij(r),    U = eps_ij (rho^-12 - 2 rho^-6)

    The defaults are the Lorentz-Berthelot rules.

    COMMON"""
    return _call(LENNARD_JONES, positions, radii, epsilons, cell, cutoff, taper, sites, pair_scales, 1.0, 1.0, radius_rule, epsilon_rule,
                 neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, mask_value, batch_idx, compute_forces,
                 compute_radius_gradients, compute_epsilon_gradients, compute_virial)


for _fn in (buffered_14_7, lennard_jones):
    _fn.__doc__ = _fn.__doc__.replace("COMMON", _COMMON_DOC)
del _fn

__all__ = ["buffered_14_7", "lennard_jones"]
