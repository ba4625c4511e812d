"""Scaled, Thole-damped bonded pairs of point dipoles: the direct-field and mutual scale factors of a polarisable force field on the
charge-dipole and dipole-dipole energy, as an energy operator and as a second small stored operator inside the induced-dipole solvers.

`pair_scale_correction` scales the complete bare pair energy with one factor per pair.  A polarisable model needs two more things: separate
factors on the charge-dipole ("direct") and dipole-dipole ("mutual") terms, and the Thole damping the solvers apply when `thole=` is given.

    dipole_pair_scale_correction   1/2 sum [(s^d - 1) l3 B1 (q_j c_i - q_i c_j) + (s^m - 1) (l3 B1 mu_i.mu_j - l5 B2 c_i c_j)] over a list
    PolarizationPairScales         (neighbor_matrix, direct_scales, mutual_scales): the `scaled_pairs=` argument of `scaled_induced_dipoles`

One HIP file (csrc/dipole_scale.hip): `mi_dipole_scale` with 8 lanes per row as `mi_pair_scale`, an 8-word record per atom, forward and
adjoint the same launch; `mi_scaled_dipole_tensors` / `mi_scaled_dipole_apply` store the mutual part once per geometry and add its product to
what `mi_induced_apply` takes as `y_in`.  Nothing uses atomics, so every output is bit-reproducible.  The reference package has no counterpart.
"""
from __future__ import annotations

import collections
import ctypes

import torch

from nvalchemiops import _capi as C
from nvalchemiops.interactions.electrostatics import _multipoles as M
from nvalchemiops.interactions.electrostatics import _pairs as P
from nvalchemiops.interactions.electrostatics import thole as TH

F64 = torch.float64
PolarizationPairScales = collections.namedtuple("PolarizationPairScales", ["neighbor_matrix", "direct_scales", "mutual_scales"])
PolarizationPairScales.__doc__ = """The bonded pairs of a polarisable model as `scaled_induced_dipoles(scaled_pairs=)` takes them: a FULL `neighbor_matrix`
[N, M] (padding: N) and `direct_scales` / `mutual_scales` [N, M] (symmetric; either may be None = all 1).  `bonded_pair_scales` drops pairs
whose factor is exactly 1, so the union list of two scale sets of equal length comes from two calls with the sets shifted by 2:

    d, m = (bonded_pair_scales(bonds, n, [s + 2 for s in scales]) for scales in (direct, mutual))
    scaled_pairs = PolarizationPairScales(d.neighbor_matrix, d.pair_scales - 2, m.pair_scales - 2)

(both calls list every pair within the depth in the same order; the scale of a padding slot is not read)."""


def _check_scales(name, scales, want):
    if scales is None:
        return
    if not isinstance(scales, torch.Tensor):
        raise ValueError(f"{name} must be a tensor shaped like the index array, got {type(scales).__name__}")
    if tuple(scales.shape) != want:
        raise ValueError(f"{name} must have the shape of the index array: expected {list(want)}, got {tuple(scales.shape)}")
    if scales.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{name} must be float32 or float64, got {scales.dtype}")
    if scales.requires_grad:
        raise NotImplementedError(f"dipole_pair_scale_correction: {name} is not differentiable (dE/ds is out of scope); detach it")


def _check(positions, charges, dipoles, direct_scales, mutual_scales, cell, polarizability, thole, neighbor_list, neighbor_ptr, neighbor_shifts,
           neighbor_matrix, neighbor_matrix_shifts, batch_idx, minimum_image, compute_virial) -> float:
    """Every argument error, before anything is launched: those of `pair_scale_correction`, plus the two scale arrays and the Thole pair.
    Returns the Thole width, 0.0 for None."""
    M.check_positions_and_format(positions, neighbor_list, neighbor_matrix)
    if minimum_image:
        if cell is None:
            raise ValueError("minimum_image needs a cell")
        if neighbor_shifts is not None or neighbor_matrix_shifts is not None:
            raise ValueError("minimum_image takes a list without shifts: every entry is reduced to its minimum image")
    M.check_optional_cell_lists(positions, charges, dipoles, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                                neighbor_matrix_shifts, batch_idx, compute_virial and not minimum_image)
    if direct_scales is None and mutual_scales is None:
        raise ValueError("direct_scales and mutual_scales are both None: nothing is scaled")
    want = tuple(neighbor_matrix.shape) if neighbor_matrix is not None else (neighbor_list.shape[1],)
    _check_scales("direct_scales", direct_scales, want)
    _check_scales("mutual_scales", mutual_scales, want)
    if thole is not None and polarizability is None:
        raise ValueError("thole needs the polarizability: the damping width of a pair is a_T r^3 / sqrt(a_i a_j)")
    if polarizability is not None:
        TH.check_polarizability(positions.shape[0], polarizability)
    return 0.0 if thole is None else TH.check_thole(thole)


def _inputs(positions, charges, dipoles, polar, direct_scales, mutual_scales, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts,
            neighbor_matrix, neighbor_matrix_shifts, mask_value, minimum_image, thole):
    lists = (neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts)
    C.require_device(positions, direct_scales, mutual_scales)
    p = P.launch_inputs(positions, charges, cell, batch_idx, lists, int(mask_value), mu=dipoles, pol=polar)
    p["sd"] = None if direct_scales is None else direct_scales.detach().to(F64).contiguous()
    p["sm"] = None if mutual_scales is None else mutual_scales.detach().to(F64).contiguous()
    p["min_image"], p["thole"] = bool(minimum_image), float(thole)
    return p


def _launch(p, flags: int, weights=None, energies: bool = True):
    """One `mi_dipole_scale` launch: float64 (energies | None, forces in the positions dtype | None, charge sums | None, dipole sums | None,
    polarisability sums | None, virial block partials [nsys, blocks, 9] | None)."""
    pos = p["pos"]
    n, dt = pos.shape[0], pos.dtype
    L = C.lib()
    e, f, cg, dg, pg = M.allocate(pos, M.THOLE, (energies, flags & P.FORCES, flags & P.CHARGE_GRAD, flags & P.THIRD_GRAD, flags & P.FOURTH_GRAD))
    nbytes = int(L.mi_dipole_scale_scratch_bytes(n, C.dtype_code(dt)))
    part, scratch = M.pair_scratch(p, flags, int(L.mi_dipole_scale_blocks()), nbytes)
    rc = L.mi_dipole_scale(C.ptr(pos), C.ptr(p["q"]), C.ptr(p["mu"]), C.ptr(p["pol"]), C.ptr(p["cells"]), C.ptr(p["bi"]), C.ptr(weights),
                           C.ptr(p["sd"]), C.ptr(p["sm"]), C.cdouble(p["thole"]), n, int(p["nsys"]), C.dtype_code(dt), C.ptr(p["idx"]),
                           C.ptr(p["sh"]), C.ptr(p["nptr"]), int(p["m"]), p["mask"], int(p["min_image"]), int(flags), C.ptr(e), C.ptr(f),
                           C.ptr(cg), C.ptr(dg), C.ptr(pg), C.ptr(part), C.ptr(scratch), ctypes.c_size_t(nbytes), C.stream_of(pos))
    C.check(rc, "mi_dipole_scale")
    return e, f, cg, dg, pg, part


def _forward(positions, charges, dipoles, polar, direct_scales, mutual_scales, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts,
             neighbor_matrix, neighbor_matrix_shifts, mask_value, minimum_image, thole, forces, cgrads, dgrads, pgrads, virial):
    """(energies, forces | None, charge_grads | None, dipole_grads | None, polarizability_grads | None, virial | None) in the positions dtype, no
    autograd graph: what the eager call and the `alchemiops::_dipole_pair_scale_correction` op both run.  `thole` 0.0: undamped."""
    p = _inputs(positions, charges, dipoles, polar, direct_scales, mutual_scales, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts,
                neighbor_matrix, neighbor_matrix_shifts, mask_value, minimum_image, thole)
    return M.pair_forward(p, _launch, M.THOLE, (True, forces, cgrads, dgrads, pgrads, virial))


def _adjoint(positions, charges, dipoles, polar, direct_scales, mutual_scales, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts,
             neighbor_matrix, neighbor_matrix_shifts, mask_value, minimum_image, thole, grad_energies):
    """Float64 (dL/dpositions, dL/dcharges, dL/ddipoles, dL/dpolarizability) of L = sum_i g_i E_i: the forward kernel with weights."""
    p = _inputs(positions, charges, dipoles, polar, direct_scales, mutual_scales, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts,
                neighbor_matrix, neighbor_matrix_shifts, mask_value, minimum_image, thole)
    return M.pair_adjoint(p, _launch, M.THOLE, grad_energies)


@C.traceable
def dipole_pair_scale_correction(positions: torch.Tensor, charges: torch.Tensor, dipoles: torch.Tensor, direct_scales: torch.Tensor | None,
                                 mutual_scales: torch.Tensor | None, cell: torch.Tensor | None = None, *, polarizability=None,
                                 thole: float | None = None, neighbor_list: torch.Tensor | None = None,
                                 neighbor_ptr: torch.Tensor | None = None, neighbor_shifts: torch.Tensor | None = None,
                                 neighbor_matrix: torch.Tensor | None = None, neighbor_matrix_shifts: torch.Tensor | None = None,
                                 mask_value: int = -1, batch_idx: torch.Tensor | None = None, minimum_image: bool = False,
                                 compute_forces: bool = False, compute_charge_gradients: bool = False, compute_dipole_gradients: bool = False,
                                 compute_polarizability_gradients: bool = False, compute_virial: bool = False):
    """What has to be ADDED to an unscaled charge-dipole and dipole-dipole total so that every listed pair carries its direct scale s^d on the
    charge-dipole term and its mutual scale s^m on the dipole-dipole term, Thole-damped when `thole` is given.  For every stored entry
    e = (i, j[, S]), with R, r, B1 = 1 / r^3, B2 = 3 / r^5 of `pair_scale_correction`, c_i = mu_i . R and l3, l5 EXACTLY the damping factors of
    `thole_dipole_correction` (l = 1 when `thole` is None, when either end has a <= 0 or NaN, and for E >= 50):

        E_i = 1/2 sum_row [ (s^d_e - 1) l3 B1 (q_j c_i - q_i c_j)  +  (s^m_e - 1) (l3 B1 mu_i . mu_j - l5 B2 c_i c_j) ]

    The unscaled total is `*_dipole_correction` (Ewald, mesh or cluster) plus `thole_dipole_correction` when damped.  Charge-charge and
    quadrupole terms are not touched: `pair_scale_correction` stays the operator for those.

    `direct_scales` and `mutual_scales` have the shape of the index array, are float32 or float64 and are not differentiable
    (`requires_grad` raises NotImplementedError); either may be None, meaning all 1; both None is a ValueError.  An entry with both factors
    equal to 1 is skipped before any arithmetic and contributes exact zeros.  `thole` without `polarizability` ([N], or a number) is a
    ValueError.  THE LIST MUST BE FULL AND THE SCALES SYMMETRIC; padding, the r <= 1e-8 skip, the `cell=None` cluster rules, the
    `minimum_image` rules and the error messages are those of `pair_scale_correction`.

    Returns ``energies`` [N], or a tuple holding only what was asked for, in this order: energies, forces [N, 3], charge_grads [N],
    dipole_grads [N, 3], polarizability_grads [N] (dE/da; zeros without `thole`), virial [num_systems, 3, 3]; all in the positions dtype with
    float64 sums.  Minus dipole_grads at mu = 0 is the scaled, damped direct field that the listed pairs add.

    Energies are differentiable once w.r.t. positions, charges, dipoles and polarizability (the same launch with per-atom weights is the
    adjoint); the call then goes through the `alchemiops::_dipole_pair_scale_correction` op, as it does under `torch.compile`.
    Differentiating the explicit outputs raises NotImplementedError, and so does a gradient w.r.t. cell: use `compute_virial`.  The
    `scaled_induced_dipoles` takes the same pairs as `scaled_pairs=PolarizationPairScales(...)`; the forces of such a step are the existing
    corrections plus this one with `compute_forces=True` at the solved dipoles.  Out of scope: per-pair Thole widths, separate p / d dipole
    sets, dE/ds, quadrupole damping.  CPU tensors raise NativeLibraryError: there is no fallback."""
    thole = _check(positions, charges, dipoles, direct_scales, mutual_scales, cell, polarizability, thole, neighbor_list, neighbor_ptr,
                   neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, batch_idx, minimum_image, compute_virial)
    n, dev, dt = positions.shape[0], positions.device, positions.dtype
    want = (True, compute_forces, compute_charge_gradients, compute_dipole_gradients, compute_polarizability_gradients, compute_virial)
    if n == 0:
        return M.no_atoms(positions, M.num_systems(cell, batch_idx), M.THOLE, want)
    polar = TH._polar_tensor(0.0 if polarizability is None else polarizability, n, dt, dev)
    return M.dispatch("dipole_pair_scale_correction_op", _forward, (positions, charges, dipoles, polar), (direct_scales, mutual_scales, cell),
                      (batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, int(mask_value),
                       bool(minimum_image), thole), want)


# ---- the mutual part as a stored operator of the induced-dipole solvers ----------------------------------------------------------------------
class ScaledOperator:
    """The bonded pairs of one geometry inside H: `mi_scaled_dipole_tensors` once, `mi_scaled_dipole_apply` per product."""

    def __init__(self, scaled_pairs, pos, polar, cells, bi, nsys, thole):
        nm, sd, sm = scaled_pairs
        n, dev = pos.shape[0], pos.device
        C.require_device(nm, sd, sm)
        self.matrix, self.direct, self.mutual = nm, sd, sm
        self.n, self.m = n, int(nm.shape[1])
        self.slots = n * self.m
        self.active = sm is not None and self.slots > 0  # without mutual scales H is unchanged: only b and the energy gain a term
        if not self.active:
            return
        L = C.lib()
        idx, smut = C.i32(nm), sm.detach().to(F64).contiguous()
        self.tensors = torch.empty((int(L.mi_scaled_dipole_tensor_words()), self.slots), dtype=F64, device=dev)
        self.nbr = torch.empty(self.slots, dtype=torch.int32, device=dev)
        rc = L.mi_scaled_dipole_tensors(C.ptr(pos), C.ptr(polar), C.ptr(cells), C.ptr(bi), C.ptr(smut), C.cdouble(0.0 if thole is None else thole),
                                        n, int(nsys), C.dtype_code(pos.dtype), C.ptr(idx), self.m, n, self.slots, C.ptr(self.tensors),
                                        C.ptr(self.nbr), C.stream_of(pos))
        C.check(rc, "mi_scaled_dipole_tensors")

    def apply(self, x, y_in=None):
        """y_in + (the bonded operator) x, float64 [N, 3]; `y_in` itself when there are no mutual scales."""
        if not self.active:
            return y_in
        y = torch.empty((self.n, 3), dtype=F64, device=x.device)
        rc = C.lib().mi_scaled_dipole_apply(C.ptr(self.tensors), C.ptr(self.nbr), C.ptr(x), C.ptr(y_in), self.n, self.m, self.slots, C.ptr(y),
                                            C.stream_of(x))
        C.check(rc, "mi_scaled_dipole_apply")
        return y


def check_scaled_pairs(scaled_pairs, n):
    """Argument errors of `scaled_induced_dipoles(scaled_pairs=)`, before anything is launched."""
    if not isinstance(scaled_pairs, tuple) or len(scaled_pairs) != 3:
        raise TypeError("scaled_pairs must be a PolarizationPairScales(neighbor_matrix, direct_scales, mutual_scales)")
    nm, sd, sm = scaled_pairs
    if not isinstance(nm, torch.Tensor) or nm.dim() != 2 or nm.shape[0] != n:
        raise ValueError(f"scaled_pairs.neighbor_matrix must have shape [{n}, M] (the matrix format `bonded_pair_scales` produces)")
    if sd is None and sm is None:
        raise ValueError("direct_scales and mutual_scales are both None: nothing is scaled")
    _check_scales("direct_scales", sd, tuple(nm.shape))
    _check_scales("mutual_scales", sm, tuple(nm.shape))


__all__ = ["dipole_pair_scale_correction", "PolarizationPairScales"]
