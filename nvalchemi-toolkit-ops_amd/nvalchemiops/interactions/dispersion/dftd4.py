"""DFT-D4 dispersion: the two-body term `dftd4`, with a C6 that depends on each atom's coordination number and partial charge, and the
three-body (Axilrod-Teller-Muto) term `dftd4_atm`, whose C6 is the same contraction at zero charge.

The reference package has no counterpart (its dispersion is DFT-D3(BJ), two-body).  Energies [num_systems], forces [N,3], coordination
numbers [N], dE/dq [N] and (optionally) virials [num_systems,3,3], all float32, from a FULL neighbour list given either as a padded
neighbour matrix or as CSR, exactly as for `dftd3`.  The passes (pack, CN, weights, energy, chain, fold) are hand-written HIP kernels
(csrc/d4.hip) behind `mi_d4` of the C ABI; the model they evaluate is stated in include/nvalchemiops_hip.h and in `dftd4`'s docstring.
`dftd4_atm` (`mi_d4_atm`, csrc/d4_atm.h) reuses those passes around one triple kernel and returns its term alone, to be added.
No element tables ship with the package: like the c6 tables of `dftd3` they are the caller's (`D4Parameters`).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import torch

from nvalchemiops import _capi as C
from nvalchemiops.interactions.dispersion import _call as K

_FLOAT_TYPES = K.FLOAT_TYPES
_INT_TYPES = (torch.int32, torch.int64)
N_REF = 7  # references per element the tables hold
K4, K5, K6 = 4.10451, 19.08857, 2.0 * 11.28174 ** 2  # the electronegativity factor of the D4 covalent coordination number
_INT_TABLES, _TABLES = K.D4_INT_TABLES, K.D4_TABLES


@dataclass
class D4Parameters:
    """Validated container of the D4 element tables, all indexed by atomic number (index 0 = padding):

    ``rcov[Z+1]`` covalent radii as the coordination number uses them (any 4/3 scaling is the caller's), ``en[Z+1]`` electronegativities,
    ``r4r2[Z+1]``, ``zeff[Z+1]`` effective nuclear charges, ``gam[Z+1]`` chemical hardnesses (float32 or float64);
    ``n_ref[Z+1]`` number of references per element, 0 ... 7 (0: the element is padding), ``ngw[Z+1,7]`` Gaussian weights per reference,
    1 ... 3 (int32 or int64); ``cn_ref[Z+1,7]``, ``q_ref[Z+1,7]`` reference coordination numbers and charges, ``c6_ref[Z+1,Z+1,7,7]`` with
    ``c6_ref[A,B,a,b] == c6_ref[B,A,b,a]`` (float).  Entries with reference index >= n_ref[Z] are never used, whatever they hold.
    Exception types are `D3Parameters`': TypeError for a non-tensor or a wrong dtype, ValueError for shapes and mixed devices."""

    rcov: torch.Tensor
    en: torch.Tensor
    r4r2: torch.Tensor
    zeff: torch.Tensor
    gam: torch.Tensor
    n_ref: torch.Tensor
    ngw: torch.Tensor
    cn_ref: torch.Tensor
    q_ref: torch.Tensor
    c6_ref: torch.Tensor

    def __post_init__(self) -> None:
        named = {k: getattr(self, k) for k in _TABLES}
        for name, value in named.items():
            if not isinstance(value, torch.Tensor):
                raise TypeError(f"Parameter '{name}' must be a torch.Tensor, got {type(value)}")
            if name in _INT_TABLES:
                if value.dtype not in _INT_TYPES:
                    raise TypeError(f"Parameter '{name}' must be int32 or int64, got {value.dtype}")
            elif value.dtype not in _FLOAT_TYPES:
                raise TypeError(f"Parameter '{name}' must be float32 or float64, got {value.dtype}")
        if self.rcov.ndim != 1:
            raise ValueError(f"rcov must be 1D tensor [max_Z+1], got shape {self.rcov.shape}")
        nz = self.rcov.size(0)
        if nz < 2:
            raise ValueError(f"rcov must have at least 2 elements (padding + 1 element), got {nz}")
        for name in ("en", "r4r2", "zeff", "gam", "n_ref"):
            if tuple(named[name].shape) != (nz,):
                raise ValueError(f"{name} must have shape [{nz}] to match rcov, got {tuple(named[name].shape)}")
        for name in ("ngw", "cn_ref", "q_ref"):
            if tuple(named[name].shape) != (nz, N_REF):
                raise ValueError(f"{name} must have shape {(nz, N_REF)}, got {tuple(named[name].shape)}")
        if tuple(self.c6_ref.shape) != (nz, nz, N_REF, N_REF):
            raise ValueError(f"c6_ref must have shape {(nz, nz, N_REF, N_REF)}, got {tuple(self.c6_ref.shape)}")
        if len({str(v.device) for v in named.values()}) > 1:
            raise ValueError("All parameters must be on the same device. Got devices: " + ", ".join(f"{k}={v.device}" for k, v in named.items()))

    @property
    def max_z(self) -> int:
        return self.rcov.size(0) - 1

    @property
    def device(self) -> torch.device:
        return self.rcov.device

    def to(self, device: str | torch.device | None = None, dtype: torch.dtype | None = None) -> "D4Parameters":
        """Moves every table; `dtype` applies to the floating-point tables only."""
        out = {}
        for k in _TABLES:
            t = getattr(self, k)
            out[k] = t.to(device=device) if k in _INT_TABLES else t.to(device=device, dtype=dtype)
        return D4Parameters(**out)


def species_slots() -> int:
    """Distinct species of one call whose contracted C6 vectors the energy pass holds in LDS at once; with more species present it walks
    each row once per group of that many (slower, same results)."""
    return int(C.lib().mi_d4_species_slots())


def _launch(positions, numbers, charges, idx, shifts, nptr, max_neighbors, fill_value, cell, batch_idx, num_systems, tables, scalars, compute_virial,
            energy, forces, coord_num, charge_grad, virial) -> None:
    """One `mi_d4` call on the caller's arrays.  `tables`: the ten tensors in `D4Parameters` order; `scalars`: the floats of `mi_d4_params`."""
    n = positions.shape[0]
    pos, code, z, cell_t, sh, bi = K.prelude(positions, numbers, shifts, cell, batch_idx)
    par, keep = K.d4_struct(pos.device, tables, scalars)
    L = C.lib()
    if not hasattr(L, "mi_d4"):
        raise C.NativeLibraryError("libnvalchemiops_hip.so does not export mi_d4: rebuild it (build_native.py)")
    q = K.f32_on(charges, pos.device)
    ws_bytes = int(L.mi_d4_workspace_bytes(n, int(num_systems), par.nz))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pos.device)
    rc = L.mi_d4(C.ptr(pos), C.ptr(z), n, code, C.ptr(idx), C.ptr(sh), C.ptr(nptr), int(max_neighbors),
                 ctypes.c_longlong(idx.shape[0] if nptr is not None else 0), int(fill_value), C.ptr(cell_t), C.ptr(bi), int(num_systems),
                 ctypes.byref(par), C.ptr(q), int(bool(compute_virial)), C.ptr(energy), C.ptr(forces), C.ptr(coord_num), C.ptr(charge_grad),
                 C.ptr(virial if compute_virial else None), C.ptr(ws), ctypes.c_size_t(ws_bytes), C.stream_of(pos))
    C.check(rc, "mi_d4")


def d4_scalars(a1, a2, s6, s8, k_cn, wf, ga, gc, cn_cutoff):
    """The floats of `mi_d4_params` (cn_cutoff None -> 0: every stored entry counts)."""
    return dict(a1=a1, a2=a2, s6=s6, s8=s8, k_cn=k_cn, k4=K4, k5=K5, k6=K6, wf=wf, ga=ga, gc=gc, cn_cutoff=0.0 if cn_cutoff is None else cn_cutoff)


def _check_d4(d4_params, neighbor_matrix, neighbor_matrix_shifts, neighbor_list, neighbor_ptr, unit_shifts, cell, compute_virial, missing_functional,
              positions, numbers, batch_idx, num_systems):
    """Argument validation of `dftd4` / `dftd4_atm`, in the order a caller meets it: a `d4_params` dictionary goes through `D4Parameters`
    first; then `dftd3`'s list-format checks; then the missing tables; then the per-atom / neighbour data.  Returns (use_matrix, the ten
    tables in `D4Parameters` order)."""
    if d4_params is not None and not isinstance(d4_params, D4Parameters):
        d4_params = D4Parameters(**{k: d4_params[k] for k in _TABLES})
    use_matrix = K.check_lists(neighbor_matrix, neighbor_matrix_shifts, neighbor_list, neighbor_ptr, unit_shifts, cell, compute_virial,
                               missing_functional)
    if d4_params is None:
        raise RuntimeError("DFT-D4 parameters must be explicitly provided: pass d4_params, a D4Parameters instance or a dictionary with its "
                           "ten tables (rcov, en, r4r2, zeff, gam, n_ref, ngw, cn_ref, q_ref, c6_ref).")
    K.check_atoms(positions, numbers, batch_idx, num_systems, neighbor_matrix, neighbor_matrix_shifts, neighbor_list, neighbor_ptr, unit_shifts,
                  cell)
    return use_matrix, tuple(getattr(d4_params, k) for k in _TABLES)


@C.hybrid
def dftd4(positions: torch.Tensor, numbers: torch.Tensor, charges: torch.Tensor, a1: float, a2: float, s8: float, s6: float = 1.0, *,
          d4_params: D4Parameters | dict[str, torch.Tensor] | None = None, cn_cutoff: float | None = None, wf: float = 6.0, ga: float = 3.0,
          gc: float = 2.0, k_cn: float = 7.5, fill_value: int | None = None, batch_idx: torch.Tensor | None = None,
          cell: torch.Tensor | None = None, neighbor_matrix: torch.Tensor | None = None, neighbor_matrix_shifts: torch.Tensor | None = None,
          neighbor_list: torch.Tensor | None = None, neighbor_ptr: torch.Tensor | None = None, unit_shifts: torch.Tensor | None = None,
          compute_virial: bool = False, num_systems: int | None = None):
    """Two-body DFT-D4 dispersion with Becke-Johnson damping: returns ``(energy[num_systems], forces[N,3], coord_num[N],
    charge_gradients[N])`` (+ ``virial[num_systems,3,3]`` if ``compute_virial``), all float32, on its own, the way `dftd3` returns its term.

    Over the entries (i, j, S) of a FULL list (every pair stored in both rows), r = r_j - r_i + S . cell, Z = ``numbers``::

        CN_i    = sum_row delta(Z_i,Z_j) 1/2 (1 + erf(-k_cn (r / (rcov_i + rcov_j) - 1)))
        delta   = k4 exp(-(|en_i - en_j| + k5)^2 / k6)                  k4 = 4.10451, k5 = 19.08857, k6 = 2 * 11.28174^2
        g_a     = sum_{s=1..ngw_a} exp(-wf s (CN_i - cn_ref_a)^2),   W_a = g_a / sum_b g_b
        zeta_a  = exp(ga (1 - exp(gc gam[Z] (1 - (zeff[Z] + q_ref_a) / (zeff[Z] + q_i)))))   if zeff[Z] + q_i > 0, else exp(ga)
        C6_ij   = sum_ab W_a zeta_a c6_ref[Z_i,Z_j,a,b] W_b zeta_b
        E       = 1/2 sum_entries -C6_ij (s6 / (r^6 + R0^6) + s8 Q / (r^8 + R0^8)),   Q = 3 r4r2_i r4r2_j,  R0 = a1 sqrt(Q) + a2

    ``charges`` [N] (float32 or float64; the kernels read float32) are the atomic partial charges, e.g. those of `charge_equilibration`.
    ``cn_cutoff``: entries with r >= cn_cutoff do not count for the coordination numbers (a hard cut, as in dftd4); None: every stored
    entry counts.  Atoms with Z <= 0, Z > max_Z or an element with ``n_ref = 0`` are padding: part of no pair and of no coordination
    number, their force, coordination number and charge gradient are 0.  Entries with r <= 1e-8 contribute nothing.  The Gaussian weights
    are evaluated with the largest exponent subtracted, so a coordination number far from every reference gives weights that sum to 1,
    not 0/0.

    ``forces`` are those at FIXED charges and include the path through the coordination numbers; ``charge_gradients`` is dE/dq_i.  With
    charges that depend on the positions the total force is ``forces - sum_i charge_gradients_i dq_i/dr``, which autograd assembles: if
    ``positions`` or ``charges`` require grad, ``energy`` carries a hand-written first-order adjoint (grad_positions = -g[batch] forces,
    grad_charges = g[batch] charge_gradients, in the inputs' dtypes); differentiating twice raises.  Gradients with respect to ``cell``
    are out of scope (use ``virial``).  Under ``torch.compile`` the call is one mutating custom op per layout (``nvalchemiops::dftd4_nm`` /
    ``::dftd4_nl``); there is no autograd on that path.

    List layouts, argument validation and its messages, ``num_systems`` inference and the empty-input contract are `dftd3`'s.  CPU tensors
    raise ``NativeLibraryError``: there is no fallback.

    D4's three-body term is `dftd4_atm` (charge-free C6 values: it cannot go through `dftd3_atm`); every published D4 parametrisation is
    fitted with it switched on (s9 = 1), so a DFT-D4 energy is the sum of the two.  Out of scope: the neighbour search's packed companion
    and search-side coordination numbers, zero damping, and element tables (`D4Parameters` holds the caller's)."""
    missing = None
    if a1 is None or a2 is None or s8 is None:
        missing = ("Functional parameters a1, a2, and s8 must be provided. "
                   "These are functional-dependent parameters required for DFT-D4 calculations.")
    use_matrix, tables = _check_d4(d4_params, neighbor_matrix, neighbor_matrix_shifts, neighbor_list, neighbor_ptr, unit_shifts, cell, compute_virial,
                                   missing, positions, numbers, batch_idx, num_systems)
    n = positions.size(0)
    if not isinstance(charges, torch.Tensor):
        raise TypeError(f"charges must be a torch.Tensor, got {type(charges)}")
    if charges.dtype not in _FLOAT_TYPES:
        raise TypeError(f"charges must be float32 or float64, got {charges.dtype}")
    if charges.dim() != 1 or charges.shape[0] != n:
        raise ValueError(f"charges must have one entry per atom: expected shape [{n}], got {tuple(charges.shape)}")
    if n == 0:
        return K.empty_result(positions, batch_idx, 2, compute_virial)
    num_systems = K.infer_num_systems(num_systems, batch_idx, cell)
    out = energy, forces, coord_num, charge_grad, virial = K.allocate(positions, num_systems, 2, compute_virial)
    result = K.select(out, compute_virial)
    if C.tracing():  # torch.compile: one mutating custom op per call, as for `dftd3`; no autograd on this path
        if use_matrix:
            torch.ops.nvalchemiops.dftd4_nm(positions, numbers, charges, neighbor_matrix, *tables, a1, a2, s8, energy, forces, coord_num,
                                            charge_grad, virial, s6, cn_cutoff, wf, ga, gc, k_cn, fill_value, batch_idx, cell,
                                            neighbor_matrix_shifts, compute_virial)
        else:
            torch.ops.nvalchemiops.dftd4_nl(positions, numbers, charges, neighbor_list[1], neighbor_ptr, *tables, a1, a2, s8, energy, forces,
                                            coord_num, charge_grad, virial, s6, cn_cutoff, wf, ga, gc, k_cn, batch_idx, cell, unit_shifts,
                                            compute_virial)
        return result
    C.require_device(positions, numbers, charges, neighbor_matrix, neighbor_list, neighbor_ptr, batch_idx)

    def run():
        lists = K.list_args(n, neighbor_matrix, neighbor_matrix_shifts, fill_value, neighbor_list, neighbor_ptr, unit_shifts)
        _launch(positions, numbers, charges, *lists, cell, batch_idx, num_systems, tables, d4_scalars(a1, a2, s6, s8, k_cn, wf, ga, gc, cn_cutoff),
                compute_virial, *out)
        return result

    if torch.is_grad_enabled() and (positions.requires_grad or charges.requires_grad):
        return K.EnergyAdjoint.apply(positions, charges, batch_idx, run)
    return run()


def atm_tile() -> int:
    """Neighbours inside ``three_body_cutoff`` a row may have before the triple pass of `dftd4_atm` works tile by tile."""
    return int(C.lib().mi_d4_atm_tile())


def _launch_atm(positions, numbers, idx, shifts, nptr, max_neighbors, fill_value, cell, batch_idx, num_systems, tables, scalars, s9, alpha,
                three_body_cutoff, compute_virial, energy, forces, virial, want_visits=False):
    """One `mi_d4_atm` call on the caller's arrays (`tables`, `scalars`: as for `_launch`; s6 / s8 are not read).  `want_visits`: return the
    per-centre triangle-visit counts the triple pass leaves in its workspace (a diagnostic for tools/d4_atm_bench.py)."""
    n = positions.shape[0]
    pos, code, z, cell_t, sh, bi = K.prelude(positions, numbers, shifts, cell, batch_idx)
    par, keep = K.d4_struct(pos.device, tables, scalars)
    L = C.lib()
    if not hasattr(L, "mi_d4_atm"):
        raise C.NativeLibraryError("libnvalchemiops_hip.so does not export mi_d4_atm: rebuild it (build_native.py)")
    ws_bytes = int(L.mi_d4_atm_workspace_bytes(n, int(num_systems), par.nz))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pos.device)
    rc = L.mi_d4_atm(C.ptr(pos), C.ptr(z), n, code, C.ptr(idx), C.ptr(sh), C.ptr(nptr), int(max_neighbors), int(fill_value), C.ptr(cell_t),
                     C.ptr(bi), int(num_systems), ctypes.byref(par), float(s9), float(alpha), float(three_body_cutoff), int(bool(compute_virial)),
                     C.ptr(energy), C.ptr(forces), C.ptr(virial if compute_virial else None), C.ptr(ws), ctypes.c_size_t(ws_bytes),
                     C.stream_of(pos))
    C.check(rc, "mi_d4_atm")
    if want_visits:
        off = int(L.mi_d4_atm_visits_offset(n, int(num_systems), par.nz))
        return ws[off:off + 4 * n].view(torch.int32).clone()
    return None


@C.hybrid
def dftd4_atm(positions: torch.Tensor, numbers: torch.Tensor, a1: float, a2: float, three_body_cutoff: float, s9: float = 1.0,
              alpha: float = 16.0, *, d4_params: D4Parameters | dict[str, torch.Tensor] | None = None, cn_cutoff: float | None = None,
              wf: float = 6.0, ga: float = 3.0, gc: float = 2.0, k_cn: float = 7.5, fill_value: int | None = None,
              batch_idx: torch.Tensor | None = None, cell: torch.Tensor | None = None, neighbor_matrix: torch.Tensor | None = None,
              neighbor_matrix_shifts: torch.Tensor | None = None, neighbor_list: torch.Tensor | None = None,
              neighbor_ptr: torch.Tensor | None = None, unit_shifts: torch.Tensor | None = None, compute_virial: bool = False,
              num_systems: int | None = None):
    """Three-body (Axilrod-Teller-Muto) dispersion of DFT-D4: returns ``(energy[num_systems], forces[N,3])`` (+ ``virial[num_systems,3,3]``
    if ``compute_virial``) of the three-body term ALONE, float32, in the units and the virial convention of `dftd4`, so that a caller adds
    them to `dftd4`'s outputs.

    For every unordered triple of distinct atom images A, B, C whose three distances are all ``< three_body_cutoff``::

        E_ABC  = s9 sqrt(C6_AB C6_AC C6_BC) ang fdamp
        ang    = 0.375 (a+b-c)(a+c-b)(b+c-a)/P^5 + 1/P^3           a, b, c squared sides, P product of the sides
        fdamp  = 1 / (1 + 6 (R0_AB R0_AC R0_BC / P)^(alpha/3))     R0_XY = a1 sqrt(3 r4r2_X r4r2_Y) + a2
        C6_XY  = sum_ab w_X[a] c6_ref[Z_X,Z_Y,a,b] w_Y[b]          w_X[a] = W_a(CN_X) zeta_a(q = 0)

    ``W_a``, ``zeta_a``, the coordination number (erf count, electronegativity factor, optional hard ``cn_cutoff``) and the padding rules
    (Z <= 0, Z > max_Z, ``n_ref[Z] = 0``; table entries beyond ``n_ref`` are never read) are exactly `dftd4`'s.  The charge scaling is
    evaluated at q = 0 for every atom -- D4's definition of the term -- so there is no ``charges`` argument and no dE/dq output; note that
    zeta_a(0) is not 1: it still depends on ``q_ref``, ``zeff``, ``gam``, ``ga`` and ``gc``.  The coordination numbers are summed over ALL
    stored entries of the list (subject to ``cn_cutoff``); entries beyond ``three_body_cutoff`` only count for them.  A triple with any
    C6 < 1e-12 contributes nothing.  A triple counts once per unit cell; forces include the path through the coordination numbers.

    Requirements on the list: it is a FULL list (every pair stored in both rows) and its cutoff is at least ``three_body_cutoff``.  A
    periodic list may hold an atom's own images and several images of one neighbour: those are distinct vertices.

    Validation order and messages, list layouts, ``num_systems`` inference and the empty-input contract are `dftd4`'s.  CPU tensors raise
    ``NativeLibraryError``: there is no fallback.  If ``positions`` requires grad, ``energy`` carries the same hand-written first-order
    adjoint as `dftd4` (grad_positions = -g[batch] forces, in the input's dtype); differentiating twice raises.  Gradients with respect to
    ``cell`` are out of scope (use ``virial``).  Under ``torch.compile`` the call is one mutating custom op per layout
    (``nvalchemiops::dftd4_atm_nm`` / ``::dftd4_atm_nl``); there is no autograd on that path.

    Out of scope: a charge-dependent three-body C6 and its dE/dq, zero damping, the packed companion and element tables."""
    if a1 is None or a2 is None:
        missing = ("Functional parameters a1 and a2 must be provided. "
                   "These are functional-dependent parameters required for DFT-D4 calculations.")
    else:
        missing = K.three_body_missing(three_body_cutoff, alpha)
    use_matrix, tables = _check_d4(d4_params, neighbor_matrix, neighbor_matrix_shifts, neighbor_list, neighbor_ptr, unit_shifts, cell, compute_virial,
                                   missing, positions, numbers, batch_idx, num_systems)
    if positions.size(0) == 0:
        return K.empty_result(positions, batch_idx, 0, compute_virial)
    num_systems = K.infer_num_systems(num_systems, batch_idx, cell)
    out = energy, forces, virial = K.allocate(positions, num_systems, 0, compute_virial)
    result = K.select(out, compute_virial)
    if C.tracing():  # torch.compile: one mutating custom op per call, as for `dftd3`; no autograd on this path
        if use_matrix:
            torch.ops.nvalchemiops.dftd4_atm_nm(positions, numbers, neighbor_matrix, *tables, a1, a2, three_body_cutoff, energy, forces, virial,
                                                s9, alpha, cn_cutoff, wf, ga, gc, k_cn, fill_value, batch_idx, cell, neighbor_matrix_shifts,
                                                compute_virial)
        else:
            torch.ops.nvalchemiops.dftd4_atm_nl(positions, numbers, neighbor_list[1], neighbor_ptr, *tables, a1, a2, three_body_cutoff, energy,
                                                forces, virial, s9, alpha, cn_cutoff, wf, ga, gc, k_cn, batch_idx, cell, unit_shifts,
                                                compute_virial)
        return result
    C.require_device(positions, numbers, neighbor_matrix, neighbor_list, neighbor_ptr, batch_idx)

    def run():
        lists = K.list_args(positions.size(0), neighbor_matrix, neighbor_matrix_shifts, fill_value, neighbor_list, neighbor_ptr, unit_shifts)
        _launch_atm(positions, numbers, *lists, cell, batch_idx, num_systems, tables, d4_scalars(a1, a2, 0.0, 0.0, k_cn, wf, ga, gc, cn_cutoff),
                    s9, alpha, three_body_cutoff, compute_virial, *out)
        return result

    if torch.is_grad_enabled() and positions.requires_grad:
        return K.EnergyAdjoint.apply(positions, None, batch_idx, run)
    return run()


__all__ = ["D4Parameters", "atm_tile", "dftd4", "dftd4_atm", "species_slots"]
