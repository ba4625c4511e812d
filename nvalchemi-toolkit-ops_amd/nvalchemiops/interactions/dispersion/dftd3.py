"""DFT-D3(BJ) dispersion: the two-body term `dftd3` -- drop-in for interactions/dispersion/dftd3.py of the reference
(`D3Parameters` :146-332, `dftd3` :2468-2874; ops `nvalchemiops::dftd3_nm` :1792, `::dftd3_nl` :2125).

Energies [num_systems], forces [N,3], coordination numbers [N] and (optionally) virials [num_systems,3,3], all
float32, from a FULL neighbour list given either as a padded neighbour matrix or as CSR (`neighbor_list[1]` +
`neighbor_ptr`).  The three passes (CN; C6 interpolation + BJ damping + energy + direct force + dE/dCN; chain-rule
force) run as hand-written HIP kernels (csrc/d3.hip) behind `mi_d3` of the C ABI.  As in the reference, positions
and cell are detached: explicit forces are returned, there is no autograd through D3.

`dftd3_zero` is `dftd3` with the zero damping of the original D3 parametrisation, D3(0) / D3M(0), instead of the Becke-Johnson one
(`mi_d3_zero`: the same three passes with another damping block in the energy pass; the pair cutoff radii are a table the caller supplies).

`dftd3_zero_atm` is `dftd3_atm` with the radii of that table (`mi_d3_zero_atm`).

`dftd3_atm` adds what the reference leaves out ("Two-body only", dftd3.py:119): the three-body Axilrod-Teller-Muto term, returned on its
own so that a caller adds it to `dftd3`'s outputs (`mi_d3_atm`, csrc/d3_atm.h).
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass

import torch

from nvalchemiops import _capi as C
from nvalchemiops.interactions.dispersion import _call as K

_FLOAT_TYPES = K.FLOAT_TYPES


@dataclass
class D3Parameters:
    """Validated container of the element tables: ``rcov[Z+1]``, ``r4r2[Z+1]``, ``c6ab[Z+1,Z+1,m,m]``, ``cn_ref[Z+1,Z+1,m,m]``
    (index 0 = padding, ``m = interp_mesh = 5``).  Same checks and exception types as dftd3.py:221-280."""

    rcov: torch.Tensor
    r4r2: torch.Tensor
    c6ab: torch.Tensor
    cn_ref: torch.Tensor
    interp_mesh: int = 5

    def __post_init__(self) -> None:
        named = {"rcov": self.rcov, "r4r2": self.r4r2, "c6ab": self.c6ab, "cn_ref": self.cn_ref}
        for name, value in named.items():
            if not isinstance(value, torch.Tensor):
                raise TypeError(f"Parameter '{name}' must be a torch.Tensor, got {type(value)}")
            if value.dtype not in _FLOAT_TYPES:
                raise TypeError(f"Parameter '{name}' must be float32 or float64, got {value.dtype}")
        if self.rcov.ndim != 1:
            raise ValueError(f"rcov must be 1D tensor [max_Z+1], got shape {self.rcov.shape}")
        nz = self.rcov.size(0)
        if nz < 2:
            raise ValueError(f"rcov must have at least 2 elements (padding + 1 element), got {nz}")
        if self.r4r2.shape != (nz,):
            raise ValueError(f"r4r2 must have shape [{nz}] to match rcov, got {self.r4r2.shape}")
        grid = (nz, nz, self.interp_mesh, self.interp_mesh)
        if self.c6ab.shape != grid:
            raise ValueError(f"c6ab must have shape {grid}, got {self.c6ab.shape}")
        if self.cn_ref.shape != grid:
            raise ValueError(f"cn_ref must have shape {grid}, got {self.cn_ref.shape}")
        if len({str(v.device) for v in named.values()}) > 1:
            raise ValueError("All parameters must be on the same device. Got devices: "
                             + ", ".join(f"{k}={v.device}" for k, v in named.items()))

    @property
    def max_z(self) -> int:
        return self.rcov.size(0) - 1

    @property
    def device(self) -> torch.device:
        return self.rcov.device

    def to(self, device: str | torch.device | None = None, dtype: torch.dtype | None = None) -> "D3Parameters":
        mv = lambda t: t.to(device=device, dtype=dtype)  # noqa: E731
        return D3Parameters(rcov=mv(self.rcov), r4r2=mv(self.r4r2), c6ab=mv(self.c6ab), cn_ref=mv(self.cn_ref),
                            interp_mesh=self.interp_mesh)


_LIB_OVERRIDE = None  # tests only: a ctypes handle of the IEEE-arithmetic build of d3.hip (error budget, tests/test_d3_gpu.py)


def _launch(positions, numbers, idx, shifts, nptr, max_neighbors, fill_value, cell, batch_idx, num_systems, tables, scalars,
            compute_virial, energy, forces, coord_num, virial, packed=None, zero=None) -> None:
    """`zero`: None (BJ damping, `mi_d3*`) or (rs6, rs8, alpha, beta, cutoff_radii[nz,nz]) for the zero damping (`mi_d3_zero*`; scalars' a1 / a2
    are then ignored).
    `packed`: the companion record the neighbour search left next to (idx, shifts) (`neighborlist/_engine.py`: `.words`, and `.cn` when the
    search also summed the coordination numbers), already validated by the caller against tensor identity / versions; the passes then stream
    4 B/slot (`mi_d3_packed_cn`), the CN pass is skipped when the device-side fingerprint check lets the search's numbers in, and every call
    re-derives a rotating sample of the companion's rows from (idx, shifts) on the device before trusting it."""
    n = positions.shape[0]
    pos, code, z, cell_t, sh, bi = K.prelude(positions, numbers, shifts, cell, batch_idx)
    par, keep = K.d3_struct(pos.device, tables, scalars)
    zargs, tag = (), ""
    if zero is not None:
        r0ab = K.f32_on(zero[4], pos.device)  # stays referenced until the launch is enqueued, like the other tables
        zpar = C.MiD3ZeroParams(rs6=float(zero[0]), rs8=float(zero[1]), alpha=float(zero[2]), beta=float(zero[3]), r0ab=r0ab.data_ptr())
        zargs, tag = (ctypes.byref(zpar),), "_zero"
    periodic = sh is not None
    # a periodic padded matrix is streamed by all three passes: the larger workspace lets the CN pass leave a 4 B/slot copy for the others
    # NVALCHEMIOPS_D3_PACKED_LIST: "1" (default) padded matrix only; "0" never (A/B on one box); "2" also CSR lists -- measured neutral
    # there (unaligned rows make the CN pass's extra write cost what the other two passes gain), so it is not the default
    mode = os.environ.get("NVALCHEMIOPS_D3_PACKED_LIST", "1")
    pack = periodic and mode != "0" and (nptr is None or mode == "2")
    n_entries = (idx.shape[0] if nptr is not None else n * int(max_neighbors)) if pack else 0
    L = _LIB_OVERRIDE or C.lib()
    if zero is not None and not hasattr(L, "mi_d3_zero"):
        raise C.NativeLibraryError("libnvalchemiops_hip.so does not export mi_d3_zero: rebuild it (build_native.py)")
    ws_bytes = int(C.lib().mi_d3_workspace_bytes_entries(n, num_systems, par.nz, int(n_entries)))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pos.device)
    vir = virial if compute_virial else None
    if packed is not None and periodic and nptr is None and mode != "0":
        from nvalchemiops.neighborlist import _engine as E

        words = packed.words
        cn = packed.cn if os.environ.get("NVALCHEMIOPS_D3_SEARCH_CN", "1") != "0" else None  # (A/B switch: "0" ignores the search's coordination numbers)
        stride, phase = E.verify_args()
        fn = L.mi_d3_packed_cn if zero is None else L.mi_d3_zero_packed_cn
        rc = fn(C.ptr(pos), C.ptr(z), n, code, C.ptr(idx), C.ptr(sh), int(max_neighbors), int(fill_value), C.ptr(cell_t), C.ptr(bi),
                int(num_systems), ctypes.byref(par), *zargs, int(bool(compute_virial)), C.ptr(energy), C.ptr(forces), C.ptr(coord_num),
                C.ptr(vir), C.ptr(ws), ctypes.c_size_t(ws_bytes), C.ptr(words), ctypes.c_size_t(words.numel() * words.element_size()),
                C.ptr(cn), ctypes.c_size_t(cn.numel() if cn is not None else 0), int(stride), int(phase), C.stream_of(pos))
        if rc != 0 and _LIB_OVERRIDE is not None:
            raise C.NativeLibraryError(f"mi_d3{tag}_packed_cn (override library) failed with code {rc}")
        C.check(rc, f"mi_d3{tag}_packed_cn")
        return
    fn = L.mi_d3 if zero is None else L.mi_d3_zero
    rc = fn(C.ptr(pos), C.ptr(z), n, code, C.ptr(idx), C.ptr(sh), C.ptr(nptr), int(max_neighbors),
            ctypes.c_longlong(idx.shape[0] if nptr is not None else 0), int(fill_value),  # CSR: the entry count (packing is decided by the workspace size)
            C.ptr(cell_t), C.ptr(bi), int(num_systems), ctypes.byref(par), *zargs, int(bool(compute_virial)), C.ptr(energy), C.ptr(forces),
            C.ptr(coord_num), C.ptr(vir), C.ptr(ws), ctypes.c_size_t(ws_bytes), C.stream_of(pos))
    if rc != 0 and _LIB_OVERRIDE is not None:
        raise C.NativeLibraryError(f"mi_d3{tag} (override library) failed with code {rc}")
    C.check(rc, f"mi_d3{tag}")


_NO_RADII = object()  # `_check_d3(cutoff_radii=...)`: the caller has no use for a table of pair cutoff radii


def _check_d3(neighbor_matrix, neighbor_matrix_shifts, neighbor_list, neighbor_ptr, unit_shifts, cell, compute_virial, missing_functional,
              d3_params, covalent_radii, r4r2, c6_reference, coord_num_ref, positions, numbers, batch_idx, num_systems, cutoff_radii=_NO_RADII):
    """Argument validation and parameter resolution of the four D3 operators (dftd3.py:2668-2757): the same checks in the same order with
    the same messages -- list format, tables, per-atom / neighbour data and, with `cutoff_radii` given (a tensor or None; zero damping),
    the pair cutoff radii.  Returns (use_matrix, (rcov, r4r2, c6ab, cn_ref)[, cutoff_radii])."""
    use_matrix = K.check_lists(neighbor_matrix, neighbor_matrix_shifts, neighbor_list, neighbor_ptr, unit_shifts, cell, compute_virial,
                               missing_functional)
    tables = K.d3_tables(d3_params, covalent_radii, r4r2, c6_reference, coord_num_ref)
    K.check_atoms(positions, numbers, batch_idx, num_systems, neighbor_matrix, neighbor_matrix_shifts, neighbor_list, neighbor_ptr, unit_shifts,
                  cell)
    if cutoff_radii is _NO_RADII:
        return use_matrix, tables
    return use_matrix, tables, K.d3_cutoff_radii(d3_params, cutoff_radii, tables[0].size(0))


def _two_body(positions, numbers, lists, neighbor_matrix, cell, batch_idx, num_systems, tables, scalars, k1, compute_virial, out,
              zero=None) -> None:
    """The eager launch of `dftd3` / `dftd3_zero` on `lists` = `K.list_args(...)`, with what a neighbour search of this package left next to
    its matrix: the companion and the search-side coordination numbers know nothing about the damping."""
    idx, shifts, fill = lists[0], lists[1], lists[4]
    packed = None
    if idx is neighbor_matrix and cell is not None and shifts is not None and int(fill) >= positions.size(0):
        from nvalchemiops.neighborlist import _engine as E

        # valid only while matrix and shifts are provably what the search wrote (tensor identity + version counters); else None
        packed = E.packed_companion(idx, shifts, fill)
        E.learn_dftd3_context(idx, numbers, tables[0], k1)  # "auto" policy: the next search into this buffer also sums the CNs
    _launch(positions, numbers, *lists, cell, batch_idx, num_systems, tables, scalars, compute_virial, *out, packed=packed, zero=zero)


@C.hybrid
def dftd3(positions: torch.Tensor, numbers: torch.Tensor, a1: float, a2: float, s8: float, k1: float = 16.0, k3: float = -4.0,
          s6: float = 1.0, s5_smoothing_on: float = 1e10, s5_smoothing_off: float = 1e10, fill_value: int | None = None,
          d3_params: D3Parameters | dict[str, torch.Tensor] | None = None, covalent_radii: torch.Tensor | None = None,
          r4r2: torch.Tensor | None = None, c6_reference: torch.Tensor | None = None, coord_num_ref: torch.Tensor | None = None,
          batch_idx: torch.Tensor | None = None, cell: torch.Tensor | None = None, neighbor_matrix: torch.Tensor | None = None,
          neighbor_matrix_shifts: torch.Tensor | None = None, neighbor_list: torch.Tensor | None = None,
          neighbor_ptr: torch.Tensor | None = None, unit_shifts: torch.Tensor | None = None, compute_virial: bool = False,
          num_systems: int | None = None, device: str | None = None):
    """Returns ``(energy[num_systems], forces[N,3], coord_num[N])`` (+ ``virial[num_systems,3,3]`` if ``compute_virial``).

    Validation, parameter resolution, num_systems inference and empty-input behaviour follow dftd3.py:2668-2804."""
    missing = None
    if a1 is None or a2 is None or s8 is None:
        missing = ("Functional parameters a1, a2, and s8 must be provided. "
                   "These are functional-dependent parameters required for DFT-D3(BJ) calculations.")
    use_matrix, (covalent_radii, r4r2, c6_reference, coord_num_ref) = _check_d3(
        neighbor_matrix, neighbor_matrix_shifts, neighbor_list, neighbor_ptr, unit_shifts, cell, compute_virial, missing, d3_params, covalent_radii,
        r4r2, c6_reference, coord_num_ref, positions, numbers, batch_idx, num_systems)
    if positions.size(0) == 0:
        return K.empty_result(positions, batch_idx, 1, compute_virial)
    num_systems = K.infer_num_systems(num_systems, batch_idx, cell)
    out = energy, forces, coord_num, virial = K.allocate(positions, num_systems, 1, compute_virial)
    if C.tracing():
        # torch.compile: the reference's own seam -- one mutating custom op per call (dftd3.py:1792-1796 / :2125-2128, called from
        # :2806-2870); the conversions the eager path does below happen inside the op
        if use_matrix:
            torch.ops.nvalchemiops.dftd3_nm(positions, numbers, neighbor_matrix, covalent_radii, r4r2, c6_reference, coord_num_ref, a1, a2, s8,
                                            energy, forces, coord_num, virial, k1, k3, s6, s5_smoothing_on, s5_smoothing_off, fill_value,
                                            batch_idx, cell, neighbor_matrix_shifts, compute_virial, None)
        else:
            torch.ops.nvalchemiops.dftd3_nl(positions, numbers, neighbor_list[1], neighbor_ptr, covalent_radii, r4r2, c6_reference,
                                            coord_num_ref, a1, a2, s8, energy, forces, coord_num, virial, k1, k3, s6, s5_smoothing_on,
                                            s5_smoothing_off, batch_idx, cell, unit_shifts, compute_virial, None)
    else:
        C.require_device(positions, numbers, neighbor_matrix, neighbor_list, neighbor_ptr, batch_idx)
        lists = K.list_args(positions.size(0), neighbor_matrix, neighbor_matrix_shifts, fill_value, neighbor_list, neighbor_ptr, unit_shifts)
        _two_body(positions, numbers, lists, neighbor_matrix, cell, batch_idx, num_systems, (covalent_radii, r4r2, c6_reference, coord_num_ref),
                  d3_scalars(a1, a2, s6, s8, k1, k3, s5_smoothing_on, s5_smoothing_off), k1, compute_virial, out)
    return K.select(out, compute_virial)


@C.hybrid
def dftd3_zero(positions: torch.Tensor, numbers: torch.Tensor, rs6: float, s8: float, rs8: float = 1.0, alpha: float = 14.0, beta: float = 0.0,
               k1: float = 16.0, k3: float = -4.0, s6: float = 1.0, s5_smoothing_on: float = 1e10, s5_smoothing_off: float = 1e10,
               fill_value: int | None = None, d3_params: D3Parameters | dict[str, torch.Tensor] | None = None,
               covalent_radii: torch.Tensor | None = None, r4r2: torch.Tensor | None = None, c6_reference: torch.Tensor | None = None,
               coord_num_ref: torch.Tensor | None = None, cutoff_radii: torch.Tensor | None = None, batch_idx: torch.Tensor | None = None,
               cell: torch.Tensor | None = None, neighbor_matrix: torch.Tensor | None = None,
               neighbor_matrix_shifts: torch.Tensor | None = None, neighbor_list: torch.Tensor | None = None,
               neighbor_ptr: torch.Tensor | None = None, unit_shifts: torch.Tensor | None = None, compute_virial: bool = False,
               num_systems: int | None = None, device: str | None = None):
    """DFT-D3 with zero damping, D3(0) and its modified form D3M(0): returns what `dftd3` returns, ``(energy[num_systems], forces[N,3],
    coord_num[N])`` (+ ``virial[num_systems,3,3]`` if ``compute_virial``), float32, with the pair energy::

        E_ij = -C6_ij(CN_i, CN_j) * (s6 f_6(r) / r^6 + s8 * 3 r4r2_i r4r2_j * f_8(r) / r^8) * sw(r)
        f_n(r) = 1 / (1 + 6 (r / (rs_n R0) + beta R0)^(-alpha_n)),   alpha_6 = alpha, alpha_8 = alpha + 2,   R0 = cutoff_radii[Z_i, Z_j]

    ``beta = 0`` is D3(0), ``beta != 0`` D3M(0).  ``cutoff_radii`` is the symmetric table of pair cutoff radii r0ab[max_Z+1, max_Z+1] in Bohr
    (index 0 = padding; float32 or float64, cast to float32 like the other tables), given explicitly or as key ``"r0ab"`` of a ``d3_params``
    dict; a `D3Parameters` instance does not carry it.  A pair whose entry is <= 0 contributes nothing.  Coordination numbers, C6
    interpolation, the half per stored directed pair, the S5 switch, the force / virial conventions, argument validation, ``num_systems``
    inference and empty-input behaviour are `dftd3`'s; so is the use of what a neighbour search of this package left next to its matrix
    (packed companion, coordination numbers)."""
    missing = None
    if rs6 is None or s8 is None:
        missing = ("Functional parameters rs6 and s8 must be provided. "
                   "These are functional-dependent parameters required for DFT-D3 zero-damping calculations.")
    elif not alpha > 0:
        missing = f"alpha must be positive, got {alpha}"
    elif not (rs6 > 0 and rs8 > 0):
        missing = f"rs6 and rs8 must be positive, got rs6={rs6}, rs8={rs8}"
    use_matrix, (covalent_radii, r4r2, c6_reference, coord_num_ref), cutoff_radii = _check_d3(
        neighbor_matrix, neighbor_matrix_shifts, neighbor_list, neighbor_ptr, unit_shifts, cell, compute_virial, missing, d3_params, covalent_radii,
        r4r2, c6_reference, coord_num_ref, positions, numbers, batch_idx, num_systems, cutoff_radii=cutoff_radii)
    if positions.size(0) == 0:
        return K.empty_result(positions, batch_idx, 1, compute_virial)
    num_systems = K.infer_num_systems(num_systems, batch_idx, cell)
    out = energy, forces, coord_num, virial = K.allocate(positions, num_systems, 1, compute_virial)
    if C.tracing():
        # torch.compile: one mutating custom op per call, as for `dftd3`
        if use_matrix:
            torch.ops.nvalchemiops.dftd3_zero_nm(positions, numbers, neighbor_matrix, covalent_radii, r4r2, c6_reference, coord_num_ref,
                                                 cutoff_radii, rs6, s8, energy, forces, coord_num, virial, rs8, alpha, beta, k1, k3, s6,
                                                 s5_smoothing_on, s5_smoothing_off, fill_value, batch_idx, cell, neighbor_matrix_shifts,
                                                 compute_virial, None)
        else:
            torch.ops.nvalchemiops.dftd3_zero_nl(positions, numbers, neighbor_list[1], neighbor_ptr, covalent_radii, r4r2, c6_reference,
                                                 coord_num_ref, cutoff_radii, rs6, s8, energy, forces, coord_num, virial, rs8, alpha, beta, k1,
                                                 k3, s6, s5_smoothing_on, s5_smoothing_off, batch_idx, cell, unit_shifts, compute_virial, None)
    else:
        C.require_device(positions, numbers, neighbor_matrix, neighbor_list, neighbor_ptr, batch_idx)
        lists = K.list_args(positions.size(0), neighbor_matrix, neighbor_matrix_shifts, fill_value, neighbor_list, neighbor_ptr, unit_shifts)
        _two_body(positions, numbers, lists, neighbor_matrix, cell, batch_idx, num_systems, (covalent_radii, r4r2, c6_reference, coord_num_ref),
                  zero_scalars(s6, s8, k1, k3, s5_smoothing_on, s5_smoothing_off), k1, compute_virial, out,
                  zero=(rs6, rs8, alpha, beta, cutoff_radii))
    return K.select(out, compute_virial)


def d3_scalars(a1, a2, s6, s8, k1, k3, on, off):
    """The floats of `mi_d3_params`."""
    return dict(a1=a1, a2=a2, s6=s6, s8=s8, k1=k1, k3=k3, s5_on=on, s5_off=off)


def zero_scalars(s6, s8, k1, k3, on, off):
    """`mi_d3_params` scalars of a zero-damping call: a1 / a2 are not read."""
    return d3_scalars(0.0, 0.0, s6, s8, k1, k3, on, off)


def atm_tile() -> int:
    """Neighbours inside ``three_body_cutoff`` a row may have before the triple pass of `dftd3_atm` works tile by tile."""
    return int(C.lib().mi_d3_atm_tile())


def _launch_atm(positions, numbers, idx, shifts, nptr, max_neighbors, fill_value, cell, batch_idx, num_systems, tables, scalars, s9, alpha,
                three_body_cutoff, compute_virial, energy, forces, virial, want_visits=False, zero=None):
    """One `mi_d3_atm` call on the caller's arrays.  `want_visits`: return the per-centre triangle-visit counts the triple pass leaves in
    its workspace (a diagnostic for tools/atm_bench.py).  `zero`: None, or (rs9, cutoff_radii[nz,nz]) for the radii of the zero damping
    (`mi_d3_zero_atm`; scalars' a1 / a2 are then ignored)."""
    n = positions.shape[0]
    pos, code, z, cell_t, sh, bi = K.prelude(positions, numbers, shifts, cell, batch_idx)
    par, keep = K.d3_struct(pos.device, tables, scalars)
    L = C.lib()
    if not hasattr(L, "mi_d3_atm"):
        raise C.NativeLibraryError("libnvalchemiops_hip.so does not export mi_d3_atm: rebuild it (build_native.py)")
    ws_bytes = int(L.mi_d3_atm_workspace_bytes(n, num_systems, par.nz))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pos.device)
    if zero is not None:
        if not hasattr(L, "mi_d3_zero_atm"):
            raise C.NativeLibraryError("libnvalchemiops_hip.so does not export mi_d3_zero_atm: rebuild it (build_native.py)")
        r0ab = K.f32_on(zero[1], pos.device)
        rc = L.mi_d3_zero_atm(C.ptr(pos), C.ptr(z), n, code, C.ptr(idx), C.ptr(sh), C.ptr(nptr), int(max_neighbors), int(fill_value), C.ptr(cell_t),
                              C.ptr(bi), int(num_systems), ctypes.byref(par), float(s9), float(alpha), float(three_body_cutoff), float(zero[0]),
                              C.ptr(r0ab), int(bool(compute_virial)), C.ptr(energy), C.ptr(forces), C.ptr(virial if compute_virial else None),
                              C.ptr(ws), ctypes.c_size_t(ws_bytes), C.stream_of(pos))
        C.check(rc, "mi_d3_zero_atm")
    else:
        rc = L.mi_d3_atm(C.ptr(pos), C.ptr(z), n, code, C.ptr(idx), C.ptr(sh), C.ptr(nptr), int(max_neighbors), int(fill_value), C.ptr(cell_t),
                         C.ptr(bi), int(num_systems), ctypes.byref(par), float(s9), float(alpha), float(three_body_cutoff), int(bool(compute_virial)),
                         C.ptr(energy), C.ptr(forces), C.ptr(virial if compute_virial else None), C.ptr(ws), ctypes.c_size_t(ws_bytes),
                         C.stream_of(pos))
        C.check(rc, "mi_d3_atm")
    if want_visits:
        off = int(L.mi_d3_atm_visits_offset(n, num_systems, par.nz))
        return ws[off:off + 4 * n].view(torch.int32).clone()
    return None


@C.hybrid
def dftd3_atm(positions: torch.Tensor, numbers: torch.Tensor, a1: float, a2: float, three_body_cutoff: float, s9: float = 1.0,
              alpha: float = 16.0, k1: float = 16.0, k3: float = -4.0, fill_value: int | None = None,
              d3_params: D3Parameters | dict[str, torch.Tensor] | None = None, covalent_radii: torch.Tensor | None = None,
              r4r2: torch.Tensor | None = None, c6_reference: torch.Tensor | None = None, coord_num_ref: torch.Tensor | None = None,
              batch_idx: torch.Tensor | None = None, cell: torch.Tensor | None = None, neighbor_matrix: torch.Tensor | None = None,
              neighbor_matrix_shifts: torch.Tensor | None = None, neighbor_list: torch.Tensor | None = None,
              neighbor_ptr: torch.Tensor | None = None, unit_shifts: torch.Tensor | None = None, compute_virial: bool = False,
              num_systems: int | None = None):
    """Three-body (Axilrod-Teller-Muto) dispersion of DFT-D3: returns ``(energy[num_systems], forces[N,3])`` (+ ``virial[num_systems,3,3]``
    if ``compute_virial``) of the three-body term ALONE, float32, in the units and the virial convention of `dftd3`, so that a caller adds
    them to `dftd3`'s outputs.

    For every unordered triple of distinct atom images A, B, C whose three distances are all ``< three_body_cutoff``::

        E_ABC = s9 * sqrt(C6_AB C6_AC C6_BC) * (3 cosA cosB cosC + 1) / (r_AB r_AC r_BC)^3 / (1 + 6 (R0_AB R0_AC R0_BC / (r_AB r_AC r_BC))^(alpha/3))

    with ``R0_XY = a1 sqrt(3 r4r2_X r4r2_Y) + a2`` and C6_XY the coordination-number interpolation of `dftd3`, evaluated with the
    coordination numbers `dftd3` returns for the same list (summed over ALL its entries).  A triple counts once per unit cell; forces
    include the path through the coordination numbers.  ``alpha = 16`` is the original D3 damping exponent (some codes use 14).

    Requirements on the list: it is a FULL list (every pair stored in both rows: what ``neighbor_list()`` / ``cell_list()`` return without
    ``half_fill``) and its cutoff is at least ``three_body_cutoff``.  Entries beyond ``three_body_cutoff`` are part of no triple (they still
    count for the coordination numbers).  A periodic list may hold an atom's own images and several images of one neighbour: those are
    distinct vertices.  Argument names, parameter resolution, validation, ``num_systems`` inference and empty-input behaviour are `dftd3`'s."""
    if a1 is None or a2 is None:
        missing = ("Functional parameters a1 and a2 must be provided. "
                   "These are functional-dependent parameters required for DFT-D3(BJ) calculations.")
    else:
        missing = K.three_body_missing(three_body_cutoff, alpha)
    use_matrix, tables = _check_d3(neighbor_matrix, neighbor_matrix_shifts, neighbor_list, neighbor_ptr, unit_shifts, cell, compute_virial, missing,
                                   d3_params, covalent_radii, r4r2, c6_reference, coord_num_ref, positions, numbers, batch_idx, num_systems)
    if positions.size(0) == 0:
        return K.empty_result(positions, batch_idx, 0, compute_virial)
    num_systems = K.infer_num_systems(num_systems, batch_idx, cell)
    out = energy, forces, virial = K.allocate(positions, num_systems, 0, compute_virial)
    if C.tracing():
        if use_matrix:
            torch.ops.nvalchemiops.dftd3_atm_nm(positions, numbers, neighbor_matrix, tables[0], tables[1], tables[2], tables[3], a1, a2,
                                                three_body_cutoff, energy, forces, virial, s9, alpha, k1, k3, fill_value, batch_idx, cell,
                                                neighbor_matrix_shifts, compute_virial)
        else:
            torch.ops.nvalchemiops.dftd3_atm_nl(positions, numbers, neighbor_list[1], neighbor_ptr, tables[0], tables[1], tables[2], tables[3],
                                                a1, a2, three_body_cutoff, energy, forces, virial, s9, alpha, k1, k3, batch_idx, cell, unit_shifts,
                                                compute_virial)
    else:
        C.require_device(positions, numbers, neighbor_matrix, neighbor_list, neighbor_ptr, batch_idx)
        lists = K.list_args(positions.size(0), neighbor_matrix, neighbor_matrix_shifts, fill_value, neighbor_list, neighbor_ptr, unit_shifts)
        _launch_atm(positions, numbers, *lists, cell, batch_idx, num_systems, tables, atm_scalars(a1, a2, k1, k3), s9, alpha, three_body_cutoff,
                    compute_virial, *out)
    return K.select(out, compute_virial)


@C.hybrid
def dftd3_zero_atm(positions: torch.Tensor, numbers: torch.Tensor, three_body_cutoff: float, cutoff_radii: torch.Tensor | None = None,
                   rs9: float = 4.0 / 3.0, s9: float = 1.0, alpha: float = 16.0, k1: float = 16.0, k3: float = -4.0,
                   fill_value: int | None = None, d3_params: D3Parameters | dict[str, torch.Tensor] | None = None,
                   covalent_radii: torch.Tensor | None = None, r4r2: torch.Tensor | None = None, c6_reference: torch.Tensor | None = None,
                   coord_num_ref: torch.Tensor | None = None, batch_idx: torch.Tensor | None = None, cell: torch.Tensor | None = None,
                   neighbor_matrix: torch.Tensor | None = None, neighbor_matrix_shifts: torch.Tensor | None = None,
                   neighbor_list: torch.Tensor | None = None, neighbor_ptr: torch.Tensor | None = None,
                   unit_shifts: torch.Tensor | None = None, compute_virial: bool = False, num_systems: int | None = None):
    """The three-body (Axilrod-Teller-Muto) term as it is paired with zero damping: `dftd3_atm` with the radii taken from the table of pair
    cutoff radii, ``R0_XY = rs9 * cutoff_radii[Z_X, Z_Y]`` (``rs9 = 4/3`` by convention), instead of ``a1 sqrt(3 r4r2_X r4r2_Y) + a2``.
    ``cutoff_radii`` is resolved as in `dftd3_zero` (explicit, or key ``"r0ab"`` of a ``d3_params`` dict); a triple with a pair whose entry
    is <= 0 contributes nothing.  The remaining arguments, the list requirements and the outputs -- ``(energy[num_systems], forces[N,3])``
    (+ ``virial[num_systems,3,3]``) of the three-body term alone, to be added to `dftd3_zero`'s -- are `dftd3_atm`'s."""
    missing = K.three_body_missing(three_body_cutoff, alpha)
    if missing is None and not rs9 > 0:
        missing = f"rs9 must be positive, got {rs9}"
    use_matrix, tables, cutoff_radii = _check_d3(
        neighbor_matrix, neighbor_matrix_shifts, neighbor_list, neighbor_ptr, unit_shifts, cell, compute_virial, missing, d3_params, covalent_radii,
        r4r2, c6_reference, coord_num_ref, positions, numbers, batch_idx, num_systems, cutoff_radii=cutoff_radii)
    if positions.size(0) == 0:
        return K.empty_result(positions, batch_idx, 0, compute_virial)
    num_systems = K.infer_num_systems(num_systems, batch_idx, cell)
    out = energy, forces, virial = K.allocate(positions, num_systems, 0, compute_virial)
    if C.tracing():
        if use_matrix:
            torch.ops.nvalchemiops.dftd3_zero_atm_nm(positions, numbers, neighbor_matrix, tables[0], tables[1], tables[2], tables[3], cutoff_radii,
                                                     three_body_cutoff, energy, forces, virial, rs9, s9, alpha, k1, k3, fill_value, batch_idx,
                                                     cell, neighbor_matrix_shifts, compute_virial)
        else:
            torch.ops.nvalchemiops.dftd3_zero_atm_nl(positions, numbers, neighbor_list[1], neighbor_ptr, tables[0], tables[1], tables[2],
                                                     tables[3], cutoff_radii, three_body_cutoff, energy, forces, virial, rs9, s9, alpha, k1, k3,
                                                     batch_idx, cell, unit_shifts, compute_virial)
    else:
        C.require_device(positions, numbers, neighbor_matrix, neighbor_list, neighbor_ptr, batch_idx)
        lists = K.list_args(positions.size(0), neighbor_matrix, neighbor_matrix_shifts, fill_value, neighbor_list, neighbor_ptr, unit_shifts)
        _launch_atm(positions, numbers, *lists, cell, batch_idx, num_systems, tables, atm_scalars(0.0, 0.0, k1, k3), s9, alpha, three_body_cutoff,
                    compute_virial, *out, zero=(rs9, cutoff_radii))
    return K.select(out, compute_virial)


def atm_scalars(a1, a2, k1, k3):
    """`mi_d3_params` scalars of a three-body call: the two-body-only ones (s6, s8, the S5 window) are not read."""
    return d3_scalars(a1, a2, 0.0, 0.0, k1, k3, 1e10, 1e10)
