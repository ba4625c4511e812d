"""ctypes binding of libnvalchemiops_hip.so (C ABI declared in include/nvalchemiops_hip.h).

Replaces the reference's Warp launch layer (``wp.from_torch`` + ``wp.launch``: e.g. neighborlist/cell_list.py:980-1034,
autograd.py:300-360).  Zero-copy: raw device pointers of torch tensors and torch's current HIP stream are handed
to the library, which never allocates, frees or retains them.
"""
from __future__ import annotations

import contextvars
import ctypes
import functools
import os

import torch

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libnvalchemiops_hip.so")
_LIB = None

MI_F32, MI_F64 = 0, 1
NL_MATRIX, NL_COUNT, NL_CSR = 0, 1, 2
NL_HALF_FILL, NL_NAIVE_EXPR, NL_REUSE_GRID, NL_NO_SHIFTS, NL_NO_PAD = 1, 2, 4, 8, 16
EW_FORCES, EW_CHARGE_GRAD = 1, 2


class NativeLibraryError(RuntimeError):
    """The HIP library is missing or failed: there is deliberately no fallback path."""


class MiD3Params(ctypes.Structure):
    _fields_ = [("rcov", ctypes.c_void_p), ("r4r2", ctypes.c_void_p), ("c6ab", ctypes.c_void_p), ("cn_ref", ctypes.c_void_p),
                ("nz", ctypes.c_int), ("a1", ctypes.c_float), ("a2", ctypes.c_float), ("s6", ctypes.c_float), ("s8", ctypes.c_float),
                ("k1", ctypes.c_float), ("k3", ctypes.c_float), ("s5_on", ctypes.c_float), ("s5_off", ctypes.c_float)]


class MiD3ZeroParams(ctypes.Structure):
    """`mi_d3_zero_params` of include/nvalchemiops_hip.h: the zero-damping parameters and the pair cutoff radii r0ab[nz,nz]."""
    _fields_ = [("rs6", ctypes.c_float), ("rs8", ctypes.c_float), ("alpha", ctypes.c_float), ("beta", ctypes.c_float), ("r0ab", ctypes.c_void_p)]


class MiD4Params(ctypes.Structure):
    """`mi_d4_params` of include/nvalchemiops_hip.h: the D4 element tables (device pointers) and the scalars of the model."""
    _fields_ = ([(name, ctypes.c_void_p) for name in ("rcov", "en", "r4r2", "zeff", "gam", "n_ref", "ngw", "cn_ref", "q_ref", "c6_ref")]
                + [("nz", ctypes.c_int)]
                + [(name, ctypes.c_float) for name in ("a1", "a2", "s6", "s8", "k_cn", "k4", "k5", "k6", "wf", "ga", "gc", "cn_cutoff")])


class MiNlCnRequest(ctypes.Structure):
    """`mi_nl_cn_request` of include/nvalchemiops_hip.h: what a search needs to sum DFT-D3 coordination numbers over the list it writes."""
    _fields_ = [("numbers", ctypes.c_void_p), ("covalent_radii", ctypes.c_void_p), ("nz", ctypes.c_int), ("k1", ctypes.c_float)]


def lib() -> ctypes.CDLL:
    global _LIB
    if _LIB is None:
        if not os.path.exists(_LIB_PATH):
            raise NativeLibraryError(
                f"{_LIB_PATH} not found: build it with `python nvalchemi-toolkit-ops_amd/build_native.py` "
                "(hipcc --offload-arch=gfx950). This package has no CPU or PyTorch fallback.")
        L = ctypes.CDLL(_LIB_PATH)
        L.mi_last_error.restype = ctypes.c_char_p
        L.mi_nl_workspace_bytes.restype = ctypes.c_size_t
        L.mi_nl_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.mi_spline_spread_workspace_bytes.restype = ctypes.c_size_t
        L.mi_pme_solve_scratch_bytes.restype = ctypes.c_size_t
        L.mi_pme_solve_scratch_bytes.argtypes = [ctypes.c_int] * 6
        L.mi_fft_lds_scratch_bytes.restype = ctypes.c_size_t
        L.mi_fft_lds_scratch_bytes.argtypes = [ctypes.c_int] * 5
        L.mi_spline_spread_workspace_bytes.argtypes = [ctypes.c_int] * 5
        L.mi_spline_spread_workspace_bytes_for.restype = ctypes.c_size_t
        L.mi_spline_spread_workspace_bytes_for.argtypes = [ctypes.c_int] * 7
        L.mi_spline_spread_order_offset.restype = ctypes.c_longlong
        L.mi_spline_spread_order_offset.argtypes = [ctypes.c_int] * 6
        L.mi_nl_packed_bytes.restype = ctypes.c_size_t
        L.mi_nl_packed_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
        L.mi_nl_cn_bytes.restype = ctypes.c_size_t
        L.mi_nl_cn_bytes.argtypes = [ctypes.c_int]
        if hasattr(L, "mi_d3_workspace_bytes"):
            L.mi_d3_workspace_bytes.restype = ctypes.c_size_t
            L.mi_d3_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
            L.mi_d3_workspace_bytes_packed.restype = ctypes.c_size_t
            L.mi_d3_workspace_bytes_packed.argtypes = [ctypes.c_int] * 4
            L.mi_d3_workspace_bytes_entries.restype = ctypes.c_size_t
            L.mi_d3_workspace_bytes_entries.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong]
        if hasattr(L, "mi_d3_atm"):  # the three-body (Axilrod-Teller-Muto) term
            for name in ("mi_d3_atm_workspace_bytes", "mi_d3_atm_visits_offset"):
                getattr(L, name).restype = ctypes.c_size_t
                getattr(L, name).argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
            L.mi_d3_atm_tile.restype = ctypes.c_int
            L.mi_d3_atm_tile.argtypes = []
            L.mi_d3_atm.restype = ctypes.c_int
            L.mi_d3_atm.argtypes = ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_float,
                                     ctypes.c_float, ctypes.c_float, ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_size_t, ctypes.c_void_p])
        if hasattr(L, "mi_d3_zero_atm"):  # ... with the radii of the zero damping: mi_d3_atm's arguments + rs9 + the r0ab table
            L.mi_d3_zero_atm.restype = ctypes.c_int
            L.mi_d3_zero_atm.argtypes = ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_float,
                                          ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4
                                         + [ctypes.c_size_t, ctypes.c_void_p])
        vp, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
        if hasattr(L, "mi_d4"):  # DFT-D4 two-body dispersion (nvalchemiops/interactions/dispersion/dftd4.py)
            L.mi_d4_workspace_bytes.restype = sz
            L.mi_d4_workspace_bytes.argtypes = [i, i, i]
            L.mi_d4_species_slots.restype = i
            L.mi_d4_species_slots.argtypes = []
            L.mi_d4_fold_blocks.restype = i
            L.mi_d4_fold_blocks.argtypes = []
            L.mi_d4.restype = i
            L.mi_d4.argtypes = [vp, vp, i, i, vp, vp, vp, i, ctypes.c_longlong, i, vp, vp, i, vp, vp, i] + [vp] * 6 + [sz, vp]
        if hasattr(L, "mi_d4_atm"):  # ... and its three-body (Axilrod-Teller-Muto) term: mi_d3_atm's argument list with the D4 tables
            for name in ("mi_d4_atm_workspace_bytes", "mi_d4_atm_visits_offset"):
                getattr(L, name).restype = sz
                getattr(L, name).argtypes = [i, i, i]
            L.mi_d4_atm_tile.restype = i
            L.mi_d4_atm_tile.argtypes = []
            L.mi_d4_atm.restype = i
            L.mi_d4_atm.argtypes = ([vp, vp, i, i, vp, vp, vp, i, i, vp, vp, i, vp, ctypes.c_float, ctypes.c_float, ctypes.c_float, i] + [vp] * 4
                                    + [sz, vp])
        # the virial entry points (forward-only -dE/d(strain) of the Ewald / PME sums)
        L.mi_ewald_real_virial.restype = i
        L.mi_ewald_real_virial.argtypes = [vp, vp, vp, vp, vp, i, i, i, vp, vp, vp, i, i, i, vp, vp, vp, vp, sz, vp, i, i, vp, vp, vp]
        L.mi_ewald_recip_virial.restype = i
        L.mi_ewald_recip_virial.argtypes = [vp, vp, vp, vp, i, i, i, vp, vp]
        L.mi_pme_virial.restype = i
        L.mi_pme_virial.argtypes = [vp, vp, vp, vp, i, i, i, i, i, i, vp, vp, i, vp, vp, vp]
        for name in ("mi_ewald_virial_blocks", "mi_ewald_recip_virial_blocks", "mi_pme_virial_blocks"):
            getattr(L, name).restype = i
            getattr(L, name).argtypes = []
        # multi-channel spline entry points and the multipole basis functions (nvalchemiops.math)
        L.mi_spline_spread_channels_workspace_bytes_for.restype = sz
        L.mi_spline_spread_channels_workspace_bytes_for.argtypes = [i] * 8
        L.mi_spline_spread_channels.restype = i
        L.mi_spline_spread_channels.argtypes = [vp, vp, vp, vp] + [i] * 9 + [vp, vp, sz, vp]
        L.mi_spline_gather_channels.restype = i
        L.mi_spline_gather_channels.argtypes = [vp, vp, vp, vp] + [i] * 8 + [vp, vp]
        L.mi_spline_gather_channels_frac_grad.restype = i
        L.mi_spline_gather_channels_frac_grad.argtypes = [vp, vp, vp, vp, vp] + [i] * 8 + [vp, vp]
        dbl = ctypes.c_double
        for name, args in (("mi_sph_harm", [vp, i, i, vp, vp]), ("mi_sph_harm_grad", [vp, i, i, vp, vp]), ("mi_gto_density", [vp, i, dbl, i, vp, vp]),
                           ("mi_gto_fourier", [vp, i, dbl, i, vp, vp, vp])):
            getattr(L, name).restype = i
            getattr(L, name).argtypes = args
        # Gaussian-smeared charge correction (nvalchemiops/interactions/electrostatics/gaussian.py)
        L.mi_gaussian_charges.restype = i
        L.mi_gaussian_charges.argtypes = [vp] * 6 + [i, i, i, vp, vp, vp, i, i, i] + [vp] * 6 + [sz, vp]
        L.mi_gaussian_charges_system_sums.restype = i
        L.mi_gaussian_charges_system_sums.argtypes = [vp, vp, vp, vp, i, i, i, vp, vp]
        L.mi_gaussian_charges_scratch_bytes.restype = sz
        L.mi_gaussian_charges_scratch_bytes.argtypes = [i, i]
        for name in ("mi_gaussian_charges_blocks", "mi_gaussian_charges_row_words"):
            getattr(L, name).restype = i
            getattr(L, name).argtypes = []
        # point-dipole Ewald sum (nvalchemiops/interactions/electrostatics/dipole.py)
        L.mi_ewald_dipole_real.restype = i
        L.mi_ewald_dipole_real.argtypes = [vp] * 7 + [i, i, i, vp, vp, vp, i, i, i] + [vp] * 6 + [sz, vp]
        L.mi_ewald_dipole_structure_factors.restype = i
        L.mi_ewald_dipole_structure_factors.argtypes = [vp] * 6 + [i, i, i, i, vp, vp]
        L.mi_ewald_dipole_recip_gather.restype = i
        L.mi_ewald_dipole_recip_gather.argtypes = [vp] * 10 + [i, i, i, i] + [vp] * 5
        L.mi_ewald_dipole_recip_virial.restype = i
        L.mi_ewald_dipole_recip_virial.argtypes = [vp, vp, vp, vp, i, i, i, vp, vp]
        L.mi_ewald_dipole_real_scratch_bytes.restype = sz
        L.mi_ewald_dipole_real_scratch_bytes.argtypes = [i, i]
        L.mi_ewald_dipole_blocks.restype = i
        L.mi_ewald_dipole_blocks.argtypes = []
        # point-quadrupole Ewald sum (nvalchemiops/interactions/electrostatics/quadrupole.py)
        L.mi_ewald_quadrupole_real.restype = i
        L.mi_ewald_quadrupole_real.argtypes = [vp] * 8 + [i, i, i, vp, vp, vp, i, i, i] + [vp] * 7 + [sz, vp]
        L.mi_ewald_quadrupole_structure_factors.restype = i
        L.mi_ewald_quadrupole_structure_factors.argtypes = [vp] * 7 + [i, i, i, i, vp, vp, vp]
        L.mi_ewald_quadrupole_recip_gather.restype = i
        L.mi_ewald_quadrupole_recip_gather.argtypes = [vp] * 11 + [i, i, i, i] + [vp] * 6
        L.mi_ewald_quadrupole_recip_virial.restype = i
        L.mi_ewald_quadrupole_recip_virial.argtypes = [vp, vp, vp, vp, vp, i, i, i, vp, vp]
        L.mi_ewald_quadrupole_real_scratch_bytes.restype = sz
        L.mi_ewald_quadrupole_real_scratch_bytes.argtypes = [i, i]
        L.mi_ewald_quadrupole_blocks.restype = i
        L.mi_ewald_quadrupole_blocks.argtypes = []
        # Thole damping of point dipoles (nvalchemiops/interactions/electrostatics/thole.py)
        L.mi_thole_dipole.restype = i
        L.mi_thole_dipole.argtypes = [vp] * 5 + [ctypes.c_double, vp, vp, i, i, i, vp, vp, vp, i, i, i] + [vp] * 7 + [sz, vp]
        L.mi_thole_dipole_scratch_bytes.restype = sz
        L.mi_thole_dipole_scratch_bytes.argtypes = [i, i]
        L.mi_thole_dipole_blocks.restype = i
        L.mi_thole_dipole_blocks.argtypes = []
        # cluster point multipoles: the bare pair sums (nvalchemiops/interactions/electrostatics/cluster.py)
        L.mi_coulomb_dipole.restype = i
        L.mi_coulomb_dipole.argtypes = [vp] * 6 + [i, i, i, vp, vp, vp, i, i, i] + [vp] * 6 + [sz, vp]
        L.mi_coulomb_quadrupole.restype = i
        L.mi_coulomb_quadrupole.argtypes = [vp] * 7 + [i, i, i, vp, vp, vp, i, i, i] + [vp] * 7 + [sz, vp]
        # scaled bonded pairs of point multipoles (nvalchemiops/interactions/electrostatics/pair_scale.py)
        L.mi_pair_scale.restype = i
        L.mi_pair_scale.argtypes = [vp] * 8 + [i, i, i, vp, vp, vp, i, i, i, i] + [vp] * 7 + [sz, vp]
        for name in ("mi_coulomb_dipole", "mi_coulomb_quadrupole", "mi_pair_scale"):
            getattr(L, name + "_scratch_bytes").restype = sz
            getattr(L, name + "_scratch_bytes").argtypes = [i, i]
            getattr(L, name + "_blocks").restype = i
            getattr(L, name + "_blocks").argtypes = []
        # particle-mesh Ewald for point dipoles (nvalchemiops/interactions/electrostatics/pme_dipole.py)
        L.mi_pme_dipole_spread.restype = i
        L.mi_pme_dipole_spread.argtypes = [vp] * 6 + [i] * 7 + [vp, vp]
        L.mi_pme_dipole_gather.restype = i
        L.mi_pme_dipole_gather.argtypes = [vp] * 9 + [i] * 8 + [vp] * 5
        L.mi_pme_dipole_virial.restype = i
        L.mi_pme_dipole_virial.argtypes = [vp] * 5 + [i] * 6 + [vp, vp]
        L.mi_pme_dipole_virial_blocks.restype = i
        L.mi_pme_dipole_virial_blocks.argtypes = []
        # particle-mesh Ewald for point quadrupoles (nvalchemiops/interactions/electrostatics/pme_quadrupole.py)
        L.mi_pme_quadrupole_spread.restype = i
        L.mi_pme_quadrupole_spread.argtypes = [vp] * 7 + [i] * 7 + [vp, vp]
        L.mi_pme_quadrupole_gather.restype = i
        L.mi_pme_quadrupole_gather.argtypes = [vp] * 10 + [i] * 8 + [vp] * 6
        L.mi_pme_quadrupole_virial.restype = i
        L.mi_pme_quadrupole_virial.argtypes = [vp] * 5 + [i] * 6 + [vp, vp]
        L.mi_pme_quadrupole_virial_blocks.restype = i
        L.mi_pme_quadrupole_virial_blocks.argtypes = []
        # charge equilibration (nvalchemiops/interactions/electrostatics/qeq.py)
        L.mi_qeq_pair_coefficients.restype = i
        L.mi_qeq_pair_coefficients.argtypes = [vp] * 6 + [i, i, i, vp, vp, vp, i, i, vp, vp, vp, vp]
        L.mi_qeq_apply.restype = i
        L.mi_qeq_apply.argtypes = [vp] * 6 + [i, i, vp, i, vp, vp, vp]
        L.mi_qeq_cg_update.restype = i
        L.mi_qeq_cg_update.argtypes = [vp] * 4 + [i, i, i] + [vp] * 7
        L.mi_qeq_cg_direction.restype = i
        L.mi_qeq_cg_direction.argtypes = [vp, vp, i, i, i, dbl, vp, vp, vp, vp, vp]
        for name in ("mi_qeq_blocks", "mi_qeq_state_words"):
            getattr(L, name).restype = i
            getattr(L, name).argtypes = []
        # induced point dipoles (nvalchemiops/interactions/electrostatics/induced.py)
        ll = ctypes.c_longlong
        L.mi_induced_pair_tensors.restype = i
        L.mi_induced_pair_tensors.argtypes = [vp] * 5 + [i, i, i, vp, vp, vp, i, i, ll, vp, vp, vp, vp, vp]
        L.mi_thole_induced_pair_tensors.restype = i
        L.mi_thole_induced_pair_tensors.argtypes = [vp] * 5 + [i, i, i, vp, vp, vp, i, i, ll, vp, vp, vp, vp, dbl, vp]
        L.mi_cluster_induced_pair_tensors.restype = i
        L.mi_cluster_induced_pair_tensors.argtypes = [vp, vp, i, i, vp, vp, i, i, ll, vp, vp, vp, vp, dbl, vp]
        L.mi_induced_apply.restype = i
        L.mi_induced_apply.argtypes = [vp] * 6 + [i, i, vp, i, ll, vp, vp, vp]
        L.mi_induced_dot.restype = i
        L.mi_induced_dot.argtypes = [vp, vp, vp, i, i, vp, vp]
        L.mi_induced_cg_update.restype = i
        L.mi_induced_cg_update.argtypes = [vp] * 4 + [i, i, i] + [vp] * 7
        L.mi_induced_cg_direction.restype = i
        L.mi_induced_cg_direction.argtypes = [vp, vp, vp, i, i, i, dbl, vp, vp, vp, vp, vp]
        for name in ("mi_induced_blocks", "mi_induced_state_words", "mi_induced_tensor_words", "mi_induced_unroll_depth"):
            getattr(L, name).restype = i
            getattr(L, name).argtypes = []
        # local-frame multipoles (nvalchemiops/interactions/electrostatics/frames.py)
        L.mi_frame_rotate.restype = i
        L.mi_frame_rotate.argtypes = [vp] * 7 + [i, i, i, vp, vp, vp]
        L.mi_frame_adjoint.restype = i
        L.mi_frame_adjoint.argtypes = [vp] * 9 + [i, i, i] + [vp] * 5
        L.mi_frame_gather.restype = i
        L.mi_frame_gather.argtypes = [vp, vp, vp, ll, vp, vp, i, i, i, dbl, vp, vp, vp]
        for name in ("mi_frame_blocks", "mi_frame_block_threads"):
            getattr(L, name).restype = i
            getattr(L, name).argtypes = []
        _LIB = L
    return _LIB


def ewald_sym_words() -> int:
    L = lib()
    L.mi_ewald_symmetry_scratch_bytes.restype = ctypes.c_size_t
    return int(L.mi_ewald_symmetry_scratch_bytes()) // 8


def ewald_scratch_bytes(n_atoms: int, dtype: int) -> int:
    L = lib()
    L.mi_ewald_real_scratch_bytes.restype = ctypes.c_size_t
    return int(L.mi_ewald_real_scratch_bytes(int(n_atoms), int(dtype)))


def fold_virial(partial: torch.Tensor) -> torch.Tensor:
    """[B, blocks, 6] float64 block partials {xx, yy, zz, xy, xz, yz} of a virial entry point -> symmetric [B, 3, 3] float64 (fixed-order sum)."""
    xx, yy, zz, xy, xz, yz = partial.sum(1).unbind(-1)
    return torch.stack((xx, xy, xz, xy, yy, yz, xz, yz, zz), dim=-1).reshape(-1, 3, 3)


def fold_virial9(partial: torch.Tensor) -> torch.Tensor:
    """[B, blocks, 9] float64 block partials (row-major, all nine components) -> [B, 3, 3] float64 (fixed-order sum).  For virials that are not
    symmetric: dipoles fixed in the laboratory frame make dU/dR point away from R."""
    return partial.sum(1).reshape(-1, 3, 3)


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise NativeLibraryError(f"{what} failed (code {rc}): {lib().mi_last_error().decode()}")


def ptr(t: torch.Tensor | None):
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


def stream_of(t: torch.Tensor):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def dtype_code(dtype: torch.dtype) -> int:
    # reference: types.py:20-29 raises ValueError for anything but f16/f32/f64; this path supports f32/f64
    if dtype == torch.float32:
        return MI_F32
    if dtype == torch.float64:
        return MI_F64
    raise ValueError(f"Unsupported dtype: {dtype}")


def require_device(*tensors: torch.Tensor | None) -> torch.device:
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise NativeLibraryError(
                "nvalchemiops (MI355X build) computes on ROCm devices only; got a tensor on "
                f"'{t.device}'. There is no CPU path in this package.")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError(f"tensors on different devices: {dev} vs {t.device}")
    return dev


def check_per_atom(n: int, **named: torch.Tensor | None) -> None:
    """`numbers`, `charges`, `batch_idx`, ...: one entry per atom.  The kernels index them with the atom index, so a shorter tensor is an
    out-of-bounds device read (and a longer one a misunderstanding): ValueError.  Host-side shape reads only."""
    for name, t in named.items():
        if t is not None and (t.dim() == 0 or t.shape[0] != n):
            raise ValueError(f"{name} must have one entry per atom: expected shape [{n}], got {tuple(t.shape)}")


def check_neighbor_data(n: int, *, neighbor_matrix=None, neighbor_matrix_shifts=None, neighbor_list=None, idx_j=None, neighbor_ptr=None,
                        neighbor_shifts=None, shifts_name: str = "neighbor_shifts", short_ptr_ok: bool = False, cell=None, num_systems=None,
                        alpha=None, **per_atom) -> None:
    """Neighbour data against the number of atoms `n`, before anything is launched.  The kernels receive bare pointers plus `n`, the row
    width and the entry count, so every disagreement checked here would be an out-of-bounds device read:

      neighbor_matrix [n, M] with neighbor_matrix_shifts [n, M, 3];
      neighbor_list [2, P] (or its second row `idx_j` [P]) with neighbor_ptr [n + 1] and shifts [P, 3]
        (`short_ptr_ok`: cut-off Coulomb defines a shorter neighbor_ptr as "the remaining rows are empty");
      `per_atom` tensors (numbers, charges, batch_idx) of length n;
      cell [B, 3, 3] against `num_systems` and a tensor `alpha` of more than one value.

    Host-side shape reads only (no device sync; TorchDynamo traces them as shape guards).  Values -- indices inside [0, n), a
    monotonic neighbor_ptr -- are NOT checked: that would need a device pass."""
    check_per_atom(n, **per_atom)
    if neighbor_matrix is not None:
        if neighbor_matrix.dim() != 2 or neighbor_matrix.shape[0] != n:
            raise ValueError(f"neighbor_matrix must have shape [{n}, max_neighbors], got {tuple(neighbor_matrix.shape)}")
        want = (n, neighbor_matrix.shape[1], 3)
        if neighbor_matrix_shifts is not None and tuple(neighbor_matrix_shifts.shape) != want:
            raise ValueError(f"neighbor_matrix_shifts must have shape {list(want)} to match neighbor_matrix, got {tuple(neighbor_matrix_shifts.shape)}")
    if neighbor_list is not None:
        if neighbor_list.dim() != 2 or neighbor_list.shape[0] != 2:
            raise ValueError(f"neighbor_list must have shape [2, num_pairs], got {tuple(neighbor_list.shape)}")
        idx_j = neighbor_list[1]
    if idx_j is not None:
        if idx_j.dim() != 1:
            raise ValueError(f"idx_j must have shape [num_pairs], got {tuple(idx_j.shape)}")
        if neighbor_ptr is not None and (neighbor_ptr.dim() != 1 or (neighbor_ptr.shape[0] > n + 1 if short_ptr_ok else neighbor_ptr.shape[0] != n + 1)):
            raise ValueError(f"neighbor_ptr must have shape [{n + 1}] (num_atoms + 1), got {tuple(neighbor_ptr.shape)}")
        want = (idx_j.shape[0], 3)
        if neighbor_shifts is not None and tuple(neighbor_shifts.shape) != want:
            raise ValueError(f"{shifts_name} must have shape {list(want)} to match neighbor_list, got {tuple(neighbor_shifts.shape)}")
    if cell is not None:
        if cell.dim() not in (2, 3) or tuple(cell.shape[-2:]) != (3, 3):
            raise ValueError(f"cell must have shape [3, 3] or [num_systems, 3, 3], got {tuple(cell.shape)}")
        n_cells = cell.shape[0] if cell.dim() == 3 else 1
        if num_systems is not None and n_cells != int(num_systems):
            raise ValueError(f"cell must have shape [{int(num_systems)}, 3, 3] (one per system), got {tuple(cell.shape)}")
        if isinstance(alpha, torch.Tensor) and alpha.numel() > 1 and alpha.numel() != n_cells:
            raise ValueError(f"alpha has {alpha.numel()} values but there are {n_cells} systems")  # the reference's message (ewald.py:230)


SPLINE_REFERENCE_ORDERS = 0x100  # MI_SPLINE_REFERENCE_ORDERS of include/nvalchemiops_hip.h
_REFERENCE_SPLINE_ORDERS = os.environ.get("NVALCHEMIOPS_REFERENCE_SPLINE_ORDERS", "0") not in ("", "0")  # process default
# context-local override (`with nvalchemiops.spline.reference_spline_orders():`): a contextvars.ContextVar, so the setting belongs to the
# thread / asyncio task that entered the block -- another thread launching PME at the same time keeps its own setting, and an exception
# anywhere cannot leave the switch flipped for someone else
_REFERENCE_SPLINE_ORDERS_CTX: contextvars.ContextVar = contextvars.ContextVar("nvalchemiops_reference_spline_orders", default=None)


def reference_spline_orders_active() -> bool:
    v = _REFERENCE_SPLINE_ORDERS_CTX.get()
    return _REFERENCE_SPLINE_ORDERS if v is None else bool(v)


SPLINE_RESOLVED = 0x200  # Python-side only (never reaches the C ABI): the reference-compatibility decision has been taken for this order value


def resolve_spline_order(order: int) -> int:
    """The spline order with the reference-compatibility decision FROZEN into it: low byte = the order, SPLINE_REFERENCE_ORDERS if
    `nvalchemiops.spline.reference_spline_orders` is active where this is called, SPLINE_RESOLVED so that later calls leave it alone.
    Every public electrostatics / spline entry point calls this once, on the caller's thread, and hands the result down; autograd nodes and
    custom-op contexts store it, so a backward pass -- which the autograd engine runs on ITS OWN worker thread for device tensors, where
    the caller's `contextvars` context does not exist -- launches with the same evaluation as its forward."""
    order = int(order)
    if order & SPLINE_RESOLVED or torch.compiler.is_compiling():
        # (while TorchDynamo traces the caller the value stays plain: a context variable cannot be guarded on, and freezing today's setting
        # into a compiled graph would outlive the `with` block; the ops then read the switch at launch time, as before round 6)
        return order
    return (order & 0xff) | SPLINE_RESOLVED | (SPLINE_REFERENCE_ORDERS if reference_spline_orders_active() else 0)


def plain_spline_order(order: int) -> int:
    """The order itself (1 - 6 ...), whatever flags ride on the value."""
    return int(order) & 0xff


def spline_order_arg(order: int) -> int:
    """The `order` argument of the C ABI: the spline order, plus the reference-compatibility bit (orders 5 / 6 evaluated as the reference
    does: zero weights, exponent 4).  A value that went through `resolve_spline_order` keeps the decision taken there; a plain order takes
    the one of the calling context.  The bit travels with every launch: the library itself holds no such state."""
    return resolve_spline_order(order) & (0xff | SPLINE_REFERENCE_ORDERS)


def cdouble(x: float):
    return ctypes.c_double(float(x))


def i32(t: torch.Tensor | None) -> torch.Tensor | None:
    if t is None:
        return None
    return t.to(torch.int32).contiguous()


def _on_device_of(args, kwargs):
    """Device of the first tensor argument when it is not the current one (HIP launches go to the CURRENT device: tensors on another
    GPU of the process need the guard the reference gets from Warp's per-device launch, `wp.launch(device=...)`)."""
    for a in (args if args else kwargs.values()):
        if isinstance(a, torch.Tensor):
            if a.is_cuda and a.device.index != torch.cuda.current_device():
                return a.device
            break
    return None


def eager(fn):
    """Decorator of the public entry points whose result SHAPE depends on device data (COO / CSR conversion, size estimates: one host
    read each).  The launch layer hands raw device pointers and the current HIP stream to ctypes, which TorchDynamo can neither trace nor
    guard, so under ``torch.compile`` these run as eager islands (a graph break around the call) -- the reference's versions of the same
    functions break the graph at their ``.item()`` as well (neighbor_utils.py:426, cell_list.py:700-722)."""
    inner = torch.compiler.disable(fn)

    @functools.wraps(fn)
    def entry(*args, **kwargs):
        # a plain frame around the disabled callable: `torch.compile(f)` unwraps a directly disabled function and would trace its body
        dev = _on_device_of(args, kwargs)
        if dev is not None:
            with torch.cuda.device(dev):
                return inner(*args, **kwargs)
        return inner(*args, **kwargs)

    return entry


def hybrid(fn):
    """Decorator of the public neighbour-list / DFT-D3 entry points.  Outside a trace the body runs as plain eager code and launches
    through ctypes (no custom-op dispatch on a path whose kernels take tens of microseconds).  While TorchDynamo traces the caller
    (`torch.compile`, also ``fullgraph=True`` under Inductor) the SAME body is traced: every launch in it branches on `tracing()` into the
    registered, mutation-annotated ``torch.ops.nvalchemiops.*`` custom op (nvalchemiops/_ops.py), which is what the reference's thin
    wrappers over ``torch.library.custom_op`` do (neighborlist/cell_list.py:725-736, 892-895, 1037-1192; dftd3.py:1792-1796) and what its
    compiled MD-step example relies on (examples/neighborlist/04_neighbors_list_torch_compile_performance.py:323-346)."""
    inner = torch.compiler.disable(fn)

    @functools.wraps(fn)
    def entry(*args, **kwargs):
        if torch.compiler.is_compiling():
            return fn(*args, **kwargs)
        dev = _on_device_of(args, kwargs)
        if dev is not None:
            with torch.cuda.device(dev):
                return inner(*args, **kwargs)
        return inner(*args, **kwargs)

    return entry


def tracing() -> bool:
    """True while TorchDynamo traces the caller (torch.compile): the public electrostatics functions then take their custom-op path."""
    return torch.compiler.is_compiling()


def traceable(fn):
    """Decorator of the public electrostatics entry points.  Unlike `eager` the body is visible to TorchDynamo: it branches on
    `tracing()` into the `alchemiops::*` custom-op composition (nvalchemiops/_eops.py), so `torch.compile(..., fullgraph=True)`
    captures it; outside a trace it only adds the device guard `eager` has."""
    @functools.wraps(fn)
    def entry(*args, **kwargs):
        if torch.compiler.is_compiling():
            return fn(*args, **kwargs)
        dev = _on_device_of(args, kwargs)
        if dev is not None:
            with torch.cuda.device(dev):
                return fn(*args, **kwargs)
        return fn(*args, **kwargs)

    return entry
