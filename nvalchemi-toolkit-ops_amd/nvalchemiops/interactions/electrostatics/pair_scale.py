"""Scaled bonded pairs of point multipoles: the 1-2 ... 1-5 scale factors of a force field on the electrostatics of charges, dipoles and
quadrupoles.

Every force field and every multipole-predicting potential with bonded multipolar atoms scales the electrostatics of bonded pairs (AMOEBA's
permanent multipoles: 0 / 0 / 0.4 / 0.8 for 1-2 / 1-3 / 1-4 / 1-5; fixed-charge force fields: 0 / 0 / 0.5 - 0.833).  None of the energy
operators of this package has a per-pair factor: the Ewald and mesh routines sum every pair through their reciprocal part, and the cluster
routines take "the list is the sum".  `pair_scale_correction` is ADDED to their unscaled total and gives every listed pair its factor:

    pair_scale_correction   1/2 sum (s - 1) U_ij over a list of scaled pairs, U_ij the complete bare pair energy of charges, dipoles, quadrupoles
    bonded_pair_scales      the list and its scales from the bonds of a topology (host, once per topology)

One HIP kernel of its own (csrc/pair_scale.hip, `mi_pair_scale`): bonded rows hold 2 to about 25 entries, so a group of 8 lanes owns a row
(8 rows per wave64) instead of the wave per row of the other pair sums.  Forward and adjoint are the same launch without and with per-atom
weights; nothing uses atomics, so every output is bit-reproducible.  The reference package has no counterpart.
"""
from __future__ import annotations

import collections
import ctypes

import numpy as np
import torch

from nvalchemiops import _capi as C
from nvalchemiops.interactions.electrostatics import _multipoles as M
from nvalchemiops.interactions.electrostatics import _pairs as P
from nvalchemiops.interactions.electrostatics import quadrupole as Q


def _check(positions, charges, dipoles, quadrupoles, pair_scales, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
           neighbor_matrix_shifts, batch_idx, minimum_image, compute_virial):
    """Every argument error, before anything is launched: those of `coulomb_quadrupole_correction`, plus the scales and the image rule."""
    if minimum_image:
        if cell is None:
            raise ValueError("minimum_image needs a cell")
        if neighbor_shifts is not None or neighbor_matrix_shifts is not None:
            raise ValueError("minimum_image takes a list without shifts: every entry is reduced to its minimum image")
    # under minimum_image the virial is formed from the reduced pair vectors and needs no shifts
    M.check_optional_cell_lists(positions, charges, dipoles, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                                neighbor_matrix_shifts, batch_idx, compute_virial and not minimum_image)
    Q.check_quadrupoles(positions, quadrupoles)
    if not isinstance(pair_scales, torch.Tensor):
        raise ValueError(f"pair_scales must be a tensor shaped like the index array, got {type(pair_scales).__name__}")
    want = tuple(neighbor_matrix.shape) if neighbor_matrix is not None else (neighbor_list.shape[1],)
    if tuple(pair_scales.shape) != want:
        raise ValueError(f"pair_scales must have the shape of the index array: expected {list(want)}, got {tuple(pair_scales.shape)}")
    if pair_scales.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"pair_scales must be float32 or float64, got {pair_scales.dtype}")
    if pair_scales.requires_grad:
        raise NotImplementedError("pair_scale_correction: pair_scales is not differentiable (dE/ds is out of scope); detach it")


def _inputs(positions, charges, dipoles, quadrupoles, pair_scales, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
            neighbor_matrix_shifts, mask_value, minimum_image):
    lists = (neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts)
    C.require_device(positions, pair_scales)
    p = P.launch_inputs(positions, charges, cell, batch_idx, lists, int(mask_value), mu=dipoles, qd=quadrupoles)
    p["scl"] = pair_scales.detach().to(torch.float64).contiguous()
    p["min_image"] = bool(minimum_image)
    return p


def _launch(p, flags: int, weights=None, energies: bool = True):
    """One `mi_pair_scale` launch: float64 (energies | None, forces in the positions dtype | None, charge sums | None, dipole sums | None,
    quadrupole sums [n, 3, 3] | None, virial block partials [nsys, blocks, 9] | None)."""
    pos = p["pos"]
    n, dt = pos.shape[0], pos.dtype
    L = C.lib()
    e, f, cg, dg, qg = M.allocate(pos, M.QUADRUPOLE, (energies, flags & P.FORCES, flags & P.CHARGE_GRAD, flags & P.THIRD_GRAD,
                                                      flags & P.FOURTH_GRAD))
    nbytes = int(L.mi_pair_scale_scratch_bytes(n, C.dtype_code(dt)))
    part, scratch = M.pair_scratch(p, flags, int(L.mi_pair_scale_blocks()), nbytes)
    rc = L.mi_pair_scale(C.ptr(pos), C.ptr(p["q"]), C.ptr(p["mu"]), C.ptr(p["qd"]), C.ptr(p["cells"]), C.ptr(p["bi"]), C.ptr(weights),
                         C.ptr(p["scl"]), n, int(p["nsys"]), C.dtype_code(dt), C.ptr(p["idx"]), C.ptr(p["sh"]), C.ptr(p["nptr"]), int(p["m"]),
                         p["mask"], int(p["min_image"]), int(flags), C.ptr(e), C.ptr(f), C.ptr(cg), C.ptr(dg), C.ptr(qg), C.ptr(part),
                         C.ptr(scratch), ctypes.c_size_t(nbytes), C.stream_of(pos))
    C.check(rc, "mi_pair_scale")
    return e, f, cg, dg, qg, part


def _forward(positions, charges, dipoles, quadrupoles, pair_scales, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
             neighbor_matrix_shifts, mask_value, minimum_image, forces, cgrads, dgrads, qgrads, virial):
    """(energies, forces | None, charge_grads | None, dipole_grads | None, quadrupole_grads | None, virial | None) in the positions dtype, no
    autograd graph: what the eager call and the `alchemiops::_pair_scale_correction` op both run."""
    p = _inputs(positions, charges, dipoles, quadrupoles, pair_scales, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts,
                neighbor_matrix, neighbor_matrix_shifts, mask_value, minimum_image)
    return M.pair_forward(p, _launch, M.QUADRUPOLE, (True, forces, cgrads, dgrads, qgrads, virial))


def _adjoint(positions, charges, dipoles, quadrupoles, pair_scales, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
             neighbor_matrix_shifts, mask_value, minimum_image, grad_energies):
    """Float64 (dL/dpositions, dL/dcharges, dL/ddipoles, dL/dquadrupoles) of L = sum_i g_i E_i: the forward kernel with weights."""
    p = _inputs(positions, charges, dipoles, quadrupoles, pair_scales, cell, batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts,
                neighbor_matrix, neighbor_matrix_shifts, mask_value, minimum_image)
    return M.pair_adjoint(p, _launch, M.QUADRUPOLE, grad_energies)


@C.traceable
def pair_scale_correction(positions: torch.Tensor, charges: torch.Tensor, dipoles: torch.Tensor | None, quadrupoles: torch.Tensor | None,
                          pair_scales: torch.Tensor, cell: torch.Tensor | None = None, *, neighbor_list: torch.Tensor | None = None,
                          neighbor_ptr: torch.Tensor | None = None, neighbor_shifts: torch.Tensor | None = None,
                          neighbor_matrix: torch.Tensor | None = None, neighbor_matrix_shifts: torch.Tensor | None = None,
                          mask_value: int = -1, batch_idx: torch.Tensor | None = None, minimum_image: bool = False,
                          compute_forces: bool = False, compute_charge_gradients: bool = False, compute_dipole_gradients: bool = False,
                          compute_quadrupole_gradients: bool = False, compute_virial: bool = False):
    """What has to be ADDED to an unscaled electrostatic total so that every listed pair carries its scale factor.  For every stored entry
    e = (i, j, S) of the list with scale s_e = `pair_scales[e]`:

        E_i = 1/2 sum_{entries of row i} (s_e - 1) U_ij,     U_ij = L_i L_j (1 / r),     L = q + mu . grad + Q : grad grad

    U_ij is the COMPLETE bare pair energy of charges, dipoles and quadrupoles, all six terms (qq, q mu, mu mu, q Q, mu Q, Q Q): with
    R = r_j - r_i (+ S . cell), r = |R|, B0 = 1 / r, B1 = 1 / r^3, B_{n+1} = (2n + 1) B_n / r^2, c_i = mu_i . R, t_i = tr Q_i,
    s_i = R . Q_i . R,

        U_ij =   B0 q_i q_j + B1 (q_j c_i - q_i c_j + mu_i . mu_j) - B2 c_i c_j
               + q_i (B2 s_j - B1 t_j) + q_j (B2 s_i - B1 t_i)
               + B3 c_i s_j - B2 (2 mu_i.Q_j.R + t_j c_i) - B3 c_j s_i + B2 (2 mu_j.Q_i.R + t_i c_j)
               + B4 s_i s_j - B3 (t_i s_j + t_j s_i + 4 R.Q_i.Q_j.R) + B2 (t_i t_j + 2 Q_i:Q_j)

    i.e. the bare charge pair energy plus the pair energies of `coulomb_dipole_correction` and `coulomb_quadrupole_correction`.  Q follows
    their convention (the second Taylor coefficient; a traceless AMOEBA / Stone quadrupole Theta enters as Q = Theta / 3; 1/2 (Q + Q^T) of
    what is given is used).  s = 0 is an exclusion; an entry with s = 1 contributes exactly 0.0 and is skipped before any arithmetic.

    ADD it to the unscaled total, and every listed pair then carries the factor s_e:

        periodic:  `ewald_summation` / `particle_mesh_ewald` + `ewald_dipole_correction` / `pme_dipole_correction`
                   + `ewald_quadrupole_correction` / `pme_quadrupole_correction`
        cluster:   `coulomb_energy(alpha=0)` + `coulomb_dipole_correction` + `coulomb_quadrupole_correction` over an all-pairs list

    None of those operators changes.  The Ewald and mesh routines count every pair through their reciprocal part, whatever their real-space
    list holds, so the bare interaction is what has to be corrected.  `dipoles=None` and / or `quadrupoles=None` mean there are none; with
    both None this is the plain charge exclusion correction for `particle_mesh_ewald`.

    `pair_scales` has the shape of the index array -- [N, M] beside `neighbor_matrix`, [nnz] beside the [2, nnz] `neighbor_list` -- is
    float32 or float64 (converted to float64 inside) and is not differentiable (`requires_grad` raises NotImplementedError).  THE LIST MUST BE
    FULL (every pair stored from both ends) AND THE SCALES SYMMETRIC (s_ij = s_ji); neither is detected.  `bonded_pair_scales` builds both from
    the bonds of a topology.  A matrix entry equal to `mask_value` or outside [0, N) is padding (the scale of a padding slot is not looked
    at); entries with r <= 1e-8 are skipped.

    Images.  `cell=None` is a cluster: no shifts may be passed, `compute_virial` raises, `batch_idx` is not needed.  With a cell and shifts,
    R = r_j - r_i + S . cell as everywhere.  With a cell and `minimum_image=True` (shifts must not be passed) every entry's R is reduced
    to its minimum image in float64 (rint of the fractional components) and then rounded once to the positions dtype: a topology list built
    once keeps working when atoms are wrapped into the cell; the virial uses the reduced R.  With `batch_idx`, `cell` is [num_systems, 3, 3].

    Returns ``energies`` [N], or a tuple holding only what was asked for, in this order: energies, forces [N, 3], charge_grads [N],
    dipole_grads [N, 3], quadrupole_grads [N, 3, 3], virial [num_systems, 3, 3]; all in the positions dtype (sums in float64), with the
    meanings they have in `coulomb_quadrupole_correction`: forces = -dE/dr, charge_grads = dE/dq, dipole_grads = dE/dmu, quadrupole_grads =
    dE/dQ (symmetric), virial = -dE/d(strain) with the multipoles fixed in the laboratory frame (nine independent components, not
    symmetric; `multipole_frame_forces` returns the term local frames add).  dipole_grads of atom i does not depend on mu_i: minus
    dipole_grads is the field that the scaling removes at each atom, so the direct-field scaling of a polarisable model is
    `external_field += dipole_grads` of this operator called with the permanent multipoles and that model's field scales.

    Energies are differentiable once w.r.t. positions, charges, dipoles and quadrupoles, for any upstream gradient on the per-atom energies
    (the same kernel runs as its own adjoint: an entry weighs (g_i + g_j) / 2 . (s_e - 1)); the call then goes through the
    `alchemiops::_pair_scale_correction` op, as it does under `torch.compile`.  Differentiating the explicit forces, gradients or virial
    raises NotImplementedError, and so does a gradient w.r.t. cell: use `compute_virial`.  Out of scope: scale factors inside the stored mutual
    operator of `induced_dipoles`, Thole-damped scaled pairs, polarisation groups, dE/ds.  CPU tensors raise NativeLibraryError: there is no
    fallback."""
    M.check_positions_and_format(positions, neighbor_list, neighbor_matrix)
    n = positions.shape[0]
    dipoles = Q._dipoles_or_zeros(positions, dipoles)
    if quadrupoles is None:
        quadrupoles = torch.zeros((n, 3, 3), dtype=positions.dtype, device=positions.device)
    _check(positions, charges, dipoles, quadrupoles, pair_scales, cell, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
           neighbor_matrix_shifts, batch_idx, minimum_image, compute_virial)
    want = (True, compute_forces, compute_charge_gradients, compute_dipole_gradients, compute_quadrupole_gradients, compute_virial)
    if n == 0:
        return M.no_atoms(positions, M.num_systems(cell, batch_idx), M.QUADRUPOLE, want)
    return M.dispatch("pair_scale_correction_op", _forward, (positions, charges, dipoles, quadrupoles), (pair_scales, cell),
                      (batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts, int(mask_value),
                       bool(minimum_image)), want)


# ---- topology helper (host, once per topology) ------------------------------------------------------------------------------------------
BondedPairScales = collections.namedtuple("BondedPairScales", ["neighbor_matrix", "pair_scales", "num_neighbors"])


def bonded_pair_scales(bonds, num_atoms: int, scales=(0.0, 0.0, 0.4, 0.8), *, dtype: torch.dtype = torch.float64, device=None):
    """The full, symmetric list of scaled pairs of a bonded topology, as `pair_scale_correction` takes it.

    `bonds` is [B, 2] (tensor, array or nested sequence of atom indices), `scales[d - 1]` the factor of a pair whose SHORTEST bond path has d
    bonds (the default is AMOEBA's permanent-multipole set for 1-2, 1-3, 1-4, 1-5): in a five-ring the atom reachable by two bonds one way
    and three the other is a 1-3 pair.  Pairs further apart than `len(scales)` bonds are not listed, and neither are pairs whose scale is
    exactly 1 (they would contribute nothing).  Duplicate bonds (in either direction) are merged; a self bond or an index outside
    [0, num_atoms) raises ValueError.  A batch of molecules is just a disjoint graph.

    Runs on the host with numpy (a breadth-first search from every atom, all atoms one level at a time), like the host check of
    `LocalFrames`; call it once per topology.  Returns the named tuple `BondedPairScales(neighbor_matrix [N, M] int32 padded with N,
    pair_scales [N, M] in `dtype` (1 on padding), num_neighbors [N] int32)` on `device`; rows are sorted by neighbour index."""
    n = int(num_atoms)
    if n < 0:
        raise ValueError(f"num_atoms must not be negative, got {num_atoms}")
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"dtype must be float32 or float64, got {dtype}")
    b = bonds.detach().cpu().numpy() if isinstance(bonds, torch.Tensor) else np.asarray(bonds)
    if b.size == 0:
        b = b.reshape(0, 2)
    if b.ndim != 2 or b.shape[1] != 2:
        raise ValueError(f"bonds must have shape [num_bonds, 2], got {tuple(b.shape)}")
    if b.size and not np.issubdtype(b.dtype, np.integer):
        raise ValueError(f"bonds must hold integer atom indices, got dtype {b.dtype}")
    b = b.astype(np.int64)
    if b.size and (b.min() < 0 or b.max() >= n):
        raise ValueError(f"bonds must hold atom indices in [0, {n}), got values from {int(b.min())} to {int(b.max())}")
    if bool((b[:, 0] == b[:, 1]).any()):
        raise ValueError(f"a bond joins an atom to itself: atom {int(b[b[:, 0] == b[:, 1]][0, 0])}")
    scales = tuple(float(s) for s in scales)
    # adjacency as CSR, every bond from both ends, duplicates merged
    keys = np.unique(np.concatenate([b[:, 0] * n + b[:, 1], b[:, 1] * n + b[:, 0]])) if b.size else np.zeros(0, dtype=np.int64)
    adj = keys % max(n, 1)
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(keys // max(n, 1), minlength=n), out=ptr[1:])
    # breadth-first search from every atom at once: `seen` holds source * n + atom of every pair met so far, the sources themselves included
    seen = np.arange(n, dtype=np.int64) * (n + 1)
    src, node = np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64)
    found_keys, found_scale = [], []
    for s in scales:
        deg = ptr[node + 1] - ptr[node]
        total = int(deg.sum())
        if total == 0:
            break
        first = np.cumsum(deg) - deg
        slots = np.arange(total, dtype=np.int64) - np.repeat(first, deg) + np.repeat(ptr[node], deg)
        new = np.unique(np.repeat(src, deg) * n + adj[slots])
        new = new[~np.isin(new, seen, assume_unique=True)]
        seen = np.union1d(seen, new)
        src, node = new // n, new % n
        if s != 1.0:
            found_keys.append(new)
            found_scale.append(np.full(new.shape[0], s))
    if found_keys:
        keys = np.concatenate(found_keys)
        order = np.argsort(keys, kind="stable")
        keys, vals = keys[order], np.concatenate(found_scale)[order]
    else:
        keys, vals = np.zeros(0, dtype=np.int64), np.zeros(0)
    rows, cols = (keys // n, keys % n) if n else (keys, keys)
    counts = np.bincount(rows, minlength=n)
    m = int(counts.max()) if n else 0
    nm = np.full((n, m), n, dtype=np.int32)
    sc = np.ones((n, m), dtype=np.float64)
    slot = np.arange(keys.shape[0], dtype=np.int64) - np.repeat(np.cumsum(counts) - counts, counts)
    nm[rows, slot] = cols
    sc[rows, slot] = vals
    return BondedPairScales(torch.as_tensor(nm, device=device), torch.as_tensor(sc, device=device).to(dtype),
                            torch.as_tensor(counts.astype(np.int32), device=device))


__all__ = ["pair_scale_correction", "bonded_pair_scales", "BondedPairScales"]
