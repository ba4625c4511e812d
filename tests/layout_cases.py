"""The fixtures of the layout sweeps of `dftd4`, `dftd4_atm`, `gaussian_charge_correction`, `charge_equilibration`, the two point-dipole
operators, `ewald_quadrupole_correction`, `thole_dipole_correction`, the induced-dipole solves, `pair_scale_correction`, the local-frame functions and
`cluster_induced_dipoles` (tests/test_arg_layouts_gpu.py), in one place and free of any device, so that the CPU suite can check on exactly these inputs the condition
that makes such a sweep worth running (tests/test_layout_sensitivity_cpu.py): a tensor argument that the entry point misreads by one row
must move the result far beyond the bar the sweep applies.  Every reference is computed once and never modified.

    system(n, seed, box)        the lattice builder of the layout tests: float32 values throughout, so float32 <-> float64 variants are equal-valued
    d4(batch, compact)          the D4 fixtures: 130 atoms in a 24 Bohr triclinic box / 70 + 60 atoms in boxes 24 and 22 (compact blocks) /
                                a compact block of 130 atoms in a box of 22 for the table sweeps of `dftd4_atm`
    gaussian(dtype, batch)      130 atoms in the 12 Bohr box / 70 + 60 in boxes 12 and 11, widths in [0.3, 0.8], two point atoms per system
    qeq_cluster(), qeq_periodic()   two clusters (no cell) / two periodic systems with their own k-vectors and alpha
    dipole(batch)               the Gaussian fixture's boxes with point dipoles, per-system alpha, a k set and a mesh: both dipole operators
    quadrupole(batch)           `dipole(batch)` plus quadrupoles (two zero rows and four unsymmetric rows per system)
    pme_quadrupole(batch)       `quadrupole(batch)` on mesh `DP_MESH` at order 6 (the dipole fixture covers order 5): `pme_quadrupole_correction`
    thole(batch)                `dipole(batch)` plus polarisabilities in [2, 8] (two non-polarisable atoms per system), width 0.39
    induced(batch)              an `induced_cases` lattice (l64 / l27 + l64) in float32 numbers with its full list, k set, an external field and
                                a warm start; polarisabilities for the undamped and for the damped solve
    pair_scale(batch)           `quadrupole(batch)` with its brute-force list and one scale per entry by distance class (0, 0.375, 1, 0.75)
    frames(batch)               a local-frame topology of every kind over 130 / 70 + 60 atoms, wrapped into the boxes of `system`
    cluster_induced()           the three clusters of tests/cluster_multipole_reference.py in float32 numbers, a field and a warm start

Why the D4 fixture is not the 12 Bohr box of the other sweeps: there the coordination numbers reach 18 while the `cn_ref` of
`d4_test_tables` lie in [0, 1]; every Gaussian weight saturates on the reference nearest to 1, and rolling `ngw` by one row moves the
float64 restatement by only 3.6 x the bar.  At 24 Bohr the coordination numbers stay inside the range of the references.
"""
import functools

import numpy as np
import torch

from tests import d4_atm_cases as K3
from tests import d4_atm_reference as R3
from tests import d4_cases as K
from tests import d4_reference as R
from tests import dipole_reference as DR
from tests import gaussian_reference as GR
from tests import induced_cases as IC
from tests import induced_reference as IR
from tests import pme_dipole_reference as PR
from tests import pme_quadrupole_reference as PQR
from tests import qeq_reference as QR
from tests import quadrupole_reference as XR
from tests import systems as S
from tests import thole_reference as TR

N, NA, NB = 130, 70, 60
F64 = torch.float64


def system(n, seed, box):
    """The first n sites of a jittered FCC lattice (no unphysical contacts) sheared into the triclinic cell `random_box` uses; neutral
    +-1 charges; Z drawn from 4 species.  Every value is a float32 number, so float32 <-> float64 variants are equal-valued."""
    pos, cell, q, _ = S.fcc_box(n, a=box / 4.0, jitter=0.05, seed=seed, dtype=np.float32)
    tri = np.array([[box, 0.0, 0.0], [0.25 * box, 0.9 * box, 0.0], [0.1 * box, -0.2 * box, 1.1 * box]])
    pos = ((pos.astype(np.float64) / float(cell[0, 0])) @ tri).astype(np.float32)
    z = np.random.default_rng(seed).choice(np.array([1, 6, 8, 17], np.int32), n)
    return pos, tri.astype(np.float32), q.astype(np.float32), z


def compact_system(n, seed, box):
    """As `system`, but the n sites of the 256-site lattice NEAREST TO THE CENTRE of the cell: a compact block, whose atoms have their
    full shells of (unlike) neighbours, where the first n sites are one or two slabs."""
    pos, cell, q, _ = S.fcc_box(256, a=box / 4.0, jitter=0.05, seed=seed, dtype=np.float32)
    tri = np.array([[box, 0.0, 0.0], [0.25 * box, 0.9 * box, 0.0], [0.1 * box, -0.2 * box, 1.1 * box]])
    pos = (pos.astype(np.float64) / float(cell[0, 0])) @ tri
    sel = np.sort(np.argsort(np.linalg.norm(pos - np.full(3, 0.5) @ tri, axis=1), kind="stable")[:n])
    z = np.random.default_rng(seed).choice(np.array([1, 6, 8, 17], np.int32), n)
    return pos[sel].astype(np.float32), tri.astype(np.float32), q[sel].astype(np.float32), z


def _join(parts):
    """[(pos, cell, q, z), ...] -> pos, cells [B, 3, 3], q, z, batch_idx (None for one system)."""
    bi = None if len(parts) == 1 else np.concatenate([np.full(len(p[0]), k, np.int32) for k, p in enumerate(parts)])
    return np.concatenate([p[0] for p in parts]), np.stack([p[1] for p in parts]), np.concatenate([p[2] for p in parts]), np.concatenate([p[3] for p in parts]), bi


# ---- dftd4 / dftd4_atm -------------------------------------------------------------------------------------------------------------------

D4_RC, D4_RC3 = 9.0, 7.0
D4_KEYS = ("energy", "forces", "cn", "charge_grad", "virial")
D4_EXTRA = {"energy": 0.0, "forces": 5e-6, "cn": 0.0, "charge_grad": 5e-6, "virial": 2e-7}  # tests/test_d4_gpu.py::EXTRA
ATM_KEYS = ("energy", "forces", "virial")


@functools.lru_cache(maxsize=None)
def d4(batch=False, compact=False):
    """single: `system(130, 7, 24.0)`.  batch: 70 + 60 atoms in boxes 24 and 22, as compact blocks -- as the first sites of the lattice
    (slabs: largest coordination number 0.04) rolled `en` moves the restatement of `dftd4` by 0.45 bars and that of `dftd4_atm` by 0.05.
    compact: one compact block of 130 atoms in a box of 22, the fixture the table sweeps of `dftd4_atm` run on besides the single
    system, on which rolled `en` moves the three-body term by 66 bars only."""
    assert not (batch and compact)
    parts = [compact_system(NA, 8, 24.0), compact_system(NB, 9, 22.0)] if batch else [compact_system(N, 7, 22.0) if compact else system(N, 7, 24.0)]
    pos, cell, q, z, bi = _join(parts)
    return dict(pos=pos, cell=cell, q=(0.3 * q.astype(np.float64)).astype(np.float32), z=z, batch_idx=bi, tables=R.d4_test_tables(17))


def d4_reference(batch=False, compact=False, work_dtype=F64, **replace):
    """The restatement of `dftd4` on the fixture, with `q=` or single tables (`ngw=`, ...) replaced."""
    c = d4(batch, compact)
    tables = {**c["tables"], **{k: v for k, v in replace.items() if k != "q"}}
    return R.reference(c["pos"], c["z"], replace.get("q", c["q"]), tables, list_cutoff=D4_RC, cell=c["cell"], batch_idx=c["batch_idx"],
                       work_dtype=work_dtype, **K.BJ)


@functools.lru_cache(maxsize=None)
def d4_references(batch=False, compact=False):
    return d4_reference(batch, compact), d4_reference(batch, compact, torch.float32)


def d4_atm_reference(batch=False, compact=False, work_dtype=F64, **replace):
    """The restatement of `dftd4_atm` on the fixture at s9 = 1 (the term is linear in s9)."""
    c = d4(batch, compact)
    return R3.reference(c["pos"], c["z"], {**c["tables"], **replace}, K3.BJ["a1"], K3.BJ["a2"], D4_RC, three_body_cutoff=D4_RC3, s9=1.0,
                        cell=c["cell"], batch_idx=c["batch_idx"], work_dtype=work_dtype)


@functools.lru_cache(maxsize=None)
def d4_atm_unit_references(batch=False, compact=False):
    return d4_atm_reference(batch, compact), d4_atm_reference(batch, compact, torch.float32)


def d4_atm_s9(batch=False, compact=False):
    """The smallest power of ten `tests/d4_atm_cases.lifted` accepts for the fixture's restatement (the rule of every `dftd4_atm` case)."""
    r64, s9 = d4_atm_unit_references(batch, compact)[0], 1.0
    while not K3.lifted(r64, s9):
        s9 *= 10.0
        assert s9 <= 1e12
    return s9


def d4_atm_references(batch=False, compact=False):
    s9 = d4_atm_s9(batch, compact)
    return tuple(K3._scaled(r, s9) for r in d4_atm_unit_references(batch, compact))


def d4_bar(r64, r32, key, extra=D4_EXTRA):
    """The elementwise bar tests/test_d4_gpu.py::_bars and tests/test_d4_atm_gpu.py::_bars apply to the quantity `key`."""
    ref = r64[key]
    dev32 = np.abs(r32[key] - ref).max() if ref.size else 0.0
    return 4.0 * np.maximum(dev32, 1e-6 + 1e-6 * np.abs(ref) + extra[key] * (np.abs(ref).max() if ref.size else 0.0))


# ---- gaussian_charge_correction ----------------------------------------------------------------------------------------------------------

GC_RC = 7.0  # the cutoff of tests/test_gaussian_charges_gpu.py
GC_NAMES = ("energies", "forces", "charge_grads", "sigma_grads", "virial")


@functools.lru_cache(maxsize=None)
def gaussian(batch=False):
    """The box of the layout tests with charges 0.5 q + 0.125 (a charged cell: the background term and its per-system sums take part),
    widths in [0.3, 0.8] and two point atoms (sigma = 0) per system; all float32 numbers."""
    parts = [system(NA, 8, 12.0), system(NB, 9, 11.0)] if batch else [system(N, 7, 12.0)]
    pos, cell, q, _, bi = _join(parts)
    g = np.random.default_rng(17 + batch)
    sigma = g.uniform(0.3, 0.8, len(pos)).astype(np.float32)
    off = 0
    for p in parts:
        sigma[off + g.choice(len(p[0]), 2, replace=False)] = 0.0
        off += len(p[0])
    return dict(pos=pos, cell=cell, q=(0.5 * q + 0.125).astype(np.float32), sigma=sigma, batch_idx=bi)


def _entries(pos, cells, bi, cutoff):
    """(i, j, S) of the full list with this cutoff, system by system (images up to +-1: the boxes are wider than the cutoff)."""
    bi = np.zeros(len(pos), np.int64) if bi is None else bi
    out = []
    for s, cell in enumerate(cells):
        sel = np.nonzero(bi == s)[0]
        i, j, sh = GR.brute_force_entries(pos[sel].astype(np.float64), cell.astype(np.float64), cutoff, 1)
        out.append((torch.as_tensor(sel)[i], torch.as_tensor(sel)[j], sh))
    return tuple(torch.cat([o[k] for o in out]) for k in range(3))


def gaussian_reference(batch=False, distance_dtype=F64, **replace):
    c = {**gaussian(batch), **replace}
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))  # noqa: E731
    bi = None if c["batch_idx"] is None else torch.as_tensor(c["batch_idx"])
    ent = _entries(c["pos"], c["cell"], c["batch_idx"], GC_RC)
    return GR.evaluate(t(c["pos"]), t(c["q"]), t(c["sigma"]), t(c["cell"]), *ent, batch_idx=bi, distance_dtype=distance_dtype)


# ---- charge_equilibration ----------------------------------------------------------------------------------------------------------------

QEQ_TOL = 1e-10


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def qeq_cluster(sizes=(37, 33), seed=71):
    """Clusters with all-pairs full lists (`systems.clusters`, the recipe tests/test_qeq_gpu.py::_cluster uses), float32 numbers in
    float64 arrays."""
    g, pos, bi, ii, jj, sigma = S.clusters(sizes, seed)
    n = len(pos)
    i, j = torch.as_tensor(ii), torch.as_tensor(jj)
    return dict(n=n, nsys=len(sizes), pos=_f32(pos), cell=None, batch_idx=bi, sigma=_f32(sigma),
                chi=_f32(g.normal(size=n)), hard=_f32(g.uniform(1.0, 2.0, n)), q0=_f32(g.uniform(-0.2, 0.2, n)), total=_f32([1.5, -0.25]),
                ent=(i, j, torch.zeros((i.shape[0], 3), dtype=torch.long)), width=max(sizes) + 1)


@functools.lru_cache(maxsize=None)
def qeq_periodic(same_cell=False):
    """40 atoms in a triclinic box 9 (charged) and 55 atoms in a cubic box 10 (neutral), cutoff 6 (the recipe of
    tests/test_qeq_gpu.py::_periodic_batch), with the half-space k-vectors of cutoff 3.2 and one alpha per system.  `same_cell`: both
    systems in the triclinic box, for the stride-0 expansion of `cell`."""
    from nvalchemiops.interactions.electrostatics import generate_k_vectors_ewald_summation

    g = np.random.default_rng(72)
    tri = lambda b: np.array([[b, 0, 0], [0.2 * b, 0.9 * b, 0], [0.1 * b, -0.15 * b, 1.1 * b]])  # noqa: E731
    cells = _f32(np.stack([tri(9.0), tri(9.0) if same_cell else np.eye(3) * 10.0]))
    pos = _f32(np.concatenate([g.uniform(0, 1, (40, 3)) @ cells[0], g.uniform(0, 1, (55, 3)) @ cells[1]]))
    bi = np.array([0] * 40 + [1] * 55, np.int32)
    ent = _entries(pos, cells, bi, 6.0)
    n = 95
    sigma = g.uniform(0.3, 0.8, n)
    sigma[[5, 60]] = 0.0
    # (the package's own generator, pure torch, as tests/test_qeq_gpu.py uses it: the k-vectors are an INPUT of the solve and of the dense
    # restatement alike, so which set they are does not enter the comparison)
    kv = generate_k_vectors_ewald_summation(torch.as_tensor(cells), 3.2)
    return dict(n=n, nsys=2, pos=pos, cell=cells, batch_idx=bi, sigma=_f32(sigma), chi=_f32(g.normal(size=n)), hard=_f32(g.uniform(1.0, 2.0, n)),
                q0=_f32(g.uniform(-0.2, 0.2, n)), total=_f32([1.25, 0.0]), alpha=_f32([0.45, 0.42]), kv=kv.numpy(), ent=ent,
                width=int(torch.bincount(ent[0]).max()) + 5)


def qeq_dense(c, device="cpu", **replace):
    """(H, chi, per-system totals, batch_idx) of the dense float64 restatement of a QEq fixture on `device`, with arguments replaced."""
    c = {**c, **replace}
    t = lambda a: None if a is None else torch.as_tensor(np.asarray(a), device=device)  # noqa: E731
    ent = tuple(e.to(device) for e in c["ent"])
    periodic = c["cell"] is not None
    h = QR.dense_operator(t(c["pos"]), t(c["sigma"]), t(c["hard"]), t(c["cell"]), t(c["alpha"]) if periodic else None, t(c["kv"]) if periodic else None,
                          *ent, batch_idx=t(c["batch_idx"]), **(dict(erfc_lr=QR.erfc_as) if periodic else {}))
    return h, t(c["chi"]), t(c["total"]), t(c["batch_idx"])


def qeq_charge_bound(h, chi, total, bi, nsys, tol=QEQ_TOL):
    """Per system: the bound tests/test_qeq_gpu.py::_check_solution derives from the dense operator for |q - q_ref|,
    10 tol ||b|| / lambda_min + 1e-14, b the projected gradient at the uniform start."""
    counts = torch.bincount(bi.long(), minlength=nsys).to(F64)
    b_norm = QR.projected_residual(h, chi, (total / counts)[bi.long()], bi, nsys)
    out = []
    for s in range(nsys):
        m = torch.nonzero(bi == s).flatten()
        out.append(10.0 * tol * float(b_norm[s]) / float(torch.linalg.eigvalsh(h[m][:, m]).min()) + 1e-14)
    return out


# ---- ewald_dipole_correction and pme_dipole_correction -----------------------------------------------------------------------------------

DP_ALPHA = (0.4, 0.375)
DP_K_CUTOFF, DP_MESH, DP_ORDER = 2.2, (12, 10, 14), 5
DP_NAMES = ("energies", "forces", "charge_grads", "dipole_grads", "virial")


@functools.lru_cache(maxsize=None)
def dipole(batch=False):
    """The boxes of the Gaussian fixture (130 atoms in the 12 Bohr box / 70 + 60 in boxes 12 and 11, list cutoff `GC_RC`), charges
    0.5 q + 0.125, dipoles 0.4 x normal with two zero rows per system, one alpha per system, and the package's half-space k set of cutoff
    2.2 ([K, 3] / [B, K, 3]).  Every value is a float32 number -- the k-vectors too, rounded after they were generated: they are an input of
    the kernels and of the restatement alike -- so float32 <-> float64 variants are equal-valued."""
    from nvalchemiops.interactions.electrostatics import generate_k_vectors_ewald_summation

    parts = [system(NA, 8, 12.0), system(NB, 9, 11.0)] if batch else [system(N, 7, 12.0)]
    pos, cell, q, _, bi = _join(parts)
    g = np.random.default_rng(27 + batch)
    mu = (0.4 * g.normal(size=(len(pos), 3))).astype(np.float32)
    off = 0
    for p in parts:
        mu[off + g.choice(len(p[0]), 2, replace=False)] = 0.0
        off += len(p[0])
    cells = torch.as_tensor(cell.astype(np.float64))
    kv = generate_k_vectors_ewald_summation(cells if batch else cells[0], DP_K_CUTOFF).numpy().astype(np.float32)
    return dict(pos=pos, cell=cell, q=(0.5 * q + 0.125).astype(np.float32), mu=mu, alpha=np.array(DP_ALPHA[:len(parts)], np.float32), kv=kv, batch_idx=bi)


def dipole_reference(batch=False, op="ewald", dtype=F64, **replace):
    """The restatement of `ewald_dipole_correction` (op "ewald": the full list of cutoff `GC_RC` and the fixture's k set; `dtype` float32 is
    its float32-distance mode) or of `pme_dipole_reciprocal_space` (op "pme": mesh `DP_MESH`, order `DP_ORDER`; `dtype` float32 is its
    float32 mode) on the fixture, with arguments replaced."""
    c = {**dipole(batch), **replace}
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))  # noqa: E731
    bi = None if c["batch_idx"] is None else torch.as_tensor(c["batch_idx"])
    if op == "pme":
        return PR.evaluate(t(c["pos"]), t(c["q"]), t(c["mu"]), t(c["cell"]), t(c["alpha"]), DP_MESH, DP_ORDER, batch_idx=bi, dtype=dtype)
    ent = _entries(c["pos"], c["cell"], c["batch_idx"], GC_RC)
    return DR.evaluate(t(c["pos"]), t(c["q"]), t(c["mu"]), t(c["cell"]), t(c["alpha"]), ent, t(c["kv"]), batch_idx=bi, distance_dtype=dtype)


# ---- ewald_quadrupole_correction and thole_dipole_correction -----------------------------------------------------------------------------

QD_NAMES = ("energies", "forces", "charge_grads", "dipole_grads", "quadrupole_grads", "virial")
TH_NAMES = ("energies", "forces", "charge_grads", "dipole_grads", "polar_grads", "virial")
THOLE = 0.39


def _per_system_rows(g, sizes, count):
    """`count` distinct rows of every system, as indices into the joined arrays."""
    off, rows = 0, []
    for n in sizes:
        rows.append(off + g.choice(n, count, replace=False))
        off += n
    return rows


@functools.lru_cache(maxsize=None)
def quadrupole(batch=False):
    """`dipole(batch)` plus quadrupoles 0.3 x normal, symmetrised; per system two zero rows and four rows with an added antisymmetric part
    (1/2 (Q + Q^T) is what counts: a sweep that reads Q transposed must still agree).  Float32 numbers."""
    c = dict(dipole(batch))
    g = np.random.default_rng(37 + batch)
    qd = 0.3 * g.normal(size=(len(c["pos"]), 3, 3))
    qd = 0.5 * (qd + qd.transpose(0, 2, 1))
    for rows in _per_system_rows(g, (NA, NB) if batch else (N,), 6):
        qd[rows[:2]] = 0.0
        skew = 0.1 * g.normal(size=(4, 3, 3))
        qd[rows[2:]] += skew - skew.transpose(0, 2, 1)
    c["qd"] = qd.astype(np.float32)
    return c


def quadrupole_reference(batch=False, part="total", dtype=F64, **replace):
    """The restatement of `ewald_quadrupole_correction` ("total"), its real-space half ("real") or its reciprocal half ("recip") on the
    fixture: the full list of cutoff `GC_RC` (brute-force entries) and the fixture's k set; `dtype` float32 is the float32-distance mode."""
    c = {**quadrupole(batch), **replace}
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))  # noqa: E731
    bi = None if c["batch_idx"] is None else torch.as_tensor(c["batch_idx"])
    ent = _entries(c["pos"], c["cell"], c["batch_idx"], GC_RC) if part != "recip" else None
    return XR.evaluate(t(c["pos"]), t(c["q"]), t(c["mu"]), t(c["qd"]), t(c["cell"]), t(c["alpha"]), ent, t(c["kv"]) if part != "real" else None,
                       batch_idx=bi, distance_dtype=dtype)


PQ_ORDER = 6


def pme_quadrupole(batch=False):
    """`quadrupole(batch)`: the mesh operator takes the same inputs, on mesh `DP_MESH` at order `PQ_ORDER`."""
    return quadrupole(batch)


def pme_quadrupole_reference(batch=False, dtype=F64, **replace):
    """The restatement of `pme_quadrupole_reciprocal_space` (tests/pme_quadrupole_reference.py) on the fixture, mesh `DP_MESH`, order
    `PQ_ORDER`; `dtype` float32 is its float32 mode."""
    c = {**pme_quadrupole(batch), **replace}
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))  # noqa: E731
    bi = None if c["batch_idx"] is None else torch.as_tensor(c["batch_idx"])
    return PQR.evaluate(t(c["pos"]), t(c["q"]), t(c["mu"]), t(c["qd"]), t(c["cell"]), t(c["alpha"]), DP_MESH, PQ_ORDER, batch_idx=bi, dtype=dtype)


@functools.lru_cache(maxsize=None)
def pme_quadrupole_references(batch=False):
    return pme_quadrupole_reference(batch), pme_quadrupole_reference(batch, torch.float32)


@functools.lru_cache(maxsize=None)
def thole(batch=False):
    """`dipole(batch)` plus polarisabilities uniform in [2, 8] with two non-polarisable atoms (0) per system; width `THOLE`.  At these values
    E = a_T r^3 / sqrt(a_i a_j) is 0.5 - 2 on the nearest neighbours (distance 2.1) and passes 50 inside the list cutoff for the smallest
    polarisabilities, so both sides of the kernel's early exit are present."""
    c = dict(dipole(batch))
    g = np.random.default_rng(37 + batch)
    polar = g.uniform(2.0, 8.0, len(c["pos"]))
    for rows in _per_system_rows(g, (NA, NB) if batch else (N,), 2):
        polar[rows] = 0.0
    c["polar"] = polar.astype(np.float32)
    return c


def thole_reference(batch=False, dtype=F64, **replace):
    """The restatement of `thole_dipole_correction` on the fixture (brute-force entries of cutoff `GC_RC`)."""
    c = {**thole(batch), **replace}
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))  # noqa: E731
    bi = None if c["batch_idx"] is None else torch.as_tensor(c["batch_idx"])
    ent = _entries(c["pos"], c["cell"], c["batch_idx"], GC_RC)
    return TR.evaluate(t(c["pos"]), t(c["q"]), t(c["mu"]), t(c["polar"]), t(c["cell"]), THOLE, ent, batch_idx=bi, distance_dtype=dtype)


# ---- induced_dipoles and thole_induced_dipoles -------------------------------------------------------------------------------------------

IND_TOL = 1e-10


@functools.lru_cache(maxsize=None)
def induced(batch=False):
    """The lattices of tests/induced_cases.py rounded to float32: l64 as one system / l27 + l64 as a batch with their own cells and alpha
    (l64: 0.45, l27: 0.625), the full list of every image within the cases' cutoff 11, the package's k set of the cases' k_cutoff per
    system (rounded to float32 after it was generated), an external field and a warm start drawn once.  At 0.625 the k sum of cutoff 3.2 is
    truncated at exp(-k^2 / 4 alpha^2) = 1.4e-3, on purpose: device and dense restatement sum the same terms, and with two converged
    parameter sets (0.45 and 0.4375) the operator would not depend on which alpha a system is given -- rolled `alpha` then moved the dense
    solution by 1.25 x (2 x bound) only, where tests/test_layout_sensitivity_cpu.py demands 100.  `polar` are the cases'
    polarisabilities (the undamped solve); `polar_thole` are those of the damped solve, drawn as the Thole fixture's: uniform in [2, 8] --
    of the order of d_min^3 = 8, where the undamped operator is indefinite -- with two non-polarisable atoms (0) per system."""
    from nvalchemiops.interactions.electrostatics import generate_k_vectors_ewald_summation

    names = ("l27", "l64") if batch else ("l64",)
    parts = [IC.lattice(k) for k in names]
    pos = _f32(np.concatenate([p["pos"] for p in parts]))
    cells = _f32(np.stack([p["cell"] for p in parts]))
    sizes = [p["n"] for p in parts]
    bi = None if not batch else np.repeat(np.arange(len(parts), dtype=np.int32), sizes)
    off, ii, jj, ss = 0, [], [], []
    for p, cell in zip(parts, cells):
        i, j, sh = GR.brute_force_entries(pos[off:off + p["n"]], cell, IC.EWALD["cutoff"], 2)
        ii.append(i + off); jj.append(j + off); ss.append(sh)  # noqa: E702
        off += p["n"]
    ent = (torch.cat(ii), torch.cat(jj), torch.cat(ss))
    g = np.random.default_rng(37 + batch)
    n = len(pos)
    kv = generate_k_vectors_ewald_summation(torch.as_tensor(cells), IC.EWALD["k_cutoff"]).numpy().astype(np.float32).astype(np.float64)
    polar = _f32(np.concatenate([p["polar"] for p in parts]))
    field, start = _f32(0.1 * g.normal(size=(n, 3))), _f32(0.05 * g.normal(size=(n, 3)))
    polar_thole = g.uniform(2.0, 8.0, n)
    for rows in _per_system_rows(g, sizes, 2):
        polar_thole[rows] = 0.0
    return dict(n=n, nsys=len(parts), pos=pos, cell=cells, q=_f32(np.concatenate([p["q"] for p in parts])), polar=polar, polar_thole=_f32(polar_thole),
                alpha=_f32([0.625, 0.45][-len(parts):]), kv=kv if batch else kv.reshape(-1, 3), batch_idx=bi, ent=ent, field=field, start=start,
                width=int(torch.bincount(ent[0]).max()) + 3)


def induced_dense(c, thole=None, device="cpu", **replace):
    """dict(H, b, polar, bi) of the dense float64 restatement of an induced-dipole fixture on `device`: undamped with `polar`, damped
    (`thole`) with `polar_thole`; arguments replaced by name (`polar` replaces whichever of the two is in use)."""
    c = {**c, **replace}
    t = lambda a: None if a is None else torch.as_tensor(np.asarray(a), device=device)  # noqa: E731
    ent = tuple(e.to(device) for e in c["ent"])
    polar = t(c["polar"] if thole is None or "polar" in replace else c["polar_thole"])
    bi = t(c["batch_idx"])
    if thole is None:
        T, lin = IR.dipole_operator(t(c["pos"]), t(c["q"]), t(c["cell"]), t(c["alpha"]), ent, t(c["kv"]), batch_idx=bi)
    else:
        T, lin = TR.damped_operator(t(c["pos"]), t(c["q"]), polar, t(c["cell"]), t(c["alpha"]), thole, ent, t(c["kv"]), batch_idx=bi)
    return dict(H=IR.system_matrix(T, polar), b=IR.right_hand_side(lin, polar, t(c["field"])), polar=polar, bi=bi)


def induced_bound(d, nsys, tol=IND_TOL):
    """Per system: the bound `_check_solution` of tests/test_induced_gpu.py derives from the dense operator for |mu - mu_ref|,
    10 tol ||b|| / lambda_min + 1e-14."""
    n = d["b"].shape[0] // 3
    sys_of = (torch.zeros(n, dtype=torch.long, device=d["b"].device) if d["bi"] is None else d["bi"].long()).repeat_interleave(3)
    out = []
    for s in range(nsys):
        m = torch.nonzero(sys_of == s).flatten()
        out.append(10.0 * tol * float(d["b"][m].norm()) / float(torch.linalg.eigvalsh(d["H"][m][:, m]).min()) + 1e-14)
    return out


# ---- pair_scale_correction -----------------------------------------------------------------------------------------------------------------

PS_EDGES, PS_SCALES = (3.3, 4.5, 5.85), (0.0, 0.375, 1.0, 0.75)  # float32 numbers, as every value of these fixtures; the edges lie between neighbour shells of the lattice (3.0 | 3.7, 4.2 | 4.7, 5.6 | 6.0)
PS_IMAGE_MARGIN = 0.45                                        # largest |fractional component| of a pair kept for the `minimum_image` calls


def pair_vectors(pos, cells, batch_idx, i, j, S):
    """[E, 3] float64 torch: (r_j - r_i) + S . cell, formed so that the mirror entry (j, i, -S) gives exactly the negative; and the same
    vectors in fractional coordinates."""
    pos, cells = pos.to(F64), cells.to(F64).reshape(-1, 3, 3)
    c = cells[torch.zeros_like(i) if batch_idx is None else batch_idx.long()[i]]
    d = (pos[j] - pos[i]) + torch.einsum("ea,eab->eb", S.to(F64), c)
    return d, torch.einsum("ea,eab->eb", d, torch.linalg.inv(c))


def distance_class_scales(pos, cells, batch_idx, i, j, S):
    """One scale per stored entry from its distance class (`PS_EDGES`, `PS_SCALES`): symmetric by construction, the third class is exactly 1."""
    r = pair_vectors(pos, cells, batch_idx, i, j, S)[0].norm(dim=1)
    return torch.tensor(PS_SCALES, dtype=F64, device=r.device)[torch.bucketize(r, torch.tensor(PS_EDGES, dtype=F64, device=r.device))]


def minimum_image_entries(pos, cells, batch_idx, i, j, S):
    """Mask of the entries whose stored shift already is the minimum image, with every fractional component at most `PS_IMAGE_MARGIN`:
    an entry and its mirror are kept or dropped together."""
    return (pair_vectors(pos, cells, batch_idx, i, j, S)[1].abs() <= PS_IMAGE_MARGIN).all(dim=1)


@functools.lru_cache(maxsize=None)
def pair_scale(batch=False):
    """`quadrupole(batch)` with the full list of cutoff `GC_RC` (brute-force entries `ent`) and one scale per entry by distance class."""
    c = dict(quadrupole(batch))
    c["ent"] = _entries(c["pos"], c["cell"], c["batch_idx"], GC_RC)
    bi = None if c["batch_idx"] is None else torch.as_tensor(c["batch_idx"])
    c["scales"] = distance_class_scales(torch.as_tensor(c["pos"]), torch.as_tensor(c["cell"]), bi, *c["ent"]).numpy()
    return c


def pair_scale_reference(batch=False, dtype=F64, **replace):
    """The restatement of `pair_scale_correction` (tests/pair_scale_reference.py) on the fixture with explicit shifts."""
    from tests import pair_scale_reference as PSR

    c = {**pair_scale(batch), **replace}
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))  # noqa: E731
    bi = None if c["batch_idx"] is None else torch.as_tensor(c["batch_idx"])
    return PSR.evaluate(t(c["pos"]), t(c["q"]), t(c["mu"]), t(c["qd"]), t(c["scales"]), c["ent"], cell=t(c["cell"]), batch_idx=bi, distance_dtype=dtype)


# ---- LocalFrames, rotate_multipoles, multipole_frame_forces ----------------------------------------------------------------------------------

FR_NAMES = ("dipoles", "quadrupoles", "positions_grad", "local_dipole_grads", "local_quadrupole_grads", "virial")
FR_MOLECULES = ("none", "z_only", "z_only_y", "water", "ammonia", "z_bisect", "chiral", "mirror")


def frame_conditions(pos, atoms, kinds, cell=None, batch_idx=None):
    """What the bars of tests/test_local_frames_gpu.py assume of a geometry, measured: dict(bond=(min, max) length of a frame vector,
    angle=(min, max) in degrees between two frame vectors of an atom, z_only=smallest | |e_z . x| - 0.866 | of a Z_ONLY atom, chiral=smallest
    |d_y . (d_z x d_x)| / (|d_y| |d_z| |d_x|) of a Z_THEN_X atom with a y atom, image=largest |fractional component| of a frame vector (with a
    cell: the distance of the minimum-image rounding from a flip is 0.5 minus this)).  float64 torch on the CPU."""
    from tests import local_frames_reference as LR

    pos, atoms, kinds = pos.to(F64), atoms.long(), kinds.long()
    cells = None if cell is None else cell.to(F64).reshape(-1, 3, 3)
    out = dict(bond=[np.inf, 0.0], angle=[180.0, 0.0], z_only=np.inf, chiral=np.inf, image=0.0)
    idx = torch.arange(pos.shape[0])
    vec = {}
    for slot in range(3):
        rows = idx[atoms[:, slot] >= 0]
        if rows.numel() == 0:
            continue
        d = LR.frame_vectors(pos, atoms, rows, slot, cells, batch_idx)
        vec[slot] = (rows, d)
        length = d.norm(dim=1)
        out["bond"] = [min(out["bond"][0], float(length.min())), max(out["bond"][1], float(length.max()))]
        if cells is not None:
            c = cells[batch_idx.long()[rows]] if batch_idx is not None else cells[:1].expand(rows.shape[0], 3, 3)
            out["image"] = max(out["image"], float(torch.einsum("na,nab->nb", d, torch.linalg.inv(c)).abs().max()))
    full = {s: torch.full((pos.shape[0], 3), float("nan"), dtype=F64).index_copy(0, r, d) for s, (r, d) in vec.items()}
    for a, b in ((0, 1), (0, 2), (1, 2)):
        if a in full and b in full:
            cos = (full[a] * full[b]).sum(1) / (full[a].norm(dim=1) * full[b].norm(dim=1))
            ang = torch.rad2deg(torch.acos(cos[~torch.isnan(cos)].clamp(-1.0, 1.0)))
            if ang.numel():
                out["angle"] = [min(out["angle"][0], float(ang.min())), max(out["angle"][1], float(ang.max()))]
    z_only = kinds == LR.Z_ONLY
    if bool(z_only.any()):
        ez = full[0][z_only]
        out["z_only"] = float(((ez[:, 0] / ez.norm(dim=1)).abs() - LR.Z_ONLY_SWITCH).abs().min())
    chiral = (kinds == LR.Z_THEN_X) & (atoms[:, 2] >= 0)
    if bool(chiral.any()):
        dz, dx, dy = (full[s][chiral] for s in range(3))
        out["chiral"] = float(((dy * torch.linalg.cross(dz, dx)).sum(1).abs() / (dy.norm(dim=1) * dz.norm(dim=1) * dx.norm(dim=1))).min())
    return out


def _frame_box(box):
    return torch.tensor([[box, 0.0, 0.0], [0.25 * box, 0.9 * box, 0.0], [0.1 * box, -0.2 * box, 1.1 * box]], dtype=F64).float().double()


@functools.lru_cache(maxsize=None)
def frames(batch=False):
    """A topology over the 130 / 70 + 60 atoms of the layout sweeps that uses every kind: the eight molecules of
    tests/local_frames_reference.py (25 atoms: every kind, Z_ONLY on both sides of its switch, Z_THEN_X with and without a y atom, both
    chiralities) and randomly rotated waters, wrapped into the triclinic boxes of `system` (12 / 12 and 11; molecules straddle faces);
    the batch's second system is a z-bisect centre, an ammonia and 17 waters.  Local multipoles and the caller gradients `w_mu`, `w_q` are
    drawn once.  Every value is a float32 number; tests/test_layout_sensitivity_cpu.py asserts the geometry conditions on these numbers."""
    from tests import local_frames_reference as LR

    mols = [LR.molecule(m) for m in FR_MOLECULES]
    if batch:
        parts = [LR.join(mols + [LR.waters(NA - 25, seed=32)[:3]])[:3], LR.join([LR.molecule("z_bisect"), LR.molecule("ammonia"), LR.waters(NB - 9, seed=33)[:3]])[:3]]
        cells = torch.stack([_frame_box(12.0), _frame_box(11.0)])
    else:
        parts = [LR.join(mols + [LR.waters(N - 25, seed=31)[:3]])[:3]]
        cells = _frame_box(12.0)[None]
    wrapped = []
    for (p, a, k), cell in zip(parts, cells):
        p = p + torch.tensor([5.7, 0.3, 6.1], dtype=F64)  # the molecules at the origin land on a face of the box
        frac = p @ torch.linalg.inv(cell)
        wrapped.append(((frac - torch.floor(frac)) @ cell, a, k))
    pos, atoms, kinds, sys_of = LR.join(wrapped)
    n = pos.shape[0]
    assert n == (NA + NB if batch else N) and sorted(set(kinds.tolist())) == list(range(6))
    mu, quad = LR.local_multipoles(n, 41 + batch)
    gen = torch.Generator().manual_seed(43 + batch)
    f32 = lambda t: t.float().double().numpy()  # noqa: E731
    return dict(n=n, pos=f32(pos), atoms=atoms.numpy(), kinds=kinds.numpy(), cell=f32(cells), batch_idx=sys_of.to(torch.int32).numpy() if batch else None,
                mu=f32(mu), quad=f32(quad), w_mu=f32(torch.randn((n, 3), dtype=F64, generator=gen)), w_q=f32(torch.randn((n, 3, 3), dtype=F64, generator=gen)))


def frames_reference(batch=False, **replace):
    """dict of float64 numpy arrays (`FR_NAMES`) of the restatement tests/local_frames_reference.py on the fixture, arguments replaced."""
    from tests import local_frames_reference as LR

    c = {**frames(batch), **replace}
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))  # noqa: E731
    bi = None if c["batch_idx"] is None else torch.as_tensor(c["batch_idx"])
    out = LR.evaluate(t(c["pos"]), t(c["mu"]), t(c["quad"]), torch.as_tensor(c["atoms"]), torch.as_tensor(c["kinds"]), t(c["w_mu"]), t(c["w_q"]),
                      cell=t(c["cell"]), batch_idx=bi)
    return {k: out[k].detach().numpy() for k in FR_NAMES}


# ---- cluster_induced_dipoles ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def cluster_induced():
    """The batch of three clusters (70, 2 and 1 atoms) of tests/cluster_multipole_reference.py rounded to float32 numbers, with an external
    field and a warm start; `polar` for the undamped solve, four times those (`polar_thole`) with `thole=0.39`, as in
    tests/test_cluster_multipole_gpu.py."""
    from tests import cluster_multipole_reference as CR

    p = dict(CR.problem("batch"))
    for k in ("pos", "q", "polar", "field"):
        p[k] = _f32(p[k])
    p["polar_thole"] = _f32(4.0 * p["polar"])
    p["start"] = _f32(0.05 * np.random.default_rng(53).normal(size=(p["n"], 3)))
    return p


def cluster_induced_dense(thole=None, device="cpu"):
    """dict(H, b, polar, bi) of the dense float64 restatement of `cluster_induced()`."""
    from tests import cluster_multipole_reference as CR

    p = cluster_induced()
    H, b, _, polar = CR.dense_problem(dict(p, polar=p["polar"] if thole is None else p["polar_thole"]), thole, device)
    return dict(H=H, b=b, polar=polar, bi=torch.as_tensor(p["batch_idx"], device=device))
