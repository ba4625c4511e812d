"""Seeded sweep cases, boundary ladders and one-scalar variants of the five newer dispersion operators (`dftd3_atm`, `dftd3_zero`,
`dftd3_zero_atm`, `dftd4`, `dftd4_atm`) and the inputs of the sweeps of `gaussian_charge_correction`, charge equilibration, the two
point-dipole operators, `ewald_quadrupole_correction`, `thole_dipole_correction`, `induced_dipoles`, `pme_quadrupole_correction` and the cluster, pair-scale and
local-frame operators (last five sections),
built on the float64 restatements tests/atm_reference.py, tests/d3_zero_reference.py,
tests/d4_reference.py and tests/d4_atm_reference.py.  Importable without a GPU and without the native library (the two tile sizes are read
lazily, by the ladder builders only).  The CPU suite asserts every condition a case must meet (tests/test_sweep_cases_cpu.py); the GPU
modules tests/test_sweep_dispersion_gpu.py and tests/test_sweep_charges_gpu.py compare the kernels with the references made here.  Every reference is computed once
(`functools.lru_cache`) and never modified.

    case(op, seed)            seeded random case; everything is drawn from np.random.default_rng(BASE[op] + seed)
    ladder_case(op, name)     one rung of a boundary ladder: "n64" ... (lane trips), "m255" ... (block trips and LDS tiles)
    variant_case(op, name)    a fixed case with ONE model scalar moved off its default ("default": none moved)
    references(kind, op, key) (float64 restatement, the same with float32 per-pair / per-atom / per-triple arithmetic), at the case's s9

A case is a dict: pos, z, cell ([B,3,3] or None), batch_idx (None for one system), tables, r0ab (zero damping), q (`dftd4`), rc (list
cutoff), rc3 (three-body ops), model (the scalars, in the restatements' names), margins (cutoff name -> smallest |distance - cutoff| of any
pair of atom images), counts / widest (entries per row of the full list, from the float64 enumeration), lists (how the GPU module stores
the list: int64, pad, foreign fill, permuted rows), and for three-body ops s9.

CUTOFFS.  The restatements enumerate pairs in float64, the kernels in float32 (rounding at these distances: 2e-6 Bohr); a pair within
rounding of a cutoff is counted by one and not by the other, which is no kernel error.  Each cutoff is therefore placed at the midpoint of
the widest gap between image-pair distances inside a window of +-0.4 Bohr around its drawn target (`place_cutoff`); the CPU suite asserts a
margin of 1e-3 Bohr for every case.

S9.  Not drawn: `d4_atm_cases.lifted`'s rule applied to the case's own float64 reference -- the smallest power of ten at which energy,
forces and (periodic) virial reach 500 x the bar the GPU comparison applies -- so a three-body case is never compared against nothing.

GEOMETRY of a sweep case: one to three systems with sizes from {1, 2, 3, 7, 20, 45} (at most 70 atoms, at least one system of 7 or more),
jittered lattices (`atm_reference.lattice_box`, spacing 3.6 - 4.6 Bohr, jitter 0.25; the first n sites of the smallest box that holds
them) or `systems.molecule(min_dist=2.0)`: the distances of a condensed phase, for the reason the restatements' docstrings give.  Periodic
in two seeds of three; in a third of those one system sits in a cell shorter than the list cutoff (rows hold the atom's own images), the
other cells are at least half a Bohr higher than it.  Systems of one or two atoms of a periodic batch sit in a cube no image reaches
across.  Positions are float64 in every fourth seed.  Species counts are scheduled over {1, 3, 6, 7, 16, 17, 20} (the thresholds of
`D3_ATM_LDS_S`, `D4_SLOTS` and the 16-species D3 paths) with tables up to Z = 24; one seed in four puts a Z = 0 atom, one a Z > max_Z atom
and one an element without references (`n_ref = 0`; for the D3 family an all-zero c6 block) into the middle of the largest system.

RADII of `dftd3_zero_atm` seeds.  With the table of tests/test_d3_zero_gpu.py (radii from 3.5 Bohr) and rs9 down to 0.8 the nearest-neighbour
triples are undamped (R0 = 2.8 Bohr below a contact of 3.5): triple terms of both signs, orders of magnitude above the sums they cancel
to, whose float32 rounding -- not the kernel's evaluation order -- then decides the virial.  The restatement's own float32 deviation
reached 2.9 of `dftd3`'s bar (seed 4; 1.3 on seed 10) with radii from 3.5 Bohr, 2.4 from 5, 1.0 from 5.5, 0.66 from 6 and 0.39 from
6.5.  The sweep therefore draws that op's radii from [6.5, 9] Bohr (`ZERO_ATM_RADII_LO`), where the damping acts at contact distance;
the CPU suite asserts the deviation below the bar for every seed.
"""
import functools

import numpy as np
import torch

from tests import atm_reference as A
from tests import d3_zero_reference as Z
from tests import d4_atm_cases as K3
from tests import d4_atm_reference as R3
from tests import d4_cases as K
from tests import d4_reference as R
from tests import pme_dipole_reference as PR
from tests import systems as S

OPS = ("dftd3_atm", "dftd3_zero", "dftd3_zero_atm", "dftd4", "dftd4_atm")
THREE_BODY = ("dftd3_atm", "dftd3_zero_atm", "dftd4_atm")
D4_OPS = ("dftd4", "dftd4_atm")
BASE = {"dftd3_atm": 7100, "dftd3_zero": 7200, "dftd3_zero_atm": 7300, "dftd4": 7400, "dftd4_atm": 7500}
SEEDS = tuple(range(12))
SIZES = (1, 2, 3, 7, 20, 45)
SPECIES_COUNTS = (1, 3, 6, 7, 16, 17, 20)
SPECIES_BY_SEED = (3, 6, 7, 16, 17, 20, 1, 7, 17, 6, 16, 3)  # every listed count at least once; the three-body thresholds twice
Z_MAX = 24
MARGIN = 1e-3
WINDOW = 0.4
ALPHAS = (13.5, 14.0, 15.2, 16.0)
ZERO_ATM_RADII_LO = 6.5  # Bohr; see RADII in the module docstring
DEFAULTS = {
    "dftd3_atm": dict(a1=0.4, a2=4.0, alpha=16.0, k1=16.0, k3=-4.0),
    "dftd3_zero": dict(rs6=1.217, s8=0.722, rs8=1.0, alpha=14.0, beta=0.0, k1=16.0, k3=-4.0, s6=1.0, s5_on=1e10, s5_off=1e10),
    "dftd3_zero_atm": dict(rs9=4.0 / 3.0, alpha=16.0, k1=16.0, k3=-4.0),
    "dftd4": dict(a1=0.4, a2=4.0, s8=0.8, s6=1.0, wf=6.0, ga=3.0, gc=2.0, k_cn=7.5, cn_cutoff=None),
    "dftd4_atm": dict(a1=0.4, a2=4.0, alpha=16.0, wf=6.0, ga=3.0, gc=2.0, k_cn=7.5, cn_cutoff=None),
}
# the scalars a sweep seed draws, per op (the coverage test wants at least three distinct values of each over the twelve seeds)
DRAWN = {
    "dftd3_atm": ("a1", "a2", "alpha", "k1", "k3"),
    "dftd3_zero": ("rs6", "s8", "rs8", "alpha", "beta", "k1", "k3", "s6"),
    "dftd3_zero_atm": ("rs9", "alpha", "k1", "k3"),
    "dftd4": ("a1", "a2", "s6", "s8", "wf", "ga", "gc", "k_cn"),
    "dftd4_atm": ("a1", "a2", "alpha", "wf", "ga", "gc", "k_cn"),
}
TWO_VALUED = ("beta",)  # drawn from {0, 0.05}: two values, both required
VARIANTS = {
    "dftd4": (("s6", 0.8), ("s8", 0.0), ("a1", 0.52), ("a2", 5.0), ("wf", 4.5), ("ga", 2.4), ("gc", 1.6), ("k_cn", 6.5)),
    "dftd4_atm": (("alpha", 14.0), ("alpha", 13.5), ("a1", 0.52), ("a2", 5.0), ("wf", 4.5), ("ga", 2.4), ("gc", 1.6), ("k_cn", 6.5)),
    "dftd3_atm": (("k1", 15.0), ("k3", -3.5), ("a1", 0.52), ("a2", 5.0)),
    "dftd3_zero_atm": (("k1", 15.0), ("k3", -3.5), ("rs9", 1.0)),
}
SEPARATION = 102.0  # a variant's float64 reference leaves the default's by this many bars: > 100 between the two kernel results, each within one
LANE_RUNGS = ("n64", "n65", "n66", "n129")
LANE_OPS = ("dftd4", "dftd3_zero")
TILES = {"dftd4_atm": 288, "dftd3_atm": 320, "dftd3_zero_atm": 320}  # `D4_ATM_TILE` / `D3_ATM_TILE`; the CPU suite reads the #defines


def tile_of(op):
    """The LDS tile of the op's triple pass, from the library."""
    if op == "dftd4_atm":
        from nvalchemiops.interactions.dispersion.dftd4 import atm_tile
    else:
        from nvalchemiops.interactions.dispersion.dftd3 import atm_tile
    return atm_tile()


def tile_rungs(op, tile=None):
    """Shell sizes of the block-trip / tile ladder: 255, 256, 257 (one stream trip short by one, exactly one, one plus one entry), then one
    full tile, one tile plus one record and -- but for the zero-damping form, which runs the same triple pass -- exactly two tiles."""
    tile = TILES[op] if tile is None else tile
    return (255, 256, 257, tile, tile + 1, 2 * tile) if op != "dftd3_zero_atm" else (tile, tile + 1)


# ---- cutoffs ------------------------------------------------------------------------------------------------------------------------------

def image_distances(pos, cell, batch_idx, reach):
    """Distances below `reach` of every pair of atom images (first atom in the home cell), all systems together; float64."""
    pos = np.asarray(pos, np.float64)
    bi = np.zeros(len(pos), np.int64) if batch_idx is None else np.asarray(batch_idx, np.int64)
    out = []
    for s in range(int(bi.max()) + 1 if len(pos) else 0):
        sel = np.nonzero(bi == s)[0]
        cs = None if cell is None else np.asarray(cell, np.float64).reshape(-1, 3, 3)[s]
        i, j, sh = A.enumerate_pairs(pos[sel], cs, reach)
        out.append(np.linalg.norm(A._np_vectors(pos[sel], cs, i, j, sh), axis=1))
    return np.concatenate(out) if out else np.zeros(0)


def place_cutoff(dist, target, window=WINDOW):
    """The midpoint of the widest gap between the distances inside target +- window (the window's ends count as distances)."""
    lo, hi = target - window, target + window
    pts = np.concatenate([[lo], np.sort(dist[(dist > lo) & (dist < hi)]), [hi]])
    k = int(np.argmax(np.diff(pts)))
    return float(0.5 * (pts[k] + pts[k + 1]))


def margin_of(dist, cutoff):
    return float(np.abs(dist - cutoff).min()) if dist.size else float("inf")


def row_counts(pos, cell, batch_idx, rc):
    """Entries per row of the full list with cutoff rc (padding atoms have rows too: a neighbour search does not know the species)."""
    pos = np.asarray(pos, np.float64)
    bi = np.zeros(len(pos), np.int64) if batch_idx is None else np.asarray(batch_idx, np.int64)
    counts = np.zeros(len(pos), np.int64)
    for s in range(int(bi.max()) + 1):
        sel = np.nonzero(bi == s)[0]
        cs = None if cell is None else np.asarray(cell, np.float64).reshape(-1, 3, 3)[s]
        i, _, _ = A.enumerate_pairs(pos[sel], cs, rc)
        counts[sel] = np.bincount(i, minlength=len(sel))
    return counts


# ---- geometry of a sweep case ------------------------------------------------------------------------------------------------------------------

_ORDINARY = {3: (3, 3, 3), 7: (3, 3, 3), 20: (3, 3, 3), 45: (3, 4, 4)}  # the first n sites are used
_SHORT = {3: (3, 1, 1), 7: (4, 2, 1), 20: (5, 4, 1), 45: (9, 5, 1)}  # one lattice plane thick: a height of one spacing (<= 5.1 Bohr)


def heights(cell):
    return 1.0 / np.linalg.norm(np.linalg.inv(np.asarray(cell, np.float64).reshape(3, 3)), axis=0)


def _sizes(g, need, single):
    for _ in range(10_000):
        sizes = [int(g.choice(SIZES)) for _ in range(1 if single else int(g.integers(1, 4)))]
        if need <= sum(sizes) <= 70 and max(sizes) >= 7:
            return sizes
    raise AssertionError("no batch of sizes found")


def _systems(g, seed, sizes, dtype, rc_target):
    """(pos, cell or None, batch_idx or None, list-cutoff target, index of the short system or None)."""
    periodic = seed % 3 != 2
    short = seed in (1, 4, 7)  # three of the eight periodic seeds
    short_sys = int(np.argmax(sizes)) if short else None
    parts, cells = [], []
    for k, n in enumerate(sizes):
        sub = int(g.integers(1 << 30))
        if not periodic:
            parts.append(S.molecule(n, density=float(g.uniform(0.02, 0.03)), min_dist=2.0, seed=sub, dtype=dtype)[0])
            continue
        if n <= 2:  # no image within reach: a single atom is exactly zero, a pair has its one distance
            p = np.array([[1.0, 2.0, 3.0], [1.0 + float(g.uniform(3.0, 5.0)), 2.5, 3.5]])[:n]
            parts.append(p.astype(dtype))
            cells.append((np.eye(3) * 2.5 * (rc_target + WINDOW)).astype(dtype))
            continue
        shape = (_SHORT if k == short_sys else _ORDINARY)[n]
        p, c = A.lattice_box(shape, a=float(g.uniform(3.6, 4.6)), jitter=0.25, seed=sub, triclinic=bool(g.integers(2)), dtype=dtype)
        parts.append(p[:n])
        cells.append(c)
    if periodic:  # ordinary cells stay at least half a Bohr above the list cutoff (window included)
        for k, c in enumerate(cells):
            if k != short_sys and sizes[k] > 2:
                rc_target = min(rc_target, float(heights(c).min()) - 0.5 - WINDOW)
    pos = np.concatenate(parts)
    bi = None if len(sizes) == 1 else np.concatenate([np.full(n, k, np.int32) for k, n in enumerate(sizes)])
    return pos, (np.stack(cells) if periodic else None), bi, rc_target, short_sys


def _d3_tables(g, seed, dead):
    t = {k: v.copy() for k, v in S.d3_test_tables(Z_MAX, seed=int(g.integers(1 << 30))).items()}
    if seed % 5 == 1:  # reference CN that depends on the partner: the 25-term form (no factorised weights)
        t["cn_ref"] *= (1.0 + 0.01 * np.arange(Z_MAX + 1, dtype=np.float32)[None, :, None, None])
    if dead is not None:  # an element whose c6 block is zero: it is counted by its neighbours and is part of no pair energy
        t["c6ab"][dead] = 0.0
        t["c6ab"][:, dead] = 0.0
    return t


def _d4_tables(g, dead):
    t = R.d4_test_tables(Z_MAX, seed=int(g.integers(1 << 30)))
    if dead is not None:
        t["n_ref"][dead] = 0
        R.blank_unused(t)
    return t


def _species(g, op, seed, sizes):
    """(z [N], kind of padding atom or None, its index or None, the element without references or None)."""
    n = sum(sizes)
    kind = (None, "z0", "beyond", "dead")[seed % 4]
    count = SPECIES_BY_SEED[seed]
    pool = g.permutation(np.arange(1, Z_MAX + 1))
    dead = int(pool[-1]) if kind == "dead" else None
    # a dead element is a species of its own for the D3 kernels (it takes part in the coordination numbers), padding for the D4 ones
    regular = count - 1 if (dead is not None and op not in D4_OPS and count > 1) else count
    sp = np.sort(pool[:regular])
    start = int(np.sum(sizes[:int(np.argmax(sizes))]))
    at = start + max(sizes) // 2 if kind is not None else None
    z = np.zeros(n, np.int32)
    others = np.array([i for i in range(n) if i != at])
    z[others] = sp[g.permutation(len(others)) % regular]
    if kind == "z0":
        z[at] = 0
    elif kind == "beyond":
        z[at] = Z_MAX + 1 + int(g.integers(0, 3))
    elif kind == "dead":
        z[at] = dead
    return z, kind, at, dead


def _model(g, op, seed, rc):
    a = int(g.integers(4))
    draw = dict(a1=g.uniform(0.3, 0.6), a2=g.uniform(3.0, 5.5), s6=g.uniform(0.7, 1.0), s8=0.0 if seed == 5 else g.uniform(0.0, 2.5),
                wf=g.uniform(4.0, 8.0), ga=g.uniform(2.0, 4.0), gc=g.uniform(1.5, 2.5), k_cn=g.uniform(6.0, 9.0), k1=g.uniform(14.0, 17.0),
                k3=g.uniform(-5.0, -3.0), alpha=ALPHAS[seed] if seed < 4 else ALPHAS[a], rs6=g.uniform(0.8, 1.3),
                rs8=g.uniform(0.8, 1.3), rs9=g.uniform(0.8, 1.3), beta=(0.0, 0.05)[seed % 2])
    m = dict(DEFAULTS[op])
    m.update({k: float(draw[k]) for k in DRAWN[op]})
    if op == "dftd3_zero" and seed % 4 == 1:
        m.update(s5_on=0.6 * rc, s5_off=0.95 * rc)
    return m


@functools.lru_cache(maxsize=None)
def _sweep(op, seed):
    g = np.random.default_rng(BASE[op] + seed)
    dtype = np.float64 if seed % 4 == 3 else np.float32
    sizes = _sizes(g, SPECIES_BY_SEED[seed] + 1, single=seed % 6 == 5)  # (one system: the unbatched search and call)
    rc_target = float(g.uniform(7.5, 9.0))
    pos, cell, bi, rc_target, short_sys = _systems(g, seed, sizes, dtype, rc_target)
    z, kind, at, dead = _species(g, op, seed, sizes)
    c = dict(op=op, pos=pos, z=z, cell=cell, batch_idx=bi, sizes=tuple(sizes), padding=kind, padding_atom=at, short_system=short_sys)
    if op in D4_OPS:
        c["tables"] = _d4_tables(g, dead)
        c["q"] = g.uniform(-0.3, 0.3, len(pos)).astype(np.float32)
    else:
        c["tables"] = _d3_tables(g, seed, dead)
        # three-body: radii from 6.5 Bohr (see RADII in the module docstring); two-body: the range of tests/test_d3_zero_gpu.py
        c["r0ab"] = Z.synthetic_r0ab(Z_MAX + 1, seed=int(g.integers(1 << 30)), lo=ZERO_ATM_RADII_LO if op == "dftd3_zero_atm" else 3.5)
    dist = image_distances(pos, cell, bi, rc_target + WINDOW + 0.1)
    c["rc"] = place_cutoff(dist, rc_target)
    c["margins"] = {"list": margin_of(dist, c["rc"])}
    if op in THREE_BODY:
        c["rc3"] = place_cutoff(dist, float(g.uniform(5.6, min(7.0, rc_target - 1.0))))
        c["margins"]["three_body"] = margin_of(dist, c["rc3"])
    c["model"] = _model(g, op, seed, c["rc"])
    if op in D4_OPS and seed % 3 == 1:
        c["model"]["cn_cutoff"] = place_cutoff(dist, float(g.uniform(4.8, 5.6)))
        c["margins"]["cn"] = margin_of(dist, c["model"]["cn_cutoff"])
    c["counts"] = row_counts(pos, cell, bi, c["rc"])
    c["widest"] = int(c["counts"].max())
    c["lists"] = dict(int64=seed % 4 == 2, pad=int(2 * g.integers(0, 5) + 1), foreign_fill=seed % 3 == 0, permuted=seed % 2 == 1)
    return c


# ---- ladders ------------------------------------------------------------------------------------------------------------------------------------

def _fixed_tables(op):
    c = {}
    if op in D4_OPS:
        c["tables"] = R.d4_test_tables(17)
    else:
        c["tables"] = S.d3_test_tables(17)
        c["r0ab"] = Z.synthetic_r0ab(18)
    return c


@functools.lru_cache(maxsize=None)
def _ladder(op, name):
    plain = dict(int64=False, pad=0, foreign_fill=False, permuted=False)
    if name.startswith("n"):  # lane trips: a free cluster, every row holds the n - 1 others; the matrix is exactly that wide
        n = int(name[1:])
        pos = S.molecule(n, density=0.03, min_dist=2.0, seed=400 + n)[0]
        z = np.random.default_rng(400 + n).choice(np.array((1, 6, 8, 17), np.int32), n)
        dist = image_distances(pos, None, None, 1e9)
        rc = 2.0 * float(dist.max())
        c = dict(op=op, pos=pos, z=z, cell=None, batch_idx=None, rc=rc, margins={"list": margin_of(dist, rc)}, model=dict(DEFAULTS[op]), widest=n - 1, counts=np.full(n, n - 1),
                 lists=plain, **_fixed_tables(op))
        if op == "dftd4":
            c["q"] = np.random.default_rng(477 + n).uniform(-0.3, 0.3, n).astype(np.float32)
        return c
    m = int(name[1:])  # block trips and LDS tiles: one row of m kept entries, every other row below one tile
    # The cutoff sits in a window from half a Bohr above the shell radius (every centre-shell distance is below radius + 0.35) to two
    # Bohr above it, far below the diameter.  Shell-shell distances near the radius R come m^2 / (4 R) to the Bohr: at R = 19 the widest gap
    # of the two-tile shells (576, 640) leaves a margin of 0.7e-3 - 1.5e-3 over eight jitter seeds, so those two sit at R = 40.
    radius = 19.0 if m < 500 else 40.0
    pos = A.centre_and_shell(m, radius=radius)
    z = np.random.default_rng(29).choice(np.array((1, 6, 8), np.int32), len(pos))
    z[0] = 17  # the heaviest element of the tables at the centre: the triples of the long row weigh in the totals (C9 grows with Z)
    dist = image_distances(pos, None, None, 1e9)
    rc3 = place_cutoff(dist, radius + 1.25, 0.75)
    rc = 2.0 * float(dist.max())
    return dict(op=op, pos=pos, z=z, cell=None, batch_idx=None, rc=rc, rc3=rc3, margins={"list": margin_of(dist, rc), "three_body": margin_of(dist, rc3)},
                model=dict(DEFAULTS[op]), widest=m, counts=np.full(m + 1, m), lists=plain, **_fixed_tables(op))


# ---- variants -----------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _variant_base(op):
    """`triclinic_f32` of tests/d4_cases.py for the D4 ops, the triclinic periodic box of tests/test_d3_atm_gpu.py for the D3 ones; the
    cutoffs are the gap-rule values next to the ones those tests use (9 / 7 and 10 / 8.5)."""
    if op in D4_OPS:
        b = K.case("triclinic_f32")
        c = dict(pos=b["pos"], z=b["z"], q=b["q"], tables=b["tables"], cell=np.asarray(b["cell"]).reshape(1, 3, 3))
        rc_t, rc3_t = 9.0, 7.0
    else:
        pos, cell = A.lattice_box((5, 5, 6), seed=7, triclinic=True)
        z = np.random.default_rng(7).choice(np.array((1, 6, 8, 17), np.int32), len(pos))
        c = dict(pos=pos, z=z, cell=cell.reshape(1, 3, 3), **_fixed_tables(op))
        rc_t, rc3_t = 10.0, 8.5
    dist = image_distances(c["pos"], c["cell"], None, rc_t + WINDOW + 0.1)
    c.update(op=op, batch_idx=None, rc=place_cutoff(dist, rc_t), lists=dict(int64=False, pad=8, foreign_fill=False, permuted=False))
    c["margins"] = {"list": margin_of(dist, c["rc"])}
    if op in THREE_BODY:
        c["rc3"] = place_cutoff(dist, rc3_t)
        c["margins"]["three_body"] = margin_of(dist, c["rc3"])
    c["counts"] = row_counts(c["pos"], c["cell"], None, c["rc"])
    c["widest"] = int(c["counts"].max())
    return c


def variant_names(op):
    return tuple(f"{k}={v:g}" for k, v in VARIANTS[op])


@functools.lru_cache(maxsize=None)
def _variant(op, name):
    c = dict(_variant_base(op))
    c["model"] = dict(DEFAULTS[op])
    if name != "default":
        k, v = name.split("=")
        assert k in c["model"], name
        c["model"][k] = float(v)
    return c


# ---- references ---------------------------------------------------------------------------------------------------------------------------------

def _geometry(kind, op, key):
    return {"sweep": _sweep, "ladder": _ladder, "variant": _variant}[kind](op, key)


def _zero_two_body(c, m, work_dtype):
    """`d3_zero_reference.reference`, system by system: a system of one atom has no pair (the restatement's C6 interpolation wants at
    least one), and is zero throughout."""
    n = len(c["pos"])
    bi = np.zeros(n, np.int64) if c["batch_idx"] is None else np.asarray(c["batch_idx"], np.int64)
    nsys = int(bi.max()) + 1
    out = dict(energy=np.zeros(nsys), forces=np.zeros((n, 3)), cn=np.zeros(n), virial=None if c["cell"] is None else np.zeros((nsys, 3, 3)),
               triples=0)
    for s in range(nsys):
        sel = np.nonzero(bi == s)[0]
        if len(sel) < 2:
            continue
        r = Z.reference(c["pos"][sel], c["z"][sel], c["tables"], c["r0ab"], m["rs6"], m["s8"], c["rc"], rs8=m["rs8"], alpha=m["alpha"], beta=m["beta"],
                        k1=m["k1"], k3=m["k3"], s6=m["s6"], s5_on=m["s5_on"], s5_off=m["s5_off"], cell=None if c["cell"] is None else c["cell"][s],
                        work_dtype=work_dtype)
        out["energy"][s], out["forces"][sel], out["cn"][sel] = r["energy"][0], r["forces"], r["cn"]
        if out["virial"] is not None:
            out["virial"][s] = r["virial"][0]
    return out


def evaluate(c, work_dtype=torch.float64, s9=1.0, **override):
    """The op's restatement on case c (model scalars overridden by `override`)."""
    op, m = c["op"], dict(c["model"], **override)
    common = dict(cell=c["cell"], batch_idx=c["batch_idx"], work_dtype=work_dtype)
    pos, z, t = c["pos"], c["z"], c["tables"]
    if op == "dftd3_atm":
        return A.reference(pos, z, t, m["a1"], m["a2"], c["rc"], three_body_cutoff=c["rc3"], s9=s9, alpha=m["alpha"], k1=m["k1"], k3=m["k3"],
                           term="atm", **common)
    if op == "dftd3_zero":
        return _zero_two_body(c, m, work_dtype)
    if op == "dftd3_zero_atm":
        return Z.reference(pos, z, t, c["r0ab"], None, None, c["rc"], three_body_cutoff=c["rc3"], rs9=m["rs9"], s9=s9, alpha=m["alpha"], k1=m["k1"],
                           k3=m["k3"], term="atm", **common)
    if op == "dftd4":
        return R.reference(pos, z, c["q"], t, m["a1"], m["a2"], m["s8"], c["rc"], s6=m["s6"], cn_cutoff=m["cn_cutoff"], wf=m["wf"], ga=m["ga"],
                           gc=m["gc"], k_cn=m["k_cn"], **common)
    if op == "dftd4_atm":
        return R3.reference(pos, z, t, m["a1"], m["a2"], c["rc"], three_body_cutoff=c["rc3"], s9=s9, alpha=m["alpha"], cn_cutoff=m["cn_cutoff"],
                            wf=m["wf"], ga=m["ga"], gc=m["gc"], k_cn=m["k_cn"], **common)
    raise ValueError(op)


@functools.lru_cache(maxsize=None)
def unit_references(kind, op, key):
    """(float64, float32-arithmetic) restatement at s9 = 1."""
    c = _geometry(kind, op, key)
    return evaluate(c), evaluate(c, work_dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def s9_of(kind, op, key):
    """1 for the two-body ops.  Three-body: the smallest power of ten that lifts the case (`d4_atm_cases.lifted`); a variant takes the s9 of
    its default, so that the two calls differ in the one scalar only."""
    if op not in THREE_BODY:
        return 1.0
    if kind == "variant" and key != "default":
        return s9_of(kind, op, "default")
    r64, _ = unit_references(kind, op, key)
    s9 = 1.0
    while not K3.lifted(r64, s9):
        s9 *= 10.0
        assert s9 <= 1e12, (kind, op, key)
    return s9


@functools.lru_cache(maxsize=None)
def references(kind, op, key):
    r64, r32 = unit_references(kind, op, key)
    s9 = s9_of(kind, op, key)
    return K3._scaled(r64, s9), K3._scaled(r32, s9)


@functools.lru_cache(maxsize=None)
def _case(kind, op, key):
    c = dict(_geometry(kind, op, key))
    if op in THREE_BODY:
        c["s9"] = s9_of(kind, op, key)
    return c


def case(op, seed):
    return _charge_sweep(op, seed) if op in CHARGE_OPS else _case("sweep", op, seed)


def ladder_case(op, name):
    return _charge_ladder(name) if op in CHARGE_OPS else _case("ladder", op, name)


def variant_case(op, name):
    return _case("variant", op, name)


# ---- bars ----------------------------------------------------------------------------------------------------------------------------------------

EXTRA = {"energy": 0.0, "forces": 5e-6, "cn": 0.0, "charge_grad": 5e-6, "virial": 2e-7}  # as the ops' GPU modules have them
OUTPUTS = {"dftd3_atm": ("energy", "forces", "virial"), "dftd3_zero": ("energy", "forces", "cn", "virial"),
           "dftd3_zero_atm": ("energy", "forces", "virial"), "dftd4": ("energy", "forces", "cn", "charge_grad", "virial"),
           "dftd4_atm": ("energy", "forces", "virial")}


def d3_bar(ref, key):
    """`dftd3`'s elementwise bar for a quantity with reference values `ref`."""
    return 1e-6 + 1e-6 * np.abs(ref) + EXTRA[key] * (np.abs(ref).max() if ref.size else 0.0)


def bar(r64, r32, key):
    """The elementwise bar of the ops' GPU modules (`_judge` / `_bars`): 4 x the larger of the restatement's float32 deviation on this case
    and `dftd3`'s bar."""
    dev32 = np.abs(r32[key] - r64[key]).max() if r64[key].size else 0.0
    return 4.0 * np.maximum(dev32, d3_bar(r64[key], key))


def separation(op, name):
    """By how many bars the variant's float64 reference leaves the default's, per output, largest first."""
    r64, r32 = references("variant", op, name)
    d64, _ = references("variant", op, "default")
    out = {k: float((np.abs(r64[k] - d64[k]) / bar(r64, r32, k)).max()) for k in OUTPUTS[op] if r64[k] is not None}
    return dict(sorted(out.items(), key=lambda kv: -kv[1]))


# ---- Gaussian charges and charge equilibration ----------------------------------------------------------------------------------------------------
# Inputs only: the references of these two ops are evaluated by the GPU modules on the entries actually stored (tests/gaussian_reference.py,
# tests/qeq_reference.py), as tests/test_gaussian_charges_gpu.py and tests/test_qeq_gpu.py do, so no cutoff needs a margin here.  The recipe
# is `_system` / `_abi_case` of those modules: uniform positions in a (triclinic or cubic) cell, sigma in [0.3, 0.8] with some exact zeros,
# brute-force entries, a matrix widest row + an odd pad wide whose padding columns hold the mask value, -1 and n + 7, one emptied row.

CHARGE_OPS = ("gaussian_charge_correction", "charge_equilibration")
BASE.update(gaussian_charge_correction=7600, charge_equilibration=7700)
CHARGE_SIZES = (1, 9, 60, 150)
_BOX = {60: 9.0, 150: 12.0}  # 1 and 9 atoms: box 5 (shorter than the cutoff: own images) or 14 (a single atom then has no entry at all)
UNROLLED_WIDTHS = (255, 256, 257, 335)
COMPUTE_FLAGS = ("compute_forces", "compute_charge_gradients", "compute_sigma_gradients", "compute_virial")


def charge_cell(box, triclinic=True):
    return np.array([[box, 0, 0], [0.2 * box, 0.9 * box, 0], [0.1 * box, -0.15 * box, 1.1 * box]]) if triclinic else np.eye(3) * box


def brute_force(pos, cell, cutoff, images):
    """Every (i, j, S) with 1e-12 < |r_j - r_i + S . cell| < cutoff, S in [-images, images]^3, sorted by row: a full list (numpy; the
    recipe of `gaussian_reference.brute_force_entries`).  `cell` None: free space."""
    rng = np.arange(-images, images + 1) if cell is not None else np.zeros(1, np.int64)
    S = np.array([(a, b, c) for a in rng for b in rng for c in rng])
    d = pos[None, :, None, :] - pos[:, None, None, :] + (S @ (np.eye(3) if cell is None else cell))[None, None, :, :]
    r = np.linalg.norm(d, axis=-1)
    i, j, k = np.nonzero((r < cutoff) & (r > 1e-12))
    return i, j, S[k]


def charge_entries(c, s, images=None):
    """The entries of system s of a charge case, with the system's own atom numbering."""
    sel = np.nonzero(c["batch_idx"] == s)[0]
    cell = None if c["cells"] is None else c["cells"][s]
    return brute_force(c["pos"][sel], cell, c["cutoff"], c["images"][s] if images is None else images)


def _with_entries(c):
    ii, jj, ss, off = [], [], [], 0
    for s in range(int(c["batch_idx"].max()) + 1):
        i, j, S = charge_entries(c, s)
        ii.append(i + off); jj.append(j + off); ss.append(S)
        off += int((c["batch_idx"] == s).sum())
    c["entries"] = (np.concatenate(ii), np.concatenate(jj), np.concatenate(ss))
    c["widest"] = int(np.bincount(c["entries"][0], minlength=len(c["pos"])).max()) if len(c["entries"][0]) else 0
    return c


@functools.lru_cache(maxsize=None)
def _charge_sweep(op, seed):
    g = np.random.default_rng(BASE[op] + seed)
    own = seed % 3 == 0  # the small systems sit in a cell shorter than the cutoff
    while True:
        sizes = tuple(int(v) for v in g.choice(CHARGE_SIZES, int(g.integers(1, 4))))
        if max(sizes) >= 9:
            break
    cutoff = float(g.uniform(6.0, 7.0))
    pos, cells, images = [], [], []
    for n in sizes:
        box = _BOX.get(n, 5.0 if own else 14.0)
        cell = charge_cell(box, bool(g.integers(2)))
        pos.append(g.uniform(0, 1, (n, 3)) @ cell)
        cells.append(cell)
        images.append(2 if box < cutoff else 1)
    ntot = sum(sizes)
    bi = np.concatenate([np.full(n, k, np.int32) for k, n in enumerate(sizes)])
    q = g.normal(size=ntot)
    neutral = seed % 2 == 1
    if neutral:
        for k in range(len(sizes)):
            q[bi == k] -= q[bi == k].mean()
    sigma = g.uniform(0.3, 0.8, ntot)
    sigma[g.choice(ntot, min(3, max(1, ntot // 20)), replace=False)] = 0.0
    big = int(np.argmax(sizes))
    while True:  # (the clusters of the seed's solve; a lone atom carries its total charge and needs no solve)
        clusters = tuple(int(v) for v in g.choice(CHARGE_SIZES, int(g.integers(1, 4))))
        if max(clusters) >= 9:
            break
    c = dict(op=op, dtype="float64" if seed % 2 == 0 else "float32", sizes=sizes, pos=np.concatenate(pos), cells=np.stack(cells), batch_idx=bi,
             cutoff=cutoff, images=tuple(images), q=q, neutral=neutral, sigma=sigma, pad=int(2 * g.integers(1, 5) + 1),
             emptied_row=int(np.sum(sizes[:big])) + sizes[big] // 2, hard=g.uniform(0.5, 1.5, ntot), x=g.normal(size=ntot), y_in=g.normal(size=ntot),
             alpha=g.uniform(0.3, 0.45, len(sizes)), flags={k: bool(g.integers(2)) for k in COMPUTE_FLAGS}, self_energy=bool(g.integers(2)),
             background=bool(g.integers(2)), cluster_sizes=clusters,
             cluster_seed=int(g.integers(1 << 30)), cluster_total=g.uniform(-1.5, 1.5, 3))
    _with_entries(c)
    i, j, S = c["entries"]
    own_image = (i == j) & (np.abs(S).sum(1) > 0)
    c["self_images"] = frozenset(int(v) for v in np.unique(bi[i[own_image]]))
    return c


@functools.lru_cache(maxsize=None)
def _charge_ladder(name):
    """Lane trips: a free cluster of n atoms without a cell, every pair stored: rows of n - 1 entries in a matrix exactly that wide."""
    n = int(name[1:])
    g = np.random.default_rng(7800 + n)
    pos = S.molecule(n, density=0.05, min_dist=1.0, seed=500 + n, dtype=np.float64)[0]
    sigma = g.uniform(0.3, 0.8, n)
    sigma[g.choice(n, 2, replace=False)] = 0.0
    c = dict(op="charges", dtype="float64", sizes=(n,), pos=pos, cells=None, batch_idx=np.zeros(n, np.int32), cutoff=1e9, images=(0,), q=g.normal(size=n),
             sigma=sigma, pad=0, emptied_row=None, hard=g.uniform(0.5, 1.5, n), x=g.normal(size=n), y_in=g.normal(size=n), alpha=None)
    return _with_entries(c)


@functools.lru_cache(maxsize=None)
def unrolled_case():
    """`box150` of tests/test_qeq_gpu.py (the same draws) at cutoff 9.5: rows of about 300 entries, more than the 256 one pass of
    `qeq_apply_kernel`'s four unrolled trips of 64 takes."""
    g = np.random.default_rng(11)
    n = 150
    cell = charge_cell(12.0)
    pos = g.uniform(0, 1, (n, 3)) @ cell
    sigma = g.uniform(0.3, 0.8, n)
    sigma[g.choice(n, 3, replace=False)] = 0.0
    c = dict(op="charge_equilibration", dtype="float64", sizes=(n,), pos=pos, cells=cell[None], batch_idx=np.zeros(n, np.int32), cutoff=9.5, images=(1,),
             sigma=sigma, pad=0, emptied_row=None, hard=g.uniform(0.5, 1.5, n), x=g.normal(size=n), y_in=g.normal(size=n), alpha=np.array([0.35]))
    return _with_entries(c)


# ---- point dipoles: ewald_dipole_correction and pme_dipole_correction -----------------------------------------------------------------------------
# Inputs, and for the mesh term the restatement in both of its modes (it runs on the CPU); the explicit sum's restatement is evaluated by
# the GPU module on the entries actually stored (tests/dipole_reference.py), as tests/test_dipole_gpu.py does.  The recipe is `_charge_sweep`
# with three differences.  CONTACTS: positions are drawn by rejection so that no two atom images are closer than `MIN_CONTACT` -- the
# real-space force goes as B3 ~ r^-7, and with uniform positions the float32 rounding of the distance of ONE close contact would decide the
# whole float32 comparison.  SPECIAL SEEDS: `ZERO_DIPOLE_SEEDS` have all dipoles zero (every output but dipole_grads is then exactly 0);
# `INTERLEAVED_SEEDS` have at least two systems and a seeded permutation `perm` of their atoms (`interleaved(c)` applies it: batch_idx is then
# not sorted; for `pme_dipole_reciprocal_space` and the real-space half only); `EMPTY_SYSTEM_SEEDS` have three systems whose middle one has
# no atom (sizes (a, 0, b), batch_idx holds 0 and 2, cells is [3, 3, 3]; both restatements accept such a batch).  MESH of a `pme_dipole` seed:
# order 4, 5, 6 in turn, dimensions drawn from {order, order + 1, 9, 10, 11, 12, 13, 16}.

DIPOLE_OPS = ("ewald_dipole", "pme_dipole")
BASE.update(ewald_dipole=7900, pme_dipole=8070)  # 8070: the first of 8000, 8010, ... whose twelve seeds meet every condition of the CPU suite
MIN_CONTACT = 1.0
DIPOLE_FLAGS = ("compute_forces", "compute_charge_gradients", "compute_dipole_gradients", "compute_virial")
DIPOLE_NAMES = ("energies", "forces", "charge_grads", "dipole_grads", "virial")
ZERO_DIPOLE_SEEDS = (1, 6, 11)
INTERLEAVED_SEEDS = (4, 8)   # even: float64, so that the interleaved and the sorted call are compared at the float64 bar of two device results
EMPTY_SYSTEM_SEEDS = (5, 10)
K_CUTOFF = 1.6               # of the sweep's explicit sums: up to 9 x 9 x 9 / 2 = 364 vectors per system
K_RUNGS = (63, 64, 65, 255, 256, 257, 513)
K_LADDER_CUTOFF = 3.0
K_LADDER_ALPHA = 1.0
ATOM_RUNGS = (255, 256, 257, 1)
ATOM_LADDER_K_CUTOFF = 0.75
SPREAD_MESH = (9, 10, 11)
SPREAD_POOL_SEED = 8480
BIG_MESH = (40, 36, 96)
PME_ORDERS = (4, 5, 6)
PG_ATOMS = 32                # atoms per block of `pme_dipole_gather_kernel`: 256 / PG_LANES; the CPU suite reads the #define


def mesh_choices(order):
    return (order, order + 1, 9, 10, 11, 12, 13, 16)


def spread_atoms_per_block(order):
    return 256 // (order * order)


def spread_rungs(order):
    apb = spread_atoms_per_block(order)
    return tuple(sorted({apb - 1, apb, apb + 1, 2 * apb, PG_ATOMS - 1, PG_ATOMS, PG_ATOMS + 1}))


def spaced_positions(g, n, cell, min_dist=MIN_CONTACT):
    """n points uniform in the cell, drawn one by one and rejected when closer than min_dist to an image of an accepted one."""
    rng = np.arange(-1, 2)
    images = np.array([(a, b, c) for a in rng for b in rng for c in rng]) @ cell
    pts = np.empty((0, 3))
    while len(pts) < n:
        p = g.uniform(0, 1, 3) @ cell
        if len(pts) == 0 or np.linalg.norm(pts[:, None, :] + images[None] - p, axis=-1).min() >= min_dist + 1e-6:  # (the margin: the CPU suite asserts >= min_dist on distances formed another way)
            pts = np.vstack([pts, p])
    return pts


def entry_distances(c):
    """|r_j - r_i + S . cell| of every entry of the case, float64."""
    i, j, S = c["entries"]
    shift = 0.0 if c["cells"] is None else np.einsum("ea,eab->eb", S.astype(np.float64), c["cells"][c["batch_idx"][i]])
    return np.linalg.norm(c["pos"][j] - c["pos"][i] + shift, axis=1)


def stored_entries(c):
    """(i, j, S) as the GPU module stores them: the emptied row taken out of the list from both ends."""
    i, j, S = c["entries"]
    if c["emptied_row"] is None:
        return i, j, S
    keep = (i != c["emptied_row"]) & (j != c["emptied_row"])
    return i[keep], j[keep], S[keep]


def interleaved(c):
    """The case with its atoms in the order `perm` (new atom k is old atom perm[k]): every per-atom array, the entries and the emptied row."""
    perm = c["perm"]
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    i, j, S = c["entries"]
    ni, nj = inv[i], inv[j]
    order = np.argsort(ni, kind="stable")
    out = dict(c, perm=None, entries=(ni[order], nj[order], S[order]), emptied_row=None if c["emptied_row"] is None else int(inv[c["emptied_row"]]))
    for k in ("pos", "q", "mu", "batch_idx", "weights"):
        out[k] = c[k][perm]
    return out


def _dipoles(g, n, zero=False):
    mu = 0.4 * g.normal(size=(n, 3))
    mu[g.choice(n, min(3, max(1, n // 20)), replace=False)] = 0.0  # a few atoms without a dipole
    return np.zeros((n, 3)) if zero else mu


@functools.lru_cache(maxsize=None)
def _dipole_sweep(op, seed):
    g = np.random.default_rng(BASE[op] + seed)
    own = seed % 3 == 0  # the small systems sit in a cell shorter than the cutoff
    while True:
        sizes = [int(v) for v in g.choice(CHARGE_SIZES, 3 if seed in EMPTY_SYSTEM_SEEDS else int(g.integers(2 if seed in INTERLEAVED_SEEDS else 1, 4)))]
        if seed in EMPTY_SYSTEM_SEEDS:
            sizes[1] = 0
        if max(sizes) >= 9:
            break
    sizes = tuple(sizes)
    cutoff = float(g.uniform(6.0, 7.0))
    pos, cells, images = [], [], []
    for n in sizes:
        box = _BOX.get(n, 5.0 if own else 14.0)
        cell = charge_cell(box, bool(g.integers(2)))
        pos.append(spaced_positions(g, n, cell))
        cells.append(cell)
        images.append(2 if box < cutoff else 1)
    ntot = sum(sizes)
    bi = np.concatenate([np.full(n, k, np.int32) for k, n in enumerate(sizes)])
    q = g.normal(size=ntot)
    neutral = seed % 2 == 1
    if neutral:
        for k in range(len(sizes)):
            if sizes[k]:
                q[bi == k] -= q[bi == k].mean()
    big = int(np.argmax(sizes))
    order = PME_ORDERS[seed % 3]
    c = dict(op=op, seed=seed, dtype="float64" if seed % 2 == 0 else "float32", sizes=sizes, pos=np.concatenate(pos), cells=np.stack(cells), batch_idx=bi,
             cutoff=cutoff, images=tuple(images), q=q, neutral=neutral, mu=_dipoles(g, ntot, zero=seed in ZERO_DIPOLE_SEEDS),
             zero_dipoles=seed in ZERO_DIPOLE_SEEDS, pad=int(2 * g.integers(1, 5) + 1), emptied_row=int(np.sum(sizes[:big])) + sizes[big] // 2,
             alpha=g.uniform(0.3, 0.45, len(sizes)), flags={k: bool(g.integers(2)) for k in DIPOLE_FLAGS}, autograd=bool(g.integers(2)),
             weights=g.uniform(0.2, 1.8, ntot), perm=g.permutation(ntot) if seed in INTERLEAVED_SEEDS else None,
             empty_system=1 if seed in EMPTY_SYSTEM_SEEDS else None, k_cutoff=K_CUTOFF, order=order,
             mesh=tuple(int(v) for v in g.choice(mesh_choices(order), 3)))
    _with_entries(c)
    i, j, S = c["entries"]
    own_image = (i == j) & (np.abs(S).sum(1) > 0)
    c["self_images"] = frozenset(int(v) for v in np.unique(bi[i[own_image]]))
    c["min_dist"] = float(entry_distances(c).min())
    return c


@functools.lru_cache(maxsize=None)
def _dipole_row_ladder(name):
    """Lane trips of `dp_pair_kernel`: a cluster of n atoms (`systems.molecule`, no contact below 1) inside a cubic cell four cluster diameters
    wide, every pair stored with a zero shift: rows of n - 1 entries, as a matrix exactly that wide and as CSR."""
    n = int(name[1:])
    g = np.random.default_rng(8100 + n)
    pos = S.molecule(n, density=0.05, min_dist=MIN_CONTACT, seed=600 + n, dtype=np.float64)[0]
    c = dict(op="ewald_dipole", dtype="float64", sizes=(n,), pos=pos, cells=None, batch_idx=np.zeros(n, np.int32), cutoff=1e9, images=(0,), q=g.normal(size=n),
             mu=_dipoles(g, n), zero_dipoles=False, pad=0, emptied_row=None, alpha=np.array([0.35]), weights=g.uniform(0.2, 1.8, n), perm=None, empty_system=None)
    _with_entries(c)
    dist = entry_distances(c)
    c["diameter"], c["min_dist"] = float(dist.max()), float(dist.min())
    c["cells"] = (np.eye(3) * 4.0 * c["diameter"])[None]
    return c


def _one_system(seed, n, box, triclinic=True, alpha=0.4):
    g = np.random.default_rng(seed)
    cell = charge_cell(box, triclinic)
    return g, dict(dtype="float64", sizes=(n,), pos=spaced_positions(g, n, cell), cells=cell[None], batch_idx=np.zeros(n, np.int32), q=g.normal(size=n) + 0.05,
                   mu=_dipoles(g, n), zero_dipoles=False, alpha=np.array([alpha]), weights=g.uniform(0.2, 1.8, n), perm=None, empty_system=None)


@functools.lru_cache(maxsize=None)
def dipole_k_case():
    """The K ladder of `dp_recip_gather_kernel` (64 k per trip) and `dp_recip_virial_kernel` (256): 60 atoms in the box of 9; the rungs are
    the first K vectors of the package's half-space set of cutoff `K_LADDER_CUTOFF`.  alpha is 1.0, not an Ewald parameter one would use with
    this set: at 0.4 the 513th vector carries 5e-17 of the largest Green weight and a kernel that skips it passes; at 1.0 every one of the 513
    carries at least 2e-7 of it (the CPU suite asserts 1e-7: 1e4 bars)."""
    _, c = _one_system(8200, 60, 9.0, alpha=K_LADDER_ALPHA)
    return dict(c, op="ewald_dipole", k_cutoff=K_LADDER_CUTOFF)


@functools.lru_cache(maxsize=None)
def dipole_atom_case():
    """The atom ladder of `dp_sf_kernel` (256 atoms per trip): one batch of 255, 256, 257 and 1 atoms in boxes of 14 to 15, about 65 k-vectors
    per system; reciprocal half only."""
    g = np.random.default_rng(8300)
    boxes, tri = (14.0, 14.5, 15.0, 14.0), (True, False, True, False)
    cells = np.stack([charge_cell(b, t) for b, t in zip(boxes, tri)])
    pos = np.concatenate([spaced_positions(g, n, cell) for n, cell in zip(ATOM_RUNGS, cells)])
    n = sum(ATOM_RUNGS)
    return dict(op="ewald_dipole", dtype="float64", sizes=ATOM_RUNGS, pos=pos, cells=cells, batch_idx=np.repeat(np.arange(4, dtype=np.int32), ATOM_RUNGS),
                q=g.normal(size=n) + 0.05, mu=_dipoles(g, n), zero_dipoles=False, alpha=g.uniform(0.3, 0.45, 4), weights=g.uniform(0.2, 1.8, n), perm=None,
                empty_system=None, k_cutoff=ATOM_LADDER_K_CUTOFF)


@functools.lru_cache(maxsize=None)
def _spread_pool(order):
    """33 atoms in the triclinic cell of tests/test_pme_dipole_gpu.py, fractional coordinates in [-0.2, 1.2]: stencils cross every face.
    The pool was drawn anew twice (DESIGN.md 3.21 says why); the CPU suite asserts the restatement's float32 deviation below 1e-5 on every rung."""
    g = np.random.default_rng(SPREAD_POOL_SEED + order)
    cell = np.array([[8.0, 0.0, 0.0], [0.7, 8.8, 0.0], [-0.4, 0.5, 7.2]])
    n = PG_ATOMS + 1
    return dict(pos=g.uniform(-0.2, 1.2, (n, 3)) @ cell, cells=cell[None], q=g.normal(size=n) + 0.05, mu=0.5 * g.normal(size=(n, 3)) / np.sqrt(3.0),
                weights=g.uniform(0.2, 1.8, n))


@functools.lru_cache(maxsize=None)
def dipole_spread_case(order, n):
    """The first n atoms of the order's pool on mesh `SPREAD_MESH`: blocks of `pme_dipole_spread_kernel` (256 // order^2 atoms) and of
    `pme_dipole_gather_kernel` (32 atoms) one atom short of full, full, and one atom into the next."""
    p = _spread_pool(order)
    return dict(op="pme_dipole", dtype=None, sizes=(n,), pos=p["pos"][:n], cells=p["cells"], batch_idx=np.zeros(n, np.int32), q=p["q"][:n], mu=p["mu"][:n],
                zero_dipoles=False, alpha=np.array([0.35]), weights=p["weights"][:n], perm=None, empty_system=None, order=order, mesh=SPREAD_MESH)


@functools.lru_cache(maxsize=None)
def dipole_big_mesh_case():
    """12 atoms on mesh (40, 36, 96): 40 x 36 x 49 = 70 560 half-spectrum points, more than the 256 x 256 one trip of
    `pme_dipole_virial_kernel`'s grid-stride loop covers."""
    _, c = _one_system(8500, 12, 9.0, alpha=0.35)
    return dict(c, op="pme_dipole", order=5, mesh=BIG_MESH)


def dipole_case(kind, key):
    """kind: "sweep" (key: (op, seed)), "row" (rung name), "k", "atoms", "spread" (key: (order, n)), "big"."""
    if kind == "sweep":
        return _dipole_sweep(*key)
    return {"row": _dipole_row_ladder, "k": lambda _: dipole_k_case(), "atoms": lambda _: dipole_atom_case(), "spread": lambda k: dipole_spread_case(*k),
            "big": lambda _: dipole_big_mesh_case()}[kind](key)


def dipole_tensors(c, dtype=torch.float64):
    """(pos, q, mu, cells, alpha, batch_idx | None) of a dipole case as CPU tensors; batch_idx None for one system."""
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype)  # noqa: E731
    bi = torch.as_tensor(c["batch_idx"]) if len(c["sizes"]) > 1 else None
    return t(c["pos"]), t(c["q"]), t(c["mu"]), t(c["cells"]), t(c["alpha"]), bi


def dipole_k_vectors(c, dtype=torch.float64):
    """The case's k set from the package's generator ([K, 3] for one system, [B, K, 3] for a batch), on the CPU."""
    from nvalchemiops.interactions.electrostatics import generate_k_vectors_ewald_summation

    cells = torch.as_tensor(c["cells"], dtype=dtype)
    return generate_k_vectors_ewald_summation(cells if len(c["sizes"]) > 1 else cells[0], c["k_cutoff"])


@functools.lru_cache(maxsize=None)
def pme_dipole_reference(kind, key, mode="float64", weighted=False):
    """`pme_dipole_reference.evaluate` on the case's mesh and order, in its float64 or its float32 mode; `weighted`: the derivatives are those
    of L = sum_i w_i E_i with the case's weights (and no virial), else of the total energy."""
    c = dipole_case(kind, key)
    pos, q, mu, cells, alpha, bi = dipole_tensors(c)
    return PR.evaluate(pos, q, mu, cells, alpha if bi is not None else float(alpha[0]), c["mesh"], c["order"], batch_idx=bi,
                       weights=torch.as_tensor(c["weights"]) if weighted else None, dtype=torch.float64 if mode == "float64" else torch.float32,
                       virial=not weighted)


def pme_float32_deviation(kind, key, weighted=False):
    """Per output: max |float32 mode - float64 mode| / max |float64 mode| of the restatement: a quarter of the float32 bar of the GPU test."""
    r64, r32 = pme_dipole_reference(kind, key, "float64", weighted), pme_dipole_reference(kind, key, "float32", weighted)
    return {k: float(np.abs(r32[k] - r64[k]).max() / np.abs(r64[k]).max()) for k in r64 if np.abs(r64[k]).max() > 0}


def green_weights(c, k_vectors):
    """G_k = (8 pi / V) exp(-k^2 / 4 alpha^2) / k^2 of the k-vectors of a one-system case (numpy)."""
    k2 = (np.asarray(k_vectors, np.float64) ** 2).sum(-1)
    return 8.0 * np.pi / abs(np.linalg.det(c["cells"][0])) * np.exp(-k2 / (4.0 * float(c["alpha"][0]) ** 2)) / k2


def hermitian_plane_virial(kind, key):
    """Per system [B, 3, 3]: what the plane k = (nz - 1) / 2 of the half spectrum of an odd-nz mesh adds to the k-space virial for one unit
    of its Hermitian weight (`pme_dipole_reference.half_spectrum_plane_virial`).  A kernel that weighs this plane once instead of twice
    (`k == nz / 2` for `2 * k == nz`) is off by exactly this much."""
    c = dipole_case(kind, key)
    assert c["mesh"][2] % 2 == 1
    pos, q, mu, cells, alpha, bi = dipole_tensors(c)
    sys_of = torch.zeros(len(pos), dtype=torch.long) if bi is None else bi.long()
    out = np.zeros((len(cells), 3, 3))
    for s, cell in enumerate(cells):
        own = torch.nonzero(sys_of == s).reshape(-1)
        if own.numel():
            out[s] = PR.half_spectrum_plane_virial(pos[own], q[own], mu[own], cell, alpha[s], c["mesh"], c["order"], c["mesh"][2] // 2)
    return out


# ---- point quadrupoles and Thole damping: ewald_quadrupole_correction and thole_dipole_correction ------------------------------------------------
# Inputs only; both restatements (tests/quadrupole_reference.py, tests/thole_reference.py) are evaluated by the GPU module on the entries
# actually stored.  A seed is the dipole recipe above under the operator's own BASE (geometry with spaced positions, charges, weights, the
# emptied row, the interleaving permutation, the system without atoms, alpha) with dipoles on EVERY seed -- the dipole section's zero-dipole
# seeds get dipoles here: without them the Thole correction and the dipole-quadrupole term vanish -- plus quadrupoles 0.3 x normal,
# symmetrised, a few zero rows and a few rows with an antisymmetric part, or polarisabilities uniform in [0.5, 4] with a few non-polarisable
# atoms (0).  With contacts from 1 to the cutoff of 6 - 7, E = a_T r^3 / sqrt(a_i a_j) runs from 0.1 to beyond the kernel's exit at 50.
# `ZERO_MULTIPOLE_SEEDS`: all quadrupoles zero (every output but quadrupole_grads exactly 0) / every atom non-polarisable (every output
# exactly 0).  `SINGLE_FLAG_SEEDS`: seed k of them asks for flag k alone; the other seeds draw a subset.

MULTIPOLE_OPS = ("ewald_quadrupole", "thole")
BASE.update(ewald_quadrupole=8600, thole=8700)
QUADRUPOLE_FLAGS = ("compute_forces", "compute_charge_gradients", "compute_dipole_gradients", "compute_quadrupole_gradients", "compute_virial")
QUADRUPOLE_NAMES = ("energies", "forces", "charge_grads", "dipole_grads", "quadrupole_grads", "virial")
THOLE_FLAGS = ("compute_forces", "compute_charge_gradients", "compute_dipole_gradients", "compute_polarizability_gradients", "compute_virial")
THOLE_NAMES = ("energies", "forces", "charge_grads", "dipole_grads", "polar_grads", "virial")
MULTIPOLE_FLAGS = {"ewald_quadrupole": QUADRUPOLE_FLAGS, "thole": THOLE_FLAGS}
MULTIPOLE_NAMES = {"ewald_quadrupole": QUADRUPOLE_NAMES, "thole": THOLE_NAMES}
ZERO_MULTIPOLE_SEEDS = ZERO_DIPOLE_SEEDS
SINGLE_FLAG_SEEDS = (0, 2, 3, 7, 9)  # the seeds with no other designation
THOLE = 0.39
THOLE_EXIT = 50.0            # `thole_dipole_correction` skips entries with E >= 50
THOLE_ROWS = (0, 1, 63, 64, 65, 128, 129)


def _quadrupoles(g, n, zero=False):
    qd = 0.3 * g.normal(size=(n, 3, 3))
    qd = 0.5 * (qd + qd.transpose(0, 2, 1))
    pick = g.permutation(n)
    few = min(3, max(1, n // 20))
    qd[pick[:few]] = 0.0  # a few atoms without a quadrupole
    if n > 2 * few:
        skew = 0.1 * g.normal(size=(few, 3, 3))
        qd[pick[few:2 * few]] += skew - skew.transpose(0, 2, 1)  # 1/2 (Q + Q^T) is what counts
    return np.zeros((n, 3, 3)) if zero else qd


def _polarisabilities(g, n, zero=False, lo=0.5, hi=4.0):
    a = g.uniform(lo, hi, n)
    if n > 3:
        a[g.choice(n, min(3, max(1, n // 20)), replace=False)] = 0.0  # a few non-polarisable atoms
    return np.zeros(n) if zero else a


@functools.lru_cache(maxsize=None)
def _multipole_sweep(op, seed):
    c = dict(_dipole_sweep(op, seed))
    g = np.random.default_rng(BASE[op] + 500 + seed)
    n = len(c["pos"])
    if c["zero_dipoles"]:
        c.update(mu=_dipoles(g, n), zero_dipoles=False)
    names = MULTIPOLE_FLAGS[op]
    if seed in SINGLE_FLAG_SEEDS:
        c["flags"] = {k: k == names[SINGLE_FLAG_SEEDS.index(seed)] for k in names}
    else:
        c["flags"] = {k: bool(g.integers(2)) for k in names}
    c["zero"] = seed in ZERO_MULTIPOLE_SEEDS
    if op == "ewald_quadrupole":
        c["qd"] = _quadrupoles(g, n, c["zero"])
    else:
        c["polar"] = _polarisabilities(g, n, c["zero"])
    return c


def multipole_interleaved(c):
    """`interleaved(c)` with the quadrupoles / polarisabilities in the new atom order too."""
    out = interleaved(c)
    for k in ("qd", "polar"):
        if k in c:
            out[k] = c[k][c["perm"]]
    return out


def thole_exponents(c, entries=None):
    """E = a_T r^3 / sqrt(a_i a_j) of the entries whose two atoms are polarisable, and the rows they belong to."""
    i, j, _ = c["entries"] if entries is None else entries
    r = entry_distances(c if entries is None else dict(c, entries=entries))
    ok = (c["polar"][i] > 0) & (c["polar"][j] > 0)
    return THOLE * r[ok] ** 3 / np.sqrt(c["polar"][i][ok] * c["polar"][j][ok]), i[ok]


@functools.lru_cache(maxsize=None)
def quadrupole_atom_case():
    """`dipole_atom_case()` (systems of 255, 256, 257 and 1 atoms in one batch, about 65 k-vectors per system) with quadrupoles: the 256-atom
    trips of `qd_sf_kernel` and its `sptr`; reciprocal half only."""
    c = dict(dipole_atom_case(), op="ewald_quadrupole")
    c["qd"] = _quadrupoles(np.random.default_rng(8610), len(c["pos"]))
    return c


@functools.lru_cache(maxsize=None)
def quadrupole_no_shift_case():
    """The 65-atom row rung of the dipole section (a cluster inside a cubic cell four diameters wide, every pair stored with a zero shift:
    rows of 64 entries) with quadrupoles: the list is passed with zero shifts and without shifts (`ush == nullptr` in `qd_pair_kernel`)."""
    c = dict(_dipole_row_ladder("n65"), op="ewald_quadrupole")
    c["qd"] = _quadrupoles(np.random.default_rng(8620), len(c["pos"]))
    return c


@functools.lru_cache(maxsize=None)
def quadrupole_shared_k_case():
    """Two systems of 60 and 9 atoms in the SAME triclinic cell of edge 9 with one alpha: one k set [1, K, 3] serves both."""
    g = np.random.default_rng(8630)
    cell = charge_cell(9.0)
    sizes = (60, 9)
    n = sum(sizes)
    pos = np.concatenate([spaced_positions(g, m, cell) for m in sizes])
    return dict(op="ewald_quadrupole", dtype="float64", sizes=sizes, pos=pos, cells=np.stack([cell, cell]), batch_idx=np.repeat(np.arange(2, dtype=np.int32), sizes),
                q=g.normal(size=n) + 0.05, mu=_dipoles(g, n), qd=_quadrupoles(g, n), zero_dipoles=False, alpha=np.array([0.4, 0.4]),
                weights=g.uniform(0.2, 1.8, n), perm=None, empty_system=None, k_cutoff=K_CUTOFF)


@functools.lru_cache(maxsize=None)
def thole_row_ladder(periodic=True):
    """Rows of exactly 0, 1, 63, 64, 65, 128 and 129 entries in a FULL list built by hand, as `_ladder` of tests/test_quadrupole_gpu.py
    builds it: ladder atom t is paired with that many distinct (filler atom, shift) combinations and the filler rows hold the reversed
    entries (j, i, -S).  periodic: 40 fillers in a triclinic box of edge 6, shifts in [-1, 1]^3 (entry distances 1 - 15).  Not periodic: a
    cluster of 130 fillers without a cell (`cell=None`), every shift zero.  The row of one entry holds the ladder atom's NEAREST partner,
    so that it lies inside the exit; polarisabilities uniform in [0.5, 2] put E = 50 at r = 4 - 6.3, inside the span of every longer row."""
    n_fill = 40 if periodic else 130
    n = len(THOLE_ROWS) + n_fill
    g = np.random.default_rng(8700 + n_fill)
    if periodic:
        cell = charge_cell(6.0)
        pos = spaced_positions(g, n, cell)
        shifts = np.array([(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)])
    else:
        cell, pos, shifts = None, S.molecule(n, density=0.05, min_dist=MIN_CONTACT, seed=700, dtype=np.float64)[0], np.zeros((1, 3), np.int64)
    combos = [(f, s) for f in range(len(THOLE_ROWS), n) for s in range(len(shifts))]
    ei, ej, eS = [], [], []
    for t, length in enumerate(THOLE_ROWS):
        if length == 1:
            d = [np.linalg.norm(pos[f] - pos[t] + (shifts[s] @ cell if periodic else 0.0)) for f, s in combos]
            chosen = [int(np.argmin(d))]
        else:
            chosen = g.choice(len(combos), length, replace=False)
        for k in chosen:
            f, s = combos[k]
            ei += [t, f]; ej += [f, t]; eS += [shifts[s], -shifts[s]]  # noqa: E702
    ei, ej, eS = np.array(ei), np.array(ej), np.array(eS).reshape(-1, 3)
    order = np.argsort(ei, kind="stable")
    polar = g.uniform(0.5, 2.0, n)
    polar[g.choice(np.arange(len(THOLE_ROWS), n), 2, replace=False)] = 0.0  # two non-polarisable fillers
    c = dict(op="thole", dtype="float64", sizes=(n,), pos=pos, cells=None if cell is None else cell[None], batch_idx=np.zeros(n, np.int32), q=g.normal(size=n) + 0.05,
             mu=_dipoles(g, n), polar=polar, zero_dipoles=False, weights=g.uniform(0.2, 1.8, n), perm=None, empty_system=None, pad=0, emptied_row=None,
             entries=(ei[order], ej[order], eS[order]))
    c["widest"] = int(np.bincount(c["entries"][0], minlength=n).max())
    c["min_dist"] = float(entry_distances(c).min())
    return c


def multipole_case(kind, key=None):
    """kind: "sweep" (key: (op, seed)), "atoms", "no_shifts", "shared_k", "thole_rows" (key: periodic)."""
    if kind == "sweep":
        return _multipole_sweep(*key)
    return {"atoms": lambda _: quadrupole_atom_case(), "no_shifts": lambda _: quadrupole_no_shift_case(), "shared_k": lambda _: quadrupole_shared_k_case(),
            "thole_rows": lambda k: thole_row_ladder(bool(k))}[kind](key)


@functools.lru_cache(maxsize=None)
def induced_idle_systems_case():
    """A batch of three cells for `induced_dipoles`: system 0 is the 27-atom lattice of tests/induced_cases.py (it iterates), system 1 has NO
    atoms, system 2 has nine charged atoms of which NONE is polarisable (a = 0): its right-hand side is zero on every atom."""
    from tests import induced_cases as IC

    a = IC.lattice("l27")
    g = np.random.default_rng(8800)
    cell2 = charge_cell(7.0)
    pos2 = spaced_positions(g, 9, cell2)
    i0, j0, S0 = (e.numpy() for e in IC.entries("l27"))
    i2, j2, S2 = brute_force(pos2, cell2, 6.0, 2)
    n = 36
    c = dict(sizes=(27, 0, 9), pos=np.concatenate([a["pos"], pos2]), cells=np.stack([a["cell"], charge_cell(8.0, False), cell2]),
             batch_idx=np.repeat(np.array([0, 2], np.int32), (27, 9)), q=np.concatenate([a["q"], g.normal(size=9)]),
             polar=np.concatenate([a["polar"], np.zeros(9)]), alpha=np.array([IC.EWALD["alpha"], 0.4, 0.5]), k_cutoff=IC.EWALD["k_cutoff"],
             entries=(np.concatenate([i0, i2 + 27]), np.concatenate([j0, j2 + 27]), np.concatenate([S0, S2])), pad=3, emptied_row=None)
    c["widest"] = int(np.bincount(c["entries"][0], minlength=n).max())
    return c


# ---- point quadrupoles on the mesh: pme_quadrupole_correction ---------------------------------------------------------------------------------------
# Inputs and the restatement (tests/pme_quadrupole_reference.py, on the CPU, on the same mesh and order) in both of its modes.  A seed is the
# dipole recipe above under its own BASE (geometry with spaced positions, one to three systems with their own cells and alpha, weights, the
# emptied row of the stored list, the interleaving permutation, the system without atoms) with dipoles on every seed but `NO_DIPOLE_SEED`
# (there the call passes `dipoles=None`; the seed is an empty-system seed, so it has two systems with atoms), quadrupoles as in the
# `ewald_quadrupole` sweep and that sweep's flags.  ORDER 5 and 6 in turn, two seeds each ((seed // 2) % 2): the dtype alternates with the
# seed, so every order meets both dtypes.  MESH: three draws from `mesh_choices(order)`.  The ladder, the knot cases and the big mesh follow
# the seeds.  tests/test_sweep_cases_cpu.py asserts the conditions; tests/test_sweep_pme_quadrupole_gpu.py runs the kernels on them.

BASE.update(pme_quadrupole=8920)  # 8920: the first of 8900, 8910, ... whose twelve seeds meet every condition of the CPU suite
PMEQ_ORDERS = (5, 6)
NO_DIPOLE_SEED = 5
PMEQ_POOL_SEED = 8990        # of the ladder's pool, + order: the first of 8980, 8990, ... whose rungs are within the float32 cap (rung 1: but for `PMEQ_LONE_ATOM_EXEMPT`) and whose first atom has a dipole and a quadrupole
PMEQ_LONE_ATOM_EXEMPT = ("forces", "dipole_grads")  # of rung 1 in float32: see `pmeq_spread_case`
PMEQ_KNOT_SEED = 8960
PMEQ_KNOT_CASES = ((5, (16, 16, 16)), (6, (16, 16, 16)), (6, (6, 8, 16)), (5, (5, 8, 16)))
PMEQ_KNOT_SHIFTS = ((0, 0, -3), (1, 1, 2), (2, 2, 1))  # (atom, axis, whole cells) of the lattice-translation check
PMEQ_GRADS = ("forces", "charge_grads", "dipole_grads", "quadrupole_grads")


def pmeq_spread_rungs(order):
    return (1,) + spread_rungs(order)


@functools.lru_cache(maxsize=None)
def _pmeq_sweep(seed):
    c = dict(_dipole_sweep("pme_quadrupole", seed))
    g = np.random.default_rng(BASE["pme_quadrupole"] + 500 + seed)
    n = len(c["pos"])
    if c["zero_dipoles"]:
        c.update(mu=_dipoles(g, n), zero_dipoles=False)
    if seed == NO_DIPOLE_SEED:
        c.update(mu=np.zeros((n, 3)))
    c["no_dipoles"] = seed == NO_DIPOLE_SEED
    if seed in SINGLE_FLAG_SEEDS:
        c["flags"] = {k: k == QUADRUPOLE_FLAGS[SINGLE_FLAG_SEEDS.index(seed)] for k in QUADRUPOLE_FLAGS}
    else:
        c["flags"] = {k: bool(g.integers(2)) for k in QUADRUPOLE_FLAGS}
    c["zero"] = seed in ZERO_MULTIPOLE_SEEDS
    c["qd"] = _quadrupoles(g, n, c["zero"])
    c["order"] = PMEQ_ORDERS[(seed // 2) % 2]
    c["mesh"] = tuple(int(v) for v in g.choice(mesh_choices(c["order"]), 3))
    return c


@functools.lru_cache(maxsize=None)
def _pmeq_pool(order):
    """`_spread_pool` with quadrupoles: 33 atoms in the triclinic cell of tests/test_pme_quadrupole_gpu.py, fractional coordinates in
    [-0.2, 1.2]; charges, dipoles, quadrupoles and weights."""
    g = np.random.default_rng(PMEQ_POOL_SEED + order)
    cell = np.array([[8.0, 0.0, 0.0], [0.7, 8.8, 0.0], [-0.4, 0.5, 7.2]])
    n = PG_ATOMS + 1
    return dict(pos=g.uniform(-0.2, 1.2, (n, 3)) @ cell, cells=cell[None], q=g.normal(size=n) + 0.05, mu=0.5 * g.normal(size=(n, 3)) / np.sqrt(3.0),
                qd=_quadrupoles(g, n), weights=g.uniform(0.2, 1.8, n))


def _pmeq_one(pos, q, mu, qd, weights, cells, order, mesh, alpha=0.35):
    n = len(pos)
    return dict(op="pme_quadrupole", dtype=None, sizes=(n,), pos=pos, cells=cells, batch_idx=np.zeros(n, np.int32), q=q, mu=mu, qd=qd, zero=False,
                zero_dipoles=False, no_dipoles=False, alpha=np.array([alpha]), weights=weights, perm=None, empty_system=None, order=order, mesh=tuple(mesh))


@functools.lru_cache(maxsize=None)
def pmeq_spread_case(order, n):
    """The first n atoms of the order's pool on `SPREAD_MESH`: blocks of `pme_quadrupole_spread_kernel` (256 // order^2 atoms: 10 and 7) and of
    `pme_quadrupole_gather_kernel` (32) one atom short of full, full, one atom into the next, two blocks; and one atom as a call of its own.
    RUNG 1: one atom among its own images feels no net force and no net field but for the mesh's own anisotropy: forces and dipole_grads
    are what is left of terms that cancel, and the restatement's float32 mode deviates from its float64 mode there by 5e-5 - 7.5e-3 of the
    output's maximum (this pool: forces 7.3e-5 / 8.9e-4, dipole_grads 5.4e-5 / 7.5e-3 at orders 5 / 6; above the cap in every draw tried).
    In float32 these two outputs -- `PMEQ_LONE_ATOM_EXEMPT`, forward and weighted backward -- are only required to be finite.  Energies,
    charge_grads, quadrupole_grads and virial of the lone atom are within the cap on this pool (4e-7 - 3e-6) and are held to the float32
    bar like every other rung; in float64 all six outputs are."""
    p = _pmeq_pool(order)
    return _pmeq_one(p["pos"][:n], p["q"][:n], p["mu"][:n], p["qd"][:n], p["weights"][:n], p["cells"], order, SPREAD_MESH)


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def pmeq_knot_case(order, mesh):
    """12 atoms in the cubic cell of edge 8 whose MESH coordinates u = n x / 8 sit on spline knots: integers for the first six atoms (at
    order 6 theta = 0 and one stencil point at u = 0), integers + 1/2 for the last six (at order 5 theta - 3/2 = -1 exactly), drawn from
    [-3, n + 3].  Atom 0 is at (0, 0, 0), atom 1 at (nx, ny, nz) (base = n, wrapped), atom 2 at (-1, ny, 1/2); atoms 3, 6 and 7 have one
    generic axis each (x, y, z).  Every position is a float32 number, so both dtypes see the same inputs; on an axis of 8 or 16 points the mesh
    coordinate is then exact in both dtypes, on the axes of 5 and 6 points it is a knot up to the rounding of x (|du| <= 4e-7), on either
    side of it.  The restatement is continuous there (the CPU suite measures by how much +-1e-7 moves it), so it is a valid yardstick."""
    g = np.random.default_rng(PMEQ_KNOT_SEED + 10 * order + mesh[0])
    dims = np.array(mesh)
    u = np.stack([g.integers(-3, dims + 4) for _ in range(12)]).astype(np.float64)
    u[6:] = np.stack([g.integers(-3, dims + 3) for _ in range(6)]) + 0.5
    u[0], u[1], u[2] = 0.0, dims, (-1.0, mesh[1], 0.5)
    for atom, axis in ((3, 0), (6, 1), (7, 2)):
        u[atom, axis] = g.uniform(-3.0, mesh[axis] + 3.0)
    pos = _f32(u / dims * 8.0)
    c = _pmeq_one(pos, _f32(g.normal(size=12) + 0.05), _f32(0.5 * g.normal(size=(12, 3)) / np.sqrt(3.0)), _f32(_quadrupoles(g, 12)),
                  _f32(g.uniform(0.2, 1.8, 12)), (np.eye(3) * 8.0)[None], order, mesh)
    c["mesh_coordinates"] = u
    return c


def pmeq_translated(c):
    """The knot case with three atoms moved by whole lattice vectors (`PMEQ_KNOT_SHIFTS`): the same periodic system."""
    pos = c["pos"].copy()
    for atom, axis, cells in PMEQ_KNOT_SHIFTS:
        pos[atom] += cells * c["cells"][0][axis]
    return dict(c, pos=pos)


@functools.lru_cache(maxsize=None)
def pmeq_big_mesh_case():
    """The atoms of `dipole_big_mesh_case()` with quadrupoles on mesh (40, 36, 96), order 5: 70 560 half-spectrum points, the second trip of
    `pme_quadrupole_virial_kernel`'s grid-stride loop.  Float64 only: the restatement's float32 mode deviates by 4.6e-4 in the forces and
    1.3e-4 in the virial on this mesh (the factor n^3 of the third derivative); four times that is no bar."""
    c = dipole_big_mesh_case()
    n = len(c["pos"])
    return _pmeq_one(c["pos"], c["q"], c["mu"], _quadrupoles(np.random.default_rng(8950), n), c["weights"], c["cells"], 5, BIG_MESH, alpha=float(c["alpha"][0]))


def pmeq_case(kind, key=None):
    """kind: "sweep" (key: seed), "spread" (key: (order, n)), "knots" (key: (order, mesh)), "big"."""
    return {"sweep": _pmeq_sweep, "spread": lambda k: pmeq_spread_case(*k), "knots": lambda k: pmeq_knot_case(*k), "big": lambda _: pmeq_big_mesh_case()}[kind](key)


def pmeq_tensors(c, dtype=torch.float64):
    """(pos, q, mu, qd, cells, alpha, batch_idx | None) of a case as CPU tensors; batch_idx None for one system."""
    pos, q, mu, cells, alpha, bi = dipole_tensors(c, dtype)
    return pos, q, mu, torch.as_tensor(np.ascontiguousarray(c["qd"]), dtype=dtype), cells, alpha, bi


def pmeq_evaluate(c, mode="float64", weighted=False):
    from tests import pme_quadrupole_reference as QR

    pos, q, mu, qd, cells, alpha, bi = pmeq_tensors(c)
    return QR.evaluate(pos, q, mu, qd, cells, alpha if bi is not None else float(alpha[0]), c["mesh"], c["order"], batch_idx=bi,
                       weights=torch.as_tensor(c["weights"]) if weighted else None, dtype=torch.float64 if mode == "float64" else torch.float32,
                       virial=not weighted)


@functools.lru_cache(maxsize=None)
def pme_quadrupole_reference(kind, key, mode="float64", weighted=False):
    """`pme_quadrupole_reference.evaluate` on the case's mesh and order, in its float64 or its float32 mode; `weighted`: the derivatives are
    those of L = sum_i w_i E_i with the case's weights (and no virial), else of the total energy."""
    return pmeq_evaluate(pmeq_case(kind, key), mode, weighted)


def pmeq_float32_deviation(kind, key, weighted=False):
    """Per output: max |float32 mode - float64 mode| / max |float64 mode| of the restatement: a quarter of the float32 bar of the GPU test."""
    r64, r32 = pme_quadrupole_reference(kind, key, "float64", weighted), pme_quadrupole_reference(kind, key, "float32", weighted)
    return {k: float(np.abs(r32[k] - r64[k]).max() / np.abs(r64[k]).max()) for k in r64 if np.abs(r64[k]).max() > 0}


def pmeq_plane_virial(kind, key):
    """Per system [B, 3, 3]: what the plane k = (nz - 1) / 2 of the half spectrum of an odd-nz mesh adds to the k-space virial of the cross
    spectrum for one unit of its Hermitian weight (`pme_quadrupole_reference.half_spectrum_plane_virial`)."""
    from tests import pme_quadrupole_reference as QR

    c = pmeq_case(kind, key)
    assert c["mesh"][2] % 2 == 1
    pos, q, mu, qd, cells, alpha, bi = pmeq_tensors(c)
    sys_of = torch.zeros(len(pos), dtype=torch.long) if bi is None else bi.long()
    out = np.zeros((len(cells), 3, 3))
    for s, cell in enumerate(cells):
        own = torch.nonzero(sys_of == s).reshape(-1)
        if own.numel():
            out[s] = QR.half_spectrum_plane_virial(pos[own], q[own], mu[own], qd[own], cell, alpha[s], c["mesh"], c["order"], c["mesh"][2] // 2)
    return out


@functools.lru_cache(maxsize=None)
def pmeq_convergence():
    """Per output: the relative difference (max |difference| / max |explicit|) between the restatement of the mesh term at order 6 on 32^3
    and the explicit reciprocal sum of tests/quadrupole_reference.py on the converged k set (cutoff 4.5: exp(-k^2 / 4 alpha^2) = 1e-18), both
    on the 37-atom system of tests/test_pme_quadrupole_gpu.py.  Ten times these are the bars of
    tests/test_sweep_pme_quadrupole_gpu.py::test_mesh_term_converges_to_the_explicit_sum_in_every_output: numbers of the two restatements."""
    from nvalchemiops.interactions.electrostatics import generate_k_vectors_ewald_summation
    from tests import pme_quadrupole_reference as QR
    from tests import quadrupole_reference as XR
    from tests import test_pme_quadrupole_gpu as TPQ

    t = lambda a: torch.tensor(a, dtype=torch.float64)  # noqa: E731
    pos, q, mu, qd = (t(a) for a in TPQ._system())
    cell = t(TPQ.CELL).reshape(1, 3, 3)
    mesh = QR.evaluate(pos, q, mu, qd, cell, TPQ.ALPHA, (32, 32, 32), 6)
    explicit = XR.evaluate(pos, q, mu, qd, cell, t([TPQ.ALPHA]), None, generate_k_vectors_ewald_summation(cell[0], 4.5))
    return {k: float(np.abs(mesh[k] - explicit[k]).max() / np.abs(explicit[k]).max()) for k in QUADRUPOLE_NAMES}


@functools.lru_cache(maxsize=None)
def pmeq_batch_seed():
    """The first seed with three systems with atoms, quadrupoles and dipoles, not interleaved: the batch of
    test_batch_systems_equal_single_calls_forward_and_backward, which runs in both dtypes."""
    for s in SEEDS:
        c = _pmeq_sweep(s)
        if len(c["sizes"]) == 3 and min(c["sizes"]) > 0 and not c["zero"] and not c["no_dipoles"] and c["perm"] is None:
            return s
    raise AssertionError("no seed with three systems with atoms")


# ---- cluster multipoles, scaled pairs, local frames: coulomb_dipole_correction, coulomb_quadrupole_correction, pair_scale_correction,
#      rotate_multipoles / multipole_frame_forces -------------------------------------------------------------------------------------------------
# Inputs only; the restatements (tests/cluster_multipole_reference.py, tests/pair_scale_reference.py, tests/local_frames_reference.py) are
# evaluated by the GPU module on the entries actually stored.  A PAIR seed: 1 - 4 systems with sizes from {1, 2, 9, 60, 150} (and one system
# of 0 atoms on `EMPTY_SYSTEM_SEEDS`), `spaced_positions` at `CLUSTER_D_MIN` = the 1.3 of tests/cluster_multipole_reference.py so that family's
# bars apply, as clusters (all pairs of every system) or in triclinic cells (`CLUSTER_PERIODIC_SEEDS`: every image within a cutoff of 4 - 5,
# the small systems in a cell of 4.5 with their own images).  `padded_matrix` stores a list as a matrix with all three kinds of padding and,
# on every other row, one padding slot BETWEEN live entries.  The designations are the quadrupole section's: `ZERO_MULTIPOLE_SEEDS` (zero
# dipoles / zero quadrupoles / for `pair_scale` unit scales: every output exactly 0), `INTERLEAVED_SEEDS`, `EMPTY_SYSTEM_SEEDS`,
# `SINGLE_FLAG_SEEDS`.  `pair_scale` only: scales from the symmetric hash of tests/pair_scale_cases.py (0, 0.4, 0.8, 1), float32 scales on
# `PS_F32_SCALE_SEEDS`, `minimum_image` on `PS_MIN_IMAGE_SEEDS` (periodic seeds whose list is cut to the pairs whose stored shift is the
# minimum image with every fractional component at most 0.45, and given without shifts: a topology list), `dipoles=None` /
# `quadrupoles=None` on one seed each, and on `PS_COINCIDENT_SEED` two atoms at the same point listed both ways (r <= 1e-8: skipped).

CLUSTER_OPS = ("coulomb_dipole", "coulomb_quadrupole", "pair_scale")
BASE.update(coulomb_dipole=9100, coulomb_quadrupole=9200, pair_scale=9300, frames=9400)
CLUSTER_D_MIN = 1.3
CLUSTER_SIZES = (1, 2, 9, 60, 150)
CLUSTER_PERIODIC_SEEDS = (0, 1, 4, 5, 6, 8, 11)
CLUSTER_FLAGS = {"coulomb_dipole": DIPOLE_FLAGS, "coulomb_quadrupole": QUADRUPOLE_FLAGS, "pair_scale": QUADRUPOLE_FLAGS}
CLUSTER_NAMES = {"coulomb_dipole": DIPOLE_NAMES, "coulomb_quadrupole": QUADRUPOLE_NAMES, "pair_scale": QUADRUPOLE_NAMES}
PS_F32_SCALE_SEEDS = (3, 6)
PS_MIN_IMAGE_SEEDS = (1, 8)
PS_NO_DIPOLE_SEED, PS_NO_QUADRUPOLE_SEED, PS_COINCIDENT_SEED = 2, 7, 9
PS_IMAGE_MARGIN = 0.45
PS_LADDER = (255, 256, 257, 1)


def hash_scale(i, j):
    """The symmetric hash of tests/pair_scale_cases.py on arrays: the classes 0, 0.4, 0.8 and 1."""
    return np.array([0.0, 0.4, 0.8, 1.0, 0.4])[(i * j + i + j) % 5]


def fractional_pair_vectors(c, entries=None):
    """r_j - r_i + S . cell of every entry in fractional coordinates of its system's cell."""
    i, j, S = c["entries"] if entries is None else entries
    cells = c["cells"][c["batch_idx"][i]]
    d = c["pos"][j] - c["pos"][i] + np.einsum("ea,eab->eb", S.astype(np.float64), cells)
    return np.einsum("ea,eab->eb", d, np.linalg.inv(cells))


def padded_matrix(entries, n, values=None):
    """(neighbor_matrix [n, M], shifts [n, M, 3], values [n, M] with NaN on padding | None) of entries sorted by row, their order kept.  Rows are
    seven columns wider than the longest; padding is the mask value n, with -1 in the last column and n + 7 in every other row of the one
    before; on every other row that holds at least two entries the second entry onwards is moved one slot to the right, which leaves one
    padding slot between live entries."""
    i, j, S = entries
    counts = np.bincount(i, minlength=n) if len(i) else np.zeros(n, np.int64)
    m = int(counts.max() if n else 0) + 8
    col = np.arange(len(i)) - (np.cumsum(counts) - counts)[i]
    col = col + ((col >= 1) & (i % 2 == 1) & (counts[i] >= 2))
    nm = np.full((n, m), n, np.int32)
    sh = np.zeros((n, m, 3), np.int32)
    nm[i, col], sh[i, col] = j, S
    nm[:, -1] = -1
    nm[::2, -2] = n + 7
    val = None
    if values is not None:
        val = np.full((n, m), np.nan)
        val[i, col] = values
    return nm, sh, val


@functools.lru_cache(maxsize=None)
def _cluster_sweep(op, seed):
    g = np.random.default_rng(BASE[op] + seed)
    periodic = seed in CLUSTER_PERIODIC_SEEDS
    while True:
        sizes = [int(v) for v in g.choice(CLUSTER_SIZES, 3 if seed in EMPTY_SYSTEM_SEEDS else int(g.integers(2 if seed in INTERLEAVED_SEEDS else 1, 5)))]
        if seed in EMPTY_SYSTEM_SEEDS:
            sizes[1] = 0
        if max(sizes) >= 9 and sum(sizes) <= 320:
            break
    sizes = tuple(sizes)
    cutoff = float(g.uniform(4.0, 5.0))
    pos, cells, images = [], [], []
    for n in sizes:
        box = _BOX.get(n, 4.5)
        cell = charge_cell(box, True)
        pos.append(spaced_positions(g, n, cell, CLUSTER_D_MIN))
        cells.append(cell)
        images.append(2 if box < cutoff else 1)
    ntot = sum(sizes)
    bi = np.concatenate([np.full(n, k, np.int32) for k, n in enumerate(sizes)])
    zero = seed in ZERO_MULTIPOLE_SEEDS
    names = CLUSTER_FLAGS[op]
    if seed in SINGLE_FLAG_SEEDS:  # the periodic one of these seeds (0) asks for the virial alone; a cluster that would be asked for it gives the forces
        alone = names[(SINGLE_FLAG_SEEDS.index(seed) - 1) % len(names)]
        alone = names[0] if alone == "compute_virial" and not periodic else alone
        flags = {k: k == alone for k in names}
    else:
        flags = {k: bool(g.integers(2)) for k in names}
    c = dict(op=op, seed=seed, dtype="float64" if seed % 2 == 0 else "float32", sizes=sizes, periodic=periodic, pos=np.concatenate(pos),
             cells=np.stack(cells) if periodic else None, batch_idx=bi, cutoff=cutoff if periodic else 1e9, images=tuple(images), q=g.normal(size=ntot) + 0.05,
             mu=_dipoles(g, ntot, zero=zero and op == "coulomb_dipole"), qd=_quadrupoles(g, ntot, zero=zero and op == "coulomb_quadrupole"), zero=zero,
             flags=flags, autograd=bool(g.integers(2)), weights=g.uniform(0.2, 1.8, ntot), perm=g.permutation(ntot) if seed in INTERLEAVED_SEEDS else None,
             empty_system=1 if seed in EMPTY_SYSTEM_SEEDS else None, emptied_row=None, minimum_image=False, coincident=None, no_dipoles=False,
             no_quadrupoles=False, scale_dtype="float64")
    if not periodic:
        c["flags"]["compute_virial"] = False  # a cluster has no virial
    if op == "pair_scale" and seed == PS_COINCIDENT_SEED:
        big = int(np.argmax(sizes))
        a = int(np.sum(sizes[:big]))
        c["pos"][a + 1] = c["pos"][a]
        c["coincident"] = (a, a + 1)
    _with_entries(c)
    if op == "pair_scale":
        i, j, S = c["entries"]
        if c["coincident"] is not None:  # the brute-force list leaves r = 0 out: the coincident pair is listed both ways by hand
            a, b = c["coincident"]
            i, j, S = np.append(i, [a, b]), np.append(j, [b, a]), np.vstack([S, np.zeros((2, 3), S.dtype)])
            order = np.lexsort((j, i))
            c["entries"] = (i[order], j[order], S[order])
        if seed in PS_MIN_IMAGE_SEEDS:
            keep = (np.abs(fractional_pair_vectors(c)) <= PS_IMAGE_MARGIN).all(axis=1)
            c["entries"] = tuple(e[keep] for e in c["entries"])
            c["minimum_image"] = True
        i, j, S = c["entries"]
        c["scales"] = np.ones(len(i)) if zero else hash_scale(i.astype(np.int64), j.astype(np.int64))
        c["scale_dtype"] = "float32" if seed in PS_F32_SCALE_SEEDS else "float64"
        c["no_dipoles"], c["no_quadrupoles"] = seed == PS_NO_DIPOLE_SEED, seed == PS_NO_QUADRUPOLE_SEED
    return c


def cluster_interleaved(c):
    """`interleaved(c)` with the quadrupoles in the new atom order and the scales in the new entry order too."""
    perm = c["perm"]
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    i, j, S = c["entries"]
    ni, nj = inv[i], inv[j]
    order = np.argsort(ni, kind="stable")
    out = dict(c, perm=None, entries=(ni[order], nj[order], S[order]))
    for k in ("pos", "q", "mu", "qd", "batch_idx", "weights"):
        out[k] = c[k][perm]
    if "scales" in c:
        out["scales"] = c["scales"][order]
    return out


@functools.lru_cache(maxsize=None)
def pair_scale_ladder():
    """255, 256, 257 and 1 atoms per system in one batch under `minimum_image`, rows of 0 - 9 entries: the group-of-8 kernel gives a wave 8
    rows, so system boundaries fall inside waves and inside blocks.  Atoms on a jittered grid of spacing 2 in cubic-ish triclinic cells of
    16; row r of a system names its (r mod 10) nearest atoms under the minimum image and is named by them: a full list whose rows hold 0 - 9
    entries before the mirror entries are added (the CPU suite asserts that empty rows and rows of 9 and more both occur)."""
    g = np.random.default_rng(BASE["pair_scale"] + 100)
    pos, cells, pairs, off = [], [], set(), 0
    for n in PS_LADDER:
        cell = charge_cell(16.0, True)
        grid = np.stack(np.meshgrid(*[np.arange(7)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n] * 2.0 + 1.0
        frac = (grid + g.uniform(-0.3, 0.3, grid.shape)) / 16.0
        pos.append(frac @ cell)
        cells.append(cell)
        d = frac[None, :, :] - frac[:, None, :]
        dist = np.linalg.norm((d - np.rint(d)) @ cell, axis=-1) + np.eye(n) * 1e9
        for r in range(n):  # row r names its r mod 10 nearest atoms (minimum image), and is named by them
            for b in np.argsort(dist[r], kind="stable")[:min(r % 10, n - 1)]:
                pairs.add((off + r, off + int(b))); pairs.add((off + int(b), off + r))
        off += n
    keys = sorted(pairs)
    i, j = np.array([k[0] for k in keys], np.int64), np.array([k[1] for k in keys], np.int64)
    ntot = off
    c = dict(op="pair_scale", seed=None, dtype="float64", sizes=PS_LADDER, periodic=True, pos=np.concatenate(pos), cells=np.stack(cells),
             batch_idx=np.concatenate([np.full(n, k, np.int32) for k, n in enumerate(PS_LADDER)]), q=g.normal(size=ntot) + 0.05, mu=_dipoles(g, ntot),
             qd=_quadrupoles(g, ntot), entries=(i, j, np.zeros((len(i), 3), np.int64)), scales=hash_scale(i, j), minimum_image=True,
             weights=g.uniform(0.2, 1.8, ntot))
    return c


# Local frames.  A seed draws molecules of every kind (tests/local_frames_reference.py: the eight smallest molecules, so Z_THEN_X comes with
# and without a y atom and in both chiralities), rotates each at random, places them on a grid of spacing 4 with NONE atoms scattered
# between them up to the seed's total, and then PERMUTES THE ATOM ORDER at random: frame atoms lie above and below their owner and, from 257
# atoms on, in another block of 256 threads.  Forms: a cluster, one triclinic cell with wrapped positions, a batch of two or three cells,
# the batch interleaved (`FRAME_INTERLEAVED_SEEDS`) or with a system without atoms (`FRAME_EMPTY_SEEDS`).  One input None on
# `FRAME_NO_DIPOLE_SEED` / `FRAME_NO_QUADRUPOLE_SEED`.  `FRAME_SEED_OFFSET` is the first of 0, 100, ... under which all twelve seeds meet
# the conditions of the CPU suite: no case is dropped.  A molecule's rotation is drawn again while it leaves a Z_ONLY axis within 0.07 of its
# switch at 0.866 (a uniform axis does so with probability 0.14, so no offset could clear fifty such atoms at once).
FRAME_TOTALS = (1, 2, 63, 64, 65, 257, 600)
FRAME_TOTAL_BY_SEED = (257, 65, 600, 1, 64, 63, 600, 2, 257, 65, 64, 600)
FRAME_FORMS = ("cluster", "cell", "batch")
FRAME_INTERLEAVED_SEEDS = (2, 8)
FRAME_EMPTY_SEEDS = (5, 11)
FRAME_NO_DIPOLE_SEED, FRAME_NO_QUADRUPOLE_SEED = 4, 9
FRAME_MOLECULES = ("z_only", "z_only_y", "water", "ammonia", "z_bisect", "chiral", "mirror")
FRAME_SEED_OFFSET = 0
FRAME_SWITCH_MARGIN = 0.06


@functools.lru_cache(maxsize=None)
def _frame_sweep(seed):
    from tests import local_frames_reference as LR

    gen = torch.Generator().manual_seed(BASE["frames"] + FRAME_SEED_OFFSET + seed)
    g = np.random.default_rng(BASE["frames"] + FRAME_SEED_OFFSET + seed)
    total = FRAME_TOTAL_BY_SEED[seed]
    form = "batch" if seed in FRAME_INTERLEAVED_SEEDS + FRAME_EMPTY_SEEDS else FRAME_FORMS[seed % 3]
    if total < 9:
        form = "cluster" if seed % 2 else "cell"
    nsys = 1 if form != "batch" else 3
    sizes = [total] if nsys == 1 else [total - 2 * (total // 3), total // 3, total // 3]
    if seed in FRAME_EMPTY_SEEDS:
        sizes = [sizes[0] + sizes[1], 0, sizes[2]]
    parts, sys_of, cells = [], [], []
    for s, n in enumerate(sizes):
        side, used, m = 14.0, 0, 0
        mols = []
        while True:  # molecules of every kind in turn, starting at a seeded one, while they fit
            p, a, k = LR.molecule(FRAME_MOLECULES[(m + seed + s) % len(FRAME_MOLECULES)])
            if used + p.shape[0] > n:
                break
            centre = torch.tensor([m % 3, (m // 3) % 3, (m // 9) % 3], dtype=torch.float64) * 4.0 + torch.rand(3, dtype=torch.float64, generator=gen)
            while True:  # a rotation is drawn again while it leaves a Z_ONLY axis within `FRAME_SWITCH_MARGIN` of the 0.866 switch (as `spaced_positions` rejects)
                rot = (p - p.mean(0)) @ LR.random_rotation(gen).T
                z = torch.nonzero(k == LR.Z_ONLY).reshape(-1)
                ez = rot[a[z, 0].long()] - rot[z]
                if z.numel() == 0 or float(((ez[:, 0] / ez.norm(dim=1)).abs() - LR.Z_ONLY_SWITCH).abs().min()) > FRAME_SWITCH_MARGIN + 0.01:
                    break
            mols.append((rot + centre + 27.0 * (m // 27), a, k))
            used += p.shape[0]
            m += 1
            if m >= 150:
                break
        for _ in range(n - used):  # NONE atoms scattered between the molecules
            mols.append((torch.rand((1, 3), dtype=torch.float64, generator=gen) * 12.0, torch.full((1, 3), -1, dtype=torch.int32),
                         torch.zeros(1, dtype=torch.int32)))
        parts += mols
        sys_of += [s] * n
        cells.append(torch.tensor(charge_cell(side + s, True)).float().double())
    if parts:
        pos, atoms, kinds, _ = LR.join(parts)
    sys_of = torch.tensor(sys_of, dtype=torch.int64)
    cells = torch.stack(cells)
    if form != "cluster":  # wrapped positions: molecules straddle faces
        frac = torch.einsum("na,nab->nb", pos, torch.linalg.inv(cells)[sys_of])
        pos = torch.einsum("na,nab->nb", frac - torch.floor(frac), cells[sys_of])
    pos = pos.float().double()  # float32 numbers, like the cells, the local multipoles and the weights below: wrapped coordinates reach 16, where
    # one float32 rounding of a position is 5e-7 of a bond; with inputs that ARE float32 numbers the float32 calls see the float64 calls' geometry
    n = pos.shape[0]
    # the random atom order: within each system unless the seed interleaves the batch
    if seed in FRAME_INTERLEAVED_SEEDS:
        perm = torch.as_tensor(g.permutation(n))
    else:
        perm = torch.cat([torch.nonzero(sys_of == s).reshape(-1)[torch.as_tensor(g.permutation(k), dtype=torch.int64)] for s, k in enumerate(sizes)]) if n else torch.zeros(0, dtype=torch.int64)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(n)
    atoms = torch.where(atoms >= 0, inv[atoms.long().clamp(min=0)].to(torch.int32), atoms)[perm]
    pos, kinds, sys_of = pos[perm], kinds[perm], sys_of[perm]
    mu, quad = (t.float().double() for t in LR.local_multipoles(n, BASE["frames"] + 50 + seed))
    return dict(seed=seed, dtype="float64" if seed % 2 == 0 else "float32", form=form, n=n, sizes=tuple(sizes), pos=pos, atoms=atoms.contiguous(), kinds=kinds,
                cells=None if form == "cluster" else (cells if form == "batch" else cells[0]), batch_idx=sys_of.to(torch.int32) if form == "batch" else None,
                mu=None if seed == FRAME_NO_DIPOLE_SEED else mu, quad=None if seed == FRAME_NO_QUADRUPOLE_SEED else quad,
                w_mu=torch.randn((n, 3), dtype=torch.float64, generator=gen).float().double(),
                w_q=torch.randn((n, 3, 3), dtype=torch.float64, generator=gen).float().double(), empty_system=1 if seed in FRAME_EMPTY_SEEDS else None)


def cluster_case(kind, key=None):
    if kind == "sweep":
        return _cluster_sweep(*key)
    if kind == "ps_ladder":
        return pair_scale_ladder()
    if kind == "frames":
        return _frame_sweep(key)
    raise KeyError(kind)
