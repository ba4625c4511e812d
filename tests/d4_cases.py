"""The systems tests/test_d4_gpu.py compares against the restatement tests/d4_reference.py, in one place, so that the CPU suite can check
the condition the tables must meet on exactly these systems (tests/test_d4_reference_cpu.py) and so that every reference is computed once.

    case(name) -> dict(pos, z, q, tables, cell, batch_idx, rc (list cutoff), kw (model arguments of `dftd4` / `reference`))
    references(name) -> (float64 restatement, the same with float32 per-pair / per-atom arithmetic); cached, never modified
"""
import functools

import numpy as np
import torch

from tests import atm_reference as A
from tests import d4_reference as R
from tests import systems as S

BJ = dict(a1=0.4, a2=4.0, s8=0.8)
SPECIES = (1, 6, 8, 17)  # includes the one-reference and the seven-reference element of `d4_test_tables`


def _zs(n, seed, choices=SPECIES):
    return np.random.default_rng(seed).choice(np.array(choices, np.int32), n)


def _qs(n, seed, scale=0.3):
    return np.random.default_rng(seed + 77).uniform(-scale, scale, n).astype(np.float32)


def _molecule(n, seed, rc=14.0, density=0.02, **kw):
    pos, _, _ = S.molecule(n, density=density, min_dist=2.0, seed=seed)
    return dict(pos=pos, z=_zs(n, seed), q=_qs(n, seed), tables=R.d4_test_tables(17), cell=None, batch_idx=None, rc=rc, kw=dict(kw))


def _species_case(count):
    """40 atoms, `count` distinct species (Z = 1 ... count), tables up to Z = 24."""
    c = _molecule(40, 23, rc=13.0, density=0.03)
    c["z"] = (np.arange(40) % count + 1).astype(np.int32)
    c["tables"] = R.d4_test_tables(24, seed=5)
    return c


def _box(shape, seed, rc, dtype=np.float32, a=4.2, **kw):
    pos, cell = A.lattice_box(shape, a=a, seed=seed, triclinic=True, dtype=dtype)
    n = len(pos)
    return dict(pos=pos, z=_zs(n, seed), q=_qs(n, seed), tables=R.d4_test_tables(17), cell=cell, batch_idx=None, rc=rc, kw=dict(kw))


def _padding():
    c = _molecule(12, 8)
    c["z"][4] = 0                    # padding inside the molecule
    c["z"][7] = 18                   # Z >= nz: outside the tables
    return c


def _no_references():
    c = _molecule(12, 9)
    t = c["tables"]
    t["n_ref"][8] = 0                # oxygen becomes an element without references: its atoms are padding
    R.blank_unused(t)
    c["z"][:3] = 8
    return c


def _zeff_negative():
    c = _molecule(9, 10)
    c["z"][2] = 1
    c["q"][2] = -1.5                 # zeff[1] = 1: zeff + q <= 0, the constant branch of zeta
    return c


def _batch():
    boxes = [A.lattice_box((3, 3, 2), seed=1, triclinic=True), A.lattice_box((2, 2, 2), a=4.6, seed=2, triclinic=False)]
    one = (np.array([[1.0, 2.0, 3.0]], np.float32), (np.eye(3) * 9.0).astype(np.float32))
    boxes.append(one)
    pos = np.concatenate([b[0] for b in boxes])
    cell = np.stack([b[1] for b in boxes])
    bi = np.concatenate([np.full(len(b[0]), k, np.int32) for k, b in enumerate(boxes)])
    n = len(pos)
    return dict(pos=pos, z=_zs(n, 5), q=_qs(n, 5), tables=R.d4_test_tables(17), cell=cell, batch_idx=bi, rc=7.0, kw={})


def _d3_limit():
    """One reference per element and ga = 0: C6_ij = c6_ref[Z_i, Z_j, 0, 0], the energy is `dftd3`'s with constant c6ab tables."""
    c = _box((3, 3, 2), 7, 9.0, ga=0.0)
    t = c["tables"]
    t["n_ref"][1:] = 1
    R.blank_unused(t)
    return c


_BUILDERS = {
    "molecule1": lambda: _molecule(1, 1),
    "molecule2": lambda: _molecule(2, 2),
    "molecule3": lambda: _molecule(3, 1),
    "molecule7": lambda: _molecule(7, 2),
    "molecule24": lambda: _molecule(24, 3),
    "molecule70": lambda: _molecule(70, 4, rc=40.0),          # every row holds the 69 other atoms: a second lane trip
    "padding": _padding,
    "no_references": _no_references,
    "species_slots": lambda: _species_case(16),
    "species_slots_plus_1": lambda: _species_case(17),
    "species_20": lambda: _species_case(20),
    "triclinic_f32": lambda: _box((3, 3, 2), 7, 9.0),
    "triclinic_f64": lambda: _box((3, 3, 2), 7, 9.0, dtype=np.float64),
    "self_images": lambda: _box((2, 1, 1), 9, 9.0),          # the cell is shorter than the cutoff: rows hold the atom's own images
    "batch": _batch,
    "zero_charges": lambda: dict(_molecule(24, 3), q=np.zeros(24, np.float32)),
    "zeff_negative": _zeff_negative,
    # 4.3: inside the shell of nearest neighbours (lattice spacing 4.2, jitter 0.25), whose counting terms are the ones float32 resolves
    "cn_cutoff": lambda: _box((3, 3, 2), 11, 9.0, cn_cutoff=4.3),
    "d3_limit": _d3_limit,
}
NAMES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def references(name):
    c = case(name)
    kw = dict(cell=c["cell"], batch_idx=c["batch_idx"], **BJ, **c["kw"])
    r64 = R.reference(c["pos"], c["z"], c["q"], c["tables"], list_cutoff=c["rc"], **kw)
    r32 = R.reference(c["pos"], c["z"], c["q"], c["tables"], list_cutoff=c["rc"], work_dtype=torch.float32, **kw)
    return r64, r32
