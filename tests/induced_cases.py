"""The systems the induced-dipole tests share: a jittered m x m x m lattice in the triclinic cell of `test_dipole_gpu._system`.

Box = m a; the fractional lattice points (k + 1/2) / m are multiplied by the cell and every position is displaced by uniform(-jitter, jitter)
per component.  Charges are 0.5 normal.  d_min is the smallest minimum-image distance of the positions, and the polarisabilities are uniform
in [0.05, 0.15] d_min^3: far enough below d_min^3 that H = diag(1 / a) + T is positive definite (tests/test_induced_reference_cpu.py checks
the smallest eigenvalue of D^1/2 H D^1/2 for every case)."""
import functools

import numpy as np
import torch

from tests.gaussian_reference import brute_force_entries

CASES = {"l27": (3, 3.0, 0.5, 101), "l64": (4, 3.0, 0.5, 102), "l27dense": (3, 2.5, 0.4, 103)}  # name: (m, a, jitter, seed)
EWALD = dict(alpha=0.45, cutoff=11.0, k_cutoff=3.2)  # converged for these boxes: test_induced_reference_cpu compares with a second set


def triclinic(box):
    return np.array([[box, 0, 0], [0.2 * box, 0.9 * box, 0], [0.1 * box, -0.15 * box, 1.1 * box]])


def minimum_distance(pos, cell):
    rng = np.arange(-1, 2)
    S = np.array([(a, b, c) for a in rng for b in rng for c in rng])
    d = np.linalg.norm(pos[None, :, None, :] - pos[:, None, None, :] + (S @ cell)[None, None, :, :], axis=-1)
    return float(d[d > 1e-12].min())


@functools.lru_cache(maxsize=None)
def lattice(name):
    """dict(pos [n, 3], cell [3, 3], q [n], polar [n], d_min) as float64 numpy arrays."""
    m, a, jitter, seed = CASES[name]
    g = np.random.default_rng(seed)
    cell = triclinic(m * a)
    grid = np.array([(x, y, z) for x in range(m) for y in range(m) for z in range(m)], dtype=np.float64)
    pos = ((grid + 0.5) / m) @ cell + g.uniform(-jitter, jitter, (m**3, 3))
    q = 0.5 * g.normal(size=m**3)
    d_min = minimum_distance(pos, cell)
    polar = g.uniform(0.05, 0.15, m**3) * d_min**3
    return dict(n=m**3, pos=pos, cell=cell, q=q, polar=polar, d_min=d_min)


@functools.lru_cache(maxsize=None)
def entries(name, cutoff=EWALD["cutoff"], images=2):
    """(i, j, S) of the full list of a case: every image within `cutoff`."""
    c = lattice(name)
    return brute_force_entries(c["pos"], c["cell"], cutoff, images)


def k_vectors(cell, k_cutoff):
    from nvalchemiops.interactions.electrostatics.k_vectors import generate_k_vectors_ewald_summation

    return generate_k_vectors_ewald_summation(torch.as_tensor(cell, dtype=torch.float64).reshape(1, 3, 3), k_cutoff).reshape(-1, 3)
