"""Hand-made problems of the `pair_scale_correction` tests (numpy on the CPU, independent of the neighbour search and of
`bonded_pair_scales`), shared by tests/test_pair_scale_reference_cpu.py, tests/test_bonded_pair_scales_cpu.py and tests/test_pair_scale_gpu.py.

Every distance of a listed pair is at least `D_MIN` = 1.3, the bound of tests/cluster_multipole_reference.py, so that family's bars apply.
"""
import collections

import numpy as np
import torch

from tests.cluster_multipole_reference import D_MIN, JITTER, SPACING, jittered_grid

PLAIN = (2, 5, 9)                    # atoms that carry a charge only
CLASSES = (0.0, 0.4, 0.8)            # the three scale classes of the hand-made lists (entries with s = 1 ride along and are skipped)
LADDER_ROWS = (0, 1, 7, 8, 9, 16, 17, 25)  # entries of rows 0 ... 7 of the 70-atom ladder
AMOEBA = (0.0, 0.0, 0.4, 0.8)


def graph_scales(bonds, n, scales):
    """{(i, j): scale} of every ordered pair whose shortest bond path has d <= len(scales) bonds, by a plain breadth-first search per atom;
    pairs whose scale is exactly 1 dropped.  The independent restatement `bonded_pair_scales` is tested against."""
    adj = collections.defaultdict(set)
    for a, b in bonds:
        adj[int(a)].add(int(b)); adj[int(b)].add(int(a))
    out = {}
    for i in range(n):
        dist, frontier = {i: 0}, [i]
        for d in range(1, len(scales) + 1):
            nxt = []
            for a in frontier:
                for b in sorted(adj[a]):
                    if b not in dist:
                        dist[b] = d
                        nxt.append(b)
            frontier = nxt
        for j, d in dist.items():
            if d and scales[d - 1] != 1.0:
                out[(i, j)] = float(scales[d - 1])
    return out


def _entries(pairs):
    """(i, j, S = 0) int64 sorted by row then column, and the scales, of a {(i, j): s} dict."""
    keys = sorted(pairs)
    i = torch.as_tensor([k[0] for k in keys], dtype=torch.long)
    j = torch.as_tensor([k[1] for k in keys], dtype=torch.long)
    return (i, j, torch.zeros((len(keys), 3), dtype=torch.long)), np.array([pairs[k] for k in keys], dtype=np.float64)


def _multipoles(n, g):
    q, mu, Q = g.normal(size=n) + 0.05, 0.4 * g.normal(size=(n, 3)), 0.3 * g.normal(size=(n, 3, 3))
    plain = [a for a in PLAIN if a < n]
    mu[plain], Q[plain] = 0.0, 0.0
    return dict(q=q, mu=mu, Q=Q, w=g.normal(size=n))


def _hash_scale(i, j):
    return (0.0, 0.4, 0.8, 1.0, 0.4)[(i * j + i + j) % 5]  # symmetric in (i, j); one entry in five is an unscaled pair


def ladder(n, seed=5):
    """A cluster of `n` atoms on a jittered grid with a hand-built full list (the pairs need not be neighbours in space).
    n = 70: rows 0 ... 7 hold `LADDER_ROWS` entries (an empty row, one trip of the 8-lane group, a group exactly full, the second and third
    trips, a tail), rows 16 ... 23 -- one whole wave of the kernel -- are empty; two blocks and a last block of 6 rows.  n = 33: hubs of 17 and
    14 entries and a chain, the last block holds one row.  n = 7: all pairs (one partial wave).  n = 1: a single atom without entries."""
    g = np.random.default_rng(seed + n)
    pos = jittered_grid((5, 5, 3), SPACING, JITTER, g)[:n]
    und = set()
    if n == 70:
        fillers = list(range(8, 16)) + list(range(24, 70))
        for a, deg in enumerate(LADDER_ROWS):
            for k in range(deg):
                und.add((a, fillers[(7 * a + k) % len(fillers)]))
    elif n == 33:
        und |= {(0, k) for k in range(1, 18)} | {(k, 32) for k in range(18, 32)} | {(k, k + 1) for k in range(1, 31)}
    elif n == 7:
        und |= {(a, b) for a in range(7) for b in range(a + 1, 7)}
    elif n != 1:
        raise ValueError(n)
    pairs = {}
    for a, b in und:
        pairs[(a, b)] = pairs[(b, a)] = _hash_scale(a, b)
    entries, scales = _entries(pairs)
    counts = np.bincount(entries[0].numpy(), minlength=n)
    if n == 70:
        assert tuple(counts[:8]) == LADDER_ROWS and not counts[16:24].any() and counts[8:16].all()
    return dict(kind=f"ladder{n}", n=n, pos=pos, cell=None, batch_idx=None, nsys=1, entries=entries, scales=scales, **_multipoles(n, g))


def periodic(seed=13):
    """24 atoms on a jittered grid that fills a triclinic cell, every image pair within 3.2 listed (explicit shifts, self images absent), the
    scale class set by the distance (symmetric by construction): rows of about 9 to 14 entries."""
    g = np.random.default_rng(seed)
    pos = jittered_grid((3, 4, 2), SPACING, 0.2, g)
    cell = np.array([[6.0, 0.0, 0.0], [0.3, 8.0, 0.0], [-0.2, 0.25, 4.0]])
    shifts = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), -1).reshape(-1, 3)
    d = pos[None, :, None, :] + (shifts @ cell)[None, None, :, :] - pos[:, None, None, :]
    r = np.linalg.norm(d, axis=-1)
    i, j, s = np.nonzero((r < 3.2) & (r > 1e-6))
    assert r[i, j, s].min() >= D_MIN
    order = np.lexsort((s, j, i))
    i, j, s = i[order], j[order], s[order]
    scales = np.where(r[i, j, s] < 2.05, 0.0, np.where(r[i, j, s] < 2.7, 0.4, 0.8))
    n = pos.shape[0]
    return dict(kind="periodic", n=n, pos=pos, cell=cell[None], batch_idx=None, nsys=1,
                entries=(torch.as_tensor(i), torch.as_tensor(j), torch.as_tensor(shifts[s])), scales=scales, **_multipoles(n, g))


CHAIN9 = [(k, k + 1) for k in range(8)]
RING5 = [(k, (k + 1) % 5) for k in range(5)]
WATER = [(0, 1), (0, 2)]


def _chain(m):
    k = np.arange(m, dtype=np.float64)
    return np.stack([1.3 * k, 0.75 * (k % 2), 0.2 * k], -1)  # bonds of 1.51


def _ring(m, radius=1.3):
    a = 2.0 * np.pi * np.arange(m) / m
    return np.stack([radius * np.cos(a), radius * np.sin(a), 0.1 * np.arange(m)], -1)  # sides of 1.53 for m = 5


def _water():
    h = np.deg2rad(104.5 / 2.0)
    return np.array([[0.0, 0.0, 0.0], [1.4 * np.sin(h), 1.4 * np.cos(h), 0.0], [-1.4 * np.sin(h), 1.4 * np.cos(h), 0.0]])


def molecules(seed=17):
    """A batch of three molecules -- a 9-atom chain, a 5-ring, a water -- each in a triclinic cell of its own and each straddling a face of
    it.  `pos` are the unwrapped coordinates (molecules whole), `pos_wrapped` the same atoms wrapped into their cells, `entries` the bonded
    list (AMOEBA's 0 / 0 / 0.4 / 0.8 by shortest path, from `graph_scales`) with the shifts that join the WRAPPED atoms, `all_pairs` the
    all-pairs list of every molecule (no shifts)."""
    g = np.random.default_rng(seed)
    base = np.array([[15.0, 0.0, 0.0], [1.5, 14.0, 0.0], [-1.0, 1.2, 13.0]])
    cells = np.stack([base, 1.1 * base, 0.9 * base])
    parts = [_chain(9) + np.array([9.5, 6.0, 6.0]), _ring(5) + np.array([0.2, 15.0, 5.0]), _water() + np.array([0.9, 5.0, 6.0])]
    bonds, sizes, off = [], [], 0
    for mol, b in zip(parts, (CHAIN9, RING5, WATER)):
        bonds += [(a + off, c + off) for a, c in b]
        sizes.append(mol.shape[0]); off += mol.shape[0]
    pos = np.concatenate(parts) + g.uniform(-0.03, 0.03, (off, 3))
    bi = np.repeat(np.arange(3), sizes).astype(np.int32)
    floor = np.floor(np.einsum("na,nab->nb", pos, np.linalg.inv(cells)[bi]))
    assert len({tuple(f) for f in floor[:9]}) > 1 and len({tuple(f) for f in floor[9:14]}) > 1 and len({tuple(f) for f in floor[14:]}) > 1
    wrapped = pos - np.einsum("na,nab->nb", floor, cells[bi])
    (i, j, _), scales = _entries(graph_scales(bonds, off, AMOEBA))
    S = torch.as_tensor((floor[j.numpy()] - floor[i.numpy()]).astype(np.int64))
    assert np.linalg.norm(pos[j.numpy()] - pos[i.numpy()], axis=-1).min() >= D_MIN
    ii, jj, o = [], [], 0
    for m in sizes:
        a, b = np.nonzero(~np.eye(m, dtype=bool))
        ii.append(a + o); jj.append(b + o); o += m
    ap = (torch.as_tensor(np.concatenate(ii)), torch.as_tensor(np.concatenate(jj)), torch.zeros((sum(len(a) for a in ii), 3), dtype=torch.long))
    return dict(kind="molecules", n=off, sizes=tuple(sizes), bonds=np.array(bonds), pos=pos, pos_wrapped=wrapped, cell=cells, batch_idx=bi, nsys=3,
                entries=(i, j, S), scales=scales, all_pairs=ap, **_multipoles(off, g))
