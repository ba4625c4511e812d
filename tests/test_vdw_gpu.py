"""`buffered_14_7` / `lennard_jones` on the device against the float64 restatement of their definition (tests/vdw_reference.py, itself pinned
in tests/test_vdw_reference_cpu.py) on the same stored entries.

float64: kernel and reference share the arithmetic model, so they differ by summation order and last bits: 1e-11 of the largest |value| per
output plus 1e-14, the bar of tests/test_gaussian_charges_gpu.py for the same model.

float32: pair vector and r^2 in float32, the rest float64, against the reference's `distance_dtype=float32` mode.  The project's 1e-6 cannot
be taken over: on the repulsive wall |d ln U / d ln r| reaches 13, so one float32 ulp of r^2 moves the largest values by close to 1e-6.  Every
fixture keeps rho >= 0.8 for every site pair.  Measured on the CPU from the reference alone (every float32 r^2 moved by one ulp with
`torch.nextafter`, largest change over the fixtures below relative to the largest |value| of the output), in the order of NAMES:
    buffered_14_7   2.44e-7  1.08e-6  1.66e-6  3.14e-7  7.84e-7        lennard_jones   2.17e-7  1.17e-6  1.26e-6  2.45e-7  6.80e-7
The bar of an output is four times its figure (FMA contraction in the three-term sum of squares, summation order): 9.8e-7, 4.3e-6, 6.6e-6,
1.3e-6, 3.1e-6 for the 14-7 and 8.7e-7, 4.7e-6, 5.0e-6, 9.8e-7, 2.7e-6 for Lennard-Jones."""
import functools

import numpy as np
import pytest
import torch

from nvalchemiops.interactions import ReducedSites, buffered_14_7, lennard_jones
from tests import vdw_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
NAMES = ("energies", "forces", "radius_grads", "epsilon_grads", "virial")
F32_FIGURE = {"buffered_14_7": (2.44e-7, 1.08e-6, 1.66e-6, 3.14e-7, 7.84e-7), "lennard_jones": (2.17e-7, 1.17e-6, 1.26e-6, 2.45e-7, 6.80e-7)}
# cluster atoms sit on a jittered 6 x 5 x 5 grid in index order, so grid neighbours are index neighbours.  (child, parent): a methane-like
# group around 37, water-like groups with the parent above (50) and below (8) its children
GROUPS = ((31, 37), (36, 37), (38, 37), (43, 37), (44, 50), (49, 50), (9, 8), (14, 8))
FN = dict(buffered_14_7=buffered_14_7, lennard_jones=lennard_jones)


def _close(got, ref, what, rel):
    got, ref = got.detach().to(F64), ref.detach().to(F64)
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    print(f"{what}: max err {err:.3e} of {scale:.3e}")
    assert err <= rel * scale + 1e-14, f"{what}: max err {err:.3e} > {rel * scale + 1e-14:.3e}"


def _sym_scales(n):
    g = np.random.default_rng(n)
    s = g.uniform(0, 1, (n, n)) * (g.uniform(0, 1, (n, n)) > 0.15)
    return np.triu(s) + np.triu(s, 1).T


def _sites(n, pairs, g, lo, hi):
    parent = np.where(np.arange(n) % 2 == 0, -1, np.arange(n))  # "none" both ways: -1 and the atom's own index
    for c, p in pairs:
        parent[c] = p
    return parent, g.uniform(lo, hi, n)


@functools.lru_cache(maxsize=None)
def cluster(n, isolated=False):
    """All-pairs cluster of n atoms: rows of n - 1 entries, as a matrix with three padding columns (one out of range) and as CSR.  n >= 66: reduced
    sites (GROUPS, and the last atom a child of the one before).  `isolated`: atom 7 is in no row and has an empty one, atom 5 has eps = 0."""
    g = np.random.default_rng(100 + n)
    k = np.arange(n)
    pos = 3.6 * np.stack([k % 6, (k // 6) % 5, k // 30], 1) + g.uniform(-0.2, 0.2, (n, 3))
    radii, eps = g.uniform(2.8, 3.6, n), g.uniform(0.05, 0.3, n)
    sites = _sites(n, GROUPS + ((n - 1, n - 2),), g, 0.8, 0.95) if n >= 66 else None
    member = np.ones(n, bool)
    if isolated:
        member[7], eps[5] = False, 0.0
    rows = [[j for j in range(n) if j != i and member[j]] if member[i] else [] for i in range(n)]
    width = n - 1 + 3
    nm = np.full((n, width), -1)
    for i, row in enumerate(rows):
        cols = np.delete(np.arange(width), [0, width // 2, width - 1])[:len(row)]
        nm[i, cols] = row
    nm[:, width // 2] = n + 5
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    jj = np.concatenate([np.array(r, int) for r in rows])
    ii = np.repeat(np.arange(n), np.diff(ptr))
    sym = _sym_scales(n)
    return dict(n=n, pos=pos, radii=radii, eps=eps, cell=None, bi=None, sites=sites, nm=nm, sh=None, nl=np.stack([ii, jj]), ptr=ptr, lsh=None,
                ms=sym[np.arange(n)[:, None], np.clip(nm, 0, n - 1)], ls=sym[ii, jj], cutoff=9.0, taper=7.5)


def _box(seed):
    """60 atoms on a jittered 4 x 4 x 4 fractional grid of a triclinic 9 A box, wrapped; groups bonded across the cell faces."""
    g = np.random.default_rng(seed)
    cell = np.array([[9.0, 0, 0], [1.8, 8.1, 0], [0.9, -1.35, 9.9]])
    k = np.arange(60)
    frac = (np.stack([k % 4, (k // 4) % 4, k // 16], 1) + 0.5 + g.uniform(-0.08, 0.08, (60, 3))) / 4.0
    pairs = ((3, 0), (1, 0), (7, 4), (5, 4), (15, 12), (13, 12), (28, 12), (59, 58))  # 3-0, 7-4 and 15-12 are bonded through the x face
    return frac @ cell, cell, g.uniform(1.7, 2.2, 60), g.uniform(0.05, 0.3, 60), _sites(60, pairs, g, 0.9, 0.95)


@functools.lru_cache(maxsize=None)
def periodic(batched=False, moved=False):
    """One triclinic box, or a batch of two, with the library's own neighbour list at 4.5 A; cutoff 4.0 and taper 3.6 lie inside it.  `moved`:
    the same system with child 3 brought next to its parent through the x face, and child 13 and parent 12 (of 15, 13, 28) each sent one
    lattice vector away, every shift of the list rebuilt for the new images: S' = S + n_i - n_j."""
    from nvalchemiops.neighborlist import neighbor_list

    boxes = [_box(11), _box(12)] if batched else [_box(11)]
    nb, n = len(boxes), 60 * len(boxes)
    pos, radii, eps = (np.concatenate([b[k] for b in boxes]) for k in (0, 2, 3))
    parent = np.concatenate([np.where(b[4][0] >= 0, b[4][0] + 60 * s, -1) for s, b in enumerate(boxes)])
    sym = _sym_scales(n)
    cells = torch.as_tensor(np.stack([b[1] for b in boxes]), device=DEV)
    bi = torch.arange(nb, device=DEV, dtype=torch.int32).repeat_interleave(60) if batched else None
    kw = dict(batch_idx=bi, batch_ptr=torch.arange(nb + 1, device=DEV, dtype=torch.int32) * 60, method="batch_cell_list") if batched else dict(method="cell_list")
    kw.update(cell=cells, pbc=torch.ones((nb, 3), dtype=torch.bool, device=DEV), max_neighbors=64)
    P = torch.as_tensor(pos, device=DEV)
    nm, num, sh = neighbor_list(P, 4.5, **kw)
    nl, ptr, lsh = neighbor_list(P, 4.5, return_neighbor_list=True, **kw)
    assert 0 < int(num.max()) <= 64
    nm_h, nl_h = nm.cpu().numpy(), nl.cpu().numpy()
    if moved:
        img = np.zeros((n, 3), int)
        img[[3, 13, 12]] = ((-1, 0, 0), (0, 1, 0), (0, 0, -1))
        pos = pos + img @ boxes[0][1]
        sh = sh + _t(img[:, None, :] - img[np.clip(nm_h, 0, n - 1)]).int()
        lsh = lsh + _t(img[nl_h[0]] - img[nl_h[1]]).int()
    return dict(n=n, pos=pos, radii=radii, eps=eps, cell=cells, bi=bi, sites=(parent, np.concatenate([b[4][1] for b in boxes])), nm=nm_h, sh=sh,
                nl=nl_h, ptr=ptr, lsh=lsh, ms=sym[np.arange(n)[:, None], np.clip(nm_h, 0, n - 1)], ls=sym[nl_h[0], nl_h[1]], cutoff=4.0, taper=3.6,
                mask=n)


def _t(a, dtype=None):
    t = None if a is None else torch.as_tensor(a, device=DEV)
    return t if t is None or dtype is None else t.to(dtype)


def _compare(f, kind, dtype, fmt, scaled, what, **extra):
    """Every output of fixture f (five with a cell, four without) against the reference at the bar of its dtype; returns the kernel's."""
    pos, radii, eps = (_t(f[k], dtype) for k in ("pos", "radii", "eps"))
    cell = None if f["cell"] is None else f["cell"].to(dtype)
    mask = f.get("mask", -1)
    sites = None if f["sites"] is None else ReducedSites(_t(f["sites"][0]), _t(f["sites"][1], dtype), batch_idx=f["bi"])
    if fmt == "matrix":
        lists = dict(neighbor_matrix=_t(f["nm"]), neighbor_matrix_shifts=f["sh"], mask_value=mask)
        scales = _t(f["ms"], dtype) if scaled else None
        entries = R.entries_from_matrix(lists["neighbor_matrix"], f["sh"], mask, scales)
    else:
        lists = dict(neighbor_list=_t(f["nl"]), neighbor_ptr=_t(f["ptr"]), neighbor_shifts=f["lsh"])
        scales = _t(f["ls"], F64) if scaled else None  # (float64 scales beside float32 positions)
        i, j = lists["neighbor_list"].long()
        entries = (i, j, torch.zeros((len(i), 3), dtype=torch.long, device=DEV) if f["lsh"] is None else f["lsh"].long(), scales)
    model = dict(cutoff=f["cutoff"], taper=f["taper"])
    got = FN[kind](pos, radii, eps, cell, sites=sites, pair_scales=scales, batch_idx=f["bi"], compute_forces=True, compute_radius_gradients=True,
                    compute_epsilon_gradients=True, compute_virial=cell is not None, **lists, **model, **extra)
    rules = dict(radius_rule="cubic-mean", epsilon_rule="hhg") if kind == "buffered_14_7" else dict(radius_rule="arithmetic", epsilon_rule="geometric")
    ref = R.evaluate(kind, pos, radii, eps, cell, *entries, batch_idx=f["bi"], distance_dtype=dtype, **{**rules, **extra},
                     sites=None if f["sites"] is None else (_t(f["sites"][0]), _t(f["sites"][1], dtype)), **model)
    for name, o, figure in zip(NAMES, got, F32_FIGURE[kind]):
        assert o.dtype == dtype
        _close(o, ref[name], f"{what} {kind} {fmt} {name}", 1e-11 if dtype == F64 else 4 * figure)
    return got


@pytest.mark.parametrize("fmt", ["matrix", "csr"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_parity_across_the_wave_stride_and_in_periodic_boxes(kind, dtype, fmt):
    for n in (2, 64, 65, 66, 130):  # rows of 1, 63, 64, 65 and 129 entries; reduced sites from 66 on
        for scaled in (False, True):
            got = _compare(cluster(n), kind, dtype, fmt, scaled, f"N={n} scaled={scaled}")
    again = _compare(cluster(130), kind, dtype, fmt, True, "again")
    assert all(torch.equal(a, b) for a, b in zip(got, again)), "two identical calls differ"
    for o in _compare(cluster(20, isolated=True), kind, dtype, fmt, False, "isolated"):  # an empty row (atom 7, in no row either) and an
        assert float(o[[5, 7]].abs().max()) == 0.0                                        # atom without a site (5): exact zeros
    for batched in (False, True):
        for scaled in (False, True):
            got = _compare(periodic(batched), kind, dtype, fmt, scaled, f"batched={batched} scaled={scaled}")
        assert got[4].shape == (2 if batched else 1, 3, 3)
    # other images of the same atoms, list shifts rebuilt: against the reference, and in float64 (where moving an atom by a lattice vector
    # does not move its rounded coordinates by more than the bar) every output as before: the site stays at its atom's image
    for batched in (False, True):
        moved = _compare(periodic(batched, moved=True), kind, dtype, fmt, True, "moved")
        if dtype == F64:
            for name, o, want in zip(NAMES, moved, _compare(periodic(batched), kind, dtype, fmt, True, "as stored")):
                _close(o, want, f"moved images {name}", 1e-11)
    _compare(periodic(), kind, dtype, fmt, False, "other rules", radius_rule="geometric", epsilon_rule="geometric" if kind == "buffered_14_7" else "hhg")


@pytest.mark.parametrize("kind", R.KINDS)
def test_autograd_and_compile_match_the_explicit_outputs(kind):
    f = periodic(True)
    sites = ReducedSites(_t(f["sites"][0]), _t(f["sites"][1]), batch_idx=f["bi"])
    kw = dict(cutoff=4.0, taper=3.6, sites=sites, pair_scales=_t(f["ms"]), batch_idx=f["bi"], neighbor_matrix=_t(f["nm"]), neighbor_matrix_shifts=f["sh"],
              mask_value=f["mask"])
    x = [_t(f[k]).requires_grad_(True) for k in ("pos", "radii", "eps")]
    e, frc, rg, eg = FN[kind](*(t.detach() for t in x), f["cell"], compute_forces=True, compute_radius_gradients=True, compute_epsilon_gradients=True, **kw)
    loss = lambda p, r, q: FN[kind](p, r, q, f["cell"], **kw).sum()  # noqa: E731
    for run in (loss, torch.compile(loss, mode="default", fullgraph=True)):
        for t in x:
            t.grad = None
        run(*x).backward()
        for name, got, want in zip(NAMES[1:], (-x[0].grad, x[1].grad, x[2].grad), (frc, rg, eg)):
            _close(got, want, f"autograd {name}", 1e-11)
    with pytest.raises(NotImplementedError, match="second derivatives"):
        FN[kind](*x, f["cell"], compute_forces=True, **kw)[1].sum().backward()
