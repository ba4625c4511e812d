"""`generalized_born` on the device against tests/born_reference.py (checked in tests/test_born_reference_cpu.py) over the same hand-built
entries.  The arithmetic model is that of the Gaussian-charge operator, so the bars are those of tests/test_gaussian_charges_gpu.py: 1e-11
(float64) and 1e-6 (float32, reference on the rounded inputs) of the largest |reference value| per output, 1e-10 for autograd and matrix against CSR."""
import itertools

import numpy as np
import pytest
import torch

from tests import born_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("energies", "forces", "charge_grads", "born_radii", "virial")
KW = dict(solute_dielectric=1.0, solvent_dielectric=78.5, coulomb_constant=332.06371, surface_tension=0.0054)


def _close(got, ref, what, rel):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, what
    err, scale = float((got - ref).abs().max()) if ref.numel() else 0.0, float(ref.abs().max()) if ref.numel() else 0.0
    print(f"{what}: rel err {err / max(scale, 1e-300):.2e}")
    assert err <= rel * scale + 1e-14, f"{what}: max err {err:.3e}, scale {scale:.3e}"


def _system(n, seed, cell=None, cutoff=None):
    """n atoms on a jittered 1.7 A grid (spheres overlap their neighbours), and the full list: all pairs, or with a cell every image
    within `cutoff` -- (i, j, S) sorted by row."""
    g = np.random.default_rng(seed)
    side = int(np.ceil(n ** (1 / 3)))
    grid = np.array(list(itertools.product(range(side), repeat=3)))[g.permutation(side**3)[:n]]
    pos = 1.7 * grid + g.uniform(-0.3, 0.3, (n, 3))
    images = [(0, 0, 0)] if cell is None else list(itertools.product((-1, 0, 1), repeat=3))
    ent = [(i, j, S) for i in range(n) for j in range(n) for S in images
           if (i != j or any(S)) and (cutoff is None or np.linalg.norm(pos[j] - pos[i] + np.array(S) @ cell) < cutoff)]
    i, j, S = (torch.tensor([e[k] for e in ent], dtype=torch.long).reshape(-1, *s) for k, s in ((0, ()), (1, ()), (2, (3,))))
    return dict(n=n, pos=pos, q=g.normal(size=n), rad=g.uniform(1.2, 2.0, n), scr=g.uniform(0.7, 0.9, n), i=i, j=j, S=S, cell=cell)


def _tensors(s, dtype):
    t = lambda a: torch.as_tensor(a, dtype=dtype, device=DEV)  # noqa: E731
    return t(s["pos"]), t(s["q"]), t(s["rad"]), t(s["scr"]), (None if s["cell"] is None else t(s["cell"]).reshape(-1, 3, 3))


def _list_kw(s, fmt, pad=3):
    """The entries as a padded matrix (padding = n, `pad` extra slots in front of and behind every row) or as a CSR list."""
    n, i, j, S, shifted = s["n"], s["i"], s["j"], s["S"], s["cell"] is not None
    counts = torch.bincount(i, minlength=n)
    if fmt == "csr":
        ptr = torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)]).to(DEV, torch.int32)
        kw = dict(neighbor_list=torch.stack([i, j]).to(DEV, torch.int32), neighbor_ptr=ptr)
        return dict(kw, neighbor_shifts=S.to(DEV, torch.int32)) if shifted else kw
    width = int(counts.max()) + 2 * pad if len(i) else 0
    slot = pad + torch.arange(len(i)) - torch.repeat_interleave(counts.cumsum(0) - counts, counts)
    nm, sh = torch.full((n, width), n, dtype=torch.int32), torch.zeros((n, width, 3), dtype=torch.int32)
    nm[i, slot], sh[i, slot] = j.int(), S.int()
    kw = dict(neighbor_matrix=nm.to(DEV), mask_value=n)
    return dict(kw, neighbor_matrix_shifts=sh.to(DEV)) if shifted else kw


def _check(s, dtype, batch_idx=None, obc=R.OBC2, pad=3, **over):
    """Every output through both formats against the reference; matrix against CSR; two calls, and the virial asked for alone, bit-identical."""
    from nvalchemiops.interactions.electrostatics import generalized_born

    kw = dict(KW, obc=obc, **over)
    pos, q, rad, scr, cell = _tensors(s, dtype)
    virial = cell is not None
    flags = dict(compute_forces=True, compute_charge_gradients=True, compute_born_radii=True, compute_virial=virial)
    ref = R.evaluate(pos, q, rad, scr, s["i"], s["j"], s["S"], cell, batch_idx, **kw)
    bi = None if batch_idx is None else batch_idx.to(DEV, torch.int32)
    outs = {}
    for fmt in ("matrix", "csr"):
        call = lambda **f: generalized_born(pos, q, rad, scr, cell, batch_idx=bi, **_list_kw(s, fmt, pad), **f, **kw)  # noqa: E731
        outs[fmt] = out = call(**flags)
        assert len(out) == 4 + virial and all(o.dtype == dtype for o in out) and all(torch.equal(a, b) for a, b in zip(out, call(**flags)))
        assert not virial or all(torch.equal(a, b) for a, b in zip(call(compute_virial=True), (out[0], out[4]))), "virial alone"
        for name, o in zip(NAMES, out):
            _close(o, ref[name], f"{fmt} {name}", 1e-11 if dtype == torch.float64 else 1e-6)
    for name, a, b in zip(NAMES, outs["matrix"], outs["csr"]):
        _close(a, b, f"matrix vs CSR {name}", 1e-10 if dtype == torch.float64 else 1e-6)
    return outs["matrix"], ref


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("pad", [0, 3])  # matrix rows of exactly the row length, and with padding slots in front of and behind the entries
@pytest.mark.parametrize("n", [1, 2, 64, 65, 66, 130])  # all-pairs rows of 0, 1, 63, 64, 65 and 129 entries: the trips of the lane stride
def test_cluster_rows(n, pad, dtype):
    out, _ = _check(_system(n, seed=n), dtype, pad=pad)
    assert float(out[1].double().sum(0).abs().max()) <= (1e-9 if dtype == torch.float64 else 1e-4) * max(float(out[1].abs().max()), 1e-30), "net force"


@pytest.mark.parametrize("obc, tension", [(R.OBC1, None), (R.OBC1, 0.0054), (R.OBC2, None)], ids=["obc1", "obc1_surface", "obc2_no_surface"])
def test_branches_and_options(obc, tension):
    """One geometry with every descreening branch: a small atom deep inside a large one (buried / engulfed), overlapping neighbours, a far atom."""
    s = _system(6, seed=3)
    s["pos"] = np.array([[0, 0, 0], [0.4, 0, 0], [2.6, 0, 0], [0, 1.9, 0], [0, 0, 9.0], [2.0, 2.0, 0.5]], dtype=float)
    s["rad"], s["scr"] = np.array([3.0, 0.6, 1.3, 0.9, 1.5, 1.1]), np.array([0.9, 0.8, 0.85, 0.8, 0.75, 0.7])
    rho = s["rad"] - 0.09
    r, ri, Sj = np.linalg.norm(s["pos"][s["j"]] - s["pos"][s["i"]], axis=1), rho[s["i"]], (s["scr"] * rho)[s["j"]]
    live, apart = r + Sj > ri, r >= s["rad"][s["i"]] + s["rad"][s["j"]]
    for branch in (~live, live & (ri < Sj - r), live & (np.abs(r - Sj) <= ri), live & (r - Sj > ri) & ~apart, live & (r - Sj > ri) & apart):
        assert branch.any()  # engulfed, buried, L = rho, L = |r - S| between overlapping atoms, separate atoms
    _check(s, torch.float64, obc=obc, surface_tension=tension)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_periodic_batch_with_virial(dtype):
    """Three systems, the middle one empty; every image inside 6 A (7.6 A in the last: self-images).  Against the reference, and each system alone."""
    cells = np.array([[[8.0, 0, 0], [1.0, 7.5, 0], [0.5, -0.8, 8.5]], np.eye(3) * 5.0, np.diag([7.0, 8.0, 7.5])])
    a, b = _system(40, seed=11, cell=cells[0], cutoff=6.0), _system(27, seed=12, cell=cells[2], cutoff=7.6)
    s = {k: np.concatenate([a[k], b[k]]) for k in ("pos", "q", "rad", "scr")}
    s.update(n=67, cell=cells, i=torch.cat([a["i"], b["i"] + 40]), j=torch.cat([a["j"], b["j"] + 40]), S=torch.cat([a["S"], b["S"]]))
    out, ref = _check(s, dtype, batch_idx=torch.tensor([0] * 40 + [2] * 27))
    assert out[4].shape == (3, 3, 3) and float(out[4][1].abs().max()) == 0.0
    for part, rows, k in ((a, slice(0, 40), 0), (b, slice(40, 67), 2)):  # each system alone on the device: the same rows, its own fold
        alone, _ = _check(part, dtype)
        assert all(torch.equal(x, y[rows]) for x, y in zip(alone[:4], out[:4]))
        _close(alone[4][0], out[4][k], f"virial of system {k} alone", 1e-10)


def test_flags_alone_autograd_and_compile():
    from nvalchemiops.interactions.electrostatics import generalized_born

    s = _system(66, seed=5)
    pos, q, rad, scr, _ = _tensors(s, torch.float64)
    kw = dict(KW, **_list_kw(s, "matrix"))
    e, f, cg, born = generalized_born(pos, q, rad, scr, compute_forces=True, compute_charge_gradients=True, compute_born_radii=True, **kw)
    for flag, want in (("compute_forces", f), ("compute_charge_gradients", cg), ("compute_born_radii", born)):
        e1, x = generalized_born(pos, q, rad, scr, **{flag: True}, **kw)
        assert torch.equal(e1, e) and torch.equal(x, want), flag
    assert torch.equal(generalized_born(pos, q, rad, scr, **kw), e)
    compiled = torch.compile(lambda p, c: generalized_born(p, c, rad, scr, compute_forces=True, **kw), fullgraph=True, backend="eager")
    assert all(torch.equal(a, b) for a, b in zip(compiled(pos, q), (e, f)))
    # autograd: the plain sum against the explicit outputs, a weighted sum against the reference's autograd
    w = torch.as_tensor(np.random.default_rng(9).normal(size=66), device=DEV)
    ref = R.evaluate(pos, q, rad, scr, s["i"], s["j"], weights=w, **KW)
    for weights, gpos, gq in ((None, -f, cg), (w, -ref["forces"], ref["charge_grads"])):
        p, c = pos.clone().requires_grad_(True), q.clone().requires_grad_(True)
        en = generalized_born(p, c, rad, scr, **kw)
        (en.sum() if weights is None else (weights * en).sum()).backward()
        _close(p.grad, gpos, "dL/dpositions", 1e-10)
        _close(c.grad, gq, "dL/dcharges", 1e-10)
    with pytest.raises(NotImplementedError, match="radii"):
        generalized_born(pos, q, rad.clone().requires_grad_(True), scr, **kw).sum().backward()
    with pytest.raises(ValueError, match="offset"):
        generalized_born(pos, q, rad, scr, offset=1.3, **kw)
