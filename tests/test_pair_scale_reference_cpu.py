"""The yardstick of `pair_scale_correction` (tests/pair_scale_reference.py) against the yardsticks that exist: per scale class it is
(s - 1) times the bare charge pair sum plus the cluster dipole and quadrupole references on the class's sub-list; an excluded dimer cancels
its unscaled cluster energy; s = 1 gives exact zeros; the minimum-image mode equals explicit shifts, wrapped or not; the virial is the pair
sum -1/2 sum (dU/dR)_a R_b."""
import numpy as np
import pytest
import torch

from tests import cluster_multipole_reference as CR
from tests import pair_scale_cases as PC
from tests import pair_scale_reference as PR

F64 = torch.float64
NAMES = ("energies", "forces", "charge_grads", "dipole_grads", "quadrupole_grads", "virial")


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=F64)


def _close(got, ref, what, rel=1e-12):
    scale = max(np.abs(ref).max(), 1e-30)
    err = np.abs(got - ref).max()
    print(f"{what:48s} rel err {err / scale:.2e}")
    assert err <= rel * scale, f"{what}: {err:.3e} > {rel * scale:.3e}"


def _charge_evaluate(pos, q, entries, cell, weights=None):
    """The bare charge pair sum E_i = 1/2 sum_row q_i q_j / r over stored entries, with its derivatives and strain virial (autograd)."""
    i, j, S = entries
    pos, q = pos.clone().requires_grad_(True), q.clone().requires_grad_(True)

    def energies(p, c):
        r = torch.linalg.norm(p[j] - p[i] + S.to(F64) @ c, dim=-1)
        return torch.zeros(p.shape[0], dtype=F64).index_add(0, i, 0.5 * q[i] * q[j] / r)

    e = energies(pos, cell)
    gp, gq = torch.autograd.grad(e.sum() if weights is None else (e * weights).sum(), [pos, q])
    eps = torch.zeros((3, 3), dtype=F64, requires_grad=True)
    defo = torch.eye(3, dtype=F64) + eps
    vir = -torch.autograd.grad(energies(pos.detach() @ defo.T, cell @ defo.T).sum(), eps)[0]
    z = np.zeros
    n = pos.shape[0]
    return dict(energies=e.detach().numpy(), forces=-gp.numpy(), charge_grads=gq.numpy(), dipole_grads=z((n, 3)), quadrupole_grads=z((n, 3, 3)),
                virial=vir.numpy()[None])


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_three_scale_classes_are_the_scaled_sums_of_the_existing_yardsticks(weighted):
    p = PC.periodic()
    pos, q, mu, Q, cell = (_t(p[k]) for k in ("pos", "q", "mu", "Q", "cell"))
    w = _t(p["w"]) if weighted else None
    s = p["scales"]
    assert sorted(set(s.tolist())) == list(PC.CLASSES)
    got = PR.evaluate(pos, q, mu, Q, _t(s), p["entries"], cell=cell, weights=w)
    want = {k: 0.0 for k in NAMES}
    for c in PC.CLASSES:
        sel = torch.as_tensor(s == c)
        sub = tuple(e[sel] for e in p["entries"])
        parts = (_charge_evaluate(pos, q, sub, cell[0], w), CR.dipole_evaluate(pos, q, mu, sub, cell=cell, weights=w),
                 CR.quadrupole_evaluate(pos, q, mu, Q, sub, cell=cell, weights=w))
        for k in NAMES:
            want[k] = want[k] + (c - 1.0) * sum(part.get(k, 0.0) for part in parts)
    for k in NAMES:
        _close(got[k], want[k], k)
    vir = got["virial"][0]
    assert np.abs(vir - vir.T).max() > 1e-3 * np.abs(vir).max(), "nine independent components"


def test_an_excluded_dimer_cancels_its_unscaled_cluster_energy():
    g = np.random.default_rng(3)
    pos = _t(np.array([[0.0, 0.0, 0.0], [1.1, 0.9, -0.6]]))
    q, mu, Q = _t(g.normal(size=2)), _t(g.normal(size=(2, 3))), _t(g.normal(size=(2, 3, 3)))
    ent = CR.all_pairs((2,))
    i, j, _ = ent
    charge = torch.zeros(2, dtype=F64).index_add(0, i, 0.5 * q[i] * q[j] / torch.linalg.norm(pos[j] - pos[i], dim=-1))
    unscaled = charge + CR.dipole_energies(pos, q, mu, ent) + CR.quadrupole_energies(pos, q, mu, Q, ent)
    corr = PR.pair_energies(pos, q, mu, Q, torch.zeros(2, dtype=F64), *ent)
    assert float(unscaled.detach().abs().max()) > 1e-2
    assert float((unscaled + corr).detach().abs().max()) <= 1e-12 * float(unscaled.detach().abs().max())


@pytest.mark.parametrize("kind", ["periodic", "ladder"])
def test_unit_scales_give_exact_zeros(kind):
    p = PC.periodic() if kind == "periodic" else PC.ladder(33)
    cell = None if p["cell"] is None else _t(p["cell"])
    out = PR.evaluate(*[_t(p[k]) for k in ("pos", "q", "mu", "Q")], torch.ones(p["scales"].shape[0], dtype=F64), p["entries"], cell=cell)
    assert all(not v.any() for v in out.values()) and ("virial" in out) == (cell is not None)


def test_minimum_image_equals_explicit_shifts_wrapped_or_not():
    """Molecules that straddle the faces of triclinic cells: explicit shifts on the wrapped atoms, minimum image on the wrapped atoms and
    minimum image on the whole molecules are the same sum."""
    p = PC.molecules()
    q, mu, Q, cell = (_t(p[k]) for k in ("q", "mu", "Q", "cell"))
    bi, s = torch.as_tensor(p["batch_idx"]), _t(p["scales"])
    i, j, S = p["entries"]
    assert bool((S != 0).any()) and not np.array_equal(p["pos"], p["pos_wrapped"])
    kw = dict(cell=cell, batch_idx=bi)
    shifted = PR.evaluate(_t(p["pos_wrapped"]), q, mu, Q, s, (i, j, S), **kw)
    for name, pos in (("wrapped", p["pos_wrapped"]), ("whole", p["pos"])):
        got = PR.evaluate(_t(pos), q, mu, Q, s, (i, j, torch.zeros_like(S)), minimum_image=True, **kw)
        for k in NAMES:
            _close(got[k], shifted[k], f"minimum image, {name}, {k}")
    assert np.abs(shifted["virial"]).min(axis=(1, 2)).max() > 0 and shifted["virial"].shape == (3, 3, 3)


@pytest.mark.parametrize("minimum_image", [False, True], ids=["shifts", "minimum_image"])
def test_the_virial_is_the_pair_sum_and_the_strain_derivative(minimum_image):
    """evaluate()'s virial is autograd with respect to a strain; it equals -sum_entries (dE/dR)_a R_b over the pair vectors, and a central
    difference of the strained total energy."""
    p = PC.molecules()
    q, mu, Q, cell = (_t(p[k]) for k in ("q", "mu", "Q", "cell"))
    bi, s = torch.as_tensor(p["batch_idx"]), _t(p["scales"])
    i, j, S = p["entries"]
    pos = _t(p["pos"] if minimum_image else p["pos_wrapped"])
    ent = (i, j, torch.zeros_like(S) if minimum_image else S)
    kw = dict(cell=cell, batch_idx=bi, minimum_image=minimum_image)
    vir = PR.evaluate(pos, q, mu, Q, s, ent, **kw)["virial"]
    # pair sum: E as a function of the pair vectors
    rv = PR._pair_vectors_of(pos, cell, *ent, bi.long(), minimum_image).detach().requires_grad_(True)
    e = PR.pair_energies(pos, q, mu, Q, s, *ent, _pair_vectors=rv, **kw)
    g = torch.autograd.grad(e.sum(), rv)[0]
    pair = torch.zeros((3, 3, 3), dtype=F64).index_add(0, bi.long()[i], -g[:, :, None] * rv.detach()[:, None, :])
    _close(pair.numpy(), vir, "pair-sum virial")
    # central difference of one strain component per system
    h = 1e-6
    for a, b in ((0, 1), (2, 0), (1, 1)):
        d = torch.zeros((3, 3), dtype=F64)
        d[a, b] = h
        tot = []
        for sign in (1.0, -1.0):
            defo = torch.eye(3, dtype=F64) + sign * d
            e = PR.pair_energies(pos @ defo.T, q, mu, Q, s, *ent, cell=cell @ defo.T, batch_idx=bi, minimum_image=minimum_image)
            tot.append(torch.zeros(3, dtype=F64).index_add(0, bi.long(), e))
        fd = -(tot[0] - tot[1]) / (2.0 * h)
        assert float((fd - torch.as_tensor(vir[:, a, b])).abs().max()) <= 1e-7 * float(np.abs(vir).max())
