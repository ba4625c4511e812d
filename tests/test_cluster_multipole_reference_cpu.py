"""The yardstick of the cluster multipole sums (tests/cluster_multipole_reference.py: the operator-definition references at alpha = 0) checked
on the CPU, without the device code:

1. the closed forms for two atoms: B1 A - B2 c_i c_j with 1 / r^3 and 3 / r^5, and q (3 R.Q.R / r^5 - tr Q / r^3), to 1e-13 relative;
2. the point-charge limit: every dipole replaced by the charge pair +-|mu| / d at +-d/2 along mu, every quadrupole Q = sym(p (x) dhat) by the
   opposite dipoles +-p / d at +-d/2 dhat (each again a charge pair), plain 1 / r summed between the atoms: the difference to the multipole
   energy shrinks as d^2 (the octupole of every replacement is the first moment that differs);
3. two identical polarisable atoms at distance r in a uniform field: mu = a F / (1 - 2 a / r^3) along the axis, a F / (1 + a / r^3) across
   it, and the dense H is not positive definite for a > r^3 / 2.
"""
import numpy as np
import torch

from tests import cluster_multipole_reference as CR
from tests import induced_reference as IR

F64 = torch.float64


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=F64)


def test_closed_forms_for_two_atoms():
    g = np.random.default_rng(3)
    pos = np.array([[0.3, -0.2, 0.1], [1.9, 1.1, -0.8]])
    q, mu = g.normal(size=2), g.normal(size=(2, 3))
    entries = CR.all_pairs((2,))
    R = pos[1] - pos[0]
    r = np.linalg.norm(R)
    ci, cj = mu[0] @ R, mu[1] @ R
    A = q[1] * ci - q[0] * cj + mu[0] @ mu[1]
    want = A / r**3 - 3.0 * ci * cj / r**5
    e = CR.dipole_energies(_t(pos), _t(q), _t(mu), entries).detach()
    assert abs(float(e.sum()) - want) <= 1e-13 * abs(want) and abs(float(e[0]) - float(e[1])) <= 1e-13 * abs(want)
    # one charge and one traceless quadrupole
    Q = g.normal(size=(3, 3))
    Q = 0.5 * (Q + Q.T)
    Q -= np.eye(3) * np.trace(Q) / 3.0
    quads = np.stack([np.zeros((3, 3)), Q])
    qq = np.array([0.7, 0.0])
    want = qq[0] * (3.0 * R @ Q @ R / r**5 - np.trace(Q) / r**3)
    e = CR.quadrupole_energies(_t(pos), _t(qq), _t(np.zeros((2, 3))), _t(quads), entries).detach()
    assert abs(float(e.sum()) - want) <= 1e-13 * abs(want)
    # ... and one with a trace: the tr Q / r^3 term is there
    Qt = Q + 0.4 * np.eye(3)
    want = qq[0] * (3.0 * R @ Qt @ R / r**5 - np.trace(Qt) / r**3)
    e = CR.quadrupole_energies(_t(pos), _t(qq), _t(np.zeros((2, 3))), _t(np.stack([np.zeros((3, 3)), Qt])), entries).detach()
    assert abs(float(e.sum()) - want) <= 1e-13 * abs(want) and abs(np.trace(Qt)) > 1.0


def _point_charges(pos, q, mu, p, dhat, d):
    """(positions [K, 3], charges [K], owner [K]) of the point-charge model of every atom at separation d."""
    xs, cs, own = [], [], []
    for a in range(pos.shape[0]):
        xs.append(pos[a]); cs.append(q[a]); own.append(a)
        m = np.linalg.norm(mu[a])
        for s in (1.0, -1.0):
            xs.append(pos[a] + s * 0.5 * d * mu[a] / m); cs.append(s * m / d); own.append(a)
        pm = np.linalg.norm(p[a])
        for s in (1.0, -1.0):      # the dipole +-p / d at +-d/2 dhat ...
            for t in (1.0, -1.0):  # ... as the charge pair +-|p| / d^2 at +-d/2 phat
                xs.append(pos[a] + s * 0.5 * d * dhat[a] + t * 0.5 * d * p[a] / pm); cs.append(s * t * pm / d**2); own.append(a)
    return np.array(xs), np.array(cs), np.array(own)


def test_point_charge_limit_converges_as_d_squared():
    g = np.random.default_rng(5)
    n = 4
    pos = CR.jittered_grid((2, 2, 1), 3.0, 0.3, g)
    q, mu, p = g.normal(size=n), 0.5 * g.normal(size=(n, 3)), 0.5 * g.normal(size=(n, 3))
    dhat = g.normal(size=(n, 3))
    dhat /= np.linalg.norm(dhat, axis=1, keepdims=True)
    Q = 0.5 * (np.einsum("na,nb->nab", p, dhat) + np.einsum("na,nb->nab", dhat, p))
    entries = CR.all_pairs((n,))
    i, j, _ = entries
    r = np.linalg.norm(pos[j] - pos[i], axis=1)
    multipole = (0.5 * (q[i] * q[j] / r).sum() + float(CR.dipole_energies(_t(pos), _t(q), _t(mu), entries).sum().detach())
                 + float(CR.quadrupole_energies(_t(pos), _t(q), _t(mu), _t(Q), entries).sum().detach()))
    errs, ds = [], (0.2, 0.1, 0.05)
    for d in ds:
        x, c, own = _point_charges(pos, q, mu, p, dhat, d)
        dist = np.linalg.norm(x[:, None] - x[None], axis=-1)
        other = own[:, None] != own[None]
        plain = 0.5 * (np.where(other, c[:, None] * c[None] / np.where(other, dist, 1.0), 0.0)).sum()
        errs.append(abs(plain - multipole))
    print(f"multipole energy {multipole:.10f}; |point charges - multipoles| at d = {ds}: " + ", ".join(f"{e:.3e}" for e in errs))
    assert errs[0] > errs[1] > errs[2] and errs[2] <= 1e-3 * abs(multipole)
    for a, b in zip(errs, errs[1:]):  # halving d quarters the difference (the next order, d^4, moves the ratio by a few per cent)
        assert 3.5 <= a / b <= 4.5, errs


def test_two_polarisable_atoms_in_a_uniform_field():
    r, a, F = 2.5, 1.3, 0.07
    pos = _t([[0.0, 0.0, 0.0], [r, 0.0, 0.0]])
    zero, polar, entries = torch.zeros(2, dtype=F64), torch.full((2,), a, dtype=F64), CR.all_pairs((2,))
    T, c = CR.operator(pos, zero, polar, None, entries)
    assert float(c.abs().max()) == 0.0
    H = IR.system_matrix(T, polar)
    for axis, want in ((0, a * F / (1.0 - 2.0 * a / r**3)), (1, a * F / (1.0 + a / r**3)), (2, a * F / (1.0 + a / r**3))):
        field = torch.zeros((2, 3), dtype=F64)
        field[:, axis] = F
        mu = IR.solve(H, IR.right_hand_side(c, polar, field))
        expect = torch.zeros((2, 3), dtype=F64)
        expect[:, axis] = want
        assert float((mu - expect).abs().max()) <= 1e-14 * abs(want) * 10, (axis, mu)
    for factor, definite in ((0.99, True), (1.01, False)):
        p = torch.full((2,), factor * r**3 / 2.0, dtype=F64)
        ev = torch.linalg.eigvalsh(IR.system_matrix(CR.operator(pos, zero, p, None, entries)[0], p))
        assert (float(ev.min()) > 0) == definite, (factor, ev)
    # Thole damping keeps the operator positive definite there
    p = torch.full((2,), 1.01 * r**3 / 2.0, dtype=F64)
    ev = torch.linalg.eigvalsh(IR.system_matrix(CR.operator(pos, zero, p, 0.39, entries)[0], p))
    assert float(ev.min()) > 0


def test_identity_cell_and_zero_shifts_are_the_cluster():
    """The wrapper's way of handing a cluster to the periodic references changes nothing: the same energies with the pair vectors formed by
    hand, and no virial in the result."""
    p = CR.problem("batch")
    pos, q, mu, Q = _t(p["pos"]), _t(p["q"]), _t(p["mu"]), _t(p["Q"])
    out = CR.dipole_evaluate(pos, q, mu, p["entries"], weights=_t(p["w"]))
    assert sorted(out) == ["charge_grads", "dipole_grads", "energies", "forces"]
    i, j, _ = p["entries"]
    R = pos[j] - pos[i]
    r = torch.linalg.norm(R, dim=-1)
    ci, cj = (mu[i] * R).sum(-1), (mu[j] * R).sum(-1)
    pair = (q[j] * ci - q[i] * cj + (mu[i] * mu[j]).sum(-1)) / r**3 - 3.0 * ci * cj / r**5
    want = torch.zeros(p["n"], dtype=F64).index_add(0, i, 0.5 * pair).numpy()
    assert np.abs(out["energies"] - want).max() <= 1e-13 * np.abs(want).max()
    assert out["energies"][-1] == 0.0 and np.abs(out["energies"][70:72]).min() > 0  # the lone atom, the pair
    qout = CR.quadrupole_evaluate(pos, q, mu, Q, p["entries"])
    assert "virial" not in qout and qout["quadrupole_grads"].shape == (p["n"], 3, 3)
