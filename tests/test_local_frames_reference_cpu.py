"""Pins tests/local_frames_reference.py, the yardstick of the local-frame tests, without a device: properties the rotation and the torque
forces must have whatever the implementation -- orthonormal right-handed frames, covariance under rigid rotation, zero net torque force per
molecule, balance of the total torque, mirror images, wrapped against unwrapped coordinates, and the stated virial term against the strain
derivative.  The geometries of the GPU tests are checked against the ranges the issue sets (bond lengths in [0.9, 1.6], angles between frame
vectors in [40, 140] degrees, Z_ONLY axes away from the 0.866 switch), and the reference's own float32-input evaluation against the float32
bar of the GPU tests."""
import math

import pytest
import torch

from tests import local_frames_reference as LR

F64 = torch.float64
MOLECULES = ("none", "z_only", "z_only_y", "water", "ammonia", "z_bisect", "chiral", "mirror")


def _weights(n, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn((n, 3), dtype=F64, generator=gen), torch.randn((n, 3, 3), dtype=F64, generator=gen)


def _mixed():
    return LR.join([LR.molecule(m) for m in MOLECULES])


@pytest.mark.parametrize("name", MOLECULES)
def test_rotation_is_orthonormal_with_determinant_one(name):
    pos, atoms, kinds = LR.molecule(name)
    R, sigma = LR.rotation(pos, atoms, kinds)
    eye = torch.eye(3, dtype=F64).expand_as(R)
    assert float((R.transpose(-1, -2) @ R - eye).abs().max()) < 1e-14
    assert float((torch.linalg.det(R) - 1.0).abs().max()) < 1e-14
    assert bool(((sigma == 1.0) | (sigma == -1.0)).all())
    if name == "none":
        assert torch.equal(R[0], torch.eye(3, dtype=F64))


@pytest.mark.parametrize("name", [m for m in MOLECULES if m != "none"])
def test_geometries_stay_inside_the_stated_ranges(name):
    """Bond lengths in [0.9, 1.6], pairwise angles between the frame vectors of an atom in [40, 140] degrees, Z_ONLY axes at least 0.05 away
    from the switch."""
    pos, atoms, kinds = LR.molecule(name)
    for i in range(pos.shape[0]):
        d = [pos[a] - pos[i] for a in atoms[i].tolist() if a >= 0]
        for v in d:
            assert 0.9 <= float(v.norm()) <= 1.6, (name, i, float(v.norm()))
        for a in range(len(d)):
            for b in range(a + 1, len(d)):
                ang = math.degrees(math.acos(float((d[a] * d[b]).sum() / (d[a].norm() * d[b].norm()))))
                assert 40.0 <= ang <= 140.0, (name, i, ang)
        if int(kinds[i]) == LR.Z_ONLY:
            assert abs(abs(float(d[0][0] / d[0].norm())) - LR.Z_ONLY_SWITCH) > 0.05


def test_z_only_rigid_rotation_with_axial_multipoles():
    """mu -> U mu, Q -> U Q U^T for Z_ONLY with axially symmetric local multipoles (the x-like lab axis does not rotate with the molecule, so
    only the axial part is covariant)."""
    pos, atoms, kinds = LR.molecule("z_only")
    mu_loc = torch.tensor([[0.0, 0.0, 0.7], [0.0, 0.0, -0.4]], dtype=F64)
    q_loc = torch.diag(torch.tensor([-0.3, -0.3, 0.6], dtype=F64)).repeat(2, 1, 1)
    mu, quad = LR.rotate(pos, mu_loc, q_loc, atoms, kinds)
    U = LR.random_rotation(torch.Generator().manual_seed(5))
    mu_r, quad_r = LR.rotate(pos @ U.T, mu_loc, q_loc, atoms, kinds)
    assert float((mu_r - mu @ U.T).abs().max()) < 1e-14
    assert float((quad_r - U @ quad @ U.T).abs().max()) < 1e-14


@pytest.mark.parametrize("name", ["water", "ammonia", "z_bisect", "chiral"])
def test_rigid_rotation_of_a_molecule_with_internal_frames(name):
    pos, atoms, kinds = LR.molecule(name)
    mu_loc, q_loc = LR.local_multipoles(pos.shape[0], 3)
    if name == "z_bisect":  # its Z_ONLY atom is covariant only for axial multipoles (then on either side of the switch)
        mu_loc[4, :2] = 0.0
        q_loc[4] = torch.diag(torch.tensor([-0.2, -0.2, 0.4], dtype=F64))
    mu, quad = LR.rotate(pos, mu_loc, q_loc, atoms, kinds)
    U = LR.random_rotation(torch.Generator().manual_seed(9))
    mu_r, quad_r = LR.rotate(pos @ U.T, mu_loc, q_loc, atoms, kinds)
    assert float((mu_r - mu @ U.T).abs().max()) < 1e-13
    assert float((quad_r - U @ quad @ U.T).abs().max()) < 1e-13


def test_torque_forces_sum_to_zero_per_molecule_and_balance_the_torque():
    """With g_mu = dE/dmu and g_Q = dE/dQ held fixed, the torque on the multipoles of a molecule is sum_i mu_i x (-g_mu_i) + the quadrupole
    analogue tau_a = -2 eps_abc (Q S)_bc; the torque forces F = -dL/dr must carry exactly that torque, sum_i r_i x F_i = tau, and no net force.
    Z_ONLY atoms are left out: their lab x-like axis is an external direction, so they exchange torque with the laboratory."""
    pos, atoms, kinds, mol = LR.join([LR.molecule(m) for m in ("water", "ammonia", "chiral", "mirror")])
    n = pos.shape[0]
    mu_loc, q_loc = LR.local_multipoles(n, 11)
    w_mu, w_q = _weights(n, 12)
    out = LR.evaluate(pos, mu_loc, q_loc, atoms, kinds, w_mu, w_q)
    forces = -out["positions_grad"]
    S = 0.5 * (w_q + w_q.transpose(-1, -2))
    qs = torch.einsum("nab,nbc->nac", out["quadrupoles"], S)
    tau_q = -2.0 * torch.stack((qs[:, 1, 2] - qs[:, 2, 1], qs[:, 2, 0] - qs[:, 0, 2], qs[:, 0, 1] - qs[:, 1, 0]), dim=-1)
    tau = torch.linalg.cross(out["dipoles"], -w_mu) + tau_q
    for m in range(int(mol.max()) + 1):
        sel = mol == m
        scale = float(forces[sel].abs().max())
        assert float(forces[sel].sum(0).abs().max()) < 1e-13 * scale
        lever = torch.linalg.cross(pos[sel], forces[sel]).sum(0)
        assert float((lever - tau[sel].sum(0)).abs().max()) < 1e-12 * max(scale, float(tau[sel].abs().max()))


def test_mirror_image_of_a_chiral_centre_gives_the_mirrored_tensors():
    """x -> -x on the positions of a chiral Z_THEN_X centre: mu -> M mu, Q -> M Q M with M = diag(-1, 1, 1), because the chirality rule flips
    the local y axis of the image."""
    pos, atoms, kinds = LR.molecule("chiral")
    pos_m, _, _ = LR.molecule("mirror")
    mu_loc, q_loc = LR.local_multipoles(pos.shape[0], 21)
    _, s0 = LR.rotation(pos, atoms, kinds)
    _, s1 = LR.rotation(pos_m, atoms, kinds)
    assert torch.equal(s0, -s1), "every centre of the image has the opposite handedness"
    mu, quad = LR.rotate(pos, mu_loc, q_loc, atoms, kinds)
    mu_m, quad_m = LR.rotate(pos_m, mu_loc, q_loc, atoms, kinds)
    M = torch.diag(torch.tensor([-1.0, 1.0, 1.0], dtype=F64))
    assert float((mu_m - mu @ M).abs().max()) < 1e-14
    assert float((quad_m - M @ quad @ M).abs().max()) < 1e-14


def _periodic():
    pos, atoms, kinds, mol = _mixed()
    cell = torch.tensor([[9.0, 0.0, 0.0], [1.5, 8.0, 0.0], [-1.0, 2.0, 7.5]], dtype=F64)
    gen = torch.Generator().manual_seed(31)
    shifts = torch.randint(-2, 3, (pos.shape[0], 3), generator=gen).to(F64)
    return pos, atoms, kinds, cell, pos + shifts @ cell


def test_wrapped_and_unwrapped_coordinates_agree():
    pos, atoms, kinds, cell, moved = _periodic()
    mu_loc, q_loc = LR.local_multipoles(pos.shape[0], 32)
    w_mu, w_q = _weights(pos.shape[0], 33)
    a = LR.evaluate(pos, mu_loc, q_loc, atoms, kinds, w_mu, w_q, cell=cell)
    b = LR.evaluate(moved, mu_loc, q_loc, atoms, kinds, w_mu, w_q, cell=cell)
    free = LR.evaluate(pos, mu_loc, q_loc, atoms, kinds, w_mu, w_q)
    for key in ("dipoles", "quadrupoles", "positions_grad", "local_dipole_grads", "local_quadrupole_grads", "virial"):
        scale = float(a[key].abs().max())
        assert float((a[key] - b[key]).abs().max()) < 1e-12 * scale, key
        if key != "virial":
            assert float((a[key] - free[key]).abs().max()) < 1e-12 * scale, key


def test_virial_is_minus_the_strain_derivative_and_the_sum_over_frame_vectors():
    """The strain derivative of sum w . mu + W : Q (autograd through x -> (I + eps) x) equals the stated term: minus
    sum_i sum_a (dL/dd_a) d_a^T, which by dL/dr_a = dL/dd_a is minus sum_i (dL/dr_i) r_i^T for unwrapped molecules; and a central difference."""
    pos, atoms, kinds, cell, _ = _periodic()
    n = pos.shape[0]
    mu_loc, q_loc = LR.local_multipoles(n, 41)
    w_mu, w_q = _weights(n, 42)
    out = LR.evaluate(pos, mu_loc, q_loc, atoms, kinds, w_mu, w_q, cell=cell)
    stated = -torch.einsum("na,nb->ab", out["positions_grad"], pos)
    assert float((out["virial"][0] - stated).abs().max()) < 1e-12 * float(stated.abs().max())

    def loss(eps):
        defo = torch.eye(3, dtype=F64) + eps
        mu, quad = LR.rotate(pos @ defo.T, mu_loc, q_loc, atoms, kinds, cell @ defo.T)
        return float((w_mu * mu).sum() + (w_q * quad).sum())

    h = 1e-6
    for a in range(3):
        for b in range(3):
            e = torch.zeros((3, 3), dtype=F64)
            e[a, b] = h
            fd = (loss(e) - loss(-e)) / (2 * h)
            assert abs(fd + float(out["virial"][0, a, b])) < 1e-7 * float(stated.abs().max())


def test_float32_input_evaluation_stays_inside_the_float32_bar():
    """The GPU tests compare float32 calls with the reference evaluated at the float32-rounded inputs, bar 1e-6 of the largest component.  On
    these geometries the rounding of the inputs itself moves the reference by 3e-8 - 1e-7, well inside the bar, so a float32 result within 1e-6
    measures the kernel; no Z_ONLY axis or chirality sign flips under the rounding."""
    pos, atoms, kinds, _ = _mixed()
    n = pos.shape[0]
    mu_loc, q_loc = LR.local_multipoles(n, 51)
    w_mu, w_q = _weights(n, 52)
    r32 = lambda t: t.to(torch.float32).to(F64)  # noqa: E731
    a = LR.evaluate(pos, mu_loc, q_loc, atoms, kinds, w_mu, w_q)
    b = LR.evaluate(r32(pos), r32(mu_loc), r32(q_loc), atoms, kinds, r32(w_mu), r32(w_q))
    for key in ("dipoles", "quadrupoles", "positions_grad", "local_dipole_grads", "local_quadrupole_grads"):
        rel = float((a[key] - b[key]).abs().max() / a[key].abs().max())
        print(f"{key:24s} float32-rounded inputs move the reference by {rel:.2e}")
        assert rel < 1e-6, key
