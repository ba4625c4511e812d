"""Float64 torch restatement of the local-frame rotation of `nvalchemiops.interactions.electrostatics.frames` (Tinker / OpenMM's axis types).

With d_a = r_a - r_i for the frame atoms a = (z, x, y) of atom i (the minimum image d - round(d cell^-1) cell when a cell is given) and
n(v) = v / |v|:

    kind         e_z                                x-like vector before orthogonalising
    Z_ONLY       n(d_z)                             lab x if |e_z . x^| < 0.866, else lab y
    Z_THEN_X     n(d_z)                             d_x
    BISECTOR     n(n(d_z) + n(d_x))                 d_x
    Z_BISECT     n(d_z)                             n(n(d_x) + n(d_y))
    THREE_FOLD   n(n(d_z) + n(d_x) + n(d_y))        d_x

e_x is the x-like vector orthogonalised against e_z and normalised, e_y = e_z x e_x, R = [e_x e_y e_z] as columns; NONE is R = I.  A Z_THEN_X
atom with a y atom has its local y axis mirrored when d_y . (d_z x d_x) < 0 (mu_y, Q_xy, Q_yz change sign; the sign is a constant for every
derivative).  mu = R mu_loc, Q = R 1/2 (Q_loc + Q_loc^T) R^T.

Nothing here is hand-differentiated: every derivative output of `evaluate` comes from autograd of L = sum_i w_i . mu_i + W_i : Q_i, the virial
term from autograd with respect to an explicit strain eps (x -> (I + eps) x on positions and cell rows, the LOCAL multipoles held fixed).  Each
kind is evaluated on its own atoms only, so no masked branch feeds a NaN into a gradient."""
import math

import torch

F64 = torch.float64
NONE, Z_ONLY, Z_THEN_X, BISECTOR, Z_BISECT, THREE_FOLD = range(6)
Z_ONLY_SWITCH = 0.866


def _unit(v):
    return v / v.norm(dim=-1, keepdim=True)


def frame_vectors(pos, atoms, idx, slot, cell=None, batch_idx=None):
    """d_a [len(idx), 3] of slot `slot` for the atoms `idx`."""
    d = pos[atoms[idx, slot].long()] - pos[idx]
    if cell is not None:
        cells = cell.reshape(-1, 3, 3)
        c = cells[batch_idx[idx].long()] if batch_idx is not None else cells[:1].expand(idx.shape[0], 3, 3)
        n = torch.round(torch.einsum("na,nab->nb", d, torch.linalg.inv(c))).detach()
        d = d - torch.einsum("na,nab->nb", n, c)
    return d


def rotation(pos, atoms, kinds, cell=None, batch_idx=None):
    """(R [N, 3, 3] with the columns e_x, e_y, e_z; sigma [N] = -1 where the local y axis is mirrored, else +1)."""
    n = pos.shape[0]
    R = torch.eye(3, dtype=F64, device=pos.device).repeat(n, 1, 1)
    sigma = torch.ones(n, dtype=F64, device=pos.device)
    for kind in (Z_ONLY, Z_THEN_X, BISECTOR, Z_BISECT, THREE_FOLD):
        idx = torch.nonzero(kinds == kind).reshape(-1)
        if idx.numel() == 0:
            continue
        dz = frame_vectors(pos, atoms, idx, 0, cell, batch_idx)
        dx = frame_vectors(pos, atoms, idx, 1, cell, batch_idx) if kind != Z_ONLY else None
        dy = frame_vectors(pos, atoms, idx, 2, cell, batch_idx) if kind in (Z_BISECT, THREE_FOLD) else None
        if kind == BISECTOR:
            ez = _unit(_unit(dz) + _unit(dx))
        elif kind == THREE_FOLD:
            ez = _unit(_unit(dz) + _unit(dx) + _unit(dy))
        else:
            ez = _unit(dz)
        if kind == Z_ONLY:
            lab = torch.eye(3, dtype=F64, device=pos.device)
            v = torch.where((ez[:, 0].abs() < Z_ONLY_SWITCH)[:, None], lab[0].expand_as(ez), lab[1].expand_as(ez))
        elif kind == Z_BISECT:
            v = _unit(_unit(dx) + _unit(dy))
        else:
            v = dx
        ex = _unit(v - (v * ez).sum(-1, keepdim=True) * ez)
        ey = torch.linalg.cross(ez, ex)
        R = R.index_copy(0, idx, torch.stack((ex, ey, ez), dim=-1))
        if kind == Z_THEN_X:
            chiral = torch.nonzero(atoms[idx, 2] >= 0).reshape(-1)
            if chiral.numel():
                cy = frame_vectors(pos, atoms, idx[chiral], 2, cell, batch_idx)
                triple = (cy * torch.linalg.cross(dz[chiral], dx[chiral])).sum(-1)
                sigma = sigma.index_copy(0, idx[chiral], torch.where(triple < 0, -1.0, 1.0).to(F64).detach())
    return R, sigma


def rotate(pos, mu_loc, q_loc, atoms, kinds, cell=None, batch_idx=None):
    """(mu [N, 3] | None, Q [N, 3, 3] | None) in the laboratory frame."""
    R, sigma = rotation(pos, atoms, kinds, cell, batch_idx)
    flip = torch.stack((torch.ones_like(sigma), sigma, torch.ones_like(sigma)), dim=-1)
    mu = None if mu_loc is None else torch.einsum("nab,nb->na", R, mu_loc * flip)
    quad = None
    if q_loc is not None:
        qs = 0.5 * (q_loc + q_loc.transpose(-1, -2)) * flip[:, :, None] * flip[:, None, :]
        quad = torch.einsum("nab,nbc,ndc->nad", R, qs, R)
    return mu, quad


def evaluate(pos, mu_loc, q_loc, atoms, kinds, w_mu=None, w_q=None, cell=None, batch_idx=None):
    """dict of float64 tensors on the inputs' device: dipoles, quadrupoles (None where the local input is None) and, of
    L = sum_i w_mu_i . mu_i + w_q_i : Q_i (weights default to zero), positions_grad = dL/dr, local_dipole_grads, local_quadrupole_grads and,
    with a cell, virial [num_systems, 3, 3] = -dL/d(strain)."""
    pos = pos.detach().to(F64).clone().requires_grad_(True)
    leaves = [pos]
    if mu_loc is not None:
        mu_loc = mu_loc.detach().to(F64).clone().requires_grad_(True)
        leaves.append(mu_loc)
    if q_loc is not None:
        q_loc = q_loc.detach().to(F64).clone().requires_grad_(True)
        leaves.append(q_loc)
    cells = None if cell is None else cell.detach().to(F64).reshape(-1, 3, 3)

    def loss(mu, quad):
        total = pos.sum() * 0.0
        if mu is not None and w_mu is not None:
            total = total + (w_mu.to(F64) * mu).sum()
        if quad is not None and w_q is not None:
            total = total + (w_q.to(F64) * quad).sum()
        return total

    mu, quad = rotate(pos, mu_loc, q_loc, atoms, kinds, cells, batch_idx)
    grads = list(torch.autograd.grad(loss(mu, quad), leaves, allow_unused=True))
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, leaves)]
    out = dict(dipoles=None if mu is None else mu.detach(), quadrupoles=None if quad is None else quad.detach(), positions_grad=grads[0],
               local_dipole_grads=grads[1] if mu_loc is not None else None, local_quadrupole_grads=grads[-1] if q_loc is not None else None)
    if cells is not None:
        nsys = cells.shape[0]
        eps = torch.zeros((nsys, 3, 3), dtype=F64, device=pos.device, requires_grad=True)
        defo = torch.eye(3, dtype=F64, device=pos.device) + eps
        per_atom = defo[batch_idx.long()] if batch_idx is not None else defo[:1].expand(pos.shape[0], 3, 3)
        pos_e = torch.einsum("nab,nb->na", per_atom, pos.detach())
        cell_e = torch.einsum("sab,skb->ska", defo, cells)  # every lattice vector (row) a -> (I + eps) a
        mu_e, quad_e = rotate(pos_e, None if mu_loc is None else mu_loc.detach(), None if q_loc is None else q_loc.detach(), atoms, kinds, cell_e,
                              batch_idx)
        total = eps.sum() * 0.0
        if mu_e is not None and w_mu is not None:
            total = total + (w_mu.to(F64) * mu_e).sum()
        if quad_e is not None and w_q is not None:
            total = total + (w_q.to(F64) * quad_e).sum()
        out["virial"] = -torch.autograd.grad(total, eps)[0]
    return out


# ---- geometries shared by the tests: bond lengths in [0.9, 1.6], angles between frame vectors in [40, 140] degrees -------------------------------
def random_rotation(gen):
    q, r = torch.linalg.qr(torch.randn((3, 3), dtype=F64, generator=gen))
    q = q * torch.sign(torch.diagonal(r))
    if torch.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def water(gen=None):
    """(positions [3, 3], frame_atoms [3, 3], frame_kinds [3]): O bisector of the two H, each H z-then-x on O and the other H.  The H-O-H
    angle is 96 degrees, so that the angle O-H-H' (42 degrees) stays inside [40, 140] as every other angle between frame vectors here."""
    h = 0.9572
    half = math.radians(0.5 * 96.0)
    pos = torch.tensor([[0.0, 0.0, 0.0], [h * math.sin(half), 0.0, h * math.cos(half)], [-h * math.sin(half), 0.0, h * math.cos(half)]], dtype=F64)
    atoms = torch.tensor([[1, 2, -1], [0, 2, -1], [0, 1, -1]], dtype=torch.int32)
    kinds = torch.tensor([BISECTOR, Z_THEN_X, Z_THEN_X], dtype=torch.int32)
    if gen is not None:
        pos = pos @ random_rotation(gen).T
    return pos, atoms, kinds


def _centre(tail):
    """A pyramidal centre: atom 0, three ligands at about 1.0 with mutual angles of about 90 degrees (so that a ligand sees the centre and
    another ligand 45 degrees and less than 1.6 apart) and, with `tail`, a fourth ligand opposite the pyramid; rotated off the lab axes."""
    beta = math.asin(math.sqrt((1.0 - math.cos(math.radians(90.0))) / 1.5))
    rows = [[0.0, 0.0, 0.0]]
    for k, (b, dphi) in enumerate(((1.0, 0.02), (1.04, -0.03), (0.97, 0.03))):
        phi = 0.3 + 2.0 * math.pi * k / 3.0 + dphi
        rows.append([b * math.sin(beta) * math.cos(phi), b * math.sin(beta) * math.sin(phi), b * math.cos(beta)])
    if tail:
        rows.append([0.09, -0.07, -1.1])
    return torch.tensor(rows, dtype=F64) @ random_rotation(torch.Generator().manual_seed(77)).T + torch.tensor([0.4, -0.3, 0.2], dtype=F64)


def molecule(name):
    """The smallest molecule that holds each kind: (positions, frame_atoms, frame_kinds)."""
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)  # noqa: E731
    f64 = lambda a: torch.tensor(a, dtype=F64)  # noqa: E731
    if name == "none":
        return f64([[0.3, -0.2, 0.1]]), i32([[-1, -1, -1]]), i32([NONE])
    if name == "z_only":  # the axis (0.39, 0.55, 0.74) and its reverse: |e_z . x^| = 0.39, well below the switch
        return f64([[0.1, 0.2, -0.3], [0.1 + 0.45, 0.2 + 0.64, -0.3 + 0.86]]), i32([[1, -1, -1], [0, -1, -1]]), i32([Z_ONLY, Z_ONLY])
    if name == "z_only_y":  # the axis (0.97, 0.17, 0.17): beyond the switch, lab y is the x-like vector
        return f64([[0.0, 0.0, 0.0], [1.1, 0.2, 0.2]]), i32([[1, -1, -1], [0, -1, -1]]), i32([Z_ONLY, Z_ONLY])
    if name == "water":
        return water()
    if name == "ammonia":  # N three-fold on its three H; each H z-then-x on N and the next H
        return _centre(False), i32([[1, 2, 3], [0, 2, -1], [0, 3, -1], [0, 1, -1]]), i32([THREE_FOLD, Z_THEN_X, Z_THEN_X, Z_THEN_X])
    if name == "z_bisect":  # a 5-atom centre: atom 0 z-bisect on (4; 1, 2), the ligands z-then-x / bisector / chiral z-then-x / z-only
        return (_centre(True), i32([[4, 1, 2], [0, 2, -1], [0, 3, -1], [0, 1, 2], [0, -1, -1]]),
                i32([Z_BISECT, Z_THEN_X, BISECTOR, Z_THEN_X, Z_ONLY]))
    if name in ("chiral", "mirror"):  # Z_THEN_X centres with a y atom; "mirror" is the image under x -> -x
        pos = _centre(False)
        if name == "mirror":
            pos = pos * f64([-1.0, 1.0, 1.0])
        return pos, i32([[1, 2, 3], [0, 2, 3], [0, 3, 1], [0, 1, 2]]), i32([Z_THEN_X, Z_THEN_X, Z_THEN_X, Z_THEN_X])
    raise KeyError(name)


def join(parts):
    """Molecules -> one system: (positions, frame_atoms with the offsets added, frame_kinds, molecule index per atom)."""
    pos, atoms, kinds, mol, off = [], [], [], [], 0
    for m, (p, a, k) in enumerate(parts):
        pos.append(p)
        atoms.append(torch.where(a >= 0, a + off, a))
        kinds.append(k)
        mol.append(torch.full((p.shape[0],), m, dtype=torch.int64))
        off += p.shape[0]
    return torch.cat(pos), torch.cat(atoms).to(torch.int32), torch.cat(kinds).to(torch.int32), torch.cat(mol)


def waters(n_atoms, seed, spacing=4.0):
    """`n_atoms` atoms: as many randomly rotated waters on a cubic grid as fit, then NONE atoms as filler."""
    gen = torch.Generator().manual_seed(seed)
    n_w = n_atoms // 3
    side = max(1, int(round(n_w ** (1.0 / 3.0) + 0.5)))
    parts = []
    for m in range(n_w):
        p, a, k = water(gen)
        origin = torch.tensor([m % side, (m // side) % side, m // (side * side)], dtype=F64) * spacing
        parts.append((p + origin + 0.3 * torch.rand(3, dtype=F64, generator=gen), a, k))
    for m in range(n_atoms - 3 * n_w):
        parts.append((torch.tensor([[-spacing * (m + 1), 0.0, 0.0]], dtype=F64), torch.tensor([[-1, -1, -1]], dtype=torch.int32),
                      torch.tensor([NONE], dtype=torch.int32)))
    return join(parts)


def local_multipoles(n, seed, traceless=True):
    """Random local dipoles [n, 3] and (not symmetric, so the symmetrisation is exercised) quadrupoles [n, 3, 3]."""
    gen = torch.Generator().manual_seed(seed)
    mu = torch.randn((n, 3), dtype=F64, generator=gen)
    quad = torch.randn((n, 3, 3), dtype=F64, generator=gen)
    if traceless:
        quad = quad - torch.eye(3, dtype=F64) * (torch.diagonal(quad, dim1=-2, dim2=-1).sum(-1) / 3.0)[:, None, None]
    return mu, quad
