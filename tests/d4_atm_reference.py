"""Float64 torch restatement of the three-body (Axilrod-Teller-Muto) term of DFT-D4: the checker of `dftd4_atm`.

Written from the definition (include/nvalchemiops_hip.h, `dftd4_atm`'s docstring), not from the kernel.  The image enumeration and the
triple loop are those of tests/atm_reference.py (explicit enumeration of atom images; a triple counts once per lattice-translation class:
the sum runs over (centre atom in the home cell, unordered pair of its neighbour images), which meets every class three times, and is
divided by three; free molecules: each triple i < j < k once).  The coordination number, the Gaussian weights W and the charge scaling zeta
are those of tests/d4_reference.py, the latter at q = 0 for every atom:

    CN_i    = sum_row delta(Z_i,Z_j) 1/2 (1 + erf(-k_cn (r / (rcov_i + rcov_j) - 1)))         over ALL pairs closer than `list_cutoff`
    w_i[a]  = W_a(CN_i) zeta_a(q = 0),      C6_XY = sum_ab w_X[a] c6_ref[Z_X,Z_Y,a,b] w_Y[b]
    E_ABC   = s9 sqrt(C6_AB C6_AC C6_BC) ang fdamp                                            (nothing if any C6 < 1e-12)
    ang     = 0.375 (a + b - c)(a + c - b)(b + c - a) / P^5 + 1 / P^3,   a, b, c squared sides, P product of the sides
    fdamp   = 1 / (1 + 6 (R0_AB R0_AC R0_BC / P)^(alpha / 3)),          R0_XY = a1 sqrt(3 r4r2_X r4r2_Y) + a2

The energy is one differentiable scalar per system; forces come by autograd through the positions INCLUDING the coordination-number
dependence of C6, the virial as minus the derivative with respect to a symmetric strain applied to positions and cell.
`work_dtype=torch.float32` evaluates every per-pair, per-atom and per-triple quantity (and its derivative) in float32 while every SUM stays
float64 -- the arithmetic model of the kernels.  `cn_path=False` holds the coordination numbers fixed when differentiating: the forces
without the chain-rule pass (tests measure what that pass contributes).  Small systems only.
"""
import numpy as np
import torch

from tests import atm_reference as A
from tests import d4_reference as R


def _system(pos, numbers, tables, cell, a1, a2, list_cutoff, rc3, s9, alpha, cn_cutoff, wf, ga, gc, k_cn, wd, chunk, cn_path, topology):
    """One system: (energy, forces[N,3], virial[3,3] or None, cn[N], triples enumerated, most kept entries in a row)."""
    f64 = torch.float64
    n = len(pos)
    ok = R.valid_atoms(numbers, tables)
    z = torch.as_tensor(np.where(ok, np.asarray(numbers), 0), dtype=torch.long)
    x0 = torch.tensor(np.asarray(pos, np.float64), dtype=f64, requires_grad=True)
    eps = torch.zeros(3, 3, dtype=f64, requires_grad=True)
    tab = lambda k: torch.as_tensor(tables[k], dtype=wd)  # noqa: E731
    rcov, en, r4r2 = tab("rcov"), tab("en"), tab("r4r2")
    c6_table = torch.as_tensor(np.nan_to_num(tables["c6_ref"]), dtype=wd)
    zero_q = torch.zeros(n, dtype=wd)
    atom_ok = torch.as_tensor(ok)[:, None]

    free = cell is None
    if topology is None:
        li, lj, ls = A.enumerate_pairs(pos, cell, list_cutoff)
        keep = ok[li] & ok[lj]
        li, lj, ls = li[keep], lj[keep], ls[keep]
        inside = np.linalg.norm(A._np_vectors(pos, cell, li, lj, ls), axis=1) < rc3
        ti, tj, ts = li[inside], lj[inside], ls[inside]
        vec_np = A._np_vectors(pos, cell, ti, tj, ts)
        counts = np.bincount(ti, minlength=n)
        start = np.concatenate([[0], np.cumsum(counts)])
        vp, vq = [], []
        for c in range(n):
            k = counts[c]
            if k < 2:
                continue
            p, q = np.triu_indices(k, 1)
            p = p + start[c]; q = q + start[c]
            djk = vec_np[q] - vec_np[p]
            r2 = (djk * djk).sum(1)
            good = (r2 < rc3 ** 2) & (r2 >= 1e-24)
            if free:  # each triple once: centre < j < k (rows are sorted by j)
                good &= tj[p] > c
            vp.append(p[good]); vq.append(q[good])
        vp = np.concatenate(vp) if vp else np.zeros(0, np.int64)
        vq = np.concatenate(vq) if vq else np.zeros(0, np.int64)
        topology = (li, lj, ls, inside, vp, vq)
    li, lj, ls, inside, vp, vq = topology
    ti, tj, ts = li[inside], lj[inside], ls[inside]
    counts = np.bincount(ti, minlength=n)
    weight = 1.0 if free else 1.0 / 3.0

    def pair_level():
        """Everything that belongs to atoms and pairs, on a fresh graph: (pair vectors of the kept entries, C6 of every atom pair, cn64)."""
        strain = torch.eye(3, dtype=f64) + 0.5 * (eps + eps.T)
        x = x0 @ strain
        h = None if cell is None else torch.as_tensor(np.asarray(cell, np.float64).reshape(3, 3)) @ strain

        def vectors(i, j, s):  # float64 difference (+ shift), then the working dtype -- as the kernels cast
            d = x[torch.as_tensor(j, dtype=torch.long)] - x[torch.as_tensor(i, dtype=torch.long)]
            if h is not None:
                d = d + torch.as_tensor(s, dtype=f64) @ h
            return d.to(wd)

        tli, tlj = torch.as_tensor(li, dtype=torch.long), torch.as_tensor(lj, dtype=torch.long)
        r = vectors(li, lj, ls).norm(dim=1)
        live = (r > 1e-8).detach()
        zi, zj = z[tli], z[tlj]
        delta = R.K4 * torch.exp(-(torch.abs(en[zi] - en[zj]) + R.K5) ** 2 / R.K6)
        count = delta * 0.5 * (1.0 + torch.erf(-k_cn * (r / (rcov[zi] + rcov[zj]) - 1.0)))
        counted = live if cn_cutoff is None else live & (r < cn_cutoff).detach()
        count = torch.where(counted, count, torch.zeros_like(count))
        cn64 = torch.zeros(n, dtype=f64).index_add(0, tli, count.to(f64))
        cn = cn64.to(wd)
        if not cn_path:
            cn = cn.detach()
        W, mask = R.gaussian_weights(cn, z, tables, wf, wd)
        # an element with one reference has W = g / g = 1 at every CN: taken as the constant it is, so that its CN derivative is exactly 0
        # (autograd's quotient rule would leave x / g - g x / g^2, zero only to rounding)
        single = (torch.as_tensor(tables["n_ref"], dtype=torch.long)[z] == 1)[:, None]
        W = torch.where(single, W.detach(), W)
        zeta = R.charge_scaling(zero_q, z, tables, ga, gc, wd)  # q = 0 for every atom: D4's definition of the three-body C6
        m = mask & atom_ok
        w = torch.where(m, torch.where(m, W, torch.zeros_like(W)) * zeta, torch.zeros_like(W))
        c6_atoms = torch.einsum("ia,ijab,jb->ij", w, c6_table[z][:, z], w)  # [n,n]: C6 depends on the two atoms, not on the image
        return vectors(ti, tj, ts), c6_atoms, cn64

    def r0_of(za, zb):
        return a1 * torch.sqrt(3.0 * r4r2[za] * r4r2[zb]) + a2

    tti, ttj = torch.as_tensor(ti, dtype=torch.long), torch.as_tensor(tj, dtype=torch.long)
    total_val = 0.0
    cn_out = None
    for lo in range(0, max(len(vp), 1), chunk):
        p = torch.as_tensor(vp[lo:lo + chunk]); q = torch.as_tensor(vq[lo:lo + chunk])
        if len(p) == 0:
            break
        # (pair quantities are re-derived per chunk so that each chunk's graph is freed after its backward pass)
        Rv, c6_atoms, cn64 = pair_level()
        cn_out = cn64.detach().numpy()
        ci, cj, ck = tti[p], ttj[p], ttj[q]
        rij, rik = Rv[p], Rv[q]
        rjk = rik - rij
        a = (rij * rij).sum(1); b = (rik * rik).sum(1); c = (rjk * rjk).sum(1)
        P = torch.sqrt(a) * torch.sqrt(b) * torch.sqrt(c)
        c6_ij, c6_ik, c6_jk = c6_atoms[ci, cj], c6_atoms[ci, ck], c6_atoms[cj, ck]
        live = (c6_ij >= 1e-12) & (c6_ik >= 1e-12) & (c6_jk >= 1e-12)
        one = torch.ones_like(c6_ij)
        c9 = torch.sqrt(torch.where(live, c6_ij, one) * torch.where(live, c6_ik, one) * torch.where(live, c6_jk, one))
        ang = 0.375 * (a + b - c) * (a + c - b) * (b + c - a) / P ** 5 + 1.0 / P ** 3
        r0 = r0_of(z[ci], z[cj]) * r0_of(z[ci], z[ck]) * r0_of(z[cj], z[ck])
        fdamp = 1.0 / (1.0 + 6.0 * (r0 / P) ** (alpha / 3.0))
        e = torch.where(live, s9 * c9 * ang * fdamp, torch.zeros_like(ang))
        part = weight * e.to(f64).sum()
        if part.requires_grad:
            part.backward()
        total_val += float(part.detach())
    if cn_out is None:
        cn_out = pair_level()[2].detach().numpy()
    forces = -x0.grad.numpy() if x0.grad is not None else np.zeros((n, 3))
    virial = None
    if cell is not None:
        virial = -eps.grad.numpy() if eps.grad is not None else np.zeros((3, 3))
        virial = 0.5 * (virial + virial.T)
    return total_val, forces, virial, cn_out, len(vp), int(counts.max()) if n else 0, topology


def reference(pos, numbers, tables, a1, a2, list_cutoff, three_body_cutoff=None, s9=1.0, alpha=16.0, cn_cutoff=None, wf=6.0, ga=3.0, gc=2.0,
              k_cn=7.5, cell=None, batch_idx=None, work_dtype=torch.float64, chunk=1_000_000, cn_path=True, topology=None):
    """Returns dict(energy[B], forces[N,3], virial[B,3,3] (periodic only, else None), cn[N], triples (enumerated: free systems each triple
    once, periodic systems once per centre), kept (the most entries inside three_body_cutoff any row holds)) as float64 numpy arrays / ints.
    `cell`: None, [3,3] or [B,3,3]; `batch_idx`: None or [N] (systems are evaluated one by one).  `topology` (single system only): the
    pairs and triples of an earlier call (its "topology" entry) to use instead of enumerating -- finite differences keep the lists of the
    undisplaced system."""
    pos = np.asarray(pos, np.float64)
    numbers = np.asarray(numbers)
    n = len(pos)
    bi = np.zeros(n, np.int64) if batch_idx is None else np.asarray(batch_idx, np.int64)
    cells = None if cell is None else np.asarray(cell, np.float64).reshape(-1, 3, 3)
    nsys = (int(bi.max()) + 1 if n else 1) if cells is None else len(cells)
    rc3 = three_body_cutoff if three_body_cutoff is not None else list_cutoff
    out = dict(energy=np.zeros(nsys), forces=np.zeros((n, 3)), virial=None if cells is None else np.zeros((nsys, 3, 3)), cn=np.zeros(n),
               triples=0, kept=0, topology=None)
    assert topology is None or nsys == 1
    for s in range(nsys):
        sel = np.nonzero(bi == s)[0]
        if len(sel) == 0:
            continue
        e, f, v, c, triples, kept, topo = _system(pos[sel], numbers[sel], tables, None if cells is None else cells[s], a1, a2, list_cutoff, rc3, s9,
                                            alpha, cn_cutoff, wf, ga, gc, k_cn, work_dtype, chunk, cn_path, topology)
        out["topology"] = topo if nsys == 1 else None
        out["energy"][s] = e
        out["forces"][sel] = f
        out["cn"][sel] = c
        out["triples"] += triples
        out["kept"] = max(out["kept"], kept)
        if out["virial"] is not None:
            out["virial"][s] = v
    return out
