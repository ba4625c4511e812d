"""Float64 torch restatement of DFT-D3 with the three-body (Axilrod-Teller-Muto) term: the checker of `dftd3_atm`.

Written from the definition of the term and from the reference's two-body formulas (interactions/dispersion/dftd3.py: `_cn_counting`
:608-645, `_c6ab_interpolate` :427-547, `_bj_damping` :648-687), not from the kernel.  Explicit enumeration of atom images, energy as one
differentiable scalar per system, forces by autograd through the positions INCLUDING the coordination-number dependence of C6, virial as
minus the derivative with respect to a symmetric strain applied to positions and cell.  Small systems only (every pair of atoms times
every lattice shift within reach is formed).

    reference(pos, numbers, tables, a1, a2, list_cutoff, ..., term="atm" | "two_body", work_dtype=torch.float64 | torch.float32)

`list_cutoff` is the cutoff of the neighbour list the coordination numbers are summed over (all pairs closer than it),
`three_body_cutoff` the bound on the three sides of a triple.  `work_dtype=torch.float32` evaluates every per-pair / per-triple quantity
(and its derivative) in float32 while every SUM stays float64 -- the arithmetic model of the kernels; the distance between the two
evaluations is what float32 pair arithmetic costs on a given system.

Three-body term, for every unordered triple of distinct atom images A, B, C with all three distances < three_body_cutoff:
    C9 = sqrt(C6_AB C6_AC C6_BC)                  (nothing if any C6 < 1e-12)
    R0_XY = a1 sqrt(3 r4r2_X r4r2_Y) + a2,  a, b, c = r_AB^2, r_AC^2, r_BC^2,  P = r_AB r_AC r_BC
    ang = 0.375 (a + b - c)(a + c - b)(b + c - a) / P^5 + 1 / P^3
    E_ABC = s9 C9 ang / (1 + 6 (R0_AB R0_AC R0_BC / P)^(alpha / 3))
A triple counts once per lattice-translation class: the sum runs over (centre atom in the home cell, unordered pair of its neighbour
images), which meets every class exactly three times, and is divided by three.  Free molecules: each triple i < j < k once.
"""
import itertools

import numpy as np
import torch


def lattice_box(n=(4, 5, 5), a=4.2, jitter=0.25, seed=3, triclinic=True, dtype=np.float32):
    """Test system: a jittered simple lattice (spacing `a` Bohr) in a triclinic (or cubic) cell -- interatomic distances of a condensed
    phase (>= ~3 Bohr), unlike uniformly random positions, whose sub-Bohr contacts make fp32 pair terms orders of magnitude larger than
    the sums they cancel to.  Returns (positions [N,3], cell [3,3])."""
    g = np.random.default_rng(seed)
    n = np.asarray(n)
    if triclinic:
        cell = np.array([[n[0] * a, 0, 0], [0.25 * n[1] * a, 0.9 * n[1] * a, 0], [0.1 * n[2] * a, -0.2 * n[2] * a, 1.1 * n[2] * a]])
    else:
        cell = np.diag(n * a).astype(np.float64)
    ijk = np.stack(np.meshgrid(*[np.arange(k) for k in n], indexing="ij"), -1).reshape(-1, 3)
    pos = ((ijk + 0.5) / n) @ cell + g.normal(0.0, jitter, (len(ijk), 3))
    return pos.astype(dtype), cell.astype(dtype)


def centre_and_shell(m, radius=19.0, jitter=0.2, seed=29):
    """Test system with ONE long row: atom 0 at the origin and m atoms on a Fibonacci sphere of `radius` Bohr around it, every coordinate
    moved by up to +-jitter.  With a three-body cutoff just above the radius the centre keeps all m, a shell atom only its cap of the
    sphere -- a row of many LDS tiles of the triple pass at a cost the float64 restatement can pay (a cluster in which EVERY row is that
    long costs it m^3 / 6 triples).  Returns positions [m + 1, 3], float32."""
    k = np.arange(m) + 0.5
    ct = 1.0 - 2.0 * k / m
    st = np.sqrt(1.0 - ct * ct)
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    shell = radius * np.stack([st * np.cos(phi), st * np.sin(phi), ct], 1) + np.random.default_rng(seed).uniform(-jitter, jitter, (m, 3))
    return np.concatenate([np.zeros((1, 3)), shell]).astype(np.float32)


def kept_and_triples(pos, cutoff):
    """Of a free system, from numpy distances: (entries each row keeps inside `cutoff` [N], shell pairs of atom 0 = pairs of its kept
    entries that are themselves closer than `cutoff`, unordered triples with all three sides inside `cutoff`, the smallest |distance -
    cutoff| of any pair -- a float32 kernel and this count agree only while that is far above float32 rounding)."""
    pos = np.asarray(pos, np.float64)
    d = np.linalg.norm(pos[:, None, :] - pos[None, :, :], axis=2)
    a = ((d < cutoff) & (d > 0)).astype(np.float64)  # (counts below 2^53: exact in float64, and a BLAS product)
    on0 = a[0] > 0
    pairs0 = int(a[np.ix_(on0, on0)].sum()) // 2
    triples = int(round(((a @ a) * a).sum())) // 6
    return a.sum(1).astype(np.int64), pairs0, triples, float(np.abs(d - cutoff).min())


def enumerate_pairs(pos, cell, cutoff):
    """All ordered pairs (i, j, integer shift) with 1e-12 <= |r_j + shift.cell - r_i| < cutoff, i's image in the home cell; sorted by i.
    `cell` None: free space (shift 0)."""
    pos = np.asarray(pos, np.float64)
    n = len(pos)
    if cell is None:
        shifts = np.zeros((1, 3), np.int64)
        cart = np.zeros((1, 3))
    else:
        cell = np.asarray(cell, np.float64).reshape(3, 3)
        inv = np.linalg.inv(cell)
        heights = 1.0 / np.linalg.norm(inv, axis=0)  # distance between opposite faces
        frac = pos @ inv
        spread = frac.max(0) - frac.min(0) if n else np.zeros(3)  # atoms need not be wrapped into the cell
        reach = [int(np.ceil(cutoff / heights[d] + spread[d])) for d in range(3)]
        shifts = np.array(list(itertools.product(*[range(-r, r + 1) for r in reach])), np.int64)
        cart = shifts @ cell
    out_i, out_j, out_s = [], [], []
    for s, c in zip(shifts, cart):
        d = pos[None, :, :] + c[None, None, :] - pos[:, None, :]
        r2 = (d * d).sum(-1)
        m = (r2 < cutoff * cutoff) & (r2 >= 1e-24)
        i, j = np.nonzero(m)
        out_i.append(i); out_j.append(j); out_s.append(np.broadcast_to(s, (len(i), 3)))
    i = np.concatenate(out_i); j = np.concatenate(out_j); s = np.concatenate(out_s)
    order = np.lexsort((s[:, 2], s[:, 1], s[:, 0], j, i))
    return i[order], j[order], s[order]


def neighbor_matrix_of(i, j, s, n):
    """Padded matrix / shifts (fill value n) of an `enumerate_pairs` list, for feeding the SAME list to another implementation."""
    counts = np.bincount(i, minlength=n)
    m = max(int(counts.max()) if n else 0, 1)
    nm = np.full((n, m), n, np.int32)
    sh = np.zeros((n, m, 3), np.int32)
    start = np.concatenate([[0], np.cumsum(counts)])
    col = np.arange(len(i)) - start[i]
    nm[i, col] = j
    sh[i, col] = s
    return nm, sh


def c6_interpolate(cn_x, cn_y, zx, zy, c6ab, cn_ref, k3):
    """`_c6ab_interpolate` for arrays of pairs: 5x5 Gaussian weights in CN, zero-C6 reference entries skipped, max-shifted exponent, terms
    below -12 dropped; cn_ref[Zx,Zy][p,q] for X and cn_ref[Zy,Zx][q,p] for Y."""
    c6r = c6ab[zx, zy]                                   # [P,5,5]
    rx = cn_ref[zx, zy]
    ry = cn_ref[zy, zx].transpose(1, 2)
    arg = k3 * ((cn_x[:, None, None] - rx) ** 2 + (cn_y[:, None, None] - ry) ** 2)
    valid = c6r != 0
    arg = torch.where(valid, arg, torch.full_like(arg, -float("inf")))
    mx = arg.reshape(len(arg), -1).max(1).values.detach()
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    rel = arg - mx[:, None, None]
    keep = valid & (rel >= -12.0)
    L = torch.where(keep, torch.exp(torch.where(keep, rel, torch.zeros_like(rel))), torch.zeros_like(rel))
    w = L.sum((1, 2))
    z = (c6r * L).sum((1, 2))
    ok = w > 1e-12
    return torch.where(ok, z / torch.where(ok, w, torch.ones_like(w)), torch.zeros_like(w))


def _system(pos, numbers, tables, cell, a1, a2, list_cutoff, three_body_cutoff, s9, alpha, k1, k3, s6, s8, term, wd, chunk):
    """One system: (energy, forces[N,3], virial[3,3] or None, cn[N]) as float64 numpy, and the number of triples enumerated (term "atm")."""
    f64 = torch.float64
    n = len(pos)
    z = torch.as_tensor(np.asarray(numbers), dtype=torch.long)
    rcov = torch.as_tensor(tables["rcov"], dtype=wd)
    r4r2 = torch.as_tensor(tables["r4r2"], dtype=wd)
    c6ab = torch.as_tensor(tables["c6ab"], dtype=wd)
    cn_ref = torch.as_tensor(tables["cn_ref"], dtype=wd)
    nz = len(rcov)
    real_np = (np.asarray(numbers) > 0) & (np.asarray(numbers) < nz)
    x0 = torch.tensor(np.asarray(pos, np.float64), dtype=f64, requires_grad=True)
    eps = torch.zeros(3, 3, dtype=f64, requires_grad=True)
    strain = torch.eye(3, dtype=f64) + 0.5 * (eps + eps.T)
    x = x0 @ strain
    h = None if cell is None else torch.as_tensor(np.asarray(cell, np.float64).reshape(3, 3)) @ strain

    def vectors(i, j, s):  # pair vectors: float64 difference (+ shift), then the working dtype -- as the kernels cast
        d = x[j] - x[i]
        if h is not None:
            d = d + torch.as_tensor(s, dtype=f64) @ h
        return d.to(wd)

    # coordination numbers over the whole list
    li, lj, ls = enumerate_pairs(pos, cell, list_cutoff)
    m = real_np[li] & real_np[lj]
    li, lj, ls = li[m], lj[m], ls[m]
    tli, tlj = torch.as_tensor(li), torch.as_tensor(lj)
    rl = vectors(li, lj, ls).norm(dim=1)
    count = 1.0 / (1.0 + torch.exp(-k1 * ((rcov[z[tli]] + rcov[z[tlj]]) / rl - 1.0)))
    cn64 = torch.zeros(n, dtype=f64).index_add(0, tli, count.to(f64))
    cn = cn64.to(wd)

    def r0_of(za, zb):
        return a1 * torch.sqrt(3.0 * r4r2[za] * r4r2[zb]) + a2

    total = torch.zeros((), dtype=f64)
    triples = 0
    if term == "two_body":
        c6 = c6_interpolate(cn[tli], cn[tlj], z[tli], z[tlj], c6ab, cn_ref, k3)
        q = 3.0 * r4r2[z[tli]] * r4r2[z[tlj]]
        r0 = a1 * torch.sqrt(q) + a2
        e = -c6 * (s6 / (rl ** 6 + r0 ** 6) + s8 * q / (rl ** 8 + r0 ** 8))
        e = torch.where(c6 < 1e-12, torch.zeros_like(e), e)
        total = 0.5 * e.to(f64).sum()
        total.backward()
    else:
        keep = np.linalg.norm(_np_vectors(pos, cell, li, lj, ls), axis=1) < three_body_cutoff
        ti, tj, ts = li[keep], lj[keep], ls[keep]
        vec_np = _np_vectors(pos, cell, ti, tj, ts)
        counts = np.bincount(ti, minlength=n)
        start = np.concatenate([[0], np.cumsum(counts)])
        vp, vq = [], []
        free = cell is None
        for c in range(n):
            k = counts[c]
            if k < 2:
                continue
            p, q = np.triu_indices(k, 1)
            p = p + start[c]; q = q + start[c]
            djk = vec_np[q] - vec_np[p]
            r2 = (djk * djk).sum(1)
            ok = (r2 < three_body_cutoff ** 2) & (r2 >= 1e-24)
            if free:  # each triple once: centre < j < k (rows are sorted by j)
                ok &= tj[p] > c
            vp.append(p[ok]); vq.append(q[ok])
        vp = np.concatenate(vp) if vp else np.zeros(0, np.int64)
        vq = np.concatenate(vq) if vq else np.zeros(0, np.int64)
        weight = 1.0 if free else 1.0 / 3.0
        triples = len(vp) if free else len(vp) // 3  # (periodic: every triple is enumerated from each of its three vertices)
        tti, ttj = torch.as_tensor(ti), torch.as_tensor(tj)
        total_val = 0.0
        for lo in range(0, max(len(vp), 1), chunk):
            p = torch.as_tensor(vp[lo:lo + chunk]); q = torch.as_tensor(vq[lo:lo + chunk])
            if len(p) == 0:
                break
            # (pair quantities are re-derived per chunk so that each chunk's graph can be freed after its backward pass)
            R = vectors(ti, tj, ts)
            c6_pair = c6_interpolate(cn[tti], cn[ttj], z[tti], z[ttj], c6ab, cn_ref, k3)
            r0_pair = r0_of(z[tti], z[ttj])
            cj, ck = ttj[p], ttj[q]
            rij, rik = R[p], R[q]
            rjk = rik - rij
            a = (rij * rij).sum(1); b = (rik * rik).sum(1); c = (rjk * rjk).sum(1)
            P = torch.sqrt(a) * torch.sqrt(b) * torch.sqrt(c)
            c6_ij, c6_ik = c6_pair[p], c6_pair[q]
            c6_jk = c6_interpolate(cn[cj], cn[ck], z[cj], z[ck], c6ab, cn_ref, k3)
            live = (c6_ij >= 1e-12) & (c6_ik >= 1e-12) & (c6_jk >= 1e-12)
            one = torch.ones_like(c6_ij)
            c9 = torch.sqrt(torch.where(live, c6_ij, one) * torch.where(live, c6_ik, one) * torch.where(live, c6_jk, one))
            ang = 0.375 * (a + b - c) * (a + c - b) * (b + c - a) / P ** 5 + 1.0 / P ** 3
            r0 = r0_pair[p] * r0_pair[q] * r0_of(z[cj], z[ck])
            fdamp = 1.0 / (1.0 + 6.0 * (r0 / P) ** (alpha / 3.0))
            e = torch.where(live, s9 * c9 * ang * fdamp, torch.zeros_like(ang))
            part = weight * e.to(f64).sum()
            part.backward(retain_graph=True)
            total_val += float(part.detach())
        total = torch.tensor(total_val, dtype=f64)
    forces = -x0.grad.numpy() if x0.grad is not None else np.zeros((n, 3))
    virial = None
    if cell is not None:
        virial = -eps.grad.numpy() if eps.grad is not None else np.zeros((3, 3))
        virial = 0.5 * (virial + virial.T)
    return float(total.detach()), forces, virial, cn64.detach().numpy(), triples


def _np_vectors(pos, cell, i, j, s):
    pos = np.asarray(pos, np.float64)
    d = pos[j] - pos[i]
    if cell is not None:
        d = d + s @ np.asarray(cell, np.float64).reshape(3, 3)
    return d


def reference(pos, numbers, tables, a1, a2, list_cutoff, three_body_cutoff=None, s9=1.0, alpha=16.0, k1=16.0, k3=-4.0, s6=1.0, s8=0.0,
              cell=None, batch_idx=None, term="atm", work_dtype=torch.float64, chunk=1_000_000):
    """Returns dict(energy[B], forces[N,3], virial[B,3,3] (periodic only, else None), cn[N]) as float64 numpy arrays, and `triples`: the
    unordered triples the three-body term summed over (0 for term "two_body").
    `cell`: None, [3,3] or [B,3,3]; `batch_idx`: None or [N] (systems are evaluated one by one)."""
    pos = np.asarray(pos, np.float64)
    numbers = np.asarray(numbers)
    n = len(pos)
    bi = np.zeros(n, np.int64) if batch_idx is None else np.asarray(batch_idx, np.int64)
    cells = None if cell is None else np.asarray(cell, np.float64).reshape(-1, 3, 3)
    nsys = (int(bi.max()) + 1 if n else 1) if cells is None else len(cells)
    energy = np.zeros(nsys)
    forces = np.zeros((n, 3))
    cn = np.zeros(n)
    virial = None if cells is None else np.zeros((nsys, 3, 3))
    triples = 0
    for s in range(nsys):
        sel = np.nonzero(bi == s)[0]
        if len(sel) == 0:
            continue
        e, f, v, c, k = _system(pos[sel], numbers[sel], tables, None if cells is None else cells[s], a1, a2, list_cutoff,
                                three_body_cutoff if three_body_cutoff is not None else list_cutoff, s9, alpha, k1, k3, s6, s8, term, work_dtype,
                                chunk)
        energy[s] = e
        forces[sel] = f
        cn[sel] = c
        triples += k
        if virial is not None:
            virial[s] = v
    return dict(energy=energy, forces=forces, virial=virial, cn=cn, triples=triples)
