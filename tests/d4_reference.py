"""Float64 torch restatement of the two-body DFT-D4 energy with charge-dependent C6: the checker of `dftd4`.

Written from the definition (include/nvalchemiops_hip.h, `dftd4`'s docstring), not from the kernel.  Pairs come from
`atm_reference.enumerate_pairs` (explicit enumeration of atom images); the energy is one differentiable scalar per system; forces (at
fixed charges, through the coordination numbers as well), dE/dq and the virial come by autograd -- the virial as minus the derivative with
respect to a symmetric strain applied to positions and cell, as `atm_reference` does it.  Small systems only.

    CN_i    = sum_row delta(Z_i,Z_j) 1/2 (1 + erf(-k_cn (r / (rcov_i + rcov_j) - 1))),  delta = k4 exp(-(|en_i - en_j| + k5)^2 / k6)
    g_a     = sum_{s=1..ngw_a} exp(-wf s (CN_i - cn_ref_a)^2),  W_a = g_a / sum_b g_b   (the largest exponent is subtracted first)
    zeta_a  = exp(ga (1 - exp(gc gam (1 - (zeff + q_ref_a) / (zeff + q_i)))))  if zeff + q_i > 0,  else exp(ga)
    C6_ij   = sum_ab W_a zeta_a c6_ref[Z_i,Z_j,a,b] W_b zeta_b
    E       = 1/2 sum_entries -C6_ij (s6 / (r^6 + R0^6) + s8 Q / (r^8 + R0^8)),  Q = 3 r4r2_i r4r2_j,  R0 = a1 sqrt(Q) + a2

`work_dtype=torch.float32` evaluates every per-pair and per-atom quantity (and its derivative) in float32 while every SUM stays float64
-- the arithmetic model of the kernels; the distance between the two evaluations is what float32 arithmetic costs on a given system.
"""
import numpy as np
import torch

from tests import atm_reference as A
from tests import systems as S

N_REF = 7
K4, K5, K6 = 4.10451, 19.08857, 2.0 * 11.28174 ** 2
TABLE_KEYS = ("rcov", "en", "r4r2", "zeff", "gam", "n_ref", "ngw", "cn_ref", "q_ref", "c6_ref")
ONE_REF_Z, SEVEN_REF_Z = 1, 6  # the elements `d4_test_tables` gives one and seven references


def d4_test_tables(z_max: int = 17, seed: int = 0):
    """Synthetic D4 tables (numpy; float32 values, int32 counts): radii and r4r2 of `systems.d3_test_tables`, seeded electronegativities,
    hardnesses and reference charges, zeff = Z; n_ref from 1 to 7 with element 1 at one reference and element 6 at seven; ngw in {1, 3};
    cn_ref drawn from [0, 1] (the coordination numbers of the test systems: see the table-condition test); NaN in every entry with
    reference index >= n_ref; c6_ref positive with c6_ref[A,B,a,b] = c6_ref[B,A,b,a]."""
    nz = z_max + 1
    base = S.d3_test_tables(z_max, seed=seed + 1000)
    g = np.random.default_rng(seed)
    en = g.uniform(0.8, 3.5, nz).astype(np.float32)
    gam = g.uniform(0.2, 0.6, nz).astype(np.float32)
    zeff = np.arange(nz, dtype=np.float32)
    n_ref = g.integers(2, 7, nz).astype(np.int32)
    n_ref[0] = 0
    if nz > ONE_REF_Z:
        n_ref[ONE_REF_Z] = 1
    if nz > SEVEN_REF_Z:
        n_ref[SEVEN_REF_Z] = 7
    ngw = g.choice(np.array([1, 3], np.int32), (nz, N_REF)).astype(np.int32)
    cn_ref = g.uniform(0.0, 1.0, (nz, N_REF)).astype(np.float32)
    q_ref = g.uniform(-0.5, 0.5, (nz, N_REF)).astype(np.float32)
    raw = g.uniform(0.5, 1.5, (nz, nz, N_REF, N_REF))
    sym = 0.5 * (raw + raw.transpose(1, 0, 3, 2))
    zi = np.arange(nz, dtype=np.float64)
    a = np.arange(N_REF, dtype=np.float64)
    c6 = 10.0 * zi[:, None, None, None] * zi[None, :, None, None] * (1.0 + 0.1 * a[None, None, :, None] + 0.1 * a[None, None, None, :]) * sym
    c6 = c6.astype(np.float32)
    t = dict(rcov=base["rcov"].copy(), en=en, r4r2=base["r4r2"].copy(), zeff=zeff, gam=gam, n_ref=n_ref, ngw=ngw, cn_ref=cn_ref, q_ref=q_ref,
             c6_ref=c6)
    return blank_unused(t)


def blank_unused(t):
    """NaN into every entry of cn_ref / q_ref / c6_ref whose reference index is >= n_ref (after n_ref was edited, too).  In place; returns t."""
    beyond = np.arange(N_REF)[None, :] >= t["n_ref"][:, None]  # [nz,7]
    t["cn_ref"][beyond] = np.nan
    t["q_ref"][beyond] = np.nan
    t["c6_ref"][beyond[:, None, :, None] | beyond[None, :, None, :]] = np.nan
    return t


def gaussian_weights(cn, z, tables, wf=6.0, wd=torch.float64):
    """W[n,7] of atoms with coordination numbers `cn` (tensor [n], dtype wd) and atomic numbers `z` (long [n]; all inside the tables with
    n_ref > 0): max-shifted, zero beyond n_ref."""
    n_ref = torch.as_tensor(tables["n_ref"], dtype=torch.long)[z]
    mask = torch.arange(N_REF)[None, :] < n_ref[:, None]
    cnr = torch.as_tensor(np.nan_to_num(tables["cn_ref"]), dtype=wd)[z]
    ngw = torch.as_tensor(tables["ngw"], dtype=torch.long)[z]
    d2 = (cn[:, None] - cnr) ** 2
    ex = torch.where(mask, -wf * d2, torch.full_like(d2, -float("inf")))
    m = ex.max(dim=1, keepdim=True).values.detach()
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))  # (an atom without references: all weights 0, not 0/0)
    g = torch.zeros_like(d2)
    for s in (1, 2, 3):
        inc = mask & (ngw >= s)
        g = g + torch.where(inc, torch.exp(torch.where(inc, -wf * s * d2 - m, torch.zeros_like(d2))), torch.zeros_like(d2))
    norm = g.sum(dim=1, keepdim=True)
    return g / torch.where(norm > 0, norm, torch.ones_like(norm)), mask


def charge_scaling(q, z, tables, ga=3.0, gc=2.0, wd=torch.float64):
    """zeta[n,7] (unmasked beyond n_ref: multiply by a masked W)."""
    zeff = torch.as_tensor(tables["zeff"], dtype=wd)[z][:, None]
    gam = torch.as_tensor(tables["gam"], dtype=wd)[z][:, None]
    qref = torch.as_tensor(np.nan_to_num(tables["q_ref"]), dtype=wd)[z]
    zq = zeff + q[:, None]
    pos = zq > 0
    safe = torch.where(pos, zq, torch.ones_like(zq))
    inner = torch.exp(gc * gam * (1.0 - (zeff + qref) / safe))
    return torch.where(pos, torch.exp(ga * (1.0 - inner)), torch.exp(torch.full_like(inner, ga)))


def valid_atoms(numbers, tables):
    z = np.asarray(numbers)
    nz = len(tables["rcov"])
    ok = (z > 0) & (z < nz)
    ok[ok] = np.asarray(tables["n_ref"])[z[ok]] > 0
    return ok


def _system(pos, numbers, charges, tables, cell, a1, a2, s8, s6, list_cutoff, cn_cutoff, wf, ga, gc, k_cn, wd, pairs):
    """One system: (energy, forces[N,3], virial[3,3] or None, cn[N], dE/dq[N], W[N,7]) as float64 numpy."""
    f64 = torch.float64
    n = len(pos)
    ok = valid_atoms(numbers, tables)
    z = torch.as_tensor(np.where(ok, np.asarray(numbers), 0), dtype=torch.long)
    x0 = torch.tensor(np.asarray(pos, np.float64), dtype=f64, requires_grad=True)
    q0 = torch.tensor(np.asarray(charges, np.float64), dtype=f64, requires_grad=True)
    eps = torch.zeros(3, 3, dtype=f64, requires_grad=True)
    strain = torch.eye(3, dtype=f64) + 0.5 * (eps + eps.T)
    x = x0 @ strain
    h = None if cell is None else torch.as_tensor(np.asarray(cell, np.float64).reshape(3, 3)) @ strain
    li, lj, ls = A.enumerate_pairs(pos, cell, list_cutoff) if pairs is None else pairs
    keep = ok[li] & ok[lj]
    li, lj, ls = li[keep], lj[keep], ls[keep]
    ti, tj = torch.as_tensor(li, dtype=torch.long), torch.as_tensor(lj, dtype=torch.long)
    d = x[tj] - x[ti]
    if h is not None:
        d = d + torch.as_tensor(ls, dtype=f64) @ h
    r = d.to(wd).norm(dim=1)  # float64 difference (+ shift), then the working dtype -- as the kernels cast
    live = (r > 1e-8).detach()
    zi, zj = z[ti], z[tj]
    tab = lambda k: torch.as_tensor(tables[k], dtype=wd)  # noqa: E731
    rcov, en, r4r2 = tab("rcov"), tab("en"), tab("r4r2")
    # coordination numbers
    delta = K4 * torch.exp(-(torch.abs(en[zi] - en[zj]) + K5) ** 2 / K6)
    count = delta * 0.5 * (1.0 + torch.erf(-k_cn * (r / (rcov[zi] + rcov[zj]) - 1.0)))
    counted = live if cn_cutoff is None else live & (r < cn_cutoff).detach()
    count = torch.where(counted, count, torch.zeros_like(count))
    cn64 = torch.zeros(n, dtype=f64).index_add(0, ti, count.to(f64))
    cn = cn64.to(wd)
    # weights (atoms outside the tables: all zero)
    W, mask = gaussian_weights(cn, z, tables, wf, wd)
    zeta = charge_scaling(q0.to(wd), z, tables, ga, gc, wd)
    atom_ok = torch.as_tensor(ok)[:, None]
    w = torch.where(mask & atom_ok, torch.where(mask & atom_ok, W, torch.zeros_like(W)) * zeta, torch.zeros_like(W))
    # energy
    c6r = torch.as_tensor(np.nan_to_num(tables["c6_ref"]), dtype=wd)[zi, zj]
    c6 = torch.einsum("pa,pab,pb->p", w[ti], c6r, w[tj])
    Q = 3.0 * r4r2[zi] * r4r2[zj]
    r0 = a1 * torch.sqrt(Q) + a2
    e = -c6 * (s6 / (r ** 6 + r0 ** 6) + s8 * Q / (r ** 8 + r0 ** 8))
    e = torch.where(live, e, torch.zeros_like(e))
    total = 0.5 * e.to(f64).sum()
    if total.requires_grad:
        total.backward()
    forces = -x0.grad.numpy() if x0.grad is not None else np.zeros((n, 3))
    dq = q0.grad.numpy() if q0.grad is not None else np.zeros(n)
    virial = None
    if cell is not None:
        virial = -eps.grad.numpy() if eps.grad is not None else np.zeros((3, 3))
        virial = 0.5 * (virial + virial.T)
    Wn = torch.where(mask & atom_ok, W, torch.zeros_like(W)).detach().to(f64).numpy()
    return float(total.detach()), forces, virial, cn64.detach().numpy(), dq, Wn


def reference(pos, numbers, charges, tables, a1, a2, s8, list_cutoff, s6=1.0, cn_cutoff=None, wf=6.0, ga=3.0, gc=2.0, k_cn=7.5, cell=None,
              batch_idx=None, work_dtype=torch.float64, pairs=None):
    """Returns dict(energy[B], forces[N,3], virial[B,3,3] (periodic only, else None), cn[N], charge_grad[N], weights[N,7] (the Gaussian
    weights W)) as float64 numpy arrays.  `cell`: None, [3,3] or [B,3,3]; `batch_idx`: None or [N] (systems are evaluated one by one).
    `pairs` (single system only): an `enumerate_pairs` triple to use instead of enumerating at `list_cutoff` -- finite differences keep the
    list of the undisplaced system."""
    pos = np.asarray(pos, np.float64)
    numbers = np.asarray(numbers)
    charges = np.asarray(charges, np.float64)
    n = len(pos)
    bi = np.zeros(n, np.int64) if batch_idx is None else np.asarray(batch_idx, np.int64)
    cells = None if cell is None else np.asarray(cell, np.float64).reshape(-1, 3, 3)
    nsys = (int(bi.max()) + 1 if n else 1) if cells is None else len(cells)
    assert pairs is None or nsys == 1
    out = dict(energy=np.zeros(nsys), forces=np.zeros((n, 3)), virial=None if cells is None else np.zeros((nsys, 3, 3)), cn=np.zeros(n),
               charge_grad=np.zeros(n), weights=np.zeros((n, N_REF)))
    for s in range(nsys):
        sel = np.nonzero(bi == s)[0]
        if len(sel) == 0:
            continue
        e, f, v, c, dq, W = _system(pos[sel], numbers[sel], charges[sel], tables, None if cells is None else cells[s], a1, a2, s8, s6,
                                    list_cutoff, cn_cutoff, wf, ga, gc, k_cn, work_dtype, pairs)
        out["energy"][s] = e
        out["forces"][sel] = f
        out["cn"][sel] = c
        out["charge_grad"][sel] = dq
        out["weights"][sel] = W
        if out["virial"] is not None:
            out["virial"][s] = v
    return out
