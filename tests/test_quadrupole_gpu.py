"""The point-quadrupole Ewald term on the device against the float64 restatement of its operator definition (tests/quadrupole_reference.py,
itself checked in tests/test_quadrupole_reference_cpu.py) on the same stored entries and the same k set.

The bars are those of tests/test_dipole_gpu.py for the same arithmetic model.  fp64 inputs: kernels and reference are fp64 throughout and differ
by summation order and the last bits of erfc / exp / sincos only: 1e-11 of the largest |value| per output.  fp32 inputs: pair vector and distance
in fp32, the rest fp64, against the reference's float32-distance mode at 1e-6 of the largest |value|.

Zero quadrupoles: energies, forces, charge_grads, dipole_grads and virial are exactly 0.0.  quadrupole_grads is dE/dQ, the field gradient of the
charges and dipoles at the atom: it does not vanish and is checked against the reference instead.

MEASURED on one MI355X (every test prints its figures under `pytest -s`; DESIGN.md section 3.24 has the table): float64 outputs 6.0e-14 of the
largest |value| at worst (the real-space virial; everything else below 3e-15), float32 3.7e-7, against the bars 1e-11 and 1e-6.  The CPU
closed-form-versus-autograd error of the same expansion is 3.0e-15 (tests/test_quadrupole_reference_cpu.py)."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import quadrupole_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("energies", "forces", "charge_grads", "dipole_grads", "quadrupole_grads", "virial")
ALL = dict(compute_forces=True, compute_charge_gradients=True, compute_dipole_gradients=True, compute_quadrupole_gradients=True,
           compute_virial=True)
GRADS = dict(compute_forces=True, compute_charge_gradients=True, compute_dipole_gradients=True, compute_quadrupole_gradients=True)


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV) if dtype is None else torch.as_tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


def _np(x):
    return x.detach().cpu().numpy().astype(np.float64)


def _close(got, ref, what, rel=1e-11):
    got = _np(got) if isinstance(got, torch.Tensor) else got
    ref = _np(ref) if isinstance(ref, torch.Tensor) else ref
    assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
    scale = max(np.abs(ref).max(), 1e-30) if ref.size else 1.0
    err = np.abs(got - ref).max() if ref.size else 0.0
    print(f"{what:56s} rel err {err / scale:.2e} (bar {rel:.0e})")
    assert err <= rel * scale + 1e-14, f"{what}: max err {err:.3e} > {rel * scale:.3e}"
    return err / scale


def _system(n, seed, box, triclinic=True, no_dipole=3, no_quadrupole=3, unsymmetric=4):
    g = np.random.default_rng(seed)
    cell = np.eye(3) * box
    if triclinic:
        cell = np.array([[box, 0, 0], [0.2 * box, 0.9 * box, 0], [0.1 * box, -0.15 * box, 1.1 * box]])
    pos = g.uniform(0, 1, (n, 3)) @ cell
    q = g.normal(size=n) + 0.05  # a charged box
    mu = 0.4 * g.normal(size=(n, 3))
    qd = 0.3 * g.normal(size=(n, 3, 3))
    qd = 0.5 * (qd + qd.transpose(0, 2, 1))  # traced, symmetric
    pick = g.permutation(n)
    if no_dipole:
        mu[pick[:min(no_dipole, n)]] = 0.0
    if no_quadrupole and n > no_dipole:
        qd[pick[no_dipole:no_dipole + no_quadrupole]] = 0.0  # other atoms than the ones without a dipole: every pair term shows alone
    if unsymmetric and n > 16:
        rows = pick[-unsymmetric:]
        skew = 0.1 * g.normal(size=(unsymmetric, 3, 3))
        qd[rows] += skew - skew.transpose(0, 2, 1)  # 1/2 (Q + Q^T) is what counts
    return pos, cell, q, mu, qd


def _lists(pos, cell, cutoff, batch_idx=None, batch_ptr=None, max_neighbors=400):
    from nvalchemiops.neighborlist import neighbor_list

    cells = _t(cell).reshape(-1, 3, 3)
    pbc = torch.ones((cells.shape[0], 3), dtype=torch.bool, device=DEV)
    kw = dict(batch_idx=batch_idx, batch_ptr=batch_ptr, method="batch_cell_list") if batch_idx is not None else dict(method="cell_list")
    nm, num, sh = neighbor_list(_t(pos), cutoff, cell=cells, pbc=pbc, max_neighbors=max_neighbors, **kw)
    assert int(num.max()) <= max_neighbors
    nl, ptr, lsh = neighbor_list(_t(pos), cutoff, cell=cells, pbc=pbc, max_neighbors=max_neighbors, return_neighbor_list=True, **kw)
    return nm, num, sh, nl, ptr, lsh


def _k_vectors(cells, k_cutoff):
    from nvalchemiops.interactions.electrostatics import generate_k_vectors_ewald_summation

    return generate_k_vectors_ewald_summation(cells, k_cutoff)


def _fmt_kw(f, fmt):
    if fmt == "matrix":
        return dict(neighbor_matrix=f["nm"], neighbor_matrix_shifts=f["sh"], mask_value=f["n"])
    return dict(neighbor_list=f["nl"], neighbor_ptr=f["ptr"], neighbor_shifts=f["lsh"])


def _csr(ei, ej, eS, n):
    """(neighbor_list, neighbor_ptr, neighbor_shifts) of entries in any order."""
    order = torch.argsort(ei, stable=True)
    ptr = torch.zeros(n + 1, dtype=torch.int32, device=ei.device)
    ptr[1:] = torch.cumsum(torch.bincount(ei, minlength=n), 0)
    return dict(neighbor_list=torch.stack([ei, ej])[:, order].int(), neighbor_ptr=ptr, neighbor_shifts=eS[order].int())


ALPHA = 0.45


def _sum(a, b):
    return {k: a[k] + b[k] for k in a}


@functools.lru_cache(maxsize=None)
def _single():
    """The parity case: 300 atoms, triclinic box of edge 12, charged, three atoms without a dipole and three others without a quadrupole, four
    with an unsymmetric quadrupole array, cutoff 7 (rows longer than 64 entries: several trips of the wave plus a tail), both list formats,
    K = 544 k-vectors (> 256, not a multiple of 64).  The reference is computed once per half; the total is their sum."""
    pos, cell, q, mu, qd = _system(300, seed=5, box=12.0)
    assert abs(q.sum()) > 1.0
    nm, num, sh, nl, ptr, lsh = _lists(pos, cell, 7.0)
    assert int(num.min()) > 64 and bool((num % 64 != 0).any())
    P, Q, M, T, C = _t(pos), _t(q), _t(mu), _t(qd), _t(cell).reshape(1, 3, 3)
    kv = _k_vectors(C, 2.2)
    assert kv.shape[0] > 256 and kv.shape[0] % 64 != 0, kv.shape
    n = pos.shape[0]
    A = torch.tensor([ALPHA], dtype=torch.float64, device=DEV)
    entries = R.entries_from_matrix(nm, sh, n)
    f = dict(P=P, Q=Q, M=M, T=T, C=C, A=A, kv=kv, nm=nm, sh=sh, nl=nl, ptr=ptr, lsh=lsh, n=n, entries=entries)
    f["ref_real"] = R.evaluate(P, Q, M, T, C, A, entries, None)
    f["ref_recip"] = R.evaluate(P, Q, M, T, C, A, None, kv)
    f["ref"] = _sum(f["ref_real"], f["ref_recip"])
    return f


def _api():
    from nvalchemiops.interactions.electrostatics import (ewald_quadrupole_correction, ewald_quadrupole_real_space,
                                                          ewald_quadrupole_reciprocal_space)

    return ewald_quadrupole_correction, ewald_quadrupole_real_space, ewald_quadrupole_reciprocal_space


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------------------
def test_parity_fp64_matrix_and_csr():
    both, real, recip = _api()
    f = _single()
    outs = {}
    for fmt in ("matrix", "list"):
        out = both(f["P"], f["Q"], f["M"], f["T"], f["C"], f["A"], f["kv"], **_fmt_kw(f, fmt), **ALL)
        assert len(out) == 6 and all(o.dtype == torch.float64 for o in out)
        assert [tuple(o.shape) for o in out] == [(300,), (300, 3), (300,), (300, 3), (300, 3, 3), (1, 3, 3)]
        for name, o in zip(NAMES, out):
            _close(o, f["ref"][name], f"fp64 {fmt} total {name}")
        part = real(f["P"], f["Q"], f["M"], f["T"], f["C"], f["A"], **_fmt_kw(f, fmt), **ALL)
        for name, o in zip(NAMES, part):
            _close(o, f["ref_real"][name], f"fp64 {fmt} real space {name}")
        outs[fmt] = out
    rec = recip(f["P"], f["Q"], f["M"], f["T"], f["C"], f["kv"], f["A"], **ALL)
    for name, o in zip(NAMES, rec):
        _close(o, f["ref_recip"][name], f"fp64 reciprocal space {name}")
    for name, a, b in zip(NAMES, outs["matrix"], outs["list"]):
        _close(a, b, f"matrix vs CSR {name}", 1e-10)
    frc = outs["matrix"][1]
    assert float(frc.sum(0).abs().max()) <= 1e-9 * float(frc.abs().max()), "net force"
    for o in (outs["matrix"][4], part[4], rec[4]):
        assert torch.equal(o, o.transpose(-1, -2)), "quadrupole_grads is symmetric"
    # a subset of the outputs is the same numbers; alpha as a Python number is the same as a tensor
    e, qg = both(f["P"], f["Q"], f["M"], f["T"], f["C"], ALPHA, f["kv"], **_fmt_kw(f, "matrix"), compute_quadrupole_gradients=True)
    assert torch.equal(e, outs["matrix"][0]) and torch.equal(qg, outs["matrix"][4])
    e = both(f["P"], f["Q"], f["M"], f["T"], f["C"], f["A"], f["kv"], **_fmt_kw(f, "list"))
    assert isinstance(e, torch.Tensor) and torch.equal(e, outs["list"][0])
    e, frc2 = real(f["P"], f["Q"], f["M"], f["T"], f["C"], f["A"], **_fmt_kw(f, "list"), compute_forces=True)  # the other instantiation
    assert torch.equal(frc2, part[1]) and torch.equal(e, part[0])
    e2, cg2 = real(f["P"], f["Q"], f["M"], f["T"], f["C"], f["A"], **_fmt_kw(f, "list"), compute_charge_gradients=True)
    _close(e2, part[0], "energies without B5", 1e-15)
    assert torch.equal(cg2, part[2])


def test_parity_fp32_inputs():
    both, real, recip = _api()
    f = _single()
    P, Q, M, T, C, A = (f[k].float() for k in ("P", "Q", "M", "T", "C", "A"))
    kv = _k_vectors(C, 2.2)
    assert kv.dtype == torch.float32 and kv.shape == f["kv"].shape
    ref = _sum(R.evaluate(P, Q, M, T, C, A, f["entries"], None, distance_dtype=torch.float32), R.evaluate(P, Q, M, T, C, A, None, kv))
    for fmt in ("matrix", "list"):
        out = both(P, Q, M, T, C, A, kv, **_fmt_kw(f, fmt), **ALL)
        assert all(o.dtype == torch.float32 for o in out)
        for name, o in zip(NAMES, out):
            _close(o, ref[name], f"fp32 {fmt} total {name}", 1e-6)


# ---- 2. padding and self-images -----------------------------------------------------------------------------------------------------------
def test_self_images_padding_kinds_empty_row_wide_matrix_and_no_dipoles():
    both, real, recip = _api()
    n, cutoff, empty_row = 9, 7.0, 4
    pos, cell, q, mu, qd = _system(n, seed=9, box=5.0, no_dipole=1, no_quadrupole=1)
    i, j, S = R.brute_force_entries(pos, cell, cutoff, 3)
    assert int(((i == j) & (S != 0).any(-1)).sum()) > 0  # self-images: i = j entries with S != 0
    keep = (i != empty_row) & (j != empty_row)  # atom 4 leaves the list from both ends: its row is empty and the list stays full
    i, j, S = i[keep], j[keep], S[keep]
    counts = np.bincount(i.numpy(), minlength=n)
    width = int(counts.max()) + 7  # a caller matrix wider than needed
    mask = n
    fills = (mask, 1000, -5)  # the three kinds of padding: the mask value, an index >= N, a negative index
    nm = np.empty((n, width), dtype=np.int32)
    sh = np.zeros((n, width, 3), dtype=np.int32)
    g = np.random.default_rng(0)
    for a in range(n):
        nm[a] = [fills[(a + c) % 3] for c in range(width)]
        cols = np.sort(g.choice(width, counts[a], replace=False))  # padding sits between the entries, not only behind them
        nm[a, cols], sh[a, cols] = j[i == a].numpy(), S[i == a].numpy()
        sh[a, nm[a] < 0] = 7  # shifts of padding slots are never read
    assert counts[empty_row] == 0
    P, Q, M, T, C = _t(pos), _t(q), _t(mu), _t(qd), _t(cell).reshape(1, 3, 3)
    kv = _k_vectors(C, 3.0)
    NM, SH = _t(nm), _t(sh)
    ei, ej, eS = R.entries_from_matrix(NM, SH, mask)
    assert ei.shape[0] == int(counts.sum())
    ref = R.evaluate(P, Q, M, T, C, 0.5, (ei, ej, eS), kv)
    out = both(P, Q, M, T, C, 0.5, kv, neighbor_matrix=NM, neighbor_matrix_shifts=SH, mask_value=mask, **ALL)
    for name, o in zip(NAMES, out):
        _close(o, ref[name], f"9 atoms, matrix {name}")
    csr = both(P, Q, M, T, C, 0.5, kv, **_csr(ei, ej, eS, n), **ALL)
    for name, o in zip(NAMES, csr):
        _close(o, ref[name], f"9 atoms, CSR {name}")
    # the emptied row: only the reciprocal part is left for that atom
    rs = real(P, Q, M, T, C, 0.5, neighbor_matrix=NM, neighbor_matrix_shifts=SH, mask_value=mask, **ALL)
    assert all(float(o[empty_row].abs().max()) == 0.0 for o in rs[:5])
    # dipoles=None is zero dipoles, bit for bit
    none = both(P, Q, None, T, C, 0.5, kv, neighbor_matrix=NM, neighbor_matrix_shifts=SH, mask_value=mask, **ALL)
    zero = both(P, Q, torch.zeros_like(M), T, C, 0.5, kv, neighbor_matrix=NM, neighbor_matrix_shifts=SH, mask_value=mask, **ALL)
    assert all(torch.equal(a, b) for a, b in zip(none, zero))
    for fn_none, fn_zero in ((lambda: real(P, Q, None, T, C, 0.5, **_csr(ei, ej, eS, n), **ALL), lambda: real(P, Q, 0 * M, T, C, 0.5, **_csr(ei, ej, eS, n), **ALL)),
                             (lambda: recip(P, Q, None, T, C, kv, 0.5, **ALL), lambda: recip(P, Q, 0 * M, T, C, kv, 0.5, **ALL))):
        assert all(torch.equal(a, b) for a, b in zip(fn_none(), fn_zero()))


# ---- 3. ladders ---------------------------------------------------------------------------------------------------------------------------
ROWS = (0, 1, 63, 64, 65, 128, 129)


@functools.lru_cache(maxsize=None)
def _ladder():
    """Seven atoms whose rows hold exactly 0, 1, 63, 64, 65, 128 and 129 entries, in a FULL list built by hand: ladder atom t is paired with its
    number of distinct (filler atom, shift) combinations, and the filler rows hold the reversed entries (j, i, -S)."""
    n_fill = 40
    n = len(ROWS) + n_fill
    pos, cell, q, mu, qd = _system(n, seed=21, box=6.0, no_dipole=2, no_quadrupole=2)
    g = np.random.default_rng(22)
    shifts = np.array([(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)])
    combos = [(f, s) for f in range(len(ROWS), n) for s in range(27)]
    ei, ej, eS = [], [], []
    for t, length in enumerate(ROWS):
        for c in g.choice(len(combos), length, replace=False):
            f, s = combos[c]
            ei += [t, f]; ej += [f, t]; eS += [shifts[s], -shifts[s]]  # noqa: E702
    ei, ej, eS = _t(np.array(ei, np.int64)), _t(np.array(ej, np.int64)), _t(np.array(eS, np.int64))
    lists = _csr(ei, ej, eS, n)
    assert tuple(int(x) for x in (lists["neighbor_ptr"][1:] - lists["neighbor_ptr"][:-1])[:len(ROWS)]) == ROWS
    P, Q, M, T, C = _t(pos), _t(q), _t(mu), _t(qd), _t(cell).reshape(1, 3, 3)
    kv = _k_vectors(C, 4.5)
    assert kv.shape[0] >= 257, kv.shape
    return dict(P=P, Q=Q, M=M, T=T, C=C, kv=kv, lists=lists, entries=R.entries_from_csr(lists["neighbor_list"], lists["neighbor_ptr"],
                                                                                       lists["neighbor_shifts"]), n=n)


def test_row_length_ladder():
    both, real, recip = _api()
    f = _ladder()
    ref = R.evaluate(f["P"], f["Q"], f["M"], f["T"], f["C"], 0.3, f["entries"], None)
    out = real(f["P"], f["Q"], f["M"], f["T"], f["C"], 0.3, **f["lists"], **ALL)
    for name, o in zip(NAMES, out):
        _close(o, ref[name], f"rows of {ROWS} entries: {name}")
        if name != "virial":  # ... and on the ladder rows themselves, relative to their own largest value
            _close(o[1:len(ROWS)], ref[name][1:len(ROWS)], f"  the ladder rows alone: {name}")
    assert all(float(o[0].abs().max()) == 0.0 for o in out[:5])  # the row of no entries
    # the same entries as a matrix of the widest row, the ladder rows padded
    ptr = f["lists"]["neighbor_ptr"].long()
    width = int((ptr[1:] - ptr[:-1]).max())
    nm = torch.full((f["n"], width), f["n"], dtype=torch.int32, device=DEV)
    sh = torch.zeros((f["n"], width, 3), dtype=torch.int32, device=DEV)
    ei = f["entries"][0]
    col = torch.arange(ei.shape[0], device=DEV) - ptr[ei]
    nm[ei, col], sh[ei, col] = f["lists"]["neighbor_list"][1], f["lists"]["neighbor_shifts"]
    mat = real(f["P"], f["Q"], f["M"], f["T"], f["C"], 0.3, neighbor_matrix=nm, neighbor_matrix_shifts=sh, mask_value=f["n"], **ALL)
    for name, a, b in zip(NAMES, mat, out):
        _close(a, b, f"ladder as a matrix: {name}", 1e-13)


@pytest.mark.parametrize("n_k", [1, 63, 64, 65, 255, 256, 257])
def test_k_count_ladder(n_k):
    both, real, recip = _api()
    f = _ladder()
    kv = f["kv"][:n_k]
    ref = R.evaluate(f["P"], f["Q"], f["M"], f["T"], f["C"], 0.6, None, kv)
    out = recip(f["P"], f["Q"], f["M"], f["T"], f["C"], kv, 0.6, **ALL)
    for name, o in zip(NAMES, out):
        _close(o, ref[name], f"K = {n_k}: {name}")


def test_empty_k_set_is_the_self_term_alone():
    both, real, recip = _api()
    f = _single()
    none = recip(f["P"], f["Q"], f["M"], f["T"], f["C"], f["kv"][:0], f["A"], **ALL)
    Ts = 0.5 * (f["T"] + f["T"].transpose(-1, -2))
    tr = Ts.diagonal(dim1=-2, dim2=-1).sum(-1)
    c3, c5 = 4.0 * ALPHA**3 / (3.0 * math.sqrt(math.pi)), 4.0 * ALPHA**5 / (5.0 * math.sqrt(math.pi))
    eye = torch.eye(3, dtype=torch.float64, device=DEV)
    _close(none[0], c3 * f["Q"] * tr - c5 * (2.0 * (Ts * Ts).sum((-1, -2)) + tr * tr), "K = 0 energies: the self term alone", 1e-14)
    _close(none[2], c3 * tr, "K = 0 charge_grads", 1e-14)
    _close(none[4], (c3 * f["Q"] - 2.0 * c5 * tr)[:, None, None] * eye - 4.0 * c5 * Ts, "K = 0 quadrupole_grads", 1e-14)
    for k in (1, 3, 5):
        assert float(none[k].abs().max()) == 0.0, NAMES[k]
    total = both(f["P"], f["Q"], f["M"], f["T"], f["C"], f["A"], f["kv"][:0], **_fmt_kw(f, "matrix"), **ALL)
    for name, o in zip(NAMES, total):
        _close(o, f["ref_real"][name] + _np(none[NAMES.index(name)]), f"K = 0 total {name}")
    # the adjoint of the self term alone
    w = _t(np.random.default_rng(2).uniform(0.2, 1.8, f["n"]))
    leaves = [f[k].clone().requires_grad_(True) for k in ("P", "Q", "M", "T")]
    e = recip(*leaves, f["C"], f["kv"][:0], f["A"])
    gp, gq, gm, gt = torch.autograd.grad((e * w).sum(), leaves)
    assert float(gp.abs().max()) == 0.0 and float(gm.abs().max()) == 0.0
    _close(gq, w * none[2], "K = 0 dL/dq", 1e-15)
    _close(gt, w[:, None, None] * none[4], "K = 0 dL/dQ", 1e-15)


# ---- 4. batch -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch():
    """A ragged batch: 130 atoms triclinic, 90 atoms orthorhombic, and a one-atom system; per-system alpha."""
    p0, c0, q0, m0, t0 = _system(130, seed=7, box=9.0)
    p1, c1, q1, m1, t1 = _system(90, seed=8, box=8.0, triclinic=False)
    p2, c2, q2, m2, t2 = _system(1, seed=10, box=8.0, triclinic=False, no_dipole=0, no_quadrupole=0)
    parts = ((p0, c0, q0, m0, t0), (p1, c1, q1, m1, t1), (p2, c2, q2, m2, t2))
    pos, q, mu, qd = (np.concatenate([p[k] for p in parts]) for k in (0, 2, 3, 4))
    cells = np.stack([c0, c1, c2])
    bi = _t(np.concatenate([np.full(130, 0, np.int32), np.full(90, 1, np.int32), np.full(1, 2, np.int32)]))
    bptr = _t(np.array([0, 130, 220, 221], np.int32))
    nm, num, sh, nl, ptr, lsh = _lists(pos, cells, 6.0, batch_idx=bi, batch_ptr=bptr)
    assert int(num[220]) == 0
    C = _t(cells)
    A = torch.tensor([0.4, 0.5, 0.45], dtype=torch.float64, device=DEV)
    kv = _k_vectors(C, 2.4)
    assert kv.dim() == 3 and kv.shape[0] == 3
    return dict(P=_t(pos), Q=_t(q), M=_t(mu), T=_t(qd), C=C, A=A, kv=kv, bi=bi, nm=nm, sh=sh, nl=nl, ptr=ptr, lsh=lsh, n=221, parts=parts)


def test_batch_equals_single_calls_and_reference():
    both, real, recip = _api()
    b = _batch()
    ref = R.evaluate(b["P"], b["Q"], b["M"], b["T"], b["C"], b["A"], R.entries_from_matrix(b["nm"], b["sh"], b["n"]), b["kv"], batch_idx=b["bi"])
    got = {}
    for fmt in ("matrix", "list"):
        got[fmt] = both(b["P"], b["Q"], b["M"], b["T"], b["C"], b["A"], b["kv"], batch_idx=b["bi"], **_fmt_kw(b, fmt), **ALL)
        assert got[fmt][5].shape == (3, 3, 3)
        for name, o in zip(NAMES, got[fmt]):
            _close(o, ref[name], f"batch {fmt} {name}")
    bounds = (0, 130, 220, 221)
    for fmt in ("matrix", "list"):
        for s in range(3):
            p, c, q, m, t = b["parts"][s]
            sl = slice(bounds[s], bounds[s + 1])
            nm, num, sh, nl, ptr, lsh = _lists(p, c, 6.0)
            one = dict(nm=nm, sh=sh, nl=nl, ptr=ptr, lsh=lsh, n=p.shape[0])
            alone = both(_t(p), _t(q), _t(m), _t(t), _t(c).reshape(1, 3, 3), b["A"][s:s + 1], b["kv"][s], **_fmt_kw(one, fmt), **ALL)
            for name, o, a in zip(NAMES[:5], got[fmt][:5], alone[:5]):
                _close(o[sl], a, f"{fmt} system {s} alone: {name}", 1e-12)
            _close(got[fmt][5][s], alone[5][0], f"{fmt} system {s} alone: virial", 1e-12)


# ---- 5. linearity and zero quadrupoles ----------------------------------------------------------------------------------------------------
def test_zero_quadrupoles_give_exact_zeros():
    both, real, recip = _api()
    f = _single()
    zero = torch.zeros_like(f["T"])
    ref = _sum(R.evaluate(f["P"], f["Q"], f["M"], zero, f["C"], f["A"], f["entries"], None), R.evaluate(f["P"], f["Q"], f["M"], zero, f["C"], f["A"], None, f["kv"]))
    for fmt in ("matrix", "list"):
        for call in (lambda: both(f["P"], f["Q"], f["M"], zero, f["C"], f["A"], f["kv"], **_fmt_kw(f, fmt), **ALL),
                     lambda: both(f["P"].float(), f["Q"].float(), f["M"].float(), zero.float(), f["C"].float(), ALPHA, f["kv"].float(),
                                  **_fmt_kw(f, fmt), **ALL)):
            out = call()
            for k in (0, 1, 2, 3, 5):
                assert float(out[k].abs().max()) == 0.0 and not bool(torch.isnan(out[k]).any()), (fmt, NAMES[k])
        # the field gradient of the charges and dipoles: not zero, and the reference's
        out = both(f["P"], f["Q"], f["M"], zero, f["C"], f["A"], f["kv"], **_fmt_kw(f, fmt), **ALL)
        _close(out[4], ref["quadrupole_grads"], f"{fmt} zero quadrupoles: quadrupole_grads")
    assert np.abs(ref["quadrupole_grads"]).max() > 1e-3


def test_linear_and_bilinear_parts_and_dipole_independence_of_dipole_grads():
    both, real, recip = _api()
    f = _single()
    kw = _fmt_kw(f, "matrix")
    zq, zm = torch.zeros_like(f["Q"]), torch.zeros_like(f["M"])
    for label, call in (("total", lambda q, m, t: both(f["P"], q, m, t, f["C"], f["A"], f["kv"], **kw, **ALL)),
                        ("real space", lambda q, m, t: real(f["P"], q, m, t, f["C"], f["A"], **kw, **ALL)),
                        ("reciprocal space", lambda q, m, t: recip(f["P"], q, m, t, f["C"], f["kv"], f["A"], **ALL))):
        base = call(f["Q"], f["M"], f["T"])
        pure = call(zq, zm, f["T"])           # quadrupole-quadrupole alone: bilinear in Q
        twice = call(f["Q"], f["M"], 2.0 * f["T"])
        # E(Q) = E_lin + E_qq with E_lin linear in Q (charge-quadrupole and dipole-quadrupole): E(2 Q) = 2 E_lin + 4 E_qq = 2 E(Q) + 2 E_qq
        for k in (0, 1, 5):
            _close(twice[k], 2.0 * base[k] + 2.0 * pure[k], f"{label}: {NAMES[k]} of 2 Q = 2 linear part + 4 bilinear part", 1e-13)
        _close(twice[2], 2.0 * base[2], f"{label}: charge_grads of 2 Q", 1e-14)
        _close(twice[3], 2.0 * base[3], f"{label}: dipole_grads of 2 Q", 1e-14)
        _close(twice[4], base[4] + pure[4], f"{label}: quadrupole_grads of 2 Q", 1e-13)
        # dipole_grads (minus the field of the quadrupoles) does not depend on the dipoles
        other = call(f["Q"], torch.flip(f["M"], (0,)) * 1.7, f["T"])
        none = call(f["Q"], zm, f["T"])
        _close(other[3], base[3], f"{label}: dipole_grads with other dipoles")
        _close(none[3], base[3], f"{label}: dipole_grads without dipoles")
        assert float((other[0] - base[0]).abs().max()) > 1e-6


# ---- 6. consistency with the charge and dipole routines -----------------------------------------------------------------------------------
def test_charge_plus_dipole_plus_quadrupole_term_at_two_alpha():
    """`ewald_summation` + `ewald_dipole_correction` + `ewald_quadrupole_correction` at alpha = 0.45 and 0.5 over the same list (cutoff 7) and the
    same k set (k_cutoff 3.5) differ by the truncation of the sums only.  The references' own difference over the same entries and k-vectors
    (exact erfc) is that truncation; twice it is allowed (the charge routine evaluates erfc by a polynomial), as in tests/test_dipole_gpu.py."""
    from nvalchemiops.interactions.electrostatics import ewald_dipole_correction, ewald_summation
    from tests import dipole_reference as D

    both, real, recip = _api()
    f = _single()
    kv = _k_vectors(f["C"], 3.5)
    totals, refs = [], []
    for alpha in (0.45, 0.5):
        cc = ewald_summation(f["P"], f["Q"], f["C"], alpha=alpha, k_vectors=kv, **_fmt_kw(f, "matrix"))
        dd = ewald_dipole_correction(f["P"], f["Q"], f["M"], f["C"], alpha, kv, **_fmt_kw(f, "matrix"))
        qq = both(f["P"], f["Q"], f["M"], f["T"], f["C"], alpha, kv, **_fmt_kw(f, "matrix"))
        totals.append(float(cc.sum()) + float(dd.sum()) + float(qq.sum()))
        refs.append(float(D.charge_ewald_total(f["P"], f["Q"], f["C"][0], alpha, *f["entries"], kv))
                    + float(D.energies(f["P"], f["Q"], f["M"], f["C"], alpha, f["entries"], kv).sum().detach())
                    + float(R.energies(f["P"], f["Q"], f["M"], f["T"], f["C"], alpha, f["entries"], kv).sum().detach()))
    print(f"device  {totals[0]:.12e} {totals[1]:.12e} difference {abs(totals[0] - totals[1]):.3e}")
    print(f"reference {refs[0]:.12e} {refs[1]:.12e} difference {abs(refs[0] - refs[1]):.3e}")
    assert abs(totals[0] - totals[1]) <= 2.0 * abs(refs[0] - refs[1])


# ---- 7. autograd --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["list", "matrix"])
def test_autograd_matches_reference_and_explicit_outputs(fmt):
    both, real, recip = _api()
    f = _single()
    w = _t(np.random.default_rng(3).uniform(0.2, 1.8, f["n"]))
    ref = _sum(R.evaluate(f["P"], f["Q"], f["M"], f["T"], f["C"], f["A"], f["entries"], None, weights=w),
               R.evaluate(f["P"], f["Q"], f["M"], f["T"], f["C"], f["A"], None, f["kv"], weights=w))
    leaves = [f[k].clone().requires_grad_(True) for k in ("P", "Q", "M", "T")]
    e = both(*leaves, f["C"], f["A"], f["kv"], **_fmt_kw(f, fmt))
    assert e.requires_grad
    gp, gq, gm, gt = torch.autograd.grad((e * w).sum(), leaves)
    _close(-gp, ref["forces"], f"{fmt} dL/dr")
    _close(gq, ref["charge_grads"], f"{fmt} dL/dq")
    _close(gm, ref["dipole_grads"], f"{fmt} dL/dmu")
    _close(gt, ref["quadrupole_grads"], f"{fmt} dL/dQ")
    assert torch.equal(gt, gt.transpose(-1, -2)), "the quadrupole gradient is symmetric"
    # w = 1: the gradients of the total energy are the explicit outputs
    leaves = [f[k].clone().requires_grad_(True) for k in ("P", "Q", "M", "T")]
    e, frc, cg, dg, qg = both(*leaves, f["C"], f["A"], f["kv"], **_fmt_kw(f, fmt), **GRADS)
    gp, gq, gm, gt = torch.autograd.grad(e.sum(), leaves)
    _close(-gp, frc, f"{fmt} -dE/dr vs forces", 1e-12)
    _close(gq, cg, f"{fmt} dE/dq vs charge_grads", 1e-12)
    _close(gm, dg, f"{fmt} dE/dmu vs dipole_grads", 1e-12)
    _close(gt, qg, f"{fmt} dE/dQ vs quadrupole_grads", 1e-12)
    eager = both(f["P"], f["Q"], f["M"], f["T"], f["C"], f["A"], f["kv"], **_fmt_kw(f, fmt), compute_forces=True)
    assert torch.equal(e.detach(), eager[0]) and torch.equal(frc.detach(), eager[1])


def test_autograd_fp32_only_quadrupoles_and_batch():
    both, real, recip = _api()
    b = _batch()
    w = _t(np.random.default_rng(4).uniform(0.2, 1.8, b["n"]))
    ref = R.evaluate(b["P"], b["Q"], b["M"], b["T"], b["C"], b["A"], R.entries_from_matrix(b["nm"], b["sh"], b["n"]), b["kv"], batch_idx=b["bi"],
                     weights=w)
    T = b["T"].clone().requires_grad_(True)  # only the quadrupoles require grad; no dipoles given
    e = both(b["P"], b["Q"], b["M"], T, b["C"], b["A"], b["kv"], batch_idx=b["bi"], **_fmt_kw(b, "list"))
    (gt,) = torch.autograd.grad((e * w).sum(), [T])
    _close(gt, ref["quadrupole_grads"], "batch dL/dQ")
    f = _single()
    P, Q, M, T, C, A, kv = (f[k].float() for k in ("P", "Q", "M", "T", "C", "A", "kv"))
    w = _t(np.random.default_rng(3).uniform(0.2, 1.8, f["n"]))
    ref = _sum(R.evaluate(P, Q, M, T, C, A, f["entries"], None, distance_dtype=torch.float32, weights=w), R.evaluate(P, Q, M, T, C, A, None, kv, weights=w))
    leaves = [t.clone().requires_grad_(True) for t in (P, Q, M, T)]
    e = both(*leaves, C, A, kv, **_fmt_kw(f, "matrix"))
    grads = torch.autograd.grad((e * w.float()).sum(), leaves)
    assert all(g.dtype == torch.float32 for g in grads)
    for g, name, sign in zip(grads, NAMES[1:5], (-1.0, 1.0, 1.0, 1.0)):
        _close(sign * g, ref[name], f"fp32 adjoint {name}", 1e-6)


def test_second_order_and_out_of_scope_gradients_are_refused():
    both, real, recip = _api()
    f = _single()
    # a loss on the explicit forces (or any explicit gradient, or the virial) is a second derivative: refused at backward, never a silent zero
    for flag in ALL:
        P = f["P"].clone().requires_grad_(True)
        _, explicit = both(P, f["Q"], f["M"], f["T"], f["C"], f["A"], f["kv"], **_fmt_kw(f, "matrix"), **{flag: True})
        with pytest.raises(NotImplementedError, match="second derivatives of the pair kernels"):
            explicit.sum().backward()
    T = f["T"].clone().requires_grad_(True)
    e = both(f["P"], f["Q"], f["M"], T, f["C"], f["A"], f["kv"], **_fmt_kw(f, "matrix"))
    (g,) = torch.autograd.grad(e.sum(), [T], create_graph=True)
    with pytest.raises(NotImplementedError, match="second derivatives of the pair kernels"):
        g.sum().backward()
    # cell and alpha gradients are out of scope: refused, with a pointer to the virial
    for name in ("C", "A"):
        leaf = f[name].clone().requires_grad_(True)
        args = dict(C=f["C"], A=f["A"])
        args[name] = leaf
        e = both(f["P"], f["Q"], f["M"], f["T"], args["C"], args["A"], f["kv"], **_fmt_kw(f, "matrix"))
        with pytest.raises(NotImplementedError, match="use compute_virial"):
            e.sum().backward()


def test_virial_is_the_strain_derivative_and_not_symmetric():
    both, real, recip = _api()
    f = _single()
    a = (f["P"], f["Q"], f["M"], f["T"], f["C"])
    for label, vir, ref in (("total", both(*a, f["A"], f["kv"], **_fmt_kw(f, "list"), compute_virial=True)[1], f["ref"]),
                            ("real space", real(*a, f["A"], **_fmt_kw(f, "list"), compute_virial=True)[1], f["ref_real"]),
                            ("reciprocal space", recip(*a, f["kv"], f["A"], compute_virial=True)[1], f["ref_recip"])):
        _close(vir, ref["virial"], f"{label} virial vs the reference's strain derivative")
        v = _np(vir)[0]
        anti = np.linalg.norm(0.5 * (v - v.T)) / np.linalg.norm(v)
        print(f"{label}: antisymmetric part / norm = {anti:.3e}")
        assert anti > 1e-6, label  # a six-word (symmetrised) virial fails here and above


# ---- 8. determinism -----------------------------------------------------------------------------------------------------------------------
def test_two_calls_and_a_side_stream_are_bit_identical():
    both, real, recip = _api()
    b = _batch()
    w = _t(np.random.default_rng(6).uniform(0.2, 1.8, b["n"]))

    def run(fmt):
        out = both(b["P"], b["Q"], b["M"], b["T"], b["C"], b["A"], b["kv"], batch_idx=b["bi"], **_fmt_kw(b, fmt), **ALL)
        leaves = [b[k].clone().requires_grad_(True) for k in ("P", "Q", "M", "T")]
        e = both(*leaves, b["C"], b["A"], b["kv"], batch_idx=b["bi"], **_fmt_kw(b, fmt))
        return tuple(out) + tuple(torch.autograd.grad((e * w).sum(), leaves))

    for fmt in ("list", "matrix"):
        first, second = run(fmt), run(fmt)
        torch.cuda.current_stream().synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            third = run(fmt)
        side.synchronize()
        for k, (a, b2, c) in enumerate(zip(first, second, third)):
            assert torch.equal(a, b2) and torch.equal(a, c), (fmt, k)


# ---- 9. compile ---------------------------------------------------------------------------------------------------------------------------
def test_compile_fullgraph_equals_eager_bitwise():
    both, real, recip = _api()
    f = _single()

    def fn(p, q, m, t):
        e, frc, qg, vir = both(p, q, m, t, f["C"], f["A"], f["kv"], neighbor_matrix=f["nm"], neighbor_matrix_shifts=f["sh"], mask_value=f["n"],
                               compute_forces=True, compute_quadrupole_gradients=True, compute_virial=True)
        return e * 2.0, frc, qg, vir

    torch._dynamo.reset()
    got = torch.compile(fn, mode="default", fullgraph=True)(f["P"], f["Q"], f["M"], f["T"])
    want = fn(f["P"], f["Q"], f["M"], f["T"])
    for a, b in zip(got, want):
        assert torch.equal(a, b)

    def parts(p, q, t):
        return (real(p, q, None, t, f["C"], f["A"], neighbor_list=f["nl"], neighbor_ptr=f["ptr"], neighbor_shifts=f["lsh"], compute_dipole_gradients=True)
                + recip(p, q, None, t, f["C"], f["kv"], f["A"], compute_dipole_gradients=True))

    got = torch.compile(parts, mode="default", fullgraph=True)(f["P"], f["Q"], f["T"])
    for a, b in zip(got, parts(f["P"], f["Q"], f["T"])):
        assert torch.equal(a, b)


# ---- 10. the other operators are untouched, and the field of the quadrupoles reaches the induced-dipole solver ------------------------------
def test_minus_dipole_grads_is_the_field_for_induced_dipoles():
    """-dipole_grads of this correction is the field of the quadrupoles: adding mu . dipole_grads to the dipole energy reproduces the
    dipole-quadrupole energy, which is linear in mu."""
    both, real, recip = _api()
    f = _single()
    zq = torch.zeros_like(f["Q"])
    kw = _fmt_kw(f, "matrix")
    e_mu, dg = both(f["P"], zq, f["M"], f["T"], f["C"], f["A"], f["kv"], **kw, compute_dipole_gradients=True)
    e_0 = both(f["P"], zq, None, f["T"], f["C"], f["A"], f["kv"], **kw)
    _close((e_mu - e_0).sum().reshape(1), (f["M"] * dg).sum().reshape(1), "sum_i mu_i . dipole_grads_i = the dipole-quadrupole energy", 1e-12)
