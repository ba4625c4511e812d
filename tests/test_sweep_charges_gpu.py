"""Seeded sweeps and boundary ladders of `gaussian_charge_correction` and of the charge-equilibration operator (`mi_qeq_pair_coefficients`,
`mi_qeq_apply`, one cluster solve per seed) against the float64 restatements tests/gaussian_reference.py and tests/qeq_reference.py,
evaluated on the entries actually stored.  The inputs are those of tests/sweep_cases.py (`_system` / `_abi_case` of the two ops' modules,
seeded: one to three systems of 1, 9, 60 or 150 atoms, float32 and float64, cells shorter than the cutoff in a third of the seeds, charged
and neutral systems, exact-zero widths, a matrix widest row + an odd pad wide whose padding is the mask value, -1 and n + 7, one emptied
row); the bounds are the ones those modules use and are imported from them: `_close` (1e-11 of max|ref| + 1e-14 in float64, 1e-6 against
the float32-distance mode) for the Gaussian correction, the analytic bounds of tests/test_qeq_gpu.py (its docstring derives them) for the
coefficients and the product, `_check_solution` for the solve.  No tolerance is new.

Ladders.  Free clusters of 64, 65, 66 and 129 atoms without a cell, every pair stored, as CSR and as a matrix exactly n - 1 wide: rows of
63, 64, 65 and 128 entries against the 64-lane trips of `gc_pair_kernel` and `qeq_coef_kernel`.  `box150` of tests/test_qeq_gpu.py at cutoff
9.5 (rows of 294 - 332 entries): as CSR, as a matrix of 335 columns, and cut to the first 255, 256 and 257 entries of every row -- full rows
of exactly one pass of `qeq_apply_kernel`'s four unrolled trips of 64, one entry less and one more (`e + 3 * MI_WAVE < end`).

MEASURED on one MI355X (every test prints its figures under `pytest -s`): Gaussian correction 8.7e-14 of max|ref| in
float64 and 2.0e-7 in float32 over the twelve seeds, 1.3e-15 on the lane ladder; coefficients at most 0.19 of their bound, products 0.042,
identical on the five layouts of the unrolled-product ladder; cluster solves at most 0.96 of (tolerance x ||b||).
"""
import numpy as np
import pytest
import torch

from tests import gaussian_reference as GR
from tests import qeq_reference as R
from tests import sweep_cases as W
from tests import test_gaussian_charges_gpu as GT
from tests import test_qeq_gpu as QT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
_t = QT._t


def _stored(c, width=None, mask_emptied=False):
    """The case's entries as a padded matrix (+ shifts) and as CSR: widest row + the case's pad wide (or cut to the first `width` entries
    of every row), one row emptied, the last padding column -1 and every other entry of the one before n + 7.  `mask_emptied`: the mask
    value is the emptied row's own index, so the entries that point to it are padding too and the list is a FULL list again (what the
    gradients of `gaussian_charge_correction` require), as in tests/test_gaussian_charges_gpu.py; else it is n."""
    n = len(c["pos"])
    i, j, S = c["entries"]
    if width is not None:
        start = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=n))])
        first = np.arange(len(i)) - start[i] < width
        i, j, S = i[first], j[first], S[first]
    m = (c["widest"] + c["pad"]) if width is None else width
    nm, sh = QT._lists(torch.as_tensor(i), torch.as_tensor(j), torch.as_tensor(S), n, m, n)
    if c["emptied_row"] is not None:
        nm[c["emptied_row"]] = n
    if c["pad"] >= 3 and width is None:
        assert bool((nm[:, -2:] == n).all())
        nm[:, -1] = -1       # out-of-range padding below ...
        nm[::2, -2] = n + 7  # ... and above [0, N), next to mask-value padding
    nm, sh = nm.contiguous(), sh.contiguous()
    mask = c["emptied_row"] if mask_emptied and c["emptied_row"] is not None else n
    nl, ptr, lsh = QT._csr(nm, sh, mask)
    return dict(n=n, m=m, mask=mask, nm=nm, sh=sh, nl=nl, ptr=ptr, lsh=lsh)


def _dtype(c):
    return torch.float64 if c["dtype"] == "float64" else torch.float32


# ---- gaussian_charge_correction -----------------------------------------------------------------------------------------------------------------

def _gaussian(c, f, tag, **flags):
    """Both layouts of one call against `gaussian_reference.evaluate` on the stored entries, every requested output."""
    from nvalchemiops.interactions.electrostatics import gaussian_charge_correction as gcc

    dt = _dtype(c)
    periodic = c["cells"] is not None
    P, Q, Sg = _t(c["pos"], dt), _t(c["q"], dt), _t(c["sigma"], dt)
    C = _t(c["cells"], dt) if periodic else None
    bi = _t(c["batch_idx"]) if len(c["sizes"]) > 1 else None
    names = ["energies"] + [k for k, flag in zip(GT.NAMES[1:], W.COMPUTE_FLAGS) if flags.get(flag)]
    switches = dict(self_energy=c.get("self_energy", True), neutralizing_background=c.get("background", True))
    ref = GR.evaluate(P, Q, Sg, C, *GR.entries_from_matrix(f["nm"], f["sh"] if periodic else None, f["mask"]), batch_idx=bi,
                      self_energy=switches["self_energy"], background=switches["neutralizing_background"], distance_dtype=dt)
    for fmt in ("matrix", "list"):
        if fmt == "matrix":
            lk = dict(neighbor_matrix=f["nm"], mask_value=f["mask"], **(dict(neighbor_matrix_shifts=f["sh"]) if periodic else {}))
        else:
            lk = dict(neighbor_list=f["nl"], neighbor_ptr=f["ptr"], **(dict(neighbor_shifts=f["lsh"]) if periodic else {}))
        args = (P, Q, Sg) + ((C,) if periodic else ())
        out = gcc(*args, batch_idx=bi, **lk, **flags, **switches)
        out = (out,) if isinstance(out, torch.Tensor) else out
        assert len(out) == len(names) and all(o.dtype == dt for o in out)
        for name, o in zip(names, out):
            err = GT._close(o, ref[name], f"{tag} {fmt} {name}", 1e-11 if dt == F64 else 1e-6)
            print(f"[sweep] {tag} {c['dtype']} {fmt:6s} {name:13s} max|ref| {np.abs(ref[name]).max():.3e} rel err {err:.2e} (bar {'1e-11' if dt == F64 else '1e-6'})")
    return ref


@pytest.mark.parametrize("seed", W.SEEDS)
def test_gaussian_sweep(seed):
    c = W.case("gaussian_charge_correction", seed)
    ref = _gaussian(c, _stored(c, mask_emptied=True), f"gaussian {seed}", **c["flags"])
    assert np.abs(ref["energies"]).max() > 0.0


@pytest.mark.parametrize("name", W.LANE_RUNGS)
def test_gaussian_lane_trip_ladder(name):
    c = W.ladder_case("gaussian_charge_correction", name)
    f = _stored(c)
    n = f["n"]
    assert f["nm"].shape == (n, n - 1) and int(f["nm"].max()) == n - 1, "every row full: no padding column"
    _gaussian(c, f, f"gaussian {name}", compute_forces=True, compute_charge_gradients=True, compute_sigma_gradients=True)


# ---- the charge-equilibration operator ------------------------------------------------------------------------------------------------------------

def _operator(c, f, fmt, tag):
    """`mi_qeq_pair_coefficients` and `mi_qeq_apply` on the stored entries against the dense reference, at the analytic bounds of
    tests/test_qeq_gpu.py::test_coefficients_and_product_against_the_dense_reference (its constants, its formulas), system by system."""
    dt = _dtype(c)
    n, m = f["n"], f["m"]
    periodic = c["cells"] is not None
    nsys = len(c["sizes"])
    P, Sg, Jd = _t(c["pos"], dt), _t(c["sigma"], dt), _t(c["hard"])
    Cl = _t(c["cells"], dt) if periodic else None
    al = _t(c["alpha"], dt) if periodic else None
    bi = _t(c["batch_idx"]) if nsys > 1 else None
    if fmt == "matrix":
        idx, sh, nptr, mm = f["nm"], f["sh"], None, m
        keep = ((f["nm"] != n) & (f["nm"] >= 0) & (f["nm"] < n)).reshape(-1)
        rows = torch.arange(n, device=DEV).unsqueeze(1).expand(n, m).reshape(-1)
        ent = GR.entries_from_matrix(f["nm"], f["sh"], n)
    else:
        idx, sh, nptr, mm = f["nl"][1].contiguous(), f["lsh"], f["ptr"], 0
        ent = GR.entries_from_csr(f["nl"], f["ptr"], f["lsh"])
        keep, rows = torch.ones(idx.numel(), dtype=torch.bool, device=DEV), ent[0]
    coef, nbr, diag = QT._coefficients(P, Sg, Jd, Cl, al, bi, nsys, idx.contiguous(), sh.contiguous() if periodic else None, nptr, mm, n)
    model = dict(batch_idx=bi, erfc_lr=R.erfc_as, distance_dtype=dt)
    c_ref = R.pair_coefficients(P, Sg, Cl, al, *ent, **model)
    lr_mag, ec_mag = R.pair_coefficients(P, Sg, Cl, al, *ent, parts=True, **model)
    assert bool((coef[~keep] == 0).all()) and bool((nbr[~keep] == rows[~keep].to(torch.int32)).all())
    assert int(nbr.min()) >= 0 and int(nbr.max()) < n
    stored = c_ref != 0
    assert bool((nbr[keep][stored] == ent[1][stored].to(torch.int32)).all())
    f32 = dt == torch.float32
    tol = QT.COND * QT.EPS * (lr_mag + ec_mag) + QT.LIBM_ERFC * ec_mag + (QT.F32_PAIR * (lr_mag + ec_mag) if f32 else 0.0)
    err = (coef[keep] - c_ref).abs()
    worst_c = float((err / tol.clamp(min=1e-300)).max()) if err.numel() else 0.0
    assert bool((err <= tol).all()), f"{tag} {fmt}: coefficients"
    d_ref = R.diagonal(Jd, Sg)
    assert bool(((diag - d_ref).abs() <= 4 * QT.EPS * d_ref.abs()).all())
    x, y_in = _t(c["x"]), _t(c["y_in"])
    y, part = QT._apply(coef, nbr, diag, x, y_in, bi, nsys, nptr, mm)
    h = R.real_space_operator(P, Sg, Jd, Cl, al, *ent, **model)
    y_ref = y_in + h @ x
    zeros = torch.zeros(n, dtype=F64, device=DEV)
    k_row = zeros.index_add(0, ent[0], torch.ones_like(c_ref))
    mag = zeros.index_add(0, ent[0], (lr_mag + ec_mag) * x[ent[1]].abs()) + (d_ref * x).abs() + y_in.abs()
    bound = 2.0 * (k_row + 8.0) * QT.EPS * mag + QT.LIBM_ERFC * zeros.index_add(0, ent[0], ec_mag * x[ent[1]].abs())
    if f32:
        bound = bound + QT.F32_PAIR * mag
    err = (y - y_ref).abs()
    print(f"[sweep] {tag} {c['dtype']} {fmt}: rows of {int(k_row.min())} - {int(k_row.max())} entries, max |dc| / bound {worst_c:.3f}, "
          f"max |dy| / bound {float((err / bound).max()):.3f}, max |dy| {float(err.max()):.2e} on |y| {float(y_ref.abs().max()):.2f}")
    assert bool((err <= bound).all()), f"{tag} {fmt}: product"
    if c["emptied_row"] is not None:
        k = c["emptied_row"]
        assert float(k_row[k]) == 0 and float(y[k]) == float(y_in[k] + diag[k] * x[k])
    sys_of = torch.zeros(n, dtype=torch.long, device=DEV) if bi is None else bi.long()
    sums = part.sum(1)
    for s in range(nsys):
        sel = sys_of == s
        ns = int(sel.sum())
        assert abs(float(sums[s, 0] - y[sel].sum())) <= ns * QT.EPS * float(y[sel].abs().sum())
        assert abs(float(sums[s, 1] - (x[sel] * y[sel]).sum())) <= ns * QT.EPS * float((x[sel] * y[sel]).abs().sum())
    return k_row


@pytest.mark.parametrize("seed", W.SEEDS)
def test_qeq_sweep(seed):
    from nvalchemiops.interactions.electrostatics import charge_equilibration as qeq

    c = W.case("charge_equilibration", seed)
    f = _stored(c)
    for fmt in ("matrix", "csr"):
        _operator(c, f, fmt, f"qeq {seed}")
    # one cluster solve against the dense KKT solution
    sizes = c["cluster_sizes"]
    k = QT._cluster(sizes, c["cluster_seed"])
    nsys = len(sizes)
    total = _t(c["cluster_total"][:nsys])
    bi = k["bi"] if nsys > 1 else None
    h = R.dense_operator(k["pos"], k["sigma"], k["hard"], None, None, None, *k["ent"], batch_idx=bi)
    fmt = ("matrix", "csr")[seed % 2]
    out = qeq(k["pos"], k["chi"], k["hard"], k["sigma"], total_charge=total, batch_idx=bi, tolerance=1e-10, return_info=True, **QT._kw(k, fmt, shifts=False))
    QT._check_solution(out, h, k["chi"], total, bi, nsys, 1e-10, 200, f"[sweep] qeq {seed}: clusters {sizes} {fmt}")


@pytest.mark.parametrize("name", W.LANE_RUNGS)
def test_qeq_lane_trip_ladder(name):
    c = W.ladder_case("charge_equilibration", name)
    f = _stored(c)
    n = f["n"]
    assert f["nm"].shape == (n, n - 1) and int(f["nm"].max()) == n - 1
    for fmt in ("matrix", "csr"):
        k_row = _operator(c, f, fmt, f"qeq {name}")
        assert bool((k_row == n - 1).all())


@pytest.mark.parametrize("width", (None,) + W.UNROLLED_WIDTHS)
def test_qeq_unrolled_product_ladder(width):
    """Rows longer than the 256 entries of one pass of the product's four unrolled trips: CSR (`width` None), a matrix of 335 columns that
    holds every row, and matrices cut to 255, 256 and 257 full columns."""
    c = W.unrolled_case()
    counts = np.bincount(c["entries"][0], minlength=150)
    assert counts.max() <= 335 and counts.max() > 256 and counts.min() > 257
    f = _stored(c, width=width if width != 335 else None) if width is not None else _stored(c)
    if width == 335:
        wide = torch.full((150, 335), 150, dtype=torch.int32, device=DEV)
        wsh = torch.zeros((150, 335, 3), dtype=torch.int32, device=DEV)
        wide[:, :f["m"]], wsh[:, :f["m"]] = f["nm"], f["sh"]
        f = dict(f, nm=wide, sh=wsh, m=335)
    k_row = _operator(c, f, "csr" if width is None else "matrix", f"qeq box150 at 9.5, {'csr' if width is None else f'matrix {width} wide'}")
    if width in (255, 256, 257):
        assert bool((k_row == width).all()), "every row is full"
    else:
        assert int(k_row.max()) == counts.max() > 256
