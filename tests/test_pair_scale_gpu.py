"""`mi_pair_scale` and its public function `pair_scale_correction` on the device, against the float64 operator-definition yardstick
tests/pair_scale_reference.py (itself checked in tests/test_pair_scale_reference_cpu.py) on the same stored entries.

Lists are built by hand (tests/pair_scale_cases.py), independent of the neighbour search.  The kernel gives a group of 8 lanes to a row, so
the shapes are: a 70-atom ladder whose rows hold 0, 1, 7, 8, 9, 16, 17 and 25 entries (an empty row, one trip, a group exactly full, the
second and third trips, a tail) with one wave of 8 empty rows; 1, 7, 33 and 70 atoms (the last wave's and the last block's partial rows);
matrix rows seven columns wider than the longest row, padded with the mask value, -1 and N + 7 (the scales of the padding are NaN); a batch
of three molecules in three triclinic cells; three atoms with a charge only; dipoles, quadrupoles or both absent; matrix and CSR; one entry
in five of the ladders has s = 1.  Every distance of a listed pair is >= 1.3.

Bars: those of tests/test_cluster_multipole_gpu.py for the same arithmetic model -- 1e-11 of the largest |value| of each output for float64
inputs, 1e-6 for float32 positions against the yardstick's float32-distance mode, matrix against CSR 1e-10 -- and 1e-10 for the fused
result against the composed existing operators.

Measured on the MI355X.  fp64 over every flag word 2.0e-16 - 1.1e-15; float32 positions 2.5e-8 - 3.9e-7 (the 1e-6 bar holds as it stands, so
the composed operators' float32 error was not needed as a second bar); fused against composed 5.4e-17 - 6.2e-16; exclusion identity
1.5e-16 - 2.8e-16; through `rotate_multipoles` 2.5e-16 - 1.4e-15; matrix against CSR 0.  DESIGN 3.32 has the table."""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import pair_scale_cases as PC
from tests import pair_scale_reference as PR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
FORCES, CHARGE_GRAD, DIPOLE_GRAD, VIRIAL, QUADRUPOLE_GRAD = 1, 2, 4, 8, 16  # MI_QD_*
OUTPUTS = (("forces", FORCES), ("charge_grads", CHARGE_GRAD), ("dipole_grads", DIPOLE_GRAD), ("quadrupole_grads", QUADRUPOLE_GRAD),
           ("virial", VIRIAL))
NAMES = ("energies",) + tuple(n for n, _ in OUTPUTS)
ALL = dict(compute_forces=True, compute_charge_gradients=True, compute_dipole_gradients=True, compute_quadrupole_gradients=True,
           compute_virial=True)
NO_VIRIAL = dict(ALL, compute_virial=False)
SIGNS = (-1.0, 1.0, 1.0, 1.0)  # forces = -dE/dr
LADDERS = ("ladder1", "ladder7", "ladder33", "ladder70")


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


def _np(x):
    return x.detach().cpu().numpy().astype(np.float64)


def _close(got, ref, what, rel):
    got = _np(got) if isinstance(got, torch.Tensor) else got
    ref = _np(ref) if isinstance(ref, torch.Tensor) else ref
    assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
    scale = max(np.abs(ref).max(), 1e-30) if ref.size else 1.0
    err = np.abs(got - ref).max() if ref.size else 0.0
    print(f"{what:72s} rel err {err / scale:.2e} (bar {rel:.0e})")
    assert err <= rel * scale + 1e-14, f"{what}: max err {err:.3e} > {rel * scale:.3e}"


def _fn():
    from nvalchemiops.interactions.electrostatics import pair_scale_correction

    return pair_scale_correction


def _csr_ptr(i, n):
    ptr = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    ptr[1:] = torch.cumsum(torch.bincount(i.to(DEV), minlength=n), 0)
    return ptr


def _lists(entries, scales, n, periodic):
    """dict(nm, sh, snm, nl, ptr, lsh, scsr, ent, s) of a full list whose entries are sorted by row.  The matrix is seven columns wider than
    the longest row and padded with the mask value n, with -1 in the last column and N + 7 in every other row of the one before; the scales
    of all padding are NaN (they must not be looked at)."""
    i, j, S = (e.to(DEV) for e in entries)
    s = _t(scales, F64)
    counts = torch.bincount(i, minlength=n)
    m = (int(counts.max()) if i.numel() else 0) + 7
    col = torch.arange(i.shape[0], device=DEV) - (torch.cumsum(counts, 0) - counts)[i]
    nm = torch.full((n, m), n, dtype=torch.int32, device=DEV)
    sh = torch.zeros((n, m, 3), dtype=torch.int32, device=DEV)
    snm = torch.full((n, m), float("nan"), dtype=F64, device=DEV)
    nm[i, col], sh[i, col], snm[i, col] = j.to(torch.int32), S.to(torch.int32), s
    nm[:, -1] = -1
    nm[::2, -2] = n + 7
    f = dict(n=n, nm=nm.contiguous(), sh=sh.contiguous(), snm=snm.contiguous(), nl=torch.stack([i, j]).to(torch.int32).contiguous(),
             ptr=_csr_ptr(i, n), lsh=S.to(torch.int32).contiguous(), scsr=s.contiguous(), ent=(i, j, S), s=s)
    if not periodic:
        f["sh"] = f["lsh"] = None
    return f


def _kw(f, fmt, shifts=True):
    if fmt == "matrix":
        return dict(pair_scales=f["snm"], neighbor_matrix=f["nm"], neighbor_matrix_shifts=f["sh"] if shifts else None, mask_value=f["n"])
    return dict(pair_scales=f["scsr"], neighbor_list=f["nl"], neighbor_ptr=f["ptr"], neighbor_shifts=f["lsh"] if shifts else None)


@functools.lru_cache(maxsize=None)
def _case(kind):
    """"ladder<N>": the clusters of tests/pair_scale_cases.py; "periodic": its triclinic box with explicit shifts; "molecules": its batch of
    three molecules in three cells, wrapped atoms with the shifts that join them ("pos_whole": the same molecules unwrapped)."""
    p = PC.ladder(int(kind[6:])) if kind.startswith("ladder") else PC.periodic() if kind == "periodic" else PC.molecules()
    f = _lists(p["entries"], p["scales"], p["n"], p["cell"] is not None)
    f.update(kind=kind, nsys=p["nsys"], cells=p["cell"], bi=None if p["batch_idx"] is None else _t(p["batch_idx"]), w=_t(p["w"]),
             pos=p["pos_wrapped"] if kind == "molecules" else p["pos"], **{k: p[k] for k in ("q", "mu", "Q")}, problem=p)
    return f


def _inputs(f, dtype=F64, pos="pos"):
    src = f["problem"]["pos"] if pos == "pos_whole" else f["pos"]
    return [_t(src, dtype)] + [_t(f[k], dtype) for k in ("q", "mu", "Q")]


def _cells(f, dtype=F64):
    return None if f["cells"] is None else _t(f["cells"], dtype)


@functools.lru_cache(maxsize=None)
def _reference(kind, dtype=F64, weighted=False, mu=True, Q=True, minimum_image=False):
    f = _case(kind)
    pos, q, m, qq = _inputs(f, dtype)
    ent = f["ent"] if not minimum_image else (f["ent"][0], f["ent"][1], torch.zeros_like(f["ent"][2]))
    return PR.evaluate(pos, q, m if mu else None, qq if Q else None, f["s"], ent, cell=_cells(f, dtype), batch_idx=f["bi"], distance_dtype=dtype,
                       weights=f["w"] if weighted else None, minimum_image=minimum_image)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def _capi(arrays, scales, cells, bi, nsys, idx, sh, nptr, m, mask, flags, weights=None, energies=True, minimum_image=False):
    """One `mi_pair_scale` call into NaN-filled buffers: dict of every output buffer, asked for or not (virial: folded [nsys, 3, 3])."""
    import ctypes

    from nvalchemiops import _capi as C

    P = arrays[0]
    L, n, dt = C.lib(), P.shape[0], P.dtype
    nan = lambda *shape, dtype=F64: torch.full(shape, float("nan"), dtype=dtype, device=DEV)  # noqa: E731
    out = dict(energies=nan(n), forces=nan(n, 3, dtype=dt), charge_grads=nan(n), dipole_grads=nan(n, 3), quadrupole_grads=nan(n, 3, 3),
               virial=nan(nsys, L.mi_pair_scale_blocks(), 9))
    nbytes = int(L.mi_pair_scale_scratch_bytes(n, C.dtype_code(dt)))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    ask = lambda key, bit: C.ptr(out[key]) if flags & bit else None  # noqa: E731
    rc = L.mi_pair_scale(*[C.ptr(a) for a in arrays], C.ptr(cells), C.ptr(bi), C.ptr(weights), C.ptr(scales), n, nsys, C.dtype_code(dt), C.ptr(idx),
                         C.ptr(sh), C.ptr(nptr), m, mask, int(minimum_image), flags, C.ptr(out["energies"]) if energies else None,
                         ask("forces", FORCES), ask("charge_grads", CHARGE_GRAD), ask("dipole_grads", DIPOLE_GRAD),
                         ask("quadrupole_grads", QUADRUPOLE_GRAD), ask("virial", VIRIAL), C.ptr(scratch), ctypes.c_size_t(nbytes), C.stream_of(P))
    C.check(rc, "mi_pair_scale")
    out["virial"] = out["virial"].sum(1).reshape(nsys, 3, 3)
    return out


def _abi_inputs(f, dtype, fmt, mu=True, Q=True):
    pos, q, m, qq = _inputs(f, dtype)
    lay = (f["snm"], _cells(f, dtype), f["bi"], f["nsys"], f["nm"], f["sh"], None, f["nm"].shape[1]) if fmt == "matrix" else \
        (f["scsr"], _cells(f, dtype), f["bi"], f["nsys"], f["nl"][1].contiguous(), f["lsh"], f["ptr"], 0)
    return ([pos, q, m if mu else None, qq if Q else None],) + lay + (f["n"],)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("fmt", ["matrix", "csr"])
@pytest.mark.parametrize("kind", ["ladder70", "molecules"])
def test_c_abi_every_flag_word_against_the_yardstick(kind, fmt, dtype):
    """Parity of every output under every flag word (2^5 with a cell, 2^4 without: a cluster has no virial), and only what was asked for is
    written."""
    f = _case(kind)
    ref = _reference(kind, dtype)
    rel = 1e-11 if dtype == torch.float64 else 1e-6
    args = _abi_inputs(f, dtype, fmt)
    bits = [b for _, b in OUTPUTS if b != VIRIAL or f["cells"] is not None]
    worst = {}
    for r in range(len(bits) + 1):
        for combo in itertools.combinations(bits, r):
            flags = sum(combo)
            out = _capi(*args, flags)
            for name, bit in (("energies", 0),) + OUTPUTS:
                if bit and not flags & bit:
                    assert bool(torch.isnan(out[name]).all()), f"{name} was written without being asked for (flags {flags})"
                    continue
                got, want = _np(out[name]), ref[name]
                assert not np.isnan(got).any(), (name, flags)
                scale = np.abs(want).max()
                worst[name] = max(worst.get(name, 0.0), np.abs(got - want).max() / scale)
    print(f"{kind} {fmt} {dtype}: worst rel err over {2 ** len(bits)} flag words (bar {rel:.0e}): " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for name, err in worst.items():
        assert err <= rel + 1e-14 / np.abs(ref[name]).max(), f"{kind} {fmt} {dtype} {name}: rel err {err:.3e} > {rel:.0e}"
    if kind == "ladder70":  # empty rows -- row 0 and the wave of rows 16 ... 23 -- are exact zeros
        full = _capi(*args, sum(bits))
        for row in [0] + list(range(16, 24)):
            assert all(float(full[k][row].abs().max()) == 0.0 for k in NAMES if k != "virial"), row


@pytest.mark.parametrize("absent", ["dipoles", "quadrupoles", "both"])
def test_c_abi_null_dipoles_and_quadrupoles(absent):
    mu, Q = absent == "quadrupoles", absent == "dipoles"
    f = _case("ladder33")
    ref = _reference("ladder33", mu=mu, Q=Q)
    flags = FORCES | CHARGE_GRAD | DIPOLE_GRAD | QUADRUPOLE_GRAD
    out = _capi(*_abi_inputs(f, F64, "csr", mu=mu, Q=Q), flags)
    for name in NAMES[:-1]:
        _close(out[name], ref[name], f"{absent} NULL, {name}", 1e-11)


def test_c_abi_weights_give_the_adjoint_and_energies_may_be_null():
    f = _case("molecules")
    ref = _reference("molecules", weighted=True)
    flags = FORCES | CHARGE_GRAD | DIPOLE_GRAD | QUADRUPOLE_GRAD
    out = _capi(*_abi_inputs(f, F64, "csr"), flags, weights=f["w"], energies=False)
    assert bool(torch.isnan(out["energies"]).all())
    for name in NAMES[1:-1]:
        _close(out[name], ref[name], f"weighted {name}", 1e-11)


# ---- the public function ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LADDERS)
def test_group_ladder_and_partial_blocks_through_the_public_function(kind):
    """1, 7, 33 and 70 atoms in both formats against the yardstick, matrix against CSR, a subset of the flags, float32."""
    fn, f = _fn(), _case(kind)
    ref = _reference(kind)
    outs = {}
    for fmt in ("matrix", "list"):
        out = outs[fmt] = fn(*_inputs(f), **_kw(f, fmt), **NO_VIRIAL)
        assert all(o.dtype == F64 for o in out) and len(out) == 5
        for name, o in zip(NAMES, out):
            _close(o, ref[name], f"{kind} {fmt} {name}", 1e-11)
        e, dg = fn(*_inputs(f), **_kw(f, fmt), compute_dipole_gradients=True)
        assert torch.equal(e, out[0]) and torch.equal(dg, out[3])
    for name, a, b in zip(NAMES, outs["matrix"], outs["list"]):
        _close(a, b, f"{kind} matrix against CSR, {name}", 1e-10)
    out32 = fn(*_inputs(f, torch.float32), **_kw(f, "matrix"), **NO_VIRIAL)
    assert all(o.dtype == torch.float32 for o in out32)
    ref32 = _reference(kind, torch.float32)
    for name, o in zip(NAMES, out32):
        _close(o, ref32[name], f"{kind} float32 {name}", 1e-6)
    if kind == "ladder1":
        assert all(not bool(o.any()) for o in outs["matrix"] + outs["list"])


@pytest.mark.parametrize("absent", ["dipoles", "quadrupoles", "both"])
def test_missing_multipoles(absent):
    """`dipoles=None` / `quadrupoles=None` are no dipoles / no quadrupoles; three atoms of every case carry a charge only."""
    fn, f = _fn(), _case("ladder33")
    mu, Q = absent == "quadrupoles", absent == "dipoles"
    ref = _reference("ladder33", mu=mu, Q=Q)
    pos, q, m, qq = _inputs(f)
    assert not f["mu"][list(PC.PLAIN)].any() and not f["Q"][list(PC.PLAIN)].any()
    for fmt in ("matrix", "list"):
        out = fn(pos, q, m if mu else None, qq if Q else None, **_kw(f, fmt), **NO_VIRIAL)
        for name, o in zip(NAMES, out):
            _close(o, ref[name], f"{absent} absent, {fmt} {name}", 1e-11)
        zeros = fn(pos, q, m if mu else torch.zeros_like(m), qq if Q else torch.zeros_like(qq), **_kw(f, fmt), **NO_VIRIAL)
        assert all(torch.equal(a, b) for a, b in zip(out, zeros))


def _sub_csr(f, sel):
    i, j, _ = f["ent"]
    return dict(neighbor_list=torch.stack([i[sel], j[sel]]).to(torch.int32).contiguous(), neighbor_ptr=_csr_ptr(i[sel], f["n"]))


def _unscaled(pos, q, mu, Q, lists):
    """(energies, forces, charge_grads, dipole_grads, quadrupole_grads) of the unscaled cluster total over a CSR list: `coulomb_energy_forces`
    (whose charge gradient comes from its autograd) + `coulomb_dipole_correction` + `coulomb_quadrupole_correction`."""
    from nvalchemiops.interactions.electrostatics import coulomb_dipole_correction, coulomb_quadrupole_correction
    from nvalchemiops.interactions.electrostatics.coulomb import coulomb_energy_forces

    n = pos.shape[0]
    nnz = lists["neighbor_list"].shape[1]
    qq = q.clone().requires_grad_(True)
    e0, f0 = coulomb_energy_forces(pos, qq, torch.eye(3, dtype=F64, device=DEV).reshape(1, 3, 3) * 1e3, 1e6, 0.0,
                                   neighbor_shifts=torch.zeros((nnz, 3), dtype=torch.int32, device=DEV), **lists)
    c0 = torch.autograd.grad(e0.sum(), qq)[0]
    e1, f1, c1, d1 = coulomb_dipole_correction(pos, q, mu, **lists, compute_forces=True, compute_charge_gradients=True, compute_dipole_gradients=True)
    e2, f2, c2, d2, g2 = coulomb_quadrupole_correction(pos, q, mu, Q, **lists, **NO_VIRIAL)
    assert n == e0.shape[0]
    return e0.detach() + e1 + e2, f0.detach() + f1 + f2, c0 + c1 + c2, d1 + d2, g2


def test_fused_equals_the_composed_existing_operators():
    """sum over the scale classes of (s_c - 1) x (`coulomb_energy_forces` + `coulomb_dipole_correction` + `coulomb_quadrupole_correction`) on
    the per-class sub-lists, all outputs."""
    fn, f = _fn(), _case("ladder70")
    pos, q, mu, Q = _inputs(f)
    fused = fn(pos, q, mu, Q, **_kw(f, "list"), **NO_VIRIAL)
    composed = None
    assert sorted(set(f["s"].tolist())) == sorted(PC.CLASSES + (1.0,))
    for c in PC.CLASSES:
        part = [(c - 1.0) * o for o in _unscaled(pos, q, mu, Q, _sub_csr(f, f["s"] == c))]
        composed = part if composed is None else [a + b for a, b in zip(composed, part)]
    for name, a, b in zip(NAMES, fused, composed):
        _close(a, b, f"fused against composed, {name}", 1e-10)


def test_exclusions_leave_the_unlisted_pairs():
    """The all-pairs cluster total of the three molecules plus this operator with s = 0 on every bonded pair is the total over the pairs
    that are not bonded.  Bar: 1e-10 of the largest |value| of the all-pairs total (every term is good to 1e-11 of its own scale)."""
    fn, f = _fn(), _case("molecules")
    p = f["problem"]
    pos, q, mu, Q = _inputs(f, pos="pos_whole")
    i, j, _ = (e.to(DEV) for e in p["all_pairs"])
    n = f["n"]
    listed = torch.zeros((n, n), dtype=torch.bool, device=DEV)
    listed[f["ent"][0], f["ent"][1]] = True
    keep = ~listed[i, j]
    assert bool(keep.any()) and not bool(keep.all())
    every = dict(neighbor_list=torch.stack([i, j]).to(torch.int32).contiguous(), neighbor_ptr=_csr_ptr(i, n))
    rest = dict(neighbor_list=torch.stack([i[keep], j[keep]]).to(torch.int32).contiguous(), neighbor_ptr=_csr_ptr(i[keep], n))
    total, want = _unscaled(pos, q, mu, Q, every), _unscaled(pos, q, mu, Q, rest)
    corr = fn(pos, q, mu, Q, torch.zeros_like(f["scsr"]), neighbor_list=f["nl"], neighbor_ptr=f["ptr"], **NO_VIRIAL)
    for name, t, c, w in zip(NAMES, total, corr, want):
        scale = float(t.abs().max())
        err = float((t + c - w).abs().max())
        print(f"exclusion identity, {name:20s} err / largest |all-pairs value| {err / scale:.2e} (bar 1e-10)")
        assert err <= 1e-10 * scale


@pytest.mark.parametrize("fmt", ["matrix", "list"])
def test_periodic_triclinic_cell_with_the_nine_word_virial(fmt):
    fn, f = _fn(), _case("periodic")
    ref = _reference("periodic")
    cells = _cells(f)
    out = fn(*_inputs(f), cell=cells, **_kw(f, fmt), **ALL)
    for name, o in zip(NAMES, out):
        _close(o, ref[name], f"periodic {fmt} {name}", 1e-11)
    vir = out[-1][0]
    assert float((vir - vir.T).abs().max()) > 1e-3 * float(vir.abs().max()), "nine independent components"
    with pytest.raises(NotImplementedError, match="cell"):
        fn(*_inputs(f), cell=cells.clone().requires_grad_(True), **_kw(f, fmt)).sum().backward()
    with pytest.raises(ValueError, match="compute_virial needs the shifts"):
        fn(*_inputs(f), cell=cells, **_kw(f, fmt, shifts=False), compute_virial=True)


@pytest.mark.parametrize("fmt", ["matrix", "list"])
def test_minimum_image_equals_explicit_shifts_wrapped_or_not(fmt):
    """The batch of three molecules that straddle the faces of three triclinic cells: explicit shifts on the wrapped atoms against the
    yardstick (nine-word virial of every system included), and `minimum_image=True` on the wrapped atoms and on the whole molecules against
    the same outputs."""
    fn, f = _fn(), _case("molecules")
    ref = _reference("molecules")
    cells = _cells(f)
    shifted = fn(*_inputs(f), cell=cells, batch_idx=f["bi"], **_kw(f, fmt), **ALL)
    for name, o in zip(NAMES, shifted):
        _close(o, ref[name], f"molecules, shifts, {fmt} {name}", 1e-11)
    assert shifted[-1].shape == (3, 3, 3) and float(shifted[-1].abs().amax((1, 2)).min()) > 0
    for which in ("pos", "pos_whole"):
        out = fn(*_inputs(f, pos=which), cell=cells, batch_idx=f["bi"], minimum_image=True, **_kw(f, fmt, shifts=False), **ALL)
        for name, o, s in zip(NAMES, out, shifted):
            _close(o, ref[name], f"molecules, minimum image, {which}, {fmt} {name}", 1e-11)
            _close(o, s, f"molecules, minimum image against shifts, {which}, {fmt} {name}", 1e-11)
    out32 = fn(*_inputs(f, torch.float32), cell=_cells(f, torch.float32), batch_idx=f["bi"], minimum_image=True, **_kw(f, fmt, shifts=False), **ALL)
    ref32 = _reference("molecules", torch.float32, minimum_image=True)
    for name, o in zip(NAMES, out32):
        _close(o, ref32[name], f"molecules, minimum image, float32, {fmt} {name}", 1e-6)
    with pytest.raises(ValueError, match="minimum_image takes a list without shifts"):
        fn(*_inputs(f), cell=cells, batch_idx=f["bi"], minimum_image=True, **_kw(f, fmt))


# ---- autograd and tracing --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ladder70", "periodic", "molecules"])
def test_autograd_against_the_yardstick(kind):
    """`energies.sum().backward()` against the explicit outputs and the yardstick, a random upstream gradient against the yardstick's
    autograd; differentiating an explicit output is refused."""
    fn, f = _fn(), _case(kind)
    ref, refw = _reference(kind), _reference(kind, weighted=True)
    kw = dict(_kw(f, "list"), cell=_cells(f), batch_idx=f["bi"])
    leaves = [t.requires_grad_(True) for t in _inputs(f)]
    e = fn(*leaves, **kw)
    _close(e, ref["energies"], f"{kind} energies under autograd", 1e-11)
    got = torch.autograd.grad((f["w"] * e).sum(), leaves, retain_graph=True)
    for name, g, sign in zip(NAMES[1:], got, SIGNS):
        assert g.dtype == F64
        _close(sign * g, refw[name], f"{kind} autograd of the weighted sum, {name}", 1e-11)
    e.sum().backward()
    for name, leaf, sign in zip(NAMES[1:], leaves, SIGNS):
        _close(sign * leaf.grad, ref[name], f"{kind} backward, {name}", 1e-11)
    with pytest.raises(NotImplementedError):
        e, frc = fn(*leaves, **kw, compute_forces=True)
        torch.autograd.grad(frc.sum(), leaves[0])
    with pytest.raises(NotImplementedError, match="pair_scales is not differentiable"):
        fn(*_inputs(f), **dict(kw, pair_scales=f["scsr"].clone().requires_grad_(True)))


def test_autograd_through_rotate_multipoles():
    """Three water-like molecules with `LocalFrames` (bonds stretched to 1.34 so that every listed distance is >= 1.3), the bonded list of
    `bonded_pair_scales`: gradients w.r.t. positions and the local multipoles against the same pipeline in the float64 references."""
    from nvalchemiops.interactions.electrostatics import LocalFrames, bonded_pair_scales, rotate_multipoles
    from tests import local_frames_reference as LR

    gen = torch.Generator().manual_seed(17)
    parts = []
    for origin in ([0.0, 0.0, 0.0], [4.1, 0.4, -0.3], [0.5, 4.0, 1.2]):
        p, a, k = LR.water(gen)
        parts.append((1.4 * p + torch.tensor(origin, dtype=F64), a, k))
    pos, atoms, kinds, _ = LR.join(parts)
    n = pos.shape[0]
    q = torch.tensor([-0.8, 0.4, 0.4] * 3, dtype=F64)
    mu_loc, quad_loc = LR.local_multipoles(n, 18)
    mu_loc, quad_loc = 0.3 * mu_loc, 0.2 * quad_loc
    bonds = [(3 * m, 3 * m + k) for m in range(3) for k in (1, 2)]
    topo = bonded_pair_scales(bonds, n, scales=(0.0, 0.3), device=DEV)
    assert topo.neighbor_matrix.shape == (n, 2) and topo.num_neighbors.tolist() == [2] * n
    entries, s = PR.matrix_entries(topo.neighbor_matrix.cpu(), topo.pair_scales.cpu(), mask_value=n)
    w = torch.randn(n, dtype=F64, generator=gen)
    rp, rm, rq = (t.clone().requires_grad_(True) for t in (pos, mu_loc, quad_loc))
    mu_r, quad_r = LR.rotate(rp, rm, rq, atoms, kinds)
    e_ref = PR.pair_energies(rp, q, mu_r, quad_r, s, *entries)
    (w * e_ref).sum().backward()
    fr = LocalFrames(atoms.to(DEV), kinds.to(DEV))
    dp, dm, dq = (t.to(DEV).clone().requires_grad_(True) for t in (pos, mu_loc, quad_loc))
    mu, quad = rotate_multipoles(dp, dm, dq, fr)
    e = _fn()(dp, q.to(DEV), mu, quad, topo.pair_scales, neighbor_matrix=topo.neighbor_matrix, mask_value=n)
    (w.to(DEV) * e).sum().backward()
    _close(e, e_ref, "through rotate_multipoles, energies", 1e-11)
    _close(dp.grad, rp.grad, "through rotate_multipoles, dL/dpositions", 1e-11)
    _close(dm.grad, rm.grad, "through rotate_multipoles, dL/dlocal_dipoles", 1e-11)
    _close(dq.grad, rq.grad, "through rotate_multipoles, dL/dlocal_quadrupoles", 1e-11)


def test_compile_fullgraph_equals_eager_bitwise():
    """Under torch.compile the call goes through the `alchemiops::_pair_scale_correction` op, forward and backward: same bits as eager."""
    fn, f = _fn(), _case("molecules")
    cells = _cells(f)

    def forward(*args):
        e, frc, dg = fn(*args, cell=cells, batch_idx=f["bi"], minimum_image=True, compute_forces=True, compute_dipole_gradients=True,
                        **_kw(f, "matrix", shifts=False))
        return e * 2.0, frc, dg

    args = _inputs(f)
    torch._dynamo.reset()
    got = torch.compile(forward, mode="default", fullgraph=True)(*args)
    for a, b in zip(got, forward(*args)):
        assert torch.equal(a, b) and float(b.abs().max()) > 0

    def loss(*args):
        return (f["w"] * fn(*args, cell=cells, batch_idx=f["bi"], **_kw(f, "list"))).sum()

    leaves = lambda: [t.clone().requires_grad_(True) for t in args]  # noqa: E731
    x, y = leaves(), leaves()
    torch.compile(loss, mode="default", fullgraph=True)(*x).backward()
    loss(*y).backward()
    for a, b in zip(x, y):
        assert torch.equal(a.grad, b.grad) and float(b.grad.abs().max()) > 0


# ---- reproducibility, exact zeros, the helper -----------------------------------------------------------------------------------------------
def test_bit_reproducible_between_calls_and_streams():
    fn, f = _fn(), _case("molecules")
    args = _inputs(f)
    kw = dict(_kw(f, "list"), cell=_cells(f), batch_idx=f["bi"], **ALL)
    a, b = fn(*args, **kw), fn(*args, **kw)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = fn(*args, **kw)
    side.synchronize()
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert float(a[0].abs().max()) > 0


@pytest.mark.parametrize("fmt", ["matrix", "list"])
def test_unit_scales_give_exact_zeros(fmt):
    fn, f = _fn(), _case("molecules")
    kw = _kw(f, fmt)
    kw["pair_scales"] = torch.ones_like(kw["pair_scales"])  # the padding of the matrix as well
    out = fn(*_inputs(f), cell=_cells(f), batch_idx=f["bi"], **kw, **ALL)
    assert len(out) == 6 and all(not bool(o.any()) and not bool(torch.isnan(o).any()) for o in out)
    leaves = [t.requires_grad_(True) for t in _inputs(f)]
    fn(*leaves, cell=_cells(f), batch_idx=f["bi"], **kw).sum().backward()
    assert all(not bool(t.grad.any()) for t in leaves)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_bonded_pair_scales_feeds_the_operator(dtype):
    """The helper's output handed straight to the operator (chain, ring and water of the molecules case, float32 scales for float32
    positions) against the yardstick on the entries read back from the matrix."""
    from nvalchemiops.interactions.electrostatics import bonded_pair_scales

    fn, f = _fn(), _case("molecules")
    p = f["problem"]
    topo = bonded_pair_scales(p["bonds"], f["n"], dtype=dtype, device=DEV)
    assert topo.pair_scales.dtype == dtype and topo.neighbor_matrix.is_cuda
    entries, s = PR.matrix_entries(topo.neighbor_matrix, topo.pair_scales, mask_value=f["n"])
    pos, q, mu, Q = _inputs(f, dtype, pos="pos_whole")
    ref = PR.evaluate(pos, q, mu, Q, s, entries, distance_dtype=dtype)
    out = fn(pos, q, mu, Q, topo.pair_scales, neighbor_matrix=topo.neighbor_matrix, mask_value=f["n"], **NO_VIRIAL)
    for name, o in zip(NAMES, out):
        _close(o, ref[name], f"bonded_pair_scales -> operator, {dtype} {name}", 1e-11 if dtype == F64 else 1e-6)
