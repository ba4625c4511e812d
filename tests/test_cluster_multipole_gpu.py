"""`mi_coulomb_dipole`, `mi_coulomb_quadrupole`, `mi_cluster_induced_pair_tensors` and their public functions `coulomb_dipole_correction`,
`coulomb_quadrupole_correction`, `cluster_induced_dipoles` on the device, against the float64 operator-definition references at alpha = 0
(tests/cluster_multipole_reference.py, itself checked in tests/test_cluster_multipole_reference_cpu.py) on the same stored entries.

Lists are all-pairs lists built by hand in torch, independent of the neighbour search.  Shapes: one cluster of 150 atoms (rows of 149
entries: two full wave trips and a tail of 21); a batch of three clusters of 70, 2 and 1 atoms (a row longer than 64, one-entry rows, an empty
row); three atoms without dipole and quadrupole; matrix rows seven columns wider than the longest row, padded with the mask value, -1 and
N + 7; matrix and CSR.  One periodic case: 96 atoms in a triclinic box, every image within 9.0 (rows of about 290 entries, self images).

Bars.  The kernels are the pair kernels of `mi_ewald_dipole_real` / `mi_ewald_quadrupole_real` with another radial part, so they hold the bars
tests/test_dipole_gpu.py holds for that arithmetic model: 1e-11 of the largest |value| of each output for fp64 inputs, 1e-6 for float32
positions against the reference's float32-distance mode; matrix against CSR 1e-10.  The stored operator holds the same two figures, and the
solves hold the bars of tests/test_induced_gpu.py and tests/test_thole_gpu.py for reciprocal="ewald": true residual within a factor 10 of the
tolerance, |mu - mu_ref| <= 10 tol ||b|| / lambda_min(H), iterations at most two more than the reference PCG, and implicit gradients within
100 tol cond(D^1/2 H D^1/2) of the largest |component|.

Measured on the MI355X.  fp64 over every flag word: dipole 2.6e-16 - 3.0e-15, quadrupole 7.2e-16 - 3.2e-15; float32 positions: dipole
6.0e-8 - 4.3e-7, quadrupole 1.6e-7 - 4.9e-7; periodic virial 4.8e-15 / 5.3e-15; matrix against CSR 0; stored tensors 1.1e-15 (float32 2.5e-7),
product 1.4e-16 (float32 1.2e-8); solves: true residual 0.10 - 0.47 of the tolerance, iterations equal to the reference PCG's (8 / 15 on
the 150-atom cluster, 8, 4, 0 / 14, 4, 0 on the batch); implicit gradients 3.7e-13 - 1.9e-12 against bars of 1.28e-10 and 2.44e-10.
DESIGN 3.29 has the table."""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import cluster_multipole_reference as CR
from tests import gaussian_reference as GR
from tests import induced_reference as IR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
A_T = 0.39
FORCES, CHARGE_GRAD, DIPOLE_GRAD, VIRIAL, QUADRUPOLE_GRAD = 1, 2, 4, 8, 16  # MI_DP_* / MI_QD_*
OUTPUTS = {"dipole": (("forces", FORCES), ("charge_grads", CHARGE_GRAD), ("dipole_grads", DIPOLE_GRAD), ("virial", VIRIAL)),
           "quadrupole": (("forces", FORCES), ("charge_grads", CHARGE_GRAD), ("dipole_grads", DIPOLE_GRAD), ("quadrupole_grads", QUADRUPOLE_GRAD),
                          ("virial", VIRIAL))}
NAMES = {w: ("energies",) + tuple(n for n, _ in o) for w, o in OUTPUTS.items()}
ALL = {"dipole": dict(compute_forces=True, compute_charge_gradients=True, compute_dipole_gradients=True, compute_virial=True),
       "quadrupole": dict(compute_forces=True, compute_charge_gradients=True, compute_dipole_gradients=True, compute_quadrupole_gradients=True,
                          compute_virial=True)}
INPUTS = {"dipole": ("pos", "q", "mu"), "quadrupole": ("pos", "q", "mu", "Q")}


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
    print(f"{what:64s} rel err {err / scale:.2e} (bar {rel:.0e})")
    assert err <= rel * scale + 1e-14, f"{what}: max err {err:.3e} > {rel * scale:.3e}"


def _matrix(i, j, S, n, m, fill):
    """Padded matrix [n, m] (+ shifts) of entries sorted by row."""
    i, j, S = i.to(DEV), j.to(DEV), S.to(DEV)
    counts = torch.bincount(i, minlength=n)
    assert int(counts.max()) <= m
    start = torch.cumsum(counts, 0) - counts
    col = torch.arange(i.shape[0], device=DEV) - start[i]
    nm = torch.full((n, m), fill, dtype=torch.int32, device=DEV)
    sh = torch.zeros((n, m, 3), dtype=torch.int32, device=DEV)
    nm[i, col] = j.to(torch.int32)
    sh[i, col] = S.to(torch.int32)
    return nm, sh


def _csr(nm, sh, mask):
    i, j, S = GR.entries_from_matrix(nm, sh, mask)
    n = nm.shape[0]
    ptr = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    ptr[1:] = torch.cumsum(torch.bincount(i, minlength=n), 0)
    return torch.stack([i, j]).to(torch.int32).contiguous(), ptr, S.to(torch.int32).contiguous()


def _lists(i, j, S, n, periodic):
    """dict(nm, sh, nl, ptr, lsh, ent) of a full list.  The matrix is seven columns wider than the longest row and padded with the mask value n,
    with -1 in the last column and N + 7 in every other row of the one before: three kinds of padding."""
    nm, sh = _matrix(i, j, S, n, int(torch.bincount(i, minlength=n).max()) + 7, n)
    nl, ptr, lsh = _csr(nm, sh, n)
    assert bool((nm[:, -7:] == n).all())
    nm[:, -1] = -1
    nm[::2, -2] = n + 7
    f = dict(n=n, nm=nm.contiguous(), sh=sh.contiguous(), nl=nl, ptr=ptr, lsh=lsh, ent=(i.to(DEV), j.to(DEV), S.to(DEV)))
    if not periodic:
        f["sh"] = f["lsh"] = None
    return f


def _kw(f, fmt):
    if fmt == "matrix":
        return dict(neighbor_matrix=f["nm"], neighbor_matrix_shifts=f["sh"], mask_value=f["n"])
    return dict(neighbor_list=f["nl"], neighbor_ptr=f["ptr"], neighbor_shifts=f["lsh"])


def _api(which=None):
    from nvalchemiops.interactions.electrostatics import (InducedDipoleError, cluster_induced_dipoles, coulomb_dipole_correction,
                                                          coulomb_quadrupole_correction, thole_dipole_correction)

    if which is None:
        return cluster_induced_dipoles, coulomb_dipole_correction, thole_dipole_correction, InducedDipoleError
    return coulomb_dipole_correction if which == "dipole" else coulomb_quadrupole_correction


@functools.lru_cache(maxsize=None)
def _case(kind):
    """"c150" and "batch": the problems of tests/cluster_multipole_reference.py (no cell); "periodic": its triclinic box."""
    if kind == "periodic":
        p = CR.periodic_problem()
        i, j, S = p["entries"]
        counts = torch.bincount(i, minlength=p["n"])
        assert int(counts.min()) > 64 and bool((counts % 64 != 0).any()) and bool(((i == j) & (S != 0).any(-1)).any())
        f = _lists(i, j, S, p["n"], True)
        f.update(kind=kind, nsys=1, cells=p["cell"][None], bi=None, **{k: p[k] for k in ("pos", "q", "mu", "Q")}, w=_t(p["w"]))
        return f
    p = CR.problem(kind)
    i, j, S = p["entries"]
    counts = torch.bincount(i, minlength=p["n"]).tolist()
    assert counts[0] == (149 if kind == "c150" else 69) and (kind == "c150" or counts[-3:] == [1, 1, 0])
    f = _lists(i, j, S, p["n"], False)
    f.update(kind=kind, nsys=1, cells=None, bi=None, problem=p, **{k: p[k] for k in ("pos", "q", "mu", "Q")}, w=_t(p["w"]))
    return f


@functools.lru_cache(maxsize=None)
def _reference(which, kind, dtype, weighted=False):
    f = _case(kind)
    args = [_t(f[k], dtype) for k in INPUTS[which]]
    cells = None if f["cells"] is None else _t(f["cells"], dtype)
    fn = CR.dipole_evaluate if which == "dipole" else CR.quadrupole_evaluate
    return fn(*args, f["ent"], cell=cells, distance_dtype=dtype, weights=f["w"] if weighted else None)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def _capi(which, arrays, cells, bi, nsys, idx, sh, nptr, m, mask, flags, weights=None, energies=True):
    """One `mi_coulomb_dipole` / `mi_coulomb_quadrupole` call into NaN-filled buffers: dict of every output buffer, asked for or not (virial:
    folded [nsys, 3, 3])."""
    from nvalchemiops import _capi as C
    import ctypes

    P = arrays[0]
    L, n, dt = C.lib(), P.shape[0], P.dtype
    name = f"mi_coulomb_{which}"
    nan = lambda *shape, dtype=F64: torch.full(shape, float("nan"), dtype=dtype, device=DEV)  # noqa: E731
    out = dict(energies=nan(n), forces=nan(n, 3, dtype=dt), charge_grads=nan(n), dipole_grads=nan(n, 3), quadrupole_grads=nan(n, 3, 3),
               virial=nan(nsys, getattr(L, name + "_blocks")(), 9))
    nbytes = int(getattr(L, name + "_scratch_bytes")(n, C.dtype_code(dt)))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    ask = lambda key, bit: C.ptr(out[key]) if flags & bit else None  # noqa: E731
    outs = [C.ptr(out["energies"]) if energies else None, ask("forces", FORCES), ask("charge_grads", CHARGE_GRAD), ask("dipole_grads", DIPOLE_GRAD)]
    if which == "quadrupole":
        outs.append(ask("quadrupole_grads", QUADRUPOLE_GRAD))
    rc = getattr(L, name)(*[C.ptr(a) for a in arrays], C.ptr(cells), C.ptr(bi), C.ptr(weights), n, nsys, C.dtype_code(dt), C.ptr(idx), C.ptr(sh),
                          C.ptr(nptr), m, mask, flags, *outs, ask("virial", VIRIAL), C.ptr(scratch), ctypes.c_size_t(nbytes), C.stream_of(P))
    C.check(rc, name)
    out["virial"] = out["virial"].sum(1).reshape(nsys, 3, 3)
    if which == "dipole":
        assert bool(torch.isnan(out.pop("quadrupole_grads")).all())
    return out


def _abi_inputs(which, f, dtype, fmt):
    arrays = [_t(f[k], dtype) for k in INPUTS[which]]
    cells = None if f["cells"] is None else _t(f["cells"], dtype)
    lay = (f["nm"], f["sh"], None, f["nm"].shape[1]) if fmt == "matrix" else (f["nl"][1].contiguous(), f["lsh"], f["ptr"], 0)
    return (arrays, cells, f["bi"], f["nsys"]) + lay + (f["n"],)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("fmt", ["matrix", "csr"])
@pytest.mark.parametrize("kind", ["c150", "batch"])
@pytest.mark.parametrize("which", ["dipole", "quadrupole"])
def test_c_abi_every_flag_combination_against_the_reference(which, kind, fmt, dtype):
    """Parity of every output under every flag word, and only what was asked for is written."""
    f = _case(kind)
    ref = _reference(which, kind, dtype)
    rel = 1e-11 if dtype == torch.float64 else 1e-6
    args = _abi_inputs(which, f, dtype, fmt)
    bits = [b for _, b in OUTPUTS[which] if b != VIRIAL]  # a cluster has no virial
    worst = {}
    for r in range(len(bits) + 1):
        for combo in itertools.combinations(bits, r):
            flags = sum(combo)
            out = _capi(which, *args, flags)
            for name, bit in (("energies", 0),) + OUTPUTS[which]:
                if bit and not flags & bit:
                    assert bool(torch.isnan(out[name]).all()), f"{name} was written without being asked for (flags {flags})"
                    continue
                got, want = _np(out[name]), ref[name]
                assert not np.isnan(got).any(), (name, flags)
                scale = np.abs(want).max()
                err = np.abs(got - want).max() / scale
                worst[name] = max(worst.get(name, 0.0), err)
                assert err <= rel + 1e-14 / scale, f"{which} {kind} {fmt} {dtype} flags {flags} {name}: rel err {err:.3e} > {rel:.0e}"
    print(f"{which} {kind} {fmt} {dtype}: worst rel err over {2 ** len(bits)} flag words (bar {rel:.0e}): "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    if kind == "batch":  # the lone atom has an empty row: exact zeros
        full = _capi(which, *args, sum(bits))
        assert all(float(full[k][-1].abs().max()) == 0.0 for k in NAMES[which] if k != "virial")


@pytest.mark.parametrize("which", ["dipole", "quadrupole"])
def test_c_abi_weights_give_the_adjoint_and_energies_may_be_null(which):
    f = _case("batch")
    ref = _reference(which, "batch", torch.float64, weighted=True)
    flags = sum(b for _, b in OUTPUTS[which] if b != VIRIAL)
    out = _capi(which, *_abi_inputs(which, f, torch.float64, "csr"), flags, weights=f["w"], energies=False)
    assert bool(torch.isnan(out["energies"]).all())
    for name, bit in OUTPUTS[which]:
        if bit != VIRIAL:
            _close(out[name], ref[name], f"{which} weighted {name}", 1e-11)


# ---- the public functions --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c150", "batch"])
@pytest.mark.parametrize("which", ["dipole", "quadrupole"])
def test_public_function_outputs_and_adjoint(which, kind):
    """Explicit outputs against the reference in both formats, matrix against CSR, a subset of the flags, gradients of sum_i g_i E_i (random g)
    from autograd against the reference's autograd, `energies.sum().backward()` against the explicit outputs, float32 dtypes."""
    fn = _api(which)
    f = _case(kind)
    ref, refw = _reference(which, kind, torch.float64), _reference(which, kind, torch.float64, weighted=True)
    flags = dict(ALL[which], compute_virial=False)
    names = [k for k in NAMES[which] if k != "virial"]
    inputs = lambda: [_t(f[k]) for k in INPUTS[which]]  # noqa: E731
    outs = {}
    for fmt in ("matrix", "list"):
        out = outs[fmt] = fn(*inputs(), **_kw(f, fmt), **flags)
        assert all(o.dtype == F64 for o in out) and len(out) == len(names)
        for name, o in zip(names, out):
            _close(o, ref[name], f"{which} {kind} {fmt} {name}", 1e-11)
        # a subset of the flags: the same bits
        e, dg = fn(*inputs(), **_kw(f, fmt), compute_dipole_gradients=True)
        assert torch.equal(e, out[0]) and torch.equal(dg, out[3])
        leaves = [t.requires_grad_(True) for t in inputs()]
        e = fn(*leaves, **_kw(f, fmt))
        assert isinstance(e, torch.Tensor) and torch.equal(e.detach(), out[0])
        got = torch.autograd.grad((f["w"] * e).sum(), leaves, retain_graph=True)
        for name, g, sign in zip(names[1:], got, (-1.0, 1.0, 1.0, 1.0)):
            _close(sign * g, refw[name], f"{which} {kind} {fmt} autograd of the weighted sum, {name}", 1e-11)
        e.sum().backward()
        for name, leaf, o, sign in zip(names[1:], leaves, out[1:], (-1.0, 1.0, 1.0, 1.0)):
            _close(sign * leaf.grad, o, f"{which} {kind} {fmt} backward against the explicit {name}", 1e-11)
    for name, a, b in zip(names, outs["matrix"], outs["list"]):
        _close(a, b, f"{which} {kind} matrix against CSR, {name}", 1e-10)
    if kind == "batch":
        with pytest.raises(NotImplementedError):
            e, frc = fn(*leaves, **_kw(f, "matrix"), compute_forces=True)
            torch.autograd.grad(frc.sum(), leaves[0])
        out32 = fn(*[t.float() for t in inputs()], **_kw(f, "list"), **flags)
        assert all(o.dtype == torch.float32 for o in out32)
        ref32 = _reference(which, kind, torch.float32)
        for name, o in zip(names, out32):
            _close(o, ref32[name], f"{which} {kind} float32 {name}", 1e-6)
        if which == "quadrupole":  # dipoles=None is no dipoles
            mu0 = torch.zeros((f["n"], 3), dtype=F64, device=DEV)
            a, b = fn(_t(f["pos"]), _t(f["q"]), None, _t(f["Q"]), **_kw(f, "list"), **flags), fn(_t(f["pos"]), _t(f["q"]), mu0, _t(f["Q"]), **_kw(f, "list"), **flags)
            assert all(torch.equal(x, y) for x, y in zip(a, b))
            sym = 0.5 * (_t(f["Q"]) + _t(f["Q"]).transpose(1, 2))  # 1/2 (Q + Q^T) of the input is used
            for x, y in zip(fn(_t(f["pos"]), _t(f["q"]), _t(f["mu"]), sym, **_kw(f, "list"), **flags), outs["list"]):
                _close(x, y, "symmetrised quadrupoles", 1e-13)


@pytest.mark.parametrize("fmt", ["matrix", "list"])
def test_zero_multipoles_give_exact_zeros(fmt):
    """Zero dipoles: every output of the dipole correction but dipole_grads (minus the field of the charges) is exactly zero.  Zero
    quadrupoles: every output of the quadrupole correction but quadrupole_grads (the field gradient) is exactly zero."""
    f = _case("c150")
    P, Q, M, QQ = (_t(f[k]) for k in ("pos", "q", "mu", "Q"))
    flags = {w: dict(ALL[w], compute_virial=False) for w in ALL}
    out = _api("dipole")(P, Q, torch.zeros_like(M), **_kw(f, fmt), **flags["dipole"])
    assert all(bool((out[k] == 0).all()) for k in (0, 1, 2)) and float(out[3].abs().amax(1).min()) > 0
    out = _api("quadrupole")(P, Q, M, torch.zeros_like(QQ), **_kw(f, fmt), **flags["quadrupole"])
    assert all(bool((out[k] == 0).all()) for k in (0, 1, 2, 3)) and float(out[4].abs().amax((1, 2)).min()) > 0


@pytest.mark.parametrize("which", ["dipole", "quadrupole"])
def test_periodic_cut_off_sum_with_the_nine_word_virial(which):
    """With a cell and shifts the routines are the cut-off sum over the listed images: every output, the virial included, against the
    reference at alpha = 0; a gradient with respect to the cell is refused."""
    fn = _api(which)
    f = _case("periodic")
    ref, refw = _reference(which, "periodic", torch.float64), _reference(which, "periodic", torch.float64, weighted=True)
    cells = _t(f["cells"])
    inputs = lambda: [_t(f[k]) for k in INPUTS[which]]  # noqa: E731
    outs = {}
    for fmt in ("matrix", "list"):
        out = outs[fmt] = fn(*inputs(), cells, **_kw(f, fmt), **ALL[which])
        for name, o in zip(NAMES[which], out):
            _close(o, ref[name], f"periodic {which} {fmt} {name}", 1e-11)
    vir = outs["matrix"][-1][0]
    assert float((vir - vir.T).abs().max()) > 1e-3 * float(vir.abs().max()), "nine independent components"
    for name, a, b in zip(NAMES[which], outs["matrix"], outs["list"]):
        _close(a, b, f"periodic {which} matrix against CSR, {name}", 1e-10)
    leaves = [t.requires_grad_(True) for t in inputs()]
    e = fn(*leaves, cells, **_kw(f, "list"))
    for name, g, sign in zip(NAMES[which][1:], torch.autograd.grad((f["w"] * e).sum(), leaves), (-1.0, 1.0, 1.0, 1.0)):
        _close(sign * g, refw[name], f"periodic {which} autograd of the weighted sum, {name}", 1e-11)
    with pytest.raises(NotImplementedError, match="cell"):
        fn(*inputs(), cells.clone().requires_grad_(True), **_kw(f, "list")).sum().backward()
    with pytest.raises(ValueError, match="compute_virial needs the shifts"):
        fn(*inputs(), cells, neighbor_matrix=f["nm"], mask_value=f["n"], compute_virial=True)


@pytest.mark.parametrize("which", ["dipole", "quadrupole"])
def test_bit_reproducible_between_calls_and_streams(which):
    fn = _api(which)
    f = _case("c150")
    args = [_t(f[k]) for k in INPUTS[which]]
    kw = dict(**_kw(f, "list"), **dict(ALL[which], compute_virial=False))
    a, b = fn(*args, **kw), fn(*args, **kw)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = fn(*args, **kw)
    side.synchronize()
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert float(a[0].abs().max()) > 0


@pytest.mark.parametrize("which", ["dipole", "quadrupole"])
def test_compile_fullgraph_equals_eager_bitwise(which):
    """Under torch.compile the call goes through the `alchemiops::_coulomb_*_correction` op, forward and backward: same bits as eager."""
    fn = _api(which)
    f = _case("batch")

    def forward(*args):
        e, frc, dg = fn(*args, compute_forces=True, compute_dipole_gradients=True, **_kw(f, "matrix"))
        return e * 2.0, frc, dg

    args = [_t(f[k]) for k in INPUTS[which]]
    torch._dynamo.reset()
    got = torch.compile(forward, mode="default", fullgraph=True)(*args)
    for a, b in zip(got, forward(*args)):
        assert torch.equal(a, b) and float(b.abs().max()) > 0

    def loss(*args):
        return (f["w"] * fn(*args, **_kw(f, "list"))).sum()

    leaves = lambda: [t.clone().requires_grad_(True) for t in args]  # noqa: E731
    x, y = leaves(), leaves()
    torch.compile(loss, mode="default", fullgraph=True)(*x).backward()
    loss(*y).backward()
    for a, b in zip(x, y):
        assert torch.equal(a.grad, b.grad) and float(b.grad.abs().max()) > 0


# ---- the stored operator ---------------------------------------------------------------------------------------------------------------
def _tensors(thole, pos, polar, idx, nptr, m, mask):
    from nvalchemiops import _capi as C

    L, n, slots = C.lib(), pos.shape[0], idx.numel()
    ten = torch.full((L.mi_induced_tensor_words(), slots), float("nan"), dtype=F64, device=DEV)
    nbr = torch.full((slots,), -12345, dtype=torch.int32, device=DEV)
    diag, pre = torch.full((n,), float("nan"), dtype=F64, device=DEV), torch.full((n,), float("nan"), dtype=F64, device=DEV)
    rc = L.mi_cluster_induced_pair_tensors(C.ptr(pos), C.ptr(polar), n, C.dtype_code(pos.dtype), C.ptr(idx), C.ptr(nptr), m, mask, slots, C.ptr(ten),
                                           C.ptr(nbr), C.ptr(diag), C.ptr(pre), C.cdouble(0.0 if thole is None else thole), C.stream_of(pos))
    C.check(rc, "mi_cluster_induced_pair_tensors")
    return ten, nbr, diag, pre


def _apply(ten, nbr, diag, x, nptr, m):
    from nvalchemiops import _capi as C

    y = torch.full((x.shape[0], 3), float("nan"), dtype=F64, device=DEV)
    rc = C.lib().mi_induced_apply(C.ptr(ten), C.ptr(nbr), C.ptr(diag), C.ptr(x), None, None, x.shape[0], 1, C.ptr(nptr), m, nbr.numel(), C.ptr(y), None,
                                  C.stream_of(x))
    C.check(rc, "mi_induced_apply")
    return y


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("fmt", ["matrix", "csr"])
@pytest.mark.parametrize("kind", ["c150", "batch"])
def test_stored_tensors_against_the_reference_and_the_pair_kernels(kind, fmt, dtype):
    """Undamped: B1 I - B2 R R^T of every slot against `induced_reference.pair_tensors` at alpha = 0 (zero on padding and on entries with a
    non-polarisable atom at either end, whose neighbour index is the row's own).  Damped: `mi_induced_apply` on a random x against
    x / a + dipole_grads of `coulomb_dipole_correction` + `thole_dipole_correction` at zero charges and mu = x."""
    _, dp, th, _ = _api()
    f = _case(kind)
    n, p = f["n"], f["problem"]
    P, A = _t(f["pos"], dtype), _t(p["polar"], dtype)
    rel = 1e-11 if dtype == torch.float64 else 1e-6
    idx, nptr, m = (f["nm"], None, f["nm"].shape[1]) if fmt == "matrix" else (f["nl"][1].contiguous(), f["ptr"], 0)
    ten, nbr, diag, pre = _tensors(None, P, A, idx, nptr, m, n)
    assert int(nbr.min()) >= 0 and int(nbr.max()) < n and not bool(torch.isnan(ten).any())
    ok = A.to(F64) > 0
    frozen = list(CR.FROZEN)
    assert bool((diag[frozen] == 1).all()) and bool((pre[frozen] == 1).all()) and torch.equal(pre[ok], A.to(F64)[ok])
    assert torch.equal(diag[ok], 1.0 / A.to(F64)[ok])
    if fmt == "matrix":
        nm = f["nm"].long()
        pad = (nm == n) | (nm < 0) | (nm >= n)
        rows = torch.arange(n, device=DEV).unsqueeze(1).expand_as(nm)
        i, j = rows[~pad], nm[~pad]
        live = (~pad).reshape(-1)
        dead = pad | ~ok.unsqueeze(1) | ~ok[nm.clamp(0, n - 1)]
        assert bool(pad.any()) and bool((ten[:, dead.reshape(-1)] == 0).all()) and bool((nbr[dead.reshape(-1)] == rows[dead].to(torch.int32)).all())
    else:
        i, j = f["nl"][0].long(), f["nl"][1].long()
        live = torch.ones(idx.numel(), dtype=torch.bool, device=DEV)
    want = CR.pair_tensors(P, (i, j, torch.zeros((i.shape[0], 3), dtype=torch.long, device=DEV)), distance_dtype=dtype)
    want = torch.where((ok[i] & ok[j])[:, None, None], want, torch.zeros_like(want))
    b1, b2, R = ten[0, live], ten[1, live], ten[2:, live].T
    got = b1[:, None, None] * torch.eye(3, dtype=F64, device=DEV) - b2[:, None, None] * R[:, :, None] * R[:, None, :]
    _close(got, want, f"undamped stored tensors {kind} {fmt} {dtype}", rel)
    # the damped operator through its product
    ten_d, nbr_d, diag_d, _ = _tensors(A_T, P, A, idx, nptr, m, n)
    assert torch.equal(ten_d[2:], ten[2:]) and torch.equal(nbr_d, nbr) and not torch.equal(ten_d[:2], ten[:2])
    x = _t(np.random.default_rng(23).normal(size=(n, 3)))
    mask = ok.to(F64).unsqueeze(1)
    xm, zero = (x * mask).to(dtype), torch.zeros(n, dtype=dtype, device=DEV)
    kw = dict(compute_dipole_gradients=True, **_kw(f, "matrix" if fmt == "matrix" else "list"))
    for thole, tt, dd in ((None, ten, diag), (A_T, ten_d, diag_d)):
        dg = dp(P, zero, xm, **kw)[1].to(F64)
        if thole is not None:
            dg = dg + th(P, zero, xm, A, None, thole=thole, **kw)[1].to(F64)
        _close(_apply(tt, nbr, dd, x, nptr, m), dd.unsqueeze(1) * x + dg * mask, f"product {kind} {fmt} {dtype} thole {thole} against the pair kernels", rel)
    with pytest.raises(Exception, match="thole_a"):
        _tensors(-1.0, P, A, idx, nptr, m, n)


# ---- solves ----------------------------------------------------------------------------------------------------------------------------
def _per_system(v, bi, nsys):
    return torch.sqrt(torch.zeros(nsys, dtype=F64, device=DEV).index_add(0, bi.long(), (v.to(F64) ** 2).sum(1)))


def _check_solution(out, H, b, polar, bi, nsys, tol, what):
    """The checks of tests/test_induced_gpu.py and tests/test_thole_gpu.py with the dense H of the cluster: true residual, dipoles, polarisation
    energy, iteration count against the reference PCG."""
    mu = out.dipoles.to(F64)
    assert not bool(torch.isnan(mu).any())
    b_norm = _per_system(b.reshape(-1, 3), bi, nsys)
    res = _per_system((b - H @ mu.reshape(-1)).reshape(-1, 3), bi, nsys)
    factor = torch.where(b_norm > 0, res / (tol * b_norm.clamp(min=1e-300)), torch.zeros_like(res))
    mu_ref = IR.solve(H, b, bi, nsys)
    d = IR.preconditioner(polar)
    counts = []
    for s in range(nsys):
        m = torch.nonzero(bi.long().repeat_interleave(3) == s).flatten()
        ev = torch.linalg.eigvalsh(H[m][:, m])
        assert float(ev.min()) > 0, "the test problem must be positive definite"
        bound = 10.0 * tol * float(b_norm[s]) / float(ev.min()) + 1e-14
        assert float((mu.reshape(-1)[m] - mu_ref.reshape(-1)[m]).abs().max()) <= bound, (what, s)
        counts.append(IR.pcg(H[m][:, m], b[m], d[m], tol)[1])
        u = float(IR.energy(H[m][:, m], b[m], mu_ref.reshape(-1)[m]))
        assert abs(float(out.polarization_energy[s]) - u) <= 100.0 * tol * abs(u) + 1e-14, (what, s)
    print(f"{what}: true residual / (tolerance ||b||) per system {[round(float(v), 3) for v in factor]}, iterations {out.iterations.tolist()} "
          f"(reference PCG {counts}), reported residual {[float(v) for v in out.residual]}")
    assert bool((factor <= 10.0).all()), "the true residual drifted more than a factor 10 above the tolerance"
    assert all(int(got) <= ref + 2 for got, ref in zip(out.iterations.tolist(), counts)), (out.iterations.tolist(), counts)
    assert bool((out.residual <= tol).all())
    return mu_ref


@functools.lru_cache(maxsize=None)
def _solver_case(kind, damped):
    """The solver problem: polarisabilities small enough for H > 0 undamped, four times those with `thole=0.39`."""
    f = dict(_case(kind))
    p = f["problem"]
    H, b, c, polar = CR.dense_problem(p, A_T if damped else None, DEV, 4.0 if damped else 1.0)
    f.update(H=H, b=b, c=c, polar=polar, field=_t(p["field"]), bi=_t(p["batch_idx"]), nsys=p["nsys"], thole=A_T if damped else None)
    return f


@pytest.mark.parametrize("fmt", ["matrix", "list"])
@pytest.mark.parametrize("damped", [False, True], ids=["undamped", "thole"])
@pytest.mark.parametrize("kind", ["c150", "batch"])
def test_solve_against_the_dense_reference(kind, damped, fmt):
    solve, dp, th, _ = _api()
    f, tol = _solver_case(kind, damped), 1e-10
    P, Q, A, n, nsys = _t(f["pos"]), _t(f["q"]), f["polar"], f["n"], f["nsys"]
    lists = {k: v for k, v in _kw(f, fmt).items() if k in ("neighbor_matrix", "neighbor_list", "neighbor_ptr")}
    batch = dict(batch_idx=f["bi"], num_systems=nsys) if nsys > 1 else {}
    out = solve(P, Q, A, thole=f["thole"], external_field=f["field"], tolerance=tol, return_info=True, **batch, **lists)
    assert out.dipoles.dtype == F64 and out.iterations.shape == (nsys,) and out.iterations.dtype == torch.int64
    _check_solution(out, f["H"], f["b"], A, f["bi"], nsys, tol, f"cluster {kind} {'thole' if damped else 'undamped'} {fmt}")
    mu = out.dipoles
    assert bool((mu[list(CR.FROZEN)] == 0).all()) and float(mu.abs().amax(1)[A > 0].min()) > 0
    # without return_info: the same dipoles, bit for bit
    assert torch.equal(solve(P, Q, A, thole=f["thole"], external_field=f["field"], tolerance=tol, **batch, **lists), mu)
    # stationarity with the public gradient calls at the returned dipoles
    pub = dict(compute_dipole_gradients=True, **_kw(f, fmt))
    e, dg = dp(P, Q, mu, **pub)
    if damped:
        e_th, dg_th = th(P, Q, mu, A, None, thole=A_T, **pub)
        e, dg = e + e_th, dg + dg_th
    ok = (A > 0).unsqueeze(1)
    a = torch.where(ok, A.unsqueeze(1), torch.ones_like(mu))
    grad = torch.where(ok, mu / a + dg - f["field"], torch.zeros_like(mu))
    stat = _per_system(grad, f["bi"], nsys) / (tol * _per_system(f["b"].reshape(-1, 3), f["bi"], nsys))
    print(f"stationarity with the public functions / (tolerance ||b||): {[round(float(v), 3) for v in stat]}")
    assert bool((stat <= 10.0).all())
    # U at the solution from the public energies
    per_atom = torch.where(ok[:, 0], (mu * mu).sum(1) / (2.0 * a[:, 0]), torch.zeros_like(e)) + e - (mu * f["field"]).sum(1)
    u = torch.zeros(nsys, dtype=F64, device=DEV).index_add(0, f["bi"].long(), per_atom)
    assert bool(((out.polarization_energy - u).abs() <= 100.0 * tol * u.abs() + 1e-14).all())
    if damped:  # the undamped solve of the same problem gives other dipoles, or none at all
        assert f["thole"] == A_T


def test_two_atom_closed_forms_breakdown_and_damping():
    """Two identical atoms at distance r in a uniform field F: mu = a F / (1 - 2 a / r^3) along the axis, a F / (1 + a / r^3) across it.  With
    a = 1.01 r^3 / 2 the undamped operator is not positive definite -- the field along the axis is the search direction of negative
    curvature -- and the damped one converges to the dense damped solution."""
    solve, _, _, Err = _api()
    r, a, F, tol = 2.5, 1.3, 0.07, 1e-12
    P, Q = _t(np.array([[0.0, 0.0, 0.0], [r, 0.0, 0.0]])), torch.zeros(2, dtype=F64, device=DEV)
    nm = _t(np.array([[1, 2], [0, 2]], dtype=np.int32))
    for axis, want in ((0, a * F / (1.0 - 2.0 * a / r**3)), (1, a * F / (1.0 + a / r**3)), (2, a * F / (1.0 + a / r**3))):
        field = torch.zeros((2, 3), dtype=F64, device=DEV)
        field[:, axis] = F
        out = solve(P, Q, a, external_field=field, neighbor_matrix=nm, tolerance=tol, return_info=True)
        expect = torch.zeros_like(field)
        expect[:, axis] = want
        assert float((out.dipoles - expect).abs().max()) <= 10.0 * tol * abs(want), (axis, out)
        assert abs(float(out.polarization_energy[0]) + want * F) <= 100.0 * tol * abs(want * F)  # U = -1/2 sum mu . F
    big = 1.01 * r**3 / 2.0
    field = torch.zeros((2, 3), dtype=F64, device=DEV)
    field[:, 0] = F
    with pytest.raises(Err, match="cluster_induced_dipoles: the operator is not positive definite for system 0"):
        solve(P, Q, big, external_field=field, neighbor_matrix=nm)
    out = solve(P, Q, big, thole=A_T, external_field=field, neighbor_matrix=nm, tolerance=tol, return_info=True)
    polar = torch.full((2,), big, dtype=F64, device=DEV)
    ent = tuple(e.to(DEV) for e in CR.all_pairs((2,)))
    T, c = CR.operator(P, Q, polar, A_T, ent)
    mu_ref = IR.solve(IR.system_matrix(T, polar), IR.right_hand_side(c, polar, field))
    assert float((out.dipoles - mu_ref).abs().max()) <= 1e-9 * float(mu_ref.abs().max()) and int(out.iterations[0]) <= 3
    with pytest.raises(Err, match="no convergence to tolerance"):
        f = _solver_case("batch", False)
        solve(_t(f["pos"]), _t(f["q"]), f["polar"], external_field=f["field"], batch_idx=f["bi"], num_systems=3, neighbor_matrix=f["nm"],
              tolerance=1e-14, max_iterations=2)


def test_warm_start_bit_reproducibility_and_side_stream():
    solve, _, _, _ = _api()
    f, tol = _solver_case("batch", True), 1e-10
    args = (_t(f["pos"]), _t(f["q"]), f["polar"])
    kw = dict(thole=A_T, external_field=f["field"], batch_idx=f["bi"], num_systems=3, neighbor_list=f["nl"], neighbor_ptr=f["ptr"], tolerance=tol)
    a = solve(*args, return_info=True, **kw)
    b = solve(*args, **kw)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = solve(*args, **kw)
    side.synchronize()
    assert torch.equal(a.dipoles, b) and torch.equal(a.dipoles, c) and float(b.abs().max()) > 0
    # the solution as warm start is accepted before any iteration counts (at a looser tolerance: the true residual of a solve is within a
    # factor 10 of its own); a start near the solution needs no more iterations than the cold start
    warm = solve(*args, initial_dipoles=a.dipoles, return_info=True, **dict(kw, tolerance=1e-8))
    assert warm.iterations.tolist() == [0, 0, 0] and bool((warm.residual <= 1e-8).all()) and torch.equal(warm.dipoles, a.dipoles)
    near = a.dipoles * (1.0 + 1e-3)
    again = solve(*args, initial_dipoles=near, return_info=True, **kw)
    assert int(again.iterations[0]) <= int(a.iterations[0]) and bool((again.residual <= tol).all())
    assert float((again.dipoles - a.dipoles).abs().max()) <= 1e-7 * float(a.dipoles.abs().max())
    # float32 positions: the dipoles come back in float32 and agree with the float64 solve to float32 accuracy
    out32 = solve(args[0].float(), args[1].float(), args[2].float(), **dict(kw, external_field=f["field"].float(), tolerance=1e-6))
    assert out32.dtype == torch.float32 and float((out32.double() - a.dipoles).abs().max()) <= 1e-4 * float(a.dipoles.abs().max())


# Relative to the largest |component| of each gradient, the bar of `test_gradients_against_the_reference_autograd` in tests/test_induced_gpu.py
# and tests/test_thole_gpu.py: both solves run to tolerance 1e-12, an error of that size in mu or z is amplified by at most the condition number
# of D^1/2 H D^1/2 (taken from the reference inside the test), and a factor 100 covers the rounding of the public energy functions' adjoints.
@pytest.mark.parametrize("damped", [False, True], ids=["undamped", "thole"])
def test_implicit_gradients_against_the_reference_autograd(damped):
    solve, _, _, _ = _api()
    f, tol = _case("batch"), 1e-12
    p, n = f["problem"], f["n"]
    thole, scale = (A_T, 4.0) if damped else (None, 1.0)
    w = _t(np.random.default_rng(91).normal(size=(n, 3)))
    bi = _t(p["batch_idx"])
    names = ["pos", "q", "polar", "field"]
    leaves = lambda: dict(pos=_t(p["pos"]).requires_grad_(True), q=_t(p["q"]).requires_grad_(True),  # noqa: E731
                          polar=_t(scale * p["polar"]).requires_grad_(True), field=_t(p["field"]).requires_grad_(True))
    r = leaves()
    T, lin = CR.operator(r["pos"], r["q"], r["polar"], thole, f["ent"], differentiable=True)
    H, b = IR.system_matrix(T, r["polar"]), IR.right_hand_side(lin, r["polar"], r["field"])
    mu_ref = IR.solve(H, b, bi, 3)
    ref = dict(zip(names, torch.autograd.grad((w * mu_ref).sum(), [r[k] for k in names])))
    ev = IR.scaled_spectrum(H.detach(), r["polar"].detach())
    assert float(ev.min()) > 0
    bar = 100.0 * tol * float(ev.max() / ev.min())
    d = leaves()
    mu = solve(d["pos"], d["q"], d["polar"], thole=thole, external_field=d["field"], batch_idx=bi, num_systems=3, neighbor_matrix=f["nm"],
               tolerance=tol)
    assert float((mu.detach() - mu_ref.detach()).abs().max()) <= 1e-9 * float(mu_ref.detach().abs().max())
    got = dict(zip(names, torch.autograd.grad((w * mu).sum(), [d[k] for k in names])))
    ok = _t(p["polar"]) > 0
    ref["polar"] = torch.where(ok, ref["polar"], torch.zeros_like(ref["polar"]))  # a non-polarisable atom has no polarisability gradient
    errs = {k: float((torch.nan_to_num(got[k]) - ref[k]).abs().max()) / float(ref[k].abs().max()) for k in names}
    print(f"implicit gradients, {'thole' if damped else 'undamped'} (bar {bar:.2e}): " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k in names:
        assert got[k].shape == d[k].shape and got[k].dtype == F64
        assert errs[k] <= bar, (k, errs[k])
