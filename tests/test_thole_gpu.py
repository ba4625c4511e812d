"""`mi_thole_dipole`, `thole_dipole_correction`, `mi_thole_induced_pair_tensors` and `thole_induced_dipoles` on the device against the float64
restatement of the model (tests/thole_reference.py, itself checked in tests/test_thole_reference_cpu.py) on the same stored entries.

Bars.  The kernel is the pair kernel of `mi_ewald_dipole_real` with another radial part, so it holds the bars tests/test_dipole_gpu.py holds for
that arithmetic model: 1e-11 of the largest |value| of each output for fp64 inputs, 1e-6 for float32 positions against the reference's
float32-distance mode.  The stored operator holds the product bar of tests/test_induced_gpu.py (the same two figures), and the solves hold
its residual and |mu - mu_ref| bars: true residual within a factor 10 of the tolerance, |mu - mu_ref| <= 10 tol ||b|| / lambda_min(H).

Measured on the MI355X.  fp64: 1.2e-16 - 5.0e-15 over every flag word of every case.  float32 positions: the 1e-6 bar holds despite the steeper
e^-E -- single 5.5e-10 - 3.3e-8, batch 1.2e-7 - 7.6e-7 (polarizability_grads the largest), cluster 1.9e-11 - 3.5e-8 -- so no wider bar is
used; for scale, the reference's float32-distance mode against its float64 mode on the same inputs is 7.9e-7 - 1.3e-6 (printed by the test).
DESIGN 3.23 has the other figures."""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import gaussian_reference as GR
from tests import induced_cases as IC
from tests import induced_reference as IR
from tests import thole_cases as TC
from tests import thole_reference as TR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
A_T = TC.THOLE
FORCES, CHARGE_GRAD, DIPOLE_GRAD, VIRIAL, POLAR_GRAD = 1, 2, 4, 8, 16  # MI_DP_*
OUTPUTS = (("forces", FORCES), ("charge_grads", CHARGE_GRAD), ("dipole_grads", DIPOLE_GRAD), ("polar_grads", POLAR_GRAD), ("virial", VIRIAL))
ALL = dict(compute_forces=True, compute_charge_gradients=True, compute_dipole_gradients=True, compute_polarizability_gradients=True,
           compute_virial=True)
NAMES = ("energies", "forces", "charge_grads", "dipole_grads", "polar_grads", "virial")


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
    print(f"{what:56s} rel err {err / scale:.2e} (bar {rel:.0e})")
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


def _lists(i, j, S, n, extra=1):
    """dict(nm, sh, nl, ptr, lsh, ent) of a full list: the matrix is `extra` columns wider than the longest row and padded with the mask value n."""
    nm, sh = _matrix(i, j, S, n, int(torch.bincount(i, minlength=n).max()) + extra, n)
    nl, ptr, lsh = _csr(nm, sh, n)
    return dict(n=n, nm=nm.contiguous(), sh=sh.contiguous(), nl=nl, ptr=ptr, lsh=lsh, ent=(i.to(DEV), j.to(DEV), S.to(DEV)))


def _kw(f, fmt, shifts=True):
    if fmt == "matrix":
        return dict(neighbor_matrix=f["nm"], neighbor_matrix_shifts=f["sh"] if shifts else None, mask_value=f["n"])
    return dict(neighbor_list=f["nl"], neighbor_ptr=f["ptr"], neighbor_shifts=f["lsh"] if shifts else None)


def _api():
    from nvalchemiops.interactions.electrostatics import InducedDipoleError, thole_dipole_correction, thole_induced_dipoles

    return thole_dipole_correction, thole_induced_dipoles, InducedDipoleError


def _undamped():
    from nvalchemiops.interactions.electrostatics import induced_dipoles

    return induced_dipoles


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def _thole_capi(P, Q, M, A, cells, bi, nsys, idx, sh, nptr, m, mask, flags, weights=None, energies=True, thole=A_T):
    """One `mi_thole_dipole` call into NaN-filled buffers: dict of every output buffer, asked for or not (virial: folded [nsys, 3, 3])."""
    from nvalchemiops import _capi as C
    import ctypes

    L, n, dt = C.lib(), P.shape[0], P.dtype
    nan = lambda *shape, dtype=F64: torch.full(shape, float("nan"), dtype=dtype, device=DEV)  # noqa: E731
    out = dict(energies=nan(n), forces=nan(n, 3, dtype=dt), charge_grads=nan(n), dipole_grads=nan(n, 3), polar_grads=nan(n),
               virial=nan(nsys, L.mi_thole_dipole_blocks(), 9))
    nbytes = int(L.mi_thole_dipole_scratch_bytes(n, C.dtype_code(dt)))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    ask = lambda name, bit: C.ptr(out[name]) if flags & bit else None  # noqa: E731
    rc = L.mi_thole_dipole(C.ptr(P), C.ptr(Q), C.ptr(M), C.ptr(cells), C.ptr(A), C.cdouble(thole), C.ptr(bi), C.ptr(weights), n, nsys, C.dtype_code(dt),
                           C.ptr(idx), C.ptr(sh), C.ptr(nptr), m, mask, flags, C.ptr(out["energies"]) if energies else None, ask("forces", FORCES),
                           ask("charge_grads", CHARGE_GRAD), ask("dipole_grads", DIPOLE_GRAD), ask("polar_grads", POLAR_GRAD), ask("virial", VIRIAL),
                           C.ptr(scratch), ctypes.c_size_t(nbytes), C.stream_of(P))
    C.check(rc, "mi_thole_dipole")
    out["virial"] = out["virial"].sum(1).reshape(nsys, 3, 3)
    return out


@functools.lru_cache(maxsize=None)
def _abi_case(kind):
    """single: the 27-atom triclinic lattice, every image within 11 (rows of about 210 entries: more than 64 and 128, so the multi-trip path
    and the lane tail both run; self-image entries present).  Atoms 3 and 11 have a = 0 and a < 0, atom 20 has a = NaN; the matrix is seven
    columns wider than the longest row, padded with the mask value, N + 7 and -1.
    batch: that system, an EMPTY system and the 64-atom lattice in one batch of three cells.
    cluster: the 27 positions without a cell, every pair within 6."""
    g = np.random.default_rng(17)
    a27 = IC.lattice("l27")
    if kind == "cluster":
        n, pos, cells, bi = 27, a27["pos"], None, None
        d = np.linalg.norm(pos[None] - pos[:, None], axis=-1)
        i, j = np.nonzero((d < 6.0) & (d > 0))
        i, j, S = torch.as_tensor(i), torch.as_tensor(j), torch.zeros((i.shape[0], 3), dtype=torch.long)
        polar = a27["polar"].copy()
    elif kind == "single":
        n, pos, cells, bi = 27, a27["pos"], a27["cell"][None], None
        i, j, S = IC.entries("l27")
        polar = a27["polar"].copy()
    else:
        a64 = IC.lattice("l64")
        n, pos, cells = 91, np.concatenate([a27["pos"], a64["pos"]]), np.stack([a27["cell"], IC.triclinic(7.0), a64["cell"]])
        bi = _t(np.array([0] * 27 + [2] * 64, dtype=np.int32))
        (i1, j1, S1), (i2, j2, S2) = IC.entries("l27"), IC.entries("l64")
        i, j, S = torch.cat([i1, i2 + 27]), torch.cat([j1, j2 + 27]), torch.cat([S1, S2])
        polar = np.concatenate([a27["polar"], a64["polar"]])
    polar[3], polar[11], polar[20] = 0.0, -0.4, float("nan")
    counts = torch.bincount(i, minlength=n)
    if kind != "cluster":
        assert int(counts[:27].min()) > 128 and bool((counts % 64 != 0).any()) and bool(((i == j) & (S != 0).any(-1)).any())
    f = _lists(i, j, S, n, extra=7)
    assert bool((f["nm"][:, -7:] == n).all())
    f["nm"][:, -1] = -1
    f["nm"][::2, -2] = n + 7
    if kind == "cluster":
        f["sh"] = f["lsh"] = None
    f.update(kind=kind, nsys=1 if cells is None else cells.shape[0], pos=pos, cells=cells, bi=bi, polar=polar, q=g.normal(size=n) + 0.05,
             mu=0.4 * g.normal(size=(n, 3)), w=_t(g.normal(size=n)))
    return f


@functools.lru_cache(maxsize=None)
def _abi_reference(kind, dtype, weighted=False):
    f = _abi_case(kind)
    P, Q, M, A = (_t(f[k], dtype) for k in ("pos", "q", "mu", "polar"))
    cells = None if f["cells"] is None else _t(f["cells"], dtype)
    return TR.evaluate(P, Q, M, A, cells, A_T, f["ent"], batch_idx=f["bi"], distance_dtype=dtype, weights=f["w"] if weighted else None)


def _abi_inputs(f, dtype, fmt):
    P, Q, M, A = (_t(f[k], dtype) for k in ("pos", "q", "mu", "polar"))
    cells = None if f["cells"] is None else _t(f["cells"], dtype)
    lay = (f["nm"], f["sh"], None, f["nm"].shape[1]) if fmt == "matrix" else (f["nl"][1].contiguous(), f["lsh"], f["ptr"], 0)
    return (P, Q, M, A, cells, f["bi"], f["nsys"]) + lay + (f["n"],)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("fmt", ["matrix", "csr"])
@pytest.mark.parametrize("kind", ["single", "batch", "cluster"])
def test_c_abi_every_flag_combination_against_the_reference(kind, fmt, dtype):
    f = _abi_case(kind)
    ref = _abi_reference(kind, dtype)
    rel = 1e-11 if dtype == torch.float64 else 1e-6
    args = _abi_inputs(f, dtype, fmt)
    bits = [b for _, b in OUTPUTS if not (b == VIRIAL and kind == "cluster")]
    worst = {}
    for r in range(len(bits) + 1):
        for combo in itertools.combinations(bits, r):
            flags = sum(combo)
            out = _thole_capi(*args, flags)
            quiet = flags not in (0, sum(bits))
            for name, bit in (("energies", 0),) + OUTPUTS:
                if bit and not flags & bit:
                    assert bool(torch.isnan(out[name]).all()), f"{name} was written without being asked for (flags {flags})"
                    continue
                got, want = _np(out[name]), ref[name]
                assert not np.isnan(got).any(), (name, flags)
                scale = np.abs(want).max()
                err = np.abs(got - want).max() / scale
                worst[name] = max(worst.get(name, 0.0), err)
                assert err <= rel + 1e-14 / scale, f"{kind} {fmt} {dtype} flags {flags} {name}: rel err {err:.3e} > {rel:.0e}"
            if not quiet:
                frozen = [3, 11, 20]
                assert all(float(out[k][frozen].abs().max()) == 0.0 for k in ("energies",) + (("forces", "charge_grads", "dipole_grads", "polar_grads")
                                                                                             if flags else ()))
    print(f"{kind} {fmt} {dtype}: worst rel err over {2 ** len(bits)} flag words (bar {rel:.0e}): " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    if kind == "batch":
        assert float(_thole_capi(*args, VIRIAL)["virial"][1].abs().max()) == 0.0, "the empty system has a zero virial"
    if dtype == torch.float32:  # what float32 distances alone cost, on the same inputs: the reference's two modes against each other
        ref64 = _abi_reference(kind, torch.float64)
        print("reference float32-distance mode against its float64 mode: "
              + ", ".join(f"{k} {np.abs(ref[k] - ref64[k]).max() / np.abs(ref64[k]).max():.2e}" for k in ref))


def test_c_abi_weights_give_the_adjoint_and_energies_may_be_null():
    f = _abi_case("batch")
    ref = _abi_reference("batch", torch.float64, weighted=True)
    args = _abi_inputs(f, torch.float64, "csr")
    flags = FORCES | CHARGE_GRAD | DIPOLE_GRAD | POLAR_GRAD
    out = _thole_capi(*args, flags, weights=f["w"], energies=False)
    assert bool(torch.isnan(out["energies"]).all())
    for name in ("forces", "charge_grads", "dipole_grads", "polar_grads"):
        _close(out[name], ref[name], f"weighted {name}", 1e-11)


# ---- early exit ------------------------------------------------------------------------------------------------------------------------
def test_entries_beyond_the_exit_contribute_exact_zeros():
    """Polarisabilities of 1e-3: E = a_T r^3 / 1e-3 >= 0.39 * 1.9^3 / 1e-3 > 2600 on every entry, so every output is exactly zero.  Then atom p and
    its nearest neighbour get a = 0.39 d^3 / 5 (E = 5 on that pair, above 50 on every other entry that has one of them, which the test
    asserts): rows p and its neighbour change and no other.  (E = 5 and not a value near the exit: the reference forms l3 - 1 by subtraction,
    so its own relative precision is 1e-16 e^E.)"""
    th, _, _ = _api()
    c = IC.lattice("l27")
    n = c["n"]
    f = _lists(*IC.entries("l27"), n)
    P, Q, M, cell = _t(c["pos"]), _t(c["q"]), _t(np.random.default_rng(5).normal(size=(n, 3))), _t(c["cell"]).reshape(1, 3, 3)
    A = torch.full((n,), 1e-3, dtype=F64, device=DEV)
    for fmt in ("matrix", "list"):
        out = th(P, Q, M, A, cell, **_kw(f, fmt), **ALL)
        assert all(bool((o == 0).all()) for o in out), fmt
    i, j, S = f["ent"]
    r = torch.linalg.norm(P[j] - P[i] + S.to(F64) @ cell[0], dim=-1)
    k = int(torch.argmin(r))
    p, nb, d = int(i[k]), int(j[k]), float(r[k])
    assert p != nb
    A2 = A.clone()
    A2[[p, nb]] = 0.39 * d**3 / 5.0
    E = A_T * r**3 / torch.sqrt(A2[i] * A2[j])
    inside = E < 50.0
    assert int(inside.sum()) == 2 and set(i[inside].tolist()) == {p, nb}
    ref = TR.evaluate(P, Q, M, A2, cell, A_T, f["ent"])
    rows = torch.ones(n, dtype=torch.bool, device=DEV)
    rows[[p, nb]] = False
    for fmt in ("matrix", "list"):
        out = th(P, Q, M, A2, cell, **_kw(f, fmt), **ALL)
        for name, o in zip(NAMES[:5], out[:5]):
            assert bool((o[rows] == 0).all()) and float(o[~rows].abs().min() if o.dim() == 1 else o[~rows].abs().amax(1).min()) > 0, (fmt, name)
        for name, o in zip(NAMES, out):
            _close(o, ref[name], f"one pair inside, {fmt} {name}", 1e-11)


# ---- the public function ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["single", "batch", "cluster"])
def test_public_function_outputs_and_adjoint(kind):
    """Explicit outputs against the reference; gradients of sum_i g_i E_i (random g) w.r.t. positions, charges, dipoles and polarizability from
    autograd against the reference's autograd; a number as polarizability; float32 dtypes."""
    th, _, _ = _api()
    f = _abi_case(kind)
    ref, refw = _abi_reference(kind, torch.float64), _abi_reference(kind, torch.float64, weighted=True)
    cells = None if f["cells"] is None else _t(f["cells"])
    common = dict(batch_idx=f["bi"]) if f["bi"] is not None else {}
    flags = dict(ALL, compute_virial=kind != "cluster")
    names = [k for k in NAMES if k != "virial" or kind != "cluster"]
    for fmt in ("matrix", "list"):
        out = th(_t(f["pos"]), _t(f["q"]), _t(f["mu"]), _t(f["polar"]), cells, **_kw(f, fmt, shifts=kind != "cluster"), **common, **flags)
        assert all(o.dtype == F64 for o in out) and len(out) == len(names)
        for name, o in zip(names, out):
            _close(o, ref[name], f"{kind} {fmt} {name}", 1e-11)
        leaves = [_t(f[k]).requires_grad_(True) for k in ("pos", "q", "mu", "polar")]
        e = th(*leaves, cells, **_kw(f, fmt, shifts=kind != "cluster"), **common)
        assert isinstance(e, torch.Tensor) and torch.equal(e.detach(), out[0])
        got = torch.autograd.grad((f["w"] * e).sum(), leaves)
        for name, g, sign in zip(("forces", "charge_grads", "dipole_grads", "polar_grads"), got, (-1.0, 1.0, 1.0, 1.0)):
            _close(sign * torch.nan_to_num(g), refw[name], f"{kind} {fmt} autograd {name}", 1e-11)
    if kind == "single":
        with pytest.raises(NotImplementedError):
            e, frc = th(*leaves, cells, **_kw(f, "matrix"), compute_forces=True)
            torch.autograd.grad(frc.sum(), leaves[0])
        uni = th(_t(f["pos"]), _t(f["q"]), _t(f["mu"]), 0.7, cells, **_kw(f, "matrix"))
        assert torch.equal(uni, th(_t(f["pos"]), _t(f["q"]), _t(f["mu"]), torch.full((27,), 0.7, dtype=F64, device=DEV), cells, **_kw(f, "matrix")))
        out32 = th(_t(f["pos"]).float(), _t(f["q"]).float(), _t(f["mu"]).float(), _t(f["polar"]).float(), cells.float(), **_kw(f, "list"), **ALL)
        assert all(o.dtype == torch.float32 for o in out32)
        # a wide width switches the correction off
        assert bool((th(_t(f["pos"]), _t(f["q"]), _t(f["mu"]), _t(f["polar"]), cells, thole=1e6, **_kw(f, "matrix")) == 0).all())


def test_bit_reproducible_between_calls_and_streams():
    th, _, _ = _api()
    f = _abi_case("batch")
    args = (_t(f["pos"]), _t(f["q"]), _t(f["mu"]), _t(f["polar"]), _t(f["cells"]))
    kw = dict(batch_idx=f["bi"], **_kw(f, "list"), **ALL)
    a, b = th(*args, **kw), th(*args, **kw)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = th(*args, **kw)
    side.synchronize()
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert float(a[0].abs().max()) > 0


def test_compile_fullgraph_equals_eager_bitwise():
    """Under torch.compile the call goes through the `alchemiops::_thole_dipole_correction` op, forward and backward: same bits as eager."""
    th, _, _ = _api()
    f = _abi_case("single")
    cells, A = _t(f["cells"]), _t(f["polar"])

    def fn(p, q, m, a):
        e, frc, pg, vir = th(p, q, m, a, cells, thole=0.5, compute_forces=True, compute_polarizability_gradients=True, compute_virial=True,
                             **_kw(f, "matrix"))
        return e * 2.0, frc, pg, vir

    args = (_t(f["pos"]), _t(f["q"]), _t(f["mu"]), A)
    torch._dynamo.reset()
    got = torch.compile(fn, mode="default", fullgraph=True)(*args)
    for a, b in zip(got, fn(*args)):
        assert torch.equal(a, b) and float(b.abs().max()) > 0

    def loss(p, q, m, a):
        return (f["w"] * th(p, q, m, a, cells, **_kw(f, "list"))).sum()

    leaves = lambda: [t.clone().requires_grad_(True) for t in args]  # noqa: E731
    x, y = leaves(), leaves()
    torch.compile(loss, mode="default", fullgraph=True)(*x).backward()
    loss(*y).backward()
    for a, b in zip(x, y):
        assert torch.equal(torch.nan_to_num(a.grad), torch.nan_to_num(b.grad)) and float(torch.nan_to_num(b.grad).abs().max()) > 0


# ---- the stored operator ---------------------------------------------------------------------------------------------------------------
def _tensors(thole, pos, polar, cells, alpha, bi, nsys, idx, sh, nptr, m, mask):
    from nvalchemiops import _capi as C

    L, n, slots = C.lib(), pos.shape[0], idx.numel()
    ten = torch.full((L.mi_induced_tensor_words(), slots), float("nan"), dtype=F64, device=DEV)
    nbr = torch.full((slots,), -12345, dtype=torch.int32, device=DEV)
    diag, pre = torch.full((n,), float("nan"), dtype=F64, device=DEV), torch.full((n,), float("nan"), dtype=F64, device=DEV)
    args = (C.ptr(pos), C.ptr(polar), C.ptr(cells), C.ptr(alpha), C.ptr(bi), n, nsys, C.dtype_code(pos.dtype), C.ptr(idx), C.ptr(sh), C.ptr(nptr), m,
            mask, slots, C.ptr(ten), C.ptr(nbr), C.ptr(diag), C.ptr(pre))
    if thole is None:
        C.check(L.mi_induced_pair_tensors(*args, C.stream_of(pos)), "mi_induced_pair_tensors")
    else:
        C.check(L.mi_thole_induced_pair_tensors(*args, C.cdouble(thole), C.stream_of(pos)), "mi_thole_induced_pair_tensors")
    return ten, nbr, diag, pre


def _apply(ten, nbr, diag, x, bi, nsys, nptr, m):
    from nvalchemiops import _capi as C

    y = torch.full((x.shape[0], 3), float("nan"), dtype=F64, device=DEV)
    rc = C.lib().mi_induced_apply(C.ptr(ten), C.ptr(nbr), C.ptr(diag), C.ptr(x), None, C.ptr(bi), x.shape[0], nsys, C.ptr(nptr), m, nbr.numel(), C.ptr(y),
                                  None, C.stream_of(x))
    C.check(rc, "mi_induced_apply")
    return y


@functools.lru_cache(maxsize=None)
def _dense_real_space_operator():
    """H = diag(1 / a) + T_real of the C ABI batch from the float64 reference: the real-space Ewald term plus the Thole correction."""
    f = _abi_case("batch")
    A = torch.nan_to_num(_t(f["polar"]), nan=0.0)
    T, _ = TR.damped_operator(_t(f["pos"]), torch.zeros(f["n"], dtype=F64, device=DEV), A, _t(f["cells"]), _t(np.array([0.45, 0.5, 0.4])), A_T,
                              f["ent"], None, batch_idx=f["bi"])
    return IR.system_matrix(T, A)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("fmt", ["matrix", "csr"])
def test_stored_operator_is_the_dipole_gradient_of_the_two_pair_kernels(fmt, dtype):
    """`mi_thole_induced_pair_tensors` + `mi_induced_apply` on a random x against x / a + dipole_grads of `mi_ewald_dipole_real` +
    `mi_thole_dipole` at zero charges and mu = x (through their public functions), on the batch of the C ABI tests (non-polarisable atoms,
    three kinds of padding, an empty system); fp64 also against the dense reference."""
    from nvalchemiops.interactions.electrostatics import ewald_dipole_real_space

    th, _, _ = _api()
    f = _abi_case("batch")
    n, nsys, bi = f["n"], f["nsys"], f["bi"]
    P, A, cells = _t(f["pos"], dtype), _t(f["polar"], dtype), _t(f["cells"], dtype)
    al = _t(np.array([0.45, 0.5, 0.4]), dtype)
    x = _t(np.random.default_rng(23).normal(size=(n, 3)))
    idx, sh, nptr, m = (f["nm"], f["sh"], None, f["nm"].shape[1]) if fmt == "matrix" else (f["nl"][1].contiguous(), f["lsh"], f["ptr"], 0)
    ten, nbr, diag, pre = _tensors(A_T, P, A, cells, al, bi, nsys, idx, sh, nptr, m, n)
    assert int(nbr.min()) >= 0 and int(nbr.max()) < n and not bool(torch.isnan(ten).any())
    ok = A.to(F64) > 0
    frozen = [3, 11, 20]
    assert bool((diag[frozen] == 1).all()) and bool((pre[frozen] == 1).all()) and torch.equal(pre[ok], A.to(F64)[ok])
    if fmt == "matrix":  # padding slots, and slots with a non-polarisable atom at either end: zero coefficients on the row's own index
        nm = f["nm"].long()
        pad = (nm == n) | (nm < 0) | (nm >= n)
        dead = pad | ~ok.unsqueeze(1) | ~ok[nm.clamp(0, n - 1)]
        rows = torch.arange(n, device=DEV).unsqueeze(1).expand_as(nm)
        assert bool(pad.any()) and bool((ten[:, dead.reshape(-1)] == 0).all()) and bool((nbr[dead.reshape(-1)] == rows[dead].to(torch.int32)).all())
    y = _apply(ten, nbr, diag, x, bi, nsys, nptr, m)
    kw = dict(batch_idx=bi, compute_dipole_gradients=True, **_kw(f, "matrix" if fmt == "matrix" else "list"))
    zero = torch.zeros(n, dtype=dtype, device=DEV)
    mask = ok.to(F64).unsqueeze(1)  # rows and columns of non-polarisable atoms are empty in the stored operator
    xm = (x * mask).to(dtype)
    dg = (ewald_dipole_real_space(P, zero, xm, cells, al, **kw)[1].to(F64) + th(P, zero, xm, A, cells, **kw)[1].to(F64)) * mask
    want = diag.unsqueeze(1) * x + dg
    rel = 1e-11 if dtype == torch.float64 else 1e-6
    _close(y, want, f"damped product {fmt} {dtype} against the pair kernels", rel)
    # the damped coefficients differ from the undamped ones only where E < 50, and the other three streams not at all
    ten0, nbr0, _, _ = _tensors(None, P, A, cells, al, bi, nsys, idx, sh, nptr, m, n)
    assert torch.equal(ten[2:], ten0[2:]) and torch.equal(nbr, nbr0) and not torch.equal(ten[:2], ten0[:2])
    if dtype == torch.float64:
        y_ref = (_dense_real_space_operator() @ x.reshape(-1)).reshape(n, 3)
        _close(y, y_ref, f"damped product {fmt} against the dense reference", rel)
    ten2, nbr2, diag2, pre2 = _tensors(A_T, P, A, cells, al, bi, nsys, idx, sh, nptr, m, n)
    assert torch.equal(ten, ten2) and torch.equal(nbr, nbr2) and torch.equal(diag, diag2) and torch.equal(pre, pre2)


# ---- solves ----------------------------------------------------------------------------------------------------------------------------
def _per_system(v, bi, nsys):
    return torch.sqrt(torch.zeros(nsys, dtype=F64, device=DEV).index_add(0, bi.long(), (v.to(F64) ** 2).sum(1)))


def _check_solution(out, H, b, polar, bi, nsys, tol, what):
    """The checks of tests/test_induced_gpu.py with the dense damped H: true residual, dipoles, iteration count against the reference PCG."""
    mu = out.dipoles.to(F64)
    n = mu.shape[0]
    bi = torch.zeros(n, dtype=torch.int32, device=DEV) if bi is None else bi
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
    print(f"{what}: true residual / (tolerance ||b||) per system {[round(float(v), 3) for v in factor]}, iterations {out.iterations.tolist()} "
          f"(reference PCG {counts})")
    assert bool((factor <= 10.0).all()), "the true residual drifted more than a factor 10 above the tolerance"
    assert all(int(got) <= ref + 2 for got, ref in zip(out.iterations.tolist(), counts)), (out.iterations.tolist(), counts)
    return mu_ref


@functools.lru_cache(maxsize=None)
def _batch_case():
    """The batch of tests/test_induced_gpu.py -- the 27-atom and the 64-atom lattice and the lone atom whose list holds only its own images,
    atoms 4, 40 and 70 not polarisable, an external field on every atom, one alpha and one k set per system -- with the dense DAMPED reference."""
    from nvalchemiops.interactions.electrostatics import generate_k_vectors_ewald_summation

    g = np.random.default_rng(81)
    parts = [TC.lattice("l27"), TC.lattice("l64"), TC.lone_atom()]
    off, ii, jj, ss = 0, [], [], []
    for c in parts:
        i, j, S = c["entries"]
        ii.append(i + off); jj.append(j + off); ss.append(S)
        off += c["n"]
    n = off
    f = _lists(torch.cat(ii), torch.cat(jj), torch.cat(ss), n, extra=5)
    polar = np.concatenate([c["polar"] for c in parts])
    polar[[4, 40, 70]] = 0.0
    f.update(nsys=3, frozen=[4, 40, 70], pos=_t(np.concatenate([c["pos"] for c in parts])), cells=_t(np.stack([c["cell"] for c in parts])),
             q=_t(np.concatenate([c["q"] for c in parts])), polar=_t(polar), field=_t(0.1 * g.normal(size=(n, 3))),
             bi=_t(np.array([0] * 27 + [1] * 64 + [2], dtype=np.int32)), alpha=_t(np.array([0.45, 0.45, 0.5])))
    f["kv"] = generate_k_vectors_ewald_summation(f["cells"], 3.2)
    T, c = TR.damped_operator(f["pos"], f["q"], f["polar"], f["cells"], f["alpha"], A_T, f["ent"], f["kv"], batch_idx=f["bi"])
    f["H"], f["b"] = IR.system_matrix(T, f["polar"]), IR.right_hand_side(c, f["polar"], f["field"])
    return f


@pytest.mark.parametrize("fmt", ["matrix", "list"])
def test_damped_solve_explicit_ewald_batch(fmt):
    from nvalchemiops.interactions.electrostatics import ewald_dipole_correction

    th, ind, _ = _api()
    f, tol = _batch_case(), 1e-10
    common = dict(batch_idx=f["bi"], **_kw(f, fmt))
    solve = dict(external_field=f["field"], reciprocal="ewald", alpha=f["alpha"], k_vectors=f["kv"], tolerance=tol, thole=A_T, **common)
    out = ind(f["pos"], f["q"], f["polar"], f["cells"], return_info=True, **solve)
    _check_solution(out, f["H"], f["b"], f["polar"], f["bi"], 3, tol, f"damped ewald batch {fmt}")
    mu = out.dipoles
    assert bool((mu[f["frozen"]] == 0).all()) and float(mu[-1].abs().max()) > 0
    # the undamped solve of the same problem gives other dipoles
    plain = ind(f["pos"], f["q"], f["polar"], f["cells"], **dict(solve, thole=None))
    assert float((plain - mu).abs().max()) > 1e-4 * float(mu.abs().max())
    # stationarity with the three public gradient calls at the returned dipoles
    e, dg = ewald_dipole_correction(f["pos"], f["q"], mu, f["cells"], f["alpha"], f["kv"], compute_dipole_gradients=True, **common)
    e_th, dg_th = th(f["pos"], f["q"], mu, f["polar"], f["cells"], thole=A_T, compute_dipole_gradients=True, **common)
    ok = (f["polar"] > 0).unsqueeze(1)
    a = torch.where(ok, f["polar"].unsqueeze(1), torch.ones_like(mu))
    grad = torch.where(ok, mu / a + dg + dg_th - f["field"], torch.zeros_like(mu))
    b_norm = _per_system(f["b"].reshape(-1, 3), f["bi"], 3)
    stat = _per_system(grad, f["bi"], 3) / (tol * b_norm)
    print(f"stationarity with the public functions / (tolerance ||b||): {[round(float(v), 3) for v in stat]}")
    assert bool((stat <= 10.0).all())
    # U at the solution
    per_atom = torch.where(ok[:, 0], (mu * mu).sum(1) / (2.0 * a[:, 0]), torch.zeros_like(e)) + e + e_th - (mu * f["field"]).sum(1)
    u = torch.zeros(3, dtype=F64, device=DEV).index_add(0, f["bi"].long(), per_atom)
    assert bool(((out.polarization_energy - u).abs() <= 100.0 * tol * u.abs() + 1e-14).all())


@functools.lru_cache(maxsize=None)
def _single_case(name, large=False):
    case = TC.two_atoms() if name == "two_atoms" else TC.lattice(name, large)
    f = _lists(*case["entries"], case["n"])
    d = TC.dense(case, A_T, DEV)
    f.update(case=case, pos=_t(case["pos"]), cell=_t(case["cell"]).reshape(1, 3, 3), q=_t(case["q"]), polar=d["polar"], kv=d["kv"], H=d["H"], b=d["b"],
             c=d["c"])
    return f


def _ewald(f, fmt="matrix"):
    return dict(reciprocal="ewald", alpha=f["case"]["alpha"], k_vectors=f["kv"], **_kw(f, fmt))


@pytest.mark.parametrize("fmt", ["matrix", "list"])
def test_damped_solve_single_system_and_thole_none_is_the_undamped_path(fmt):
    _, ind, _ = _api()
    f, tol = _single_case("l27"), 1e-10
    args = (f["pos"], f["q"], f["polar"], f["cell"])
    out = ind(*args, tolerance=tol, thole=A_T, return_info=True, **_ewald(f, fmt))
    _check_solution(out, f["H"], f["b"], f["polar"], None, 1, tol, f"damped ewald single {fmt}")
    a, b = _undamped()(*args, tolerance=tol, **_ewald(f, fmt)), ind(*args, tolerance=tol, thole=None, **_ewald(f, fmt))
    assert torch.equal(a, b) and not torch.equal(a, out.dipoles)


# The deviation of PME itself is that of the undamped solve (the damping is a real-space term): the bar of `test_solve_pme_against_ewald` in
# tests/test_induced_gpu.py, 3 x 4.001e-7 of max |mu| for mesh 64^3 and order 5 at alpha 0.45.
PME_MESH, PME_ORDER, PME_REFERENCE = (64, 64, 64), 5, 4.001e-7


def test_damped_solve_pme_single_and_batched():
    _, ind, _ = _api()
    f = _single_case("l64")
    args = (f["pos"], f["q"], f["polar"], f["cell"])
    mu_ew = ind(*args, tolerance=1e-11, thole=A_T, **_ewald(f))
    pme = dict(tolerance=1e-11, thole=A_T, reciprocal="pme", mesh_dimensions=PME_MESH, spline_order=PME_ORDER)
    mu_pme = ind(*args, alpha=f["case"]["alpha"], **pme, **_kw(f, "matrix"))
    dev = float((mu_pme - mu_ew).abs().max()) / float(mu_ew.abs().max())
    print(f"damped pme vs ewald dipoles, single: max deviation {dev:.3e} of max |mu| (bar {3.0 * PME_REFERENCE:.3e})")
    assert dev <= 3.0 * PME_REFERENCE
    b = _batch_case()
    args = (b["pos"], b["q"], b["polar"], b["cells"])
    common = dict(external_field=b["field"], batch_idx=b["bi"], alpha=b["alpha"], **_kw(b, "list"))
    mu_ew = ind(*args, tolerance=1e-11, thole=A_T, reciprocal="ewald", k_vectors=b["kv"], **common)
    out = ind(*args, return_info=True, **pme, **common)
    dev = float((out.dipoles - mu_ew).abs().max()) / float(mu_ew.abs().max())
    print(f"damped pme vs ewald dipoles, batch: max deviation {dev:.3e} of max |mu| (bar {3.0 * PME_REFERENCE:.3e}), iterations {out.iterations.tolist()}")
    assert dev <= 3.0 * PME_REFERENCE and bool((out.residual <= 1e-11).all())


def test_damping_cures_the_breakdown():
    """The two-atom case of `test_breakdown_is_reported` (the most negative eigenvector of the undamped H as the external field) and the 27-atom
    lattice with polarisabilities x 4: "not positive definite" without `thole`, the dense damped solution with it."""
    _, ind, Err = _api()
    for name, large in (("two_atoms", False), ("l27", True)):
        f, tol = _single_case(name, large), 1e-10
        plain = TC.dense(f["case"], None, DEV)
        ev, vec = torch.linalg.eigh(plain["H"])
        assert float(ev[0]) < 0, "the undamped dense H must have a negative eigenvalue"
        field = vec[:, 0].reshape(-1, 3).contiguous()
        args = (f["pos"], f["q"], f["polar"], f["cell"])
        with pytest.raises(Err, match="not positive definite for system 0"):
            _undamped()(*args, external_field=field, **_ewald(f))
        out = ind(*args, external_field=field, tolerance=tol, thole=A_T, return_info=True, **_ewald(f))
        b = IR.right_hand_side(f["c"], f["polar"], field)
        _check_solution(out, f["H"], b, f["polar"], None, 1, tol, f"damped {name}{' x 4' if large else ''}")


# Relative to the largest |component| of each gradient, the bar of `test_gradients_against_the_reference_autograd` in tests/test_induced_gpu.py:
# both solves run to tolerance 1e-12, an error of that size in mu or z is amplified by at most the condition number of D^1/2 H D^1/2 (taken
# from the reference inside the test), and a factor 100 covers the rounding of the public energy functions' adjoints: 100 * 1e-12 * cond.
def test_damped_gradients_against_the_reference_autograd():
    _, ind, _ = _api()
    c = IC.lattice("l27")
    n, tol = c["n"], 1e-12
    f = _lists(*IC.entries("l27", 7.0, 1), n, extra=2)
    cell, kv = _t(c["cell"]).reshape(1, 3, 3), IC.k_vectors(c["cell"], IC.EWALD["k_cutoff"]).to(DEV)
    g = np.random.default_rng(91)
    field0, w = 0.1 * g.normal(size=(n, 3)), _t(g.normal(size=(n, 3)))
    names = ["pos", "q", "polar", "field"]
    leaves = lambda: dict(pos=_t(c["pos"]).requires_grad_(True), q=_t(c["q"]).requires_grad_(True),  # noqa: E731
                          polar=_t(2.0 * c["polar"]).requires_grad_(True), field=_t(field0).requires_grad_(True))
    r = leaves()
    T, lin = TR.damped_operator(r["pos"], r["q"], r["polar"], cell, IC.EWALD["alpha"], A_T, f["ent"], kv, differentiable=True)
    H, b = IR.system_matrix(T, r["polar"]), IR.right_hand_side(lin, r["polar"], r["field"])
    mu_ref = IR.solve(H, b)
    ref = dict(zip(names, torch.autograd.grad((w * mu_ref).sum(), [r[k] for k in names])))
    ev = IR.scaled_spectrum(H.detach(), r["polar"].detach())
    assert float(ev.min()) > 0
    bar = 100.0 * tol * float(ev.max() / ev.min())
    d = leaves()
    mu = ind(d["pos"], d["q"], d["polar"], cell, external_field=d["field"], reciprocal="ewald", alpha=IC.EWALD["alpha"], k_vectors=kv, tolerance=tol,
             thole=A_T, **_kw(f, "matrix"))
    assert float((mu.detach() - mu_ref.detach()).abs().max()) <= 1e-9 * float(mu_ref.detach().abs().max())
    got = dict(zip(names, torch.autograd.grad((w * mu).sum(), [d[k] for k in names], retain_graph=True)))
    errs = {k: float((got[k] - ref[k]).abs().max()) / float(ref[k].abs().max()) for k in names}
    print(f"damped gradients (bar {bar:.2e}): " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k in names:
        assert got[k].shape == d[k].shape and got[k].dtype == F64
        assert errs[k] <= bar, (k, errs[k])
    # the polarisability gradient alone takes the path without the Ewald energies and gives the same numbers
    (alone,) = torch.autograd.grad((w * mu).sum(), [d["polar"]])
    assert float((alone - got["polar"]).abs().max()) <= bar * float(ref["polar"].abs().max())
