"""Seeded sweeps and boundary ladders of the two point-dipole operators, `ewald_dipole_correction` (csrc/dipole.hip) and
`pme_dipole_correction` (last section of csrc/pme.hip), against the float64 restatements tests/dipole_reference.py -- evaluated on the
entries actually stored and on the same k set -- and tests/pme_dipole_reference.py -- on the same mesh and order.  The inputs are those of
tests/sweep_cases.py (dipole section; tests/test_sweep_cases_cpu.py asserts their conditions without a device).  No tolerance is new; the
comparison functions are imported from the two operators' parity modules:

    explicit sums, float64     1e-11 of max |ref| + 1e-14 per output                       tests/test_dipole_gpu.py::_close
    explicit sums, float32     1e-6 of max |ref| against the restatement's float32-distance mode
    mesh term, float64         1e-10 of max |ref|                                          tests/test_pme_dipole_gpu.py::_close
    mesh term, float32         4 x the restatement's own float32-against-float64 deviation on the same case (at most 4e-5: CPU suite)
    two device results         1e-12 of max (float64), the bar of tests/test_pme_dipole_gpu.py between two runs of the mesh term

What the sweeps and ladders reach that the parity modules do not: rows of exactly 63, 64, 65 and 128 entries and a list without shifts
(`dp_pair_kernel`); K on both sides of 64 and 256 (`dp_recip_gather_kernel`, `dp_recip_virial_kernel`); systems of 255, 256 and 257 atoms
and a system without atoms inside a batch (`dp_sf_kernel`); full, short and overfull blocks of `pme_dipole_spread_kernel` (16, 10, 7 atoms)
and `pme_dipole_gather_kernel` (32) at every order; odd and prime mesh dimensions, a dimension equal to the order, an odd nz
(`pme_dipole_virial_kernel`'s Hermitian weight) and a half spectrum of more than 256 x 256 points (its second grid-stride trip); both paths of
the mesh solve for the two meshes of the forward call and the four of the adjoint; the adjoint in batches, in float32 and at orders 4 and 6;
interleaved batches; exact zeros for zero dipoles.

MEASURED on one MI355X (worst error / bar; every test prints its figures under `pytest -s`): explicit sums 0.002 in
float64 (1.7e-14 of max |ref|) and 0.41 in float32 over the twelve seeds, 0.001 on the row, K and atom ladders, the list without shifts
bit-equal to the list with zero shifts; mesh term 0.001 in float64 (9.5e-15) and 0.31 in float32 over the twelve seeds, interleaved against
sorted 1.3e-15, spread / gather ladder 0.0002 and 0.64, second virial trip 0.001, both solve paths 0.00003.  60 tests in 22 s.
"""
import functools

import numpy as np
import pytest
import torch

from tests import dipole_reference as DR
from tests import pme_dipole_reference as PR
from tests import sweep_cases as W
from tests import test_dipole_gpu as TD
from tests import test_pme_dipole_gpu as TP
from tests import test_sweep_charges_gpu as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
NAMES = TD.NAMES
ALL = TD.ALL
GRADS = ("forces", "charge_grads", "dipole_grads")
TWO_RUNS = 1e-12  # two device results of the mesh term, float64 (tests/test_pme_dipole_gpu.py)


def _dtype(c, dt=None):
    return dt if dt is not None else (F64 if c["dtype"] == "float64" else F32)


def _device(c, dt):
    """(positions, charges, dipoles, cells [B, 3, 3], alpha [B], batch_idx | None, weights) of a case on the device in dtype dt."""
    t = lambda a: TD._t(a, dt)  # noqa: E731
    bi = TD._t(c["batch_idx"]) if len(c["sizes"]) > 1 else None
    return t(c["pos"]), t(c["q"]), t(c["mu"]), t(c["cells"]), t(c["alpha"]), bi, TD._t(c["weights"], F64)


def _k_vectors(c, cells):
    return TD._k_vectors(cells if cells.shape[0] > 1 else cells[0], c["k_cutoff"])


def _lists(f, fmt, shifts=True):
    kw = TD._fmt_kw(dict(f, n=f["mask"]), fmt)
    if not shifts:
        kw = {k: v for k, v in kw.items() if k not in ("neighbor_matrix_shifts", "neighbor_shifts")}
    return kw


def _select(ref, flags):
    return ["energies"] + [name for name, flag in zip(NAMES[1:], W.DIPOLE_FLAGS) if flags.get(flag)]


def _exactly_zero(o, what):
    assert float(o.abs().max()) == 0.0 and not bool(torch.isnan(o).any()), f"{what}: must be exactly 0.0"


def _explicit(out, ref, names, dt, tag, zero_dipoles=False):
    """Outputs of an explicit-sum call against the restatement at the bar of tests/test_dipole_gpu.py; returns the worst error / bar."""
    out = (out,) if isinstance(out, torch.Tensor) else out
    assert len(out) == len(names) and all(o.dtype == dt for o in out), tag
    rel, worst = (1e-11 if dt == F64 else 1e-6), 0.0
    for name, o in zip(names, out):
        if zero_dipoles and name != "dipole_grads":
            _exactly_zero(o, f"{tag} {name}")
            continue
        worst = max(worst, TD._close(o, ref[name], f"{tag} {name}", rel) / rel)
    return worst


def _explicit_backward(call, leaves, w, ref, dt, tag):
    """dL/d(positions, charges, dipoles) of L = sum_i w_i E_i through autograd against the restatement's."""
    leaves = [x.clone().requires_grad_(True) for x in leaves]
    e = call(*leaves)
    gp, gq, gm = torch.autograd.grad((e * w.to(dt)).sum(), leaves)
    return _explicit((-gp, gq, gm), ref, GRADS, dt, tag)


# ---- mesh term ----------------------------------------------------------------------------------------------------------------------------------

def _mesh(out, ref, names, dt, tag, own=None, take=None):
    """Outputs of a mesh call against the restatement: 1e-10 of max |ref| in float64, 4 x `own` (the restatement's float32 deviation) in
    float32; an output whose reference is exactly zero must be exactly zero.  `take`: the atom order of the call (interleaved batches)."""
    out = (out,) if isinstance(out, torch.Tensor) else out
    assert len(out) == len(names) and all(o.dtype == dt for o in out), tag
    worst = 0.0
    for name, o in zip(names, out):
        r = ref[name] if take is None or name == "virial" else ref[name][take]
        if not r.any():
            _exactly_zero(o, f"{tag} {name}")
            continue
        rel = 1e-10 if dt == F64 else 4.0 * own[name]
        err = float(np.abs(TP._np(o).reshape(r.shape) - r).max() / np.abs(r).max())
        worst = max(worst, err / rel)
        TP._close(o.reshape(r.shape), r, f"{tag} {name}", rel)
    return worst


def _mesh_call(c, dt, flags=ALL):
    _, recip = TP._api()
    P, Q, M, C, A, BI, _ = _device(c, dt)
    return recip(P, Q, M, C, A, mesh_dimensions=c["mesh"], spline_order=c["order"], batch_idx=BI, **flags)


def _mesh_backward(c, dt):
    _, recip = TP._api()
    P, Q, M, C, A, BI, w = _device(c, dt)
    leaves = [x.clone().requires_grad_(True) for x in (P, Q, M)]
    e = recip(*leaves, C, A, mesh_dimensions=c["mesh"], spline_order=c["order"], batch_idx=BI)
    gp, gq, gm = torch.autograd.grad((e * w.to(dt)).sum(), leaves)
    return -gp, gq, gm


def _mesh_case(kind, key, dt, tag, backward, take=None, c=None):
    """Forward (all outputs) and, with `backward`, the weighted backward of one mesh case in dtype dt; returns the worst error / bar."""
    c = W.dipole_case(kind, key) if c is None else c
    own = W.pme_float32_deviation(kind, key) if dt == F32 else None
    worst = _mesh(_mesh_call(c, dt), W.pme_dipole_reference(kind, key), NAMES, dt, tag, own, take)
    if backward:
        own_w = W.pme_float32_deviation(kind, key, weighted=True) if dt == F32 else None
        worst = max(worst, _mesh(_mesh_backward(c, dt), W.pme_dipole_reference(kind, key, "float64", True), GRADS, dt, f"{tag} weighted backward", own_w, take))
    return worst


# ---- sweeps -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", W.SEEDS)
def test_ewald_dipole_sweep(seed):
    both, real, _ = TD._api()
    c = W.dipole_case("sweep", ("ewald_dipole", seed))
    halves = "total"
    if c["perm"] is not None:  # `ewald_dipole_reciprocal_space` documents contiguous systems: the real-space half alone
        c, halves = W.interleaved(c), "real space"
    dt = _dtype(c)
    P, Q, M, C, A, BI, w = _device(c, dt)
    f = SC._stored(c, mask_emptied=True)
    entries = DR.entries_from_matrix(f["nm"], f["sh"], f["mask"])
    assert entries[0].shape[0] == len(W.stored_entries(c)[0]) and not bool((entries[0] == c["emptied_row"]).any())
    kv = _k_vectors(c, C) if halves == "total" else None
    ref = DR.evaluate(P, Q, M, C, A, entries, kv, batch_idx=BI, distance_dtype=dt)
    names = _select(ref, c["flags"])
    tag = f"ewald_dipole {seed} {c['dtype']} {halves}"

    def call(p, q, m, fmt, **flags):
        if halves == "total":
            return both(p, q, m, C, A, kv, batch_idx=BI, **_lists(f, fmt), **flags)
        return real(p, q, m, C, A, batch_idx=BI, **_lists(f, fmt), **flags)

    worst = 0.0
    for fmt in ("matrix", "list"):
        out = call(P, Q, M, fmt, **c["flags"])
        worst = max(worst, _explicit(out, ref, names, dt, f"{tag} {fmt}", c["zero_dipoles"]))
        if c["empty_system"] is not None and c["flags"]["compute_virial"]:
            _exactly_zero(out[-1][c["empty_system"]], f"{tag} {fmt}: virial row of the system without atoms")
    if c["autograd"]:
        fmt = ("matrix", "list")[seed % 2]
        ref_w = DR.evaluate(P, Q, M, C, A, entries, kv, batch_idx=BI, distance_dtype=dt, weights=w)
        leaves = [x.clone().requires_grad_(True) for x in (P, Q, M)]
        gp, gq, gm = torch.autograd.grad((call(*leaves, fmt) * w.to(dt)).sum(), leaves)
        for name, g in zip(GRADS, (-gp, gq, gm)):
            if c["zero_dipoles"] and name != "dipole_grads":
                _exactly_zero(g, f"{tag} {fmt} weighted backward {name}")
            else:
                worst = max(worst, TD._close(g, ref_w[name], f"{tag} {fmt} weighted backward {name}", 1e-11 if dt == F64 else 1e-6) / (1e-11 if dt == F64 else 1e-6))
    print(f"[sweep] {tag}: sizes {c['sizes']}, {entries[0].shape[0]} entries, K {0 if kv is None else kv.shape[-2]}, outputs {names}, "
          f"backward {c['autograd']}, worst error / bar {worst:.3f}")


@pytest.mark.parametrize("seed", W.SEEDS)
def test_pme_dipole_sweep(seed):
    both, recip = TP._api()
    key = ("pme_dipole", seed)
    base = W.dipole_case("sweep", key)
    c, take = (W.interleaved(base), base["perm"]) if base["perm"] is not None else (base, None)
    dt = _dtype(c)
    tag = f"pme_dipole {seed} {c['dtype']} order {c['order']} mesh {c['mesh']}"
    worst = _mesh_case("sweep", key, dt, tag, backward=True, take=take, c=c)
    out = _mesh_call(c, dt)
    if c["empty_system"] is not None:
        _exactly_zero(out[4][c["empty_system"]], f"{tag}: virial row of the system without atoms")
    if take is not None:  # the same call on the sorted batch: two device results
        for name, a, b in zip(NAMES + GRADS, out + _mesh_backward(c, dt), _mesh_call(base, dt) + _mesh_backward(base, dt)):
            TP._close(a, b if name == "virial" else b[TD._t(take)], f"{tag} interleaved vs sorted {name}", TWO_RUNS)
    if seed % 4 == 0:  # `pme_dipole_correction` with the stored list: minus the mesh half it is the real-space half, the explicit sum's bar
        P, Q, M, C, A, BI, _ = _device(c, dt)
        f = SC._stored(c, mask_emptied=True)
        ref = DR.evaluate(P, Q, M, C, A, DR.entries_from_matrix(f["nm"], f["sh"], f["mask"]), None, batch_idx=BI, distance_dtype=dt)
        for fmt in ("matrix", "list"):
            total = both(P, Q, M, C, A, mesh_dimensions=c["mesh"], spline_order=c["order"], batch_idx=BI, **_lists(f, fmt), **ALL)
            worst = max(worst, _explicit(tuple(a - b for a, b in zip(total, out)), ref, NAMES, dt, f"{tag} correction {fmt} minus the mesh half"))
    print(f"[sweep] {tag}: sizes {c['sizes']}, interleaved {take is not None}, worst error / bar {worst:.3f}")


# ---- ladders ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", W.LANE_RUNGS)
def test_row_ladder(name):
    """Rows of 63, 64, 65 and 128 entries against the 64-lane trips of `dp_pair_kernel`, in both formats; and the same list without its
    (all-zero) shifts, the kernel's `ush == nullptr` branch, whose bits must be those of the call with zero shifts."""
    _, real, _ = TD._api()
    c = W.dipole_case("row", name)
    P, Q, M, C, A, _, w = _device(c, F64)
    f = SC._stored(c)
    n = f["n"]
    assert f["nm"].shape == (n, n - 1) and int(f["nm"].max()) == n - 1 and int(f["nm"].min()) == 0 and not bool(f["sh"].any()), "every row full, every shift zero"
    entries = DR.entries_from_matrix(f["nm"], f["sh"], f["mask"])
    ref = DR.evaluate(P, Q, M, C, A, entries, None)
    ref_w = DR.evaluate(P, Q, M, C, A, entries, None, weights=w)
    no_virial = {k: v for k, v in ALL.items() if k != "compute_virial"}
    worst = 0.0
    for fmt in ("matrix", "list"):
        worst = max(worst, _explicit(real(P, Q, M, C, A, **_lists(f, fmt), **ALL), ref, NAMES, F64, f"{name} {fmt}"))
        worst = max(worst, _explicit_backward(lambda p, q, m: real(p, q, m, C, A, **_lists(f, fmt)), (P, Q, M), w, ref_w, F64, f"{name} {fmt} weighted backward"))
        with_zero = real(P, Q, M, C, A, **_lists(f, fmt), **no_virial)
        without = real(P, Q, M, C, A, **_lists(f, fmt, shifts=False), **no_virial)
        worst = max(worst, _explicit(without, ref, NAMES[:4], F64, f"{name} {fmt} without shifts"))
        for k, a, b in zip(NAMES, without, with_zero):
            assert torch.equal(a, b), f"{name} {fmt} {k}: a list without shifts is not bit-equal to the list with zero shifts (max difference {float((a - b).abs().max()):.3e})"
    print(f"[ladder] rows of {n - 1} entries: worst error / bar {worst:.3f}; without shifts: bit-equal")


@functools.lru_cache(maxsize=None)
def _k_fixture():
    c = W.dipole_case("k", None)
    P, Q, M, C, A, _, w = _device(c, F64)
    kv = _k_vectors(c, C)
    assert kv.dim() == 2 and kv.shape[0] >= max(W.K_RUNGS)
    return c, P, Q, M, C, A, w, kv


@pytest.mark.parametrize("K", W.K_RUNGS)
def test_k_ladder(K):
    """K on both sides of the 64 k of one trip of `dp_recip_gather_kernel` and the 256 of `dp_recip_virial_kernel`."""
    _, _, recip = TD._api()
    c, P, Q, M, C, A, w, kv = _k_fixture()
    k = kv[:K].contiguous()
    worst = _explicit(recip(P, Q, M, C, k, A, **ALL), DR.evaluate(P, Q, M, C, A, None, k), NAMES, F64, f"K = {K}")
    if K in (64, 257):
        worst = max(worst, _explicit_backward(lambda p, q, m: recip(p, q, m, C, k, A), (P, Q, M), w, DR.evaluate(P, Q, M, C, A, None, k, weights=w), F64,
                                              f"K = {K} weighted backward"))
    print(f"[ladder] K = {K}: worst error / bar {worst:.3f}")


def test_atom_ladder():
    """Systems of 255, 256, 257 and 1 atoms in one batch against the 256 atoms of one trip of `dp_sf_kernel`.  Judged system by system at the
    bar of the whole batch (1e-11 of the largest |reference value| of the output), so that a failure names its system."""
    _, _, recip = TD._api()
    c = W.dipole_case("atoms", None)
    P, Q, M, C, A, BI, w = _device(c, F64)
    kv = _k_vectors(c, C)
    assert kv.shape[0] == 4 and 60 <= kv.shape[1] <= 70
    ref = DR.evaluate(P, Q, M, C, A, None, kv, batch_idx=BI)
    ref_w = DR.evaluate(P, Q, M, C, A, None, kv, batch_idx=BI, weights=w)
    out = recip(P, Q, M, C, kv, A, batch_idx=BI, **ALL)
    leaves = [x.clone().requires_grad_(True) for x in (P, Q, M)]
    gp, gq, gm = torch.autograd.grad((recip(*leaves, C, kv, A, batch_idx=BI) * w).sum(), leaves)
    bounds = np.concatenate([[0], np.cumsum(c["sizes"])])
    failed = []
    for label, names, outs, r in (("", NAMES, out, ref), ("weighted backward ", GRADS, (-gp, gq, gm), ref_w)):
        for name, o in zip(names, outs):
            got, want = TD._np(o), r[name]
            bar = 1e-11 * np.abs(want).max() + 1e-14
            for s, size in enumerate(c["sizes"]):
                sl = slice(s, s + 1) if name == "virial" else slice(bounds[s], bounds[s + 1])
                err = float(np.abs(got[sl] - want[sl]).max())
                print(f"[ladder] system of {size:3d} atoms {label}{name:13s} error / bar {err / bar:.3f}")
                if err > bar:
                    failed.append(f"system of {size} atoms: {label}{name} error / bar {err / bar:.3g}")
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("order,n", [(order, n) for order in W.PME_ORDERS for n in W.spread_rungs(order)])
def test_spread_gather_ladder(order, n):
    """Blocks of `pme_dipole_spread_kernel` (256 // order^2 atoms) and `pme_dipole_gather_kernel` (32 atoms) one atom short of full, full and
    one atom into the next block, on the prime-and-odd mesh (9, 10, 11), in float64 and float32."""
    backward = n in (W.spread_atoms_per_block(order) + 1, W.PG_ATOMS + 1)
    worst = {str(dt): _mesh_case("spread", (order, n), dt, f"order {order} N {n} {dt}", backward) for dt in (F64, F32)}
    print(f"[ladder] order {order} N = {n}{' with backward' if backward else ''}: worst error / bar {worst}")


def test_virial_second_trip():
    """Mesh (40, 36, 96): 70 560 half-spectrum points, the second trip of `pme_dipole_virial_kernel`'s grid-stride loop."""
    worst = _mesh_case("big", None, F64, f"mesh {W.BIG_MESH}", backward=False)
    print(f"[ladder] mesh {W.BIG_MESH}: worst error / bar {worst:.3f}")


# ---- the two paths of the mesh solve ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _solve_references(order):
    pos, q, mu = TP._system()
    t = lambda a: torch.tensor(a, dtype=F64)  # noqa: E731
    w = np.random.default_rng(31).uniform(0.2, 1.8, len(pos))
    return w, TP._reference(order, TP.MESH), PR.evaluate(t(pos), t(q), t(mu), t(TP.CELL), TP.ALPHA, TP.MESH, order, weights=t(w), virial=False)


@pytest.mark.parametrize("order", W.PME_ORDERS)
def test_both_solve_paths(order, monkeypatch):
    """Mesh (12, 10, 16) is one the fused in-LDS solve supports for the two meshes of the forward call and the four of the adjoint.  Forward
    and weighted backward against the restatement as the library chooses, then with `_MESH_SOLVE = False`: FFT plans (or their dense-DFT
    replacement) and `mi_pme_convolve`."""
    from nvalchemiops import _capi as C
    from nvalchemiops.interactions.electrostatics import pme

    _, recip = TP._api()
    code = C.dtype_code(F64)
    assert C.lib().mi_pme_solve_supported(2, *TP.MESH, code) and C.lib().mi_pme_solve_supported(4, *TP.MESH, code)
    assert pme._MESH_SOLVE is not False
    w, ref, ref_w = _solve_references(order)
    P, Q, M, Cl = TP._inputs()
    for path in ("fused", "plans"):
        if path == "plans":
            monkeypatch.setattr(pme, "_MESH_SOLVE", False)
        worst = _mesh(recip(P, Q, M, Cl, TP.ALPHA, mesh_dimensions=TP.MESH, spline_order=order, **ALL), ref, NAMES, F64, f"order {order} {path}")
        leaves = [x.clone().requires_grad_(True) for x in (P, Q, M)]
        e = recip(*leaves, Cl, TP.ALPHA, mesh_dimensions=TP.MESH, spline_order=order)
        gp, gq, gm = torch.autograd.grad((e * TP._t(w)).sum(), leaves)
        worst = max(worst, _mesh((-gp, gq, gm), ref_w, GRADS, F64, f"order {order} {path} weighted backward"))
        print(f"[solve] order {order} mesh {TP.MESH} {path}: worst error / bar {worst:.3f}")
