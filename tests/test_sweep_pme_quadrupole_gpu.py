"""Seeded sweep, boundary ladder, spline-knot cases and the solve paths of `pme_quadrupole_correction` / `pme_quadrupole_reciprocal_space`
(last section of csrc/pme.hip, driver interactions/electrostatics/pme_quadrupole.py) against the float64 restatement
tests/pme_quadrupole_reference.py, evaluated on the CPU on the same mesh and order, in float64 and in its float32 mode.  The inputs are those
of tests/sweep_cases.py (section "point quadrupoles on the mesh"; tests/test_sweep_cases_cpu.py asserts their conditions without a device).
No tolerance is new:

    float64 against the yardstick   1e-10 of max |ref| per output                                tests/test_pme_quadrupole_gpu.py::test_parity_fp64
    float32 against the yardstick   4 x the yardstick's own float32-mode deviation on the same case (at most 1e-4: the CPU suite caps the
                                    deviation at 2.5e-5)                                         tests/test_pme_quadrupole_gpu.py::test_parity_fp32
    two device results, float64     1e-12 of max                                                 tests/test_pme_quadrupole_gpu.py (batch, no dipoles)
    exact zeros                     torch.equal / == 0.0

What this module reaches that the parity module does not (the numbers are the gaps of the issue that asked for it):
  1 the weighted adjoint (four meshes, `accumulate` launch) in batches of two and three systems with per-system alpha, in float32, at order 6:
    test_sweep (every seed), test_batch_systems_equal_single_calls_forward_and_backward
  2 which solve path the forward call (b = 2 B) and the adjoint (b = 4 B) took: test_solve_paths_forward_and_adjoint
  3 blocks of `pme_quadrupole_spread_kernel` (10 / 7 atoms) and `pme_quadrupole_gather_kernel` (32) one short of full, full, one over, two
    blocks, and N = 1: test_spread_gather_ladder
  4 atoms exactly on spline knots, at fractional coordinate 0, 1 and -1 / n: test_atoms_on_spline_knots
  5 unsorted `batch_idx`, a system without atoms inside a batch, a float32 batch, `dipoles=None` in a batch: test_sweep
  6 all six outputs of `pme_quadrupole_correction` against separate calls of its two halves (test_sweep, every fourth seed) and against the
    explicit Ewald routine (test_mesh_term_converges_to_the_explicit_sum_in_every_output)
  7 an axis equal to the order at order 6 and odd nz (test_sweep), the second grid-stride trip of `mi_pme_quadrupole_virial`
    (test_virial_second_trip), the host's strain terms with an empty system (test_sweep, empty-system seeds)

CONVERGENCE BARS (gap 6).  Per output, 10 x the relative difference between the mesh restatement at order 6 on 32^3 and the explicit
restatement tests/quadrupole_reference.py on the converged k set, both on the 37-atom system of the parity module
(`sweep_cases.pmeq_convergence`, printed by tests/test_sweep_cases_cpu.py::test_pme_quadrupole_convergence_bars).  Measured differences:
energies 2.24e-6, forces 4.59e-5, charge_grads 1.93e-6, dipole_grads 2.36e-6, quadrupole_grads 3.53e-6, virial 9.64e-6 (of the largest
explicit value of the output); the device's mesh and explicit totals differ by 1.8e-8 (energies) to 4.0e-8 of the totals' largest values.

MEASURED on one MI355X (worst error / bar; every test prints its figures under `pytest -s`):
sweep 1.1e-4 in float64 and 0.46 in float32 over the twelve seeds, interleaved against sorted and the correction against its halves within
1e-12 / bit-equal; batch against single calls 1.4e-4 and 0.46; ladder from 6 atoms on 3.9e-4 in float64 and 0.18 - 0.46 in float32, rung 1
0.002 (order 5) and 0.16 (order 6) in float64 and 0.98 (order 5) and 0.53 (order 6) in float32 (four outputs; forces and dipole_grads finite only); knots 3.2e-4 and 0.45; second virial trip 0.034; both solve paths 5.1e-4.

FOUND BY THE LADDER.  test_spread_gather_ladder[6-6-float32] and [6-7-float32] failed at first: forward forces off by 1.70e-5 and 8.10e-6 of
max |force| against bars of 1.42e-5 and 7.18e-6 (1.19 and 1.13 bars), float64 at 4e-14 on the same rungs.  `pme_quadrupole_gather_kernel`
formed its stencil from the float32 mesh coordinate while a float32 call spreads in float64: the gather's weights were those of an atom
displaced by up to 1e-6 of a mesh spacing, on which its own density then pulled -- a force of constant size, visible where 6 or 7 atoms far
apart leave small net forces.  The kernel now forms stencil and tables in double and rounds them once: 2.44e-6 and 2.15e-6 on those rungs
(0.17 and 0.30 bars); over all float32 comparisons of this module the kernel's force error went from 0.2 - 4.8 to 0.18 - 1.5 x the
restatement's own float32 deviation.
"""
import functools

import numpy as np
import pytest
import torch

from tests import poison
from tests import sweep_cases as W
from tests import test_pme_quadrupole_gpu as TPQ
from tests import test_sweep_charges_gpu as SC
from tests import test_sweep_dipoles_gpu as SD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
NAMES = TPQ.NAMES
ALL = TPQ.ALL
GRADS = W.PMEQ_GRADS
FP64_BAR = 1e-10   # against the yardstick (tests/test_pme_quadrupole_gpu.py)
TWO_RUNS = 1e-12   # two device results in float64 (tests/test_pme_quadrupole_gpu.py)
DTYPES = pytest.mark.parametrize("dt", [F64, F32], ids=["float64", "float32"])
_t = TPQ._t
_np = TPQ._np


@pytest.fixture(autouse=True)
def _device_guard(request):
    with poison.device_guard(request.node.nodeid):
        yield


def _device(c, dt):
    """(positions, charges, dipoles | None, quadrupoles, cells [B, 3, 3], alpha [B], batch_idx | None, weights) of a case in dtype dt."""
    P, Q, M, C, A, BI, w = SD._device(c, dt)
    return P, Q, (None if c["no_dipoles"] else M), _t(c["qd"], dt), C, A, BI, w


def _call(c, dt, flags=ALL):
    _, recip = TPQ._api()
    P, Q, M, T, C, A, BI, _ = _device(c, dt)
    return recip(P, Q, M, T, C, A, mesh_dimensions=c["mesh"], spline_order=c["order"], batch_idx=BI, **flags)


def _backward(c, dt):
    """(-dL/dr, dL/dq, dL/dmu | None, dL/dQ) of L = sum_i w_i E_i through autograd (`dipoles=None`: no dipole leaf)."""
    _, recip = TPQ._api()
    P, Q, M, T, C, A, BI, w = _device(c, dt)
    P, Q, T = (x.clone().requires_grad_(True) for x in (P, Q, T))
    M = None if M is None else M.clone().requires_grad_(True)
    e = recip(P, Q, M, T, C, A, mesh_dimensions=c["mesh"], spline_order=c["order"], batch_idx=BI)
    leaves = [x for x in (P, Q, M, T) if x is not None]
    g = dict(zip([n for n, x in zip(GRADS, (P, Q, M, T)) if x is not None], torch.autograd.grad((e * w.to(dt)).sum(), leaves)))
    g["forces"] = -g["forces"]
    return g


def _judge(out, ref, names, dt, tag, own=None, take=None, scale=None, finite_only=()):
    """Outputs (a tuple in the order `names`, or a dict) against the yardstick: `FP64_BAR` of max |ref| in float64, 4 x `own[name]` (the
    yardstick's float32-mode deviation) in float32; an output whose reference is exactly zero must be exactly zero.  `take`: the atom order of
    the call (interleaved batches).  `scale`: max |ref| per output where `ref` is a slice of a larger case.  `finite_only`: outputs that are
    only required to be finite (their figures are printed all the same).  Returns the worst error / bar."""
    out = dict(zip(names, (out,) if isinstance(out, torch.Tensor) else out)) if not isinstance(out, dict) else out
    assert set(out) == set(names), (tag, sorted(out), names)
    worst, failed = 0.0, []
    for name in names:
        o = out[name]
        assert o.dtype == dt, (tag, name, o.dtype)
        r = ref[name] if take is None or name == "virial" else ref[name][take]
        assert bool(torch.isfinite(o).all()), f"{tag} {name}: not finite"
        if not r.any() and scale is None:
            SD._exactly_zero(o, f"{tag} {name}")
            continue
        rel = FP64_BAR if dt == F64 else 4.0 * own[name]
        top = np.abs(r).max() if scale is None else scale[name]
        err = float(np.abs(_np(o).reshape(r.shape) - r).max())
        print(f"{tag + ' ' + name:90s} rel err {err / top:.2e} (bar {rel:.2e})")
        if name in finite_only:
            continue
        if not err <= rel * top:  # every output's figure is printed before the first one fails the test
            failed.append(f"{tag} {name}: max err {err:.3e} > {rel * top:.3e} ({err / (rel * top):.3g} bars)")
        worst = max(worst, err / (rel * top))
    assert not failed, "\n".join(failed)
    return worst


def _selected(flags):
    return ["energies"] + [name for name, flag in zip(NAMES[1:], W.QUADRUPOLE_FLAGS) if flags.get(flag)]


def _grad_names(c):
    return [n for n in GRADS if not (c["no_dipoles"] and n == "dipole_grads")]


def _case(kind, key, dt, tag, c=None, take=None, flags=ALL, finite_only=()):
    """Forward with `flags` and the weighted backward of one case in dtype dt against the yardstick; returns (worst error / bar, outputs)."""
    c = W.pmeq_case(kind, key) if c is None else c
    own = W.pmeq_float32_deviation(kind, key) if dt == F32 else None
    out = _call(c, dt, flags)
    own_w = W.pmeq_float32_deviation(kind, key, weighted=True) if dt == F32 else None
    back = _backward(c, dt)
    worst, failed = 0.0, []
    for o, r, names, label, dev in ((out, W.pme_quadrupole_reference(kind, key), _selected(flags), tag, own),
                                    (back, W.pme_quadrupole_reference(kind, key, "float64", True), _grad_names(c), f"{tag} weighted backward", own_w)):
        try:
            worst = max(worst, _judge(o, r, names, dt, label, dev, take, finite_only=finite_only))
        except AssertionError as e:  # (the backward is judged, and its figures printed, whatever the forward call did)
            failed.append(str(e))
    assert not failed, "\n".join(failed)
    return worst, out, back


def _two_runs(a, b, what, dt):
    """Two device results of the same sums: 1e-12 of max in float64 (the spread adds in arrival order), the same bits in float32."""
    if dt == F32:
        assert torch.equal(a, b), f"{what}: float32 results differ by up to {float((a - b).abs().max()):.3e}"
    else:
        TPQ._close(a, b, what, TWO_RUNS)


# ---- the sweep ----------------------------------------------------------------------------------------------------------------------------------

def _correction_equals_its_halves(c, dt, tag):
    """`pme_quadrupole_correction` with the stored list (matrix and CSR) against `ewald_quadrupole_real_space` +
    `pme_quadrupole_reciprocal_space` of separate calls, all six outputs: a flag or a list argument not passed on shows here."""
    from nvalchemiops.interactions.electrostatics import ewald_quadrupole_real_space

    both, recip = TPQ._api()
    P, Q, M, T, C, A, BI, _ = _device(c, dt)
    f = SC._stored(c, mask_emptied=True)
    assert f["mask"] == c["emptied_row"] != f["n"], "a mask value that is not the default"
    mesh = dict(mesh_dimensions=c["mesh"], spline_order=c["order"], batch_idx=BI)
    rec = recip(P, Q, M, T, C, A, **mesh, **ALL)
    for fmt in ("matrix", "list"):
        lists = SD._lists(f, fmt)
        rs = ewald_quadrupole_real_space(P, Q, M, T, C, A, batch_idx=BI, **lists, **ALL)
        total = both(P, Q, M, T, C, A, **mesh, **lists, **ALL)
        assert len(total) == 6
        for name, t, a, b in zip(NAMES, total, rs, rec):
            assert float(a.abs().max()) > 0 or c["zero"], f"{tag} {fmt} {name}: the real-space half is trivial"
            _two_runs(t, a + b, f"{tag} correction {fmt} vs the two halves {name}", dt)
        # with the seed's flags (another instantiation of the gather where no forces are asked for: compared with the halves at the same flags)
        tup = lambda o: (o,) if isinstance(o, torch.Tensor) else o  # noqa: E731
        some = tup(both(P, Q, M, T, C, A, **mesh, **lists, **c["flags"]))
        halves = zip(tup(ewald_quadrupole_real_space(P, Q, M, T, C, A, batch_idx=BI, **lists, **c["flags"])), tup(recip(P, Q, M, T, C, A, **mesh, **c["flags"])))
        assert len(some) == len(_selected(c["flags"]))
        for name, t, (a, b) in zip(_selected(c["flags"]), some, halves):
            _two_runs(t, a + b, f"{tag} correction {fmt} with the seed's flags vs the two halves {name}", dt)


@pytest.mark.parametrize("seed", W.SEEDS)
def test_sweep(seed):
    base = W.pmeq_case("sweep", seed)
    c, take = (W.multipole_interleaved(base), base["perm"]) if base["perm"] is not None else (base, None)
    dt = SD._dtype(c)
    tag = f"pme_quadrupole {seed} {c['dtype']} order {c['order']} mesh {c['mesh']}"
    worst, _, back = _case("sweep", seed, dt, tag, c=c, take=take, flags=c["flags"])
    odd = c["mesh"][2] % 2 == 1 and not c["zero"]  # the Hermitian weight of the last half-spectrum plane: the virial, whatever the seed's flags
    if c["empty_system"] is not None or take is not None or c["no_dipoles"] or odd:
        out = _call(c, dt)
        worst = max(worst, _judge(out, W.pme_quadrupole_reference("sweep", seed), NAMES, dt, f"{tag} all outputs",
                                  W.pmeq_float32_deviation("sweep", seed) if dt == F32 else None, take))
    if c["empty_system"] is not None:
        assert out[5].shape == (3, 3, 3) and tuple(c["sizes"])[1] == 0
        SD._exactly_zero(out[5][c["empty_system"]], f"{tag}: virial row of the system without atoms")
    if take is not None:  # the same call on the sorted batch: two device results
        ordered, sorted_back = _call(base, dt), _backward(base, dt)
        where = torch.as_tensor(take, device=DEV)
        for name, a, b in zip(NAMES, out, ordered):
            TPQ._close(a, b if name == "virial" else b[where], f"{tag} interleaved vs sorted {name}", TWO_RUNS)
        for name in GRADS:
            TPQ._close(back[name], sorted_back[name][where], f"{tag} interleaved vs sorted weighted backward {name}", TWO_RUNS)
    if seed % 4 == 0:
        for other in (F64, F32):
            _correction_equals_its_halves(c, other, f"{tag} as {other}")
    print(f"[sweep] {tag}: sizes {c['sizes']}, flags {_selected(c['flags'])[1:]}, interleaved {take is not None}, zero {c['zero']}, "
          f"no dipoles {c['no_dipoles']}, worst error / bar {worst:.3g}")


@DTYPES
def test_batch_systems_equal_single_calls_forward_and_backward(dt):
    """Each system of the three-system seed alone gives the batch's slices, forward (all outputs) and weighted backward: in float64 at the bar
    of two device results, in float32 with both sides at the float32 bar against the yardstick (of the batch: 4 x its float32-mode deviation
    of the largest |value| of the output in the batch)."""
    seed = W.pmeq_batch_seed()
    c = W.pmeq_case("sweep", seed)
    assert len(c["sizes"]) == 3 and min(c["sizes"]) > 0
    tag = f"batch seed {seed} sizes {c['sizes']} {dt}"
    worst, out, back = _case("sweep", seed, dt, tag)
    ref, ref_w = W.pme_quadrupole_reference("sweep", seed), W.pme_quadrupole_reference("sweep", seed, "float64", True)
    own, own_w = (W.pmeq_float32_deviation("sweep", seed), W.pmeq_float32_deviation("sweep", seed, weighted=True)) if dt == F32 else (None, None)
    top, top_w = {k: np.abs(v).max() for k, v in ref.items()}, {k: np.abs(v).max() for k, v in ref_w.items()}
    for s in range(3):
        sel = np.nonzero(c["batch_idx"] == s)[0]
        one = dict(c, sizes=(len(sel),), batch_idx=np.zeros(len(sel), np.int32), cells=c["cells"][s:s + 1], alpha=c["alpha"][s:s + 1],
                   **{k: c[k][sel] for k in ("pos", "q", "mu", "qd", "weights")})
        single, single_back = _call(one, dt), _backward(one, dt)
        part = lambda name, x: x[s:s + 1] if name == "virial" else x[sel]  # noqa: E731
        if dt == F64:
            for name, o, full in zip(NAMES, single, out):
                scale = float(full.abs().max())
                assert float((o - part(name, full)).abs().max()) <= TWO_RUNS * scale, f"{tag} system {s} alone vs in the batch {name}"
            for name in GRADS:
                assert float((single_back[name] - back[name][sel]).abs().max()) <= TWO_RUNS * float(back[name].abs().max()), f"{tag} system {s} backward {name}"
        else:
            worst = max(worst, _judge(single, {k: part(k, v) for k, v in ref.items()}, NAMES, dt, f"{tag} system {s} alone", own, scale=top))
            worst = max(worst, _judge(single_back, {k: v[sel] for k, v in ref_w.items() if k in GRADS}, GRADS, dt, f"{tag} system {s} alone, weighted backward",
                                      own_w, scale=top_w))
    print(f"[batch] {tag}: worst error / bar {worst:.3g}")


# ---- ladders and knots ----------------------------------------------------------------------------------------------------------------------------

LADDER = [(order, n, dt) for order in W.PMEQ_ORDERS for n in W.pmeq_spread_rungs(order) for dt in (F64, F32)]


@pytest.mark.parametrize("order,n,dt", LADDER, ids=[f"{o}-{n}-{str(d)[6:]}" for o, n, d in LADDER])
def test_spread_gather_ladder(order, n, dt):
    """Blocks of `pme_quadrupole_spread_kernel` (256 // order^2 atoms) and `pme_quadrupole_gather_kernel` (32 atoms) one atom short of full,
    full, one atom into the next block and two blocks, and one atom alone, on the prime-and-odd mesh (9, 10, 11): forward with all flags and
    weighted backward, in both dtypes.  One atom alone in float32 (one gather block whose 31 surplus groups recompute atom 0): energies,
    charge_grads, quadrupole_grads and virial at the float32 bar, forward and weighted backward; forces and dipole_grads, which vanish for
    one atom but for the mesh's anisotropy, must be finite -- only these two, only there (`sweep_cases.pmeq_spread_case`)."""
    worst, _, _ = _case("spread", (order, n), dt, f"order {order} N {n} {dt}", finite_only=W.PMEQ_LONE_ATOM_EXEMPT if n == 1 and dt == F32 else ())
    print(f"[ladder] order {order} N = {n} {dt}: worst error / bar {worst:.3g}")


@DTYPES
@pytest.mark.parametrize("order,mesh", W.PMEQ_KNOT_CASES)
def test_atoms_on_spline_knots(order, mesh, dt):
    """Atoms whose mesh coordinates are integers and integers + 1/2 (`sweep_cases.pmeq_knot_case`): `floor` in `make_stencil`, the cut
    `u >= 0 && u < ORDER` and the indicator functions of `quadrupole_spline`.  Forward with all flags and weighted backward against the
    yardstick (continuous there: CPU suite), every output finite; and the same system with three atoms moved by -3, +2 and +1 whole cells."""
    key = (order, tuple(mesh))
    c = W.pmeq_case("knots", key)
    tag = f"knots order {order} mesh {mesh} {dt}"
    worst, out, back = _case("knots", key, dt, tag)
    moved = W.pmeq_translated(c)
    if dt == F64:
        for name, a, b in zip(NAMES, _call(moved, dt), out):
            TPQ._close(a, b, f"{tag} translated vs original {name}", TWO_RUNS)
        moved_back = _backward(moved, dt)
        for name in GRADS:
            TPQ._close(moved_back[name], back[name], f"{tag} translated vs original weighted backward {name}", TWO_RUNS)
    else:  # both sides at the float32 bar against the yardstick, which is periodic
        worst = max(worst, _case("knots", key, dt, f"{tag} translated", c=moved)[0])
    print(f"[knots] {tag}: worst error / bar {worst:.3g}")


def test_virial_second_trip():
    """Mesh (40, 36, 96): 70 560 half-spectrum points, the second trip of `pme_quadrupole_virial_kernel`'s grid-stride loop.  Float64 only
    (`sweep_cases.pmeq_big_mesh_case` says why)."""
    c = W.pmeq_case("big")
    out = _call(c, F64)
    worst = _judge(out, W.pme_quadrupole_reference("big", None), NAMES, F64, f"mesh {W.BIG_MESH}")
    print(f"[ladder] mesh {W.BIG_MESH}: worst error / bar {worst:.3g}")


# ---- the two paths of the mesh solve ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _home_references(order, dims):
    pos, q, mu, qd = TPQ._system()
    t = lambda a: torch.tensor(a, dtype=F64)  # noqa: E731
    w = np.random.default_rng(31).uniform(0.2, 1.8, len(pos))
    from tests import pme_quadrupole_reference as QR

    return w, TPQ._reference(order, dims), QR.evaluate(t(pos), t(q), t(mu), t(qd), t(TPQ.CELL), TPQ.ALPHA, dims, order, weights=t(w), virial=False)


def test_solve_paths_forward_and_adjoint(monkeypatch):
    """`_solve` takes the fused in-LDS solve where `mi_pme_solve_supported(m x B, ...)` says so, m = 2 meshes forward and 4 in the adjoint, and
    the hipFFT plans otherwise.  The table of what the meshes of this module take is printed; mesh (12, 10, 16) must run the fused solve and
    mesh (14, 12, 16) the plans, each in the forward call AND in the adjoint, observed (not inferred) by counting the calls of the two things
    only one path needs: the solve's twiddle tables and the FFT plans.  Then with `_MESH_SOLVE = False` mesh (12, 10, 16) through the plans:
    against the yardstick at its float64 bar (the bar of tests/test_sweep_dipoles_gpu.py::test_both_solve_paths), and against the fused result."""
    from nvalchemiops import _capi as C
    from nvalchemiops.interactions.electrostatics import pme

    _, recip = TPQ._api()
    code = C.dtype_code(F64)
    supported = lambda b, dims, cd=code: bool(C.lib().mi_pme_solve_supported(b, *dims, cd))  # noqa: E731
    used = {(W.pmeq_case("sweep", s)["mesh"], len(W.pmeq_case("sweep", s)["sizes"])) for s in W.SEEDS}
    used |= {(W.SPREAD_MESH, 1), (W.BIG_MESH, 1)} | {(tuple(m), 1) for _, m in W.PMEQ_KNOT_CASES}
    mixed = []
    for dims, nsys in sorted(used):
        fwd, adj = supported(2 * nsys, dims), supported(4 * nsys, dims)
        print(f"[solve] mesh {dims} x {nsys} systems: forward (b = {2 * nsys}) {'fused' if fwd else 'plans'}, adjoint (b = {4 * nsys}) {'fused' if adj else 'plans'}")
        if fwd != adj:
            mixed.append((dims, nsys))
    print(f"[solve] meshes whose forward call and adjoint take different paths: {mixed}")
    assert supported(2, TPQ.MESH) and supported(4, TPQ.MESH) and not supported(2, TPQ.MESH_PLAN) and not supported(4, TPQ.MESH_PLAN)
    assert pme._MESH_SOLVE is not False
    calls = {"tables": 0, "plans": 0}
    tables, plans = pme._solve_tables, pme._fft_plan

    def counted_tables(*a, **k):
        calls["tables"] += 1
        return tables(*a, **k)

    def counted_plans(*a, **k):
        calls["plans"] += 1
        return plans(*a, **k)

    monkeypatch.setattr(pme, "_solve_tables", counted_tables)
    monkeypatch.setattr(pme, "_fft_plan", counted_plans)
    P, Q, M, T, Cl = TPQ._inputs()
    results = {}
    for order, dims, switch, path in ((5, TPQ.MESH, None, "fused"), (6, TPQ.MESH_PLAN, None, "plans"), (5, TPQ.MESH, False, "plans")):
        if switch is False:
            monkeypatch.setattr(pme, "_MESH_SOLVE", False)
        w, ref, ref_w = _home_references(order, dims)
        before = dict(calls)
        out = recip(P, Q, M, T, Cl, TPQ.ALPHA, mesh_dimensions=dims, spline_order=order, **ALL)
        forward = {k: calls[k] - before[k] for k in calls}
        leaves = [x.clone().requires_grad_(True) for x in (P, Q, M, T)]
        e = recip(*leaves, Cl, TPQ.ALPHA, mesh_dimensions=dims, spline_order=order)
        before = dict(calls)
        gp, gq, gm, gt = torch.autograd.grad((e * _t(w)).sum(), leaves)
        adjoint = {k: calls[k] - before[k] for k in calls}
        print(f"[solve] order {order} mesh {dims} expected {path}: forward {forward}, adjoint {adjoint}")
        for label, seen in (("forward", forward), ("adjoint", adjoint)):
            if path == "fused":
                assert seen["tables"] >= 1 and seen["plans"] == 0, f"mesh {dims} {label}: the fused solve did not run ({seen})"
            else:
                assert seen["plans"] >= 2 and seen["tables"] == 0, f"mesh {dims} {label}: the FFT plans did not run ({seen})"
        tag = f"order {order} mesh {dims} {path}{' (fused solve switched off)' if switch is False else ''}"
        worst = _judge(out, ref, NAMES, F64, tag)
        back = dict(zip(GRADS, (-gp, gq, gm, gt)))
        worst = max(worst, _judge(back, ref_w, GRADS, F64, f"{tag} weighted backward"))
        print(f"[solve] {tag}: worst error / bar {worst:.3g}")
        results[(dims, path)] = (out, back)
    (a, ab), (b, bb) = results[(TPQ.MESH, "fused")], results[(TPQ.MESH, "plans")]
    for name, x, y in zip(NAMES, a, b):
        TPQ._close(x, y, f"fused vs plans {name}", FP64_BAR)
    for name in GRADS:
        TPQ._close(ab[name], bb[name], f"fused vs plans weighted backward {name}", FP64_BAR)


# ---- the explicit routine ----------------------------------------------------------------------------------------------------------------------------

def test_mesh_term_converges_to_the_explicit_sum_in_every_output():
    """The comparison of tests/test_pme_quadrupole_gpu.py::test_correction_agrees_with_the_explicit_ewald_routine (same full list, same alpha,
    order 6 on 32^3 against the explicit sum over the converged k set) with all six outputs asserted.  The bar per output is 10 x what the two
    RESTATEMENTS differ by on the same system (module docstring; the factor and the rule of that test's energy bar)."""
    from nvalchemiops.interactions.electrostatics import (ewald_quadrupole_correction, ewald_quadrupole_reciprocal_space,
                                                          generate_k_vectors_ewald_summation)

    both, _ = TPQ._api()
    order, dims = 6, (32, 32, 32)
    measured = W.pmeq_convergence()
    P, Q, M, T, C = TPQ._inputs()
    lists = TPQ._neighbours(P, C)
    kv = generate_k_vectors_ewald_summation(C, 4.5)
    want = ewald_quadrupole_correction(P, Q, M, T, C, TPQ.ALPHA, kv, **lists, **ALL)
    got = both(P, Q, M, T, C, TPQ.ALPHA, mesh_dimensions=dims, spline_order=order, **lists, **ALL)
    half = ewald_quadrupole_reciprocal_space(P, Q, M, T, C, kv, TPQ.ALPHA, **ALL)
    assert len(got) == len(want) == len(half) == 6
    for name, a, b, h in zip(NAMES, got, want, half):
        TPQ._close(a, b, f"mesh vs explicit {name}", 10.0 * measured[name])
        # the real-space halves are the same launch, so the difference is that of the reciprocal halves: held to the same factor of THEIR
        # largest value, which is what the restatements' difference is relative to (the totals are up to 100 x larger: close contacts)
        err, scale = float((a - b).abs().max()), float(h.abs().max())
        print(f"mesh vs explicit {name:16s} difference {err / scale:.2e} of the largest reciprocal value (bar {10.0 * measured[name]:.2e})")
        assert err <= 10.0 * measured[name] * scale, f"{name}: {err:.3e} > {10.0 * measured[name] * scale:.3e}"
