"""Seeded sweeps and boundary ladders of `ewald_quadrupole_correction` (csrc/quadrupole.hip) and `thole_dipole_correction` (the second
instantiation of `dp_pair_kernel`, csrc/dipole.hip), and one batch of idle systems for `induced_dipoles` (csrc/induced.hip), against the
float64 restatements tests/quadrupole_reference.py, tests/thole_reference.py and tests/induced_reference.py -- evaluated on the entries
actually stored and on the same k set.  The inputs are those of tests/sweep_cases.py (multipole section; tests/test_sweep_cases_cpu.py
asserts their conditions without a device).  No tolerance is new; the comparison functions are those of the operators' parity modules:

    float64     1e-11 of max |ref| + 1e-14 per output                       tests/test_quadrupole_gpu.py::_close, tests/test_thole_gpu.py::_close
    float32     1e-6 of max |ref| against the restatement's float32-distance mode
    the solve   `_check_solution` of tests/test_induced_gpu.py: |mu - mu_ref| <= 10 tol ||b|| / lambda_min + 1e-14

What the sweeps and ladders reach that the parity modules do not.  Quadrupoles: a list without shifts (`ush == nullptr` in `qd_pair_kernel`),
systems of 255 / 256 / 257 atoms and a system without atoms inside a batch (`qd_sf_kernel`'s stride and `sptr`), an interleaved batch in real
space, `k_vectors` [1, K, 3] over several systems, each flag alone, the instantiation without forces and virial in float32, twelve seeds.
Thole: rows of exactly 0, 1, 63, 64, 65, 128 and 129 entries with entries on both sides of the exit at E = 50 in every row (lanes leave the
trip early), the cluster form, a batch with a system without atoms.  Induced dipoles: a system without atoms and a system without a
polarisable atom next to one that iterates.

MEASURED on one MI355X (worst error / bar; every test prints its figures under `pytest -s`): quadrupole sweep 0.0019
in float64 (1.8e-14 of max |ref|, the interleaved seed 4) and 0.40 in float32 over the twelve seeds, Thole sweep 0.0004 and 0.35;
interleaved against sorted: per-atom outputs bit-equal, virial within the float64 bar; the list without shifts bit-equal to the list with
zero shifts (0.0001 against the restatement); `k_vectors` [1, K, 3] bit-equal to [B, K, 3] (0.0004); atom ladder 0.0004; Thole row ladder
0.00008 (periodic) and 0.00009 (cluster); the idle-systems batch: 11 iterations for the lattice (reference PCG 11), 0 for the other two.
32 tests in 15 s.
"""
import numpy as np
import pytest
import torch

from tests import dipole_reference as DR
from tests import induced_reference as IR
from tests import quadrupole_reference as XR
from tests import sweep_cases as W
from tests import test_induced_gpu as TI
from tests import test_quadrupole_gpu as TQD
from tests import test_sweep_charges_gpu as SC
from tests import test_sweep_dipoles_gpu as SD
from tests import test_thole_gpu as TTH
from tests import thole_reference as TR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
_t = TQD._t


def _rel(dt):
    return 1e-11 if dt == F64 else 1e-6


def _selected(op, flags):
    names = W.MULTIPOLE_NAMES[op]
    return [names[0]] + [name for name, flag in zip(names[1:], W.MULTIPOLE_FLAGS[op]) if flags.get(flag)]


def _judge(out, ref, names, dt, tag, exact_zero=()):
    """Outputs against the restatement at the parity modules' bar (their `_close` is one function: rel x max |ref| + 1e-14); the outputs
    named in `exact_zero` must be exactly 0.0.  Returns the worst error / bar."""
    out = (out,) if isinstance(out, torch.Tensor) else out
    assert len(out) == len(names) and all(o.dtype == dt for o in out), tag
    worst = 0.0
    for name, o in zip(names, out):
        if name in exact_zero:
            SD._exactly_zero(o, f"{tag} {name}")
        else:
            worst = max(worst, TQD._close(o, ref[name], f"{tag} {name}", _rel(dt)) / _rel(dt))
    return worst


def _sweep(op, seed):
    """One seed of either operator: both list formats with the seed's flags, the weighted backward on the seeds that ask for it, and on the
    interleaved seeds the same call on the sorted batch."""
    quadrupole = op == "ewald_quadrupole"
    both, real, _ = TQD._api()
    th = TTH._api()[0]
    base = W.multipole_case("sweep", (op, seed))
    c = W.multipole_interleaved(base) if base["perm"] is not None else base
    halves = "total" if quadrupole and base["perm"] is None else "real space"  # `ewald_quadrupole_reciprocal_space` documents contiguous systems
    dt = SD._dtype(c)
    names_all, grads = W.MULTIPOLE_NAMES[op], W.MULTIPOLE_NAMES[op][1:5]
    zero_names = () if not c["zero"] else tuple(n for n in names_all if n != "quadrupole_grads")

    def device(case):
        P, Q, M, C, A, BI, w = SD._device(case, dt)
        f = SC._stored(case, mask_emptied=True)
        return P, Q, M, _t(case["qd" if quadrupole else "polar"], dt), C, A, BI, w, f

    def run(dev, p, q, m, x, fmt, **flags):
        _, _, _, _, C, A, BI, _, f = dev
        if not quadrupole:
            return th(p, q, m, x, C, thole=W.THOLE, batch_idx=BI, **SD._lists(f, fmt), **flags)
        if halves == "total":
            return both(p, q, m, x, C, A, kv, batch_idx=BI, **SD._lists(f, fmt), **flags)
        return real(p, q, m, x, C, A, batch_idx=BI, **SD._lists(f, fmt), **flags)

    dev = device(c)
    P, Q, M, X, C, A, BI, w, f = dev
    entries = DR.entries_from_matrix(f["nm"], f["sh"], f["mask"])
    assert entries[0].shape[0] == len(W.stored_entries(c)[0]) and not bool((entries[0] == c["emptied_row"]).any())
    kv = SD._k_vectors(c, C) if halves == "total" else None

    def reference(weights=None):
        if quadrupole:
            return XR.evaluate(P, Q, M, X, C, A, entries, kv, batch_idx=BI, distance_dtype=dt, weights=weights)
        return TR.evaluate(P, Q, M, X, C, W.THOLE, entries, batch_idx=BI, distance_dtype=dt, weights=weights)

    ref = reference()
    names = _selected(op, c["flags"])
    tag = f"{op} {seed} {c['dtype']} {halves}"
    worst = 0.0
    for fmt in ("matrix", "list"):
        out = run(dev, P, Q, M, X, fmt, **c["flags"])
        worst = max(worst, _judge(out, ref, names, dt, f"{tag} {fmt}", zero_names))
        if c["empty_system"] is not None and c["flags"]["compute_virial"]:
            SD._exactly_zero(out[-1][c["empty_system"]], f"{tag} {fmt}: virial row of the system without atoms")
    if c["autograd"]:
        fmt = ("matrix", "list")[seed % 2]
        leaves = [x.clone().requires_grad_(True) for x in (P, Q, M, X)]
        gp, gq, gm, gx = torch.autograd.grad((run(dev, *leaves, fmt) * w.to(dt)).sum(), leaves)
        if not quadrupole:
            gx = torch.nan_to_num(gx)  # (as tests/test_thole_gpu.py reads the polarisability gradient)
        worst = max(worst, _judge((-gp, gq, gm, gx), reference(w), grads, dt, f"{tag} {fmt} weighted backward"))
    if base["perm"] is not None:
        # the sorted batch: the rows hold the same entries in the same order, so every per-atom output has the same bits, atom by atom; the
        # per-system virial is folded over the rows in another order and is held to the bar of the module
        flags = dict(zip(W.MULTIPOLE_FLAGS[op], [True] * 5))
        sdev = device(base)
        take = _t(base["perm"])
        for fmt in ("matrix", "list"):
            a, b = run(dev, P, Q, M, X, fmt, **flags), run(sdev, *sdev[:4], fmt, **flags)
            for name, x, y in zip(names_all[:5], a, b):
                assert torch.equal(x, y[take]), f"{tag} {fmt} {name}: the interleaved batch differs from the sorted one by up to {float((x - y[take]).abs().max()):.3e}"
            worst = max(worst, TQD._close(a[5], b[5], f"{tag} {fmt} interleaved vs sorted virial", _rel(dt)) / _rel(dt))
    print(f"[sweep] {tag}: sizes {c['sizes']}, {entries[0].shape[0]} entries, K {0 if kv is None else kv.shape[-2]}, outputs {names}, "
          f"backward {c['autograd']}, interleaved {base['perm'] is not None}, zero {c['zero']}, worst error / bar {worst:.3g}")


@pytest.mark.parametrize("seed", W.SEEDS)
def test_ewald_quadrupole_sweep(seed):
    _sweep("ewald_quadrupole", seed)


@pytest.mark.parametrize("seed", W.SEEDS)
def test_thole_sweep(seed):
    _sweep("thole", seed)


# ---- ladders ------------------------------------------------------------------------------------------------------------------------------------

def test_quadrupole_atom_ladder():
    """Systems of 255, 256, 257 and 1 atoms in one batch against the 256 atoms of one trip of `qd_sf_kernel`; judged system by system at
    the bar of the whole batch, so that a failure names its system."""
    _, _, recip = TQD._api()
    c = W.multipole_case("atoms")
    P, Q, M, C, A, BI, w = SD._device(c, F64)
    T = _t(c["qd"])
    kv = SD._k_vectors(c, C)
    assert kv.shape[0] == 4 and 60 <= kv.shape[1] <= 70
    ref = XR.evaluate(P, Q, M, T, C, A, None, kv, batch_idx=BI)
    ref_w = XR.evaluate(P, Q, M, T, C, A, None, kv, batch_idx=BI, weights=w)
    out = recip(P, Q, M, T, C, kv, A, batch_idx=BI, **TQD.ALL)
    leaves = [x.clone().requires_grad_(True) for x in (P, Q, M, T)]
    gp, gq, gm, gt = torch.autograd.grad((recip(*leaves, C, kv, A, batch_idx=BI) * w).sum(), leaves)
    bounds = np.concatenate([[0], np.cumsum(c["sizes"])])
    failed, worst = [], 0.0
    for label, names, outs, r in (("", TQD.NAMES, out, ref), ("weighted backward ", TQD.NAMES[1:5], (-gp, gq, gm, gt), ref_w)):
        for name, o in zip(names, outs):
            got, want = TQD._np(o), r[name]
            bar = 1e-11 * np.abs(want).max() + 1e-14
            for s, size in enumerate(c["sizes"]):
                sl = slice(s, s + 1) if name == "virial" else slice(bounds[s], bounds[s + 1])
                err = float(np.abs(got[sl] - want[sl]).max())
                worst = max(worst, err / bar)
                if err > bar:
                    failed.append(f"system of {size} atoms: {label}{name} error / bar {err / bar:.3g}")
    print(f"[ladder] quadrupole systems of {c['sizes']} atoms: worst error / bar {worst:.3g}")
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("fmt", ["matrix", "list"])
def test_quadrupole_list_without_shifts(fmt):
    """A list without shifts is the list with zero shifts, bit for bit (`cm = 0` in `qd_pair_kernel`); the virial needs the shifts."""
    _, real, _ = TQD._api()
    c = W.multipole_case("no_shifts")
    P, Q, M, C, A, _, w = SD._device(c, F64)
    T = _t(c["qd"])
    f = SC._stored(c)
    assert not bool(f["sh"].any()) and f["nm"].shape == (65, 64)
    ref = XR.evaluate(P, Q, M, T, C, A, DR.entries_from_matrix(f["nm"], f["sh"], f["mask"]), None)
    with_zero = real(P, Q, M, T, C, A, **SD._lists(f, fmt), **TQD.GRADS)
    without = real(P, Q, M, T, C, A, **SD._lists(f, fmt, shifts=False), **TQD.GRADS)
    worst = _judge(without, ref, TQD.NAMES[:5], F64, f"quadrupole {fmt} without shifts")
    for name, a, b in zip(TQD.NAMES, without, with_zero):
        assert torch.equal(a, b), f"{fmt} {name}: a list without shifts is not bit-equal to the list with zero shifts (max difference {float((a - b).abs().max()):.3e})"
    leaves = [x.clone().requires_grad_(True) for x in (P, Q, M, T)]
    gp, gq, gm, gt = torch.autograd.grad((real(*leaves, C, A, **SD._lists(f, fmt, shifts=False)) * w).sum(), leaves)
    worst = max(worst, _judge((-gp, gq, gm, gt), XR.evaluate(P, Q, M, T, C, A, DR.entries_from_matrix(f["nm"], f["sh"], f["mask"]), None, weights=w),
                              TQD.NAMES[1:5], F64, f"quadrupole {fmt} without shifts, weighted backward"))
    with pytest.raises(ValueError, match="compute_virial needs the shifts of the list"):
        real(P, Q, M, T, C, A, **SD._lists(f, fmt, shifts=False), compute_virial=True)
    print(f"[ladder] quadrupole {fmt} without shifts: worst error / bar {worst:.3g}; bit-equal to zero shifts")


def test_quadrupole_k_vectors_shared_by_a_batch():
    """`k_vectors` [1, K, 3] over two systems in the same cell: the bits of the repeated [2, K, 3] set, and the restatement's numbers."""
    _, _, recip = TQD._api()
    c = W.multipole_case("shared_k")
    P, Q, M, C, A, BI, _ = SD._device(c, F64)
    T = _t(c["qd"])
    kv = TQD._k_vectors(C[0], c["k_cutoff"])
    assert kv.dim() == 2 and kv.shape[0] > 64
    one = recip(P, Q, M, T, C, kv[None], A, batch_idx=BI, **TQD.ALL)
    full = recip(P, Q, M, T, C, kv[None].repeat(2, 1, 1).contiguous(), A, batch_idx=BI, **TQD.ALL)
    worst = _judge(one, XR.evaluate(P, Q, M, T, C, A, None, kv, batch_idx=BI), TQD.NAMES, F64, "k_vectors [1, K, 3] over two systems")
    for name, a, b in zip(TQD.NAMES, one, full):
        assert torch.equal(a, b), f"{name}: k_vectors [1, K, 3] is not bit-equal to [2, K, 3]"
    print(f"[ladder] k_vectors [1, {kv.shape[0]}, 3] over systems of {c['sizes']} atoms: worst error / bar {worst:.3g}; bit-equal to [2, K, 3]")


@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "cluster"])
def test_thole_row_ladder(periodic):
    """Rows of exactly 0, 1, 63, 64, 65, 128 and 129 entries, every row from 63 up with entries on both sides of E = 50 (the CPU suite
    asserts it), in both list formats; judged on the whole system and on the ladder rows alone, relative to their own largest value."""
    th = TTH._api()[0]
    c = W.multipole_case("thole_rows", periodic)
    rows = len(W.THOLE_ROWS)
    t = lambda a: _t(a, F64)  # noqa: E731
    P, Q, M, A, w = t(c["pos"]), t(c["q"]), t(c["mu"]), t(c["polar"]), t(c["weights"])
    C = t(c["cells"]) if periodic else None
    f = SC._stored(c)
    ptr = f["ptr"].long()
    assert tuple(int(x) for x in (ptr[1:] - ptr[:-1])[:rows]) == W.THOLE_ROWS and (periodic or not bool(f["sh"].any()))
    entries = DR.entries_from_matrix(f["nm"], f["sh"], f["mask"])
    ref, ref_w = TR.evaluate(P, Q, M, A, C, W.THOLE, entries), TR.evaluate(P, Q, M, A, C, W.THOLE, entries, weights=w)
    flags = dict(TTH.ALL, compute_virial=periodic)
    names = [k for k in TTH.NAMES if k != "virial" or periodic]
    worst = 0.0
    for fmt in ("matrix", "list"):
        lists = SD._lists(f, fmt, shifts=periodic)
        out = th(P, Q, M, A, C, thole=W.THOLE, **lists, **flags)
        worst = max(worst, _judge(out, ref, names, F64, f"thole rows of {W.THOLE_ROWS} entries, {fmt}"))
        for name, o in zip(names[:5], out):
            worst = max(worst, TQD._close(o[1:rows], ref[name][1:rows], f"  the ladder rows alone, {fmt} {name}", 1e-11) / 1e-11)
            SD._exactly_zero(o[0], f"the row without entries, {fmt} {name}")
        leaves = [x.clone().requires_grad_(True) for x in (P, Q, M, A)]
        gp, gq, gm, ga = torch.autograd.grad((th(*leaves, C, thole=W.THOLE, **lists) * w).sum(), leaves)
        worst = max(worst, _judge((-gp, gq, gm, torch.nan_to_num(ga)), ref_w, TTH.NAMES[1:5], F64, f"thole row ladder {fmt} weighted backward"))
    print(f"[ladder] thole rows of {W.THOLE_ROWS} entries ({'periodic' if periodic else 'cluster, cell=None'}): worst error / bar {worst:.3g}")


# ---- induced dipoles: idle systems next to one that iterates ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["matrix", "list"])
def test_induced_dipoles_with_a_system_without_atoms_and_one_without_a_polarisable_atom(fmt):
    from nvalchemiops.interactions.electrostatics import InducedDipoleResult, generate_k_vectors_ewald_summation, induced_dipoles

    tol = 1e-10
    c = W.induced_idle_systems_case()
    t = lambda a: _t(a, F64)  # noqa: E731
    P, Q, A, C, AL, BI = t(c["pos"]), t(c["q"]), t(c["polar"]), t(c["cells"]), t(c["alpha"]), _t(c["batch_idx"])
    f = SC._stored(c)
    kv = generate_k_vectors_ewald_summation(C, c["k_cutoff"])
    assert kv.shape[0] == 3
    out = induced_dipoles(P, Q, A, C, batch_idx=BI, reciprocal="ewald", alpha=AL, k_vectors=kv, tolerance=tol, return_info=True, **SD._lists(f, fmt))
    assert out.dipoles.shape == (36, 3) and out.iterations.shape == (3,) and not bool(torch.isnan(out.dipoles).any())
    SD._exactly_zero(out.dipoles[27:], "dipoles of the system without a polarisable atom")
    assert out.iterations[1:].tolist() == [0, 0] and out.residual[1:].tolist() == [0.0, 0.0] and out.polarization_energy[1:].tolist() == [0.0, 0.0]
    # system 0 against the dense solve with the k set the call used for it
    i, j, S = DR.entries_from_matrix(f["nm"], f["sh"], f["mask"])
    own = i < 27
    T, lin = IR.dipole_operator(P[:27], Q[:27], C[0], float(AL[0]), (i[own], j[own], S[own]), kv[0])
    H, b = IR.system_matrix(T, A[:27]), IR.right_hand_side(lin, A[:27])
    first = InducedDipoleResult(out.dipoles[:27], out.polarization_energy[:1], out.iterations[:1], out.residual[:1])
    TI._check_solution(first, H, b, A[:27], None, 1, tol, f"induced {fmt}: the system that iterates, next to two idle ones")
    assert int(out.iterations[0]) > 4
