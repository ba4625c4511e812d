"""Seeded sweeps and ladders of `coulomb_dipole_correction`, `coulomb_quadrupole_correction`, `pair_scale_correction`, `rotate_multipoles` and
`multipole_frame_forces` (cases: tests/sweep_cases.py, whose conditions tests/test_sweep_cases_cpu.py asserts per seed).

What a hand-made fixture does not happen to hold: a batch with a system without atoms, an interleaved `batch_idx`, each compute flag alone
(the `FV = false` kernels in float32 too), `minimum_image` on batches, matrix rows with a padding slot between live entries, an entry with
r <= 1e-8, float32 scales next to float64 positions and the reverse, one multipole input None; for the frames a randomly permuted atom order
(frame atoms above and below their owner and in another block of 256 threads), every kind mixed, Z_THEN_X with and without a y atom side
by side, wrapped positions in one cell and in batches.

No new tolerance: every comparison is `_close` of the operator's parity module against its float64 restatement on the entries actually
stored -- 1e-11 of max|ref| (+ 1e-14) in float64, 1e-6 against the restatement's float32 mode -- or bits: zero-multipole seeds give exact
zeros, the interleaved call gives the bits of the sorted call (CSR form: a row's entries then sit in the same slots), a pair at r = 0 the
bits of the call that skips it, a system without atoms an exactly zero virial row.

MEASURED on one MI355X (`pytest -s` prints one line per case).  Worst error / bar over the twelve seeds, float64 / float32: coulomb_dipole
9.4e-4 / 0.22, coulomb_quadrupole 4.5e-4 / 0.69, pair_scale 8.9e-4 / 0.60; the pair-scale batch ladder 2.2e-4 / 0.49 in both formats; frames
1.3e-3 / 0.049.  Every exact-zero and every bit-for-bit assertion held: zero-multipole seeds, interleaved seeds 4 and 8, the systems without
atoms, the coincident pair of seed 9.  DESIGN.md section 3.33 has the table."""
import numpy as np
import pytest
import torch

from tests import cluster_multipole_reference as CR
from tests import local_frames_reference as LR
from tests import pair_scale_reference as PR
from tests import sweep_cases as W
from tests import test_cluster_multipole_gpu as TCM
from tests import test_local_frames_gpu as TLF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64, F32, I32 = torch.float64, torch.float32, torch.int32
_WORST = {}


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


def _dt(c):
    return F64 if c["dtype"] == "float64" else F32


def _close(o, ref, what, rel, key):
    ref = ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else ref
    got = o.detach().cpu().numpy().astype(np.float64)
    scale = max(np.abs(ref).max(), 1e-30) if ref.size else 1.0
    _WORST[key] = max(_WORST.get(key, 0.0), float(np.abs(got - ref).max() / (rel * scale + 1e-14)) if ref.size else 0.0)
    TCM._close(o, ref, what, rel)


def _fn(op):
    from nvalchemiops.interactions.electrostatics import coulomb_dipole_correction, coulomb_quadrupole_correction, pair_scale_correction

    return dict(coulomb_dipole=coulomb_dipole_correction, coulomb_quadrupole=coulomb_quadrupole_correction, pair_scale=pair_scale_correction)[op]


def _atoms(c):
    """The positional arguments of the op in the case's dtype (None for a multipole the seed leaves out)."""
    dt = _dt(c)
    P, Q, MU, QD = (_t(c[k], dt) for k in ("pos", "q", "mu", "qd"))
    if c["op"] == "coulomb_dipole":
        return [P, Q, MU]
    if c["op"] == "coulomb_quadrupole":
        return [P, Q, MU, QD]
    return [P, Q, None if c.get("no_dipoles") else MU, None if c.get("no_quadrupoles") else QD]


def _scales(c, values=None):
    sdt = F64 if c.get("scale_dtype", "float64") == "float64" else F32
    return _t(c["scales"] if values is None else values, sdt)


def _lists(c, fmt, scales=None):
    """The keyword arguments that carry the list (and, for `pair_scale`, the scales beside it; NaN on the padding of the matrix)."""
    i, j, S = c["entries"]
    n = len(c["pos"])
    shifts = c["periodic"] and not c["minimum_image"]
    sc = None if c["op"] != "pair_scale" else (c["scales"] if scales is None else scales)
    if fmt == "matrix":
        nm, sh, val = W.padded_matrix(c["entries"], n, sc)
        kw = dict(neighbor_matrix=_t(nm), mask_value=n, **(dict(neighbor_matrix_shifts=_t(sh)) if shifts else {}))
        if sc is not None:
            kw["pair_scales"] = _scales(c, val)
    else:
        ptr = np.zeros(n + 1, np.int32)
        ptr[1:] = np.cumsum(np.bincount(i, minlength=n))
        kw = dict(neighbor_list=_t(np.stack([i, j]).astype(np.int32)), neighbor_ptr=_t(ptr), **(dict(neighbor_shifts=_t(S.astype(np.int32))) if shifts else {}))
        if sc is not None:
            kw["pair_scales"] = _scales(c, sc)
    return kw


def _call(c, fmt, flags, atoms=None, scales=None):
    dt = _dt(c)
    atoms = _atoms(c) if atoms is None else atoms
    kw = _lists(c, fmt, scales)
    cell = _t(c["cells"], dt) if c["periodic"] else None
    if c["op"] == "pair_scale":
        return _fn(c["op"])(*atoms, kw.pop("pair_scales"), cell, batch_idx=_t(c["batch_idx"]) if c["periodic"] else None,
                            minimum_image=c["minimum_image"], **kw, **flags)
    return _fn(c["op"])(*atoms, cell, batch_idx=_t(c["batch_idx"]) if c["periodic"] else None, **kw, **flags)


def _reference(c, weighted=False):
    """The float64 restatement at the inputs rounded to the case's dtype (and the scales to theirs), on the stored entries."""
    dt = _dt(c)
    P, Q, MU, QD = (_t(c[k], dt) for k in ("pos", "q", "mu", "qd"))
    ent = tuple(_t(e).long() for e in c["entries"])
    cell = _t(c["cells"], dt) if c["periodic"] else None
    bi = _t(c["batch_idx"]) if c["periodic"] else None
    w = _t(c["weights"]) if weighted else None
    if c["op"] == "coulomb_dipole":
        return CR.dipole_evaluate(P, Q, MU, ent, cell=cell, batch_idx=bi, distance_dtype=dt, weights=w)
    if c["op"] == "coulomb_quadrupole":
        return CR.quadrupole_evaluate(P, Q, MU, QD, ent, cell=cell, batch_idx=bi, distance_dtype=dt, weights=w)
    return PR.evaluate(P, Q, None if c.get("no_dipoles") else MU, None if c.get("no_quadrupoles") else QD, _scales(c).to(F64), ent, cell=cell, batch_idx=bi,
                       distance_dtype=dt, weights=w, minimum_image=c["minimum_image"])


def _named(c, flags, out):
    out = out if isinstance(out, tuple) else (out,)
    names = ["energies"] + [n for n, f in zip(W.CLUSTER_NAMES[c["op"]][1:], W.CLUSTER_FLAGS[c["op"]]) if flags.get(f)]
    assert len(names) == len(out)
    return dict(zip(names, out))


def _all_flags(c):
    return {f: (f != "compute_virial" or c["periodic"]) for f in W.CLUSTER_FLAGS[c["op"]]}


@pytest.mark.parametrize("seed", W.SEEDS)
@pytest.mark.parametrize("op", W.CLUSTER_OPS)
def test_cluster_and_pair_scale_sweep(op, seed):
    c = W.cluster_case("sweep", (op, seed))
    dt, rel = _dt(c), (1e-11 if c["dtype"] == "float64" else 1e-6)
    key = f"{op} {c['dtype']}"
    ref = _reference(c)
    for fmt in ("matrix", "list"):
        got = _named(c, c["flags"], _call(c, fmt, c["flags"]))
        for name, o in got.items():
            assert o.dtype == dt
            _close(o, ref[name], f"sweep {op} seed {seed} {fmt} {name}", rel, key)
    every = _all_flags(c)
    full = _named(c, every, _call(c, "list", every))
    for name, o in full.items():
        _close(o, ref[name], f"sweep {op} seed {seed} every flag, {name}", rel, key)
    if c["zero"]:  # zero dipoles / zero quadrupoles / unit scales: exact zeros but for the field (gradient) of the charges
        keep = {"coulomb_dipole": "dipole_grads", "coulomb_quadrupole": "quadrupole_grads", "pair_scale": None}[op]
        for name, o in full.items():
            assert name == keep or not bool(o.any()), f"{op} seed {seed}: {name} is not exactly zero"
        assert keep is None or float(full[keep].abs().max()) > 0
    if c["perm"] is not None:  # the interleaved batch: bits of the sorted call, atom by atom
        ci = W.cluster_interleaved(c)
        mixed = _named(ci, every, _call(ci, "list", every))
        assert bool((np.diff(ci["batch_idx"]) < 0).any())
        perm = _t(c["perm"])
        for name, o in mixed.items():
            if name == "virial":
                _close(o, full[name], f"sweep {op} seed {seed} interleaved virial against the sorted call", 1e-11, key)
            else:
                assert torch.equal(o, full[name][perm]), f"{op} seed {seed} interleaved: {name} differs from the sorted call's"
    if c["empty_system"] is not None and c["periodic"]:
        assert full["virial"].shape[0] == len(c["sizes"]) and not bool(full["virial"][c["empty_system"]].any())
    if c["coincident"] is not None:  # the pair at r = 0 contributes exactly nothing: the bits of the call in which its scale is 1
        i, j, _ = c["entries"]
        pair = ((i == c["coincident"][0]) & (j == c["coincident"][1])) | ((i == c["coincident"][1]) & (j == c["coincident"][0]))
        assert int(pair.sum()) == 2 and bool((c["scales"][pair] != 1.0).all())
        skipped = _named(c, every, _call(c, "list", every, scales=np.where(pair, 1.0, c["scales"])))
        for name, o in full.items():
            assert torch.equal(o, skipped[name]) and not bool(torch.isnan(o).any()), name
    if c["autograd"]:
        refw = _reference(c, weighted=True)
        leaves = [None if a is None else a.clone().requires_grad_(True) for a in _atoms(c)]
        e = _call(c, "list", {}, atoms=leaves)
        (_t(c["weights"]).to(dt) * e).sum().backward()
        for name, leaf, sign in zip(W.CLUSTER_NAMES[op][1:-1], leaves, (-1.0, 1.0, 1.0, 1.0)):
            if leaf is not None:
                _close(sign * leaf.grad, refw[name], f"sweep {op} seed {seed} weighted backward, {name}", rel, key)
    print(f"[sweep] {op:18s} seed {seed:2d} {c['dtype']} sizes {c['sizes']} {'cells' if c['periodic'] else 'clusters'}"
          f"{' minimum image' if c['minimum_image'] else ''}: worst error / bar so far {_WORST[key]:.3g}")


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("fmt", ["matrix", "list"])
def test_pair_scale_batch_ladder_under_minimum_image(fmt, dtype):
    """255, 256, 257 and 1 atoms per system in one batch: the group-of-8 kernel at system boundaries that fall inside a wave and a block."""
    c = dict(W.cluster_case("ps_ladder"), dtype=dtype)
    rel, every = (1e-11 if dtype == "float64" else 1e-6), _all_flags(c)
    ref = _reference(c)
    for name, o in _named(c, every, _call(c, fmt, every)).items():
        _close(o, ref[name], f"pair scale ladder {fmt} {dtype} {name}", rel, f"ladder {dtype}")
    print(f"[sweep] pair scale ladder {fmt} {dtype}: worst error / bar {_WORST[f'ladder {dtype}']:.3g}")


@pytest.mark.parametrize("seed", W.SEEDS)
def test_local_frames_sweep(seed):
    """Rotation, `backward()` with random output weights, and the explicit path with local gradients and (with a cell) the virial term, on a
    random topology in a random atom order."""
    from nvalchemiops.interactions.electrostatics import LocalFrames, multipole_frame_forces, rotate_multipoles

    c = W.cluster_case("frames", seed)
    dt, rel = _dt(c), (1e-11 if c["dtype"] == "float64" else 1e-6)
    key = f"frames {c['dtype']}"
    dev = lambda x: None if x is None else x.to(DEV, dt)  # noqa: E731
    P, MU, QD, WMU, WQ, cell = (dev(c[k]) for k in ("pos", "mu", "quad", "w_mu", "w_q", "cells"))
    bi = None if c["batch_idx"] is None else c["batch_idx"].to(DEV)
    rnd = lambda x: None if x is None else x.to(dt).to(F64)  # noqa: E731
    ref = LR.evaluate(rnd(c["pos"]), rnd(c["mu"]), rnd(c["quad"]), c["atoms"], c["kinds"], rnd(c["w_mu"]), rnd(c["w_q"]), cell=rnd(c["cells"]), batch_idx=c["batch_idx"])
    fr = LocalFrames(c["atoms"].to(DEV), c["kinds"].to(DEV), batch_idx=bi)
    mu, quad = rotate_multipoles(P, MU, QD, fr, cell, batch_idx=bi)
    assert (mu is None) == (MU is None) and (quad is None) == (QD is None)
    tag = f"frames seed {seed} {c['form']} {c['n']} atoms"
    for name, o in (("dipoles", mu), ("quadrupoles", quad)):
        if o is not None:
            assert o.dtype == dt
            _close(o, ref[name], f"{tag} {name}", rel, key)
    leaves = [None if x is None else x.clone().requires_grad_(True) for x in (P, MU, QD)]
    mu_g, quad_g = rotate_multipoles(*leaves, fr, cell, batch_idx=bi)
    loss = sum((w * o).sum() for w, o in ((WMU, mu_g), (WQ, quad_g)) if o is not None)
    loss.backward()
    for name, leaf in zip(TLF.GRADS, leaves):
        if leaf is not None:
            _close(leaf.grad, ref[name], f"{tag} backward {name}", rel, key)
    periodic = cell is not None
    out = multipole_frame_forces(P, MU, QD, fr, None if MU is None else WMU, None if QD is None else WQ, cell, batch_idx=bi, compute_local_gradients=True,
                                 compute_virial=periodic)
    _close(out[0], -ref["positions_grad"], f"{tag} torque forces", rel, key)
    for name, o in (("local_dipole_grads", out[1]), ("local_quadrupole_grads", out[2])):
        assert (o is None) == (ref[name] is None)
        if o is not None:
            _close(o, ref[name], f"{tag} explicit {name}", rel, key)
    if periodic:
        _close(out[3], ref["virial"], f"{tag} virial term", rel, key)
        if c["empty_system"] is not None:
            assert not bool(out[3][c["empty_system"]].any()), "a system without atoms has an exactly zero virial row"
    print(f"[sweep] {tag} {c['dtype']}: worst error / bar so far {_WORST[key]:.3g}")
