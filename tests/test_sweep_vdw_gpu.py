"""Seeded sweep, edge case and row ladder of `buffered_14_7` and `lennard_jones` (cases: tests/sweep_cases.py, whose conditions
tests/test_sweep_cases_cpu.py asserts per seed), against tests/vdw_reference.py on the entries actually stored, in both list formats.

What the fixtures of tests/test_vdw_gpu.py do not hold: batches whose systems each have a cell of their own shape (rotated on three seeds,
so that a transposed or a borrowed cell is another lattice), `taper=None`, drawn `delta` / `gamma`, all six rule pairs for both kinds,
each compute flag alone, the virial alone with sites, energies alone, a parent without a site that has children, a child without a site,
`validate=False` with parents out of range, an int64 `parent`, an interleaved `batch_idx`, a system without atoms, float32 scales beside
float64 positions and the reverse, a padding slot between live entries, and entries placed on r^2 == cutoff^2, one float32 ulp inside it,
r == taper and r = 0.

Bars.  float64: 1e-11 of max|ref| + 1e-14.  float32: four times the restatement's own sensitivity to one float32 ulp of every r^2
(`nudge_r2`), measured ON THE CPU FROM THE RESTATEMENT ALONE on these fixtures by `sweep_cases.measured_f32_figures("vdw", kind)` (largest
change relative to max|value|, in the order energies, forces, radius_grads, epsilon_grads, virial; tests/test_sweep_cases_cpu.py repeats
the measurement):
    buffered_14_7   sweep 3.23e-7 3.73e-7 2.78e-7 3.05e-7 3.58e-7   edge 1.35e-6 1.01e-6 8.88e-7 2.53e-6 1.01e-6   rows 3.18e-7 3.66e-7 3.05e-7 3.18e-7 3.64e-7
    lennard_jones   sweep 2.87e-7 3.78e-7 2.59e-7 2.92e-7 3.46e-7   edge 1.53e-6 1.09e-6 9.73e-7 2.55e-6 1.09e-6   rows 2.83e-7 3.35e-7 2.64e-7 2.83e-7 3.31e-7
Everything else is bits: a repeated call, a flag alone against the all-flags call, the interleaved against the sorted call (per atom; the
virial at the float64 bar), `validate=False` against parents of -1, int64 against int32 parents, exact zeros for atoms without a site.

MEASURED on one MI355X: see DESIGN.md section 3.37."""
import numpy as np
import pytest
import torch

from nvalchemiops.interactions import ReducedSites, buffered_14_7, lennard_jones
from tests import sweep_cases as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
FN = dict(buffered_14_7=buffered_14_7, lennard_jones=lennard_jones)
_WORST = {}


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV, dtype=dtype)


def _close(o, ref, what, rel, key):
    got, ref = o.detach().to(F64), ref.detach().to(F64)
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    _WORST[key] = max(_WORST.get(key, 0.0), err / (rel * scale + 1e-14))
    print(f"{what}: max err {err:.3e} of {scale:.3e} ({err / (rel * scale + 1e-14):.3g} bars)")
    assert got.shape == ref.shape and err <= rel * scale + 1e-14, f"{what}: max err {err:.3e} > {rel * scale + 1e-14:.3e}"


def _bars(kind, group, dt):
    return {n: 1e-11 if dt == F64 else 4.0 * f for n, f in zip(W.VDW_NAMES, W.VDW_F32_FIGURE[kind][group])}


def _batch(c):
    return _t(c["batch_idx"]) if c["periodic"] and len(c["sizes"]) > 1 else None


def _sites(c, dt, parent=None, index_dtype=torch.int32, validate=True):
    if c["parent"] is None:
        return None
    return ReducedSites(_t(c["parent"] if parent is None else parent, index_dtype), _t(c["kappa"], dt), batch_idx=_batch(c), validate=validate)


def _lists(c, fmt):
    i, j, S = c["entries"]
    n = len(c["pos"])
    sdt = F32 if c["scale_dtype"] == "float32" else F64
    if fmt == "matrix":
        nm, sh, val = W.padded_matrix(c["entries"], n, c["scales"])
        kw = dict(neighbor_matrix=_t(nm), mask_value=n, **(dict(neighbor_matrix_shifts=_t(sh)) if c["periodic"] else {}))
        scales = val  # NaN on the padding
    else:
        ptr = np.zeros(n + 1, np.int32)
        ptr[1:] = np.cumsum(np.bincount(i, minlength=n))
        kw = dict(neighbor_list=_t(np.stack([i, j]).astype(np.int32)), neighbor_ptr=_t(ptr), **(dict(neighbor_shifts=_t(S.astype(np.int32))) if c["periodic"] else {}))
        scales = c["scales"]
    return dict(kw, pair_scales=None if scales is None else _t(scales, sdt))


def _call(c, kind, fmt, dt, flags, sites=None, leaves=None):
    pos, radii, eps = leaves if leaves is not None else (_t(c[k], dt) for k in ("pos", "radii", "eps"))
    return FN[kind](pos, radii, eps, _t(c["cells"], dt) if c["periodic"] else None, sites=_sites(c, dt) if sites is None else sites, batch_idx=_batch(c),
                    **_lists(c, fmt), **W.vdw_model(c, kind), **flags)


def _named(flags, out):
    out = out if isinstance(out, tuple) else (out,)
    names = ["energies"] + [n for n, f in zip(W.VDW_NAMES[1:], W.VDW_FLAGS) if flags.get(f)]
    assert len(names) == len(out)
    return dict(zip(names, out))


def _every(c):
    return {f: (f != "compute_virial" or c["periodic"]) for f in W.VDW_FLAGS}


def _compare(c, kind, dt, group, what):
    """Every output in both formats against the restatement at the bars of `group`; returns {format: named outputs}."""
    ref, bars, every, out = W.vdw_reference(c, kind, dt, DEV), _bars(kind, group, dt), _every(c), {}
    for fmt in ("matrix", "list"):
        out[fmt] = _named(every, _call(c, kind, fmt, dt, every))
        for name, o in out[fmt].items():
            assert o.dtype == dt
            _close(o, ref[name], f"{what} {kind} {fmt} {name}", bars[name], f"{group} {kind} {'f64' if dt == F64 else 'f32'}")
    return out, ref, bars


@pytest.mark.parametrize("seed", W.SEEDS)
@pytest.mark.parametrize("kind", W.VDW_KINDS)
def test_vdw_sweep(kind, seed):
    c = W.vdw_case("sweep", (kind, seed))
    dt = F64 if c["dtype"] == "float64" else F32
    key = f"sweep {kind} {'f64' if dt == F64 else 'f32'}"
    every, n = _every(c), len(c["pos"])
    full, ref, bars = _compare(c, kind, dt, "sweep", f"seed {seed}")
    for fmt in ("matrix", "list"):
        again = _named(every, _call(c, kind, fmt, dt, every))
        alone = _named(c["flags"], _call(c, kind, fmt, dt, c["flags"]))
        for name, o in full[fmt].items():
            assert torch.equal(o, again[name]), f"seed {seed} {fmt}: two identical calls differ in {name}"
        for name, o in alone.items():  # the seed's own flags (one alone, none, or a drawn set): the bits of the all-flags call
            assert torch.equal(o, full[fmt][name]), f"seed {seed} {fmt} flags {c['flags']}: {name} differs from the all-flags call's"
    out = full["list"]
    head, child = c["no_site"]  # a parent with eps = 0 keeps its children's share of the force; a child with R = 0 has nothing at all
    for name in ("energies", "radius_grads", "epsilon_grads"):
        assert float(out[name][[head, child]].abs().max()) == 0.0, name
    assert float(out["forces"][child].abs().max()) == 0.0 and float(out["forces"][head].abs().max()) > 0.0
    # parents outside [0, N) without validation are parents of -1; an int64 table is the int32 one
    wild = c["parent"].astype(np.int64)
    gone = np.nonzero(wild == -1)[0]
    wild[gone] = np.where(np.arange(len(gone)) % 2 == 0, n + 3, -7)
    for sites, what in ((_sites(c, dt, wild, torch.int64, validate=False), "validate=False"), (_sites(c, dt, index_dtype=torch.int64), "int64 parent")):
        for name, o in _named(every, _call(c, kind, "list", dt, every, sites=sites)).items():
            assert torch.equal(o, out[name]), f"seed {seed} {what}: {name} differs"
    if c["perm"] is not None:  # the interleaved batch: bits of the sorted call atom by atom, the virial at the float64 bar
        ci = W.vdw_interleaved(c)
        perm = _t(c["perm"])
        for name, o in _named(every, _call(ci, kind, "list", dt, every)).items():
            if name == "virial":
                _close(o, out[name], f"seed {seed} interleaved virial against the sorted call", 1e-11, key)
            else:
                assert torch.equal(o, out[name][perm]), f"seed {seed} interleaved: {name} differs from the sorted call's"
    if c["empty_system"] is not None:
        assert out["virial"].shape == (len(c["sizes"]), 3, 3) and not bool(out["virial"][c["empty_system"]].any())
    if c["autograd"]:
        leaves = [_t(c[k], dt).requires_grad_(True) for k in ("pos", "radii", "eps")]
        _call(c, kind, "list", dt, {}, leaves=leaves).sum().backward()
        for name, leaf, sign in zip(W.VDW_NAMES[1:4], leaves, (-1.0, 1.0, 1.0)):
            _close(sign * leaf.grad, ref[name], f"seed {seed} backward {name}", bars[name], key)
    print(f"[sweep] {kind:14s} seed {seed:2d} {c['dtype']} {c['form']} sizes {c['sizes']} rules {c['rules']} taper {c['taper']}: worst error / bar so far {_WORST[key]:.3g}")


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", W.VDW_KINDS)
def test_vdw_entries_on_the_cutoff_the_taper_and_r_zero(kind, dtype):
    c = W.vdw_case("edge")
    out, _, _ = _compare(c, kind, dtype, "edge", "edge")
    for fmt in ("matrix", "list"):
        for name, o in out[fmt].items():
            assert not bool(torch.isnan(o).any()), name
            if name != "virial":  # atoms whose only entry sits at r^2 == cutoff^2: exact zeros
                assert float(o[list(c["at_cutoff"])].abs().max()) == 0.0, f"{fmt} {name}"


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", W.VDW_KINDS)
def test_vdw_rows_across_the_wave_stride_with_sites(kind, dtype):
    c = W.vdw_case("rows")
    out, _, _ = _compare(c, kind, dtype, "rows", "rows")
    for fmt in ("matrix", "list"):
        for name, o in out[fmt].items():
            assert name == "virial" or float(o[0].abs().max()) == 0.0, f"the empty row: {fmt} {name}"
