"""Seeded sweep, edge case and reciprocal ladders of `ewald_dispersion_real_space`, `ewald_dispersion_reciprocal_space` and
`ewald_dispersion_correction` (cases: tests/sweep_cases.py, whose conditions tests/test_sweep_cases_cpu.py asserts per seed), against
tests/dispersion_ewald_reference.py on the entries and k-vectors actually stored, the real half in both list formats.

What the fixtures of tests/test_dispersion_ewald_gpu.py do not hold: batches whose systems each have a cell of their own shape AND
K-VECTORS GENERATED FROM THEIR OWN CELL (there every system repeats one cell and one k set, so a kernel that read system 0's cell,
volume or k-vectors for every system passed), `counted_taper=None`, each compute flag alone and energies alone, a system without atoms in
the middle of a batch, K = 0 in a batch, an interleaved `batch_idx` (real half), a gather block that spans four systems, and entries
placed on a^2 == 1 (the switch between the series and the difference), r^2 == counted_cutoff^2, r == counted_taper and r = 0, and a
caller's k-vector with |k|^2 < 1e-10.

Bars.  float64: 1e-11 of max|ref| + 1e-14.  float32, real half: four times the restatement's own sensitivity to one float32 ulp of every
r^2 (`nudge_r2`), measured ON THE CPU FROM THE RESTATEMENT ALONE on these fixtures by `sweep_cases.measured_f32_figures("dispersion")`
(largest change relative to max|value|, in the order energies, forces, coefficient_grads, virial; tests/test_sweep_cases_cpu.py repeats
the measurement):
    sweep 5.20e-7 1.65e-6 4.27e-7 2.46e-6          edge 3.93e-7 4.29e-7 3.81e-7 3.92e-7
float32, reciprocal half: 1e-6 (phases are float64); the sum of both halves takes the larger of the two.  Everything else is bits.

MEASURED on one MI355X: see DESIGN.md section 3.37."""
import numpy as np
import pytest
import torch

from nvalchemiops import _capi as C
from nvalchemiops.interactions import ewald_dispersion_correction, ewald_dispersion_real_space, ewald_dispersion_reciprocal_space
from tests import sweep_cases as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
EVERY = {f: True for f in W.DE_FLAGS}
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


def _bars(half, group, dt):
    real = [1e-11 if dt == F64 else 4.0 * f for f in W.DE_F32_FIGURE[group]]
    recip = 1e-11 if dt == F64 else 1e-6
    return dict(zip(W.DE_NAMES, {"real": real, "recip": [recip] * 4, "sum": [max(r, recip) for r in real]}[half]))


def _atoms(c, dt, leaves=None):
    pos, coeff = leaves if leaves is not None else (_t(c["pos"], dt), _t(c["c"], dt))
    return pos, coeff, _t(c["cells"], dt), _t(c["alpha"], dt)


def _batch(c):
    return _t(c["batch_idx"]) if len(c["sizes"]) > 1 else None


def _lists(c, fmt):
    i, j, S = c["entries"]
    n = len(c["pos"])
    if fmt == "matrix":
        nm, sh, _ = W.padded_matrix(c["entries"], n)
        kw = dict(neighbor_matrix=_t(nm), neighbor_matrix_shifts=_t(sh), mask_value=n)
    else:
        ptr = np.zeros(n + 1, np.int32)
        ptr[1:] = np.cumsum(np.bincount(i, minlength=n))
        kw = dict(neighbor_list=_t(np.stack([i, j]).astype(np.int32)), neighbor_ptr=_t(ptr), neighbor_shifts=_t(S.astype(np.int32)))
    if c["counted"] is not None:
        kw.update(counted_cutoff=c["counted"][0], counted_taper=c["counted"][1])
    return kw


def _real(c, fmt, dt, flags, leaves=None):
    return ewald_dispersion_real_space(*_atoms(c, dt, leaves), batch_idx=_batch(c), **_lists(c, fmt), **flags)


def _k(c, dt, k_vectors=None):
    return (c["k_vectors"] if k_vectors is None else k_vectors).to(DEV).to(dt)


def _recip(c, dt, flags, leaves=None, k_vectors=None):
    pos, coeff, cell, alpha = _atoms(c, dt, leaves)
    kv = _k(c, dt, k_vectors)
    return ewald_dispersion_reciprocal_space(pos, coeff, cell, kv if kv.shape[1] else None, alpha, batch_idx=_batch(c), **flags)


def _named(flags, out):
    out = out if isinstance(out, tuple) else (out,)
    names = ["energies"] + [n for n, f in zip(W.DE_NAMES[1:], W.DE_FLAGS) if flags.get(f)]
    assert len(names) == len(out)
    return dict(zip(names, out))


def _check(got, ref, bars, dt, what, key):
    for name, o in got.items():
        assert o.dtype == dt
        _close(o, ref[name], f"{what} {name}", bars[name], key)


def _same(a, b, what):
    for name, o in a.items():
        assert torch.equal(o, b[name]), f"{what}: {name} differs"


@pytest.mark.parametrize("seed", W.SEEDS)
def test_dispersion_sweep(seed):
    c = W.dispersion_case("sweep", seed)
    dt = F64 if c["dtype"] == "float64" else F32
    key = "sweep f64" if dt == F64 else "sweep f32"
    gone = _t(np.nonzero(c["c"] == 0)[0])
    # real half, both formats
    ref, bars = W.dispersion_reference(c, "real", dt, DEV), _bars("real", "sweep", dt)
    full = {}
    for fmt in ("matrix", "list"):
        full[fmt] = _named(EVERY, _real(c, fmt, dt, EVERY))
        _check(full[fmt], ref, bars, dt, f"seed {seed} real {fmt}", key + " real")
        _same(_named(EVERY, _real(c, fmt, dt, EVERY)), full[fmt], f"seed {seed} real {fmt}: two identical calls")
        _same(_named(c["flags"], _real(c, fmt, dt, c["flags"])), full[fmt], f"seed {seed} real {fmt} flags {c['flags']} against the all-flags call")
        assert float(full[fmt]["energies"][gone].abs().max()) == 0.0 and float(full[fmt]["forces"][gone].abs().max()) == 0.0, "c = 0: exact zeros"
    if c["perm"] is not None:
        ci = W.dispersion_interleaved(c)
        perm = _t(c["perm"])
        for name, o in _named(EVERY, _real(ci, "list", dt, EVERY)).items():
            if name == "virial":
                _close(o, full["list"][name], f"seed {seed} interleaved virial against the sorted call", 1e-11, key + " real")
            else:
                assert torch.equal(o, full["list"][name][perm]), f"seed {seed} interleaved: {name} differs from the sorted call's"
    if c["empty_system"] is not None:
        assert full["list"]["virial"].shape == (len(c["sizes"]), 3, 3) and not bool(full["list"]["virial"][c["empty_system"]].any())
    # reciprocal half on every system's own k-vectors
    ref_k, bars_k = W.dispersion_reference(c, "recip", dt, DEV), _bars("recip", "sweep", dt)
    rec = _named(EVERY, _recip(c, dt, EVERY))
    _check(rec, ref_k, bars_k, dt, f"seed {seed} reciprocal K={c['k_vectors'].shape[1]}", key + " reciprocal")
    _same(_named(EVERY, _recip(c, dt, EVERY)), rec, f"seed {seed} reciprocal: two identical calls")
    _same(_named(c["flags"], _recip(c, dt, c["flags"])), rec, f"seed {seed} reciprocal flags {c['flags']} against the all-flags call")
    if c["empty_system"] is not None:
        assert not bool(rec["virial"][c["empty_system"]].any())
    # the sum of both halves
    ref_s, bars_s = W.dispersion_reference(c, "sum", dt, DEV), _bars("sum", "sweep", dt)
    both = _named(EVERY, ewald_dispersion_correction(*_atoms(c, dt), k_vectors=_k(c, dt), batch_idx=_batch(c), **_lists(c, "list"), **EVERY))
    _check(both, ref_s, bars_s, dt, f"seed {seed} sum", key + " sum")
    if c["autograd"]:
        for half, fn, r, b in (("real", lambda lv: _real(c, "list", dt, {}, lv), ref, bars), ("reciprocal", lambda lv: _recip(c, dt, {}, lv), ref_k, bars_k)):
            leaves = [_t(c["pos"], dt).requires_grad_(True), _t(c["c"], dt).requires_grad_(True)]
            fn(leaves).sum().backward()
            _close(-leaves[0].grad, r["forces"], f"seed {seed} {half} backward forces", b["forces"], key + " " + half)
            _close(leaves[1].grad, r["coefficient_grads"], f"seed {seed} {half} backward coefficient_grads", b["coefficient_grads"], key + " " + half)
    print(f"[sweep] dispersion seed {seed:2d} {c['dtype']} sizes {c['sizes']} counted {c['counted']} K {c['k_counts']} -> {c['k_vectors'].shape[1]}: worst error / bar "
          + ", ".join(f"{h} {_WORST.get(key + ' ' + h, 0.0):.3g}" for h in ("real", "reciprocal", "sum")))


@pytest.mark.parametrize("fmt", ["matrix", "list"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_dispersion_entries_on_the_series_switch_the_counted_edges_and_r_zero(dtype, fmt):
    c = W.dispersion_case("edge")
    got = _named(EVERY, _real(c, fmt, dtype, EVERY))
    _check(got, W.dispersion_reference(c, "real", dtype, DEV), _bars("real", "edge", dtype), dtype, f"edge {fmt}", "edge real")
    assert not any(bool(torch.isnan(o).any()) for o in got.values())
    assert float(got["energies"][6].abs()) == 0.0 and float(got["forces"][6].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_a_k_vector_below_the_threshold_weighs_nothing(dtype):
    c = W.dispersion_case("edge")
    plain = _named(EVERY, _recip(c, dtype, EVERY))
    _check(plain, W.dispersion_reference(c, "recip", dtype, DEV), _bars("recip", "edge", dtype), dtype, "edge reciprocal", "edge reciprocal")
    tiny = _named(EVERY, _recip(c, dtype, EVERY, k_vectors=c["k_tiny"]))
    _check(tiny, W.dispersion_reference(dict(c, k_vectors=c["k_tiny"]), "recip", dtype, DEV), _bars("recip", "edge", dtype), dtype, "edge reciprocal, tiny k", "edge reciprocal")
    _same(tiny, plain, "the set with |k|^2 = 1e-12 appended against the set without it")


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_reciprocal_ladders_on_systems_with_their_own_cells(dtype):
    L = C.lib()
    assert W.DE_TILES == {"atom": int(L.mi_ewald_dispersion_atom_tile()), "k": int(L.mi_ewald_dispersion_k_tile())}
    for sizes, n_k in W.dispersion_recip_rungs():
        c = W.dispersion_case("recip", (sizes, n_k))
        got = _named(EVERY, _recip(c, dtype, EVERY))
        _check(got, W.dispersion_reference(c, "recip", dtype, DEV), _bars("recip", "sweep", dtype), dtype, f"reciprocal N={sizes} K={n_k}", "ladder")
        if c["empty_system"] is not None:
            assert got["virial"].shape == (len(sizes), 3, 3) and not bool(got["virial"][c["empty_system"]].any())
    print(f"[sweep] dispersion reciprocal ladders: worst error / bar {_WORST['ladder']:.3g}")
