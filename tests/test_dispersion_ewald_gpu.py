"""`ewald_dispersion_*` on the device against the float64 restatement of their definition (tests/dispersion_ewald_reference.py, itself pinned in
tests/test_dispersion_ewald_reference_cpu.py) on the same stored entries and k-vectors.

float64: kernel and reference share the arithmetic model: 1e-11 of the largest |value| per output plus 1e-14.

float32, real space: pair vector and r^2 in float32, the rest float64, against the reference's `distance_dtype=float32` mode at the float32-rounded
inputs.  As in 3.35 the bar is four times the reference's own sensitivity to one ulp of every float32 r^2 (`nudge_r2`), measured on the CPU
on the fixtures below, largest change relative to the largest |value| of the output, in the order of NAMES:
    plain     2.93e-7  2.93e-7  2.82e-7  3.55e-7          counted   4.82e-7  1.66e-6  4.41e-7  4.91e-7
(the counted part is a small remainder of the same pair terms, so one ulp of r^2 weighs more in it)
float32, reciprocal space: the phases are float64, so against the reference at the float32-rounded inputs at 1e-6, the bar of
tests/test_dipole_gpu.py for its reciprocal half; the sum of both halves takes the larger of the two bars."""
import functools

import pytest
import torch

from nvalchemiops import _capi as C
from nvalchemiops.interactions import ewald_dispersion_correction, ewald_dispersion_real_space, ewald_dispersion_reciprocal_space
from nvalchemiops.interactions.electrostatics.k_vectors import generate_k_vectors_ewald_summation
from tests import dispersion_ewald_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
NAMES = ("energies", "forces", "coefficient_grads", "virial")
ALL = dict(compute_forces=True, compute_coefficient_gradients=True, compute_virial=True)
F32_FIGURE = {None: (2.93e-7, 2.93e-7, 2.82e-7, 3.55e-7), (4.0, 3.6): (4.82e-7, 1.66e-6, 4.41e-7, 4.91e-7)}
CELL = torch.tensor([[9.0, 0, 0], [1.8, 8.1, 0], [0.9, -1.35, 9.9]], dtype=F64)  # the triclinic 9 A box of tests/test_vdw_gpu.py


def _close(got, ref, what, rel):
    got, ref = got.detach().to(F64), ref.detach().to(F64)
    scale, err = float(ref.abs().max()), float((got - ref).abs().max())
    print(f"{what}: max err {err:.3e} of {scale:.3e} ({err / max(scale, 1e-300):.2e}, bar {rel:.1e})")
    assert err <= rel * scale + 1e-14, f"{what}: max err {err:.3e} > {rel * scale + 1e-14:.3e}"


def _box(seed, list_cutoff):
    """60 atoms on a jittered 4 x 4 x 4 fractional grid of the box (tests/test_vdw_gpu.py), atom 7 with c = 0, and their full list by brute force."""
    g = torch.Generator().manual_seed(seed)
    k = torch.arange(60)
    frac = (torch.stack([k % 4, (k // 4) % 4, k // 16], 1) + 0.5 + 0.16 * (torch.rand(60, 3, generator=g, dtype=F64) - 0.5)) / 4.0
    c = 2.0 + 3.0 * torch.rand(60, generator=g, dtype=F64)
    c[7] = 0.0
    pos = frac @ CELL
    return pos, c, R.entries_within(pos, CELL, list_cutoff)


@functools.lru_cache(maxsize=None)
def real_fixture(batched):
    """One box listed to 7.6 A (rows above 128 entries), or a batch of two listed to 4.5 A (below 64) and 6.2 A (64 to 128) with their own
    alpha; as a matrix with three padding columns (one index out of range) and as CSR.  CPU tensors."""
    boxes = [_box(11, 4.5), _box(12, 6.2)] if batched else [_box(13, 7.6)]
    pos, c = torch.cat([b[0] for b in boxes]), torch.cat([b[1] for b in boxes])
    i, j, S = (torch.cat([b[2][w] + (60 * s if w < 2 else 0) for s, b in enumerate(boxes)]) for w in range(3))
    order = torch.argsort(i, stable=True)
    i, j, S = i[order], j[order], S[order]
    n = pos.shape[0]
    counts = torch.bincount(i, minlength=n)
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(counts, 0)])
    spans = [(int(counts[60 * s:60 * s + 60].min()), int(counts[60 * s:60 * s + 60].max())) for s in range(len(boxes))]
    assert (spans[0][1] < 64 and 64 <= spans[1][0] and spans[1][1] <= 128) if batched else spans[0][0] > 128, spans
    width = int(counts.max()) + 3
    cols = torch.tensor([w for w in range(width) if w not in (0, width // 2, width - 1)])
    nm, sh = torch.full((n, width), -1), torch.zeros((n, width, 3), dtype=torch.long)
    slot = cols[torch.arange(len(i)) - ptr[i]]
    nm[i, slot], sh[i, slot] = j, S
    nm[:, width // 2] = n + 5
    return dict(pos=pos, c=c, cell=CELL.repeat(len(boxes), 1, 1), alpha=torch.tensor([0.3, 0.4][:len(boxes)], dtype=F64), entries=(i, j, S), nm=nm,
                sh=sh, nl=torch.stack([i, j]), ptr=ptr, bi=torch.arange(len(boxes)).repeat_interleave(60) if batched else None)


def _lists(f, fmt):
    d = lambda t: t.to(DEV).int()  # noqa: E731
    if fmt == "matrix":
        return dict(neighbor_matrix=d(f["nm"]), neighbor_matrix_shifts=d(f["sh"]), mask_value=-1)
    return dict(neighbor_list=d(f["nl"]), neighbor_ptr=d(f["ptr"]), neighbor_shifts=d(f["entries"][2]))


def _rounded(f, dtype):
    """The fixture's float inputs on the device in `dtype`, and what the reference takes: the same values."""
    return {k: f[k].to(DEV).to(dtype) for k in ("pos", "c", "cell", "alpha")}, None if f["bi"] is None else f["bi"].to(DEV).int()


@pytest.mark.parametrize("fmt", ["matrix", "csr"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_real_space_and_the_sum_of_both_halves(dtype, fmt):
    for batched in (False, True):
        f = real_fixture(batched)
        x, bi = _rounded(f, dtype)
        entries = tuple(t.to(DEV) for t in f["entries"])
        r2 = ((f["pos"][f["entries"][1]] - f["pos"][f["entries"][0]] + f["entries"][2].to(F64) @ CELL) ** 2).sum(-1)
        assert bool((r2 * 0.3 ** 2 < R.SERIES_BELOW).any()) and bool(((r2 > 3.6 ** 2) & (r2 < 4.0 ** 2)).any())  # series branch, taper window
        for counted in (None, (4.0, 3.6)):
            kw = dict(batch_idx=bi, **_lists(f, fmt), **({} if counted is None else dict(counted_cutoff=counted[0], counted_taper=counted[1])))
            got = ewald_dispersion_real_space(x["pos"], x["c"], x["cell"], x["alpha"], **ALL, **kw)
            ref = R.evaluate(x["pos"], x["c"], x["cell"], x["alpha"], entries, batch_idx=bi, counted=counted, distance_dtype=dtype)
            for name, o, figure in zip(NAMES, got, F32_FIGURE[counted]):
                assert o.dtype == dtype
                _close(o, ref[name], f"real batched={batched} counted={counted} {fmt} {name}", 1e-11 if dtype == F64 else 4 * figure)
            assert float(got[0][7].abs()) == 0.0 and float(got[1][7].abs().max()) == 0.0  # c = 0: exact zeros
            again = ewald_dispersion_real_space(x["pos"], x["c"], x["cell"], x["alpha"], **ALL, **kw)
            assert all(torch.equal(a, b) for a, b in zip(got, again)), "two identical calls differ"
        kv = generate_k_vectors_ewald_summation(x["cell"], 2.2)
        got = ewald_dispersion_correction(x["pos"], x["c"], x["cell"], x["alpha"], k_vectors=kv, **ALL, **kw)
        ref = R.evaluate(x["pos"], x["c"], x["cell"], x["alpha"], entries, kv, batch_idx=bi, counted=counted, distance_dtype=dtype)
        for name, o, figure in zip(NAMES, got, F32_FIGURE[counted]):
            _close(o, ref[name], f"sum batched={batched} {fmt} {name}", 1e-11 if dtype == F64 else max(4 * figure, 1e-6))


@functools.lru_cache(maxsize=None)
def recip_fixture(sizes, n_k):
    """Systems of `sizes` atoms at random places of the box, the first n_k vectors of its half-space set, alpha 1.1, 1.3, ... (f(b) of order one)."""
    g = torch.Generator().manual_seed(sum(sizes) + n_k)
    n, nsys = sum(sizes), len(sizes)
    kv = generate_k_vectors_ewald_summation(CELL, 4.6)[:n_k]
    assert kv.shape[0] == n_k
    return dict(pos=torch.rand(n, 3, generator=g, dtype=F64) @ CELL, c=1.0 + torch.rand(n, generator=g, dtype=F64), cell=CELL.repeat(nsys, 1, 1),
                alpha=1.1 + 0.2 * torch.arange(nsys, dtype=F64), kv=kv if nsys == 1 else kv.repeat(nsys, 1, 1),
                bi=torch.arange(nsys).repeat_interleave(torch.tensor(sizes)) if nsys > 1 else None)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_reciprocal_space_around_the_tile_edges(dtype):
    L = C.lib()
    ta, tk = int(L.mi_ewald_dispersion_atom_tile()), int(L.mi_ewald_dispersion_k_tile())
    cases = [((n,), tk + 1) for n in (1, ta - 1, ta, ta + 1, 2 * ta + 3)] + [((ta + 1,), k) for k in (0, 1, tk - 1, tk, 2 * tk + 3)]
    cases.append(((ta - 56, ta // 2 - 28, 7), tk + 1))  # three unequal systems, the second across an atom-tile edge, alpha per system
    for sizes, n_k in cases:
        f = recip_fixture(sizes, n_k)
        x, bi = _rounded(f, dtype)
        kv = f["kv"].to(DEV).to(dtype)
        got = ewald_dispersion_reciprocal_space(x["pos"], x["c"], x["cell"], None if n_k == 0 else kv, x["alpha"], batch_idx=bi, **ALL)
        ref = R.evaluate(x["pos"], x["c"], x["cell"], x["alpha"], None, kv, batch_idx=bi)
        for name, o in zip(NAMES, got):
            assert o.dtype == dtype
            _close(o, ref[name], f"reciprocal N={sizes} K={n_k} {name}", 1e-11 if dtype == F64 else 1e-6)
    again = ewald_dispersion_reciprocal_space(x["pos"], x["c"], x["cell"], kv, x["alpha"], batch_idx=bi, **ALL)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), "two identical calls differ"


def test_autograd_and_compile_match_the_explicit_outputs():
    f = real_fixture(True)
    x, bi = _rounded(f, F64)
    kv = generate_k_vectors_ewald_summation(x["cell"], 2.2)
    real = functools.partial(ewald_dispersion_real_space, batch_idx=bi, counted_cutoff=4.0, counted_taper=3.6, **_lists(f, "csr"))
    halves = {"real": lambda p, c, **kw: real(p, c, x["cell"], x["alpha"], **kw),
              "reciprocal": lambda p, c, **kw: ewald_dispersion_reciprocal_space(p, c, x["cell"], kv, x["alpha"], batch_idx=bi, **kw)}
    for half, fn in halves.items():
        p, c = x["pos"].clone().requires_grad_(True), x["c"].clone().requires_grad_(True)
        _, frc, cg = fn(x["pos"], x["c"], compute_forces=True, compute_coefficient_gradients=True)
        loss = lambda a, b: fn(a, b).sum()  # noqa: E731
        for run in (loss, torch.compile(loss, mode="default", fullgraph=True)):
            p.grad = c.grad = None
            run(p, c).backward()
            _close(-p.grad, frc, f"{half} autograd forces", 1e-11)
            _close(c.grad, cg, f"{half} autograd coefficient_grads", 1e-11)
