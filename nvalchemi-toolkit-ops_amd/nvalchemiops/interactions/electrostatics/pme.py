"""Particle-mesh Ewald -- drop-in for interactions/electrostatics/pme.py of the reference
(`particle_mesh_ewald` :1673-1994, `pme_reciprocal_space` :1482-1665, `_pme_reciprocal_space_impl` :1338-1479,
`pme_green_structure_factor` :555-676, `pme_energy_corrections[_with_charge_grad]` :1166-1336).

Reciprocal-space pipeline on MI355X:
    spline_spread (HIP atomics)  ->  rfftn (rocFFT via torch.fft, unscaled)  ->  ONE fused HIP pass producing
    conv = spec/sf^2*G and -i k_d conv (4 spectra)  ->  ONE batched irfftn over the 4 channels  ->  ONE fused HIP
    gather of potential + field with self/background corrections and the force factor.
The reference runs 1 forward + 4 separate inverse FFTs, ~10 elementwise torch passes over the spectrum and four
N*order^3-thread atomic gathers for the same result (pme.py:1398-1477).

Spline order: 1-4 match the reference formula for formula.  Orders 5-6 are true cardinal B-splines here with structure-factor
exponent = order; the reference evaluates their weights as zero and caps the exponent at 4 (spline.py:150-193,
pme_kernels.py:213-225).  `nvalchemiops.spline.reference_spline_orders()` switches to the reference's evaluation.
"""
from __future__ import annotations

import functools
import math
import os

import torch

from nvalchemiops import _capi as C
from nvalchemiops.interactions.electrostatics.ewald import _real_space_inputs, _real_space_launch, _with_virial, ewald_real_space
from nvalchemiops.interactions.electrostatics.parameters import (estimate_pme_mesh_dimensions, estimate_pme_parameters,
                                                                 mesh_spacing_to_dimensions)
from nvalchemiops.spline import _launch_spread, spline_gather, spline_gather_vec3, spline_spread

TWOPI = 2.0 * math.pi


@functools.lru_cache(maxsize=64)
def _alpha_constant(value: float, num_systems: int, dtype: torch.dtype, device: torch.device) -> torch.Tensor:
    # a Python-float alpha becomes the same read-only device tensor on every call of an MD loop: no fill kernel per step
    t = torch.full((num_systems,), value, dtype=dtype, device=device)
    if t.is_cuda:
        # the fill is enqueued on the stream that is current NOW, but the cached tensor is handed to every later caller on whatever stream
        # is current THEN, and a caller who passed a Python float has nothing to wait on: the filling stream is waited for once, at
        # creation (as `_solve_tables` does); afterwards the block is read-only and any stream may use it
        torch.cuda.current_stream(t.device).synchronize()
    return t


def _prepare_alpha(alpha: float | torch.Tensor, num_systems: int, dtype: torch.dtype, device: torch.device) -> torch.Tensor:
    """float | 0-d tensor | (B,) tensor -> (B,) tensor (pme.py:191-229)."""
    if isinstance(alpha, (int, float)):
        dev = torch.device(device)
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            # a tensor first created inside a HIP-graph capture lives in that graph's private pool: never cache it for later calls
            return torch.full((num_systems,), float(alpha), dtype=dtype, device=dev)
        return _alpha_constant(float(alpha), int(num_systems), dtype, dev)
    if isinstance(alpha, torch.Tensor):
        if alpha.dim() == 0:
            return alpha.expand(num_systems).to(dtype=dtype, device=device)
        if alpha.shape[0] != num_systems:
            raise ValueError(f"alpha has {alpha.shape[0]} values but there are {num_systems} systems")
        return alpha.to(dtype=dtype, device=device)
    raise TypeError(f"alpha must be float or torch.Tensor, got {type(alpha)}")


def _traceable_alpha(alpha, num_systems: int, dtype, device) -> torch.Tensor:
    """`_prepare_alpha` without the constant cache (an lru_cache'd helper is opaque to TorchDynamo)."""
    if isinstance(alpha, (int, float)):
        return torch.full((num_systems,), float(alpha), dtype=dtype, device=device)
    if isinstance(alpha, torch.Tensor):
        if alpha.dim() == 0:
            return alpha.expand(num_systems).to(dtype=dtype, device=device)
        if alpha.shape[0] != num_systems:
            raise ValueError(f"alpha has {alpha.shape[0]} values but there are {num_systems} systems")
        return alpha.to(dtype=dtype, device=device)
    raise TypeError(f"alpha must be float or torch.Tensor, got {type(alpha)}")


def _prepare_cell(cell: torch.Tensor) -> tuple[torch.Tensor, int]:
    if cell.dim() == 2:
        cell = cell.unsqueeze(0)
    return cell, cell.shape[0]


def _miller_placeholders(device):
    # the reference passes fftfreq index arrays into the op (pme.py:630-640); this build evaluates them in the kernel
    z = torch.empty(0, dtype=torch.float32, device=device)
    return z, z, z


@C.traceable
def pme_green_structure_factor(k_squared: torch.Tensor, mesh_dimensions: tuple[int, int, int], alpha: torch.Tensor, cell: torch.Tensor,
                               spline_order: int = 4, batch_idx: torch.Tensor | None = None):
    """G(k) = 2 pi exp(-k^2/4 alpha^2)/(V k^2) (0 at k = 0) and sf^2 = sinc-product^(2 order) (pme.py:555-676; the reference's exponent
    is 2 min(order, 4): identical for orders 1-4, selected for 5-6 by `nvalchemiops.spline.reference_spline_orders()`).
    Differentiable w.r.t. k_squared, alpha and the cell (through the volume): op `alchemiops::_[batch_]pme_green_structure_factor`."""
    C.require_device(k_squared, cell)
    spline_order = C.resolve_spline_order(spline_order)
    nx, ny, nz = (int(v) for v in mesh_dimensions)
    dt, dev = k_squared.dtype, k_squared.device
    cells = (cell if cell.dim() == 3 else cell.unsqueeze(0)).to(dt)  # the volume below is computed in the dtype of the call, whatever the cell's own
    nsys = cells.shape[0] if batch_idx is not None else 1
    if C.tracing() or (torch.is_grad_enabled() and any(t.requires_grad for t in (k_squared, alpha, cell))):
        from nvalchemiops import _eops  # noqa: F401

        vol_d = torch.abs(torch.linalg.det(cells)).to(dt).reshape(-1)
        mx, my, mz = _miller_placeholders(dev)
        if batch_idx is not None:
            return torch.ops.alchemiops._batch_pme_green_structure_factor(k_squared, mx, my, mz, alpha.to(dt).reshape(-1), vol_d, nx, ny, nz,
                                                                          int(spline_order), nsys)
        return torch.ops.alchemiops._pme_green_structure_factor(k_squared, mx, my, mz, alpha.to(dt).reshape(-1), vol_d[:1], nx, ny, nz, int(spline_order))
    vol = torch.abs(torch.det(cells)).to(dt).reshape(-1).contiguous()
    k2 = k_squared.detach().contiguous()
    al = alpha.detach().to(dt).reshape(-1).contiguous()
    green = torch.empty_like(k2)
    sf2 = torch.empty((nx, ny, nz // 2 + 1), dtype=dt, device=dev)
    # exponent of the sinc product: `order` (the true order-5/6 splines of this build need it), or min(order, 4) as in
    # pme_kernels.py:213-225 under reference_spline_orders() -- identical for every order the reference implements (1-4)
    rc = C.lib().mi_pme_green_sf(C.ptr(k2), C.ptr(al), C.ptr(vol), nsys, nx, ny, nz, C.spline_order_arg(spline_order), C.dtype_code(dt), C.ptr(green),
                                 C.ptr(sf2), C.stream_of(k2))
    C.check(rc, "mi_pme_green_sf")
    return green, sf2


def _total_charge(charges: torch.Tensor, batch_idx, num_systems: int) -> torch.Tensor:
    out = torch.zeros(num_systems, dtype=charges.dtype, device=charges.device)
    rc = C.lib().mi_segment_sum(C.ptr(charges), C.ptr(batch_idx), charges.shape[0], C.dtype_code(charges.dtype), C.ptr(out), C.stream_of(charges))
    C.check(rc, "mi_segment_sum")
    return out


def _corrections(raw, charges, cell, alpha, batch_idx, want_cg):
    C.require_device(raw, charges, cell)
    dt, dev = raw.dtype, raw.device
    cells = (cell if cell.dim() == 3 else cell.unsqueeze(0)).to(dt)  # the volume below is computed in the dtype of the call, whatever the cell's own
    nsys = cells.shape[0] if batch_idx is not None else 1
    if C.tracing() or (torch.is_grad_enabled() and any(t.requires_grad for t in (raw, charges, cell, alpha))):
        from nvalchemiops import _eops  # noqa: F401

        O = torch.ops.alchemiops
        q = charges.to(dt)
        vol_d = torch.abs(torch.linalg.det(cells)).to(dt).reshape(-1)
        al = alpha.to(dt).reshape(-1)
        if batch_idx is None:
            args = (raw, q, vol_d[:1], al[:1], q.sum().reshape(1))
            return O._pme_energy_corrections_with_charge_grad(*args) if want_cg else O._pme_energy_corrections(*args)
        qtot = torch.zeros(nsys, dtype=dt, device=dev).index_add(0, batch_idx.long(), q)
        args = (raw, q, batch_idx, vol_d, al, qtot)
        return O._batch_pme_energy_corrections_with_charge_grad(*args) if want_cg else O._batch_pme_energy_corrections(*args)
    q = charges.detach().to(dt).contiguous()
    bi = None if batch_idx is None else C.i32(batch_idx)
    vol = torch.abs(torch.linalg.det(cells)).to(dt).reshape(-1).contiguous()
    al = alpha.detach().to(dt).reshape(-1).contiguous()
    qtot = _total_charge(q, bi, nsys)
    rawc = raw.detach().contiguous()
    e = torch.empty_like(rawc)
    cg = torch.empty_like(rawc) if want_cg else None
    rc = C.lib().mi_pme_corrections(C.ptr(rawc), C.ptr(q), C.ptr(bi), C.ptr(vol), C.ptr(al), C.ptr(qtot), rawc.shape[0], C.dtype_code(dt),
                                    C.ptr(e), C.ptr(cg), C.stream_of(rawc))
    C.check(rc, "mi_pme_corrections")
    return (e, cg) if want_cg else e


@C.traceable
def pme_energy_corrections(raw_energies, charges, cell, alpha, batch_idx=None) -> torch.Tensor:
    """E_i = q_i phi_i - q_i^2 alpha/sqrt(pi) - q_i pi Q_tot/(2 alpha^2 V) (pme.py:1166-1250, pme_kernels.py:340-409)."""
    return _corrections(raw_energies, charges, cell, alpha, batch_idx, False)


@C.traceable
def pme_energy_corrections_with_charge_grad(raw_energies, charges, cell, alpha, batch_idx=None):
    """... plus dE/dq_i = 2 phi_i - 2 alpha q_i/sqrt(pi) - pi Q_tot/(alpha^2 V) (pme.py:1253-1336)."""
    return _corrections(raw_energies, charges, cell, alpha, batch_idx, True)


class _FftPlan:
    """One hipFFT plan of the library (`mi_fft_plan_create`, csrc/fft.cpp), owned by the plan cache below and destroyed when it leaves it."""

    def __init__(self, dims, batch, code, inverse):
        import ctypes

        self.handle = ctypes.c_void_p()
        self.pinned = False  # executed while a HIP graph was being captured: the graph replays into this plan's work area, so the cache keeps it
        self.shape = (tuple(int(v) for v in dims), int(batch), int(code), bool(inverse))
        C.check(C.lib().mi_fft_plan_create(int(dims[0]), int(dims[1]), int(dims[2]), int(batch), int(code), int(inverse), ctypes.byref(self.handle)),
                "mi_fft_plan_create")

    def __call__(self, src: torch.Tensor, dst: torch.Tensor) -> None:
        # enqueued under the cache's lock: another thread's eviction cannot destroy the plan between look-up and launch; a plan
        # that was evicted after the caller fetched it serves this one call through the dense DFT
        with _FFT_LOCK:
            if not self.handle:
                _DenseDft(*self.shape)(src, dst)
                return
            if src.is_cuda and torch.cuda.is_current_stream_capturing():
                self.pinned = True
            C.check(C.lib().mi_fft_plan_exec(self.handle, C.ptr(src), C.ptr(dst), C.stream_of(src)), "mi_fft_plan_exec")

    def destroy(self) -> None:
        h, self.handle = getattr(self, "handle", None), None
        if h:
            C.lib().mi_fft_plan_destroy(h)  # hipfftDestroy frees the work area (a device-wide wait): only ever on eviction / a failed self-test

    def self_test(self, device, dims, batch, code, inverse):
        """Known-answer test of a NEW plan, once, at creation: the transform of one unit impulse per batch entry against its closed form.
        Round 4 met a hipFFT plan that computed a different transform (60 % off) depending on which other plans were alive.
        Returns (ok, detail): ok = True / False, or None when the check itself could not run -- the cache treats None like False (a plan that
        cannot be vouched for is not used).  Costs two small launches and one host read when a (mesh, batch, dtype, direction, stream) is first seen."""
        import math

        try:
            nx, ny, nz = (int(v) for v in dims)
            rdt = torch.float32 if code == C.dtype_code(torch.float32) else torch.float64
            cdt = torch.complex64 if rdt == torch.float32 else torch.complex128
            nzr = nz // 2 + 1
            # three weighted impulses per batch entry at positions that differ from entry to entry and never sit on an axis plane of the
            # mesh together: a transposed, partially applied or mis-strided transform cannot reproduce their spectrum by accident
            b = torch.arange(batch, device=device)
            kx = torch.arange(nx, device=device, dtype=torch.float64).view(1, nx, 1, 1)
            ky = torch.arange(ny, device=device, dtype=torch.float64).view(1, 1, ny, 1)
            kz = torch.arange(nzr, device=device, dtype=torch.float64).view(1, 1, 1, nzr)
            spectrum = torch.zeros((batch, nx, ny, nzr), dtype=torch.complex128, device=device)
            impulse = torch.zeros((batch, nx, ny, nz), dtype=torch.float64, device=device)
            for w, (ax, bx), (ay, by), (az, bz) in ((1.0, (1, 0), (2, 1), (3, 2)), (-0.5, (3, 1), (1, 0), (5, 1)), (0.25, (5, 2), (7, 3), (1, 0))):
                x0, y0, z0 = (ax * b + bx) % nx, (ay * b + by) % ny, (az * b + bz) % nz
                phase = -2.0 * math.pi * (kx * x0.view(-1, 1, 1, 1) / nx + ky * y0.view(-1, 1, 1, 1) / ny + kz * z0.view(-1, 1, 1, 1) / nz)
                spectrum += w * torch.polar(torch.ones_like(phase), phase)   # rfftn of an impulse, unscaled
                impulse.index_put_((b, x0, y0, z0), torch.full((batch,), w, dtype=torch.float64, device=device), accumulate=True)
            spectrum, impulse = spectrum.to(cdt).contiguous(), impulse.to(rdt)
            if inverse:
                out = torch.empty((batch, nx, ny, nz), dtype=rdt, device=device)
                self(spectrum.clone(), out)
                err = float((out / float(nx * ny * nz) - impulse).abs().max())
            else:
                out = torch.empty((batch, nx, ny, nzr), dtype=cdt, device=device)
                self(impulse.clone(), out)
                err = float((out - spectrum).abs().max())
            ok = err < (1e-3 if rdt == torch.float32 else 1e-9)  # NaN compares False
            return ok, f"max error {err:.3e}"
        except Exception as exc:
            return None, f"{type(exc).__name__}: {exc}"


class _DenseDft:
    """Stand-in for a plan that failed (or could not run) its self-test, with the same (src, dst) call: the library's dense DFT (`mi_dft3d`,
    csrc/dft.hip) -- the transform evaluated from its definition, any mesh size, no plan and no library state.  Slower than an FFT (O(n) per
    output), exact by construction.  Not torch.fft: in the process where the hipFFT plans for (16, 8, 32) failed their self-test, torch.fft
    -- the same rocFFT underneath -- returned a transform 5 % off for the same shape (gpurun r05_s5)."""

    def __init__(self, dims, batch, code, inverse):
        self.dims, self.batch, self.code, self.inverse = tuple(int(v) for v in dims), int(batch), int(code), bool(inverse)

    def __call__(self, src: torch.Tensor, dst: torch.Tensor) -> None:
        nx, ny, nz = self.dims
        C.check(C.lib().mi_dft3d(C.ptr(src), C.ptr(dst), nx, ny, nz, self.batch, self.code, int(self.inverse), C.stream_of(src)), "mi_dft3d")

    def destroy(self) -> None:
        pass


class _LdsFft:
    """The mesh solve's in-LDS kernels as a transform on their own (`mi_fft_lds`, round 6), with the (src, dst) call of a plan: real
    [batch, nx, ny, nz] <-> half spectrum in natural order, unscaled both ways.  No plan object, no library state, no rocFFT: the scratch (one
    half spectrum + the per-shape tables) is a tensor of the call, so it is capturable and there is nothing to evict or self-test.  Serves every
    `_fft_plan` request whose mesh the solve supports (axis lengths 2^a 3^b 5^c, one complex plane within LDS): the backward of the autograd
    node, the composed differentiable path, caller-supplied k arrays."""

    pinned = True  # (nothing to destroy: the cache may hold any number of these)

    def __init__(self, dims, batch, code, inverse):
        self.dims, self.batch, self.code, self.inverse = tuple(int(v) for v in dims), int(batch), int(code), bool(inverse)
        nx, ny, nz = self.dims
        self.nbytes = int(C.lib().mi_fft_lds_scratch_bytes(self.batch, nx, ny, nz, self.code))

    def __call__(self, src: torch.Tensor, dst: torch.Tensor) -> None:
        import ctypes

        nx, ny, nz = self.dims
        scratch = torch.empty(self.nbytes, dtype=torch.uint8, device=src.device)
        C.check(C.lib().mi_fft_lds(C.ptr(src), C.ptr(dst), self.batch, nx, ny, nz, self.code, int(self.inverse), C.ptr(scratch),
                                   ctypes.c_size_t(self.nbytes), C.ptr(_solve_tables(src.device, self.dims, self.code)), C.stream_of(src)), "mi_fft_lds")

    def destroy(self) -> None:
        pass


import collections  # noqa: E402

# LRU of live plans, keyed by (device, mesh, batch, dtype, direction, stream): bounded, so an MD run over varying batch sizes or meshes does
# not pile up dozens of live rocFFT plans (the condition round 4's wrong-transform plan appeared under); a plan that leaves the cache is
# destroyed, and one that comes back is created -- and self-tested -- again.  The stream is part of the key because a plan owns ONE work
# area: two streams running the same shape concurrently must not share it.
import threading  # noqa: E402

_FFT_LOCK = threading.RLock()  # the cache is shared by every thread of the process: look-up, creation (+ self-test) and eviction are one critical section
_FFT_PLANS: "collections.OrderedDict" = collections.OrderedDict()
_FFT_PLAN_CAP = max(2, int(os.environ.get("NVALCHEMIOPS_FFT_PLAN_CACHE", "16")))
_FFT_FALLBACKS: list = []  # (key, detail) of every plan replaced by the dense DFT in this process (tests and bench read it)
# NVALCHEMIOPS_PME_FFT=torch: the round-3 path (torch.fft.rfftn / irfftn: rocFFT behind torch's plan cache, two clones around the C2R) for A/B;
# =dft: every transform of the plan path through the library's dense DFT (no rocFFT at all; the parity tests' cross-check)
_OWN_FFT = os.environ.get("NVALCHEMIOPS_PME_FFT", "own") != "torch"
_FORCE_DFT = os.environ.get("NVALCHEMIOPS_PME_FFT", "own") == "dft"
_FFT_SELFTEST = os.environ.get("NVALCHEMIOPS_FFT_SELFTEST", "1") != "0"
# NVALCHEMIOPS_FFT_LDS=0: plan requests go to hipFFT even where the in-LDS transforms (`mi_fft_lds`) support the mesh (A/B runs, and the tests
# that exercise the guarded hipFFT plans on small meshes)
_FFT_LDS = os.environ.get("NVALCHEMIOPS_FFT_LDS", "1") != "0"
# NVALCHEMIOPS_PME_FUSED_AUTOGRAD=0: energies under autograd through the op-by-op composition as in round 3 (A/B and cross-check of the adjoint)
_FUSED_AUTOGRAD = os.environ.get("NVALCHEMIOPS_PME_FUSED_AUTOGRAD", "1") != "0"
# "auto": the library's measured policy (mi_pme_solve_preferred); True / NVALCHEMIOPS_PME_MESH_SOLVE=1: the fused mesh solve wherever it is
# supported; False / =0: always hipFFT plans + mi_pme_convolve (A/B runs, and the parity tests that drive the solve's batch kernels)
_MESH_SOLVE = {"0": False, "1": True}.get(os.environ.get("NVALCHEMIOPS_PME_MESH_SOLVE", "auto"), "auto")
# NVALCHEMIOPS_PME_SOLVE_AUTOGRAD=1: the autograd node's forward takes the fused mesh solve too, with the charge spectrum its backward needs
# written as a by-product (`mi_pme_solve_keep`).  Default since round 5 (first run on a GPU then: 4 parity tests green, forward under grad
# 0.427 -> 0.418 / 0.582 -> 0.565 ms on the 100k box, profiles/r05_bench_pme_train_*.json); =0 keeps the hipFFT plans in the node's forward.
_SOLVE_AUTOGRAD = os.environ.get("NVALCHEMIOPS_PME_SOLVE_AUTOGRAD", "1") != "0"


_SOLVE_TABLES: "collections.OrderedDict" = collections.OrderedDict()  # (device, mesh, dtype) -> the in-LDS kernels' per-shape tables (a few KB each)


def _solve_tables(device: torch.device, dims, code: int):
    """The per-shape tables of the in-LDS kernels (unit roots, Miller indices, sinc per slot), filled ONCE per (device, mesh, dtype) by
    `mi_fft_lds_tables` into a tensor this module keeps, so that `mi_pme_solve*` / `mi_fft_lds` skip their table launch (~6 us per call).  The
    filling stream is waited for once, at creation: afterwards the block is read-only and any stream may use it.  Returns None -- the call then
    computes its own tables, as before -- while a HIP graph is being captured and the shape has not been seen yet (no host wait inside a capture)."""
    import ctypes

    key = (device.index, tuple(int(v) for v in dims), int(code))
    with _FFT_LOCK:
        t = _SOLVE_TABLES.get(key)
        if t is not None:
            _SOLVE_TABLES.move_to_end(key)
            return t
        if torch.cuda.is_current_stream_capturing():
            return None
        L = C.lib()
        L.mi_fft_lds_tables_bytes.restype = ctypes.c_size_t
        nbytes = int(L.mi_fft_lds_tables_bytes(key[1][0], key[1][1], key[1][2], key[2]))
        if nbytes == 0:
            return None
        t = torch.empty(nbytes, dtype=torch.uint8, device=device)
        stream = torch.cuda.current_stream(device)
        C.check(L.mi_fft_lds_tables(key[1][0], key[1][1], key[1][2], key[2], C.ptr(t), ctypes.c_void_p(stream.cuda_stream)), "mi_fft_lds_tables")
        stream.synchronize()
        _SOLVE_TABLES[key] = t
        while len(_SOLVE_TABLES) > 64:
            _SOLVE_TABLES.popitem(last=False)
        return t


_FFT_VERSION_CHECKED = False


def _check_fft_library_once() -> None:
    """First use of a hipFFT plan: warn when the hipFFT loaded into this process (torch's bundled copy wins the SONAME) is another major
    version than the headers the library was compiled against.  Results are still guarded by the per-plan self-test."""
    global _FFT_VERSION_CHECKED
    if _FFT_VERSION_CHECKED:
        return
    _FFT_VERSION_CHECKED = True
    import ctypes
    import warnings

    try:
        comp, load = ctypes.c_int(0), ctypes.c_int(0)
        if C.lib().mi_fft_library_versions(ctypes.byref(comp), ctypes.byref(load)) == 0 and comp.value // 10000 != load.value // 10000:
            warnings.warn(f"hipFFT {load.value} is loaded but libnvalchemiops_hip.so was compiled against {comp.value}; plans are self-tested, "
                          "a failing one is replaced by the dense DFT")
    except Exception:
        pass


def _fft_plan(device: torch.device, dims, batch: int, code: int, inverse: bool):
    """Plan cache (see `_FFT_PLANS`).  Plans are created outside any HIP-graph capture (creation allocates the work area); a step that is
    captured must have run once eagerly -- as every capture recipe does for its warm-up.  FAIL-SAFE: a new plan that does not reproduce the
    closed-form transform of three impulses -- or whose check cannot run -- is destroyed on the spot and this key is served by the library's
    dense DFT (`mi_dft3d`) from then on (one warning); a wrong plan is never executed on user data."""
    import warnings

    # the in-LDS transforms first: stateless, so nothing is cached and a captured step needs no warm-up for them
    # (`_MESH_SOLVE = False` -- "always hipFFT plans", the A/B setting -- keeps its meaning: no in-LDS kernels anywhere)
    if (_FFT_LDS and _MESH_SOLVE is not False and _OWN_FFT and not _FORCE_DFT and device.type == "cuda"
            and C.lib().mi_fft_lds_supported(int(batch), int(dims[0]), int(dims[1]), int(dims[2]), int(code))):
        return _LdsFft(dims, batch, code, inverse)
    with _FFT_LOCK:
        stream = torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0
        key = (device.index, tuple(int(v) for v in dims), int(batch), int(code), bool(inverse), int(stream))
        plan = _FFT_PLANS.get(key)
        if plan is not None:
            _FFT_PLANS.move_to_end(key)
            return plan
        capturing = device.type == "cuda" and torch.cuda.is_current_stream_capturing()
        if capturing:
            raise RuntimeError("particle_mesh_ewald: run one eager step before capturing it in a HIP graph (FFT plans are created on first use)")
        if _FORCE_DFT:
            plan = _FFT_PLANS[key] = _DenseDft(dims, batch, code, inverse)
            return plan
        _check_fft_library_once()
        plan = _FftPlan(dims, batch, code, inverse)
        if _FFT_SELFTEST:
            ok, detail = plan.self_test(device, dims, batch, code, inverse)
            if not ok:
                plan.destroy()
                plan = _DenseDft(dims, batch, code, inverse)
                _FFT_FALLBACKS.append((key, detail))
                warnings.warn(f"hipFFT plan {tuple(dims)} x {batch} ({'C2R' if inverse else 'R2C'}) " +
                              ("failed its impulse test at creation" if ok is False else "could not be self-tested") +
                              f" ({detail}): destroyed; this shape runs through the library's dense DFT in this process (DESIGN.md 3.7)")
        _FFT_PLANS[key] = plan
        while len(_FFT_PLANS) > _FFT_PLAN_CAP:
            # oldest plan that no captured HIP graph replays into (a graph holds the plan's work area by address: ADVICE r5)
            victim = next((k for k, v in _FFT_PLANS.items() if not getattr(v, "pinned", False) and k != key), None)
            if victim is None:
                break
            _FFT_PLANS.pop(victim).destroy()
        return plan


def _reciprocal_fused(pos, q, cells, alpha, mesh_dimensions, spline_order, bi, compute_forces, compute_charge_gradients, add=(None, None, None),
                      k_vectors=None, k_squared=None, keep=None):
    """The MI355X path: k-space algebra and the gather epilogue fused (k evaluated in registers).  `add` = (float64 energies, forces,
    float64 charge gradients) of the real-space sum, added in the gather epilogue (particle_mesh_ewald's `real + reciprocal`).
    (Running the real-space sum beside the front half on a second stream inside one call was measured in round 4 and dropped: config 4
    0.887 -> 0.871 ms, but the headline step 4.22 - 4.39 -> 4.40 - 4.57 ms and config 5 12.0 -> 12.2: the two halves then compete for the
    same CUs and the outer two-stream schedule already fills them, profiles/r04_ab_pme_fork.log.)"""
    dt, dev = pos.dtype, pos.device
    code = C.dtype_code(dt)
    n = pos.shape[0]
    nx, ny, nz = mesh_dimensions
    batched = bi is not None
    nsys = cells.shape[0] if batched else 1
    spec, real, cit, recip, vol, qtot, al, tile_order = _reciprocal_front(pos, q, cells, alpha, (nx, ny, nz), spline_order, bi, nsys, batched,
                                                                          compute_forces, k_vectors, k_squared, code,
                                                                          need_spec=keep is not None)
    st = C.stream_of(pos)
    energies = torch.empty(n, dtype=dt, device=dev)
    forces = torch.empty((n, 3), dtype=dt, device=dev) if compute_forces else None
    cgrads = torch.empty(n, dtype=dt, device=dev) if compute_charge_gradients else None
    add_e, add_f, add_cg = add
    rc = C.lib().mi_pme_gather_finish(C.ptr(pos), C.ptr(q), C.ptr(bi), C.ptr(cit), C.ptr(real), C.ptr(al), C.ptr(vol), C.ptr(qtot), n, nsys, nx,
                                      ny, nz, C.spline_order_arg(spline_order), int(compute_forces), code, C.ptr(energies), C.ptr(forces), C.ptr(cgrads),
                                      C.ptr(add_e), C.ptr(add_f if compute_forces else None), C.ptr(add_cg if compute_charge_gradients else None),
                                      C.ptr(tile_order), st)
    C.check(rc, "mi_pme_gather_finish")
    if keep is not None:  # what the hand-written adjoint of `_FusedReciprocal` needs: nothing here is recomputed in its backward
        keep.update(spec=spec, real=real, cit=cit, recip=recip, vol=vol, qtot=qtot, alpha=al)
    return energies, forces, cgrads


def _reciprocal_front(pos, q, cells, alpha, dims, spline_order, bi, nsys, batched, compute_forces, k_vectors, k_squared, code, need_spec=True):
    """prepare -> spread -> k-space step -> real meshes, on the current stream.  The k-space step is the library's fused mesh solve
    (`mi_pme_solve`: three kernels with the FFT planes / columns in LDS) for power-of-two meshes when nobody needs the charge spectrum,
    and R2C (hipFFT plan) -> fused k-space pass -> ONE batched C2R otherwise.  Returns
    (spec | None, real meshes [B, 1|4, nx, ny, nz], cell^-T, 2 pi cell^-1, volume, total charge, alpha, tile-grouped atom list | None)."""
    dt, dev = pos.dtype, pos.device
    n = pos.shape[0]
    nx, ny, nz = dims
    st = C.stream_of(pos)
    cc = cells.to(dt).contiguous()
    cit, recip = torch.empty_like(cc), torch.empty_like(cc)
    vol = torch.empty(cc.shape[0], dtype=dt, device=dev)
    qtot = torch.empty(cc.shape[0], dtype=dt, device=dev)
    # cell^-T, 2 pi cell^-1, |det| and the per-system total charge: one launch
    C.check(C.lib().mi_pme_prepare(C.ptr(cc), C.ptr(q), C.ptr(bi), n, cc.shape[0], code, C.ptr(cit), C.ptr(recip), C.ptr(vol), C.ptr(qtot), st),
            "mi_pme_prepare")
    al = alpha.to(dt).contiguous()
    # tile_order: the atoms grouped by mesh tile, a by-product of the tile-owned spread; the gather epilogue walks the atoms in that order
    mesh, tile_order = _launch_spread(pos, q, cit, bi, nsys, (nx, ny, nz), int(spline_order), batched, want_order=True)
    nch = 4 if compute_forces else 1
    cdt = torch.complex64 if dt == torch.float32 else torch.complex128
    if (_MESH_SOLVE and (not need_spec or _SOLVE_AUTOGRAD) and k_squared is None and k_vectors is None
            and (C.lib().mi_pme_solve_supported if _MESH_SOLVE is True else C.lib().mi_pme_solve_preferred)(nsys, nx, ny, nz, code)):
        import ctypes

        nbytes = int(C.lib().mi_pme_solve_scratch_bytes(nsys, nx, ny, nz, nch, code))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        real = torch.empty((nsys, nch, nx, ny, nz), dtype=dt, device=dev)
        # need_spec (the autograd node): the forward column kernel leaves the natural-order charge spectrum as a by-product
        spec = torch.empty((nsys, nx, ny, nz // 2 + 1), dtype=cdt, device=dev) if need_spec else None
        rc = C.lib().mi_pme_solve_tabled(C.ptr(mesh), C.ptr(recip), C.ptr(al), C.ptr(vol), nsys, nx, ny, nz, C.spline_order_arg(spline_order),
                                         int(compute_forces), code, C.ptr(scratch), ctypes.c_size_t(nbytes), C.ptr(real), C.ptr(spec),
                                         C.ptr(_solve_tables(dev, (nx, ny, nz), code)), st)
        C.check(rc, "mi_pme_solve_tabled")
        return spec, real, cit, recip, vol, qtot, al, tile_order
    if _OWN_FFT:
        # the library's own hipFFT plans (mi_fft_plan_*): the spectra and the real meshes are buffers of this call, so the C2R transform may
        # consume its input in place -- torch.fft.irfftn has to clone it first and copies its result once more (2 x 68 MB per headline step)
        spec = torch.empty((nsys, nx, ny, nz // 2 + 1), dtype=cdt, device=dev)
        _fft_plan(dev, (nx, ny, nz), nsys, code, False)(mesh, spec)  # unscaled forward (pme.py:1398)
    else:
        spec = torch.fft.rfftn(mesh, norm="backward", dim=(1, 2, 3))
    conv = torch.empty((nsys, nch, nx, ny, nz // 2 + 1), dtype=cdt, device=dev)
    # caller-supplied k arrays are READ by the same kernel instead of being evaluated in registers (the reference's benchmark protocol
    # passes them precomputed); [nx,ny,nzr(,3)] shared by all systems or with a leading batch dimension
    kv = k2 = None
    if k_squared is not None:
        k2 = k_squared.detach().to(dt).contiguous()
        kv = k_vectors.detach().to(dt).contiguous() if (k_vectors is not None and compute_forces) else None
        # the kernel indexes these through raw pointers: check the layout here (the composed path would fail in torch broadcasting)
        half = (nx, ny, nz // 2 + 1)
        if tuple(k2.shape[-3:]) != half or k2.dim() not in (3, 4) or (k2.dim() == 4 and k2.shape[0] not in (1, nsys)):
            raise ValueError(f"k_squared must have shape {half} or (B, {nx}, {ny}, {nz // 2 + 1}) with B in (1, {nsys}) -- the rfft half grid of "
                             f"generate_k_vectors_pme -- got {tuple(k_squared.shape)}")
        if kv is not None:
            if tuple(kv.shape[-4:]) != half + (3,) or kv.dim() not in (4, 5) or (kv.dim() == 5 and kv.shape[0] not in (1, nsys)):
                raise ValueError(f"k_vectors must have shape {half + (3,)} or (B,) + that with B in (1, {nsys}), got {tuple(k_vectors.shape)}")
            if (kv.dim() == 5 and kv.shape[0] == nsys and nsys > 1) != (k2.dim() == 4 and k2.shape[0] == nsys and nsys > 1):
                raise ValueError("k_vectors and k_squared must both be shared by all systems or both carry the batch dimension")
    k_batched = int(k2 is not None and k2.dim() == 4 and k2.shape[0] == nsys and nsys > 1)
    rc = C.lib().mi_pme_convolve(C.ptr(spec), C.ptr(recip), C.ptr(al), C.ptr(vol), nsys, nx, ny, nz, C.spline_order_arg(spline_order), int(compute_forces), code,
                                 C.ptr(kv), C.ptr(k2), k_batched, C.ptr(conv), st)
    C.check(rc, "mi_pme_convolve")
    if _OWN_FFT:
        real = torch.empty((nsys, nch, nx, ny, nz), dtype=dt, device=dev)
        _fft_plan(dev, (nx, ny, nz), nsys * nch, code, True)(conv, real)  # ONE batched unscaled inverse over all channels (pme.py:1422, 1455-1457)
    else:
        real = torch.fft.irfftn(conv, norm="forward", s=(nx, ny, nz), dim=(2, 3, 4)).contiguous()
    return spec, real, cit, recip, vol, qtot, al, tile_order


def _fusable(compute_forces, compute_charge_gradients, k_vectors, k_squared) -> bool:
    """Can this call run as one fused autograd node?  Energies, explicit forces and (round 5) charge gradients; not caller-supplied k arrays,
    never inside a torch.compile trace (those take the op-by-op composition)."""
    return _FUSED_AUTOGRAD and not C.tracing() and k_vectors is None and k_squared is None


class _FusedReciprocal(torch.autograd.Function):
    """Reciprocal-space PME energies (+ explicit forces) under autograd with the fused forward kernels (round 4).

    Until round 3 anything that required grad left the fused path for the op-by-op composition (`_reciprocal_composed`), 2.7x the inference
    forward.  Here the forward IS the inference path (spread -> R2C -> fused k-space pass -> C2R -> fused gather + corrections) and keeps
    what its adjoint needs -- the charge spectrum, the potential (and field) meshes, the per-atom charge gradients -- and the backward is the
    closed form of what the reference's Warp tape + torch autograd compute for pme.py:1338-1479 (`_reciprocal_adjoint`).

    First order only on this path: when the backward itself is being recorded (`create_graph=True`) it re-runs the differentiable composition
    instead, which supports what it supported before and raises for the rest -- never a silent zero."""

    @staticmethod
    def forward(ctx, positions, charges, cells, alpha, mesh_dimensions, spline_order, batch_idx, compute_forces, compute_charge_gradients=False):
        dt = positions.dtype
        pos = positions.detach().contiguous()
        q = charges.detach().to(dt).contiguous()
        cc = cells.detach().to(dt).contiguous()
        bi = None if batch_idx is None else C.i32(batch_idx)
        keep = {}
        energies, forces, cg = _reciprocal_fused(pos, q, cc, alpha.detach(), mesh_dimensions, spline_order, bi, compute_forces, True, keep=keep)
        # (the saved copy of the charge gradients is the adjoint's own: an output handed to the caller may be modified in place)
        ctx.save_for_backward(positions, charges, cells, alpha, keep["spec"], keep["real"], cg.clone() if compute_charge_gradients else cg, keep["cit"],
                              keep["recip"], keep["vol"], keep["qtot"])
        ctx.dims, ctx.order, ctx.bi, ctx.batch_idx, ctx.with_forces = tuple(mesh_dimensions), int(spline_order), bi, batch_idx, bool(compute_forces)
        ctx.with_cg = bool(compute_charge_gradients)
        ctx.set_materialize_grads(False)
        out = (energies,) + ((forces,) if compute_forces else ()) + ((cg,) if compute_charge_gradients else ())
        return out if len(out) > 1 else out[0]

    @staticmethod
    def backward(ctx, g_energies, *g_rest):
        g_rest = list(g_rest)
        g_forces = g_rest.pop(0) if ctx.with_forces else None
        g_cg = g_rest.pop(0) if ctx.with_cg else None
        positions, charges, cells, alpha = ctx.saved_tensors[:4]
        need = ctx.needs_input_grad
        if torch.is_grad_enabled():
            # the backward is being differentiated (create_graph=True): take it from the differentiable composition
            with torch.enable_grad():
                e, f, c = _reciprocal_composed(positions, charges, cells, alpha, ctx.dims, ctx.order, ctx.batch_idx, ctx.with_forces, ctx.with_cg)
                grads = _composed_grads(((e, g_energies), (f, g_forces), (c, g_cg)), (positions, charges, cells, alpha), need)
            return grads + (None,) * 5
        return _reciprocal_adjoint(ctx.saved_tensors, need, g_energies, g_forces, ctx.dims, ctx.order, ctx.bi, g_cg) + (None,) * 5


def _composed_grads(outputs_and_grads, inputs, need):
    """autograd.grad of the differentiable composition for the inputs that need a gradient (create_graph=True hand-over of the fused nodes)."""
    outs = [o for o, g in outputs_and_grads if o is not None and g is not None]
    gs = [g for o, g in outputs_and_grads if o is not None and g is not None]
    wanted = [t for t, n in zip(inputs, need[:len(inputs)]) if n]
    got = iter(torch.autograd.grad(outs, wanted, gs, create_graph=True, allow_unused=True)) if outs and wanted else iter(())
    return tuple(next(got) if n else None for n in need[:len(inputs)])


def _reciprocal_adjoint(saved, need, g_energies, g_forces, dims, order, bi, g_cgrads=None):
    """(dL/dpositions, dL/dcharges, dL/dcells, dL/dalpha) of L = sum_i g_i E_i + sum_i G_i . F_i + sum_i v_i cg_i for the reciprocal-space outputs,
    from what the fused forward kept.  Raw launches on detached tensors: first order only.  The charge gradient cg_i = 2 phi_i - 2 alpha q_i /
    sqrt(pi) - pi Q / (alpha^2 V) sees the mesh through phi_i only, like E_i = q_i phi_i - ...: its upstream weight joins the energy's,
    w = g q + 2 v, and everything that depends on the mesh (A_E, B, the k-space sums, the position gradient) follows from w unchanged (round 5).
    With that w and u_d = 2 G_d q the upstream weights:

        A_E = spread(w), A_d = spread(u_d);   B = F^H D (A_E_hat + sum_d i k_d A_d_hat)      (one pass: `mi_pme_convolve_bwd`; self-adjoint operator)
        dL/dq   = g (phi - 2 q alpha/sqrt(pi) - pi Q/(2 alpha^2 V)) - pi/(2 alpha^2 V) sum(w) + gather(B) + sum_d 2 G_d gather(E_d)
        dL/dr   = [w grad_u gather(phi) + q grad_u gather(B) + sum_d u_d grad_u gather(E_d)] . cell^-T          (u = fractional coordinates)
        dL/dalpha, dL/dV, dL/d(2 pi cell^-1): the 20 sums of the same pass + the correction terms
        dL/dcell: through cell^-T (fractional coordinates), 2 pi cell^-1 (k vectors) and V = |det cell| in closed form"""
    from nvalchemiops import _eops as E
    from nvalchemiops.spline import _launch_gather

    positions, charges, cells, alpha, spec, real, cg, cit, recip, vol, qtot = saved
    dt, dev = positions.dtype, positions.device
    code = C.dtype_code(dt)
    nx, ny, nz = dims
    batched = bi is not None
    nsys = cit.shape[0] if batched else 1
    pos = positions.detach().contiguous()
    q = charges.detach().to(dt).contiguous()
    al = alpha.detach().to(dt).reshape(-1).contiguous()
    n = pos.shape[0]
    g = None if g_energies is None else g_energies.detach().to(dt).contiguous()
    gf = None if g_forces is None else g_forces.detach().to(dt).contiguous()
    gv = None if g_cgrads is None else g_cgrads.detach().to(dt).contiguous()
    if g is None and gf is None and gv is None:
        return None, None, None, None
    has_w = g is not None or gv is not None
    sel = bi.long() if batched else None
    per = (lambda t: t[sel]) if batched else (lambda t: t[0])  # per-system value at every atom
    st = C.stream_of(pos)
    cdt = torch.complex64 if dt == torch.float32 else torch.complex128
    nchan = 1 if gf is None else 4
    w = g * q if g is not None else torch.zeros(n, dtype=dt, device=dev)
    if gv is not None:
        w = w + 2.0 * gv
    weights = [w] + ([] if gf is None else [(2.0 * gf[:, d] * q).contiguous() for d in range(3)])
    # spectra of the spread upstream weights, channel-major
    a_spec = torch.empty((nchan, nsys, nx, ny, nz // 2 + 1), dtype=cdt, device=dev)
    # ONE batched transform over all channels (round 6): a single 128^3 mesh is 128 planes for 256 CUs -- four of them in one launch fill the chip
    a_mesh = torch.empty((nchan, nsys, nx, ny, nz), dtype=dt, device=dev)
    for c, wt in enumerate(weights):
        _launch_spread(pos, wt, cit, bi, nsys, (nx, ny, nz), order, batched, out=a_mesh[c])
    _fft_plan(dev, (nx, ny, nz), nchan * nsys, code, False)(a_mesh, a_spec)
    nblk = int(C.lib().mi_pme_convolve_bwd_blocks())
    partial = torch.empty((nsys, nblk, 20), dtype=torch.float64, device=dev)
    conv = torch.empty((nsys, 1, nx, ny, nz // 2 + 1), dtype=cdt, device=dev)
    C.check(C.lib().mi_pme_convolve_bwd(C.ptr(spec), C.ptr(a_spec), nchan, C.ptr(recip), C.ptr(al), C.ptr(vol), nsys, nx, ny, nz, C.spline_order_arg(order),
                                        code, C.ptr(conv), C.ptr(partial), st), "mi_pme_convolve_bwd")
    b_mesh = torch.empty((nsys, nx, ny, nz), dtype=dt, device=dev)
    _fft_plan(dev, (nx, ny, nz), nsys, code, True)(conv, b_mesh)
    sqrt_pi = math.sqrt(math.pi)
    a_i, v_i, qt_i = per(al), per(vol), per(qtot)
    phi = real[:, 0]
    field = [real[:, d + 1].contiguous() for d in range(3)] if gf is not None else None
    g_pos = g_q = g_cells = g_alpha = g_cit = None
    if need[1]:
        g_q = _launch_gather(pos, b_mesh, cit, bi, order)
        if has_w:
            wsum = E.seg_sum(w, bi, nsys)  # sum_i (g_i q_i + 2 v_i) per system: the total-charge term of both outputs (dQ/dq_j = 1)
            g_q = g_q - math.pi / (2.0 * a_i * a_i * v_i) * per(wsum)
        if g is not None:
            # phi_j from the forward's charge gradient 2 phi - 2 alpha q/sqrt(pi) - pi Q/(alpha^2 V)
            phi_j = 0.5 * (cg + 2.0 * a_i * q / sqrt_pi + math.pi * qt_i / (a_i * a_i * v_i))
            g_q = g_q + g * (phi_j - 2.0 * q * a_i / sqrt_pi - math.pi * qt_i / (2.0 * a_i * a_i * v_i))
        if gv is not None:
            g_q = g_q - 2.0 * a_i / sqrt_pi * gv
        if gf is not None:
            for d in range(3):
                g_q = g_q + 2.0 * gf[:, d] * _launch_gather(pos, field[d], cit, bi, order)
        g_q = g_q.to(charges.dtype)
    if need[0] or need[2]:
        gfrac = q.unsqueeze(-1) * _launch_gather(pos, b_mesh, cit, bi, order, grad=True)
        if has_w:
            gfrac = gfrac + w.unsqueeze(-1) * _launch_gather(pos, phi.contiguous(), cit, bi, order, grad=True)
        if gf is not None:
            for d in range(3):
                gfrac = gfrac + weights[d + 1].unsqueeze(-1) * _launch_gather(pos, field[d], cit, bi, order, grad=True)
        g_pos, g_cit = E._coordinate_grads(torch.ones_like(q), gfrac, pos, cit, bi)
    sums = partial.sum(1).to(dt) if (need[2] or (need[3] and alpha.dim() > 0)) else None  # [B, 20]
    if need[3] and alpha.dim() > 0:
        g_alpha = sums[:, 1]
        if g is not None:
            g_alpha = g_alpha + E.seg_sum(g * (-q * q / sqrt_pi + q * math.pi * qt_i / (a_i ** 3 * v_i)), bi, nsys)
        if gv is not None:
            g_alpha = g_alpha + E.seg_sum(gv * (-2.0 * q / sqrt_pi + 2.0 * math.pi * qt_i / (a_i ** 3 * v_i)), bi, nsys)
        g_alpha = g_alpha.reshape(alpha.shape).to(alpha.dtype)
    if need[2]:
        g_vol = -sums[:, 0] / vol
        if g is not None:
            g_vol = g_vol + E.seg_sum(g * q * math.pi * qt_i / (2.0 * a_i * a_i * v_i * v_i), bi, nsys)
        if gv is not None:
            g_vol = g_vol + E.seg_sum(gv * math.pi * qt_i / (a_i * a_i * v_i * v_i), bi, nsys)
        inv_t = cit                      # cell^-T;  recip = 2 pi cell^-1
        d_inv = 2.0 * math.pi * (sums[:, 2:11] + sums[:, 11:20]).reshape(nsys, 3, 3) + g_cit.transpose(-1, -2)
        g_cells = -(inv_t @ d_inv @ inv_t) + (g_vol * vol).reshape(-1, 1, 1) * inv_t
        g_cells = g_cells.reshape(cells.shape).to(cells.dtype)
    return (g_pos if need[0] else None), g_q, g_cells, g_alpha


class _FusedPME(torch.autograd.Function):
    """`particle_mesh_ewald` energies (+ explicit forces) under autograd as ONE node: the inference step forward (real-space kernel, then the
    fused reciprocal pipeline whose gather epilogue adds the real-space outputs), `_reciprocal_adjoint` + `mi_ewald_real_bwd` /
    `mi_ewald_real_forces_bwd` backward.  Saves the custom-op dispatches, the four separate inverse FFTs and the torch adds of the two parts
    that the round-3 path paid on every forward."""

    @staticmethod
    def forward(ctx, positions, charges, cells, alpha, mesh_dimensions, spline_order, batch_idx, mask_value, nl, compute_forces,
                compute_charge_gradients=False):
        p = _real_space_inputs(positions, charges, cells, alpha, nl[0], nl[1], nl[2], nl[3], nl[4], batch_idx)
        keep = {}
        add = _real_space_launch(p, mask_value, compute_forces, compute_charge_gradients)
        # the reciprocal charge gradients stay free of the real-space part: the adjoint reads phi back out of them
        energies, forces, cg = _reciprocal_fused(p["pos"], p["q"], p["cells"], p["alpha"], mesh_dimensions, spline_order, p["bi"], compute_forces, True,
                                                 keep=keep, add=(add[0], add[1], None))
        ctx.save_for_backward(positions, charges, cells, alpha, keep["spec"], keep["real"], cg, keep["cit"], keep["recip"], keep["vol"], keep["qtot"],
                              *[t for t in nl if t is not None])
        ctx.nl_present = [t is not None for t in nl]
        ctx.dims, ctx.order, ctx.bi, ctx.batch_idx, ctx.mask_value = tuple(mesh_dimensions), int(spline_order), p["bi"], batch_idx, int(mask_value)
        ctx.with_forces, ctx.with_cg = bool(compute_forces), bool(compute_charge_gradients)
        ctx.set_materialize_grads(False)
        out = (energies,) + ((forces,) if compute_forces else ()) + ((cg + add[2].to(cg.dtype),) if compute_charge_gradients else ())
        return out if len(out) > 1 else out[0]

    @staticmethod
    def backward(ctx, g_energies, *g_rest):
        g_rest = list(g_rest)
        g_forces = g_rest.pop(0) if ctx.with_forces else None
        g_cg = g_rest.pop(0) if ctx.with_cg else None
        saved = ctx.saved_tensors
        positions, charges, cells, alpha = saved[:4]
        rest = iter(saved[11:])
        nl = [next(rest) if present else None for present in ctx.nl_present]
        need = ctx.needs_input_grad
        if torch.is_grad_enabled():  # create_graph=True: the differentiable composition (see _FusedReciprocal.backward)
            with torch.enable_grad():
                real = ewald_real_space(positions=positions, charges=charges, cell=cells, alpha=alpha, neighbor_list=nl[0], neighbor_ptr=nl[1],
                                        neighbor_shifts=nl[2], neighbor_matrix=nl[3], neighbor_matrix_shifts=nl[4], mask_value=ctx.mask_value,
                                        batch_idx=ctx.batch_idx, compute_forces=ctx.with_forces, compute_charge_gradients=ctx.with_cg)
                real = real if isinstance(real, tuple) else (real,)
                e, f, c = _reciprocal_composed(positions, charges, cells, alpha, ctx.dims, ctx.order, ctx.batch_idx, ctx.with_forces, ctx.with_cg)
                e_tot = real[0] + e
                f_tot = real[1] + f if ctx.with_forces else None
                c_tot = real[-1] + c if ctx.with_cg else None
                grads = _composed_grads(((e_tot, g_energies), (f_tot, g_forces), (c_tot, g_cg)), (positions, charges, cells, alpha), need)
            return grads + (None,) * 7
        from nvalchemiops import _eops as E

        out = list(_reciprocal_adjoint(saved[:11], need, g_energies, g_forces, ctx.dims, ctx.order, ctx.bi, g_cg))
        parts = []
        if g_energies is not None:
            parts.append(E._real_bwd(positions, charges, cells, alpha, ctx.batch_idx, nl[0], nl[1], nl[2], nl[3], nl[4], ctx.mask_value, g_energies))
        if g_forces is not None or g_cg is not None:
            parts.append(E._real_forces_bwd(positions, charges, cells, alpha, ctx.batch_idx, nl[0], nl[1], nl[2], nl[3], nl[4], ctx.mask_value, g_forces, g_cg))
        for r_pos, r_q, r_cell, r_alpha in parts:
            for k, r in enumerate((r_pos, r_q, r_cell, r_alpha)):
                if need[k] and out[k] is not None:
                    out[k] = out[k] + r.reshape(out[k].shape).to(out[k].dtype)
        return tuple(out[k] if need[k] else None for k in range(4)) + (None,) * 7


def _reciprocal_composed(positions, charges, cells, alpha, mesh_dimensions, spline_order, batch_idx, compute_forces, compute_charge_gradients,
                         k_vectors=None, k_squared=None):
    """The reference's composition (pme.py:1338-1479) on the `alchemiops::*` custom ops (nvalchemiops/_eops.py): what runs when an input
    requires grad or the call is being traced by torch.compile.  Every step is differentiable -- spread / gather / gather_vec3 by
    hand-written adjoint kernels, Green function and corrections in closed form, FFTs and the spectrum algebra by torch -- so energies
    AND reciprocal forces can be differentiated w.r.t. positions, charges, cell and alpha."""
    from nvalchemiops import _eops  # noqa: F401
    from nvalchemiops.interactions.electrostatics.k_vectors import generate_k_vectors_pme

    O = torch.ops.alchemiops
    dt, dev = positions.dtype, positions.device
    nx, ny, nz = mesh_dimensions
    order = int(spline_order)
    batched = batch_idx is not None
    nsys = cells.shape[0] if batched else 1
    cc = cells.to(dt)
    cell_inv = torch.linalg.inv(cc)
    cit = cell_inv.transpose(-1, -2)
    vol = torch.abs(torch.linalg.det(cc))
    q, al = charges.to(dt), alpha.to(dt).reshape(-1)
    fdims = (1, 2, 3) if batched else (0, 1, 2)
    if batched:
        mesh = O._batch_spline_spread(positions, q, batch_idx, cc, nsys, nx, ny, nz, order, cit)
    else:
        mesh = O._spline_spread(positions, q, cc[0], nx, ny, nz, order, cit[:1])
    # the FFTs go through the library's self-tested plans / dense DFT (`nvalchemiops::mesh_rfftn` / `::mesh_irfftn`, _eops.py), not through
    # torch.fft as in the reference: rocFFT's wrong-transform defect reaches torch.fft as well
    guarded = _OWN_FFT and positions.is_cuda
    rfftn = _eops.mesh_rfftn if guarded else (lambda m: torch.fft.rfftn(m, norm="backward", dim=fdims))
    irfftn = (lambda sp: _eops.mesh_irfftn(sp, nz)) if guarded else (lambda sp: torch.fft.irfftn(sp, norm="forward", s=(nx, ny, nz), dim=fdims))
    spec = rfftn(mesh)  # unscaled forward (pme.py:1398)
    if k_vectors is None or k_squared is None:
        k_vectors, k_squared = generate_k_vectors_pme(cc if batched else cc[0], (nx, ny, nz), reciprocal_cell=TWOPI * (cell_inv if batched else cell_inv[:1]))
    k_squared = k_squared.to(dt)
    mx, my, mz = _miller_placeholders(dev)
    if batched:
        k2 = k_squared if k_squared.dim() == 4 else k_squared.unsqueeze(0).expand(nsys, -1, -1, -1)
        kv = k_vectors if k_vectors.dim() == 5 else k_vectors.unsqueeze(0).expand(nsys, -1, -1, -1, -1)
        green, sf2 = O._batch_pme_green_structure_factor(k2.contiguous(), mx, my, mz, al, vol, nx, ny, nz, order, nsys)
    else:
        k2, kv = k_squared.reshape(nx, ny, nz // 2 + 1), k_vectors.reshape(nx, ny, nz // 2 + 1, 3)
        green, sf2 = O._pme_green_structure_factor(k2.contiguous(), mx, my, mz, al[:1], vol[:1], nx, ny, nz, order)
    conv = spec / sf2 * green                                                                   # pme.py:1418-1419
    phi = irfftn(conv).to(dt)                                                                   # unscaled inverse (pme.py:1422)
    if batched:
        raw = O._batch_spline_gather(positions, phi, batch_idx, cc, order, cit)
        qtot = torch.zeros(nsys, dtype=dt, device=dev).index_add(0, batch_idx.long(), q)
        args = (raw, q, batch_idx, vol, al, qtot)
        corr = O._batch_pme_energy_corrections_with_charge_grad(*args) if compute_charge_gradients else O._batch_pme_energy_corrections(*args)
    else:
        raw = O._spline_gather(positions, phi, cc[0], order, cit[:1])
        args = (raw, q, vol[:1], al[:1], q.sum().reshape(1))
        corr = O._pme_energy_corrections_with_charge_grad(*args) if compute_charge_gradients else O._pme_energy_corrections(*args)
    energies, cgrads = corr if compute_charge_gradients else (corr, None)
    forces = None
    if compute_forces:
        comps = [irfftn(-1j * kv[..., d] * conv) for d in range(3)]
        field = torch.stack(comps, dim=-1).to(dt)
        if batched:
            forces = 2.0 * O._batch_spline_gather_vec3(positions, q, field, batch_idx, cc, order, cit)
        else:
            forces = 2.0 * O._spline_gather_vec3(positions, q, field, cc[0], order, cit[:1])
    return energies, forces, cgrads


@C.traceable
def pme_reciprocal_space(positions: torch.Tensor, charges: torch.Tensor, cell: torch.Tensor, alpha: float | torch.Tensor,
                         mesh_dimensions: tuple[int, int, int] | None = None, mesh_spacing: float | None = None, spline_order: int = 4,
                         batch_idx: torch.Tensor | None = None, k_vectors: torch.Tensor | None = None,
                         k_squared: torch.Tensor | None = None, compute_forces: bool = False, compute_charge_gradients: bool = False):
    """Reciprocal-space PME energies per atom (+ forces, + charge gradients), self and background corrections included.

    Return arity as pme.py:1655-1665."""
    spline_order = C.resolve_spline_order(spline_order)  # the reference-orders switch is read HERE, once: backward passes reuse this value
    cells, num_systems = _prepare_cell(cell)
    n, dev, dt = positions.shape[0], positions.device, positions.dtype
    composed = C.tracing() or (torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (positions, charges, cell, alpha)))
    alpha_t = None if composed else _prepare_alpha(alpha, num_systems, torch.float64, dev)
    if mesh_dimensions is None:
        if mesh_spacing is None:
            raise ValueError("Either mesh_dimensions or mesh_spacing must be provided")
        lengths = torch.norm(cells[0], dim=1)
        mesh_dimensions = tuple(int(torch.ceil(length / mesh_spacing).item()) for length in lengths)  # plain ceil (pme.py:1638-1641)
    mesh_dimensions = tuple(int(v) for v in mesh_dimensions)
    if n == 0:
        energies = torch.zeros(0, device=dev, dtype=dt)
        forces = torch.zeros((0, 3), device=dev, dtype=dt) if compute_forces else None
        cgrads = torch.zeros(0, device=dev, dtype=dt) if compute_charge_gradients else None
    else:
        C.require_device(positions, charges, cell, batch_idx)
        C.dtype_code(dt)
        if composed:
            alpha_g = _traceable_alpha(alpha, num_systems, dt, dev)
            if _fusable(compute_forces, compute_charge_gradients, k_vectors, k_squared):
                # eager autograd: the inference kernels forward, a hand-written adjoint backward (`_FusedReciprocal`)
                out = _FusedReciprocal.apply(positions, charges, cells, alpha_g, mesh_dimensions, spline_order, batch_idx, bool(compute_forces),
                                             bool(compute_charge_gradients))
                out = list(out) if isinstance(out, tuple) else [out]
                energies = out.pop(0)
                forces = out.pop(0) if compute_forces else None
                cgrads = out.pop(0) if compute_charge_gradients else None
            elif C.tracing() and _FUSED_AUTOGRAD and k_vectors is None and k_squared is None and positions.is_cuda:
                # torch.compile: the same node as ONE traceable op (`nvalchemiops::pme_reciprocal_fused`, _eops.py; round 5)
                from nvalchemiops import _eops

                nx, ny, nz = (int(v) for v in mesh_dimensions)
                energies, forces, cgrads = _eops.pme_fused_op(positions, charges, cells, alpha_g, batch_idx, nx, ny, nz, int(spline_order),
                                                              bool(compute_forces))[:3]
                forces = forces if compute_forces else None
                cgrads = cgrads if compute_charge_gradients else None
            else:
                energies, forces, cgrads = _reciprocal_composed(positions, charges, cells, alpha_g, mesh_dimensions, spline_order, batch_idx,
                                                                compute_forces, compute_charge_gradients, k_vectors, k_squared)
        else:
            bi = None if batch_idx is None else C.i32(batch_idx)
            pos = positions.detach().contiguous()
            q = charges.detach().to(dt).contiguous()
            cells_t = cells.detach().to(dt).contiguous()
            args = (pos, q, cells_t, alpha_t, mesh_dimensions, spline_order, bi, compute_forces, compute_charge_gradients)
            have_k = k_vectors is not None and k_squared is not None
            energies, forces, cgrads = _reciprocal_fused(*args, k_vectors=k_vectors if have_k else None, k_squared=k_squared if have_k else None)
    if compute_forces and compute_charge_gradients:
        return energies, forces, cgrads
    if compute_forces:
        return energies, forces
    if compute_charge_gradients:
        return energies, cgrads
    return energies


@C.traceable
def particle_mesh_ewald(positions: torch.Tensor, charges: torch.Tensor, cell: torch.Tensor, alpha: float | torch.Tensor | None = None,
                        mesh_spacing: float | None = None, mesh_dimensions: tuple[int, int, int] | None = None, spline_order: int = 4,
                        batch_idx: torch.Tensor | None = None, k_vectors: torch.Tensor | None = None, k_squared: torch.Tensor | None = None,
                        neighbor_list: torch.Tensor | None = None, neighbor_ptr: torch.Tensor | None = None,
                        neighbor_shifts: torch.Tensor | None = None, neighbor_matrix: torch.Tensor | None = None,
                        neighbor_matrix_shifts: torch.Tensor | None = None, mask_value: int | None = None, compute_forces: bool = False,
                        compute_charge_gradients: bool = False, accuracy: float = 1e-6):
    """Total Coulomb energy per atom = erfc-damped real-space sum over the neighbour list + mesh reciprocal sum
    (+ forces / charge gradients).  Coulomb constant 1.  Same argument handling as pme.py:1917-1994."""
    spline_order = C.resolve_spline_order(spline_order)  # the reference-orders switch is read HERE, once: backward passes reuse this value
    num_atoms = positions.shape[0]
    cells, num_systems = _prepare_cell(cell)
    if alpha is None:
        est = estimate_pme_parameters(positions, cells, batch_idx, accuracy)
        alpha = est.alpha
        if mesh_dimensions is None and mesh_spacing is None:
            mesh_dimensions = tuple(est.mesh_dimensions)
    wants_grad = C.tracing() or (torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (positions, charges, cell, alpha)))
    # a Python-float alpha under eager autograd needs no gradient: the cached constant tensor serves (no fill kernel per call); the
    # uncached form is for traces (an lru_cache'd helper is opaque to TorchDynamo) and for tensors that carry a graph
    plain_alpha = isinstance(alpha, (int, float)) and not C.tracing()
    alpha = (_traceable_alpha if (wants_grad and not plain_alpha) else _prepare_alpha)(alpha, num_systems, positions.dtype, positions.device)
    if mask_value is None:
        mask_value = num_atoms
    if mesh_dimensions is None:
        if mesh_spacing is not None:
            mesh_dimensions = mesh_spacing_to_dimensions(cells, mesh_spacing)
        else:
            mesh_dimensions = estimate_pme_mesh_dimensions(cells, alpha, accuracy)
    if not wants_grad and num_atoms > 0 and (k_vectors is None or k_squared is None):
        # the whole step on HIP kernels + two FFTs, no torch elementwise pass: the real-space sum hands its float64 energies (and
        # forces / charge gradients) to the gather epilogue of the reciprocal part, which adds them (pme.py:1975-1990 adds with torch)
        p = _real_space_inputs(positions, charges, cells, alpha, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                               neighbor_matrix_shifts, batch_idx)
        if p["n_entries"] > 0:
            mesh_dimensions = tuple(int(v) for v in mesh_dimensions)
            add = _real_space_launch(p, mask_value, compute_forces, compute_charge_gradients)
            energies, forces, cgrads = _reciprocal_fused(p["pos"], p["q"], p["cells"], p["alpha"], mesh_dimensions, spline_order, p["bi"],
                                                         compute_forces, compute_charge_gradients, add=add)
            out = (energies,) + ((forces,) if compute_forces else ()) + ((cgrads,) if compute_charge_gradients else ())
            return out if len(out) > 1 else out[0]
    if (wants_grad and num_atoms > 0 and _fusable(compute_forces, compute_charge_gradients, k_vectors, k_squared)
            and ((neighbor_matrix is not None and neighbor_matrix.numel() > 0) or (neighbor_list is not None and neighbor_list.numel() > 0))):
        # eager autograd: ONE node, inference kernels forward, hand-written adjoints backward (`_FusedPME`)
        C.require_device(positions, charges, cell, batch_idx)
        return _FusedPME.apply(positions, charges, cells, alpha, tuple(int(v) for v in mesh_dimensions), spline_order, batch_idx, int(mask_value),
                               (neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix, neighbor_matrix_shifts), bool(compute_forces),
                               bool(compute_charge_gradients))
    real = ewald_real_space(positions=positions, charges=charges, cell=cells, alpha=alpha, neighbor_list=neighbor_list,
                            neighbor_ptr=neighbor_ptr, neighbor_shifts=neighbor_shifts, neighbor_matrix=neighbor_matrix,
                            neighbor_matrix_shifts=neighbor_matrix_shifts, mask_value=mask_value, batch_idx=batch_idx,
                            compute_forces=compute_forces, compute_charge_gradients=compute_charge_gradients)
    recip = pme_reciprocal_space(positions=positions, charges=charges, cell=cells, alpha=alpha, mesh_dimensions=mesh_dimensions,
                                 spline_order=spline_order, batch_idx=batch_idx, compute_forces=compute_forces,
                                 compute_charge_gradients=compute_charge_gradients, k_vectors=k_vectors, k_squared=k_squared)
    if isinstance(real, tuple):
        return tuple(a + b for a, b in zip(real, recip))
    return real + recip


# ---- virial (forward only) -------------------------------------------------------------------------------------------------------------
def _pme_virial(spec, recip, al, vol, qtot, nsys, dims, spline_order, k_vectors=None, k_squared=None) -> torch.Tensor:
    """float64 [nsys, 3, 3] virial of the reciprocal sum from the charge spectrum the k-space step left (`mi_pme_virial`: one pass over the
    half spectrum, block partials folded here), the background term -pi Q^2 / (2 alpha^2 V) * I included by the same kernel (it scales as
    1/V; the self term is strain-free).  k from 2 pi cell^-1, or the caller's k_vectors / k_squared when both are given (as the forward read
    them)."""
    nx, ny, nz = dims
    dt, dev = recip.dtype, recip.device
    kv = k2 = None
    k_batched = 0
    if k_vectors is not None and k_squared is not None:
        half = (nx, ny, nz // 2 + 1)
        k2 = k_squared.detach().to(dt).contiguous()
        kv = k_vectors.detach().to(dt).contiguous()
        if tuple(k2.shape[-3:]) != half or k2.dim() not in (3, 4) or (k2.dim() == 4 and k2.shape[0] not in (1, nsys)):
            raise ValueError(f"k_squared must have shape {half} or (B, {nx}, {ny}, {nz // 2 + 1}) with B in (1, {nsys}) -- the rfft half grid of "
                             f"generate_k_vectors_pme -- got {tuple(k_squared.shape)}")
        if tuple(kv.shape[-4:]) != half + (3,) or kv.dim() not in (4, 5) or (kv.dim() == 5 and kv.shape[0] not in (1, nsys)):
            raise ValueError(f"k_vectors must have shape {half + (3,)} or (B,) + that with B in (1, {nsys}), got {tuple(k_vectors.shape)}")
        k_batched = int(k2.dim() == 4 and k2.shape[0] == nsys and nsys > 1)
        if k_batched != int(kv.dim() == 5 and kv.shape[0] == nsys and nsys > 1):
            raise ValueError("k_vectors and k_squared must both be shared by all systems or both carry the batch dimension")
    part = torch.empty((nsys, int(C.lib().mi_pme_virial_blocks()), 6), dtype=torch.float64, device=dev)
    C.check(C.lib().mi_pme_virial(C.ptr(spec), C.ptr(recip), C.ptr(al), C.ptr(vol), nsys, nx, ny, nz, C.spline_order_arg(spline_order), C.dtype_code(dt),
                                  C.ptr(kv), C.ptr(k2), k_batched, C.ptr(qtot.contiguous()), C.ptr(part), C.stream_of(recip)), "mi_pme_virial")
    return C.fold_virial(part)


def _pme_virial_only(positions, charges, cells, alpha, batch_idx, dims, spline_order, k_vectors=None, k_squared=None) -> torch.Tensor:
    """The reciprocal virial alone, [nsys, 3, 3] in the positions dtype (the `nvalchemiops::pme_reciprocal_space_virial` op): spread and
    k-space step with the charge spectrum kept, no gather."""
    dt, dev = positions.dtype, positions.device
    batched = batch_idx is not None
    cells = cells if cells.dim() == 3 else cells.unsqueeze(0)
    nsys = cells.shape[0] if batched else 1
    if positions.shape[0] == 0:
        return torch.zeros((nsys, 3, 3), dtype=dt, device=dev)
    C.require_device(positions, charges, cells, batch_idx)
    code = C.dtype_code(dt)
    bi = None if batch_idx is None else C.i32(batch_idx)
    al = alpha.to(dt).reshape(-1)
    if al.shape[0] == 1 and cells.shape[0] > 1:
        al = al.expand(cells.shape[0])
    have_k = k_vectors is not None and k_squared is not None
    spec, _, _, recip, vol, qtot, al, _ = _reciprocal_front(positions.contiguous(), charges.to(dt).contiguous(), cells.to(dt).contiguous(), al.contiguous(),
                                                            tuple(int(v) for v in dims), int(spline_order), bi, nsys, batched, False,
                                                            k_vectors if have_k else None, k_squared if have_k else None, code, need_spec=True)
    return _pme_virial(spec, recip, al, vol, qtot, nsys, dims, spline_order, k_vectors if have_k else None, k_squared if have_k else None).to(dt)


@C.traceable
def pme_reciprocal_space_with_virial(positions: torch.Tensor, charges: torch.Tensor, cell: torch.Tensor, alpha: float | torch.Tensor,
                                     mesh_dimensions: tuple[int, int, int] | None = None, mesh_spacing: float | None = None, spline_order: int = 4,
                                     batch_idx: torch.Tensor | None = None, k_vectors: torch.Tensor | None = None,
                                     k_squared: torch.Tensor | None = None, compute_forces: bool = False, compute_charge_gradients: bool = False):
    """`pme_reciprocal_space` plus the virial W_s = -dE_s/d eps (positions and cell rows strained; alpha, mesh and spline order fixed):
    W[a][b] = sum_m E_m (delta_ab - 2 (1/k^2 + 1/(4 alpha^2)) k_a k_b) over the half spectrum (E_m the mode's share of the mesh energy, B-spline
    moduli included) + E_bg delta_ab.  One reduction pass over the charge spectrum the k-space step already holds (fused mesh solve, hipFFT or
    dense DFT), k from the cell or from the caller's k_vectors / k_squared.  Returns the sibling's result with the [num_systems, 3, 3] virial
    (positions dtype) appended; under autograd / torch.compile the other outputs are the sibling's and the virial has no adjoint."""
    spline_order = C.resolve_spline_order(spline_order)
    cells, num_systems = _prepare_cell(cell)
    n, dev, dt = positions.shape[0], positions.device, positions.dtype
    nsys = num_systems if batch_idx is not None else 1
    composed = C.tracing() or (torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (positions, charges, cell, alpha)))
    if mesh_dimensions is None:
        if mesh_spacing is None:
            raise ValueError("Either mesh_dimensions or mesh_spacing must be provided")
        lengths = torch.norm(cells[0], dim=1)
        mesh_dimensions = tuple(int(torch.ceil(length / mesh_spacing).item()) for length in lengths)
    mesh_dimensions = tuple(int(v) for v in mesh_dimensions)
    if n == 0 or composed:
        out = pme_reciprocal_space(positions, charges, cell, alpha, mesh_dimensions=mesh_dimensions, spline_order=spline_order, batch_idx=batch_idx,
                                   k_vectors=k_vectors, k_squared=k_squared, compute_forces=compute_forces,
                                   compute_charge_gradients=compute_charge_gradients)
        if n == 0:
            return _with_virial(out, torch.zeros((nsys, 3, 3), dtype=dt, device=dev))
        from nvalchemiops import _eops

        have_k = k_vectors is not None and k_squared is not None
        vir = _eops.pme_recip_virial_op(positions, charges.to(dt), cells.to(dt), _traceable_alpha(alpha, num_systems, dt, dev), batch_idx, *mesh_dimensions,
                                        int(spline_order), k_vectors if have_k else None, k_squared if have_k else None)
        return _with_virial(out, vir)
    C.require_device(positions, charges, cell, batch_idx)
    C.dtype_code(dt)
    alpha_t = _prepare_alpha(alpha, num_systems, torch.float64, dev)
    bi = None if batch_idx is None else C.i32(batch_idx)
    pos = positions.detach().contiguous()
    q = charges.detach().to(dt).contiguous()
    cells_t = cells.detach().to(dt).contiguous()
    have_k = k_vectors is not None and k_squared is not None
    keep = {}
    energies, forces, cgrads = _reciprocal_fused(pos, q, cells_t, alpha_t, mesh_dimensions, spline_order, bi, compute_forces, compute_charge_gradients,
                                                 k_vectors=k_vectors if have_k else None, k_squared=k_squared if have_k else None, keep=keep)
    virial = _pme_virial(keep["spec"], keep["recip"], keep["alpha"], keep["vol"], keep["qtot"], nsys, mesh_dimensions, spline_order,
                         k_vectors if have_k else None, k_squared if have_k else None)
    out = (energies,) + ((forces,) if compute_forces else ()) + ((cgrads,) if compute_charge_gradients else ())
    return out + (virial.to(dt),)


@C.traceable
def particle_mesh_ewald_with_virial(positions: torch.Tensor, charges: torch.Tensor, cell: torch.Tensor, alpha: float | torch.Tensor | None = None,
                                    mesh_spacing: float | None = None, mesh_dimensions: tuple[int, int, int] | None = None, spline_order: int = 4,
                                    batch_idx: torch.Tensor | None = None, k_vectors: torch.Tensor | None = None, k_squared: torch.Tensor | None = None,
                                    neighbor_list: torch.Tensor | None = None, neighbor_ptr: torch.Tensor | None = None,
                                    neighbor_shifts: torch.Tensor | None = None, neighbor_matrix: torch.Tensor | None = None,
                                    neighbor_matrix_shifts: torch.Tensor | None = None, mask_value: int | None = None, compute_forces: bool = False,
                                    compute_charge_gradients: bool = False, accuracy: float = 1e-6):
    """`particle_mesh_ewald` plus the total electrostatic virial [num_systems, 3, 3] (positions dtype, fp64 sums): the real-space virial from
    the same owner pass as the real-space energies and the reciprocal virial from the charge spectrum of the same k-space step
    (`ewald_real_space_with_virial`, `pme_reciprocal_space_with_virial`).  W_s = -dE_s/d eps with alpha, mesh and order fixed; it adds to
    `dftd3(..., compute_virial=True)`'s virial (same convention).  Returns the sibling's result with the virial appended."""
    spline_order = C.resolve_spline_order(spline_order)
    num_atoms = positions.shape[0]
    cells, num_systems = _prepare_cell(cell)
    nsys = num_systems if batch_idx is not None else 1
    if alpha is None:
        est = estimate_pme_parameters(positions, cells, batch_idx, accuracy)
        alpha = est.alpha
        if mesh_dimensions is None and mesh_spacing is None:
            mesh_dimensions = tuple(est.mesh_dimensions)
    wants_grad = C.tracing() or (torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (positions, charges, cell, alpha)))
    plain_alpha = isinstance(alpha, (int, float)) and not C.tracing()
    alpha_in = alpha
    alpha = (_traceable_alpha if (wants_grad and not plain_alpha) else _prepare_alpha)(alpha, num_systems, positions.dtype, positions.device)
    if mask_value is None:
        mask_value = num_atoms
    if mesh_dimensions is None:
        if mesh_spacing is not None:
            mesh_dimensions = mesh_spacing_to_dimensions(cells, mesh_spacing)
        else:
            mesh_dimensions = estimate_pme_mesh_dimensions(cells, alpha, accuracy)
    mesh_dimensions = tuple(int(v) for v in mesh_dimensions)
    if not wants_grad and num_atoms > 0 and (k_vectors is None or k_squared is None):
        # the sibling's inference step (real-space owner pass -> reciprocal pipeline adding it in the gather epilogue) with the virial flag on
        # the owner pass and the charge spectrum of the k-space step kept for one more reduction
        p = _real_space_inputs(positions, charges, cells, alpha, neighbor_list, neighbor_ptr, neighbor_shifts, neighbor_matrix,
                               neighbor_matrix_shifts, batch_idx)
        if p["n_entries"] > 0:
            add_e, add_f, add_cg, w_real = _real_space_launch(p, mask_value, compute_forces, compute_charge_gradients, virial_systems=nsys)
            keep = {}
            energies, forces, cgrads = _reciprocal_fused(p["pos"], p["q"], p["cells"], p["alpha"], mesh_dimensions, spline_order, p["bi"],
                                                         compute_forces, compute_charge_gradients, add=(add_e, add_f, add_cg), keep=keep)
            w_recip = _pme_virial(keep["spec"], keep["recip"], keep["alpha"], keep["vol"], keep["qtot"], nsys, mesh_dimensions, spline_order)
            out = (energies,) + ((forces,) if compute_forces else ()) + ((cgrads,) if compute_charge_gradients else ())
            return out + ((w_real + w_recip).to(positions.dtype),)
    out = particle_mesh_ewald(positions, charges, cell, alpha=alpha_in, mesh_spacing=mesh_spacing, mesh_dimensions=mesh_dimensions,
                              spline_order=spline_order, batch_idx=batch_idx, k_vectors=k_vectors, k_squared=k_squared, neighbor_list=neighbor_list,
                              neighbor_ptr=neighbor_ptr, neighbor_shifts=neighbor_shifts, neighbor_matrix=neighbor_matrix,
                              neighbor_matrix_shifts=neighbor_matrix_shifts, mask_value=mask_value, compute_forces=compute_forces,
                              compute_charge_gradients=compute_charge_gradients, accuracy=accuracy)
    # the sibling's outputs (autograd node, composition or trace) as they are; the virial beside them from the two forward-only virial ops
    from nvalchemiops import _eops

    dt = positions.dtype
    have_k = k_vectors is not None and k_squared is not None
    w_real = _eops.ewald_real_virial_op(positions, charges.to(dt), cells.to(dt), alpha.to(dt), batch_idx, neighbor_list, neighbor_ptr, neighbor_shifts,
                                        neighbor_matrix, neighbor_matrix_shifts, int(mask_value), nsys)
    w_recip = _eops.pme_recip_virial_op(positions, charges.to(dt), cells.to(dt), alpha.to(dt), batch_idx, *mesh_dimensions, int(spline_order),
                                        k_vectors if have_k else None, k_squared if have_k else None)
    return _with_virial(out, w_real + w_recip)


__all__ = ["particle_mesh_ewald", "pme_reciprocal_space", "pme_green_structure_factor", "pme_energy_corrections",
           "pme_energy_corrections_with_charge_grad", "particle_mesh_ewald_with_virial", "pme_reciprocal_space_with_virial"]
