"""The multi-channel spline entry points, the multipole basis functions and their ops, checked without a GPU: declared and exported
symbols, argument validation before any device call, the `nvalchemiops.math` surface, op registration, and the trace count -- a function
that spreads 9 channels, scales the mesh and gathers back is ONE graph with ONE spread-channels op and ONE gather-channels op (the
per-channel loops of before traced to nine scalar spreads and nine scalar gathers)."""
import ctypes

import pytest
import torch
from torch._dynamo.backends.common import aot_autograd

from nvalchemiops import _capi as C
from nvalchemiops._capi import NativeLibraryError
from tools.abi_symbols import declared_symbols

SPLINE = ("mi_spline_spread_channels", "mi_spline_spread_channels_workspace_bytes_for", "mi_spline_gather_channels",
          "mi_spline_gather_channels_frac_grad")
MATH = ("mi_sph_harm", "mi_sph_harm_grad", "mi_gto_density", "mi_gto_fourier")
MI_OK, MI_EINVAL = 0, -1  # include/nvalchemiops_hip.h


def _err():
    return C.lib().mi_last_error().decode()


def test_new_entry_points_declared_and_exported():
    declared = declared_symbols()
    lib = C.lib()
    for name in SPLINE + MATH:
        assert name in declared, f"{name} is not declared in include/nvalchemiops_hip.h"
        assert hasattr(lib, name), f"libnvalchemiops_hip.so does not export {name}"


# a non-null host address: validation must reject the call before anything dereferences it or touches the device
_BUF = (ctypes.c_double * 64)()
P = ctypes.cast(_BUF, ctypes.c_void_p)


def _spread(n=4, nsys=1, nch=3, dims=(8, 8, 8), order=4, dtype=C.MI_F64, pos=P, vals=P, cit=P, mesh=P):
    return C.lib().mi_spline_spread_channels(pos, vals, None, cit, n, nsys, nch, *dims, order, 0, dtype, mesh, None, ctypes.c_size_t(0), None)


def _gather(n=4, nsys=1, nch=3, dims=(8, 8, 8), order=4, dtype=C.MI_F64, pos=P, mesh=P, cit=P, out=P):
    return C.lib().mi_spline_gather_channels(pos, mesh, None, cit, n, nsys, nch, *dims, order, dtype, out, None)


def _frac(n=4, nsys=1, nch=3, dims=(8, 8, 8), order=4, dtype=C.MI_F64, pos=P, mesh=P, coef=P, cit=P, out=P):
    return C.lib().mi_spline_gather_channels_frac_grad(pos, mesh, coef, None, cit, n, nsys, nch, *dims, order, dtype, out, None)


@pytest.mark.parametrize("call", [_spread, _gather, _frac])
def test_spline_channel_entry_points_validate_before_any_device_call(call):
    for bad, fragment in ((dict(nch=0), "n_channels"), (dict(nch=-2), "n_channels"), (dict(order=7), "spline order"), (dict(order=0), "spline order"),
                          (dict(dtype=5), "dtype"), (dict(pos=None), "null pointer"), (dict(cit=None), "null pointer"),
                          (dict(dims=(8, 0, 8)), "mesh dimensions")):
        assert call(**bad) == MI_EINVAL, bad
        assert fragment in _err(), (bad, _err())
    assert call(mesh=None) == MI_EINVAL and "null pointer" in _err()
    # nothing to do: MI_OK without looking at the pointers
    assert call(n=0, pos=None, cit=None, mesh=None) == MI_OK
    assert _frac(coef=None) == MI_EINVAL and "null pointer" in _err()
    assert _spread(vals=None) == MI_EINVAL and "null pointer" in _err()
    assert _gather(out=None) == MI_EINVAL and "null pointer" in _err()


def test_spread_channels_workspace_size():
    ws = C.lib().mi_spline_spread_channels_workspace_bytes_for
    one = C.lib().mi_spline_spread_workspace_bytes_for
    args = (1000, 1, 32, 32, 32)
    # one channel: the scalar pipeline's size; nine fp64 channels at order 5 run as three blocks of three, so the box scratch -- the only part
    # that grows -- is three boxes per tile, not nine
    assert ws(*args, 5, 1, C.MI_F64) == one(*args, 5, C.MI_F64)
    base = one(*args, 5, C.MI_F64)
    boxes = 8 * 64 * 12 ** 3  # 64 tiles of 8^3, (8 + 4)^3 points each
    assert ws(*args, 5, 9, C.MI_F64) == base + 2 * boxes
    assert ws(*args, 5, 0, C.MI_F64) == 0 and ws(*args, 7, 9, C.MI_F64) == 0 and ws(*args, 5, 9, 7) == 0
    assert ws(1000, 1, 31, 9, 6, 4, 9, C.MI_F64) == 256  # a mesh that does not tile: the atomic kernel needs no scratch
    assert ws(*args, 5 | C.SPLINE_REFERENCE_ORDERS, 9, C.MI_F64) == 256


def test_math_entry_points_validate_before_any_device_call():
    lib = C.lib()
    for l_max in (-1, 3):
        assert lib.mi_sph_harm(P, 4, l_max, P, None) == MI_EINVAL and "L_max" in _err()
        assert lib.mi_sph_harm_grad(P, 4, l_max, P, None) == MI_EINVAL and "L_max" in _err()
        assert lib.mi_gto_density(P, 4, 1.0, l_max, P, None) == MI_EINVAL and "L_max" in _err()
        assert lib.mi_gto_fourier(P, 4, 1.0, l_max, P, P, None) == MI_EINVAL and "L_max" in _err()
    assert lib.mi_gto_density(P, 4, 0.0, 2, P, None) == MI_EINVAL and "sigma" in _err()
    assert lib.mi_gto_fourier(P, 4, -1.0, 2, P, P, None) == MI_EINVAL and "sigma" in _err()
    assert lib.mi_sph_harm(None, 4, 2, P, None) == MI_EINVAL and "null pointer" in _err()
    assert lib.mi_sph_harm_grad(P, 4, 2, None, None) == MI_EINVAL and "null pointer" in _err()
    assert lib.mi_gto_density(P, 4, 1.0, 2, None, None) == MI_EINVAL and "null pointer" in _err()
    assert lib.mi_gto_fourier(P, 4, 1.0, 2, P, None, None) == MI_EINVAL and "null pointer" in _err()
    for rc in (lib.mi_sph_harm(None, 0, 2, None, None), lib.mi_sph_harm_grad(None, 0, 2, None, None), lib.mi_gto_density(None, 0, 1.0, 2, None, None),
               lib.mi_gto_fourier(None, 0, 1.0, 2, None, None, None)):
        assert rc == MI_OK


def test_math_package_surface():
    import nvalchemiops.math as M

    for name in ("eval_spherical_harmonics_pytorch", "eval_spherical_harmonics_gradient_pytorch", "eval_gto_density_pytorch",
                 "eval_gto_fourier_pytorch"):
        assert callable(getattr(M, name)) and name in M.__all__
    pos = torch.zeros(3, 3, dtype=torch.float64)
    # an unsupported L_max is the reference's dict lookup failing; a CPU tensor is refused, there is no CPU path
    for fn, args in ((M.eval_spherical_harmonics_pytorch, ()), (M.eval_spherical_harmonics_gradient_pytorch, ()), (M.eval_gto_density_pytorch, (1.0,)),
                     (M.eval_gto_fourier_pytorch, (1.0,))):
        with pytest.raises(KeyError):
            fn(pos, *args, L_max=3)
        with pytest.raises(NativeLibraryError, match="ROCm devices only"):
            fn(pos, *args, L_max=2)


def test_channel_ops_registered():
    from nvalchemiops import _eops  # noqa: F401

    for name in ("_spline_spread_channels", "_spline_gather_channels", "_batch_spline_spread_channels", "_batch_spline_gather_channels"):
        assert hasattr(torch.ops.alchemiops, name), name
    assert hasattr(torch.ops.nvalchemiops, "spline_gather_channels_frac_grad")
    # fake implementations carry the true shapes and dtype
    pos, cell = torch.zeros(5, 3, device="meta"), torch.eye(3, device="meta")
    vals = torch.zeros(5, 9, device="meta")
    mesh = torch.ops.alchemiops._spline_spread_channels(pos, vals, cell, 9, 8, 10, 12, 4)
    assert mesh.shape == (9, 8, 10, 12) and mesh.dtype == torch.float32
    assert torch.ops.alchemiops._spline_gather_channels(pos, mesh, cell, 4).shape == (5, 9)
    bi = torch.zeros(5, dtype=torch.int32, device="meta")
    cells = torch.zeros(2, 3, 3, device="meta")
    bm = torch.ops.alchemiops._batch_spline_spread_channels(pos, vals, bi, cells, 2, 9, 8, 10, 12, 4)
    assert bm.shape == (2, 9, 8, 10, 12)
    assert torch.ops.alchemiops._batch_spline_gather_channels(pos, bm, bi, cells, 4).shape == (5, 9)


def _graph_targets(fn, *args):
    graphs = []

    def keep(gm, example_inputs):
        graphs.append(gm)
        return gm.forward

    compiled = torch.compile(fn, fullgraph=True, backend=aot_autograd(fw_compiler=keep))
    with pytest.raises(NativeLibraryError, match="ROCm devices only"):  # the graph is captured; the op then refuses to run off the device
        compiled(*args)
    assert len(graphs) == 1, "the function must be captured as ONE graph"
    return [str(n.target) for n in graphs[0].graph.nodes if n.op == "call_function"]


@pytest.mark.parametrize("batched", [False, True])
def test_nine_channels_trace_to_one_spread_and_one_gather(batched):
    from nvalchemiops.spline import spline_gather_channels, spline_spread_channels

    g = torch.Generator().manual_seed(3)
    pos = torch.rand(12, 3, generator=g, dtype=torch.float64) * 8
    vals = torch.randn(12, 9, generator=g, dtype=torch.float64)
    cell = torch.eye(3, dtype=torch.float64) * 8
    bi = torch.tensor([0] * 6 + [1] * 6, dtype=torch.int32) if batched else None
    cells = torch.stack([cell, cell]) if batched else cell

    def roundtrip(p, v):
        mesh = spline_spread_channels(p, v, cells, (8, 8, 8), 4, batch_idx=bi)
        return spline_gather_channels(p, mesh * 2.0, cells, 4, batch_idx=bi)

    targets = _graph_targets(roundtrip, pos, vals)
    prefix = "alchemiops._batch_spline_" if batched else "alchemiops._spline_"
    spreads = [t for t in targets if "spline_spread" in t]
    gathers = [t for t in targets if "spline_gather" in t]
    assert len(spreads) == 1 and spreads[0].startswith(prefix + "spread_channels"), targets
    assert len(gathers) == 1 and gathers[0].startswith(prefix + "gather_channels"), targets
