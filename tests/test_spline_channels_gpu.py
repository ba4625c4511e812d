"""The fused multi-channel spread / gather (`spline_spread_channels`, `spline_gather_channels`; kernels behind `mi_spline_spread_channels`,
`mi_spline_gather_channels`, `mi_spline_gather_channels_frac_grad`) on the device: every channel against the CPU oracle and against the
scalar op of that channel, adjointness, autograd (first order against central differences and the per-channel composition, second order
through the values / mesh branches), torch.compile, and the full-size 100k-atom / 128^3 configuration.

Bars.  Oracle: the `_close` bar of tests/test_pme_gpu.py (1e-10 relative + 1e-12 in fp64, 1e-4 + 1e-5 in fp32).  Spread against the scalar
spread of the same channel: the two differ only in the order LDS / global atomics add the same terms.  Densest case here: 260 atoms, order
6, 8^3 mesh: about 110 terms per mesh point whose magnitudes sum to about 0.5, so reordering moves a point by at most about
110 * 1.1e-16 * 0.5 = 6e-15 in fp64: bar 1e-13 (that of the existing channel test); fp32 with the same headroom over 110 * 6e-8 * 0.5 =
3.3e-6: 5e-5.  Gather against the scalar gather: bit equality (one thread per atom, the same operations in the same order)."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import systems as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MESHES = [(8, 8, 8), (16, 8, 24), (32, 32, 32), (30, 36, 45), (12, 10, 14), (31, 9, 6)]
CHANNELS = (1, 3, 4, 9, 11)


@pytest.fixture(autouse=True, params=["tile", "atomic", "auto"])
def spread_path(request, monkeypatch):
    """Every test runs with the tile pipeline forced wherever the mesh allows it, with the atomic kernel forced, and with the library's policy."""
    from nvalchemiops import spline

    monkeypatch.setattr(spline, "_SPREAD_PATH", request.param)
    return request.param


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _close(got, ref, dtype, what, scale=None):
    got = got.detach().cpu().numpy()
    ref = ref.detach().cpu().numpy() if isinstance(ref, torch.Tensor) else ref
    scale = np.abs(ref).max() if scale is None else scale
    tol = (1e-10 if dtype == np.float64 else 1e-4) * scale + (1e-12 if dtype == np.float64 else 1e-5)
    err = np.abs(got - ref).max()
    print(f"{what}: max err {err:.3e} (bar {tol:.3e})")
    assert err <= tol, f"{what}: max err {err:.3e} > {tol:.3e}"


def _system(n, dtype, seed, box=12.0):
    g = np.random.default_rng(seed)
    cell = np.array([[box, 0, 0], [0.2 * box, 0.9 * box, 0], [0.1 * box, -0.15 * box, 1.1 * box]])
    pos = g.uniform(0, 1, (n, 3)) @ cell
    pos = pos + g.integers(-1, 2, (n, 1)) * cell[0]  # some atoms outside the cell
    return pos.astype(dtype), cell.astype(dtype), g


def _cases(dims, order, dtype, nch):
    """(positions, values[N, C], cell(s), batch_idx) for a single system and a two-system batch with different cells."""
    pos, cell, g = _system(260, dtype, seed=order + dims[0] + 7 * nch)
    vals = g.normal(size=(260, nch)).astype(dtype)
    yield "single", pos, vals, cell, None
    pos2, vals2 = np.concatenate([pos, pos * 0.8]).astype(dtype), np.concatenate([vals, 2 * vals]).astype(dtype)
    yield "batch", pos2, vals2, np.stack([cell, cell * 0.8]).astype(dtype), np.repeat(np.arange(2, dtype=np.int32), 260)


@pytest.mark.parametrize("dims", MESHES)
@pytest.mark.parametrize("order", [1, 2, 3, 4, 5, 6])
def test_spread_channels_match_oracle_and_scalar(dims, order):
    from nvalchemiops.spline import spline_gather, spline_gather_channels, spline_spread, spline_spread_channels

    for dtype in (np.float64, np.float32):
        for nch in CHANNELS:
            for kind, pos, vals, cell, bi in _cases(dims, order, dtype, nch):
                tp, tv, tc = _t(pos), _t(vals), _t(cell)
                tb = None if bi is None else _t(bi)
                mesh = spline_spread_channels(tp, tv, tc, dims, order, batch_idx=tb)
                assert mesh.shape == ((2, nch) if bi is not None else (nch,)) + dims and mesh.dtype == tp.dtype
                for ch in range(nch):
                    got = mesh[ch] if bi is None else mesh[:, ch]
                    what = f"{kind} C={nch} ch={ch} order={order} {dims} {np.dtype(dtype).name}"
                    if order <= 4:
                        _close(got, O.spline_spread(pos, vals[:, ch].copy(), cell, dims, order, batch_idx=bi), dtype, "oracle " + what)
                    scalar = spline_spread(tp, tv[:, ch].contiguous(), tc, dims, order, batch_idx=tb)
                    err = float((got - scalar).abs().max())
                    bar = (1e-13 if dtype == np.float64 else 5e-5) * (2.0 if bi is not None else 1.0)  # the second system carries 2 x the values
                    assert err <= bar, f"scalar {what}: {err:.3e} > {bar:.1e}"
                if order >= 5:
                    # per-channel charge conservation and adjointness with the gather.  fp64, single system: the bars of
                    # test_spline_high_order_properties (1e-10, 1e-6).  The batch kernels drop weights <= 1e-8 (reference semantics), so a
                    # batch conserves to that level only, and fp32 has its own rounding: the bars of test_tile_owned_spread for those.
                    tol = (1e-10 if dtype == np.float64 else 2e-3) if bi is None else (1e-4 if dtype == np.float64 else 2e-3)
                    sums = (mesh.sum(dim=(-1, -2, -3)) if bi is None else mesh[0].sum(dim=(-1, -2, -3))).cpu().numpy()
                    ref = vals[:260].astype(np.float64).sum(0)
                    print(f"conservation {kind} C={nch} order={order} {dims} {np.dtype(dtype).name}: {np.abs(sums - ref).max():.3e} (bar {tol:.1e})")
                    assert np.abs(sums - ref).max() < tol, (kind, nch, np.abs(sums - ref).max())
                    gen = torch.Generator(device=DEV).manual_seed(order * 100 + dims[0] + nch)
                    field = torch.randn(mesh.shape, dtype=tp.dtype, device=DEV, generator=gen)
                    back = spline_gather_channels(tp, field, tc, order, batch_idx=tb)
                    for ch in range(nch):
                        lhs = float(((mesh[ch] if bi is None else mesh[:, ch]) * (field[ch] if bi is None else field[:, ch])).sum())
                        rhs = float((tv[:, ch] * back[:, ch]).sum())
                        assert abs(lhs - rhs) < (1e-6 if dtype == np.float64 else 1e-2), (kind, nch, ch, lhs, rhs)


@pytest.mark.parametrize("dims", MESHES)
@pytest.mark.parametrize("order", [1, 2, 3, 4, 5, 6])
def test_gather_channels_match_oracle_and_scalar_bitwise(dims, order):
    from nvalchemiops.spline import spline_gather, spline_gather_channels

    for dtype in (np.float64, np.float32):
        for nch in CHANNELS:
            for kind, pos, _, cell, bi in _cases(dims, order, dtype, nch):
                g = np.random.default_rng(nch + order)
                mesh = g.normal(size=((2, nch) if bi is not None else (nch,)) + dims).astype(dtype)
                tp, tm, tc = _t(pos), _t(mesh), _t(cell)
                tb = None if bi is None else _t(bi)
                out = spline_gather_channels(tp, tm, tc, order, batch_idx=tb)
                assert out.shape == (len(pos), nch) and out.dtype == tp.dtype
                for ch in range(nch):
                    plane = mesh[ch] if bi is None else np.ascontiguousarray(mesh[:, ch])
                    what = f"{kind} C={nch} ch={ch} order={order} {dims} {np.dtype(dtype).name}"
                    assert torch.equal(out[:, ch], spline_gather(tp, _t(plane), tc, order, batch_idx=tb)), "not bit-identical to the scalar gather: " + what
                    if order <= 4:
                        _close(out[:, ch], O.spline_gather(pos, plane, cell, order, batch_idx=bi), dtype, "oracle gather " + what)


@pytest.mark.parametrize("batched", [False, True])
def test_adjointness_across_channels(batched):
    from nvalchemiops.spline import spline_gather_channels, spline_spread_channels

    for order in (3, 4, 5):
        for nch in (4, 9):
            for kind, pos, vals, cell, bi in _cases((16, 8, 24), order, np.float64, nch):
                if (bi is not None) != batched:
                    continue
                tp, tv, tc = _t(pos), _t(vals), _t(cell)
                tb = None if bi is None else _t(bi)
                mesh = spline_spread_channels(tp, tv, tc, (16, 8, 24), order, batch_idx=tb)
                gen = torch.Generator(device=DEV).manual_seed(order + nch)
                field = torch.randn(mesh.shape, dtype=torch.float64, device=DEV, generator=gen)
                lhs, rhs = float((mesh * field).sum()), float((tv * spline_gather_channels(tp, field, tc, order, batch_idx=tb)).sum())
                assert abs(lhs - rhs) < 1e-6, (order, nch, lhs, rhs)  # the gather drops weights <= 1e-8


def test_reference_spline_orders_give_a_zero_mesh():
    from nvalchemiops.spline import reference_spline_orders, spline_gather_channels, spline_spread_channels

    for _, pos, vals, cell, bi in _cases((16, 8, 24), 5, np.float64, 9):
        tb = None if bi is None else _t(bi)
        with reference_spline_orders():
            mesh = spline_spread_channels(_t(pos), _t(vals), _t(cell), (16, 8, 24), 5, batch_idx=tb)
            back = spline_gather_channels(_t(pos), torch.ones_like(mesh), _t(cell), 5, batch_idx=tb)
            m4 = spline_spread_channels(_t(pos), _t(vals), _t(cell), (16, 8, 24), 4, batch_idx=tb)
        assert float(mesh.abs().max()) == 0.0 and float(back.abs().max()) == 0.0 and float(m4.abs().max()) > 0.0
        assert float(spline_spread_channels(_t(pos), _t(vals), _t(cell), (16, 8, 24), 5, batch_idx=tb).abs().max()) > 0.0


def test_empty_inputs_and_shared_cell():
    from nvalchemiops.spline import spline_gather_channels, spline_spread_channels

    pos, cell, g = _system(40, np.float64, 3)
    tp, tc = _t(pos), _t(cell)
    dims = (12, 10, 14)
    assert spline_spread_channels(tp, torch.zeros((40, 0), dtype=torch.float64, device=DEV), tc, dims, 3).shape == (0,) + dims
    assert spline_gather_channels(tp, torch.zeros((0,) + dims, dtype=torch.float64, device=DEV), tc, 3).shape == (40, 0)
    e = spline_spread_channels(tp[:0], torch.zeros((0, 3), dtype=torch.float64, device=DEV), tc, dims, 3)
    assert e.shape == (3,) + dims and float(e.abs().max()) == 0.0
    assert spline_gather_channels(tp[:0], torch.zeros((3,) + dims, dtype=torch.float64, device=DEV), tc, 3).shape == (0, 3)
    # one shared 2-D cell for a batch: two copies of the system give two copies of the mesh
    vals = _t(g.normal(size=(40, 3)))
    bi = torch.tensor([0] * 40 + [1] * 40, dtype=torch.int32, device=DEV)
    mb = spline_spread_channels(torch.cat([tp, tp]), torch.cat([vals, vals]), tc, dims, 3, batch_idx=bi)
    assert mb.shape == (2, 3) + dims and torch.allclose(mb[0], mb[1], rtol=0, atol=1e-13)
    vb = spline_gather_channels(torch.cat([tp, tp]), mb, tc, 3, batch_idx=bi)
    assert torch.allclose(vb[:40], vb[40:], rtol=0, atol=1e-13)  # (the two meshes differ by the order of the atomic adds)


# ---- autograd -------------------------------------------------------------------------------------------------------------------------
def _small(n=20, box=11.0, seed=0):
    """The 20-atom triclinic system of tests/test_autograd_gpu.py (same generator, so the same distance from the spline knots)."""
    g = torch.Generator().manual_seed(seed)
    cell = torch.tensor([[box, 0, 0], [0.15 * box, 0.95 * box, 0], [0.1 * box, -0.1 * box, 1.05 * box]], dtype=torch.float64)
    pos = torch.rand((n, 3), generator=g, dtype=torch.float64) @ cell
    q = torch.randn(n, generator=g, dtype=torch.float64)
    vals = torch.randn((n, 9), generator=g, dtype=torch.float64)
    return pos.to(DEV), cell.to(DEV), vals.to(DEV)


def _loop_spread(p, v, c, dims, order, bi=None):
    from nvalchemiops.spline import spline_spread

    return torch.stack([spline_spread(p, v[:, ch], c, dims, order, bi) for ch in range(v.shape[1])], dim=0 if bi is None else 1)


def _loop_gather(p, m, c, order, bi=None):
    from nvalchemiops.spline import spline_gather

    nch = m.shape[0] if bi is None else m.shape[1]
    return torch.stack([spline_gather(p, m[ch] if bi is None else m[:, ch], c, order, bi) for ch in range(nch)], dim=1)


@pytest.mark.parametrize("batched", [False, True])
def test_channel_adjoints_match_finite_differences_and_the_loop(batched):
    from nvalchemiops.spline import spline_gather_channels, spline_spread_channels

    pos, cell, vals = _small(20)
    dims = (10, 12, 9)
    bi = torch.as_tensor(np.repeat(np.arange(2, dtype=np.int32), 10), device=DEV) if batched else None
    cells = torch.stack([cell, cell * 1.1]) if batched else cell
    shape = ((2, 9) if batched else (9,)) + dims
    gen = torch.Generator(device=DEV).manual_seed(11)
    field = torch.randn(shape, dtype=torch.float64, device=DEV, generator=gen)
    wout = torch.randn((20, 9), dtype=torch.float64, device=DEV, generator=gen)
    eps = 1e-6
    cidx = (1, 1, 0) if batched else (1, 0)
    for order in (3, 4, 5):
        def spread_loss(p, v, c, fn=spline_spread_channels):
            return (fn(p, v, c, dims, order, bi) * field).sum()

        def gather_loss(p, m, c, fn=spline_gather_channels):
            return (fn(p, m, c, order, bi) * wout).sum()

        for loss, second, loop in ((spread_loss, vals, _loop_spread), (gather_loss, field, _loop_gather)):
            p, s, c = (t.clone().requires_grad_(True) for t in (pos, second, cells))
            gp, gs, gc = torch.autograd.grad(loss(p, s, c), (p, s, c))
            # first derivatives equal those of the per-channel composition
            p2, s2, c2 = (t.clone().requires_grad_(True) for t in (pos, second, cells))
            lp, ls, lc = torch.autograd.grad(loss(p2, s2, c2, fn=loop), (p2, s2, c2))
            for got, ref, what in ((gp, lp, "positions"), (gs, ls, "values / mesh"), (gc, lc, "cell")):
                _close(got, ref, np.float64, f"{loss.__name__} order {order} d/d{what} vs the per-channel loop")
            with torch.no_grad():
                for (idx, d) in ((3, 0), (7, 2), (15, 1)):
                    pp, pm = pos.clone(), pos.clone()
                    pp[idx, d] += eps
                    pm[idx, d] -= eps
                    fd = float(loss(pp, second, cells) - loss(pm, second, cells)) / (2 * eps)
                    assert abs(fd - gp[idx, d].item()) < 1e-5 * max(1.0, abs(fd)), (loss.__name__, order, idx, d, fd, gp[idx, d].item())
                cp, cm = cells.clone(), cells.clone()
                cp[cidx] += eps
                cm[cidx] -= eps
                fd = float(loss(pos, second, cp) - loss(pos, second, cm)) / (2 * eps)
                assert abs(fd - gc[cidx].item()) < 1e-5 * max(1.0, abs(fd)), (loss.__name__, order, "cell", fd, gc[cidx].item())
                for sidx in (((4, 2), (17, 8)) if second is vals else (((1, 3, 4, 5, 2) if batched else (3, 4, 5, 2)),)):
                    sp, sm = second.clone(), second.clone()
                    sp[sidx] += eps
                    sm[sidx] -= eps
                    fd = float(loss(pos, sp, cells) - loss(pos, sm, cells)) / (2 * eps)
                    assert abs(fd - gs[sidx].item()) < 1e-5 * max(1.0, abs(fd)), (loss.__name__, order, sidx, fd, gs[sidx].item())


def test_second_order_through_values_and_mesh_branches():
    from nvalchemiops.spline import spline_gather_channels, spline_spread_channels

    pos, cell, vals = _small(20)
    dims = (10, 12, 9)
    gen = torch.Generator(device=DEV).manual_seed(12)
    field = torch.randn((9,) + dims, dtype=torch.float64, device=DEV, generator=gen)
    wout = torch.randn((20, 9), dtype=torch.float64, device=DEV, generator=gen)

    def spread_second(fn):
        # L = sum(mesh^2): dL/dvalues = gather(2 mesh) depends on the values again; differentiate |dL/dvalues|^2 w.r.t. the values
        v = vals.clone().requires_grad_(True)
        mesh = fn(pos, v, cell, dims, 4)
        (gv,) = torch.autograd.grad((mesh * mesh * field).sum(), v, create_graph=True)
        (hv,) = torch.autograd.grad((gv * gv).sum(), v)
        return gv.detach(), hv

    def gather_second(fn):
        m = field.clone().requires_grad_(True)
        out = fn(pos, m, cell, 4)
        (gm,) = torch.autograd.grad((out * out * wout).sum(), m, create_graph=True)
        (hm,) = torch.autograd.grad((gm * gm).sum(), m)
        return gm.detach(), hm

    for second, fused, loop in ((spread_second, spline_spread_channels, lambda p, v, c, d, o: _loop_spread(p, v, c, d, o)),
                                (gather_second, spline_gather_channels, lambda p, m, c, o: _loop_gather(p, m, c, o))):
        (g1, h1), (g2, h2) = second(fused), second(loop)
        _close(g1, g2, np.float64, second.__name__ + " first derivative")
        _close(h1, h2, np.float64, second.__name__ + " second derivative")
    # the position branch is refused, as by the scalar ops
    from nvalchemiops.spline import spline_spread

    for fn, args in ((spline_spread_channels, (vals, cell, dims, 4)), (spline_gather_channels, (field, cell, 4)), (spline_spread, (vals[:, 0], cell, dims, 4))):
        p = pos.clone().requires_grad_(True)
        (gp,) = torch.autograd.grad(fn(p, *args).pow(2).sum(), p, create_graph=True)
        with pytest.raises(NotImplementedError, match="second derivatives of the pair kernels"):
            torch.autograd.grad(gp.pow(2).sum(), p)


# ---- torch.compile --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", ["aot_eager", "inductor"])
def test_nine_channel_roundtrip_compiles_fullgraph(backend):
    from nvalchemiops.spline import spline_gather_channels, spline_spread_channels

    pos, cell, vals = _small(20)
    dims = (10, 12, 9)

    def roundtrip(p, v, c):
        mesh = spline_spread_channels(p, v, c, dims, 4)
        return spline_gather_channels(p, mesh * 2.0, c, 4)

    torch._dynamo.reset()
    compiled = torch.compile(roundtrip, fullgraph=True, backend=backend)
    outs = []
    for fn in (roundtrip, compiled):
        p, v, c = (t.clone().requires_grad_(True) for t in (pos, vals, cell))
        out = fn(p, v, c)
        outs.append((out.detach(),) + torch.autograd.grad(out.pow(2).sum(), (p, v, c)))
    for got, ref, what in zip(outs[1], outs[0], ("forward", "d/dpositions", "d/dvalues", "d/dcell")):
        _close(got, ref, np.float64, f"{backend} {what}")


# ---- full size ------------------------------------------------------------------------------------------------------------------------
_FULL = {}


def _full_size(dtype):
    """Config-4 box with nine random channels and the oracle's order-4 meshes (evaluated once per dtype, not once per spread path)."""
    if dtype not in _FULL:
        pos, cell, _, _ = S.fcc_box(100000, dtype=dtype)
        vals = np.random.default_rng(9).normal(size=(100000, 9)).astype(dtype)
        _FULL[dtype] = (pos, cell, vals, [O.spline_spread(pos, vals[:, ch].copy(), cell, (128, 128, 128), 4) for ch in range(9)])
    return _FULL[dtype]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_full_size_config4_nine_channels(dtype):
    """100 000 atoms, 128^3 mesh, C = 9: the tile pipeline (forced, and chosen by the library's own policy at this size) and the atomic kernel."""
    from nvalchemiops.spline import spline_spread, spline_spread_channels

    pos, cell, vals, oracle4 = _full_size(dtype)
    dims = (128, 128, 128)
    g = np.random.default_rng(10)
    tp, tv, tc = _t(pos), _t(vals), _t(cell)
    perm = g.permutation(100000)
    for order in (4, 5):
        mesh = spline_spread_channels(tp, tv, tc, dims, order)
        shuffled = spline_spread_channels(_t(pos[perm]), _t(vals[perm]), tc, dims, order)
        _close(shuffled, mesh, dtype, f"order {order}: atoms in a random order")
        del shuffled
        for ch in range(9):
            if order == 4:
                _close(mesh[ch], oracle4[ch], dtype, f"100k order 4 channel {ch} vs the oracle")
            else:
                _close(mesh[ch], spline_spread(tp, tv[:, ch].contiguous(), tc, dims, 5), dtype, f"100k order 5 channel {ch} vs the scalar spread")
