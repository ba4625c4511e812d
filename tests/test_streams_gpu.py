"""The ops on non-default streams.  bench.py runs PME and D3 on two streams, so side streams are the intended use; every launch of this
package goes to torch's CURRENT stream (`_capi.stream_of`), and whatever a module caches across calls must be safe to hand to a caller on
another stream.  Three tests: a fresh side stream gives the default stream's results; PME and D3 side by side on two streams, joined by
events, give the serial results; and a Python-float alpha -- cached as a device tensor by `pme._alpha_constant` -- is complete before a
second stream can read it.  Shapes, systems and tolerances are those of tests/test_arg_layouts_gpu.py."""
import pytest
import torch

from oracle import oracle as O
from tests import test_arg_layouts_gpu as L
from tests import test_pme_gpu as TP

pytestmark = pytest.mark.gpu
DEV = L.DEV
LDS_MESH, PLAN_MESH = (16, 8, 24), (14, 12, 10)  # the fused in-LDS solve / hipFFT plans (14 has a factor 7)


def _tables():
    from nvalchemiops.interactions.dispersion import D3Parameters

    t = L.S.d3_test_tables(17)
    return D3Parameters(rcov=L._t(t["rcov"]), r4r2=L._t(t["r4r2"]), c6ab=L._t(t["c6ab"]), cn_ref=L._t(t["cn_ref"]))


def _step(f, params, dims, alpha=0.4):
    """cell_list -> dftd3 -> particle_mesh_ewald with a Python-float alpha, on whatever stream is current."""
    from nvalchemiops.interactions.dispersion import dftd3
    from nvalchemiops.interactions.electrostatics import particle_mesh_ewald
    from nvalchemiops.neighborlist import cell_list

    nm, num, sh = cell_list(f.P, L.RC, f.C[0], f.PBC[0], max_neighbors=L.M)
    d3 = dftd3(f.P, f.Zt, d3_params=params, neighbor_matrix=nm, neighbor_matrix_shifts=sh, cell=f.C, compute_virial=True, **L.D3_BJ)
    pme = particle_mesh_ewald(f.P, f.Q, f.C[0], alpha=alpha, mesh_dimensions=dims, spline_order=4, neighbor_matrix=nm, neighbor_matrix_shifts=sh,
                              mask_value=f.n, compute_forces=True)
    return (nm, num, sh) + tuple(d3) + tuple(pme)


def _same(out, ref, f, what):
    """(matrix, counts, shifts) exact; (energy, forces, coord_num, virial) of D3 and (energies, forces) of PME at the bars of part 1."""
    pme = L._close_pme(f.dtype)
    L._compare(out, ref, lambda o, r, w, i: L.CLOSE_D3(o, r, w, i - 3) if i < 7 else pme(o, r, w, i), what)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("dims", [LDS_MESH, PLAN_MESH])
def test_side_stream_equals_default_stream(dtype, dims):
    from nvalchemiops import _capi as C

    f, params = L._fx(dtype), _tables()
    assert bool(C.lib().mi_pme_solve_supported(1, *dims, C.dtype_code(f.tdtype))) == (dims == LDS_MESH)
    torch.cuda.synchronize()
    ref = _step(f, params, dims)
    torch.cuda.current_stream().synchronize()
    want = O.particle_mesh_ewald(f.pos, f.q, f.cell[0], 0.4, dims, 4, neighbor_matrix=f.nm_np, neighbor_matrix_shifts=f.sh_np, mask_value=f.n,
                                 compute_forces=True)
    TP._close(ref[-2], want[0], f.dtype, "default stream energies vs oracle")
    TP._close(ref[-1], want[1], f.dtype, "default stream forces vs oracle")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = _step(f, params, dims)
    side.synchronize()
    _same(out, ref, f, f"side stream {dims}")


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_pme_and_d3_on_two_streams_equal_the_serial_run(dtype):
    """As bench.py: one list, then PME on one stream and D3 on another, joined by events."""
    from nvalchemiops.interactions.dispersion import dftd3
    from nvalchemiops.interactions.electrostatics import particle_mesh_ewald
    from nvalchemiops.neighborlist import cell_list

    f, params = L._fx(dtype), _tables()
    dims = LDS_MESH
    ref = _step(f, params, dims)
    torch.cuda.synchronize()
    main, s_pme, s_d3 = torch.cuda.current_stream(), torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(3):  # several rounds: the second and third reuse what the first cached and freed
        nm, num, sh = cell_list(f.P, L.RC, f.C[0], f.PBC[0], max_neighbors=L.M)
        listed = torch.cuda.Event()
        listed.record(main)
        s_pme.wait_event(listed)
        s_d3.wait_event(listed)
        with torch.cuda.stream(s_pme):
            pme = particle_mesh_ewald(f.P, f.Q, f.C[0], alpha=0.4, mesh_dimensions=dims, spline_order=4, neighbor_matrix=nm, neighbor_matrix_shifts=sh,
                                      mask_value=f.n, compute_forces=True)
            done_pme = torch.cuda.Event()
            done_pme.record(s_pme)
        with torch.cuda.stream(s_d3):
            d3 = dftd3(f.P, f.Zt, d3_params=params, neighbor_matrix=nm, neighbor_matrix_shifts=sh, cell=f.C, compute_virial=True, **L.D3_BJ)
            done_d3 = torch.cuda.Event()
            done_d3.record(s_d3)
        for t in (nm, num, sh):  # the list is read by both side streams: its blocks must not be handed out again before they are done
            t.record_stream(s_pme)
            t.record_stream(s_d3)
        main.wait_event(done_pme)
        main.wait_event(done_d3)
        total = pme[0].sum() + d3[0].sum().to(pme[0].dtype)  # consumed on the main stream, as an MD step would
        main.synchronize()
        assert bool(torch.isfinite(total))
        _same((nm, num, sh) + tuple(d3) + tuple(pme), ref, f, "two streams")


def _delay(stream_device):
    """Keep the current stream busy for a few milliseconds."""
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(20_000_000)
    else:
        a = torch.randn(2048, 2048, device=stream_device)
        for _ in range(20):
            a = (a @ a) * 1e-3


def _alpha_cache_scenario(dtype="float64"):
    """(energies on stream A, energies on stream B, oracle energies): `pme_reciprocal_space(..., alpha=0.37)` first on a stream A that is
    still busy, then at once on a stream B that has waited for nothing but the inputs.  A's allocator pool has been primed so that the
    block the cached alpha tensor gets holds NaN until its fill runs: a B that reads it early computes NaN energies.  (A read of stale
    memory inside the allocation, not a fault.)"""
    from nvalchemiops.interactions.electrostatics import pme as P
    from nvalchemiops.interactions.electrostatics import pme_reciprocal_space

    f = L._fx(dtype)
    dims = LDS_MESH  # no FFT plan to create (and self-test, with a host read) on the new streams: nothing else orders B after A's fill
    run = lambda alpha: pme_reciprocal_space(f.P, f.Q, f.C[0], alpha, mesh_dimensions=dims, spline_order=4)  # noqa: E731
    want = O.pme_reciprocal_space(f.pos, f.q, f.cell[0], 0.37, dims, 4)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    for s in (torch.cuda.current_stream(), a, b):  # warm-up with a TENSOR alpha: per-shape tables and allocator pools exist, the cache stays empty
        with torch.cuda.stream(s):
            run(torch.tensor([0.37], dtype=f.tdtype, device=DEV))
    torch.cuda.synchronize()
    P._alpha_constant.cache_clear()
    with torch.cuda.stream(a):
        junk = [torch.full((n,), float("nan"), dtype=f.tdtype, device=DEV) for n in (1,) * 32]
        a.synchronize()
        del junk  # A's pool now hands these NaN blocks out again
        _delay(DEV)
        ea = run(0.37)
    with torch.cuda.stream(b):
        eb = run(0.37)
    b.synchronize()
    a.synchronize()
    return ea, eb, want, f.dtype


def test_cached_float_alpha_is_complete_before_another_stream_reads_it():
    """`pme._alpha_constant` caches the tensor of a Python-float alpha across calls.  Its fill is enqueued on the stream that is current at
    the FIRST call; a second call on another stream gets the cached tensor at once, and a caller who passed a float has nothing to wait
    on -- so the creation itself must be ordered before the tensor is published (one stream.synchronize() at creation, as `_solve_tables`).
    The test can only bite by timing and by allocator reuse: with the unsynchronised cache of the parent commit stream B read NaN energies
    in 2 of 3 runs of this scenario on an MI355X and the correct ones in the third; with the synchronised one 0 of 3.  A pass is therefore
    no proof, a failure is."""
    ea, eb, want, dt = _alpha_cache_scenario()
    TP._close(ea, want, dt, "stream A (created the cached alpha)")
    assert bool(torch.isfinite(eb).all()), "stream B read the cached alpha tensor before its fill had run"
    TP._close(eb, want, dt, "stream B (got the cached alpha)")
