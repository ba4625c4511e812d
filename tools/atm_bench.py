"""Cost of the DFT-D3 three-body term (`dftd3_atm`) on the headline box (100 000 atoms, periodic, tests/_headline.py::system) for
three_body_cutoff = 10, 15 and 20 Bohr, on (a) the 40-Bohr list `dftd3` runs on and (b) a list built at the three-body cutoff.  Per case:
median ms of `dftd3_atm` (event-bracketed, with virial), the number of triangle visits (every triangle is visited from its three vertices;
read from the diagnostic counters the triple pass leaves in its workspace), visits per second, and the two-body `dftd3` time on the 40-Bohr
list of the same box for scale.
Usage: python tools/atm_bench.py [--reps 7] [--warmup 2] [--cutoffs 10,15,20] [--atoms 100000]   -> one JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "nvalchemi-toolkit-ops_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cutoffs", default="10,15,20")
    ap.add_argument("--atoms", type=int, default=100000)
    args = ap.parse_args()
    from nvalchemiops import _capi as C
    from nvalchemiops.interactions.dispersion import D3Parameters, dftd3, dftd3_atm
    import importlib

    d3mod = importlib.import_module("nvalchemiops.interactions.dispersion.dftd3")
    from nvalchemiops.neighborlist import neighbor_list
    from tests import _headline as H
    from tests import systems as S

    dev = "cuda:0"
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731
    if args.atoms == H.N:
        pos, cell, numbers = H.system()
    else:
        pos, cell, _, numbers = S.fcc_box(args.atoms, dtype=np.float32)
        pos, cell = (pos * H.BOHR).astype(np.float32), (cell * H.BOHR).astype(np.float32)
    n = len(pos)
    tp, tc, tz = t(pos), t(cell), t(numbers.astype(np.int32))
    pbc = torch.tensor([True] * 3, device=dev)
    tab = S.d3_test_tables(17)
    params = D3Parameters(rcov=t(tab["rcov"]), r4r2=t(tab["r4r2"]), c6ab=t(tab["c6ab"]), cn_ref=t(tab["cn_ref"]))
    tables = (params.rcov, params.r4r2, params.c6ab, params.cn_ref)
    bj = dict(a1=0.4289, a2=4.4407)

    def build(rc):
        density = n / abs(float(np.linalg.det(cell.astype(np.float64))))
        width = int(1.25 * density * 4.19 * rc ** 3) + 32
        nm, num, sh = neighbor_list(tp, rc, cell=tc, pbc=pbc, method="cell_list", max_neighbors=width)
        assert int(num.max()) <= width
        return nm, sh, float(num.float().mean())

    long_rc = H.CUTOFF
    nm40, sh40, mean40 = build(long_rc)
    two_body = lambda: dftd3(tp, tz, s8=0.7875, d3_params=params, neighbor_matrix=nm40, neighbor_matrix_shifts=sh40, cell=tc[None], compute_virial=True, **bj)  # noqa: E731
    d3_ms = _median_ms(two_body, args.reps, args.warmup)
    rows = []
    for rc3 in [float(x) for x in args.cutoffs.split(",")]:
        for label, (nm, sh, mean) in (("list40", (nm40, sh40, mean40)), ("list_at_cutoff", build(rc3))):
            run = lambda: dftd3_atm(tp, tz, three_body_cutoff=rc3, d3_params=params, neighbor_matrix=nm, neighbor_matrix_shifts=sh, cell=tc[None],  # noqa: E731
                                    compute_virial=True, **bj)
            med, lo, hi = _median_ms(run, args.reps, args.warmup)
            e, f, v = run()
            energy = torch.empty(1, device=dev)
            forces = torch.empty((n, 3), device=dev)
            virial = torch.empty((1, 3, 3), device=dev)
            visits = d3mod._launch_atm(tp, tz, C.i32(nm), sh, None, nm.shape[1], n, tc[None], None, 1, tables, d3mod.atm_scalars(bj["a1"], bj["a2"], 16.0, -4.0),
                                       1.0, 16.0, rc3, True, energy, forces, virial, want_visits=True)
            nv = int(visits.to(torch.int64).sum())
            rows.append(dict(three_body_cutoff=rc3, list=label, list_width=int(nm.shape[1]), mean_list_neighbors=round(mean, 1), median_ms=round(med, 3),
                             min_max_ms=[round(lo, 3), round(hi, 3)], triangle_visits=nv, visits_per_s=round(nv / (med * 1e-3), 1),
                             energy_ha=float(e), max_force=float(f.abs().max())))
    print(json.dumps({"bench": "atm", "atoms": n, "reps": args.reps, "dftd3_two_body_ms_on_list40": round(d3_ms[0], 3), "cases": rows}))


if __name__ == "__main__":
    main()
