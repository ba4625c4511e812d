"""Cost of the DFT-D4 three-body term (`dftd4_atm`) next to `dftd3_atm` on the headline box (100 000 atoms, periodic,
tests/_headline.py::system) for three_body_cutoff = 10, 15 and 20 Bohr, each on (a) the 40-Bohr list and (b) a list built at the three-body
cutoff: the same lists, the same process, the two interleaved call by call (fp32, with virial).  Per case and function: the median
end-to-end ms (event-bracketed), the triangle visits (every triangle is visited from its three vertices; read from the counters the triple
passes leave in their workspaces), visits per second, the ratio dftd4_atm / dftd3_atm, and the per-pass medians of the library's own
HIP-event brackets (`mi_timing_*`: d4_atm_species / _pack / _cn / _weights / _triples / _chain / _fold, d3_atm_cn / _triples / _chain),
measured in a second interleaved round so that the event records do not sit in the end-to-end figures.  Tables are synthetic
(tests/d4_reference.py::d4_test_tables, tests/systems.py::d3_test_tables; the arithmetic does not care).
Usage: python tools/d4_atm_bench.py [--reps 7] [--warmup 3] [--cutoffs 10,15,20] [--atoms 100000] [--long-list 40]   -> one JSON line."""
import argparse
import ctypes
import importlib
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


def _kernel_report(lib):
    buf = ctypes.create_string_buffer(1 << 16)
    lib.mi_timing_report_stats(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, cnt, tot, med, lo, hi = line.rsplit(" ", 5)
        out[name] = float(tot)  # one call per report: the total of a bracket is that call's time in it
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cutoffs", default="10,15,20")
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--long-list", type=float, default=None, help="cutoff of the long list (default: the headline's 40 Bohr; 0: skip it)")
    args = ap.parse_args()
    from nvalchemiops import _capi as C
    from nvalchemiops.interactions.dispersion import D3Parameters, D4Parameters, dftd3_atm, dftd4_atm
    from nvalchemiops.neighborlist import neighbor_list
    from tests import _headline as H
    from tests import d4_reference as R4
    from tests import systems as S

    d3mod = importlib.import_module("nvalchemiops.interactions.dispersion.dftd3")
    d4mod = importlib.import_module("nvalchemiops.interactions.dispersion.dftd4")
    dev = "cuda:0"
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731
    if args.atoms == H.N:
        pos, cell, numbers = H.system()
    else:
        pos, cell, _, numbers = S.fcc_box(args.atoms, dtype=np.float32)
        pos, cell = (pos * H.BOHR).astype(np.float32), (cell * H.BOHR).astype(np.float32)
        numbers = np.where(numbers == 6, 6, 8)
    n = len(pos)
    tp, tc, tz = t(pos), t(cell), t(numbers.astype(np.int32))
    pbc = torch.tensor([True] * 3, device=dev)
    tab3 = S.d3_test_tables(17)
    p3 = D3Parameters(rcov=t(tab3["rcov"]), r4r2=t(tab3["r4r2"]), c6ab=t(tab3["c6ab"]), cn_ref=t(tab3["cn_ref"]))
    tab4 = R4.d4_test_tables(17)
    p4 = D4Parameters(**{k: t(tab4[k]) for k in R4.TABLE_KEYS})
    t3 = (p3.rcov, p3.r4r2, p3.c6ab, p3.cn_ref)
    t4 = tuple(getattr(p4, k) for k in R4.TABLE_KEYS)
    bj = dict(a1=0.4289, a2=4.4407)
    lib = C.lib()

    def build(rc):
        density = n / abs(float(np.linalg.det(cell.astype(np.float64))))
        width = int(1.25 * density * 4.19 * rc ** 3) + 32
        nm, num, sh = neighbor_list(tp, rc, cell=tc, pbc=pbc, method="cell_list", max_neighbors=width)
        assert int(num.max()) <= width
        return nm, sh, float(num.float().mean())

    long_rc = H.CUTOFF if args.long_list is None else args.long_list
    long_list = build(long_rc) if long_rc > 0 else None
    rows = []
    for rc3 in [float(x) for x in args.cutoffs.split(",")]:
        lists = ([(f"list{long_rc:g}", long_list)] if long_list is not None else []) + [("list_at_cutoff", build(rc3))]
        for label, (nm, sh, mean) in lists:
            common = dict(three_body_cutoff=rc3, neighbor_matrix=nm, neighbor_matrix_shifts=sh, cell=tc[None], compute_virial=True, **bj)
            variants = {"dftd3_atm": lambda: dftd3_atm(tp, tz, d3_params=p3, **common), "dftd4_atm": lambda: dftd4_atm(tp, tz, d4_params=p4, **common)}
            for _ in range(args.warmup):
                for fn in variants.values():
                    fn()
            torch.cuda.synchronize()
            total = {k: [] for k in variants}
            for _ in range(args.reps):  # round 1: end to end, interleaved
                for k, fn in variants.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    b.synchronize()
                    total[k].append(a.elapsed_time(b))
            passes = {k: {} for k in variants}
            lib.mi_timing_select(None)
            for _ in range(args.reps):  # round 2: the library's per-pass brackets, interleaved
                for k, fn in variants.items():
                    lib.mi_timing_enable(1)
                    fn()
                    torch.cuda.synchronize()
                    lib.mi_timing_enable(0)
                    for name, ms in _kernel_report(lib).items():
                        if name.startswith(("d3_atm", "d4_atm")):
                            passes[k].setdefault(name, []).append(ms)
            f32 = dict(dtype=torch.float32, device=dev)
            e, f, v = torch.empty(1, **f32), torch.empty((n, 3), **f32), torch.empty((1, 3, 3), **f32)
            visits = {
                "dftd3_atm": d3mod._launch_atm(tp, tz, C.i32(nm), sh, None, nm.shape[1], n, tc[None], None, 1, t3, d3mod.atm_scalars(bj["a1"], bj["a2"], 16.0, -4.0),
                                               1.0, 16.0, rc3, True, e, f, v, want_visits=True),
                "dftd4_atm": d4mod._launch_atm(tp, tz, C.i32(nm), sh, None, nm.shape[1], n, tc[None], None, 1, t4,
                                               d4mod.d4_scalars(bj["a1"], bj["a2"], 0.0, 0.0, 7.5, 6.0, 3.0, 2.0, None), 1.0, 16.0, rc3, True, e, f, v,
                                               want_visits=True),
            }
            row = dict(three_body_cutoff=rc3, list=label, list_width=int(nm.shape[1]), mean_list_neighbors=round(mean, 1))
            for k, fn in variants.items():
                out = fn()
                med = statistics.median(total[k])
                nv = int(visits[k].to(torch.int64).sum())
                row[k] = dict(median_ms=round(med, 3), min_max_ms=[round(min(total[k]), 3), round(max(total[k]), 3)], triangle_visits=nv,
                              visits_per_s=round(nv / (med * 1e-3), 1),
                              passes_median_ms={name: round(statistics.median(x), 4) for name, x in sorted(passes[k].items())},
                              energy_ha=float(out[0]), max_force=float(out[1].abs().max()))
            row["dftd4_atm_over_dftd3_atm"] = round(row["dftd4_atm"]["median_ms"] / row["dftd3_atm"]["median_ms"], 3)
            rows.append(row)
    print(json.dumps({"bench": "d4_atm", "atoms": n, "reps": args.reps, "warmup": args.warmup, "tile": int(lib.mi_d4_atm_tile()), "cases": rows}))


if __name__ == "__main__":
    main()
