"""Cost of the zero-damping energy kernels (`dftd3_zero`) next to the BJ ones (`dftd3`) on the headline box (100 000 atoms, periodic,
40-Bohr list; tests/_headline.py::system): the same list, the same process, the variants interleaved call by call.  Per variant -- `dftd3`,
`dftd3_zero` with alpha = 14 (powers by squaring), `dftd3_zero` with a non-integer alpha (log2 / exp2), `dftd3_zero` with beta != 0 --
the median end-to-end ms (event-bracketed, with virial) and the per-kernel medians of the library's own HIP-event brackets (`mi_timing_*`:
d3_cn, d3_energy, d3_chain), measured in a second interleaved round so that the event records do not sit in the end-to-end figures.
Then the three-body term with table radii, `dftd3_zero_atm`, next to `dftd3_atm` (BJ radii) for three_body_cutoff = 10 / 15 / 20 Bohr on
lists built at the cutoff (the cases of tools/atm_bench.py), interleaved likewise.
Usage: python tools/d3_zero_bench.py [--reps 9] [--warmup 3] [--atoms 100000] [--alpha 13.5] [--cutoffs 10,15,20]   -> one JSON line."""
import argparse
import ctypes
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
        out[name] = dict(launches=int(cnt), median_ms=round(float(med), 4), min_ms=round(float(lo), 4), max_ms=round(float(hi), 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--alpha", type=float, default=13.5, help="the non-integer exponent")
    ap.add_argument("--cutoffs", default="10,15,20", help="three-body cutoffs (empty: skip the three-body part)")
    args = ap.parse_args()
    from nvalchemiops import _capi as C
    from nvalchemiops.interactions.dispersion import D3Parameters, dftd3, dftd3_atm, dftd3_zero, dftd3_zero_atm
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
    g = np.random.default_rng(11)  # a synthetic symmetric table of pair cutoff radii, 3.5 - 9 Bohr (the arithmetic does not care)
    r0 = g.uniform(3.5, 9.0, (18, 18))
    r0 = 0.5 * (r0 + r0.T)
    r0[0, :] = r0[:, 0] = 0.0
    r0ab = t(r0.astype(np.float32))
    density = n / abs(float(np.linalg.det(cell.astype(np.float64))))
    width = int(1.25 * density * 4.19 * H.CUTOFF ** 3) + 32
    nm, num, sh = neighbor_list(tp, H.CUTOFF, cell=tc, pbc=pbc, method="cell_list", max_neighbors=width)
    assert int(num.max()) <= width
    common = dict(d3_params=params, neighbor_matrix=nm, neighbor_matrix_shifts=sh, cell=tc[None], compute_virial=True)
    variants = {
        "dftd3_bj": lambda: dftd3(tp, tz, a1=0.4289, a2=4.4407, s8=0.7875, **common),
        "dftd3_zero_alpha14": lambda: dftd3_zero(tp, tz, rs6=1.217, s8=0.722, cutoff_radii=r0ab, **common),
        f"dftd3_zero_alpha{args.alpha:g}": lambda: dftd3_zero(tp, tz, rs6=1.217, s8=0.722, alpha=args.alpha, cutoff_radii=r0ab, **common),
        "dftd3_zero_alpha14_beta0.03": lambda: dftd3_zero(tp, tz, rs6=1.217, s8=0.722, beta=0.03, cutoff_radii=r0ab, **common),
    }
    lib = C.lib()
    for _ in range(args.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    # round 1: end to end, interleaved
    total = {k: [] for k in variants}
    for _ in range(args.reps):
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            total[k].append(a.elapsed_time(b))
    # round 2: the library's per-kernel brackets, interleaved; one report per variant per repetition
    per_kernel = {k: {} for k in variants}
    lib.mi_timing_select(None)
    for _ in range(args.reps):
        for k, fn in variants.items():
            lib.mi_timing_enable(1)
            fn()
            torch.cuda.synchronize()
            lib.mi_timing_enable(0)
            for name, rec in _kernel_report(lib).items():
                if name.startswith("d3_"):
                    per_kernel[k].setdefault(name, []).append(rec["median_ms"])
    rows = {}
    for k in variants:
        out = variants[k]()
        rows[k] = dict(median_ms=round(statistics.median(total[k]), 4), min_max_ms=[round(min(total[k]), 4), round(max(total[k]), 4)],
                       kernels_median_ms={name: round(statistics.median(v), 4) for name, v in sorted(per_kernel[k].items())},
                       energy_ha=float(out[0]), max_force=float(out[1].abs().max()))
    base = rows["dftd3_bj"]["kernels_median_ms"].get("d3_energy")
    for k, r in rows.items():
        e = r["kernels_median_ms"].get("d3_energy")
        r["d3_energy_vs_bj"] = round(e / base, 4) if e and base else None
    # the three-body term: BJ radii and table radii on a list built at the three-body cutoff, interleaved
    atm_rows = []
    common.clear()  # frees the 40-Bohr list
    variants.clear()
    del nm, sh
    for rc3 in [float(x) for x in args.cutoffs.split(",") if x]:
        w3 = int(1.25 * density * 4.19 * rc3 ** 3) + 32
        nm3, num3, sh3 = neighbor_list(tp, rc3, cell=tc, pbc=pbc, method="cell_list", max_neighbors=w3)
        assert int(num3.max()) <= w3
        c3 = dict(d3_params=params, neighbor_matrix=nm3, neighbor_matrix_shifts=sh3, cell=tc[None], compute_virial=True)
        pair = {"dftd3_atm": lambda: dftd3_atm(tp, tz, a1=0.4289, a2=4.4407, three_body_cutoff=rc3, **c3),
                "dftd3_zero_atm": lambda: dftd3_zero_atm(tp, tz, rc3, cutoff_radii=r0ab, **c3)}
        for _ in range(args.warmup):
            for fn in pair.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in pair}
        for _ in range(args.reps):
            for k, fn in pair.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms[k].append(a.elapsed_time(b))
        atm_rows.append(dict(three_body_cutoff=rc3, list_width=w3, mean_list_neighbors=round(float(num3.float().mean()), 1),
                             **{k + "_median_ms": round(statistics.median(v), 3) for k, v in ms.items()},
                             **{k + "_energy_ha": float(fn()[0]) for k, fn in pair.items()}))
        del nm3, sh3, c3, pair
    print(json.dumps({"bench": "d3_zero", "atoms": n, "list_width": width, "mean_neighbors": round(float(num.float().mean()), 1),
                      "reps": args.reps, "variants": rows, "three_body": atm_rows}))


if __name__ == "__main__":
    main()
