"""Cost of `dftd4` next to `dftd3` on the headline box's list (100 000 atoms, periodic, 40-Bohr padded matrix; tests/_headline.py::system):
the same list, the same process, the two interleaved call by call.  Per function the median end-to-end ms (event-bracketed, with virial)
and the per-pass medians of the library's own HIP-event brackets (`mi_timing_*`: d3_cn / d3_energy / d3_chain ..., d4_species / d4_pack /
d4_cn / d4_weights / d4_energy / d4_chain / d4_fold), measured in a second interleaved round so that the event records do not sit in the
end-to-end figures.  Tables are synthetic (tests/d4_reference.py::d4_test_tables; the arithmetic does not care), charges uniform in
[-0.3, 0.3].  `algorithmic_bytes` is what each D4 pass must move per stored entry and per atom.
Usage: python tools/d4_bench.py [--reps 9] [--warmup 3] [--atoms 100000] [--cutoff 40]   -> one JSON line."""
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
        out[name] = float(med)  # (d4_species and d4_fold bracket their two / three small launches together)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--cutoff", type=float, default=None)
    args = ap.parse_args()
    from nvalchemiops import _capi as C
    from nvalchemiops.interactions.dispersion import D3Parameters, D4Parameters, dftd3, dftd4
    from nvalchemiops.neighborlist import neighbor_list
    from tests import _headline as H
    from tests import d4_reference as R4
    from tests import systems as S

    dev = "cuda:0"
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731
    if args.atoms == H.N:
        pos, cell, numbers = H.system()
    else:
        pos, cell, _, numbers = S.fcc_box(args.atoms, dtype=np.float32)
        pos, cell = (pos * H.BOHR).astype(np.float32), (cell * H.BOHR).astype(np.float32)
        numbers = np.where(numbers == 6, 6, 8)
    rc = H.CUTOFF if args.cutoff is None else args.cutoff
    n = len(pos)
    tp, tc, tz = t(pos), t(cell), t(numbers.astype(np.int32))
    tq = t(np.random.default_rng(5).uniform(-0.3, 0.3, n).astype(np.float32))
    pbc = torch.tensor([True] * 3, device=dev)
    tab3 = S.d3_test_tables(17)
    p3 = D3Parameters(rcov=t(tab3["rcov"]), r4r2=t(tab3["r4r2"]), c6ab=t(tab3["c6ab"]), cn_ref=t(tab3["cn_ref"]))
    tab4 = R4.d4_test_tables(17)
    p4 = D4Parameters(**{k: t(tab4[k]) for k in R4.TABLE_KEYS})
    density = n / abs(float(np.linalg.det(cell.astype(np.float64))))
    width = int(1.25 * density * 4.19 * rc ** 3) + 32
    nm, num, sh = neighbor_list(tp, rc, cell=tc, pbc=pbc, method="cell_list", max_neighbors=width)
    assert int(num.max()) <= width
    common = dict(neighbor_matrix=nm, neighbor_matrix_shifts=sh, cell=tc[None], compute_virial=True)
    variants = {
        "dftd3": lambda: dftd3(tp, tz, a1=0.4289, a2=4.4407, s8=0.7875, d3_params=p3, **common),
        "dftd4": lambda: dftd4(tp, tz, tq, a1=0.4289, a2=4.4407, s8=0.7875, d4_params=p4, **common),
    }
    lib = C.lib()
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
    per_kernel = {k: {} for k in variants}
    lib.mi_timing_select(None)
    for _ in range(args.reps):  # round 2: the library's per-pass brackets, interleaved
        for k, fn in variants.items():
            lib.mi_timing_enable(1)
            fn()
            torch.cuda.synchronize()
            lib.mi_timing_enable(0)
            for name, ms in _kernel_report(lib).items():
                if name.startswith(("d3_", "d4_")):
                    per_kernel[k].setdefault(name, []).append(ms)
    rows = {}
    for k, fn in variants.items():
        out = fn()
        rows[k] = dict(median_ms=round(statistics.median(total[k]), 4), min_max_ms=[round(min(total[k]), 4), round(max(total[k]), 4)],
                       passes_median_ms={name: round(statistics.median(v), 4) for name, v in sorted(per_kernel[k].items())},
                       energy_ha=float(out[0]), max_force=float(out[1].abs().max()))
    entries = int(num.sum())
    slots = n * width
    # bytes every D4 pass has to move: list words it streams (index 4 B + shift 12 B per SLOT of the padded matrix), gathers per stored
    # ENTRY (record 16 B; energy: + 32 B of neighbour weights; chain: + 8 B dE/dCN), per-atom traffic
    algorithmic = dict(
        d4_cn=16 * slots + 16 * entries + n * (16 + 12),
        d4_energy=16 * slots + (16 + 32) * entries + n * (16 + 96 + 8 * 13 + 8 + 24 + 4),
        d4_chain=16 * slots + (16 + 8) * entries + n * (16 + 8 + 24 + 12 + 48),
        d4_weights=n * (8 + 4 + 4 + 96),
        d4_pack=n * (12 + 4 + 16))
    print(json.dumps({"bench": "d4", "atoms": n, "cutoff": rc, "list_width": width, "mean_neighbors": round(float(num.float().mean()), 1),
                      "entries": entries, "reps": args.reps, "variants": rows, "algorithmic_bytes": algorithmic,
                      "dftd4_over_dftd3": round(rows["dftd4"]["median_ms"] / rows["dftd3"]["median_ms"], 3)}))


if __name__ == "__main__":
    main()
