"""Cost of the fused multi-channel spread / gather against the per-channel loop over the scalar ops -- what `spline_spread_channels` /
`spline_gather_channels` ran before they were fused, written out below; the scalar functions are the same in both.  C = 4 and 9, fp32
and fp64, order 4 and 5, on three regimes: the config-4 box (100 000 atoms, 128^3 mesh: tile path), a 2 000-atom box on a 32^3 mesh
(atomic path) and a batch of 16 such boxes.  Event-bracketed medians, fused and loop alternated inside one process, every shape warmed up.
Usage: python tools/channels_bench.py [--reps 30] [--warmup 5] [--only config4|small|batch16]   -> one JSON line."""
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


def _regimes(dev, dtype):
    from tests import systems as S

    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731
    pos, cell, _, _ = S.fcc_box(100000, seed=1234, dtype=dtype)
    yield "config4", t(pos), t(cell), None, (128, 128, 128)
    pos, cell, _, _ = S.fcc_box(2000, seed=1234, dtype=dtype)
    yield "small", t(pos), t(cell), None, (32, 32, 32)
    bi = np.repeat(np.arange(16, dtype=np.int32), 2000)
    yield "batch16", t(np.tile(pos, (16, 1))), t(np.tile(cell[None], (16, 1, 1))), t(bi), (32, 32, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    from nvalchemiops.spline import spline_gather, spline_gather_channels, spline_spread, spline_spread_channels

    dev = "cuda:0"
    cases = []
    for dtype in (np.float64, np.float32):
        for regime, pos, cell, bi, dims in _regimes(dev, dtype):
            if args.only and regime != args.only:
                continue
            for nch in (4, 9):
                g = torch.Generator(device=dev).manual_seed(nch)
                vals = torch.randn((pos.shape[0], nch), dtype=pos.dtype, device=dev, generator=g)
                mesh = torch.randn(((16, nch) if bi is not None else (nch,)) + dims, dtype=pos.dtype, device=dev, generator=g)
                for order in (4, 5):
                    def spread_fused(pos=pos, vals=vals, cell=cell, dims=dims, order=order, bi=bi):
                        return spline_spread_channels(pos, vals, cell, dims, order, bi)

                    def spread_loop(pos=pos, vals=vals, cell=cell, dims=dims, order=order, bi=bi):
                        return torch.stack([spline_spread(pos, vals[:, ch], cell, dims, order, bi) for ch in range(vals.shape[1])], dim=0 if bi is None else 1)

                    def gather_fused(pos=pos, mesh=mesh, cell=cell, order=order, bi=bi):
                        return spline_gather_channels(pos, mesh, cell, order, bi)

                    def gather_loop(pos=pos, mesh=mesh, cell=cell, order=order, bi=bi, nch=nch):
                        return torch.stack([spline_gather(pos, mesh[ch] if bi is None else mesh[:, ch], cell, order, bi) for ch in range(nch)], dim=1)

                    cases.append((dict(regime=regime, dtype=np.dtype(dtype).name, channels=nch, order=order),
                                  {"spread_fused": spread_fused, "spread_loop": spread_loop, "gather_fused": gather_fused, "gather_loop": gather_loop}))
    for _, variants in cases:
        for fn in variants.values():
            for _ in range(args.warmup):
                fn()
    torch.cuda.synchronize()
    rows = []
    for tag, variants in cases:
        times = {k: [] for k in variants}
        for _ in range(args.reps):
            for name, fn in variants.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                times[name].append(a.elapsed_time(b))
        med = {k: statistics.median(v) for k, v in times.items()}
        rows.append(dict(tag, median_ms={k: round(v, 4) for k, v in med.items()},
                         spread_loop_over_fused=round(med["spread_loop"] / med["spread_fused"], 3),
                         gather_loop_over_fused=round(med["gather_loop"] / med["gather_fused"], 3),
                         min_max_ms={k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()}))
    print(json.dumps({"bench": "channels", "reps": args.reps, "cases": rows}))


if __name__ == "__main__":
    main()
