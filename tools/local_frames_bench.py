"""Times the local-frame rotation and the torque forces on a water-like box and puts them beside the pair sum they feed and beside the same
maths written in torch ops on the device.

    python tools/local_frames_bench.py [--atoms 100000] [--dtype float32|float64] [--repeat 200] [--out FILE.json]

The box: `--atoms` atoms (default 100 000) as waters on a jittered cubic grid of 3.1 per site, each randomly rotated, O a bisector of its two
H, each H z-then-x on O and the other H, NONE atoms as filler; random local dipoles and quadrupoles.  Timed, after a warm-up, with device
events around `--repeat` calls each (the device is synchronised at both ends):

    rotate_multipoles                       one `mi_frame_rotate`
    multipole_frame_forces                  `mi_frame_adjoint` + `mi_frame_gather` (forces alone; and with local gradients and the virial term)
    rotate_multipoles -> backward()         the same kernels through the `alchemiops::_rotate_multipoles` op and autograd
    ewald_quadrupole_real_space             the pair sum the rotated multipoles feed, on a 6.0 list of the same box, with forces and gradients
    torch composition                       tests/local_frames_reference.rotate on device tensors (float64): forward, and forward + backward

and, from the library's own per-kernel event records (`mi_timing_enable`), the time of each of the three kernels with the bytes the algorithm
has to move (computed here from the shapes and the frame table) and the bandwidth that makes.  Prints one JSON line.  Needs a device: there is
no CPU path to time."""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "nvalchemi-toolkit-ops_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from tests import local_frames_reference as LR  # noqa: E402

F64 = torch.float64


def water_box(n_atoms, seed=0, site=3.1):
    """(positions [n, 3], frame_atoms, frame_kinds, cell [3, 3]) float64 / int32 on the CPU, vectorised."""
    gen = torch.Generator().manual_seed(seed)
    n_w = n_atoms // 3
    side = 1
    while side ** 3 < n_w + (n_atoms - 3 * n_w):
        side += 1
    sites = torch.stack(torch.meshgrid(*[torch.arange(side, dtype=F64)] * 3, indexing="ij"), -1).reshape(-1, 3) * site
    sites = sites + 0.4 * (torch.rand(sites.shape, dtype=F64, generator=gen) - 0.5)
    mol, _, _ = LR.water()
    q, r = torch.linalg.qr(torch.randn((n_w, 3, 3), dtype=F64, generator=gen))
    q = q * torch.sign(torch.diagonal(r, dim1=-2, dim2=-1))[:, None, :]
    q[:, :, 0] *= torch.linalg.det(q)[:, None]
    pos_w = (torch.einsum("wab,kb->wka", q, mol - mol.mean(0)) + sites[:n_w, None, :]).reshape(-1, 3)
    base = 3 * torch.arange(n_w, dtype=torch.int32)[:, None]
    atoms_w = torch.stack([torch.cat([base + 1, base + 2, 0 * base - 1], 1), torch.cat([base, base + 2, 0 * base - 1], 1),
                           torch.cat([base, base + 1, 0 * base - 1], 1)], 1).reshape(-1, 3)
    kinds_w = torch.tensor([LR.BISECTOR, LR.Z_THEN_X, LR.Z_THEN_X], dtype=torch.int32).repeat(n_w)
    fill = n_atoms - 3 * n_w
    pos = torch.cat([pos_w, sites[n_w:n_w + fill]])
    atoms = torch.cat([atoms_w, torch.full((fill, 3), -1, dtype=torch.int32)])
    kinds = torch.cat([kinds_w, torch.zeros(fill, dtype=torch.int32)])
    return pos, atoms, kinds, torch.eye(3, dtype=F64) * (side * site)


def algorithmic_bytes(frames, size, local, virial):
    """Bytes each kernel has to move: every input element read once per use and every output element written once (`size` bytes per element
    of the positions dtype, frame-atom positions counted as the gathers they are)."""
    n, named = frames.num_atoms, int((frames.frame_atoms >= 0).sum())
    tables = n * (12 + 4)
    rotate = tables + (n + named) * 3 * size + n * (3 + 9) * size + n * 9 * size + n * (3 + 9) * size
    adjoint = tables + (n + named) * 3 * size + n * (3 + 9) * size * 2 + n * 9 * size + n * 96 + (n * 96 if local else 0) + (n * 72 if virial else 0)
    gather = n * (24 + 8) + named * (4 + 24) + n * 3 * size + (n * 72 if virial else 0)
    return dict(frame_rotate=rotate, frame_adjoint=adjoint, frame_gather=gather)


def timed(fn, repeat, warmup=10):
    """Milliseconds per call: device events around `repeat` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(repeat):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / repeat


def kernel_times(fn, repeat):
    """{bracket name: milliseconds per launch} from the library's event records."""
    from nvalchemiops import _capi as C

    L = C.lib()
    torch.cuda.synchronize()
    L.mi_timing_select(None)
    L.mi_timing_enable(1)
    for _ in range(repeat):
        fn()
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 14)
    L.mi_timing_report(buf, len(buf))
    L.mi_timing_enable(0)
    out = {}
    for line in buf.value.decode().splitlines():
        name, launches, total = line.split()
        out[name] = float(total) / int(launches)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--atoms", type=int, default=100000)
    ap.add_argument("--dtype", choices=("float32", "float64"), default="float32")
    ap.add_argument("--repeat", type=int, default=200)
    ap.add_argument("--cutoff", type=float, default=6.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/local_frames_bench.py needs a device: nothing here can be timed on the CPU")
    from nvalchemiops.interactions.electrostatics import LocalFrames, ewald_quadrupole_real_space, multipole_frame_forces, rotate_multipoles
    from nvalchemiops.neighborlist import neighbor_list

    dev, dt = "cuda:0", getattr(torch, args.dtype)
    pos64, atoms, kinds, cell64 = water_box(args.atoms)
    n = pos64.shape[0]
    mu64, quad64 = LR.local_multipoles(n, 1)
    pos, cell, mu_loc, quad_loc = (t.to(dev, dt) for t in (pos64, cell64, 0.3 * mu64, 0.2 * quad64))
    frames = LocalFrames(atoms.to(dev), kinds.to(dev))
    gen = torch.Generator().manual_seed(2)
    g_mu, g_q = torch.randn((n, 3), dtype=F64, generator=gen).to(dev, dt), torch.randn((n, 3, 3), dtype=F64, generator=gen).to(dev, dt)
    res = dict(atoms=n, dtype=args.dtype, repeat=args.repeat, named_slots=int((frames.frame_atoms >= 0).sum()), device=torch.cuda.get_device_name(0))

    # what is timed computes what the reference computes
    mu, quad = rotate_multipoles(pos, mu_loc, quad_loc, frames, cell)
    ref = LR.evaluate(pos.to(F64), mu_loc.to(F64), quad_loc.to(F64), frames.frame_atoms, frames.frame_kinds, g_mu.to(F64), g_q.to(F64), cell=cell.to(F64))
    f, lm, lq, vir = multipole_frame_forces(pos, mu_loc, quad_loc, frames, g_mu, g_q, cell, compute_local_gradients=True, compute_virial=True)
    rel = lambda a, b: float((a.to(F64) - b).abs().max() / b.abs().max())  # noqa: E731
    res["parity"] = dict(dipoles=rel(mu, ref["dipoles"]), quadrupoles=rel(quad, ref["quadrupoles"]), forces=rel(f, -ref["positions_grad"]),
                         local_dipole_grads=rel(lm, ref["local_dipole_grads"]), local_quadrupole_grads=rel(lq, ref["local_quadrupole_grads"]),
                         virial=rel(vir, ref["virial"]))

    ms = res["ms_per_call"] = {}
    ms["rotate_multipoles"] = timed(lambda: rotate_multipoles(pos, mu_loc, quad_loc, frames, cell), args.repeat)
    ms["multipole_frame_forces"] = timed(lambda: multipole_frame_forces(pos, mu_loc, quad_loc, frames, g_mu, g_q, cell), args.repeat)
    ms["multipole_frame_forces_local_virial"] = timed(lambda: multipole_frame_forces(pos, mu_loc, quad_loc, frames, g_mu, g_q, cell,
                                                                                      compute_local_gradients=True, compute_virial=True), args.repeat)

    leaves = [t.clone().requires_grad_(True) for t in (pos, mu_loc, quad_loc)]

    def through_autograd():
        for t in leaves:
            t.grad = None
        m, q = rotate_multipoles(*leaves, frames, cell)
        torch.autograd.backward((m, q), (g_mu, g_q))

    ms["rotate_multipoles_and_backward"] = timed(through_autograd, args.repeat)

    # the torch-op restatement of the same maths, float64 on the device
    t_pos, t_mu, t_q, t_cell = (t.to(F64) for t in (pos, mu_loc, quad_loc, cell))
    t_gm, t_gq = g_mu.to(F64), g_q.to(F64)
    fa, fk = frames.frame_atoms, frames.frame_kinds
    few = max(5, args.repeat // 10)
    ms["torch_rotate"] = timed(lambda: LR.rotate(t_pos, t_mu, t_q, fa, fk, t_cell), few, warmup=3)
    t_leaves = [t.clone().requires_grad_(True) for t in (t_pos, t_mu, t_q)]

    def torch_backward():
        for t in t_leaves:
            t.grad = None
        m, q = LR.rotate(*t_leaves, fa, fk, t_cell)
        torch.autograd.backward((m, q), (t_gm, t_gq))

    ms["torch_rotate_and_backward"] = timed(torch_backward, few, warmup=3)

    # the pair sum the rotated multipoles feed
    charges = torch.where(frames.frame_kinds == LR.BISECTOR, -0.8, 0.4).to(dt) * (frames.frame_kinds != LR.NONE)
    pbc = torch.tensor([True] * 3, device=dev)
    nm, num, sh = neighbor_list(pos, args.cutoff, cell=cell, pbc=pbc, method="cell_list", max_neighbors=192)
    res["neighbors_mean"], res["neighbors_max"] = float(num.double().mean()), int(num.max())
    assert res["neighbors_max"] <= 192
    ms["ewald_quadrupole_real_space"] = timed(lambda: ewald_quadrupole_real_space(
        pos, charges, mu, quad, cell, 0.35, neighbor_matrix=nm, neighbor_matrix_shifts=sh, compute_forces=True, compute_dipole_gradients=True,
        compute_quadrupole_gradients=True), max(5, args.repeat // 10), warmup=3)

    res["ratio_torch_over_hip"] = dict(rotate=ms["torch_rotate"] / ms["rotate_multipoles"],
                                       rotate_and_backward=ms["torch_rotate_and_backward"] / ms["rotate_multipoles_and_backward"],
                                       backward_against_explicit_forces=(ms["torch_rotate_and_backward"] - ms["torch_rotate"]) / ms["multipole_frame_forces"])
    res["share_of_ewald_quadrupole_real_space"] = (ms["rotate_multipoles"] + ms["multipole_frame_forces"]) / ms["ewald_quadrupole_real_space"]

    # per-kernel times, bytes and bandwidth
    size = 4 if dt == torch.float32 else 8
    kernels = res["kernels"] = {}
    for label, local, virial in (("forces", False, False), ("forces_local_virial", True, True)):
        def both():
            rotate_multipoles(pos, mu_loc, quad_loc, frames, cell)
            multipole_frame_forces(pos, mu_loc, quad_loc, frames, g_mu, g_q, cell, compute_local_gradients=local, compute_virial=virial)

        times, nbytes = kernel_times(both, args.repeat), algorithmic_bytes(frames, size, local, virial)
        kernels[label] = {k: dict(ms=times[k], bytes=nbytes[k], gb_per_s=nbytes[k] / times[k] * 1e-6) for k in nbytes if k in times}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
