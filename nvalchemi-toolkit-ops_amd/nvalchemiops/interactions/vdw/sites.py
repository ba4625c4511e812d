"""Reduced van der Waals sites: the hydrogen reduction of AMOEBA-class force fields as a table built once."""
from __future__ import annotations

import torch

from nvalchemiops import _capi as C


class ReducedSites:
    """The van der Waals sites of a topology: a plain container of tensors, built once.

    The vdW site of a hydrogen does not sit on its nucleus but on the bond to its heavy atom, at kappa_i of
    the bond: site_i = r_i - (1 - kappa_i) (r_i - r_p) with p = `parent[i]` and kappa_i = `reduction[i]` (AMOEBA: about 0.9); with a cell the bond
    vector is the minimum image and the site stays at the atom's own image.  `parent` int32 [N] names the heavy atom of every atom; an atom's own index,
    or -1, means the atom is its own site.  `reduction` [N] is read only where an atom has a parent.  `batch_idx` [N] is only read by the
    validation.

    The constructor also builds the inverse map the force redistribution needs: `child_ptr` int32 [N + 1] and `child_idx` int32 [E], a CSR
    over atoms of the children of each atom in ascending order.

    With `validate=True` the table is checked once, on the host (one device read), and a ValueError names the first offending atom: an index
    outside [-1, N), a parent that is itself reduced, and with `batch_idx` a parent in another system.  `validate=False` skips the read; the
    kernels then treat an index outside [0, N) as "no parent" (never an out-of-bounds access).

    `to(device)` returns a copy on another device."""

    def __init__(self, parent: torch.Tensor, reduction: torch.Tensor, *, batch_idx: torch.Tensor | None = None, validate: bool = True):
        if not isinstance(parent, torch.Tensor) or parent.dim() != 1:
            raise ValueError(f"parent must have shape [num_atoms], got {tuple(getattr(parent, 'shape', ()))}")
        n = parent.shape[0]
        if parent.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"parent must be an int32 (or int64) tensor, got {parent.dtype}")
        if not isinstance(reduction, torch.Tensor) or tuple(reduction.shape) != (n,):
            raise ValueError(f"reduction must have one entry per atom: expected shape [{n}], got {tuple(getattr(reduction, 'shape', ()))}")
        if not reduction.dtype.is_floating_point:
            raise ValueError(f"reduction must be a floating-point tensor, got {reduction.dtype}")
        if reduction.device != parent.device:
            raise ValueError(f"tensors on different devices: {parent.device} vs {reduction.device}")
        C.check_per_atom(n, batch_idx=batch_idx)
        if validate:
            _validate(parent, batch_idx)
        dev = parent.device
        own = torch.arange(n, dtype=torch.int64, device=dev)
        par = parent.to(torch.int64)
        par = torch.where((par >= 0) & (par < n) & (par != own), par, -1)
        reduced = par >= 0
        child, target = own[reduced], par[reduced]
        order = torch.argsort(target * max(n, 1) + child)  # by parent, then by child: all keys are distinct
        ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        if n:
            ptr[1:] = torch.cumsum(torch.bincount(target, minlength=n), 0)
        self.num_atoms = n
        self.parent = par.to(torch.int32).contiguous()
        self.reduction = torch.where(reduced, reduction.detach(), torch.ones_like(reduction)).contiguous()
        self.child_ptr = ptr.to(torch.int32).contiguous()
        self.child_idx = child[order].to(torch.int32).contiguous()

    def to(self, device) -> "ReducedSites":
        other = object.__new__(ReducedSites)
        other.num_atoms = self.num_atoms
        for name in ("parent", "reduction", "child_ptr", "child_idx"):
            setattr(other, name, getattr(self, name).to(device))
        return other

    @property
    def device(self) -> torch.device:
        return self.parent.device

    def __repr__(self) -> str:
        return f"ReducedSites(num_atoms={self.num_atoms}, reduced={self.child_idx.shape[0]}, device={self.device})"


def _validate(parent, batch_idx) -> None:
    """Every ValueError of the table's VALUES, on the host."""
    par = parent.detach().cpu().long()
    n = par.shape[0]
    bad = (par < -1) | (par >= n)
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        raise ValueError(f"atom {i}: parent index {int(par[i])} is outside [-1, {n})")
    own = torch.arange(n)
    reduced = (par >= 0) & (par != own)
    safe = par.clamp(min=0)
    bad = reduced & reduced[safe]
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        raise ValueError(f"atom {i}: its parent {int(par[i])} is itself reduced (parent {int(par[par[i]])}); a parent must be its own site")
    if batch_idx is not None:
        bi = batch_idx.detach().cpu().long()
        bad = reduced & (bi[safe] != bi)
        if bool(bad.any()):
            i = int(torch.nonzero(bad)[0])
            raise ValueError(f"atom {i} (system {int(bi[i])}): its parent {int(par[i])} is in another system ({int(bi[par[i]])})")


__all__ = ["ReducedSites"]
