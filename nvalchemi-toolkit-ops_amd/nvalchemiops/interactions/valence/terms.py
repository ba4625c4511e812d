"""The atom tuples of one kind of valence term (bonds, angles, torsions ...) as a table built once."""
from __future__ import annotations

import torch

from nvalchemiops import _capi as C


class ValenceTerms:
    """The terms of one kind of a topology: a plain container of tensors, built once.

    `atoms` int32 (or int64) [T, A] names the A = 2, 3 or 4 atoms of every term, in the order the function that takes the table defines
    (bonds a-b; angles a-b-c with b the vertex; out-of-plane bends a, b, c, d with b the centre and d out of plane; torsions a-b-c-d).
    `num_atoms` is N, the number of atoms of the positions the table will be used with.  `batch_idx` [N] is only read by the validation.

    The constructor also builds the inverse map the force gather needs: `slot_ptr` int32 [N + 1] and `slot_idx` int32 [E], a CSR over atoms of
    the slots t * A + p (term t, position p) that name each atom, in ascending slot order.

    With `validate=True` the table is checked once, on the host (one device read), and a ValueError names the first offending term: an index
    outside [0, N), two equal atoms in a term, and with `batch_idx` atoms of one term in different systems.  `validate=False` skips the read;
    a term that names an index outside [0, N) then contributes exact zeros everywhere (never an out-of-bounds access).

    `to(device)` returns a copy on another device."""

    def __init__(self, atoms: torch.Tensor, num_atoms: int, *, batch_idx: torch.Tensor | None = None, validate: bool = True):
        if not isinstance(atoms, torch.Tensor) or atoms.dim() != 2 or atoms.shape[1] not in (2, 3, 4):
            raise ValueError(f"atoms must have shape [num_terms, A] with A = 2, 3 or 4, got {tuple(getattr(atoms, 'shape', ()))}")
        if atoms.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"atoms must be an int32 (or int64) tensor, got {atoms.dtype}")
        n, (t, a) = int(num_atoms), atoms.shape
        if not 0 <= n <= (1 << 29):
            raise ValueError(f"num_atoms must be in [0, 2^29], got {n}")
        if t > (1 << 28):
            raise ValueError(f"at most 2^28 terms, got {t}")
        C.check_per_atom(n, batch_idx=batch_idx)
        if validate:
            _validate(atoms, n, batch_idx)
        dev = atoms.device
        idx = atoms.to(torch.int64)
        slots = torch.arange(t * a, dtype=torch.int64, device=dev).reshape(t, a)
        named = (idx >= 0) & (idx < n)
        target, slot = idx[named], slots[named]
        order = torch.argsort(target * max(t * a, 1) + slot)  # by the atom named, then by slot: all keys are distinct
        ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        if n:
            ptr[1:] = torch.cumsum(torch.bincount(target, minlength=n), 0)
        self.num_atoms = n
        self.atoms = atoms.to(torch.int32).contiguous()
        self.slot_ptr = ptr.to(torch.int32).contiguous()
        self.slot_idx = slot[order].to(torch.int32).contiguous()

    def to(self, device) -> "ValenceTerms":
        other = object.__new__(ValenceTerms)
        other.num_atoms = self.num_atoms
        for name in ("atoms", "slot_ptr", "slot_idx"):
            setattr(other, name, getattr(self, name).to(device))
        return other

    @property
    def device(self) -> torch.device:
        return self.atoms.device

    @property
    def num_terms(self) -> int:
        return self.atoms.shape[0]

    @property
    def arity(self) -> int:
        return self.atoms.shape[1]

    def __repr__(self) -> str:
        return f"ValenceTerms(num_terms={self.num_terms}, arity={self.arity}, num_atoms={self.num_atoms}, device={self.device})"


def _validate(atoms, n, batch_idx) -> None:
    """Every ValueError of the table's VALUES, on the host."""
    idx = atoms.detach().cpu().long()
    a = idx.shape[1]
    bad = (idx < 0) | (idx >= n)
    if bool(bad.any()):
        t, p = (int(v) for v in torch.nonzero(bad)[0])
        raise ValueError(f"term {t}: atom index {int(idx[t, p])} is outside [0, {n})")
    bad = torch.zeros(idx.shape[0], dtype=torch.bool)
    for p in range(a):
        for q in range(p + 1, a):
            bad |= idx[:, p] == idx[:, q]
    if bool(bad.any()):
        t = int(torch.nonzero(bad)[0])
        raise ValueError(f"term {t}: an atom appears twice in {idx[t].tolist()}")
    if batch_idx is not None:
        sys = batch_idx.detach().cpu().long()[idx]
        bad = (sys != sys[:, :1]).any(1)
        if bool(bad.any()):
            t = int(torch.nonzero(bad)[0])
            raise ValueError(f"term {t}: its atoms {idx[t].tolist()} are in different systems {sys[t].tolist()}")


__all__ = ["ValenceTerms"]
