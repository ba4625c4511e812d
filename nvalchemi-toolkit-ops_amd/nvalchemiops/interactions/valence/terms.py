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

    _ARITIES, _ARITY_TEXT = (2, 3, 4), "A = 2, 3 or 4"
    _TENSORS = ("atoms", "slot_ptr", "slot_idx")

    def __init__(self, atoms: torch.Tensor, num_atoms: int, *, batch_idx: torch.Tensor | None = None, validate: bool = True):
        self.num_atoms, self.atoms, self.slot_ptr, self.slot_idx = _build(atoms, num_atoms, batch_idx, validate, self._ARITIES, self._ARITY_TEXT)

    def to(self, device) -> "ValenceTerms":
        other = object.__new__(type(self))
        other.num_atoms = self.num_atoms
        for name in self._TENSORS:
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
        return f"{type(self).__name__}(num_terms={self.num_terms}, arity={self.arity}, num_atoms={self.num_atoms}, device={self.device})"


class WideValenceTerms(ValenceTerms):
    """`ValenceTerms` for the terms of A = 5 or 6 atoms: the same attributes, inverse CSR, validation and `to()`.  Pi-torsions name
    (a, b, c, d, e, f) with c-d the bond, a and b bonded to c, e and f bonded to d; torsion-torsions take `TorsionTorsionTerms`."""

    _ARITIES, _ARITY_TEXT = (5, 6), "A = 5 or 6"


class TorsionTorsionTerms(WideValenceTerms):
    """The torsion-torsion (CMAP) terms of a topology: `atoms` [T, 5] = (a, b, c, d, e), `map_index` int32 (or int64) [T], the map of
    `TorsionTorsionMaps` each term reads, and `signs` [T] of +1 or -1 (default +1), the chirality sign s in E = F_m(s phi_1, s phi_2);
    the caller decides it.  Everything else is `ValenceTerms`; the rows stay in the caller's order.

    With `validate=True` (which synchronises: the signs are copied to the host and the extremes of `map_index` are read, once, here) a sign
    other than +-1 or a negative `map_index` raises ValueError, and the largest `map_index` is kept so that `torsion_torsion` can refuse a
    table that names a map its `maps` does not hold without another device read.  With `validate=False` a term whose map is outside [0, M)
    contributes exact zeros."""

    _ARITIES, _ARITY_TEXT = (5,), "A = 5"
    _TENSORS = ValenceTerms._TENSORS + ("map_index", "signs")

    def __init__(self, atoms: torch.Tensor, map_index: torch.Tensor, num_atoms: int, *, signs: torch.Tensor | None = None,
                 batch_idx: torch.Tensor | None = None, validate: bool = True):
        super().__init__(atoms, num_atoms, batch_idx=batch_idx, validate=validate)
        t = self.num_terms
        if not isinstance(map_index, torch.Tensor) or map_index.dtype not in (torch.int32, torch.int64) or tuple(map_index.shape) != (t,):
            raise ValueError(f"map_index must be an int32 (or int64) tensor of shape [{t}], got {getattr(map_index, 'dtype', None)} "
                             f"{tuple(getattr(map_index, 'shape', ()))}")
        if signs is None:
            signs = torch.ones(t, dtype=torch.float64, device=self.device)
        if not isinstance(signs, torch.Tensor) or tuple(signs.shape) != (t,):
            raise ValueError(f"signs must have shape [{t}], got {tuple(getattr(signs, 'shape', ()))}")
        self.max_map = None
        if validate and t:
            bad = signs.detach().abs().cpu() != 1
            if bool(bad.any()):
                k = int(torch.nonzero(bad)[0])
                raise ValueError(f"term {k}: sign {float(signs[k])} is not +1 or -1")
            low, self.max_map = int(map_index.min()), int(map_index.max())
            if low < 0:
                raise ValueError(f"term {int(torch.nonzero(map_index < 0)[0])}: map_index {low} is negative")
        self.map_index = map_index.to(device=self.device, dtype=torch.int32).contiguous()
        self.signs = signs.to(device=self.device, dtype=torch.float64).contiguous()

    def to(self, device) -> "TorsionTorsionTerms":
        other = super().to(device)
        other.max_map = self.max_map
        return other


def _build(atoms, num_atoms, batch_idx, validate, arities, arity_text):
    """What every table holds: (N, atoms int32 [T, A], slot_ptr int32 [N + 1], slot_idx int32 [E]), after the argument checks."""
    if not isinstance(atoms, torch.Tensor) or atoms.dim() != 2 or atoms.shape[1] not in arities:
        raise ValueError(f"atoms must have shape [num_terms, A] with {arity_text}, got {tuple(getattr(atoms, 'shape', ()))}")
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
    return n, atoms.to(torch.int32).contiguous(), ptr.to(torch.int32).contiguous(), slot[order].to(torch.int32).contiguous()


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


__all__ = ["ValenceTerms", "WideValenceTerms", "TorsionTorsionTerms"]
