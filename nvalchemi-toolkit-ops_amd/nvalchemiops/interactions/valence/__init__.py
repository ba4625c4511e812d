"""Valence terms of the force-field stack: bond stretch, angle bend, stretch-bend, out-of-plane bend and Fourier torsion over tables of atom
tuples (HIP: csrc/valence.hip)."""
from nvalchemiops.interactions.valence.functions import angle_bend, bond_stretch, out_of_plane_bend, stretch_bend, torsion
from nvalchemiops.interactions.valence.terms import ValenceTerms

__all__ = ["ValenceTerms", "bond_stretch", "angle_bend", "stretch_bend", "out_of_plane_bend", "torsion"]
