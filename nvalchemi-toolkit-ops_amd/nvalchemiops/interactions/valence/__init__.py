"""Valence terms of the force-field stack: bond stretch, angle bend, stretch-bend, out-of-plane bend and Fourier torsion over tables of atom
tuples, and the coupled torsion terms: stretch-torsion, angle-torsion, pi-torsion and torsion-torsion (HIP: csrc/valence.hip)."""
from nvalchemiops.interactions.valence.functions import (angle_bend, angle_torsion, bond_stretch, out_of_plane_bend, pi_torsion, stretch_bend,
                                                         stretch_torsion, torsion)
from nvalchemiops.interactions.valence.terms import TorsionTorsionTerms, ValenceTerms, WideValenceTerms
from nvalchemiops.interactions.valence.tortor import TorsionTorsionMaps, torsion_torsion

__all__ = ["ValenceTerms", "WideValenceTerms", "TorsionTorsionTerms", "TorsionTorsionMaps", "bond_stretch", "angle_bend", "stretch_bend",
           "out_of_plane_bend", "torsion", "stretch_torsion", "angle_torsion", "pi_torsion", "torsion_torsion"]
